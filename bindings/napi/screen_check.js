// node screen_check.js   on an MI355X (ZKATTEST_NODE: the addon): the witness screen behind the facade (tests/test_napi_screen.py).
// screenSignatureLists over three rings: valid statements come back ok with the signer's index found; a wrong message, a foreign signature, a key that is not
// in the ring and a wrong `which` are flagged with their bit; and exactly the statements that were ok yield proofs that verifySignatureLists accepts.
const assert = require('assert')
const crypto = require('crypto')
const zk = require('./zkattest.js')
const { generateParamsList, keyToInt, screenSignatureLists, findKey, proveSignatureLists, verifySignatureLists, SCREEN, WHICH_NONE } = zk

async function main() {
    const params = generateParamsList(20)
    const st = []
    for (let r = 0; r < 3; r++) {
        const keyPair = crypto.generateKeyPairSync('ec', { namedCurve: 'P-256' }), msg = Buffer.from('screen ' + r)
        const msgHash = crypto.createHash('sha256').update(msg).digest()
        const sigBytes = crypto.sign('sha256', msg, { key: keyPair.privateKey, dsaEncoding: 'ieee-p1363' })
        const keys = [BigInt(31 + r), BigInt(7)]
        for (let k = 0; k < 2 + 3 * r; k++) keys.push(BigInt(200 + k))
        keys.push(await keyToInt(keyPair.publicKey))   // the signer's key last: index 4, 7, 10
        keys.push(BigInt(9))
        Object.freeze(keys)
        st.push({ msgHash, sigBytes, publicKey: keyPair.publicKey, keys })
    }
    const at = [4, 7, 10]
    const wrongMsg = Object.assign({}, st[0], { msgHash: crypto.createHash('sha256').update('another').digest() })
    const foreignSig = Object.assign({}, st[1], { sigBytes: st[2].sigBytes })
    const otherRing = Object.assign({}, st[2], { keys: st[0].keys })
    const all = [st[0], st[1], st[2], wrongMsg, foreignSig, otherRing, st[1]]
    const found = await screenSignatureLists(params, all)
    assert.deepStrictEqual(found.map((r) => r.flags), [0, 0, 0, SCREEN.SIG_INVALID, SCREEN.SIG_INVALID, SCREEN.NOT_IN_RING, 0])
    assert.deepStrictEqual(found.map((r) => r.which), [4, 7, 10, 4, 7, WHICH_NONE, 7])
    assert.deepStrictEqual(found.map((r) => r.ok), found.map((r) => r.flags === 0))
    // check mode: the right index passes, a wrong one and one past the padded ring do not
    const checked = await screenSignatureLists(params, [Object.assign({ which: 4 }, st[0]), Object.assign({ which: 3 }, st[1]), Object.assign({ which: 64 }, st[2])])
    assert.deepStrictEqual(checked.map((r) => [r.which, r.flags]), [[4, 0], [3, SCREEN.NOT_IN_RING], [64, SCREEN.NOT_IN_RING]])
    await assert.rejects(screenSignatureLists(params, [Object.assign({ which: 4 }, st[0]), st[1]]), RangeError)
    assert.deepStrictEqual(await screenSignatureLists(params, []), [])
    // findKey: the lookup alone
    assert.strictEqual(await findKey(st[1].publicKey, st[1].keys), 7)
    assert.strictEqual(await findKey(st[1].publicKey, st[0].keys, params), -1)
    // the screen means what it says: every statement proved with the index it reported (0 where there is none), the verifier accepts exactly the ok ones
    const which = found.map((r) => (r.which === WHICH_NONE ? 0 : r.which)), col = (f) => all.map((s) => s[f])
    const proofs = await proveSignatureLists(params, col('msgHash'), col('sigBytes'), col('publicKey'), which, col('keys'))
    const ok = await verifySignatureLists(params, col('msgHash'), col('keys'), proofs)
    assert.deepStrictEqual(Array.from(ok), found.map((r) => r.ok))
    assert.deepStrictEqual(at, found.slice(0, 3).map((r) => r.which))
    console.log('screen ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
