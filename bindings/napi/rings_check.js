// node rings_check.js   on an MI355X (ZKATTEST_NODE: the addon): resident rings behind the facade (tests/test_napi_rings.py).  verifySignatureList over
// two rings in alternation rebuilds neither after its first use (ringInfo generation), and verifySignatureLists on a mixed batch answers like per-ring calls.
const assert = require('assert')
const crypto = require('crypto')
const zk = require('./zkattest.js')
const { generateParamsList, keyToInt, proveSignatureList, verifySignatureList, verifySignatureListBatch, verifySignatureLists } = zk

async function main() {
    const params = generateParamsList(80)
    const signers = [], proofs = [], rings = []
    for (let r = 0; r < 2; r++) {
        const keyPair = crypto.generateKeyPairSync('ec', { namedCurve: 'P-256' }), msg = Buffer.from('rings ' + r)
        const msgHash = crypto.createHash('sha256').update(msg).digest()
        const signature = crypto.sign('sha256', msg, { key: keyPair.privateKey, dsaEncoding: 'ieee-p1363' })
        const keys = [BigInt(11 + r), await keyToInt(keyPair.publicKey), BigInt(5), BigInt(6 + 10 * r), BigInt(7)]
        if (r === 1) keys.push(BigInt(8), BigInt(9), BigInt(10), BigInt(12))   // another n
        Object.freeze(keys)
        signers.push(msgHash), rings.push(keys)
        proofs.push(await proveSignatureList(params, msgHash, signature, keyPair.publicKey, 1, keys))
    }
    const gens = []
    for (let i = 0; i < 6; i++) {
        const r = i % 2
        assert.strictEqual(await verifySignatureList(params, signers[r], rings[r], proofs[r]), true)
        assert.strictEqual(await verifySignatureList(params, signers[r], rings[1 - r], proofs[r]), false)
        gens.push(zk._ringGenerations(params))
    }
    assert.deepStrictEqual(gens[5], gens[1], 'a resident ring was rebuilt')
    assert.strictEqual(Object.keys(gens[5]).length, 2)
    const msgs = [signers[0], signers[1], signers[0], signers[1], signers[0]]
    const keyLists = [rings[0], rings[1], rings[1], rings[0], rings[0]]
    const plist = [proofs[0], proofs[1], proofs[0], proofs[1], Buffer.from('not a proof')]
    const got = await verifySignatureLists(params, msgs, keyLists, plist)
    const want = []
    for (let i = 0; i < plist.length; i++) want.push((await verifySignatureListBatch(params, [msgs[i]], keyLists[i], [plist[i]]))[0])
    assert.deepStrictEqual(Array.from(got), want)
    assert.deepStrictEqual(Array.from(got), [true, true, false, false, false])
    assert.ok(got.errors[4] instanceof Error && got.errors[0] === null)
    assert.deepStrictEqual(zk._ringGenerations(params), gens[5], 'verifySignatureLists rebuilt a resident ring')
    console.log('rings ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
