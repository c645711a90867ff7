// node accountable_rings_check.js   on an MI355X (ZKATTEST_NODE: the addon): accountable attestations whose signers sit in different rings, behind the facade
// (tests/test_napi_accountable_rings.py).  proveAccountables / verifyAccountables take one key list per proof in the place of `keys` (the convention of
// reringSignatureLists) and openAccountables opens straight from the bundles: three signers over two registries of different size -> AccountableProofs that
// verifyAccountables accepts with the same lists and that open to (registry, index); the parts are what the existing calls accept; the wrong registry, swapped
// tags and another hash give false; a key enrolled in both registries opens in the registry it is asked in; with one list throughout the bundles verify
// through the one-ring form as well.
const assert = require('assert')
const crypto = require('crypto')
const zk = require('./zkattest.js')
const { generateParamsList, keyToInt, proveAccountables, verifyAccountables, openAccountables, splitAccountable, AccountableProof, verifySignatureLists, openEscrowTags,
    escrowAuditorKey } = zk

async function main() {
    assert.strictEqual(openAccountables.length, 4)
    const params = generateParamsList(80)
    const a = 0x1234567890abcdef1234567890abcdefn
    const A = await escrowAuditorKey(params, a), A2 = await escrowAuditorKey(params, a + 1n)
    const signers = []
    for (let r = 0; r < 3; r++) {
        const keyPair = crypto.generateKeyPairSync('ec', { namedCurve: 'P-256' }), msg = Buffer.from('accountable rings ' + r)
        signers.push({ msgHash: crypto.createHash('sha256').update(msg).digest(), publicKey: keyPair.publicKey, x: await keyToInt(keyPair.publicKey),
            signature: crypto.sign('sha256', msg, { key: keyPair.privateKey, dsaEncoding: 'ieee-p1363' }) })
    }
    // registry A: 7 keys (padded to 8), signers 0 and 2 at 1 and 5; registry B: 19 keys (padded to 32), signer 1 at 3 and signer 0 AGAIN at 17
    const keysA = Object.freeze([21n, signers[0].x, 5n, 6n, 77n, signers[2].x, 9n])
    const keysB = Object.freeze(Array.from({ length: 19 }, (_, i) => (i === 3 ? signers[1].x : i === 17 ? signers[0].x : BigInt(1000 + i))))
    const col = (f) => signers.map((s) => s[f]), msgs = col('msgHash')
    const whichs = [1, 3, 5], lists = [keysA, keysB, keysA]
    const proofs = await proveAccountables(params, A, msgs, col('signature'), col('publicKey'), whichs, lists)
    assert.strictEqual(proofs.length, 3)
    for (const p of proofs) assert.ok(p instanceof AccountableProof && p.bytes.readUInt32BE(4) === p.bytes.length && p.tag.bytes.length === 472)
    assert.deepStrictEqual(proofs.map((p) => p.attestation.bytes.readUInt32BE(12)), [3, 5, 3])   // the inner headers' n: rings of 8, 32 and 8 padded keys
    assert.deepStrictEqual(Array.from(await verifyAccountables(params, A, msgs, lists, proofs)), [true, true, true])
    assert.deepStrictEqual(Array.from(await verifyAccountables(params, A, msgs, lists, proofs.map((p) => p.bytes))), [true, true, true])
    // the parts are what the existing calls accept, and the split tags open to what the bundles open to
    const parts = await splitAccountable(params, proofs)
    assert.deepStrictEqual(Array.from(await verifySignatureLists(params, msgs, lists, parts.map((x) => x.attestation))), [true, true, true])
    const opened = await openAccountables(params, a, lists, proofs)
    assert.deepStrictEqual(opened, [{ ring: 0, index: 1 }, { ring: 1, index: 3 }, { ring: 0, index: 5 }])
    assert.deepStrictEqual(opened, await openEscrowTags(params, a, lists, parts.map((x) => x.tag)))
    // signer 0's key is enrolled in registry B too: asked there, it is found there; asked in a registry that lacks the key, nobody
    assert.deepStrictEqual(await openAccountables(params, a, [keysB, keysA, keysB], proofs), [{ ring: 0, index: 17 }, null, null])
    assert.deepStrictEqual(await openAccountables(params, a + 1n, lists, proofs), [null, null, null])   // another auditor's secret decrypts to nobody's key
    // the wrong registry for proof 1; swapped tags; another hash; another auditor's key
    assert.deepStrictEqual(Array.from(await verifyAccountables(params, A, msgs, [keysA, keysA, keysA], proofs)), [true, false, true])
    const swap = (p, q) => Buffer.concat([p.bytes.slice(0, p.bytes.length - 472), q.bytes.slice(q.bytes.length - 472)])
    assert.deepStrictEqual(Array.from(await verifyAccountables(params, A, msgs, lists, [swap(proofs[0], proofs[2]), proofs[1], swap(proofs[2], proofs[0])])), [false, true, false])
    assert.deepStrictEqual(Array.from(await verifyAccountables(params, A, [msgs[1], msgs[1], msgs[2]], lists, proofs)), [false, true, true])
    assert.deepStrictEqual(Array.from(await verifyAccountables(params, A2, msgs, lists, proofs)), [false, false, false])
    // one list per proof, all the same: one-ring bundles
    const two = [0, 2], pick = (f) => two.map((i) => signers[i][f])
    const same = await proveAccountables(params, A, pick('msgHash'), pick('signature'), pick('publicKey'), [1, 5], [keysA, keysA])
    assert.deepStrictEqual(Array.from(await verifyAccountables(params, A, pick('msgHash'), keysA, same)), [true, true])
    assert.deepStrictEqual(Array.from(await verifyAccountables(params, A, pick('msgHash'), [keysA, keysA], same)), [true, true])
    // one key list per proof, no more, no fewer
    await assert.rejects(verifyAccountables(params, A, msgs, [keysA, keysB], proofs), RangeError)
    await assert.rejects(proveAccountables(params, A, msgs, col('signature'), col('publicKey'), whichs, [keysA, keysB]), RangeError)
    await assert.rejects(openAccountables(params, a, [keysA, keysB], proofs), RangeError)
    console.log('accountable rings ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
