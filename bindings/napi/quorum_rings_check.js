// node quorum_rings_check.js   on an MI355X (ZKATTEST_NODE: the addon): quorum proofs whose members sit in different rings, behind the facade
// (tests/test_napi_quorum_rings.py).  proveQuorum / verifyQuorum take one key list per member in the place of `keys` (the convention of reringSignatureLists):
// three signers over two registries of different size -> a QuorumProof that verifyQuorum accepts with the same lists; a key enrolled in both registries and
// used through both throws 'the same key'; the wrong registry for a member, a tampered bundle and another hash give false; with one list throughout the
// bundle verifies through the one-ring form as well.
const assert = require('assert')
const crypto = require('crypto')
const zk = require('./zkattest.js')
const { generateParamsList, keyToInt, proveQuorum, verifyQuorum, QuorumProof, verifySignatureLists } = zk

async function main() {
    const params = generateParamsList(80)
    const signers = []
    for (let r = 0; r < 4; r++) {
        const keyPair = crypto.generateKeyPairSync('ec', { namedCurve: 'P-256' }), msg = Buffer.from('quorum rings ' + r)
        signers.push({ msgHash: crypto.createHash('sha256').update(msg).digest(), publicKey: keyPair.publicKey, x: await keyToInt(keyPair.publicKey),
            signature: crypto.sign('sha256', msg, { key: keyPair.privateKey, dsaEncoding: 'ieee-p1363' }) })
    }
    // registry A: 7 keys (padded to 8), signers 0 and 2 at 1 and 5; registry B: 19 keys (padded to 32), signer 1 at 3 and signer 0 AGAIN at 17
    const keysA = Object.freeze([21n, signers[0].x, 5n, 6n, 77n, signers[2].x, 9n])
    const keysB = Object.freeze(Array.from({ length: 19 }, (_, i) => (i === 3 ? signers[1].x : i === 17 ? signers[0].x : BigInt(1000 + i))))
    const pick = (idx, f) => idx.map((i) => signers[i][f])
    const three = [0, 1, 2], whichs = [1, 3, 5], lists = [keysA, keysB, keysA]
    const proof = await proveQuorum(params, pick(three, 'msgHash'), pick(three, 'signature'), pick(three, 'publicKey'), whichs, lists)
    assert.ok(proof instanceof QuorumProof && proof.k === 3 && proof.bytes.readUInt32BE(4) === proof.bytes.length)
    const att = proof.attestations
    assert.deepStrictEqual(att.map((a) => a.bytes.readUInt32BE(12)), [3, 5, 3])   // the inner headers' n: rings of 8, 32 and 8 padded keys
    assert.deepStrictEqual(Array.from(await verifySignatureLists(params, pick(three, 'msgHash'), lists, att)), [true, true, true])
    assert.strictEqual(await verifyQuorum(params, pick(three, 'msgHash'), lists, proof), true)
    assert.strictEqual(await verifyQuorum(params, pick(three, 'msgHash'), lists, proof.bytes), true)
    // the wrong registry for member 1; a tampered pair; another hash
    assert.strictEqual(await verifyQuorum(params, pick(three, 'msgHash'), [keysA, keysA, keysA], proof), false)
    assert.strictEqual(await verifyQuorum(params, pick(three, 'msgHash'), [keysB, keysA, keysA], proof), false)
    const bad = Buffer.from(proof.bytes)
    bad[bad.length - 1] ^= 1
    assert.strictEqual(await verifyQuorum(params, pick(three, 'msgHash'), lists, bad), false)
    assert.strictEqual(await verifyQuorum(params, pick([0, 3, 2], 'msgHash'), lists, proof), false)
    // signer 0 through registry A and again through registry B: the same key, whatever ring it is shown in
    await assert.rejects(proveQuorum(params, pick([0, 1, 0], 'msgHash'), pick([0, 1, 0], 'signature'), pick([0, 1, 0], 'publicKey'), [1, 3, 17], [keysA, keysB, keysB]), /the same key/)
    // one list per member, all the same: the bundle is a one-ring bundle
    const two = [0, 2]
    const same = await proveQuorum(params, pick(two, 'msgHash'), pick(two, 'signature'), pick(two, 'publicKey'), [1, 5], [keysA, keysA])
    assert.strictEqual(await verifyQuorum(params, pick(two, 'msgHash'), keysA, same), true)
    assert.strictEqual(await verifyQuorum(params, pick(two, 'msgHash'), [keysA, keysA], same), true)
    // one key list per member, no more, no fewer
    await assert.rejects(verifyQuorum(params, pick(three, 'msgHash'), [keysA, keysB], proof), RangeError)
    await assert.rejects(proveQuorum(params, pick(three, 'msgHash'), pick(three, 'signature'), pick(three, 'publicKey'), whichs, [keysA, keysB]), RangeError)
    console.log('quorum rings ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
