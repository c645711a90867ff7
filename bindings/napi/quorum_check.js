// node quorum_check.js   on an MI355X (ZKATTEST_NODE: the addon): quorum proofs behind the facade (tests/test_napi_quorum.py).
// proveQuorum over three attestations by three different ring members -> a QuorumProof that verifyQuorum accepts; a repeated signer throws; a tampered
// bundle, another message hash and swapped members give false; a bundle that does not deserialise throws.
const assert = require('assert')
const crypto = require('crypto')
const zk = require('./zkattest.js')
const { generateParamsList, keyToInt, proveQuorum, verifyQuorum, QuorumProof, SignatureProofList, DistinctProof, verifySignatureListBatch, distinctPairs } = zk

async function main() {
    assert.strictEqual(proveQuorum.length, 6)
    assert.strictEqual(verifyQuorum.length, 4)
    const params = generateParamsList(80)
    const signers = []
    for (let r = 0; r < 4; r++) {
        const keyPair = crypto.generateKeyPairSync('ec', { namedCurve: 'P-256' }), msg = Buffer.from('quorum ' + r)
        signers.push({ msgHash: crypto.createHash('sha256').update(msg).digest(), publicKey: keyPair.publicKey, x: await keyToInt(keyPair.publicKey),
            signature: crypto.sign('sha256', msg, { key: keyPair.privateKey, dsaEncoding: 'ieee-p1363' }) })
    }
    const keys = Object.freeze([21n, signers[0].x, 5n, signers[1].x, 77n, signers[2].x, 9n])   // signers 0, 1, 2 at 1, 3, 5
    const pick = (idx, f) => idx.map((i) => signers[i][f])
    const three = [0, 1, 2], whichs = [1, 3, 5]
    const proof = await proveQuorum(params, pick(three, 'msgHash'), pick(three, 'signature'), pick(three, 'publicKey'), whichs, keys)
    assert.ok(proof instanceof QuorumProof && proof.k === 3 && proof.bytes.slice(0, 4).toString('latin1') === 'ZKQ1' && proof.bytes.readUInt32BE(4) === proof.bytes.length)
    const att = proof.attestations, dps = proof.distinctProofs
    assert.ok(att.length === 3 && att.every((a) => a instanceof SignatureProofList) && dps.length === distinctPairs(3).length && dps.every((d) => d instanceof DistinctProof))
    assert.strictEqual(16 + att.reduce((s, a) => s + a.bytes.length, 0) + 744 * 3, proof.bytes.length)
    assert.deepStrictEqual(Array.from(await verifySignatureListBatch(params, pick(three, 'msgHash'), keys, att)), [true, true, true])
    assert.strictEqual(await verifyQuorum(params, pick(three, 'msgHash'), keys, proof), true)
    assert.strictEqual(await verifyQuorum(params, pick(three, 'msgHash'), keys, proof.bytes), true)   // raw bytes are taken too
    assert.ok(new QuorumProof(Buffer.from(proof.bytes)).eq(proof))
    // a repeated signer: members 0 and 2 are the same ring member (another message would do as well)
    await assert.rejects(proveQuorum(params, pick([0, 1, 0], 'msgHash'), pick([0, 1, 0], 'signature'), pick([0, 1, 0], 'publicKey'), [1, 3, 1], keys), /the same key/)
    // tampered: the last response of the last pair; another message hash for member 1; the hashes in another order
    const bad = Buffer.from(proof.bytes)
    bad[bad.length - 1] ^= 1
    assert.strictEqual(await verifyQuorum(params, pick(three, 'msgHash'), keys, bad), false)
    assert.strictEqual(await verifyQuorum(params, pick([0, 3, 2], 'msgHash'), keys, proof), false)
    assert.strictEqual(await verifyQuorum(params, pick([1, 0, 2], 'msgHash'), keys, proof), false)
    // members 0 and 1 swapped with their hashes: the attestations verify, the pair (0, 1) does not
    const o = proof.offsets, b = proof.bytes
    const swapped = Buffer.concat([b.slice(0, 16), b.slice(o[1], o[2]), b.slice(o[0], o[1]), b.slice(o[2])])
    assert.strictEqual(await verifyQuorum(params, pick([1, 0, 2], 'msgHash'), keys, swapped), false)
    // what does not deserialise throws
    assert.throws(() => new QuorumProof(b.slice(0, b.length - 4)), /deserializing/)
    const k4 = Buffer.from(b)
    k4.writeUInt32BE(4, 8)
    assert.throws(() => new QuorumProof(k4), /deserializing/)
    await assert.rejects(verifyQuorum(params, pick([0, 1], 'msgHash'), keys, proof), RangeError)
    await assert.rejects(proveQuorum(params, pick([0], 'msgHash'), pick([0], 'signature'), pick([0], 'publicKey'), [1], keys), RangeError)
    assert.ok(!(await proveQuorum(params, pick(three, 'msgHash'), pick(three, 'signature'), pick(three, 'publicKey'), whichs, keys)).eq(proof))   // fresh seeds per call
    console.log('quorum ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
