// node member_check.js   on an MI355X (ZKATTEST_NODE: the addon): ring membership on its own behind the facade (tests/test_napi_member.py).
// commit / proveMembership / verifyMembership with the reference's signatures: proofs for ring entries and a padding-free ring verify; a commitment to a value
// outside the ring, a proof moved to another commitment, a flipped response and a proof of another ring's length do not; a commitment that does not open to
// keys[index] is refused by the prover; the batched forms agree with the single ones.
const assert = require('assert')
const zk = require('./zkattest.js')
const { generatePedersenParams, tomEdwards256, commit, proveMembership, verifyMembership, proveMemberships, verifyMemberships, GKProof, Commitment } = zk

async function main() {
    const params = generatePedersenParams(tomEdwards256)
    const keys = Object.freeze([11n, 22n, 33n, 44n, 55n]), big = Object.freeze(Array.from({ length: 20 }, (_, i) => BigInt(1000 + i)))
    const com = commit(params, keys[3])
    assert.ok(com instanceof Commitment && tomEdwards256.isOnGroup(com.p))
    const proof = await proveMembership(params, com, 3, keys)
    assert.ok(proof instanceof GKProof && proof.n === 3 && proof.bytes.length === 16 + 384 * 3 + 32)
    assert.strictEqual(proof.cl.length, 3)
    assert.ok(proof.cd.every((p) => tomEdwards256.isOnGroup(p)) && proof.zd.k < tomEdwards256.order)
    assert.strictEqual(await verifyMembership(params, com.p, keys, proof), true)
    // not a member; another commitment; a flipped response; another ring
    const outside = commit(params, 34n)
    await assert.rejects(proveMembership(params, outside, 2, keys), /does not commit/)
    assert.strictEqual(await verifyMembership(params, outside.p, keys, proof), false)
    const bad = Buffer.from(proof.bytes)
    bad[bad.length - 1] ^= 1
    assert.strictEqual(await verifyMembership(params, com.p, keys, new GKProof(bad)), false)
    const coms = [0, 7, 19].map((i) => commit(params, big[i]))
    const proofs = await proveMemberships(params, coms, [0, 7, 19], big)
    assert.ok(proofs.every((p) => p.n === 5))
    assert.deepStrictEqual(Array.from(await verifyMemberships(params, coms.map((c) => c.p), big, proofs)), [true, true, true])
    assert.deepStrictEqual(Array.from(await verifyMemberships(params, [coms[1].p, coms[0].p, coms[2].p], big, proofs)), [false, false, true])
    assert.strictEqual(await verifyMembership(params, com.p, big, proof), false)       // n = 3 against a ring of n = 5
    assert.strictEqual(await verifyMembership(params, coms[0].p, keys, proofs[0]), false)   // and the other way round
    assert.strictEqual(await verifyMembership(params, com.p, keys, proof), true)
    assert.throws(() => new GKProof(proof.bytes.slice(0, 100)), /deserializing/)
    console.log('member ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
