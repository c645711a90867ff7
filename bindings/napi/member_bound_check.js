// node member_bound_check.js   on an MI355X (ZKATTEST_NODE: the addon): bound membership proofs ("ZKMB") behind the facade (tests/test_napi_member_bound.py).
// options.context on proveMembership / verifyMembership, their batched forms and the Lists forms: a proof made with a context is a ZKMB proof of the ZKM1
// size, verifies with that context and its commitment, and gives false with a flipped context bit, another entry's context or another commitment; in a
// call without a context it does not deserialise, and neither does an unbound proof in a call with one; with one key list per entry every proof is bound to
// its own list; the calls without options are what they were; malformed options are refused before the engine is asked.
const assert = require('assert')
const zk = require('./zkattest.js')
const { generatePedersenParams, tomEdwards256, commit, proveMembership, verifyMembership, proveMemberships, verifyMemberships, proveMembershipLists, verifyMembershipLists,
    GKProof } = zk

const ctxOf = (i) => Uint8Array.from({ length: 32 }, (_, k) => (37 * i + 11 * k + 5) & 255)
const flip = (c, byte, bit) => { const d = Uint8Array.from(c); d[byte] ^= bit; return d }

async function main() {
    const params = generatePedersenParams(tomEdwards256)
    const keys = Object.freeze([11n, 22n, 33n, 44n, 55n]), other = Object.freeze([12n, 23n, 33n, 45n, 56n])   // 33n sits at index 2 of both
    const big = Object.freeze(Array.from({ length: 20 }, (_, i) => BigInt(1000 + i)))
    assert.strictEqual(proveMembership.length, 4)   // the reference's parameter lists; options ride behind them
    assert.strictEqual(verifyMembership.length, 4)
    // ---- the single calls
    const com = commit(params, keys[2]), context = ctxOf(0)
    const proof = await proveMembership(params, com, 2, keys, { context })
    assert.ok(proof instanceof GKProof && proof.bound && proof.n === 3 && proof.bytes.length === 16 + 384 * 3 + 32)
    assert.strictEqual(proof.bytes.slice(0, 4).toString('latin1'), 'ZKMB')
    assert.ok(proof.cd.every((p) => tomEdwards256.isOnGroup(p)) && proof.zd.k < tomEdwards256.order)
    assert.strictEqual(await verifyMembership(params, com.p, keys, proof, { context }), true)
    assert.strictEqual(await verifyMembership(params, com.p, keys, proof, { context: flip(context, 0, 1) }), false)
    assert.strictEqual(await verifyMembership(params, com.p, keys, proof, { context: flip(context, 31, 0x80) }), false)
    assert.strictEqual(await verifyMembership(params, com.p, keys, proof, { context: ctxOf(1) }), false)
    assert.strictEqual(await verifyMembership(params, com.p, other, proof, { context }), false)   // a ring of the same size that holds the value at the same index
    const again = commit(params, keys[2])   // the same value under another blinder
    assert.strictEqual(await verifyMembership(params, again.p, keys, proof, { context }), false)
    // each verifier takes its own magic only
    await assert.rejects(verifyMembership(params, com.p, keys, proof), /deserializ/)
    const plain = await proveMembership(params, com, 2, keys)
    assert.ok(!plain.bound && plain.bytes.slice(0, 4).toString('latin1') === 'ZKM1')
    assert.strictEqual(await verifyMembership(params, com.p, keys, plain), true)
    assert.strictEqual(await verifyMembership(params, com.p, keys, plain, {}), true)   // options without a context: the unbound call
    await assert.rejects(verifyMembership(params, com.p, keys, plain, { context }), /deserializ/)
    const relabelled = Buffer.from(plain.bytes)
    relabelled.write('ZKMB', 0, 'latin1')   // the unbound transcript under the bound magic: another challenge
    assert.strictEqual(await verifyMembership(params, com.p, keys, new GKProof(relabelled), { context }), false)
    // the prover's own check is the unbound call's
    await assert.rejects(proveMembership(params, commit(params, 34n), 2, keys, { context }), /does not commit/)
    // ---- batched over one list
    const idx = [0, 7, 19], coms = idx.map((i) => commit(params, big[i])), ctxs = idx.map((_, i) => ctxOf(10 + i)), pts = coms.map((c) => c.p)
    const proofs = await proveMemberships(params, coms, idx, big, { context: ctxs })
    assert.ok(proofs.every((p) => p.bound && p.n === 5))
    assert.deepStrictEqual(Array.from(await verifyMemberships(params, pts, big, proofs, { context: ctxs })), [true, true, true])
    assert.deepStrictEqual(Array.from(await verifyMemberships(params, pts, big, proofs, { context: [ctxs[1], ctxs[0], ctxs[2]] })), [false, false, true])
    assert.deepStrictEqual(Array.from(await verifyMemberships(params, [pts[1], pts[0], pts[2]], big, proofs, { context: ctxs })), [false, false, true])
    assert.strictEqual(await verifyMembership(params, pts[1], big, proofs[1], { context: ctxs[1] }), true)   // the single call on a batch's proof
    // ---- one key list per entry
    const lists = [keys, big, other, big, keys], lidx = [2, 19, 2, 0, 4]
    const lcoms = lists.map((l, i) => commit(params, l[lidx[i]])), lctx = lists.map((_, i) => ctxOf(20 + i)), lpts = lcoms.map((c) => c.p)
    const lproofs = await proveMembershipLists(params, lcoms, lidx, lists, { context: lctx })
    assert.deepStrictEqual(lproofs.map((p) => [p.n, p.bound]), [[3, true], [5, true], [3, true], [5, true], [3, true]])
    assert.deepStrictEqual(Array.from(await verifyMembershipLists(params, lpts, lists, lproofs, { context: lctx })), lists.map(() => true))
    // entries 0 and 2 commit to 33n at index 2 of two lists of equal size: each proof holds under its own list only
    assert.deepStrictEqual(Array.from(await verifyMembershipLists(params, lpts, [other, big, keys, big, keys], lproofs, { context: lctx })), [false, true, false, true, true])
    assert.deepStrictEqual(Array.from(await verifyMembershipLists(params, lpts, lists, lproofs, { context: [lctx[0], lctx[3], lctx[2], lctx[1], lctx[4]] })), [true, false, true, false, true])
    // the one-list bound verifier agrees on a Lists proof
    assert.deepStrictEqual(Array.from(await verifyMemberships(params, [lpts[1], lpts[3]], big, [lproofs[1], lproofs[3]], { context: [lctx[1], lctx[3]] })), [true, true])
    await assert.rejects(verifyMembershipLists(params, lpts, lists, lproofs), /deserializ/)
    // ---- options that are not what the calls take
    await assert.rejects(proveMembership(params, com, 2, keys, { context: new Uint8Array(31) }), TypeError)
    await assert.rejects(proveMembership(params, com, 2, keys, { context: 'nonce' }), TypeError)
    await assert.rejects(proveMemberships(params, coms, idx, big, { context: ctxs.slice(1) }), RangeError)
    await assert.rejects(proveMemberships(params, coms, idx, big, { context: ctxs[0] }), RangeError)
    await assert.rejects(verifyMembershipLists(params, lpts, lists, lproofs, { context: lctx.concat([ctxOf(99)]) }), RangeError)
    assert.deepStrictEqual(await proveMemberships(params, [], [], big, { context: [] }), [])
    console.log('member bound ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
