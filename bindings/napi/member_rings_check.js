// node member_rings_check.js   on an MI355X (ZKATTEST_NODE: the addon): membership proofs with one key list per entry behind the facade
// (tests/test_napi_member_rings.py).  proveMembershipLists / verifyMembershipLists over three interleaved key lists of different sizes: every proof verifies
// under its own list and is byte for byte what the one-list call gives; under another list of the same size it does not verify, under a list of another size
// the length check says false; a commitment that does not open to its list's keys[index] is refused; a batch of one list and an empty batch work.
const assert = require('assert')
const zk = require('./zkattest.js')
const { generatePedersenParams, tomEdwards256, Commitment, Scalar, proveMembershipLists, verifyMembershipLists, proveMemberships, verifyMemberships } = zk

async function main() {
    const params = generatePedersenParams(tomEdwards256)
    const small = Object.freeze([11n, 22n, 33n, 44n, 55n]), other = Object.freeze([12n, 23n, 34n, 45n, 56n])
    const big = Object.freeze(Array.from({ length: 20 }, (_, i) => BigInt(1000 + i)))
    const lists = [small, big, other, big, small, other, big]
    const indices = [3, 19, 0, 7, 4, 2, 0]
    // blinders fixed here, so that the one-list calls below prove the same statements
    const coms = lists.map((keys, i) => { const r = new Scalar(tomEdwards256, BigInt(7000 + i)); return new Commitment(params.h.mul(r).add(params.g.mul(new Scalar(tomEdwards256, keys[indices[i]]))), r) })
    const pts = coms.map((c) => c.p)
    const proofs = await proveMembershipLists(params, coms, indices, lists)
    assert.deepStrictEqual(proofs.map((p) => p.n), [3, 5, 3, 5, 3, 3, 5])
    assert.deepStrictEqual(Array.from(await verifyMembershipLists(params, pts, lists, proofs)), lists.map(() => true))
    // the one-list calls agree: the verifier on every proof, the statements' commitments through the prover's own check
    for (const keys of [small, big, other]) {
        const sel = lists.map((l, i) => (l === keys ? i : -1)).filter((i) => i >= 0)
        assert.deepStrictEqual(Array.from(await verifyMemberships(params, sel.map((i) => pts[i]), keys, sel.map((i) => proofs[i]))), sel.map(() => true))
        const again = await proveMemberships(params, sel.map((i) => coms[i]), sel.map((i) => indices[i]), keys)
        assert.deepStrictEqual(Array.from(await verifyMembershipLists(params, sel.map((i) => pts[i]), sel.map(() => keys), again)), sel.map(() => true))
    }
    // another list of the same size: the relations fail; a list of another size: the length check; another commitment: false
    const swapped = [other, small, small, big, big, other, small]
    assert.deepStrictEqual(Array.from(await verifyMembershipLists(params, pts, swapped, proofs)), [false, false, false, true, false, true, false])
    assert.deepStrictEqual(Array.from(await verifyMembershipLists(params, [pts[4], pts[1], pts[2]], [small, big, other], proofs.slice(0, 3))), [false, true, true])
    // a commitment that does not open to its list's keys[index]
    await assert.rejects(proveMembershipLists(params, coms, [3, 19, 1, 7, 4, 2, 0], lists), /does not commit/)
    await assert.rejects(proveMembershipLists(params, coms, indices, lists.slice(1)), RangeError)
    // one list only; nothing
    const one = await proveMembershipLists(params, [coms[1], coms[3]], [19, 7], [big, big])
    assert.deepStrictEqual(Array.from(await verifyMembershipLists(params, [pts[1], pts[3]], [big, big], one)), [true, true])
    assert.deepStrictEqual(one.map((p) => p.n), [5, 5])
    assert.deepStrictEqual(await proveMembershipLists(params, [], [], []), [])
    assert.deepStrictEqual(Array.from(await verifyMembershipLists(params, [], [], [])), [])
    console.log('member rings ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
