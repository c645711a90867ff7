// node escrow_rings_check.js   on an MI355X (ZKATTEST_NODE: the addon): escrow tags opened against several key rings in one call (tests/test_napi_escrow_rings.py).
// openEscrowTags with one key list per tag: tags interleaved over three rings open to { ring, index } in their own list (the lowest index of a key that occurs
// twice, the ring counted by first appearance), a key outside its list and a key that sits in ANOTHER list than the tag's open to nobody, and the answers equal
// the one-ring form's ring by ring.
const assert = require('assert')
const zk = require('./zkattest.js')
const { generatePedersenParams, tomEdwards256, commit, proveEscrowTags, openEscrowTags, escrowAuditorKey } = zk

async function main() {
    assert.strictEqual(openEscrowTags.length, 4)
    const pp = generatePedersenParams(tomEdwards256)
    const a = 0xfedcba0987654321fedcba0987654321n
    const A = await escrowAuditorKey(pp, a)
    const ringA = Object.freeze([11n, 12n, 13n, 12n, 15n]), ringB = Object.freeze([21n, 22n]), ringC = Object.freeze(Array.from({ length: 300 }, (_, i) => 1000n + BigInt(i)))
    const xs = [12n, 22n, 1299n, 11n, 21n, 1000n, 777n, 13n]
    const cs = xs.map((x) => commit(pp, x))
    const tags = await proveEscrowTags(pp, A, xs, cs.map((c) => c.p), cs.map((c) => c.r))
    //            12 in A   22 in B   1299 in C   11 in A   21 in B   1000 in C   777 nowhere   13 asked of B: it sits in A only
    const lists = [ringA, ringB, ringC, ringA, ringB, ringC, ringC, ringB]
    const got = await openEscrowTags(pp, a, lists, tags)
    assert.deepStrictEqual(got, [{ ring: 0, index: 1 }, { ring: 1, index: 1 }, { ring: 2, index: 299 }, { ring: 0, index: 0 }, { ring: 1, index: 0 }, { ring: 2, index: 0 }, null, null])
    // ring by ring, the one-ring form says the same
    for (const [r, ring] of [ringA, ringB, ringC].entries()) {
        const sel = lists.map((l, i) => (l === ring ? i : -1)).filter((i) => i >= 0)
        const one = await openEscrowTags(pp, a, ring, sel.map((i) => tags[i]))
        assert.deepStrictEqual(one, sel.map((i) => (got[i] === null ? null : got[i].index)))
        assert.ok(sel.every((i) => got[i] === null || got[i].ring === r))
    }
    // the order of first appearance numbers the rings; raw bytes are taken too
    assert.deepStrictEqual(await openEscrowTags(pp, a, [ringC, ringA], [tags[2].bytes, tags[0]]), [{ ring: 0, index: 299 }, { ring: 1, index: 1 }])
    await assert.rejects(openEscrowTags(pp, a, [ringA], tags.slice(0, 2)), RangeError)
    assert.deepStrictEqual(await openEscrowTags(pp, a, [ringA], []), [])
    assert.deepStrictEqual(await openEscrowTags(pp, a + 1n, [ringA, ringB], tags.slice(0, 2)), [null, null])   // another auditor's secret opens to nobody
    console.log('escrow rings ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
