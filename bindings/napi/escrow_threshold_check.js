// node escrow_threshold_check.js   on an MI355X (ZKATTEST_NODE: the addon): t of n auditors open escrow tags (tests/test_napi_escrow_threshold.py).
// splitAuditorKey 3-of-5; every auditor's shares verify; three subsets of auditors combine to what openEscrowTags gives for the undivided secret, with one key
// list and with one key list per tag; a share with another D fails its verifier and combines to nobody; a wrong share secret, too few rows and a set with one
// replaced key are refused.
const assert = require('assert')
const zk = require('./zkattest.js')
const { generatePedersenParams, tomEdwards256, commit, proveEscrowTags, openEscrowTags, splitAuditorKey, shareEscrowTags, verifyEscrowShares, combineEscrowShares, EscrowShare } = zk

async function main() {
    assert.strictEqual(combineEscrowShares.length, 5)
    const pp = generatePedersenParams(tomEdwards256)
    const a = 0xfedcba0987654321fedcba0987654321n
    const set = await splitAuditorKey(pp, a, 3, 5)
    assert.ok(set.t === 3 && set.keys.length === 5 && set.shares.length === 5 && set.shares.every((s) => s.length === 32))
    const ringA = Object.freeze([11n, 12n, 13n, 12n, 15n]), ringB = Object.freeze([21n, 22n])
    const xs = [12n, 22n, 11n, 777n]
    const cs = xs.map((x) => commit(pp, x))
    const tags = await proveEscrowTags(pp, set.key, xs, cs.map((c) => c.p), cs.map((c) => c.r))
    const lists = [ringA, ringB, ringA, ringB]
    const want = await openEscrowTags(pp, a, lists, tags)
    assert.deepStrictEqual(want, [{ ring: 0, index: 1 }, { ring: 1, index: 1 }, { ring: 0, index: 0 }, null])
    const sh = {}
    for (let j = 1; j <= 5; j++) {
        sh[j] = await shareEscrowTags(pp, set, j, set.shares[j - 1], tags)
        assert.ok(sh[j].every((s) => s instanceof EscrowShare && s.j === j && s.bytes.length === 264))
        assert.deepStrictEqual(await verifyEscrowShares(pp, set, tags, sh[j]), [true, true, true, true])
    }
    for (const S of [[1, 2, 3], [5, 4, 3], [5, 2, 3]]) assert.deepStrictEqual(await combineEscrowShares(pp, set, lists, tags, S.map((j) => sh[j])), want)
    // one key list: indices, as openEscrowTags' one-ring form; raw bytes are taken too
    const inA = [0, 2]
    assert.deepStrictEqual(await combineEscrowShares(pp, set, ringA, inA.map((i) => tags[i].bytes), [2, 4, 1].map((j) => inA.map((i) => sh[j][i].bytes))), [1, 0])
    assert.deepStrictEqual(await combineEscrowShares(pp, set, ringA, inA.map((i) => tags[i]), [2, 4, 1].map((j) => inA.map((i) => sh[j][i]))), await openEscrowTags(pp, a, ringA, inA.map((i) => tags[i])))
    // a share whose D is another auditor's: it fails its verifier, and the combine opens that tag to nobody
    const bad = Buffer.from(sh[2][0].bytes)
    sh[4][0].bytes.copy(bad, 16, 16, 88)
    assert.deepStrictEqual(await verifyEscrowShares(pp, set, tags, [bad, ...sh[2].slice(1)]), [false, true, true, true])
    assert.deepStrictEqual(await combineEscrowShares(pp, set, lists, tags, [sh[1], [bad, ...sh[2].slice(1)], sh[3]]), [null, ...want.slice(1)])
    // refusals: a share secret of another auditor, too few rows, the same auditor twice, a set with one replaced key
    await assert.rejects(shareEscrowTags(pp, set, 1, set.shares[1], tags))
    await assert.rejects(combineEscrowShares(pp, set, lists, tags, [sh[1], sh[2]]), RangeError)
    await assert.rejects(combineEscrowShares(pp, set, lists, tags, [sh[1], sh[2], sh[1]]))
    await assert.rejects(verifyEscrowShares(pp, { key: set.key, t: 3, keys: [set.keys[1], ...set.keys.slice(1)] }, tags, sh[1]))
    assert.deepStrictEqual(await verifyEscrowShares(pp, set, tags, sh[5]), [true, true, true, true])   // ... and the good set is installed again
    assert.throws(() => new EscrowShare(Buffer.alloc(264)))
    assert.deepStrictEqual(await combineEscrowShares(pp, set, lists, [], [[], [], []]), [])
    console.log('escrow threshold ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
