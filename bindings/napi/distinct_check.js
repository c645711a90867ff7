// node distinct_check.js   on an MI355X (ZKATTEST_NODE: the addon): distinct-key proofs behind the facade (tests/test_napi_distinct.py).
// proveDifferentKeys / verifyDifferentKeys over two commitments to different keys: the proof verifies, a flipped response, swapped commitments and another
// commitment do not, the prover refuses equal keys and an opening that does not hold; the batched forms and distinctPairs count three signers.  The last line
// is a JSON record of one proof made from pinned seeds, with everything the Python binding needs to make the same bytes.
const assert = require('assert')
const crypto = require('crypto')
const zk = require('./zkattest.js')
const { generateParamsList, tomEdwards256, commit, proveDifferentKeys, verifyDifferentKeys, proveDifferentKeysBatch, verifyDifferentKeysBatch, distinctPairs, DistinctProof,
    proveSameKey, verifySameKey } = zk

async function main() {
    assert.strictEqual(proveDifferentKeys.length, 7)
    assert.strictEqual(verifyDifferentKeys.length, 4)
    assert.deepStrictEqual(distinctPairs(3), [[0, 1], [0, 2], [1, 2]])
    assert.deepStrictEqual(distinctPairs(4), [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]])
    assert.deepStrictEqual(distinctPairs(1), [])
    const params = generateParamsList(80), pp = params.ProofGroup
    const keys = [1234567n, 1234568n, 99n, 1234567n]
    const c = keys.map((k) => commit(pp, k))
    const d = await proveDifferentKeys(params, keys[0], c[0].p, c[0].r, keys[1], c[1].p, c[1].r)
    assert.ok(d instanceof DistinctProof && d.bytes.length === 744 && d.bytes.slice(0, 4).toString('latin1') === 'ZKD1' && d.bytes.readUInt32BE(4) === 744)
    assert.ok([d.C_w, d.C_4, d.A_x, d.A_y, d.A_z, d.A_4_1, d.A_4_2].every((p) => tomEdwards256.isOnGroup(p)) && d.t_r4.k < tomEdwards256.order)
    assert.strictEqual(await verifyDifferentKeys(params, c[0].p, c[1].p, d), true)
    assert.strictEqual(await verifyDifferentKeys(params, c[0], c[1], d.bytes), true)           // Commitments and raw bytes are taken too
    assert.strictEqual(await verifyDifferentKeys(params, c[1].p, c[0].p, d), false)            // the proof is directional
    assert.strictEqual(await verifyDifferentKeys(params, c[0].p, c[2].p, d), false)
    assert.strictEqual(await verifyDifferentKeys(params, c[0].p, c[0].p, d), false)
    const bad = Buffer.from(d.bytes)
    bad[743] ^= 1                                                                              // t_r4 alone: relation 4
    assert.strictEqual(await verifyDifferentKeys(params, c[0].p, c[1].p, new DistinctProof(bad)), false)
    await assert.rejects(proveDifferentKeys(params, keys[0], c[0].p, c[0].r, keys[3], c[3].p, c[3].r), /hide the same key/)
    assert.strictEqual(await verifySameKey(params, c[0].p, c[3].p, await proveSameKey(params, keys[0], c[0].p, c[0].r, c[3].p, c[3].r)), true)
    await assert.rejects(proveDifferentKeys(params, keys[0], c[0].p, c[1].r, keys[1], c[1].p, c[1].r), /do not open/)
    const offCurve = Buffer.concat([Buffer.alloc(35), Buffer.from([5]), Buffer.alloc(35), Buffer.from([7])])
    await assert.rejects(proveDifferentKeys(params, keys[0], offCurve, c[0].r, keys[1], c[1].p, c[1].r), /deserializ/)
    await assert.rejects(verifyDifferentKeys(params, offCurve, c[1].p, d), /deserializ/)
    assert.throws(() => new DistinctProof(d.bytes.slice(0, 743)), /deserializing/)
    assert.ok(!(await proveDifferentKeys(params, keys[0], c[0].p, c[0].r, keys[1], c[1].p, c[1].r)).eq(d))   // fresh seeds per call
    // three signers: one proof per pair
    const pairs = distinctPairs(3), col = (f) => pairs.map(f)
    const ds = await proveDifferentKeysBatch(params, col(([i]) => keys[i]), col(([i]) => c[i].p), col(([i]) => c[i].r), col(([, j]) => keys[j]), col(([, j]) => c[j].p), col(([, j]) => c[j].r))
    assert.deepStrictEqual(Array.from(await verifyDifferentKeysBatch(params, col(([i]) => c[i].p), col(([, j]) => c[j].p), ds)), [true, true, true])
    assert.deepStrictEqual(Array.from(await verifyDifferentKeysBatch(params, col(([, j]) => c[j].p), col(([i]) => c[i].p), ds)), [false, false, false])
    await assert.rejects(proveDifferentKeysBatch(params, [1n], [c[0].p, c[1].p], [c[0].r], [2n], [c[1].p], [c[1].r]), RangeError)
    assert.deepStrictEqual(await proveDifferentKeysBatch(params, [], [], [], [], [], []), [])
    // one proof from pinned seeds, for the Python binding to make again
    const pinned = (n) => Buffer.from(Array.from({ length: n }, (_, i) => (13 * i + 7) & 255))
    const randomBytes = crypto.randomBytes
    crypto.randomBytes = pinned
    let fixed
    try {
        fixed = await proveDifferentKeys(params, keys[0], c[0].p, c[0].r, keys[2], c[2].p, c[2].r)
    } finally {
        crypto.randomBytes = randomBytes
    }
    const ep = params.engineParams(), hex = (b) => Buffer.from(b).toString('hex'), xy = (p) => p.x.toString(16).padStart(72, '0') + p.y.toString(16).padStart(72, '0')
    console.log('distinct ok')
    console.log(JSON.stringify({ nistH: hex(ep.nistH), tomG: hex(ep.tomG), tomH: hex(ep.tomH), sec: ep.secLevel, key1: keys[0].toString(), r1: c[0].r.k.toString(), com1: xy(c[0].p),
        key2: keys[2].toString(), r2: c[2].r.k.toString(), com2: xy(c[2].p), seed: hex(pinned(32)), proof: hex(fixed.bytes) }))
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
