// node escrow_check.js   on an MI355X (ZKATTEST_NODE: the addon): escrow tags behind the facade (tests/test_napi_escrow.py).
// proveEscrowTag / verifyEscrowTag over a commitment and an auditor's key: the tag verifies, a flipped response, another commitment and another auditor's key do
// not, the prover refuses an opening that does not hold; openEscrowTags finds the ring member (the lowest index of a key that occurs twice) and nobody for a key
// outside the ring; the batched forms agree with the single ones.  Then the flow the calls exist for: attestations, their keyXcoms and blinders, a tag beside
// each, both verifiers, the opening -- in both wire layouts.
const assert = require('assert')
const crypto = require('crypto')
const zk = require('./zkattest.js')
const { generatePedersenParams, generateParamsList, tomEdwards256, commit, keyToInt, proveSignatureListBatch, verifySignatureListBatch, keyBlinders, keyCommitments,
    proveEscrowTag, verifyEscrowTag, proveEscrowTags, verifyEscrowTags, openEscrowTags, escrowAuditorKey, EscrowTag, setWireLayout } = zk

async function main() {
    assert.strictEqual(proveEscrowTag.length, 5)
    assert.strictEqual(verifyEscrowTag.length, 4)
    assert.strictEqual(openEscrowTags.length, 4)
    // one commitment on bare Pedersen parameters
    const pp = generatePedersenParams(tomEdwards256)
    const a = 0x1234567890abcdef1234567890abcdefn, a2 = a + 1n
    const A = await escrowAuditorKey(pp, a), A2 = await escrowAuditorKey(pp, a2)
    assert.ok(tomEdwards256.isOnGroup(A) && !A.eq(A2))
    await assert.rejects(escrowAuditorKey(pp, tomEdwards256.order), /argument/i)   // a = 0 mod q
    const c = commit(pp, 1234567n), other = commit(pp, 1234568n)
    const tag = await proveEscrowTag(pp, A, 1234567n, c.p, c.r)
    assert.ok(tag instanceof EscrowTag && tag.bytes.length === 472 && tag.bytes.slice(0, 4).toString('latin1') === 'ZKT1' && tag.bytes.readUInt32BE(4) === 472)
    assert.ok([tag.E1, tag.E2, tag.T1, tag.T2, tag.T3].every((p) => tomEdwards256.isOnGroup(p)) && tag.t_x.k < tomEdwards256.order)
    assert.strictEqual(await verifyEscrowTag(pp, A, c.p, tag), true)
    assert.strictEqual(await verifyEscrowTag(pp, A, c, tag.bytes), true)             // Commitments and raw bytes are taken too
    assert.strictEqual(await verifyEscrowTag(pp, A, other.p, tag), false)
    assert.strictEqual(await verifyEscrowTag(pp, A2, c.p, tag), false)               // a tag made for A under A'
    assert.strictEqual(await verifyEscrowTag(pp, A, c.p, tag), true)                 // ... and the engine is back on A
    const bad = Buffer.from(tag.bytes)
    bad[471] ^= 1                                                                    // t_rho alone
    assert.strictEqual(await verifyEscrowTag(pp, A, c.p, new EscrowTag(bad)), false)
    await assert.rejects(proveEscrowTag(pp, A, 1234567n, other.p, other.r), /do not open/)
    await assert.rejects(proveEscrowTag(pp, A, 1234567n, c.p, other.r), /do not open/)
    const offCurve = Buffer.concat([Buffer.alloc(35), Buffer.from([5]), Buffer.alloc(35), Buffer.from([7])])
    await assert.rejects(proveEscrowTag(pp, A, 1234567n, offCurve, c.r), /deserializ/)
    await assert.rejects(verifyEscrowTag(pp, A, offCurve, tag), /deserializ/)
    await assert.rejects(proveEscrowTag(pp, offCurve, 1234567n, c.p, c.r), /deserializ/)   // the auditor's key is checked when it is set
    assert.throws(() => new EscrowTag(tag.bytes.slice(0, 471)), /deserializing/)
    assert.ok(!(await proveEscrowTag(pp, A, 1234567n, c.p, c.r)).eq(tag))            // fresh seeds per call
    // the opening: a ring of five keys with 1234567 at 1 and 4, another key's tag, a key outside the ring
    const keys = Object.freeze([99n, 1234567n, 1234568n, 5n, 1234567n])
    const tags = await proveEscrowTags(pp, A, [1234567n, 1234568n], [c.p, other.p], [c.r, other.r])
    assert.deepStrictEqual(Array.from(await verifyEscrowTags(pp, A, [c.p, other.p], tags)), [true, true])
    assert.deepStrictEqual(Array.from(await verifyEscrowTags(pp, A, [other.p, c.p], tags)), [false, false])
    const out = commit(pp, 777n)
    const outside = await proveEscrowTag(pp, A, 777n, out.p, out.r)
    assert.deepStrictEqual(await openEscrowTags(pp, a, keys, [tag, tags[1], outside, tags[0].bytes]), [1, 2, null, 1])
    assert.deepStrictEqual(await openEscrowTags(pp, a2, keys, [tag]), [null])       // another auditor's secret opens a tag made for A to nobody (and its verify says no)
    assert.strictEqual(await verifyEscrowTag(pp, A, c.p, tag), true)
    await assert.rejects(proveEscrowTags(pp, A, [1n], [c.p, other.p], [c.r]), RangeError)
    assert.deepStrictEqual(await proveEscrowTags(pp, A, [], [], []), [])
    assert.deepStrictEqual(await openEscrowTags(pp, a, keys, []), [])

    // attestations with a tag beside each
    const params = generateParamsList(80)
    const kp = [0, 1].map(() => crypto.generateKeyPairSync('ec', { namedCurve: 'P-256' }))
    const mk = async (who, text) => {
        const msg = Buffer.from(text)
        return { msgHash: crypto.createHash('sha256').update(msg).digest(), publicKey: kp[who].publicKey, x: await keyToInt(kp[who].publicKey),
            signature: crypto.sign('sha256', msg, { key: kp[who].privateKey, dsaEncoding: 'ieee-p1363' }) }
    }
    const att = [await mk(0, 'first'), await mk(0, 'second'), await mk(1, 'third')]
    const ring = Object.freeze([21n, att[0].x, 5n, att[2].x, 77n]), which = [1, 1, 3]
    const col = (f) => att.map((s) => s[f]), msgs = col('msgHash')
    const pinned = (n) => Buffer.from(Array.from({ length: n }, (_, i) => (11 * i + 5) & 255))
    const randomBytes = crypto.randomBytes
    const AA = await escrowAuditorKey(params, a)
    for (const layout of ['zka1', 'zka1p']) {
        setWireLayout(layout)
        crypto.randomBytes = pinned
        let proofs
        try {
            proofs = await proveSignatureListBatch(params, msgs, col('signature'), col('publicKey'), which, ring)
        } finally {
            crypto.randomBytes = randomBytes
        }
        assert.deepStrictEqual(Array.from(await verifySignatureListBatch(params, msgs, ring, proofs)), [true, true, true])
        const blinders = await keyBlinders(pinned(96), params)
        const kx = await keyCommitments(proofs, params)
        const et = await proveEscrowTags(params, AA, col('x'), kx, blinders)
        assert.deepStrictEqual(Array.from(await verifyEscrowTags(params, AA, kx, et)), [true, true, true])
        assert.strictEqual(await verifyEscrowTag(params, AA, kx[2], et[0]), false)    // signer 0's tag beside signer 1's attestation
        assert.deepStrictEqual(await openEscrowTags(params, a, ring, et), which)
    }
    setWireLayout('zka1')
    console.log('escrow ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
