// node link_check.js   on an MI355X (ZKATTEST_NODE: the addon): link proofs behind the facade (tests/test_napi_link.py).
// proveSameKey / verifySameKey over two commitments to one key: the proof verifies, a flipped response, swapped commitments and a commitment to another key do
// not, the prover refuses an opening that does not hold; the batched forms agree with the single ones.  Then the flow the calls exist for: two attestations by
// one signer and a membership proof in a second registry, tied together through keyCommitment and keyBlinders, in both wire layouts.
const assert = require('assert')
const crypto = require('crypto')
const zk = require('./zkattest.js')
const { generatePedersenParams, generateParamsList, tomEdwards256, commit, keyToInt, proveSignatureListBatch, verifySignatureListBatch, keyBlinders, proveMembership, verifyMembership,
    proveSameKey, verifySameKey, proveSameKeys, verifySameKeys, keyCommitment, keyCommitments, LinkProof, Commitment, setWireLayout } = zk

async function main() {
    assert.strictEqual(proveSameKey.length, 6)
    assert.strictEqual(verifySameKey.length, 4)
    // two commitments on bare Pedersen parameters
    const pp = generatePedersenParams(tomEdwards256)
    const a = commit(pp, 1234567n), b = commit(pp, 1234567n), other = commit(pp, 1234568n)
    const link = await proveSameKey(pp, 1234567n, a.p, a.r, b.p, b.r)
    assert.ok(link instanceof LinkProof && link.bytes.length === 256 && link.bytes.slice(0, 4).toString('latin1') === 'ZKL1' && link.bytes.readUInt32BE(4) === 256)
    assert.ok(tomEdwards256.isOnGroup(link.A_1) && tomEdwards256.isOnGroup(link.A_2) && link.t_x.k < tomEdwards256.order)
    assert.strictEqual(await verifySameKey(pp, a.p, b.p, link), true)
    assert.strictEqual(await verifySameKey(pp, a, b, link.bytes), true)              // Commitments and raw bytes are taken too
    assert.strictEqual(await verifySameKey(pp, b.p, a.p, link), false)
    assert.strictEqual(await verifySameKey(pp, a.p, other.p, link), false)
    const bad = Buffer.from(link.bytes)
    bad[255] ^= 1                                                                    // t_r2 alone: a verifier that checks one relation accepts it
    assert.strictEqual(await verifySameKey(pp, a.p, b.p, new LinkProof(bad)), false)
    await assert.rejects(proveSameKey(pp, 1234567n, a.p, a.r, other.p, other.r), /do not open/)
    await assert.rejects(proveSameKey(pp, 1234567n, a.p, b.r, b.p, b.r), /do not open/)
    const offCurve = Buffer.concat([Buffer.alloc(35), Buffer.from([5]), Buffer.alloc(35), Buffer.from([7])])
    await assert.rejects(proveSameKey(pp, 1234567n, offCurve, a.r, b.p, b.r), /deserializ/)
    await assert.rejects(verifySameKey(pp, offCurve, b.p, link), /deserializ/)
    assert.throws(() => new LinkProof(link.bytes.slice(0, 255)), /deserializing/)
    assert.ok(!(await proveSameKey(pp, 1234567n, a.p, a.r, b.p, b.r)).eq(link))      // fresh seeds per call
    const same = await proveSameKey(pp, 1234567n, a.p, a.r, a.p, a.r)               // com1 = com2 is an honest statement
    assert.strictEqual(await verifySameKey(pp, a.p, a.p, same), true)
    const links = await proveSameKeys(pp, [1234567n, 1234568n], [a.p, other.p], [a.r, other.r], [b.p, other.p], [b.r, other.r])
    assert.deepStrictEqual(Array.from(await verifySameKeys(pp, [a.p, other.p], [b.p, other.p], links)), [true, true])
    assert.deepStrictEqual(Array.from(await verifySameKeys(pp, [other.p, a.p], [other.p, b.p], links)), [false, false])
    await assert.rejects(proveSameKeys(pp, [1n], [a.p, b.p], [a.r], [b.p], [b.r]), RangeError)
    assert.deepStrictEqual(await proveSameKeys(pp, [], [], [], [], []), [])

    // two attestations by one signer (and one by another), a second registry
    const params = generateParamsList(80)
    const kp = [0, 1].map(() => crypto.generateKeyPairSync('ec', { namedCurve: 'P-256' }))
    const mk = async (who, text) => {
        const msg = Buffer.from(text)
        return { msgHash: crypto.createHash('sha256').update(msg).digest(), publicKey: kp[who].publicKey, x: await keyToInt(kp[who].publicKey),
            signature: crypto.sign('sha256', msg, { key: kp[who].privateKey, dsaEncoding: 'ieee-p1363' }) }
    }
    const att = [await mk(0, 'first'), await mk(0, 'second'), await mk(1, 'third')]
    const keysA = Object.freeze([21n, att[0].x, 5n, att[2].x, 77n]), which = [1, 1, 3]
    const registry = Object.freeze([100n, 101n, att[0].x, 103n, 104n, 105n, att[2].x, 107n, 108n])
    const col = (f) => att.map((s) => s[f]), msgs = col('msgHash')
    const pinned = (n) => Buffer.from(Array.from({ length: n }, (_, i) => (11 * i + 5) & 255))
    const randomBytes = crypto.randomBytes
    for (const layout of ['zka1', 'zka1p']) {
        setWireLayout(layout)
        crypto.randomBytes = pinned
        let proofs
        try {
            proofs = await proveSignatureListBatch(params, msgs, col('signature'), col('publicKey'), which, keysA)
        } finally {
            crypto.randomBytes = randomBytes
        }
        assert.deepStrictEqual(Array.from(await verifySignatureListBatch(params, msgs, keysA, proofs)), [true, true, true])
        const blinders = await keyBlinders(pinned(96), params)
        const kx = await keyCommitments(proofs, params)
        assert.ok(kx.length === 3 && kx.every((p) => tomEdwards256.isOnGroup(p)) && !kx[0].eq(kx[1]))
        assert.ok((await keyCommitment(proofs[1].bytes, params)).eq(kx[1]))
        // attestation 0 and attestation 1 were signed by one key
        const l01 = await proveSameKey(params, att[0].x, kx[0], blinders[0], kx[1], blinders[1])
        assert.strictEqual(await verifySameKey(params, kx[0], kx[1], l01), true)
        assert.strictEqual(await verifySameKey(params, kx[0], kx[2], l01), false)    // presented with the other signer's attestation
        await assert.rejects(proveSameKey(params, att[0].x, kx[0], blinders[0], kx[2], blinders[2]), /do not open/)
        // the signer of attestation 0 is a member of a second registry
        const com = commit(params.ProofGroup, att[0].x)
        assert.ok(com instanceof Commitment)
        const member = await proveMembership(params, com, 2, registry)
        assert.strictEqual(await verifyMembership(params, com.p, registry, member), true)
        const lm = await proveSameKey(params, att[0].x, kx[0], blinders[0], com, com.r)
        assert.strictEqual(await verifySameKey(params, kx[0], com.p, lm), true)
        assert.strictEqual(await verifySameKey(params, kx[2], com.p, lm), false)
    }
    setWireLayout('zka1')
    await assert.rejects(keyCommitment(Buffer.alloc(64), params), /deserializ/)
    console.log('link ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
