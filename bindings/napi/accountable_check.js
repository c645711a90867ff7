// node accountable_check.js   on an MI355X (ZKATTEST_NODE: the addon): accountable attestations behind the facade (tests/test_napi_accountable.py).
// proveAccountables over three attestations -> AccountableProofs that verifyAccountables accepts; the parts are what the existing verifiers accept; a flipped tag
// byte, swapped tags, another message hash and another auditor's key give false; split and join are inverse; the split tags open to the signers; what does not
// deserialise throws -- in both wire layouts.
const assert = require('assert')
const crypto = require('crypto')
const zk = require('./zkattest.js')
const { generateParamsList, keyToInt, proveAccountable, proveAccountables, verifyAccountable, verifyAccountables, splitAccountable, joinAccountable, AccountableProof,
    SignatureProofList, EscrowTag, verifySignatureListBatch, keyCommitments, verifyEscrowTags, openEscrowTags, escrowAuditorKey, setWireLayout } = zk

async function main() {
    assert.strictEqual(proveAccountable.length, 7)
    assert.strictEqual(proveAccountables.length, 7)
    assert.strictEqual(verifyAccountable.length, 5)
    assert.strictEqual(verifyAccountables.length, 5)
    assert.strictEqual(splitAccountable.length, 2)
    assert.strictEqual(joinAccountable.length, 3)
    const params = generateParamsList(80)
    const a = 0x1234567890abcdef1234567890abcdefn
    const A = await escrowAuditorKey(params, a), A2 = await escrowAuditorKey(params, a + 1n)
    const kp = [0, 1].map(() => crypto.generateKeyPairSync('ec', { namedCurve: 'P-256' }))
    const mk = async (who, text) => {
        const msg = Buffer.from(text)
        return { msgHash: crypto.createHash('sha256').update(msg).digest(), publicKey: kp[who].publicKey, x: await keyToInt(kp[who].publicKey),
            signature: crypto.sign('sha256', msg, { key: kp[who].privateKey, dsaEncoding: 'ieee-p1363' }) }
    }
    const att = [await mk(0, 'first'), await mk(0, 'second'), await mk(1, 'third')]
    const ring = Object.freeze([21n, att[0].x, 5n, att[2].x, 77n]), which = [1, 1, 3]
    const col = (f) => att.map((s) => s[f]), msgs = col('msgHash')
    for (const layout of ['zka1', 'zka1p']) {
        setWireLayout(layout)
        const proofs = await proveAccountables(params, A, msgs, col('signature'), col('publicKey'), which, ring)
        assert.strictEqual(proofs.length, 3)
        for (const p of proofs) {
            assert.ok(p instanceof AccountableProof && p.bytes.slice(0, 4).toString('latin1') === 'ZKC1' && p.bytes.readUInt32BE(4) === p.bytes.length)
            assert.ok(p.attestation instanceof SignatureProofList && p.tag instanceof EscrowTag && p.tag.bytes.length === 472)
            assert.strictEqual(p.bytes.slice(16, 20).toString('latin1'), layout === 'zka1' ? 'ZKA1' : 'ZK1P')
            assert.ok(new AccountableProof(Buffer.from(p.bytes)).eq(p))
        }
        assert.deepStrictEqual(Array.from(await verifyAccountables(params, A, msgs, ring, proofs)), [true, true, true])
        assert.strictEqual(await verifyAccountable(params, A, msgs[1], ring, proofs[1].bytes), true)   // raw bytes are taken too
        // the parts are what the existing calls accept: the recipe's verifier agrees
        const parts = await splitAccountable(params, proofs)
        assert.deepStrictEqual(Array.from(await verifySignatureListBatch(params, msgs, ring, parts.map((x) => x.attestation))), [true, true, true])
        const coms = await keyCommitments(parts.map((x) => x.attestation), params)
        assert.deepStrictEqual(Array.from(await verifyEscrowTags(params, A, coms, parts.map((x) => x.tag))), [true, true, true])
        parts.forEach((x, i) => assert.ok(x.attestation.bytes.equals(proofs[i].attestation.bytes) && x.tag.eq(proofs[i].tag)))
        assert.deepStrictEqual(await openEscrowTags(params, a, ring, parts.map((x) => x.tag)), [1, 1, 3])
        // join is split's inverse; tags swapped between two bundles: the point of the format
        const joined = await joinAccountable(params, parts.map((x) => x.attestation), parts.map((x) => x.tag))
        joined.forEach((j, i) => assert.ok(j.eq(proofs[i])))
        const swapped = await joinAccountable(params, [parts[0].attestation, parts[2].attestation], [parts[2].tag, parts[0].tag])
        assert.deepStrictEqual(Array.from(await verifyAccountables(params, A, [msgs[0], msgs[2]], ring, swapped)), [false, false])
        // a flipped byte of t_rho; another message hash; another auditor's key; and the engine is back on A
        const bad = Buffer.from(proofs[0].bytes)
        bad[bad.length - 1] ^= 1
        assert.strictEqual(await verifyAccountable(params, A, msgs[0], ring, bad), false)
        assert.strictEqual(await verifyAccountable(params, A, msgs[1], ring, proofs[0]), false)
        assert.strictEqual(await verifyAccountable(params, A2, msgs[0], ring, proofs[0]), false)
        assert.strictEqual(await verifyAccountable(params, A, msgs[0], ring, proofs[0]), true)
        const one = await proveAccountable(params, A, msgs[2], att[2].signature, att[2].publicKey, 3, ring)
        assert.ok(!one.eq(proofs[2]) && await verifyAccountable(params, A, msgs[2], ring, one))        // fresh seeds per call
        // what does not deserialise throws
        const b = proofs[0].bytes
        assert.throws(() => new AccountableProof(b.slice(0, b.length - 4)), /deserializing/)
        const inner = Buffer.from(b)
        inner.writeUInt32BE(inner.readUInt32BE(20) + 4, 20)
        assert.throws(() => new AccountableProof(inner), /deserializing/)
        const res = Buffer.from(b)
        res[15] = 1
        assert.throws(() => new AccountableProof(res), /deserializing/)
        await assert.rejects(verifyAccountables(params, A, msgs.slice(0, 2), ring, proofs), RangeError)
        await assert.rejects(joinAccountable(params, [parts[0].attestation], []), RangeError)
    }
    setWireLayout('zka1')
    assert.deepStrictEqual(await proveAccountables(params, A, [], [], [], [], ring), [])
    console.log('accountable ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
