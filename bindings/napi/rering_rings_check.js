// node rering_rings_check.js   on an MI355X (ZKATTEST_NODE: the addon): re-ring with one key list per proof behind the facade (tests/test_napi_rering_rings.py).
// Three proofs made over one key list are moved in ONE reringSignatureLists call to three different lists -- a larger one, one of the same size with the
// signers' keys at other indices, and the larger one again: each result verifies under its own list only (verifySignatureLists with the same lists), its head
// is the old proof's byte for byte and its header follows its own ring; the same move through the one-list form proof by proof verifies the same way; a wrong
// blinder, an index past ITS ring (legal in the larger one) and a list count that is not the proofs' are refused; both wire layouts.
const assert = require('assert')
const crypto = require('crypto')
const zk = require('./zkattest.js')
const { generateParamsList, keyToInt, proveSignatureListBatch, verifySignatureLists, verifySignatureListBatch, reringSignatureLists, keyBlinders, setWireLayout, SignatureProofList } = zk

const gkSize = (n, tc) => n * (8 * tc + 96) + 32

async function main() {
    const params = generateParamsList(80)
    const signers = []
    for (let r = 0; r < 3; r++) {
        const keyPair = crypto.generateKeyPairSync('ec', { namedCurve: 'P-256' }), msg = Buffer.from('rering rings ' + r)
        signers.push({ msgHash: crypto.createHash('sha256').update(msg).digest(), publicKey: keyPair.publicKey, x: await keyToInt(keyPair.publicKey),
            signature: crypto.sign('sha256', msg, { key: keyPair.privateKey, dsaEncoding: 'ieee-p1363' }) })
    }
    const x = signers.map((s) => s.x)
    const keysA = Object.freeze([21n, x[0], 5n, x[1], x[2]])                                       // 5 keys: n = 3; signers at 1, 3, 4
    const keysB = Object.freeze([100n, 101n, x[2], x[1], 104n, 105n, 106n, x[0], 108n])            // 9 keys: n = 4; signers at 7, 3, 2
    const keysC = Object.freeze([x[1], 31n, x[2], 33n, x[0]])                                      // 5 keys: n = 3; signers at 4, 0, 2
    const col = (f) => signers.map((s) => s[f]), msgs = col('msgHash')
    assert.strictEqual(reringSignatureLists.length, 6)
    const pinned = (n) => Buffer.from(Array.from({ length: n }, (_, i) => (11 * i + 5) & 255))
    const randomBytes = crypto.randomBytes
    for (const layout of ['zka1', 'zka1p']) {
        const tc = layout === 'zka1' ? 36 : 33
        setWireLayout(layout)
        crypto.randomBytes = pinned
        let proofs
        try {
            proofs = await proveSignatureListBatch(params, msgs, col('signature'), col('publicKey'), [1, 3, 4], keysA)
        } finally {
            crypto.randomBytes = randomBytes
        }
        const blinders = await keyBlinders(pinned(96))
        const lists = [keysB, keysC, keysB], idx = [7, 0, 2], ns = [4, 3, 4]
        const moved = await reringSignatureLists(params, msgs, proofs, idx, blinders, lists)
        moved.forEach((p, i) => {
            const a = proofs[i].bytes, b = p.bytes, ha = a.length - gkSize(3, tc)
            assert.ok(p instanceof SignatureProofList && b.length === ha + gkSize(ns[i], tc) && b.readUInt32BE(4) === b.length && b.readUInt32BE(12) === ns[i])
            assert.ok(b.slice(0, 4).equals(a.slice(0, 4)) && b.slice(8, 12).equals(a.slice(8, 12)) && b.slice(16, ha).equals(a.slice(16, ha)), 'the head of proof ' + i + ' changed')
        })
        assert.deepStrictEqual(Array.from(await verifySignatureLists(params, msgs, lists, moved)), [true, true, true])
        assert.deepStrictEqual(Array.from(await verifySignatureLists(params, msgs, [keysC, keysB, keysC], moved)), [false, false, false])
        assert.deepStrictEqual(Array.from(await verifySignatureLists(params, msgs, lists, proofs)), [false, false, false])   // the originals are proofs for keysA
        assert.deepStrictEqual(Array.from(await verifySignatureListBatch(params, msgs, keysA, proofs)), [true, true, true])
        // the one-list form, proof by proof, lands where the mixed call did: same lengths, same verdicts (fresh seeds: other sections)
        for (let i = 0; i < 3; i++) {
            const one = await reringSignatureLists(params, [msgs[i]], [proofs[i]], [idx[i]], [blinders[i]], lists[i])
            assert.ok(one[0].bytes.length === moved[i].bytes.length && !one[0].bytes.equals(moved[i].bytes))
            assert.deepStrictEqual(Array.from(await verifySignatureListBatch(params, [msgs[i]], lists[i], one)), [true])
        }
        // refusals: a wrong blinder; index 7 is legal in keysB and past keysC's padded ring; counts
        await assert.rejects(reringSignatureLists(params, msgs, proofs, idx, [blinders[1], blinders[0], blinders[2]], lists), /do not open/)
        await assert.rejects(reringSignatureLists(params, msgs, proofs, [7, 8, 2], blinders, lists), TypeError)
        await assert.rejects(reringSignatureLists(params, msgs, proofs, [7, 7, 2], blinders, [keysB, keysB, keysB]), /do not open/)
        await assert.rejects(reringSignatureLists(params, msgs, proofs, idx, blinders, [keysB, keysC]), RangeError)
        const broken = Buffer.from(proofs[0].bytes)
        broken.writeUInt32BE(64, 12)
        await assert.rejects(reringSignatureLists(params, msgs, [broken, proofs[1], proofs[2]], idx, blinders, lists), /deserializ/)
    }
    setWireLayout('zka1')
    console.log('rering rings ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
