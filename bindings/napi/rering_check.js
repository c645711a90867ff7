// node rering_check.js   on an MI355X (ZKATTEST_NODE: the addon): re-ring behind the facade (tests/test_napi_rering.py).
// Proofs made over one key list are moved with reringSignatureLists to a larger list that holds the signers' keys at other indices, and to the first list with
// an unrelated key rotated: the results verify under the new list only, their heads are the old proofs' byte for byte, header n and length follow the new
// ring; keyBlinders gives the blinders for the seeds the proofs were made with (the facade's seed source is pinned while they are made, so they are known
// here); a wrong blinder, a wrong index and an index past the ring are refused; both wire layouts.
const assert = require('assert')
const crypto = require('crypto')
const zk = require('./zkattest.js')
const { generateParamsList, keyToInt, proveSignatureListBatch, verifySignatureListBatch, reringSignatureLists, keyBlinders, setWireLayout, SignatureProofList } = zk

const gkSize = (n, tc) => n * (8 * tc + 96) + 32

async function main() {
    const params = generateParamsList(80)
    const signers = []
    for (let r = 0; r < 2; r++) {
        const keyPair = crypto.generateKeyPairSync('ec', { namedCurve: 'P-256' }), msg = Buffer.from('rering ' + r)
        signers.push({ msgHash: crypto.createHash('sha256').update(msg).digest(), publicKey: keyPair.publicKey, x: await keyToInt(keyPair.publicKey),
            signature: crypto.sign('sha256', msg, { key: keyPair.privateKey, dsaEncoding: 'ieee-p1363' }) })
    }
    const keysA = Object.freeze([21n, signers[0].x, 5n, signers[1].x, 77n])                                        // 5 keys: n = 3; signers at 1 and 3
    const keysB = Object.freeze([100n, 101n, 102n, signers[1].x, 104n, 105n, 106n, signers[0].x, 108n])          // 9 keys: n = 4; signers at 7 and 3
    const keysA2 = Object.freeze([21n, signers[0].x, 5n, signers[1].x, 78n])                                       // A with an unrelated key rotated
    const col = (f) => signers.map((s) => s[f]), msgs = col('msgHash')
    assert.strictEqual(reringSignatureLists.length, 6)
    const pinned = (n) => Buffer.from(Array.from({ length: n }, (_, i) => (7 * i + 3) & 255))
    const randomBytes = crypto.randomBytes
    for (const layout of ['zka1', 'zka1p']) {
        const tc = layout === 'zka1' ? 36 : 33
        setWireLayout(layout)
        crypto.randomBytes = pinned
        let proofs
        try {
            proofs = await proveSignatureListBatch(params, msgs, col('signature'), col('publicKey'), [1, 3], keysA)
        } finally {
            crypto.randomBytes = randomBytes
        }
        const blinders = await keyBlinders(pinned(64))
        assert.ok(blinders.length === 2 && blinders.every((b) => b.length === 32) && !blinders[0].equals(blinders[1]))
        assert.deepStrictEqual((await keyBlinders([pinned(64).slice(0, 32), pinned(64).slice(32)], params)).map((b) => b.toString('hex')), blinders.map((b) => b.toString('hex')))
        // A -> B: n 3 -> 4
        const moved = await reringSignatureLists(params, msgs, proofs, [7, 3], blinders, keysB)
        moved.forEach((p, i) => {
            const a = proofs[i].bytes, b = p.bytes, ha = a.length - gkSize(3, tc)
            assert.ok(p instanceof SignatureProofList && b.length === ha + gkSize(4, tc) && b.readUInt32BE(4) === b.length && b.readUInt32BE(12) === 4)
            assert.ok(b.slice(0, 4).equals(a.slice(0, 4)) && b.slice(8, 12).equals(a.slice(8, 12)) && b.slice(16, ha).equals(a.slice(16, ha)), 'the head of proof ' + i + ' changed')
        })
        assert.deepStrictEqual(Array.from(await verifySignatureListBatch(params, msgs, keysB, moved)), [true, true])
        assert.deepStrictEqual(Array.from(await verifySignatureListBatch(params, msgs, keysA, moved)), [false, false])
        assert.deepStrictEqual(Array.from(await verifySignatureListBatch(params, msgs, keysB, proofs)), [false, false])
        // ... and back to the first list after one of its other keys was rotated: the old proofs are gone, the re-ringed ones hold
        assert.deepStrictEqual(Array.from(await verifySignatureListBatch(params, msgs, keysA2, proofs)), [false, false])
        const back = await reringSignatureLists(params, msgs, moved.map((p) => p.bytes), [1, 3], blinders, keysA2)
        assert.deepStrictEqual(Array.from(await verifySignatureListBatch(params, msgs, keysA2, back)), [true, true])
        assert.ok(back.every((p, i) => p.bytes.length === proofs[i].bytes.length && !p.bytes.equals(proofs[i].bytes)))
        // fresh seeds per call: the same move twice gives two different sections
        const again = await reringSignatureLists(params, msgs, proofs, [7, 3], blinders, keysB)
        assert.ok(!again[0].bytes.equals(moved[0].bytes))
        // refusals
        await assert.rejects(reringSignatureLists(params, msgs, proofs, [7, 3], [blinders[1], blinders[0]], keysB), /do not open/)
        await assert.rejects(reringSignatureLists(params, msgs, proofs, [3, 7], blinders, keysB), /do not open/)
        await assert.rejects(reringSignatureLists(params, msgs, proofs, [7, 16], blinders, keysB), TypeError)
        const broken = Buffer.from(proofs[0].bytes)
        broken.writeUInt32BE(64, 12)
        await assert.rejects(reringSignatureLists(params, msgs, [broken, proofs[1]], [7, 3], blinders, keysB), /deserializ/)
        await assert.rejects(reringSignatureLists(params, msgs, proofs, [7], blinders, keysB), RangeError)
        await assert.rejects(reringSignatureLists(params, msgs, proofs, [7, 3], [blinders[0], blinders[1].slice(1)], keysB), TypeError)
    }
    setWireLayout('zka1')
    assert.deepStrictEqual(await reringSignatureLists(params, [], [], [], [], keysB), [])
    console.log('rering ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
