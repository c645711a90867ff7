// node prove_rings_check.js   on an MI355X (ZKATTEST_NODE: the addon): mixed-ring proving behind the facade (tests/test_napi_prove_rings.py).
// proveSignatureLists over five rings -- more than the four the engine keeps resident, so the call is split once -- returns, statement by statement, the bytes of
// proveSignatureListBatch over that statement's ring, and verifySignatureLists accepts them under their own rings only.  The facade draws one fresh seed per
// proof from crypto.randomBytes; for the comparison that source is pinned to a constant, so that equal statements get equal seeds in both calls.
const assert = require('assert')
const crypto = require('crypto')
const zk = require('./zkattest.js')
const { generateParamsList, keyToInt, proveSignatureLists, proveSignatureListBatch, verifySignatureLists } = zk

async function main() {
    const params = generateParamsList(80)
    const st = []   // one signer per ring: { msgHash, signature, publicKey, which, keys }
    for (let r = 0; r < 5; r++) {
        const keyPair = crypto.generateKeyPairSync('ec', { namedCurve: 'P-256' }), msg = Buffer.from('prove rings ' + r)
        const msgHash = crypto.createHash('sha256').update(msg).digest()
        const signature = crypto.sign('sha256', msg, { key: keyPair.privateKey, dsaEncoding: 'ieee-p1363' })
        const keys = [BigInt(21 + r), BigInt(5), await keyToInt(keyPair.publicKey), BigInt(6 + 10 * r)]
        for (let k = 0; k < 3 * r; k++) keys.push(BigInt(100 + k))   // 4, 7, 10, 13, 16 keys: n = 2, 3, 4, 4, 4
        Object.freeze(keys)
        st.push({ msgHash, signature, publicKey: keyPair.publicKey, which: 2, keys })
    }
    const order = [0, 1, 2, 0, 3, 4, 1, 2]
    const col = (f) => order.map((r) => st[r][f])
    const randomBytes = crypto.randomBytes
    crypto.randomBytes = (n) => Buffer.alloc(n, 0x5a)
    let got, want = []
    try {
        got = await proveSignatureLists(params, col('msgHash'), col('signature'), col('publicKey'), col('which'), col('keys'))
        for (const r of order) {
            const s = st[r]
            want.push((await proveSignatureListBatch(params, [s.msgHash], [s.signature], [s.publicKey], [s.which], s.keys))[0])
        }
    } finally {
        crypto.randomBytes = randomBytes
    }
    assert.strictEqual(got.length, order.length)
    got.forEach((p, i) => assert.ok(p.bytes.equals(want[i].bytes), 'proof ' + i + ' differs from the per-ring call'))
    assert.ok(got[0].bytes.equals(got[3].bytes) && !got[0].bytes.equals(got[1].bytes))
    const ok = await verifySignatureLists(params, col('msgHash'), col('keys'), got)
    assert.deepStrictEqual(Array.from(ok), order.map(() => true))
    const other = await verifySignatureLists(params, col('msgHash'), order.map((r) => st[(r + 1) % 5].keys), got)
    assert.deepStrictEqual(Array.from(other), order.map(() => false))
    // one ring only: the same call is the per-ring batch
    const fresh = await proveSignatureLists(params, [st[1].msgHash, st[1].msgHash], [st[1].signature, st[1].signature], [st[1].publicKey, st[1].publicKey], [2, 2], [st[1].keys, st[1].keys])
    assert.deepStrictEqual(Array.from(await verifySignatureLists(params, [st[1].msgHash, st[1].msgHash], [st[1].keys, st[1].keys], fresh)), [true, true])
    assert.ok(!fresh[0].bytes.equals(fresh[1].bytes), 'two proofs of one call share their seed')
    await assert.rejects(proveSignatureLists(params, [st[0].msgHash], [st[0].signature], [st[0].publicKey], [2], []), RangeError)
    console.log('prove rings ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
