// node recover_check.js   on an MI355X (ZKATTEST_NODE: the addon): key recovery behind the facade (tests/test_napi_recover.py).
// recoverSignatureLists on an 8-key ring: every signer's key comes back as the raw point OpenSSL exports, at the index it stands at; a wrong message gives
// NOT_IN_RING and no key; and the recovered keys, handed to proveSignatureLists as they are, yield proofs that verifySignatureLists accepts.
const assert = require('assert')
const crypto = require('crypto')
const zk = require('./zkattest.js')
const { generateParamsList, keyToInt, recoverSignatureLists, recoverKey, proveSignatureLists, verifySignatureLists, RECOVER, WHICH_NONE } = zk

async function main() {
    const params = generateParamsList(20)
    const pairs = [], keys = []
    for (let k = 0; k < 8; k++) {
        pairs.push(crypto.generateKeyPairSync('ec', { namedCurve: 'P-256' }))
        keys.push(await keyToInt(pairs[k].publicKey))
    }
    Object.freeze(keys)
    const st = pairs.map((kp, k) => {
        const msg = Buffer.from('recover ' + k)
        return { msgHash: crypto.createHash('sha256').update(msg).digest(), sigBytes: crypto.sign('sha256', msg, { key: kp.privateKey, dsaEncoding: 'ieee-p1363' }), keys }
    })
    const mutant = Object.assign({}, st[3], { msgHash: crypto.createHash('sha256').update('another').digest() })
    const got = await recoverSignatureLists(params, st.concat([mutant]))
    assert.deepStrictEqual(got.map((r) => r.flags), [0, 0, 0, 0, 0, 0, 0, 0, RECOVER.NOT_IN_RING])
    assert.deepStrictEqual(got.map((r) => r.which), [0, 1, 2, 3, 4, 5, 6, 7, WHICH_NONE])
    assert.strictEqual(got[8].publicKey, null)
    for (let k = 0; k < 8; k++) assert.deepStrictEqual(got[k].publicKey, pairs[k].publicKey.export({ type: 'spki', format: 'der' }).slice(-65))
    const one = await recoverKey(st[5].msgHash, st[5].sigBytes, keys)
    assert.deepStrictEqual(one, got[5])
    assert.deepStrictEqual(await recoverSignatureLists(params, []), [])
    // the raw point is an ECDSA P-256 key: behind the fixed SubjectPublicKeyInfo prefix it makes a KeyObject that verifies the signature (and, where this
    // node has WebCrypto, importKey('raw', ...) makes a CryptoKey of it)
    const spki = Buffer.concat([Buffer.from('3059301306072a8648ce3d020106082a8648ce3d030107034200', 'hex'), got[2].publicKey])
    const keyObject = crypto.createPublicKey({ key: spki, format: 'der', type: 'spki' })
    assert.ok(crypto.verify('sha256', Buffer.from('recover 2'), { key: keyObject, dsaEncoding: 'ieee-p1363' }, st[2].sigBytes))
    if (crypto.webcrypto && crypto.webcrypto.subtle) {
        const imported = await crypto.webcrypto.subtle.importKey('raw', got[2].publicKey, { name: 'ECDSA', namedCurve: 'P-256' }, true, ['verify'])
        assert.ok(await crypto.webcrypto.subtle.verify({ name: 'ECDSA', hash: 'SHA-256' }, imported, st[2].sigBytes, Buffer.from('recover 2')))
    }
    // recover -> prove -> verify, the recovered raw points as public keys
    const col = (f) => st.map((s) => s[f])
    const proofs = await proveSignatureLists(params, col('msgHash'), col('sigBytes'), got.slice(0, 8).map((r) => r.publicKey), got.slice(0, 8).map((r) => r.which), col('keys'))
    const ok = await verifySignatureLists(params, col('msgHash'), col('keys'), proofs)
    assert.deepStrictEqual(Array.from(ok), new Array(8).fill(true))
    console.log('recover ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
