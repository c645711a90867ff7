// node verify_reps_check.js   on an MI355X (ZKATTEST_NODE: the addon): setVerifyReps('all') -- every repetition of a proof is checked, where the
// default 'sample' checks the 20 that generateIndices draws, as the reference's verifier does (tests/test_gpu_verify_all.py)
const assert = require('assert')
const crypto = require('crypto')
const zk = require('./zkattest.js')
const { generateParamsList, keyToInt, proveSignatureList, verifySignatureList, SignatureProofList } = zk

// ZKA1 (include/zkattest.h): 304 fixed bytes, then the repetitions -- 336 bytes, and a PointAdd proof of 3392 where the header's challenge bit is 0;
// the second response scalar of repetition i (beta1 or z2) is at byte 240 of it
function breakRepetition(bytes, i) {
    const b = Buffer.from(bytes), bits = BigInt('0x' + b.slice(16, 32).toString('hex'))
    let off = 304
    for (let k = 0; k < i; k++) off += 336 + ((bits >> BigInt(k)) & 1n ? 0 : 3392)
    b[off + 240 + 31] ^= 1
    return new SignatureProofList(b)
}

async function main() {
    const keyPair = crypto.generateKeyPairSync('ec', { namedCurve: 'P-256' }), msg = Buffer.from('reps')
    const msgHash = crypto.createHash('sha256').update(msg).digest()
    const signature = crypto.sign('sha256', msg, { key: keyPair.privateKey, dsaEncoding: 'ieee-p1363' })
    const keys = [await keyToInt(keyPair.publicKey), BigInt(4), BigInt(5), BigInt(6), BigInt(7)]
    const params = generateParamsList(80)
    const proof = await proveSignatureList(params, msgHash, signature, keyPair.publicKey, 0, keys)
    const broken = breakRepetition(proof.bytes, 61)
    assert.strictEqual(zk.getVerifyReps(), 'sample')
    assert.strictEqual(await verifySignatureList(params, msgHash, keys, proof), true)
    // one broken repetition out of 80 is sampled with probability 1/4 per call (fresh verifier randomness): 60 calls all reject with probability 4^-60 ...
    let accepted = 0
    for (let k = 0; k < 60 && !accepted; k++) accepted += (await verifySignatureList(params, msgHash, keys, broken)) ? 1 : 0
    assert.strictEqual(accepted, 1)
    console.log('sample: a broken repetition passes')
    zk.setVerifyReps('all')   // the engine is cached already: the switch reaches it
    assert.strictEqual(zk.getVerifyReps(), 'all')
    assert.strictEqual(await verifySignatureList(params, msgHash, keys, proof), true)
    for (let k = 0; k < 8; k++) assert.strictEqual(await verifySignatureList(params, msgHash, keys, broken), false)   // ... and never passes here
    console.log('all: rejected')
    zk.setVerifyReps('sample')
    assert.strictEqual(await verifySignatureList(params, msgHash, keys, proof), true)
    assert.throws(() => zk.setVerifyReps('most'), TypeError)
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
