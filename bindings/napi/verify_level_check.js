// node verify_level_check.js   on an MI355X (ZKATTEST_NODE: the addon): setVerifyLevel('proof') -- verifySignatureList at the proof's own
// repetition count, as the reference's verifier does -- against the default 'context' (tests/test_gpu_verify_levels.py)
const assert = require('assert')
const crypto = require('crypto')
const zk = require('./zkattest.js')
const { generateParamsList, keyToInt, proveSignatureList, verifySignatureList, SystemParametersList } = zk

async function main() {
    const keyPair = crypto.generateKeyPairSync('ec', { namedCurve: 'P-256' }), msg = Buffer.from('levels')
    const msgHash = crypto.createHash('sha256').update(msg).digest()
    const signature = crypto.sign('sha256', msg, { key: keyPair.privateKey, dsaEncoding: 'ieee-p1363' })
    const keys = [await keyToInt(keyPair.publicKey), BigInt(4), BigInt(5), BigInt(6), BigInt(7)]
    const p128 = generateParamsList(128)
    const p80 = new SystemParametersList(p128.NistGroup, p128.ProofGroup, 80)   // the same groups, SecLevel 80
    const proof = await proveSignatureList(p128, msgHash, signature, keyPair.publicKey, 0, keys)
    assert.strictEqual(zk.getVerifyLevel(), 'context')
    await assert.rejects(verifySignatureList(p80, msgHash, keys, proof), /deserializ/)
    console.log('context: false')
    zk.setVerifyLevel('proof')   // the engine of p80 is cached already: the switch reaches it
    assert.strictEqual(await verifySignatureList(p80, msgHash, keys, proof), true)
    assert.strictEqual(await verifySignatureList(p128, msgHash, keys, proof), true)
    assert.strictEqual(await verifySignatureList(p80, crypto.createHash('sha256').update('x').digest(), keys, proof), false)
    console.log('proof: true')
    zk.setVerifyLevel('context')
    await assert.rejects(verifySignatureList(p80, msgHash, keys, proof), /deserializ/)
    assert.throws(() => zk.setVerifyLevel('ring'), TypeError)
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
