// node ring_update_check.js   on an MI355X (ZKATTEST_NODE: the addon): Engine.updateRing and the facade's ringDelta option (tests/test_napi_ring_update.py).
// With ringDelta 16 two verifySignatureList calls whose key lists differ in 2 entries leave ONE resident ring with its generation up by one; with ringDelta 0
// they leave two rings, as before.  Verdicts are those of the key list each call names -- also when the caller keeps the list in one Buffer and overwrites it in place.
const assert = require('assert')
const crypto = require('crypto')
const zk = require('./zkattest.js')
const { generateParamsList, keyToInt, proveSignatureList, verifySignatureList } = zk

async function main() {
    const params = generateParamsList(80)
    const keyPair = crypto.generateKeyPairSync('ec', { namedCurve: 'P-256' }), msg = Buffer.from('ring update')
    const msgHash = crypto.createHash('sha256').update(msg).digest()
    const signature = crypto.sign('sha256', msg, { key: keyPair.privateKey, dsaEncoding: 'ieee-p1363' })
    const pkInt = await keyToInt(keyPair.publicKey)
    const base = []
    for (let i = 0; i < 40; i++) base.push(BigInt(1000 + i))
    base[3] = pkInt
    const listA = Object.freeze(base.slice())
    const listB = base.slice()
    listB[7] = BigInt(777), listB[30] = BigInt(778)   // two entries differ; the signer's key stays
    Object.freeze(listB)
    const listC = base.slice()
    listC[9] = BigInt(900), listC[3] = BigInt(901)    // the signer's key is rotated out
    Object.freeze(listC)

    // ---- ringDelta off: two lists, two resident rings (today's behaviour)
    const proofA = await proveSignatureList(params, msgHash, signature, keyPair.publicKey, 3, listA)
    assert.strictEqual(await verifySignatureList(params, msgHash, listA, proofA), true)
    assert.strictEqual(await verifySignatureList(params, msgHash, listB, proofA), false)   // (membership is over the whole ring)
    let gens = zk._ringGenerations(params)
    assert.strictEqual(Object.keys(gens).length, 2, 'ringDelta 0 must build a second ring')
    zk.shutdown()

    // ---- ringDelta 16: the second list updates the first ring in place
    zk.setOption('ringDelta', 16)
    const params2 = generateParamsList(80)
    const proofA1 = await proveSignatureList(params2, msgHash, signature, keyPair.publicKey, 3, listA)   // list A becomes resident on this engine
    assert.strictEqual(await verifySignatureList(params2, msgHash, listA, proofA1), true)
    const g0 = zk._ringGenerations(params2)
    assert.strictEqual(Object.keys(g0).length, 1)
    const proofB = await proveSignatureList(params2, msgHash, signature, keyPair.publicKey, 3, listB)
    const g1 = zk._ringGenerations(params2)
    assert.strictEqual(Object.keys(g1).length, 1, 'ringDelta 16 must update the resident ring, not add one')
    assert.notStrictEqual(Object.keys(g1)[0], Object.keys(g0)[0], 'the slot was not re-tagged')
    assert.strictEqual(Object.values(g1)[0], Object.values(g0)[0] + 1, 'one update = one generation')
    assert.strictEqual(await verifySignatureList(params2, msgHash, listB, proofB), true)
    assert.deepStrictEqual(zk._ringGenerations(params2), g1)
    // back to list A (again 2 entries away): updated again, and the proof over B no longer verifies; a proof over A made now does
    assert.strictEqual(await verifySignatureList(params2, msgHash, listA, proofB), false)
    const proofA2 = await proveSignatureList(params2, msgHash, signature, keyPair.publicKey, 3, listA)
    assert.strictEqual(await verifySignatureList(params2, msgHash, listA, proofA2), true)
    const g2 = zk._ringGenerations(params2)
    assert.strictEqual(Object.keys(g2).length, 1)
    assert.strictEqual(Object.values(g2)[0], Object.values(g0)[0] + 2)
    assert.strictEqual(await verifySignatureList(params2, msgHash, listC, proofA2), false)   // the signer's key left the ring
    assert.strictEqual(Object.keys(zk._ringGenerations(params2)).length, 1)

    // ---- a registry held as ONE Buffer and changed in place: the facade's record of what is resident must not alias the caller's memory
    const be32 = (v) => Buffer.from(v.toString(16).padStart(64, '0'), 'hex')
    const reg = Buffer.concat(listA.map(be32))
    await proveSignatureList(params2, msgHash, signature, keyPair.publicKey, 3, reg)   // (list A's bytes: the ring of proofA2, resident already)
    assert.strictEqual(await verifySignatureList(params2, msgHash, reg, proofA2), true)
    const g3 = zk._ringGenerations(params2)
    assert.strictEqual(Object.keys(g3).length, 1)
    be32(BigInt(4242)).copy(reg, 32 * 11)                       // key 11 is rotated: the same Buffer object, other bytes
    assert.strictEqual(await verifySignatureList(params2, msgHash, reg, proofA2), false, 'a proof over the old ring verified after the key list changed in place')
    const g4 = zk._ringGenerations(params2)
    assert.strictEqual(Object.keys(g4).length, 1)
    assert.strictEqual(Object.values(g4)[0], Object.values(g3)[0] + 1, 'the in-place change must update the resident ring once')
    const proofR2 = await proveSignatureList(params2, msgHash, signature, keyPair.publicKey, 3, reg)
    assert.strictEqual(await verifySignatureList(params2, msgHash, reg, proofR2), true)
    be32(BigInt(1011)).copy(reg, 32 * 11)                       // ... and back: list A again
    assert.strictEqual(await verifySignatureList(params2, msgHash, reg, proofR2), false)
    assert.strictEqual(await verifySignatureList(params2, msgHash, reg, proofA2), true)
    assert.strictEqual(Object.values(zk._ringGenerations(params2))[0], Object.values(g3)[0] + 2)

    // ---- Engine.updateRing directly: equal to a ring built from the new list
    const eng = new zk.Engine(0)
    const ep = eng.synthParams(7)
    eng.setParams(ep)
    const w = eng.synthWorkload(7, 600, 4)
    const ring = Buffer.from(w.ring)
    const old = Buffer.from(ring)
    crypto.createHash('sha256').update('old key').digest().copy(old, 32 * 2)   // the ring the engine starts with: key 2 is another one
    const id = eng.addRing(old)
    const before = eng.ringInfo(id)
    eng.useRing(id)
    eng.updateRing(id, [2], ring.subarray(64, 96))
    const after = eng.ringInfo(id)
    assert.strictEqual(after.generation, before.generation + 1)
    assert.strictEqual(after.nKeys, 600)
    const made = eng.proveBatch(w.msg, w.sig, w.pk, w.which, w.seeds)
    const fresh = new zk.Engine(0)
    fresh.setParams(ep)
    fresh.setRing(ring)
    const want = fresh.proveBatch(w.msg, w.sig, w.pk, w.which, w.seeds)
    assert.strictEqual(made.length, 4)
    for (let i = 0; i < 4; i++) assert.ok(made[i].equals(want[i]), 'proof ' + i + ' differs from the fresh ring')
    assert.deepStrictEqual(eng.verifyBatch(w.msg, made), Array(4).fill(true))
    assert.throws(() => eng.updateRing(id, [600], ring.subarray(0, 32)))           // an index out of range
    assert.throws(() => eng.updateRing(id + 5, [0], ring.subarray(0, 32)))         // an unknown id
    assert.strictEqual(eng.ringInfo(id).generation, after.generation)
    eng.close(), fresh.close()
    console.log('ring update ok')
    zk.shutdown()
}
main().catch((e) => { console.error(e); process.exit(1) })
