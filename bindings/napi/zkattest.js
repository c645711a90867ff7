// JavaScript façade over the N-API addon with the reference's public surface (src/index.ts:17-19):
//
//   generateParamsList(secLevel = 80) -> SystemParametersList                      src/zkpAttestList.ts:88-92
//   keyToInt(publicKey) -> Promise<bigint>                                         src/zkpAttestList.ts:94-102
//   proveSignatureList(params, msgHash, sigBytes, publicKey, which, keys)          src/zkpAttestList.ts:104-145
//        -> Promise<SignatureProofList>
//   verifySignatureList(params, msgHash, keys, proof) -> Promise<boolean>          src/zkpAttestList.ts:147-184
//   writeJson(Class, object) -> string, readJson(Class, text) -> object            src/serde.ts:21-36
//   SignatureProofList, SystemParametersList, PedersenParams (each with eq())      src/zkpAttestList.ts:27-78
//   p256, tomEdwards256, ALL_GROUPS                                                src/curves/instances.ts:22-56
//
// plus the batch calls the engine is built for (proveSignatureListBatch / verifySignatureListBatch) and the low-level
// Engine.  Same argument order, same Promise-returning functions, same error texts as the reference.  The GPU contexts are
// created on first use and CACHED by the identity of (params, ring): building the fixed-base tables costs 0.2-1 s and the
// per-ring table a few ms, so they are built once per SystemParametersList / key ring, not once per call.
// Runs on the Node 12 of this image (the TypeScript sources of the reference need Node >= 24 and tsc).
'use strict'
const crypto = require('crypto')
const path = require('path')
const native = require(process.env.ZKATTEST_NODE || path.join(__dirname, 'zkattest.node'))

const STATUS_TEXT = { 1: 'point not in group', 2: 'invalid public key', 3: 'T[i] is at infinity', 4: 'T1 is at infinity', 5: 'P/Q/R is at infinity',
    6: "Points don't add up!", 7: 'R is at infinity', 8: 'params not found', 9: 'security level not achieved', 10: 'error deserializing',
    11: 'randomness stream exhausted', 16: "the index and blinder do not open the proof's key commitment" }
// The two places where the reference dies with a TypeError of the JavaScript runtime instead of one of its own errors (include/zkattest.h):
// `which` past the padded ring reads values[index].k of undefined (src/proofGK/gk.ts:162, engine status 14), and a ring of ONE key pads to
// length 1, n = 0, where interpolate([], []) evaluates -x[0] % m with x[0] undefined (src/proofGK/interpolate.ts:40).
function statusError(st) {
    if (st === 14) return new TypeError("Cannot read properties of undefined (reading 'k')")
    return new Error(STATUS_TEXT[st] || ('status ' + st))
}
function checkRingSize(nKeys, proving) {
    if (nKeys === 1 && proving) throw new TypeError('Cannot mix BigInt and other types, use explicit conversions')
    if (nKeys < 2) throw new RangeError('the key ring needs at least two keys (the reference cannot prove over fewer: interpolate.ts:40)')
}

// ---------------------------------------------------------------- big numbers and the two groups (host side, BigInt)
const mod = (a, m) => { const r = a % m; return r < 0n ? r + m : r }
function invMod(a, m) { // extended Euclid; invMod(0) = 0 like src/bignum/big.ts:80-119
    let [r0, r1, s0, s1] = [mod(a, m), m, 1n, 0n]
    while (r1 !== 0n) { const q = r0 / r1; [r0, r1] = [r1, r0 - q * r1]; [s0, s1] = [s1, s0 - q * s1] }
    return r0 === 1n ? mod(s0, m) : 0n
}
const hex = (v) => (v < 0n ? '-0x' + (-v).toString(16) : '0x' + v.toString(16))   // src/bignum/big.ts:230-239
const unhex = (s) => { if (typeof s !== 'string' || !s) throw new Error('the field is required'); return s[0] === '-' ? -BigInt(s.slice(1)) : BigInt(s) }
function toBE(v, len) { return Buffer.from(v.toString(16).padStart(2 * len, '0'), 'hex') }
const fromBE = (buf) => (buf.length ? BigInt('0x' + Buffer.from(buf).toString('hex')) : 0n)
function rnd(n) { // src/bignum/big.ts:171-181: byteLen(n) random bytes, retry while >= n
    const len = Math.ceil(n.toString(2).length / 8)
    for (;;) { const v = fromBE(crypto.randomBytes(len)); if (v < n) return v }
}

class Group { // src/curves/group.ts:20-61 (name, p, order); the arithmetic here is affine and only serves the one-time calls
    constructor(name, p, order, gen) { this.name = name; this.p = p; this.order = order; this.gen = gen }
    eq(g) { return this.name === g.name }
    generator() { return new Point(this, this.gen[0], this.gen[1]) }
    sizeFieldBytes() { return Math.ceil(this.p.toString(2).length / 8) }
    newScalar(k) { return new Scalar(this, k) }
    randomScalar() { return new Scalar(this, rnd(this.order)) }
    toJSON() { return { name: this.name } }
}
class WeierstrassGroup extends Group { // y^2 = x^3 + ax + b, src/curves/weier.ts:25-89
    constructor(name, p, a, b, order, gen) { super(name, p, order, gen); this.a = a; this.b = b }
    isOnGroup(pt) { const { p } = this; return pt.inf || mod(pt.y * pt.y - (pt.x * pt.x * pt.x + this.a * pt.x + this.b), p) === 0n }
    add(P, Q) {
        const { p } = this
        if (P.inf) return Q
        if (Q.inf) return P
        let l
        if (P.x === Q.x) {
            if (mod(P.y + Q.y, p) === 0n) return new Point(this, 0n, 1n, true)
            l = mod((3n * P.x * P.x + this.a) * invMod(2n * P.y, p), p)
        } else l = mod((Q.y - P.y) * invMod(Q.x - P.x, p), p)
        const x = mod(l * l - P.x - Q.x, p)
        return new Point(this, x, mod(l * (P.x - x) - P.y, p))
    }
    identity() { return new Point(this, 0n, 1n, true) }
}
class TEdwards extends Group { // a x^2 + y^2 = 1 + d x^2 y^2, src/curves/edwards.ts:25-86; the addition law is complete
    constructor(name, p, a, d, order, gen) { super(name, p, order, gen); this.a = a; this.d = d }
    isOnGroup(pt) { const { p } = this, x2 = pt.x * pt.x, y2 = pt.y * pt.y; return mod(this.a * x2 + y2 - 1n - this.d * x2 % p * y2, p) === 0n }
    add(P, Q) {
        const { p } = this, t = mod(this.d * P.x * Q.x % p * P.y * Q.y, p)
        return new Point(this, mod((P.x * Q.y + P.y * Q.x) * invMod(1n + t, p), p), mod((P.y * Q.y - this.a * P.x * Q.x) * invMod(1n - t, p), p))
    }
    identity() { return new Point(this, 0n, 1n) }
}
class Point { // affine; src/curves/weier.ts:92-101 / edwards.ts:89-98 serialise group, x, y
    constructor(group, x, y, inf = false) { this.group = group; this.x = x; this.y = y; this.inf = inf }
    eq(o) { return this.group.eq(o.group) && this.inf === o.inf && (this.inf || (this.x === o.x && this.y === o.y)) }
    add(o) { return this.group.add(this, o) }
    mul(k) { // double-and-add, MSB first (a one-time call: generateParamsList)
        const s = typeof k === 'bigint' ? mod(k, this.group.order) : k.k
        let r = this.group.identity()
        for (const bit of s.toString(2)) { r = r.add(r); if (bit === '1') r = r.add(this) }
        return r
    }
    isIdentity() { return this.group instanceof TEdwards ? this.x === 0n && this.y === 1n : this.inf }
    toAffine() { return this.group instanceof TEdwards || !this.inf ? { x: this.x, y: this.y } : false }
    toJSON() { return { group: this.group.toJSON(), x: hex(this.x), y: hex(this.y) } }
}
class Scalar { // src/curves/group.ts:155-218
    constructor(group, k) { this.group = group; this.k = k ? mod(BigInt(k), group.order) : 0n }
    eq(o) { return this.group.eq(o.group) && this.k === o.k }
    toJSON() { return { group: this.group.toJSON(), k: hex(this.k) } }
}
const P = (s) => BigInt(s)
const p256 = new WeierstrassGroup('p256', P('0xffffffff00000001000000000000000000000000ffffffffffffffffffffffff'),
    P('0xffffffff00000001000000000000000000000000fffffffffffffffffffffffc'), P('0x5ac635d8aa3a93e7b3ebbd55769886bc651d06b0cc53b0f63bce3c3e27d2604b'),
    P('0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551'),
    [P('0x6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296'), P('0x4fe342e2fe1a7f9b8ee7eb4a7c0f9e162bce33576b315ececbb6406837bf51f5')])
const tomEdwards256 = new TEdwards('tomEdwards256', P('0x3fffffffc000000040000000000000002ae382c7957cc4ff9713c3d82bc47d3af'),
    P('0x1abce3fd8e1d7a21252515332a512e09d4249bd5b1ec35e316c02254fe8cedf5d'), P('0x051781d9823abde00ec99295ba542c8b1401874bcbeb9e9c861174c7bca6a02aa'),
    P('0xffffffff00000001000000000000000000000000ffffffffffffffffffffffff'),
    [P('0x7907055d0a7d4abc3eafdc25d431d9659fbe007ee2d8ddc4e906206ea9ba4fdb'), P('0xbe231cb9f9bf18319c9f081141559b0a33dddccd2221f0464a9cd57081b01a01')])
const ALL_GROUPS = [p256, tomEdwards256]   // the reference also lists war256, which the ZKAttest path never touches
function groupByName(name) { // src/curves/instances.ts:58-78
    for (const g of ALL_GROUPS) if (g.name === name) return g
    throw new Error('invalid group name: ' + name)
}
function pointFromJson(o, want) { // onDeserialized: 'afterJson' re-validates every point (weier.ts:256-260, edwards.ts:204-209)
    if (!o || typeof o !== 'object' || !o.group) throw new Error('error deserializing a point')
    const g = groupByName(o.group.name)
    if (want && !g.eq(want)) throw new Error('point not in group')
    const pt = new Point(g, unhex(o.x), unhex(o.y))
    if (!g.isOnGroup(pt)) throw new Error('point not in group')
    return pt
}

// ---------------------------------------------------------------- parameter and proof classes
class PedersenParams { // src/commit/pedersen.ts:38-58
    constructor(c, g, h) { this.c = c; this.g = g; this.h = h }
    eq(o) { return this.c.eq(o.c) && this.g.eq(o.g) && this.h.eq(o.h) }
    toJSON() { return { c: this.c.toJSON(), g: this.g.toJSON(), h: this.h.toJSON() } }
    static fromJson(o) {
        if (!o || !o.c) throw new Error('error deserializing PedersenParams')
        const c = groupByName(o.c.name)
        return new PedersenParams(c, pointFromJson(o.g, c), pointFromJson(o.h, c))
    }
}
function generatePedersenParams(c, g) { // src/commit/pedersen.ts:61-69 (h = g * rnd; the TODO about hashing to the curve is the reference's)
    g = g || c.generator()
    return new PedersenParams(c, g, g.mul(c.randomScalar()))
}
class SystemParametersList { // src/zkpAttestList.ts:62-78
    constructor(NistGroup, ProofGroup, SecLevel) { this.NistGroup = NistGroup; this.ProofGroup = ProofGroup; this.SecLevel = SecLevel }
    eq(o) { return this.NistGroup.eq(o.NistGroup) && this.ProofGroup.eq(o.ProofGroup) && this.SecLevel == o.SecLevel }
    toJSON() { return { NistGroup: this.NistGroup.toJSON(), ProofGroup: this.ProofGroup.toJSON(), SecLevel: this.SecLevel } }
    static fromJson(o) {
        if (!o || typeof o.SecLevel !== 'number') throw new Error('error deserializing SystemParametersList')
        return new SystemParametersList(PedersenParams.fromJson(o.NistGroup), PedersenParams.fromJson(o.ProofGroup), o.SecLevel)
    }
    // the engine's form of the parameters: affine big-endian coordinates (include/zkattest.h)
    engineParams() {
        if (!this.NistGroup.c.eq(p256) || !this.ProofGroup.c.eq(tomEdwards256)) throw new Error('params: NistGroup must be p256 and ProofGroup tomEdwards256')
        if (!this.NistGroup.g.eq(p256.generator())) throw new Error('params: NistGroup.g must be the P-256 generator')
        const h = this.NistGroup.h, g2 = this.ProofGroup.g, h2 = this.ProofGroup.h
        return { nistH: Buffer.concat([toBE(h.x, 32), toBE(h.y, 32)]), tomG: Buffer.concat([toBE(g2.x, 36), toBE(g2.y, 36)]),
            tomH: Buffer.concat([toBE(h2.x, 36), toBE(h2.y, 36)]), secLevel: this.SecLevel }
    }
}
function generateParamsList(secLevel = 80) { // src/zkpAttestList.ts:88-92
    return new SystemParametersList(generatePedersenParams(p256), generatePedersenParams(tomEdwards256), secLevel)
}
// Hardened mode (include/zkattest.h; NOT byte-compatible with the reference, both sides must opt in): h of both groups derived
// from SHA-256 (nobody knows log_g h: the TODO of src/commit/pedersen.ts:62) and the statement hashed into the membership
// challenge (the TODO of src/proofGK/gk.ts:178).  `params.hardened = true` selects the mode for proveSignatureList /
// verifySignatureList; the flag is not part of the JSON form (set it again after readJson).
function generateParamsListHardened(secLevel = 80, tag = Buffer.alloc(0)) {
    const h = native.hardenedH(Buffer.from(tag))
    const pt = (g, buf, w) => new Point(g, fromBE(buf.slice(0, w)), fromBE(buf.slice(w)))
    const params = new SystemParametersList(new PedersenParams(p256, p256.generator(), pt(p256, h.nistH, 32)),
        new PedersenParams(tomEdwards256, tomEdwards256.generator(), pt(tomEdwards256, h.tomH, 36)), secLevel)
    params.hardened = true
    return params
}

// Proof objects keep the engine's ZKA1 bytes (the binary equivalent of the reference's object graph, include/zkattest.h) and
// materialise the reference's members (R, comS1, keyXcom, keyYcom, expProof[], membershipProof: Points and Scalars) on demand.
// ZKA1 framing (include/zkattest.h): magic, big-endian total length at byte 4 equal to the buffer's length, 4-byte granular.  Checked
// before a proof may enter a packed batch: a proof with a wrong length would shift every later proof of the blob.
function wellFormedProof(b) { return Buffer.isBuffer(b) && b.length >= 32 && b.length % 4 === 0 && (b.slice(0, 4).toString('latin1') === 'ZKA1' || b.slice(0, 4).toString('latin1') === 'ZK1P') && b.readUInt32BE(4) === b.length }
function revive(v) {
    if (Array.isArray(v)) return v.map(revive)
    if (v && typeof v === 'object') {
        if (v.group && 'x' in v && 'y' in v) return new Point(groupByName(v.group.name), unhex(v.x), unhex(v.y))
        if (v.group && 'k' in v) return new Scalar(groupByName(v.group.name), unhex(v.k))
        const o = {}
        for (const k of Object.keys(v)) if (k !== '__type') o[k] = revive(v[k])
        return o
    }
    return v
}
class SignatureProofList { // src/zkpAttestList.ts:27-60
    constructor(bytes) { if (!wellFormedProof(bytes)) throw new Error('error deserializing'); this.bytes = bytes }
    // the encoding is canonical: equal members <=> equal bytes of ONE layout; a ZKA1 and a ZK1P image of the same proof are equal through their (layout-free) JSON text
    eq(o) {
        if (!(o instanceof SignatureProofList)) return false
        if (this.bytes.slice(0, 4).equals(o.bytes.slice(0, 4))) return this.bytes.equals(o.bytes)
        return this.toJson() === o.toJson()
    }
    toJson() { return native.proofToJson(this.bytes) }
    get members() { if (!this._m) Object.defineProperty(this, '_m', { value: revive(JSON.parse(this.toJson())) }); return this._m }
    get R() { return this.members.R }
    get comS1() { return this.members.comS1 }
    get keyXcom() { return this.members.keyXcom }
    get keyYcom() { return this.members.keyYcom }
    get expProof() { return this.members.expProof }
    get membershipProof() { return this.members.membershipProof }
}
// Whole batches on every host core, off the event loop (zk_proofs_to_json_batch / zk_proofs_from_json_batch): at ~600 KB of text per
// proof the per-proof writeJson / readJson below cannot keep up with a GPU that makes 300 000 proofs a second.
function blobOf(items) {
    const off = new BigUint64Array(items.length + 1)
    let o = 0n
    items.forEach((b, i) => { off[i] = o; o += BigInt(b.length) })
    off[items.length] = o
    return { blob: items.length === 1 ? items[0] : Buffer.concat(items), offsets: Buffer.from(off.buffer) }
}
function cut(r) {
    const off = u64(r.offsets), st = i32(r.status), out = []
    for (let i = 0; i < st.length; i++) out.push(st[i] === 0 ? r.blob.slice(Number(off[i]), Number(off[i + 1])) : null)
    return out
}
// proofs: SignatureProofList[] | Buffer[]  ->  Promise<string[]>   (null where a proof is malformed)
async function writeJsonBatch(proofs, threads = 0) {
    const { blob, offsets } = blobOf(proofs.map((p) => (p instanceof SignatureProofList ? p.bytes : p)))
    return cut(await native.proofsToJsonBatch(blob, offsets, threads)).map((b) => (b === null ? null : b.toString('latin1')))
}
// texts: (string | Buffer)[]  ->  Promise<(SignatureProofList | null)[]>   (null where readJson would throw)
async function readJsonBatch(texts, threads = 0) {
    const { blob, offsets } = blobOf(texts.map((t) => (Buffer.isBuffer(t) ? t : Buffer.from(t, 'utf8'))))
    return cut(await native.proofsFromJsonBatch(blob, offsets, threads)).map((b) => (b === null ? null : new SignatureProofList(b)))
}
function writeJson(type, object) { // src/serde.ts:34-36
    if (type === SignatureProofList) return (object instanceof SignatureProofList ? object : new SignatureProofList(object)).toJson()
    if (type === SystemParametersList || type === PedersenParams) return JSON.stringify(object.toJSON())
    throw new Error('writeJson: unsupported class')
}
function readJson(type, text) { // src/serde.ts:21-32 (throws on bad input)
    if (type === SignatureProofList) return new SignatureProofList(native.proofFromJson(text))
    if (type === SystemParametersList) return SystemParametersList.fromJson(JSON.parse(text))
    if (type === PedersenParams) return PedersenParams.fromJson(JSON.parse(text))
    throw new Error('readJson: unsupported class')
}

// ---------------------------------------------------------------- low-level engine (one handle = the listed GPUs)
function be32(v) { return Buffer.isBuffer(v) ? v : toBE(mod(BigInt(v), 1n << 256n), 32) }
const i32 = (buf) => new Int32Array(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.length))
const u64 = (buf) => new BigUint64Array(buf.buffer.slice(buf.byteOffset, buf.byteOffset + buf.length))
function defaultDevices() { return (process.env.ZKATTEST_DEVICES || '0').split(',').map((s) => parseInt(s, 10)) }
function unpackProofs(r, B) {
    const st = i32(r.status), off = u64(r.offsets), len = u64(r.lengths), out = []
    for (let b = 0; b < B; b++) {
        if (st[b] !== 0) throw statusError(st[b])
        out.push(r.proofs.slice(Number(off[b]), Number(off[b] + len[b])))   // views of one (page-locked) buffer, no copies
    }
    return out
}
// Only well-formed proofs are packed (back to back, so every one starts 4-byte aligned); a malformed one never reaches the engine
// and cannot misalign its neighbours -- it is reported on its own as 'error deserializing', like the reference's readJson would.
function packProofs(proofs) {
    const good = [], slot = new Int32Array(proofs.length).fill(-1)
    for (let b = 0; b < proofs.length; b++) if (wellFormedProof(proofs[b])) { slot[b] = good.length; good.push(proofs[b]) }
    const B = good.length, off = new BigUint64Array(B), len = new BigUint64Array(B)
    let o = 0n
    for (let b = 0; b < B; b++) { off[b] = o; len[b] = BigInt(good[b].length); o += len[b] }
    return { blob: B === 1 ? good[0] : Buffer.concat(good), off: Buffer.from(off.buffer), len: Buffer.from(len.buffer), slot, n: B }
}
// -> booleans, one per submitted proof.  A proof for which the reference's verifier would THROW ('params not found', a point that
// does not deserialise, ...) is `false` here and its Error sits in the result's non-enumerable `errors[b]` (null otherwise): one bad
// proof must not deny the verdicts of the others.  verifySignatureList (one proof) rethrows, as the reference does.
function verdicts(r, slot) {
    const st = r ? i32(r.status) : null, out = [], errors = []
    for (let b = 0; b < slot.length; b++) {
        const k = slot[b]
        if (k < 0) { out.push(false); errors.push(new Error('error deserializing')); continue }
        errors.push(st[k] !== 0 ? statusError(st[k]) : null)
        out.push(st[k] === 0 && r.ok[k] === 1)
    }
    Object.defineProperty(out, 'errors', { value: errors })
    return out
}
function msgOf(msg, pk) {   // the message hashes of the packed proofs only
    if (pk.n === pk.slot.length) return msg
    const parts = []
    for (let b = 0; b < pk.slot.length; b++) if (pk.slot[b] >= 0) parts.push(msg.slice(32 * b, 32 * b + 32))
    return Buffer.concat(parts)
}
function idsOf(ids, pk) {   // the ring ids of the packed proofs only, as u32
    const all = Uint32Array.from(ids)
    return Buffer.from(pk.n === pk.slot.length ? all.buffer : all.filter((_, b) => pk.slot[b] >= 0).buffer)
}
function seedsOf(seeds, pk) {
    if (!seeds || pk.n === pk.slot.length) return seeds || null
    const parts = []
    for (let b = 0; b < pk.slot.length; b++) if (pk.slot[b] >= 0) parts.push(seeds.slice(32 * b, 32 * b + 32))
    return Buffer.concat(parts)
}
class Engine {
    constructor(devices = 0) {
        const ids = Array.isArray(devices) ? devices : [devices]
        this.h = native.createPool(Int32Array.from(ids))
        this.tail = Promise.resolve()
    }
    close() { if (this.h) native.destroyPool(this.h); this.h = null }
    info() { return native.poolInfo(this.h) }
    // chunk, lanes, combBits (before setParams), hostTaper, batchVerify, mode, slice, ringFold, verifyGroups, wire (0 ZKA1, 1 ZKA1P), verifyLevel (0 context, 1 per proof), verifyReps (0 sampled, 1 all), inflight;
    // residentRings (default 4): how many key rings the facade's context cache keeps built on this engine (engineFor: LRU by ring)
    setOption(name, value) {
        if (name === 'residentRings') {
            if (!(Number.isInteger(value) && value >= 1 && value <= 16)) throw new RangeError('residentRings: 1 .. 16')
            this.residentRings = value
            return
        }
        if (name === 'ringDelta') {   // facade only: a key list that differs from a resident ring in at most this many entries updates that ring in place (0 = off)
            if (!(Number.isInteger(value) && value >= 0)) throw new RangeError('ringDelta: an integer >= 0')
            this.ringDelta = value
            return
        }
        native.setOption(this.h, name, value)
    }
    wipe() { native.setOption(this.h, 'wipe', 0) }   // zk_ctx_wipe on every device: prover workspaces and staged inputs zeroed (also done by close() and after a failed prove)
    // params: { nistH: 64 B, tomG: 72 B, tomH: 72 B, secLevel } -- SystemParametersList as affine big-endian coordinates
    setParams(p) { native.setParams(this.h, p.nistH, p.tomG, p.tomH, p.secLevel || 80); this.params = p; this.auditor = null; this.auditors = null }   // (zk_ctx_set_params drops the auditor's key)
    setRing(keys) { return native.setRing(this.h, Buffer.isBuffer(keys) ? keys : Buffer.concat(keys.map(be32))) }
    // resident rings (include/zkattest.h zk_ctx_add_ring): built once, switched by id without a rebuild
    addRing(keys) { return native.addRing(this.h, Buffer.isBuffer(keys) ? keys : Buffer.concat(keys.map(be32))) }   // -> ring id (not made active)
    useRing(id) { native.useRing(this.h, id) }
    dropRing(id) { native.dropRing(this.h, id) }   // the active ring cannot be dropped
    ringInfo(id) { return native.ringInfo(this.h, id) }   // -> { nKeys, logN, flags, generation }
    // zk_pool_update_ring: the resident ring becomes what setRing of the changed key list would build, rewriting only what the change touches.
    // indices[j] gets keys[j] (a Buffer of 32-byte entries or bigint[]; a later entry for the same index wins); nKeys: the new key count (default: unchanged)
    updateRing(id, indices, keys, nKeys) {
        const idx = Buffer.from(BigUint64Array.from(Array.from(indices, (i) => BigInt(i))).buffer)
        const kb = Buffer.isBuffer(keys) ? keys : Buffer.concat(keys.map(be32))
        native.updateRing(this.h, id, idx, kb, nKeys === undefined ? this.ringInfo(id).nKeys : nKeys)
    }
    synthParams(seed) { return Object.assign(native.synthParams(this.h, seed), { secLevel: 80 }) }
    synthWorkload(seed, nKeys, B) { return native.synthWorkload(this.h, seed, nKeys, B) }
    keysToInts(pkxy) { return native.keysToInts(this.h, pkxy) }                       // keyToInt over a key set
    _proveArgs(msg, which, seeds) {
        const B = msg.length / 32
        return [B, Buffer.isBuffer(which) ? which : Buffer.from(Uint32Array.from(which).buffer), seeds || crypto.randomBytes(32 * B)]   // one fresh seed per proof
    }
    // -> array of proof Buffers; throws the reference's error text for the first failed proof
    proveBatch(msg, sig, pk, which, seeds) {
        const [B, w, s] = this._proveArgs(msg, which, seeds)
        return unpackProofs(native.proveBatch(this.h, msg, sig, pk, w, s), B)
    }
    // -> array of booleans; exceptions of the reference's verifier are thrown for the first proof that has one
    verifyBatch(msg, proofs, seeds) {
        const pk = packProofs(proofs)
        return verdicts(pk.n ? native.verifyBatch(this.h, msgOf(msg, pk), pk.blob, pk.off, pk.len, seedsOf(seeds, pk)) : null, pk.slot)
    }
    // Promise-returning variants: the batch runs on a libuv worker thread; jobs of one engine are chained (one batch at a time)
    _chain(run) { this.tail = this.tail.then(run, run); return this.tail }
    _proveNow(msg, sig, pk, which, seeds) {
        const [B, w, s] = this._proveArgs(msg, which, seeds)
        return native.proveBatchAsync(this.h, msg, sig, pk, w, s).then((r) => unpackProofs(r, B))
    }
    _verifyNow(msg, proofs, seeds) {
        const pk = packProofs(proofs)
        if (!pk.n) return Promise.resolve(verdicts(null, pk.slot))
        return native.verifyBatchAsync(this.h, msgOf(msg, pk), pk.blob, pk.off, pk.len, seedsOf(seeds, pk)).then((r) => verdicts(r, pk.slot))
    }
    // one resident ring id per proof (zk_verify_batch_rings): -> array of booleans with .errors, like verifyBatch
    verifyBatchRings(msg, proofs, ringIds, seeds) {
        const pk = packProofs(proofs)
        return verdicts(pk.n ? native.verifyBatchRings(this.h, msgOf(msg, pk), pk.blob, pk.off, pk.len, idsOf(ringIds, pk), seedsOf(seeds, pk)) : null, pk.slot)
    }
    _verifyRingsNow(msg, proofs, ringIds, seeds) {
        const pk = packProofs(proofs)
        if (!pk.n) return Promise.resolve(verdicts(null, pk.slot))
        return native.verifyBatchRingsAsync(this.h, msgOf(msg, pk), pk.blob, pk.off, pk.len, idsOf(ringIds, pk), seedsOf(seeds, pk)).then((r) => verdicts(r, pk.slot))
    }
    // one resident ring id per proof (zk_prove_batch_rings): which[b] indexes ring ringIds[b]; the active ring plays no part.  -> array of proof Buffers
    proveBatchRings(msg, sig, pk, which, ringIds, seeds) {
        const [B, w, s] = this._proveArgs(msg, which, seeds)
        return unpackProofs(native.proveBatchRings(this.h, msg, sig, pk, w, Buffer.from(Uint32Array.from(ringIds).buffer), s), B)
    }
    _proveRingsNow(msg, sig, pk, which, ringIds, seeds) {
        const [B, w, s] = this._proveArgs(msg, which, seeds)
        return native.proveBatchRingsAsync(this.h, msg, sig, pk, w, Buffer.from(Uint32Array.from(ringIds).buffer), s).then((r) => unpackProofs(r, B))
    }
    // zk_screen_batch_rings: is each witness worth a proof?  which: indices to check, or null to find them; -> { which: number[] (WHICH_NONE where absent), flags: number[] (SCREEN_* bits) }
    screenBatchRings(msg, sig, pk, which, ringIds) {
        const r = native.screenBatchRings(this.h, msg, sig, pk, which ? Buffer.from(Uint32Array.from(which).buffer) : null, Buffer.from(Uint32Array.from(ringIds).buffer))
        const u32 = (b) => Array.from({ length: b.length / 4 }, (_, i) => b.readUInt32LE(4 * i))
        return { which: u32(r.which), flags: u32(r.flags) }
    }
    // zk_recover_batch_rings: -> { pk: Buffer (64 B per witness, zeros where flags != 0), which, flags }
    recoverBatchRings(msg, sig, ringIds) {
        const r = native.recoverBatchRings(this.h, msg, sig, Buffer.from(Uint32Array.from(ringIds).buffer))
        const u32 = (b) => Array.from({ length: b.length / 4 }, (_, i) => b.readUInt32LE(4 * i))
        return { pk: r.pk, which: u32(r.which), flags: u32(r.flags) }
    }
    // ring membership on its own (zk_member_*), on the ACTIVE ring: -> { proofs: Buffer[] | null per entry, coms: Buffer[] (72 B), blinders: Buffer[] (32 B), status: Int32Array }
    memberProofSize() { return native.memberProofSize(this.h) }
    // context (B x 32 bytes, or null): the bound forms, "ZKMB" (zk_member_*_bound)
    memberProveBatch(which, blinders, seeds, context) {
        const B = which.length, size = this.memberProofSize(), w = Buffer.from(Uint32Array.from(which).buffer), sd = seeds || crypto.randomBytes(32 * B)   // one fresh seed per proof
        const r = context ? native.memberProveBatchBound(this.h, w, blinders || null, sd, context) : native.memberProveBatch(this.h, w, blinders || null, sd)
        const st = i32(r.status), cut = (b, w) => Array.from({ length: B }, (_, i) => b.slice(w * i, w * i + w))
        return { proofs: cut(r.proofs, size).map((p, i) => (st[i] === 0 ? p : null)), coms: cut(r.coms, 72), blinders: cut(r.blinders, 32), status: st }
    }
    memberVerifyBatch(coms, proofs, context) {   // -> { ok: boolean[], status: Int32Array }
        const r = context ? native.memberVerifyBatchBound(this.h, Buffer.concat(coms), Buffer.concat(proofs), context) : native.memberVerifyBatch(this.h, Buffer.concat(coms), Buffer.concat(proofs))
        return { ok: Array.from(r.ok, (v) => v === 1), status: i32(r.status) }
    }
    // ... with one resident ring id per entry (zk_member_*_batch_rings): the active ring plays no part; an id that is not resident gives status 14 and no proof
    memberProofSizeRing(ringId) { return native.memberProofSizeRing(this.h, ringId) }
    memberProveBatchRings(which, ringIds, blinders, seeds, context) {
        const B = which.length, u32 = (a) => Buffer.from(Uint32Array.from(a).buffer), sd = seeds || crypto.randomBytes(32 * B)   // one fresh seed per proof
        const r = context ? native.memberProveBatchRingsBound(this.h, u32(which), u32(ringIds), blinders || null, sd, context) : native.memberProveBatchRings(this.h, u32(which), u32(ringIds), blinders || null, sd)
        const st = i32(r.status), cut = (b, w) => Array.from({ length: B }, (_, i) => b.slice(w * i, w * i + w))
        const off = Array.from({ length: B + 1 }, (_, i) => Number(r.off.readBigUInt64LE(8 * i)))
        return { proofs: st.length ? Array.from(st, (s, i) => (s === 0 ? r.proofs.slice(off[i], off[i + 1]) : null)) : [], coms: cut(r.coms, 72), blinders: cut(r.blinders, 32), status: st, off, raw: r.proofs }
    }
    memberVerifyBatchRings(coms, proofs, ringIds, context) {   // proofs: one Buffer per entry, laid back to back -> { ok: boolean[], status: Int32Array }
        const off = Buffer.alloc(8 * (proofs.length + 1))
        let run = 0
        proofs.forEach((p, i) => { run += p.length; off.writeBigUInt64LE(BigInt(run), 8 * (i + 1)) })
        const ids = Buffer.from(Uint32Array.from(ringIds).buffer)
        const r = context ? native.memberVerifyBatchRingsBound(this.h, Buffer.concat(coms), Buffer.concat(proofs), off, ids, context) : native.memberVerifyBatchRings(this.h, Buffer.concat(coms), Buffer.concat(proofs), off, ids)
        return { ok: Array.from(r.ok, (v) => v === 1), status: i32(r.status) }
    }
    // re-ring (zk_prove_key_blinders, zk_proof_rering_batch).  keyBlinders: seeds (B x 32 bytes) -> Buffer[] of keyXcom's blinders, as secret as the seeds.
    keyBlinders(seeds) {
        const r = native.keyBlinders(this.h, seeds)
        return Array.from({ length: seeds.length / 32 }, (_, i) => r.slice(32 * i, 32 * i + 32))
    }
    // proofs (Buffers in the engine's wire layout) moved to the ACTIVE ring: -> { proofs: Buffer | null per entry, status: Int32Array }.  seeds must be FRESH:
    // never the ones the proofs were made with (default: crypto.randomBytes)
    reringBatch(msg, proofs, whichNew, blinders, seeds) {
        const B = proofs.length, off = Buffer.alloc(8 * (B + 1))
        let run = 0
        proofs.forEach((p, i) => { run += p.length; off.writeBigUInt64LE(BigInt(run), 8 * (i + 1)) })
        const r = native.reringBatch(this.h, msg, Buffer.concat(proofs), off, Buffer.from(Uint32Array.from(whichNew).buffer), blinders, seeds || crypto.randomBytes(32 * B))
        const st = i32(r.status), o = u64(r.off)
        return { proofs: Array.from(st, (s, i) => (s === 0 ? r.proofs.slice(Number(o[i]), Number(o[i + 1])) : null)), status: st }
    }
    // zk_proof_rering_batch_rings: proof i moved to the RESIDENT ring ringIds[i]; the active ring is neither read nor changed.  A proof whose status is not 0
    // comes back as null (its slot in the call's output is empty or zero-filled).  seeds must be FRESH (default: crypto.randomBytes)
    reringBatchRings(msg, proofs, whichNew, ringIds, blinders, seeds) {
        const B = proofs.length, off = Buffer.alloc(8 * (B + 1))
        let run = 0
        proofs.forEach((p, i) => { run += p.length; off.writeBigUInt64LE(BigInt(run), 8 * (i + 1)) })
        const r = native.reringBatchRings(this.h, msg, Buffer.concat(proofs), off, Buffer.from(Uint32Array.from(whichNew).buffer), Buffer.from(Uint32Array.from(ringIds).buffer), blinders,
            seeds || crypto.randomBytes(32 * B))
        const st = i32(r.status), o = u64(r.off)
        return { proofs: Array.from(st, (s, i) => (s === 0 ? r.proofs.slice(Number(o[i]), Number(o[i + 1])) : null)), status: st }
    }
    // link proofs (zk_link_*): "ZKL1", 256 bytes -- com1[i] and com2[i] (72-byte Tom-256 points) open to keys[i] under blinder1[i] / blinder2[i].  Arrays of Buffers
    // -> { proofs: Buffer | null per entry, status: Int32Array }.  seeds must be FRESH: never the ones either commitment's proof was made with (default: crypto.randomBytes)
    linkProveBatch(keys, com1, blinder1, com2, blinder2, seeds) {
        const B = keys.length, cat = (a) => Buffer.concat(a.map((v) => Buffer.from(v)))
        const r = native.linkProveBatch(this.h, cat(keys), cat(com1), cat(blinder1), cat(com2), cat(blinder2), seeds || crypto.randomBytes(32 * B))
        const st = i32(r.status)
        return { proofs: Array.from(st, (s, i) => (s === 0 ? r.proofs.slice(256 * i, 256 * i + 256) : null)), status: st }
    }
    linkVerifyBatch(com1, com2, proofs) {   // -> { ok: boolean[], status: Int32Array }
        const r = native.linkVerifyBatch(this.h, Buffer.concat(com1), Buffer.concat(com2), Buffer.concat(proofs))
        return { ok: Array.from(r.ok, (v) => v === 1), status: i32(r.status) }
    }
    // escrow tags (zk_ctx_set_auditor, zk_escrow_*): "ZKT1", 472 bytes -- ElGamal of keys[i] under the auditor's key with a proof that com[i] opens to it under
    // blinder[i].  setAuditor: the key A as a 72-byte Tom-256 point, again after every setParams; escrowKeygen: A = a g for a 32-byte secret.  Arrays of Buffers
    // -> { tags: Buffer | null per entry, status: Int32Array }.  seeds must be FRESH: never the ones the commitment's proof was made with (default: crypto.randomBytes)
    setAuditor(key72) { native.setAuditor(this.h, Buffer.from(key72)); this.auditor = Buffer.from(key72).toString('hex'); this.auditors = null }
    escrowKeygen(secret32) { return native.escrowKeygen(this.h, Buffer.from(secret32)) }
    escrowProveBatch(keys, com, blinder, seeds) {
        const B = keys.length, cat = (a) => Buffer.concat(a.map((v) => Buffer.from(v)))
        const r = native.escrowProveBatch(this.h, cat(keys), cat(com), cat(blinder), seeds || crypto.randomBytes(32 * B))
        const st = i32(r.status)
        return { tags: Array.from(st, (s, i) => (s === 0 ? r.tags.slice(472 * i, 472 * i + 472) : null)), status: st }
    }
    escrowVerifyBatch(com, tags) {   // -> { ok: boolean[], status: Int32Array }
        const r = native.escrowVerifyBatch(this.h, Buffer.concat(com), Buffer.concat(tags))
        return { ok: Array.from(r.ok, (v) => v === 1), status: i32(r.status) }
    }
    // the auditor's call against the ACTIVE ring -> { index: number[] (0xffffffff: nobody), status: Int32Array }.  It does not verify.
    escrowOpenBatch(secret32, tags) {
        const r = native.escrowOpenBatch(this.h, Buffer.from(secret32), Buffer.concat(tags))
        return { index: Array.from(tags, (_, i) => r.index.readUInt32LE(4 * i)), status: i32(r.status) }
    }
    // zk_rings_escrow_open_batch: one resident ring id per tag (0xffffffff: any resident ring, ascending ids); the active ring is not involved
    ringsEscrowOpenBatch(secret32, tags, ringIds) {
        const r = native.ringsEscrowOpenBatch(this.h, Buffer.from(secret32), Buffer.concat(tags), Buffer.from(Uint32Array.from(ringIds).buffer))
        return { ring: Array.from(tags, (_, i) => r.ring.readUInt32LE(4 * i)), index: Array.from(tags, (_, i) => r.index.readUInt32LE(4 * i)), status: i32(r.status) }
    }
    // threshold opening (zk_auditors_*, zk_ctx_set_auditors): t of n auditors open a tag through 264-byte shares "ZKS1".  auditorsSplitKey: the dealer's split
    // -> { shares: n 32-byte Buffers, keys: n 72-byte Buffers }; auditorsSetKeys: the share keys, behind setAuditor (which drops them, as setParams does).
    auditorsSplitKey(secret32, t, n, seed) {
        const r = native.auditorsSplitKey(this.h, Buffer.from(secret32), t, n, seed || crypto.randomBytes(32))
        return { shares: Array.from({ length: n }, (_, j) => r.shares.slice(32 * j, 32 * j + 32)), keys: Array.from({ length: n }, (_, j) => r.keys.slice(72 * j, 72 * j + 72)) }
    }
    auditorsSetKeys(t, keys) {
        this.auditors = null
        native.auditorsSetKeys(this.h, t, Buffer.concat(keys.map((k) => Buffer.from(k))))
        this.auditors = t + ':' + keys.map((k) => Buffer.from(k).toString('hex')).join('')
    }
    auditorsShareBatch(j, shareSecret32, tags, seeds) {   // -> { shares: Buffer | null per tag, status: Int32Array }; seeds must be FRESH (default: crypto.randomBytes)
        const r = native.auditorsShareBatch(this.h, j, Buffer.from(shareSecret32), Buffer.concat(tags), seeds || crypto.randomBytes(32 * tags.length))
        const st = i32(r.status)
        return { shares: Array.from(st, (s, i) => (s === 0 ? r.shares.slice(264 * i, 264 * i + 264) : null)), status: st }
    }
    auditorsShareVerifyBatch(tags, shares) {   // -> { ok: boolean[], status: Int32Array }; the auditor's index comes from each share's header
        const r = native.auditorsShareVerifyBatch(this.h, Buffer.concat(tags), Buffer.concat(shares))
        return { ok: Array.from(r.ok, (v) => v === 1), status: i32(r.status) }
    }
    // shares[s][b]: auditors[s]'s share of tags[b]; one resident ring id per tag (0xffffffff: any resident ring) -> ringsEscrowOpenBatch's result.  It does not verify.
    auditorsCombineBatch(auditors, tags, shares, ringIds) {
        const r = native.auditorsCombineBatch(this.h, Buffer.from(Uint32Array.from(auditors).buffer), Buffer.concat(tags), Buffer.concat(shares.map((row) => Buffer.concat(row))),
            Buffer.from(Uint32Array.from(ringIds).buffer))
        return { ring: Array.from(tags, (_, i) => r.ring.readUInt32LE(4 * i)), index: Array.from(tags, (_, i) => r.index.readUInt32LE(4 * i)), status: i32(r.status) }
    }
    // distinct-key proofs (zk_distinct_*): "ZKD1", 744 bytes -- com1[i] opens to key1[i] under blinder1[i], com2[i] to key2[i] under blinder2[i], and the keys differ;
    // the proof verifies for (com1, com2) in this order only.  Arrays of Buffers -> { proofs: Buffer | null per entry, status: Int32Array } (status 14: equal keys).
    // seeds must be FRESH: never the ones either commitment's proof was made with (default: crypto.randomBytes)
    distinctProveBatch(key1, com1, blinder1, key2, com2, blinder2, seeds) {
        const B = key1.length, cat = (a) => Buffer.concat(a.map((v) => Buffer.from(v)))
        const r = native.distinctProveBatch(this.h, cat(key1), cat(com1), cat(blinder1), cat(key2), cat(com2), cat(blinder2), seeds || crypto.randomBytes(32 * B))
        const st = i32(r.status)
        return { proofs: Array.from(st, (s, i) => (s === 0 ? r.proofs.slice(744 * i, 744 * i + 744) : null)), status: st }
    }
    distinctVerifyBatch(com1, com2, proofs) {   // -> { ok: boolean[], status: Int32Array }
        const r = native.distinctVerifyBatch(this.h, Buffer.concat(com1), Buffer.concat(com2), Buffer.concat(proofs))
        return { ok: Array.from(r.ok, (v) => v === 1), status: i32(r.status) }
    }
    // quorum proofs (zk_quorum_*): "ZKQ1" bundles over the ACTIVE ring -- Q quorums of k members; member m = q k + i takes row m of msg, sig, pk (64-byte x | y),
    // whichs and seeds, pair p of quorum q row q k (k - 1) / 2 + p of pairSeeds.  -> { bundles: Buffer | null per quorum, status: Int32Array, memberStatus: Int32Array }
    // (status 14: two members of the quorum have the same key).  Both seed sets must be FRESH and independent of each other (default: crypto.randomBytes)
    quorumProveBatch(k, msg, sig, pk, whichs, seeds, pairSeeds) {
        const n = whichs.length, Q = n / k, P = k * (k - 1) / 2
        const r = native.quorumProveBatch(this.h, k, msg, sig, pk, Buffer.from(Uint32Array.from(whichs).buffer), seeds || crypto.randomBytes(32 * n), pairSeeds || crypto.randomBytes(32 * Q * P))
        const st = i32(r.status), o = u64(r.off)
        return { bundles: Array.from(st, (s, q) => (s === 0 ? r.bundles.slice(Number(o[q]), Number(o[q + 1])) : null)), status: st, memberStatus: i32(r.memberStatus) }
    }
    // -> { ok: boolean[], status: Int32Array, firstBad: Uint32Array } -- firstBad names the first member (< k) or pair (k + p) that failed, 0xFFFFFFFF where ok
    quorumVerifyBatch(k, msg, bundles) {
        const Q = bundles.length, off = Buffer.alloc(8 * (Q + 1))
        let run = 0
        bundles.forEach((b, q) => { run += b.length; off.writeBigUInt64LE(BigInt(run), 8 * (q + 1)) })
        const r = native.quorumVerifyBatch(this.h, k, msg, Buffer.concat(bundles), off)
        return { ok: Array.from(r.ok, (v) => v === 1), status: i32(r.status), firstBad: new Uint32Array(Uint8Array.from(r.firstBad).buffer) }
    }
    // accountable attestations (zk_accountable_*): "ZKC1" bundles over the ACTIVE ring under the engine's auditor key -- bundle b takes row b of msg, sig, pk (64-byte
    // x | y), whichs, seeds and tagSeeds.  -> { bundles: Buffer | null per bundle, status: Int32Array, partStatus: Int32Array (attestation, tag per bundle) }.  Both
    // seed sets must be FRESH and independent of each other (default: crypto.randomBytes)
    accountableProveBatch(msg, sig, pk, whichs, seeds, tagSeeds) {
        const B = whichs.length
        const r = native.accountableProveBatch(this.h, msg, sig, pk, Buffer.from(Uint32Array.from(whichs).buffer), seeds || crypto.randomBytes(32 * B), tagSeeds || crypto.randomBytes(32 * B))
        const st = i32(r.status), o = u64(r.off)
        return { bundles: Array.from(st, (s, b) => (s === 0 ? r.bundles.slice(Number(o[b]), Number(o[b + 1])) : null)), status: st, partStatus: i32(r.partStatus) }
    }
    // -> { ok: boolean[], status: Int32Array, firstBad: Uint32Array } -- firstBad is 0 for the attestation, 1 for the tag, 0xFFFFFFFF where ok
    accountableVerifyBatch(msg, bundles) {
        const r = native.accountableVerifyBatch(this.h, msg, Buffer.concat(bundles), slotOffsets(bundles))
        return { ok: Array.from(r.ok, (v) => v === 1), status: i32(r.status), firstBad: new Uint32Array(Uint8Array.from(r.firstBad).buffer) }
    }
    // zk_accountable_split_batch, pure layout: -> { attestations: Buffer[] (empty for a refused bundle), tags: Buffer[] (472 bytes each, zero for a refused bundle), status }
    accountableSplitBatch(bundles) {
        const B = bundles.length, r = native.accountableSplitBatch(this.h, Buffer.concat(bundles), slotOffsets(bundles)), o = u64(r.off)
        return { attestations: Array.from({ length: B }, (_, b) => r.attestations.slice(Number(o[b]), Number(o[b + 1]))),
            tags: Array.from({ length: B }, (_, b) => r.tags.slice(472 * b, 472 * b + 472)), status: i32(r.status) }
    }
    // zk_accountable_join_batch, pure layout: -> { bundles: Buffer | null per proof, status }
    accountableJoinBatch(proofs, tags) {
        const r = native.accountableJoinBatch(this.h, Buffer.concat(proofs), slotOffsets(proofs), Buffer.concat(tags)), st = i32(r.status), o = u64(r.off)
        return { bundles: Array.from(st, (s, b) => (s === 0 ? r.bundles.slice(Number(o[b]), Number(o[b + 1])) : null)), status: st }
    }
    // zk_rings_accountable_prove_batch / _verify_batch / _open_batch: the same with one RESIDENT ring id per bundle (ringIds[b]; whichs[b] indexes that ring); the
    // active ring is neither read nor changed.  The open is the auditor's call straight on bundles (0xffffffff = any resident ring) -> { ring, index, status } as
    // ringsEscrowOpenBatch; it does NOT verify
    accountableProveBatchRings(msg, sig, pk, whichs, ringIds, seeds, tagSeeds) {
        const B = whichs.length, u32 = (v) => Buffer.from(Uint32Array.from(v).buffer)
        const r = native.accountableProveBatchRings(this.h, msg, sig, pk, u32(whichs), u32(ringIds), seeds || crypto.randomBytes(32 * B), tagSeeds || crypto.randomBytes(32 * B))
        const st = i32(r.status), o = u64(r.off)
        return { bundles: Array.from(st, (s, b) => (s === 0 ? r.bundles.slice(Number(o[b]), Number(o[b + 1])) : null)), status: st, partStatus: i32(r.partStatus) }
    }
    accountableVerifyBatchRings(msg, bundles, ringIds) {
        const r = native.accountableVerifyBatchRings(this.h, msg, Buffer.concat(bundles), slotOffsets(bundles), Buffer.from(Uint32Array.from(ringIds).buffer))
        return { ok: Array.from(r.ok, (v) => v === 1), status: i32(r.status), firstBad: new Uint32Array(Uint8Array.from(r.firstBad).buffer) }
    }
    accountableOpenBatchRings(secret32, bundles, ringIds) {
        const r = native.accountableOpenBatchRings(this.h, Buffer.from(secret32), Buffer.concat(bundles), slotOffsets(bundles), Buffer.from(Uint32Array.from(ringIds).buffer))
        const w = (b) => new Uint32Array(Uint8Array.from(b).buffer)
        return { ring: w(r.ring), index: w(r.index), status: i32(r.status) }
    }
    // zk_rings_quorum_prove_batch / zk_rings_quorum_verify_batch: the same with one RESIDENT ring id per member (ringIds[m]; whichs[m] indexes that ring); the
    // active ring plays no part.  A key enrolled in two rings and used through both is "the same key" (status 14)
    ringsQuorumProveBatch(k, msg, sig, pk, whichs, ringIds, seeds, pairSeeds) {
        const n = whichs.length, Q = n / k, P = k * (k - 1) / 2
        const u32 = (a) => Buffer.from(Uint32Array.from(a).buffer)
        const r = native.ringsQuorumProveBatch(this.h, k, msg, sig, pk, u32(whichs), u32(ringIds), seeds || crypto.randomBytes(32 * n), pairSeeds || crypto.randomBytes(32 * Q * P))
        const st = i32(r.status), o = u64(r.off)
        return { bundles: Array.from(st, (s, q) => (s === 0 ? r.bundles.slice(Number(o[q]), Number(o[q + 1])) : null)), status: st, memberStatus: i32(r.memberStatus) }
    }
    ringsQuorumVerifyBatch(k, msg, bundles, ringIds) {
        const Q = bundles.length, off = Buffer.alloc(8 * (Q + 1))
        let run = 0
        bundles.forEach((b, q) => { run += b.length; off.writeBigUInt64LE(BigInt(run), 8 * (q + 1)) })
        const r = native.ringsQuorumVerifyBatch(this.h, k, msg, Buffer.concat(bundles), off, Buffer.from(Uint32Array.from(ringIds).buffer))
        return { ok: Array.from(r.ok, (v) => v === 1), status: i32(r.status), firstBad: new Uint32Array(Uint8Array.from(r.firstBad).buffer) }
    }
    // zk_proof_key_commitments: keyXcom of every proof (Buffers in the engine's wire layout) as a 72-byte point -> { coms: Buffer | null per entry, status: Int32Array }
    keyCommitments(proofs) {
        const B = proofs.length, off = Buffer.alloc(8 * (B + 1))
        let run = 0
        proofs.forEach((p, i) => { run += p.length; off.writeBigUInt64LE(BigInt(run), 8 * (i + 1)) })
        const r = native.keyCommitments(this.h, Buffer.concat(proofs), off)
        const st = i32(r.status)
        return { coms: Array.from(st, (s, i) => (s === 0 ? r.coms.slice(72 * i, 72 * i + 72) : null)), status: st }
    }
    proveBatchRingsAsync(msg, sig, pk, which, ringIds, seeds) { return this._chain(() => this._proveRingsNow(msg, sig, pk, which, ringIds, seeds)) }
    verifyBatchRingsAsync(msg, proofs, ringIds, seeds) { return this._chain(() => this._verifyRingsNow(msg, proofs, ringIds, seeds)) }
    proveBatchAsync(msg, sig, pk, which, seeds) { return this._chain(() => this._proveNow(msg, sig, pk, which, seeds)) }
    verifyBatchAsync(msg, proofs, seeds) { return this._chain(() => this._verifyNow(msg, proofs, seeds)) }
    run(f) { return this._chain(f) }   // any other call on the handle, queued behind the running batches
    // Streamed form (zk_pool_prove_submit / _wait, DESIGN.md 5c): every call returns its Promise at once and up to `inflight` batches are
    // inside the engine together (setOption('inflight', n), default 3), so the pipeline does not drain between batches.  `out` /
    // `blob` are page-locked Buffers (Engine.hostAlloc) owned by the job until its Promise settles -- one per batch in flight.
    // No other call on this engine until every streamed Promise has settled.
    static hostAlloc(bytes) { return native.hostAlloc(bytes) }
    proveStream(msg, sig, pk, which, seeds, out) {   // -> { proofs: Buffer[] (views into out), status: Int32Array }
        const [B, w, s] = this._proveArgs(msg, which, seeds)
        return native.proveSubmit(this.h, msg, sig, pk, w, s, out).then((r) => {
            const off = u64(r.offsets), len = u64(r.lengths)
            return { proofs: Array.from({ length: B }, (_, b) => r.proofs.slice(Number(off[b]), Number(off[b] + len[b]))), status: i32(r.status), used: r.used }
        })
    }
    verifyStream(msg, blob, offsets, lengths, seeds) {   // packed proofs in a page-locked Buffer -> { ok: boolean[], status: Int32Array }
        return native.verifySubmit(this.h, msg, blob, offsets, lengths, seeds || null).then((r) => ({ ok: Array.from(r.ok, (v) => v === 1), status: i32(r.status) }))
    }
}

// ---------------------------------------------------------------- context cache: (params) -> engine, (engine, ring) -> loaded
const engines = new Map()      // sha256(params bytes | secLevel | devices) -> { engine, ringTag }
const ringCache = new WeakMap() // keys array -> { buf, tag }: valid only while the array is FROZEN (nobody can change it in place)
// The loaded ring is identified by the SHA-256 of the whole key list (2 MiB at 2^16 keys: a few milliseconds).  A mutable bigint[]
// is serialised and hashed on EVERY call -- a cached copy validated by a sample would silently prove against a stale ring after an
// in-place change of an unsampled element; callers that want the serialisation cached pass a Buffer or Object.freeze(keys).
function ringOf(keys) {
    if (Buffer.isBuffer(keys)) return { buf: keys, tag: crypto.createHash('sha256').update(keys).digest('hex') }
    const frozen = Object.isFrozen(keys)
    let c = frozen ? ringCache.get(keys) : undefined
    if (!c) {
        const buf = Buffer.concat(keys.map(be32))
        c = { buf, tag: crypto.createHash('sha256').update(buf).digest('hex') }
        if (frozen) ringCache.set(keys, c)
    }
    return c
}
// (B + 1) u64 LE offsets of byte strings laid back to back
function slotOffsets(blobs) {
    const off = Buffer.alloc(8 * (blobs.length + 1))
    let run = 0
    blobs.forEach((b, i) => { run += b.length; off.writeBigUInt64LE(BigInt(run), 8 * (i + 1)) })
    return off
}
function engineFor(params, keys) {
    if (!(params instanceof SystemParametersList)) throw new TypeError('params: a SystemParametersList (generateParamsList / readJson)')
    if (!params._ep) {
        const ep = params.engineParams(), devices = defaultDevices()
        const tag = crypto.createHash('sha256').update(ep.nistH).update(ep.tomG).update(ep.tomH).update(String(ep.secLevel) + '|' + devices.join(',')).digest('hex')
        Object.defineProperty(params, '_tag0', { value: tag })
        Object.defineProperty(params, '_ep', { value: ep })
    }
    lastParams = params
    const key = params._tag0 + (params.hardened ? '|hardened' : '')
    let slot = engines.get(key)
    if (!slot) {
        const engine = new Engine(defaultDevices())
        if (process.env.ZKATTEST_COMB_BITS) engine.setOption('combBits', parseInt(process.env.ZKATTEST_COMB_BITS, 10))
        if (params.hardened) engine.setOption('mode', 1)
        engine.setParams(params._ep)           // builds the fixed-base tables: once per SystemParametersList
        slot = { engine, rings: new Map(), active: null, bufs: new Map() }   // rings: ring tag -> resident ring id, least recently used first; bufs: ring tag -> key bytes (ringDelta)
        engines.set(key, slot)
    }
    if (keys === null) return { engine: slot.engine, run: (job) => slot.engine.run(() => job(slot.engine)) }   // a call that reads no ring (keyBlinders)
    const ring = ringOf(keys)
    // one queued unit per call: make the ring resident and active (table E and the rest: once per key ring while it stays among the engine's
    // `residentRings` most recently used), then run the batch; units of one engine run strictly one after the other, so interleaved callers with
    // different rings cannot mix them up
    const withRing = (job) => slot.engine.run(() => {
        residentRing(slot, ring)
        if (slot.active !== ring.tag) { slot.engine.useRing(slot.rings.get(ring.tag)); slot.active = ring.tag }
        return job(slot.engine)
    })
    // several rings in one unit: every one resident (the caller names at most residentRings), -> their ids in the order given
    const withRings = (rings, job) => slot.engine.run(() => job(slot.engine, rings.map((r) => residentRing(slot, r, rings))))
    return { engine: slot.engine, withRing, withRings, capacity: () => slot.engine.residentRings || 4 }
}
// ring -> its resident id on the slot's engine: a hit moves it to the back of the LRU order; a miss adds it, dropping the least recently used ring
// first when residentRings are built (never the active one, nor one of `keep`; with a single resident ring that is active, it is rebuilt in place)
function residentRing(slot, ring, keep = []) {
    const e = slot.engine, cap = e.residentRings || 4
    let id = slot.rings.get(ring.tag)
    if (id !== undefined) {
        slot.rings.delete(ring.tag)
        slot.rings.set(ring.tag, id)
        return id
    }
    const busy = new Set(keep.map((r) => r.tag))
    const delta = e.ringDelta !== undefined ? e.ringDelta : facadeRingDelta
    if (delta > 0) {   // opt-in: a resident ring of the same length that differs in a few entries is updated in place and re-tagged (Engine.updateRing)
        for (const [tag, old] of slot.bufs) {
            if (busy.has(tag) || old.length !== ring.buf.length || !slot.rings.has(tag)) continue
            const diff = ringDiff(old, ring.buf, delta)
            if (!diff || !diff.length) continue   // (no difference under another tag cannot be: never re-tag a ring without writing it)
            id = slot.rings.get(tag)
            const fresh = Buffer.from(ring.buf)   // a PRIVATE copy is the record of what is resident: the caller may overwrite its Buffer in place
            try {
                e.updateRing(id, diff, Buffer.concat(diff.map((i) => fresh.subarray(32 * i, 32 * i + 32))), fresh.length / 32)
            } catch (err) {   // a failed update may have dropped the ring (and with it the active ring): the slot forgets it, the next call builds it anew
                let resident = true
                try { e.ringInfo(id) } catch (_) { resident = false }
                if (!resident) {
                    slot.rings.delete(tag), slot.bufs.delete(tag)
                    if (slot.active === tag) slot.active = null
                }
                throw err
            }
            slot.rings.delete(tag), slot.bufs.delete(tag)
            slot.rings.set(ring.tag, id), slot.bufs.set(ring.tag, fresh)
            if (slot.active === tag) slot.active = ring.tag
            return id
        }
    }
    while (slot.rings.size >= cap) {
        const victim = [...slot.rings.keys()].find((t) => t !== slot.active && !busy.has(t))
        if (victim === undefined) break
        e.dropRing(slot.rings.get(victim))
        slot.rings.delete(victim), slot.bufs.delete(victim)
    }
    if (slot.rings.size >= cap && slot.active !== null && !busy.has(slot.active)) {   // only the active ring is left: rebuilt in place under its id
        id = slot.rings.get(slot.active)
        slot.rings.delete(slot.active), slot.bufs.delete(slot.active)
        e.setRing(ring.buf)
        slot.active = ring.tag
    } else {
        id = e.addRing(ring.buf)
    }
    slot.rings.set(ring.tag, id)
    if (delta > 0) slot.bufs.set(ring.tag, Buffer.from(ring.buf))   // a private copy (see above)
    return id
}
// Facade-wide options.  ringDelta (default 0 = off): when a call names a key list that is not resident but has the length of a resident ring of the same
// engine and differs from it in at most `value` 32-byte entries, that ring is updated in place (Engine.updateRing: only the touched keys and blocks are
// rebuilt) and re-tagged, instead of a new ring being built beside it.  An engine's own setOption('ringDelta') overrides it for that engine.
let facadeRingDelta = 0
function setOption(name, value) {
    if (name !== 'ringDelta') throw new RangeError('setOption: unknown option ' + name)
    if (!(Number.isInteger(value) && value >= 0)) throw new RangeError('ringDelta: an integer >= 0')
    facadeRingDelta = value
}
// the 32-byte entries in which two key lists of one length differ (a linear comparison), or null when there are more than `max` of them
function ringDiff(a, b, max) {
    const out = []
    for (let i = 0; 32 * i < a.length; i++)
        if (a.compare(b, 32 * i, 32 * i + 32, 32 * i, 32 * i + 32) !== 0) {
            if (out.length === max) return null
            out.push(i)
        }
    return out
}
function _ringGenerations(params) {   // (tests) ring tag -> build generation of every ring resident on the engine of `params`
    const slot = params._tag0 && engines.get(params._tag0 + (params.hardened ? '|hardened' : ''))
    const out = {}
    if (slot) for (const [tag, id] of slot.rings) out[tag] = slot.engine.ringInfo(id).generation
    return out
}
function shutdown() { for (const s of engines.values()) s.engine.close(); engines.clear() }
// The wire layout of the proofs the reference-shaped calls below PRODUCE: 'zka1' (default; 36-byte Tom coordinates) or 'zka1p' (33-byte, 5.3 % fewer bytes
// to move: include/zkattest.h "packed wire layout"; ZKATTEST_WIRE sets the default).  Verification takes either layout, per proof, whatever this is set
// to; the JSON text of a proof does not depend on it.
let wireLayout = /^zka1p$/i.test(process.env.ZKATTEST_WIRE || '') ? 1 : 0
function setWireLayout(name) {
    if (!/^zka1p?$/i.test(name)) throw new TypeError("wire layout: 'zka1' or 'zka1p'")
    wireLayout = /p$/i.test(name) ? 1 : 0
}
function getWireLayout() { return wireLayout ? 'zka1p' : 'zka1' }
function useWire(slotEngine, wire) {   // inside a queued unit of the engine (nothing of it is in flight)
    if (slotEngine._wire !== wire) { slotEngine.setOption('wire', wire); slotEngine._wire = wire }
}
// The level verifySignatureList verifies a proof at: 'context' (default) = the SecLevel of the params it is called with -- a proof made under
// another SecLevel is 'error deserializing' --, or 'proof' = the proof's own repetition count, as the reference's verifier does
// (src/zkpAttestList.ts:147-184, src/exp/exp.ts:233-262; include/zkattest.h zk_ctx_set_verify_level).  Applies to every engine, cached ones included.
let verifyLevel = 0
function setVerifyLevel(name) {
    if (name !== 'context' && name !== 'proof') throw new TypeError("verify level: 'context' or 'proof'")
    verifyLevel = name === 'proof' ? 1 : 0
}
function getVerifyLevel() { return verifyLevel ? 'proof' : 'context' }
function useVerifyLevel(slotEngine, level) {   // inside a queued unit of the engine (nothing of it is in flight)
    if ((slotEngine._verifyLevel || 0) !== level) { slotEngine.setOption('verifyLevel', level); slotEngine._verifyLevel = level }
}
// The repetitions verifySignatureList checks: 'sample' (default) = the 20 that generateIndices draws, as the reference's verifier does, or 'all' = every
// repetition of the proof (include/zkattest.h zk_ctx_set_verify_reps: stricter than the reference).  Applies to every engine, cached ones included.
let verifyReps = 0
function setVerifyReps(name) {
    if (name !== 'sample' && name !== 'all') throw new TypeError("verify reps: 'sample' or 'all'")
    verifyReps = name === 'all' ? 1 : 0
}
function getVerifyReps() { return verifyReps ? 'all' : 'sample' }
function useVerifyReps(slotEngine, reps) {   // inside a queued unit of the engine (nothing of it is in flight)
    if ((slotEngine._verifyReps || 0) !== reps) { slotEngine.setOption('verifyReps', reps); slotEngine._verifyReps = reps }
}
const isPacked = (b) => Buffer.isBuffer(b) && b.length >= 4 && b.slice(0, 4).toString('latin1') === 'ZK1P'

// ---------------------------------------------------------------- the reference's API
// publicKey: a WebCrypto CryptoKey (where crypto.subtle exists), a Node KeyObject, or the 65-byte 'raw' export 04 || X || Y
async function rawPublicKey(publicKey) {
    if (Buffer.isBuffer(publicKey) || publicKey instanceof Uint8Array) return Buffer.from(publicKey)
    if (publicKey && publicKey.type === 'public' && typeof publicKey.export === 'function') return publicKey.export({ type: 'spki', format: 'der' }).slice(-65)
    const subtle = (crypto.webcrypto && crypto.webcrypto.subtle) || (global.crypto && global.crypto.subtle)
    if (subtle && publicKey && publicKey.algorithm) return Buffer.from(await subtle.exportKey('raw', publicKey))
    throw new Error('invalid public key')
}
function checkedKeyPoint(raw) { // p256.deserializePoint + toAffine (zkpAttestList.ts:95-101, 113-118; weier.ts:74-89)
    if (raw.length !== 65 || raw[0] !== 4) throw new Error('error deserializing uncompressed point')
    const pt = new Point(p256, fromBE(raw.slice(1, 33)), fromBE(raw.slice(33)))
    if (!p256.isOnGroup(pt)) throw new Error('point not in group')
    return new Point(p256, mod(pt.x, p256.p), mod(pt.y, p256.p))
}
async function keyToInt(publicKey) { return checkedKeyPoint(await rawPublicKey(publicKey)).x }

async function proveSignatureList(params, msgHash, sigBytes, publicKey, which, keys) {
    return (await proveSignatureListBatch(params, [msgHash], [sigBytes], [publicKey], [which], keys))[0]
}
async function verifySignatureList(params, msgHash, keys, proof) {
    const r = await verifySignatureListBatch(params, [msgHash], keys, [proof])
    if (r.errors[0]) throw r.errors[0]   // the reference's verifier throws these (src/exp/exp.ts:244,270,302; deserialisation)
    return r[0]
}
// B statements over one ring in one call (what the engine is built for): arrays of the single-proof arguments
async function proveSignatureListBatch(params, msgHashes, sigs, publicKeys, whichs, keys) {
    const raws = await Promise.all(publicKeys.map(rawPublicKey))
    for (const r of raws) if (r.length !== 65 || r[0] !== 4) throw new Error('invalid public key')
    const msg = Buffer.concat(msgHashes.map((m) => Buffer.from(m))), sig = Buffer.concat(sigs.map((s) => Buffer.from(s)))
    checkRingSize(Buffer.isBuffer(keys) ? keys.length / 32 : keys.length, true)
    const wire = wireLayout
    const proofs = await engineFor(params, keys).withRing((engine) => { useWire(engine, wire); return engine._proveNow(msg, sig, Buffer.concat(raws.map((r) => r.slice(1))), whichs) })
    return proofs.map((b) => new SignatureProofList(b))
}
async function verifySignatureListBatch(params, msgHashes, keys, proofs) {
    const msg = Buffer.concat(msgHashes.map((m) => Buffer.from(m))), raw = proofs.map((p) => (p instanceof SignatureProofList ? p.bytes : p))
    checkRingSize(Buffer.isBuffer(keys) ? keys.length / 32 : keys.length, false)
    // a context verifies ONE layout at a time (zk_ctx_set_wire): the batch is split by the proofs' magic and the verdicts are put back in order
    const idx = [[], []]
    raw.forEach((b, i) => idx[isPacked(b) ? 1 : 0].push(i))
    const out = new Array(raw.length), errors = new Array(raw.length)
    for (const wire of [0, 1]) {
        const sel = idx[wire]
        if (!sel.length) continue
        const m = sel.length === raw.length ? msg : Buffer.concat(sel.map((i) => msg.slice(32 * i, 32 * i + 32)))
        const level = verifyLevel, reps = verifyReps
        const r = await engineFor(params, keys).withRing((engine) => { useWire(engine, wire); useVerifyLevel(engine, level); useVerifyReps(engine, reps); return engine._verifyNow(m, sel.map((i) => raw[i])) })
        sel.forEach((i, k) => { out[i] = r[k]; errors[i] = r.errors[k] })
    }
    Object.defineProperty(out, 'errors', { value: errors })
    return out
}
// Re-ring (include/zkattest.h: zk_proof_rering_batch): proofs made for any ring become proofs for `keys` -- after a registry update, for a second registry, for
// a larger ring -- without their signature part being touched: only the GKProof section is made anew, over the same keyXcom.  whichNew[i]: the index of proof
// i's key in `keys`; keyBlinders[i]: the blinder of its keyXcom (keyBlinders below, 32 bytes).  The signature is not needed.  -> SignatureProofList[] in the order
// given, in each proof's own wire layout; throws for the first proof that fails: 'error deserializing', the reference's TypeError for an index past the padded
// ring, or "the index and blinder do not open the proof's key commitment".  The engine draws fresh seeds (crypto.randomBytes).  Two GKProofs over one keyXcom
// tell a verifier who sees both that the key lies in the intersection of the two rings (INTEGRATION.md).
async function reringSignatureLists(params, msgHashes, proofs, whichNew, keyBlinders, keys) {
    const B = msgHashes.length
    if (proofs.length !== B || whichNew.length !== B || keyBlinders.length !== B) throw new RangeError('reringSignatureLists: one proof, one index and one blinder per message hash')
    const raw = proofs.map((p) => (p instanceof SignatureProofList ? p.bytes : p))
    for (const b of raw) if (!wellFormedProof(b)) throw new Error('error deserializing')
    for (const k of keyBlinders) if (!((Buffer.isBuffer(k) || k instanceof Uint8Array) && k.length === 32)) throw new TypeError('a key blinder is a Uint8Array(32)')
    if (isKeyLists(keys)) return reringToLists(params, msgHashes, raw, whichNew, keyBlinders, keys)
    checkRingSize(Buffer.isBuffer(keys) ? keys.length / 32 : keys.length, true)
    const idx = [[], []], out = new Array(B)   // a context works in ONE layout at a time: split by the proofs' magic like the verifier
    raw.forEach((b, i) => idx[isPacked(b) ? 1 : 0].push(i))
    for (const wire of [0, 1]) {
        const sel = idx[wire]
        if (!sel.length) continue
        const msg = Buffer.concat(sel.map((i) => Buffer.from(msgHashes[i]))), bl = Buffer.concat(sel.map((i) => Buffer.from(keyBlinders[i])))
        const r = await engineFor(params, keys).withRing((engine) => { useWire(engine, wire); return engine.reringBatch(msg, sel.map((i) => raw[i]), sel.map((i) => whichNew[i]), bl) })
        sel.forEach((i, k) => { if (r.status[k] !== 0) throw statusError(r.status[k]); out[i] = new SignatureProofList(r.proofs[k]) })
    }
    return out
}
// `keys` of reringSignatureLists as one key list PER PROOF (an array of bigint[] / Buffer, as proveSignatureLists and verifySignatureLists name rings): proof i
// moves to keys[i] and whichNew[i] indexes that list.  The lists are made resident through the same cache (residentRings at a time: a call that names more is
// split by ring) and every layout's proofs of a group go through ONE zk_proof_rering_batch_rings; the active ring is not touched.
const isKeyLists = (keys) => Array.isArray(keys) && keys.length > 0 && (Array.isArray(keys[0]) || Buffer.isBuffer(keys[0]))
async function reringToLists(params, msgHashes, raw, whichNew, keyBlinders, keyLists) {
    const B = raw.length
    if (keyLists.length !== B) throw new RangeError('reringSignatureLists: one key list per proof')
    const rings = [], ringOfProof = new Array(B), byTag = new Map()
    keyLists.forEach((keys, i) => {
        checkRingSize(Buffer.isBuffer(keys) ? keys.length / 32 : keys.length, true)
        const r = ringOf(keys)
        if (!byTag.has(r.tag)) { byTag.set(r.tag, rings.length); rings.push(r) }
        ringOfProof[i] = byTag.get(r.tag)
    })
    const { withRings, capacity } = engineFor(params, keyLists[0])
    const out = new Array(B), per = capacity()
    for (let g = 0; g < rings.length; g += per) {   // groups of at most residentRings rings
        for (const wire of [0, 1]) {
            const sel = []
            raw.forEach((b, i) => { if (ringOfProof[i] >= g && ringOfProof[i] < g + per && (isPacked(b) ? 1 : 0) === wire) sel.push(i) })
            if (!sel.length) continue
            const msg = Buffer.concat(sel.map((i) => Buffer.from(msgHashes[i]))), bl = Buffer.concat(sel.map((i) => Buffer.from(keyBlinders[i])))
            const r = await withRings(rings.slice(g, g + per), (engine, ids) => {
                useWire(engine, wire)
                return engine.reringBatchRings(msg, sel.map((i) => raw[i]), sel.map((i) => whichNew[i]), sel.map((i) => ids[ringOfProof[i] - g]), bl)
            })
            sel.forEach((i, k) => { if (r.status[k] !== 0) throw statusError(r.status[k]); out[i] = new SignatureProofList(r.proofs[k]) })
        }
    }
    return out
}
// The blinders of keyXcom in the proofs made from `seeds` (a Buffer of B x 32 bytes, or an array of 32-byte seeds): what reringSignatureLists needs later.  A
// prover that wants to re-ring keeps its seeds (Engine.proveBatch takes them) or these blinders beside the proofs; they are as secret as the seeds.  -> Buffer[]
async function keyBlinders(seeds, params = lastParams) {
    const buf = Buffer.isBuffer(seeds) ? seeds : Buffer.concat(Array.from(seeds, (s) => Buffer.from(s)))
    if (buf.length % 32) throw new RangeError('keyBlinders: 32 bytes per seed')
    if (!params) throw new Error('keyBlinders: no parameters yet (pass a SystemParametersList)')
    return engineFor(params, null).run((engine) => engine.keyBlinders(buf))
}
// B statements over several rings in one call, proved: keyLists[i] is the ring of proof i and whichs[i] indexes it -- the reference's proveSignatureList takes
// `keys` with every call (src/zkpAttestList.ts:104-145), this is that interface over a batch.  The rings are kept resident through the cache
// verifySignatureLists uses; a call is split only when it names more rings than residentRings, and each part is ONE zk_prove_batch_rings.  -> SignatureProofList[]
// in the order given; throws the reference's error text for the first proof that fails, like proveSignatureListBatch.
async function proveSignatureLists(params, msgHashes, sigs, publicKeys, whichs, keyLists) {
    const B = msgHashes.length
    if (sigs.length !== B || publicKeys.length !== B || whichs.length !== B || keyLists.length !== B)
        throw new RangeError('proveSignatureLists: one signature, one public key, one index and one key list per message hash')
    const raws = await Promise.all(publicKeys.map(rawPublicKey))
    for (const r of raws) if (r.length !== 65 || r[0] !== 4) throw new Error('invalid public key')
    const rings = [], ringOfProof = new Array(B), byTag = new Map()
    keyLists.forEach((keys, i) => {
        checkRingSize(Buffer.isBuffer(keys) ? keys.length / 32 : keys.length, true)
        const r = ringOf(keys)
        if (!byTag.has(r.tag)) { byTag.set(r.tag, rings.length); rings.push(r) }
        ringOfProof[i] = byTag.get(r.tag)
    })
    if (!B) return []
    const { withRings, capacity } = engineFor(params, keyLists[0])
    const out = new Array(B), wire = wireLayout, per = capacity()
    for (let g = 0; g < rings.length; g += per) {   // groups of at most residentRings rings: one group unless the call names more
        const sel = []
        for (let i = 0; i < B; i++) if (ringOfProof[i] >= g && ringOfProof[i] < g + per) sel.push(i)
        const cat = (f) => Buffer.concat(sel.map(f))
        const proofs = await withRings(rings.slice(g, g + per), (engine, ids) => {
            useWire(engine, wire)
            return engine._proveRingsNow(cat((i) => Buffer.from(msgHashes[i])), cat((i) => Buffer.from(sigs[i])), cat((i) => raws[i].slice(1)), sel.map((i) => whichs[i]),
                sel.map((i) => ids[ringOfProof[i] - g]))
        })
        sel.forEach((i, k) => { out[i] = new SignatureProofList(proofs[k]) })
    }
    return out
}
// B statements over several rings in one call: keyLists[i] is the ring of proof i.  The rings are made resident on the params' engine (residentRings at a
// time: a call that names more rings than that is split by ring) and every wire layout's proofs go through ONE zk_verify_batch_rings.  -> booleans with
// .errors, like verifySignatureListBatch.
async function verifySignatureLists(params, msgHashes, keyLists, proofs) {
    if (keyLists.length !== proofs.length || msgHashes.length !== proofs.length) throw new RangeError('verifySignatureLists: one message hash and one key list per proof')
    const raw = proofs.map((p) => (p instanceof SignatureProofList ? p.bytes : p))
    const rings = [], ringOfProof = new Array(raw.length), byTag = new Map()
    keyLists.forEach((keys, i) => {
        checkRingSize(Buffer.isBuffer(keys) ? keys.length / 32 : keys.length, false)
        const r = ringOf(keys)
        if (!byTag.has(r.tag)) { byTag.set(r.tag, rings.length); rings.push(r) }
        ringOfProof[i] = byTag.get(r.tag)
    })
    const { withRings, capacity } = engineFor(params, keyLists[0] || [])
    const out = new Array(raw.length), errors = new Array(raw.length), level = verifyLevel, reps = verifyReps
    const per = capacity()
    for (let g = 0; g < rings.length; g += per) {   // groups of at most residentRings rings
        const group = rings.slice(g, g + per)
        for (const wire of [0, 1]) {
            const sel = []
            raw.forEach((b, i) => { if (ringOfProof[i] >= g && ringOfProof[i] < g + per && (isPacked(b) ? 1 : 0) === wire) sel.push(i) })
            if (!sel.length) continue
            const m = Buffer.concat(sel.map((i) => Buffer.from(msgHashes[i])))
            const r = await withRings(group, (engine, ids) => {
                useWire(engine, wire)
                useVerifyLevel(engine, level)
                useVerifyReps(engine, reps)
                return engine._verifyRingsNow(m, sel.map((i) => raw[i]), sel.map((i) => ids[ringOfProof[i] - g]))
            })
            sel.forEach((i, k) => { out[i] = r[k]; errors[i] = r.errors[k] })
        }
    }
    Object.defineProperty(out, 'errors', { value: errors })
    return out
}

// The witness screen (include/zkattest.h: zk_screen_batch_rings) behind the facade: before paying for proofs, ask for each statement { msgHash, sigBytes, publicKey,
// keys, which? } where the signer's key stands in `keys` and whether the ECDSA signature verifies.  `which` given: that index is checked; absent: the lowest index of
// the key among `keys` is found (WHICH_NONE when it is not there).  -> [{ which, flags, ok }] in the order given; flags is a set of SCREEN bits and ok = (flags === 0)
// means that proveSignatureList with that `which` gives a proof that verifies.  SCREEN.SIG_RANGE is stricter than the prover, which reduces r and s mod n
// (src/zkpAttestList.ts:119-127).  An unusable public key is flagged, not thrown.  Uses the engine and the resident rings of the prove / verify calls.
const SCREEN = Object.freeze({ KEY_NOT_ON_CURVE: 1, SIG_RANGE: 2, SIG_INVALID: 4, NOT_IN_RING: 8, RING_NOT_RESIDENT: 16 })
const WHICH_NONE = 0xFFFFFFFF
async function screenSignatureLists(params, statements) {
    const B = statements.length
    if (!B) return []
    const raws = await Promise.all(statements.map((s) => rawPublicKey(s.publicKey)))
    for (const r of raws) if (r.length !== 65 || r[0] !== 4) throw new Error('invalid public key')
    const check = statements[0].which !== undefined && statements[0].which !== null
    if (statements.some((s) => (s.which !== undefined && s.which !== null) !== check)) throw new RangeError('screenSignatureLists: `which` in every statement or in none')
    const rings = [], ringOfSt = new Array(B), byTag = new Map()
    statements.forEach((s, i) => {
        checkRingSize(Buffer.isBuffer(s.keys) ? s.keys.length / 32 : s.keys.length, true)
        const r = ringOf(s.keys)
        if (!byTag.has(r.tag)) { byTag.set(r.tag, rings.length); rings.push(r) }
        ringOfSt[i] = byTag.get(r.tag)
    })
    const { withRings, capacity } = engineFor(params, statements[0].keys)
    const out = new Array(B), per = capacity()
    for (let g = 0; g < rings.length; g += per) {   // groups of at most residentRings rings: one group unless the call names more
        const sel = []
        for (let i = 0; i < B; i++) if (ringOfSt[i] >= g && ringOfSt[i] < g + per) sel.push(i)
        const cat = (f) => Buffer.concat(sel.map(f))
        const r = await withRings(rings.slice(g, g + per), (engine, ids) =>
            engine.screenBatchRings(cat((i) => Buffer.from(statements[i].msgHash)), cat((i) => Buffer.from(statements[i].sigBytes)), cat((i) => raws[i].slice(1)),
                check ? sel.map((i) => statements[i].which) : null, sel.map((i) => ids[ringOfSt[i] - g])))
        sel.forEach((i, k) => { out[i] = { which: r.which[k], flags: r.flags[k], ok: r.flags[k] === 0 } })
    }
    return out
}
// Key recovery (include/zkattest.h: zk_recover_batch_rings) behind the facade: from { msgHash, sigBytes, keys } alone -- no public key -- the signer's key and
// where it stands in `keys`.  -> [{ publicKey, which, flags }] in the order given: flags is a set of RECOVER bits; with flags === 0 publicKey is the raw 65-byte
// uncompressed point (0x04 || x || y) and which its lowest index; otherwise publicKey is null and which WHICH_NONE.  proveSignatureList(s) takes that raw
// point as its publicKey as it is (rawPublicKey accepts a Buffer); a caller that wants a CryptoKey imports it:
//   crypto.webcrypto.subtle.importKey('raw', publicKey, { name: 'ECDSA', namedCurve: 'P-256' }, true, ['verify']).
// Uses the engine and the resident rings of the prove / verify / screen calls.  The reference has no counterpart (src/zkpAttestList.ts:104-118 takes the key).
const RECOVER = Object.freeze({ SIG_RANGE: 2, NOT_IN_RING: 8, RING_NOT_RESIDENT: 16, NO_POINT: 32 })
async function recoverSignatureLists(params, statements) {
    const B = statements.length
    if (!B) return []
    const rings = [], ringOfSt = new Array(B), byTag = new Map()
    statements.forEach((s, i) => {
        checkRingSize(Buffer.isBuffer(s.keys) ? s.keys.length / 32 : s.keys.length, true)
        const r = ringOf(s.keys)
        if (!byTag.has(r.tag)) { byTag.set(r.tag, rings.length); rings.push(r) }
        ringOfSt[i] = byTag.get(r.tag)
    })
    const { withRings, capacity } = engineFor(params, statements[0].keys)
    const out = new Array(B), per = capacity()
    for (let g = 0; g < rings.length; g += per) {   // groups of at most residentRings rings: one group unless the call names more
        const sel = []
        for (let i = 0; i < B; i++) if (ringOfSt[i] >= g && ringOfSt[i] < g + per) sel.push(i)
        const cat = (f) => Buffer.concat(sel.map(f))
        const r = await withRings(rings.slice(g, g + per), (engine, ids) =>
            engine.recoverBatchRings(cat((i) => Buffer.from(statements[i].msgHash)), cat((i) => Buffer.from(statements[i].sigBytes)), sel.map((i) => ids[ringOfSt[i] - g])))
        sel.forEach((i, k) => {
            const ok = r.flags[k] === 0
            out[i] = { publicKey: ok ? Buffer.concat([Buffer.from([4]), r.pk.slice(64 * k, 64 * k + 64)]) : null, which: r.which[k], flags: r.flags[k] }
        })
    }
    return out
}
// the one-statement form
async function recoverKey(msgHash, sigBytes, keys, params = lastParams) {
    if (!params) throw new Error('recoverKey: no params given and none used yet')
    return (await recoverSignatureLists(params, [{ msgHash, sigBytes, keys }]))[0]
}
// the lookup alone: the lowest index of publicKey's x-coordinate among keys, or -1 (the engine compares integers: a key off the curve is looked up like any
// other).  The ring lives on the engine of a SystemParametersList: `params`, or by default the one the facade used last.
let lastParams = null
async function findKey(publicKey, keys, params = lastParams) {
    if (!params) throw new Error('findKey: no params given and none used yet')
    const r = (await screenSignatureLists(params, [{ msgHash: Buffer.alloc(32), sigBytes: Buffer.alloc(64), publicKey, keys }]))[0]
    return r.flags & SCREEN.NOT_IN_RING ? -1 : r.which
}

// ---------------------------------------------------------------- ring membership on its own (src/proofGK/gk.ts:31-262, src/commit/pedersen.ts:21-58)
class Commitment { // src/commit/pedersen.ts:21-36: the point and its blinder
    constructor(p, r) { this.p = p; this.r = r }
}
// A GKProof keeps the engine's ZKM1 bytes (include/zkattest.h; "ZKMB" for a proof made with a context: `bound`) and materialises the reference's members (cl, ca, cb, cd: Points; f, za, zb: Scalars; zd) on demand.
class GKProof { // src/proofGK/gk.ts:31-73
    constructor(bytes) {
        if (!(Buffer.isBuffer(bytes) && bytes.length >= 16 && ['ZKM1', 'ZKMB'].includes(bytes.slice(0, 4).toString('latin1')) && bytes.readUInt32BE(4) === bytes.length &&
            bytes.length === 16 + 384 * bytes.readUInt32BE(8) + 32)) throw new Error('error deserializing GKProof')
        this.bytes = bytes
    }
    get n() { return this.bytes.readUInt32BE(8) }
    get bound() { return this.bytes[3] === 0x42 }   // "ZKMB": verifies only with the context, the commitment and the ring it was made with
    _pts(k) { const n = this.n; return Array.from({ length: n }, (_, i) => { const o = 16 + 72 * (k * n + i); return new Point(tomEdwards256, fromBE(this.bytes.slice(o, o + 36)), fromBE(this.bytes.slice(o + 36, o + 72))) }) }
    _scs(k) { const n = this.n; return Array.from({ length: n }, (_, i) => { const o = 16 + 288 * n + 32 * (k * n + i); return new Scalar(tomEdwards256, fromBE(this.bytes.slice(o, o + 32))) }) }
    get cl() { return this._pts(0) }
    get ca() { return this._pts(1) }
    get cb() { return this._pts(2) }
    get cd() { return this._pts(3) }
    get f() { return this._scs(0) }
    get za() { return this._scs(1) }
    get zb() { return this._scs(2) }
    get zd() { const o = this.bytes.length - 32; return new Scalar(tomEdwards256, fromBE(this.bytes.slice(o))) }
    eq(o) { return o instanceof GKProof && this.bytes.equals(o.bytes) }
}
// pedersen.ts:53-58 -- commit(value): a fresh blinder from crypto.getRandomValues (a one-time host call, like generateParamsList)
function commit(pedersenParams, value) {
    const c = pedersenParams.c, r = c.randomScalar(), v = new Scalar(c, value)
    return new Commitment(pedersenParams.h.mul(r).add(pedersenParams.g.mul(v)), r)
}
// The engine holds whole parameter sets: a bare Tom-256 PedersenParams rides in a SystemParametersList whose P-256 half plays no part in these calls.
const memberParams = new WeakMap()
function paramsOf(pedersenParams) {
    if (pedersenParams instanceof SystemParametersList) return pedersenParams
    if (!(pedersenParams instanceof PedersenParams) || !pedersenParams.c.eq(tomEdwards256)) throw new TypeError('params: PedersenParams on tomEdwards256')
    let sp = memberParams.get(pedersenParams)
    if (!sp) {
        sp = new SystemParametersList(new PedersenParams(p256, p256.generator(), p256.generator()), pedersenParams, 80)
        memberParams.set(pedersenParams, sp)
    }
    return sp
}
const tomBytes = (pt) => Buffer.concat([toBE(pt.x, 36), toBE(pt.y, 36)])
// Bound proofs ("ZKMB", include/zkattest.h: zk_member_*_bound): every call below takes one more argument than the reference's list, `options`, and
// options.context binds the proof -- 32 bytes of the caller's (a session nonce, a message hash, a verifier's id) that the challenge hashes together with the
// ring's digest and the commitment.  The single calls take one Uint8Array(32), the batched and Lists calls an array of them, one per entry.  The same context
// must be given to the verifier; a proof made without one does not deserialise there, and a bound proof does not deserialise in a call without one.
// The declared parameter lists stay the reference's (Function.length and the call shape are what callers of gk.ts know): the fifth argument is read here.
function memberContexts(args, at, B, name) {
    const options = args[at]
    if (options === undefined || options === null || options.context === undefined || options.context === null) return null
    const list = B === null ? [options.context] : options.context
    if (!Array.isArray(list) || list.length !== (B === null ? 1 : B)) throw new RangeError(name + ': options.context holds one Uint8Array(32) per entry')
    list.forEach((c) => { if (!(c instanceof Uint8Array) || c.length !== 32) throw new TypeError(name + ': a context is a Uint8Array(32)') })
    return list.map((c) => Buffer.from(c.buffer, c.byteOffset, 32))
}
// proveMembership(params, com, index, keys) (gk.ts:94-195): com.r is the blinder; the engine's commitment to keys[index] under it must be com.p
async function proveMembership(pedersenParams, com, index, keys) {   // (+ options: { context: Uint8Array(32) })
    const ctx = memberContexts(arguments, 4, null, 'proveMembership')
    return (await proveMemberships(pedersenParams, [com], [index], keys, ctx ? { context: ctx } : undefined))[0]
}
// verifyMembership(params, comPoint, keys, proof) (gk.ts:197-262) -> boolean; what does not deserialise throws
async function verifyMembership(pedersenParams, comPoint, keys, proof) {   // (+ options: { context: Uint8Array(32) })
    const ctx = memberContexts(arguments, 4, null, 'verifyMembership')
    return (await verifyMemberships(pedersenParams, [comPoint], keys, [proof], ctx ? { context: ctx } : undefined))[0]
}
// batched: one ring, B commitments and indices -> GKProof[]
async function proveMemberships(pedersenParams, coms, indices, keys) {
    if (coms.length !== indices.length) throw new RangeError('proveMemberships: one index per commitment')
    const ctx = memberContexts(arguments, 4, coms.length, 'proveMemberships')   // (+ options: { context: Uint8Array(32)[] })
    checkRingSize(Buffer.isBuffer(keys) ? keys.length / 32 : keys.length, true)
    if (!coms.length) return []
    const { withRing } = engineFor(paramsOf(pedersenParams), keys)
    const r = await withRing((engine) => engine.memberProveBatch(indices, Buffer.concat(coms.map((c) => toBE(c.r.k, 32))), null, ctx && Buffer.concat(ctx)))
    return r.proofs.map((p, i) => {
        if (r.status[i] !== 0) throw statusError(r.status[i])
        if (!r.coms[i].equals(tomBytes(coms[i].p))) throw new Error('proveMembership: com does not commit to keys[index] with blinder com.r')
        return new GKProof(p)
    })
}
async function verifyMemberships(pedersenParams, comPoints, keys, proofs) {
    if (comPoints.length !== proofs.length) throw new RangeError('verifyMemberships: one proof per commitment')
    const ctx = memberContexts(arguments, 4, proofs.length, 'verifyMemberships')   // (+ options: { context: Uint8Array(32)[] })
    checkRingSize(Buffer.isBuffer(keys) ? keys.length / 32 : keys.length, false)
    if (!proofs.length) return []
    const { withRing } = engineFor(paramsOf(pedersenParams), keys)
    return withRing((engine) => {
        const size = engine.memberProofSize()
        // a GKProof of another ring's length: the reference's length check returns false (gk.ts:208-218); the engine sees fixed-size slots
        const fit = proofs.map((p) => { const b = p.bytes; return b.length === size ? b : b.length > size ? b.slice(0, size) : Buffer.concat([b, Buffer.alloc(size - b.length)]) })
        const r = engine.memberVerifyBatch(comPoints.map(tomBytes), fit, ctx && Buffer.concat(ctx))
        r.status.forEach((st) => { if (st !== 0) throw statusError(st) })
        return r.ok
    })
}
// One key list per entry: keysList[i] is the ring of commitment i and indices[i] indexes it -- the reference takes `keys` with every proveMembership /
// verifyMembership call, this is that interface over a batch.  The key lists are resolved to resident rings the way proveSignatureLists / verifySignatureLists
// resolve theirs; a call is split only when it names more rings than residentRings, and each part is ONE zk_member_prove_batch_rings /
// zk_member_verify_batch_rings.  -> GKProof[] / boolean[] in the order given.
function memberRingsOf(keysList, prove) {
    const rings = [], ringOf_ = new Array(keysList.length), byTag = new Map()
    keysList.forEach((keys, i) => {
        checkRingSize(Buffer.isBuffer(keys) ? keys.length / 32 : keys.length, prove)
        const r = ringOf(keys)
        if (!byTag.has(r.tag)) { byTag.set(r.tag, rings.length); rings.push(r) }
        ringOf_[i] = byTag.get(r.tag)
    })
    return { rings, ringOfEntry: ringOf_ }
}
async function proveMembershipLists(pedersenParams, coms, indices, keysList) {
    const B = coms.length
    if (indices.length !== B || keysList.length !== B) throw new RangeError('proveMembershipLists: one index and one key list per commitment')
    const ctx = memberContexts(arguments, 4, B, 'proveMembershipLists')   // (+ options: { context: Uint8Array(32)[] }: entry i's proof hashes ITS ring's digest and context[i])
    const { rings, ringOfEntry } = memberRingsOf(keysList, true)
    if (!B) return []
    const { withRings, capacity } = engineFor(paramsOf(pedersenParams), keysList[0])
    const out = new Array(B), per = capacity()
    for (let g = 0; g < rings.length; g += per) {   // groups of at most residentRings rings: one group unless the call names more
        const sel = []
        for (let i = 0; i < B; i++) if (ringOfEntry[i] >= g && ringOfEntry[i] < g + per) sel.push(i)
        const r = await withRings(rings.slice(g, g + per), (engine, ids) =>
            engine.memberProveBatchRings(sel.map((i) => indices[i]), sel.map((i) => ids[ringOfEntry[i] - g]), Buffer.concat(sel.map((i) => toBE(coms[i].r.k, 32))), null,
                ctx && Buffer.concat(sel.map((i) => ctx[i]))))
        sel.forEach((i, k) => {
            if (r.status[k] !== 0) throw statusError(r.status[k])
            if (!r.coms[k].equals(tomBytes(coms[i].p))) throw new Error('proveMembership: com does not commit to keys[index] with blinder com.r')
            out[i] = new GKProof(r.proofs[k])
        })
    }
    return out
}
async function verifyMembershipLists(pedersenParams, comPoints, keysList, proofs) {
    const B = proofs.length
    if (comPoints.length !== B || keysList.length !== B) throw new RangeError('verifyMembershipLists: one commitment and one key list per proof')
    const ctx = memberContexts(arguments, 4, B, 'verifyMembershipLists')   // (+ options: { context: Uint8Array(32)[] })
    const { rings, ringOfEntry } = memberRingsOf(keysList, false)
    if (!B) return []
    const { withRings, capacity } = engineFor(paramsOf(pedersenParams), keysList[0])
    const out = new Array(B), per = capacity()
    for (let g = 0; g < rings.length; g += per) {
        const sel = []
        for (let i = 0; i < B; i++) if (ringOfEntry[i] >= g && ringOfEntry[i] < g + per) sel.push(i)
        const r = await withRings(rings.slice(g, g + per), (engine, ids) => {
            const rid = sel.map((i) => ids[ringOfEntry[i] - g])
            // a GKProof of another ring's length: the reference's length check returns false (gk.ts:208-218); the engine sees slots of the ring's size
            const fit = sel.map((i, k) => { const b = proofs[i].bytes, size = engine.memberProofSizeRing(rid[k]); return b.length === size ? b : b.length > size ? b.slice(0, size) : Buffer.concat([b, Buffer.alloc(size - b.length)]) })
            return engine.memberVerifyBatchRings(sel.map((i) => tomBytes(comPoints[i])), fit, rid, ctx && Buffer.concat(sel.map((i) => ctx[i])))
        })
        sel.forEach((i, k) => {
            if (r.status[k] !== 0) throw statusError(r.status[k])
            out[i] = r.ok[k]
        })
    }
    return out
}

// ---------------------------------------------------------------- link proofs: two key commitments hide the same key (src/commit/equality.ts:27-116)
// A LinkProof keeps the engine's ZKL1 bytes (include/zkattest.h) and materialises the reference's EqualityProof members (A_1, A_2: Points; t_x, t_r1, t_r2: Scalars).
class LinkProof {
    constructor(bytes) {
        if (!(Buffer.isBuffer(bytes) && bytes.length === 256 && bytes.slice(0, 4).toString('latin1') === 'ZKL1' && bytes.readUInt32BE(4) === 256 && bytes.readUInt32BE(8) === 0 &&
            bytes.readUInt32BE(12) === 0)) throw new Error('error deserializing LinkProof')
        this.bytes = bytes
    }
    _pt(o) { return new Point(tomEdwards256, fromBE(this.bytes.slice(o, o + 36)), fromBE(this.bytes.slice(o + 36, o + 72))) }
    _sc(o) { return new Scalar(tomEdwards256, fromBE(this.bytes.slice(o, o + 32))) }
    get A_1() { return this._pt(16) }
    get A_2() { return this._pt(88) }
    get t_x() { return this._sc(160) }
    get t_r1() { return this._sc(192) }
    get t_r2() { return this._sc(224) }
    eq(o) { return o instanceof LinkProof && this.bytes.equals(o.bytes) }
}
const scalarBytes = (v) => (v instanceof Scalar ? toBE(v.k, 32) : (Buffer.isBuffer(v) || v instanceof Uint8Array) ? Buffer.from(v) : toBE(mod(BigInt(v), tomEdwards256.order), 32))
const comBytes = (c) => (Buffer.isBuffer(c) ? c : tomBytes(c instanceof Commitment ? c.p : c))
// proveSameKey(params, key, comA, blinderA, comB, blinderB): comA = key g + blinderA h and comB = key g + blinderB h (Points, Commitments or 72-byte Buffers; the
// key a bigint, the blinders Scalars, bigints or 32-byte Buffers -- keyBlinders gives a keyXcom's) -> LinkProof.  The engine draws fresh seeds.  A link proof
// deliberately makes the two proofs linkable to anyone who sees it.  Throws 'error deserializing' for a commitment off the curve and "... do not open ..." when the
// key and a blinder do not open a commitment.
async function proveSameKey(params, key, comA, blinderA, comB, blinderB) {
    return (await proveSameKeys(params, [key], [comA], [blinderA], [comB], [blinderB]))[0]
}
async function verifySameKey(params, comA, comB, link) {   // -> boolean; what does not deserialise throws
    return (await verifySameKeys(params, [comA], [comB], [link]))[0]
}
// batched: arrays of equal length
async function proveSameKeys(params, keys, comsA, blindersA, comsB, blindersB) {
    const B = keys.length
    if ([comsA, blindersA, comsB, blindersB].some((a) => a.length !== B)) throw new RangeError('proveSameKeys: one key, two commitments and two blinders per entry')
    if (!B) return []
    const r = await engineFor(paramsOf(params), null).run((engine) => engine.linkProveBatch(keys.map(scalarBytes), comsA.map(comBytes), blindersA.map(scalarBytes), comsB.map(comBytes),
        blindersB.map(scalarBytes)))
    return r.proofs.map((p, i) => { if (r.status[i] !== 0) throw statusError(r.status[i]); return new LinkProof(p) })
}
async function verifySameKeys(params, comsA, comsB, links) {
    const B = links.length
    if (comsA.length !== B || comsB.length !== B) throw new RangeError('verifySameKeys: two commitments per link proof')
    if (!B) return []
    const r = await engineFor(paramsOf(params), null).run((engine) => engine.linkVerifyBatch(comsA.map(comBytes), comsB.map(comBytes), links.map((l) => (l instanceof LinkProof ? l.bytes : new LinkProof(l).bytes))))
    r.status.forEach((st) => { if (st !== 0) throw statusError(st) })
    return r.ok
}
// keyXcom of a proof (a SignatureProofList or its bytes, either wire layout) as a Point: what takes a verifier from two attestations to verifySameKey
async function keyCommitment(proof, params = lastParams) { return (await keyCommitments([proof], params))[0] }
async function keyCommitments(proofs, params = lastParams) {
    if (!params) throw new Error('keyCommitment: no parameters yet (pass a SystemParametersList)')
    const raw = proofs.map((p) => (p instanceof SignatureProofList ? p.bytes : p)), out = new Array(raw.length)
    for (const b of raw) if (!wellFormedProof(b)) throw new Error('error deserializing')
    for (const wire of [0, 1]) {   // a context works in ONE layout at a time
        const sel = []
        raw.forEach((b, i) => { if ((isPacked(b) ? 1 : 0) === wire) sel.push(i) })
        if (!sel.length) continue
        const r = await engineFor(params, null).run((engine) => { useWire(engine, wire); return engine.keyCommitments(sel.map((i) => raw[i])) })
        sel.forEach((i, k) => { if (r.status[k] !== 0) throw statusError(r.status[k]); out[i] = new Point(tomEdwards256, fromBE(r.coms[k].slice(0, 36)), fromBE(r.coms[k].slice(36))) })
    }
    return out
}

// ---------------------------------------------------------------- escrow tags: an auditor can open which ring member attested (include/zkattest.h: zk_escrow_*)
// An EscrowTag keeps the engine's ZKT1 bytes and materialises its members (E1, E2, T1, T2, T3: Points; t_x, t_r, t_rho: Scalars).
class EscrowTag {
    constructor(bytes) {
        if (!(Buffer.isBuffer(bytes) && bytes.length === 472 && bytes.slice(0, 4).toString('latin1') === 'ZKT1' && bytes.readUInt32BE(4) === 472 && bytes.readUInt32BE(8) === 0 &&
            bytes.readUInt32BE(12) === 0)) throw new Error('error deserializing EscrowTag')
        this.bytes = bytes
    }
    _pt(o) { return new Point(tomEdwards256, fromBE(this.bytes.slice(o, o + 36)), fromBE(this.bytes.slice(o + 36, o + 72))) }
    _sc(o) { return new Scalar(tomEdwards256, fromBE(this.bytes.slice(o, o + 32))) }
    get E1() { return this._pt(16) }
    get E2() { return this._pt(88) }
    get T1() { return this._pt(160) }
    get T2() { return this._pt(232) }
    get T3() { return this._pt(304) }
    get t_x() { return this._sc(376) }
    get t_r() { return this._sc(408) }
    get t_rho() { return this._sc(440) }
    eq(o) { return o instanceof EscrowTag && this.bytes.equals(o.bytes) }
}
// inside a queued unit of the engine: the auditor's key of this call (a Point or 72 bytes) is the one the engine holds -- its comb table is built once per key
function useAuditor(engine, auditor) {
    const key = comBytes(auditor)
    if (engine.auditor !== key.toString('hex')) engine.setAuditor(key)
}
// escrowAuditorKey(params, secret): the auditor's public key A = a g (a Point) for a secret a (a bigint, a Scalar or 32 bytes).  Keep a where the court order is kept:
// anyone who knows it opens every tag made for A.
async function escrowAuditorKey(params, secret) {
    const k = await engineFor(paramsOf(params), null).run((engine) => engine.escrowKeygen(scalarBytes(secret)))
    return new Point(tomEdwards256, fromBE(k.slice(0, 36)), fromBE(k.slice(36)))
}
// proveEscrowTag(params, auditor, key, com, blinder): com = key g + blinder h (a Point, a Commitment or 72 bytes; keyXcom of an attestation with keyBlinders' blinder,
// or a membership commitment) -> EscrowTag: the key encrypted to the auditor's key, tied to com.  The engine draws fresh seeds.  The tag is bound to com and the
// auditor's key, not to a message or a ring.  Throws 'error deserializing' for a commitment off the curve and "... do not open ..." when key and blinder do not open com.
async function proveEscrowTag(params, auditor, key, com, blinder) {
    return (await proveEscrowTags(params, auditor, [key], [com], [blinder]))[0]
}
async function verifyEscrowTag(params, auditor, com, tag) {   // -> boolean; what does not deserialise throws
    return (await verifyEscrowTags(params, auditor, [com], [tag]))[0]
}
async function proveEscrowTags(params, auditor, keys, coms, blinders) {
    const B = keys.length
    if (coms.length !== B || blinders.length !== B) throw new RangeError('proveEscrowTags: one key, one commitment and one blinder per entry')
    if (!B) return []
    const r = await engineFor(paramsOf(params), null).run((engine) => { useAuditor(engine, auditor); return engine.escrowProveBatch(keys.map(scalarBytes), coms.map(comBytes), blinders.map(scalarBytes)) })
    return r.tags.map((t, i) => { if (r.status[i] !== 0) throw statusError(r.status[i]); return new EscrowTag(t) })
}
async function verifyEscrowTags(params, auditor, coms, tags) {
    const B = tags.length
    if (coms.length !== B) throw new RangeError('verifyEscrowTags: one commitment per tag')
    if (!B) return []
    const raw = tags.map((t) => (t instanceof EscrowTag ? t.bytes : new EscrowTag(t).bytes))
    const r = await engineFor(paramsOf(params), null).run((engine) => { useAuditor(engine, auditor); return engine.escrowVerifyBatch(coms.map(comBytes), raw) })
    r.status.forEach((st) => { if (st !== 0) throw statusError(st) })
    return r.ok
}
// openEscrowTags(params, secret, keys, tags): the auditor's call -> per tag the index in `keys` of the ring member whose key it carries (the lowest, where a key
// occurs twice) or null for nobody.  It does NOT verify: call verifyEscrowTag (and the attestation's verifier) first.  Throws when the secret is 0 mod q.
// With one key list per tag in the place of `keys` (the convention of reringSignatureLists) the tags of a sharded registry open in one zk_rings_escrow_open_batch
// per group of at most residentRings rings, through the rings' resident point indexes: -> per tag { ring, index } -- ring counts the distinct key lists in the
// order of their first appearance, index is the member's index in that list -- or null for nobody.
async function openEscrowTags(params, secret, keys, tags) {
    if (!tags.length) return []
    const raw = tags.map((t) => (t instanceof EscrowTag ? t.bytes : new EscrowTag(t).bytes)), a = scalarBytes(secret)
    if (isKeyLists(keys)) {
        if (keys.length !== tags.length) throw new RangeError('openEscrowTags: one key list per tag')
        const { rings, ringOfEntry } = memberRingsOf(keys, false)
        const { withRings, capacity } = engineFor(paramsOf(params), keys[0])
        const out = new Array(tags.length), per = capacity()
        for (let g = 0; g < rings.length; g += per) {
            const sel = []
            for (let i = 0; i < tags.length; i++) if (ringOfEntry[i] >= g && ringOfEntry[i] < g + per) sel.push(i)
            const r = await withRings(rings.slice(g, g + per), (engine, ids) => {
                useAuditor(engine, engine.escrowKeygen(a))
                return engine.ringsEscrowOpenBatch(a, sel.map((i) => raw[i]), sel.map((i) => ids[ringOfEntry[i] - g]))
            })
            sel.forEach((i, k) => {
                if (r.status[k] !== 0) throw statusError(r.status[k])
                out[i] = r.index[k] === 0xffffffff ? null : { ring: ringOfEntry[i], index: r.index[k] }
            })
        }
        return out
    }
    const r = await engineFor(paramsOf(params), keys).withRing((engine) => { useAuditor(engine, engine.escrowKeygen(a)); return engine.escrowOpenBatch(a, raw) })
    return r.index.map((w, i) => { if (r.status[i] !== 0) throw statusError(r.status[i]); return w === 0xffffffff ? null : w })
}

// ---------------------------------------------------------------- threshold opening: t of n auditors open a tag (include/zkattest.h: zk_auditors_*)
// An EscrowShare keeps the engine's ZKS1 bytes and materialises its members (j: the auditor's index; D, U1, U2: Points; s: a Scalar).
class EscrowShare {
    constructor(bytes) {
        if (!(Buffer.isBuffer(bytes) && bytes.length === 264 && bytes.slice(0, 4).toString('latin1') === 'ZKS1' && bytes.readUInt32BE(4) === 264 && bytes.readUInt32BE(12) === 0))
            throw new Error('error deserializing EscrowShare')
        this.bytes = bytes
    }
    _pt(o) { return new Point(tomEdwards256, fromBE(this.bytes.slice(o, o + 36)), fromBE(this.bytes.slice(o + 36, o + 72))) }
    get j() { return this.bytes.readUInt32BE(8) }
    get D() { return this._pt(16) }
    get U1() { return this._pt(88) }
    get U2() { return this._pt(160) }
    get s() { return new Scalar(tomEdwards256, fromBE(this.bytes.slice(232, 264))) }
    eq(o) { return o instanceof EscrowShare && this.bytes.equals(o.bytes) }
}
// `auditors` names a t-of-n set in every call below: { key: the auditor's key A, t, keys: the share keys A_1 .. A_n } (Points or 72 bytes).  Inside a queued
// unit of the engine: the set is the one the engine holds -- it is checked against A once per set
function useAuditors(engine, auditors) {
    useAuditor(engine, auditors.key)
    const keys = auditors.keys.map(comBytes)
    if (engine.auditors !== auditors.t + ':' + keys.map((k) => k.toString('hex')).join('')) engine.auditorsSetKeys(auditors.t, keys)
}
const shareBytes = (s) => (s instanceof EscrowShare ? s.bytes : new EscrowShare(s).bytes)
const tagBytes = (t) => (t instanceof EscrowTag ? t.bytes : new EscrowTag(t).bytes)
// splitAuditorKey(params, secret, t, n): the dealer's Shamir split of the auditor's secret -> { key: A (a Point), t, keys: A_1 .. A_n (Points), shares: a_1 .. a_n
// (32-byte Buffers, one per auditor) }; the first three members are the `auditors` of the other calls.  The dealer sees the secret: run it where that is acceptable.
async function splitAuditorKey(params, secret, t, n) {
    const a = scalarBytes(secret)
    const r = await engineFor(paramsOf(params), null).run((engine) => ({ key: engine.escrowKeygen(a), split: engine.auditorsSplitKey(a, t, n) }))
    const pt = (k) => new Point(tomEdwards256, fromBE(k.slice(0, 36)), fromBE(k.slice(36)))
    return { key: pt(r.key), t, keys: r.split.keys.map(pt), shares: r.split.shares }
}
// shareEscrowTags(params, auditors, j, shareSecret, tags): auditor j's shares of the tags -> EscrowShare[].  Throws when the share secret is not A_j's.
async function shareEscrowTags(params, auditors, j, shareSecret, tags) {
    if (!tags.length) return []
    const raw = tags.map(tagBytes)
    const r = await engineFor(paramsOf(params), null).run((engine) => { useAuditors(engine, auditors); return engine.auditorsShareBatch(j, scalarBytes(shareSecret), raw) })
    return r.shares.map((s, i) => { if (r.status[i] !== 0) throw statusError(r.status[i]); return new EscrowShare(s) })
}
// verifyEscrowShares(params, auditors, tags, shares): one share per tag -> boolean[]; what does not deserialise throws.  Call it on every share before combining.
async function verifyEscrowShares(params, auditors, tags, shares) {
    if (shares.length !== tags.length) throw new RangeError('verifyEscrowShares: one share per tag')
    if (!tags.length) return []
    const rawT = tags.map(tagBytes), rawS = shares.map(shareBytes)
    const r = await engineFor(paramsOf(params), null).run((engine) => { useAuditors(engine, auditors); return engine.auditorsShareVerifyBatch(rawT, rawS) })
    r.status.forEach((st) => { if (st !== 0) throw statusError(st) })
    return r.ok
}
// combineEscrowShares(params, auditors, keys, tags, shares): shares[s][b] is one auditor's share of tags[b], t rows of different auditors (their indices come
// from the shares) -> what openEscrowTags gives for the undivided secret: with one key list the index or null per tag, with one key list per tag
// { ring, index } or null.  It does NOT verify: call verifyEscrowShares first.
async function combineEscrowShares(params, auditors, keys, tags, shares) {
    if (shares.length !== auditors.t || shares.some((row) => row.length !== tags.length)) throw new RangeError('combineEscrowShares: t rows of one share per tag')
    if (!tags.length) return []
    const raw = tags.map(tagBytes), rows = shares.map((row) => row.map(shareBytes)), who = rows.map((row) => row[0].readUInt32BE(8))
    const lists = isKeyLists(keys), perTag = lists ? keys : tags.map(() => keys)
    if (perTag.length !== tags.length) throw new RangeError('combineEscrowShares: one key list per tag')
    const { rings, ringOfEntry } = memberRingsOf(perTag, false)
    const { withRings, capacity } = engineFor(paramsOf(params), perTag[0])
    const out = new Array(tags.length), per = capacity()
    for (let g = 0; g < rings.length; g += per) {
        const sel = []
        for (let i = 0; i < tags.length; i++) if (ringOfEntry[i] >= g && ringOfEntry[i] < g + per) sel.push(i)
        const r = await withRings(rings.slice(g, g + per), (engine, ids) => {
            useAuditors(engine, auditors)
            return engine.auditorsCombineBatch(who, sel.map((i) => raw[i]), rows.map((row) => sel.map((i) => row[i])), sel.map((i) => ids[ringOfEntry[i] - g]))
        })
        sel.forEach((i, k) => {
            if (r.status[k] !== 0) throw statusError(r.status[k])
            out[i] = r.index[k] === 0xffffffff ? null : lists ? { ring: ringOfEntry[i], index: r.index[k] } : r.index[k]
        })
    }
    return out
}

// ---------------------------------------------------------------- distinct-key proofs: two key commitments hide different keys (src/commit/mult.ts:26-175)
// A DistinctProof keeps the engine's ZKD1 bytes (include/zkattest.h) and materialises C_w and the reference's MultProof members (six Points, seven Scalars).
class DistinctProof {
    constructor(bytes) {
        if (!(Buffer.isBuffer(bytes) && bytes.length === 744 && bytes.slice(0, 4).toString('latin1') === 'ZKD1' && bytes.readUInt32BE(4) === 744 && bytes.readUInt32BE(8) === 0 &&
            bytes.readUInt32BE(12) === 0)) throw new Error('error deserializing DistinctProof')
        this.bytes = bytes
    }
    _pt(o) { return new Point(tomEdwards256, fromBE(this.bytes.slice(o, o + 36)), fromBE(this.bytes.slice(o + 36, o + 72))) }
    _sc(o) { return new Scalar(tomEdwards256, fromBE(this.bytes.slice(o, o + 32))) }
    get C_w() { return this._pt(16) }
    get C_4() { return this._pt(88) }
    get A_x() { return this._pt(160) }
    get A_y() { return this._pt(232) }
    get A_z() { return this._pt(304) }
    get A_4_1() { return this._pt(376) }
    get A_4_2() { return this._pt(448) }
    get t_x() { return this._sc(520) }
    get t_y() { return this._sc(552) }
    get t_z() { return this._sc(584) }
    get t_rx() { return this._sc(616) }
    get t_ry() { return this._sc(648) }
    get t_rz() { return this._sc(680) }
    get t_r4() { return this._sc(712) }
    eq(o) { return o instanceof DistinctProof && this.bytes.equals(o.bytes) }
}
// the k (k - 1) / 2 pairs [i, j], i < j, of k commitments in lexicographic order: one distinct-key proof per pair shows k different keys
function distinctPairs(k) {
    const out = []
    for (let i = 0; i < k; i++) for (let j = i + 1; j < k; j++) out.push([i, j])
    return out
}
// proveDifferentKeys(params, keyA, comA, blinderA, keyB, comB, blinderB): comA = keyA g + blinderA h and comB = keyB g + blinderB h (Points, Commitments or 72-byte
// Buffers; keys and blinders Scalars, bigints or 32-byte Buffers -- keyBlinders gives a keyXcom's) hide different keys -> DistinctProof, which verifies for
// (comA, comB) in this order only.  The engine draws fresh seeds.  Throws 'error deserializing' for a commitment off the curve, '... hide the same key ...' for equal
// keys and "... do not open ..." when a key and its blinder do not open their commitment.
async function proveDifferentKeys(params, keyA, comA, blinderA, keyB, comB, blinderB) {
    return (await proveDifferentKeysBatch(params, [keyA], [comA], [blinderA], [keyB], [comB], [blinderB]))[0]
}
async function verifyDifferentKeys(params, comA, comB, proof) {   // -> boolean; what does not deserialise throws
    return (await verifyDifferentKeysBatch(params, [comA], [comB], [proof]))[0]
}
// batched: arrays of equal length
async function proveDifferentKeysBatch(params, keysA, comsA, blindersA, keysB, comsB, blindersB) {
    const B = keysA.length
    if ([comsA, blindersA, keysB, comsB, blindersB].some((a) => a.length !== B)) throw new RangeError('proveDifferentKeysBatch: two keys, two commitments and two blinders per entry')
    if (!B) return []
    const r = await engineFor(paramsOf(params), null).run((engine) => engine.distinctProveBatch(keysA.map(scalarBytes), comsA.map(comBytes), blindersA.map(scalarBytes),
        keysB.map(scalarBytes), comsB.map(comBytes), blindersB.map(scalarBytes)))
    return r.proofs.map((p, i) => {
        if (r.status[i] === 14) throw new Error('the two commitments hide the same key: no distinct-key proof exists')
        if (r.status[i] !== 0) throw statusError(r.status[i])
        return new DistinctProof(p)
    })
}
async function verifyDifferentKeysBatch(params, comsA, comsB, proofs) {
    const B = proofs.length
    if (comsA.length !== B || comsB.length !== B) throw new RangeError('verifyDifferentKeysBatch: two commitments per distinct-key proof')
    if (!B) return []
    const r = await engineFor(paramsOf(params), null).run((engine) => engine.distinctVerifyBatch(comsA.map(comBytes), comsB.map(comBytes),
        proofs.map((l) => (l instanceof DistinctProof ? l.bytes : new DistinctProof(l).bytes))))
    r.status.forEach((st) => { if (st !== 0) throw statusError(st) })
    return r.ok
}

// ---------------------------------------------------------------- quorum proofs: k attestations by k different ring members as one artifact
// A QuorumProof keeps the engine's ZKQ1 bytes (include/zkattest.h): a 16-byte header, k attestations in one wire layout, k (k - 1) / 2 distinct-key proofs between
// their keyXcoms in distinctPairs(k)'s order.  The key commitments are the ones inside the attestations: the distinct-key proofs cannot be checked against others.
class QuorumProof {
    constructor(bytes) {
        const bad = () => new Error('error deserializing QuorumProof')
        if (!(Buffer.isBuffer(bytes) && bytes.length >= 16 && bytes.slice(0, 4).toString('latin1') === 'ZKQ1' && bytes.readUInt32BE(4) === bytes.length && bytes.readUInt32BE(12) === 0)) throw bad()
        const k = bytes.readUInt32BE(8)
        if (k < 2 || k > 16) throw bad()
        const end = bytes.length - 744 * (k * (k - 1) / 2)
        let pos = 16
        this.offsets = [pos]
        for (let i = 0; i < k; i++) {
            if (end - pos < 32) throw bad()
            const len = bytes.readUInt32BE(pos + 4)
            if (len < 32 || len % 4 || len > end - pos) throw bad()
            pos += len
            this.offsets.push(pos)
        }
        if (pos !== end) throw bad()
        this.bytes = bytes
        this.k = k
    }
    get attestations() { return Array.from({ length: this.k }, (_, i) => new SignatureProofList(this.bytes.slice(this.offsets[i], this.offsets[i + 1]))) }
    get distinctProofs() { return distinctPairs(this.k).map((_, p) => new DistinctProof(this.bytes.slice(this.offsets[this.k] + 744 * p, this.offsets[this.k] + 744 * p + 744))) }
    eq(o) { return o instanceof QuorumProof && this.bytes.equals(o.bytes) }
}
// `keys` of proveQuorum / verifyQuorum as one key list PER MEMBER: the different rings among them, and each member's.  A quorum is one call: all its rings are
// resident at once, so it may name at most residentRings of them.
function quorumRings(keyLists, k, proving) {
    if (keyLists.length !== k) throw new RangeError('one key list per member')
    const rings = [], ringOfMember = new Array(k), byTag = new Map()
    keyLists.forEach((keys, i) => {
        checkRingSize(Buffer.isBuffer(keys) ? keys.length / 32 : keys.length, proving)
        const r = ringOf(keys)
        if (!byTag.has(r.tag)) { byTag.set(r.tag, rings.length); rings.push(r) }
        ringOfMember[i] = byTag.get(r.tag)
    })
    return { rings, ringOfMember }
}
function quorumEngine(params, keyLists, rings) {
    const e = engineFor(params, keyLists[0])
    if (rings.length > e.capacity()) throw new RangeError('a quorum names more rings than residentRings')
    return e
}
// proveQuorum(params, msgHashes, sigs, publicKeys, whichs, keys): k = msgHashes.length attestations over the ring `keys` (the arguments of proveSignatureListBatch),
// signed by k DIFFERENT members -> QuorumProof.  Throws '... the same key ...' when two of the signers are the same member.  The engine draws both seed sets.
async function proveQuorum(params, msgHashes, sigs, publicKeys, whichs, keys) {
    const k = msgHashes.length
    if (k < 2 || k > 16 || sigs.length !== k || publicKeys.length !== k || whichs.length !== k) throw new RangeError('proveQuorum: 2 to 16 members, one hash, signature, key and index each')
    const raws = await Promise.all(publicKeys.map(rawPublicKey))
    for (const r of raws) if (r.length !== 65 || r[0] !== 4) throw new Error('invalid public key')
    const msg = Buffer.concat(msgHashes.map((m) => Buffer.from(m))), sig = Buffer.concat(sigs.map((s) => Buffer.from(s))), pk = Buffer.concat(raws.map((x) => x.slice(1)))
    const wire = wireLayout
    let r
    if (isKeyLists(keys)) {   // one key list per member (the convention of reringSignatureLists): ONE zk_rings_quorum_prove_batch, the active ring is not touched
        const { rings, ringOfMember } = quorumRings(keys, k, true)
        r = await quorumEngine(params, keys, rings).withRings(rings, (engine, ids) => { useWire(engine, wire); return engine.ringsQuorumProveBatch(k, msg, sig, pk, whichs, ringOfMember.map((i) => ids[i])) })
    } else {
        checkRingSize(Buffer.isBuffer(keys) ? keys.length / 32 : keys.length, true)
        r = await engineFor(params, keys).withRing((engine) => { useWire(engine, wire); return engine.quorumProveBatch(k, msg, sig, pk, whichs) })
    }
    if (r.status[0] === 14 && r.memberStatus.every((s) => s === 0)) throw new Error('two members of the quorum have the same key: no quorum proof exists')
    if (r.status[0] !== 0) throw statusError(r.status[0])
    return new QuorumProof(r.bundles[0])
}
// -> boolean: every attestation verifies over `keys` for its message hash and every pair of them comes from different keys.  What does not deserialise throws.
async function verifyQuorum(params, msgHashes, keys, proof) {
    const q = proof instanceof QuorumProof ? proof : new QuorumProof(proof)
    if (msgHashes.length !== q.k) throw new RangeError('verifyQuorum: one message hash per member')
    const msg = Buffer.concat(msgHashes.map((m) => Buffer.from(m)))
    const wire = isPacked(q.bytes.slice(16)) ? 1 : 0, level = verifyLevel, reps = verifyReps
    const set = (engine) => { useWire(engine, wire); useVerifyLevel(engine, level); useVerifyReps(engine, reps) }
    let r
    if (isKeyLists(keys)) {
        const { rings, ringOfMember } = quorumRings(keys, q.k, false)
        r = await quorumEngine(params, keys, rings).withRings(rings, (engine, ids) => { set(engine); return engine.ringsQuorumVerifyBatch(q.k, msg, [q.bytes], ringOfMember.map((i) => ids[i])) })
    } else {
        checkRingSize(Buffer.isBuffer(keys) ? keys.length / 32 : keys.length, false)
        r = await engineFor(params, keys).withRing((engine) => { set(engine); return engine.quorumVerifyBatch(q.k, msg, [q.bytes]) })
    }
    if (r.status[0] !== 0) throw statusError(r.status[0])
    return r.ok[0]
}

// ---------------------------------------------------------------- accountable attestations: an attestation that carries its escrow tag
// An AccountableProof keeps the engine's ZKC1 bytes (include/zkattest.h): a 16-byte header, one attestation in one wire layout, the 472-byte ZKT1 tag of the keyXcom
// inside that attestation.  The commitment is not repeated: the tag cannot be checked against another attestation.
class AccountableProof {
    constructor(bytes) {
        const bad = () => new Error('error deserializing AccountableProof')
        if (!(Buffer.isBuffer(bytes) && bytes.length >= 16 + 32 + 472 && bytes.length % 4 === 0 && bytes.slice(0, 4).toString('latin1') === 'ZKC1' && bytes.readUInt32BE(4) === bytes.length &&
            bytes.readUInt32BE(8) === 0 && bytes.readUInt32BE(12) === 0)) throw bad()
        if (bytes.readUInt32BE(20) !== bytes.length - 16 - 472) throw bad()   // the inner total_len walks exactly to the tag
        this.bytes = bytes
    }
    get attestation() { return new SignatureProofList(this.bytes.slice(16, this.bytes.length - 472)) }
    get tag() { return new EscrowTag(this.bytes.slice(this.bytes.length - 472)) }
    eq(o) { return o instanceof AccountableProof && this.bytes.equals(o.bytes) }
}
const accountableBytes = (p) => (p instanceof AccountableProof ? p.bytes : new AccountableProof(p).bytes)
// One key list per entry in the place of `keys`: the distinct lists, in groups of at most residentRings, and per group the entries that belong to it.
// job(withRings, the group's rings, the group's entries, entry -> position of its ring in the group)
async function accountableGroups(params, keyLists, prove, job) {
    const { rings, ringOfEntry } = memberRingsOf(keyLists, prove)
    const { withRings, capacity } = engineFor(paramsOf(params), keyLists[0])
    const per = capacity()
    for (let g = 0; g < rings.length; g += per) {
        const sel = []
        for (let i = 0; i < keyLists.length; i++) if (ringOfEntry[i] >= g && ringOfEntry[i] < g + per) sel.push(i)
        await job(withRings, rings.slice(g, g + per), sel, (i) => ringOfEntry[i] - g)
    }
    return ringOfEntry
}
// proveAccountables(params, auditor, msgHashes, sigs, publicKeys, whichs, keys): one attestation per row over the ring `keys` (the arguments of
// proveSignatureListBatch), each with the escrow tag of its keyXcom under the auditor's key (a Point or 72 bytes) -> AccountableProof[].  The engine draws both seed sets.
async function proveAccountables(params, auditor, msgHashes, sigs, publicKeys, whichs, keys) {
    const B = msgHashes.length
    if (sigs.length !== B || publicKeys.length !== B || whichs.length !== B) throw new RangeError('proveAccountables: one hash, signature, key and index per attestation')
    if (!B) return []
    const raws = await Promise.all(publicKeys.map(rawPublicKey))
    for (const r of raws) if (r.length !== 65 || r[0] !== 4) throw new Error('invalid public key')
    const msg = Buffer.concat(msgHashes.map((m) => Buffer.from(m))), sig = Buffer.concat(sigs.map((x) => Buffer.from(x))), pk = Buffer.concat(raws.map((x) => x.slice(1)))
    const wire = wireLayout
    if (isKeyLists(keys)) {   // one key list per proof (the convention of reringSignatureLists): zk_rings_accountable_prove_batch per group of resident rings, no active ring
        if (keys.length !== B) throw new RangeError('proveAccountables: one key list per attestation')
        const out = new Array(B), cut = (a, w, sel) => Buffer.concat(sel.map((i) => a.slice(w * i, w * i + w)))
        await accountableGroups(params, keys, true, async (withRings, rings, sel, idOf) => {
            const r = await withRings(rings, (engine, ids) => { useWire(engine, wire); useAuditor(engine, auditor)
                return engine.accountableProveBatchRings(cut(msg, 32, sel), cut(sig, 64, sel), cut(pk, 64, sel), sel.map((i) => whichs[i]), sel.map((i) => ids[idOf(i)])) })
            sel.forEach((i, k) => { if (r.status[k] !== 0) throw statusError(r.status[k]); out[i] = new AccountableProof(r.bundles[k]) })
        })
        return out
    }
    checkRingSize(Buffer.isBuffer(keys) ? keys.length / 32 : keys.length, true)
    const r = await engineFor(params, keys).withRing((engine) => { useWire(engine, wire); useAuditor(engine, auditor); return engine.accountableProveBatch(msg, sig, pk, whichs) })
    return r.bundles.map((b, i) => { if (r.status[i] !== 0) throw statusError(r.status[i]); return new AccountableProof(b) })
}
async function proveAccountable(params, auditor, msgHash, sig, publicKey, which, keys) {
    return (await proveAccountables(params, auditor, [msgHash], [sig], [publicKey], [which], keys))[0]
}
// -> boolean[]: the attestation verifies over `keys` for its message hash AND its tag verifies against the keyXcom inside it under the auditor's key.  What does not
// deserialise throws.  All proofs of a call are in one wire layout.
async function verifyAccountables(params, auditor, msgHashes, keys, proofs) {
    const B = proofs.length
    if (msgHashes.length !== B) throw new RangeError('verifyAccountables: one message hash per proof')
    if (!B) return []
    const raw = proofs.map(accountableBytes), msg = Buffer.concat(msgHashes.map((m) => Buffer.from(m)))
    const wire = isPacked(raw[0].slice(16)) ? 1 : 0, level = verifyLevel, reps = verifyReps
    if (isKeyLists(keys)) {   // one key list per proof: zk_rings_accountable_verify_batch
        if (keys.length !== B) throw new RangeError('verifyAccountables: one key list per proof')
        const out = new Array(B)
        await accountableGroups(params, keys, false, async (withRings, rings, sel, idOf) => {
            const r = await withRings(rings, (engine, ids) => { useWire(engine, wire); useVerifyLevel(engine, level); useVerifyReps(engine, reps); useAuditor(engine, auditor)
                return engine.accountableVerifyBatchRings(Buffer.concat(sel.map((i) => msg.slice(32 * i, 32 * i + 32))), sel.map((i) => raw[i]), sel.map((i) => ids[idOf(i)])) })
            sel.forEach((i, k) => { if (r.status[k] !== 0) throw statusError(r.status[k]); out[i] = r.ok[k] })
        })
        return out
    }
    checkRingSize(Buffer.isBuffer(keys) ? keys.length / 32 : keys.length, false)
    const r = await engineFor(params, keys).withRing((engine) => { useWire(engine, wire); useVerifyLevel(engine, level); useVerifyReps(engine, reps); useAuditor(engine, auditor)
        return engine.accountableVerifyBatch(msg, raw) })
    r.status.forEach((st) => { if (st !== 0) throw statusError(st) })
    return r.ok
}
async function verifyAccountable(params, auditor, msgHash, keys, proof) {
    return (await verifyAccountables(params, auditor, [msgHash], keys, [proof]))[0]
}
// openAccountables(params, secret, keyLists, proofs): the auditor's call straight on bundles, one key list per proof (zk_rings_accountable_open_batch: no split,
// only the tags move) -> per proof { ring, index } -- ring counts the distinct key lists in the order of their first appearance, as openEscrowTags has it -- or
// null for nobody.  It does NOT verify: call verifyAccountables first.
async function openAccountables(params, secret, keyLists, proofs) {
    const B = proofs.length
    if (!isKeyLists(keyLists) || keyLists.length !== B) { if (!B) return []; throw new RangeError('openAccountables: one key list per proof') }
    const raw = proofs.map(accountableBytes), a = scalarBytes(secret), out = new Array(B)
    const wire = isPacked(raw[0].slice(16)) ? 1 : 0
    const ringOfEntry = await accountableGroups(params, keyLists, false, async (withRings, rings, sel, idOf) => {
        const r = await withRings(rings, (engine, ids) => { useWire(engine, wire); useAuditor(engine, engine.escrowKeygen(a))
            return engine.accountableOpenBatchRings(a, sel.map((i) => raw[i]), sel.map((i) => ids[idOf(i)])) })
        sel.forEach((i, k) => { if (r.status[k] !== 0) throw statusError(r.status[k]); out[i] = r.index[k] === 0xffffffff ? null : r.index[k] })
    })
    return out.map((w, i) => (w === null ? null : { ring: ringOfEntry[i], index: w }))
}
// splitAccountable(params, proofs) -> [{ attestation: SignatureProofList, tag: EscrowTag }]: pure layout, for verifySignatureLists, reringSignatureLists and the
// auditor's calls (openEscrowTags, shareEscrowTags, combineEscrowShares).  joinAccountable(params, attestations, tags) -> AccountableProof[] is its inverse: a tag is
// bound to keyXcom and the auditor's key, not to the ring, so split -> reringSignatureLists -> join keeps it.
async function splitAccountable(params, proofs) {
    if (!proofs.length) return []
    const raw = proofs.map(accountableBytes), wire = isPacked(raw[0].slice(16)) ? 1 : 0
    const r = await engineFor(paramsOf(params), null).run((engine) => { useWire(engine, wire); return engine.accountableSplitBatch(raw) })
    return raw.map((_, i) => { if (r.status[i] !== 0) throw statusError(r.status[i]); return { attestation: new SignatureProofList(r.attestations[i]), tag: new EscrowTag(r.tags[i]) } })
}
async function joinAccountable(params, attestations, tags) {
    if (tags.length !== attestations.length) throw new RangeError('joinAccountable: one tag per attestation')
    if (!tags.length) return []
    const pr = attestations.map((a) => (Buffer.isBuffer(a) ? a : a.bytes)), tg = tags.map((t) => (t instanceof EscrowTag ? t.bytes : new EscrowTag(t).bytes))
    const wire = isPacked(pr[0]) ? 1 : 0
    const r = await engineFor(paramsOf(params), null).run((engine) => { useWire(engine, wire); return engine.accountableJoinBatch(pr, tg) })
    return r.bundles.map((b, i) => { if (r.status[i] !== 0) throw statusError(r.status[i]); return new AccountableProof(b) })
}

module.exports = { openAccountables, proveAccountable, proveAccountables, verifyAccountable, verifyAccountables, splitAccountable, joinAccountable, AccountableProof, splitAuditorKey, shareEscrowTags, verifyEscrowShares, combineEscrowShares, EscrowShare, proveEscrowTag, verifyEscrowTag, proveEscrowTags, verifyEscrowTags, openEscrowTags, escrowAuditorKey, EscrowTag, proveQuorum, verifyQuorum, QuorumProof, proveDifferentKeys, verifyDifferentKeys, proveDifferentKeysBatch, verifyDifferentKeysBatch, distinctPairs, DistinctProof, proveSameKey, verifySameKey, proveSameKeys, verifySameKeys, keyCommitment, keyCommitments, LinkProof, reringSignatureLists, keyBlinders, proveMembership, verifyMembership, proveMemberships, verifyMemberships, proveMembershipLists, verifyMembershipLists, GKProof, Commitment, commit, screenSignatureLists, findKey, SCREEN, WHICH_NONE, recoverSignatureLists, recoverKey, RECOVER, verifySignatureLists, proveSignatureLists, _ringGenerations, setVerifyLevel, getVerifyLevel, setVerifyReps, getVerifyReps, generateParamsList, generateParamsListHardened, keyToInt, proveSignatureList, verifySignatureList, proveSignatureListBatch, verifySignatureListBatch,
    writeJson, readJson, writeJsonBatch, readJsonBatch, SignatureProofList, SystemParametersList, PedersenParams, generatePedersenParams, p256, tomEdwards256, ALL_GROUPS,
    Group, Point, Scalar, Engine, shutdown, setWireLayout, getWireLayout, setOption, native }
