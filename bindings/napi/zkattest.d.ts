// Type declarations of bindings/napi/zkattest.js: the reference's public surface (src/index.ts:17-19) over the MI355X engine.
/// <reference types="node" />
export class Group { readonly name: string; readonly p: bigint; readonly order: bigint; eq(g: Group): boolean; generator(): Point; isOnGroup(p: Point): boolean }
export class Point { readonly group: Group; x: bigint; y: bigint; eq(o: Point): boolean; add(o: Point): Point; mul(k: bigint | Scalar): Point; isIdentity(): boolean }
export class Scalar { readonly group: Group; k: bigint; eq(o: Scalar): boolean }
export const p256: Group, tomEdwards256: Group, ALL_GROUPS: Group[]
export class PedersenParams { c: Group; g: Point; h: Point; constructor(c: Group, g: Point, h: Point); eq(o: PedersenParams): boolean }
export function generatePedersenParams(c: Group, g?: Point): PedersenParams
export class SystemParametersList {
    NistGroup: PedersenParams; ProofGroup: PedersenParams; SecLevel: number
    constructor(NistGroup: PedersenParams, ProofGroup: PedersenParams, SecLevel: number)
    eq(o: SystemParametersList): boolean
}
export interface MultProof { C_4: Point; A_x: Point; A_y: Point; A_z: Point; A_4_1: Point; A_4_2: Point; t_x: Scalar; t_y: Scalar; t_z: Scalar; t_rx: Scalar; t_ry: Scalar; t_rz: Scalar; t_r4: Scalar }
export interface EqualityProof { A_1: Point; A_2: Point; t_x: Scalar; t_r1: Scalar; t_r2: Scalar }
export interface PointAddProof { C_8: Point; C_10: Point; C_11: Point; C_13: Point; pi_8: MultProof; pi_10: MultProof; pi_11: MultProof; pi_13: MultProof; pi_x: EqualityProof; pi_y: EqualityProof }
export interface ExpProof { A: Point; Tx: Point; Ty: Point; alpha?: Scalar; beta1?: Scalar; beta2?: Scalar; beta3?: Scalar; z?: Scalar; z2?: Scalar; proof?: PointAddProof; r1?: Scalar; r2?: Scalar }
export interface GKProof { cl: Point[]; ca: Point[]; cb: Point[]; cd: Point[]; f: Scalar[]; za: Scalar[]; zb: Scalar[]; zd: Scalar }
export class SignatureProofList {
    /** the engine's binary form of the proof (ZKA1, include/zkattest.h); the members below are materialised from it on demand */
    readonly bytes: Buffer
    constructor(zka1: Buffer)
    readonly R: Point; readonly comS1: Point; readonly keyXcom: Point; readonly keyYcom: Point
    readonly expProof: ExpProof[]; readonly membershipProof: GKProof
    eq(o: SignatureProofList): boolean
}
export type PublicKey = Buffer | Uint8Array | import('crypto').KeyObject | CryptoKey
export function generateParamsList(secLevel?: number): SystemParametersList
/** hardened mode: NUMS generators + statement-bound membership challenge; not byte-compatible with the reference */
export function generateParamsListHardened(secLevel?: number, tag?: Uint8Array): SystemParametersList & { hardened: boolean }
export function keyToInt(publicKey: PublicKey): Promise<bigint>
export function proveSignatureList(params: SystemParametersList, msgHash: Uint8Array, sigBytes: Uint8Array, publicKey: PublicKey, which: number, keys: bigint[]): Promise<SignatureProofList>
export function verifySignatureList(params: SystemParametersList, msgHash: Uint8Array, keys: bigint[], proof: SignatureProofList): Promise<boolean>
export function proveSignatureListBatch(params: SystemParametersList, msgHashes: Uint8Array[], sigs: Uint8Array[], publicKeys: PublicKey[], whichs: number[], keys: bigint[] | Buffer): Promise<SignatureProofList[]>
/** booleans per proof; `errors[b]` holds what verifySignatureList would have thrown for proof b (null otherwise) -- a malformed proof never affects its neighbours */
export type Verdicts = boolean[] & { readonly errors: (Error | null)[] }
export function verifySignatureListBatch(params: SystemParametersList, msgHashes: Uint8Array[], keys: bigint[] | Buffer, proofs: (SignatureProofList | Buffer)[]): Promise<Verdicts>
/** facade-wide options.  ringDelta (default 0 = off): a key list that is not resident but differs from a resident ring of the same length in at most `value`
 *  32-byte entries updates that ring in place (Engine.updateRing) and re-tags it instead of building a new ring; Engine.setOption('ringDelta') overrides it per engine */
export function setOption(name: 'ringDelta', value: number): void
/** one statement per proof over its own ring: keyLists[i] is proof i's ring.  The rings stay resident on the params' engine (Engine.setOption('residentRings')),
 *  every call is one mixed-ring batch on the GPU (split only when it names more rings than are kept resident) */
export function verifySignatureLists(params: SystemParametersList, msgHashes: Uint8Array[], keyLists: (bigint[] | Buffer)[], proofs: (SignatureProofList | Buffer)[]): Promise<Verdicts>
/** B statements over several rings in one call, proved: keyLists[i] is the ring of proof i and whichs[i] indexes it (zk_prove_batch_rings).  The rings stay resident
 *  through the cache verifySignatureLists uses; a call is split only when it names more rings than residentRings. */
export function proveSignatureLists(params: SystemParametersList, msgHashes: Uint8Array[], sigs: Uint8Array[], publicKeys: PublicKey[], whichs: number[], keyLists: (bigint[] | Buffer)[]): Promise<SignatureProofList[]>
/** re-ring (zk_proof_rering_batch): proofs made for any ring become proofs for `keys` with their signature part untouched -- only the GKProof section is made anew,
 *  over the same keyXcom.  whichNew[i]: the index of proof i's key in `keys`; keyBlinders[i]: the blinder of its keyXcom (keyBlinders).  Throws for the first proof
 *  that fails.  Two GKProofs over one keyXcom place the key in the intersection of the two rings. */
export function reringSignatureLists(params: SystemParametersList, msgHashes: Uint8Array[], proofs: (SignatureProofList | Buffer)[], whichNew: number[], keyBlinders: Uint8Array[], keys: bigint[] | Buffer): Promise<SignatureProofList[]>
/** ... with one key list per proof (zk_proof_rering_batch_rings; rings named as in proveSignatureLists / verifySignatureLists): proof i moves to keyLists[i],
 *  whichNew[i] indexes that list; the lists are made resident, the active ring is not touched. */
export function reringSignatureLists(params: SystemParametersList, msgHashes: Uint8Array[], proofs: (SignatureProofList | Buffer)[], whichNew: number[], keyBlinders: Uint8Array[], keyLists: (bigint[] | Buffer)[]): Promise<SignatureProofList[]>
/** zk_prove_key_blinders: the blinders of keyXcom in the proofs made from `seeds` (B x 32 bytes, or one Uint8Array(32) per proof); as secret as the seeds */
export function keyBlinders(seeds: Buffer | Uint8Array[], params?: SystemParametersList): Promise<Buffer[]>
/** the witness screen (zk_screen_batch_rings): before a proof is paid for, where the signer's key stands in `keys` (`which` absent: the lowest index is found; given: that
 *  index is checked) and whether the ECDSA signature verifies.  flags is a set of SCREEN bits; ok = (flags === 0) means proveSignatureList with `which` gives a proof that
 *  verifies.  SCREEN.SIG_RANGE (r or s outside [1, n - 1]) is stricter than the prover, which reduces them mod n. */
export interface ScreenStatement { msgHash: Uint8Array; sigBytes: Uint8Array; publicKey: PublicKey; keys: bigint[] | Buffer; which?: number }
export interface ScreenVerdict { which: number; flags: number; ok: boolean }
export const SCREEN: { readonly KEY_NOT_ON_CURVE: 1; readonly SIG_RANGE: 2; readonly SIG_INVALID: 4; readonly NOT_IN_RING: 8; readonly RING_NOT_RESIDENT: 16 }
export const WHICH_NONE: number
export function screenSignatureLists(params: SystemParametersList, statements: ScreenStatement[]): Promise<ScreenVerdict[]>
/** the lookup alone: the lowest index of the key's x-coordinate among keys, or -1; params default to those the facade used last */
export function findKey(publicKey: PublicKey, keys: bigint[] | Buffer, params?: SystemParametersList): Promise<number>
/** Key recovery (zk_recover_batch_rings): the signer's key from (msgHash, sigBytes) alone and its lowest index among `keys`.  flags is a set of RECOVER bits; with
 *  flags === 0 publicKey is the raw 65-byte uncompressed point, which proveSignatureList(s) takes as its publicKey as it is (or import it:
 *  subtle.importKey('raw', publicKey, { name: 'ECDSA', namedCurve: 'P-256' }, true, ['verify'])); otherwise publicKey is null and which is WHICH_NONE. */
export interface RecoverStatement { msgHash: Uint8Array; sigBytes: Uint8Array; keys: bigint[] | Buffer }
export interface RecoveredKey { publicKey: Buffer | null; which: number; flags: number }
export const RECOVER: { readonly SIG_RANGE: 2; readonly NOT_IN_RING: 8; readonly RING_NOT_RESIDENT: 16; readonly NO_POINT: 32 }
export function recoverSignatureLists(params: SystemParametersList, statements: RecoverStatement[]): Promise<RecoveredKey[]>
export function recoverKey(msgHash: Uint8Array, sigBytes: Uint8Array, keys: bigint[] | Buffer, params?: SystemParametersList): Promise<RecoveredKey>
/** ring membership of a committed value on its own (src/proofGK/gk.ts:94-262): ZKM1 proofs (ZKMB with a context: MemberOptions) over the engine's resident rings */
export class Commitment { p: Point; r: Scalar; constructor(p: Point, r: Scalar) }
export class GKProof {
    readonly bytes: Buffer; readonly n: number
    /** true for a "ZKMB" proof: made with a context, verifies only with it */
    readonly bound: boolean
    readonly cl: Point[]; readonly ca: Point[]; readonly cb: Point[]; readonly cd: Point[]
    readonly f: Scalar[]; readonly za: Scalar[]; readonly zb: Scalar[]; readonly zd: Scalar
    constructor(bytes: Buffer); eq(o: GKProof): boolean
}
/** pedersen.ts:53-58: value * g + r * h with a fresh blinder r */
export function commit(params: PedersenParams, value: bigint): Commitment
/** bound proofs ("ZKMB", include/zkattest.h: zk_member_*_bound): `context` -- 32 caller bytes per proof (a session nonce, a message hash, a verifier's id) -- is hashed
 *  into the challenge with the ring's digest and the commitment; the verifier must be given the same context.  One Uint8Array(32) for the single calls, an array of
 *  them (one per entry) for the batched and Lists calls.  No counterpart in the reference beyond the TODO at src/proofGK/gk.ts:178. */
export interface MemberOptions { context?: Uint8Array }
export interface MemberBatchOptions { context?: Uint8Array[] }
/** com.r is the blinder; throws unless com.p commits to keys[index] under it */
export function proveMembership(params: PedersenParams | SystemParametersList, com: Commitment, index: number, keys: bigint[] | Buffer): Promise<GKProof>
export function proveMembership(params: PedersenParams | SystemParametersList, com: Commitment, index: number, keys: bigint[] | Buffer, options: MemberOptions): Promise<GKProof>
export function verifyMembership(params: PedersenParams | SystemParametersList, com: Point, keys: bigint[] | Buffer, proof: GKProof): Promise<boolean>
export function verifyMembership(params: PedersenParams | SystemParametersList, com: Point, keys: bigint[] | Buffer, proof: GKProof, options: MemberOptions): Promise<boolean>
/** batched over one key list */
export function proveMemberships(params: PedersenParams | SystemParametersList, coms: Commitment[], indices: number[], keys: bigint[] | Buffer): Promise<GKProof[]>
export function proveMemberships(params: PedersenParams | SystemParametersList, coms: Commitment[], indices: number[], keys: bigint[] | Buffer, options: MemberBatchOptions): Promise<GKProof[]>
export function verifyMemberships(params: PedersenParams | SystemParametersList, coms: Point[], keys: bigint[] | Buffer, proofs: GKProof[]): Promise<boolean[]>
export function verifyMemberships(params: PedersenParams | SystemParametersList, coms: Point[], keys: bigint[] | Buffer, proofs: GKProof[], options: MemberBatchOptions): Promise<boolean[]>
/** batched with one key list per entry: keysList[i] is the ring of commitment i (resolved to the engine's resident rings like proveSignatureLists' key lists) */
export function proveMembershipLists(params: PedersenParams | SystemParametersList, coms: Commitment[], indices: number[], keysList: (bigint[] | Buffer)[]): Promise<GKProof[]>
export function proveMembershipLists(params: PedersenParams | SystemParametersList, coms: Commitment[], indices: number[], keysList: (bigint[] | Buffer)[], options: MemberBatchOptions): Promise<GKProof[]>
export function verifyMembershipLists(params: PedersenParams | SystemParametersList, coms: Point[], keysList: (bigint[] | Buffer)[], proofs: GKProof[]): Promise<boolean[]>
export function verifyMembershipLists(params: PedersenParams | SystemParametersList, coms: Point[], keysList: (bigint[] | Buffer)[], proofs: GKProof[], options: MemberBatchOptions): Promise<boolean[]>
/** Link proofs ("ZKL1", zk_link_*): comA = key g + blinderA h and comB = key g + blinderB h hide the same key (src/commit/equality.ts).  A link proof
 *  deliberately makes the two proofs linkable to anyone who sees it; the engine draws fresh seeds. */
export class LinkProof {
    constructor(bytes: Buffer)
    readonly bytes: Buffer
    readonly A_1: Point
    readonly A_2: Point
    readonly t_x: Scalar
    readonly t_r1: Scalar
    readonly t_r2: Scalar
    eq(o: LinkProof): boolean
}
type LinkCom = Point | Commitment | Buffer
type LinkScalar = Scalar | bigint | Uint8Array
export function proveSameKey(params: PedersenParams | SystemParametersList, key: LinkScalar, comA: LinkCom, blinderA: LinkScalar, comB: LinkCom, blinderB: LinkScalar): Promise<LinkProof>
export function verifySameKey(params: PedersenParams | SystemParametersList, comA: LinkCom, comB: LinkCom, link: LinkProof | Buffer): Promise<boolean>
export function proveSameKeys(params: PedersenParams | SystemParametersList, keys: LinkScalar[], comsA: LinkCom[], blindersA: LinkScalar[], comsB: LinkCom[], blindersB: LinkScalar[]): Promise<LinkProof[]>
export function verifySameKeys(params: PedersenParams | SystemParametersList, comsA: LinkCom[], comsB: LinkCom[], links: (LinkProof | Buffer)[]): Promise<boolean[]>
/** Escrow tags ("ZKT1", zk_ctx_set_auditor / zk_escrow_*): beside com = key g + blinder h, the key encrypted (exponential ElGamal) to the key A = a g of a designated
 *  auditor with a proof that it is com's key.  Anyone verifies a tag; who holds a opens it to the ring member's index.  A tag is bound to com and A, not to a
 *  message or a ring; opening does NOT verify; the engine draws fresh seeds; anyone who knows a can open every tag made for A. */
export class EscrowTag {
    constructor(bytes: Buffer)
    readonly bytes: Buffer
    readonly E1: Point
    readonly E2: Point
    readonly T1: Point
    readonly T2: Point
    readonly T3: Point
    readonly t_x: Scalar
    readonly t_r: Scalar
    readonly t_rho: Scalar
    eq(o: EscrowTag): boolean
}
export function escrowAuditorKey(params: PedersenParams | SystemParametersList, secret: LinkScalar): Promise<Point>
export function proveEscrowTag(params: PedersenParams | SystemParametersList, auditor: Point | Buffer, key: LinkScalar, com: LinkCom, blinder: LinkScalar): Promise<EscrowTag>
export function verifyEscrowTag(params: PedersenParams | SystemParametersList, auditor: Point | Buffer, com: LinkCom, tag: EscrowTag | Buffer): Promise<boolean>
export function proveEscrowTags(params: PedersenParams | SystemParametersList, auditor: Point | Buffer, keys: LinkScalar[], coms: LinkCom[], blinders: LinkScalar[]): Promise<EscrowTag[]>
export function verifyEscrowTags(params: PedersenParams | SystemParametersList, auditor: Point | Buffer, coms: LinkCom[], tags: (EscrowTag | Buffer)[]): Promise<boolean[]>
/** the auditor's call: per tag the index in `keys` of the ring member whose key it carries (the lowest where a key occurs twice), null for nobody */
export function openEscrowTags(params: PedersenParams | SystemParametersList, secret: LinkScalar, keys: bigint[] | Buffer, tags: (EscrowTag | Buffer)[]): Promise<(number | null)[]>
/** ... with ONE KEY LIST PER TAG in the place of `keys`: the tags of a registry sharded over several rings open in one zk_rings_escrow_open_batch (per group of at
 *  most residentRings rings), through each ring's resident point index.  Per tag { ring, index } -- ring counts the distinct key lists in the order of their first
 *  appearance, index is the member's (lowest) index in the tag's list -- or null for nobody. */
export function openEscrowTags(params: PedersenParams | SystemParametersList, secret: LinkScalar, keys: (bigint[] | Buffer)[], tags: (EscrowTag | Buffer)[]): Promise<({ ring: number; index: number } | null)[]>
/** Threshold opening ("ZKS1", zk_auditors_* / zk_ctx_set_auditors): a dealer splits the auditor's secret into Shamir shares; each of t of n auditors turns a tag into
 *  a 264-byte verifiable share (D = a_j E1 with a proof against A_j); anyone verifies shares and combines t of them into what openEscrowTags gives. */
export class EscrowShare {
    constructor(bytes: Buffer)
    readonly bytes: Buffer
    readonly j: number
    readonly D: Point
    readonly U1: Point
    readonly U2: Point
    readonly s: Scalar
    eq(o: EscrowShare): boolean
}
/** a t-of-n set: the auditor's key A, the threshold and the share keys A_1 .. A_n */
export interface AuditorSet { key: Point | Buffer; t: number; keys: (Point | Buffer)[] }
/** the dealer's split (the dealer sees the secret): the set to publish, and one 32-byte share secret per auditor */
export function splitAuditorKey(params: PedersenParams | SystemParametersList, secret: LinkScalar, t: number, n: number): Promise<{ key: Point; t: number; keys: Point[]; shares: Buffer[] }>
/** auditor j's shares of the tags; throws when the share secret is not A_j's */
export function shareEscrowTags(params: PedersenParams | SystemParametersList, auditors: AuditorSet, j: number, shareSecret: LinkScalar, tags: (EscrowTag | Buffer)[]): Promise<EscrowShare[]>
/** one share per tag; run it on every share before combining */
export function verifyEscrowShares(params: PedersenParams | SystemParametersList, auditors: AuditorSet, tags: (EscrowTag | Buffer)[], shares: (EscrowShare | Buffer)[]): Promise<boolean[]>
/** shares[s][b]: one auditor's share of tags[b], t rows of different auditors.  The answer is openEscrowTags' for the undivided secret; it does not verify */
export function combineEscrowShares(params: PedersenParams | SystemParametersList, auditors: AuditorSet, keys: bigint[] | Buffer, tags: (EscrowTag | Buffer)[], shares: (EscrowShare | Buffer)[][]): Promise<(number | null)[]>
export function combineEscrowShares(params: PedersenParams | SystemParametersList, auditors: AuditorSet, keys: (bigint[] | Buffer)[], tags: (EscrowTag | Buffer)[], shares: (EscrowShare | Buffer)[][]): Promise<({ ring: number; index: number } | null)[]>
/** Distinct-key proofs ("ZKD1", zk_distinct_*): comA = keyA g + blinderA h and comB = keyB g + blinderB h hide DIFFERENT keys: one MultProof (src/commit/mult.ts)
 *  for (keyA - keyB) * w = 1.  A proof verifies for (comA, comB) in this order only; equal keys throw '... hide the same key ...'; the engine draws fresh seeds. */
export class DistinctProof {
    constructor(bytes: Buffer)
    readonly bytes: Buffer
    readonly C_w: Point
    readonly C_4: Point
    readonly A_x: Point
    readonly A_y: Point
    readonly A_z: Point
    readonly A_4_1: Point
    readonly A_4_2: Point
    readonly t_x: Scalar
    readonly t_y: Scalar
    readonly t_z: Scalar
    readonly t_rx: Scalar
    readonly t_ry: Scalar
    readonly t_rz: Scalar
    readonly t_r4: Scalar
    eq(o: DistinctProof): boolean
}
export function proveDifferentKeys(params: PedersenParams | SystemParametersList, keyA: LinkScalar, comA: LinkCom, blinderA: LinkScalar, keyB: LinkScalar, comB: LinkCom, blinderB: LinkScalar): Promise<DistinctProof>
export function verifyDifferentKeys(params: PedersenParams | SystemParametersList, comA: LinkCom, comB: LinkCom, proof: DistinctProof | Buffer): Promise<boolean>
export function proveDifferentKeysBatch(params: PedersenParams | SystemParametersList, keysA: LinkScalar[], comsA: LinkCom[], blindersA: LinkScalar[], keysB: LinkScalar[], comsB: LinkCom[], blindersB: LinkScalar[]): Promise<DistinctProof[]>
export function verifyDifferentKeysBatch(params: PedersenParams | SystemParametersList, comsA: LinkCom[], comsB: LinkCom[], proofs: (DistinctProof | Buffer)[]): Promise<boolean[]>
/** the k (k - 1) / 2 pairs [i, j], i < j, of k commitments in lexicographic order: one distinct-key proof per pair shows k different signers */
export function distinctPairs(k: number): [number, number][]
/** `keys` of proveQuorum / verifyQuorum: one ring for all members, or one key list PER MEMBER (the convention of reringSignatureLists) for a registry sharded over
 *  several rings -- then whichs[i] indexes list i, all lists of a quorum are resident at once (at most residentRings different ones), and a key enrolled in two
 *  lists and used through both counts as the same key. */
export type QuorumKeys = bigint[] | Buffer | Array<bigint[] | Buffer>
/** Quorum proofs ("ZKQ1", zk_quorum_*): k attestations over one ring by k DIFFERENT members as one artifact -- a 16-byte header, the k attestations, the
 *  k (k - 1) / 2 distinct-key proofs between their keyXcoms in distinctPairs(k)'s order.  It tells whoever sees it that its attestations come from different signers. */
export class QuorumProof {
    readonly bytes: Buffer
    readonly k: number
    constructor(zkq1: Buffer)
    readonly attestations: SignatureProofList[]
    readonly distinctProofs: DistinctProof[]
    eq(o: QuorumProof): boolean
}
/** k = msgHashes.length attestations (2..16) signed by k different members of `keys`; throws when two signers are the same member */
export function proveQuorum(params: SystemParametersList, msgHashes: Uint8Array[], sigs: Uint8Array[], publicKeys: PublicKey[], whichs: number[], keys: QuorumKeys): Promise<QuorumProof>
/** true iff every attestation verifies over `keys` for its message hash and every pair of them comes from different keys; what does not deserialise throws */
export function verifyQuorum(params: SystemParametersList, msgHashes: Uint8Array[], keys: QuorumKeys, proof: QuorumProof | Buffer): Promise<boolean>
/** Accountable attestations ("ZKC1", zk_accountable_*): one attestation and the escrow tag of the keyXcom inside it as one artifact -- a 16-byte header, the
 *  attestation, the 472-byte ZKT1 tag.  The commitment is not repeated, so the tag can only be checked against the attestation it travels with. */
export class AccountableProof {
    readonly bytes: Buffer
    constructor(zkc1: Buffer)
    readonly attestation: SignatureProofList
    readonly tag: EscrowTag
    eq(o: AccountableProof): boolean
}
/** an attestation over `keys` with the escrow tag of its keyXcom under the auditor's key; the engine draws both seed sets */
/** one ring for every proof, or one key list per proof (the convention of reringSignatureLists: the zk_rings_accountable_* calls, no active ring) */
export type AccountableKeys = bigint[] | Buffer | Array<bigint[] | Buffer>
export function proveAccountable(params: SystemParametersList, auditor: LinkCom, msgHash: Uint8Array, sig: Uint8Array, publicKey: PublicKey, which: number, keys: AccountableKeys): Promise<AccountableProof>
export function proveAccountables(params: SystemParametersList, auditor: LinkCom, msgHashes: Uint8Array[], sigs: Uint8Array[], publicKeys: PublicKey[], whichs: number[], keys: AccountableKeys): Promise<AccountableProof[]>
/** true iff the attestation verifies over `keys` for its message hash and its tag verifies against the keyXcom inside it under the auditor's key; what does not deserialise throws */
export function verifyAccountable(params: SystemParametersList, auditor: LinkCom, msgHash: Uint8Array, keys: AccountableKeys, proof: AccountableProof | Buffer): Promise<boolean>
export function verifyAccountables(params: SystemParametersList, auditor: LinkCom, msgHashes: Uint8Array[], keys: AccountableKeys, proofs: (AccountableProof | Buffer)[]): Promise<boolean[]>
/** the auditor's call straight on bundles (zk_rings_accountable_open_batch), one key list per proof: { ring, index } as openEscrowTags gives, null for nobody; it does NOT verify */
export function openAccountables(params: PedersenParams | SystemParametersList, secret: bigint | Uint8Array, keyLists: Array<bigint[] | Buffer>, proofs: (AccountableProof | Buffer)[]): Promise<({ ring: number; index: number } | null)[]>
/** pure layout: the attestations for verifySignatureLists / reringSignatureLists, the tags for the auditor's calls; joinAccountable is the inverse (split, re-ring, join keeps the tag) */
export function splitAccountable(params: PedersenParams | SystemParametersList, proofs: (AccountableProof | Buffer)[]): Promise<{ attestation: SignatureProofList; tag: EscrowTag }[]>
export function joinAccountable(params: PedersenParams | SystemParametersList, attestations: (SignatureProofList | Buffer)[], tags: (EscrowTag | Buffer)[]): Promise<AccountableProof[]>
/** keyXcom of a proof (either wire layout; zk_proof_key_commitments) */
export function keyCommitment(proof: SignatureProofList | Buffer, params?: SystemParametersList): Promise<Point>
export function keyCommitments(proofs: (SignatureProofList | Buffer)[], params?: SystemParametersList): Promise<Point[]>
type Newable<T> = new (...args: any[]) => T
export function writeJson<T>(type: Newable<T>, object: T): string
export function readJson<T>(type: Newable<T>, text: string): T
/** whole batches on every host core, off the event loop; null where an item is malformed */
export function writeJsonBatch(proofs: (SignatureProofList | Buffer)[], threads?: number): Promise<(string | null)[]>
export function readJsonBatch(texts: (string | Buffer)[], threads?: number): Promise<(SignatureProofList | null)[]>
/** closes every cached GPU context (they are keyed by SystemParametersList content and device list) */
export function shutdown(): void
export interface EngineParams { nistH: Buffer; tomG: Buffer; tomH: Buffer; secLevel?: number }
export class Engine {
    constructor(devices?: number | number[])
    close(): void
    info(): { devices: number; ringTransport: string; proofMaxSize: number }
    /** residentRings (1..16, default 4): key rings the facade's context cache keeps built on this engine, least recently used dropped first;
     *  ringDelta (default 0 = off): a key list that misses the cache but differs from a resident ring of the same length in at most this many 32-byte entries
     *  updates that ring in place (updateRing) instead of building a new one */
    setOption(name: 'chunk' | 'lanes' | 'combBits' | 'hostTaper' | 'batchVerify' | 'mode' | 'slice' | 'ringFold' | 'verifyGroups' | 'wire' | 'verifyLevel' | 'verifyReps' | 'inflight' | 'residentRings' | 'ringDelta', value: number): void
    /** zero the witness-derived device memory (prover workspaces, staged signatures and seeds) of every device now; close() and a failed prove do it by themselves */
    wipe(): void
    setParams(p: EngineParams): void
    setRing(keys: Buffer | bigint[]): string
    /** resident rings (zk_pool_add_ring): built once, then switched by id without a rebuild; the active ring cannot be dropped */
    addRing(keys: Buffer | bigint[]): number
    useRing(id: number): void
    dropRing(id: number): void
    /** zk_pool_update_ring: ring `id` becomes what setRing of the changed key list would build; indices[j] gets keys[j] (the last entry for an index wins),
     *  nKeys is the new key count (default: unchanged).  The id, the active state and every other ring are untouched; the generation goes up by one. */
    updateRing(id: number, indices: ArrayLike<number | bigint>, keys: Buffer | bigint[], nKeys?: number): void
    ringInfo(id: number): { nKeys: number; logN: number; flags: number; generation: number }
    /** one resident ring id per proof (zk_pool_verify_batch_rings) */
    verifyBatchRings(msg: Buffer, proofs: Buffer[], ringIds: number[] | Uint32Array, seeds?: Buffer): Verdicts
    verifyBatchRingsAsync(msg: Buffer, proofs: Buffer[], ringIds: number[] | Uint32Array, seeds?: Buffer): Promise<Verdicts>
    /** zk_prove_batch_rings: which[b] indexes resident ring ringIds[b]; the active ring plays no part */
    proveBatchRings(msg: Buffer, sig: Buffer, pk: Buffer, which: number[] | Buffer, ringIds: number[] | Uint32Array, seeds?: Buffer): Buffer[]
    proveBatchRingsAsync(msg: Buffer, sig: Buffer, pk: Buffer, which: number[] | Buffer, ringIds: number[] | Uint32Array, seeds?: Buffer): Promise<Buffer[]>
    /** zk_prove_key_blinders: keyXcom's blinder of the proof made from each 32-byte seed */
    keyBlinders(seeds: Buffer): Buffer[]
    /** zk_proof_rering_batch: proofs moved to the ACTIVE ring; seeds must be fresh (default: crypto.randomBytes).  status 16: the index and blinder do not open keyXcom */
    reringBatch(msg: Buffer, proofs: Buffer[], whichNew: number[] | Uint32Array, blinders: Buffer, seeds?: Buffer): { proofs: (Buffer | null)[]; status: Int32Array }
    /** zk_proof_rering_batch_rings: proof i moved to the RESIDENT ring ringIds[i], the active ring neither read nor changed; a proof whose status is not 0 is null */
    reringBatchRings(msg: Buffer, proofs: Buffer[], whichNew: number[] | Uint32Array, ringIds: number[] | Uint32Array, blinders: Buffer, seeds?: Buffer): { proofs: (Buffer | null)[]; status: Int32Array }
    /** zk_link_prove_batch: per entry a 32-byte key, two 72-byte commitments and their 32-byte blinders; seeds must be fresh (default: crypto.randomBytes).  status 16: the key and a blinder do not open a commitment */
    linkProveBatch(keys: Buffer[], com1: Buffer[], blinder1: Buffer[], com2: Buffer[], blinder2: Buffer[], seeds?: Buffer): { proofs: (Buffer | null)[]; status: Int32Array }
    /** zk_distinct_prove_batch: per entry two 32-byte keys, two 72-byte commitments and their 32-byte blinders; seeds must be fresh (default: crypto.randomBytes).  status 14: equal keys; 16: a key and its blinder do not open their commitment */
    distinctProveBatch(key1: Buffer[], com1: Buffer[], blinder1: Buffer[], key2: Buffer[], com2: Buffer[], blinder2: Buffer[], seeds?: Buffer): { proofs: (Buffer | null)[]; status: Int32Array }
    /** zk_distinct_verify_batch */
    distinctVerifyBatch(com1: Buffer[], com2: Buffer[], proofs: Buffer[]): { ok: boolean[]; status: Int32Array }
    /** zk_quorum_prove_batch over the active ring: Q quorums of k members, rows in member order (pk: 64-byte x | y per member); both seed sets must be fresh and independent (default: crypto.randomBytes).  status 14 with every memberStatus 0: two members have the same key */
    quorumProveBatch(k: number, msg: Buffer, sig: Buffer, pk: Buffer, whichs: number[], seeds?: Buffer, pairSeeds?: Buffer): { bundles: (Buffer | null)[]; status: Int32Array; memberStatus: Int32Array }
    /** zk_quorum_verify_batch: firstBad names the first member (< k) or pair (k + p) that failed, 0xFFFFFFFF where ok */
    quorumVerifyBatch(k: number, msg: Buffer, bundles: Buffer[]): { ok: boolean[]; status: Int32Array; firstBad: Uint32Array }
    /** zk_accountable_prove_batch over the active ring under the engine's auditor key: rows in bundle order (pk: 64-byte x | y); both seed sets must be fresh and independent (default: crypto.randomBytes); partStatus: (attestation, tag) per bundle */
    accountableProveBatch(msg: Buffer, sig: Buffer, pk: Buffer, whichs: number[], seeds?: Buffer, tagSeeds?: Buffer): { bundles: (Buffer | null)[]; status: Int32Array; partStatus: Int32Array }
    /** zk_accountable_verify_batch: firstBad is 0 for the attestation, 1 for the tag, 0xFFFFFFFF where ok */
    accountableVerifyBatch(msg: Buffer, bundles: Buffer[]): { ok: boolean[]; status: Int32Array; firstBad: Uint32Array }
    /** zk_rings_accountable_prove_batch: accountableProveBatch with one resident ring id per bundle (whichs[b] indexes ring ringIds[b]); no active ring is read */
    accountableProveBatchRings(msg: Buffer, sig: Buffer, pk: Buffer, whichs: number[], ringIds: number[], seeds?: Buffer, tagSeeds?: Buffer): { bundles: (Buffer | null)[]; status: Int32Array; partStatus: Int32Array }
    /** zk_rings_accountable_verify_batch */
    accountableVerifyBatchRings(msg: Buffer, bundles: Buffer[], ringIds: number[]): { ok: boolean[]; status: Int32Array; firstBad: Uint32Array }
    /** zk_rings_accountable_open_batch: the auditor's call straight on bundles (0xffffffff: any resident ring); it does NOT verify */
    accountableOpenBatchRings(secret32: Uint8Array, bundles: Buffer[], ringIds: number[]): { ring: Uint32Array; index: Uint32Array; status: Int32Array }
    /** zk_accountable_split_batch, pure layout: a refused bundle gives an empty attestation, 472 zero bytes and status 10 */
    accountableSplitBatch(bundles: Buffer[]): { attestations: Buffer[]; tags: Buffer[]; status: Int32Array }
    /** zk_accountable_join_batch, pure layout: null and status 10 where the proof's header or the tag's header is refused */
    accountableJoinBatch(proofs: Buffer[], tags: Buffer[]): { bundles: (Buffer | null)[]; status: Int32Array }
    /** zk_rings_quorum_prove_batch: quorumProveBatch with one RESIDENT ring id per member (whichs[m] indexes ring ringIds[m]); the active ring plays no part */
    ringsQuorumProveBatch(k: number, msg: Buffer, sig: Buffer, pk: Buffer, whichs: number[], ringIds: number[], seeds?: Buffer, pairSeeds?: Buffer): { bundles: (Buffer | null)[]; status: Int32Array; memberStatus: Int32Array }
    /** zk_rings_quorum_verify_batch: quorumVerifyBatch with one RESIDENT ring id per member; an id that is not resident fails its member with status 14 */
    ringsQuorumVerifyBatch(k: number, msg: Buffer, bundles: Buffer[], ringIds: number[]): { ok: boolean[]; status: Int32Array; firstBad: Uint32Array }
    /** zk_link_verify_batch */
    linkVerifyBatch(com1: Buffer[], com2: Buffer[], proofs: Buffer[]): { ok: boolean[]; status: Int32Array }
    /** zk_ctx_set_auditor: the auditor's key as a 72-byte Tom-256 point, for the escrow calls; setParams drops it */
    setAuditor(key72: Uint8Array): void
    /** zk_escrow_keygen: A = a g (72 bytes) for a 32-byte big-endian secret */
    escrowKeygen(secret32: Uint8Array): Buffer
    /** zk_escrow_prove_batch: per entry a 32-byte key, a 72-byte commitment and its 32-byte blinder; seeds must be fresh (default: crypto.randomBytes).  status 16: key and blinder do not open the commitment */
    escrowProveBatch(keys: Buffer[], com: Buffer[], blinder: Buffer[], seeds?: Buffer): { tags: (Buffer | null)[]; status: Int32Array }
    escrowVerifyBatch(com: Buffer[], tags: Buffer[]): { ok: boolean[]; status: Int32Array }
    /** zk_escrow_open_batch against the ACTIVE ring: index 0xffffffff = nobody; it does not verify */
    escrowOpenBatch(secret32: Uint8Array, tags: Buffer[]): { index: number[]; status: Int32Array }
    /** zk_rings_escrow_open_batch: one resident ring id per tag (0xffffffff: any resident ring, ascending ids), through the rings' resident point indexes; the
     *  active ring is not involved.  ring / index 0xffffffff = nobody; it does not verify */
    ringsEscrowOpenBatch(secret32: Uint8Array, tags: Buffer[], ringIds: number[]): { ring: number[]; index: number[]; status: Int32Array }
    /** zk_auditors_split_key: the dealer's Shamir split -> n 32-byte share secrets and n 72-byte share keys; the seed must be fresh (default: crypto.randomBytes) */
    auditorsSplitKey(secret32: Uint8Array, t: number, n: number, seed?: Buffer): { shares: Buffer[]; keys: Buffer[] }
    /** zk_ctx_set_auditors: the share keys of a t-of-n opening, checked against the auditor's key; setAuditor and setParams drop them */
    auditorsSetKeys(t: number, keys: Uint8Array[]): void
    /** zk_auditors_share_batch: auditor j's 264-byte shares of the tags; status 16 at call level: the share secret is not A_j's */
    auditorsShareBatch(j: number, shareSecret32: Uint8Array, tags: Buffer[], seeds?: Buffer): { shares: (Buffer | null)[]; status: Int32Array }
    auditorsShareVerifyBatch(tags: Buffer[], shares: Buffer[]): { ok: boolean[]; status: Int32Array }
    /** zk_auditors_combine_batch: shares[s][b] is auditors[s]'s share of tags[b]; one resident ring id per tag (0xffffffff: any); it does not verify */
    auditorsCombineBatch(auditors: number[], tags: Buffer[], shares: Buffer[][], ringIds: number[]): { ring: number[]; index: number[]; status: Int32Array }
    /** zk_proof_key_commitments: keyXcom of proofs in the engine's wire layout, 72 bytes each; null where the status is not 0 */
    keyCommitments(proofs: Buffer[]): { coms: (Buffer | null)[]; status: Int32Array }
    keysToInts(pkxy: Buffer): { keys: Buffer; status: Buffer }
    proveBatch(msg: Buffer, sig: Buffer, pk: Buffer, which: number[] | Buffer, seeds?: Buffer): Buffer[]
    verifyBatch(msg: Buffer, proofs: Buffer[], seeds?: Buffer): Verdicts
    proveBatchAsync(msg: Buffer, sig: Buffer, pk: Buffer, which: number[] | Buffer, seeds?: Buffer): Promise<Buffer[]>
    /** Streamed form (zk_pool_prove_submit / _wait): up to `inflight` batches inside the engine; `out` is a page-locked Buffer (Engine.hostAlloc) owned by the job until its Promise settles. */
    static hostAlloc(bytes: number): Buffer
    proveStream(msg: Buffer, sig: Buffer, pk: Buffer, which: number[] | Buffer, seeds: Buffer | undefined, out: Buffer): Promise<{ proofs: Buffer[]; status: Int32Array; used: number }>
    verifyStream(msg: Buffer, blob: Buffer, offsets: Buffer, lengths: Buffer, seeds?: Buffer): Promise<{ ok: boolean[]; status: Int32Array }>
    verifyBatchAsync(msg: Buffer, proofs: Buffer[], seeds?: Buffer): Promise<Verdicts>
}
/** Wire layout of the proofs proveSignatureList / proveSignatureListBatch return: 'zka1' (default) or 'zka1p' (33-byte Tom coordinates, 5.3 % fewer bytes; env ZKATTEST_WIRE).
 *  verifySignatureList / ...Batch accept either layout per proof; writeJson gives the same text for both. */
export function setWireLayout(name: 'zka1' | 'zka1p'): void
export function getWireLayout(): 'zka1' | 'zka1p'
/** The level verifySignatureList / ...Batch verify a proof at: 'context' (default; the params' SecLevel, a proof of another count is 'error deserializing')
 *  or 'proof' (the proof's own repetition count, as the reference's verifier does).  Applies to every engine, cached ones included. */
export function setVerifyLevel(name: 'context' | 'proof'): void
export function getVerifyLevel(): 'context' | 'proof'
export function setVerifyReps(name: 'sample' | 'all'): void
export function getVerifyReps(): 'sample' | 'all'
