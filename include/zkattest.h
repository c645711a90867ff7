/*
 * zkattest.h -- C ABI of libzkattest_hip.so, the MI355X (gfx950) engine behind the reference's
 * proveSignatureList / verifySignatureList / generateParamsList API.
 *
 * The reference (cloudflare/zkp-ecdsa, TypeScript) has no FFI layer; its boundary for this path is the ESM
 * surface of src/index.ts:17-19.  Each entry point below names the reference interface it replaces.  A thin
 * N-API addon or the Python mirror in zkp-ecdsa_amd/ binds these symbols.
 *
 * Conventions: caller allocates every buffer; the library never frees caller memory; a context is not
 * re-entrant (one in-flight batch per ctx); several contexts (one per GPU / process) may coexist.  All
 * integers inside byte buffers are big-endian, like the reference's toBytes (src/bignum/big.ts:121-134).
 *
 * Byte formats
 *   P-256 point   64 B  x(32) || y(32)                       (affine; src/curves/weier.ts:244-255 without 0x04)
 *   Tom-256 point 72 B  x(36) || y(36)  zero-padded from the reference's 33-byte coordinates so that every
 *                                         field is 4-byte aligned (src/curves/edwards.ts:194-203)
 *   scalar        32 B
 *   proof         "ZKA1" layout, the binary equivalent of SignatureProofList (src/zkpAttestList.ts:27-60):
 *     header 32 B : "ZKA1" | total_len u32 | secLevel u32 | n = log2(padded ring) u32 | challenge bits (16 B)
 *     R (P), comS1 (P), keyXcom (T), keyYcom (T)
 *     expProof[secLevel], each: A (P), Tx (T), Ty (T), then
 *        challenge bit 1: alpha, beta1 (mod n), beta2, beta3 (mod q)                     (src/exp/exp.ts:171-185)
 *        challenge bit 0: z, z2 (mod n), r1, r2 (mod q), PointAddProof                   (src/exp/exp.ts:186-226)
 *     PointAddProof: C_8, C_10, C_11, C_13 (T), pi_8, pi_10, pi_11, pi_13 (MultProof), pi_x, pi_y (EqualityProof)
 *        MultProof: C_4, A_x, A_y, A_z, A_4_1, A_4_2 (T), t_x, t_y, t_z, t_rx, t_ry, t_rz, t_r4   (src/commit/mult.ts:26-52)
 *        EqualityProof: A_1, A_2 (T), t_x, t_r1, t_r2                                              (src/commit/equality.ts:27-40)
 *     GKProof: cl[n], ca[n], cb[n], cd[n] (T), f[n], za[n], zb[n], zd                              (src/proofGK/gk.ts:31-58)
 *   membership proof on its own  "ZKM1" layout, the binary equivalent of a bare GKProof (src/proofGK/gk.ts:31-58; zk_member_* below):
 *     header 16 B : "ZKM1" | total_len u32 | n = log2(padded ring) u32 | 0 u32
 *     GKProof: cl[n], ca[n], cb[n], cd[n] (T), f[n], za[n], zb[n], zd      -- byte for byte the GKProof section of a ZKA1 proof
 *     total_len = 16 + 288 n + 32 (3 n + 1): fixed per ring (6 192 B at n = 16).  Always 36-byte coordinates (zk_ctx_set_wire plays no part).  The commitment
 *     the proof is about is not part of it: it travels beside the proof as one Tom-256 point.
 *   bound membership proof  "ZKMB": the ZKM1 layout and size under the magic "ZKMB"; its challenge also hashes a statement (zk_member_*_bound below).
 *
 * Randomness contract (replaces crypto.getRandomValues in src/bignum/big.ts:171-181): the k-th 32-byte fill
 * of proof b is SHA-256(seed_b || be64(k)) (ZK_RNG_SEED) or block k of a caller-supplied stream
 * (ZK_RNG_STREAM); fills are consumed in the reference's draw order.
 */
#ifndef ZKATTEST_H
#define ZKATTEST_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct zk_ctx zk_ctx;
typedef int32_t zk_status;

/* call-level and per-proof status codes; the per-proof ones mirror the reference's thrown errors */
enum {
    ZK_OK = 0,
    ZK_E_POINT_NOT_IN_GROUP = 1, /* 'point not in group'            src/curves/weier.ts:83 */
    ZK_E_INVALID_KEY = 2,        /* 'invalid public key'            src/zkpAttestList.ts:117 */
    ZK_E_T_INF = 3,              /* 'T[i] is at infinity'           src/exp/exp.ts:151 */
    ZK_E_T1_INF = 4,             /* 'T1 is at infinity'             src/exp/exp.ts:193 */
    ZK_E_PADD_INF = 5,           /* 'P/Q/R is at infinity'          src/exp/pointAdd.ts:117-125 (no input reaches it) */
    ZK_E_POINTS_DONT_ADD = 6,    /* "Points don't add up!"          src/exp/pointAdd.ts:105 (a signature with r = 0 mod n: invMod(0) = 0) */
    ZK_E_R_INF = 7,              /* 'R is at infinity'              src/zkpAttestList.ts:159 */
    ZK_E_PARAMS_NOT_FOUND = 8,   /* 'params not found'              src/exp/exp.ts:270,302 */
    ZK_E_SECLEVEL = 9,           /* 'security level not achieved'   src/exp/exp.ts:244 */
    ZK_E_BAD_ENCODING = 10,      /* deserialisation failures        src/curves/weier.ts:87,258, edwards.ts:84,207 */
    ZK_E_RNG_EXHAUSTED = 11,     /* stream too short / too many rejected fills */
    ZK_E_BUFFER = 12,            /* output buffer too small, or context not configured */
    ZK_E_INTERPOLATION = 13,     /* 'incorrect interpolation'       src/proofGK/interpolate.ts:65 */
    ZK_E_ARG = 14,               /* invalid argument */
    ZK_E_DEVICE = 15,            /* HIP runtime failure (zk_last_error has the text) */
    ZK_E_OPENING = 16            /* zk_proof_rering_batch: ring[which_new] and the blinder do not open the proof's keyXcom; zk_link_prove_batch: the key and a
                                    blinder do not open com1 or com2 */
};

enum { ZK_RNG_SEED = 0, ZK_RNG_STREAM = 1 };
typedef struct {
    int32_t mode;           /* ZK_RNG_SEED: data = B x 32-byte seeds; ZK_RNG_STREAM: data = B x stride_blocks x 32 bytes */
    const uint8_t *data;
    uint64_t stride_blocks; /* ZK_RNG_STREAM only */
} zk_rng;

/* Creates an engine bound to one GPU.  Owns the HIP streams, the fixed-base tables and the workspace.  (SURVEY.md section 8(b)
 * sketched zk_ctx_create(device_ids, n_dev); here one zk_ctx is one GPU and zk_pool_create below takes the device list.) */
zk_status zk_ctx_create(int device_id, zk_ctx **out);   /* *out = NULL on failure (never a half-built context) */
void zk_ctx_destroy(zk_ctx *ctx);
const char *zk_strerror(zk_status s);
const char *zk_last_error(const zk_ctx *ctx);           /* ctx = NULL: why this thread's last zk_ctx_create failed */

/* Replaces SystemParametersList as produced by generateParamsList (src/zkpAttestList.ts:88-92,62-78):
 * NistGroup.h, ProofGroup.g, ProofGroup.h and SecLevel.  Builds the fixed-base tables for g, h, G, h_NIST. */
zk_status zk_ctx_set_params(zk_ctx *ctx, const uint8_t nist_h[64], const uint8_t tom_g[72], const uint8_t tom_h[72], uint32_t sec_level);

/* Replaces the `keys: bigint[]` argument (src/zkpAttestList.ts:110,150): n_keys big-endian 32-byte scalars.
 * Pads to the next power of two with copies of keys[0] (src/proofGK/gk.ts:75-86).  The _device variant takes a
 * pointer already resident on this context's GPU (e.g. the target of an RCCL broadcast).
 * n_keys >= 2.  A ONE-key ring is refused with ZK_E_ARG: the reference cannot prove over it either -- the padded length is 1, n = 0, and
 * proveMembership's interpolate([], []) evaluates `-x[0] % m` with x[0] undefined (src/proofGK/interpolate.ts:40), a TypeError
 * ("Cannot mix BigInt and other types") for every `which` -- so no proof over such a ring exists to be verified; the facade throws that
 * TypeError.  `which` (zk_prove_batch) indexes the PADDED ring: [0, n_keys) are the caller's keys, [n_keys, N) the padding copies of keys[0]
 * (the owner of keys[0] may name any of them; the index bits enter the proof), and which >= N is per-proof status ZK_E_ARG, the
 * reference's `values[index].k` on undefined (gk.ts:162; proveMembership runs last, so an invalid key and 'T[i] is at infinity' are
 * reported in its place when they apply too; 'T1 is at infinity' -- a planted nonce and a bad index in one call -- is not). */
zk_status zk_ctx_set_ring(zk_ctx *ctx, const uint8_t *keys_be32, uint64_t n_keys);
zk_status zk_ctx_set_ring_device(zk_ctx *ctx, const void *d_keys_be32, uint64_t n_keys);

/* keyToInt (src/zkpAttestList.ts:94-102) for a whole key set: n_keys public keys as 64-byte affine (x, y) big-endian
 * (the WebCrypto 'raw' export without its 0x04 prefix) -> n_keys 32-byte big-endian ring entries (the x coordinate,
 * reduced mod p like toAffine does).  per_key_status[i] = ZK_E_POINT_NOT_IN_GROUP where deserializePoint would throw
 * (src/curves/weier.ts:74-89: curve equation mod p, coordinates not range-checked); such entries are written as zero.
 * Host pointers; the return value is ZK_OK even if some keys are bad (check the statuses). */
zk_status zk_keys_to_ints(zk_ctx *ctx, uint64_t n_keys, const uint8_t *pk_xy64, uint8_t *keys_be32, int32_t *per_key_status);

/* Proofs processed per pipeline pass (workspace grows linearly with it: about 0.9 MB per proof at secLevel 80).
 * Default 4096, maximum 2^18. */
zk_status zk_ctx_set_chunk(zk_ctx *ctx, uint32_t proofs_per_chunk);

/* Pipeline lanes (1..4, default 2; ZKATTEST_LANES): consecutive chunks rotate over that many HIP streams and workspaces, so the
 * low-occupancy per-proof kernels, the host's waits and (host-pointer calls) the output phases of one chunk overlap the heavy
 * kernels of the others; 1 = strictly serial kernels (what bench.py uses for its per-kernel roofline pass).  Every lane holds
 * a workspace of `chunk` proofs. */
zk_status zk_ctx_set_lanes(zk_ctx *ctx, uint32_t lanes);
/* (The lane-scheduling experiments of round 5 -- a "heavy queue", stream priorities, CU masks, staggered starts: none beat this default -- are recorded in
 * profiles/r05_overlap.txt; their switches are gone from the library.) */
/* Width W (8..26 bits, default 16) of the fixed-base comb tables of the Tom-256 bases g and h: a commitment
 * v*g + r*h (PedersenParams.commit, src/commit/pedersen.ts:53-58) costs 2*ceil(256/W) table additions, the tables
 * take 2 * ceil(256/W) * 2^W * 128 bytes of HBM (0.27 GB at 16, 3.5 GB at 20, 47 GB at 24); 25 and 26 select SIGNED
 * digits (half the entries per window): 25 = the 22 additions of 24 bits in 23.6 GB, 26 = 20 additions in 86 GB.  They are rebuilt by the
 * next zk_ctx_set_params, which must follow.  The proof bytes do not depend on W.  The environment variable
 * ZKATTEST_COMB_BITS sets the default of new contexts. */
zk_status zk_ctx_set_comb_bits(zk_ctx *ctx, uint32_t bits);

/* zk_prove_batch on a page-locked `out`: 1 (default) = the first chunks of the L lanes hold chunk/L, 2*chunk/L, ... proofs, so
 * the lanes run out of phase and their output phases (PCIe transfers) interleave; 0 = uniform chunks; n >= 2 = n rising first
 * chunks (chunk/n, 2*chunk/n, ...) whatever the number of lanes.  The proof bytes do not depend on it. */
zk_status zk_ctx_set_host_taper(zk_ctx *ctx, uint32_t on);
/* The prover runs a chunk's PointAdd phase (src/exp/pointAdd.ts:92-163: 80 % of the proof bytes) in slices of `proofs`
 * consecutive proofs; with a page-locked `out` every slice is followed by the DMA of the proofs it completed.  0 (default) =
 * 4096 for page-locked output (512 / 1024 in the small chunks of short calls -- one chunk of at most 2048 / 8192 proofs, or chunks
 * of at most 2048 / 4096 in a call of at most 32768 -- whose output's transfer is a large part of their time), no slicing otherwise; at least 64.  The proof bytes do not depend on it. */
zk_status zk_ctx_set_slice(zk_ctx *ctx, uint32_t proofs);

/* Verifier strategy for the Tom-256 relations: in a chunk of at least min_chunk proofs (default 256) the relations of ALL
 * proofs are checked with one bucket-method multi-scalar sum (independent 128-bit multipliers per relation and per proof);
 * a chunk is cut into 8 (or 64: zk_ctx_set_verify_groups) contiguous groups of proofs whose sums come out of the same pass, and only
 * the groups whose sum is not the identity -- some proof of theirs is bad -- go through the per-proof sums to tell which.  ok[] and the
 * statuses are the same either way; a forged proof costs the per-proof sums of its group, and the chunk-wide sum has a fixed
 * cost of a few milliseconds, hence the threshold.  0 = never, 1 = always.  (ZKATTEST_VERIFY_BATCH)
 * Chunks of at least 8192 proofs (ZKATTEST_P256_BATCH, read by zk_ctx_create; 0 = never) that take this path sum their P-256 relations the same way, per group,
 * beside the Tom-256 sums; if a group's P-256 total is not the identity the chunk's P-256 relations are checked per proof (zk_test_counter 3 counts the
 * proofs settled by the pass). */
zk_status zk_ctx_set_batch_verify(zk_ctx *ctx, uint32_t min_chunk);
/* Groups per chunk of that check: 8 (default; 16-bit windows) or 64 (13-bit windows: 25 % more bucket additions and four more sorts on
 * every chunk -- about 8 % of the device-resident verification rate at the headline shape, nothing where the PCIe link is the
 * bound -- for a forged proof that costs a 64th of its chunk instead of an eighth).  Verdicts and statuses do not depend on it.
 * (ZKATTEST_VERIFY_GROUPS) */
zk_status zk_ctx_set_verify_groups(zk_ctx *ctx, uint32_t groups);

/* Per-key tables (default on; rings of up to 65 536 keys): zk_ctx_set_ring stores 128 multiples x 33 byte positions of EVERY ring key
 * (264 KB per key, 17.7 GB at 2^16 keys, built in ~0.1 s), so that the prover's u2 * publicKey (src/zkpAttestList.ts:129-131) and the
 * alpha_i * R of proveExp (src/exp/exp.ts:144-149, as (alpha_i u1) * G + (alpha_i u2) * publicKey) are sums of 33 gathered entries instead of
 * a doubling chain and a per-proof table of R.  A proof whose `which` names a ring value that is not its own key's x-coordinate takes
 * the per-proof path; the bytes are the same either way.  0 = per-proof tables for every proof.  Call before zk_ctx_set_ring.
 * (ZKATTEST_KEYTAB) */
zk_status zk_ctx_set_key_tables(zk_ctx *ctx, uint32_t on);

/* The ring fold's 8 low index bits on the matrix cores (v_mfma_i32_16x16x64_i8; rings of at least 4096 keys), 1 (default), or as
 * 64-bit multiply-adds on the vector ALU, 0.  Verifier: verifyMembership's total (src/proofGK/gk.ts:239-250), every block of 256 keys
 * as int8 matrix products (ZKATTEST_GK_MFMA).  Prover: the table path's coefficient classes 2..6 of proveMembership's polynomial
 * (gk.ts:141-171), per group of proofs with equal low index bits; its operand table (0.83 GB at 2^16 keys, 13 GB at 2^20) is built
 * by zk_ctx_set_ring unless ZKATTEST_GK_MFMA_PROVE=0.  Exact integer arithmetic either way: same proofs, totals and verdicts.
 * Takes effect with the next prove / verify call.
 * Every zk_ctx_set_* above returns ZK_E_ARG while streamed jobs are queued on the context (zk_prove_submit below): a queued job keeps
 * the lanes, chunk size, workspaces and mode it was planned with. */
zk_status zk_ctx_set_ring_fold(zk_ctx *ctx, uint32_t matrix_pipe);

/* Wire layout of the proofs (default ZK_WIRE_ZKA1).  ZK_WIRE_ZKA1P is ZKA1 with every Tom-256 coordinate in the reference's own 33 bytes
 * instead of 36 (src/curves/edwards.ts:194-203) and the magic "ZK1P": every run of Tom points in the layout holds an even number of points, so
 * all other fields stay 4-byte aligned; 5.3 % fewer bytes (160.0 instead of 169.0 KB per proof at secLevel 80, n = 16), which is what the
 * host-pointer entry points are bound by (PCIe).  The prover's writers emit the chosen layout directly (every entry point, device pointers
 * included); the verifier expands packed proofs on the device, chunk by chunk, before its unchanged kernels read them (every entry point; a
 * device-pointer call reads one offset per chunk back first).  Verdicts and statuses are those of the ZKA1 form of the same proofs.
 * zk_proof_pack / zk_proof_unpack convert single proofs on the host; the JSON converters accept both layouts and write ZKA1. */
enum { ZK_WIRE_ZKA1 = 0, ZK_WIRE_ZKA1P = 1 };
zk_status zk_ctx_set_wire(zk_ctx *ctx, uint32_t wire);
/* host-side conversions of ONE proof; *out_len is always set to the required size, ZK_E_BUFFER when out_cap is too small, ZK_E_BAD_ENCODING
 * when the input is not a structurally complete proof of its layout (header, length, challenge bits) */
zk_status zk_proof_pack(const uint8_t *zka1, uint64_t len, uint8_t *out, uint64_t out_cap, uint64_t *out_len);
zk_status zk_proof_unpack(const uint8_t *zka1p, uint64_t len, uint8_t *out, uint64_t out_cap, uint64_t *out_len);

/* Upper bound of one proof's size, in the context's wire layout, for the current params/ring. */
uint64_t zk_proof_max_size(const zk_ctx *ctx);

/* The same for a resident ring that need not be active (what zk_prove_batch_rings can write per proof of that ring); 0 for an id that is not resident. */
uint64_t zk_ring_proof_max_size(const zk_ctx *ctx, uint32_t ring);

/* Page-locked host memory for the big buffers of the host-pointer entry points (`out` of zk_prove_batch, `proofs` of
 * zk_verify_batch: ~169 KB per proof at secLevel 80).  With such a buffer the proof bytes move by DMA chunk by chunk while
 * the neighbouring chunks are being proved / verified; with ordinary (pageable) memory the runtime stages one blocking copy
 * through its own bounce buffers (measured 8.6 GB/s, several times the proving time).  Memory that the caller page-locked
 * itself (hipHostMalloc, hipHostRegister) is recognised too.  NULL when the allocation fails. */
void *zk_host_alloc(size_t bytes);
void zk_host_free(void *p);

/* Replaces B calls of proveSignatureList(params, msgHash, sigBytes, publicKey, which, keys)
 * (src/zkpAttestList.ts:104-145).  pk_xy is the WebCrypto 'raw' export without its 0x04 prefix.
 * out receives the proofs back to back; out_off[b]..out_off[b+1] delimits proof b (empty when
 * per_proof_status[b] != 0).  Host pointers; `out` from zk_host_alloc is filled by overlapped DMA.  `out` may also be memory of
 * this context's GPU (hipMalloc): the proofs then stay in HBM and only the inputs cross the link. */
zk_status zk_prove_batch(zk_ctx *ctx, uint64_t B, const uint8_t *msg_hash /*Bx32*/, const uint8_t *sig /*Bx64*/,
                         const uint8_t *pk_xy /*Bx64*/, const uint32_t *which /*B*/, const zk_rng *rng,
                         uint8_t *out, uint64_t out_cap, uint64_t *out_off /*B+1*/, int32_t *per_proof_status /*B*/);

/* Same, every pointer (including rng->data) resident in this GPU's HBM; nothing crosses PCIe.  Synchronous. */
zk_status zk_prove_batch_device(zk_ctx *ctx, uint64_t B, const void *d_msg_hash, const void *d_sig, const void *d_pk_xy,
                                const void *d_which, const zk_rng *rng_device, void *d_out, uint64_t out_cap,
                                void *d_out_off /*u64[B+1]*/, void *d_per_proof_status /*i32[B]*/);

/* Replaces B calls of verifySignatureList(params, msgHash, keys, proof) (src/zkpAttestList.ts:147-184):
 * ok[b] = 1 iff the reference verifier returns true; per_proof_status[b] != 0 mirrors a thrown error
 * ('params not found', 'T is at infinity', deserialisation failures ...), in which case ok[b] = 0.
 * The reference verifier is randomised: it checks a random 20-subset of the secLevel reps (src/exp/exp.ts:95-109,
 * 261-264).  verifier_seeds (B x 32 bytes, may be NULL) fixes that choice under the same contract as the prover's
 * RNG: verifier fill k = SHA-256(seed_b || be64(k)), randomScalar() consumes a 32-byte fill, rnd(small) the first
 * byte of a fill; fills are consumed in the reference's order (2n+1 randomScalar draws of verifyMembership, then
 * generateIndices).  The random multipliers of Relation.drain (src/curves/multimult.ts:168-173) do not influence the
 * boolean; the engine draws its own 128-bit ones (from the same seed).  The seeds must be unpredictable to whoever made
 * the proofs and independent across proofs.  NULL: the engine draws fresh OS randomness for the call (what the
 * reference does with crypto.getRandomValues); pass seeds only to reproduce a run.
 * proofs must be packed back to back (proof_off[0] = 0, 4-byte aligned).  Host pointers; `proofs` from zk_host_alloc is
 * read by overlapped DMA.
 * Non-canonical encodings: a P-256 coordinate in [p, 2^256) is accepted where deserializePoint accepts it (the curve equation is
 * checked mod p, src/curves/weier.ts:74-89) and enters the Fiat-Shamir hashes REDUCED, as toBytes -> toAffine does
 * (src/curves/weier.ts:231-255).  Tom-256 coordinates must be canonical (< the field prime, zero padding bytes): ZKA1 is this
 * engine's format and is stricter here than the reference's JSON reader, which reduces out-of-range values silently
 * (src/curves/edwards.ts:204-209); such a proof gets ZK_E_BAD_ENCODING.
 * Status codes are exact (tests/test_gpu_mutants.py: seeded mutants, engine == oracle): ZK_E_BAD_ENCODING for anything that does not
 * deserialise -- magic, lengths, a header n above 63, challenge bits set above secLevel, any point of the announced structure off its
 * curve, also inside a GKProof of the wrong length --; ok = 0 with status 0 where the reference returns false (membership, a GKProof
 * whose length is not the ring's, gk.ts:208-218, a failed relation); otherwise the exception verifyExp throws FIRST when it walks
 * the 20 sampled repetitions in order (exp.ts:265-346): ZK_E_PARAMS_NOT_FOUND, ZK_E_T_INF or ZK_E_T1_INF.  ZK_E_R_INF cannot occur (R
 * travels in affine form).  One restriction in the default mode (ZK_VERIFY_LEVEL_CONTEXT): a batch is homogeneous in secLevel -- a proof
 * whose header announces another repetition count than the context's gets ZK_E_BAD_ENCODING, where the reference would verify it with
 * its own count (exp.ts:243-260); a context with secLevel < 20 refuses the call with ZK_E_SECLEVEL.  zk_ctx_set_verify_level below lifts
 * it: in ZK_VERIFY_LEVEL_PER_PROOF every proof is verified at its own header's count, as the reference does. */
zk_status zk_verify_batch(zk_ctx *ctx, uint64_t B, const uint8_t *msg_hash /*Bx32*/, const uint8_t *proofs,
                          const uint64_t *proof_off /*B+1*/, const uint8_t *verifier_seeds /*Bx32 or NULL*/,
                          uint8_t *ok /*B*/, int32_t *per_proof_status /*B*/);
zk_status zk_verify_batch_device(zk_ctx *ctx, uint64_t B, const void *d_msg_hash, const void *d_proofs,
                                 const void *d_proof_off, const void *d_verifier_seeds, void *d_ok, void *d_per_proof_status);

/* Verify levels.  ZK_VERIFY_LEVEL_CONTEXT (default): every proof is verified at the context's secLevel (zk_verify_batch above).
 * ZK_VERIFY_LEVEL_PER_PROOF: the reference's verifySignatureList never reads the caller's SecLevel -- verifyExp(..., 20, Q) hashes every
 * repetition the proof holds and samples generateIndices(20, count) (src/zkpAttestList.ts:147-184, src/exp/exp.ts:233-262) -- and neither
 * does the engine in this mode: a proof's level is its header's secLevel field, 0..128 (above 128: ZK_E_BAD_ENCODING, the header holds 128
 * challenge bits), and everything checked in the default mode is checked against that count.  Per proof, in the reference's order:
 * ZK_E_BAD_ENCODING for a structural error; ok 0 / status 0 where membership fails; ZK_E_SECLEVEL for fewer than 20 repetitions (only the
 * membership proof of such a proof is verified); otherwise verifyExp's verdict and exceptions at the proof's count.  The verifier-seed
 * contract is unchanged, per proof (2n+1 fills for membership, then count - 2 for generateIndices(20, count)).  Every verify entry point
 * (host, page-locked, HBM and device-pointer proofs, submit / wait, the pool calls) and both wire layouts and protocol modes follow it.
 * How: a census of the batch's levels -- the headers read on the host for host-pointer calls; for zk_verify_batch_device one kernel and
 * ONE read-back of 130 counters per call.  A batch whose well-formed proofs share one level runs the usual pipeline planned at that level
 * (workspaces grow to it and are never shrunk; the next prove call plans at the context's level again).  A batch of several levels is
 * split: the proofs of each level are gathered on the device into a window of at most 2 x chunk x lanes proofs (zk_ctx_set_chunk,
 * zk_ctx_set_lanes), verified there, and their verdicts scattered back to their indices; host-pointer mixed batches first copy their
 * bytes to HBM in one transfer.  A streamed job (zk_verify_submit) whose proofs are all at the level of the jobs already queued is
 * queued as usual; any other job (several levels, a level below 20, another level) waits for the queue ahead of it to drain and runs at
 * its zk_verify_wait like the synchronous call -- the results are the same.  The setter follows the rules of the other zk_ctx_set_*
 * (takes effect with the next call; ZK_E_ARG while streamed jobs are queued, or for an unknown mode).  zk_pool_set_verify_level sets the
 * mode of every shard context. */
enum { ZK_VERIFY_LEVEL_CONTEXT = 0, ZK_VERIFY_LEVEL_PER_PROOF = 1 };
zk_status zk_ctx_set_verify_level(zk_ctx *ctx, uint32_t mode);

/* Verified repetitions.  ZK_VERIFY_REPS_SAMPLE (default): the 20-subset above -- generateIndices(20, count) from the verifier's seed, as
 * verifySignatureList does (src/zkpAttestList.ts:177, `// TODO: raise!`); one broken repetition out of 80 is then missed with probability
 * 60/80.  ZK_VERIFY_REPS_ALL: every repetition the proof holds is checked.  The semantics are verifySignatureList with
 * verifyExp(..., secparam = pi.length, Q) and the repetitions walked in ascending index order in place of a random permutation.  Per proof,
 * in order: ZK_E_BAD_ENCODING for a structural error (exactly the default mode's); ok 0 / status 0 where membership fails; ZK_E_SECLEVEL
 * below 20 repetitions (the context's level, or the header's in ZK_VERIFY_LEVEL_PER_PROOF -- as in the default mode); otherwise the
 * exception of the LOWEST-index repetition that throws -- ZK_E_PARAMS_NOT_FOUND where its header bit disagrees with the recomputed
 * challenge bit, ZK_E_T_INF / ZK_E_T1_INF where its point is the identity, the type looked at before the point --; otherwise ok = 1 if and
 * only if every relation of every repetition holds.  This is STRICTER than the reference: a proof it accepts under some seed may be
 * rejected here.  The verifier-seed contract keeps its 2n+1 membership fills; generateIndices draws nothing; the engine's 128-bit
 * randomisers still come from the seed, and the passes below reuse them.
 * How: P = ceil(count / 20) passes over the sampled verifier's pipeline at the level the call is planned for.  Pass r < P - 1 checks
 * repetitions 20 r .. 20 r + 19, the last pass count - 20 .. count - 1 (it overlaps the one before it where 20 does not divide count); the
 * verdicts are merged as ok &= ok_r, status = status ? status : status_r.  Each pass repeats the challenge hashes, R's table and the
 * membership check, so a call costs about P sampled calls.  Independent of zk_ctx_set_verify_level (each level's window runs its own P),
 * of the wire layout (ZKA1P input is expanded once) and of the protocol mode.  Every blocking verify entry point follows it
 * (zk_verify_batch, zk_verify_batch_device, the _rings forms, the pool's blocking calls); a host-pointer call of more than one pass first
 * copies its proofs to HBM in one transfer.  zk_last_timing reports the families summed over the passes, plus "v_merge".
 * Not provided: streamed variants -- zk_verify_submit returns ZK_E_ARG in this mode.
 * The setter follows the rules of zk_ctx_set_verify_level (takes effect with the next call; ZK_E_ARG while streamed jobs are queued, or for
 * an unknown mode).  zk_pool_set_verify_reps sets the mode of every shard context. */
enum { ZK_VERIFY_REPS_SAMPLE = 0, ZK_VERIFY_REPS_ALL = 1 };
zk_status zk_ctx_set_verify_reps(zk_ctx *ctx, uint32_t mode);

/* Resident rings.  The reference takes the ring as an argument of every call (proveSignatureList / verifySignatureList,
 * src/zkpAttestList.ts:104-184); a context keeps up to ZK_MAX_RINGS rings built at once, so that a verifier serving several key sets
 * never rebuilds one (a rebuild costs tens of milliseconds at 2^16 keys, a verification ~1.5 ms).  Exactly one of them, or none, is ACTIVE:
 * every prove, verify, submit and pool entry point, zk_ring_digest and zk_proof_max_size work on the active ring, and a context whose
 * rings are all inactive answers like a context without a ring.
 * zk_ctx_add_ring[_device] builds a new ring (padding, the one-key refusal and the bounds of zk_ctx_set_ring) and returns its id in *ring;
 * ids are never reused within a context.  It does not make the ring active.  Every table beyond the ring's limbs and digest is optional
 * (table E, the digit planes, the per-key tables): what does not fit is skipped and zk_ring_info's flags say so; the call fails only where
 * the limbs themselves cannot be allocated.  When a later workspace does not fit, the key tables of the rings the call does not use are
 * given up first, then those of the ring it runs on -- same bytes and verdicts, slower proving.
 * zk_ctx_use_ring makes a ring active: host work only, no allocation and no kernel.  zk_ctx_set_ring[_device] (re)builds the ACTIVE ring in
 * place and keeps its id; on a context without an active ring it creates one (ring 0 on a fresh context) and makes it active.
 * zk_ctx_drop_ring frees a ring; dropping the active ring is refused.  zk_ring_info: the ring's key count before padding, n = log2 of the
 * padded size, ZK_RING_* flags and a generation counter that every build of the ring increments (use_ring does not).
 * All four return ZK_E_ARG for an id that is not resident and while streamed jobs are queued on the context, like the zk_ctx_set_*.
 * zk_pool_add_ring / use_ring / drop_ring do the same on every shard context with the same id (a shard that fails to add drops it again on
 * the others). */
#define ZK_MAX_RINGS 16
enum {
    ZK_RING_TABLE_E = 1,          /* table E of the GK block transform (rings of 2^8 .. 2^20 keys) */
    ZK_RING_DIGIT_PLANES = 2,     /* the ring as int8 digit planes: the verifier's ring fold on the matrix pipe (rings of >= 2^12 keys) */
    ZK_RING_TABLE_E_DIGITS = 4,   /* table E as digit planes: the prover's matrix-pipe table path */
    ZK_RING_KEY_TABLES = 8,       /* per-key tables (zk_ctx_set_key_tables) */
    ZK_RING_ACTIVE = 16           /* the context's active ring */
};
zk_status zk_ctx_add_ring(zk_ctx *ctx, const uint8_t *keys_be32, uint64_t n_keys, uint32_t *ring);
zk_status zk_ctx_add_ring_device(zk_ctx *ctx, const void *d_keys_be32, uint64_t n_keys, uint32_t *ring);
zk_status zk_ctx_use_ring(zk_ctx *ctx, uint32_t ring);
zk_status zk_ctx_drop_ring(zk_ctx *ctx, uint32_t ring);
zk_status zk_ring_info(zk_ctx *ctx, uint32_t ring, uint64_t *n_keys, uint32_t *log_n, uint32_t *flags, uint64_t *generation);

/* Updating a resident ring in place.  A registry of attested keys gains a few keys, rotates one, revokes one; rebuilding the ring for that redoes every table
 * of N keys.  Every table of a ring is indexed by key or by block of 256 keys, so zk_ctx_update_ring rewrites only what the change touches: k limbs, k per-key
 * tables, the touched blocks of table E and of the two digit tables, their leaves of the digest and its root -- through the SAME kernels as the full build,
 * handed an index list, so the result is bit for bit what zk_ctx_set_ring of the new list builds.  The reference has no counterpart (it takes `keys` with every
 * call); it fixes the semantics: afterwards the context behaves exactly as if it had been given the new key list.
 *   L = the ring's n_keys caller keys.  The new list L' has new_n_keys entries: L'[i] = the LAST keys_be32[j] with index[j] == i, else L[i].  new_n_keys > n_keys
 *   appends (every index in [n_keys, new_n_keys) must be supplied); new_n_keys < n_keys truncates (the dropped tail becomes padding, copies of L'[0]).
 *   The id and the active / inactive state stay, zk_ring_info reports new_n_keys, the generation goes up by one.  count == 0 with new_n_keys == n_keys is a
 *   no-op (ZK_OK, generation unchanged).
 * Same padded size (the next power of two): the tables are patched in place, no table is reallocated and none that was absent is created; the per-key tables of
 * padding entries are copied from entry 0's.  The padded size changes: the ring is rebuilt from the assembled list like zk_ctx_add_ring builds it.
 * ZK_E_ARG, nothing written, zk_last_error set: NULL arguments, an id that is not resident, new_n_keys < 2, an index >= new_n_keys, an appended position without
 * a key, streamed jobs queued on the context.  A HIP failure after the first write returns ZK_E_DEVICE and DROPS the ring (a context whose active ring this was
 * has none afterwards): a half-updated ring never stays resident.  A ZK_E_DEVICE from BEFORE the first write (the update's temporary memory, its upload) leaves
 * the ring of a single context unchanged -- zk_last_error says which of the two happened, zk_ring_info whether the id is still resident.  All pointers are host pointers.
 * zk_pool_update_ring: the same on every shard context, concurrently; if a shard fails on its device -- before or after its first write -- the ring is dropped on
 * all of them, so that no shard serves a ring the others lost or did not update. */
zk_status zk_ctx_update_ring(zk_ctx *ctx, uint32_t ring, uint64_t count, const uint64_t *index /*count*/, const uint8_t *keys_be32 /*count x 32*/,
                             uint64_t new_n_keys);

/* Mixed-ring verification: zk_verify_batch[_device] with one resident ring id per proof.  A proof whose id is not resident gets ok 0 and
 * ZK_E_ARG; every other proof gets exactly the (ok, status) zk_verify_batch gives it with that ring active -- both wire layouts, hardened
 * mode with each ring's own digest, per-proof verify levels.  The active ring is neither read nor changed.  How: the proofs are classed by
 * (ring, level) -- on the host for host-pointer calls, by one census kernel and ONE read-back of the per-class counters for the device
 * call; a batch of one class runs the usual pipeline on the caller's buffers with that ring bound, several classes are gathered class by
 * class into windows of at most 2 x chunk x lanes proofs, verified there and their verdicts scattered back (a host-pointer batch of several
 * classes first copies its bytes to HBM in one transfer).  zk_pool_verify_batch_rings shards by contiguous proof ranges like
 * zk_pool_verify_batch; the ids are those of zk_pool_add_ring. */
zk_status zk_verify_batch_rings(zk_ctx *ctx, uint64_t B, const uint8_t *msg_hash /*Bx32*/, const uint8_t *proofs, const uint64_t *proof_off /*B+1*/,
                                const uint32_t *ring_ids /*B*/, const uint8_t *verifier_seeds /*Bx32 or NULL*/, uint8_t *ok /*B*/,
                                int32_t *per_proof_status /*B*/);
zk_status zk_verify_batch_rings_device(zk_ctx *ctx, uint64_t B, const void *d_msg_hash, const void *d_proofs, const void *d_proof_off,
                                       const void *d_ring_ids, const void *d_verifier_seeds, void *d_ok, void *d_per_proof_status);

/* Mixed-ring proving: zk_prove_batch[_device] with one resident ring id per proof -- the reference takes `keys` with every proveSignatureList call
 * (src/zkpAttestList.ts:104-145); this is that interface over a batch.  Proof b and per_proof_status[b] are byte for byte what zk_prove_batch returns for
 * input b with ring ring_ids[b] active, under the same randomness contract (fill k of proof b depends on b's own seed or stream only): which[b] indexes THAT
 * ring's padded size, every per-proof status of the one-ring call appears unchanged and touches no neighbour, both wire layouts and hardened mode (each ring
 * with its own digest) are honoured, and the per-key tables are used where the proof's ring has them.  A proof whose id is not resident gets ZK_E_ARG and an
 * empty proof.  The proofs lie in `out` back to back in index order, out_off[0] = 0: the result can be handed to zk_verify_batch_rings with the same ring_ids
 * as it is.  `out` may be pageable, page-locked or HBM of the context's device, as for zk_prove_batch; ZK_E_BUFFER when out_cap is too small (no proof is
 * larger than zk_proof_max_size with the batch's largest ring active).  The active ring is neither read nor changed, and a context whose rings are all
 * inactive can prove.  ZK_E_BUFFER before zk_ctx_set_params, ZK_E_ARG for NULL arguments and while streamed jobs are queued; there are no streamed variants.
 * How: the ids are classed -- on the host for host-pointer calls, by one census kernel and ONE read-back of its counters for the device call.  A batch of one
 * ring runs the usual pipeline on the caller's buffers with that ring bound and nothing else.  Otherwise the batch is cut into index-contiguous segments
 * (multiples of 256 proofs) whose proofs fit a grow-only staging buffer in HBM (8 GiB of proofs at most; it is an optional workspace like the lanes': the
 * per-key tables are given up before it); per segment and ring, windows of at most 2 x chunk x lanes proofs are gathered (inputs and seeds, or the
 * proof's whole stream in ZK_RNG_STREAM mode), proved with their ring bound into the staging buffer, and -- a proof's size being known only once it is
 * made -- one scan over the segment's lengths in index order writes out_off and one kernel moves the bytes to their final place behind the previous
 * segment's; with a page-locked `out` a finished segment crosses the link while the next one is proved.  zk_test_counter 7 / 8 count the segments and
 * windows.  The gathered signatures, seeds and streams are witness-derived: zk_ctx_wipe, zk_ctx_destroy and a failed call zero them.
 * Memory of a mixed batch beyond the one-ring call's: the staging buffer (at most 8 GiB, or 256 of the largest proofs), the window's inputs (2 x chunk x lanes x
 * 196 bytes; in ZK_RNG_STREAM mode 2 x chunk x lanes whole streams, 32 x stride_blocks bytes each -- 1.9 GB at the default chunk and lanes, secLevel 80), and, for
 * host pointers, the whole batch's inputs in HBM at once (B streams in ZK_RNG_STREAM mode: callers of that mode bound B themselves); all grow-only.
 * zk_pool_prove_batch_rings: zk_pool_prove_batch's contiguous shards and output regions with the ids of zk_pool_add_ring. */
zk_status zk_prove_batch_rings(zk_ctx *ctx, uint64_t B, const uint8_t *msg_hash /*Bx32*/, const uint8_t *sig /*Bx64*/, const uint8_t *pk_xy /*Bx64*/,
                               const uint32_t *which /*B*/, const uint32_t *ring_ids /*B*/, const zk_rng *rng, uint8_t *out, uint64_t out_cap,
                               uint64_t *out_off /*B+1*/, int32_t *per_proof_status /*B*/);
zk_status zk_prove_batch_rings_device(zk_ctx *ctx, uint64_t B, const void *d_msg_hash, const void *d_sig, const void *d_pk_xy, const void *d_which,
                                      const void *d_ring_ids /*u32[B]*/, const zk_rng *rng_device, void *d_out, uint64_t out_cap,
                                      void *d_out_off /*u64[B+1]*/, void *d_per_proof_status /*i32[B]*/);

/* Witness screen: is a witness worth a proof?  The reference's prover starts with "a signature verification to recover R" (src/zkpAttestList.ts:124-131)
 * but never compares R.x with r, takes `which` from the caller (zkpAttestList.ts:110) and finds out last whether keys[which] is the signer's key
 * (proveMembership, src/proofGK/gk.ts:94-195); zk_prove_batch does the same, so a wrong signature, a wrong message, -pk for pk or a key that is not at
 * `which` all return status 0 and a proof that zk_verify_batch rejects.  zk_screen_batch answers both questions for B witnesses at the cost of a few dozen
 * point additions each, against the ring's resident limbs: which_out[b] is the signer's index, flags[b] a set of ZK_SCREEN_* bits, and flags[b] == 0 means
 * that zk_prove_batch with which_out[b] gives a proof that verifies.
 *   ZK_SCREEN_KEY_NOT_ON_CURVE   pk fails the prover's own key check: deserializePoint's rule (src/curves/weier.ts:74-89: the curve equation mod p, coordinates
 *                                reduced and not range-checked), the condition of the prover's ZK_E_POINT_NOT_IN_GROUP.
 *   ZK_SCREEN_SIG_RANGE          r or s is outside [1, n - 1] as a 256-bit integer (FIPS 186-5 section 6.4.2).  DELIBERATELY STRICTER THAN THE PROVER, which reduces
 *                                r and s mod n (zkpAttestList.ts:119-127) and proves for r + n as it does for r: such a witness is flagged although its proof verifies.
 *   ZK_SCREEN_SIG_INVALID        evaluated only when the two bits above are clear: R = (z / s) G + (r / s) pk is the identity or R.x mod n != r, with
 *                                z = truncateToN(msg_hash) (zkpAttestList.ts:80-86) -- exactly where ECDSA verification of the in-range signature fails.
 *   ZK_SCREEN_NOT_IN_RING        the lookup failed (below); evaluated whatever the other bits, it compares integers.
 *   ZK_SCREEN_RING_NOT_RESIDENT  (_rings forms) ring_ids[b] is not resident: no other bit is evaluated and which_out[b] = ZK_WHICH_NONE.
 * Lookup, with x = pk.x mod p, the value keyToInt (zkpAttestList.ts:94-102) / zk_keys_to_ints puts into a ring:
 *   which == NULL (find): which_out[b] = the LOWEST i in [0, n_keys) with ring[i] == x -- never one of the padding copies of keys[0] at [n_keys, N) --, or
 *                         ZK_WHICH_NONE and ZK_SCREEN_NOT_IN_RING when there is none;
 *   which != NULL (check): which_out[b] = which[b]; ZK_SCREEN_NOT_IN_RING iff which[b] >= N or ring[which[b]] != x (padded indices are legal, as for the prover).
 * The lookup reads the limbs zk_ctx_set_ring / add_ring / update_ring keep resident and stores nothing per ring, so a screen issued after zk_ctx_update_ring
 * sees the updated ring.  The plain forms work on the active ring, the _rings forms take one resident ring id per witness like zk_prove_batch_rings and neither
 * read nor change the active ring.  The _device forms take every pointer in this context's HBM; which_out (u32[B]) can be handed to zk_prove_batch_device /
 * zk_prove_batch_rings_device as d_which as it is (replace ZK_WHICH_NONE first, or skip those witnesses: the prover answers it with ZK_E_ARG).
 * The call changes no prover or verifier state and may be issued between prove calls; it works in chunks of 16 384 witnesses on one scratch buffer of about
 * 23 MB whatever B is, and does not need the prover's workspaces.  The scratch holds u1 = z / s and u2 = r / s: witness-derived, so zk_ctx_wipe,
 * zk_ctx_destroy and a failed screen call zero it.  zk_last_timing afterwards reports the call's two phases, "screen_lookup" and "screen_ecdsa" (under the
 * rules of zk_ctx_set_timing).  ZK_E_BUFFER before zk_ctx_set_params (the comb of G is built there) and, for the plain forms, without an active ring;
 * ZK_E_ARG for NULL pointers other than `which` and while streamed jobs are queued; B = 0 is ZK_OK.
 * How: find mode runs blocks of 256 witnesses against tiles of the ring's lowest limb in LDS, compares at full width where that limb matches and keeps the
 * lowest index; the ECDSA part is one lane per witness -- one inversion (of s), u1 G by the comb of G (13 additions), u2 pk through the key's table where the
 * looked-up entry has one (33 additions; zk_ctx_set_key_tables) and by the prover's 65-window walk otherwise, and the comparison X == r Z, X == (r + n) Z
 * without a field inversion.  A _rings call makes one pass per resident ring.  A chunk of at most 4 096 witnesses (ZK_SCREEN_CO_MAX; the decision is taken per
 * chunk, so a call of 16 384 + 3 runs its last three that way) takes the point arithmetic on cooperating waves instead, one workgroup of four waves per witness:
 * on the key-table path a quarter of the comb's and of the table's windows per wave, on the walk one wave for the 65 windows while the others sum u1 G.  Same
 * which_out and flags bit for bit; ZKATTEST_ONE_LANE_CHAINS (any value) keeps every chunk on the one-lane kernels; zk_test_counter 4 counts four chains per
 * witness of a cooperative chunk.
 * Not provided: streamed (submit / wait) variants, zk_pool_* variants. */
#define ZK_WHICH_NONE 0xFFFFFFFFu
enum {
    ZK_SCREEN_KEY_NOT_ON_CURVE = 1,
    ZK_SCREEN_SIG_RANGE = 2,
    ZK_SCREEN_SIG_INVALID = 4,
    ZK_SCREEN_NOT_IN_RING = 8,
    ZK_SCREEN_RING_NOT_RESIDENT = 16
};
zk_status zk_screen_batch(zk_ctx *ctx, uint64_t B, const uint8_t *msg_hash /*Bx32*/, const uint8_t *sig /*Bx64*/, const uint8_t *pk_xy /*Bx64*/,
                          const uint32_t *which /*B or NULL*/, uint32_t *which_out /*B*/, uint32_t *flags /*B*/);
zk_status zk_screen_batch_device(zk_ctx *ctx, uint64_t B, const void *d_msg_hash, const void *d_sig, const void *d_pk_xy, const void *d_which /*u32[B] or NULL*/,
                                 void *d_which_out /*u32[B]*/, void *d_flags /*u32[B]*/);
zk_status zk_screen_batch_rings(zk_ctx *ctx, uint64_t B, const uint8_t *msg_hash /*Bx32*/, const uint8_t *sig /*Bx64*/, const uint8_t *pk_xy /*Bx64*/,
                                const uint32_t *which /*B or NULL*/, const uint32_t *ring_ids /*B*/, uint32_t *which_out /*B*/, uint32_t *flags /*B*/);
zk_status zk_screen_batch_rings_device(zk_ctx *ctx, uint64_t B, const void *d_msg_hash, const void *d_sig, const void *d_pk_xy,
                                       const void *d_which /*u32[B] or NULL*/, const void *d_ring_ids /*u32[B]*/, void *d_which_out /*u32[B]*/,
                                       void *d_flags /*u32[B]*/);

/* Key recovery: the signer's key from (msg_hash, signature) alone, and its place in the ring.  A witness of zk_prove_batch is (msg_hash, sig, pk, which)
 * and zk_screen_batch can drop `which`, but a P-256 signature already determines its signer up to four points Q = (s R - z G) / r, and only the ring can say
 * which of them is a member.  zk_recover_batch computes them and looks them up in the ring's resident limbs; its outputs are laid out as
 * zk_prove_batch_device takes its inputs, so recover -> prove is device-resident from (msg, sig) alone.  The reference has no counterpart: its prover takes
 * the key from the caller (src/zkpAttestList.ts:104-118).  Per witness:
 *   Range.       r or s outside [1, n - 1] as a 256-bit integer: flags = ZK_RECOVER_SIG_RANGE, which_out = ZK_WHICH_NONE, pk_xy_out = 64 zero bytes; nothing else
 *                is evaluated.
 *   Candidates.  At most four, in this order: c = 0: R = (r, even y), 1: R = (r, odd y), 2: R = (r + n, even y), 3: R = (r + n, odd y).  Candidates 2 and 3 exist
 *                only when r + n < p.  An x-candidate exists only when v = x^3 - 3x + b is a square mod p (y = v^((p+1)/4), tested by y^2 == v).  If no
 *                x-candidate lifts: flags = ZK_RECOVER_NO_POINT | ZK_RECOVER_NOT_IN_RING.
 *   Keys.        Q_c = u1 G + u2 R_c with u1 = -z / r, u2 = s / r mod n and z = truncateToN(msg_hash) as the prover and the screen compute it
 *                (zkpAttestList.ts:80-86).  A Q_c that is the identity is not a key and is skipped; its sibling of the other parity is still exact.
 *   Lookup.      x(Q_c) among the caller's keys [0, n_keys) -- never the padding --: the lowest matching index, as in the screen's find mode.
 *   Winner.      The candidate with the lowest index; ties (z = 0 mod n makes Q_0 = -Q_1: one x) go to the lowest c.  With a winner pk_xy_out is its canonical
 *                affine x || y, big-endian, which_out its index, flags = 0; without one ZK_RECOVER_NOT_IN_RING, ZK_WHICH_NONE and zero bytes.
 *   _rings.      One resident ring id per witness, as in zk_screen_batch_rings; an id that is not resident gives ZK_RECOVER_RING_NOT_RESIDENT alone (ZK_WHICH_NONE,
 *                zero bytes, nothing else evaluated).  These forms neither read nor change the active ring.
 * Guarantee: flags[b] == 0 implies that zk_screen_batch in find mode on (msg, sig, pk_xy_out) returns (which_out[b], 0), hence that zk_prove_batch with these
 * values gives a proof that verifies.
 * Call-level rules are the screen's: ZK_E_BUFFER before zk_ctx_set_params and, for the plain forms, without an active ring; ZK_E_ARG for NULL pointers and
 * while streamed jobs are queued; B = 0 is ZK_OK; chunks of 16 384 witnesses on the context's main stream; a call issued after zk_ctx_update_ring sees the
 * updated ring; prover, verifier and screen state is untouched.  The _device forms take every pointer in this context's HBM (4-byte aligned).  zk_last_timing
 * reports three families, "recover_lift", "recover_points" and "recover_lookup".  Memory: one buffer of about 26 MB of its own, allocated by the first call
 * (the screen's scratch keeps its documented size); it holds u1, u2, the lifted R and the candidate keys, all witness-derived, so zk_ctx_wipe, zk_ctx_destroy
 * and a failed call zero it.
 * How: one lane per witness; per pass (x = r, then x = r + n, whose workgroups leave at once outside adversarial inputs) a front end (the lift, ONE inversion
 * of r, u2's digits), u1 G by the comb of G and 1..8 R, then ONE 65-window walk u2 R that serves both parities (Q_0 = A + Bp, Q_1 = A - Bp) and one shared
 * field inversion; the screen's LDS-tiled lookup over the candidates ("recover_lookup" times the lookup alone), and the selection.  A chunk of at most
 * 4 096 witnesses (ZK_SCREEN_CO_MAX; decided per chunk, like the screen) takes the square root and the point arithmetic on cooperating waves instead: one
 * wave per witness raises v to (p+1)/4, then one workgroup of four waves per witness -- wave 0 holds 1..8 R in LDS and owns the walk, waves 1..3 sum u1 G
 * from the comb -- ends with A +- Bp and the same shared inversion.  Same pk_xy_out, which_out and flags bit for bit; ZKATTEST_ONE_LANE_CHAINS (any value)
 * keeps every chunk on the one-lane kernels; zk_test_counter 4 counts four chains per witness and pass (two passes) of a cooperative chunk.
 * Not provided: streamed (submit / wait) variants, zk_pool_* variants. */
enum {                                   /* values shared with ZK_SCREEN_* where the meaning is the same */
    ZK_RECOVER_SIG_RANGE = 2,
    ZK_RECOVER_NOT_IN_RING = 8,
    ZK_RECOVER_RING_NOT_RESIDENT = 16,
    ZK_RECOVER_NO_POINT = 32
};
zk_status zk_recover_batch(zk_ctx *ctx, uint64_t B, const uint8_t *msg_hash /*Bx32*/, const uint8_t *sig /*Bx64*/, uint8_t *pk_xy_out /*Bx64*/,
                           uint32_t *which_out /*B*/, uint32_t *flags /*B*/);
zk_status zk_recover_batch_device(zk_ctx *ctx, uint64_t B, const void *d_msg_hash, const void *d_sig, void *d_pk_xy_out /*Bx64*/, void *d_which_out /*u32[B]*/,
                                  void *d_flags /*u32[B]*/);
zk_status zk_recover_batch_rings(zk_ctx *ctx, uint64_t B, const uint8_t *msg_hash /*Bx32*/, const uint8_t *sig /*Bx64*/, const uint32_t *ring_ids /*B*/,
                                 uint8_t *pk_xy_out /*Bx64*/, uint32_t *which_out /*B*/, uint32_t *flags /*B*/);
zk_status zk_recover_batch_rings_device(zk_ctx *ctx, uint64_t B, const void *d_msg_hash, const void *d_sig, const void *d_ring_ids /*u32[B]*/,
                                        void *d_pk_xy_out /*Bx64*/, void *d_which_out /*u32[B]*/, void *d_flags /*u32[B]*/);

/* ---- ring membership of a committed value on its own.  Replaces B calls of proveMembership(params, com, index, values) /
 * verifyMembership(params, com, values, proof) (src/proofGK/gk.ts:94-262, with com = params.commit(values[index]), src/commit/pedersen.ts:53-58): a proof
 * that a Pedersen commitment on Tom-256 opens to one entry of the ACTIVE ring, without revealing which -- the one-of-many part of a ZKAttest proof without
 * its 80 cut-and-choose repetitions (4 n commitments and one ring fold per proof).  Proofs are "ZKM1" (byte formats above): proof b of a batch lies at
 * b * zk_member_proof_size(ctx).
 * Prover: the committed value is entry which[b] of the padded ring (padding indices allowed, as in zk_prove_batch); which[b] >= N gives per-proof ZK_E_ARG.
 * Randomness, per proof: with blinder_be32 == NULL fill 0 is commit()'s randomScalar and the 5 n draws of proveMembership follow in the reference's order
 * (r_i, a_i, s_i, t_i, rho_i for i = 0 .. n-1), every draw mod q with the contract's rejection sampling; the blinder comes back in blinder_out if that is
 * given.  With a caller's blinders (B x 32 bytes, reduced mod q as newScalar does) the 5 n draws start at fill 0.  com_xy72[b] = v g + r h is always
 * written; out[b * size ..] is the proof, or zeros where per_proof_status[b] != 0 (ZK_E_ARG, ZK_E_RNG_EXHAUSTED; ZK_E_INTERPOLATION cannot occur, as in
 * the full prover).  out_cap < B * size: ZK_E_BUFFER.
 * Verifier, per proof and in this order: ZK_E_BAD_ENCODING for a wrong magic, a total_len that is not the one the header's n announces (or, where n is the
 * ring's, not the slot's size), a nonzero reserved word, n > 63, com or a point of the announced structure off its curve or non-canonical (exactly what
 * zk_verify_batch checks on the same bytes inside ZKA1; of a structure longer than its slot, the points that lie inside the slot -- no byte outside a slot
 * is read); ok = 0 with status 0 where the header's n is not the ring's (the reference's length check returns false) or the summed relations are not the
 * identity; otherwise ok = 1.  verifier_seeds follow zk_verify_batch's contract (2 n + 1 fills per proof; the engine draws its own 128-bit randomisers
 * from the same seed); NULL: fresh OS randomness.
 * Both run in chunks (zk_ctx_set_chunk) on the context's lanes, on workspaces of their own sized for what a membership proof holds; the ring fold, the
 * commitments, the challenge hash and the verifier's sums are the kernels of the full proof, so zk_ctx_set_ring_fold, zk_ctx_set_comb_bits and the uniform
 * build apply, and the bytes depend on none of them.  Blinders, nonces and RNG fills are wiped as the prover's are (zk_ctx_wipe, zk_ctx_destroy, a failed
 * call).  zk_last_timing reports the families "rng_prepass", "gk_fold", "tom_commit", "tom_normalize", "hash", "respond_write" (prover) and
 * "v_parse_validate", "v_gk_total", "v_sums" (verifier).  ZK_E_BUFFER before zk_ctx_set_params or without an active ring; ZK_E_ARG for NULL pointers
 * (other than the optional ones), while streamed jobs are queued, and in ZK_MODE_HARDENED (an unbound proof hashes no statement; the _bound forms below
 * name theirs in the call and run in either mode).  B = 0 is ZK_OK.
 * Not provided: submit / wait forms, zk_pool_* forms, JSON, a packed layout -- of these calls and of their _bound forms. */
uint64_t zk_member_proof_size(const zk_ctx *ctx);   /* active ring; 0 without one */
zk_status zk_member_prove_batch(zk_ctx *ctx, uint64_t B, const uint32_t *which /*B*/, const uint8_t *blinder_be32 /*Bx32 or NULL*/, const zk_rng *rng,
                                uint8_t *com_xy72 /*Bx72 out*/, uint8_t *blinder_out /*Bx32 or NULL*/, uint8_t *out, uint64_t out_cap,
                                int32_t *per_proof_status /*B*/);
zk_status zk_member_prove_batch_device(zk_ctx *ctx, uint64_t B, const void *d_which, const void *d_blinder_be32, const zk_rng *rng /* rng->data in HBM */,
                                       void *d_com_xy72, void *d_blinder_out, void *d_out, uint64_t out_cap, void *d_per_proof_status);
zk_status zk_member_verify_batch(zk_ctx *ctx, uint64_t B, const uint8_t *com_xy72 /*Bx72*/, const uint8_t *proofs /*B x size*/,
                                 const uint8_t *verifier_seeds /*Bx32 or NULL*/, uint8_t *ok /*B*/, int32_t *per_proof_status /*B*/);
zk_status zk_member_verify_batch_device(zk_ctx *ctx, uint64_t B, const void *d_com_xy72, const void *d_proofs, const void *d_verifier_seeds, void *d_ok,
                                        void *d_per_proof_status);
/* One resident ring id per proof (zk_ctx_add_ring): the reference takes `values` with every call, so a batch over several key sets is its own interface.
 * Neither form reads or changes the active ring -- a context whose rings are all inactive can prove and verify -- and a proof's size follows from its
 * ring alone: zk_member_proof_size_ring(ctx, ring) = 16 + 288 n + 32 (3 n + 1) for a resident id, 0 otherwise.
 * Prover: proof b, com_xy72[b], blinder_out[b] and per_proof_status[b] are byte for byte what zk_member_prove_batch returns for input b with ring
 * ring_ids[b] active -- the same randomness contract (the fills of proof b depend on b's own seed or stream row alone), engine-drawn or caller blinders,
 * which[b] indexing THAT ring's padded size (which[b] >= its N: ZK_E_ARG and a zeroed slot).  out_off[0] = 0, out_off[b + 1] = out_off[b] +
 * zk_member_proof_size_ring(ctx, ring_ids[b]): the proofs lie back to back in index order, and the result can be handed to zk_member_verify_batch_rings
 * with the same ring_ids as it is.  An id that is not resident: ZK_E_ARG, a zero-length slot, 72 zero bytes of com (32 of blinder_out).  out_cap <
 * out_off[B]: ZK_E_BUFFER, decided before a byte of any output is written.
 * Verifier, per proof and in this order: an id that is not resident: ok 0, ZK_E_ARG; a slot whose length proof_off[b + 1] - proof_off[b] is not
 * zk_member_proof_size_ring(ctx, ring_ids[b]), whose offset is no multiple of 4, or with proof_off[b + 1] < proof_off[b] or > proof_off[B]: ok 0,
 * ZK_E_BAD_ENCODING, and no byte of the slot is read; otherwise exactly the (ok, status) zk_member_verify_batch gives these 72 + size bytes with that
 * ring active (a header whose n is not the ring's: ok 0, status 0).  No byte outside a proof's slot is read; verifier_seeds as above.
 * How: the ids are classed (host pointers: on the host; device pointers: by one kernel and ONE read-back of the per-class counters).  A batch of one
 * resident ring runs the one-ring pipeline on the caller's buffers with that ring bound.  Otherwise, per ring, windows of at most 2 x chunk x lanes
 * proofs: one gather collects the window's small inputs (whole stream rows in ZK_RNG_STREAM mode), and the window's kernels write every proof, com,
 * blinder, status and verdict once, at its final place; the verifier reads the proof bytes where they lie.  zk_test_counter 13 counts the windows.
 * zk_last_timing reports the one-ring families summed over the windows, plus "m_class" and "m_gather".  The gathered inputs are witness-derived: a failed
 * call, zk_ctx_wipe and zk_ctx_destroy zero them.  ZK_E_BUFFER before zk_ctx_set_params; ZK_E_ARG for NULL pointers (other than the optional ones), while
 * streamed jobs are queued, and in ZK_MODE_HARDENED; B = 0 is ZK_OK (out_off[0] = 0).  The _device forms take every pointer in this context's HBM (4-byte
 * aligned; offsets 8-byte aligned), rng->data too. */
uint64_t zk_member_proof_size_ring(const zk_ctx *ctx, uint32_t ring);   /* 0 for an id that is not resident */
zk_status zk_member_prove_batch_rings(zk_ctx *ctx, uint64_t B, const uint32_t *which /*B*/, const uint32_t *ring_ids /*B*/,
                                      const uint8_t *blinder_be32 /*Bx32 or NULL*/, const zk_rng *rng, uint8_t *com_xy72 /*Bx72 out*/,
                                      uint8_t *blinder_out /*Bx32 or NULL*/, uint8_t *out, uint64_t out_cap, uint64_t *out_off /*B+1*/,
                                      int32_t *per_proof_status /*B*/);
zk_status zk_member_prove_batch_rings_device(zk_ctx *ctx, uint64_t B, const void *d_which, const void *d_ring_ids, const void *d_blinder_be32,
                                             const zk_rng *rng /* rng->data in HBM */, void *d_com_xy72, void *d_blinder_out, void *d_out, uint64_t out_cap,
                                             void *d_out_off /*u64[B+1]*/, void *d_per_proof_status);
zk_status zk_member_verify_batch_rings(zk_ctx *ctx, uint64_t B, const uint8_t *com_xy72 /*Bx72*/, const uint8_t *proofs, const uint64_t *proof_off /*B+1*/,
                                       const uint32_t *ring_ids /*B*/, const uint8_t *verifier_seeds /*Bx32 or NULL*/, uint8_t *ok /*B*/,
                                       int32_t *per_proof_status /*B*/);
zk_status zk_member_verify_batch_rings_device(zk_ctx *ctx, uint64_t B, const void *d_com_xy72, const void *d_proofs, const void *d_proof_off /*u64[B+1]*/,
                                              const void *d_ring_ids, const void *d_verifier_seeds, void *d_ok, void *d_per_proof_status);
/* Bound membership proofs, "ZKMB".  A ZKM1 proof is a bare Groth-Kohlweiss transcript -- its challenge hashes the 4 n commitment points and nothing else
 * (gk.ts:178-180, under the TODO "we should hash in the statement") --, so whoever sees one (com, proof) pair can present it again to any verifier, in any
 * session, even for another ring of the same size that holds the value.  The _bound forms close that: the eight calls above with `context`, 32 bytes per
 * proof chosen by the caller (a session nonce, a message hash, a verifier's id; the engine does not interpret them), after `which` (prove) or after
 * com_xy72 (verify), and the challenge becomes
 *     x = first 10 bytes of SHA-256( cl || ca || cb || cd  ||  S_b ),   the 4 n points in their hashPoints encodings (04 || x(33) || y(33)) as before,
 *     S_b = "ZKAttest-GK-member-v1" (21 bytes, no terminator) || ring digest (32: zk_ring_digest of the proof's ring, padded) || context_b (32)
 *           || 04 || com_b.x (33, big-endian) || com_b.y (33)                                                            -- 152 bytes.
 * Everything else is the unbound call's: draws and their order, blinder rules, responses, sizes (zk_member_proof_size[_ring]), the verifier's order of
 * checks, its status codes and its seeds, chunks, lanes, windows, timing families, wiping.  The proof's first four bytes are "ZKMB".  The bound verifier
 * accepts exactly "ZKMB" and the unbound one exactly "ZKM1": the other magic is ZK_E_BAD_ENCODING, like any wrong magic.  A proof verifies only with the
 * context and the com it was made with, against the ring it was made for: another context, another proof's com or another ring give ok = 0, status 0.
 * The ring digest is read when the call runs: after zk_ctx_update_ring a bound call hashes the updated ring's digest, so a proof made before the update
 * no longer verifies (ok = 0, status 0) even where the key it is about was not touched -- re-prove after an update.  In the _rings forms proof b hashes
 * the digest of ring ring_ids[b].  The binding is in the call, not in a mode: the _bound forms run in ZK_MODE_REFERENCE and ZK_MODE_HARDENED alike and give
 * the same bytes in both.  Contexts are not secret: they are not wiped.  context == NULL: ZK_E_ARG (also for B = 0); otherwise the call-level rules above.
 * No counterpart in the reference beyond its TODO; oracle/zkattest_ref.py states it as proveMembership / verifyMembership(..., statement = S_b). */
zk_status zk_member_prove_batch_bound(zk_ctx *ctx, uint64_t B, const uint32_t *which /*B*/, const uint8_t *context /*Bx32*/,
                                      const uint8_t *blinder_be32 /*Bx32 or NULL*/, const zk_rng *rng, uint8_t *com_xy72 /*Bx72 out*/,
                                      uint8_t *blinder_out /*Bx32 or NULL*/, uint8_t *out, uint64_t out_cap, int32_t *per_proof_status /*B*/);
zk_status zk_member_prove_batch_bound_device(zk_ctx *ctx, uint64_t B, const void *d_which, const void *d_context, const void *d_blinder_be32,
                                             const zk_rng *rng /* rng->data in HBM */, void *d_com_xy72, void *d_blinder_out, void *d_out, uint64_t out_cap,
                                             void *d_per_proof_status);
zk_status zk_member_verify_batch_bound(zk_ctx *ctx, uint64_t B, const uint8_t *com_xy72 /*Bx72*/, const uint8_t *context /*Bx32*/,
                                       const uint8_t *proofs /*B x size*/, const uint8_t *verifier_seeds /*Bx32 or NULL*/, uint8_t *ok /*B*/,
                                       int32_t *per_proof_status /*B*/);
zk_status zk_member_verify_batch_bound_device(zk_ctx *ctx, uint64_t B, const void *d_com_xy72, const void *d_context, const void *d_proofs,
                                              const void *d_verifier_seeds, void *d_ok, void *d_per_proof_status);
zk_status zk_member_prove_batch_rings_bound(zk_ctx *ctx, uint64_t B, const uint32_t *which /*B*/, const uint8_t *context /*Bx32*/,
                                            const uint32_t *ring_ids /*B*/, const uint8_t *blinder_be32 /*Bx32 or NULL*/, const zk_rng *rng,
                                            uint8_t *com_xy72 /*Bx72 out*/, uint8_t *blinder_out /*Bx32 or NULL*/, uint8_t *out, uint64_t out_cap,
                                            uint64_t *out_off /*B+1*/, int32_t *per_proof_status /*B*/);
zk_status zk_member_prove_batch_rings_bound_device(zk_ctx *ctx, uint64_t B, const void *d_which, const void *d_context, const void *d_ring_ids,
                                                   const void *d_blinder_be32, const zk_rng *rng /* rng->data in HBM */, void *d_com_xy72,
                                                   void *d_blinder_out, void *d_out, uint64_t out_cap, void *d_out_off /*u64[B+1]*/,
                                                   void *d_per_proof_status);
zk_status zk_member_verify_batch_rings_bound(zk_ctx *ctx, uint64_t B, const uint8_t *com_xy72 /*Bx72*/, const uint8_t *context /*Bx32*/,
                                             const uint8_t *proofs, const uint64_t *proof_off /*B+1*/, const uint32_t *ring_ids /*B*/,
                                             const uint8_t *verifier_seeds /*Bx32 or NULL*/, uint8_t *ok /*B*/, int32_t *per_proof_status /*B*/);
zk_status zk_member_verify_batch_rings_bound_device(zk_ctx *ctx, uint64_t B, const void *d_com_xy72, const void *d_context, const void *d_proofs,
                                                    const void *d_proof_off /*u64[B+1]*/, const void *d_ring_ids, const void *d_verifier_seeds, void *d_ok,
                                                    void *d_per_proof_status);

/* ---- re-ring: a ZKA1 proof moved to another ring, its signature part untouched.  A proof is R, comS1, keyXcom, keyYcom, expProof[secLevel] followed by a GKProof,
 * and only the GKProof depends on the ring (src/zkpAttestList.ts:104-145: proveMembership(params.ProofGroup, pkX, which, keys) runs last, on the commitment
 * keyXcom); the rest -- about 96 % of the bytes and 87 % of a proof's time (profiles/rering_rate.json) -- stays valid for any ring that holds the key.  So after zk_ctx_update_ring, for a second
 * registry or for a larger ring, a proof for the new ring is the old head plus a fresh GKProof over the same keyXcom: what zk_member_prove_batch computes when
 * it is given keyXcom's blinder.  The signature witness is not needed again, the blinder is.
 * zk_prove_key_blinders: the blinder of keyXcom of the proof zk_prove_batch makes from the same rng -- logical draw 1 of each proof under the randomness
 *   contract (draw 0 is comS1's, mod n; draw 1 mod q), 32 bytes big-endian per proof.  A prover that wants to re-ring later keeps it (or the seed) with the
 *   proof; it is as secret as the seed.  ZK_E_BUFFER before zk_ctx_set_params, ZK_E_ARG for NULL pointers, B >= 2^32 and while streamed jobs are queued, B = 0
 *   is ZK_OK.  ZK_RNG_STREAM: a proof whose stream does not hold the draw (fewer than two blocks, or rejected fills in front of it) gets 32 zero bytes and the
 *   call returns ZK_E_RNG_EXHAUSTED; the other proofs' blinders are written.  Works in chunks of 2^18 proofs on one scratch buffer of 18 MB, wiped with the rest.
 * zk_proof_rering_batch: the target is the ACTIVE ring.  Nothing of the ring a proof was made for is read: it need not be resident or exist any more.
 *   Output proof b is input proof b with its GKProof section (the last 288 n_old + 32 (3 n_old + 1) bytes, 264 n_old + ... in ZKA1P) replaced by a new one for
 *   the active ring and the header's n and total_len updated; every other byte -- magic, secLevel, challenge bits, R, comS1, keyXcom, keyYcom, every
 *   repetition -- is copied unchanged.  In ZK_MODE_REFERENCE the new section is byte for byte bytes [16, size) of the proof zk_member_prove_batch(which_new,
 *   key_blinder, rng) returns with this ring active, under that call's caller-blinder contract: the 5 n draws start at fill 0, all mod q.  In
 *   ZK_MODE_HARDENED its challenge hashes the full proof's statement (ring digest, msgHash, R, keyXcom: zk_ctx_set_mode), R and keyXcom read from the proof,
 *   as zk_prove_batch does in that mode.  msg_hash is required in both modes.  Input and output are in the context's wire layout (zk_ctx_set_wire).
 *   Per proof, in this order; a failed proof gets an empty output slot and touches no neighbour:
 *     ZK_E_BAD_ENCODING   a wrong magic (the other layout's included), a header total_len that is not the slot's length, a header n > 63, a total_len smaller
 *                         than the fixed head plus the GKProof its n announces, a slot offset or a slot length that is not a multiple of 4, offsets that do
 *                         not ascend.  No
 *                         curve check is made -- this is not a verifier -- and no byte outside a slot is read.
 *     ZK_E_ARG            which_new[b] >= N of the active ring.
 *     ZK_E_OPENING        ring[which_new[b]] g + key_blinder[b] h is not the proof's keyXcom (the blinder reduced mod q as newScalar does; one comb commitment
 *                         per proof, compared as canonical bytes): a wrong blinder, or a key that is not at which_new -- caught before a proof that cannot
 *                         verify is written.
 *     ZK_E_RNG_EXHAUSTED  as in zk_member_prove_batch.
 *   out_off[0] = 0 and the proofs lie back to back in index order, ready for zk_verify_batch.  ZK_E_BUFFER when out_cap is too small, decided before a byte is
 *   written, from the headers alone: out_cap must hold the new proofs of all inputs that pass the first two checks (what the output is unless a proof fails
 *   its opening or its RNG stream; those slots are then empty and the proofs behind them close up).
 *   In place: out == proofs is allowed in the _device form when every well-formed proof's n equals the ring's.  Only the GKProof sections are rewritten,
 *   out_off is a copy of proof_off, a failed proof keeps its bytes and gets its status, no byte of any repetition is read or written, and out_cap must be
 *   at least proof_off[B].  If some well-formed proof has another n the call returns ZK_E_ARG and writes nothing.  The _device form decides both rules with
 *   one census kernel and ONE read-back of its counters.  The host-pointer form stages the batch in HBM; out == proofs is in place there too, by the same rules
 *   (the staged copy is re-ringed in place and copied back).  Any other overlap of out and proofs is refused with ZK_E_ARG, nothing written.
 *   Call-level rules are the member calls': ZK_E_BUFFER without params or without an active ring; ZK_E_ARG for NULL pointers and while streamed jobs are
 *   queued; B = 0 is ZK_OK (out_off[0] = 0); chunks (zk_ctx_set_chunk) on the context's lanes; both protocol modes.  The _device form takes every pointer and
 *   rng->data in this context's HBM (proofs and out 4-byte aligned, offsets 8-byte aligned).  zk_last_timing reports the member prover's families plus
 *   "rr_census", "rr_offsets" and "rr_move".  The staged blinders and RNG fills are witness-derived: zk_ctx_wipe, zk_ctx_destroy and a failed call zero them.
 *   Not provided: streamed and zk_pool_* forms.
 * zk_proof_rering_batch_rings: one resident ring id per proof.  Proof b is moved to resident ring ring_ids[b]; the active ring is neither read nor changed,
 *   so a context without an active ring can make the call.  Where proof b succeeds, its output bytes are byte for byte what zk_proof_rering_batch writes for
 *   input b alone with that ring active, under the same rng row or seed -- in both protocol modes (in ZK_MODE_HARDENED the statement hashes the digest of
 *   ring ring_ids[b]) and both wire layouts.  Per proof, the first rule that matches:
 *     1. ring_ids[b] is not resident                      ZK_E_ARG, a zero-length slot (no byte of the proof is read)
 *     2. the header or slot rules above fail              ZK_E_BAD_ENCODING, a zero-length slot (no byte beyond the header is read)
 *     3. which_new[b] >= N of ITS ring                    ZK_E_ARG, a zero-length slot
 *     4. the opening fails                                ZK_E_OPENING
 *     5. the RNG stream is too short                      ZK_E_RNG_EXHAUSTED
 *   The one difference from the one-ring call: the layout is fixed by ids and headers alone -- out_off[b + 1] - out_off[b] = head_b + gk(n of ring_ids[b])
 *   for every proof that passes rules 1-3 and 0 otherwise, and a proof that then fails rule 4 or 5 KEEPS its slot, filled with zero bytes (ZK_E_BAD_ENCODING
 *   to every verifier), instead of the slots behind it closing up.  A batch whose ids all name one ring follows the same rule: it belongs to the call, not
 *   to the mix.  So every proof's place is known before anything is proved, and out_cap is decided exactly: ZK_E_BUFFER when out_cap < out_off[B], before a
 *   byte of out, out_off or the statuses is written.
 *   In place: out == proofs is allowed in both forms when every proof that passes rules 1-3 has the n of its destination ring; otherwise ZK_E_ARG, nothing
 *   written.  Then only GKProof sections are rewritten, out_off is a copy of proof_off, a failed proof keeps its bytes and gets its status, no byte of a
 *   repetition is read or written, and out_cap >= proof_off[B].  Any other overlap of out and proofs is ZK_E_ARG.
 *   Call-level rules are zk_proof_rering_batch's, except that "no active ring" is no refusal: a context with params but no resident ring gives every proof
 *   rule 1.  The _device form makes ONE read-back, of the census counters.  zk_last_timing reports the member prover's families plus "rr_census",
 *   "rr_offsets", "rr_move" and "m_gather"; zk_test_counter 13 counts the windows (none for a batch of one ring without refusals, which runs on the caller's
 *   arrays).  The gathered blinders, seeds and stream rows are witness-derived: a failed call, zk_ctx_wipe and zk_ctx_destroy zero them.
 *   The host-pointer form stages proofs[0, end of the last slot it reads) in HBM as one copy: rules 1 and 2 say which bytes are PARSED, not which cross the link.
 *   How: DESIGN.md section 5d'.
 * Two warnings.  (1) Two GKProofs over one keyXcom tell a verifier who sees both that the key lies in the INTERSECTION of the two rings: re-ringing to a ring
 *   that shares few keys with the old one gives most of the anonymity away to whoever holds both proofs.  (2) rng must be fresh and independent of the rng the
 *   proof was made with: with the original seeds, fill 0 and fill 1 of the new call are comS1's and keyXcom's blinders reused as GK nonces, and the responses
 *   za, zb then reveal them.
 * How: one lane per proof reads the header, keyXcom (and R in hardened mode) and gathers ring[which_new] from the ring's resident limbs; the claimed opening
 *   rides in the same commitment launch as the proof's 4 n membership commitments and is compared behind the normaliser; an exclusive scan of the new lengths
 *   gives the offsets; one kernel moves the heads, 16 bytes per lane with the work divided by bytes; the membership prover's fold, hash, responses and point
 *   writers run unchanged, pointed at each proof's own GKProof section. */
zk_status zk_prove_key_blinders(zk_ctx *ctx, uint64_t B, const zk_rng *rng, uint8_t *blinder_be32 /*Bx32*/);   /* host pointers */
zk_status zk_prove_key_blinders_device(zk_ctx *ctx, uint64_t B, const zk_rng *rng_device, void *d_blinder_be32);
zk_status zk_proof_rering_batch(zk_ctx *ctx, uint64_t B, const uint8_t *msg_hash /*Bx32*/, const uint8_t *proofs, const uint64_t *proof_off /*B+1*/,
                                const uint32_t *which_new /*B*/, const uint8_t *key_blinder_be32 /*Bx32*/, const zk_rng *rng, uint8_t *out, uint64_t out_cap,
                                uint64_t *out_off /*B+1*/, int32_t *per_proof_status /*B*/);
zk_status zk_proof_rering_batch_device(zk_ctx *ctx, uint64_t B, const void *d_msg_hash, const void *d_proofs, const void *d_proof_off /*u64[B+1]*/,
                                       const void *d_which_new /*u32[B]*/, const void *d_key_blinder_be32, const zk_rng *rng_device, void *d_out,
                                       uint64_t out_cap, void *d_out_off /*u64[B+1]*/, void *d_per_proof_status /*i32[B]*/);
zk_status zk_proof_rering_batch_rings(zk_ctx *ctx, uint64_t B, const uint8_t *msg_hash /*Bx32*/, const uint8_t *proofs, const uint64_t *proof_off /*B+1*/,
                                      const uint32_t *which_new /*B*/, const uint32_t *ring_ids /*B*/, const uint8_t *key_blinder_be32 /*Bx32*/, const zk_rng *rng,
                                      uint8_t *out, uint64_t out_cap, uint64_t *out_off /*B+1*/, int32_t *per_proof_status /*B*/);
zk_status zk_proof_rering_batch_rings_device(zk_ctx *ctx, uint64_t B, const void *d_msg_hash, const void *d_proofs, const void *d_proof_off /*u64[B+1]*/,
                                             const void *d_which_new /*u32[B]*/, const void *d_ring_ids /*u32[B]*/, const void *d_key_blinder_be32,
                                             const zk_rng *rng_device, void *d_out, uint64_t out_cap, void *d_out_off /*u64[B+1]*/,
                                             void *d_per_proof_status /*i32[B]*/);

/* ---- link proofs: two key commitments hide the same key.  The engine hands out Tom-256 commitments to a signer's key in three places -- keyXcom of every
 * ZKA1 proof (its blinder: zk_prove_key_blinders), com of zk_member_prove_batch, and the keyXcom a re-ringed proof keeps -- and a link proof is the one statement
 * that ties two of them together: ZK(x, r1, r2 : C1 = x g + r1 h  and  C2 = x g + r2 h), the reference's proveEquality / verifyEquality
 * (src/commit/equality.ts:60-116) on its own, outside any PointAddProof.  With it the signer of attestation A shows that they also signed attestation B (two
 * different proofs, two unrelated keyXcoms), or that they are a member of a second registry (keyXcom and a ZKM1 commitment), without re-ringing.  No signature,
 * no P-256, no ring: the calls need zk_ctx_set_params only.
 * Wire format "ZKL1", 256 bytes:
 *     header 16 B : "ZKL1" | total_len u32 big-endian (= 256) | 0 u32 | 0 u32
 *     EqualityProof 240 B : A_1, A_2 (Tom-256 points, 72 bytes each), t_x, t_r1, t_r2 (32 bytes big-endian each)
 *   the body exactly as an EqualityProof lies inside ZKA1, always with 36-byte coordinates: zk_ctx_set_wire plays no part, as for ZKM1.  The two commitments
 *   travel beside the proof as 72-byte Tom-256 points, as com does for ZKM1.
 * zk_link_prove_batch: proof b is byte for byte proveEquality(params.ProofGroup, x, Commitment(C1, r1), Commitment(C2, r2)) under the randomness contract:
 *   fill 0 is k = rnd(q), fills 1 and 2 the randomScalars s1, s2 of the two commit(k), all mod q with the contract's rejection sampling; key and both blinders
 *   are reduced mod q as newScalar does; c = hashPoints([C1, C2, A_1, A_2]) (80 bits); t_x = k - c x, t_r1 = s1 - c r1, t_r2 = s2 - c r2.
 *   Per proof, in this order; a failed proof gets 256 zero bytes and touches no neighbour:
 *     ZK_E_BAD_ENCODING   com1 or com2 has a coordinate that is not below the field prime (padding bytes set included) or is off the curve: the rule
 *                         zk_member_verify_batch applies to com.
 *     ZK_E_OPENING        x g + r1 h is not com1, or x g + r2 h is not com2 (compared as canonical bytes, as the re-ring opening check): caught before a proof
 *                         that cannot verify is written.
 *     ZK_E_RNG_EXHAUSTED  as in zk_member_prove_batch: ZK_RNG_STREAM with fewer blocks than the three draws and their rejected fills need.
 *   ZK_E_BUFFER when out_cap < 256 B, before a byte of out or the statuses is written.  The bytes depend neither on zk_ctx_set_comb_bits nor on the uniform
 *   build, and both protocol modes work: the challenge binds both commitments, and ZK_MODE_HARDENED only changes h.
 * zk_link_verify_batch: per proof, in this order:
 *     ZK_E_BAD_ENCODING   a wrong magic, total_len != 256, a nonzero reserved word, or com1, com2, A_1 or A_2 non-canonical or off the curve.
 *   Scalars >= q are REDUCED mod q, exactly as zk_verify_batch treats the scalars of an EqualityProof inside ZKA1 (the reference's Scalar constructor reduces):
 *   they are no encoding error.  Otherwise ok = 1 iff both relations hold exactly,
 *     t_x g + t_r1 h + c C1 - A_1 = O   and   t_x g + t_r2 h + c C2 - A_2 = O,
 *   and the status is 0 either way.  The reference sums the two relations under random multipliers (multimult.ts:168-173); checking each one exactly gives the
 *   same boolean without any verifier randomness, so there is no verifier_seeds argument.
 * zk_proof_key_commitments: keyXcom of each ZKA1 / ZK1P proof (the context's wire layout, zk_ctx_set_wire), packed coordinates widened to 36 bytes -- what takes
 *   a verifier from two attestations to zk_link_verify_batch.  Header and slot rules, and ZK_E_BAD_ENCODING, are zk_proof_rering_batch's; no curve check is made,
 *   no byte outside a slot is read, no ring is needed.  A failed slot gets 72 zero bytes.
 * Call-level rules are the member calls': ZK_E_BUFFER before zk_ctx_set_params; ZK_E_ARG for NULL pointers, B >= 2^32 and while streamed jobs are queued; B = 0
 *   is ZK_OK; chunks (zk_ctx_set_chunk) on the context's lanes.  The _device forms take every pointer and rng->data in this context's HBM, 4-byte aligned
 *   (proof_off 8-byte aligned), else ZK_E_ARG.  The staged keys, blinders and RNG fills and the nonces are witness-derived: zk_ctx_wipe, zk_ctx_destroy and a failed
 *   call zero them.  zk_last_timing reports "rng_prepass", "tom_commit", "tom_normalize", "hash", "link_respond" (prover) and "link_parse", "tom_commit",
 *   "link_ladder" (verifier).  Not provided: submit / wait, zk_pool_*, JSON, a caller-context binding.
 * Two warnings.  (1) A link proof deliberately makes the two proofs linkable to anyone who sees it: that is its statement.  Show it only to whom the link is
 *   meant for.  (2) rng must be independent of the seeds either commitment's proof was made with.  With a ZKA1 proof's own seed, fills 0 and 1 are comS1's and
 *   keyXcom's blinders; reused as k and s1, the responses t_x and t_r1 reveal them.
 * How: the four commitments of a proof are two pair launches that share the g-part, (k g + s1 h, k g + s2 h) and (x g + r1 h, x g + r2 h); the verifier's
 *   c C_j is a left-to-right double-and-add over the 80 challenge bits, one lane per (proof, relation).  DESIGN.md section 5e. */
uint64_t zk_link_proof_size(void);   /* 256 */
zk_status zk_link_prove_batch(zk_ctx *ctx, uint64_t B, const uint8_t *key_be32 /*Bx32*/, const uint8_t *com1_xy72 /*Bx72*/, const uint8_t *blinder1_be32 /*Bx32*/,
                              const uint8_t *com2_xy72 /*Bx72*/, const uint8_t *blinder2_be32 /*Bx32*/, const zk_rng *rng, uint8_t *out, uint64_t out_cap,
                              int32_t *per_proof_status /*B*/);
zk_status zk_link_prove_batch_device(zk_ctx *ctx, uint64_t B, const void *d_key_be32, const void *d_com1_xy72, const void *d_blinder1_be32, const void *d_com2_xy72,
                                     const void *d_blinder2_be32, const zk_rng *rng_device, void *d_out, uint64_t out_cap, void *d_per_proof_status /*i32[B]*/);
zk_status zk_link_verify_batch(zk_ctx *ctx, uint64_t B, const uint8_t *com1_xy72 /*Bx72*/, const uint8_t *com2_xy72 /*Bx72*/, const uint8_t *proofs /*Bx256*/,
                               uint8_t *ok /*B*/, int32_t *per_proof_status /*B*/);
zk_status zk_link_verify_batch_device(zk_ctx *ctx, uint64_t B, const void *d_com1_xy72, const void *d_com2_xy72, const void *d_proofs, void *d_ok,
                                      void *d_per_proof_status /*i32[B]*/);
zk_status zk_proof_key_commitments(zk_ctx *ctx, uint64_t B, const uint8_t *proofs, const uint64_t *proof_off /*B+1*/, uint8_t *com_xy72 /*Bx72*/,
                                   int32_t *per_proof_status /*B*/);
zk_status zk_proof_key_commitments_device(zk_ctx *ctx, uint64_t B, const void *d_proofs, const void *d_proof_off /*u64[B+1]*/, void *d_com_xy72,
                                          void *d_per_proof_status /*i32[B]*/);

/* ---- distinct-key proofs: two key commitments hide DIFFERENT keys.  The opposite statement of a link proof, over the same commitments (a keyXcom from
 * zk_proof_key_commitments with its blinder from zk_prove_key_blinders, or a com of the member calls): ZK(x1, r1, x2, r2 : C1 = x1 g + r1 h, C2 = x2 g + r2 h,
 * x1 != x2 mod q).  q is P-256's field prime and a ring entry is a key's x-coordinate, so this means two different ring entries.  With one proof per pair, k
 * attestations that zk_verify_batch[_rings] accepts become "k different members of the ring approved this" with no member identified: the quorum or threshold
 * use (INTEGRATION.md "Counting signers").  A value is non-zero exactly when it has an inverse, so the proof is one MultProof of the reference
 * (src/commit/mult.ts:93-175) for (x1 - x2) * w = 1 over Cx = C1 - C2, Cy = C_w = commit(w), Cz = g.  No signature, no P-256, no ring: zk_ctx_set_params only.
 * Wire format "ZKD1", 744 bytes:
 *     header 16 B : "ZKD1" | total_len u32 big-endian (= 744) | 0 u32 | 0 u32
 *     C_w 72 B : the commitment to 1 / (x1 - x2), a Tom-256 point
 *     MultProof 656 B : C_4, A_x, A_y, A_z, A_4_1, A_4_2 (72 bytes each), t_x, t_y, t_z, t_rx, t_ry, t_rz, t_r4 (32 bytes big-endian each)
 *   the MultProof exactly as one lies inside ZKA1, always with 36-byte coordinates: zk_ctx_set_wire plays no part, as for ZKL1.  The two commitments travel
 *   beside the proof as 72-byte Tom-256 points.
 * The proof is DIRECTIONAL: (C1, C2, proof) does not verify as (C2, C1, proof).  Prover and verifier name the pair in the same order.
 * zk_distinct_prove_batch: with d = x1 - x2, rd = r1 - r2, w = 1 / d (all mod q), proof b is byte for byte
 *     Cw = params.commit(w);  proveMult(params, d, w, 1, Commitment(C1 - C2, rd), Cw, Commitment(g, 0))
 *   under the randomness contract: fill 0 is r_w, fills 1..3 are k_x, k_y, k_z, fills 4..7 the blinders of A_x, A_y, A_z, A_4_1, all mod q with the contract's
 *   rejection sampling (a stream needs 8 blocks plus one per rejected fill); keys and blinders are reduced mod q as newScalar does;
 *   c = hashPoints([Cx, C_w, g, C_4, A_x, A_y, A_z, A_4_1, A_4_2]) (80 bits).  Per proof, in this order; a failed proof gets 744 zero bytes and touches no
 *   neighbour:
 *     ZK_E_BAD_ENCODING   com1 or com2 has a coordinate that is not below the field prime (padding bytes set included) or is off the curve: the link calls' rule.
 *     ZK_E_ARG            x1 = x2 mod q: the statement is false and no proof exists.
 *     ZK_E_OPENING        x1 g + r1 h is not com1, or x2 g + r2 h is not com2 (compared as canonical bytes), before anything is written.
 *     ZK_E_RNG_EXHAUSTED  as in zk_link_prove_batch: ZK_RNG_STREAM with fewer blocks than the eight draws and their rejected fills need.
 *   ZK_E_BUFFER when out_cap < 744 B, before a byte of out or the statuses is written.  The bytes depend neither on zk_ctx_set_comb_bits nor on the uniform
 *   build, and both protocol modes work: ZK_MODE_HARDENED only changes h.
 * zk_distinct_verify_batch: per proof, in this order:
 *     ZK_E_BAD_ENCODING   a wrong magic, total_len != 744, a nonzero reserved word, or com1, com2, C_w or one of the six points non-canonical or off the curve.
 *   Scalars >= q are REDUCED mod q, not refused.  Otherwise the status is 0 and ok = 1 iff the five relations of aggregateMult hold exactly, with Cx = C1 - C2
 *   (the identity is a legal point here) and c as above:
 *     t_x g + t_rx h + c Cx - A_x = O,   t_y g + t_ry h + c C_w - A_y = O,   t_z g + t_rz h + c g - A_z = O,
 *     t_z g + t_r4 h + c C_4 - A_4_1 = O,   t_x C_w + c C_4 - A_4_2 = O.
 *   The reference sums them under random multipliers (multimult.ts:168-173); checking each one exactly gives the same boolean without verifier randomness, so
 *   there is no verifier_seeds argument.  There is no special case for C1 = C2: with Cx = O a forger would need z = 0 against Cz = g, which the relations refuse.
 * Call-level rules are the link calls': ZK_E_BUFFER before zk_ctx_set_params; ZK_E_ARG for NULL pointers, B >= 2^32 and while streamed jobs are queued; B = 0
 *   is ZK_OK; chunks (zk_ctx_set_chunk) on the context's lanes.  The _device forms take every pointer and rng->data in this context's HBM, 4-byte aligned, else
 *   ZK_E_ARG.  The staged keys and blinders, d, w, r_w, the nonces and the RNG fills are witness-derived: zk_ctx_wipe, zk_ctx_destroy and a failed call zero
 *   them.  zk_last_timing reports "rng_prepass", "tom_commit", "tom_normalize", "hash", "distinct_respond" (prover) and "distinct_parse", "tom_normalize",
 *   "hash", "tom_commit", "distinct_short", "distinct_long" (verifier).  Not provided: submit / wait, zk_pool_*, JSON, a caller-context binding.
 * Two warnings.  (1) A distinct-key proof tells whoever sees it that the two commitments belong to different signers; keep it for whom it is meant.  (2) rng
 *   must be independent of the seeds either commitment's proof was made with: with a ZKA1 proof's own seed the fills that blinded comS1 and keyXcom would come
 *   back as r_w and k_x, and the responses would be further equations in those blinders.
 * How: every point the prover makes is a fixed-base commitment with a known opening -- C_4 = (1, d r_w), A_4_2 = (k_x w, k_x r_w), (A_z, A_4_1) one pair
 *   launch -- so its side has no variable-base multiplication; the verifier's relation 5 is a joint left-to-right double-and-add over the 256 bits of t_x and
 *   the 80 of c in a kernel of its own, relations 1, 2, 4 are the link verifier's 80-bit ladder, relation 3 folds c into its comb part.  DESIGN.md section 5f. */
uint64_t zk_distinct_proof_size(void);   /* 744 */
zk_status zk_distinct_prove_batch(zk_ctx *ctx, uint64_t B, const uint8_t *key1_be32 /*Bx32*/, const uint8_t *com1_xy72 /*Bx72*/, const uint8_t *blinder1_be32 /*Bx32*/,
                                  const uint8_t *key2_be32 /*Bx32*/, const uint8_t *com2_xy72 /*Bx72*/, const uint8_t *blinder2_be32 /*Bx32*/, const zk_rng *rng,
                                  uint8_t *out, uint64_t out_cap, int32_t *per_proof_status /*B*/);
zk_status zk_distinct_prove_batch_device(zk_ctx *ctx, uint64_t B, const void *d_key1_be32, const void *d_com1_xy72, const void *d_blinder1_be32,
                                         const void *d_key2_be32, const void *d_com2_xy72, const void *d_blinder2_be32, const zk_rng *rng_device, void *d_out,
                                         uint64_t out_cap, void *d_per_proof_status /*i32[B]*/);
zk_status zk_distinct_verify_batch(zk_ctx *ctx, uint64_t B, const uint8_t *com1_xy72 /*Bx72*/, const uint8_t *com2_xy72 /*Bx72*/, const uint8_t *proofs /*Bx744*/,
                                   uint8_t *ok /*B*/, int32_t *per_proof_status /*B*/);
zk_status zk_distinct_verify_batch_device(zk_ctx *ctx, uint64_t B, const void *d_com1_xy72, const void *d_com2_xy72, const void *d_proofs, void *d_ok,
                                          void *d_per_proof_status /*i32[B]*/);

/* ---- quorum proofs: k attestations by k DIFFERENT ring members, as one artifact.  The recipe of INTEGRATION.md "Counting signers" -- zk_prove_batch,
 * zk_prove_key_blinders with the same seeds, zk_proof_key_commitments, zk_distinct_prove_batch over the pairs (and the mirror image for the verifier) -- as one
 * prove call and one verify call with a wire format of its own; the pairs are expanded, gathered and judged on the device.  No existing call changes.
 * Wire format "ZKQ1" (a bundle), 2 <= k <= 16, P = k (k - 1) / 2 <= 120:
 *     header 16 B : "ZKQ1" | total_len u32 big-endian | k u32 big-endian | 0 u32
 *     k attestations : ZKA1 / ZK1P proofs in the context's wire layout (zk_ctx_set_wire), back to back in member order, each exactly as zk_prove_batch writes
 *                      it (each carries its own total_len, a multiple of 4)
 *     P distinct-key proofs : ZKD1, 744 B each, in the order (0,1), (0,2), ..., (0,k-1), (1,2), ..., (k-2,k-1); pair (i, j) is proved for
 *                      (com1, com2) = (keyXcom of member i, keyXcom of member j), in that direction
 *   The key commitments are not repeated: they are the keyXcoms inside the k attestations, read by the rules of zk_proof_key_commitments, so the distinct-key
 *   proofs can only be checked against the attestations they travel with.  Attestation lengths vary with the Exp challenge, so a bundle's length varies;
 *   zk_quorum_proof_max_size(ctx, k) = 16 + k zk_proof_max_size(ctx) + 744 P.
 * Member m = q k + i of quorum q uses row m of msg_hash, sig, pk_xy, which and rng; pair p of quorum q uses row q P + p of rng_pairs.
 * zk_quorum_prove_batch: where quorum q succeeds its bundle is, byte for byte, the header, the k proofs zk_prove_batch makes for those members with the active
 *   ring under rng's rows, and the P proofs zk_distinct_prove_batch makes under rng_pairs' rows with key = pk_xy[0:32], com = the member's keyXcom and blinder =
 *   what zk_prove_key_blinders gives for the member's row: the bytes of the recipe, in both protocol modes and wire layouts, whatever the comb width or build.
 *   A quorum's status is the first non-zero one of: its members' zk_prove_batch statuses in member order; ZK_E_ARG if two of its members have the same key mod
 *   q (no distinct-key proof exists); its pairs' statuses in pair order (ZK_E_RNG_EXHAUSTED on a short pair stream).  A failed quorum gets an empty slot
 *   (out_off[q + 1] = out_off[q]), the bundles behind it close up, no neighbour's byte changes.  per_member_status (may be NULL) receives the Q k member
 *   statuses.  ZK_E_BUFFER when out_cap < Q zk_quorum_proof_max_size, decided before a byte of any output is written.
 * zk_quorum_verify_batch: per quorum, the first rule that matches:
 *     ZK_E_BAD_ENCODING with ok 0 and first_bad 0, no byte outside the slot read: a wrong magic, total_len != the slot's length, header k != the call's k, a
 *       non-zero reserved word, a slot offset or length that is no multiple of 4 or offsets that do not ascend, or the k inner headers (magic of the context's
 *       layout, total_len, the rules of zk_proof_rering_batch) not walking from byte 16 exactly to total_len - 744 P.
 *   Otherwise the k members are verified exactly as zk_verify_batch verifies them (the active ring, zk_ctx_set_verify_level and zk_ctx_set_verify_reps,
 *   verifier_seeds row m or the library's own) and the P pairs exactly as zk_distinct_verify_batch does over the members' keyXcoms.  ok = 1 iff all k + P
 *   elements are ok; per_quorum_status is the first non-zero element status, members before pairs, in index order; first_bad (may be NULL) is the smallest
 *   element index e whose ok is 0 or whose status is non-zero -- 0 <= e < k names a member, k <= e < k + P a pair -- and 0xFFFFFFFF where ok = 1.
 * Call-level rules are the distinct calls' plus the prover's: ZK_E_BUFFER without params or without an active ring; ZK_E_ARG for NULL pointers other than the
 *   two optional arrays, for k outside 2..16, for Q k or Q P >= 2^32 and while streamed jobs are queued; Q = 0 is ZK_OK with out_off[0] = 0.  The _device
 *   forms take every pointer, both rng->data included, in this context's HBM, 4-byte aligned, else ZK_E_ARG.  A call runs in windows of whole quorums of at
 *   most chunk x lanes members; what is witness-derived -- the gathered keys and blinders, both RNG fills, the distinct prover's arena, the staged inputs --
 *   is zeroed by zk_ctx_wipe, zk_ctx_destroy and a failed call.  zk_last_timing reports the families of the calls above plus "quorum_blinders",
 *   "quorum_gather", "quorum_layout" (prover) and "quorum_walk", "quorum_verdict" (verifier).
 * Not provided: one ring id per member, submit / wait forms, zk_pool_* forms, JSON, a caller-context binding.
 * Two warnings.  (1) rng_pairs must be independent of rng: with an attestation's own seed the fills that blinded comS1 and keyXcom would come back as a
 *   distinct-key proof's r_w and k_x.  (2) A bundle tells whoever sees it that its attestations come from different signers; keep it for whom it is meant.
 * DESIGN.md section 5g. */
uint64_t zk_quorum_pair_count(uint32_t k);                         /* k (k - 1) / 2; 0 for k outside 2..16 */
uint64_t zk_quorum_proof_max_size(const zk_ctx *ctx, uint32_t k);  /* 0 without params / an active ring, or k outside 2..16 */
zk_status zk_quorum_prove_batch(zk_ctx *ctx, uint64_t Q, uint32_t k, const uint8_t *msg_hash /*Qkx32*/, const uint8_t *sig /*Qkx64*/, const uint8_t *pk_xy /*Qkx64*/,
                                const uint32_t *which /*Qk*/, const zk_rng *rng /*Qk rows*/, const zk_rng *rng_pairs /*QP rows*/, uint8_t *out, uint64_t out_cap,
                                uint64_t *out_off /*Q+1*/, int32_t *per_quorum_status /*Q*/, int32_t *per_member_status /*Qk or NULL*/);
zk_status zk_quorum_prove_batch_device(zk_ctx *ctx, uint64_t Q, uint32_t k, const void *d_msg_hash, const void *d_sig, const void *d_pk_xy, const void *d_which,
                                       const zk_rng *rng_device, const zk_rng *rng_pairs_device, void *d_out, uint64_t out_cap, void *d_out_off /*u64[Q+1]*/,
                                       void *d_per_quorum_status /*i32[Q]*/, void *d_per_member_status /*i32[Qk] or NULL*/);
zk_status zk_quorum_verify_batch(zk_ctx *ctx, uint64_t Q, uint32_t k, const uint8_t *msg_hash /*Qkx32*/, const uint8_t *bundles, const uint64_t *bundle_off /*Q+1*/,
                                 const uint8_t *verifier_seeds /*Qkx32 or NULL*/, uint8_t *ok /*Q*/, int32_t *per_quorum_status /*Q*/, uint32_t *first_bad /*Q or NULL*/);
zk_status zk_quorum_verify_batch_device(zk_ctx *ctx, uint64_t Q, uint32_t k, const void *d_msg_hash, const void *d_bundles, const void *d_bundle_off /*u64[Q+1]*/,
                                        const void *d_verifier_seeds, void *d_ok, void *d_per_quorum_status /*i32[Q]*/, void *d_first_bad /*u32[Q] or NULL*/);

/* ---- quorum proofs over several rings: one RESIDENT ring id per member (the sharded registry of zk_prove_batch_rings / zk_verify_batch_rings) -- what the
 * zk_quorum_* calls above do not provide.  These calls are named zk_rings_quorum_*: the set of zk_quorum_* names stays the six above.  The wire format
 * is ZKQ1, unchanged: a bundle does not name rings, the verifier is told them as zk_verify_batch_rings is.  Member m = q k + i uses row m of every per-member
 * array, ring_ids included; which[m] indexes the padded size of ring ring_ids[m].  "k different members" means k different KEYS mod q, whatever ring each is
 * shown to be in: a key enrolled in two rings and used through both is refused like a key used twice in one ring.
 * Prover: where quorum q succeeds its bundle is, byte for byte, the 16-byte header, the k proofs zk_prove_batch_rings makes for those members under rng's rows (in
 *   hardened mode each hashes the digest of its own ring), and the P proofs zk_distinct_prove_batch makes under rng_pairs' rows with key = pk_xy[0:32], com = the
 *   member's keyXcom and blinder = what zk_prove_key_blinders gives for the member's row -- in both protocol modes and wire layouts, whatever the comb width or
 *   build.  A quorum's status is the first non-zero one of: its members' zk_prove_batch_rings statuses in member order (ZK_E_ARG for an id that is not resident);
 *   ZK_E_ARG if two of its members have the same key mod q, in the same ring or in different ones; its pairs' statuses in pair order.  A failed quorum gets an
 *   empty slot and the bundles behind it close up.  per_member_status (may be NULL) receives the Q k statuses zk_prove_batch_rings would return.
 * Verifier: the header and inner-header walk is zk_quorum_verify_batch's and needs no ring.  The k members are then verified exactly as zk_verify_batch_rings
 *   verifies them with those ids (verify level, verify reps, seeds row m; ok 0 / ZK_E_ARG for an id that is not resident), the P pairs exactly as
 *   zk_distinct_verify_batch does over the members' keyXcoms; ok, per_quorum_status and first_bad are folded by zk_quorum_verify_batch's rules.
 * When all ring_ids name one ring, both calls return exactly what zk_quorum_prove_batch / zk_quorum_verify_batch return with that ring active.
 * The active ring is neither read nor changed: a context whose rings are all inactive can make both calls (the "no active ring" refusal above does not apply;
 *   ZK_E_BUFFER without params does).
 * Buffer sizes: zk_rings_quorum_proof_max_size(ctx, k, ring_ids) = 16 + the sum of zk_ring_proof_max_size(ctx, ring_ids[i]) over the k members + 744 P, and 0 for
 *   k outside 2..16 or an id that is not resident.  ZK_E_BUFFER when out_cap < the sum over the quorums of (16 + the members' rings' max sizes + 744 P), a member
 *   whose id is not resident counting 0: exact, decided from the ids alone before a byte of any output is written (the _device form: one kernel, one read-back).
 * Call-level rules are zk_quorum_prove_batch's / zk_quorum_verify_batch's: ZK_E_ARG for NULL pointers other than the optional arrays, for k outside 2..16, for
 *   Q k or Q P >= 2^32 and while streamed jobs are queued; _device pointers (d_ring_ids included) in this context's HBM, 4-byte aligned, else ZK_E_ARG; Q = 0 is
 *   ZK_OK with out_off[0] = 0.  A window's attestation staging follows the largest ring the call names.  What is witness-derived -- the gathered keys and
 *   blinders, both RNG fills, the staged inputs, the windows the mixed-ring prover gathers per ring -- is zeroed by zk_ctx_wipe, zk_ctx_destroy and a failed call.
 *   zk_last_timing reports what the inner calls report (zk_prove_batch_rings reports no families for a window that mixes rings), the "quorum_*" families above
 *   and "quorum_caps" for the capacity kernel of the _device prover.
 * Still not provided: submit / wait forms, zk_pool_* forms, JSON, a caller-context binding.  DESIGN.md section 5g'. */
uint64_t zk_rings_quorum_proof_max_size(const zk_ctx *ctx, uint32_t k, const uint32_t *ring_ids /*k*/);
zk_status zk_rings_quorum_prove_batch(zk_ctx *ctx, uint64_t Q, uint32_t k, const uint8_t *msg_hash /*Qkx32*/, const uint8_t *sig /*Qkx64*/, const uint8_t *pk_xy /*Qkx64*/,
                                      const uint32_t *which /*Qk*/, const uint32_t *ring_ids /*Qk*/, const zk_rng *rng /*Qk rows*/, const zk_rng *rng_pairs /*QP rows*/,
                                      uint8_t *out, uint64_t out_cap, uint64_t *out_off /*Q+1*/, int32_t *per_quorum_status /*Q*/,
                                      int32_t *per_member_status /*Qk or NULL*/);
zk_status zk_rings_quorum_prove_batch_device(zk_ctx *ctx, uint64_t Q, uint32_t k, const void *d_msg_hash, const void *d_sig, const void *d_pk_xy, const void *d_which,
                                             const void *d_ring_ids /*u32[Qk]*/, const zk_rng *rng_device, const zk_rng *rng_pairs_device, void *d_out, uint64_t out_cap,
                                             void *d_out_off /*u64[Q+1]*/, void *d_per_quorum_status /*i32[Q]*/, void *d_per_member_status /*i32[Qk] or NULL*/);
zk_status zk_rings_quorum_verify_batch(zk_ctx *ctx, uint64_t Q, uint32_t k, const uint8_t *msg_hash /*Qkx32*/, const uint8_t *bundles, const uint64_t *bundle_off /*Q+1*/,
                                       const uint32_t *ring_ids /*Qk*/, const uint8_t *verifier_seeds /*Qkx32 or NULL*/, uint8_t *ok /*Q*/,
                                       int32_t *per_quorum_status /*Q*/, uint32_t *first_bad /*Q or NULL*/);
zk_status zk_rings_quorum_verify_batch_device(zk_ctx *ctx, uint64_t Q, uint32_t k, const void *d_msg_hash, const void *d_bundles, const void *d_bundle_off /*u64[Q+1]*/,
                                              const void *d_ring_ids /*u32[Qk]*/, const void *d_verifier_seeds, void *d_ok, void *d_per_quorum_status /*i32[Q]*/,
                                              void *d_first_bad /*u32[Q] or NULL*/);

/* ---- escrow tags: let an auditor open which ring member attested.  Every statement above is about a committed key and never says which key it is.  An
 * escrow tag adds the accountable path ("opening" in group signatures and DAA): beside a commitment C = x g + r h -- keyXcom of a ZKA1 proof (its blinder:
 * zk_prove_key_blinders) or a ZKM1 commitment -- the prover puts an exponential ElGamal encryption of x under the key A = a g of a designated auditor and a
 * sigma proof that the ciphertext carries the x of C.  Anyone verifies the tag; only who holds a learns which ring member it is.
 *     E1 = rho g      E2 = x g + rho A      T1 = k_x g + k_r h      T2 = k_rho g      T3 = k_x g + k_rho A
 *     c = hashPoints([C, E1, E2, A, T1, T2, T3])   (the ZKL1 challenge's hash and 80-bit truncation, seven points, this order)
 *     t_x = k_x - c x      t_r = k_r - c r      t_rho = k_rho - c rho      (mod q)
 * Wire format "ZKT1", 472 bytes:
 *     header 16 B : "ZKT1" | total_len u32 big-endian (= 472) | 0 u32 | 0 u32
 *     E1, E2, T1, T2, T3 : five Tom-256 points, 72 bytes each, as A_1 lies in ZKL1
 *     t_x, t_r, t_rho    : 32 bytes big-endian each
 *   always with 36-byte coordinates: zk_ctx_set_wire plays no part.  C travels beside the tag as com1 / com2 do for ZKL1; A is context state.
 * zk_ctx_set_auditor: the auditor's public key as a 72-byte Tom-256 point.  In this order: ZK_E_BUFFER before zk_ctx_set_params; ZK_E_BAD_ENCODING for a
 *   coordinate that is not below the field prime (padding bytes set included) or a point off the curve; ZK_E_ARG for the identity or a point with q A != O
 *   (the curve has cofactor 4).  It builds the comb set of (g, A) on the device (16-bit combs of its own, about 0.13 GB per base; g's table is the context's
 *   where the widths agree).  A second call replaces the key; zk_ctx_set_params drops it, and the escrow calls then give ZK_E_BUFFER until it is set again.
 * zk_escrow_keygen: A = a g for a 32-byte big-endian secret, a REDUCED mod q; ZK_E_BUFFER before zk_ctx_set_params (g is the context's), ZK_E_ARG for
 *   a = 0 mod q.  One comb walk; the staged secret is witness-flagged and zeroed before the call returns.  It needs no auditor key and sets none.
 * zk_escrow_prove_batch: draws under the randomness contract, all mod q with the rejection handling of zk_link_prove_batch: fill 0 is rho, 1 k_x, 2 k_r,
 *   3 k_rho; key and blinder are reduced mod q as newScalar does.  Per tag, in this order; a failed tag gets 472 zero bytes and touches no neighbour:
 *     ZK_E_BAD_ENCODING   com has a coordinate that is not below the field prime (padding bytes set included) or is off the curve.
 *     ZK_E_OPENING        x g + r h is not com (compared as canonical bytes): caught before a tag that cannot verify is written.
 *     ZK_E_RNG_EXHAUSTED  ZK_RNG_STREAM with fewer blocks than the four draws and their rejected fills need.
 *   ZK_E_BUFFER when out_cap < 472 B, or when no auditor is set, before a byte of out or the statuses is written.  The bytes depend neither on
 *   zk_ctx_set_comb_bits, nor on the auditor set's width, nor on the uniform build; ZK_MODE_HARDENED only changes h, as for ZKL1.
 * zk_escrow_verify_batch: per tag ZK_E_BAD_ENCODING for a wrong magic, total_len != 472, a nonzero reserved word, or any of the six points (com, E1, E2, T1,
 *   T2, T3) non-canonical or off the curve.  Scalars >= q are REDUCED mod q, not refused, as in ZKL1.  Otherwise the status is 0 and ok = 1 iff all three
 *   relations hold exactly,
 *     (t_x g + t_r h) + c C - T1 = O      (t_rho g) + c E1 - T2 = O      (t_x g + t_rho A) + c E2 - T3 = O;
 *   there is no verifier randomness and no verifier_seeds argument.  A tag made for auditor A gives ok = 0 under another key.
 * zk_escrow_open_batch: the auditor's call, against the ACTIVE ring.  ZK_E_BUFFER when no auditor is set or no ring is active (before the secret is looked
 *   at).  ZK_E_OPENING at call level, nothing written, when a g is not the context's auditor key; zk_last_timing then holds "escrow_open" alone.
 *   Per tag ZK_E_BAD_ENCODING for the header, E1 or E2 (the index is then 0xffffffff); otherwise status 0 and the index is the lowest i below the ring's key
 *   count with 4 y_i g = 4 E2 - a (4 E1), or 0xffffffff when there is none.  The factor 4 is part of the rule: E1 and E2 come out of a proof and may carry a
 *   component of order 2 or 4 that a prover ground the challenge for until it cancelled in the relations; without the factor such a tag would verify and open
 *   to nobody, with it the prime-order parts decide, and the relations force those to be rho g and x g + rho A with the x of C.  The _device form takes the
 *   secret in HBM as well.  The table of the ring's points 4 y_i g is rebuilt by every call: its residency (and zk_ctx_update_ring's part in it) is left out.
 * What a tag does and does not say.  It is bound to C and to A, not to a message or a ring: it stays valid after zk_proof_rering_batch, because keyXcom is
 *   kept, and it can be copied together with its attestation -- that is the attestation's own replay property.  Opening does not verify: an auditor calls
 *   zk_escrow_verify_batch (and the attestation's verifier) first.  rng must be independent of the seeds C's proof was made with: warning (2) of ZKL1, for
 *   the same reason.  Anyone who knows a can open every tag made for A.
 * Call-level rules are the link calls': ZK_E_ARG for NULL pointers, B >= 2^32 and while streamed jobs are queued; B = 0 is ZK_OK; chunks (zk_ctx_set_chunk) on
 *   the context's lanes.  The _device forms take every pointer and rng->data in this context's HBM, 4-byte aligned, else ZK_E_ARG.  The staged keys, blinders,
 *   draws and RNG fills, the staged secret a and a E1 are witness-derived: zk_ctx_wipe, zk_ctx_destroy and a failed call zero them.  zk_last_timing reports
 *   "rng_prepass", "escrow_front", "tom_commit", "tom_normalize", "hash", "escrow_respond" (prover), "escrow_parse", "tom_commit", "escrow_ladder" (verifier)
 *   and "escrow_open", "escrow_ladder", "tom_normalize", "escrow_ring_points", "escrow_match" (opening).  Not provided: submit / wait, zk_pool_*, JSON.
 * How: six commitments per tag, four on the (g, h) combs and two on the (g, A) set; the verifier runs link_relation on one lane per (tag, relation); the
 *   opening multiplies E1 by the 256-bit secret on one lane per tag, one doubling and one addition per bit, the addend chosen between the base and the
 *   identity by a mask: no branch and no address depends on a bit of a, in every build.  DESIGN.md section 5h. */
zk_status zk_ctx_set_auditor(zk_ctx *ctx, const uint8_t auditor_xy72[72]);
zk_status zk_escrow_keygen(zk_ctx *ctx, const uint8_t secret_be32[32], uint8_t auditor_xy72[72]);
uint64_t zk_escrow_tag_size(void);   /* 472 */
zk_status zk_escrow_prove_batch(zk_ctx *ctx, uint64_t B, const uint8_t *key_be32 /*Bx32*/, const uint8_t *com_xy72 /*Bx72*/, const uint8_t *blinder_be32 /*Bx32*/,
                                const zk_rng *rng, uint8_t *out, uint64_t out_cap, int32_t *per_tag_status /*B*/);
zk_status zk_escrow_prove_batch_device(zk_ctx *ctx, uint64_t B, const void *d_key_be32, const void *d_com_xy72, const void *d_blinder_be32, const zk_rng *rng_device,
                                       void *d_out, uint64_t out_cap, void *d_per_tag_status /*i32[B]*/);
zk_status zk_escrow_verify_batch(zk_ctx *ctx, uint64_t B, const uint8_t *com_xy72 /*Bx72*/, const uint8_t *tags /*Bx472*/, uint8_t *ok /*B*/,
                                 int32_t *per_tag_status /*B*/);
zk_status zk_escrow_verify_batch_device(zk_ctx *ctx, uint64_t B, const void *d_com_xy72, const void *d_tags, void *d_ok, void *d_per_tag_status /*i32[B]*/);
zk_status zk_escrow_open_batch(zk_ctx *ctx, uint64_t B, const uint8_t secret_be32[32], const uint8_t *tags /*Bx472*/, uint32_t *index_u32 /*B*/,
                               int32_t *per_tag_status /*B*/);
zk_status zk_escrow_open_batch_device(zk_ctx *ctx, uint64_t B, const void *d_secret_be32, const void *d_tags, void *d_index_u32 /*u32[B]*/,
                                      void *d_per_tag_status /*i32[B]*/);

/* ---- opening escrow tags against any resident ring: one resident ring id per tag, through a resident point index.  The auditor of a registry sharded over
 * the resident rings (zk_ctx_add_ring; zk_prove_batch_rings -> tags -> zk_verify_batch_rings) opens a mixed batch in ONE call: the 256-bit ladder a E1, the
 * largest part of an opening and independent of the ring, runs once per tag, and the tag's point is looked up in the ring its id names.
 * ring_ids[b] is the id of a resident ring, or ZK_ESCROW_RING_ANY: the resident rings are then searched in ascending id order and the first one that holds the
 *   key answers.  The ACTIVE ring is neither read nor changed, and "no active ring" is no refusal.
 * Per tag, in this order: ZK_E_ARG when ring_ids[b] is neither resident nor ZK_ESCROW_RING_ANY (before the tag's bytes are judged); ZK_E_BAD_ENCODING for the
 *   header, E1 or E2; otherwise 0.  ring_out and index are both 0xffffffff unless the status is 0 and a match exists; then index is the lowest i below that
 *   ring's key count with 4 y_i g = 4 E2 - a (4 E1) -- the rule, its factor 4 and its warnings are zk_escrow_open_batch's -- and ring_out the ring's id.
 * Call level: zk_escrow_open_batch's rules (ZK_E_BUFFER without parameters or an auditor key, ZK_E_OPENING with nothing written for a secret that is not the
 *   auditor key's, B = 0 is ZK_OK, ZK_E_ARG for NULL pointers and while streamed jobs are queued; the staged secret, a E1 and the tags' points are
 *   witness-derived and wiped as there).  The _device form takes every pointer and the secret in this context's HBM, 4-byte aligned, else ZK_E_ARG.
 * The point index.  The call first builds the index of every resident ring that lacks one (a failed allocation is the call's failure, ZK_E_DEVICE, nothing
 *   written): the ring's affine points 4 y_i g, 72 bytes per entry of the padded ring, and an open-addressed table of u32 key indices over them with twice as
 *   many slots as the padded ring has entries (a power of two, at least twice the key count), 0xffffffff for an empty slot, linear probing with wrap-around.
 *   The home slot of a point is a function of the two low 32-bit words w0, w1 of its canonical x:
 *       h = w0 * 0x9e3779b1 + w1 * 0x85ebca6b;  h ^= h >> 16;  h *= 0xc2b2ae35;  h ^= h >> 13  (mod 2^32);  slot = h & (slots - 1)
 *   (csrc/escrow_index.h is its one definition).  Every distinct point owns one slot, which holds its lowest index; a crafted ring whose points share a home
 *   slot lengthens probes -- bounded by the slot count -- and changes no answer.  The index depends on g and the ring only: it is public, not wiped, and is
 *   kept from call to call.  zk_ctx_update_ring patches it where the padded size stays (the touched keys' points are recomputed and the slots refilled from
 *   the resident points; no tombstones); every rebuild of a ring (a size change, zk_ctx_set_ring) and zk_ctx_set_params drop it, and the next call builds
 *   it again.  A ring that no such call has named in a context costs nothing: zk_ctx_add_ring, zk_ctx_set_ring and zk_ring_info are unchanged.
 * zk_last_timing: "escrow_index_build" (only in a call that built one), "escrow_open", "escrow_ladder", "tom_normalize", "escrow_lookup".
 * Not provided: pool, streamed and JSON forms.  DESIGN.md section 5h'. */
#define ZK_ESCROW_RING_ANY 0xffffffffu
zk_status zk_rings_escrow_open_batch(zk_ctx *ctx, uint64_t B, const uint8_t secret_be32[32], const uint8_t *tags /*Bx472*/, const uint32_t *ring_ids /*B*/,
                                     uint32_t *ring_out_u32 /*B*/, uint32_t *index_u32 /*B*/, int32_t *per_tag_status /*B*/);
zk_status zk_rings_escrow_open_batch_device(zk_ctx *ctx, uint64_t B, const void *d_secret_be32, const void *d_tags, const void *d_ring_ids /*u32[B]*/,
                                            void *d_ring_out_u32 /*u32[B]*/, void *d_index_u32 /*u32[B]*/, void *d_per_tag_status /*i32[B]*/);

/* ---- threshold escrow opening: t of n auditors open a tag.  Anyone who knows a can open every tag made for A (above); here a is split once, by a dealer,
 * into Shamir shares a_1 .. a_n, and opening takes t of the n auditors.  From a tag, auditor j makes a partial opening D_j = a_j E1 and a Chaum-Pedersen proof
 * (a share, "ZKS1") that D_j was made with the secret behind the published key A_j = a_j g.  Anyone can verify a share; anyone who holds t verified shares of a
 * tag can combine them into the ring and index zk_rings_escrow_open_batch gives.  Provers, tags, verifiers and the single-auditor calls do not change: a ZKT1
 * tag made for A is opened either way.  With q the group order and 1 <= t <= n <= 16:
 *     split:    f(X) = a + c_1 X + ... + c_{t-1} X^{t-1};  a_j = f(j) mod q,  A_j = a_j g,  j = 1..n
 *     share:    D = a_j E1    U1 = k g    U2 = k E1    c = hashPoints([A_j, E1, D, U1, U2])    s = k - c a_j  (mod q)
 *               (the ZKL1 challenge's hash and 80-bit truncation, five points, this order)
 *     verify:   s g + c A_j - U1 = O   and   s E1 + c D - U2 = O
 *     combine:  lambda_j = prod_{m in S, m != j} m / (m - j)  (mod q);   M = 4 (E2 - sum_{j in S} lambda_j D_j)   for a set S of exactly t different auditors
 * Wire format "ZKS1", 264 bytes:
 *     header 16 B : "ZKS1" | total_len u32 big-endian (= 264) | j u32 big-endian | 0 u32
 *     D, U1, U2   : three Tom-256 points, 72 bytes each, as the points lie in ZKT1
 *     s           : 32 bytes big-endian
 * zk_auditors_split_key: the dealer's call; it works as zk_escrow_keygen does and needs parameters only (ZK_E_BUFFER before zk_ctx_set_params).  a is REDUCED
 *   mod q; the coefficients c_1 .. c_{t-1} are rnd(q) draws, fills 0 .. t-2 of the call's rng under the randomness contract (rng->data: one 32-byte seed, or
 *   one stream of stride_blocks blocks), rejection handled as in zk_link_prove_batch; ZK_E_RNG_EXHAUSTED, nothing written, for a stream that does not hold
 *   them; ZK_E_ARG unless 1 <= t <= n <= 16.  A share a_j = 0 is possible only with negligible probability: it is returned as it is, and
 *   zk_ctx_set_auditors refuses its key.  Everything the call stages is witness-flagged and zeroed before it returns.  The dealer sees a: distributed key
 *   generation is not provided.
 * zk_ctx_set_auditors: the n share keys.  It needs an auditor key (zk_ctx_set_auditor), else ZK_E_BUFFER; ZK_E_ARG unless 1 <= t <= n <= 16.  Every A_j is
 *   checked as zk_ctx_set_auditor checks A (ZK_E_BAD_ENCODING; ZK_E_ARG for the identity or q A_j != O), and the keys must lie on one polynomial of degree
 *   t - 1 through A: interpolating A_1 .. A_t at 0 gives A and at every m > t gives A_m -- n - t + 1 sums through the combine's ladder, compared as canonical
 *   bytes.  A mismatch is ZK_E_OPENING, and nothing is kept: a call that fails behind its argument checks leaves the context without a set.
 *   zk_ctx_set_auditor and zk_ctx_set_params drop the set.
 * zk_auditors_share_batch: auditor j's shares of B tags.  Call level, in this order: ZK_E_BUFFER without an auditor set; ZK_E_ARG for j outside 1..n;
 *   ZK_E_OPENING with nothing written when a_j g is not A_j; ZK_E_BUFFER for out_cap < 264 B.  Per tag, in this order: ZK_E_BAD_ENCODING for the tag's header
 *   or E1; ZK_E_RNG_EXHAUSTED.  k = rnd(q) is fill 0 of the tag's rng.  A failed share is 264 zero bytes and touches no neighbour.  Both a_j E1 and k E1 go
 *   through the masked ladder of the single-auditor opening: no branch and no address depends on a bit of a_j or k, in every build; a refused tag walks the
 *   identity.  U1 comes from the (g, h) comb with r = 0.  The bytes depend on neither the comb widths, nor the mode (h plays no part), nor the uniform build.
 * zk_auditors_share_verify_batch: a share against the tag it belongs to and the context's A_j, j from the share's header.  Per share ZK_E_BAD_ENCODING for the
 *   share's header (magic, total_len != 264, a nonzero reserved word, j outside 1..n), the tag's header, or any of the points E1, D, U1, U2 non-canonical or
 *   off the curve.  A scalar s >= q is REDUCED, not refused.  Otherwise the status is 0 and ok = 1 iff both relations hold exactly; there is no verifier
 *   randomness.  Relation 1 is one comb opening plus the link verifier's short ladder on A_j, relation 2 the two-base ladder of the distinct-key verifier.
 * zk_auditors_combine_batch: shares holds t slots of B shares, slot-major: share b of slot s lies at (s B + b) x 264 and belongs to auditors[s].  Call level:
 *   ZK_E_ARG when t is not the context's threshold, or when auditors holds a 0, a value above n, or a duplicate; the rest of the call-level rules are
 *   zk_rings_escrow_open_batch's: the ACTIVE ring is neither read nor changed, and missing point indexes are built first.  Per tag, in this order: ZK_E_ARG
 *   for a ring id that is neither resident nor ZK_ESCROW_RING_ANY; ZK_E_BAD_ENCODING for the tag's header, E1 or E2, for any slot's share header (j !=
 *   auditors[s] included), or for a D that is non-canonical or off the curve; else 0.  M is looked up exactly as zk_rings_escrow_open_batch looks up its
 *   point: lowest index, both outputs 0xffffffff where there is none.  The lambda_j are computed once per call; they are public.  One lane per tag walks
 *   sum lambda_j D_j as one joint left-to-right ladder that shares the 256 doublings; its branches on the bits of lambda are wave-uniform.  The factor 4 is
 *   part of the rule for the reason it is in the single-auditor rule: E1, and a D_j that a dishonest auditor adjusted, may carry a component of order 2 or 4.
 * Combining does not verify, as opening does not: run zk_auditors_share_verify_batch first.  A wrong D_j then shows as "no member" or, for a party that
 *   already knows the key, as whatever member it chooses.  A share reveals a_j E1 for that tag only.
 * Call-level rules are the link calls': ZK_E_ARG for NULL pointers, B >= 2^32 and while streamed jobs are queued; B = 0 is ZK_OK; chunks on the context's
 *   lanes; the _device forms take every pointer (auditors and rng->data included) in this context's HBM, 4-byte aligned, else ZK_E_ARG.  The staged a_j, k and
 *   the RNG fills are witness-derived: zk_ctx_wipe, zk_ctx_destroy and a failed call zero them.  zk_last_timing reports "rng_prepass", "escrow_open",
 *   "share_front", "tom_commit", "share_ladder", "tom_normalize", "hash", "share_respond" (share), "share_parse", "tom_commit", "share_relations" (verify)
 *   and "escrow_index_build", "combine_ladder", "tom_normalize", "escrow_lookup" (combine).
 * Not provided: distributed key generation, resharing, pool, streamed and JSON forms.  DESIGN.md section 5h''. */
uint64_t zk_auditors_share_size(void);   /* 264 */
zk_status zk_auditors_split_key(zk_ctx *ctx, const uint8_t secret_be32[32], uint32_t t, uint32_t n, const zk_rng *rng, uint8_t *shares_be32 /*nx32*/,
                                uint8_t *share_keys_xy72 /*nx72*/);
zk_status zk_ctx_set_auditors(zk_ctx *ctx, uint32_t t, uint32_t n, const uint8_t *share_keys_xy72 /*nx72*/);
zk_status zk_auditors_share_batch(zk_ctx *ctx, uint64_t B, uint32_t j, const uint8_t share_secret_be32[32], const uint8_t *tags /*Bx472*/, const zk_rng *rng,
                                  uint8_t *out /*Bx264*/, uint64_t out_cap, int32_t *per_tag_status /*B*/);
zk_status zk_auditors_share_batch_device(zk_ctx *ctx, uint64_t B, uint32_t j, const void *d_share_secret_be32, const void *d_tags, const zk_rng *rng_device,
                                         void *d_out, uint64_t out_cap, void *d_per_tag_status /*i32[B]*/);
zk_status zk_auditors_share_verify_batch(zk_ctx *ctx, uint64_t B, const uint8_t *tags /*Bx472*/, const uint8_t *shares /*Bx264*/, uint8_t *ok /*B*/,
                                         int32_t *per_share_status /*B*/);
zk_status zk_auditors_share_verify_batch_device(zk_ctx *ctx, uint64_t B, const void *d_tags, const void *d_shares, void *d_ok, void *d_per_share_status /*i32[B]*/);
zk_status zk_auditors_combine_batch(zk_ctx *ctx, uint64_t B, uint32_t t, const uint32_t *auditors_u32 /*t*/, const uint8_t *tags /*Bx472*/,
                                    const uint8_t *shares /*txBx264*/, const uint32_t *ring_ids /*B*/, uint32_t *ring_out_u32 /*B*/, uint32_t *index_u32 /*B*/,
                                    int32_t *per_tag_status /*B*/);
zk_status zk_auditors_combine_batch_device(zk_ctx *ctx, uint64_t B, uint32_t t, const void *d_auditors_u32 /*u32[t]*/, const void *d_tags, const void *d_shares,
                                           const void *d_ring_ids /*u32[B]*/, void *d_ring_out_u32 /*u32[B]*/, void *d_index_u32 /*u32[B]*/,
                                           void *d_per_tag_status /*i32[B]*/);

/* ---- accountable attestations: an attestation that CARRIES its escrow tag, as one artifact.  The recipe of INTEGRATION.md "Accountable attestations" --
 * zk_prove_batch, zk_prove_key_blinders with the same seeds, zk_proof_key_commitments, zk_escrow_prove_batch with key = pk_xy[0:32] (and zk_verify_batch,
 * zk_proof_key_commitments, zk_escrow_verify_batch for the verifier) -- as one prove call and one verify call with a wire format of its own; keys, blinders
 * and keyXcoms are gathered and the two verdicts folded on the device.  No existing call changes, a ZKT1 tag stays byte for byte what it is, and every
 * auditor call (zk_escrow_open_batch, zk_rings_escrow_open_batch, zk_auditors_share_batch, zk_auditors_share_verify_batch, zk_auditors_combine_batch) works
 * on the tags zk_accountable_split_batch takes out of bundles.
 * Wire format "ZKC1" (a bundle):
 *     header 16 B : "ZKC1" | total_len u32 big-endian | 0 u32 | 0 u32
 *     attestation : one ZKA1 / ZK1P proof in the context's wire layout (zk_ctx_set_wire), exactly as zk_prove_batch writes it (its own total_len, a multiple
 *                   of 4)
 *     tag 472 B   : one ZKT1 tag, exactly as zk_escrow_prove_batch writes it, for C = the keyXcom inside that attestation (read by the rules of
 *                   zk_proof_key_commitments) and the context's auditor key A
 *   C is not repeated, so a tag can only be checked against the attestation it travels with.  An attestation's length varies with the Exp challenge, so a
 *   bundle's length varies; zk_accountable_proof_max_size(ctx) = 16 + zk_proof_max_size(ctx) + 472.
 * Bundle b uses row b of msg_hash, sig, pk_xy, which, rng and rng_tags.
 * zk_accountable_prove_batch: where proof b succeeds its bundle is, byte for byte, the header, the proof zk_prove_batch makes for row b of rng with the
 *   active ring, and the tag zk_escrow_prove_batch makes under row b of rng_tags with key = pk_xy[64 b : 64 b + 32], com = that proof's keyXcom and blinder =
 *   what zk_prove_key_blinders gives for row b: the bytes of the recipe, in both protocol modes and wire layouts, whatever the comb width or build.
 *   per_proof_status is the first non-zero one of the attestation's status, then the tag's (ZK_E_RNG_EXHAUSTED on a short rng_tags stream).  A failed bundle
 *   gets an empty slot (out_off[b + 1] = out_off[b]), the bundles behind it close up, no neighbour's byte changes.  per_part_status (may be NULL) receives
 *   both statuses: 2 b the attestation's, 2 b + 1 the tag's as zk_escrow_prove_batch reports it (for the all-zero commitment of a failed attestation too).
 *   ZK_E_BUFFER, before a byte of any output is written: out_cap < B zk_accountable_proof_max_size, no params, no active ring, no auditor key.
 * zk_accountable_verify_batch: per bundle, the first rule that matches:
 *     ZK_E_BAD_ENCODING with ok 0 and first_bad 0, no byte outside the slot read: a wrong magic, total_len != the slot's length, a non-zero reserved word, a
 *       slot offset or length that is no multiple of 4 or offsets that do not ascend, or an inner header (magic of the context's layout, total_len, the rules
 *       of zk_proof_rering_batch) that does not walk from byte 16 exactly to total_len - 472.
 *   Otherwise the attestation is verified exactly as zk_verify_batch verifies it (the active ring, zk_ctx_set_verify_level and zk_ctx_set_verify_reps,
 *   verifier_seeds row b or the library's own) and the tag exactly as zk_escrow_verify_batch does against the attestation's keyXcom.  ok = 1 iff both parts
 *   are ok; per_proof_status is the first non-zero one, attestation before tag; first_bad (may be NULL) is 0 for the attestation, 1 for the tag and
 *   0xFFFFFFFF where ok = 1.  ZK_E_BUFFER without params, an active ring or an auditor key.
 * zk_accountable_split_batch and zk_accountable_join_batch are pure layout: they prove nothing and check no curve, and need neither params nor a ring nor
 *   an auditor key -- only the context's wire layout.  Split applies the verifier's walk: the attestations come out back to back (att_off, B + 1 entries),
 *   ready for zk_verify_batch, zk_verify_batch_rings and zk_proof_rering_batch, the tags dense at 472 b, ready for every auditor call; a refused bundle is
 *   ZK_E_BAD_ENCODING, an empty attestation slot and 472 zero bytes.  ZK_E_BUFFER, before a byte is written, when att_cap is less than the sum of
 *   (slot length - 488) over the slots of at least 520 bytes: what the offsets alone allow.  Join checks the proof's header by the rules of
 *   zk_proof_rering_batch and the tag's 16 header bytes ("ZKT1" | 472 | 0 | 0); it refuses with ZK_E_BAD_ENCODING and an empty slot.  ZK_E_BUFFER when
 *   out_cap is less than the sum of (slot length + 488) over the readable slots.  join(split(x)) = x and split(join(p, t)) = (p, t).  A tag is bound to
 *   keyXcom and A, not to the ring: split, zk_proof_rering_batch, join moves an accountable attestation to another ring with its tag intact, and split /
 *   join are how a sharded registry (zk_prove_batch_rings, zk_verify_batch_rings) uses ZKC1.  Input and output buffers must not overlap.
 * Call-level rules are the quorum prover's: ZK_E_ARG for NULL pointers other than the optional arrays, for B >= 2^32 and while streamed jobs are queued; B = 0
 *   is ZK_OK with out_off[0] = 0 (att_off[0] = 0).  The _device forms take every pointer, both rng->data included, in this context's HBM, 4-byte aligned, else
 *   ZK_E_ARG.  A call runs in windows of at most chunk x lanes bundles; what is witness-derived -- the staged keys and blinders, both RNG fills, the tag
 *   prover's arena, the staged inputs -- is zeroed by zk_ctx_wipe, zk_ctx_destroy and a failed call.  zk_last_timing reports the families of the calls above
 *   plus "accountable_blinders", "accountable_layout" (prover, join) and "accountable_walk", "accountable_verdict" (verifier, split, join).
 * Not provided: one ring id per proof, tags inside ZKQ1 bundles, submit / wait, zk_pool_* and JSON forms, opening straight from bundles (split first), a
 *   caller-context binding.
 * Warning (2) of ZKL1 applies: rng_tags must be independent of rng -- with an attestation's own seed the fills that blinded it would come back as a tag's
 *   rho and nonces.  A bundle tells the auditor, and nobody else, which ring member attested.  DESIGN.md section 5h'''. */
uint64_t zk_accountable_proof_max_size(const zk_ctx *ctx);   /* 0 without params / an active ring */
zk_status zk_accountable_prove_batch(zk_ctx *ctx, uint64_t B, const uint8_t *msg_hash /*Bx32*/, const uint8_t *sig /*Bx64*/, const uint8_t *pk_xy /*Bx64*/,
                                     const uint32_t *which /*B*/, const zk_rng *rng, const zk_rng *rng_tags, uint8_t *out, uint64_t out_cap,
                                     uint64_t *out_off /*B+1*/, int32_t *per_proof_status /*B*/, int32_t *per_part_status /*2B or NULL*/);
zk_status zk_accountable_prove_batch_device(zk_ctx *ctx, uint64_t B, const void *d_msg_hash, const void *d_sig, const void *d_pk_xy, const void *d_which,
                                            const zk_rng *rng_device, const zk_rng *rng_tags_device, void *d_out, uint64_t out_cap,
                                            void *d_out_off /*u64[B+1]*/, void *d_per_proof_status /*i32[B]*/, void *d_per_part_status /*i32[2B] or NULL*/);
zk_status zk_accountable_verify_batch(zk_ctx *ctx, uint64_t B, const uint8_t *msg_hash /*Bx32*/, const uint8_t *bundles, const uint64_t *bundle_off /*B+1*/,
                                      const uint8_t *verifier_seeds /*Bx32 or NULL*/, uint8_t *ok /*B*/, int32_t *per_proof_status /*B*/,
                                      uint32_t *first_bad /*B or NULL*/);
zk_status zk_accountable_verify_batch_device(zk_ctx *ctx, uint64_t B, const void *d_msg_hash, const void *d_bundles, const void *d_bundle_off /*u64[B+1]*/,
                                             const void *d_verifier_seeds, void *d_ok, void *d_per_proof_status /*i32[B]*/, void *d_first_bad /*u32[B] or NULL*/);
zk_status zk_accountable_split_batch(zk_ctx *ctx, uint64_t B, const uint8_t *bundles, const uint64_t *bundle_off /*B+1*/, uint8_t *att_out, uint64_t att_cap,
                                     uint64_t *att_off /*B+1*/, uint8_t *tags_out /*Bx472*/, int32_t *per_proof_status /*B*/);
zk_status zk_accountable_split_batch_device(zk_ctx *ctx, uint64_t B, const void *d_bundles, const void *d_bundle_off /*u64[B+1]*/, void *d_att_out,
                                            uint64_t att_cap, void *d_att_off /*u64[B+1]*/, void *d_tags_out, void *d_per_proof_status /*i32[B]*/);
zk_status zk_accountable_join_batch(zk_ctx *ctx, uint64_t B, const uint8_t *proofs, const uint64_t *proof_off /*B+1*/, const uint8_t *tags /*Bx472*/,
                                    uint8_t *out, uint64_t out_cap, uint64_t *out_off /*B+1*/, int32_t *per_proof_status /*B*/);
zk_status zk_accountable_join_batch_device(zk_ctx *ctx, uint64_t B, const void *d_proofs, const void *d_proof_off /*u64[B+1]*/, const void *d_tags, void *d_out,
                                           uint64_t out_cap, void *d_out_off /*u64[B+1]*/, void *d_per_proof_status /*i32[B]*/);
/* The `_rings` forms of the above -- one resident ring id per bundle, no active ring, and the auditor's opening straight from bundles -- are the
 * zk_rings_accountable_* calls.  Their declarations and their contract are in zkattest_rings_accountable.h, which is part of this header. */
#include "zkattest_rings_accountable.h"

/* ---- two (or more) batches in flight on one context.  zk_prove_batch / zk_verify_batch are synchronous: each call pays its own head
 * (no byte of a chunk exists before its stage 1 is over) and its own tail (the copies of the last slices, with nothing left to
 * hide them).  The submit / wait pair splits a call so that the pipeline keeps running ACROSS calls: submit stages the inputs and
 * queues the job (the verifier's proof bytes start crossing PCIe at once, right behind the bytes of the job before), wait drives the
 * job's chunks -- enqueueing stage 1 of the NEXT job's first chunks while this job's last chunks are in their output phase -- and
 * hands the results back.  Steady state:  submit(0); submit(1); wait(0); submit(2); wait(1); submit(3); wait(2); ...
 * Rules: one thread per context; waits in submission order; at most 4 jobs queued; jobs of one kind (prove or verify) at a time;
 * `out` / `proofs` page-locked (zk_host_alloc; ZK_E_ARG otherwise); every pointer of a job -- inputs included -- stays valid and
 * untouched until its wait returns; chunk, lanes, parameters and ring do not change while jobs are queued; the synchronous calls
 * return ZK_E_ARG while jobs are queued.  Bytes, statuses and verdicts are those of the synchronous calls.  zk_ctx_destroy abandons
 * queued jobs.  (The reference proves one signature per call on one thread, src/zkpAttestList.ts:104-145: no counterpart.) */
typedef struct zk_job zk_job;
zk_status zk_prove_submit(zk_ctx *ctx, uint64_t B, const uint8_t *msg_hash, const uint8_t *sig, const uint8_t *pk_xy, const uint32_t *which,
                          const zk_rng *rng, uint8_t *out, uint64_t out_cap, uint64_t *out_off /*B+1*/, int32_t *per_proof_status /*B*/, zk_job **job);
/* the same job with every buffer already in HBM (zk_prove_batch_device's arguments; rng->data is a device pointer): nothing crosses
 * the link, consecutive batches keep the lanes' pipelines full.  The buffers must be complete when the call is made. */
zk_status zk_prove_submit_device(zk_ctx *ctx, uint64_t B, const uint8_t *d_msg_hash, const uint8_t *d_sig, const uint8_t *d_pk_xy, const uint32_t *d_which,
                                 const zk_rng *rng, uint8_t *d_out, uint64_t out_cap, uint64_t *d_out_off /*B+1*/, int32_t *d_per_proof_status /*B*/,
                                 zk_job **job);
zk_status zk_prove_wait(zk_ctx *ctx, zk_job *job);   /* the job is released whatever the result */
zk_status zk_verify_submit(zk_ctx *ctx, uint64_t B, const uint8_t *msg_hash, const uint8_t *proofs, const uint64_t *proof_off /*B+1*/,
                           const uint8_t *verifier_seeds /*Bx32 or NULL*/, uint8_t *ok /*B*/, int32_t *per_proof_status /*B*/, zk_job **job);
zk_status zk_verify_wait(zk_ctx *ctx, zk_job *job);

/* ---- several GPUs of one node behind one handle (the reference is single-threaded,
 * src/zkpAttestList.ts:104-145 proves one signature per call).  Proofs are independent given (params, ring): a batch is split
 * into contiguous shards, shard i = proofs [i*B/G, (i+1)*B/G) on device_ids[i], one host thread per device, no exchange while
 * proving or verifying.  zk_pool_set_ring uploads the ring once and broadcasts it device-to-device (RCCL ncclBroadcast over
 * xGMI; hipMemcpyPeer when RCCL is not usable -- zk_pool_ring_transport tells which: "rccl", "peer-copy", "single");
 * fixed-base tables and the per-ring table are rebuilt locally on every device, concurrently.  zk_pool_ctx(i) gives the
 * per-device context for the settings above (chunk, lanes, comb width: before zk_pool_set_params) and for zk_last_error.
 * A pool call is not re-entrant; the listed devices may repeat (several contexts on one GPU). */
typedef struct zk_pool zk_pool;
zk_status zk_pool_create(const int *device_ids, int n_dev, zk_pool **out);   /* *out = NULL on failure (never a half-built pool) */
void zk_pool_destroy(zk_pool *pool);
int zk_pool_size(const zk_pool *pool);
zk_ctx *zk_pool_ctx(zk_pool *pool, int i);
const char *zk_pool_last_error(const zk_pool *pool);                        /* pool = NULL: why this thread's last zk_pool_create failed;
                                                                             * after a zk_pool_set_ring whose transport is not "rccl": why RCCL was not used */
/* Host side of a shard.  Every shard of a pool call runs on its own host thread, bound to the CPUs next to its device (sysfs
 * local_cpulist of the device's PCI address; ZKATTEST_POOL_AFFINITY=0 switches the binding off).  zk_pool_host_alloc returns a
 * page-locked buffer for `out` of zk_pool_prove_batch / `proofs` of zk_pool_verify_batch whose per-shard regions
 * [i * R, (i+1) * R), R = (bytes / G) & ~255, were first touched on the NUMA node of device i, so that the ~40 GB/s of proof
 * bytes per device stay on that device's socket.  Free with zk_pool_host_free.  zk_pool_numa_node: -1 = unknown. */
void *zk_pool_host_alloc(zk_pool *pool, size_t bytes);
void zk_pool_host_free(void *p);
int zk_pool_numa_node(const zk_pool *pool, int i);
/* wall milliseconds every shard's host thread spent in its part of the last pool call (set_params, set_ring, prove, verify);
 * returns the number of shards */
int zk_pool_shard_ms(const zk_pool *pool, float *ms, int cap);
const char *zk_pool_ring_transport(const zk_pool *pool);
/* the file the nccl* entry points were taken from ("" while RCCL was never loaded).  zk_pool_set_ring looks for librccl in this order: the path in
 * ZKATTEST_RCCL_LIB (if it cannot be loaded RCCL is not used at all); a librccl the process has already mapped (under PyTorch: the wheel's own, bound to
 * the HIP runtime this library is then running on as well); the system's librccl.so.1.  ZKATTEST_NO_RCCL=1 goes straight to peer copies. */
const char *zk_pool_rccl_library(const zk_pool *pool);
void zk_pool_shard(const zk_pool *pool, uint64_t B, int i, uint64_t *first, uint64_t *count);
zk_status zk_pool_set_params(zk_pool *pool, const uint8_t nist_h[64], const uint8_t tom_g[72], const uint8_t tom_h[72], uint32_t sec_level);
zk_status zk_pool_set_ring(zk_pool *pool, const uint8_t *keys_be32, uint64_t n_keys);
zk_status zk_pool_set_verify_level(zk_pool *pool, uint32_t mode);   /* zk_ctx_set_verify_level on every shard context */
zk_status zk_pool_set_verify_reps(zk_pool *pool, uint32_t mode);    /* zk_ctx_set_verify_reps on every shard context */
zk_status zk_pool_add_ring(zk_pool *pool, const uint8_t *keys_be32, uint64_t n_keys, uint32_t *ring);   /* resident rings: see zk_ctx_add_ring */
zk_status zk_pool_use_ring(zk_pool *pool, uint32_t ring);
zk_status zk_pool_drop_ring(zk_pool *pool, uint32_t ring);
zk_status zk_pool_update_ring(zk_pool *pool, uint32_t ring, uint64_t count, const uint64_t *index /*count*/, const uint8_t *keys_be32 /*count x 32*/,
                              uint64_t new_n_keys);   /* see zk_ctx_update_ring */
/* zk_prove_batch over all devices.  Shard i writes its proofs back to back from out + i * ((out_cap / G) & ~255): proof b lies
 * at out_off[b] .. out_off[b] + out_len[b] (its ZKA1 header carries the same length); there are gaps between shards, none
 * inside one.  ZK_E_BUFFER when a shard does not fit its region.  `out` from zk_host_alloc is filled by overlapped DMA. */
zk_status zk_pool_prove_batch(zk_pool *pool, uint64_t B, const uint8_t *msg_hash, const uint8_t *sig, const uint8_t *pk_xy, const uint32_t *which,
                              const zk_rng *rng, uint8_t *out, uint64_t out_cap, uint64_t *out_off /*B*/, uint64_t *out_len /*B*/,
                              int32_t *per_proof_status /*B*/);
/* zk_prove_batch_rings over all devices, with the output layout of zk_pool_prove_batch */
zk_status zk_pool_prove_batch_rings(zk_pool *pool, uint64_t B, const uint8_t *msg_hash, const uint8_t *sig, const uint8_t *pk_xy, const uint32_t *which,
                                    const uint32_t *ring_ids /*B*/, const zk_rng *rng, uint8_t *out, uint64_t out_cap, uint64_t *out_off /*B*/,
                                    uint64_t *out_len /*B*/, int32_t *per_proof_status /*B*/);
/* The same with the proofs left in HBM: shard i writes its proofs back to back from d_out[i], a buffer of out_cap[i] bytes on
 * device_ids[i] (zk_pool_device_alloc / zk_pool_device_free); out_off[b] is relative to the proof's own shard buffer.  Only the 160 bytes of
 * inputs per proof cross PCIe: through this entry point a multi-GPU run measures the GPUs and their host threads without the node's host
 * memory (eight shards of zk_pool_prove_batch emit ~55 GB/s of page-locked writes each).  zk_prove_batch accepts a
 * device-resident `out` the same way for one context. */
zk_status zk_pool_prove_batch_device(zk_pool *pool, uint64_t B, const uint8_t *msg_hash, const uint8_t *sig, const uint8_t *pk_xy, const uint32_t *which,
                                     const zk_rng *rng, void *const *d_out /*G*/, const uint64_t *out_cap /*G*/, uint64_t *out_off /*B*/, uint64_t *out_len /*B*/,
                                     int32_t *per_proof_status /*B*/);
void *zk_pool_device_alloc(zk_pool *pool, int i, size_t bytes);   /* hipMalloc on device_ids[i]; the calling thread's current device is kept */
void zk_pool_device_free(zk_pool *pool, int i, void *p);
/* zk_verify_batch over all devices.  Inside every shard the proofs must lie back to back in index order (true for the output
 * of zk_pool_prove_batch and for any fully packed buffer), every shard starting 4-byte aligned; ZK_E_ARG otherwise. */
zk_status zk_pool_verify_batch(zk_pool *pool, uint64_t B, const uint8_t *msg_hash, const uint8_t *proofs, const uint64_t *proof_off /*B*/,
                               const uint64_t *proof_len /*B*/, const uint8_t *verifier_seeds /*Bx32 or NULL*/, uint8_t *ok /*B*/,
                               int32_t *per_proof_status /*B*/);
/* zk_verify_batch_rings over all devices, with the packing rules of zk_pool_verify_batch */
zk_status zk_pool_verify_batch_rings(zk_pool *pool, uint64_t B, const uint8_t *msg_hash, const uint8_t *proofs, const uint64_t *proof_off /*B*/,
                                     const uint64_t *proof_len /*B*/, const uint32_t *ring_ids /*B*/, const uint8_t *verifier_seeds /*Bx32 or NULL*/,
                                     uint8_t *ok /*B*/, int32_t *per_proof_status /*B*/);

/* The streamed form of the two pool calls (see "two batches in flight"): every device's shard goes through zk_prove_submit / zk_prove_wait on
 * its own context, so a node keeps two or three batches in flight per GPU.  Same rules per device (waits in submission order, `out` /
 * `proofs` page-locked -- zk_pool_host_alloc --, every pointer valid until the wait returns); (out_off, out_len) are filled by the wait. */
typedef struct zk_pool_job zk_pool_job;
zk_status zk_pool_prove_submit(zk_pool *pool, uint64_t B, const uint8_t *msg_hash, const uint8_t *sig, const uint8_t *pk_xy, const uint32_t *which, const zk_rng *rng,
                               uint8_t *out, uint64_t out_cap, uint64_t *out_off /*B*/, uint64_t *out_len /*B*/, int32_t *per_proof_status /*B*/, zk_pool_job **job);
zk_status zk_pool_prove_wait(zk_pool *pool, zk_pool_job *job);
zk_status zk_pool_verify_submit(zk_pool *pool, uint64_t B, const uint8_t *msg_hash, const uint8_t *proofs, const uint64_t *proof_off /*B*/, const uint64_t *proof_len /*B*/,
                                const uint8_t *verifier_seeds /*Bx32 or NULL*/, uint8_t *ok /*B*/, int32_t *per_proof_status /*B*/, zk_pool_job **job);
zk_status zk_pool_verify_wait(zk_pool *pool, zk_pool_job *job);

/* ---- hardened mode: the two protocol hardenings the reference leaves as TODOs, as an explicit opt-in.  NOT byte-compatible
 * with the reference: a proof made in one mode only verifies in that mode.  Default: ZK_MODE_REFERENCE (byte parity).
 *   (1) src/commit/pedersen.ts:62 "we must generate h without using scalar mult": zk_hardened_h derives NistGroup.h and
 *       ProofGroup.h from SHA-256 by try-and-increment (specification in csrc/h2c_host.cpp), so that nobody knows their
 *       discrete logarithms; pass them to zk_ctx_set_params like any other parameters.  Host-only, no context.
 *   (2) src/proofGK/gk.ts:178 "we should hash in the statement": with zk_ctx_set_mode(ctx, ZK_MODE_HARDENED) the challenge of
 *       the membership proof is SHA-256(cl || ca || cb || cd || "ZKAttest-GK-statement-v1" || ring digest || msgHash || R ||
 *       keyXcom)[0..10) instead of the hash of the commitments alone; ring digest = zk_ring_digest: SHA-256("ZKAttest-ring-v1" ||
 *       be64(N) || SHA-256 of every 256 consecutive entries of the padded ring).  Prover and verifier must use the same mode. */
enum { ZK_MODE_REFERENCE = 0, ZK_MODE_HARDENED = 1 };
zk_status zk_ctx_set_mode(zk_ctx *ctx, uint32_t mode);

/* Zeroes the witness-derived device memory of the context: the prover lanes' workspaces (per proof: the RNG stream -- 116 KB --, the nonces, s1 = s / r, the
 * blinders of every commitment) and the staging copy of the inputs of the host-pointer calls (signatures, seeds).  The library does this by itself in
 * zk_ctx_destroy and when a prove call fails; a successful call leaves the memory to be overwritten by the next one, and a host that wants it gone earlier
 * calls this (cost: one memset of the workspaces, ~4 ms per lane at 22 016 proofs per chunk).  No streamed job may be in flight.  The reference has no
 * counterpart (src/zkpAttestList.ts:104-145 leaves its BigInts to the garbage collector). */
zk_status zk_ctx_wipe(zk_ctx *ctx);
zk_status zk_ring_digest(zk_ctx *ctx, uint8_t digest[32]);
zk_status zk_hardened_h(const uint8_t *tag, uint64_t tag_len, uint8_t nist_h[64], uint8_t tom_h[72]);

/* Seeded synthetic workload generator: fills device or host buffers with a ring of
 * n_keys uniform scalars, and B valid ECDSA P-256 signatures whose public keys' x-coordinates are planted at
 * ring[which_b], which_b = b mod n_keys.  Mirrors oracle/zkattest_ref.py synth_* byte for byte.  Host pointers. */
zk_status zk_synth_workload(zk_ctx *ctx, uint64_t seed, uint64_t n_keys, uint64_t B, uint8_t *ring_be32 /*n_keys x 32*/,
                            uint8_t *msg_hash, uint8_t *sig, uint8_t *pk_xy, uint32_t *which, uint8_t *rng_seeds /*Bx32*/);
/* Derives the synthetic SystemParametersList of seed S (h = k*g with k = SHA-256 tags). */
zk_status zk_synth_params(zk_ctx *ctx, uint64_t seed, uint8_t nist_h[64], uint8_t tom_g[72], uint8_t tom_h[72]);

/* JSON wire format of SignatureProofList (writeJson/readJson, src/serde.ts:21-36, over the typedjson decorators of
 * src/zkpAttestList.ts:27-35, exp/exp.ts:26-40, exp/pointAdd.ts:28-38, commit/mult.ts:26-40, commit/equality.ts:27-33,
 * proofGK/gk.ts:31-40, curves/{weier.ts:92-101, edwards.ts:89-98, group.ts:155-161}, bignum/big.ts:230-248).
 * Host-only conversions between one ZKA1 proof and its JSON text; no context and no GPU needed.  *out_len is always
 * set to the required size; ZK_E_BUFFER if out_cap is too small (call once with out = NULL to size).  from_json is
 * order-tolerant and ignores "__type"/unknown members; like JSON.parse it keeps the LAST of duplicated members, decodes the string
 * escapes (\uXXXX included) and rejects text that is not JSON (stray tokens, raw control characters, unknown escapes); it checks
 * structure, group names and hex syntax/width --
 * curve membership is checked where the reference checks it semantically, in zk_verify_batch's validation. */
zk_status zk_proof_to_json(const uint8_t *proof, uint64_t proof_len, char *out, uint64_t out_cap, uint64_t *out_len);
zk_status zk_proof_from_json(const char *json, uint64_t json_len, uint8_t *out, uint64_t out_cap, uint64_t *out_len);
/* The same for whole batches on `threads` host threads (0 = one per hardware thread; ZKATTEST_JSON_THREADS): the reference's bench
 * times toJson / fromJson per proof (bench/zkpAttestList.bench.ts:63-68); at ~600 KB of text per proof a batch of the GPU's size
 * needs every core.  Item i is proofs[proof_off[i] .. proof_off[i+1]) (texts[text_off[i] .. text_off[i+1])); the results lie back
 * to back in `out`, delimited by the n + 1 offsets written; an item that does not convert gets its status and an empty result.
 * ZK_E_BUFFER when `out` is too small: the offsets are complete anyway (the last one is the size to come back with). */
zk_status zk_proofs_to_json_batch(uint64_t n, const uint8_t *proofs, const uint64_t *proof_off /*n+1*/, char *out, uint64_t out_cap,
                                  uint64_t *text_off /*n+1*/, int32_t *per_proof_status /*n*/, uint32_t threads);
zk_status zk_proofs_from_json_batch(uint64_t n, const char *texts, const uint64_t *text_off /*n+1*/, uint8_t *out, uint64_t out_cap,
                                    uint64_t *proof_off /*n+1*/, int32_t *per_proof_status /*n*/, uint32_t threads);

/* Timing of the last prove/verify call from HIP events around every kernel family: per family the accumulated GPU milliseconds (names[i] are static
 * strings; a name that starts with '+' is a part of another family), and *total_ms = their SUM ('+' parts excluded).  With one lane and a large chunk the
 * families run one after the other and the sum is the GPU time of the call; with several lanes, and in small calls that fork work onto side streams, the
 * families overlap and the sum exceeds the time that passed -- zk_last_wall_ms gives that: earliest start to latest end over the same events.
 * The events sit between the kernels of a stream and cost a call of a few proofs 0.15-0.45 ms (two per family and chunk): by default (ZK_TIMING_AUTO) only
 * blocking calls of more than 8 192 proofs record them, and after a smaller call zk_last_timing reports no families (returns 0, *total_ms = 0);
 * zk_ctx_set_timing(ctx, ZK_TIMING_ON) records them in every blocking call, ZK_TIMING_OFF in none.  Streamed jobs (zk_prove_submit ...) never record them. */
#define ZK_TIMING_OFF 0
#define ZK_TIMING_ON 1
#define ZK_TIMING_AUTO 2
zk_status zk_ctx_set_timing(zk_ctx *ctx, int mode);
uint32_t zk_last_timing(const zk_ctx *ctx, float *total_ms, const char **names, float *ms, uint32_t cap);
float zk_last_wall_ms(const zk_ctx *ctx);

/* Diagnostic: the rate (GB/s) a page-locked copy of `bytes` (at least 1 MiB) reaches on the copy stream of pipeline lane `lane` (0..3), device
 * to host and host to device, measured with HIP events.  ~57 GB/s is what the link carries on MI355X boxes; ~27 GB/s says that the runtime of this
 * PROCESS serves copies with shader blits instead of an SDMA engine, and every host-pointer call will run at about 0.6 of
 * its usual rate whatever the buffers are. */
zk_status zk_ctx_copy_probe(zk_ctx *ctx, uint32_t lane, size_t bytes, int numa_node /* >= 0: the host buffer is bound to that node; -1: wherever
                            the runtime puts it */, float *d2h_gbps, float *h2d_gbps);

/* Unit-test hooks (tests/ call these through the C ABI to compare single primitives with the oracle).
 * zk_pool_test_locality: NUMA node and local CPUs of a PCI address as the pool reads them from sysfs (ZKATTEST_SYSFS_ROOT). */
int zk_pool_test_locality(const char *pci_bus_id, int *numa_node, int *cpus, int cap);
/* work counters: 0 = proofs that went through the verifier's per-proof sums since the context was created (fallback of the batched check);
 * 1 = proofs of the last chunk on lane 0 whose scalar multiplications by the signer's key went through the per-key tables;
 * 2 = live terms that went through the verifier's batched Tom-256 check (bucket pass) since the context was created;
 * 3 = proofs whose P-256 relation was accepted by the cross-proof P-256 pass (chunks of at least ZKATTEST_P256_BATCH proofs, default 8192): every GROUP
 *     without a failing proof counts (a failing group, not its chunk, goes through the per-proof sums);
 * 4 = dependent chains of small calls handed to cooperating waves so far (k_coop.hip: Straus sums, the table of R; k_p256.hip: the prover's table sums;
 *     k_screen.hip: four per witness of a screen chunk of at most ZK_SCREEN_CO_MAX witnesses, whatever paths they take), process-wide;
 * 5 = per-key tables COMPUTED by the ring builder since the context was created (a full build computes one per padded entry; the tables zk_ctx_update_ring
 *     copies from entry 0 for padding entries do not count);
 * 6 = 256-key blocks whose table E was built since the context was created;
 * 7 = segments that mixed-ring prove calls (zk_prove_batch_rings) staged since the context was created -- a call of one ring stages none;
 * 8 = windows those calls proved;
 * 9 = bytes of the staging buffer those calls have grown so far (grow-only);
 * 10 = form of the context's comb tables of g and h: 1 = the a = -1 model (7 products per table addition; chosen by zk_ctx_set_params when q * g = q * h =
 *     identity), 0 = the a = 1 image (any other pair of curve points); ~0 before zk_ctx_set_params.  Bytes and verdicts are the same;
 * 11 = nonzero 32-bit words in the buffers a witness wipe zeroes, with nothing in flight;
 * 12 = passes of the verifier's pipeline run by blocking calls since the context was created: one per call (or per window of a split batch), ceil(count / 20)
 *     in ZK_VERIFY_REPS_ALL;
 * 13 = windows that mixed-ring membership calls (zk_member_*_batch_rings) proved or verified since the context was created -- a batch of one ring runs none. */
uint64_t zk_test_counter(const zk_ctx *ctx, int which);
/* Only in the test build (lib/libzkattest_hip_testhooks.so, csrc/api_pool.hip under ZK_TEST_HOOKS); the product library exports neither:
 *   void zk_test_pool_fail_next_submit, arguments (zk_pool *pool, int slot):
 *       the next streamed pool submit fails at device slot `slot` (one shot)
 *   zk_status zk_test_ring_checksum, arguments (zk_ctx *ctx, uint32_t ring, uint64_t sums[8]):
 *       one order-independent 64-bit checksum per table of a resident ring -- limbs, table E, gk_kdig, gk_edig, ktab, ktab_ok, leaves, digest: the sum mod 2^64 of
 *       a mix of (word index, word); 0 for a table the ring does not have.  Per-key tables of ring values that are no x-coordinate are never written and left out.
 *   zk_status zk_test_set_prove_segment, arguments (zk_ctx *ctx, uint32_t proofs):
 *       mixed-ring prove calls of this context cut their batch into segments of `proofs` proofs (rounded down to a multiple of 256, at least 256) instead of
 *       what the staging buffer's default size holds; 0 = the default again */
/*
 * which_field: 0 = F_q (p256.p), 1 = Z_n, 2 = F_t;  op: 0 mul, 1 add, 2 sub, 3 inverse, 4 a*b - a - b (fused double subtraction), 5 (a + b)^2 (dedicated squaring).  count x 40-byte BE operands. */
zk_status zk_test_field_op(zk_ctx *ctx, int which_field, int op, uint64_t count, const uint8_t *a_be40, const uint8_t *b_be40, uint8_t *out_be40);
/* out[i] = v[i]*g + r[i]*h on Tom-256 (72-byte affine), through the fixed-base comb kernel */
zk_status zk_test_tom_commit(zk_ctx *ctx, uint64_t count, const uint8_t *v_be32, const uint8_t *r_be32, uint8_t *out_xy72);
/* the same through ONE named kernel of the comb sums whatever the count (shape 0: as zk_test_tom_commit, the launch wrapper chooses): 1 = one lane per commitment;
 * 2 = the list is list B of count / 34 items, slot = k * items + item (unpaired slots one lane each, the nine pairs through the kernel that shares v * g: it takes v
 * of a pair from its first slot); 3 = four lanes; 4 = four cooperating waves; 5 = the compacted-list kernel of the verifier.  ZK_E_ARG where a shape does not
 * apply (3 and 4 with the signed comb widths 25 and 26; 2 with a count that is no multiple of 34). */
zk_status zk_test_tom_commit_shape(zk_ctx *ctx, uint32_t shape, uint64_t count, const uint8_t *v_be32, const uint8_t *r_be32, uint8_t *out_xy72);
/* out[i] = k[i]*G (base_sel 0) or k[i]*h_NIST (base_sel 1) on P-256 (64-byte affine; all-zero for the identity) */
zk_status zk_test_p256_fixed_mul(zk_ctx *ctx, int base_sel, uint64_t count, const uint8_t *k_be32, uint8_t *out_xy64);
/* the table sums of the Exp commit phase on given scalars, key-table path of the active ring: T = g * G + k * (+- ring key `key`), A = T + b * h_NIST for count
 * triples gkb[i] = g || k || b (3 x 32 bytes big-endian, reduced mod n); neg != 0: the key is the negative of its table's base point.  out: 4 x count points of 64
 * bytes (affine; all-zero for the identity) -- T[0..count), A[0..count) through the device functions the prover's kernel runs, then T, A through the complete-law
 * walks alone.  fell[i]: bit 0 / bit 1 = the first T / A was recomputed with the complete law.  ZK_E_BUFFER without parameters or key tables. */
zk_status zk_test_exp_sum(zk_ctx *ctx, uint32_t key, int neg, uint64_t count, const uint8_t *gkb_be96, uint8_t *out_xy64, uint32_t *fell);
/* The verifier's cross-proof Tom-256 bucket pass (the production launch sequence, on a workspace carved as the verifier carves a chunk of cap_proofs proofs)
 * on caller-chosen terms, by value.  groups: 8 (16 windows of 16 bits) or 64 (20 windows of 13 bits); count <= cap_proofs live proofs; nq in 1..4 membership
 * groups per proof.  A proof slot has T = 720 + 8 nq + 3 term slots; term ids as in the pass: k * (20 cap) + 20 p + j for term k < 36 of repetition j < 20 of
 * proof slot p, then 720 cap + k * (nq cap) + nq p + i for term k < 8 of membership group i < nq, then (720 + 8 nq) cap + k * cap + p for k < 3.  Term id t
 * is term_sc[t] (32 bytes big-endian, reduced mod q) times entry term_idx[t] of the table of ntab affine points (72 bytes each; an index >= ntab: the identity
 * entry).  coef: per live proof the fixed-base coefficients mg, mh, eg, eh (4 x 32 bytes).  Out: tw_xy72[(w * groups + grp) * 72 ..] the window sums
 * (sum_d d B_d) 2^(C w) as affine points (all-zero: the identity; all-0xff: a point with Z = 0), one_xy72[grp] the group's fixed-base point, flags[grp] the
 * pass's verdict, counters[0] the live terms, counters[1] the oversized buckets seen.  ZK_E_BUFFER without parameters. */
zk_status zk_test_msm_sum(zk_ctx *ctx, uint32_t groups, uint32_t cap_proofs, uint32_t count, uint32_t nq, uint32_t ntab, const uint8_t *table_xy72,
                          const uint32_t *term_idx, const uint8_t *term_sc_be32, const uint8_t *coef_be32, uint8_t *tw_xy72, uint8_t *one_xy72, uint32_t *flags,
                          uint32_t *counters);
/* The same for the P-256 pass's pack, group, bucket and reduce kernels: groups 8 (11 windows of 13 bits) or 64 (14 windows of 10 bits).  Term ids: 20 p + j for
 * A term j of proof slot p, then 20 cap + p for the Clambda term; table of 64-byte affine points (every index below ntab), scalars reduced mod n.  Out:
 * tw_xy64[(w * groups + grp) * 64 ..] the window sums sum_d d B_d (NOT times 2^(C w); all-zero: the identity), flags[grp] the pass's verdict with identity R
 * parts, counters[0] = 1 if a scalar reached beyond the windows, counters[1] the oversized buckets seen. */
zk_status zk_test_pmsm_sum(zk_ctx *ctx, uint32_t groups, uint32_t cap_proofs, uint32_t count, uint32_t ntab, const uint8_t *table_xy64, const uint32_t *term_idx,
                           const uint8_t *term_sc_be32, uint8_t *tw_xy64, uint32_t *flags, uint32_t *counters);
/* digest[i] = SHA-256(msg[i]) for count messages of identical length len */
zk_status zk_test_sha256(zk_ctx *ctx, uint64_t count, uint64_t len, const uint8_t *msgs, uint8_t *digests32);
/* logical RNG draw k of each proof (after rejection mapping), 32 bytes BE */
zk_status zk_test_rng_draws(zk_ctx *ctx, uint64_t B, const zk_rng *rng, uint32_t first_k, uint32_t n_k, uint8_t *out /*B x n_k x 32*/);

#ifdef __cplusplus
}
#endif
#endif
