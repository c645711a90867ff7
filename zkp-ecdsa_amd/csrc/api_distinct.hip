// zk_distinct_prove_batch / zk_distinct_verify_batch (include/zkattest.h): "these two Tom-256 commitments open to DIFFERENT keys", one MultProof
// (mult.ts:93-175) over Cx = C1 - C2, Cy = commit(1 / (x1 - x2)), Cz = g.  Host-side pipeline; the kernels of its own are in k_distinct.hip, the commitments
// are k_tom.hip's comb kernels, the challenge hash k_hash.hip's message path.  No ring takes part.  The chunks run on the context's lanes (their streams are
// the prover lanes'), every lane's arena carved from one witness-flagged buffer.
#include "ctx.h"
#include "sigma.h"
#include "distinct.h"

static void dist_carve(SoaCarver& k, DistLane& X, uint32_t C) {
    X = DistLane{};
    sigma_carve_core(k, X, C, DIST_SLOTS, DIST_RNG_BLOCKS, ZKD1_MSG_BLOCKS);
    X.cw = (uint32_t*)k.take(4 * 36 * (size_t)C);
    X.tw = (uint32_t*)k.take(32 * (size_t)C);
    X.tab = (DistQuad*)k.take(sizeof(DistQuad) * DIST_TAB_QUADS * (size_t)C);
    X.rel = (uint32_t*)k.take(12 * (size_t)C);
}
extern "C" uint64_t zk_distinct_proof_size(void) { return ZKD1_SIZE; }
typedef SigmaRun<DistLane> DistRun;

// ------------------------------------------------------------------ prover
static zk_status dist_prove_device(zk_ctx* c, uint64_t B, const DistProveIo& io, const zk_rng& rng, uint64_t out_cap) {
    zk_status gate;
    if (sigma_prove_gate(c, B, rng, out_cap, ZKD1_SIZE, gate)) return gate;
    if (!words_aligned({io.key1, io.com1, io.blinder1, io.key2, io.com2, io.blinder2, io.out, io.status, rng.data})) return ZK_E_ARG;
    timing_begin(c);   // (behind every refusal: a call that runs nothing leaves the last call's record as it is)
    DistRun R;
    if (zk_status zs = sigma_plan(c, B, B_dk, R, dist_carve)) return zs;
    const bool timed = zk_timed(c, B);
    return sigma_run_chunks(c, R, true, [&](DistLane& K, hipStream_t s, uint32_t cnt, uint64_t first) {
        sigma_chunk_rng(c, timed, s, K.rng, K.rng_fill, rng, first, cnt, DIST_RNG_BLOCKS);
        {
            MaybeScope t(timed, c, "tom_commit", s);
            launch_dist_front(s, K, cnt, first, io);
            launch_tom_commit_pair_slots(s, c->P, K.L, cnt);                                    // (A_z, A_4_1): k_z g once
            launch_tom_commit(s, c->P, tom_list_from(K.L, 2 * cnt), DIST_SINGLES * cnt, 1, 1);  // C_w, C_4, A_x, A_y, A_4_2 and the two claimed openings
        }
        {
            MaybeScope t(timed, c, "tom_normalize", s);
            launch_tom_normalize(s, K.L, DIST_SLOTS * cnt, 0, 1, 1);                            // ... and Cx behind them
        }
        {
            MaybeScope t(timed, c, "hash", s);
            launch_dist_opening_msg(s, c->P, K, cnt);
            launch_sigma_hash(s, K, cnt, ZKD1_MSG_BLOCKS);
        }
        {
            MaybeScope t(timed, c, "distinct_respond", s);
            launch_dist_respond(s, K, cnt, first, io);
        }
    });   // (a failed call leaves no key, inverse, nonce, blinder or RNG block behind)
}
extern "C" zk_status zk_distinct_prove_batch_device(zk_ctx* c, uint64_t B, const void* d_key1, const void* d_com1, const void* d_blinder1, const void* d_key2, const void* d_com2,
                                                    const void* d_blinder2, const zk_rng* rng, void* d_out, uint64_t out_cap, void* d_status) {
    if (!c || !rng || (B && (!d_key1 || !d_com1 || !d_blinder1 || !d_key2 || !d_com2 || !d_blinder2 || !rng->data || !d_out || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const zk_status zs = dist_prove_device(c, B, {(const uint8_t*)d_key1, (const uint8_t*)d_com1, (const uint8_t*)d_blinder1, (const uint8_t*)d_key2, (const uint8_t*)d_com2,
                                                  (const uint8_t*)d_blinder2, (uint8_t*)d_out, (int32_t*)d_status}, *rng, out_cap);
    if (zs && c->params_set && !c->stream_busy) wipe_witness(c);
    return zs;
}
// Host pointers: keys, blinders and seeds through the context's witness-flagged input buffer, the proofs through its output staging buffer.
struct DistProveIn {
    uint8_t *key1, *com1, *blinder1, *key2, *com2, *blinder2, *rng;
    int32_t* st;
};
static size_t dist_prove_in_layout(DistProveIn& I, uint8_t* base, size_t B, size_t rng_bytes) {
    Carver k(base);
    I.key1 = (uint8_t*)k.take(32 * B), I.com1 = (uint8_t*)k.take(72 * B), I.blinder1 = (uint8_t*)k.take(32 * B);
    I.key2 = (uint8_t*)k.take(32 * B), I.com2 = (uint8_t*)k.take(72 * B), I.blinder2 = (uint8_t*)k.take(32 * B);
    I.rng = (uint8_t*)k.take(rng_bytes ? rng_bytes : 32), I.st = (int32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_distinct_prove_batch(zk_ctx* c, uint64_t B, const uint8_t* key1, const uint8_t* com1, const uint8_t* blinder1, const uint8_t* key2, const uint8_t* com2,
                                             const uint8_t* blinder2, const zk_rng* rng, uint8_t* out, uint64_t out_cap, int32_t* status) {
    if (!c || !rng || (B && (!key1 || !com1 || !blinder1 || !key2 || !com2 || !blinder2 || !rng->data || !out || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    zk_status gate;
    if (sigma_prove_gate(c, B, *rng, out_cap, ZKD1_SIZE, gate)) return gate;
    DistProveIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return dist_prove_in_layout(I, base, B, rng_bytes(rng, B)); })) return zs;
    if (zk_status zs = reserve(c, B_io, B * ZKD1_SIZE)) return zs;
    uint8_t* const d_out = (uint8_t*)c->buf[B_io].p;
    // from the first upload on, keys, blinders and seeds lie in the input buffer: every failure below zeroes them
    if (zk_status zs = upload_or_wipe(c, {{I.key1, key1, 32 * B}, {I.com1, com1, 72 * B}, {I.blinder1, blinder1, 32 * B}, {I.key2, key2, 32 * B}, {I.com2, com2, 72 * B},
                                          {I.blinder2, blinder2, 32 * B}, {I.rng, rng->data, rng_bytes(rng, B)}}))
        return zs;
    if (zk_status zs = dist_prove_device(c, B, {I.key1, I.com1, I.blinder1, I.key2, I.com2, I.blinder2, d_out, I.st}, zk_rng{rng->mode, I.rng, rng->stride_blocks}, B * ZKD1_SIZE)) {
        wipe_witness(c);
        return zs;
    }
    return download_or_wipe(c, {{d_out, out, B * ZKD1_SIZE}, {I.st, status, 4 * B}});
}

// ------------------------------------------------------------------ verifier
static zk_status dist_verify_device(zk_ctx* c, uint64_t B, const DistVerifyIo& io) {
    if (zk_status zs = sigma_refusal(c, B)) return zs;
    if (B == 0) return ZK_OK;
    if (!words_aligned({io.com1, io.com2, io.proofs, io.status})) return ZK_E_ARG;
    timing_begin(c);
    DistRun R;
    if (zk_status zs = sigma_plan(c, B, B_dk, R, dist_carve)) return zs;
    const bool timed = zk_timed(c, B);
    return sigma_run_chunks(c, R, false, [&](const DistLane& K, hipStream_t s, uint32_t cnt, uint64_t first) {
        {
            MaybeScope t(timed, c, "distinct_parse", s);
            launch_dist_parse(s, c->P, K, cnt, first, io);
        }
        {
            MaybeScope t(timed, c, "tom_normalize", s);
            launch_tom_normalize(s, K.L, cnt, 4 * cnt, 1, 1);   // Cx = C1 - C2, for the challenge and as relation 1's base
        }
        {
            MaybeScope t(timed, c, "hash", s);
            launch_dist_cx_msg(s, K, cnt);
            launch_sigma_hash(s, K, cnt, ZKD1_MSG_BLOCKS);
        }
        {
            MaybeScope t(timed, c, "tom_commit", s);
            launch_dist_fold(s, K, cnt);
            launch_tom_commit(s, c->P, K.L, 4 * cnt, 1, 1);     // t_x g + t_rx h, t_y g + t_ry h, (t_z + c) g + t_rz h, t_z g + t_r4 h
        }
        {
            MaybeScope t(timed, c, "distinct_short", s);
            launch_dist_short(s, K, cnt, first, io);
        }
        {
            MaybeScope t(timed, c, "distinct_long", s);
            launch_dist_long(s, K, cnt, first, io);
        }
    });
}
extern "C" zk_status zk_distinct_verify_batch_device(zk_ctx* c, uint64_t B, const void* d_com1, const void* d_com2, const void* d_proofs, void* d_ok, void* d_status) {
    if (!c || (B && (!d_com1 || !d_com2 || !d_proofs || !d_ok || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return dist_verify_device(c, B, {(const uint8_t*)d_com1, (const uint8_t*)d_com2, (const uint8_t*)d_proofs, (uint8_t*)d_ok, (int32_t*)d_status});
}
struct DistVerifyIn {   // no witness is staged: a failing copy returns as it is
    uint8_t *com1, *com2, *ok;
    int32_t* st;
};
static size_t dist_verify_in_layout(DistVerifyIn& I, uint8_t* base, size_t B) {
    Carver k(base);
    I.com1 = (uint8_t*)k.take(72 * B), I.com2 = (uint8_t*)k.take(72 * B), I.ok = (uint8_t*)k.take(B), I.st = (int32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_distinct_verify_batch(zk_ctx* c, uint64_t B, const uint8_t* com1, const uint8_t* com2, const uint8_t* proofs, uint8_t* ok, int32_t* status) {
    if (!c || (B && (!com1 || !com2 || !proofs || !ok || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = sigma_refusal(c, B)) return zs;
    if (B == 0) return ZK_OK;
    DistVerifyIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return dist_verify_in_layout(I, base, B); })) return zs;
    if (zk_status zs = reserve(c, B_io, B * ZKD1_SIZE)) return zs;
    uint8_t* const d_proofs = (uint8_t*)c->buf[B_io].p;
    if (zk_status zs = upload_rows(c, {{I.com1, com1, 72 * B}, {I.com2, com2, 72 * B}, {d_proofs, proofs, B * ZKD1_SIZE}})) return zs;
    if (zk_status zs = dist_verify_device(c, B, {I.com1, I.com2, d_proofs, I.ok, I.st})) return zs;
    return download_rows(c, {{I.ok, ok, B}, {I.st, status, 4 * B}});
}

// ------------------------------------------------------------------ the two pipelines for api_quorum.hip (quorum.h), behind the entry points' argument checks
zk_status zkq_distinct_prove(zk_ctx* c, uint64_t B, const uint8_t* key1, const uint8_t* com1, const uint8_t* blinder1, const uint8_t* key2, const uint8_t* com2,
                             const uint8_t* blinder2, const zk_rng& rng, uint8_t* out, int32_t* status) {
    return dist_prove_device(c, B, {key1, com1, blinder1, key2, com2, blinder2, out, status}, rng, B * ZKD1_SIZE);
}
zk_status zkq_distinct_verify(zk_ctx* c, uint64_t B, const uint8_t* com1, const uint8_t* com2, const uint8_t* proofs, uint8_t* ok, int32_t* status) {
    return dist_verify_device(c, B, {com1, com2, proofs, ok, status});
}
