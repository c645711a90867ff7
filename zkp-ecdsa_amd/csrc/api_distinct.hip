// zk_distinct_prove_batch / zk_distinct_verify_batch (include/zkattest.h): "these two Tom-256 commitments open to DIFFERENT keys", one MultProof
// (mult.ts:93-175) over Cx = C1 - C2, Cy = commit(1 / (x1 - x2)), Cz = g.  Host-side pipeline; the kernels of its own are in k_distinct.hip, the commitments
// are k_tom.hip's comb kernels, the challenge hash k_hash.hip's message path.  No ring takes part.  The chunks run on the context's lanes (their streams are
// the prover lanes'), every lane's arena carved from one witness-flagged buffer.
#include "ctx.h"
#include "jobs.h"
#include "distinct.h"

static size_t dist_carve(DistLane* K, uint32_t nlanes, uint8_t* base, uint32_t C) {
    SoaCarver k(base);
    for (uint32_t l = 0; l < nlanes; l++) {
        DistLane& X = K[l];
        X = DistLane{};
        X.C = C;
        X.L = k.list(DIST_SLOTS * (size_t)C);
        X.rng.exc_idx = (uint32_t*)k.take(4 * RNG_MAX_EXC * (size_t)C);
        X.rng.exc_flags = (uint32_t*)k.take(4 * RNG_MAX_EXC * (size_t)C);
        X.rng.exc_cnt = (uint32_t*)k.take(4 * (size_t)C);
        X.rng_fill = (uint32_t*)k.take(32 * (size_t)DIST_RNG_BLOCKS * C);
        X.st = (int32_t*)k.take(4 * (size_t)C);
        X.flags = (uint32_t*)k.take(4 * (size_t)C);
        X.cw = (uint32_t*)k.take(4 * 36 * (size_t)C);
        X.msg = (uint8_t*)k.take((size_t)ZKD1_MSG_BLOCKS * 64 * C);
        X.wk = (uint32_t*)k.take((size_t)ZKD1_MSG_BLOCKS * 256 * C);
        X.chal = (uint32_t*)k.take(16 * (size_t)C);
        X.tw = (uint32_t*)k.take(32 * (size_t)C);
        X.tab = (DistQuad*)k.take(sizeof(DistQuad) * DIST_TAB_QUADS * (size_t)C);
        X.rel = (uint32_t*)k.take(12 * (size_t)C);
    }
    return k.off + ZK_LAYOUT_TAIL;
}
static zk_status dist_refusal(zk_ctx* c, uint64_t B) {
    if (!c->params_set) return ZK_E_BUFFER;
    if (c->stream_busy) return busy_refusal(c);
    if (B > 0xffffffffull) return ZK_E_ARG;
    return ZK_OK;
}
static bool dist_aligned(std::initializer_list<const void*> ps) {   // the kernels read and write 32-bit words
    for (const void* p : ps)
        if ((uintptr_t)p & 3) return false;
    return true;
}
extern "C" uint64_t zk_distinct_proof_size(void) { return ZKD1_SIZE; }

// The chunk plan of a call of B proofs and its lanes' arenas
struct DistRun {
    std::vector<ChunkPlan> plan;
    uint32_t NL = 0;
    DistLane K[ZK_MAX_LANES];
};
static zk_status dist_plan(zk_ctx* c, uint64_t B, DistRun& R) {
    const uint32_t C = (uint32_t)std::min<uint64_t>(c->chunk, B);
    R.plan = make_chunk_plan(B, C, 1, false);
    R.NL = (uint32_t)std::min<size_t>(std::min<uint32_t>(c->lanes, ZK_MAX_LANES), R.plan.size());
    return lay_out(c, B_dk, [&](uint8_t* base) { return dist_carve(R.K, R.NL, base, C); });
}

// ------------------------------------------------------------------ prover
static zk_status dist_prove_device(zk_ctx* c, uint64_t B, const DistProveIo& io, const zk_rng& rng, uint64_t out_cap) {
    if (zk_status zs = dist_refusal(c, B)) return zs;
    if (!rng_mode_ok(&rng)) return ZK_E_ARG;
    if (B > out_cap / ZKD1_SIZE) {
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    if (B == 0) return ZK_OK;
    if (!dist_aligned({io.key1, io.com1, io.blinder1, io.key2, io.com2, io.blinder2, io.out, io.status, rng.data})) return ZK_E_ARG;
    timing_begin(c);   // (behind every refusal: a call that runs nothing leaves the last call's record as it is)
    DistRun R;
    if (zk_status zs = dist_plan(c, B, R)) return zs;
    const bool timed = zk_timed(c, B);
    for (uint64_t k = 0; k < R.plan.size(); k++) {
        const uint32_t lane = (uint32_t)(k % R.NL), cnt = R.plan[k].cnt;
        const uint64_t first = R.plan[k].first;
        DistLane& K = R.K[lane];
        hipStream_t s = c->pl[lane].stream;
        K.rng.seeds = rng.data, K.rng.stream = rng.data, K.rng.stride_blocks = rng.stride_blocks, K.rng.mode = rng.mode, K.rng.sec = -1, K.rng.proof_base = (uint32_t)first;
        {
            MaybeScope t(timed, c, "rng_prepass", s);
            Workspace W{};   // the prepass reads a workspace's RNG view
            W.rng = K.rng;
            launch_rng_prepass(s, W, cnt, 0, DIST_RNG_BLOCKS, DIST_RNG_BLOCKS, rng.mode == ZK_RNG_SEED ? K.rng_fill : nullptr, false);
        }
        if (rng.mode == ZK_RNG_SEED) K.rng.mode = ZK_RNG_STREAM, K.rng.stream = (const uint8_t*)K.rng_fill, K.rng.stride_blocks = DIST_RNG_BLOCKS, K.rng.proof_base = 0;
        {
            MaybeScope t(timed, c, "tom_commit", s);
            launch_dist_front(s, K, cnt, first, io);
            launch_tom_commit_pair_slots(s, c->P, K.L, cnt);                                    // (A_z, A_4_1): k_z g once
            launch_tom_commit(s, c->P, dist_view(K.L, 2 * cnt), DIST_SINGLES * cnt, 1, 1);      // C_w, C_4, A_x, A_y, A_4_2 and the two claimed openings
        }
        {
            MaybeScope t(timed, c, "tom_normalize", s);
            launch_tom_normalize(s, K.L, DIST_SLOTS * cnt, 0, 1, 1);                            // ... and Cx behind them
        }
        {
            MaybeScope t(timed, c, "hash", s);
            launch_dist_opening_msg(s, c->P, K, cnt);
            launch_dist_hash(s, K, cnt);
        }
        {
            MaybeScope t(timed, c, "distinct_respond", s);
            launch_dist_respond(s, K, cnt, first, io);
        }
    }
    const hipError_t e_sync = drain_lanes(c, R.NL);
    if (e_sync != hipSuccess) wipe_witness(c);   // a failed call leaves no key, inverse, nonce, blinder or RNG block behind
    HIPCHK(c, e_sync);
    HIPCHK(c, hipGetLastError());
    timing_end(c);
    return ZK_OK;
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
    if (zk_status zs = dist_refusal(c, B)) return zs;
    if (!rng_mode_ok(rng)) return ZK_E_ARG;
    if (B > out_cap / ZKD1_SIZE) {
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    if (B == 0) return ZK_OK;
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
    if (zk_status zs = dist_refusal(c, B)) return zs;
    if (B == 0) return ZK_OK;
    if (!dist_aligned({io.com1, io.com2, io.proofs, io.status})) return ZK_E_ARG;
    timing_begin(c);
    DistRun R;
    if (zk_status zs = dist_plan(c, B, R)) return zs;
    const bool timed = zk_timed(c, B);
    for (uint64_t k = 0; k < R.plan.size(); k++) {
        const uint32_t lane = (uint32_t)(k % R.NL), cnt = R.plan[k].cnt;
        const uint64_t first = R.plan[k].first;
        const DistLane& K = R.K[lane];
        hipStream_t s = c->pl[lane].stream;
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
            launch_dist_hash(s, K, cnt);
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
    }
    HIPCHK(c, drain_lanes(c, R.NL));
    HIPCHK(c, hipGetLastError());
    timing_end(c);
    return ZK_OK;
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
    if (zk_status zs = dist_refusal(c, B)) return zs;
    if (B == 0) return ZK_OK;
    DistVerifyIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return dist_verify_in_layout(I, base, B); })) return zs;
    if (zk_status zs = reserve(c, B_io, B * ZKD1_SIZE)) return zs;
    uint8_t* const d_proofs = (uint8_t*)c->buf[B_io].p;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(I.com1, com1, 72 * B, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(I.com2, com2, 72 * B, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_proofs, proofs, B * ZKD1_SIZE, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (zk_status zs = dist_verify_device(c, B, {I.com1, I.com2, d_proofs, I.ok, I.st})) return zs;
    HIPCHK(c, hipMemcpyAsync(ok, I.ok, B, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(status, I.st, 4 * B, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return ZK_OK;
}

// ------------------------------------------------------------------ the two pipelines for api_quorum.hip (quorum.h), behind the entry points' argument checks
zk_status zkq_distinct_prove(zk_ctx* c, uint64_t B, const uint8_t* key1, const uint8_t* com1, const uint8_t* blinder1, const uint8_t* key2, const uint8_t* com2,
                             const uint8_t* blinder2, const zk_rng& rng, uint8_t* out, int32_t* status) {
    return dist_prove_device(c, B, {key1, com1, blinder1, key2, com2, blinder2, out, status}, rng, B * ZKD1_SIZE);
}
zk_status zkq_distinct_verify(zk_ctx* c, uint64_t B, const uint8_t* com1, const uint8_t* com2, const uint8_t* proofs, uint8_t* ok, int32_t* status) {
    return dist_verify_device(c, B, {com1, com2, proofs, ok, status});
}
