// zk_ctx_set_auditors / zk_auditors_split_key / zk_auditors_share_batch / zk_auditors_share_verify_batch / zk_auditors_combine_batch (include/zkattest.h):
// t of n auditors open an escrow tag "ZKT1" through shares "ZKS1".  Host-side pipeline; the kernels of its own are in k_escrow_share.hip, U1 = k g and s g are
// k_tom.hip's over the context's (g, h) combs, the challenge hash k_hash.hip's message path, the normaliser and the lookup in the resident point indexes the
// single-auditor opening's (api_escrow.hip).  The chunks run on the context's lanes, every lane's arena carved from the escrow calls' witness-flagged buffer.
#include "ctx.h"
#include "sigma.h"
#include "escrow_share.h"

extern "C" uint64_t zk_auditors_share_size(void) { return ZKS1_SIZE; }

static zk_status share_refusal(zk_ctx* c, uint64_t B) {   // of every call that needs the set of share keys
    if (zk_status zs = sigma_refusal(c, B)) return zs;
    if (!c->auditor_set || !c->auditors_n) {
        c->err = "no set of share keys is in place (zk_ctx_set_auditor, then zk_ctx_set_auditors)";
        return ZK_E_BUFFER;
    }
    return ZK_OK;
}

// ------------------------------------------------------------------ the share keys
struct AuditorsSet {
    uint8_t *xy, *out;
    uint32_t *w, *idx, *at, *lam, *tab;
    int32_t* res;
    TomList L;
};
static size_t auditors_set_layout(AuditorsSet& X, uint8_t* base, uint32_t t, uint32_t evals) {
    SoaCarver k(base);
    X.xy = (uint8_t*)k.take(72 * ZK_AUDITORS_MAX), X.out = (uint8_t*)k.take(72 * (size_t)evals);
    X.w = (uint32_t*)k.take(4 * 18 * ZK_AUDITORS_MAX), X.idx = (uint32_t*)k.take(4 * ZK_AUDITORS_MAX), X.at = (uint32_t*)k.take(4 * ZK_AUDITORS_MAX);
    X.lam = (uint32_t*)k.take(32 * (size_t)t * evals), X.tab = (uint32_t*)k.take(4 * 27 * (size_t)t * evals);
    X.res = (int32_t*)k.take(16 * ZK_AUDITORS_MAX);
    X.L = k.list(evals);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_ctx_set_auditors(zk_ctx* c, uint32_t t, uint32_t n, const uint8_t* share_keys_xy72) {
    if (!c || !share_keys_xy72) return ZK_E_ARG;
    if (c->stream_busy) return busy_refusal(c);
    if (!c->params_set) return ZK_E_BUFFER;
    if (!c->auditor_set) {
        c->err = "no auditor key is set (zk_ctx_set_auditor)";
        return ZK_E_BUFFER;
    }
    if (t < 1 || t > n || n > ZK_AUDITORS_MAX) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const uint32_t evals = n - t + 1;   // the value at 0, then at every m > t
    AuditorsSet X;
    DevBuf d;
    HIPCHK(c, hipMalloc(&d.p, auditors_set_layout(X, nullptr, t, evals)));
    auditors_set_layout(X, d.as<uint8_t>(), t, evals);
    c->auditors_t = 0, c->auditors_n = 0;   // from here on the previous set is gone: a failure below leaves the context without one
    HIPCHK(c, hipMemcpyAsync(X.xy, share_keys_xy72, 72 * (size_t)n, hipMemcpyHostToDevice, s));
    for (uint32_t i = 0; i < n; i++) {   // every A_j as zk_ctx_set_auditor checks A
        launch_escrow_check_key(s, X.xy + 72 * i, X.w + 18 * i, X.res + 4 * i);
        launch_tom_order_check(s, X.w + 18 * i, X.w + 18 * i, X.res + 4 * i + 2);
    }
    int32_t res[4 * ZK_AUDITORS_MAX] = {};
    HIPCHK(c, hipMemcpyAsync(res, X.res, 16 * (size_t)n, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    for (uint32_t i = 0; i < n; i++)
        if (!res[4 * i]) return ZK_E_BAD_ENCODING;
    for (uint32_t i = 0; i < n; i++)
        if (res[4 * i + 1] || !res[4 * i + 2]) {
            c->err = "a share key is the identity or has a component outside the group of prime order";
            return ZK_E_ARG;
        }
    // one polynomial of degree t - 1 through A: A_1 .. A_t interpolate to A at 0 and to A_m at every m > t
    uint32_t idx[ZK_AUDITORS_MAX] = {}, at[ZK_AUDITORS_MAX] = {};
    for (uint32_t i = 0; i < t; i++) idx[i] = i + 1;
    for (uint32_t i = 1; i < evals; i++) at[i] = t + i;
    HIPCHK(c, hipMemcpyAsync(X.idx, idx, sizeof idx, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(X.at, at, sizeof at, hipMemcpyHostToDevice, s));
    launch_share_lagrange(s, X.idx, t, X.at, evals, X.lam);
    launch_share_interpolate(s, X.xy, t, X.lam, evals, X.tab, X.L);
    launch_tom_normalize(s, X.L, evals, 0, 1, 1);
    launch_affine_to_bytes(s, X.L.ax, X.L.ay, evals, 1, X.out);
    uint8_t out[72 * ZK_AUDITORS_MAX];
    HIPCHK(c, hipMemcpyAsync(out, X.out, 72 * (size_t)evals, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    bool same = memcmp(out, c->aud_xy, 72) == 0;
    for (uint32_t i = 1; i < evals; i++) same = same && memcmp(out + 72 * i, share_keys_xy72 + 72 * (size_t)(t + i - 1), 72) == 0;
    if (!same) {
        c->err = "the share keys do not lie on one polynomial of degree t - 1 through the auditor's key";
        return ZK_E_OPENING;
    }
    if (!c->auditors_w) HIPCHK(c, hipMalloc(&c->auditors_w, 4 * 18 * ZK_AUDITORS_MAX));
    HIPCHK(c, hipMemcpy(c->auditors_w, X.w, 4 * 18 * (size_t)n, hipMemcpyDeviceToDevice));
    memcpy(c->auditors_xy, share_keys_xy72, 72 * (size_t)n);
    c->auditors_t = t, c->auditors_n = n;
    return ZK_OK;
}

// ------------------------------------------------------------------ the dealer
struct ShareSplit {
    uint8_t *secret, *rng, *shares, *keys;
    uint32_t *exc_idx, *exc_flags, *exc_cnt, *fill, *flag;
    TomList L;
};
static size_t share_split_layout(ShareSplit& G, uint8_t* base, size_t rng_bytes) {
    SoaCarver k(base);
    G.secret = (uint8_t*)k.take(32), G.rng = (uint8_t*)k.take(rng_bytes ? rng_bytes : 32);
    G.shares = (uint8_t*)k.take(32 * ZK_AUDITORS_MAX), G.keys = (uint8_t*)k.take(72 * ZK_AUDITORS_MAX);
    G.exc_idx = (uint32_t*)k.take(4 * RNG_MAX_EXC), G.exc_flags = (uint32_t*)k.take(4 * RNG_MAX_EXC), G.exc_cnt = (uint32_t*)k.take(4);
    G.fill = (uint32_t*)k.take(32 * SPLIT_RNG_BLOCKS), G.flag = (uint32_t*)k.take(4);
    G.L = k.list(ZK_AUDITORS_MAX);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_auditors_split_key(zk_ctx* c, const uint8_t secret_be32[32], uint32_t t, uint32_t n, const zk_rng* rng, uint8_t* shares_be32, uint8_t* share_keys_xy72) {
    if (!c || !secret_be32 || !rng || !rng->data || !shares_be32 || !share_keys_xy72) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = sigma_refusal(c, 1)) return zs;
    if (t < 1 || t > n || n > ZK_AUDITORS_MAX || !rng_mode_ok(rng)) return ZK_E_ARG;
    ShareSplit G;
    if (zk_status zs = lay_out(c, B_et, [&](uint8_t* base) { return share_split_layout(G, base, rng_bytes(rng, 1)); })) return zs;
    // from the first upload on the secret and the seed lie in a witness-flagged buffer: every exit below zeroes them
    if (zk_status zs = upload_or_wipe(c, {{G.secret, secret_be32, 32}, {G.rng, rng->data, rng_bytes(rng, 1)}})) return zs;
    hipStream_t s = c->stream;
    RngCtx R{};
    R.exc_idx = G.exc_idx, R.exc_flags = G.exc_flags, R.exc_cnt = G.exc_cnt;
    sigma_chunk_rng(c, false, s, R, G.fill, zk_rng{rng->mode, G.rng, rng->stride_blocks}, 0, 1, SPLIT_RNG_BLOCKS);   // one "proof", in no timed scope
    launch_share_split(s, R, G.secret, t, n, G.L, G.shares, G.flag);
    launch_tom_commit(s, c->P, G.L, n, 1, 1);
    launch_tom_normalize(s, G.L, n, 0, 1, 1);
    launch_affine_to_bytes(s, G.L.ax, G.L.ay, n, 1, G.keys);
    uint32_t flag = 0;
    zk_status zs = download_or_wipe(c, {{G.flag, &flag, 4}});
    // the shares go straight into the caller's buffers, and only from a split whose draws were all there: no second host copy exists
    if (zs == ZK_OK && !flag) zs = download_or_wipe(c, {{G.shares, shares_be32, 32 * (size_t)n}, {G.keys, share_keys_xy72, 72 * (size_t)n}});
    wipe_witness(c);   // one key per call: nothing of it stays behind
    return zs ? zs : flag ? ZK_E_RNG_EXHAUSTED : ZK_OK;
}

// ------------------------------------------------------------------ lanes
static void share_carve(SoaCarver& k, ShareLane& X, uint32_t C) {
    X = ShareLane{};
    sigma_carve_core(k, X, C, SHR_SLOTS, SHR_RNG_BLOCKS, ZKS1_MSG_BLOCKS);
    X.kw = (uint32_t*)k.take(32 * (size_t)C);
    X.tab = (DistQuad*)k.take(sizeof(DistQuad) * DIST_TAB_QUADS * (size_t)C);
    X.rel = (uint32_t*)k.take(8 * (size_t)C);
}
// ... and, in front of the lanes, an auditor's call's staged secret
struct ShareRun : SigmaRun<ShareLane> {
    TomList S;            // [1] (a_j, 0), whose commitment is compared with A_j
    uint32_t* a8 = nullptr;
    uint8_t* ag = nullptr;
};
static zk_status share_plan(zk_ctx* c, uint64_t B, ShareRun& R) {
    return sigma_plan(c, B, B_et, R, share_carve, [&](SoaCarver& k) { R.S = k.list(1), R.a8 = (uint32_t*)k.take(32), R.ag = (uint8_t*)k.take(72); });
}

// ------------------------------------------------------------------ an auditor's shares
static zk_status share_device(zk_ctx* c, uint64_t B, uint32_t j, const uint8_t* d_secret, const ShareProveIo& io, const zk_rng& rng, uint64_t out_cap) {
    if (zk_status zs = share_refusal(c, B)) return zs;
    if (j < 1 || j > c->auditors_n || !rng_mode_ok(&rng)) return ZK_E_ARG;
    if (B == 0) return ZK_OK;
    if (!words_aligned({d_secret, io.tags, io.out, io.status, rng.data})) return ZK_E_ARG;
    ShareRun R;
    if (zk_status zs = share_plan(c, B, R)) return zs;
    timing_begin(c);   // (behind every refusal and the arenas: a call that runs nothing leaves the last call's record as it is)
    const bool timed = zk_timed(c, B);
    {
        MaybeScope t(timed, c, "escrow_open", c->stream);
        escrow_secret_point(c, c->stream, d_secret, R.S, R.a8, R.ag);
    }
    uint8_t ag[72];
    if (zk_status zs = download_or_wipe(c, {{R.ag, ag, 72}})) {   // (a blocking copy: the staged share secret is in place for every lane behind it)
        timing_end(c);
        return zs;
    }
    if (memcmp(ag, c->auditors_xy[j - 1], 72) != 0) {
        wipe_witness(c);
        timing_end(c);   // the key check ran: the call's record is its "escrow_open" family alone
        c->err = "the share secret does not belong to the share key A_j of the context's set";
        return ZK_E_OPENING;
    }
    if (B > out_cap / ZKS1_SIZE) {
        wipe_witness(c);
        timing_end(c);
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    const ShareSecret A{R.a8, j};
    return sigma_run_chunks(c, R, true, [&](ShareLane& K, hipStream_t s, uint32_t cnt, uint64_t first) {
        sigma_chunk_rng(c, timed, s, K.rng, K.rng_fill, rng, first, cnt, SHR_RNG_BLOCKS);
        {
            MaybeScope t(timed, c, "share_front", s);
            launch_share_front(s, K, cnt, first, io);
        }
        {
            MaybeScope t(timed, c, "tom_commit", s);
            launch_tom_commit(s, c->P, K.L, cnt, 1, 1);   // U1 = k g: the (g, h) comb with r = 0
        }
        {
            MaybeScope t(timed, c, "share_ladder", s);
            launch_share_ladder(s, K, A, cnt, first, io);   // D = a_j E1, U2 = k E1
        }
        {
            MaybeScope t(timed, c, "tom_normalize", s);
            launch_tom_normalize(s, K.L, SHR_SLOTS * cnt, 0, 1, 1);
        }
        {
            MaybeScope t(timed, c, "hash", s);
            launch_share_msg(s, K, c->auditors_w, j, cnt, first, io);
            launch_sigma_hash(s, K, cnt, ZKS1_MSG_BLOCKS);
        }
        {
            MaybeScope t(timed, c, "share_respond", s);
            launch_share_respond(s, K, A, cnt, first, io);
        }
    });   // (a failed call leaves neither a_j nor a nonce or RNG block behind)
}
extern "C" zk_status zk_auditors_share_batch_device(zk_ctx* c, uint64_t B, uint32_t j, const void* d_share_secret, const void* d_tags, const zk_rng* rng, void* d_out,
                                                    uint64_t out_cap, void* d_status) {
    if (!c || !rng || !d_share_secret || (B && (!d_tags || !rng->data || !d_out || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const zk_status zs = share_device(c, B, j, (const uint8_t*)d_share_secret, {(const uint8_t*)d_tags, (uint8_t*)d_out, (int32_t*)d_status}, *rng, out_cap);
    if (zs && zs != ZK_E_OPENING && c->params_set && !c->stream_busy) wipe_witness(c);
    return zs;
}
struct ShareProveIn {
    uint8_t *secret, *rng;
    int32_t* st;
};
static size_t share_prove_in_layout(ShareProveIn& I, uint8_t* base, size_t B, size_t rng_bytes) {
    Carver k(base);
    I.secret = (uint8_t*)k.take(32), I.rng = (uint8_t*)k.take(rng_bytes ? rng_bytes : 32), I.st = (int32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_auditors_share_batch(zk_ctx* c, uint64_t B, uint32_t j, const uint8_t share_secret_be32[32], const uint8_t* tags, const zk_rng* rng, uint8_t* out,
                                             uint64_t out_cap, int32_t* status) {
    if (!c || !rng || !share_secret_be32 || (B && (!tags || !rng->data || !out || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = share_refusal(c, B)) return zs;
    if (j < 1 || j > c->auditors_n || !rng_mode_ok(rng)) return ZK_E_ARG;
    if (B == 0) return ZK_OK;
    ShareProveIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return share_prove_in_layout(I, base, B, rng_bytes(rng, B)); })) return zs;
    if (zk_status zs = reserve(c, B_io, B * (ZKT1_SIZE + ZKS1_SIZE))) return zs;
    uint8_t* const d_tags = (uint8_t*)c->buf[B_io].p;
    uint8_t* const d_out = d_tags + B * ZKT1_SIZE;
    // from the first upload on the share secret and the seeds lie in the input buffer: every failure below zeroes them
    if (zk_status zs = upload_or_wipe(c, {{I.secret, share_secret_be32, 32}, {I.rng, rng->data, rng_bytes(rng, B)}, {d_tags, tags, B * ZKT1_SIZE}})) return zs;
    // (the capacity is judged behind the secret, as the contract orders the refusals: the staging buffer itself holds B shares)
    if (zk_status zs = share_device(c, B, j, I.secret, {d_tags, d_out, I.st}, zk_rng{rng->mode, I.rng, rng->stride_blocks}, out_cap)) {
        wipe_witness(c);
        return zs;
    }
    return download_or_wipe(c, {{d_out, out, B * ZKS1_SIZE}, {I.st, status, 4 * B}});
}

// ------------------------------------------------------------------ the share verifier
static zk_status share_verify_device(zk_ctx* c, uint64_t B, const ShareVerifyIo& io) {
    if (zk_status zs = share_refusal(c, B)) return zs;
    if (B == 0) return ZK_OK;
    if (!words_aligned({io.tags, io.shares, io.status})) return ZK_E_ARG;
    ShareRun R;
    if (zk_status zs = share_plan(c, B, R)) return zs;
    timing_begin(c);
    const bool timed = zk_timed(c, B);
    return sigma_run_chunks(c, R, false, [&](const ShareLane& K, hipStream_t s, uint32_t cnt, uint64_t first) {
        {
            MaybeScope t(timed, c, "share_parse", s);
            launch_share_parse(s, K, c->auditors_w, c->auditors_n, cnt, first, io);
            launch_sigma_hash(s, K, cnt, ZKS1_MSG_BLOCKS);
        }
        {
            MaybeScope t(timed, c, "tom_commit", s);
            launch_tom_commit(s, c->P, K.L, cnt, 1, 1);   // s g
        }
        {
            MaybeScope t(timed, c, "share_relations", s);
            launch_share_relations(s, K, c->auditors_w, cnt, first, io);
            launch_share_verdict(s, K, cnt, first, io);
        }
    });
}
extern "C" zk_status zk_auditors_share_verify_batch_device(zk_ctx* c, uint64_t B, const void* d_tags, const void* d_shares, void* d_ok, void* d_status) {
    if (!c || (B && (!d_tags || !d_shares || !d_ok || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return share_verify_device(c, B, {(const uint8_t*)d_tags, (const uint8_t*)d_shares, (uint8_t*)d_ok, (int32_t*)d_status});
}
struct ShareVerifyIn {   // no witness is staged: a failing copy returns as it is
    uint8_t* ok;
    int32_t* st;
};
static size_t share_verify_in_layout(ShareVerifyIn& I, uint8_t* base, size_t B) {
    Carver k(base);
    I.ok = (uint8_t*)k.take(B), I.st = (int32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_auditors_share_verify_batch(zk_ctx* c, uint64_t B, const uint8_t* tags, const uint8_t* shares, uint8_t* ok, int32_t* status) {
    if (!c || (B && (!tags || !shares || !ok || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = share_refusal(c, B)) return zs;
    if (B == 0) return ZK_OK;
    ShareVerifyIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return share_verify_in_layout(I, base, B); })) return zs;
    if (zk_status zs = reserve(c, B_io, B * (ZKT1_SIZE + ZKS1_SIZE))) return zs;
    uint8_t* const d_tags = (uint8_t*)c->buf[B_io].p;
    uint8_t* const d_shares = d_tags + B * ZKT1_SIZE;
    if (zk_status zs = upload_rows(c, {{d_tags, tags, B * ZKT1_SIZE}, {d_shares, shares, B * ZKS1_SIZE}})) return zs;
    if (zk_status zs = share_verify_device(c, B, {d_tags, d_shares, I.ok, I.st})) return zs;
    return download_rows(c, {{I.ok, ok, B}, {I.st, status, 4 * B}});
}

// ------------------------------------------------------------------ combine
// call level: t is the context's threshold and `auditors` holds t different indices in 1..n
static zk_status combine_refusal(zk_ctx* c, uint64_t B, uint32_t t, const uint32_t* auditors) {
    if (zk_status zs = share_refusal(c, B)) return zs;
    if (t != c->auditors_t) {
        c->err = "t is not the threshold of the context's set of share keys";
        return ZK_E_ARG;
    }
    uint32_t seen = 0;
    for (uint32_t s = 0; s < t; s++) {
        if (auditors[s] < 1 || auditors[s] > c->auditors_n || (seen >> auditors[s]) & 1) {
            c->err = "the auditors of a combine are t different indices in 1..n";
            return ZK_E_ARG;
        }
        seen |= 1u << auditors[s];
    }
    return ZK_OK;
}
// 1. the index of every resident ring that lacks one; 2. the t coefficients, once; 3. one lane per tag: the joint ladder and 4 (E2 - sum), normalised;
// 4. one lane per tag: the lookup in the ring its id names (the single-auditor opening's kernels).  The active ring is not read.
static zk_status combine_device(zk_ctx* c, uint64_t B, uint32_t t, const uint32_t* d_auditors, const uint8_t* d_tags, const uint8_t* d_shares, const uint32_t* d_ids,
                                uint32_t* d_ring_out, uint32_t* d_index, int32_t* d_status) {
    if (B == 0) return ZK_OK;
    if (!words_aligned({d_auditors, d_tags, d_shares, d_ids, d_ring_out, d_index, d_status})) return ZK_E_ARG;
    timing_begin(c);
    const bool timed = zk_timed(c, B);
    hipStream_t s0 = c->stream;
    Ring* rs[ZK_MAX_RINGS];
    uint32_t nr = 0;
    for (auto& R : c->rings)
        if (R.live && R.N) rs[nr++] = &R;
    std::sort(rs, rs + nr, [](const Ring* a, const Ring* b) { return a->id < b->id; });
    EscIndexSet S{};
    for (uint32_t k = 0; k < nr; k++) {
        zk_status built = ZK_OK;
        if (!rs[k]->esc_pts) {
            MaybeScope tm(timed, c, "escrow_index_build", s0);
            built = escrow_index_build(c, *rs[k]);
        }
        if (built) {
            timing_end(c);   // the record closes on every exit behind timing_begin
            return built;
        }
        S.r[S.count++] = escrow_index_desc(*rs[k], rs[k]->nkeys);
    }
    const uint32_t C = (uint32_t)std::min<uint64_t>(c->chunk, B);
    const std::vector<ChunkPlan> plan = make_chunk_plan(B, C, 1, false);
    const uint32_t NL = (uint32_t)std::min<size_t>(std::min<uint32_t>(c->lanes, ZK_MAX_LANES), plan.size());
    EscrowOpen O;
    uint32_t *lam = nullptr, *tab[ZK_MAX_LANES] = {};
    if (zk_status zs = lay_out(c, B_et, [&](uint8_t* base) {
            SoaCarver k(base);
            k.off = escrow_open_carve(O, base, B, 0);
            lam = (uint32_t*)k.take(32 * (size_t)t);
            for (uint32_t l = 0; l < NL; l++) tab[l] = (uint32_t*)k.take(4 * 27 * (size_t)t * C);   // a lane's addends: t entries of 27 words per tag of its chunk
            return k.off + ZK_LAYOUT_TAIL;
        })) {
        timing_end(c);
        return zs;
    }
    {
        MaybeScope tm(timed, c, "combine_ladder", s0);
        launch_share_lagrange(s0, d_auditors, t, nullptr, 1, lam);
    }
    hipError_t e = hipStreamSynchronize(s0);   // the coefficients are in place for every lane behind it
    const ShareCombineIo io{d_tags, d_shares, d_auditors, B, t};
    for (uint64_t k = 0; e == hipSuccess && k < plan.size(); k++) {
        hipStream_t s = c->pl[k % NL].stream;
        MaybeScope tm(timed, c, "combine_ladder", s);
        launch_share_combine(s, O, io, lam, tab[k % NL], plan[k].cnt, plan[k].first, d_index, d_status);
    }
    if (e == hipSuccess) e = drain_lanes(c, NL);
    if (e == hipSuccess) {
        {
            MaybeScope tm(timed, c, "tom_normalize", s0);
            launch_tom_normalize(s0, O.T, (uint32_t)B, 0, 1, 1);
        }
        {
            MaybeScope tm(timed, c, "escrow_lookup", s0);
            launch_escrow_index_lookup(s0, S, O, B, d_ids, d_ring_out, d_index, d_status);
        }
        e = hipStreamSynchronize(s0);
    }
    if (e != hipSuccess) wipe_witness(c);   // a failed call leaves no a_j E1 behind
    HIPCHK(c, e);
    HIPCHK(c, hipGetLastError());
    timing_end(c);
    return ZK_OK;
}
extern "C" zk_status zk_auditors_combine_batch_device(zk_ctx* c, uint64_t B, uint32_t t, const void* d_auditors, const void* d_tags, const void* d_shares,
                                                      const void* d_ring_ids, void* d_ring_out, void* d_index, void* d_status) {
    if (!c || !d_auditors || (B && (!d_tags || !d_shares || !d_ring_ids || !d_ring_out || !d_index || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (t < 1 || t > ZK_AUDITORS_MAX || ((uintptr_t)d_auditors & 3)) return ZK_E_ARG;
    if (zk_status zs = share_refusal(c, B)) return zs;
    uint32_t auditors[ZK_AUDITORS_MAX];
    HIPCHK(c, hipMemcpy(auditors, d_auditors, 4 * (size_t)t, hipMemcpyDeviceToHost));   // the call-level rules read them; they are public
    if (zk_status zs = combine_refusal(c, B, t, auditors)) return zs;
    const zk_status zs = combine_device(c, B, t, (const uint32_t*)d_auditors, (const uint8_t*)d_tags, (const uint8_t*)d_shares, (const uint32_t*)d_ring_ids, (uint32_t*)d_ring_out,
                                        (uint32_t*)d_index, (int32_t*)d_status);
    if (zs && c->params_set && !c->stream_busy) wipe_witness(c);
    return zs;
}
struct CombineIn {
    uint32_t *auditors, *ids, *ring, *index;
    int32_t* st;
};
static size_t combine_in_layout(CombineIn& I, uint8_t* base, size_t B) {
    Carver k(base);
    I.auditors = (uint32_t*)k.take(4 * ZK_AUDITORS_MAX), I.ids = (uint32_t*)k.take(4 * B), I.ring = (uint32_t*)k.take(4 * B), I.index = (uint32_t*)k.take(4 * B);
    I.st = (int32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_auditors_combine_batch(zk_ctx* c, uint64_t B, uint32_t t, const uint32_t* auditors_u32, const uint8_t* tags, const uint8_t* shares,
                                               const uint32_t* ring_ids, uint32_t* ring_out_u32, uint32_t* index_u32, int32_t* status) {
    if (!c || !auditors_u32 || (B && (!tags || !shares || !ring_ids || !ring_out_u32 || !index_u32 || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (t < 1 || t > ZK_AUDITORS_MAX) return ZK_E_ARG;
    if (zk_status zs = combine_refusal(c, B, t, auditors_u32)) return zs;
    if (B == 0) return ZK_OK;
    CombineIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return combine_in_layout(I, base, B); })) return zs;
    if (zk_status zs = reserve(c, B_io, B * (ZKT1_SIZE + (size_t)t * ZKS1_SIZE))) return zs;
    uint8_t* const d_tags = (uint8_t*)c->buf[B_io].p;
    uint8_t* const d_shares = d_tags + B * ZKT1_SIZE;
    if (zk_status zs = upload_or_wipe(c, {{I.auditors, auditors_u32, 4 * (size_t)t}, {I.ids, ring_ids, 4 * B}, {d_tags, tags, B * ZKT1_SIZE}, {d_shares, shares, B * t * ZKS1_SIZE}}))
        return zs;
    if (zk_status zs = combine_device(c, B, t, I.auditors, d_tags, d_shares, I.ids, I.ring, I.index, I.st)) {
        wipe_witness(c);
        return zs;
    }
    return download_or_wipe(c, {{I.ring, ring_out_u32, 4 * B}, {I.index, index_u32, 4 * B}, {I.st, status, 4 * B}});
}
