// zk_member_prove_batch / zk_member_verify_batch (include/zkattest.h): proveMembership / verifyMembership (gk.ts:94-262) on the active ring, without a ZKAttest
// proof around them.  Host-side pipeline; the kernels of its own are in k_member.hip, everything heavy is the GK phase of the full prover and verifier.
#include "ctx.h"
#include "jobs.h"
#include "member.h"

zk_status make_default_vseeds(zk_ctx* c, uint64_t B, uint8_t* d_seeds, hipStream_t s);   // api_verify.hip

// A lane's arena: the fields of Workspace / VWork that the GK kernels, the commitment kernels and k_member.hip read -- every other pointer stays nullptr.
// W.sec only sizes the challenge hash's message buffers here (k_hash.hip: launch_gk_hash compares against the Exp challenge's block count): the GK message of
// 4 n points fits the buffers of 2 n repetitions; the layout's repetition terms are zero (wire.rep_head = wire.padd = 0), so it moves no byte of the output.
static size_t mcarve(zk_ctx* c, zk_ctx::MemberLane& L, uint8_t* base, uint32_t C, uint32_t n, uint64_t N) {
    SoaCarver k(base);
    Workspace& W = L.W;
    W = Workspace{};
    W.C = C, W.sec = 2 * n, W.n = n, W.N = (uint32_t)N;
    W.st = (int32_t*)k.take(4 * (size_t)C);
    W.zcnt = (uint32_t*)k.take(4 * (size_t)C);
    W.out_base = (uint64_t*)k.take(8 * ((size_t)C + 1));
    W.lc = k.list((size_t)C * (4 * n + 1));
    W.gk_blind = k.soa(C);
    W.gk_x = (uint32_t*)k.take(12 * (size_t)C);
    W.gk_coef = k.soa((size_t)(n + 1) * C);
    L.gk_am = k.soa((size_t)n * C);
    L.which_s = (uint32_t*)k.take(4 * (size_t)C);
    // the fold's buffers, as the full prover's workspace sizes them (api.hip: carve)
    const uint64_t g = std::max<uint64_t>(1, std::min<uint64_t>(C, ((uint64_t)1 << 16) / N));
    W.gk_group = (uint32_t)g;
    const uint32_t T = c->ring->gk_etab ? 8 : std::min<uint32_t>(n, 12);
    const uint64_t tile_elems = (uint64_t)(T + 1) * C * (N >> T);
    W.gk_adig = c->ring->gk_edig ? (int8_t*)k.take(gkm_asub_frag_bytes(C)) : nullptr;
    W.gk_toff = (uint32_t*)k.take(4 * 264);
    W.gk_asub = c->ring->gk_etab ? (uint32_t*)k.take(36 * 256 * (size_t)C) : nullptr;
    W.gk_order = (uint32_t*)k.take(4 * (size_t)C);
    W.gk_goff = (uint32_t*)k.take(4 * 264);
    W.gk_bufA = (uint32_t*)k.take(36 * std::max<uint64_t>(g * N, tile_elems));
    W.gk_bufB = (uint32_t*)k.take(36 * std::max<uint64_t>(g * N, (uint64_t)(n + 1) * C * std::max<uint64_t>(1, (N >> T) / gk_finish_gsz(T, (uint32_t)(N >> T)))));
    W.rng.exc_idx = (uint32_t*)k.take(4 * RNG_MAX_EXC * (size_t)C);
    W.rng.exc_flags = (uint32_t*)k.take(4 * RNG_MAX_EXC * (size_t)C);
    W.rng.exc_cnt = (uint32_t*)k.take(4 * (size_t)C);
    W.rng_fill = (uint32_t*)k.take(32 * (size_t)(1 + 5 * n + RNG_MAX_EXC) * C);
    {
        const size_t blocks = (2 * 67 + (size_t)W.sec * (65 + 2 * 67) + 9 + 63) / 64, np = std::min<size_t>(C, EXPH_MAXP);
        W.exph_msg = (uint8_t*)k.take(np * blocks * 64), W.exph_wk = (uint32_t*)k.take(np * blocks * 256), W.exph_cap = (uint32_t)np;
    }
    W.wire = wire_make(false);
    W.wire.fixed = ZKM1_HDR, W.wire.rep_head = 0, W.wire.padd = 0, W.wire.magic = ZK_MAGIC_ZKM1;
    // the verifier's view
    VWork& V = L.V;
    V = VWork{};
    V.C = C, V.sec = 0, V.n = n;
    V.gk_fixed = ZKM1_HDR;
    V.st = (int32_t*)k.take(4 * (size_t)C);
    V.okflags = (uint32_t*)k.take(4 * (size_t)C);
    V.zcnt = (uint32_t*)k.take(4 * (size_t)C);
    V.gkx = (uint32_t*)k.take(12 * (size_t)C);
    V.gk_f = k.soa((size_t)n * C), V.gk_g = k.soa((size_t)n * C);
    V.gk_total = k.soa(C);
    V.gk_csub = (uint32_t*)k.take(n >= GK_ETAB_MINN && n <= GK_ETAB_MAXN ? std::max<size_t>(36 * 256 * (size_t)C, n >= GKM_MINN ? gkm_coef_frag_bytes(C) : 0) : 16);
    V.gk_swap = (uint32_t*)k.take(4 * (size_t)n * C);
    const size_t nq = (n + 1) / 2;
    auto terms = [&](size_t cnt) {
        return VTerms{(uint32_t*)k.take(cnt * VT_ENTRY_WORDS * 4), k.soa(cnt), (uint32_t*)k.take(cnt * 8 * 36 * 4), (uint8_t*)k.take(cnt * 65), (uint32_t)cnt};
    };
    auto soa4 = [&](size_t cnt) { return Soa4{k.soa(cnt), k.soa(cnt), k.soa(cnt), k.soa(cnt)}; };
    V.gk_terms = terms((size_t)C * nq * 8);
    V.misc_terms = terms((size_t)C * 3);
    V.gk_acc = soa4((size_t)C * nq), V.misc_acc = soa4((size_t)C * 3);
    const uint32_t VT = n >= GK_ETAB_MINN && n <= GK_ETAB_MAXN ? 8 : std::min<uint32_t>(n, 13);
    L.res = k.soa((size_t)C * (N >> VT));
    L.res2 = k.soa((size_t)C * std::max<uint64_t>(1, (N >> VT) / 512));
    return k.off + 256;
}
static zk_status ensure_member_lanes(zk_ctx* c, uint32_t C, uint32_t nlanes) {
    const uint32_t n = c->ring->n;
    const bool etab = c->ring->gk_etab != nullptr, edig = c->ring->gk_edig != nullptr;
    if (!(c->ms_C == C && c->ms_n == n && c->ms_etab == etab && c->ms_edig == edig)) {
        for (auto& L : c->ml) L.ready = false;
        c->ms_C = C, c->ms_n = n, c->ms_etab = etab, c->ms_edig = edig;
    }
    for (uint32_t l = 0; l < nlanes && l < ZK_MAX_LANES; l++) {
        auto& L = c->ml[l];
        if (!L.ready) {
            if (zk_status zs = lay_out(c, L.arena, GROW_SHED, [&](uint8_t* base) { return mcarve(c, L, base, C, n, c->ring->N); })) return zs;
            L.ready = true;
        }
        // the ring's pointers are bound on every call (zk_ctx_use_ring, zk_ctx_update_ring, zk_ctx_set_ring_fold)
        L.W.ring = Soa{c->ring->ring_mem, (uint32_t)c->ring->N};
        L.W.gk_etab = c->ring->gk_etab;
        L.W.gk_kdig = c->gk_mfma ? c->ring->gk_kdig : nullptr;
        L.W.gk_edig = c->gk_mfma && L.W.gk_adig ? c->ring->gk_edig : nullptr;
    }
    return ZK_OK;
}
static zk_status member_refusal(zk_ctx* c) {
    if (!c->params_set || !c->ring->N) return ZK_E_BUFFER;
    if (c->stream_busy) return busy_refusal(c);
    if (c->mode == ZK_MODE_HARDENED) {
        c->err = "membership proofs on their own have no statement to bind: not available in ZK_MODE_HARDENED";
        return ZK_E_ARG;
    }
    return ZK_OK;
}
extern "C" uint64_t zk_member_proof_size(const zk_ctx* c) {
    if (!c || !c->ring->N) return 0;
    return zkm1_size(c->ring->n);
}

// ------------------------------------------------------------------ prover
static zk_status member_prove_device(zk_ctx* c, uint64_t B, const uint32_t* d_which, const uint8_t* d_blinder, int rng_mode, const uint8_t* d_rng, uint64_t stride,
                                     uint8_t* d_com, uint8_t* d_blinder_out, uint8_t* d_out, uint64_t out_cap, int32_t* d_status) {
    if (zk_status zs = member_refusal(c)) return zs;
    if (rng_mode != ZK_RNG_SEED && rng_mode != ZK_RNG_STREAM) return ZK_E_ARG;
    const uint32_t size = (uint32_t)zkm1_size(c->ring->n);
    if (B > out_cap / size) {
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    timing_begin(c);
    if (B == 0) return ZK_OK;
    const DevParams& P = c->P;
    const uint32_t C = (uint32_t)std::min<uint64_t>(c->chunk, B);
    const std::vector<ChunkPlan> plan = make_chunk_plan(B, C, 1, false);
    const uint32_t NL = (uint32_t)std::min<size_t>(c->lanes, plan.size());
    if (zk_status zs = ensure_member_lanes(c, C, NL)) return zs;
    const bool timed = zk_timed(c, B);
    zk_status zs = ZK_OK;
    auto chunk = [&](uint64_t k) -> zk_status {
        const uint32_t lane = (uint32_t)(k % NL), cnt = plan[k].cnt;
        const uint64_t first = plan[k].first;
        auto& L = c->ml[lane];
        Workspace& W = L.W;
        hipStream_t s = c->pl[lane].stream;
        W.gk_fill0 = d_blinder ? 0 : 1;
        const uint32_t nblk = W.gk_fill0 + 5 * W.n + RNG_MAX_EXC;   // + margin: rejected fills shift later draws
        W.rng.seeds = d_rng, W.rng.stream = d_rng, W.rng.stride_blocks = stride, W.rng.mode = rng_mode, W.rng.sec = -1, W.rng.proof_base = (uint32_t)first;
        {
            MaybeScope t(timed, c, "rng_prepass", s);
            launch_rng_prepass(s, W, cnt, 0, nblk, nblk, rng_mode == 0 ? W.rng_fill : nullptr, false);
        }
        if (rng_mode == 0)   // from here on the chunk reads the fills the prepass wrote
            W.rng.mode = 1, W.rng.stream = (const uint8_t*)W.rng_fill, W.rng.stride_blocks = nblk, W.rng.proof_base = 0;
        const ChunkIn in{nullptr, nullptr, nullptr, L.which_s, cnt};
        const uint32_t nc = cnt * (4 * W.n + 1);   // the 4 n membership commitments of every proof, then every proof's com
        {
            MaybeScope t(timed, c, "gk_fold", s);
            launch_m_front(s, W, cnt, d_which, d_blinder, first, L.which_s);
            launch_gk_scalars_fold(s, W, in, L.gk_am);
            launch_gk_cd_scalars(s, W, cnt);
        }
        {
            MaybeScope t(timed, c, "tom_commit", s);
            launch_tom_commit(s, P, W.lc, nc, 1, 1);
        }
        {
            MaybeScope t(timed, c, "tom_normalize", s);
            launch_tom_normalize(s, W.lc, nc, 0, 1, 1);
        }
        {
            MaybeScope t(timed, c, "hash", s);
            launch_gk_hash(s, W, cnt, nullptr);
        }
        {
            MaybeScope t(timed, c, "respond_write", s);
            uint8_t* out = d_out + first * size;
            launch_m_write_head(s, W, cnt, first, size, out, d_com, d_blinder_out, d_status);
            launch_gk_respond(s, W, in, out);
        }
        return ZK_OK;
    };
    for (uint64_t k = 0; k < plan.size() && !zs; k++) zs = chunk(k);
    hipError_t e_sync = hipSuccess;
    for (uint32_t l = 0; l < NL; l++) {
        const hipError_t e = hipStreamSynchronize(c->pl[l].stream);
        if (e_sync == hipSuccess) e_sync = e;
    }
    if (zs || e_sync != hipSuccess) wipe_witness(c);   // a failed call leaves no nonce, blinder or RNG block behind
    if (zs) return zs;
    HIPCHK(c, e_sync);
    HIPCHK(c, hipGetLastError());
    timing_end(c);
    return ZK_OK;
}
extern "C" zk_status zk_member_prove_batch_device(zk_ctx* c, uint64_t B, const void* d_which, const void* d_blinder, const zk_rng* rng, void* d_com, void* d_blinder_out,
                                                  void* d_out, uint64_t out_cap, void* d_status) {
    if (!c || !rng || (B && (!d_which || !rng->data || !d_com || !d_out || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return member_prove_device(c, B, (const uint32_t*)d_which, (const uint8_t*)d_blinder, rng->mode, rng->data, rng->stride_blocks, (uint8_t*)d_com, (uint8_t*)d_blinder_out,
                               (uint8_t*)d_out, out_cap, (int32_t*)d_status);
}
// Host pointers: the small arrays through the context's input buffer (witness-derived: wiped with it), the proofs through its output staging buffer.
struct MemberProveIn {
    uint32_t* which;
    uint8_t *blinder, *rng, *com, *blinder_out;
    int32_t* st;
};
static size_t member_prove_in_layout(MemberProveIn& I, uint8_t* base, size_t B, size_t rng_bytes) {
    Carver k(base);
    I.which = (uint32_t*)k.take(4 * B), I.blinder = (uint8_t*)k.take(32 * B), I.rng = (uint8_t*)k.take(rng_bytes ? rng_bytes : 32), I.com = (uint8_t*)k.take(72 * B);
    I.blinder_out = (uint8_t*)k.take(32 * B), I.st = (int32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_member_prove_batch(zk_ctx* c, uint64_t B, const uint32_t* which, const uint8_t* blinder, const zk_rng* rng, uint8_t* com, uint8_t* blinder_out,
                                           uint8_t* out, uint64_t out_cap, int32_t* status) {
    if (!c || !rng || (B && (!which || !rng->data || !com || !out || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = member_refusal(c)) return zs;
    if (rng->mode != ZK_RNG_SEED && rng->mode != ZK_RNG_STREAM) return ZK_E_ARG;
    const uint64_t size = zkm1_size(c->ring->n);
    if (B > out_cap / size) {
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    if (B == 0) return ZK_OK;
    const size_t rng_bytes = rng->mode == ZK_RNG_SEED ? 32 * B : 32 * B * rng->stride_blocks;
    MemberProveIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return member_prove_in_layout(I, base, B, rng_bytes); })) return zs;
    if (zk_status zs = reserve(c, B_io, B * size)) return zs;
    uint8_t* const d_out = (uint8_t*)c->buf[B_io].p;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(I.which, which, 4 * B, hipMemcpyHostToDevice, s));
    if (blinder) HIPCHK(c, hipMemcpyAsync(I.blinder, blinder, 32 * B, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(I.rng, rng->data, rng_bytes, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));   // the lanes' streams start behind the inputs
    zk_status zs = member_prove_device(c, B, I.which, blinder ? I.blinder : nullptr, rng->mode, I.rng, rng->stride_blocks, I.com, blinder_out ? I.blinder_out : nullptr, d_out,
                                       B * size, I.st);
    if (zs) return zs;
    HIPCHK(c, hipMemcpyAsync(out, d_out, B * size, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(com, I.com, 72 * B, hipMemcpyDeviceToHost, s));
    if (blinder_out) HIPCHK(c, hipMemcpyAsync(blinder_out, I.blinder_out, 32 * B, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(status, I.st, 4 * B, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return ZK_OK;
}

// ------------------------------------------------------------------ verifier
static zk_status member_verify_device(zk_ctx* c, uint64_t B, const uint8_t* d_com, const uint8_t* d_proofs, const uint8_t* d_vseeds, uint8_t* d_ok, int32_t* d_status) {
    if (zk_status zs = member_refusal(c)) return zs;
    timing_begin(c);
    if (B == 0) return ZK_OK;
    const DevParams& P = c->P;
    const uint64_t size = zkm1_size(c->ring->n);
    const uint32_t C = (uint32_t)std::min<uint64_t>(c->chunk, B);
    const std::vector<ChunkPlan> plan = make_chunk_plan(B, C, 1, false);
    const uint32_t NL = (uint32_t)std::min<size_t>(c->lanes, plan.size());
    if (zk_status zs = ensure_member_lanes(c, C, NL)) return zs;
    if (zk_status zs = reserve(c, B_m_off, 8 * (B + 1))) return zs;
    uint64_t* const d_off = (uint64_t*)c->buf[B_m_off].p;
    launch_mv_offsets(c->stream, d_off, B, size);
    if (!d_vseeds) {   // the verifier's own seeds (api_verify.hip): fresh OS randomness per call
        if (zk_status zs = reserve(c, B_seed, 32 * B)) return zs;
        if (zk_status zs = make_default_vseeds(c, B, (uint8_t*)c->buf[B_seed].p, c->stream)) return zs;
        d_vseeds = (const uint8_t*)c->buf[B_seed].p;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));   // offsets and seeds are there before any lane reads them
    const bool timed = zk_timed(c, B);
    for (uint64_t k = 0; k < plan.size(); k++) {
        const uint32_t lane = (uint32_t)(k % NL), cnt = plan[k].cnt;
        const uint64_t first = plan[k].first;
        auto& L = c->ml[lane];
        Workspace& W = L.W;
        VWork& V = L.V;
        V.com = d_com;
        hipStream_t s = c->pl[lane].stream;
        const uint32_t nq = (V.n + 1) / 2;
        {
            MaybeScope t(timed, c, "v_parse_validate", s);
            launch_mv_header_validate(s, V, cnt, d_proofs, d_off, first);
        }
        {
            MaybeScope t(timed, c, "v_gk_total", s);
            launch_v_challenges(s, V, cnt, d_proofs, d_off, nullptr, first, 2);
            launch_v_gk_total(s, V, W.ring, W.gk_etab, W.gk_kdig, cnt, W.N, d_proofs, d_off, first, L.res, L.res2);
            launch_v_proof_points(s, V, cnt, d_proofs, d_off, first, 1);
            launch_v_proof_terms(s, W, V, cnt, d_proofs, d_off, d_vseeds, first);
        }
        {
            MaybeScope t(timed, c, "v_sums", s);
            launch_v_straus(s, V.gk_terms, cnt * nq, V.C * nq, 4, 4, V.gk_acc, nullptr, nullptr);
            launch_v_straus(s, V.misc_terms, cnt, 3 * V.C, 1, 0, V.misc_acc, nullptr, nullptr);
            launch_tom_commit(s, P, W.lc, cnt, 1, 4 * W.n);
            launch_mv_final(s, W, V, cnt, d_ok, d_status, first);
        }
    }
    hipError_t e_sync = hipSuccess;
    for (uint32_t l = 0; l < NL; l++) {
        const hipError_t e = hipStreamSynchronize(c->pl[l].stream);
        if (e_sync == hipSuccess) e_sync = e;
    }
    HIPCHK(c, e_sync);
    HIPCHK(c, hipGetLastError());
    timing_end(c);
    return ZK_OK;
}
extern "C" zk_status zk_member_verify_batch_device(zk_ctx* c, uint64_t B, const void* d_com, const void* d_proofs, const void* d_vseeds, void* d_ok, void* d_status) {
    if (!c || (B && (!d_com || !d_proofs || !d_ok || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return member_verify_device(c, B, (const uint8_t*)d_com, (const uint8_t*)d_proofs, (const uint8_t*)d_vseeds, (uint8_t*)d_ok, (int32_t*)d_status);
}
struct MemberVerifyIn {
    uint8_t *com, *seeds, *ok;
    int32_t* st;
};
static size_t member_verify_in_layout(MemberVerifyIn& I, uint8_t* base, size_t B) {
    Carver k(base);
    I.com = (uint8_t*)k.take(72 * B), I.seeds = (uint8_t*)k.take(32 * B), I.ok = (uint8_t*)k.take(B), I.st = (int32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_member_verify_batch(zk_ctx* c, uint64_t B, const uint8_t* com, const uint8_t* proofs, const uint8_t* vseeds, uint8_t* ok, int32_t* status) {
    if (!c || (B && (!com || !proofs || !ok || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = member_refusal(c)) return zs;
    if (B == 0) return ZK_OK;
    const uint64_t size = zkm1_size(c->ring->n);
    MemberVerifyIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return member_verify_in_layout(I, base, B); })) return zs;
    if (zk_status zs = reserve(c, B_io, B * size)) return zs;
    uint8_t* const d_proofs = (uint8_t*)c->buf[B_io].p;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(I.com, com, 72 * B, hipMemcpyHostToDevice, s));
    if (vseeds) HIPCHK(c, hipMemcpyAsync(I.seeds, vseeds, 32 * B, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_proofs, proofs, B * size, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (zk_status zs = member_verify_device(c, B, I.com, d_proofs, vseeds ? I.seeds : nullptr, I.ok, I.st)) return zs;
    HIPCHK(c, hipMemcpyAsync(ok, I.ok, B, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(status, I.st, 4 * B, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return ZK_OK;
}
