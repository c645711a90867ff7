// zk_member_prove_batch / zk_member_verify_batch (include/zkattest.h): proveMembership / verifyMembership (gk.ts:94-262) on the active ring, without a ZKAttest
// proof around them, their _rings forms with one resident ring id per proof, and the _bound forms of all of them ("ZKMB": the challenge also hashes the ring's
// digest, 32 context bytes of the caller's and the commitment -- the `ctx` of MemberProveArgs / MemberVerifyArgs below; nullptr = the unbound call).  Host-side
// pipeline; the kernels of its own are in k_member.hip and k_member_rings.hip, everything heavy is the GK phase of the full prover and verifier.
// Every bound / unbound pair of entry points is one path: `bound` says which of the two was called (the NULL check's only), context == nullptr the unbound one.
// The host-pointer workers check their arguments themselves; a *_device_entry does it for the _device pair and hands the device worker its arguments checked.
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
    carve_gk_scalars(k, W, L.gk_am);
    L.which_s = (uint32_t*)k.take(4 * (size_t)C);
    carve_gk_fold(k, W, *c->ring, N);
    carve_rng(k, W, member_rng_blocks(n, 1));
    carve_exph(k, W);
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
    carve_v_gk_scalars(k, V);
    const size_t nq = (n + 1) / 2;
    auto terms = [&](size_t cnt) {
        return VTerms{(uint32_t*)k.take(cnt * VT_ENTRY_WORDS * 4), k.soa(cnt), (uint32_t*)k.take(cnt * 8 * 36 * 4), (uint8_t*)k.take(cnt * 65), (uint32_t)cnt};
    };
    auto soa4 = [&](size_t cnt) { return Soa4{k.soa(cnt), k.soa(cnt), k.soa(cnt), k.soa(cnt)}; };
    V.gk_terms = terms((size_t)C * nq * 8);
    V.misc_terms = terms((size_t)C * 3);
    V.gk_acc = soa4((size_t)C * nq), V.misc_acc = soa4((size_t)C * 3);
    carve_v_gk_fold(k, L.res, L.res2, C, n, N);
    return k.off + 256;
}
zk_status ensure_member_lanes(zk_ctx* c, uint32_t C, uint32_t nlanes) {   // (also api_rering.hip)
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
        bind_ring(L.W, c);
    }
    return ZK_OK;
}
static zk_status member_refusal(zk_ctx* c, bool bound, bool need_ring = true) {   // (the mixed-ring forms read no active ring)
    if (!c->params_set || (need_ring && !c->ring->N)) return ZK_E_BUFFER;
    if (c->stream_busy) return busy_refusal(c);
    if (c->mode == ZK_MODE_HARDENED && !bound) {   // a bound call names its statement itself, in either mode
        c->err = "an unbound membership proof hashes no statement: not available in ZK_MODE_HARDENED (use the _bound calls)";
        return ZK_E_ARG;
    }
    return ZK_OK;
}
extern "C" uint64_t zk_member_proof_size(const zk_ctx* c) {
    if (!c || !c->ring->N) return 0;
    return zkm1_size(c->ring->n);
}
// What differs between a whole call and one window of a mixed-ring call.  C: the chunk size the lanes are carved for.  sel.sel != nullptr: a window -- its
// inputs lie gathered in the window's arrays, its results go through `sel` to their final places in the batch's buffers, the lanes start behind `ready`, and
// (verifier) every slot is `slot` bytes long.
struct MemberRun {
    uint32_t C;
    bool timed;
    uint32_t slot = 0;
    MemberSel sel{};
    hipEvent_t ready = nullptr;
};

// ------------------------------------------------------------------ prover
// The device pointers of a prove call, or of one window of it (member_prove_window_args)
struct MemberProveArgs {
    const uint32_t* which;
    const uint8_t* blinder;   // nullptr: the engine draws com's blinders
    zk_rng rng;               // data: a device pointer (the _device entry points leave it empty: *_device_entry copies the caller's once it is known not to be NULL)
    const uint8_t* ctx;       // nullptr: the unbound call; else 32 context bytes per proof, indexed like `which`
    uint8_t *com, *blinder_out, *out;
    int32_t* status;
};
// The chunks of B proofs over the bound ring on the lanes: a one-ring call, or one window of a mixed-ring call (R.sel), whose proofs lie where the batch's
// offsets say.  Every lane is drained before it returns; *e_sync is what draining them gave.  Wipes nothing and leaves the call's timing to its caller.
static zk_status member_prove_run(zk_ctx* c, uint64_t B, const MemberProveArgs& A, const MemberRun& R, hipError_t* e_sync) {
    const uint32_t size = (uint32_t)zkm1_size(c->ring->n);
    const std::vector<ChunkPlan> plan = make_chunk_plan(B, R.C, 1, false);
    const uint32_t NL = (uint32_t)std::min<size_t>(c->lanes, plan.size());
    if (zk_status zs = ensure_member_lanes(c, R.C, NL)) return zs;
    if (R.ready)
        for (uint32_t l = 0; l < NL; l++) HIPCHK(c, hipStreamWaitEvent(c->pl[l].stream, R.ready, 0));
    for (uint64_t k = 0; k < plan.size(); k++) {
        const uint32_t lane = (uint32_t)(k % NL), cnt = plan[k].cnt;
        const uint64_t first = plan[k].first;
        auto& L = c->ml[lane];
        Workspace& W = L.W;
        hipStream_t s = c->pl[lane].stream;
        W.gk_fill0 = A.blinder ? 0 : 1;
        // bound: the challenge hashes the bound ring's digest, the proof's context and its com; the header says so
        W.gk_stmt = A.ctx ? GK_STMT_MEMBER : GK_STMT_NONE, W.ring_digest = c->ring->ring_digest, W.wire.magic = A.ctx ? ZK_MAGIC_ZKMB : ZK_MAGIC_ZKM1;
        member_chunk_rng(c, R.timed, s, W, A.rng, first, cnt);
        const ChunkIn in = member_chunk_commit(c, R.timed, s, W, L, cnt, [&] { launch_m_front(s, W, cnt, A.which, A.blinder, first, L.which_s); });
        {
            MaybeScope t(R.timed, c, "hash", s);
            launch_gk_hash(s, W, cnt, A.ctx ? A.ctx + 32 * first : nullptr);   // behind the normaliser: com's affine coordinates are the ones k_m_write_head writes out
        }
        {
            MaybeScope t(R.timed, c, "respond_write", s);
            uint8_t* out = R.sel.sel ? A.out : A.out + first * size;   // (a window's proofs lie where the batch's offsets say: W.out_base)
            launch_m_write_head(s, W, cnt, first, size, out, A.com, A.blinder_out, A.status, R.sel);
            launch_gk_respond(s, W, in, out);
        }
    }
    *e_sync = drain_lanes(c, NL);
    return ZK_OK;
}
static zk_status member_prove_device(zk_ctx* c, uint64_t B, const MemberProveArgs& A, uint64_t out_cap) {
    if (zk_status zs = member_refusal(c, A.ctx != nullptr)) return zs;
    if (!rng_mode_ok(&A.rng)) return ZK_E_ARG;
    if (B > out_cap / zkm1_size(c->ring->n)) {
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    timing_begin(c);
    if (B == 0) return ZK_OK;
    hipError_t e_sync = hipSuccess;
    const zk_status zs = member_prove_run(c, B, A, MemberRun{(uint32_t)std::min<uint64_t>(c->chunk, B), zk_timed(c, B)}, &e_sync);
    if (zs || e_sync != hipSuccess) wipe_witness(c);   // a failed call leaves no nonce, blinder or RNG block behind
    if (zs) return zs;
    HIPCHK(c, e_sync);
    HIPCHK(c, hipGetLastError());
    timing_end(c);
    return ZK_OK;
}
static zk_status member_prove_device_entry(zk_ctx* c, uint64_t B, bool bound, const zk_rng* rng, MemberProveArgs A, uint64_t out_cap) {
    if (!c || !rng || (bound && !A.ctx) || (B && (!A.which || !rng->data || !A.com || !A.out || !A.status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    A.rng = *rng;
    return member_prove_device(c, B, A, out_cap);
}
extern "C" zk_status zk_member_prove_batch_device(zk_ctx* c, uint64_t B, const void* d_which, const void* d_blinder, const zk_rng* rng, void* d_com, void* d_blinder_out,
                                                  void* d_out, uint64_t out_cap, void* d_status) {
    return member_prove_device_entry(c, B, false, rng, {(const uint32_t*)d_which, (const uint8_t*)d_blinder, {}, nullptr, (uint8_t*)d_com, (uint8_t*)d_blinder_out,
                                                        (uint8_t*)d_out, (int32_t*)d_status}, out_cap);
}
extern "C" zk_status zk_member_prove_batch_bound_device(zk_ctx* c, uint64_t B, const void* d_which, const void* d_context, const void* d_blinder, const zk_rng* rng, void* d_com,
                                                        void* d_blinder_out, void* d_out, uint64_t out_cap, void* d_status) {
    return member_prove_device_entry(c, B, true, rng, {(const uint32_t*)d_which, (const uint8_t*)d_blinder, {}, (const uint8_t*)d_context, (uint8_t*)d_com,
                                                       (uint8_t*)d_blinder_out, (uint8_t*)d_out, (int32_t*)d_status}, out_cap);
}
// Host pointers: the small arrays through the context's input buffer (witness-derived: wiped with it), the proofs through its output staging buffer.
// `rings`: the _rings form, whose ids cross too and whose offsets come back.
struct MemberProveIn {
    uint32_t *which, *ids;
    uint8_t *blinder, *rng, *com, *blinder_out, *ctx;
    int32_t* st;
    uint64_t* off;
};
static size_t member_prove_in_layout(MemberProveIn& I, uint8_t* base, size_t B, size_t rng_bytes, bool rings) {
    Carver k(base);
    I.which = (uint32_t*)k.take(4 * B), I.blinder = (uint8_t*)k.take(32 * B), I.rng = (uint8_t*)k.take(rng_bytes ? rng_bytes : 32), I.com = (uint8_t*)k.take(72 * B);
    I.blinder_out = (uint8_t*)k.take(32 * B), I.st = (int32_t*)k.take(4 * B), I.ctx = (uint8_t*)k.take(32 * B);
    I.ids = rings ? (uint32_t*)k.take(4 * B) : nullptr, I.off = rings ? (uint64_t*)k.take(8 * (B + 1)) : nullptr;
    return k.off + ZK_LAYOUT_TAIL;
}
static MemberProveArgs member_prove_staged(const MemberProveIn& I, const uint8_t* blinder, const zk_rng* rng, const uint8_t* blinder_out, const uint8_t* context, uint8_t* d_out) {
    return {I.which, blinder ? I.blinder : nullptr, {rng->mode, I.rng, rng->stride_blocks}, context ? I.ctx : nullptr, I.com, blinder_out ? I.blinder_out : nullptr, d_out, I.st};
}
// zk_member_prove_batch on the ring the context is bound to: the active one, or the one ring of a zk_member_prove_batch_rings call (RingBind).  The copies
// run on c->stream with one wait per direction (a call of one proof does not pay four blocking copies); from the first upload on, blinders and seeds lie in
// the input buffer, and every failing exit zeroes them.
static zk_status member_prove_host(zk_ctx* c, uint64_t B, bool bound, const uint32_t* which, const uint8_t* context, const uint8_t* blinder, const zk_rng* rng, uint8_t* com,
                                   uint8_t* blinder_out, uint8_t* out, uint64_t out_cap, int32_t* status) {
    if (!c || !rng || (bound && !context) || (B && (!which || !rng->data || !com || !out || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = member_refusal(c, bound)) return zs;
    if (!rng_mode_ok(rng)) return ZK_E_ARG;
    const uint64_t size = zkm1_size(c->ring->n);
    if (B > out_cap / size) {
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    if (B == 0) return ZK_OK;
    MemberProveIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return member_prove_in_layout(I, base, B, rng_bytes(rng, B), false); })) return zs;
    if (zk_status zs = reserve(c, B_io, B * size)) return zs;
    uint8_t* const d_out = (uint8_t*)c->buf[B_io].p;
    hipStream_t s = c->stream;
    hipError_t e = hipSuccess;   // the first error of the copies in flight
    auto copy = [&](void* dst, const void* src, size_t n, hipMemcpyKind kind) {
        if (e == hipSuccess && n) e = hipMemcpyAsync(dst, src, n, kind, s);
    };
    auto settle = [&]() -> zk_status {   // the copies have arrived; else the stream is drained (wipe_witness does not drain it) and the witness zeroed
        const hipError_t e_sync = hipStreamSynchronize(s);
        if (e == hipSuccess) e = e_sync;
        if (e != hipSuccess) wipe_witness(c);
        HIPCHK(c, e);
        return ZK_OK;
    };
    copy(I.which, which, 4 * B, hipMemcpyHostToDevice), copy(I.blinder, blinder, blinder ? 32 * B : 0, hipMemcpyHostToDevice);
    copy(I.rng, rng->data, rng_bytes(rng, B), hipMemcpyHostToDevice), copy(I.ctx, context, context ? 32 * B : 0, hipMemcpyHostToDevice);
    if (zk_status zs = settle()) return zs;   // the lanes' streams start behind the inputs
    if (zk_status zs = member_prove_device(c, B, member_prove_staged(I, blinder, rng, blinder_out, context, d_out), B * size)) {
        wipe_witness(c);   // (it drains what it started before it returns)
        return zs;
    }
    copy(out, d_out, B * size, hipMemcpyDeviceToHost), copy(com, I.com, 72 * B, hipMemcpyDeviceToHost);
    copy(blinder_out, I.blinder_out, blinder_out ? 32 * B : 0, hipMemcpyDeviceToHost), copy(status, I.st, 4 * B, hipMemcpyDeviceToHost);
    return settle();
}
extern "C" zk_status zk_member_prove_batch(zk_ctx* c, uint64_t B, const uint32_t* which, const uint8_t* blinder, const zk_rng* rng, uint8_t* com, uint8_t* blinder_out,
                                           uint8_t* out, uint64_t out_cap, int32_t* status) {
    return member_prove_host(c, B, false, which, nullptr, blinder, rng, com, blinder_out, out, out_cap, status);
}
extern "C" zk_status zk_member_prove_batch_bound(zk_ctx* c, uint64_t B, const uint32_t* which, const uint8_t* context, const uint8_t* blinder, const zk_rng* rng, uint8_t* com,
                                                 uint8_t* blinder_out, uint8_t* out, uint64_t out_cap, int32_t* status) {
    return member_prove_host(c, B, true, which, context, blinder, rng, com, blinder_out, out, out_cap, status);
}

// ------------------------------------------------------------------ verifier
// The device pointers of a verify call, or of one window of it (member_verify_window_args)
struct MemberVerifyArgs {
    const uint8_t *com, *proofs;
    const uint64_t* off;     // proof b starts at off[b] (a one-ring call without offsets of the caller's: member_verify_device makes them)
    const uint8_t* vseeds;   // nullptr: the engine's own (member_default_vseeds puts them here)
    const uint8_t* ctx;      // nullptr: the unbound call; else indexed like `com`
    uint8_t* ok;
    int32_t* status;
};
// The chunks of B proofs over the bound ring on the lanes, read in place through A.off: a one-ring call (proof first + p starts at off[first + p] and ends
// where the next one starts), or one window of a mixed-ring call (R.sel) -- com, off, vseeds and ctx are the window's gathered arrays, every slot is R.slot
// bytes long.  Every lane is drained before it returns.
static zk_status member_verify_run(zk_ctx* c, uint64_t B, const MemberVerifyArgs& A, const MemberRun& R) {
    const std::vector<ChunkPlan> plan = make_chunk_plan(B, R.C, 1, false);
    const uint32_t NL = (uint32_t)std::min<size_t>(c->lanes, plan.size());
    if (zk_status zs = ensure_member_lanes(c, R.C, NL)) return zs;
    if (R.ready)
        for (uint32_t l = 0; l < NL; l++) HIPCHK(c, hipStreamWaitEvent(c->pl[l].stream, R.ready, 0));
    for (uint64_t k = 0; k < plan.size(); k++) {
        const uint32_t lane = (uint32_t)(k % NL), cnt = plan[k].cnt;
        const uint64_t first = plan[k].first;
        auto& L = c->ml[lane];
        Workspace& W = L.W;
        VWork& V = L.V;
        V.com = A.com;
        V.gk_stmt = A.ctx ? GK_STMT_MEMBER : GK_STMT_NONE, V.ring_digest = c->ring->ring_digest;   // bound: "ZKMB" and its statement, else "ZKM1"
        hipStream_t s = c->pl[lane].stream;
        const uint32_t nq = (V.n + 1) / 2;
        {
            MaybeScope t(R.timed, c, "v_parse_validate", s);
            launch_mv_header_validate(s, V, cnt, A.proofs, A.off, first, R.slot);
        }
        {
            MaybeScope t(R.timed, c, "v_gk_total", s);
            launch_v_challenges(s, V, cnt, A.proofs, A.off, A.ctx, first, 2);
            launch_v_gk_total(s, V, W.ring, W.gk_etab, W.gk_kdig, cnt, W.N, A.proofs, A.off, first, L.res, L.res2);
            launch_v_proof_points(s, V, cnt, A.proofs, A.off, first, 1);
            launch_v_proof_terms(s, W, V, cnt, A.proofs, A.off, A.vseeds, first);
        }
        {
            MaybeScope t(R.timed, c, "v_sums", s);
            launch_v_straus(s, V.gk_terms, cnt * nq, V.C * nq, 4, 4, V.gk_acc, nullptr, nullptr);
            launch_v_straus(s, V.misc_terms, cnt, 3 * V.C, 1, 0, V.misc_acc, nullptr, nullptr);
            launch_tom_commit(s, c->P, W.lc, cnt, 1, 4 * W.n);
            launch_mv_final(s, W, V, cnt, A.ok, A.status, first, R.sel);
        }
    }
    HIPCHK(c, drain_lanes(c, NL));
    HIPCHK(c, hipGetLastError());
    return ZK_OK;
}
static zk_status member_default_vseeds(zk_ctx* c, uint64_t B, const uint8_t** d_vseeds) {   // the verifier's own seeds (api_verify.hip): fresh OS randomness per call
    if (*d_vseeds) return ZK_OK;
    if (zk_status zs = reserve(c, B_seed, 32 * B)) return zs;
    if (zk_status zs = make_default_vseeds(c, B, (uint8_t*)c->buf[B_seed].p, c->stream)) return zs;
    *d_vseeds = (const uint8_t*)c->buf[B_seed].p;
    return ZK_OK;
}
static zk_status member_verify_device(zk_ctx* c, uint64_t B, MemberVerifyArgs A) {   // (A.off: made here, the proofs are equally long)
    if (zk_status zs = member_refusal(c, A.ctx != nullptr)) return zs;
    timing_begin(c);
    if (B == 0) return ZK_OK;
    if (zk_status zs = reserve(c, B_m_off, 8 * (B + 1))) return zs;
    A.off = (const uint64_t*)c->buf[B_m_off].p;
    launch_mv_offsets(c->stream, (uint64_t*)c->buf[B_m_off].p, B, zkm1_size(c->ring->n));
    if (zk_status zs = member_default_vseeds(c, B, &A.vseeds)) return zs;
    HIPCHK(c, hipStreamSynchronize(c->stream));   // offsets and seeds are there before any lane reads them
    if (zk_status zs = member_verify_run(c, B, A, MemberRun{(uint32_t)std::min<uint64_t>(c->chunk, B), zk_timed(c, B)})) return zs;
    timing_end(c);
    return ZK_OK;
}
static zk_status member_verify_device_entry(zk_ctx* c, uint64_t B, bool bound, const MemberVerifyArgs& A) {
    if (!c || (bound && !A.ctx) || (B && (!A.com || !A.proofs || !A.ok || !A.status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return member_verify_device(c, B, A);
}
extern "C" zk_status zk_member_verify_batch_device(zk_ctx* c, uint64_t B, const void* d_com, const void* d_proofs, const void* d_vseeds, void* d_ok, void* d_status) {
    return member_verify_device_entry(c, B, false, {(const uint8_t*)d_com, (const uint8_t*)d_proofs, nullptr, (const uint8_t*)d_vseeds, nullptr, (uint8_t*)d_ok, (int32_t*)d_status});
}
extern "C" zk_status zk_member_verify_batch_bound_device(zk_ctx* c, uint64_t B, const void* d_com, const void* d_context, const void* d_proofs, const void* d_vseeds, void* d_ok,
                                                         void* d_status) {
    return member_verify_device_entry(c, B, true, {(const uint8_t*)d_com, (const uint8_t*)d_proofs, nullptr, (const uint8_t*)d_vseeds, (const uint8_t*)d_context, (uint8_t*)d_ok,
                                                   (int32_t*)d_status});
}
// Host pointers (`rings`: the _rings form, whose ids and offsets cross too).  No witness is staged: a failing copy returns as it is.
struct MemberVerifyIn {
    uint8_t *com, *seeds, *ok, *ctx;
    int32_t* st;
    uint32_t* ids;
    uint64_t* off;
};
static size_t member_verify_in_layout(MemberVerifyIn& I, uint8_t* base, size_t B, bool rings) {
    Carver k(base);
    I.com = (uint8_t*)k.take(72 * B), I.seeds = (uint8_t*)k.take(32 * B), I.ok = (uint8_t*)k.take(B), I.st = (int32_t*)k.take(4 * B), I.ctx = (uint8_t*)k.take(32 * B);
    I.ids = rings ? (uint32_t*)k.take(4 * B) : nullptr, I.off = rings ? (uint64_t*)k.take(8 * (B + 1)) : nullptr;
    return k.off + ZK_LAYOUT_TAIL;
}
static zk_status member_verify_host(zk_ctx* c, uint64_t B, bool bound, const uint8_t* com, const uint8_t* context, const uint8_t* proofs, const uint8_t* vseeds, uint8_t* ok,
                                    int32_t* status) {
    if (!c || (bound && !context) || (B && (!com || !proofs || !ok || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = member_refusal(c, bound)) return zs;
    if (B == 0) return ZK_OK;
    const uint64_t size = zkm1_size(c->ring->n);
    MemberVerifyIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return member_verify_in_layout(I, base, B, false); })) return zs;
    if (zk_status zs = reserve(c, B_io, B * size)) return zs;
    uint8_t* const d_proofs = (uint8_t*)c->buf[B_io].p;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(I.com, com, 72 * B, hipMemcpyHostToDevice, s));
    if (vseeds) HIPCHK(c, hipMemcpyAsync(I.seeds, vseeds, 32 * B, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_proofs, proofs, B * size, hipMemcpyHostToDevice, s));
    if (context) HIPCHK(c, hipMemcpyAsync(I.ctx, context, 32 * B, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (zk_status zs = member_verify_device(c, B, {I.com, d_proofs, nullptr, vseeds ? I.seeds : nullptr, context ? I.ctx : nullptr, I.ok, I.st})) return zs;
    HIPCHK(c, hipMemcpyAsync(ok, I.ok, B, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(status, I.st, 4 * B, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return ZK_OK;
}
extern "C" zk_status zk_member_verify_batch(zk_ctx* c, uint64_t B, const uint8_t* com, const uint8_t* proofs, const uint8_t* vseeds, uint8_t* ok, int32_t* status) {
    return member_verify_host(c, B, false, com, nullptr, proofs, vseeds, ok, status);
}
extern "C" zk_status zk_member_verify_batch_bound(zk_ctx* c, uint64_t B, const uint8_t* com, const uint8_t* context, const uint8_t* proofs, const uint8_t* vseeds, uint8_t* ok,
                                                  int32_t* status) {
    return member_verify_host(c, B, true, com, context, proofs, vseeds, ok, status);
}

// ------------------------------------------------------------------ one resident ring id per proof (include/zkattest.h: zk_member_*_batch_rings)
// The classing kernel (k_mr_class) classes every proof by its ring's slot -- the verifier's also by its slot's geometry -- and counts the classes per workgroup
// of MR_BLOCK proofs; the scan (partition.h) turns the counts into prefix sums over the workgroups, and the host reads the per-class totals and starts back
// ONCE.  A ZKM1 proof's size follows from its ring's n, so the prover's offsets exist before anything is proved (k_mr_offsets: the workgroup's prefix counts
// times the classes' sizes, then a scan inside the workgroup) and out_cap is decided there.
//   One resident ring and nothing else: the one-ring pipeline on the caller's buffers with that ring bound.  No permutation, no gather.
//   Otherwise, per ring, WINDOWS of at most 2 x chunk x lanes proofs through the stable permutation by class (k_part_perm): one gather collects the window's small
//   inputs into c->buf[B_mw] (whole stream rows in ZK_RNG_STREAM mode), the window runs with its ring bound (ensure_member_lanes re-binds, and re-carves only
//   when n or the tables change, and hands a bound call that ring's digest), and its writers put every proof, com, blinder, status and verdict at its final place through the window's `sel` list: no
//   staging buffer, no byte written twice.  The verifier reads the proof bytes in place through the window's gathered offsets.
//   A window's arguments are the call's with the gathered arrays in their places (member_*_window_args): an optional input the call does not have stays nullptr.
struct MemberCensus {
    uint8_t* cls;
    uint32_t *cnts, *perm;
};
static size_t member_census_layout(MemberCensus& X, uint8_t* base, uint64_t B, size_t ncnt) {
    Carver k(base);
    X.cls = (uint8_t*)k.take(B), X.cnts = (uint32_t*)k.take(4 * ncnt), X.perm = (uint32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
struct MemberProveWindow {
    uint32_t* which;
    uint8_t *blinder, *rng, *ctx;
};
static size_t member_prove_window_layout(MemberProveWindow& W, uint8_t* base, size_t Wp, size_t rng_row) {
    Carver k(base);
    W.which = (uint32_t*)k.take(4 * Wp), W.blinder = (uint8_t*)k.take(32 * Wp), W.rng = (uint8_t*)k.take(rng_row * Wp + 32), W.ctx = (uint8_t*)k.take(32 * Wp);
    return k.off + ZK_LAYOUT_TAIL;
}
static MemberProveArgs member_prove_window_args(const MemberProveArgs& A, const MemberProveWindow& W) {
    MemberProveArgs a = A;
    a.which = W.which, a.rng.data = W.rng;
    if (A.blinder) a.blinder = W.blinder;
    if (A.ctx) a.ctx = W.ctx;
    return a;
}
struct MemberVerifyWindow {
    uint64_t* off;
    uint8_t *com, *seeds, *ctx;
};
static size_t member_verify_window_layout(MemberVerifyWindow& W, uint8_t* base, size_t Wp) {
    Carver k(base);
    W.off = (uint64_t*)k.take(8 * Wp), W.com = (uint8_t*)k.take(72 * Wp), W.seeds = (uint8_t*)k.take(32 * Wp), W.ctx = (uint8_t*)k.take(32 * Wp);
    return k.off + ZK_LAYOUT_TAIL;
}
static MemberVerifyArgs member_verify_window_args(const MemberVerifyArgs& A, const MemberVerifyWindow& W) {
    MemberVerifyArgs a = A;
    a.com = W.com, a.off = W.off, a.vseeds = W.seeds;   // (the call's seeds are there, the caller's or the engine's own)
    if (A.ctx) a.ctx = W.ctx;
    return a;
}
static void member_rings(zk_ctx* c, MrRings& R, Ring** slot) {   // the resident rings in slot order, with their proofs' sizes
    RingSlots rs;
    ring_slots(c, rs, slot);
    mr_rings_clear(R);
    for (uint32_t r = 0; r < rs.count; r++) mr_rings_add(R, rs.id[r], slot[r]->n);
}
// classes, per-workgroup counts and their scan on the device; c->h_mr[0 .. MR_CLASSES) = proofs per class, [MR_CLASSES ..) = where each class starts in the permutation
static zk_status member_class(zk_ctx* c, uint64_t B, const uint32_t* d_ids, const MrRings& R, const uint64_t* d_proof_off, uint8_t* d_ok, int32_t* d_status, MemberCensus& X,
                              bool timed) {
    const uint64_t nblk = (B + MR_BLOCK - 1) / MR_BLOCK;
    const size_t ncnt = (size_t)(2 + nblk) * MR_CLASSES;
    if (zk_status zs = lay_out(c, B_mr, [&](uint8_t* base) { return member_census_layout(X, base, B, ncnt); })) return zs;
    if (!c->h_mr) HIPCHK(c, hipHostMalloc((void**)&c->h_mr, 4 * 2 * MR_CLASSES, hipHostMallocDefault));
    if (!c->mr_ready) HIPCHK(c, hipEventCreateWithFlags(&c->mr_ready, hipEventDisableTiming));
    {
        MaybeScope t(timed, c, "m_class", c->stream);
        launch_mr_class(c->stream, B, d_ids, R, d_proof_off, X.cls, X.cnts + 2 * MR_CLASSES, X.cnts, d_ok, d_status);
    }
    HIPCHK(c, hipMemcpyAsync(c->h_mr, X.cnts, 4 * 2 * MR_CLASSES, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ZK_OK;
}
static zk_status member_prove_rings_device(zk_ctx* c, uint64_t B, const MemberProveArgs& A, const uint32_t* d_ids, uint64_t out_cap, uint64_t* d_out_off) {
    if (zk_status zs = member_refusal(c, A.ctx != nullptr, false)) return zs;
    if (!rng_mode_ok(&A.rng)) return ZK_E_ARG;
    if (B > 0xffffffffull) return ZK_E_ARG;
    hipStream_t s = c->stream;
    timing_begin(c);
    if (B == 0) {
        HIPCHK(c, hipMemsetAsync(d_out_off, 0, 8, s));
        HIPCHK(c, hipStreamSynchronize(s));
        return ZK_OK;
    }
    MrRings R;
    Ring* slot[ZK_MAX_RINGS] = {};
    member_rings(c, R, slot);
    const bool timed = zk_timed(c, B);
    MemberCensus X;
    if (zk_status zs = member_class(c, B, d_ids, R, nullptr, nullptr, nullptr, X, timed)) return zs;
    const uint32_t *cnt = c->h_mr, *start = c->h_mr + MR_CLASSES;
    if (!mr_fits(mr_bytes(cnt, R), out_cap)) {   // before a byte of any output is written
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    {
        MaybeScope t(timed, c, "m_class", s);
        launch_mr_offsets(s, B, X.cls, X.cnts + 2 * MR_CLASSES, R, d_out_off, A.com, A.blinder_out, A.status);
    }
    zk_status zs = ZK_OK;
    hipError_t he = hipSuccess;
    const uint32_t one = mr_single_class(cnt, R);
    if (one < MR_CLASSES) {   // the common case: one ring -- the caller's buffers as they are
        RingBind rb(c, slot[one]);
        he = hipStreamSynchronize(s);
        if (he == hipSuccess) zs = member_prove_run(c, B, A, MemberRun{(uint32_t)std::min<uint64_t>(c->chunk, B), timed}, &he);
    } else {
        launch_mr_perm(s, B, X.cls, X.cnts + 2 * MR_CLASSES, X.cnts, X.perm);
        const uint32_t Wp = mr_window_cap(c->chunk, c->lanes, cnt, R), C = std::min<uint32_t>(c->chunk, Wp);
        const size_t rng_row = rng_bytes(&A.rng, 1);
        MemberProveWindow W{};
        zs = lay_out(c, B_mw, [&](uint8_t* base) { return member_prove_window_layout(W, base, Wp, rng_row); });
        const MemberProveArgs Aw = member_prove_window_args(A, W);
        for (uint32_t r = 0; r < R.count && !zs && he == hipSuccess; r++) {
            RingBind rb(c, slot[r]);
            for (uint32_t w = 0; w < mr_window_count(cnt[r], Wp) && !zs && he == hipSuccess; w++) {
                uint32_t first, n;
                mr_window(cnt[r], Wp, w, &first, &n);
                const uint32_t* sel = X.perm + start[r] + first;
                c->dbg_mr_windows++;
                {
                    MaybeScope t(timed, c, "m_gather", s);
                    launch_mr_pgather(s, n, B, sel, A.which, A.blinder, A.rng.mode == ZK_RNG_SEED ? A.rng.data : nullptr, A.ctx, W.which, W.blinder, W.rng, W.ctx);
                    if (A.rng.mode == ZK_RNG_STREAM) launch_pr_gather_rows(s, n, sel, A.rng.data, rng_row, W.rng);
                }
                if ((he = hipEventRecord(c->mr_ready, s)) != hipSuccess) break;
                zs = member_prove_run(c, n, Aw, MemberRun{C, timed, 0, MemberSel{sel, d_out_off, B}, c->mr_ready}, &he);
            }
        }
    }
    // nothing of this call may still be running (or writing into the caller's buffers) when it returns
    if (const hipError_t e = hipStreamSynchronize(s); he == hipSuccess) he = e;
    if (zs || he != hipSuccess) wipe_witness(c);   // a failed call leaves no gathered blinder, seed or stream row, no nonce and no RNG block behind
    if (zs) return zs;
    HIPCHK(c, he);
    HIPCHK(c, hipGetLastError());
    timing_end(c);
    return ZK_OK;
}
static Ring* member_resident(zk_ctx* c, uint32_t id) {
    for (auto& R : c->rings)
        if (R.live && R.id == id && R.N) return &R;
    return nullptr;
}
extern "C" uint64_t zk_member_proof_size_ring(const zk_ctx* c, uint32_t ring) {
    if (!c) return 0;
    const Ring* R = member_resident(const_cast<zk_ctx*>(c), ring);
    return R ? zkm1_size(R->n) : 0;
}
static zk_status member_prove_rings_device_entry(zk_ctx* c, uint64_t B, bool bound, const zk_rng* rng, MemberProveArgs A, const uint32_t* d_ids, uint64_t out_cap,
                                                 uint64_t* d_out_off) {
    if (!c || !rng || (bound && !A.ctx) || !d_out_off || (B && (!A.which || !d_ids || !rng->data || !A.com || !A.out || !A.status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    A.rng = *rng;
    return member_prove_rings_device(c, B, A, d_ids, out_cap, d_out_off);
}
extern "C" zk_status zk_member_prove_batch_rings_device(zk_ctx* c, uint64_t B, const void* d_which, const void* d_ids, const void* d_blinder, const zk_rng* rng, void* d_com,
                                                        void* d_blinder_out, void* d_out, uint64_t out_cap, void* d_out_off, void* d_status) {
    return member_prove_rings_device_entry(c, B, false, rng, {(const uint32_t*)d_which, (const uint8_t*)d_blinder, {}, nullptr, (uint8_t*)d_com, (uint8_t*)d_blinder_out,
                                                              (uint8_t*)d_out, (int32_t*)d_status}, (const uint32_t*)d_ids, out_cap, (uint64_t*)d_out_off);
}
extern "C" zk_status zk_member_prove_batch_rings_bound_device(zk_ctx* c, uint64_t B, const void* d_which, const void* d_context, const void* d_ids, const void* d_blinder,
                                                              const zk_rng* rng, void* d_com, void* d_blinder_out, void* d_out, uint64_t out_cap, void* d_out_off, void* d_status) {
    return member_prove_rings_device_entry(c, B, true, rng, {(const uint32_t*)d_which, (const uint8_t*)d_blinder, {}, (const uint8_t*)d_context, (uint8_t*)d_com,
                                                             (uint8_t*)d_blinder_out, (uint8_t*)d_out, (int32_t*)d_status}, (const uint32_t*)d_ids, out_cap, (uint64_t*)d_out_off);
}
// Host pointers: the ids are classed here, and with them the offsets and the out_cap decision.  All of one resident ring: zk_member_prove_batch with that ring
// bound.  Anything else: the inputs cross to HBM and take the device path; the proofs lie in order in the context's staging copy of `out` and cross the link in
// one copy.
static zk_status member_prove_rings_host(zk_ctx* c, uint64_t B, bool bound, const uint32_t* which, const uint8_t* context, const uint32_t* ring_ids, const uint8_t* blinder,
                                         const zk_rng* rng, uint8_t* com, uint8_t* blinder_out, uint8_t* out, uint64_t out_cap, uint64_t* out_off, int32_t* status) {
    if (!c || !rng || (bound && !context) || !out_off || (B && (!which || !ring_ids || !rng->data || !com || !out || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = member_refusal(c, bound, false)) return zs;
    if (!rng_mode_ok(rng)) return ZK_E_ARG;
    if (B > 0xffffffffull) return ZK_E_ARG;
    if (B == 0) {
        out_off[0] = 0;
        return ZK_OK;
    }
    MrRings R;
    Ring* slot[ZK_MAX_RINGS] = {};
    member_rings(c, R, slot);
    uint32_t cnt[MR_CLASSES];
    std::vector<uint64_t> off(B + 1);
    mr_plan_host(R, B, ring_ids, nullptr, cnt, off.data());
    const uint64_t total = off[B];
    if (!mr_fits(total, out_cap)) {   // before a byte of any output is written
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    const uint32_t one = mr_single_class(cnt, R);
    if (one < MR_CLASSES) {
        RingBind rb(c, slot[one]);
        if (zk_status zs = member_prove_host(c, B, bound, which, context, blinder, rng, com, blinder_out, out, total, status)) return zs;
        memcpy(out_off, off.data(), 8 * (B + 1));
        return ZK_OK;
    }
    MemberProveIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return member_prove_in_layout(I, base, B, rng_bytes(rng, B), true); })) return zs;
    if (zk_status zs = reserve(c, B_io, total ? total : 32)) return zs;
    uint8_t* const d_out = (uint8_t*)c->buf[B_io].p;
    // from the first upload on, blinders and seeds lie in the input buffer: every failure below zeroes them (member_prove_rings_device does so itself)
    if (zk_status zs = upload_or_wipe(c, {{I.which, which, 4 * B}, {I.ids, ring_ids, 4 * B}, {I.blinder, blinder, blinder ? 32 * B : 0}, {I.rng, rng->data, rng_bytes(rng, B)},
                                          {I.ctx, context, context ? 32 * B : 0}}))
        return zs;
    if (zk_status zs = member_prove_rings_device(c, B, member_prove_staged(I, blinder, rng, blinder_out, context, d_out), I.ids, total, I.off)) return zs;
    return download_or_wipe(c, {{d_out, out, total}, {I.com, com, 72 * B}, {I.blinder_out, blinder_out, blinder_out ? 32 * B : 0}, {I.st, status, 4 * B},
                                {I.off, out_off, 8 * (B + 1)}});
}
extern "C" zk_status zk_member_prove_batch_rings(zk_ctx* c, uint64_t B, const uint32_t* which, const uint32_t* ring_ids, const uint8_t* blinder, const zk_rng* rng, uint8_t* com,
                                                 uint8_t* blinder_out, uint8_t* out, uint64_t out_cap, uint64_t* out_off, int32_t* status) {
    return member_prove_rings_host(c, B, false, which, nullptr, ring_ids, blinder, rng, com, blinder_out, out, out_cap, out_off, status);
}
extern "C" zk_status zk_member_prove_batch_rings_bound(zk_ctx* c, uint64_t B, const uint32_t* which, const uint8_t* context, const uint32_t* ring_ids, const uint8_t* blinder,
                                                       const zk_rng* rng, uint8_t* com, uint8_t* blinder_out, uint8_t* out, uint64_t out_cap, uint64_t* out_off, int32_t* status) {
    return member_prove_rings_host(c, B, true, which, context, ring_ids, blinder, rng, com, blinder_out, out, out_cap, out_off, status);
}

static zk_status member_verify_rings_device(zk_ctx* c, uint64_t B, MemberVerifyArgs A, const uint32_t* d_ids) {
    if (zk_status zs = member_refusal(c, A.ctx != nullptr, false)) return zs;
    if (B > 0xffffffffull || ((uintptr_t)A.proofs & 3)) return ZK_E_ARG;
    timing_begin(c);
    if (B == 0) return ZK_OK;
    hipStream_t s = c->stream;
    MrRings R;
    Ring* slot[ZK_MAX_RINGS] = {};
    member_rings(c, R, slot);
    const bool timed = zk_timed(c, B);
    if (zk_status zs = member_default_vseeds(c, B, &A.vseeds)) return zs;
    MemberCensus X;
    if (zk_status zs = member_class(c, B, d_ids, R, A.off, A.ok, A.status, X, timed)) return zs;   // (the seeds are there too when it returns)
    const uint32_t *cnt = c->h_mr, *start = c->h_mr + MR_CLASSES;
    const uint32_t one = mr_single_class(cnt, R);
    if (one < MR_CLASSES) {   // one ring, every slot as long as its proofs: the caller's buffers and offsets as they are
        RingBind rb(c, slot[one]);
        if (zk_status zs = member_verify_run(c, B, A, MemberRun{(uint32_t)std::min<uint64_t>(c->chunk, B), timed})) return zs;
    } else {
        launch_mr_perm(s, B, X.cls, X.cnts + 2 * MR_CLASSES, X.cnts, X.perm);
        const uint32_t Wp = mr_window_cap(c->chunk, c->lanes, cnt, R), C = std::min<uint32_t>(c->chunk, Wp);
        MemberVerifyWindow W;
        if (zk_status zs = lay_out(c, B_mw, [&](uint8_t* base) { return member_verify_window_layout(W, base, Wp); })) return zs;
        const MemberVerifyArgs Aw = member_verify_window_args(A, W);
        for (uint32_t r = 0; r < R.count; r++) {
            RingBind rb(c, slot[r]);
            for (uint32_t w = 0; w < mr_window_count(cnt[r], Wp); w++) {
                uint32_t first, n;
                mr_window(cnt[r], Wp, w, &first, &n);
                const uint32_t* sel = X.perm + start[r] + first;
                c->dbg_mr_windows++;
                {
                    MaybeScope t(timed, c, "m_gather", s);
                    launch_mr_vgather(s, n, B, sel, A.off, A.com, A.vseeds, A.ctx, W.off, W.com, W.seeds, W.ctx);
                }
                HIPCHK(c, hipEventRecord(c->mr_ready, s));
                if (zk_status zs = member_verify_run(c, n, Aw, MemberRun{C, timed, R.size[r], MemberSel{sel, nullptr, B}, c->mr_ready})) return zs;
            }
        }
    }
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    timing_end(c);
    return ZK_OK;
}
static zk_status member_verify_rings_device_entry(zk_ctx* c, uint64_t B, bool bound, const MemberVerifyArgs& A, const uint32_t* d_ids) {
    if (!c || (bound && !A.ctx) || (B && (!A.com || !A.proofs || !A.off || !d_ids || !A.ok || !A.status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return member_verify_rings_device(c, B, A, d_ids);
}
extern "C" zk_status zk_member_verify_batch_rings_device(zk_ctx* c, uint64_t B, const void* d_com, const void* d_proofs, const void* d_proof_off, const void* d_ids,
                                                         const void* d_vseeds, void* d_ok, void* d_status) {
    return member_verify_rings_device_entry(c, B, false, {(const uint8_t*)d_com, (const uint8_t*)d_proofs, (const uint64_t*)d_proof_off, (const uint8_t*)d_vseeds, nullptr, (uint8_t*)d_ok,
                                                    (int32_t*)d_status}, (const uint32_t*)d_ids);
}
extern "C" zk_status zk_member_verify_batch_rings_bound_device(zk_ctx* c, uint64_t B, const void* d_com, const void* d_context, const void* d_proofs, const void* d_proof_off,
                                                               const void* d_ids, const void* d_vseeds, void* d_ok, void* d_status) {
    return member_verify_rings_device_entry(c, B, true, {(const uint8_t*)d_com, (const uint8_t*)d_proofs, (const uint64_t*)d_proof_off, (const uint8_t*)d_vseeds,
                                                   (const uint8_t*)d_context, (uint8_t*)d_ok, (int32_t*)d_status}, (const uint32_t*)d_ids);
}
// Host pointers: classed here as the classing kernel does.  One resident ring and every slot in order: zk_member_verify_batch on the bytes from the first slot
// on, with that ring bound.  Anything else: everything crosses to HBM and takes the device path (which classes again; bytes behind proof_off[B] do not cross).
static zk_status member_verify_rings_host(zk_ctx* c, uint64_t B, bool bound, const uint8_t* com, const uint8_t* context, const uint8_t* proofs, const uint64_t* proof_off,
                                          const uint32_t* ring_ids, const uint8_t* vseeds, uint8_t* ok, int32_t* status) {
    if (!c || (bound && !context) || (B && (!com || !proofs || !proof_off || !ring_ids || !ok || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = member_refusal(c, bound, false)) return zs;
    if (B > 0xffffffffull) return ZK_E_ARG;
    if (B == 0) return ZK_OK;
    MrRings R;
    Ring* slot[ZK_MAX_RINGS] = {};
    member_rings(c, R, slot);
    uint32_t cnt[MR_CLASSES] = {};
    for (uint64_t b = 0; b < B; b++) {
        uint32_t k = mr_class_of_id(R, ring_ids[b]);
        if (k < MR_SLOTS && !mr_slot_ok(proof_off[b], proof_off[b + 1], proof_off[B], R.size[k])) k = MR_BAD;
        cnt[k]++;
    }
    const uint32_t one = mr_single_class(cnt, R);
    if (one < MR_CLASSES) {
        RingBind rb(c, slot[one]);
        return member_verify_host(c, B, bound, com, context, proofs + proof_off[0], vseeds, ok, status);
    }
    const uint64_t bytes = proof_off[B];
    MemberVerifyIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return member_verify_in_layout(I, base, B, true); })) return zs;
    if (zk_status zs = reserve(c, B_io, bytes ? bytes : 32)) return zs;
    uint8_t* const d_proofs = (uint8_t*)c->buf[B_io].p;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemcpyAsync(I.com, com, 72 * B, hipMemcpyHostToDevice, s));
    if (vseeds) HIPCHK(c, hipMemcpyAsync(I.seeds, vseeds, 32 * B, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(I.ids, ring_ids, 4 * B, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(I.off, proof_off, 8 * (B + 1), hipMemcpyHostToDevice, s));
    if (bytes) HIPCHK(c, hipMemcpyAsync(d_proofs, proofs, bytes, hipMemcpyHostToDevice, s));
    if (context) HIPCHK(c, hipMemcpyAsync(I.ctx, context, 32 * B, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (zk_status zs = member_verify_rings_device(c, B, {I.com, d_proofs, I.off, vseeds ? I.seeds : nullptr, context ? I.ctx : nullptr, I.ok, I.st}, I.ids)) return zs;
    HIPCHK(c, hipMemcpyAsync(ok, I.ok, B, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(status, I.st, 4 * B, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return ZK_OK;
}
extern "C" zk_status zk_member_verify_batch_rings(zk_ctx* c, uint64_t B, const uint8_t* com, const uint8_t* proofs, const uint64_t* proof_off, const uint32_t* ring_ids,
                                                  const uint8_t* vseeds, uint8_t* ok, int32_t* status) {
    return member_verify_rings_host(c, B, false, com, nullptr, proofs, proof_off, ring_ids, vseeds, ok, status);
}
extern "C" zk_status zk_member_verify_batch_rings_bound(zk_ctx* c, uint64_t B, const uint8_t* com, const uint8_t* context, const uint8_t* proofs, const uint64_t* proof_off,
                                                        const uint32_t* ring_ids, const uint8_t* vseeds, uint8_t* ok, int32_t* status) {
    return member_verify_rings_host(c, B, true, com, context, proofs, proof_off, ring_ids, vseeds, ok, status);
}
