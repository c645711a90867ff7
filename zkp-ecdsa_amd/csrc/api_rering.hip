// zk_proof_rering_batch / zk_prove_key_blinders (include/zkattest.h): a ZKA1 proof moved to the active ring -- its GKProof section replaced by the one
// zk_member_prove_batch makes for (which_new, keyXcom's blinder), every other byte kept.  Host-side pipeline: the member lanes of api_member.hip run their
// kernels unchanged on a view of their workspace whose writers point into the ZKA1 proofs; the kernels of its own are in k_rering.hip.
#include "ctx.h"
#include "jobs.h"
#include "member.h"
#include "rering.h"

// ------------------------------------------------------------------ the blinder of keyXcom
// Logical draw 1 of every proof under the randomness contract (draw 0 is comS1's, mod n; draw 1 mod q): the prepass and the draw mapping behind
// zk_test_rng_draws on the caller's device buffers, in chunks of KB_CHUNK proofs on one scratch buffer of the context (the rejection lists are derived from
// the seeds: it is witness-flagged and wiped with the rest).  A proof whose stream does not hold the draw gets 32 zero bytes and the call ZK_E_RNG_EXHAUSTED.
#define KB_CHUNK (1u << 18)
static zk_status key_blinders_device(zk_ctx* c, uint64_t B, const zk_rng& rng, uint8_t* d_out) {   // (rng.data: a device pointer)
    if (!c->params_set) return ZK_E_BUFFER;
    if (c->stream_busy) return busy_refusal(c);
    if (!rng_mode_ok(&rng) || B > 0xffffffffull) return ZK_E_ARG;
    if (B == 0) return ZK_OK;
    if (zk_status zs = reserve(c, B_kb, 4 * (size_t)KB_CHUNK * (2 * RNG_MAX_EXC + 1) + 256)) return zs;
    uint32_t* const flag = (uint32_t*)c->buf[B_kb].p;
    hipStream_t s = c->stream;
    HIPCHK(c, hipMemsetAsync(flag, 0, 4, s));
    Workspace W{};
    W.sec = c->P.sec;
    W.rng.seeds = rng.data, W.rng.stream = rng.data, W.rng.stride_blocks = rng.stride_blocks, W.rng.mode = rng.mode, W.rng.sec = (int)c->P.sec;
    W.rng.exc_idx = flag + 64, W.rng.exc_flags = W.rng.exc_idx + RNG_MAX_EXC * (size_t)KB_CHUNK, W.rng.exc_cnt = W.rng.exc_flags + RNG_MAX_EXC * (size_t)KB_CHUNK;
    for (uint64_t first = 0; first < B; first += KB_CHUNK) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(KB_CHUNK, B - first);
        W.rng.proof_base = (uint32_t)first;
        launch_rng_prepass(s, W, cnt, 0, 2 + RNG_MAX_EXC, 0, nullptr, false);
        launch_rr_blinders(s, W.rng, cnt, first, d_out, flag);
    }
    uint32_t exhausted = 0;
    HIPCHK(c, hipMemcpyAsync(&exhausted, flag, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    if (exhausted) {
        c->err = "a proof's RNG stream does not hold its draw 1 (its blinder is written as zeros)";
        return ZK_E_RNG_EXHAUSTED;
    }
    return ZK_OK;
}
extern "C" zk_status zk_prove_key_blinders_device(zk_ctx* c, uint64_t B, const zk_rng* rng, void* d_blinder) {
    if (!c || !rng || (B && (!rng->data || !d_blinder))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return key_blinders_device(c, B, *rng, (uint8_t*)d_blinder);
}
struct KeyBlindersIn {
    uint8_t *rng, *out;
};
static size_t key_blinders_in_layout(KeyBlindersIn& I, uint8_t* base, size_t B, size_t rng_bytes) {
    Carver k(base);
    I.rng = (uint8_t*)k.take(rng_bytes ? rng_bytes : 32), I.out = (uint8_t*)k.take(32 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_prove_key_blinders(zk_ctx* c, uint64_t B, const zk_rng* rng, uint8_t* blinder) {
    if (!c || !rng || (B && (!rng->data || !blinder))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->params_set) return ZK_E_BUFFER;
    if (c->stream_busy) return busy_refusal(c);
    if (!rng_mode_ok(rng)) return ZK_E_ARG;
    if (B == 0) return ZK_OK;
    KeyBlindersIn I;   // seeds and blinders lie in the witness-flagged input buffer: every failure below zeroes them
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return key_blinders_in_layout(I, base, B, rng_bytes(rng, B)); })) return zs;
    if (zk_status zs = upload_or_wipe(c, {{I.rng, rng->data, rng_bytes(rng, B)}})) return zs;
    if (zk_status zs = key_blinders_device(c, B, zk_rng{rng->mode, I.rng, rng->stride_blocks}, I.out)) {
        wipe_witness(c);
        return zs;
    }
    return download_or_wipe(c, {{I.out, blinder, 32 * B}});
}

// ------------------------------------------------------------------ re-ring
static zk_status rering_refusal(zk_ctx* c) {
    if (!c->params_set || !c->ring->N) return ZK_E_BUFFER;
    if (c->stream_busy) return busy_refusal(c);
    return ZK_OK;
}
struct RrBufs {
    unsigned long long* cnt;
    RrLane lane[ZK_MAX_LANES];
};
static size_t rering_layout(RrBufs& R, uint8_t* base, uint32_t C, uint32_t nlanes) {
    SoaCarver k(base);
    R.cnt = (unsigned long long*)k.take(8 * RR_CENSUS_WORDS);
    for (uint32_t l = 0; l < nlanes; l++) {
        RrLane& X = R.lane[l];
        X.kx = (uint32_t*)k.take(4 * 18 * (size_t)C), X.head = (uint32_t*)k.take(4 * (size_t)C), X.flags = (uint32_t*)k.take(4 * (size_t)C);
        X.len = (uint64_t*)k.take(8 * (size_t)C);
        X.Rx = k.soa(C), X.Ry = k.soa(C), X.kax = k.soa(2 * (size_t)C), X.kay = k.soa(2 * (size_t)C);
    }
    return k.off + ZK_LAYOUT_TAIL;
}
// Every pointer in this context's HBM.  The census (one kernel, ONE read-back) decides the call before a byte of any output is written: ZK_E_BUFFER against
// the bytes of the proofs that can still succeed -- sound header, index inside the ring --, which is what the output holds when no proof fails its opening
// or its RNG stream; in place (d_out == d_proofs), ZK_E_ARG where a well-formed proof has another n than the ring.
// Then the chunks on the lanes.  Per chunk: the RNG prepass, the front end, the member prover's fold and commitments with the claimed opening as one more
// slot, the comparison (final statuses, new lengths), the offsets -- a chunk's proofs start where the chunk before ended, so its scan waits for that chunk's,
// and for nothing else of it --, the challenge hash, then the heads' mover and the member prover's writers, into disjoint bytes.
static zk_status rering_device(zk_ctx* c, uint64_t B, const uint8_t* d_msg, const uint8_t* d_proofs, const uint64_t* d_off, const uint32_t* d_which, const uint8_t* d_blinder,
                               const zk_rng& rng, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off, int32_t* d_status) {   // (rng.data: a device pointer)
    if (zk_status zs = rering_refusal(c)) return zs;
    if (!rng_mode_ok(&rng) || B > 0xffffffffull || ((uintptr_t)d_proofs & 3) || ((uintptr_t)d_out & 3)) return ZK_E_ARG;
    hipStream_t s0 = c->stream;
    timing_begin(c);
    if (B == 0) {
        HIPCHK(c, hipMemsetAsync(d_out_off, 0, 8, s0));
        HIPCHK(c, hipStreamSynchronize(s0));
        return ZK_OK;
    }
    const bool in_place = d_out == d_proofs, timed = zk_timed(c, B), full = c->mode == ZK_MODE_HARDENED;
    const uint32_t n = c->ring->n, C = (uint32_t)std::min<uint64_t>(c->chunk, B);
    Wire wire = wire_make(c->wire != 0);
    const std::vector<ChunkPlan> plan = make_chunk_plan(B, C, 1, false);
    const uint32_t NL = (uint32_t)std::min<size_t>(c->lanes, plan.size());
    if (zk_status zs = ensure_member_lanes(c, C, NL)) return zs;
    RrBufs R;
    if (zk_status zs = lay_out(c, B_rr, [&](uint8_t* base) { return rering_layout(R, base, C, NL); })) return zs;
    if (!c->h_rr) HIPCHK(c, hipHostMalloc((void**)&c->h_rr, 8 * RR_CENSUS_WORDS, hipHostMallocDefault));
    for (uint32_t l = 0; l < NL; l++)
        if (!c->rr_scan[l]) HIPCHK(c, hipEventCreateWithFlags(&c->rr_scan[l], hipEventDisableTiming));
    {
        MaybeScope t(timed, c, "rr_census", s0);
        launch_rr_census(s0, B, d_proofs, d_off, d_which, wire, n, (uint32_t)c->ring->N, R.cnt);
    }
    HIPCHK(c, hipMemcpyAsync(c->h_rr, R.cnt, 8 * RR_CENSUS_WORDS, hipMemcpyDeviceToHost, s0));
    HIPCHK(c, hipStreamSynchronize(s0));
    if (in_place && c->h_rr[1]) {
        c->err = "in place: a well-formed proof's n is not the active ring's (its GKProof section changes size)";
        return ZK_E_ARG;
    }
    if (!in_place && d_out < d_proofs + c->h_rr[2] && d_proofs < d_out + c->h_rr[0]) {
        c->err = "out overlaps proofs (only out == proofs is supported: the in-place form)";
        return ZK_E_ARG;
    }
    if ((in_place ? c->h_rr[2] : c->h_rr[0]) > out_cap) {
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    // the lanes' view of their member workspace: writers at the proof's own place (out_base[p] = start of its GKProof section), the wire's coordinates
    wire.fixed = 0, wire.rep_head = 0, wire.padd = 0;
    hipError_t he = hipSuccess;
    for (uint64_t k = 0; k < plan.size() && he == hipSuccess; k++) {
        const uint32_t lane = (uint32_t)(k % NL), cnt = plan[k].cnt;
        const uint64_t first = plan[k].first;
        auto& L = c->ml[lane];
        const RrLane& X = R.lane[lane];
        hipStream_t s = c->pl[lane].stream;
        Workspace W = L.W;
        W.gk_fill0 = 0;   // the caller-blinder contract of zk_member_prove_batch: the 5 n draws start at fill 0
        W.gk_stmt = full ? GK_STMT_FULL : GK_STMT_NONE, W.ring_digest = c->ring->ring_digest, W.wire = wire_make(c->wire != 0);
        W.Rx = X.Rx, W.Ry = X.Ry, W.la.ax = X.kax, W.la.ay = X.kay;
        member_chunk_rng(c, timed, s, W, rng, first, cnt);
        const ChunkIn in = member_chunk_commit(c, timed, s, W, L, cnt, [&] { launch_rr_front(s, W, X, cnt, first, d_proofs, d_off, d_which, d_blinder, L.which_s); });
        {
            MaybeScope t(timed, c, "rr_offsets", s);
            launch_rr_compare(s, W, X, cnt, first, d_status);
            if (in_place) launch_rr_place(s, W, X, cnt, first, B, d_off, d_out_off);
            else {
                if (k && NL > 1 && (he = hipStreamWaitEvent(s, c->rr_scan[(k - 1) % NL], 0)) != hipSuccess) break;
                launch_rr_scan(s, W, X, cnt, first, d_out_off);
                if (NL > 1 && (he = hipEventRecord(c->rr_scan[lane], s)) != hipSuccess) break;
            }
        }
        {
            MaybeScope t(timed, c, "hash", s);
            Workspace H = W;   // the full statement's keyXcom lies in list A at slot p (2 + 2 sec): sec = 0 here; the small-call hash path is sized by sec and stays out
            if (full) H.sec = 0;
            launch_gk_hash(s, H, cnt, full ? d_msg + 32 * first : nullptr);
        }
        W.wire = wire;
        if (!in_place) {
            MaybeScope t(timed, c, "rr_move", s);
            launch_rr_move(s, X, cnt, first, d_proofs, d_off, d_out_off, n, d_out);
        }
        {
            MaybeScope t(timed, c, "respond_write", s);
            launch_gk_respond(s, W, in, d_out);
        }
    }
    if (const hipError_t e = drain_lanes(c, NL); he == hipSuccess) he = e;
    if (he != hipSuccess) wipe_witness(c);   // a failed call leaves no blinder, nonce or RNG block behind
    HIPCHK(c, he);
    HIPCHK(c, hipGetLastError());
    timing_end(c);
    return ZK_OK;
}
extern "C" zk_status zk_proof_rering_batch_device(zk_ctx* c, uint64_t B, const void* d_msg, const void* d_proofs, const void* d_off, const void* d_which, const void* d_blinder,
                                                  const zk_rng* rng, void* d_out, uint64_t out_cap, void* d_out_off, void* d_status) {
    if (!c || !rng || !d_out_off || (B && (!d_msg || !d_proofs || !d_off || !d_which || !d_blinder || !rng->data || !d_out || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return rering_device(c, B, (const uint8_t*)d_msg, (const uint8_t*)d_proofs, (const uint64_t*)d_off, (const uint32_t*)d_which, (const uint8_t*)d_blinder, *rng,
                         (uint8_t*)d_out, out_cap, (uint64_t*)d_out_off, (int32_t*)d_status);
}
// Host pointers: the batch is staged in HBM -- the small arrays in the context's input buffer (blinders and seeds: wiped with it), the proofs in its staging
// buffers -- and takes the device path.  The headers are read here first, so out_cap is decided (by the census' rule) and the output staged at its size.
struct RrIn {
    uint8_t *msg, *blinder, *rng;
    uint32_t* which;
    uint64_t *off, *out_off;
    int32_t* st;
};
static size_t rering_in_layout(RrIn& I, uint8_t* base, size_t B, size_t rng_bytes) {
    Carver k(base);
    I.msg = (uint8_t*)k.take(32 * B), I.blinder = (uint8_t*)k.take(32 * B), I.rng = (uint8_t*)k.take(rng_bytes ? rng_bytes : 32), I.which = (uint32_t*)k.take(4 * B);
    I.off = (uint64_t*)k.take(8 * (B + 1)), I.out_off = (uint64_t*)k.take(8 * (B + 1)), I.st = (int32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_proof_rering_batch(zk_ctx* c, uint64_t B, const uint8_t* msg, const uint8_t* proofs, const uint64_t* off, const uint32_t* which, const uint8_t* blinder,
                                           const zk_rng* rng, uint8_t* out, uint64_t out_cap, uint64_t* out_off, int32_t* status) {
    if (!c || !rng || !out_off || !off || (B && (!msg || !proofs || !which || !blinder || !rng->data || !out || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = rering_refusal(c)) return zs;
    if (!rng_mode_ok(rng) || B > 0xffffffffull) return ZK_E_ARG;
    if (B == 0) {
        out_off[0] = 0;
        return ZK_OK;
    }
    const Wire wire = wire_make(c->wire != 0);
    const uint64_t N = c->ring->N, gk_new = (uint64_t)wire.gk_n * c->ring->n + 32;
    const bool in_place = out == proofs;   // the in-place rules hold here too: the staged copy is re-ringed in place and comes back as a whole
    uint64_t need = 0, in_bytes = 0;   // what the proofs that can still succeed need, and the bytes of the slots that are read at all
    for (uint64_t b = 0; b < B; b++) {
        if (rr_slot_readable(off[b], off[b + 1])) in_bytes = std::max(in_bytes, off[b + 1]);
        const RrHead h = rr_head(proofs, off[b], off[b + 1], wire);
        if (h.ok && which[b] < N) need += h.head + gk_new;
    }
    if (in_place) need = in_bytes = off[B];
    if (need > out_cap) {
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    RrIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return rering_in_layout(I, base, B, rng_bytes(rng, B)); })) return zs;
    if (zk_status zs = reserve(c, B_io, in_bytes + 32)) return zs;
    if (!in_place)
        if (zk_status zs = reserve(c, B_ro, need + 32)) return zs;
    uint8_t *const d_proofs = (uint8_t*)c->buf[B_io].p, *const d_out = in_place ? d_proofs : (uint8_t*)c->buf[B_ro].p;
    // from the first upload on, blinders and seeds lie in the input buffer: every failure below zeroes them
    if (zk_status zs = upload_or_wipe(c, {{I.msg, msg, 32 * B}, {I.blinder, blinder, 32 * B}, {I.rng, rng->data, rng_bytes(rng, B)}, {I.which, which, 4 * B},
                                          {I.off, off, 8 * (B + 1)}, {d_proofs, proofs, in_bytes}}))
        return zs;
    if (zk_status zs = rering_device(c, B, I.msg, d_proofs, I.off, I.which, I.blinder, zk_rng{rng->mode, I.rng, rng->stride_blocks}, d_out, need, I.out_off, I.st)) {
        wipe_witness(c);
        return zs;
    }
    if (zk_status zs = download_or_wipe(c, {{I.out_off, out_off, 8 * (B + 1)}, {I.st, status, 4 * B}})) return zs;
    return download_or_wipe(c, {{d_out, out, in_place ? need : out_off[B]}});   // (out_off[B] has arrived)
}

// ------------------------------------------------------------------ one destination ring id per proof (include/zkattest.h: zk_proof_rering_batch_rings)
// The census classes every proof against ITS ring and measures its slot from the header (rering_plan.h: rules 1-3), counts per workgroup, and the host reads
// the totals back ONCE: with them every decision of the call is made -- exact, since a proof that later fails its opening or its RNG stream keeps its slot --
// and every proof's place is known before anything is proved (k_rrr_offsets).  All heads move in ONE launch over [0, out_off[B]) on the call's stream, behind
// the first window's gather: the layout depends on no window, the windows' writers touch other bytes, so lanes above 0 prove beside it (lane 0 shares the
// call's stream and starts behind it; a per-window mover would put the same bytes in front of every window's lane 0 instead).
//   One resident ring and no refusal: the chunk pipeline on the caller's arrays with that ring bound.  No permutation, no gather.
//   Otherwise, per ring, WINDOWS of at most 2 x chunk x lanes proofs through the stable permutation by class: the member prover's gather collects the window's
//   indices, blinders, seeds (whole stream rows in ZK_RNG_STREAM mode) and, in hardened mode, message hashes into c->buf[B_mw]; the window runs with its ring
//   bound and puts statuses and GKProof sections at their final places through the window's `sel` list.
// Behind the windows one kernel zero-fills the slots of the proofs that failed there.  No scan between chunks, no event between lanes.
static zk_status rering_rings_refusal(zk_ctx* c) {   // (no active ring is read)
    if (!c->params_set) return ZK_E_BUFFER;
    if (c->stream_busy) return busy_refusal(c);
    return ZK_OK;
}
static void rering_ring_table(zk_ctx* c, RrRings& R, Ring** slot) {   // the resident rings in slot order
    RingSlots rs;
    ring_slots(c, rs, slot);
    rrr_rings_clear(R);
    for (uint32_t r = 0; r < rs.count; r++) rrr_rings_add(R, rs.id[r], slot[r]->n, slot[r]->N);
}
static size_t rering_census_layout(RrCensus& X, uint8_t* base, uint64_t B) {
    Carver k(base);
    const size_t nblk = (size_t)((B + MR_BLOCK - 1) / MR_BLOCK);
    uint8_t* const head = (uint8_t*)k.take(RRR_READBACK);
    X.cnt = (uint64_t*)head, X.cls_tot = head ? (uint32_t*)(head + RRR_HEAD_BYTES) : nullptr;
    X.blk_bytes = (uint64_t*)k.take(8 * (nblk + 1)), X.blk_other = (uint64_t*)k.take(8 * nblk), X.blk_cnt = (uint32_t*)k.take(4 * nblk * MR_CLASSES);
    X.len = (uint32_t*)k.take(4 * B), X.head = (uint32_t*)k.take(4 * B), X.perm = (uint32_t*)k.take(4 * B), X.cls = (uint8_t*)k.take(B);
    return k.off + ZK_LAYOUT_TAIL;
}
struct RrWindow {
    uint32_t* which;
    uint8_t *blinder, *rng, *msg;
};
static size_t rering_window_layout(RrWindow& W, uint8_t* base, size_t Wp, size_t rng_row) {
    Carver k(base);
    W.which = (uint32_t*)k.take(4 * Wp), W.blinder = (uint8_t*)k.take(32 * Wp), W.rng = (uint8_t*)k.take(rng_row * Wp + 32), W.msg = (uint8_t*)k.take(32 * Wp);
    return k.off + ZK_LAYOUT_TAIL;
}
// The device pointers of a call, or of one window of it (msg, which, blinder and rng.data are then the window's gathered arrays)
struct RrArgs {
    const uint8_t *msg, *proofs;
    const uint64_t* off;
    const uint32_t* which;
    const uint8_t* blinder;
    zk_rng rng;
    uint8_t* out;
    uint64_t* out_off;
    int32_t* status;
};
// The chunks of n proofs over the bound ring on the lanes: a one-class call (sel == nullptr), or one window of a mixed call, whose entry j is proof sel[j]
// of the batch of B.  rering_device's chunk with the sel-indexed kernels; the offsets exist already.  The lanes start behind `ready` and are drained before
// it returns; *he is what draining them gave.
static zk_status rering_rings_run(zk_ctx* c, uint64_t n, const RrArgs& A, const RrBufs& R, uint32_t C, bool timed, const uint32_t* sel, uint64_t B, hipEvent_t ready,
                                  hipError_t* he) {
    const bool full = c->mode == ZK_MODE_HARDENED;
    const std::vector<ChunkPlan> plan = make_chunk_plan(n, C, 1, false);
    const uint32_t NL = (uint32_t)std::min<size_t>(c->lanes, plan.size());
    if (zk_status zs = ensure_member_lanes(c, C, NL)) return zs;
    for (uint32_t l = 0; l < NL; l++) HIPCHK(c, hipStreamWaitEvent(c->pl[l].stream, ready, 0));
    Wire wire = wire_make(c->wire != 0);
    wire.fixed = 0, wire.rep_head = 0, wire.padd = 0;   // the writers' view: W.out_base[p] = the start of proof p's GKProof section
    for (uint64_t k = 0; k < plan.size(); k++) {
        const uint32_t lane = (uint32_t)(k % NL), cnt = plan[k].cnt;
        const uint64_t first = plan[k].first;
        auto& L = c->ml[lane];
        const RrLane& X = R.lane[lane];
        hipStream_t s = c->pl[lane].stream;
        Workspace W = L.W;
        W.gk_fill0 = 0;
        W.gk_stmt = full ? GK_STMT_FULL : GK_STMT_NONE, W.ring_digest = c->ring->ring_digest, W.wire = wire_make(c->wire != 0);
        W.Rx = X.Rx, W.Ry = X.Ry, W.la.ax = X.kax, W.la.ay = X.kay;
        member_chunk_rng(c, timed, s, W, A.rng, first, cnt);
        const ChunkIn in =
            member_chunk_commit(c, timed, s, W, L, cnt, [&] { launch_rrr_front(s, W, X, cnt, first, sel, B, A.proofs, A.off, A.which, A.blinder, L.which_s); });
        {
            MaybeScope t(timed, c, "rr_offsets", s);
            launch_rrr_compare(s, W, X, cnt, first, sel, B, A.status);
            launch_rrr_place(s, W, X, cnt, first, sel, B, A.out_off);
        }
        {
            MaybeScope t(timed, c, "hash", s);
            Workspace H = W;   // (as in rering_device)
            if (full) H.sec = 0;
            launch_gk_hash(s, H, cnt, full ? A.msg + 32 * first : nullptr);
        }
        W.wire = wire;
        {
            MaybeScope t(timed, c, "respond_write", s);
            launch_gk_respond(s, W, in, A.out);
        }
    }
    *he = drain_lanes(c, NL);
    return ZK_OK;
}
static zk_status rering_rings_device(zk_ctx* c, uint64_t B, const RrArgs& A, const uint32_t* d_ids, uint64_t out_cap) {   // (A.rng.data: a device pointer)
    if (zk_status zs = rering_rings_refusal(c)) return zs;
    if (!rng_mode_ok(&A.rng) || B > 0xffffffffull || ((uintptr_t)A.proofs & 3) || ((uintptr_t)A.out & 3)) return ZK_E_ARG;
    hipStream_t s0 = c->stream;
    timing_begin(c);
    if (B == 0) {
        HIPCHK(c, hipMemsetAsync(A.out_off, 0, 8, s0));
        HIPCHK(c, hipStreamSynchronize(s0));
        return ZK_OK;
    }
    RrRings R;
    Ring* slot[ZK_MAX_RINGS] = {};
    rering_ring_table(c, R, slot);
    const bool in_place = A.out == A.proofs, timed = zk_timed(c, B);
    const Wire wire = wire_make(c->wire != 0);
    RrCensus X;
    if (zk_status zs = lay_out(c, B_mr, [&](uint8_t* base) { return rering_census_layout(X, base, B); })) return zs;
    if (!c->h_rrr) HIPCHK(c, hipHostMalloc((void**)&c->h_rrr, RRR_READBACK, hipHostMallocDefault));
    if (!c->mr_ready) HIPCHK(c, hipEventCreateWithFlags(&c->mr_ready, hipEventDisableTiming));
    {
        MaybeScope t(timed, c, "rr_census", s0);
        launch_rrr_census(s0, B, A.proofs, A.off, A.which, d_ids, wire, R, X);
    }
    HIPCHK(c, hipMemcpyAsync(c->h_rrr, X.cnt, RRR_READBACK, hipMemcpyDeviceToHost, s0));   // counters and per-class totals lie side by side: the call's ONE read-back
    HIPCHK(c, hipStreamSynchronize(s0));
    const uint64_t* tot = (const uint64_t*)c->h_rrr;
    const uint32_t *cnt = (const uint32_t*)(c->h_rrr + RRR_HEAD_BYTES), *start = cnt + MR_CLASSES;
    if (zk_status zs = rrr_decide(A.proofs, A.out, out_cap, tot[0], tot[1], tot[2])) {   // before a byte of out, out_off or the statuses is written
        c->err = zs == ZK_E_BUFFER ? "output buffer too small"
                 : in_place        ? "in place: a proof's n is not its destination ring's (its GKProof section changes size)"
                                   : "out overlaps proofs (only out == proofs is supported: the in-place form)";
        wipe_witness(c);
        return zs;
    }
    {
        MaybeScope t(timed, c, "rr_offsets", s0);
        launch_rrr_offsets(s0, B, X, A.off, in_place, A.out_off, A.status);
    }
    const uint32_t one = mr_single_class(cnt, R.m);
    uint32_t Wp = (uint32_t)B;
    RrWindow Wn{};
    zk_status zs = ZK_OK;
    if (one >= MR_CLASSES) {
        launch_rrr_perm(s0, B, X);
        Wp = mr_window_cap(c->chunk, c->lanes, cnt, R.m);
        zs = lay_out(c, B_mw, [&](uint8_t* base) { return rering_window_layout(Wn, base, Wp, rng_bytes(&A.rng, 1)); });
    }
    const uint32_t C = std::min<uint32_t>(c->chunk, Wp);
    RrBufs Rb;
    if (!zs) zs = lay_out(c, B_rr, [&](uint8_t* base) { return rering_layout(Rb, base, C, std::min<uint32_t>(c->lanes, ZK_MAX_LANES)); });
    hipError_t he = hipSuccess;
    bool moved = in_place;   // in place no head moves
    auto move_heads = [&] {
        if (moved) return;
        MaybeScope t(timed, c, "rr_move", s0);
        launch_rrr_move(s0, B, X, R, A.proofs, A.off, A.out_off, A.out);
        moved = true;
    };
    if (!zs && one < MR_CLASSES) {
        RingBind rb(c, slot[one]);
        if ((he = hipEventRecord(c->mr_ready, s0)) == hipSuccess) {
            move_heads();
            zs = rering_rings_run(c, B, A, Rb, C, timed, nullptr, B, c->mr_ready, &he);
        }
    } else if (!zs) {
        RrArgs Aw = A;
        Aw.which = Wn.which, Aw.blinder = Wn.blinder, Aw.rng.data = Wn.rng, Aw.msg = Wn.msg;
        const bool full = c->mode == ZK_MODE_HARDENED;
        for (uint32_t r = 0; r < R.m.count && !zs && he == hipSuccess; r++) {
            RingBind rb(c, slot[r]);
            for (uint32_t w = 0; w < mr_window_count(cnt[r], Wp) && !zs && he == hipSuccess; w++) {
                uint32_t first, n;
                mr_window(cnt[r], Wp, w, &first, &n);
                const uint32_t* sel = X.perm + start[r] + first;
                c->dbg_mr_windows++;
                {
                    MaybeScope t(timed, c, "m_gather", s0);
                    launch_mr_pgather(s0, n, B, sel, A.which, A.blinder, A.rng.mode == ZK_RNG_SEED ? (const uint8_t*)A.rng.data : nullptr, full ? A.msg : nullptr, Wn.which,
                                      Wn.blinder, Wn.rng, Wn.msg);
                    if (A.rng.mode == ZK_RNG_STREAM) launch_pr_gather_rows(s0, n, sel, (const uint8_t*)A.rng.data, rng_bytes(&A.rng, 1), Wn.rng);
                }
                if ((he = hipEventRecord(c->mr_ready, s0)) != hipSuccess) break;
                move_heads();
                zs = rering_rings_run(c, n, Aw, Rb, C, timed, sel, B, c->mr_ready, &he);
            }
        }
    }
    if (!zs && he == hipSuccess) {
        move_heads();   // (a batch none of whose proofs entered a window)
        if (!in_place) launch_rrr_blank(s0, B, A.out_off, A.status, A.out);
    }
    // nothing of this call may still be running (or writing into the caller's buffers) when it returns
    if (const hipError_t e = hipStreamSynchronize(s0); he == hipSuccess) he = e;
    if (zs || he != hipSuccess) wipe_witness(c);   // a failed call leaves no gathered blinder, seed or stream row, no nonce and no RNG block behind
    if (zs) return zs;
    HIPCHK(c, he);
    HIPCHK(c, hipGetLastError());
    timing_end(c);
    return ZK_OK;
}
extern "C" zk_status zk_proof_rering_batch_rings_device(zk_ctx* c, uint64_t B, const void* d_msg, const void* d_proofs, const void* d_off, const void* d_which, const void* d_ids,
                                                        const void* d_blinder, const zk_rng* rng, void* d_out, uint64_t out_cap, void* d_out_off, void* d_status) {
    if (!c || !rng || !d_out_off || (B && (!d_msg || !d_proofs || !d_off || !d_which || !d_ids || !d_blinder || !rng->data || !d_out || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return rering_rings_device(c, B, {(const uint8_t*)d_msg, (const uint8_t*)d_proofs, (const uint64_t*)d_off, (const uint32_t*)d_which, (const uint8_t*)d_blinder, *rng,
                                      (uint8_t*)d_out, (uint64_t*)d_out_off, (int32_t*)d_status}, (const uint32_t*)d_ids, out_cap);
}
// Host pointers: the batch is planned HERE from ids, headers and indices (rering_plan.h: what the census and the offsets kernel compute), so every decision of
// the call falls before anything is uploaded; then it is staged as zk_proof_rering_batch stages its own and takes the device path.
struct RrRingsIn {
    RrIn one;
    uint32_t* ids;
};
static size_t rering_rings_in_layout(RrRingsIn& I, uint8_t* base, size_t B, size_t rng_bytes) {
    Carver k(base);
    k.off = rering_in_layout(I.one, base, B, rng_bytes);
    I.ids = (uint32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_proof_rering_batch_rings(zk_ctx* c, uint64_t B, const uint8_t* msg, const uint8_t* proofs, const uint64_t* off, const uint32_t* which, const uint32_t* ids,
                                                 const uint8_t* blinder, const zk_rng* rng, uint8_t* out, uint64_t out_cap, uint64_t* out_off, int32_t* status) {
    if (!c || !rng || !out_off || !off || (B && (!msg || !proofs || !which || !ids || !blinder || !rng->data || !out || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = rering_rings_refusal(c)) return zs;
    if (!rng_mode_ok(rng) || B > 0xffffffffull) return ZK_E_ARG;
    if (B == 0) {
        out_off[0] = 0;
        return ZK_OK;
    }
    RrRings R;
    Ring* slot[ZK_MAX_RINGS] = {};
    rering_ring_table(c, R, slot);
    const bool in_place = out == proofs;   // the staged copy is re-ringed in place and comes back as a whole
    const RrBatch t = rrr_plan_host(R, wire_make(c->wire != 0), B, proofs, off, ids, which, nullptr, nullptr);
    if (zk_status zs = rrr_decide(proofs, out, out_cap, t.bytes, t.other, off[B])) {
        c->err = zs == ZK_E_BUFFER ? "output buffer too small"
                 : in_place        ? "in place: a proof's n is not its destination ring's (its GKProof section changes size)"
                                   : "out overlaps proofs (only out == proofs is supported: the in-place form)";
        wipe_witness(c);
        return zs;
    }
    const uint64_t in_bytes = in_place ? std::max(t.in_bytes, off[B]) : t.in_bytes, need = in_place ? in_bytes : t.bytes;
    RrRingsIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return rering_rings_in_layout(I, base, B, rng_bytes(rng, B)); })) return zs;
    if (zk_status zs = reserve(c, B_io, in_bytes + 32)) return zs;
    if (!in_place)
        if (zk_status zs = reserve(c, B_ro, need + 32)) return zs;
    uint8_t *const d_proofs = (uint8_t*)c->buf[B_io].p, *const d_out = in_place ? d_proofs : (uint8_t*)c->buf[B_ro].p;
    // from the first upload on, blinders and seeds lie in the input buffer: every failure below zeroes them
    if (zk_status zs = upload_or_wipe(c, {{I.one.msg, msg, 32 * B}, {I.one.blinder, blinder, 32 * B}, {I.one.rng, rng->data, rng_bytes(rng, B)}, {I.one.which, which, 4 * B},
                                          {I.ids, ids, 4 * B}, {I.one.off, off, 8 * (B + 1)}, {d_proofs, proofs, in_bytes}}))
        return zs;
    if (zk_status zs = rering_rings_device(c, B, {I.one.msg, d_proofs, I.one.off, I.one.which, I.one.blinder, zk_rng{rng->mode, I.one.rng, rng->stride_blocks}, d_out, I.one.out_off,
                                                  I.one.st}, I.ids, need)) {
        wipe_witness(c);
        return zs;
    }
    return download_or_wipe(c, {{I.one.out_off, out_off, 8 * (B + 1)}, {I.one.st, status, 4 * B}, {d_out, out, need}});
}

// zk_prove_key_blinders_device's pipeline for api_quorum.hip (quorum.h)
zk_status zkq_key_blinders(zk_ctx* c, uint64_t B, const zk_rng& rng, uint8_t* d_out) { return key_blinders_device(c, B, rng, d_out); }
