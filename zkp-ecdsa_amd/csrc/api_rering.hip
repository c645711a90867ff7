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
