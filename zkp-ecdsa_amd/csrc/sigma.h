// The host layer the sigma proofs share (api_link.hip, api_distinct.hip, api_escrow.hip, api_escrow_share.hip): every call carves one arena per lane from a
// witness-flagged buffer, runs its chunks over the lanes -- per chunk the RNG prepass, then the proof type's own list of launches -- and drains the lanes.
// What differs per proof type is that list, a few lane fields (engine.h: SigmaLane and what derives from it) and the I/O struct; the rest is here.
#pragma once
#include "jobs.h"   // ctx.h (engine.h), MaybeScope, words_aligned

// ------------------------------------------------------------------ lanes
// The shared fields of a lane of C proofs: `slots` list slots, `rng_blocks` 32-byte RNG blocks and `msg_blocks` 64-byte message blocks per proof
static inline void sigma_carve_core(SoaCarver& k, SigmaLane& X, uint32_t C, size_t slots, size_t rng_blocks, size_t msg_blocks) {
    X.C = C;
    X.L = k.list(slots * C);
    X.rng.exc_idx = (uint32_t*)k.take(4 * RNG_MAX_EXC * (size_t)C);
    X.rng.exc_flags = (uint32_t*)k.take(4 * RNG_MAX_EXC * (size_t)C);
    X.rng.exc_cnt = (uint32_t*)k.take(4 * (size_t)C);
    X.rng_fill = (uint32_t*)k.take(32 * rng_blocks * C);
    X.st = (int32_t*)k.take(4 * (size_t)C);
    X.flags = (uint32_t*)k.take(4 * (size_t)C);
    X.msg = (uint8_t*)k.take(msg_blocks * 64 * C);
    X.wk = (uint32_t*)k.take(msg_blocks * 256 * C);
    X.chal = (uint32_t*)k.take(16 * (size_t)C);
}
// The chunk plan of a call of B proofs and its lanes' arenas
template <class Lane>
struct SigmaRun {
    std::vector<ChunkPlan> plan;
    uint32_t NL = 0;
    Lane K[ZK_MAX_LANES];
};
struct SigmaNoFront {
    void operator()(SoaCarver&) const {}
};
// carve_lane(k, lane, C) takes one lane's arena; carve_front(k) what the call keeps in front of the lanes
template <class Run, class CarveLane, class CarveFront = SigmaNoFront>
static inline zk_status sigma_plan(zk_ctx* c, uint64_t B, BufId id, Run& R, CarveLane&& carve_lane, CarveFront&& carve_front = CarveFront{}) {
    const uint32_t C = (uint32_t)std::min<uint64_t>(c->chunk, B);
    R.plan = make_chunk_plan(B, C, 1, false);
    R.NL = (uint32_t)std::min<size_t>(std::min<uint32_t>(c->lanes, ZK_MAX_LANES), R.plan.size());
    return lay_out(c, id, [&](uint8_t* base) {
        SoaCarver k(base);
        carve_front(k);
        for (uint32_t l = 0; l < R.NL; l++) carve_lane(k, R.K[l], C);
        return k.off + ZK_LAYOUT_TAIL;
    });
}

// ------------------------------------------------------------------ a chunk's RNG
// Binds R to proofs first .. first + cnt of `rng`, whose data is a device pointer, and runs the prepass over nblk blocks per proof; then, in seed mode, R reads
// the fills the prepass wrote, which are the chunk's own: proof 0 of the fills is proof `first` of the call.  (The prepass takes a workspace and reads its RNG
// view alone: k_hash.hip: k_rng_prepass without by_zcnt.)
static inline void sigma_chunk_rng(zk_ctx* c, bool timed, hipStream_t s, RngCtx& R, uint32_t* fill, const zk_rng& rng, uint64_t first, uint32_t cnt, uint32_t nblk) {
    R.seeds = rng.data, R.stream = rng.data, R.stride_blocks = rng.stride_blocks, R.mode = rng.mode, R.sec = -1, R.proof_base = (uint32_t)first;
    {
        MaybeScope t(timed, c, "rng_prepass", s);
        Workspace W{};
        W.rng = R;
        launch_rng_prepass(s, W, cnt, 0, nblk, nblk, rng.mode == ZK_RNG_SEED ? fill : nullptr, false);
    }
    if (rng.mode == ZK_RNG_SEED) R.mode = ZK_RNG_STREAM, R.stream = (const uint8_t*)fill, R.stride_blocks = nblk, R.proof_base = 0;
}

// ------------------------------------------------------------------ the chunks of a call
// body(lane, stream, cnt, first) enqueues one chunk; chunk k runs on lane k % NL.  Then the call ends: the lanes are drained, a prover whose lanes failed
// leaves no nonce, blinder or RNG block behind, and the timing record closes.
template <class Run, class Body>
static inline zk_status sigma_run_chunks(zk_ctx* c, Run& R, bool prover, Body&& body) {
    for (uint64_t k = 0; k < R.plan.size(); k++) {
        const uint32_t lane = (uint32_t)(k % R.NL);
        body(R.K[lane], c->pl[lane].stream, R.plan[k].cnt, R.plan[k].first);
    }
    const hipError_t e_sync = drain_lanes(c, R.NL);
    if (prover && e_sync != hipSuccess) wipe_witness(c);
    HIPCHK(c, e_sync);
    HIPCHK(c, hipGetLastError());
    timing_end(c);
    return ZK_OK;
}

// ------------------------------------------------------------------ gates
static inline zk_status sigma_refusal(zk_ctx* c, uint64_t B) {
    if (!c->params_set) return ZK_E_BUFFER;
    if (c->stream_busy) return busy_refusal(c);
    if (B > 0xffffffffull) return ZK_E_ARG;
    return ZK_OK;
}
// A prover's gate, the device form's and the host-pointer form's alike: the refusal, the RNG's mode, room for B proofs of `size` bytes, B = 0.  True: the call
// ends here with `zs`.
static inline bool sigma_prove_gate(zk_ctx* c, uint64_t B, const zk_rng& rng, uint64_t out_cap, uint64_t size, zk_status& zs,
                                    zk_status (*refusal)(zk_ctx*, uint64_t) = sigma_refusal) {
    zs = refusal(c, B);
    if (zs == ZK_OK && !rng_mode_ok(&rng)) zs = ZK_E_ARG;
    if (zs == ZK_OK && B > out_cap / size) {
        c->err = "output buffer too small";
        zs = ZK_E_BUFFER;
    }
    return zs != ZK_OK || B == 0;
}
