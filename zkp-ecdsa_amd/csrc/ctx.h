// Shared host-side context of libzkattest_hip.so (api.hip: prover pipeline; api_verify.hip: verifier pipeline): the context itself, its grow-only device
// buffers (GrowBuf, reserve, lay_out), the refusal while streamed jobs are queued, the timed scopes and the chunk plan.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "engine.h"
#include "layout.h"

struct TimerRec {
    const char* name;
    hipEvent_t e0, e1;
};
#define ZK_MAX_LANES 4
// A grow-only device buffer: a call that needs more frees it and allocates anew, nothing shrinks it before the context goes.
struct GrowBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool witness = false;   // holds signatures, seeds, nonces or candidate keys: zeroed by wipe_witness
};
enum GrowPolicy {
    GROW_EXACT,   // hipMalloc of what is needed
    GROW_SHED,    // ... through malloc_or_shed: the optional per-ring tables go first
    GROW_SLACK,   // need + need / 4 + 4096: buffers that follow B call by call
    GROW_SPARE,   // a staging buffer of a finished streamed job where one is large enough (stream_take_spare_dev), else exact
    GROW_ONCE,    // allocated by the first call; its size does not depend on the call
};
// The context's device buffers: name, policy, witness-derived?  One line here is all a new buffer takes -- zk_ctx_destroy frees and wipe_witness zeroes by this table.
#define ZK_CTX_BUFS(X)                                                                                                                                             \
    X(rg, GROW_EXACT, false)      /* mixed-ring verify calls (api_verify.hip): census, permutation and counters */                                                \
    X(pr, GROW_EXACT, false)      /* mixed-ring prove calls (api.hip): classes, per-workgroup counters, permutation, the segment's (staging offset, length) */   \
    X(pw, GROW_SHED, true)        /* ... the window one ring's inputs are gathered into: signatures, seeds or RNG streams */                                      \
    X(ps, GROW_SHED, false)       /* ... staging of a segment's proofs until their final offsets are known */                                                     \
    X(scr, GROW_ONCE, true)       /* witness screen (api_screen.hip): a chunk's scratch areas (u1, u2) and, host-pointer forms, its inputs and results */         \
    X(rec, GROW_ONCE, true)       /* key recovery (api_recover.hip): a chunk's scratch areas, lifted R, candidate keys and, host-pointer forms, its inputs */     \
    X(lv, GROW_EXACT, false)      /* per-proof verify levels: census, permutation and counters of a mixed batch */                                                \
    X(lw, GROW_EXACT, false)      /* partitioned verification: offsets, message hashes, seeds and verdicts of the window one class's proofs are gathered into */ \
    X(lb, GROW_EXACT, false)      /* ... and the window's proof bytes */                                                                                          \
    X(io, GROW_SPARE, false)      /* host-pointer entry points: staging of the proof bytes (a multi-GB hipMalloc / hipFree per call costs as much as the copy) */ \
    X(seed, GROW_SLACK, false)    /* the verifier's own seeds when the caller gives none (32 B bytes) */                                                          \
    X(in, GROW_SLACK, true)       /* host-pointer entry points: the small per-proof arrays (inputs, offsets, statuses, verdicts) */                               \
    X(unp, GROW_EXACT, false)     /* ZKA1P input of the synchronous verify calls: staging of the expanded proofs */                                               \
    X(unp_off, GROW_EXACT, false) /* ... and their per-chunk offsets */                                                                                           \
    X(m_off, GROW_SLACK, false)   /* membership proofs on their own: offsets of a verify call's equally long proofs */                                            \
    X(vp, GROW_SLACK, false)      /* exhaustive verify mode: verdicts and statuses of a pass behind the first (5 B bytes), until they are merged */           \
    X(mr, GROW_EXACT, false)      /* mixed-ring membership and re-ring calls (api_member.hip, api_rering.hip): classes, per-workgroup counters, permutation */    \
    X(mw, GROW_SHED, true)        /* ... the window one ring's inputs are gathered into: indices, blinders, seeds or RNG streams; coms, offsets, verifier seeds; message hashes */ \
    X(rr, GROW_EXACT, false)      /* re-ring calls (api_rering.hip): the census counters and every lane's per-proof arrays (head lengths, keyXcom, R: public) */ \
    X(ro, GROW_SPARE, false)      /* ... host-pointer form: staging of the re-ringed proofs (the input proofs lie in io) */ \
    X(kb, GROW_ONCE, true)        /* zk_prove_key_blinders: a chunk's rejection lists (derived from the seeds) and the call's exhaustion flag */ \
    X(lk, GROW_SHED, true)        /* link proofs (api_link.hip): the lanes' arenas -- the staged key and blinders, the nonces k, s1, s2, the RNG fills, the challenge's message */ \
    X(dk, GROW_SHED, true)        /* distinct-key proofs (api_distinct.hip): the lanes' arenas -- the staged keys and blinders, d, 1 / d, r_w, the nonces, the RNG fills, the challenge's message */ \
    X(qs, GROW_SHED, true)        /* quorum proofs (api_quorum.hip): a window's staging -- the gathered keys, keyXcoms and blinders of its pairs, its attestations and distinct-key proofs until they are in place; verifier: the walked offsets, the members' and pairs' bytes and verdicts */ \
    X(et, GROW_SHED, true)        /* escrow tags (api_escrow.hip): the lanes' arenas -- the staged key and blinder, rho and the nonces, the RNG fills, the challenge's message; an open call's staged secret a, the points 4 (E2 - a E1) and a slab of the ring's points */ \
    X(qc, GROW_SLACK, false)      /* ... the quorum calls' `_rings` forms: every quorum's capacity, the call's total and the set of rings its ids name (from ring ids: public) */ \
    X(as, GROW_SHED, true)        /* accountable attestations (api_accountable.hip): a window's staging -- the gathered keys, blinders and keyXcoms, its attestations and tags until they are in place; verifier, split and join: the walk's records, the attestations' and tags' bytes and verdicts */
enum BufId {
#define X(name, policy, witness) B_##name,
    ZK_CTX_BUFS(X)
#undef X
        B_COUNT
};
// One resident ring of a context: the padded ring's limbs and the tables built from it.  Every table but the limbs and the digest is optional.
struct Ring {
    uint32_t id = 0;
    bool live = false;
    uint64_t generation = 0;       // bumped by every build (zk_ring_info)
    uint32_t* ring_mem = nullptr;
    uint32_t* gk_etab = nullptr;   // table of the GK block transform (k_gk.hip); nullptr for small / huge rings
    uint32_t* ktab = nullptr;      // per-key tables (k_ktab.hip): 264 KB per key (KTAB_KEY_WORDS), rings of up to 2^KTAB_MAXN keys
    uint8_t* ktab_ok = nullptr;    // [N] which ring values are x-coordinates and own a table
    int8_t* gk_kdig = nullptr;     // the ring as int8 digit fragments (k_gk_mfma.hip), built with table E for rings of >= 2^12 keys
    int8_t* gk_edig = nullptr;     // table E's coefficient classes 2..6 as digit fragments: the prover's matrix-pipe table path (k_gk_mfma.hip)
    uint64_t N = 0, nkeys = 0;
    uint32_t n = 0;
    uint32_t* ring_digest = nullptr;   // [8] SHA-256 words of the padded ring (hardened mode)
    uint32_t* leaves = nullptr;        // [8 x ceil(N / 256)] the digest's leaf hashes, kept so that zk_ctx_update_ring rehashes the touched leaves and the root only
    uint32_t* esc_pts = nullptr;       // [18][N] the points 4 y_i g of the keys below nkeys (escrow_index.h), built by the first zk_rings_escrow_open_batch
    uint32_t* esc_slots = nullptr;     // [2 N] ... and the open-addressed table of key indices over them; both or neither
};
struct zk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // params
    DevParams P{};
    bool params_set = false;
    // the auditor's key of the escrow tags (zk_ctx_set_auditor, api_escrow.hip): a second comb set over (g, A) in the shape of P, so that the commitment
    // kernels produce x g + rho A unchanged.  Its width is its own (ZK_AUDITOR_BITS); g's table is the context's where the widths agree, else aud_tab_g.
    DevParams PA{};
    bool auditor_set = false;
    uint32_t* aud_tab_g = nullptr;    // g at the auditor set's width where the context's differs (owned; nullptr: PA.tom_tab_g is P.tom_tab_g)
    uint32_t aud_w[18] = {};          // A as nine little-endian words per coordinate, and as the caller's bytes
    uint8_t aud_xy[72] = {};
    // the share keys A_1 .. A_n of a t-of-n opening (zk_ctx_set_auditors, api_escrow_share.hip): public, checked against the auditor's key and dropped with it
    uint32_t auditors_t = 0, auditors_n = 0;   // n = 0: no set
    uint8_t auditors_xy[16][72] = {};
    uint32_t* auditors_w = nullptr;   // [16][18] on the device: nine little-endian words per coordinate (allocated by the first set, freed by zk_ctx_destroy)
    uint32_t tom_g_w[18] = {};       // g in the same form (zk_ctx_set_params)
    uint32_t* tom_tab_gen = nullptr;  // 8-bit comb table of the Tom generator (synthetic params only)
    uint32_t tom_bits = TOM_DEFAULT_BITS;  // comb width requested for g, h (zk_ctx_set_comb_bits)
    uint32_t tab_bits_alloc = 0;      // width the allocated P.tom_tab_g/h were sized for (0 = not allocated)
    size_t scratch_words = 0;
    uint32_t* tab_scratch = nullptr;
    int32_t* d_flag = nullptr;
    // ring: the resident rings (zk_ctx_add_ring; zk_ctx_set_ring builds the active one) and the one the running call is bound to
    Ring rings[ZK_MAX_RINGS];
    Ring no_ring;                  // what `ring` points at while no ring is active: N = 0, every table nullptr
    Ring* ring = &no_ring;         // the active ring between calls; a mixed-ring verify call binds each class's ring in turn (RingBind)
    int active = -1;               // slot of the active ring in `rings`, -1 = none
    uint32_t next_ring_id = 0;     // ids are never reused within a context
    bool gk_table = true;          // ZKATTEST_GK_TABLE=0 disables table E (plain fold for every ring)
    bool key_tables = true;        // ZKATTEST_KEYTAB=0 / zk_ctx_set_key_tables(ctx, 0): per-proof tables of R for every proof (read when a ring is built)
    bool gk_mfma_prove = true;     // build gk_edig with the ring (ZKATTEST_GK_MFMA_PROVE; read when a ring is built)
    bool gk_mfma = true;           // verifier's ring fold on the matrix pipe where gk_kdig exists (zk_ctx_set_ring_fold, ZKATTEST_GK_MFMA)
    GrowBuf buf[B_COUNT];          // the device buffers of ZK_CTX_BUFS, policy and witness flag as listed there (zk_ctx's constructor)
    uint32_t* h_rg = nullptr;      // mixed-ring verify calls: page-locked read-back of the per-class counters
    uint32_t* h_pr = nullptr;      // mixed-ring prove calls (api.hip: prove_rings_device): page-locked read-back of the counters
    size_t h_pr_bytes = 0;
    hipEvent_t pr_ready = nullptr; // "the window is gathered": the lanes' stage 1 waits for it
    uint32_t* h_mr = nullptr;      // mixed-ring membership calls (api_member.hip): page-locked read-back of the per-class counters
    hipEvent_t mr_ready = nullptr; // ... "the window is gathered": the lanes wait for it
    unsigned long long* h_rr = nullptr;   // re-ring calls (api_rering.hip): page-locked read-back of the census counters
    uint8_t* h_rrr = nullptr;             // ... their mixed-ring form: of the census counters and the per-class totals (RRR_READBACK bytes)
    hipEvent_t rr_scan[ZK_MAX_LANES] = {};   // ... "this lane's chunk has written its offsets": the next chunk's scan, on another lane, starts behind it
    uint32_t pr_seg_force = 0;     // test build only (zk_test_set_prove_segment): proofs per segment instead of what ZK_PR_STAGE_BYTES holds; 0 = off
    uint32_t mode = 0;                 // zk_ctx_set_mode: ZK_MODE_REFERENCE / ZK_MODE_HARDENED
    uint32_t verify_level = 0;         // zk_ctx_set_verify_level: ZK_VERIFY_LEVEL_CONTEXT / ZK_VERIFY_LEVEL_PER_PROOF
    uint32_t verify_reps = 0;          // zk_ctx_set_verify_reps: ZK_VERIFY_REPS_SAMPLE / ZK_VERIFY_REPS_ALL
    // per-proof mode: the repetition count the verifier's workspaces are planned for during one call (or while streamed verify jobs are queued); the
    // context's own P.sec otherwise (plan_sec below), so that the next prove call plans at the context's level again
    uint32_t v_sec = 0;
    bool v_sec_on = false;
    uint32_t* h_lv = nullptr;          // per-proof mode: page-locked read-back of the per-level counters; partitioned verification: of a window's byte count
    // workspace: up to ZK_MAX_LANES pipeline lanes, each with its own HIP stream and prover / verifier workspace; consecutive
    // chunks go to consecutive lanes, so the low-occupancy per-proof kernels, the scans the host waits for and (host-pointer
    // calls) the output phases of different chunks fall into each other's heavy phases.  Lane 0 runs on `stream`.
    uint32_t chunk = 4096;
    uint32_t ws_C = 0, ws_sec = 0, ws_n = 0;
    bool ws_etab = false, ws_edig = false;   // the prover workspaces' layout also follows which of the bound ring's tables E exist
    struct ProveLane {
        hipStream_t stream = nullptr;
        Workspace W{};
        Soa gk_am{};
        uint32_t* d_totals = nullptr;
        GrowBuf arena{nullptr, 0, true};   // witness-derived (the RNG stream of every proof, nonces, s1 = s / r, blinders): wiped by wipe_witness
        bool ready = false;
        uint32_t last_cnt = 0;          // proofs of the last chunk this lane started (zk_test_counter)
        hipStream_t side = nullptr;     // small chunks: the membership phase of stage 2 runs beside the PointAdd phase (api.hip: ProveJob::stage2)
        hipEvent_t side_fork = nullptr, side_done = nullptr;
        void* h_scan = nullptr;         // page-locked: the chunk's totals (4 x u32), item prefix sums (u32[C+1]) and byte prefix sums
        size_t h_scan_bytes = 0;        // (u64[C+1]) read back after the scan.  Pageable destinations made the runtime wait for
                                        // EVERY stream of the device (measured: the host sat 50 ms behind the other lane's kernels)
        hipEvent_t copy_ev = nullptr;   // host-buffer entry points: "this lane's bytes are final" for the lane's copy stream
        hipStream_t copy_stream = nullptr;   // D2H of this lane's finished slices: one stream per lane, so a lane whose slices
                                             // are ready never queues behind the unfinished slices of another (FIFO per stream)
    } pl[ZK_MAX_LANES];
    uint32_t lanes = 2;
    // verifier workspace
    struct VerifyLane {
        VWork V{};
        GrowBuf arena;
        Soa res{}, res2{};
        MsmBuf M{};               // batched Tom check buffers (k_msm.hip), carved with V
        uint32_t* h_msm = nullptr;   // page-locked read-back words of run_msm
        hipEvent_t msm_done = nullptr;   // recorded behind a chunk's batched passes (stage2a); stage2b waits for it before it reads the verdicts
        bool msm_pending = false, pm_pending = false;   // ... which passes of the chunk between stage2a and stage2b are in flight
        uint32_t msm_gsz = 0;
        PMsmBuf PM{};             // cross-proof P-256 pass (k_pmsm.hip); PM.aos == nullptr: not carved (chunks below p256_batch_min)
        hipStream_t aux[V_AUX_STREAMS] = {};   // small batches: the independent per-proof sums run side by side (api_verify.hip: per_proof_range)
        hipEvent_t aux_fork = nullptr, aux_done[V_AUX_STREAMS] = {};
        bool p256_launched = false;   // stage2a launched the small chunk's P-256 sums (else stage2b does, behind the Tom-256 sums' kernels)
        bool stage2_forked = false;   // the auxiliary streams already wait for this chunk's stage 1 (stage2a of a small chunk)
        bool released_by_host = false;   // ... or the host waits for it in stage2b and launches their kernels then (VerifyJob::host_release)
        bool ready = false;
    } vl[ZK_MAX_LANES];
    // membership proofs on their own (api_member.hip): a lane holds what a chunk's GK phase needs and nothing of the repetitions -- the prover's view W (list C with
    // one more slot per proof for com, the fold's buffers, the RNG fills, the blinders) and the verifier's view V (the GK terms and sums).  Lane l runs on pl[l].stream.
    struct MemberLane {
        Workspace W{};
        VWork V{};
        Soa gk_am{}, res{}, res2{};
        uint32_t* which_s = nullptr;   // [C] the indices the fold kernels read (0 for one outside the ring)
        GrowBuf arena{nullptr, 0, true};   // witness-derived (blinders, nonces, the RNG stream): wiped with the prover lanes' (api.hip: wipe_witness)
        bool ready = false;
    } ml[ZK_MAX_LANES];
    uint32_t ms_C = 0, ms_n = 0;
    bool ms_etab = false, ms_edig = false;
    uint32_t vs_C = 0, vs_sec = 0, vs_n = 0;
    uint32_t p256_batch_min = 8192;   // chunks of at least this many proofs sum their P-256 relations across proofs too (ZKATTEST_P256_BATCH; 0 = never)
    uint32_t verify_groups = 8;   // groups per chunk of the batched Tom check: 8 (16-bit windows) or 64 (13-bit windows); zk_ctx_set_verify_groups
    uint32_t vs_groups = 8;       // ... the lanes' workspaces were carved for
    bool vs_pm = false;           // ... and of the cross-proof P-256 pass
    bool vs_msm = false;          // the lanes' workspaces hold the buffers of the batched Tom check
    uint32_t verify_batch_min = 256;   // zk_ctx_set_batch_verify: chunks of at least this many proofs get the batched check (0 = never)
    // host-buffer entry points: DMA stream for page-locked caller buffers (zk_host_alloc), one event per lane
    hipStream_t copy_stream = nullptr;
    uint8_t* h_stage = nullptr;    // page-locked mirror of in_buf's head for calls of a few proofs: the input arrays cross in ONE copy that no host thread waits for, and
    size_t h_stage_bytes = 0;      // the offsets / statuses / verdicts come back in one (api.hip: ensure_h_stage; wiped with the witness)
    hipEvent_t in_ready = nullptr; // ... the lanes wait for this event instead (the job's inputs_ready)
    uint32_t wire = 0;             // zk_ctx_set_wire: 0 = ZKA1 (36-byte Tom coordinates), 1 = ZKA1P (33-byte): what the prover emits and the verifier is handed
    uint32_t host_taper = 1;       // host-pointer calls on page-locked buffers: tapered chunk plan (zk_ctx_set_host_taper)
    uint32_t slice = 0;            // proofs per PointAdd slice of the prover (zk_ctx_set_slice): 0 = 4096 with a page-locked sink, else none
    // streamed calls (api_stream.hip): jobs submitted and not yet waited for, in submission order
    bool stream_busy = false;
    std::vector<struct zk_job*> jobs;
    uint64_t next_lane_base = 0;       // global chunk number of the next job's first chunk (lanes rotate across jobs)
    hipStream_t fin_stream = nullptr;  // collects a job's results (offsets, statuses, verdicts) behind its last kernels and copies
    struct Spare {                     // buffers of finished jobs, reused by the next ones (grow-only, like io_buf)
        void* p;
        size_t bytes;
    };
    std::vector<Spare> spare_dev, spare_pinned;
    // unit-test counters (zk_test_counter): work done, so that tests can assert on counts instead of timings
    uint64_t dbg_recheck_proofs = 0;   // proofs that went through the verifier's per-proof sums since the context was created
    uint64_t dbg_p256_batched = 0;     // proofs whose P-256 relation was accepted by the cross-proof pass (k_pmsm.hip) since the context was created
    uint64_t dbg_msm_terms = 0;        // live terms that went through the batched Tom-256 check (k_msm.hip) since the context was created
    uint64_t dbg_ktab_keys = 0;        // per-key tables computed by the builder (k_ktab.hip) since the context was created; copied tables do not count
    uint64_t dbg_etab_blocks = 0;      // 256-key blocks whose table E was built (k_gk.hip) since the context was created
    uint64_t dbg_pr_segments = 0;      // segments that mixed-ring prove calls staged since the context was created (a one-ring call stages none)
    uint64_t dbg_pr_windows = 0;       // ... and the windows they proved
    uint64_t dbg_mr_windows = 0;       // windows that mixed-ring membership calls proved or verified since the context was created (a one-ring call runs none)
    uint64_t dbg_v_passes = 0;         // passes of the verifier's pipeline since the context was created: one per blocking call or window, ceil(sec / VK) in ZK_VERIFY_REPS_ALL
    // timing
    std::vector<TimerRec> trecs;
    std::vector<hipEvent_t> epool;
    size_t eused = 0;
    std::vector<std::pair<const char*, float>> last_timing;
    float last_total_ms = 0, last_wall_ms = 0;   // sum of the timed scopes ('+' parts excluded); first start -> last end of the same call
    int timing_mode = ZK_TIMING_AUTO;   // zk_ctx_set_timing
    bool timing_forked = false;   // this call put timed scopes on forked streams (small one-chunk calls): its scopes overlap, the total is first start -> last end
    zk_ctx() {
#define X(name, policy, w) buf[B_##name].witness = w;
        ZK_CTX_BUFS(X)
#undef X
    }
};
static const GrowPolicy zk_buf_policy[B_COUNT] = {
#define X(name, policy, witness) policy,
    ZK_CTX_BUFS(X)
#undef X
};

#define HIPCHK(ctx, x)                                                                                      \
    do {                                                                                                    \
        hipError_t e_ = (x);                                                                                \
        if (e_ != hipSuccess) {                                                                             \
            char buf_[256];                                                                                 \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            (ctx)->err = buf_;                                                                              \
            return ZK_E_DEVICE;                                                                             \
        }                                                                                                   \
    } while (0)

static inline hipEvent_t get_event(zk_ctx* c) {
    if (c->eused == c->epool.size()) {
        hipEvent_t e;
        hipEventCreate(&e);
        c->epool.push_back(e);
    }
    return c->epool[c->eused++];
}
struct Scope {
    zk_ctx* c;
    TimerRec r;
    hipStream_t st;
    Scope(zk_ctx* c_, const char* name, hipStream_t s_ = nullptr) : c(c_), st(s_ ? s_ : c_->stream) {
        r.name = name, r.e0 = get_event(c), r.e1 = get_event(c);
        hipEventRecord(r.e0, st);
    }
    ~Scope() {
        hipEventRecord(r.e1, st);
        c->trecs.push_back(r);
    }
};
// Per-family events of a blocking call of B proofs?  Two events per family and chunk cost a call of a few proofs 0.15-0.45 ms of idle GPU between kernels
// (profiles/r06_ab_variants.txt (14)); a call of more than V_SIDE_MAXP proofs does not notice them.
// the repetition count the workspaces are planned for: the context's secLevel, or the level of the proofs a per-proof-mode verify call is running
static inline uint32_t plan_sec(const zk_ctx* c) { return c->v_sec_on ? c->v_sec : c->P.sec; }
// binds `r` as the ring of the running call (mixed-ring verification and proving) and puts the active ring back when the scope ends
struct RingBind {
    zk_ctx* c;
    Ring* prev;
    RingBind(zk_ctx* c_, Ring* r) : c(c_), prev(c_->ring) { c->ring = r; }
    ~RingBind() { c->ring = prev; }
};
static inline bool zk_timed(const zk_ctx* c, uint64_t B) { return c->timing_mode == ZK_TIMING_ON || (c->timing_mode == ZK_TIMING_AUTO && B > V_SIDE_MAXP); }
static inline void timing_begin(zk_ctx* c) { c->trecs.clear(), c->eused = 0, c->timing_forked = false; }
static inline void timing_end(zk_ctx* c) {
    c->last_timing.clear();
    c->last_total_ms = 0, c->last_wall_ms = 0;
    float wall = 0;
    hipEvent_t first = c->trecs.empty() ? nullptr : c->trecs[0].e0;
    for (auto& r : c->trecs) {   // the earliest start over all records: scopes of different lanes and forked streams are not in start order
        float d = 0;
        if (hipEventElapsedTime(&d, r.e0, first) == hipSuccess && d > 0) first = r.e0;
    }
    for (auto& r : c->trecs) {
        float ms = 0;
        hipEventElapsedTime(&ms, r.e0, r.e1);
        bool found = false;
        for (auto& p : c->last_timing)
            if (p.first == r.name) p.second += ms, found = true;
        if (!found) c->last_timing.push_back({r.name, ms});
        if (r.name[0] != '+') c->last_total_ms += ms;   // '+name': a part of another scope
        float end = 0;
        if (hipEventElapsedTime(&end, first, r.e1) == hipSuccess && end > wall) wall = end;
    }
    c->last_wall_ms = wall;   // first start -> last end; last_total_ms stays the SUM of the scopes (forked scopes overlap: the sum is then not a time)
}

// device allocation released on every exit path of an entry point
struct DevBuf {
    void* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { hipFree(p); }
    template <class T>
    T* as() const { return (T*)p; }
};
void escrow_index_drop(Ring& R);   // api_escrow.hip: frees a ring's point index (free_ring; zk_ctx_set_params for every ring: it was built for g)
// ... zk_ctx_update_ring's patch: the points of the touched real entries d_ent[0 .. real-1] recomputed, the slots refilled for nkeys keys.  Where the
// temporary memory is not there the index is dropped instead (the next open call rebuilds it).  Runs on c->stream, behind the patch of the ring's limbs.
hipError_t escrow_index_patch(zk_ctx* c, Ring& R, const uint32_t* d_ent, uint32_t real, uint64_t nkeys);
void escrow_drop_auditor(zk_ctx* c);   // api_escrow.hip: frees the (g, A) set (zk_ctx_set_params, zk_ctx_destroy; nothing may be in flight)
void wipe_witness(zk_ctx* c);   // api.hip: zeroes every witness-derived buffer of the context (nothing may be in flight)
// lanes 0 .. NL-1 drained: the first error one of their streams gave
static inline hipError_t drain_lanes(zk_ctx* c, uint32_t NL) {
    hipError_t first = hipSuccess;
    for (uint32_t l = 0; l < NL; l++) {
        const hipError_t e = hipStreamSynchronize(c->pl[l].stream);
        if (first == hipSuccess) first = e;
    }
    return first;
}
static inline bool rng_mode_ok(const zk_rng* rng) { return rng->mode == ZK_RNG_SEED || rng->mode == ZK_RNG_STREAM; }
static inline size_t rng_bytes(const zk_rng* rng, uint64_t B) { return rng->mode == ZK_RNG_SEED ? 32 * B : 32 * B * rng->stride_blocks; }   // what rng->data holds for B proofs
// The blocking copies of a host-pointer call whose staged inputs are witness-derived (signatures, blinders, seeds in c->buf[B_in]): rows of no bytes are
// skipped, and a failed copy zeroes every witness-derived buffer before the call returns.
struct UploadRow {
    void* dev;
    const void* host;
    size_t bytes;
};
struct DownloadRow {
    const void* dev;
    void* host;
    size_t bytes;
};
static inline zk_status upload_or_wipe(zk_ctx* c, std::initializer_list<UploadRow> rows) {
    for (auto& r : rows)
        if (r.bytes && hipMemcpy(r.dev, r.host, r.bytes, hipMemcpyHostToDevice) != hipSuccess) {
            c->err = "upload of the inputs failed";
            (void)hipGetLastError();
            wipe_witness(c);
            return ZK_E_DEVICE;
        }
    return ZK_OK;
}
static inline zk_status download_or_wipe(zk_ctx* c, std::initializer_list<DownloadRow> rows) {
    hipError_t e = hipSuccess;
    for (auto& r : rows)
        if (e == hipSuccess && r.bytes) e = hipMemcpy(r.host, r.dev, r.bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) wipe_witness(c);
    HIPCHK(c, e);
    return ZK_OK;
}
// The same rows where nothing staged is witness-derived (the host-pointer verify calls): copies on c->stream and one wait; a failing copy returns as it is
static inline zk_status upload_rows(zk_ctx* c, std::initializer_list<UploadRow> rows) {
    for (auto& r : rows)
        if (r.bytes) HIPCHK(c, hipMemcpyAsync(r.dev, r.host, r.bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ZK_OK;
}
static inline zk_status download_rows(zk_ctx* c, std::initializer_list<DownloadRow> rows) {
    for (auto& r : rows)
        if (r.bytes) HIPCHK(c, hipMemcpyAsync(r.host, r.dev, r.bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return ZK_OK;
}
// api_verify.hip: a verifier lane's arena for chunks of C proofs (base == nullptr: the size only); ensure_vworkspace carves the lanes with it, the bucket passes' test hooks a scratch arena
size_t vcarve(VWork& V, Soa& res, Soa& res2, MsmBuf& M, PMsmBuf& PM, uint8_t* base, uint32_t C, uint32_t sec, uint32_t n, uint64_t N, bool want_msm, bool want_pm, uint32_t want_groups);
zk_status ensure_workspace(zk_ctx* c, uint32_t C, uint32_t nlanes = 1);   // api.hip: prover workspaces of lanes 0..nlanes-1
hipError_t malloc_or_shed(zk_ctx* c, void** p, size_t bytes);   // api.hip: a workspace allocation that sheds the optional per-ring tables first
// settings a queued streamed job was planned with (its lane rotation, chunk size, workspaces, mode) and the buffers it reads stay frozen until it is waited for
static inline zk_status busy_refusal(zk_ctx* c) {
    c->err = "streamed jobs are in flight on this context (zk_prove_wait / zk_verify_wait them first)";
    return ZK_E_ARG;
}
zk_status reserve(zk_ctx* c, GrowBuf& b, size_t need, GrowPolicy policy);   // api.hip: `b` of at least `need` bytes
static inline zk_status reserve(zk_ctx* c, BufId id, size_t need) { return reserve(c, c->buf[id], need, zk_buf_policy[id]); }
// sizes `layout` (base -> bytes), reserves the buffer, carves it for real
template <class Layout>
static inline zk_status lay_out(zk_ctx* c, GrowBuf& b, GrowPolicy policy, Layout&& layout) {
    return lay_out(layout, [&](size_t need, uint8_t** base) {
        const zk_status zs = reserve(c, b, need, policy);
        *base = (uint8_t*)b.p;
        return zs;
    });
}
template <class Layout>
static inline zk_status lay_out(zk_ctx* c, BufId id, Layout&& layout) { return lay_out(c, c->buf[id], zk_buf_policy[id], layout); }
// The resident rings in slot order: the censuses class a proof by the place of its id in rs.id
static inline uint32_t ring_slots(zk_ctx* c, RingSlots& rs, Ring** slot) {
    rs = RingSlots{};
    for (auto& R : c->rings)
        if (R.live && R.N) slot[rs.count] = &R, rs.id[rs.count++] = R.id;
    return rs.count;
}
#define ZK_STAGE_MAX (1u << 20)   // input arrays up to this size take the page-locked mirror
zk_status ensure_h_stage(zk_ctx* c, size_t bytes);  // api.hip: c->h_stage of at least `bytes`, c->in_ready

// One pipeline pass = one chunk of consecutive proofs.  Device-pointer calls use uniform chunks of C proofs.  Host-pointer
// calls on page-locked buffers move ~169 KB per proof across PCIe on a copy stream under the kernels of the neighbouring
// chunks, and the transfer of a step takes almost as long as its kernels (11 GB at ~57 GB/s = 194 ms against ~250 ms), so the
// copy stream has to be fed early and evenly and whatever is still in flight at the end stays exposed:
//   * prove: a chunk's PointAdd phase -- 80 % of its bytes -- runs in proof-aligned SLICES (api.hip), each followed by the
//     D2H of the proofs it completed; what stays exposed is the last slice of each lane, so a chunk's slices taper;
//   * verify: the H2D of all chunks is enqueued up front and the lanes wait per chunk; what stays exposed is the kernels of
//     the last chunks.  Small chunks are inefficient (fixed cost of the chunk-wide bucket sum: 351 k verifies/s at 8 192
//     proofs per chunk, 250 k at 4 096), so a tapered tail was measured to LOSE (263 k against 287 k verifies/s): uniform chunks;
//   * prove: the first chunks of the lanes grow C/L, 2C/L, ... so that the lanes run out of phase and one lane's output
//     phase falls into the others' compute-only phases.
// The bytes of a proof do not depend on the plan (tests/test_gpu_scale.py::test_tapered_chunk_plan_...).
struct ChunkPlan {
    uint64_t first;
    uint32_t cnt;
};
#define ZK_TAPER_MIN 2048u
#define ZK_PROVE_SIDE_MAX 2048u   // chunks up to this size: stage 2's membership phase on the lane's side stream
#define ZK_SLICE_MIN 1024u
// sizes summing to B: the first `stagger` chunks grow C/stagger, 2C/stagger, ... (the lanes then finish out of phase), then
// chunks of C, then (tail) halving chunks C/2, C/4, ... >= lo with the last size twice
static inline std::vector<ChunkPlan> make_chunk_plan(uint64_t B, uint32_t C, uint32_t stagger, bool tail, uint32_t lo = ZK_TAPER_MIN) {
    std::vector<uint32_t> sizes, tl;
    uint64_t left = B;
    if (tail && C >= 2 * lo && B >= 2ull * C) {
        for (uint32_t s = C / 2; s >= lo; s /= 2) tl.push_back(s);
        tl.push_back(tl.back());
        for (uint32_t s : tl) left -= s;
    }
    if (stagger > 1 && C >= stagger * lo && left > (uint64_t)C * (stagger + 1) / 2) {
        for (uint32_t l = 1; l < stagger; l++) {
            uint32_t s = (uint32_t)(((uint64_t)C * l / stagger) & ~255ull);
            sizes.push_back(s), left -= s;
        }
    }
    while (left) {
        uint32_t c = (uint32_t)std::min<uint64_t>(C, left);
        sizes.push_back(c), left -= c;
    }
    for (uint32_t s : tl) sizes.push_back(s);
    std::vector<ChunkPlan> plan;
    uint64_t f = 0;
    for (uint32_t s : sizes) plan.push_back({f, s}), f += s;
    return plan;
}
float pinned_d2h_rate(void* p, size_t bytes);   // api.hip: slowest D2H rate over three windows of a page-locked range (the "slow pages" check)
void* alloc_fast_pinned(size_t bytes, const std::function<void*()>& alloc, const std::function<void(void*)>& release);   // api.hip: the fastest of up to three candidates
bool host_ptr_is_pinned(const void* p);     // api.hip: page-locked (zk_host_alloc / hipHostMalloc / hipHostRegister) host memory?
zk_status ensure_copy_stream(zk_ctx* c);    // api.hip: c->copy_stream and the lanes' copy events

struct SoaCarver : Carver {   // the workspace arenas' conveniences on top of layout.h
    using Carver::Carver;
    Soa soa(size_t elems) { return Soa{(uint32_t*)take(elems * 36), (uint32_t)elems}; }
    Soa3 soa3(size_t elems) { return Soa3{soa(elems), soa(elems), soa(elems)}; }
    TomList list(size_t cap) {
        TomList L;
        L.v = soa(cap), L.r = soa(cap), L.proj = soa3(cap), L.ax = soa(cap), L.ay = soa(cap), L.cap = (uint32_t)cap;
        return L;
    }
};
// The GK (ring membership) sections of a lane's arena.  The prover's, the verifier's and the member lanes' arenas (api.hip: carve; api_verify.hip: vcarve;
// api_member.hip: mcarve) take them from here, each run at its own place in the arena, every size from gk_plan.h.  W.C, W.sec, W.n (V.C, V.n) are set before.
static inline void carve_gk_scalars(SoaCarver& k, Workspace& W, Soa& gk_am) {
    W.gk_x = (uint32_t*)k.take(12 * (size_t)W.C);
    W.gk_coef = k.soa((size_t)(W.n + 1) * W.C);
    gk_am = k.soa((size_t)W.n * W.C);
}
// the prover's fold of a ring of N keys: what the table path adds where R has the tables, then the two ping-pong buffers
static inline void carve_gk_fold(SoaCarver& k, Workspace& W, const Ring& R, uint64_t N) {
    const GkProvePlan p = gk_prove_plan(W.C, W.n, N, R.gk_etab != nullptr);
    W.gk_group = p.group;
    W.gk_adig = R.gk_edig ? (int8_t*)k.take(gkm_asub_frag_bytes(W.C)) : nullptr;
    W.gk_toff = (uint32_t*)k.take(4 * 264);
    W.gk_asub = R.gk_etab ? (uint32_t*)k.take(36 * 256 * (size_t)W.C) : nullptr;
    W.gk_order = (uint32_t*)k.take(4 * (size_t)W.C);
    W.gk_goff = (uint32_t*)k.take(4 * 264);
    W.gk_bufA = (uint32_t*)k.take(36 * p.bufA);
    W.gk_bufB = (uint32_t*)k.take(36 * p.bufB);
}
// the RNG prepass's rejection lists and the chunk's fills, `blocks` 32-byte blocks per proof
static inline void carve_rng(SoaCarver& k, Workspace& W, size_t blocks) {
    W.rng.exc_idx = (uint32_t*)k.take(4 * RNG_MAX_EXC * (size_t)W.C);
    W.rng.exc_flags = (uint32_t*)k.take(4 * RNG_MAX_EXC * (size_t)W.C);
    W.rng.exc_cnt = (uint32_t*)k.take(4 * (size_t)W.C);
    W.rng_fill = (uint32_t*)k.take(32 * blocks * W.C);
}
// message and schedule buffers of the challenge hash of a chunk of up to EXPH_MAXP proofs (k_hash.hip: k_exph_*), exph_blocks(W.sec) blocks per proof
static inline void carve_exph(SoaCarver& k, Workspace& W) {
    const size_t blocks = exph_blocks(W.sec), np = std::min<size_t>(W.C, EXPH_MAXP);
    W.exph_msg = (uint8_t*)k.take(np * blocks * 64), W.exph_wk = (uint32_t*)k.take(np * blocks * 256), W.exph_cap = (uint32_t)np;
}
static inline void carve_v_gk_scalars(SoaCarver& k, VWork& V) {
    const size_t C = V.C, n = V.n;
    V.gk_f = k.soa(n * C), V.gk_g = k.soa(n * C);
    V.gk_total = k.soa(C);
    V.gk_csub = (uint32_t*)k.take(gk_etab_range(V.n) ? std::max<size_t>(36 * 256 * C, V.n >= GKM_MINN ? gkm_coef_frag_bytes(V.C) : 0) : 16);
    V.gk_swap = (uint32_t*)k.take(4 * n * C);
}
static inline void carve_v_gk_fold(SoaCarver& k, Soa& res, Soa& res2, uint32_t C, uint32_t n, uint64_t N) {
    const GkVerifyPlan p = gk_verify_plan(C, n, N);
    res = k.soa(p.res), res2 = k.soa(p.res2);
}
// the ring's pointers of a prover workspace, bound on every call (zk_ctx_use_ring, zk_ctx_update_ring, zk_ctx_set_ring_fold, RingBind)
static inline void bind_ring(Workspace& W, const zk_ctx* c) {
    W.ring = Soa{c->ring->ring_mem, (uint32_t)c->ring->N};
    W.gk_etab = c->ring->gk_etab;
    W.gk_kdig = c->gk_mfma ? c->ring->gk_kdig : nullptr;
    W.gk_edig = c->gk_mfma && W.gk_adig ? c->ring->gk_edig : nullptr;
}
