// zk_accountable_prove_batch / zk_accountable_verify_batch / zk_accountable_split_batch / zk_accountable_join_batch (include/zkattest.h): an attestation that
// carries the escrow tag of its own keyXcom, as one "ZKC1" bundle.  Host-side pipeline.  The attestations, the key blinders, the keyXcom extractor and the tags
// run through the internal paths of their own calls, unchanged; the kernels of its own are in k_accountable.hip, the scan of the lengths and the byte mover are
// k_prove_rings.hip's.  A call runs in WINDOWS of at most chunk x lanes bundles: what is not yet at its final place -- a window's attestations and tags, the
// gathered keys, blinders and keyXcoms -- lies in one witness-flagged buffer (c->buf[B_as]) whose size follows the window, not B (DESIGN.md section 5h''').
// The zk_rings_accountable_* calls (include/zkattest_rings_accountable.h; one resident ring id per bundle, DESIGN.md section 5h'''') run the same window
// loops: their attestation step enters the mixed-ring pipelines, their staging follows the largest ring the call names, their out_cap is decided by k_acc_caps
// from the ids alone; the open on bundles moves the tags alone and enters zk_rings_escrow_open_batch_device's internal path.
#include "ctx.h"
#include "jobs.h"
#include "link.h"
#include "escrow.h"
#include "quorum.h"
#include "accountable.h"

static_assert(ZKC_TAG_BYTES == ZKT1_SIZE && ZKC_TAG_MAGIC == ZK_MAGIC_ZKT1, "a bundle's tag is a ZKT1 tag");

extern "C" uint64_t zk_accountable_proof_max_size(const zk_ctx* c) { return c ? zkc_max_size(zk_proof_max_size(c)) : 0; }

// NULL pointers are the caller's to check first.  proving: what the prover and the verifier need beyond the layout calls -- params, a ring, an auditor.
// rings: a `_rings` form, which reads no active ring.
static zk_status acc_refusal(zk_ctx* c, uint64_t B, bool proving, bool rings = false) {
    if (B > 0xffffffffull) return ZK_E_ARG;
    if (proving && (!c->params_set || (!rings && !c->ring->N))) return ZK_E_BUFFER;
    if (proving && !c->auditor_set) {
        c->err = "no auditor key is set (zk_ctx_set_auditor)";
        return ZK_E_BUFFER;
    }
    if (c->stream_busy) return busy_refusal(c);
    return ZK_OK;
}
static uint32_t acc_window(const zk_ctx* c) { return window_rows(c, 1); }   // bundles per window
static size_t acc_rng_row(const zk_rng& r) { return rng_row_bytes(r); }
using AccTiming = PipelineTiming;   // (jobs.h)
// the offsets of a _device call on the host: one read-back
static zk_status acc_offsets(zk_ctx* c, uint64_t B, const uint64_t* d_off, std::vector<uint64_t>& copy, const uint64_t*& h_off) {
    if (h_off) return ZK_OK;
    copy.resize(B + 1);
    HIPCHK(c, hipMemcpy(copy.data(), d_off, 8 * (B + 1), hipMemcpyDeviceToHost));
    h_off = copy.data();
    return ZK_OK;
}

// The `_rings` forms (one resident ring id per bundle, DESIGN.md section 5h''''): what a call's ids come to, by accountable_plan.h's rule over quorum_plan.h's table
static const uint32_t acc_no_ids[1] = {0};   // a `_rings` call of B = 0 may pass no ids and reads none
struct AccCaps {
    uint64_t total;       // the sum of the bundles' slots: what out_cap is held against
    uint64_t proof_max;   // the largest proof of the rings the ids name: a window's attestation staging follows it
};
extern "C" uint64_t zk_rings_accountable_proof_max_size(const zk_ctx* c, uint32_t ring_id) {
    if (!c || !c->params_set) return 0;
    QuorumRings R;
    quorum_rings_table(c, R);
    return zkc_capacity_rings(R, ring_id, nullptr);
}
static AccCaps acc_caps_host(const zk_ctx* c, uint64_t B, const uint32_t* ids) {
    QuorumRings R;
    quorum_rings_table(c, R);
    uint32_t used = 0;
    const uint64_t total = zkc_capacity_total(R, B, ids, &used);
    return {total, quorum_largest(R, used)};
}
// ids on the device: one kernel, ONE read-back (the total and the set of named entries, next to each other in c->buf[B_qc])
static zk_status acc_caps_device(zk_ctx* c, uint64_t B, const uint32_t* d_ids, AccCaps& caps) {
    QuorumRings R;
    quorum_rings_table(c, R);
    if (!zkc_capacity_fits(R, B)) {   // no buffer holds it: the kernel's sum is not asked to represent it
        caps = {~0ull, 0};
        return ZK_OK;
    }
    if (zk_status zs = reserve(c, B_qc, 16)) return zs;
    uint64_t* const d_tot = (uint64_t*)c->buf[B_qc].p;
    uint64_t h[2] = {0, 0};
    HIPCHK(c, hipMemsetAsync(d_tot, 0, 16, c->stream));
    launch_acc_caps(c->stream, (uint32_t)B, d_ids, R, d_tot);
    HIPCHK(c, hipMemcpyAsync(h, d_tot, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    caps = {h[0], quorum_largest(R, (uint32_t)h[1])};
    return ZK_OK;
}

// ------------------------------------------------------------------ prover
struct AccProveWin {
    uint8_t *key, *blinder, *com, *stage;
    uint64_t *w_off, *len, *rec_off, *rec_len, *rec_dst;
    int32_t *w_st, *kc_st, *tag_st;
    uint64_t tag_stage;   // where the window's tags start in `stage`
};
static size_t acc_prove_layout(AccProveWin& W, uint8_t* base, size_t n, uint64_t proof_max) {
    Carver c(base);
    W.key = (uint8_t*)c.take(32 * n), W.blinder = (uint8_t*)c.take(32 * n), W.com = (uint8_t*)c.take(72 * n);
    W.w_off = (uint64_t*)c.take(8 * (n + 1)), W.len = (uint64_t*)c.take(8 * n);
    W.rec_off = (uint64_t*)c.take(16 * n), W.rec_len = (uint64_t*)c.take(16 * n), W.rec_dst = (uint64_t*)c.take(16 * n);
    W.w_st = (int32_t*)c.take(4 * n), W.kc_st = (int32_t*)c.take(4 * n), W.tag_st = (int32_t*)c.take(4 * n);
    W.tag_stage = n * proof_max;
    W.stage = (uint8_t*)c.take(W.tag_stage + n * ZKC_TAG_BYTES);
    return c.off + ZK_LAYOUT_TAIL;
}
struct AccProveIo {   // device pointers
    const uint8_t *msg, *sig, *pk;
    const uint32_t* which;
    uint8_t* out;
    uint64_t* out_off;
    int32_t *status, *part_status;
    const uint32_t* ids;   // the `_rings` forms: one resident ring id per bundle; nullptr: the active ring
};
// known: the host-pointer `_rings` form has the ids on the host and has decided already
static zk_status acc_prove_device(zk_ctx* c, uint64_t B, const AccProveIo& io, const zk_rng& rng, const zk_rng& rng_tags, uint64_t out_cap, const AccCaps* known = nullptr) {
    if (zk_status zs = acc_refusal(c, B, true, io.ids != nullptr)) return zs;
    if (!rng_mode_ok(&rng) || !rng_mode_ok(&rng_tags)) return ZK_E_ARG;
    hipStream_t s = c->stream;
    if (B == 0) {
        if (!words_aligned({io.out_off})) return ZK_E_ARG;
        HIPCHK(c, hipMemsetAsync(io.out_off, 0, 8, s));
        HIPCHK(c, hipStreamSynchronize(s));
        return ZK_OK;
    }
    AccCaps caps{0, io.ids ? 0 : zk_proof_max_size(c)};
    AccTiming T{c, zk_timed(c, B)};
    if (known) caps = *known;
    else if (io.ids) {   // from the ids alone, before a byte of any output is written
        if (!words_aligned({io.ids})) return ZK_E_ARG;
        if (zk_status zs = T.phase("accountable_caps", [&] { return acc_caps_device(c, B, io.ids, caps); })) return zs;
    }
    const uint64_t proof_max = caps.proof_max;
    if (io.ids ? out_cap < caps.total : out_cap / zkc_max_size(proof_max) < B) {   // before a byte of any output is written
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    if (!words_aligned({io.msg, io.sig, io.pk, io.which, io.out, io.out_off, io.status, io.part_status, rng.data, rng_tags.data})) return ZK_E_ARG;
    const uint32_t Wn = (uint32_t)std::min<uint64_t>(B, acc_window(c));
    AccProveWin W;
    if (zk_status zs = lay_out(c, B_as, [&](uint8_t* base) { return acc_prove_layout(W, base, Wn, proof_max); })) return zs;
    const Wire wire = wire_make(c->wire == ZK_WIRE_ZKA1P);
    uint64_t base = 0;   // bytes of the finished windows: where this window's bundles start in `out`
    for (uint64_t b0 = 0; b0 < B; b0 += Wn) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(Wn, B - b0);
        const zk_rng rng_w{rng.mode, rng.data + acc_rng_row(rng) * b0, rng.stride_blocks}, rng_t{rng_tags.mode, rng_tags.data + acc_rng_row(rng_tags) * b0, rng_tags.stride_blocks};
        // the attestations, back to back in the staging area
        if (zk_status zs = io.ids ? zkq_prove_members_rings(c, n, io.msg + 32 * b0, io.sig + 64 * b0, io.pk + 64 * b0, io.which + b0, io.ids + b0, rng_w, W.stage, W.tag_stage,
                                                            W.w_off, W.w_st)
                                  : zkq_prove_members(c, n, io.msg + 32 * b0, io.sig + 64 * b0, io.pk + 64 * b0, io.which + b0, rng_w, W.stage, W.tag_stage, W.w_off, W.w_st))
            return zs;
        T.absorb();
        // the blinders of their keyXcoms (a stream too short for draw 1 is that attestation's own status already), the keys, the keyXcoms themselves
        if (zk_status zs = T.phase("accountable_blinders", [&]() -> zk_status {
                const zk_status zb = zkq_key_blinders(c, n, rng_w, W.blinder);
                if (zb && zb != ZK_E_RNG_EXHAUSTED) return zb;
                launch_acc_keys(s, n, io.pk + 64 * b0, W.key);
                launch_link_keycoms(s, n, W.stage, W.w_off, wire, W.com, W.kc_st);
                return ZK_OK;
            }))
            return zs;
        // the tags, at 472 b behind the attestations
        if (zk_status zs = zkc_escrow_prove(c, n, W.key, W.com, W.blinder, rng_t, W.stage + W.tag_stage, W.tag_st)) return zs;
        T.absorb();
        // statuses and lengths, the scan, headers and records, the bytes; the host takes the window's end as the next window's base
        if (zk_status zs = T.phase("accountable_layout", [&] {
                launch_acc_fold_prove(s, n, W.w_off, W.w_st, W.tag_st, io.status + b0, io.part_status ? io.part_status + 2 * b0 : nullptr, W.len);
                launch_pr_offsets(s, n, W.len, base, io.out_off + b0);
                launch_acc_place(s, n, W.w_off, W.len, W.tag_stage, io.out_off + b0, io.out, W.rec_off, W.rec_len, W.rec_dst);
                launch_pr_move(s, 2 * n, W.rec_off, W.rec_len, W.stage, W.rec_dst, io.out);
                HIPCHK(c, hipMemcpyAsync(&base, io.out_off + b0 + n, 8, hipMemcpyDeviceToHost, s));
                return ZK_OK;
            }))
            return zs;
    }
    T.publish();
    return ZK_OK;
}
extern "C" zk_status zk_accountable_prove_batch_device(zk_ctx* c, uint64_t B, const void* d_msg, const void* d_sig, const void* d_pk, const void* d_which, const zk_rng* rng,
                                                       const zk_rng* rng_tags, void* d_out, uint64_t out_cap, void* d_out_off, void* d_status, void* d_part_status) {
    if (!c || !rng || !rng_tags || !d_out_off || (B && (!d_msg || !d_sig || !d_pk || !d_which || !rng->data || !rng_tags->data || !d_out || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const zk_status zs = acc_prove_device(c, B, {(const uint8_t*)d_msg, (const uint8_t*)d_sig, (const uint8_t*)d_pk, (const uint32_t*)d_which, (uint8_t*)d_out, (uint64_t*)d_out_off,
                                                 (int32_t*)d_status, (int32_t*)d_part_status}, *rng, *rng_tags, out_cap);
    if (zs && c->params_set && !c->stream_busy) wipe_witness(c);   // a failed call leaves no gathered key or blinder, nonce or RNG block behind
    return zs;
}
extern "C" zk_status zk_rings_accountable_prove_batch_device(zk_ctx* c, uint64_t B, const void* d_msg, const void* d_sig, const void* d_pk, const void* d_which,
                                                             const void* d_ring_ids, const zk_rng* rng, const zk_rng* rng_tags, void* d_out, uint64_t out_cap, void* d_out_off,
                                                             void* d_status, void* d_part_status) {
    if (!c || !rng || !rng_tags || !d_out_off || (B && (!d_msg || !d_sig || !d_pk || !d_which || !d_ring_ids || !rng->data || !rng_tags->data || !d_out || !d_status)))
        return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const zk_status zs = acc_prove_device(c, B, {(const uint8_t*)d_msg, (const uint8_t*)d_sig, (const uint8_t*)d_pk, (const uint32_t*)d_which, (uint8_t*)d_out, (uint64_t*)d_out_off,
                                                 (int32_t*)d_status, (int32_t*)d_part_status, d_ring_ids ? (const uint32_t*)d_ring_ids : acc_no_ids}, *rng, *rng_tags, out_cap);
    if (zs && c->params_set && !c->stream_busy) wipe_witness(c);   // ... nor a gathered per-ring window
    return zs;
}
// Host pointers: the inputs and both seed sets through the context's witness-flagged input buffer, the bundles through its output staging buffer.
struct AccProveIn {
    uint8_t *msg, *sig, *pk, *rng, *rng_tags;
    uint32_t *which, *ids;   // ids: the `_rings` form only
    uint64_t* off;
    int32_t *st, *pst;
};
static size_t acc_prove_in_layout(AccProveIn& I, uint8_t* base, size_t B, size_t rng_b, size_t rng_tags_b, bool ids) {
    Carver k(base);
    I.msg = (uint8_t*)k.take(32 * B), I.sig = (uint8_t*)k.take(64 * B), I.pk = (uint8_t*)k.take(64 * B), I.which = (uint32_t*)k.take(4 * B);
    I.ids = ids ? (uint32_t*)k.take(4 * B) : nullptr;
    I.rng = (uint8_t*)k.take(rng_b ? rng_b : 32), I.rng_tags = (uint8_t*)k.take(rng_tags_b ? rng_tags_b : 32);
    I.off = (uint64_t*)k.take(8 * (B + 1)), I.st = (int32_t*)k.take(4 * B), I.pst = (int32_t*)k.take(8 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
// ids: the `_rings` form (the slots come from the ids here on the host, by the rule the kernel uses); nullptr: the active ring
static zk_status acc_prove_host(zk_ctx* c, uint64_t B, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk, const uint32_t* which, const uint32_t* ids, const zk_rng* rng,
                                const zk_rng* rng_tags, uint8_t* out, uint64_t out_cap, uint64_t* out_off, int32_t* status, int32_t* part_status) {
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = acc_refusal(c, B, true, ids != nullptr)) return zs;
    if (!rng_mode_ok(rng) || !rng_mode_ok(rng_tags)) return ZK_E_ARG;
    if (B == 0) {
        out_off[0] = 0;
        return ZK_OK;
    }
    const uint64_t need = ids ? 0 : zkc_max_size(zk_proof_max_size(c));
    const AccCaps caps = ids ? acc_caps_host(c, B, ids) : AccCaps{B * need, 0};
    if (ids ? out_cap < caps.total : out_cap / need < B) {   // before a byte of any output is written
        c->err = "output buffer too small";
        wipe_witness(c);
        return ZK_E_BUFFER;
    }
    AccProveIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return acc_prove_in_layout(I, base, B, rng_bytes(rng, B), rng_bytes(rng_tags, B), ids != nullptr); })) return zs;
    if (zk_status zs = reserve(c, B_io, caps.total)) return zs;
    uint8_t* const d_out = (uint8_t*)c->buf[B_io].p;
    // from the first upload on, signatures and seeds lie in the input buffer: every failure below zeroes them
    if (zk_status zs = upload_or_wipe(c, {{I.msg, msg, 32 * B}, {I.sig, sig, 64 * B}, {I.pk, pk, 64 * B}, {I.which, which, 4 * B}, {I.ids, ids, ids ? 4 * B : 0},
                                          {I.rng, rng->data, rng_bytes(rng, B)}, {I.rng_tags, rng_tags->data, rng_bytes(rng_tags, B)}}))
        return zs;
    if (zk_status zs = acc_prove_device(c, B, {I.msg, I.sig, I.pk, I.which, d_out, I.off, I.st, I.pst, I.ids}, zk_rng{rng->mode, I.rng, rng->stride_blocks},
                                        zk_rng{rng_tags->mode, I.rng_tags, rng_tags->stride_blocks}, caps.total, ids ? &caps : nullptr)) {
        wipe_witness(c);
        return zs;
    }
    if (zk_status zs = download_or_wipe(c, {{I.off, out_off, 8 * (B + 1)}, {I.st, status, 4 * B}, {I.pst, part_status, part_status ? 8 * B : 0}})) return zs;
    return download_or_wipe(c, {{d_out, out, out_off[B]}});
}
extern "C" zk_status zk_accountable_prove_batch(zk_ctx* c, uint64_t B, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk, const uint32_t* which, const zk_rng* rng,
                                                const zk_rng* rng_tags, uint8_t* out, uint64_t out_cap, uint64_t* out_off, int32_t* status, int32_t* part_status) {
    if (!c || !rng || !rng_tags || !out_off || (B && (!msg || !sig || !pk || !which || !rng->data || !rng_tags->data || !out || !status))) return ZK_E_ARG;
    return acc_prove_host(c, B, msg, sig, pk, which, nullptr, rng, rng_tags, out, out_cap, out_off, status, part_status);
}
extern "C" zk_status zk_rings_accountable_prove_batch(zk_ctx* c, uint64_t B, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk, const uint32_t* which,
                                                      const uint32_t* ring_ids, const zk_rng* rng, const zk_rng* rng_tags, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                                                      int32_t* status, int32_t* part_status) {
    if (!c || !rng || !rng_tags || !out_off || (B && (!msg || !sig || !pk || !which || !ring_ids || !rng->data || !rng_tags->data || !out || !status))) return ZK_E_ARG;
    return acc_prove_host(c, B, msg, sig, pk, which, ring_ids ? ring_ids : acc_no_ids, rng, rng_tags, out, out_cap, out_off, status, part_status);
}

// ------------------------------------------------------------------ verifier
struct AccWalkWin {   // what the walk leaves per bundle (verifier, split and join)
    uint8_t* good;
    uint64_t *a_src, *a_len, *t_src, *t_len, *t_dst, *len, *rec_off, *rec_len, *rec_dst;
};
static void acc_walk_carve(AccWalkWin& W, Carver& c, size_t n) {
    W.good = (uint8_t*)c.take(n);
    W.a_src = (uint64_t*)c.take(8 * n), W.a_len = (uint64_t*)c.take(8 * n), W.t_src = (uint64_t*)c.take(8 * n), W.t_len = (uint64_t*)c.take(8 * n);
    W.t_dst = (uint64_t*)c.take(8 * n), W.len = (uint64_t*)c.take(8 * n);
    W.rec_off = (uint64_t*)c.take(16 * n), W.rec_len = (uint64_t*)c.take(16 * n), W.rec_dst = (uint64_t*)c.take(16 * n);
}
struct AccVerifyWin {
    AccWalkWin k;
    uint8_t *com, *a_ok, *t_ok, *stage_att, *stage_tags;
    uint64_t* s_off;
    int32_t *kc_st, *a_st, *t_st;
};
static size_t acc_verify_layout(AccVerifyWin& W, uint8_t* base, size_t n, uint64_t att_bytes) {
    Carver c(base);
    acc_walk_carve(W.k, c, n);
    W.com = (uint8_t*)c.take(72 * n), W.a_ok = (uint8_t*)c.take(n), W.t_ok = (uint8_t*)c.take(n);
    W.s_off = (uint64_t*)c.take(8 * (n + 1));
    W.kc_st = (int32_t*)c.take(4 * n), W.a_st = (int32_t*)c.take(4 * n), W.t_st = (int32_t*)c.take(4 * n);
    W.stage_att = (uint8_t*)c.take(att_bytes + 64), W.stage_tags = (uint8_t*)c.take(n * ZKC_TAG_BYTES);
    return c.off + ZK_LAYOUT_TAIL;
}
// the largest window's attestations, from the offsets alone (only a slot the walk can accept is moved, and never its header or tag)
static uint64_t acc_window_att_bytes(uint64_t B, uint32_t Wn, const uint64_t* h_off) {
    uint64_t most = 0;
    for (uint64_t b0 = 0; b0 < B; b0 += Wn) {
        uint64_t sum = 0;
        for (uint64_t b = b0; b < std::min<uint64_t>(B, b0 + Wn); b++) sum += zkc_slot_att_bytes(h_off[b], h_off[b + 1]);
        most = std::max(most, sum);
    }
    return most;
}
struct AccVerifyIo {   // device pointers
    const uint8_t *msg, *bundles;
    const uint64_t* off;
    const uint8_t* vseeds;
    uint8_t* ok;
    int32_t* status;
    uint32_t* first_bad;
    const uint32_t* ids;   // the `_rings` forms: one resident ring id per bundle; nullptr: the active ring
};
// h_off: the offsets on the host (the device form reads them back once) -- a window's staging is as large as the slots it may move
static zk_status acc_verify_device(zk_ctx* c, uint64_t B, const AccVerifyIo& io, const uint64_t* h_off) {
    if (zk_status zs = acc_refusal(c, B, true, io.ids != nullptr)) return zs;
    if (B == 0) return ZK_OK;
    if (!words_aligned({io.msg, io.bundles, io.off, io.vseeds, io.ok, io.status, io.first_bad, io.ids})) return ZK_E_ARG;
    hipStream_t s = c->stream;
    std::vector<uint64_t> off_copy;
    if (zk_status zs = acc_offsets(c, B, io.off, off_copy, h_off)) return zs;
    const uint32_t Wn = (uint32_t)std::min<uint64_t>(B, acc_window(c));
    AccVerifyWin W;
    if (zk_status zs = lay_out(c, B_as, [&](uint8_t* base) { return acc_verify_layout(W, base, Wn, acc_window_att_bytes(B, Wn, h_off)); })) return zs;
    const Wire wire = wire_make(c->wire == ZK_WIRE_ZKA1P);
    AccTiming T{c, zk_timed(c, B)};
    for (uint64_t b0 = 0; b0 < B; b0 += Wn) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(Wn, B - b0);
        // the headers; the attestations back to back and the tags at 472 b in the staging area (a refused bundle's tag: zero bytes); the keyXcoms
        if (zk_status zs = T.phase("accountable_walk", [&] {
                launch_acc_walk(s, n, io.bundles, io.off + b0, nullptr, wire, W.k.good, W.k.a_src, W.k.a_len, W.k.t_src, W.k.t_len, W.k.t_dst, nullptr, nullptr);
                launch_pr_offsets(s, n, W.k.a_len, 0, W.s_off);
                launch_pr_move(s, n, W.k.a_src, W.k.a_len, io.bundles, W.s_off, W.stage_att);
                HIPCHK(c, hipMemsetAsync(W.stage_tags, 0, (size_t)n * ZKC_TAG_BYTES, s));
                launch_pr_move(s, n, W.k.t_src, W.k.t_len, io.bundles, W.k.t_dst, W.stage_tags);
                launch_link_keycoms(s, n, W.stage_att, W.s_off, wire, W.com, W.kc_st);
                return ZK_OK;
            }))
            return zs;
        const uint8_t* const seeds_w = io.vseeds ? io.vseeds + 32 * b0 : nullptr;
        if (zk_status zs = io.ids ? zkq_verify_members_rings(c, n, io.msg + 32 * b0, W.stage_att, W.s_off, io.ids + b0, seeds_w, W.a_ok, W.a_st)
                                  : zkq_verify_members(c, n, io.msg + 32 * b0, W.stage_att, W.s_off, seeds_w, W.a_ok, W.a_st))
            return zs;
        T.absorb();
        if (zk_status zs = zkc_escrow_verify(c, n, W.com, W.stage_tags, W.t_ok, W.t_st)) return zs;
        T.absorb();
        if (zk_status zs = T.phase("accountable_verdict", [&] {
                launch_acc_verdict(s, n, W.k.good, W.a_ok, W.a_st, W.t_ok, W.t_st, io.ok + b0, io.status + b0, io.first_bad ? io.first_bad + b0 : nullptr);
                return ZK_OK;
            }))
            return zs;
    }
    T.publish();
    return ZK_OK;
}
extern "C" zk_status zk_accountable_verify_batch_device(zk_ctx* c, uint64_t B, const void* d_msg, const void* d_bundles, const void* d_bundle_off, const void* d_vseeds, void* d_ok,
                                                        void* d_status, void* d_first_bad) {
    if (!c || (B && (!d_msg || !d_bundles || !d_bundle_off || !d_ok || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return acc_verify_device(c, B, {(const uint8_t*)d_msg, (const uint8_t*)d_bundles, (const uint64_t*)d_bundle_off, (const uint8_t*)d_vseeds, (uint8_t*)d_ok, (int32_t*)d_status,
                                    (uint32_t*)d_first_bad}, nullptr);
}
extern "C" zk_status zk_rings_accountable_verify_batch_device(zk_ctx* c, uint64_t B, const void* d_msg, const void* d_bundles, const void* d_bundle_off, const void* d_ring_ids,
                                                              const void* d_vseeds, void* d_ok, void* d_status, void* d_first_bad) {
    if (!c || (B && (!d_msg || !d_bundles || !d_bundle_off || !d_ring_ids || !d_ok || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return acc_verify_device(c, B, {(const uint8_t*)d_msg, (const uint8_t*)d_bundles, (const uint64_t*)d_bundle_off, (const uint8_t*)d_vseeds, (uint8_t*)d_ok, (int32_t*)d_status,
                                    (uint32_t*)d_first_bad, d_ring_ids ? (const uint32_t*)d_ring_ids : acc_no_ids}, nullptr);
}
// the end of the last slot a byte of which may be read
static uint64_t acc_readable_end(uint64_t B, const uint64_t* off) {
    uint64_t bytes = 0;
    for (uint64_t b = 0; b < B; b++)
        if (rr_slot_readable(off[b], off[b + 1])) bytes = std::max(bytes, off[b + 1]);
    return bytes;
}
struct AccVerifyIn {   // no witness is staged: a failing copy returns as it is
    uint8_t *msg, *seeds, *ok;
    uint64_t* off;
    int32_t* st;
    uint32_t *bad, *ids;   // ids: the `_rings` form only
};
static size_t acc_verify_in_layout(AccVerifyIn& I, uint8_t* base, size_t B, bool seeds, bool ids) {
    Carver k(base);
    I.msg = (uint8_t*)k.take(32 * B), I.seeds = (uint8_t*)k.take(seeds ? 32 * B : 32), I.off = (uint64_t*)k.take(8 * (B + 1));
    I.ids = ids ? (uint32_t*)k.take(4 * B) : nullptr;
    I.ok = (uint8_t*)k.take(B), I.st = (int32_t*)k.take(4 * B), I.bad = (uint32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
static zk_status acc_verify_host(zk_ctx* c, uint64_t B, const uint8_t* msg, const uint8_t* bundles, const uint64_t* bundle_off, const uint32_t* ids, const uint8_t* vseeds,
                                 uint8_t* ok, int32_t* status, uint32_t* first_bad) {
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = acc_refusal(c, B, true, ids != nullptr)) return zs;
    if (B == 0) return ZK_OK;
    const uint64_t bytes = acc_readable_end(B, bundle_off);
    AccVerifyIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return acc_verify_in_layout(I, base, B, vseeds != nullptr, ids != nullptr); })) return zs;
    if (zk_status zs = reserve(c, B_io, bytes + 64)) return zs;
    uint8_t* const d_bundles = (uint8_t*)c->buf[B_io].p;
    HIPCHK(c, hipMemcpy(I.msg, msg, 32 * B, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(I.off, bundle_off, 8 * (B + 1), hipMemcpyHostToDevice));
    if (bytes) HIPCHK(c, hipMemcpy(d_bundles, bundles, bytes, hipMemcpyHostToDevice));
    if (vseeds) HIPCHK(c, hipMemcpy(I.seeds, vseeds, 32 * B, hipMemcpyHostToDevice));
    if (ids) HIPCHK(c, hipMemcpy(I.ids, ids, 4 * B, hipMemcpyHostToDevice));
    if (zk_status zs = acc_verify_device(c, B, {I.msg, d_bundles, I.off, vseeds ? I.seeds : nullptr, I.ok, I.st, I.bad, I.ids}, bundle_off)) return zs;
    HIPCHK(c, hipMemcpy(ok, I.ok, B, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(status, I.st, 4 * B, hipMemcpyDeviceToHost));
    if (first_bad) HIPCHK(c, hipMemcpy(first_bad, I.bad, 4 * B, hipMemcpyDeviceToHost));
    return ZK_OK;
}
extern "C" zk_status zk_accountable_verify_batch(zk_ctx* c, uint64_t B, const uint8_t* msg, const uint8_t* bundles, const uint64_t* bundle_off, const uint8_t* vseeds, uint8_t* ok,
                                                 int32_t* status, uint32_t* first_bad) {
    if (!c || (B && (!msg || !bundles || !bundle_off || !ok || !status))) return ZK_E_ARG;
    return acc_verify_host(c, B, msg, bundles, bundle_off, nullptr, vseeds, ok, status, first_bad);
}
extern "C" zk_status zk_rings_accountable_verify_batch(zk_ctx* c, uint64_t B, const uint8_t* msg, const uint8_t* bundles, const uint64_t* bundle_off, const uint32_t* ring_ids,
                                                       const uint8_t* vseeds, uint8_t* ok, int32_t* status, uint32_t* first_bad) {
    if (!c || (B && (!msg || !bundles || !bundle_off || !ring_ids || !ok || !status))) return ZK_E_ARG;
    return acc_verify_host(c, B, msg, bundles, bundle_off, ring_ids ? ring_ids : acc_no_ids, vseeds, ok, status, first_bad);
}

// ------------------------------------------------------------------ the open: the auditor's call on bundles (the `_rings` forms only)
// Per window: the walk; the tags -- and nothing else -- to 472 b of the staging area (a refused bundle's: zero bytes); the opener of zk_rings_escrow_open_batch on
// them, into the window's own (status, ring, index); the fold into the caller's arrays.  A secret that is not the auditor key's ends the call in its first
// window, before the first fold: nothing of the caller's is written.
struct AccOpenWin {
    uint8_t *good, *tags;
    uint64_t *a_src, *a_len, *t_src, *t_len, *t_dst;
    uint32_t *o_ring, *o_index;
    int32_t* o_st;
};
static size_t acc_open_layout(AccOpenWin& W, uint8_t* base, size_t n) {
    Carver c(base);
    W.good = (uint8_t*)c.take(n);
    W.a_src = (uint64_t*)c.take(8 * n), W.a_len = (uint64_t*)c.take(8 * n), W.t_src = (uint64_t*)c.take(8 * n), W.t_len = (uint64_t*)c.take(8 * n), W.t_dst = (uint64_t*)c.take(8 * n);
    W.o_ring = (uint32_t*)c.take(4 * n), W.o_index = (uint32_t*)c.take(4 * n), W.o_st = (int32_t*)c.take(4 * n);
    W.tags = (uint8_t*)c.take(n * ZKC_TAG_BYTES);
    return c.off + ZK_LAYOUT_TAIL;
}
static zk_status acc_open_device(zk_ctx* c, uint64_t B, const uint8_t* secret, const uint8_t* bundles, const uint64_t* off, const uint32_t* ids, uint32_t* ring_out,
                                 uint32_t* index, int32_t* status) {
    if (zk_status zs = acc_refusal(c, B, true, true)) return zs;
    if (B == 0) return ZK_OK;
    if (!words_aligned({secret, bundles, off, ids, ring_out, index, status})) return ZK_E_ARG;
    hipStream_t s = c->stream;
    const uint32_t Wn = (uint32_t)std::min<uint64_t>(B, acc_window(c));
    AccOpenWin W;
    if (zk_status zs = lay_out(c, B_as, [&](uint8_t* base) { return acc_open_layout(W, base, Wn); })) return zs;
    const Wire wire = wire_make(c->wire == ZK_WIRE_ZKA1P);
    AccTiming T{c, zk_timed(c, B)};
    for (uint64_t b0 = 0; b0 < B; b0 += Wn) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(Wn, B - b0);
        if (zk_status zs = T.phase("accountable_walk", [&] {
                launch_acc_walk(s, n, bundles, off + b0, nullptr, wire, W.good, W.a_src, W.a_len, W.t_src, W.t_len, W.t_dst, nullptr, nullptr);
                HIPCHK(c, hipMemsetAsync(W.tags, 0, (size_t)n * ZKC_TAG_BYTES, s));
                launch_pr_move(s, n, W.t_src, W.t_len, bundles, W.t_dst, W.tags);
                return ZK_OK;
            }))
            return zs;
        // The opener is entered once per window: each time it checks the secret (a g, a blocking 72-byte copy to the host, a compare) and lists the rings again.
        // That blocking copy is also what orders the tags staged above on c->stream before the opener's lanes, as in zk_rings_escrow_open_batch_device itself.
        if (zk_status zs = zkc_rings_escrow_open(c, n, secret, W.tags, ids + b0, W.o_ring, W.o_index, W.o_st)) return zs;
        T.absorb();
        if (zk_status zs = T.phase("accountable_verdict", [&] {
                launch_acc_fold_open(s, n, W.good, W.o_st, W.o_ring, W.o_index, ring_out + b0, index + b0, status + b0);
                return ZK_OK;
            }))
            return zs;
    }
    T.publish();
    return ZK_OK;
}
extern "C" zk_status zk_rings_accountable_open_batch_device(zk_ctx* c, uint64_t B, const void* d_secret, const void* d_bundles, const void* d_bundle_off, const void* d_ring_ids,
                                                            void* d_ring_out, void* d_index, void* d_status) {
    if (!c || !d_secret || (B && (!d_bundles || !d_bundle_off || !d_ring_ids || !d_ring_out || !d_index || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const zk_status zs = acc_open_device(c, B, (const uint8_t*)d_secret, (const uint8_t*)d_bundles, (const uint64_t*)d_bundle_off, (const uint32_t*)d_ring_ids, (uint32_t*)d_ring_out,
                                         (uint32_t*)d_index, (int32_t*)d_status);
    if (zs && zs != ZK_E_OPENING && c->params_set && !c->stream_busy) wipe_witness(c);   // (the opener has wiped already where the secret was refused)
    return zs;
}
struct AccOpenIn {   // the secret is staged in the witness-flagged input buffer: every failure behind its upload zeroes it
    uint8_t* secret;
    uint64_t* off;
    uint32_t *ids, *ring, *index;
    int32_t* st;
};
static size_t acc_open_in_layout(AccOpenIn& I, uint8_t* base, size_t B) {
    Carver k(base);
    I.secret = (uint8_t*)k.take(32), I.off = (uint64_t*)k.take(8 * (B + 1));
    I.ids = (uint32_t*)k.take(4 * B), I.ring = (uint32_t*)k.take(4 * B), I.index = (uint32_t*)k.take(4 * B), I.st = (int32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_rings_accountable_open_batch(zk_ctx* c, uint64_t B, const uint8_t secret_be32[32], const uint8_t* bundles, const uint64_t* bundle_off,
                                                     const uint32_t* ring_ids, uint32_t* ring_out_u32, uint32_t* index_u32, int32_t* status) {
    if (!c || !secret_be32 || (B && (!bundles || !bundle_off || !ring_ids || !ring_out_u32 || !index_u32 || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = acc_refusal(c, B, true, true)) return zs;
    if (B == 0) return ZK_OK;
    const uint64_t bytes = acc_readable_end(B, bundle_off);
    AccOpenIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return acc_open_in_layout(I, base, B); })) return zs;
    if (zk_status zs = reserve(c, B_io, bytes + 64)) return zs;
    uint8_t* const d_bundles = (uint8_t*)c->buf[B_io].p;
    if (zk_status zs = upload_or_wipe(c, {{I.secret, secret_be32, 32}, {I.off, bundle_off, 8 * (B + 1)}, {I.ids, ring_ids, 4 * B}, {d_bundles, bundles, bytes}})) return zs;
    if (zk_status zs = acc_open_device(c, B, I.secret, d_bundles, I.off, I.ids, I.ring, I.index, I.st)) {
        wipe_witness(c);
        return zs;
    }
    return download_or_wipe(c, {{I.ring, ring_out_u32, 4 * B}, {I.index, index_u32, 4 * B}, {I.st, status, 4 * B}});
}

// ------------------------------------------------------------------ split and join: pure layout
static size_t acc_walk_layout(AccWalkWin& W, uint8_t* base, size_t n) {
    Carver c(base);
    acc_walk_carve(W, c, n);
    return c.off + ZK_LAYOUT_TAIL;
}
static zk_status acc_split_device(zk_ctx* c, uint64_t B, const uint8_t* bundles, const uint64_t* off, uint8_t* att_out, uint64_t att_cap, uint64_t* att_off, uint8_t* tags_out,
                                  int32_t* status, const uint64_t* h_off) {
    if (zk_status zs = acc_refusal(c, B, false)) return zs;
    hipStream_t s = c->stream;
    if (B == 0) {
        if (!words_aligned({att_off})) return ZK_E_ARG;
        HIPCHK(c, hipMemsetAsync(att_off, 0, 8, s));
        HIPCHK(c, hipStreamSynchronize(s));
        return ZK_OK;
    }
    if (!words_aligned({bundles, off, att_out, att_off, tags_out, status})) return ZK_E_ARG;
    std::vector<uint64_t> off_copy;
    if (zk_status zs = acc_offsets(c, B, off, off_copy, h_off)) return zs;
    uint64_t need = 0;   // what the attestations can come to, from the offsets alone: before a byte of any output is written
    for (uint64_t b = 0; b < B; b++) need += zkc_slot_att_bytes(h_off[b], h_off[b + 1]);
    if (att_cap < need) {
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    const uint32_t Wn = (uint32_t)std::min<uint64_t>(B, acc_window(c));
    AccWalkWin W;
    if (zk_status zs = lay_out(c, B_as, [&](uint8_t* base) { return acc_walk_layout(W, base, Wn); })) return zs;
    const Wire wire = wire_make(c->wire == ZK_WIRE_ZKA1P);
    AccTiming T{c, zk_timed(c, B)};
    uint64_t base = 0;
    for (uint64_t b0 = 0; b0 < B; b0 += Wn) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(Wn, B - b0);
        if (zk_status zs = T.phase("accountable_walk", [&] {
                launch_acc_walk(s, n, bundles, off + b0, nullptr, wire, W.good, W.a_src, W.a_len, W.t_src, W.t_len, W.t_dst, nullptr, status + b0);
                launch_pr_offsets(s, n, W.a_len, base, att_off + b0);
                launch_pr_move(s, n, W.a_src, W.a_len, bundles, att_off + b0, att_out);
                HIPCHK(c, hipMemsetAsync(tags_out + b0 * ZKC_TAG_BYTES, 0, (size_t)n * ZKC_TAG_BYTES, s));
                launch_pr_move(s, n, W.t_src, W.t_len, bundles, W.t_dst, tags_out + b0 * ZKC_TAG_BYTES);
                HIPCHK(c, hipMemcpyAsync(&base, att_off + b0 + n, 8, hipMemcpyDeviceToHost, s));
                return ZK_OK;
            }))
            return zs;
    }
    T.publish();
    return ZK_OK;
}
extern "C" zk_status zk_accountable_split_batch_device(zk_ctx* c, uint64_t B, const void* d_bundles, const void* d_bundle_off, void* d_att_out, uint64_t att_cap, void* d_att_off,
                                                       void* d_tags_out, void* d_status) {
    if (!c || !d_att_off || (B && (!d_bundles || !d_bundle_off || !d_att_out || !d_tags_out || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return acc_split_device(c, B, (const uint8_t*)d_bundles, (const uint64_t*)d_bundle_off, (uint8_t*)d_att_out, att_cap, (uint64_t*)d_att_off, (uint8_t*)d_tags_out,
                            (int32_t*)d_status, nullptr);
}
struct AccLayoutIn {   // the host-pointer forms of split and join: the offsets in, the offsets and statuses out (nothing witness-derived)
    uint64_t *off, *out_off;
    int32_t* st;
};
static size_t acc_layout_in_layout(AccLayoutIn& I, uint8_t* base, size_t B) {
    Carver k(base);
    I.off = (uint64_t*)k.take(8 * (B + 1)), I.out_off = (uint64_t*)k.take(8 * (B + 1)), I.st = (int32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
static uint64_t acc_round64(uint64_t v) { return (v + 63) & ~63ull; }
extern "C" zk_status zk_accountable_split_batch(zk_ctx* c, uint64_t B, const uint8_t* bundles, const uint64_t* bundle_off, uint8_t* att_out, uint64_t att_cap, uint64_t* att_off,
                                                uint8_t* tags_out, int32_t* status) {
    if (!c || !att_off || (B && (!bundles || !bundle_off || !att_out || !tags_out || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = acc_refusal(c, B, false)) return zs;
    if (B == 0) {
        att_off[0] = 0;
        return ZK_OK;
    }
    uint64_t need = 0;
    for (uint64_t b = 0; b < B; b++) need += zkc_slot_att_bytes(bundle_off[b], bundle_off[b + 1]);
    if (att_cap < need) {   // before a byte of any output is written
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    const uint64_t bytes = acc_readable_end(B, bundle_off), in_b = acc_round64(bytes + 64), att_b = acc_round64(need + 64);
    AccLayoutIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return acc_layout_in_layout(I, base, B); })) return zs;
    if (zk_status zs = reserve(c, B_io, in_b + att_b + B * ZKC_TAG_BYTES)) return zs;   // the bundles, the attestations, the tags
    uint8_t* const d_in = (uint8_t*)c->buf[B_io].p;
    uint8_t *const d_att = d_in + in_b, *const d_tags = d_att + att_b;
    HIPCHK(c, hipMemcpy(I.off, bundle_off, 8 * (B + 1), hipMemcpyHostToDevice));
    if (bytes) HIPCHK(c, hipMemcpy(d_in, bundles, bytes, hipMemcpyHostToDevice));
    if (zk_status zs = acc_split_device(c, B, d_in, I.off, d_att, need, I.out_off, d_tags, I.st, bundle_off)) return zs;
    HIPCHK(c, hipMemcpy(att_off, I.out_off, 8 * (B + 1), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(status, I.st, 4 * B, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(tags_out, d_tags, B * ZKC_TAG_BYTES, hipMemcpyDeviceToHost));
    if (att_off[B]) HIPCHK(c, hipMemcpy(att_out, d_att, att_off[B], hipMemcpyDeviceToHost));
    return ZK_OK;
}

// what the bundles of the proofs in these slots can come to, from the offsets alone
static uint64_t acc_join_need(uint64_t B, const uint64_t* off) {
    uint64_t need = 0;
    for (uint64_t b = 0; b < B; b++)
        if (rr_slot_readable(off[b], off[b + 1])) need += zkc_size(off[b + 1] - off[b]);
    return need;
}
static zk_status acc_join_device(zk_ctx* c, uint64_t B, const uint8_t* proofs, const uint64_t* off, const uint8_t* tags, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                                 int32_t* status, const uint64_t* h_off) {
    if (zk_status zs = acc_refusal(c, B, false)) return zs;
    hipStream_t s = c->stream;
    if (B == 0) {
        if (!words_aligned({out_off})) return ZK_E_ARG;
        HIPCHK(c, hipMemsetAsync(out_off, 0, 8, s));
        HIPCHK(c, hipStreamSynchronize(s));
        return ZK_OK;
    }
    if (!words_aligned({proofs, off, tags, out, out_off, status})) return ZK_E_ARG;
    std::vector<uint64_t> off_copy;
    if (zk_status zs = acc_offsets(c, B, off, off_copy, h_off)) return zs;
    if (out_cap < acc_join_need(B, h_off)) {   // before a byte of any output is written
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    const uint32_t Wn = (uint32_t)std::min<uint64_t>(B, acc_window(c));
    AccWalkWin W;
    if (zk_status zs = lay_out(c, B_as, [&](uint8_t* base) { return acc_walk_layout(W, base, Wn); })) return zs;
    const Wire wire = wire_make(c->wire == ZK_WIRE_ZKA1P);
    AccTiming T{c, zk_timed(c, B)};
    uint64_t base = 0;
    for (uint64_t b0 = 0; b0 < B; b0 += Wn) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(Wn, B - b0);
        const uint8_t* const tags_w = tags + b0 * ZKC_TAG_BYTES;
        if (zk_status zs = T.phase("accountable_walk", [&] {
                launch_acc_walk(s, n, proofs, off + b0, tags_w, wire, W.good, W.a_src, W.a_len, W.t_src, W.t_len, W.t_dst, W.len, status + b0);
                return ZK_OK;
            }))
            return zs;
        // the scan, the headers, the records (the proofs' first, then the tags'), the bytes from their two sources
        if (zk_status zs = T.phase("accountable_layout", [&] {
                launch_pr_offsets(s, n, W.len, base, out_off + b0);
                launch_acc_place(s, n, W.a_src, W.len, 0, out_off + b0, out, W.rec_off, W.rec_len, W.rec_dst);
                launch_pr_move(s, n, W.rec_off, W.rec_len, proofs, W.rec_dst, out);
                launch_pr_move(s, n, W.rec_off + n, W.rec_len + n, tags_w, W.rec_dst + n, out);
                HIPCHK(c, hipMemcpyAsync(&base, out_off + b0 + n, 8, hipMemcpyDeviceToHost, s));
                return ZK_OK;
            }))
            return zs;
    }
    T.publish();
    return ZK_OK;
}
extern "C" zk_status zk_accountable_join_batch_device(zk_ctx* c, uint64_t B, const void* d_proofs, const void* d_proof_off, const void* d_tags, void* d_out, uint64_t out_cap,
                                                      void* d_out_off, void* d_status) {
    if (!c || !d_out_off || (B && (!d_proofs || !d_proof_off || !d_tags || !d_out || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return acc_join_device(c, B, (const uint8_t*)d_proofs, (const uint64_t*)d_proof_off, (const uint8_t*)d_tags, (uint8_t*)d_out, out_cap, (uint64_t*)d_out_off, (int32_t*)d_status,
                           nullptr);
}
extern "C" zk_status zk_accountable_join_batch(zk_ctx* c, uint64_t B, const uint8_t* proofs, const uint64_t* proof_off, const uint8_t* tags, uint8_t* out, uint64_t out_cap,
                                               uint64_t* out_off, int32_t* status) {
    if (!c || !out_off || (B && (!proofs || !proof_off || !tags || !out || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = acc_refusal(c, B, false)) return zs;
    if (B == 0) {
        out_off[0] = 0;
        return ZK_OK;
    }
    const uint64_t need = acc_join_need(B, proof_off);
    if (out_cap < need) {   // before a byte of any output is written
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    const uint64_t bytes = acc_readable_end(B, proof_off), in_b = acc_round64(bytes + 64), tag_b = acc_round64(B * ZKC_TAG_BYTES);
    AccLayoutIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return acc_layout_in_layout(I, base, B); })) return zs;
    if (zk_status zs = reserve(c, B_io, in_b + tag_b + need + 64)) return zs;   // the proofs, the tags, the bundles
    uint8_t* const d_in = (uint8_t*)c->buf[B_io].p;
    uint8_t *const d_tags = d_in + in_b, *const d_out = d_tags + tag_b;
    HIPCHK(c, hipMemcpy(I.off, proof_off, 8 * (B + 1), hipMemcpyHostToDevice));
    if (bytes) HIPCHK(c, hipMemcpy(d_in, proofs, bytes, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_tags, tags, B * ZKC_TAG_BYTES, hipMemcpyHostToDevice));
    if (zk_status zs = acc_join_device(c, B, d_in, I.off, d_tags, d_out, need, I.out_off, I.st, proof_off)) return zs;
    HIPCHK(c, hipMemcpy(out_off, I.out_off, 8 * (B + 1), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(status, I.st, 4 * B, hipMemcpyDeviceToHost));
    if (out_off[B]) HIPCHK(c, hipMemcpy(out, d_out, out_off[B], hipMemcpyDeviceToHost));
    return ZK_OK;
}
