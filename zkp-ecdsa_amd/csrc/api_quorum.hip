// zk_quorum_prove_batch / zk_quorum_verify_batch (include/zkattest.h): "k different ring members attested", as one "ZKQ1" bundle of k attestations and the
// k (k - 1) / 2 distinct-key proofs between their keyXcoms.  Host-side pipeline.  The attestations, the key blinders, the keyXcom extractor and the
// distinct-key proofs run through the internal paths of their own calls, unchanged; the kernels of its own are in k_quorum.hip, the scan of the lengths and
// the byte mover are k_prove_rings.hip's.  A call runs in WINDOWS of whole quorums of at most chunk x lanes members: what is not yet at its final place -- a
// window's attestations and pair proofs, the gathered keys, commitments and blinders -- lies in one witness-flagged buffer (c->buf[B_qs]) whose size follows
// the window, not Q.  The `_rings` forms (one resident ring id per member, DESIGN.md section 5g') run the same window loop: their member
// step enters the mixed-ring pipelines, their staging follows the largest ring the call names, and their out_cap is decided by k_q_caps from the ids alone.
#include "ctx.h"
#include "jobs.h"
#include "link.h"
#include "distinct.h"
#include "quorum.h"

static_assert(ZKQ_PAIR_BYTES == ZKD1_SIZE, "a bundle's pairs are ZKD1 proofs");

extern "C" uint64_t zk_quorum_pair_count(uint32_t k) { return zkq_pairs(k); }
extern "C" uint64_t zk_quorum_proof_max_size(const zk_ctx* c, uint32_t k) { return c ? zkq_max_size(k, zk_proof_max_size(c)) : 0; }

// NULL pointers and k are the caller's to check first; then the distinct calls' rules plus the prover's.  rings: a `_rings` form, which reads no active ring.
static zk_status quorum_refusal(zk_ctx* c, uint64_t Q, uint32_t k, bool rings) {
    if (!zkq_k_ok(k) || Q > 0xffffffffull / k || Q > 0xffffffffull / zkq_pairs(k)) return ZK_E_ARG;
    if (!c->params_set || (!rings && !c->ring->N)) return ZK_E_BUFFER;
    if (c->stream_busy) return busy_refusal(c);
    return ZK_OK;
}
// The `_rings` forms: the context's rings as the capacity rule sees them (quorum_plan.h), and what a call's ids come to
void quorum_rings_table(const zk_ctx* c, QuorumRings& R) {
    R = QuorumRings{};
    for (auto& ring : c->rings)
        if (ring.live && R.count < ZKQ_RINGS) {
            const uint64_t pm = zk_ring_proof_max_size(c, ring.id);
            R.id[R.count] = ring.id, R.resident[R.count] = pm != 0, R.proof_max[R.count] = (uint32_t)pm, R.count++;
        }
}
static const uint32_t quorum_no_ids[1] = {0};   // a `_rings` call of Q = 0 may pass no ids and reads none
struct QuorumCaps {
    uint64_t total;       // the sum of the quorums' capacities: what out_cap is held against
    uint64_t proof_max;   // the largest proof of the rings the ids name: a window's attestation staging follows it
};
uint64_t quorum_largest(const QuorumRings& R, uint32_t used) {
    uint64_t m = 0;
    for (uint32_t r = 0; r < R.count; r++)
        if (used >> r & 1) m = std::max<uint64_t>(m, R.proof_max[r]);
    return m;
}
static QuorumCaps quorum_caps_host(const zk_ctx* c, uint64_t Q, uint32_t k, const uint32_t* ids) {
    QuorumRings R;
    quorum_rings_table(c, R);
    uint64_t total = 0;
    uint32_t used = 0;
    for (uint64_t q = 0; q < Q; q++) total += zkq_capacity_rings(R, k, ids + q * k, &used);
    return {total, quorum_largest(R, used)};
}
// ids on the device: one kernel, ONE read-back (the total and the set of named entries, next to each other behind the capacities in c->buf[B_qc])
static zk_status quorum_caps_device(zk_ctx* c, uint64_t Q, uint32_t k, const uint32_t* d_ids, QuorumCaps& caps) {
    QuorumRings R;
    quorum_rings_table(c, R);
    if (zk_status zs = reserve(c, B_qc, 8 * Q + 16)) return zs;
    uint64_t* const d_caps = (uint64_t*)c->buf[B_qc].p;
    uint64_t* const d_tot = d_caps + Q;
    uint64_t h[2] = {0, 0};
    HIPCHK(c, hipMemsetAsync(d_tot, 0, 16, c->stream));
    launch_q_caps(c->stream, (uint32_t)Q, k, d_ids, R, d_caps, d_tot);
    HIPCHK(c, hipMemcpyAsync(h, d_tot, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    caps = {h[0], quorum_largest(R, (uint32_t)h[1])};
    return ZK_OK;
}
extern "C" uint64_t zk_rings_quorum_proof_max_size(const zk_ctx* c, uint32_t k, const uint32_t* ring_ids) {
    if (!c || !ring_ids || !c->params_set) return 0;
    QuorumRings R;
    quorum_rings_table(c, R);
    return zkq_max_size_rings(R, k, ring_ids);
}
static uint32_t quorum_window(const zk_ctx* c, uint32_t k) { return window_rows(c, k); }   // quorums per window
static size_t rng_row(const zk_rng& r) { return rng_row_bytes(r); }

using QuorumTiming = PipelineTiming;   // (jobs.h)

// ------------------------------------------------------------------ prover
struct QuorumProveWin {
    uint8_t *blinder, *com, *key1, *com1, *blinder1, *key2, *com2, *blinder2, *stage;
    uint64_t *w_off, *len, *rec_off, *rec_len, *rec_dst;
    int32_t *w_st, *kc_st, *pair_st;
    uint64_t pair_stage;   // where the window's distinct-key proofs start in `stage`
};
static size_t quorum_prove_layout(QuorumProveWin& W, uint8_t* base, size_t nq, uint32_t k, uint64_t proof_max) {
    Carver c(base);
    const size_t n = nq * k, np = nq * zkq_pairs(k);
    W.blinder = (uint8_t*)c.take(32 * n), W.com = (uint8_t*)c.take(72 * n);
    W.key1 = (uint8_t*)c.take(32 * np), W.com1 = (uint8_t*)c.take(72 * np), W.blinder1 = (uint8_t*)c.take(32 * np);
    W.key2 = (uint8_t*)c.take(32 * np), W.com2 = (uint8_t*)c.take(72 * np), W.blinder2 = (uint8_t*)c.take(32 * np);
    W.w_off = (uint64_t*)c.take(8 * (n + 1)), W.len = (uint64_t*)c.take(8 * nq);
    W.rec_off = (uint64_t*)c.take(16 * nq), W.rec_len = (uint64_t*)c.take(16 * nq), W.rec_dst = (uint64_t*)c.take(16 * nq);
    W.w_st = (int32_t*)c.take(4 * n), W.kc_st = (int32_t*)c.take(4 * n), W.pair_st = (int32_t*)c.take(4 * np);
    W.pair_stage = n * proof_max;
    W.stage = (uint8_t*)c.take(W.pair_stage + np * ZKQ_PAIR_BYTES);
    return c.off + ZK_LAYOUT_TAIL;
}
struct QuorumProveIo {   // device pointers
    const uint8_t *msg, *sig, *pk;
    const uint32_t* which;
    uint8_t* out;
    uint64_t* out_off;
    int32_t *status, *member_status;
    const uint32_t* ids;   // the `_rings` forms: one resident ring id per member; nullptr: the active ring
};
// known: the host-pointer `_rings` form has the ids on the host and has decided already
static zk_status quorum_prove_device(zk_ctx* c, uint64_t Q, uint32_t k, const QuorumProveIo& io, const zk_rng& rng, const zk_rng& rng_pairs, uint64_t out_cap,
                                     const QuorumCaps* known = nullptr) {
    if (zk_status zs = quorum_refusal(c, Q, k, io.ids != nullptr)) return zs;
    if (!rng_mode_ok(&rng) || !rng_mode_ok(&rng_pairs)) return ZK_E_ARG;
    hipStream_t s = c->stream;
    if (Q == 0) {
        HIPCHK(c, hipMemsetAsync(io.out_off, 0, 8, s));
        HIPCHK(c, hipStreamSynchronize(s));
        return ZK_OK;
    }
    const uint64_t P = zkq_pairs(k);
    QuorumCaps caps{0, zk_proof_max_size(c)};
    QuorumTiming T{c, zk_timed(c, Q * k)};
    if (known) caps = *known;
    else if (io.ids) {   // from the ids alone, before a byte of any output is written
        if (!words_aligned({io.ids})) return ZK_E_ARG;
        if (zk_status zs = T.phase("quorum_caps", [&] { return quorum_caps_device(c, Q, k, io.ids, caps); })) return zs;
    }
    const uint64_t proof_max = caps.proof_max;
    if (io.ids ? out_cap < caps.total : out_cap / zkq_max_size(k, proof_max) < Q) {
        c->err = "output buffer too small";
        return ZK_E_BUFFER;
    }
    if (!words_aligned({io.msg, io.sig, io.pk, io.which, io.out, io.out_off, io.status, io.member_status, rng.data, rng_pairs.data})) return ZK_E_ARG;
    const uint32_t Wq = (uint32_t)std::min<uint64_t>(Q, quorum_window(c, k));
    QuorumProveWin W;
    if (zk_status zs = lay_out(c, B_qs, [&](uint8_t* base) { return quorum_prove_layout(W, base, Wq, k, proof_max); })) return zs;
    const Wire wire = wire_make(c->wire == ZK_WIRE_ZKA1P);
    uint64_t base = 0;   // bytes of the finished windows: where this window's bundles start in `out`
    for (uint64_t q0 = 0; q0 < Q; q0 += Wq) {
        const QuorumShape S{(uint32_t)std::min<uint64_t>(Wq, Q - q0), k, (uint32_t)P};
        const uint64_t n = (uint64_t)S.nq * k, np = (uint64_t)S.nq * P, m0 = q0 * k, p0 = q0 * P;
        const zk_rng rng_w{rng.mode, rng.data + rng_row(rng) * m0, rng.stride_blocks}, rng_p{rng_pairs.mode, rng_pairs.data + rng_row(rng_pairs) * p0, rng_pairs.stride_blocks};
        // the attestations, back to back in the staging area
        if (zk_status zs = io.ids ? zkq_prove_members_rings(c, n, io.msg + 32 * m0, io.sig + 64 * m0, io.pk + 64 * m0, io.which + m0, io.ids + m0, rng_w, W.stage, W.pair_stage,
                                                            W.w_off, W.w_st)
                                  : zkq_prove_members(c, n, io.msg + 32 * m0, io.sig + 64 * m0, io.pk + 64 * m0, io.which + m0, rng_w, W.stage, W.pair_stage, W.w_off, W.w_st))
            return zs;
        T.absorb();
        // the blinders of their keyXcoms (a stream too short for draw 1 is that member's own status already), the keyXcoms themselves, the pairs' six arrays
        if (zk_status zs = T.phase("quorum_blinders", [&] {
                const zk_status zb = zkq_key_blinders(c, n, rng_w, W.blinder);
                return zb == ZK_E_RNG_EXHAUSTED ? ZK_OK : zb;
            }))
            return zs;
        if (zk_status zs = T.phase("quorum_gather", [&] {
                launch_link_keycoms(s, n, W.stage, W.w_off, wire, W.com, W.kc_st);
                launch_q_gather_prove(s, S, io.pk + 64 * m0, W.com, W.blinder, W.key1, W.com1, W.blinder1, W.key2, W.com2, W.blinder2);
                return ZK_OK;
            }))
            return zs;
        if (zk_status zs = zkq_distinct_prove(c, np, W.key1, W.com1, W.blinder1, W.key2, W.com2, W.blinder2, rng_p, W.stage + W.pair_stage, W.pair_st)) return zs;
        T.absorb();
        // statuses and lengths, the scan, headers and records, the bytes; the host takes the window's end as the next window's base
        if (zk_status zs = T.phase("quorum_layout", [&] {
                launch_q_fold_prove(s, S, W.w_off, W.w_st, W.pair_st, io.status + q0, io.member_status ? io.member_status + m0 : nullptr, W.len);
                launch_pr_offsets(s, S.nq, W.len, base, io.out_off + q0);
                launch_q_place(s, S, W.w_off, W.len, W.pair_stage, io.out_off + q0, io.out, W.rec_off, W.rec_len, W.rec_dst);
                launch_pr_move(s, 2 * S.nq, W.rec_off, W.rec_len, W.stage, W.rec_dst, io.out);
                HIPCHK(c, hipMemcpyAsync(&base, io.out_off + q0 + S.nq, 8, hipMemcpyDeviceToHost, s));
                return ZK_OK;
            }))
            return zs;
    }
    T.publish();
    return ZK_OK;
}
extern "C" zk_status zk_quorum_prove_batch_device(zk_ctx* c, uint64_t Q, uint32_t k, const void* d_msg, const void* d_sig, const void* d_pk, const void* d_which, const zk_rng* rng,
                                                  const zk_rng* rng_pairs, void* d_out, uint64_t out_cap, void* d_out_off, void* d_status, void* d_member_status) {
    if (!c || !rng || !rng_pairs || !d_out_off || (Q && (!d_msg || !d_sig || !d_pk || !d_which || !rng->data || !rng_pairs->data || !d_out || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const zk_status zs = quorum_prove_device(c, Q, k, {(const uint8_t*)d_msg, (const uint8_t*)d_sig, (const uint8_t*)d_pk, (const uint32_t*)d_which, (uint8_t*)d_out,
                                                       (uint64_t*)d_out_off, (int32_t*)d_status, (int32_t*)d_member_status}, *rng, *rng_pairs, out_cap);
    if (zs && c->params_set && !c->stream_busy) wipe_witness(c);   // a failed call leaves no gathered key or blinder, nonce or RNG block behind
    return zs;
}
extern "C" zk_status zk_rings_quorum_prove_batch_device(zk_ctx* c, uint64_t Q, uint32_t k, const void* d_msg, const void* d_sig, const void* d_pk, const void* d_which,
                                                        const void* d_ring_ids, const zk_rng* rng, const zk_rng* rng_pairs, void* d_out, uint64_t out_cap, void* d_out_off,
                                                        void* d_status, void* d_member_status) {
    if (!c || !rng || !rng_pairs || !d_out_off ||
        (Q && (!d_msg || !d_sig || !d_pk || !d_which || !d_ring_ids || !rng->data || !rng_pairs->data || !d_out || !d_status)))
        return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const zk_status zs = quorum_prove_device(c, Q, k, {(const uint8_t*)d_msg, (const uint8_t*)d_sig, (const uint8_t*)d_pk, (const uint32_t*)d_which, (uint8_t*)d_out,
                                                       (uint64_t*)d_out_off, (int32_t*)d_status, (int32_t*)d_member_status, d_ring_ids ? (const uint32_t*)d_ring_ids : quorum_no_ids},
                                             *rng, *rng_pairs, out_cap);
    if (zs && c->params_set && !c->stream_busy) wipe_witness(c);   // ... nor a gathered per-ring window
    return zs;
}
// Host pointers: the inputs and both seed sets through the context's witness-flagged input buffer, the bundles through its output staging buffer.
struct QuorumProveIn {
    uint8_t *msg, *sig, *pk, *rng, *rng_pairs;
    uint32_t *which, *ids;   // ids: the `_rings` form only
    uint64_t* off;
    int32_t *st, *mst;
};
static size_t quorum_prove_in_layout(QuorumProveIn& I, uint8_t* base, size_t Q, size_t n, size_t rng_b, size_t rng_pairs_b, bool ids) {
    Carver k(base);
    I.msg = (uint8_t*)k.take(32 * n), I.sig = (uint8_t*)k.take(64 * n), I.pk = (uint8_t*)k.take(64 * n), I.which = (uint32_t*)k.take(4 * n);
    I.ids = ids ? (uint32_t*)k.take(4 * n) : nullptr;
    I.rng = (uint8_t*)k.take(rng_b ? rng_b : 32), I.rng_pairs = (uint8_t*)k.take(rng_pairs_b ? rng_pairs_b : 32);
    I.off = (uint64_t*)k.take(8 * (Q + 1)), I.st = (int32_t*)k.take(4 * Q), I.mst = (int32_t*)k.take(4 * n);
    return k.off + ZK_LAYOUT_TAIL;
}
// ids: the `_rings` form (the capacities come from the ids here on the host, by the rule the kernel uses); nullptr: the active ring
static zk_status quorum_prove_host(zk_ctx* c, uint64_t Q, uint32_t k, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk, const uint32_t* which, const uint32_t* ids,
                                   const zk_rng* rng, const zk_rng* rng_pairs, uint8_t* out, uint64_t out_cap, uint64_t* out_off, int32_t* status, int32_t* member_status) {
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = quorum_refusal(c, Q, k, ids != nullptr)) return zs;
    if (!rng_mode_ok(rng) || !rng_mode_ok(rng_pairs)) return ZK_E_ARG;
    if (Q == 0) {
        out_off[0] = 0;
        return ZK_OK;
    }
    const uint64_t n = Q * k, np = Q * zkq_pairs(k), need = ids ? 0 : zkq_max_size(k, zk_proof_max_size(c));
    const QuorumCaps caps = ids ? quorum_caps_host(c, Q, k, ids) : QuorumCaps{Q * need, 0};
    if (ids ? out_cap < caps.total : out_cap / need < Q) {   // before a byte of any output is written
        c->err = "output buffer too small";
        wipe_witness(c);
        return ZK_E_BUFFER;
    }
    QuorumProveIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return quorum_prove_in_layout(I, base, Q, n, rng_bytes(rng, n), rng_bytes(rng_pairs, np), ids != nullptr); }))
        return zs;
    if (zk_status zs = reserve(c, B_io, caps.total)) return zs;
    uint8_t* const d_out = (uint8_t*)c->buf[B_io].p;
    // from the first upload on, signatures and seeds lie in the input buffer: every failure below zeroes them
    if (zk_status zs = upload_or_wipe(c, {{I.msg, msg, 32 * n}, {I.sig, sig, 64 * n}, {I.pk, pk, 64 * n}, {I.which, which, 4 * n}, {I.ids, ids, ids ? 4 * n : 0},
                                          {I.rng, rng->data, rng_bytes(rng, n)}, {I.rng_pairs, rng_pairs->data, rng_bytes(rng_pairs, np)}}))
        return zs;
    if (zk_status zs = quorum_prove_device(c, Q, k, {I.msg, I.sig, I.pk, I.which, d_out, I.off, I.st, I.mst, I.ids}, zk_rng{rng->mode, I.rng, rng->stride_blocks},
                                           zk_rng{rng_pairs->mode, I.rng_pairs, rng_pairs->stride_blocks}, caps.total, ids ? &caps : nullptr)) {
        wipe_witness(c);
        return zs;
    }
    if (zk_status zs = download_or_wipe(c, {{I.off, out_off, 8 * (Q + 1)}, {I.st, status, 4 * Q}, {I.mst, member_status, member_status ? 4 * n : 0}})) return zs;
    return download_or_wipe(c, {{d_out, out, out_off[Q]}});
}
extern "C" zk_status zk_quorum_prove_batch(zk_ctx* c, uint64_t Q, uint32_t k, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk, const uint32_t* which, const zk_rng* rng,
                                           const zk_rng* rng_pairs, uint8_t* out, uint64_t out_cap, uint64_t* out_off, int32_t* status, int32_t* member_status) {
    if (!c || !rng || !rng_pairs || !out_off || (Q && (!msg || !sig || !pk || !which || !rng->data || !rng_pairs->data || !out || !status))) return ZK_E_ARG;
    return quorum_prove_host(c, Q, k, msg, sig, pk, which, nullptr, rng, rng_pairs, out, out_cap, out_off, status, member_status);
}
extern "C" zk_status zk_rings_quorum_prove_batch(zk_ctx* c, uint64_t Q, uint32_t k, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk, const uint32_t* which,
                                                 const uint32_t* ring_ids, const zk_rng* rng, const zk_rng* rng_pairs, uint8_t* out, uint64_t out_cap, uint64_t* out_off,
                                                 int32_t* status, int32_t* member_status) {
    if (!c || !rng || !rng_pairs || !out_off || (Q && (!msg || !sig || !pk || !which || !ring_ids || !rng->data || !rng_pairs->data || !out || !status))) return ZK_E_ARG;
    return quorum_prove_host(c, Q, k, msg, sig, pk, which, ring_ids ? ring_ids : quorum_no_ids, rng, rng_pairs, out, out_cap, out_off, status, member_status);
}

// ------------------------------------------------------------------ verifier
struct QuorumVerifyWin {
    uint8_t *good, *com, *com1, *com2, *m_ok, *p_ok, *stage_att, *stage_pairs;
    uint64_t *walk, *m_src, *m_len, *s_off, *p_src, *p_len, *p_dst;
    int32_t *kc_st, *m_st, *p_st;
};
static size_t quorum_verify_layout(QuorumVerifyWin& W, uint8_t* base, size_t nq, uint32_t k, uint64_t att_bytes) {
    Carver c(base);
    const size_t n = nq * k, np = nq * zkq_pairs(k);
    W.good = (uint8_t*)c.take(nq), W.com = (uint8_t*)c.take(72 * n), W.com1 = (uint8_t*)c.take(72 * np), W.com2 = (uint8_t*)c.take(72 * np);
    W.m_ok = (uint8_t*)c.take(n), W.p_ok = (uint8_t*)c.take(np);
    W.walk = (uint64_t*)c.take(8 * nq * (k + 1)), W.m_src = (uint64_t*)c.take(8 * n), W.m_len = (uint64_t*)c.take(8 * n), W.s_off = (uint64_t*)c.take(8 * (n + 1));
    W.p_src = (uint64_t*)c.take(8 * nq), W.p_len = (uint64_t*)c.take(8 * nq), W.p_dst = (uint64_t*)c.take(8 * nq);
    W.kc_st = (int32_t*)c.take(4 * n), W.m_st = (int32_t*)c.take(4 * n), W.p_st = (int32_t*)c.take(4 * np);
    W.stage_att = (uint8_t*)c.take(att_bytes + 64), W.stage_pairs = (uint8_t*)c.take(np * ZKQ_PAIR_BYTES);
    return c.off + ZK_LAYOUT_TAIL;
}
struct QuorumVerifyIo {   // device pointers
    const uint8_t *msg, *bundles;
    const uint64_t* off;
    const uint8_t* vseeds;
    uint8_t* ok;
    int32_t* status;
    uint32_t* first_bad;
    const uint32_t* ids;   // the `_rings` forms: one resident ring id per member; nullptr: the active ring
};
// h_off: the offsets on the host (the device form reads them back once) -- a window's staging is as large as the slots it may move
static zk_status quorum_verify_device(zk_ctx* c, uint64_t Q, uint32_t k, const QuorumVerifyIo& io, const uint64_t* h_off) {
    if (zk_status zs = quorum_refusal(c, Q, k, io.ids != nullptr)) return zs;
    if (Q == 0) return ZK_OK;
    if (!words_aligned({io.msg, io.bundles, io.off, io.vseeds, io.ok, io.status, io.first_bad, io.ids})) return ZK_E_ARG;
    hipStream_t s = c->stream;
    std::vector<uint64_t> off_copy;
    if (!h_off) {
        off_copy.resize(Q + 1);
        HIPCHK(c, hipMemcpy(off_copy.data(), io.off, 8 * (Q + 1), hipMemcpyDeviceToHost));
        h_off = off_copy.data();
    }
    const uint32_t Wq = (uint32_t)std::min<uint64_t>(Q, quorum_window(c, k)), P = zkq_pairs(k);
    uint64_t att_bytes = 0;   // the largest window's slots (only a slot the walk can accept is moved, and never its header or pairs)
    for (uint64_t q0 = 0; q0 < Q; q0 += Wq) {
        uint64_t sum = 0;
        for (uint64_t q = q0; q < std::min<uint64_t>(Q, q0 + Wq); q++)
            if (h_off[q + 1] > h_off[q] && h_off[q + 1] - h_off[q] <= 0xffffffffull) sum += h_off[q + 1] - h_off[q];
        att_bytes = std::max(att_bytes, sum);
    }
    QuorumVerifyWin W;
    if (zk_status zs = lay_out(c, B_qs, [&](uint8_t* base) { return quorum_verify_layout(W, base, Wq, k, att_bytes); })) return zs;
    const Wire wire = wire_make(c->wire == ZK_WIRE_ZKA1P);
    QuorumTiming T{c, zk_timed(c, Q * k)};
    for (uint64_t q0 = 0; q0 < Q; q0 += Wq) {
        const QuorumShape S{(uint32_t)std::min<uint64_t>(Wq, Q - q0), k, P};
        const uint64_t n = (uint64_t)S.nq * k, np = (uint64_t)S.nq * P, m0 = q0 * k;
        // the headers; the members' bytes back to back and the pairs' proofs at q P x 744 in the staging area; the keyXcoms and the pairs' two arrays
        if (zk_status zs = T.phase("quorum_walk", [&] {
                launch_q_walk(s, S, io.bundles, io.off + q0, wire, W.good, W.walk, W.m_src, W.m_len, W.p_src, W.p_len, W.p_dst);
                launch_pr_offsets(s, (uint32_t)n, W.m_len, 0, W.s_off);
                launch_pr_move(s, (uint32_t)n, W.m_src, W.m_len, io.bundles, W.s_off, W.stage_att);
                launch_pr_move(s, S.nq, W.p_src, W.p_len, io.bundles, W.p_dst, W.stage_pairs);
                launch_link_keycoms(s, n, W.stage_att, W.s_off, wire, W.com, W.kc_st);
                launch_q_gather_verify(s, S, W.com, W.com1, W.com2);
                return ZK_OK;
            }))
            return zs;
        const uint8_t* const seeds_w = io.vseeds ? io.vseeds + 32 * m0 : nullptr;
        if (zk_status zs = io.ids ? zkq_verify_members_rings(c, n, io.msg + 32 * m0, W.stage_att, W.s_off, io.ids + m0, seeds_w, W.m_ok, W.m_st)
                                  : zkq_verify_members(c, n, io.msg + 32 * m0, W.stage_att, W.s_off, seeds_w, W.m_ok, W.m_st))
            return zs;
        T.absorb();
        if (zk_status zs = zkq_distinct_verify(c, np, W.com1, W.com2, W.stage_pairs, W.p_ok, W.p_st)) return zs;
        T.absorb();
        if (zk_status zs = T.phase("quorum_verdict", [&] {
                launch_q_verdict(s, S, W.good, W.m_ok, W.m_st, W.p_ok, W.p_st, io.ok + q0, io.status + q0, io.first_bad ? io.first_bad + q0 : nullptr);
                return ZK_OK;
            }))
            return zs;
    }
    T.publish();
    return ZK_OK;
}
extern "C" zk_status zk_quorum_verify_batch_device(zk_ctx* c, uint64_t Q, uint32_t k, const void* d_msg, const void* d_bundles, const void* d_bundle_off, const void* d_vseeds,
                                                   void* d_ok, void* d_status, void* d_first_bad) {
    if (!c || (Q && (!d_msg || !d_bundles || !d_bundle_off || !d_ok || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return quorum_verify_device(c, Q, k, {(const uint8_t*)d_msg, (const uint8_t*)d_bundles, (const uint64_t*)d_bundle_off, (const uint8_t*)d_vseeds, (uint8_t*)d_ok,
                                          (int32_t*)d_status, (uint32_t*)d_first_bad}, nullptr);
}
extern "C" zk_status zk_rings_quorum_verify_batch_device(zk_ctx* c, uint64_t Q, uint32_t k, const void* d_msg, const void* d_bundles, const void* d_bundle_off,
                                                         const void* d_ring_ids, const void* d_vseeds, void* d_ok, void* d_status, void* d_first_bad) {
    if (!c || (Q && (!d_msg || !d_bundles || !d_bundle_off || !d_ring_ids || !d_ok || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return quorum_verify_device(c, Q, k, {(const uint8_t*)d_msg, (const uint8_t*)d_bundles, (const uint64_t*)d_bundle_off, (const uint8_t*)d_vseeds, (uint8_t*)d_ok,
                                          (int32_t*)d_status, (uint32_t*)d_first_bad, d_ring_ids ? (const uint32_t*)d_ring_ids : quorum_no_ids}, nullptr);
}
struct QuorumVerifyIn {   // no witness is staged: a failing copy returns as it is
    uint8_t *msg, *seeds, *ok;
    uint64_t* off;
    int32_t* st;
    uint32_t *bad, *ids;   // ids: the `_rings` form only
};
static size_t quorum_verify_in_layout(QuorumVerifyIn& I, uint8_t* base, size_t Q, size_t n, bool seeds, bool ids) {
    Carver k(base);
    I.msg = (uint8_t*)k.take(32 * n), I.seeds = (uint8_t*)k.take(seeds ? 32 * n : 32), I.off = (uint64_t*)k.take(8 * (Q + 1));
    I.ids = ids ? (uint32_t*)k.take(4 * n) : nullptr;
    I.ok = (uint8_t*)k.take(Q), I.st = (int32_t*)k.take(4 * Q), I.bad = (uint32_t*)k.take(4 * Q);
    return k.off + ZK_LAYOUT_TAIL;
}
static zk_status quorum_verify_host(zk_ctx* c, uint64_t Q, uint32_t k, const uint8_t* msg, const uint8_t* bundles, const uint64_t* bundle_off, const uint32_t* ids,
                                    const uint8_t* vseeds, uint8_t* ok, int32_t* status, uint32_t* first_bad) {
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = quorum_refusal(c, Q, k, ids != nullptr)) return zs;
    if (Q == 0) return ZK_OK;
    const uint64_t n = Q * k;
    uint64_t bytes = 0;   // the end of the last slot a byte of which may be read
    for (uint64_t q = 0; q < Q; q++)
        if (bundle_off[q + 1] > bundle_off[q] && bundle_off[q + 1] - bundle_off[q] <= 0xffffffffull) bytes = std::max(bytes, bundle_off[q + 1]);
    QuorumVerifyIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return quorum_verify_in_layout(I, base, Q, n, vseeds != nullptr, ids != nullptr); })) return zs;
    if (zk_status zs = reserve(c, B_io, bytes + 64)) return zs;
    uint8_t* const d_bundles = (uint8_t*)c->buf[B_io].p;
    HIPCHK(c, hipMemcpy(I.msg, msg, 32 * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(I.off, bundle_off, 8 * (Q + 1), hipMemcpyHostToDevice));
    if (bytes) HIPCHK(c, hipMemcpy(d_bundles, bundles, bytes, hipMemcpyHostToDevice));
    if (vseeds) HIPCHK(c, hipMemcpy(I.seeds, vseeds, 32 * n, hipMemcpyHostToDevice));
    if (ids) HIPCHK(c, hipMemcpy(I.ids, ids, 4 * n, hipMemcpyHostToDevice));
    if (zk_status zs = quorum_verify_device(c, Q, k, {I.msg, d_bundles, I.off, vseeds ? I.seeds : nullptr, I.ok, I.st, I.bad, I.ids}, bundle_off)) return zs;
    HIPCHK(c, hipMemcpy(ok, I.ok, Q, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(status, I.st, 4 * Q, hipMemcpyDeviceToHost));
    if (first_bad) HIPCHK(c, hipMemcpy(first_bad, I.bad, 4 * Q, hipMemcpyDeviceToHost));
    return ZK_OK;
}
extern "C" zk_status zk_quorum_verify_batch(zk_ctx* c, uint64_t Q, uint32_t k, const uint8_t* msg, const uint8_t* bundles, const uint64_t* bundle_off, const uint8_t* vseeds,
                                            uint8_t* ok, int32_t* status, uint32_t* first_bad) {
    if (!c || (Q && (!msg || !bundles || !bundle_off || !ok || !status))) return ZK_E_ARG;
    return quorum_verify_host(c, Q, k, msg, bundles, bundle_off, nullptr, vseeds, ok, status, first_bad);
}
extern "C" zk_status zk_rings_quorum_verify_batch(zk_ctx* c, uint64_t Q, uint32_t k, const uint8_t* msg, const uint8_t* bundles, const uint64_t* bundle_off, const uint32_t* ring_ids,
                                                  const uint8_t* vseeds, uint8_t* ok, int32_t* status, uint32_t* first_bad) {
    if (!c || (Q && (!msg || !bundles || !bundle_off || !ring_ids || !ok || !status))) return ZK_E_ARG;
    return quorum_verify_host(c, Q, k, msg, bundles, bundle_off, ring_ids ? ring_ids : quorum_no_ids, vseeds, ok, status, first_bad);
}
