// Quorum proofs (include/zkattest.h: zk_quorum_*): the kernels between the existing pipelines of a window of whole quorums -- the pair gathers, the header
// walker, the prover's fold and placement, the verifier's verdict.  None of them does field arithmetic: they move words and fold statuses.  The scan of the
// lengths and the byte mover are k_prove_rings.hip's (launch_pr_offsets, launch_pr_move); the pair order, sizes and header rules are quorum_plan.h's.
#define ZK_QUORUM_KERNELS_ONLY
#include "quorum.h"

template <uint32_t WORDS>
ZK_DEV void q_copy_words(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src) {   // both 4-byte aligned
#pragma unroll
    for (uint32_t i = 0; i < WORDS; i++) ((uint32_t*)dst)[i] = ((const uint32_t*)src)[i];
}

// ------------------------------------------------------------------ prover
// lane t = (quorum q, pair p): members i < j of the quorum from the pair's rank; member m = q k + i owns row m of pk, com and blinder
__global__ void __launch_bounds__(256) k_q_gather_prove(QuorumShape W, const uint8_t* __restrict__ pk, const uint8_t* __restrict__ com, const uint8_t* __restrict__ blinder,
                                                        uint8_t* __restrict__ key1, uint8_t* __restrict__ com1, uint8_t* __restrict__ blinder1, uint8_t* __restrict__ key2,
                                                        uint8_t* __restrict__ com2, uint8_t* __restrict__ blinder2) {
    const uint32_t t = gtid();
    if (t >= W.nq * W.P) return;
    const uint32_t q = t / W.P;
    uint32_t i, j;
    zkq_unrank(W.k, t - q * W.P, i, j);
    const size_t a = (size_t)q * W.k + i, b = (size_t)q * W.k + j;
    q_copy_words<8>(key1 + 32 * (size_t)t, pk + 64 * a), q_copy_words<8>(key2 + 32 * (size_t)t, pk + 64 * b);
    q_copy_words<18>(com1 + 72 * (size_t)t, com + 72 * a), q_copy_words<18>(com2 + 72 * (size_t)t, com + 72 * b);
    q_copy_words<8>(blinder1 + 32 * (size_t)t, blinder + 32 * a), q_copy_words<8>(blinder2 + 32 * (size_t)t, blinder + 32 * b);
}
// lane q: the first non-zero status of the members in member order; then ZK_E_ARG where a pair found equal keys (the one status of the distinct prover that
// says so once both commitments parse, which they do where every member succeeded); then the pairs' in pair order
__global__ void __launch_bounds__(256) k_q_fold_prove(QuorumShape W, const uint64_t* __restrict__ w_off, const int32_t* __restrict__ w_st, const int32_t* __restrict__ pair_st,
                                                      int32_t* __restrict__ q_status, int32_t* __restrict__ member_status, uint64_t* __restrict__ len) {
    const uint32_t q = gtid();
    if (q >= W.nq) return;
    const size_t m0 = (size_t)q * W.k, p0 = (size_t)q * W.P;
    int32_t st = ZK_OK;
    for (uint32_t i = 0; i < W.k; i++) {
        const int32_t v = w_st[m0 + i];
        if (member_status) member_status[m0 + i] = v;
        if (st == ZK_OK) st = v;
    }
    if (st == ZK_OK) {
        int32_t first = ZK_OK;
        bool equal = false;
        for (uint32_t p = 0; p < W.P; p++) {
            const int32_t v = pair_st[p0 + p];
            equal |= v == ZK_E_ARG;
            if (first == ZK_OK) first = v;
        }
        st = equal ? (int32_t)ZK_E_ARG : first;
    }
    q_status[q] = st;
    len[q] = st == ZK_OK ? zkq_size(W.k, w_off[m0 + W.k] - w_off[m0]) : 0;
}
// lane q, behind the scan: a successful quorum's header at out_off[q]; record 2 q = its k attestations (back to back in the staging area since every
// member succeeded), record 2 q + 1 = its P distinct-key proofs.  A failed quorum's records are empty.
__global__ void __launch_bounds__(256) k_q_place(QuorumShape W, const uint64_t* __restrict__ w_off, const uint64_t* __restrict__ len, uint64_t pair_stage,
                                                 const uint64_t* __restrict__ out_off, uint8_t* __restrict__ out, uint64_t* __restrict__ rec_off, uint64_t* __restrict__ rec_len,
                                                 uint64_t* __restrict__ rec_dst) {
    const uint32_t q = gtid();
    if (q >= W.nq) return;
    const uint64_t total = len[q], at = out_off[q], pairs = (uint64_t)W.P * ZKQ_PAIR_BYTES;
    const uint64_t att = total ? total - ZKQ1_HDR - pairs : 0;
    rec_off[2 * q] = w_off[(size_t)q * W.k], rec_len[2 * q] = att, rec_dst[2 * q] = at + ZKQ1_HDR;
    rec_off[2 * q + 1] = pair_stage + (uint64_t)q * pairs, rec_len[2 * q + 1] = total ? pairs : 0, rec_dst[2 * q + 1] = at + ZKQ1_HDR + att;
    if (!total) return;
    uint32_t hw[4];
    zkq_header(hw, (uint32_t)total, W.k);
    uint32_t* o = (uint32_t*)(out + at);
    o[0] = hw[0], o[1] = hw[1], o[2] = hw[2], o[3] = hw[3];
}
// The `_rings` forms.  lane q: the capacity of quorum q's slot from its k ring ids (quorum_plan.h: zkq_capacity_rings; `R` lies in the kernel's arguments); a
// wave adds its lanes' capacities and ors their ring sets, and its first lane adds the wave's into the call's two words.
__global__ void __launch_bounds__(256) k_q_caps(uint32_t Q, uint32_t k, const uint32_t* __restrict__ ids, QuorumRings R, uint64_t* __restrict__ caps,
                                                unsigned long long* __restrict__ total) {
    const uint32_t q = gtid();
    unsigned long long cap = 0;
    uint32_t used = 0;
    if (q < Q) caps[q] = cap = zkq_capacity_rings(R, k, ids + (size_t)q * k, &used);
    for (int d = 32; d; d >>= 1) cap += __shfl_down(cap, d), used |= __shfl_down(used, d);
    if ((threadIdx.x & 63) == 0 && (cap | used)) atomicAdd(total, cap), atomicOr(total + 1, (unsigned long long)used);
}

// ------------------------------------------------------------------ verifier
// lane q: walk[q (k + 1) ..] receives the walk's offsets; a refused bundle's members and pairs get empty records (no byte of it is moved)
__global__ void __launch_bounds__(256) k_q_walk(QuorumShape W, const uint8_t* __restrict__ bundles, const uint64_t* __restrict__ bundle_off, Wire wire, uint8_t* __restrict__ good,
                                                uint64_t* __restrict__ walk, uint64_t* __restrict__ m_src, uint64_t* __restrict__ m_len, uint64_t* __restrict__ p_src,
                                                uint64_t* __restrict__ p_len, uint64_t* __restrict__ p_dst) {
    const uint32_t q = gtid();
    if (q >= W.nq) return;
    uint64_t* mo = walk + (size_t)q * (W.k + 1);
    const bool ok = zkq_walk(bundles, bundle_off[q], bundle_off[q + 1], W.k, wire, mo);
    good[q] = ok;
    for (uint32_t i = 0; i < W.k; i++) {
        const uint64_t a = ok ? mo[i] : 0, b = ok ? mo[i + 1] : 0;
        m_src[(size_t)q * W.k + i] = a, m_len[(size_t)q * W.k + i] = b - a;
    }
    const uint64_t pairs = (uint64_t)W.P * ZKQ_PAIR_BYTES;
    p_src[q] = ok ? mo[W.k] : 0, p_len[q] = ok ? pairs : 0, p_dst[q] = (uint64_t)q * pairs;
}
__global__ void __launch_bounds__(256) k_q_gather_verify(QuorumShape W, const uint8_t* __restrict__ com, uint8_t* __restrict__ com1, uint8_t* __restrict__ com2) {
    const uint32_t t = gtid();
    if (t >= W.nq * W.P) return;
    const uint32_t q = t / W.P;
    uint32_t i, j;
    zkq_unrank(W.k, t - q * W.P, i, j);
    q_copy_words<18>(com1 + 72 * (size_t)t, com + 72 * ((size_t)q * W.k + i)), q_copy_words<18>(com2 + 72 * (size_t)t, com + 72 * ((size_t)q * W.k + j));
}
// lane q: elements 0 .. k - 1 are the members, k .. k + P - 1 the pairs
__global__ void __launch_bounds__(256) k_q_verdict(QuorumShape W, const uint8_t* __restrict__ good, const uint8_t* __restrict__ m_ok, const int32_t* __restrict__ m_st,
                                                   const uint8_t* __restrict__ p_ok, const int32_t* __restrict__ p_st, uint8_t* __restrict__ ok, int32_t* __restrict__ status,
                                                   uint32_t* __restrict__ first_bad) {
    const uint32_t q = gtid();
    if (q >= W.nq) return;
    int32_t st = ZK_OK;
    uint32_t bad = 0xffffffffu;
    if (!good[q]) st = ZK_E_BAD_ENCODING, bad = 0;
    else
        for (uint32_t e = 0; e < W.k + W.P; e++) {
            const bool member = e < W.k;
            const size_t at = member ? (size_t)q * W.k + e : (size_t)q * W.P + (e - W.k);
            const uint8_t o = member ? m_ok[at] : p_ok[at];
            const int32_t v = member ? m_st[at] : p_st[at];
            if (st == ZK_OK) st = v;
            if (bad == 0xffffffffu && (!o || v != ZK_OK)) bad = e;
        }
    ok[q] = bad == 0xffffffffu ? 1 : 0, status[q] = st;
    if (first_bad) first_bad[q] = bad;
}

static dim3 q_grid(uint32_t n) { return dim3((n + 255) / 256); }
void launch_q_gather_prove(hipStream_t s, const QuorumShape& W, const uint8_t* pk, const uint8_t* com, const uint8_t* blinder, uint8_t* key1, uint8_t* com1, uint8_t* blinder1,
                           uint8_t* key2, uint8_t* com2, uint8_t* blinder2) {
    if (W.nq * W.P) hipLaunchKernelGGL(k_q_gather_prove, q_grid(W.nq * W.P), dim3(256), 0, s, W, pk, com, blinder, key1, com1, blinder1, key2, com2, blinder2);
}
void launch_q_fold_prove(hipStream_t s, const QuorumShape& W, const uint64_t* w_off, const int32_t* w_st, const int32_t* pair_st, int32_t* q_status, int32_t* member_status,
                         uint64_t* len) {
    if (W.nq) hipLaunchKernelGGL(k_q_fold_prove, q_grid(W.nq), dim3(256), 0, s, W, w_off, w_st, pair_st, q_status, member_status, len);
}
void launch_q_place(hipStream_t s, const QuorumShape& W, const uint64_t* w_off, const uint64_t* len, uint64_t pair_stage, const uint64_t* out_off, uint8_t* out, uint64_t* rec_off,
                    uint64_t* rec_len, uint64_t* rec_dst) {
    if (W.nq) hipLaunchKernelGGL(k_q_place, q_grid(W.nq), dim3(256), 0, s, W, w_off, len, pair_stage, out_off, out, rec_off, rec_len, rec_dst);
}
void launch_q_walk(hipStream_t s, const QuorumShape& W, const uint8_t* bundles, const uint64_t* bundle_off, const Wire& wire, uint8_t* good, uint64_t* walk, uint64_t* m_src,
                   uint64_t* m_len, uint64_t* p_src, uint64_t* p_len, uint64_t* p_dst) {
    if (W.nq) hipLaunchKernelGGL(k_q_walk, q_grid(W.nq), dim3(256), 0, s, W, bundles, bundle_off, wire, good, walk, m_src, m_len, p_src, p_len, p_dst);
}
void launch_q_gather_verify(hipStream_t s, const QuorumShape& W, const uint8_t* com, uint8_t* com1, uint8_t* com2) {
    if (W.nq * W.P) hipLaunchKernelGGL(k_q_gather_verify, q_grid(W.nq * W.P), dim3(256), 0, s, W, com, com1, com2);
}
void launch_q_verdict(hipStream_t s, const QuorumShape& W, const uint8_t* good, const uint8_t* m_ok, const int32_t* m_st, const uint8_t* p_ok, const int32_t* p_st, uint8_t* ok,
                      int32_t* status, uint32_t* first_bad) {
    if (W.nq) hipLaunchKernelGGL(k_q_verdict, q_grid(W.nq), dim3(256), 0, s, W, good, m_ok, m_st, p_ok, p_st, ok, status, first_bad);
}
void launch_q_caps(hipStream_t s, uint32_t Q, uint32_t k, const uint32_t* ring_ids, const QuorumRings& R, uint64_t* caps, uint64_t* total) {
    if (Q) hipLaunchKernelGGL(k_q_caps, q_grid(Q), dim3(256), 0, s, Q, k, ring_ids, R, caps, (unsigned long long*)total);
}
