// Accountable attestations (include/zkattest.h: zk_accountable_*): the kernels between the existing pipelines of a window of bundles -- the key gather, the
// prover's fold and placement, the header walker of the verifier, of split and of join, the verifier's verdict.  None of them does field arithmetic: they move
// words and fold statuses, one lane per bundle.  The scan of the lengths and the byte mover are k_prove_rings.hip's (launch_pr_offsets, launch_pr_move); the
// sizes, the header words and the walk are accountable_plan.h's.
#define ZK_ACCOUNTABLE_KERNELS_ONLY
#include "accountable.h"

// ------------------------------------------------------------------ prover
__global__ void __launch_bounds__(256) k_acc_keys(uint32_t n, const uint8_t* __restrict__ pk, uint8_t* __restrict__ key) {
    const uint32_t b = gtid();
    if (b >= n) return;
    const uint32_t* src = (const uint32_t*)(pk + 64 * (size_t)b);
    uint32_t* dst = (uint32_t*)(key + 32 * (size_t)b);
#pragma unroll
    for (uint32_t i = 0; i < 8; i++) dst[i] = src[i];
}
// lane b: the first non-zero of the attestation's status and the tag's, in that order
__global__ void __launch_bounds__(256) k_acc_fold_prove(uint32_t n, const uint64_t* __restrict__ w_off, const int32_t* __restrict__ w_st, const int32_t* __restrict__ tag_st,
                                                        int32_t* __restrict__ status, int32_t* __restrict__ part_status, uint64_t* __restrict__ len) {
    const uint32_t b = gtid();
    if (b >= n) return;
    const int32_t a = w_st[b], t = tag_st[b];
    if (part_status) part_status[2 * (size_t)b] = a, part_status[2 * (size_t)b + 1] = t;
    const int32_t st = a != ZK_OK ? a : t;
    status[b] = st;
    len[b] = st == ZK_OK ? zkc_size(w_off[b + 1] - w_off[b]) : 0;
}
// lane b, behind the scan: a successful bundle's header at out_off[b]; record b = its attestation, record n + b = its tag (join moves the two halves from two
// sources); a failed bundle's records are empty
__global__ void __launch_bounds__(256) k_acc_place(uint32_t n, const uint64_t* __restrict__ w_off, const uint64_t* __restrict__ len, uint64_t tag_stage,
                                                   const uint64_t* __restrict__ out_off, uint8_t* __restrict__ out, uint64_t* __restrict__ rec_off, uint64_t* __restrict__ rec_len,
                                                   uint64_t* __restrict__ rec_dst) {
    const uint32_t b = gtid();
    if (b >= n) return;
    const uint64_t total = len[b], at = out_off[b];
    const uint64_t att = total ? total - ZKC1_HDR - ZKC_TAG_BYTES : 0;
    rec_off[b] = w_off[b], rec_len[b] = att, rec_dst[b] = at + ZKC1_HDR;
    rec_off[(size_t)n + b] = tag_stage + (uint64_t)b * ZKC_TAG_BYTES, rec_len[(size_t)n + b] = total ? ZKC_TAG_BYTES : 0, rec_dst[(size_t)n + b] = at + ZKC1_HDR + att;
    if (!total) return;
    uint32_t hw[4];
    zkc_header(hw, (uint32_t)total);
    uint32_t* o = (uint32_t*)(out + at);
    o[0] = hw[0], o[1] = hw[1], o[2] = hw[2], o[3] = hw[3];
}

// ------------------------------------------------------------------ verifier, split, join
__global__ void __launch_bounds__(256) k_acc_walk(uint32_t n, const uint8_t* __restrict__ bundles, const uint64_t* __restrict__ bundle_off, const uint8_t* __restrict__ tags,
                                                  Wire wire, uint8_t* __restrict__ good, uint64_t* __restrict__ a_src, uint64_t* __restrict__ a_len, uint64_t* __restrict__ t_src,
                                                  uint64_t* __restrict__ t_len, uint64_t* __restrict__ t_dst, uint64_t* __restrict__ len, int32_t* __restrict__ status) {
    const uint32_t b = gtid();
    if (b >= n) return;
    const uint64_t o0 = bundle_off[b], o1 = bundle_off[b + 1];
    uint64_t at0 = 0, at1 = 0, tag_at = 0;
    bool ok;
    if (tags) {   // join: the slot holds a bare proof, its tag is row b of `tags`
        tag_at = (uint64_t)b * ZKC_TAG_BYTES;
        ok = zkc_join_len(bundles, o0, o1, tags + tag_at, wire) != 0;
        at0 = o0, at1 = o1;
    } else {
        uint64_t att[2] = {0, 0};
        ok = zkc_walk(bundles, o0, o1, wire, att);
        at0 = att[0], at1 = tag_at = att[1];
    }
    good[b] = ok;
    a_src[b] = ok ? at0 : 0, a_len[b] = ok ? at1 - at0 : 0;
    t_src[b] = ok ? tag_at : 0, t_len[b] = ok ? ZKC_TAG_BYTES : 0, t_dst[b] = (uint64_t)b * ZKC_TAG_BYTES;
    if (len) len[b] = ok ? zkc_size(at1 - at0) : 0;
    if (status) status[b] = ok ? ZK_OK : ZK_E_BAD_ENCODING;
}
// lane b: element 0 is the attestation, element 1 the tag
__global__ void __launch_bounds__(256) k_acc_verdict(uint32_t n, const uint8_t* __restrict__ good, const uint8_t* __restrict__ a_ok, const int32_t* __restrict__ a_st,
                                                     const uint8_t* __restrict__ t_ok, const int32_t* __restrict__ t_st, uint8_t* __restrict__ ok, int32_t* __restrict__ status,
                                                     uint32_t* __restrict__ first_bad) {
    const uint32_t b = gtid();
    if (b >= n) return;
    int32_t st = ZK_OK;
    uint32_t bad = 0xffffffffu;
    if (!good[b]) st = ZK_E_BAD_ENCODING, bad = 0;
    else {
        const int32_t a = a_st[b], t = t_st[b];
        st = a != ZK_OK ? a : t;
        if (!a_ok[b] || a != ZK_OK) bad = 0;
        else if (!t_ok[b] || t != ZK_OK) bad = 1;
    }
    ok[b] = bad == 0xffffffffu ? 1 : 0, status[b] = st;
    if (first_bad) first_bad[b] = bad;
}

// ------------------------------------------------------------------ the `_rings` forms
// lane b: its slot by accountable_plan.h's rule; every lane of a wave stays to the end (the shuffles read all 64), one pair of atomics per wave that has
// anything to add.  The host has checked zkc_capacity_fits: the total cannot wrap.
__global__ void __launch_bounds__(256) k_acc_caps(uint32_t n, const uint32_t* __restrict__ ids, QuorumRings R, unsigned long long* __restrict__ total) {
    const uint32_t b = gtid();
    unsigned long long cap = 0;
    uint32_t used = 0;
    if (b < n) cap = zkc_capacity_rings(R, ids[b], &used);
    for (int d = 32; d; d >>= 1) cap += __shfl_down(cap, d), used |= __shfl_down(used, d);
    if ((threadIdx.x & 63) == 0 && (cap | used)) atomicAdd(total, cap), atomicOr(total + 1, (unsigned long long)used);
}
// lane b of the open: the opener's answer for the tag of bundle b (a refused bundle's tag was 472 zero bytes).  Its ZK_E_ARG -- an id that is neither resident
// nor ZK_ESCROW_RING_ANY -- comes first; then the walk's refusal; then what the opener found.  Both outputs are "none" under every non-zero status.
__global__ void __launch_bounds__(256) k_acc_fold_open(uint32_t n, const uint8_t* __restrict__ good, const int32_t* __restrict__ o_st, const uint32_t* __restrict__ o_ring,
                                                       const uint32_t* __restrict__ o_index, uint32_t* __restrict__ ring_out, uint32_t* __restrict__ index,
                                                       int32_t* __restrict__ status) {
    const uint32_t b = gtid();
    if (b >= n) return;
    const int32_t o = o_st[b];
    const int32_t st = o == ZK_E_ARG ? ZK_E_ARG : !good[b] ? ZK_E_BAD_ENCODING : o;
    status[b] = st;
    ring_out[b] = st == ZK_OK ? o_ring[b] : 0xffffffffu;
    index[b] = st == ZK_OK ? o_index[b] : 0xffffffffu;
}

static dim3 acc_grid(uint32_t n) { return dim3((n + 255) / 256); }
void launch_acc_caps(hipStream_t s, uint32_t n, const uint32_t* ring_ids, const QuorumRings& R, uint64_t* total) {
    if (n) hipLaunchKernelGGL(k_acc_caps, acc_grid(n), dim3(256), 0, s, n, ring_ids, R, (unsigned long long*)total);
}
void launch_acc_fold_open(hipStream_t s, uint32_t n, const uint8_t* good, const int32_t* o_st, const uint32_t* o_ring, const uint32_t* o_index, uint32_t* ring_out,
                          uint32_t* index, int32_t* status) {
    if (n) hipLaunchKernelGGL(k_acc_fold_open, acc_grid(n), dim3(256), 0, s, n, good, o_st, o_ring, o_index, ring_out, index, status);
}
void launch_acc_keys(hipStream_t s, uint32_t n, const uint8_t* pk, uint8_t* key) {
    if (n) hipLaunchKernelGGL(k_acc_keys, acc_grid(n), dim3(256), 0, s, n, pk, key);
}
void launch_acc_fold_prove(hipStream_t s, uint32_t n, const uint64_t* w_off, const int32_t* w_st, const int32_t* tag_st, int32_t* status, int32_t* part_status, uint64_t* len) {
    if (n) hipLaunchKernelGGL(k_acc_fold_prove, acc_grid(n), dim3(256), 0, s, n, w_off, w_st, tag_st, status, part_status, len);
}
void launch_acc_place(hipStream_t s, uint32_t n, const uint64_t* w_off, const uint64_t* len, uint64_t tag_stage, const uint64_t* out_off, uint8_t* out, uint64_t* rec_off,
                      uint64_t* rec_len, uint64_t* rec_dst) {
    if (n) hipLaunchKernelGGL(k_acc_place, acc_grid(n), dim3(256), 0, s, n, w_off, len, tag_stage, out_off, out, rec_off, rec_len, rec_dst);
}
void launch_acc_walk(hipStream_t s, uint32_t n, const uint8_t* bundles, const uint64_t* bundle_off, const uint8_t* tags, const Wire& wire, uint8_t* good, uint64_t* a_src,
                     uint64_t* a_len, uint64_t* t_src, uint64_t* t_len, uint64_t* t_dst, uint64_t* len, int32_t* status) {
    if (n) hipLaunchKernelGGL(k_acc_walk, acc_grid(n), dim3(256), 0, s, n, bundles, bundle_off, tags, wire, good, a_src, a_len, t_src, t_len, t_dst, len, status);
}
void launch_acc_verdict(hipStream_t s, uint32_t n, const uint8_t* good, const uint8_t* a_ok, const int32_t* a_st, const uint8_t* t_ok, const int32_t* t_st, uint8_t* ok,
                        int32_t* status, uint32_t* first_bad) {
    if (n) hipLaunchKernelGGL(k_acc_verdict, acc_grid(n), dim3(256), 0, s, n, good, a_ok, a_st, t_ok, t_st, ok, status, first_bad);
}
