// Mixed-ring proving (include/zkattest.h: zk_prove_batch_rings): the census of a batch's ring ids, the gather of one ring's inputs into a window, and
// what puts the windows' proofs back into index order -- the record of where every proof was staged, the scan of the lengths and the byte mover.
// The partition itself is partition.h's (k_part_scan, k_part_perm over uint8_t classes in workgroups of PR_BLOCK proofs); the prover's kernels run
// unchanged on each window with its ring bound (api.hip: prove_rings_device).
#include "partition.h"

// class of every proof: the place of its ring id in rs.id, PR_UNKNOWN for an id that is not resident.  Per workgroup of PR_BLOCK proofs, how many of
// them fall into each class: one ballot per class and wave, the wave's first lane adds the count to the workgroup's LDS counters (no global atomics).
__global__ void __launch_bounds__(PR_BLOCK) k_pr_census(uint64_t B, const uint32_t* __restrict__ ring_ids, RingSlots rs, uint8_t* __restrict__ cls,
                                                        uint32_t* __restrict__ blk_cnt /* [blocks][PR_CLASSES] */) {
    __shared__ uint32_t cnt[PR_CLASSES];
    if (threadIdx.x < PR_CLASSES) cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t b = (uint64_t)blockIdx.x * PR_BLOCK + threadIdx.x;
    uint32_t k = 0xffu;   // past the batch: no class
    if (b < B) {
        const uint32_t id = ring_ids[b];
        k = PR_UNKNOWN;
#pragma unroll
        for (uint32_t s = 0; s < ZK_MAX_RINGS; s++)
            if (s < rs.count && rs.id[s] == id) k = s;
        cls[b] = (uint8_t)k;
    }
#pragma unroll
    for (uint32_t s = 0; s < PR_CLASSES; s++) {
        const uint64_t m = __ballot(k == s);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt[s], (uint32_t)__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x < PR_CLASSES) blk_cnt[(size_t)blockIdx.x * PR_CLASSES + threadIdx.x] = cnt[threadIdx.x];
}

// 16 bytes of a caller's array: one load where the array is 16-byte aligned (al), bytes otherwise (the C ABI asks no alignment of them)
ZK_DEV uint4 pr_load16(const uint8_t* __restrict__ s, bool al) {
    if (al) return *(const uint4*)s;
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = (uint32_t)s[4 * i] | ((uint32_t)s[4 * i + 1] << 8) | ((uint32_t)s[4 * i + 2] << 16) | ((uint32_t)s[4 * i + 3] << 24);
    return make_uint4(w[0], w[1], w[2], w[3]);
}
// window entry j = proof sel[j]: 16 threads per entry, one 16-byte piece each of the message hash (2), the signature (4), the key (4) and the seed
// (2; seeds == nullptr in stream mode), and `which`.  Consecutive threads write consecutive pieces of the window's arrays.
__global__ void __launch_bounds__(256) k_pr_gather(uint32_t n, const uint32_t* __restrict__ sel, const uint8_t* __restrict__ msg, const uint8_t* __restrict__ sig,
                                                   const uint8_t* __restrict__ pk, const uint32_t* __restrict__ which, const uint8_t* __restrict__ seeds, uint32_t al,
                                                   uint8_t* __restrict__ w_msg, uint8_t* __restrict__ w_sig, uint8_t* __restrict__ w_pk, uint32_t* __restrict__ w_which,
                                                   uint8_t* __restrict__ w_seeds) {
    const uint32_t t = gtid();
    if (t >= 16 * n) return;
    const uint32_t j = t >> 4, q = t & 15;
    const uint64_t b = sel[j];
    if (q < 2) ((uint4*)(w_msg + 32 * (size_t)j))[q] = pr_load16(msg + 32 * b + 16 * q, al & 1);
    else if (q < 6) ((uint4*)(w_sig + 64 * (size_t)j))[q - 2] = pr_load16(sig + 64 * b + 16 * (q - 2), al & 2);
    else if (q < 10) ((uint4*)(w_pk + 64 * (size_t)j))[q - 6] = pr_load16(pk + 64 * b + 16 * (q - 6), al & 4);
    else if (q < 12) {
        if (seeds) ((uint4*)(w_seeds + 32 * (size_t)j))[q - 10] = pr_load16(seeds + 32 * b + 16 * (q - 10), al & 8);
    } else if (q == 12) w_which[j] = which[b];
}
// ZK_RNG_STREAM: the whole stream of proof sel[j] (row_bytes = 32 x stride_blocks) becomes row j of the window; one workgroup per entry
__global__ void __launch_bounds__(256) k_pr_gather_rows(uint32_t n, const uint32_t* __restrict__ sel, const uint8_t* __restrict__ src, uint64_t row_bytes, uint32_t al,
                                                        uint8_t* __restrict__ dst) {
    const uint32_t j = blockIdx.x;
    if (j >= n) return;
    const uint8_t* s = src + row_bytes * (uint64_t)sel[j];
    uint4* d = (uint4*)(dst + row_bytes * (uint64_t)j);
    const uint64_t nq = row_bytes >> 4;   // (a multiple of 32 bytes)
#pragma unroll 4
    for (uint64_t i = threadIdx.x; i < nq; i += 256) d[i] = pr_load16(s + 16 * i, al != 0);
}
// where window entry j's proof lies in the staging area and how long it is, recorded at the proof's own place in its segment, and its status
__global__ void __launch_bounds__(256) k_pr_record(uint32_t n, const uint32_t* __restrict__ sel, uint64_t seg_first, const uint64_t* __restrict__ w_off,
                                                   const int32_t* __restrict__ w_st, uint64_t stage_base, uint64_t* __restrict__ rec_off, uint64_t* __restrict__ rec_len,
                                                   int32_t* __restrict__ status, int32_t st) {
    const uint32_t j = gtid();
    if (j >= n) return;
    const uint64_t b = sel[j], i = b - seg_first;
    rec_off[i] = w_off ? stage_base + w_off[j] : 0;
    rec_len[i] = w_off ? w_off[j + 1] - w_off[j] : 0;   // w_off == nullptr: an empty proof with status `st` (an id that is not resident)
    status[b] = w_off ? w_st[j] : st;
}
// the bytes: one workgroup per proof of the segment, from its place in the staging area to its final place; 16-byte stores at 16-byte aligned
// destinations, 16-byte loads where the source has the same alignment mod 16 and four dwords otherwise (k_lv_gather_bytes' pattern; every offset
// and length is a multiple of 4)
__global__ void __launch_bounds__(256) k_pr_move(uint32_t n, const uint64_t* __restrict__ rec_off, const uint64_t* __restrict__ rec_len, const uint8_t* __restrict__ stage,
                                                 const uint64_t* __restrict__ out_off, uint8_t* __restrict__ out) {
    const uint32_t j = blockIdx.x, t = threadIdx.x;
    if (j >= n) return;
    const uint64_t nd = rec_len[j] >> 2;
    if (!nd) return;
    const uint32_t* src = (const uint32_t*)(stage + rec_off[j]);
    uint32_t* dst = (uint32_t*)(out + out_off[j]);
    uint64_t head = ((16 - ((uintptr_t)dst & 15)) & 15) >> 2;
    if (head > nd) head = nd;
    if (t < head) dst[t] = src[t];
    const uint64_t nq = (nd - head) >> 2;
    uint4* dq = (uint4*)(dst + head);
    const uint32_t* sb = src + head;
    if (!(((uintptr_t)sb) & 15)) {
        const uint4* sq = (const uint4*)sb;
#pragma unroll 4
        for (uint64_t i = t; i < nq; i += 256) dq[i] = sq[i];
    } else {
#pragma unroll 4
        for (uint64_t i = t; i < nq; i += 256) dq[i] = make_uint4(sb[4 * i], sb[4 * i + 1], sb[4 * i + 2], sb[4 * i + 3]);
    }
    const uint64_t done = head + 4 * nq;
    if (t < nd - done) dst[done + t] = src[done + t];
}

void launch_pr_census(hipStream_t s, uint64_t B, const uint32_t* ring_ids, const RingSlots& rs, uint8_t* cls, uint32_t* blk_cnt, uint32_t* out) {
    const uint32_t blocks = (uint32_t)((B + PR_BLOCK - 1) / PR_BLOCK);
    hipLaunchKernelGGL(k_pr_census, dim3(blocks), dim3(PR_BLOCK), 0, s, B, ring_ids, rs, cls, blk_cnt);
    hipLaunchKernelGGL((k_part_scan<PR_CLASSES, 64>), dim3(1), dim3(64), 0, s, blocks, blk_cnt, out);
}
void launch_pr_perm(hipStream_t s, uint64_t B, const uint8_t* cls, const uint32_t* blk_base, const uint32_t* out, uint32_t* perm) {
    hipLaunchKernelGGL((k_part_perm<uint8_t, PR_CLASSES, PR_BLOCK>), dim3((uint32_t)((B + PR_BLOCK - 1) / PR_BLOCK)), dim3(PR_BLOCK), 0, s, B, cls, blk_base, out, perm);
}
static uint32_t aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
void launch_pr_gather(hipStream_t s, uint32_t n, const uint32_t* sel, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk, const uint32_t* which, const uint8_t* seeds,
                      uint8_t* w_msg, uint8_t* w_sig, uint8_t* w_pk, uint32_t* w_which, uint8_t* w_seeds) {
    const uint32_t al = aligned16(msg) | aligned16(sig) << 1 | aligned16(pk) << 2 | aligned16(seeds) << 3;
    if (n) hipLaunchKernelGGL(k_pr_gather, dim3((16 * n + 255) / 256), dim3(256), 0, s, n, sel, msg, sig, pk, which, seeds, al, w_msg, w_sig, w_pk, w_which, w_seeds);
}
void launch_pr_gather_rows(hipStream_t s, uint32_t n, const uint32_t* sel, const uint8_t* src, uint64_t row_bytes, uint8_t* dst) {
    if (n && row_bytes) hipLaunchKernelGGL(k_pr_gather_rows, dim3(n), dim3(256), 0, s, n, sel, src, row_bytes, aligned16(src), dst);
}
void launch_pr_record(hipStream_t s, uint32_t n, const uint32_t* sel, uint64_t seg_first, const uint64_t* w_off, const int32_t* w_st, uint64_t stage_base, uint64_t* rec_off,
                      uint64_t* rec_len, int32_t* status, int32_t st) {
    if (n) hipLaunchKernelGGL(k_pr_record, dim3((n + 255) / 256), dim3(256), 0, s, n, sel, seg_first, w_off, w_st, stage_base, rec_off, rec_len, status, st);
}
void launch_pr_offsets(hipStream_t s, uint32_t n, const uint64_t* rec_len, uint64_t base, uint64_t* out_off) {
    hipLaunchKernelGGL(k_part_offsets<1024>, dim3(1), dim3(1024), 0, s, n, rec_len, base, out_off);   // out_off[i] = base + the bytes of the segment's proofs before i
}
void launch_pr_move(hipStream_t s, uint32_t n, const uint64_t* rec_off, const uint64_t* rec_len, const uint8_t* stage, const uint64_t* out_off, uint8_t* out) {
    if (n) hipLaunchKernelGGL(k_pr_move, dim3(n), dim3(256), 0, s, n, rec_off, rec_len, stage, out_off, out);
}
