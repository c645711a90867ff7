// Per-proof verify levels (include/zkattest.h: zk_ctx_set_verify_level): the census of a batch's header levels, the stable partition of its
// proofs by level, the gather of one level's proofs into a contiguous window (bytes, offsets as prefix sums, message hashes, verifier seeds) and
// the scatter of the window's verdicts back to the proofs' own indices.  The verifier's kernels run unchanged on the window (api_verify.hip).
#include "partition.h"

// class of every proof (wire_level_class: 0..128, or ZK_LV_BAD) and, per workgroup, how many of its proofs fall into each class
__global__ void __launch_bounds__(LV_BLOCK) k_lv_census(uint64_t B, const uint8_t* __restrict__ proofs, const uint64_t* __restrict__ off, uint32_t packed,
                                                        uint8_t* __restrict__ cls, uint32_t* __restrict__ blk_cnt /* [blocks][ZK_LV_CLASSES] */) {
    __shared__ uint32_t cnt[ZK_LV_CLASSES];
    for (uint32_t i = threadIdx.x; i < ZK_LV_CLASSES; i += LV_BLOCK) cnt[i] = 0;
    __syncthreads();
    const uint64_t b = (uint64_t)blockIdx.x * LV_BLOCK + threadIdx.x;
    if (b < B) {
        const uint64_t o0 = off[b], o1 = off[b + 1];
        const uint32_t l = o1 >= o0 + ZK_HDR ? wire_level_class(proofs + o0, o0, o1, wire_make(packed != 0)) : ZK_LV_BAD;
        cls[b] = (uint8_t)l;
        atomicAdd(&cnt[l], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < ZK_LV_CLASSES; i += LV_BLOCK) blk_cnt[(size_t)blockIdx.x * ZK_LV_CLASSES + i] = cnt[i];
}
// window entry j = proof sel[j]: its length (turned into offsets by k_part_offsets), message hash and verifier seed
__global__ void __launch_bounds__(256) k_lv_gather_meta(uint32_t n, const uint32_t* __restrict__ sel, const uint64_t* __restrict__ off, const uint8_t* __restrict__ msg,
                                                        const uint8_t* __restrict__ vseeds, uint64_t* __restrict__ w_len, uint8_t* __restrict__ w_msg, uint8_t* __restrict__ w_seeds) {
    const uint32_t t = gtid();   // 8 threads per entry: one 16-byte piece of the message hash or of the seed each, and the length
    if (t >= 8 * n) return;
    const uint32_t j = t >> 3, q = t & 7;
    const uint64_t b = sel[j];
    if (q < 2) ((uint4*)(w_msg + 32 * (size_t)j))[q] = ((const uint4*)(msg + 32 * b))[q];
    else if (q < 4) ((uint4*)(w_seeds + 32 * (size_t)j))[q - 2] = ((const uint4*)(vseeds + 32 * b))[q - 2];
    else if (q == 4) w_len[j] = off[b + 1] - off[b];
}
// the bytes: one workgroup per window entry, 16-byte stores at 16-byte aligned destinations; the source is read with 16-byte loads where it has the same
// alignment mod 16, as four dwords otherwise (offsets are 4-byte aligned, k_lv_census refused every other proof)
__global__ void __launch_bounds__(256) k_lv_gather_bytes(uint32_t n, const uint32_t* __restrict__ sel, const uint64_t* __restrict__ off, const uint8_t* __restrict__ proofs,
                                                         const uint64_t* __restrict__ w_off, uint8_t* __restrict__ w_bytes) {
    const uint32_t j = blockIdx.x, t = threadIdx.x;
    if (j >= n) return;
    const uint64_t b = sel[j];
    const uint32_t* src = (const uint32_t*)(proofs + off[b]);
    uint32_t* dst = (uint32_t*)(w_bytes + w_off[j]);
    const uint64_t nd = (w_off[j + 1] - w_off[j]) >> 2;
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
// verdicts of window entry j -> proof sel[j]; st_only: ok = 0 and status `st` for every proof of sel (the class of malformed headers)
__global__ void __launch_bounds__(256) k_lv_scatter(uint32_t n, const uint32_t* __restrict__ sel, const uint8_t* __restrict__ w_ok, const int32_t* __restrict__ w_st,
                                                    uint8_t* __restrict__ ok, int32_t* __restrict__ status, int32_t st) {
    const uint32_t j = gtid();
    if (j >= n) return;
    const uint64_t b = sel[j];
    ok[b] = w_ok ? w_ok[j] : 0;
    status[b] = w_ok ? w_st[j] : st;
}

void launch_lv_census(hipStream_t s, uint64_t B, const uint8_t* proofs, const uint64_t* off, bool packed, uint8_t* cls, uint32_t* blk_cnt, uint32_t* out) {
    const uint32_t blocks = (uint32_t)((B + LV_BLOCK - 1) / LV_BLOCK);
    hipLaunchKernelGGL(k_lv_census, dim3(blocks), dim3(LV_BLOCK), 0, s, B, proofs, off, packed ? 1u : 0u, cls, blk_cnt);
    hipLaunchKernelGGL((k_part_scan<ZK_LV_CLASSES, 256>), dim3(1), dim3(256), 0, s, blocks, blk_cnt, out);
}
void launch_lv_perm(hipStream_t s, uint64_t B, const uint8_t* cls, const uint32_t* blk_base, const uint32_t* out, uint32_t* perm) {
    hipLaunchKernelGGL((k_part_perm<uint8_t, ZK_LV_CLASSES>), dim3((uint32_t)((B + LV_BLOCK - 1) / LV_BLOCK)), dim3(LV_BLOCK), 0, s, B, cls, blk_base, out, perm);
}
void launch_lv_gather_meta(hipStream_t s, uint32_t n, const uint32_t* sel, const uint64_t* off, const uint8_t* msg, const uint8_t* vseeds, uint64_t* w_off, uint8_t* w_msg,
                           uint8_t* w_seeds) {
    hipLaunchKernelGGL(k_lv_gather_meta, dim3((8 * n + 255) / 256), dim3(256), 0, s, n, sel, off, msg, vseeds, w_off, w_msg, w_seeds);
    hipLaunchKernelGGL(k_part_offsets<1024>, dim3(1), dim3(1024), 0, s, n, w_off, (uint64_t)0, w_off);   // lengths -> offsets in place, w_off[n] = the window's bytes
}
void launch_lv_gather_bytes(hipStream_t s, uint32_t n, const uint32_t* sel, const uint64_t* off, const uint8_t* proofs, const uint64_t* w_off, uint8_t* w_bytes) {
    hipLaunchKernelGGL(k_lv_gather_bytes, dim3(n), dim3(256), 0, s, n, sel, off, proofs, w_off, w_bytes);
}
void launch_lv_scatter(hipStream_t s, uint32_t n, const uint32_t* sel, const uint8_t* w_ok, const int32_t* w_st, uint8_t* ok, int32_t* status, int32_t st) {
    if (n) hipLaunchKernelGGL(k_lv_scatter, dim3((n + 255) / 256), dim3(256), 0, s, n, sel, w_ok, w_st, ok, status, st);
}
