// The stable partition of a batch's proofs by class, shared by per-proof verify levels (k_levels.hip: uint8_t classes, ZK_LV_CLASSES of them),
// mixed-ring verification (k_rings.hip: uint16_t classes, ring slot x level class) and mixed-ring proving (k_prove_rings.hip: uint8_t classes, one per
// ring slot, in workgroups of PR_BLOCK proofs).  A census kernel of the caller's writes every proof's class and, per workgroup of BLOCK proofs
// (LV_BLOCK unless said otherwise), how many of its proofs fall into each class (blk_cnt[blocks][NCLS]); k_part_scan and k_part_perm do the rest.
#pragma once
#include "engine.h"

// one workgroup: blk_cnt becomes, per class, the exclusive prefix over the workgroups; out[0 .. NCLS) = proofs per class (what the host reads
// back), out[NCLS ..) = where each class starts in the permutation.  Up to THREADS classes the starts are one thread's running sum; more classes
// are summed per thread over a contiguous segment and the THREADS partial sums scanned across the workgroup.
template <uint32_t NCLS, uint32_t THREADS>
__global__ void __launch_bounds__(THREADS) k_part_scan(uint32_t blocks, uint32_t* __restrict__ blk_cnt, uint32_t* __restrict__ out) {
    __shared__ uint32_t tot[NCLS];
    for (uint32_t l = threadIdx.x; l < NCLS; l += THREADS) {
        uint32_t run = 0;
#pragma unroll 8
        for (uint32_t k = 0; k < blocks; k++) {
            uint32_t* q = blk_cnt + (size_t)k * NCLS + l;
            const uint32_t v = *q;
            *q = run, run += v;
        }
        tot[l] = run;
        out[l] = run;
    }
    __syncthreads();
    if constexpr (NCLS <= THREADS) {
        if (threadIdx.x == 0) {
            uint32_t run = 0;
            for (uint32_t i = 0; i < NCLS; i++) out[NCLS + i] = run, run += tot[i];
        }
    } else {
        __shared__ uint32_t part[THREADS];
        constexpr uint32_t per = (NCLS + THREADS - 1) / THREADS;
        const uint32_t t = threadIdx.x, lo = t * per < NCLS ? t * per : NCLS, hi = lo + per < NCLS ? lo + per : NCLS;
        uint32_t sum = 0;
        for (uint32_t i = lo; i < hi; i++) sum += tot[i];
        part[t] = sum;
        __syncthreads();
        for (uint32_t d = 1; d < THREADS; d <<= 1) {   // inclusive Hillis-Steele scan of the partial sums
            const uint32_t v = t >= d ? part[t - d] : 0;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        uint32_t run = part[t] - sum;
        for (uint32_t i = lo; i < hi; i++) out[NCLS + i] = run, run += tot[i];
    }
}
// perm[start[class] + rank] = b, rank = the proof's place among the proofs of its class in index order (stable)
template <class T, uint32_t NCLS, uint32_t BLOCK = LV_BLOCK>
__global__ void __launch_bounds__(BLOCK) k_part_perm(uint64_t B, const T* __restrict__ cls, const uint32_t* __restrict__ blk_base, const uint32_t* __restrict__ out,
                                                        uint32_t* __restrict__ perm) {
    __shared__ T sc[BLOCK];
    const uint64_t b = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t l = b < B ? (uint32_t)cls[b] : (uint32_t)(T)~0u;
    sc[threadIdx.x] = (T)l;
    __syncthreads();
    if (b >= B) return;
    uint32_t rank = 0;
    for (uint32_t j = 0; j < threadIdx.x; j++) rank += sc[j] == l;   // (every lane of a wave reads the same entry: an LDS broadcast)
    perm[out[NCLS + l] + blk_base[(size_t)blockIdx.x * NCLS + l] + rank] = (uint32_t)b;
}
// lengths -> offsets: off[j] = base + the sum of len[0 .. j), off[n] = base + all of them (one workgroup; len == off turns lengths into offsets in
// place).  Every thread sums a contiguous run of ceil(n / THREADS) lengths, the THREADS partial sums are scanned across the workgroup.
template <uint32_t THREADS>
__global__ void __launch_bounds__(THREADS) k_part_offsets(uint32_t n, const uint64_t* len, uint64_t base, uint64_t* off) {
    __shared__ uint64_t sb[THREADS];
    const uint64_t t = threadIdx.x, per = ((uint64_t)n + (THREADS - 1)) / THREADS;
    const uint64_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    uint64_t sum = 0;
    for (uint64_t j = lo; j < hi; j++) sum += len[j];
    sb[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < THREADS; d <<= 1) {   // inclusive Hillis-Steele scan of the THREADS partial sums
        const uint64_t v = t >= d ? sb[t - d] : 0;
        __syncthreads();
        sb[t] += v;
        __syncthreads();
    }
    uint64_t run = base + sb[t] - sum;
    for (uint64_t j = lo; j < hi; j++) {
        const uint64_t v = len[j];
        off[j] = run, run += v;
    }
    if (t == (THREADS - 1)) off[n] = base + sb[(THREADS - 1)];
}
