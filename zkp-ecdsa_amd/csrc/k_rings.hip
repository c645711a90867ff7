// Mixed-ring verification (include/zkattest.h: zk_verify_batch_rings): the census of a batch's (ring, level) classes.  The partition itself is the
// per-level one's (partition.h: k_part_scan, k_part_perm over uint16_t classes), and so are the gather into windows and the scatter of the verdicts
// (k_levels.hip); the verifier's kernels run unchanged on each window with its ring bound (api_verify.hip).
#include "partition.h"

// class of every proof: slot * ZK_LV_CLASSES + level class, where slot is the place of the proof's ring id in rs.id and the level class is
// wire_level_class (per-proof levels) or 0 (every well-formed header at the context's level), ZK_LV_BAD for a malformed header either way;
// RG_UNKNOWN for an id that is not resident.  Per workgroup, how many of its proofs fall into each class (LDS counters, no global atomics).
__global__ void __launch_bounds__(LV_BLOCK) k_rg_census(uint64_t B, const uint32_t* __restrict__ ring_ids, RingSlots rs, const uint8_t* __restrict__ proofs,
                                                        const uint64_t* __restrict__ off, uint32_t packed, uint32_t per_proof, uint16_t* __restrict__ cls,
                                                        uint32_t* __restrict__ blk_cnt /* [blocks][RG_CLASSES] */) {
    __shared__ uint32_t cnt[RG_CLASSES];
    for (uint32_t i = threadIdx.x; i < RG_CLASSES; i += LV_BLOCK) cnt[i] = 0;
    __syncthreads();
    const uint64_t b = (uint64_t)blockIdx.x * LV_BLOCK + threadIdx.x;
    if (b < B) {
        const uint32_t id = ring_ids[b];
        uint32_t slot = ZK_MAX_RINGS;
#pragma unroll
        for (uint32_t s = 0; s < ZK_MAX_RINGS; s++)
            if (s < rs.count && rs.id[s] == id) slot = s;
        uint32_t k = RG_UNKNOWN;
        if (slot < ZK_MAX_RINGS) {
            const uint64_t o0 = off[b], o1 = off[b + 1];
            uint32_t l = o1 >= o0 + ZK_HDR ? wire_level_class(proofs + o0, o0, o1, wire_make(packed != 0)) : ZK_LV_BAD;
            if (!per_proof && l != ZK_LV_BAD) l = 0;
            k = slot * ZK_LV_CLASSES + l;
        }
        cls[b] = (uint16_t)k;
        atomicAdd(&cnt[k], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < RG_CLASSES; i += LV_BLOCK) blk_cnt[(size_t)blockIdx.x * RG_CLASSES + i] = cnt[i];
}

void launch_rg_census(hipStream_t s, uint64_t B, const uint32_t* ring_ids, const RingSlots& rs, const uint8_t* proofs, const uint64_t* off, bool packed, bool per_proof,
                      uint16_t* cls, uint32_t* blk_cnt, uint32_t* out) {
    const uint32_t blocks = (uint32_t)((B + LV_BLOCK - 1) / LV_BLOCK);
    hipLaunchKernelGGL(k_rg_census, dim3(blocks), dim3(LV_BLOCK), 0, s, B, ring_ids, rs, proofs, off, packed ? 1u : 0u, per_proof ? 1u : 0u, cls, blk_cnt);
    hipLaunchKernelGGL((k_part_scan<RG_CLASSES, 1024>), dim3(1), dim3(1024), 0, s, blocks, blk_cnt, out);
}
void launch_rg_perm(hipStream_t s, uint64_t B, const uint16_t* cls, const uint32_t* blk_base, const uint32_t* out, uint32_t* perm) {
    hipLaunchKernelGGL((k_part_perm<uint16_t, RG_CLASSES>), dim3((uint32_t)((B + LV_BLOCK - 1) / LV_BLOCK)), dim3(LV_BLOCK), 0, s, B, cls, blk_base, out, perm);
}
