// Exhaustive verify mode (include/zkattest.h: zk_ctx_set_verify_reps, ZK_VERIFY_REPS_ALL): every repetition of a proof is checked, VK at a time, in
// P = ceil(sec / VK) passes over the unchanged pipeline (api_verify.hip: verify_device).  A pass differs from a sampled call in ONE kernel -- k_v_sample_all
// names the pass's VK repetitions in ascending order where k_v_sample_fills + k_v_sample draw generateIndices' subset -- and k_v_merge_pass folds the
// verdicts of a later pass into the caller's.
#include "engine.h"

// Pass r checks repetitions VK r .. VK r + VK - 1; the last pass checks sec - VK .. sec - 1 (it overlaps the pass before it where VK does not divide sec).
// What k_v_sample leaves behind, and nothing else: the slots' repetitions with the bit the proof's HEADER claims for each, and "no identity found yet".
__global__ void __launch_bounds__(64) k_v_sample_all(VWork V, uint32_t count, uint32_t pass) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint32_t base = VK * pass + VK <= V.sec ? VK * pass : V.sec - VK;   // (V.sec >= VK: a level below VK never samples)
    const uint32_t* hb = V.hbits + 4 * p;
    for (uint32_t j = 0; j < VK; j++) {
        const uint32_t i = base + j;
        V.idx[p * VK + j] = i | (((hb[i >> 5] >> (i & 31)) & 1) << 8);
    }
    V.exp_jz[p] = VK;
}
// Verdicts of pass r > 0 into the caller's: a proof is accepted if every pass accepts it, and its status is that of the first pass that has one -- the
// passes walk the repetitions in ascending order, so that is the exception of the lowest repetition that throws (structural errors and a failed
// membership check are the same in every pass).
__global__ void __launch_bounds__(256) k_v_merge_pass(uint64_t B, const uint8_t* __restrict__ ok_r, const int32_t* __restrict__ st_r, uint8_t* __restrict__ ok,
                                                      int32_t* __restrict__ status) {
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    ok[b] &= ok_r[b];
    const int32_t st = status[b];
    status[b] = st ? st : st_r[b];
}

void launch_v_sample_all(hipStream_t s, const VWork& V, uint32_t count, uint32_t pass) {   // needs the header only
    hipLaunchKernelGGL(k_v_sample_all, dim3((count + 63) / 64), dim3(64), 0, s, V, count, pass);
}
void launch_v_merge_pass(hipStream_t s, uint64_t B, const uint8_t* ok_r, const int32_t* st_r, uint8_t* ok, int32_t* status) {
    hipLaunchKernelGGL(k_v_merge_pass, dim3((uint32_t)((B + 255) / 256)), dim3(256), 0, s, B, ok_r, st_r, ok, status);
}
