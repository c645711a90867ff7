// Mixed-ring membership calls (include/zkattest.h: zk_member_prove_batch_rings / zk_member_verify_batch_rings): the classing of a batch's ring ids, the
// offsets of the prover's output, and the gathers of one ring's inputs into a window.  The partition is partition.h's (k_part_scan, k_part_perm over
// uint8_t classes in workgroups of MR_BLOCK proofs); the index arithmetic is member_plan.h's; the membership kernels run on each window with its ring bound
// and write every result at its final place through the window's `sel` list (k_member.hip: k_m_write_head, k_mv_final).
#include "member.h"
#include "partition.h"

static_assert(MR_SLOTS == ZK_MAX_RINGS, "member_plan.h restates the number of resident rings");

// Class of every proof (member_plan.h) and, per workgroup of MR_BLOCK proofs, how many of them fall into each class: one ballot per class and wave, the
// wave's first lane adds the count to the workgroup's LDS counters (no global atomics).  The prover (proof_off == nullptr) knows two kinds of proof, of a
// resident ring or not.  The verifier also refuses here every slot whose length is not its ring's, whose offset is misaligned or whose ends are out of order
// -- a census that took equally long proofs for granted could not --, and settles both kinds of refusal itself: they never enter a window, no byte of
// their slots is read.
__global__ void __launch_bounds__(MR_BLOCK) k_mr_class(uint64_t B, const uint32_t* __restrict__ ring_ids, MrRings R, const uint64_t* __restrict__ proof_off,
                                                       uint8_t* __restrict__ cls, uint32_t* __restrict__ blk_cnt /* [blocks][MR_CLASSES] */, uint8_t* __restrict__ ok,
                                                       int32_t* __restrict__ status) {
    __shared__ uint32_t cnt[MR_CLASSES];
    if (threadIdx.x < MR_CLASSES) cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t b = (uint64_t)blockIdx.x * MR_BLOCK + threadIdx.x;
    uint32_t k = 0xffu;   // past the batch: no class
    if (b < B) {
        k = mr_class_of_id(R, ring_ids[b]);
        if (proof_off) {
            if (k < MR_SLOTS && !mr_slot_ok(proof_off[b], proof_off[b + 1], proof_off[B], R.size[k])) k = MR_BAD;
            if (k >= MR_SLOTS) ok[b] = 0, status[b] = k == MR_UNKNOWN ? ZK_E_ARG : ZK_E_BAD_ENCODING;
        }
        cls[b] = (uint8_t)k;
    }
#pragma unroll
    for (uint32_t s = 0; s < MR_CLASSES; s++) {
        const uint64_t m = __ballot(k == s);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt[s], (uint32_t)__popcll(m));
    }
    __syncthreads();
    if (threadIdx.x < MR_CLASSES) blk_cnt[(size_t)blockIdx.x * MR_CLASSES + threadIdx.x] = cnt[threadIdx.x];
}
// The prover's output offsets, in index order: a workgroup starts where the proofs of the workgroups before it end -- the scan's per-class prefix counts
// times the classes' sizes, no second scan over the batch -- and scans its own MR_BLOCK sizes through LDS.  A proof whose id is not resident is settled
// here: a zero-length slot, ZK_E_ARG, zero bytes of com and blinder_out.
__global__ void __launch_bounds__(MR_BLOCK) k_mr_offsets(uint64_t B, const uint8_t* __restrict__ cls, const uint32_t* __restrict__ blk_base, MrRings R,
                                                         uint64_t* __restrict__ out_off, uint8_t* __restrict__ com, uint8_t* __restrict__ blinder_out,
                                                         int32_t* __restrict__ status) {
    __shared__ uint32_t sc[MR_BLOCK];
    const uint32_t t = threadIdx.x;
    const uint64_t b = (uint64_t)blockIdx.x * MR_BLOCK + t;
    uint32_t k = MR_UNKNOWN;
    if (b < B) k = cls[b];
    if (k >= MR_CLASSES) k = MR_UNKNOWN;   // (a class the census cannot write: size 0, never an index past R.size)
    const uint32_t sz = b < B ? R.size[k] : 0;
    sc[t] = sz;
    __syncthreads();
    for (uint32_t d = 1; d < MR_BLOCK; d <<= 1) {   // inclusive Hillis-Steele scan
        const uint32_t v = t >= d ? sc[t - d] : 0;
        __syncthreads();
        sc[t] += v;
        __syncthreads();
    }
    if (b >= B) return;
    const uint64_t at = mr_bytes(blk_base + (size_t)blockIdx.x * MR_CLASSES, R) + sc[t] - sz;
    out_off[b] = at;
    if (b == B - 1) out_off[B] = at + sz;
    if (k >= MR_SLOTS) {
        status[b] = ZK_E_ARG;
        uint32_t* cw = (uint32_t*)(com + 72 * b);
        for (int i = 0; i < 18; i++) cw[i] = 0;
        if (blinder_out) {
            uint32_t* bw = (uint32_t*)(blinder_out + 32 * b);
            for (int i = 0; i < 8; i++) bw[i] = 0;
        }
    }
}

// 16 or 8 bytes of a caller's array: one load where the array has that alignment (al), bytes otherwise (k_prove_rings.hip: pr_load16)
ZK_DEV uint4 mr_load16(const uint8_t* __restrict__ s, bool al) {
    if (al) return *(const uint4*)s;
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = (uint32_t)s[4 * i] | ((uint32_t)s[4 * i + 1] << 8) | ((uint32_t)s[4 * i + 2] << 16) | ((uint32_t)s[4 * i + 3] << 24);
    return make_uint4(w[0], w[1], w[2], w[3]);
}
ZK_DEV uint2 mr_load8(const uint8_t* __restrict__ s, bool al) {
    if (al) return *(const uint2*)s;
    uint32_t w[2];
#pragma unroll
    for (int i = 0; i < 2; i++) w[i] = (uint32_t)s[4 * i] | ((uint32_t)s[4 * i + 1] << 8) | ((uint32_t)s[4 * i + 2] << 16) | ((uint32_t)s[4 * i + 3] << 24);
    return make_uint2(w[0], w[1]);
}
// prover: window entry j = proof sel[j].  8 threads per entry: `which`, two 16-byte pieces of the blinder (blinder == nullptr: the engine draws it), two
// of the seed (seeds == nullptr in stream mode: k_pr_gather_rows moves the rows), two of the context (a bound call).  Consecutive threads write consecutive
// pieces of the window's arrays.
__global__ void __launch_bounds__(256) k_mr_pgather(uint32_t n, uint64_t B, const uint32_t* __restrict__ sel, const uint32_t* __restrict__ which,
                                                    const uint8_t* __restrict__ blinder, const uint8_t* __restrict__ seeds, const uint8_t* __restrict__ context, uint32_t al,
                                                    uint32_t* __restrict__ w_which, uint8_t* __restrict__ w_blinder, uint8_t* __restrict__ w_seeds,
                                                    uint8_t* __restrict__ w_context) {
    const uint32_t t = gtid();
    if (t >= 8 * n) return;
    const uint32_t j = t >> 3, q = t & 7;
    const uint64_t b = sel[j];
    if (b >= B) return;
    if (q == 0) w_which[j] = which[b];
    else if (q < 3) {
        if (blinder) ((uint4*)(w_blinder + 32 * (size_t)j))[q - 1] = mr_load16(blinder + 32 * b + 16 * (q - 1), al & 1);
    } else if (q < 5) {
        if (seeds) ((uint4*)(w_seeds + 32 * (size_t)j))[q - 3] = mr_load16(seeds + 32 * b + 16 * (q - 3), al & 2);
    } else if (q < 7) {
        if (context) ((uint4*)(w_context + 32 * (size_t)j))[q - 5] = mr_load16(context + 32 * b + 16 * (q - 5), al & 4);
    }
}
// verifier: 16 threads per entry -- nine 8-byte pieces of com (72 bytes: an entry of the window starts on a multiple of 8), two 16-byte pieces of the
// verifier's seed, the slot's offset, two 16-byte pieces of the context (a bound call).  The proof bytes stay where they are: the GK kernels read them through
// the window's offsets.
__global__ void __launch_bounds__(256) k_mr_vgather(uint32_t n, uint64_t B, const uint32_t* __restrict__ sel, const uint64_t* __restrict__ proof_off,
                                                    const uint8_t* __restrict__ com, const uint8_t* __restrict__ seeds, const uint8_t* __restrict__ context, uint32_t al,
                                                    uint64_t* __restrict__ w_off, uint8_t* __restrict__ w_com, uint8_t* __restrict__ w_seeds, uint8_t* __restrict__ w_context) {
    const uint32_t t = gtid();
    if (t >= 16 * n) return;
    const uint32_t j = t >> 4, q = t & 15;
    const uint64_t b = sel[j];
    if (b >= B) return;
    if (q < 9) ((uint2*)(w_com + 72 * (size_t)j))[q] = mr_load8(com + 72 * b + 8 * q, al & 1);
    else if (q < 11) ((uint4*)(w_seeds + 32 * (size_t)j))[q - 9] = mr_load16(seeds + 32 * b + 16 * (q - 9), al & 2);
    else if (q == 11) w_off[j] = proof_off[b];
    else if (q < 14) {
        if (context) ((uint4*)(w_context + 32 * (size_t)j))[q - 12] = mr_load16(context + 32 * b + 16 * (q - 12), al & 4);
    }
}

void launch_mr_class(hipStream_t s, uint64_t B, const uint32_t* ring_ids, const MrRings& R, const uint64_t* proof_off, uint8_t* cls, uint32_t* blk_cnt, uint32_t* out,
                     uint8_t* ok, int32_t* status) {
    const uint32_t blocks = (uint32_t)((B + MR_BLOCK - 1) / MR_BLOCK);
    hipLaunchKernelGGL(k_mr_class, dim3(blocks), dim3(MR_BLOCK), 0, s, B, ring_ids, R, proof_off, cls, blk_cnt, ok, status);
    hipLaunchKernelGGL((k_part_scan<MR_CLASSES, 64>), dim3(1), dim3(64), 0, s, blocks, blk_cnt, out);
}
void launch_mr_perm(hipStream_t s, uint64_t B, const uint8_t* cls, const uint32_t* blk_base, const uint32_t* out, uint32_t* perm) {
    hipLaunchKernelGGL((k_part_perm<uint8_t, MR_CLASSES, MR_BLOCK>), dim3((uint32_t)((B + MR_BLOCK - 1) / MR_BLOCK)), dim3(MR_BLOCK), 0, s, B, cls, blk_base, out, perm);
}
void launch_mr_offsets(hipStream_t s, uint64_t B, const uint8_t* cls, const uint32_t* blk_base, const MrRings& R, uint64_t* out_off, uint8_t* com, uint8_t* blinder_out,
                       int32_t* status) {
    hipLaunchKernelGGL(k_mr_offsets, dim3((uint32_t)((B + MR_BLOCK - 1) / MR_BLOCK)), dim3(MR_BLOCK), 0, s, B, cls, blk_base, R, out_off, com, blinder_out, status);
}
static uint32_t mr_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
void launch_mr_pgather(hipStream_t s, uint32_t n, uint64_t B, const uint32_t* sel, const uint32_t* which, const uint8_t* blinder, const uint8_t* seeds, const uint8_t* context,
                       uint32_t* w_which, uint8_t* w_blinder, uint8_t* w_seeds, uint8_t* w_context) {
    const uint32_t al = mr_aligned(blinder, 16) | mr_aligned(seeds, 16) << 1 | mr_aligned(context, 16) << 2;
    if (n) hipLaunchKernelGGL(k_mr_pgather, dim3((8 * n + 255) / 256), dim3(256), 0, s, n, B, sel, which, blinder, seeds, context, al, w_which, w_blinder, w_seeds, w_context);
}
void launch_mr_vgather(hipStream_t s, uint32_t n, uint64_t B, const uint32_t* sel, const uint64_t* proof_off, const uint8_t* com, const uint8_t* seeds, const uint8_t* context,
                       uint64_t* w_off, uint8_t* w_com, uint8_t* w_seeds, uint8_t* w_context) {
    const uint32_t al = mr_aligned(com, 8) | mr_aligned(seeds, 16) << 1 | mr_aligned(context, 16) << 2;
    if (n) hipLaunchKernelGGL(k_mr_vgather, dim3((16 * n + 255) / 256), dim3(256), 0, s, n, B, sel, proof_off, com, seeds, context, al, w_off, w_com, w_seeds, w_context);
}
