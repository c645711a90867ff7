// Re-ring proofs with one destination ring id per proof (include/zkattest.h: zk_proof_rering_batch_rings): the kernels of the call's front end -- the
// census that classes every proof against ITS ring and measures its output slot, the offsets over the whole batch, the mover of all heads, the zero-fill of
// the slots of proofs that failed behind the census -- and the sel-indexed forms of k_rering.hip's front, compare and place kernels, which run on one window
// of one ring's proofs.  The plan's arithmetic is rering_plan.h's, the partition is partition.h's (k_part_scan, k_part_perm over uint8_t classes in
// workgroups of MR_BLOCK proofs), the window gathers are k_member_rings.hip's and k_prove_rings.hip's (k_mr_pgather, k_pr_gather_rows), everything between
// front and place is the member lanes' (api_member.hip).
#include "member.h"
#include "partition.h"
#include "rering.h"

typedef Fe<ModQ, 1> Sq;
typedef Fe<ModT, 1> St;

// ------------------------------------------------------------------ census
// One lane per proof, header bytes only (rrr_plan_proof: rules 1-3).  Per workgroup of MR_BLOCK proofs: how many fall into each class -- one ballot per class
// and wave, the wave's first lane adds the count to the workgroup's LDS counters, as k_mr_class does --, the bytes of their slots and how many pass rules 1-3
// with another n than their ring's.  No global atomics: k_part_scan and k_rrr_totals sum over the workgroups.  Nothing the caller sees is written here.
__global__ void __launch_bounds__(MR_BLOCK) k_rrr_census(uint64_t B, const uint8_t* __restrict__ proofs, const uint64_t* __restrict__ off, const uint32_t* __restrict__ which,
                                                         const uint32_t* __restrict__ ids, Wire wire, RrRings R, RrCensus X) {
    __shared__ uint32_t cnt[MR_CLASSES];
    __shared__ unsigned long long sb[MR_BLOCK / 64], so[MR_BLOCK / 64];
    if (threadIdx.x < MR_CLASSES) cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t b = (uint64_t)blockIdx.x * MR_BLOCK + threadIdx.x;
    uint32_t k = 0xffu;   // past the batch: no class
    unsigned long long bytes = 0, other = 0;
    if (b < B) {
        const RrPlan p = rrr_plan_proof(R, wire, proofs, off[b], off[b + 1], ids[b], which[b]);
        k = p.cls, bytes = p.len, other = p.other;
        X.cls[b] = (uint8_t)k, X.len[b] = p.len, X.head[b] = p.head;
    }
#pragma unroll
    for (uint32_t s = 0; s < MR_CLASSES; s++) {
        const uint64_t m = __ballot(k == s);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt[s], (uint32_t)__popcll(m));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bytes += __shfl_down(bytes, o, 64), other += __shfl_down(other, o, 64);
    if ((threadIdx.x & 63) == 0) sb[threadIdx.x >> 6] = bytes, so[threadIdx.x >> 6] = other;
    __syncthreads();
    if (threadIdx.x < MR_CLASSES) X.blk_cnt[(size_t)blockIdx.x * MR_CLASSES + threadIdx.x] = cnt[threadIdx.x];
    if (threadIdx.x == 0) {
        unsigned long long tb = 0, to = 0;
        for (int i = 0; i < MR_BLOCK / 64; i++) tb += sb[i], to += so[i];
        X.blk_bytes[blockIdx.x] = tb, X.blk_other[blockIdx.x] = to;
    }
}
// One workgroup, k_part_offsets' scan: blk_bytes becomes the exclusive prefix over the workgroups (blk_bytes[blocks] = the batch's bytes); the counters the
// host reads back.
__global__ void __launch_bounds__(1024) k_rrr_totals(uint32_t blocks, uint64_t B, const uint64_t* __restrict__ off, RrCensus X) {
    __shared__ uint64_t sb[1024], so[1024];
    const uint64_t t = threadIdx.x, per = ((uint64_t)blocks + 1023) / 1024;
    const uint64_t lo = t * per < blocks ? t * per : blocks, hi = lo + per < blocks ? lo + per : blocks;
    uint64_t sum = 0, osum = 0;
    for (uint64_t j = lo; j < hi; j++) sum += X.blk_bytes[j], osum += X.blk_other[j];
    sb[t] = sum, so[t] = osum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {   // inclusive Hillis-Steele scan of the partial sums
        const uint64_t v = t >= d ? sb[t - d] : 0, w = t >= d ? so[t - d] : 0;
        __syncthreads();
        sb[t] += v, so[t] += w;
        __syncthreads();
    }
    uint64_t run = sb[t] - sum;
    for (uint64_t j = lo; j < hi; j++) {
        const uint64_t v = X.blk_bytes[j];
        X.blk_bytes[j] = run, run += v;
    }
    if (t == 1023) X.blk_bytes[blocks] = sb[1023], X.cnt[0] = sb[1023], X.cnt[1] = so[1023], X.cnt[2] = off[B], X.cnt[3] = 0;
}
void launch_rrr_census(hipStream_t s, uint64_t B, const uint8_t* proofs, const uint64_t* off, const uint32_t* which, const uint32_t* ids, const Wire& wire, const RrRings& R,
                       const RrCensus& X) {
    const uint32_t blocks = (uint32_t)((B + MR_BLOCK - 1) / MR_BLOCK);
    hipLaunchKernelGGL(k_rrr_census, dim3(blocks), dim3(MR_BLOCK), 0, s, B, proofs, off, which, ids, wire, R, X);
    hipLaunchKernelGGL((k_part_scan<MR_CLASSES, 64>), dim3(1), dim3(64), 0, s, blocks, X.blk_cnt, X.cls_tot);
    hipLaunchKernelGGL(k_rrr_totals, dim3(1), dim3(1024), 0, s, blocks, B, off, X);
}

// ------------------------------------------------------------------ offsets
// The exclusive scan of the slots' lengths over the whole batch, in index order: a workgroup starts where the workgroups before it end (blk_bytes) and scans
// its own MR_BLOCK lengths through LDS.  The lengths are the census', real ones: heads differ from proof to proof.  In place the slots stay where they are:
// out_off is a copy of proof_off.  A proof refused by rules 1-3 is settled here.
__global__ void __launch_bounds__(MR_BLOCK) k_rrr_offsets(uint64_t B, RrCensus X, const uint64_t* __restrict__ proof_off, uint32_t in_place, uint64_t* __restrict__ out_off,
                                                          int32_t* __restrict__ status) {
    __shared__ uint64_t sc[MR_BLOCK];
    const uint32_t t = threadIdx.x;
    const uint64_t b = (uint64_t)blockIdx.x * MR_BLOCK + t;
    const uint64_t len = b < B ? X.len[b] : 0;
    sc[t] = len;
    __syncthreads();
    for (uint32_t d = 1; d < MR_BLOCK; d <<= 1) {   // inclusive Hillis-Steele scan
        const uint64_t v = t >= d ? sc[t - d] : 0;
        __syncthreads();
        sc[t] += v;
        __syncthreads();
    }
    if (b >= B) return;
    if (in_place) {
        if (out_off != proof_off) {
            out_off[b] = proof_off[b];
            if (b == B - 1) out_off[B] = proof_off[B];
        }
    } else {
        const uint64_t at = X.blk_bytes[blockIdx.x] + sc[t] - len;
        out_off[b] = at;
        if (b == B - 1) out_off[B] = at + len;
    }
    const uint32_t k = X.cls[b];
    if (k >= MR_SLOTS) status[b] = rrr_class_status(k);
}
void launch_rrr_offsets(hipStream_t s, uint64_t B, const RrCensus& X, const uint64_t* proof_off, bool in_place, uint64_t* out_off, int32_t* status) {
    hipLaunchKernelGGL(k_rrr_offsets, dim3((uint32_t)((B + MR_BLOCK - 1) / MR_BLOCK)), dim3(MR_BLOCK), 0, s, B, X, proof_off, in_place ? 1u : 0u, out_off, status);
}
void launch_rrr_perm(hipStream_t s, uint64_t B, const RrCensus& X) {
    hipLaunchKernelGGL((k_part_perm<uint8_t, MR_CLASSES, MR_BLOCK>), dim3((uint32_t)((B + MR_BLOCK - 1) / MR_BLOCK)), dim3(MR_BLOCK), 0, s, B, X.cls, X.blk_cnt, X.cls_tot, X.perm);
}

// ------------------------------------------------------------------ the heads
// k_rr_move's method over the whole batch at once -- the layout depends on no window --: the work is divided by BYTES, a lane owns one 16-byte aligned unit
// of [out + out_off[0], out + out_off[B]) per step, finds the proof it lies in (the proof of its last unit, else by bisection over the offsets) and moves it
// with one 16-byte load and store; a unit that is not wholly inside one head -- a proof's first 16 bytes with the two header words to patch (total_len, and n:
// the n of THIS proof's destination ring), a unit across two proofs or into a GKProof section, which the windows' writers fill -- goes dword by dword.
#define RRR_SPAN 4096u
ZK_DEV uint64_t rrr_find(const uint64_t* __restrict__ oo, uint64_t count, uint64_t x) {   // the proof j with oo[j] <= x < oo[j + 1]; oo[0] <= x < oo[count]
    uint64_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (oo[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}
__global__ void __launch_bounds__(256) k_rrr_move(uint64_t B, const uint32_t* __restrict__ head, const uint8_t* __restrict__ cls, RrRings R, const uint8_t* __restrict__ proofs,
                                                  const uint64_t* __restrict__ off, const uint64_t* __restrict__ oo, uint8_t* __restrict__ out) {
    const uint64_t lo = oo[0], hi = oo[B];
    if (hi == lo) return;
    const uintptr_t A = ((uintptr_t)out + lo) & ~(uintptr_t)15;
    const uint64_t units = ((uintptr_t)out + hi - A + 15) >> 4;
    uint64_t j = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * RRR_SPAN; base < units; base += (uint64_t)gridDim.x * RRR_SPAN) {
        for (uint32_t k = threadIdx.x; k < RRR_SPAN && base + k < units; k += 256) {
            const int64_t d0 = (int64_t)(A + 16 * (base + k) - (uintptr_t)out);   // the unit's place in `out`; the span's first unit may start in front of it
            if (d0 >= (int64_t)lo && (uint64_t)d0 + 16 <= hi) {
                if (!(oo[j] <= (uint64_t)d0 && (uint64_t)d0 < oo[j + 1])) j = rrr_find(oo, B, (uint64_t)d0);
                const uint64_t pos = (uint64_t)d0 - oo[j];
                if (pos >= 16 && pos + 16 <= head[j]) {
                    const uint8_t* src = proofs + off[j] + pos;
                    uint4 v;
                    if (((uintptr_t)src & 15) == 0) v = *(const uint4*)src;
                    else {
                        const uint32_t* q = (const uint32_t*)src;
                        v = make_uint4(q[0], q[1], q[2], q[3]);
                    }
                    *(uint4*)(out + d0) = v;
                    continue;
                }
            }
            for (int q4 = 0; q4 < 4; q4++) {
                const int64_t x = d0 + 4 * q4;
                if (x < (int64_t)lo || (uint64_t)x >= hi) continue;
                const uint64_t jj = rrr_find(oo, B, (uint64_t)x);
                const uint64_t pos = (uint64_t)x - oo[jj];
                if (pos >= head[jj]) continue;
                uint32_t v = *(const uint32_t*)(proofs + off[jj] + pos);
                if (pos == 4) v = bswap32((uint32_t)(oo[jj + 1] - oo[jj]));
                if (pos == 12) v = bswap32(cls[jj] < MR_SLOTS ? R.n[cls[jj]] : 0);
                *(uint32_t*)(out + x) = v;
            }
        }
    }
}
void launch_rrr_move(hipStream_t s, uint64_t B, const RrCensus& X, const RrRings& R, const uint8_t* proofs, const uint64_t* off, const uint64_t* out_off, uint8_t* out) {
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(4096, std::max<uint64_t>(1, B) * 16);
    hipLaunchKernelGGL(k_rrr_move, dim3(blocks), dim3(256), 0, s, B, X.head, X.cls, R, proofs, off, out_off, out);
}

// ------------------------------------------------------------------ blank
// One wave per proof: the slot of a proof that failed its opening or its RNG stream (its head was moved before that was known) becomes zero bytes, which is
// ZK_E_BAD_ENCODING to every verifier.  Slots and offsets are multiples of 4 bytes.
__global__ void __launch_bounds__(256) k_rrr_blank(uint64_t B, const uint64_t* __restrict__ out_off, const int32_t* __restrict__ status, uint8_t* __restrict__ out) {
    const uint64_t b = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B || status[b] == ZK_OK) return;
    const uint64_t o0 = out_off[b], o1 = out_off[b + 1];
    for (uint64_t x = o0 + 4 * (threadIdx.x & 63); x + 4 <= o1; x += 256) *(uint32_t*)(out + x) = 0;
}
void launch_rrr_blank(hipStream_t s, uint64_t B, const uint64_t* out_off, const int32_t* status, uint8_t* out) {
    hipLaunchKernelGGL(k_rrr_blank, dim3((uint32_t)((B + 3) / 4)), dim3(256), 0, s, B, out_off, status, out);
}

// ------------------------------------------------------------------ a window's front end, comparison and places
// `tc` big-endian bytes at any alignment -> nine little-endian words
ZK_DEV void rrr_load_coord(const uint8_t* p, uint32_t tc, uint32_t w[9]) {
#pragma unroll
    for (int i = 0; i < 9; i++) w[i] = 0;
    for (uint32_t i = 0; i < tc; i++) w[i >> 2] |= (uint32_t)p[tc - 1 - i] << (8 * (i & 3));
}
// the proof of the batch behind window entry e; B (no proof) for an entry the permutation cannot have written
ZK_DEV uint64_t rrr_proof(const uint32_t* __restrict__ sel, uint64_t e, uint64_t B) {
    const uint64_t b = sel ? sel[e] : e;
    return b < B ? b : B;
}
// k_rr_front for window entry e = first + p, which is proof b = sel[e] of the batch: header and offsets are read at b from the caller's arrays, index and
// blinder at e from the window's gathered ones (sel == nullptr: the caller's own, e = b).  W is bound to the window's ring, so W.N and W.n are that ring's.
// It writes what k_rr_front writes; an entry that names no proof of the batch is failed here and nothing of it is read.
__global__ void __launch_bounds__(64) k_rrr_front(Workspace W, RrLane X, uint32_t count, uint64_t first, const uint32_t* __restrict__ sel, uint64_t B,
                                                  const uint8_t* __restrict__ proofs, const uint64_t* __restrict__ off, const uint32_t* __restrict__ which,
                                                  const uint8_t* __restrict__ blinder, uint32_t* which_s) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint64_t e = first + p, b = rrr_proof(sel, e, B);
    const bool there = b < B;
    const uint64_t o0 = there ? off[b] : 0;
    RrHead h{false, 0, 0, 0};
    if (there) h = rr_head(proofs, o0, off[b + 1], W.wire);
    const uint32_t w = there ? which[e] : 0;
    const bool inside = there && w < W.N;
    const int32_t st = !there ? ZK_E_ARG : !h.ok ? ZK_E_BAD_ENCODING : !inside ? ZK_E_ARG : ZK_OK;
    const uint32_t ndraw = 5 * W.n, cnt = W.rng.exc_cnt[p];
    uint32_t rej = 0;
    for (uint32_t i = 0; i < (cnt < RNG_MAX_EXC ? cnt : RNG_MAX_EXC); i++) rej += (W.rng.exc_flags[p * RNG_MAX_EXC + i] >> 1) & 1;
    X.flags[p] = cnt > RNG_MAX_EXC || (W.rng.mode == 1 && ndraw + rej > W.rng.stride_blocks);
    uint32_t bw[8];
#pragma unroll
    for (int i = 0; i < 8; i++) bw[i] = 0;
    if (there) load_be32(blinder + 32 * e, bw);
    const Sq r = fe_from_words256_reduce<ModQ>(bw);   // newScalar reduces (group.ts:164-167)
    W.st[p] = st;
    W.zcnt[p] = 0;
    which_s[p] = inside ? w : 0;
    soa_st(W.gk_blind, p, r);
    soa_st(W.lc.v, 4 * W.n * count + p, soa_ld<ModQ, 1>(W.ring, inside ? w : 0));
    soa_st(W.lc.r, 4 * W.n * count + p, r);
    X.head[p] = st == ZK_OK ? h.head : 0;
    uint32_t kw[18];
#pragma unroll
    for (int i = 0; i < 18; i++) kw[i] = 0;
    Sq rx = fe_zero<ModQ>(), ry = fe_zero<ModQ>();
    if (h.ok) {
        const uint8_t* pr = proofs + o0;
        rrr_load_coord(pr + ZK_HDR + 128, W.wire.tc, kw);
        rrr_load_coord(pr + ZK_HDR + 128 + W.wire.tc, W.wire.tc, kw + 9);
        if (W.gk_stmt == GK_STMT_FULL) {   // a coordinate in [p, 2^256) enters the hash reduced, as in the verifier
            load_be32(pr + ZK_HDR, bw);
            rx = fe_from_words256_reduce<ModQ>(bw);
            load_be32(pr + ZK_HDR + 32, bw);
            ry = fe_from_words256_reduce<ModQ>(bw);
        }
    }
#pragma unroll
    for (int i = 0; i < 18; i++) X.kx[18 * p + i] = kw[i];
    if (W.gk_stmt == GK_STMT_FULL) {
        St kx, ky;
        limbs_from_words<9>(kx.l, kw), limbs_from_words<9>(ky.l, kw + 9);
        soa_st(X.Rx, p, rx), soa_st(X.Ry, p, ry);
        soa_st(X.kax, 2 * p, kx), soa_st(X.kay, 2 * p, ky);
    }
}
void launch_rrr_front(hipStream_t s, const Workspace& W, const RrLane& X, uint32_t count, uint64_t first, const uint32_t* sel, uint64_t B, const uint8_t* proofs,
                      const uint64_t* off, const uint32_t* which, const uint8_t* blinder, uint32_t* which_s) {
    hipLaunchKernelGGL(k_rrr_front, dim3((count + 63) / 64), dim3(64), 0, s, W, X, count, first, sel, B, proofs, off, which, blinder, which_s);
}
// k_rr_compare, the final status scattered to the proof's place in the batch
__global__ void __launch_bounds__(64) k_rrr_compare(Workspace W, RrLane X, uint32_t count, uint64_t first, const uint32_t* __restrict__ sel, uint64_t B,
                                                    int32_t* __restrict__ status) {
    const uint32_t p = gtid();
    if (p >= count) return;
    int32_t st = W.st[p];
    if (st == ZK_OK) {
        const uint32_t e = 4 * W.n * count + p;
        uint32_t cx[9], cy[9];
        words_from_limbs<9>(cx, soa_ld<ModT, 1>(W.lc.ax, e).l);
        words_from_limbs<9>(cy, soa_ld<ModT, 1>(W.lc.ay, e).l);
        uint32_t diff = 0;
#pragma unroll
        for (int i = 0; i < 9; i++) diff |= (cx[i] ^ X.kx[18 * p + i]) | (cy[i] ^ X.kx[18 * p + 9 + i]);
        if (diff) st = ZK_E_OPENING;
        else if (X.flags[p] & 1) st = ZK_E_RNG_EXHAUSTED;
    }
    W.st[p] = st;
    const uint64_t b = rrr_proof(sel, first + p, B);
    if (b < B) status[b] = st;
}
void launch_rrr_compare(hipStream_t s, const Workspace& W, const RrLane& X, uint32_t count, uint64_t first, const uint32_t* sel, uint64_t B, int32_t* status) {
    hipLaunchKernelGGL(k_rrr_compare, dim3((count + 63) / 64), dim3(64), 0, s, W, X, count, first, sel, B, status);
}
// where the window's writers put proof p's GKProof section: behind its head in its slot of the batch (the offsets kernel ran before the windows)
__global__ void __launch_bounds__(256) k_rrr_place(Workspace W, RrLane X, uint32_t count, uint64_t first, const uint32_t* __restrict__ sel, uint64_t B,
                                                   const uint64_t* __restrict__ out_off) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint64_t b = rrr_proof(sel, first + p, B);
    W.out_base[p] = (b < B ? out_off[b] : 0) + X.head[p];   // (an entry without a proof has failed: nothing of it is written)
}
void launch_rrr_place(hipStream_t s, const Workspace& W, const RrLane& X, uint32_t count, uint64_t first, const uint32_t* sel, uint64_t B, const uint64_t* out_off) {
    hipLaunchKernelGGL(k_rrr_place, dim3((count + 255) / 256), dim3(256), 0, s, W, X, count, first, sel, B, out_off);
}
