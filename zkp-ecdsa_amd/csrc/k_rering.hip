// Re-ring proofs (include/zkattest.h: zk_proof_rering_batch): the kernels around the membership prover when its GKProof goes INTO a ZKA1 proof -- the
// census that decides the call, the front end (header, offsets, keyXcom and R read from the proof, the opening the caller claims), the comparison of that
// opening with keyXcom, the scan of the new lengths and the mover of the proofs' heads.  Fold, commitments, challenge hash and responses are the member
// lanes' (api_member.hip: k_scalar.hip, k_gk*.hip, k_tom.hip, k_hash.hip), run with W.wire.fixed = 0 and W.out_base[p] = where proof p's section starts.
#include "rering.h"

typedef Fe<ModQ, 1> Sq;
typedef Fe<ModT, 1> St;

// ------------------------------------------------------------------ census
// One lane per proof, header bytes only.  cnt[0] += the new length of every proof that can still succeed (well-formed, index inside the ring): what the output
// needs at most, known before anything is computed; cnt[1] += well-formed proofs whose n is not the ring's (the in-place rule); cnt[2] = proof_off[B].
__global__ void __launch_bounds__(256) k_rr_census(uint64_t B, const uint8_t* __restrict__ proofs, const uint64_t* __restrict__ off, const uint32_t* __restrict__ which, Wire wire,
                                                   uint32_t n, uint32_t N, unsigned long long* cnt) {
    __shared__ unsigned long long sb[4], sm[4];
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long bytes = 0, other = 0;
    if (b < B) {
        const RrHead h = rr_head(proofs, off[b], off[b + 1], wire);
        if (h.ok) {
            other = h.n != n;
            if (which[b] < N) bytes = (unsigned long long)h.head + wire.gk_n * n + 32;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bytes += __shfl_down(bytes, o, 64), other += __shfl_down(other, o, 64);
    if ((threadIdx.x & 63) == 0) sb[threadIdx.x >> 6] = bytes, sm[threadIdx.x >> 6] = other;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long tb = sb[0] + sb[1] + sb[2] + sb[3], tm = sm[0] + sm[1] + sm[2] + sm[3];
        if (tb) atomicAdd(&cnt[0], tb);
        if (tm) atomicAdd(&cnt[1], tm);
        if (blockIdx.x == 0) cnt[2] = off[B];
    }
}
void launch_rr_census(hipStream_t s, uint64_t B, const uint8_t* proofs, const uint64_t* off, const uint32_t* which, const Wire& wire, uint32_t n, uint32_t N,
                      unsigned long long* cnt) {
    hipMemsetAsync(cnt, 0, 8 * RR_CENSUS_WORDS, s);
    hipLaunchKernelGGL(k_rr_census, dim3((uint32_t)((B + 255) / 256)), dim3(256), 0, s, B, proofs, off, which, wire, n, N, cnt);
}

// ------------------------------------------------------------------ keyXcom's blinder
// One lane per proof: logical draw 1 (draw 0 is comS1's, mod n; draw 1 mod q) through the rejection lists the prepass made for fills 0 .. 1 + RNG_MAX_EXC.
// A stream that does not hold the draw's fill (or more rejected fills than the lists hold) gives 32 zero bytes and raises the call's flag.
__global__ void __launch_bounds__(256) k_rr_blinders(RngCtx g, uint32_t count, uint64_t first, uint8_t* __restrict__ out, uint32_t* exhausted) {
    const uint32_t p = gtid();
    if (p >= count) return;
    uint32_t w[8];
    const uint32_t fill = rng_map(g, p, 1);
    const bool bad = g.exc_cnt[p] > RNG_MAX_EXC || (g.mode == 1 && fill >= g.stride_blocks);
    rng_block(g, p, fill, w);
    if (bad) {
#pragma unroll
        for (int i = 0; i < 8; i++) w[i] = 0;
        atomicOr(exhausted, 1u);
    }
    store_be<8>(out + 32 * (first + p), w);
}
void launch_rr_blinders(hipStream_t s, const RngCtx& g, uint32_t count, uint64_t first, uint8_t* out, uint32_t* exhausted) {
    hipLaunchKernelGGL(k_rr_blinders, dim3((count + 255) / 256), dim3(256), 0, s, g, count, first, out, exhausted);
}

// ------------------------------------------------------------------ front end
// `tc` big-endian bytes at any alignment -> nine little-endian words
ZK_DEV void rr_load_coord(const uint8_t* p, uint32_t tc, uint32_t w[9]) {
#pragma unroll
    for (int i = 0; i < 9; i++) w[i] = 0;
    for (uint32_t i = 0; i < tc; i++) w[i >> 2] |= (uint32_t)p[tc - 1 - i] << (8 * (i & 3));
}
// One lane per proof, k_m_front's part for a proof that brings its commitment with it.  Statuses in the call's order: the header (ZK_E_BAD_ENCODING), the
// index (ZK_E_ARG); the opening and the RNG stream are judged by k_rr_compare, behind the commitments.  The 5 n draws start at fill 0, all mod q.
// Writes what k_m_front writes -- the status, the index the fold reads, the blinder, the opening (v, r) in list slot 4 n count + p -- and, read from the proof
// (its header is sound, so bytes [0, fixed) lie inside the slot): keyXcom's words for the comparison and, where the challenge hashes the full statement, R and
// keyXcom as k_gk_hash reads them.  No byte of a slot whose header is not sound is read beyond that header.
__global__ void __launch_bounds__(64) k_rr_front(Workspace W, RrLane X, uint32_t count, uint64_t first, const uint8_t* __restrict__ proofs, const uint64_t* __restrict__ off,
                                                 const uint32_t* __restrict__ which, const uint8_t* __restrict__ blinder, uint32_t* which_s) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint64_t b = first + p, o0 = off[b];
    const RrHead h = rr_head(proofs, o0, off[b + 1], W.wire);
    const uint32_t w = which[b];
    const bool inside = w < W.N;
    const int32_t st = !h.ok ? ZK_E_BAD_ENCODING : !inside ? ZK_E_ARG : ZK_OK;
    const uint32_t ndraw = 5 * W.n, cnt = W.rng.exc_cnt[p];
    uint32_t rej = 0;
    for (uint32_t i = 0; i < (cnt < RNG_MAX_EXC ? cnt : RNG_MAX_EXC); i++) rej += (W.rng.exc_flags[p * RNG_MAX_EXC + i] >> 1) & 1;
    X.flags[p] = cnt > RNG_MAX_EXC || (W.rng.mode == 1 && ndraw + rej > W.rng.stride_blocks);
    uint32_t bw[8];
    load_be32(blinder + 32 * b, bw);
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
        rr_load_coord(pr + ZK_HDR + 128, W.wire.tc, kw);
        rr_load_coord(pr + ZK_HDR + 128 + W.wire.tc, W.wire.tc, kw + 9);
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
void launch_rr_front(hipStream_t s, const Workspace& W, const RrLane& X, uint32_t count, uint64_t first, const uint8_t* proofs, const uint64_t* off, const uint32_t* which,
                     const uint8_t* blinder, uint32_t* which_s) {
    hipLaunchKernelGGL(k_rr_front, dim3((count + 63) / 64), dim3(64), 0, s, W, X, count, first, proofs, off, which, blinder, which_s);
}
// Behind the normaliser: ring[which] g + blinder h (list slot 4 n count + p, canonical) against the proof's keyXcom, word for word -- a coordinate the proof
// states non-canonically (not below the field prime, or with padding bytes set) equals no canonical one.  Then the RNG stream.  The proof's final status.
__global__ void __launch_bounds__(64) k_rr_compare(Workspace W, RrLane X, uint32_t count, uint64_t first, int32_t* __restrict__ status) {
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
    status[first + p] = st;
    X.len[p] = st == ZK_OK ? (uint64_t)X.head[p] + W.wire.gk_n * W.n + 32 : 0;
}
void launch_rr_compare(hipStream_t s, const Workspace& W, const RrLane& X, uint32_t count, uint64_t first, int32_t* status) {
    hipLaunchKernelGGL(k_rr_compare, dim3((count + 63) / 64), dim3(64), 0, s, W, X, count, first, status);
}

// ------------------------------------------------------------------ offsets
// One workgroup per chunk, k_part_offsets' scan with its base read on the device: the chunk's proofs start where the chunk before ended, out_off[first], which
// that chunk's scan wrote (the host orders the two with an event); the first chunk starts at 0.  W.out_base[p] = the start of proof p's new GKProof section.
__global__ void __launch_bounds__(1024) k_rr_scan(Workspace W, RrLane X, uint32_t count, uint64_t first, uint64_t* out_off) {
    __shared__ uint64_t sb[1024];
    const uint64_t t = threadIdx.x, per = ((uint64_t)count + 1023) / 1024;
    const uint64_t lo = t * per < count ? t * per : count, hi = lo + per < count ? lo + per : count;
    uint64_t sum = 0;
    for (uint64_t j = lo; j < hi; j++) sum += X.len[j];
    sb[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {   // inclusive Hillis-Steele scan of the partial sums
        const uint64_t v = t >= d ? sb[t - d] : 0;
        __syncthreads();
        sb[t] += v;
        __syncthreads();
    }
    const uint64_t base = first ? out_off[first] : 0;
    uint64_t run = base + sb[t] - sum;
    for (uint64_t j = lo; j < hi; j++) {
        if (j) out_off[first + j] = run;   // (out_off[first] is the chunk before's to write)
        W.out_base[j] = run + X.head[j];
        run += X.len[j];
    }
    if (first == 0 && t == 0) out_off[0] = 0;
    if (t == 1023) out_off[first + count] = base + sb[1023];
}
void launch_rr_scan(hipStream_t s, const Workspace& W, const RrLane& X, uint32_t count, uint64_t first, uint64_t* out_off) {
    hipLaunchKernelGGL(k_rr_scan, dim3(1), dim3(1024), 0, s, W, X, count, first, out_off);
}
// in place: the proofs stay where they are -- out_off = proof_off, a failed proof keeps its bytes
__global__ void __launch_bounds__(256) k_rr_place(Workspace W, RrLane X, uint32_t count, uint64_t first, uint64_t B, const uint64_t* off, uint64_t* out_off) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint64_t o = off[first + p];
    W.out_base[p] = o + X.head[p];
    if (out_off != off) {
        out_off[first + p] = o;
        if (first + p + 1 == B) out_off[B] = off[B];
    }
}
void launch_rr_place(hipStream_t s, const Workspace& W, const RrLane& X, uint32_t count, uint64_t first, uint64_t B, const uint64_t* off, uint64_t* out_off) {
    hipLaunchKernelGGL(k_rr_place, dim3((count + 255) / 256), dim3(256), 0, s, W, X, count, first, B, off, out_off);
}

// ------------------------------------------------------------------ the heads
// The chunk's heads, from the caller's proofs to their new places.  The work is divided by BYTES: a lane owns one 16-byte aligned unit of the chunk's output
// span per step (workgroups walk the span in runs of RR_SPAN units), finds the proof the unit lies in -- the proof of its last unit, else by bisection over
// the chunk's offsets --, and moves it with one 16-byte load (four dwords where
// source and destination differ mod 16) and one 16-byte store; consecutive lanes move consecutive units.  A unit that is not wholly inside one head -- the
// first 16 bytes of a proof with the two header words to patch (total_len, n), a unit across two proofs or into a GKProof section, which the membership
// prover's writers fill -- goes dword by dword.  Every offset and length is a multiple of 4.
#define RR_SPAN 4096u
ZK_DEV uint32_t rr_find(const uint64_t* __restrict__ oo, uint32_t count, uint64_t x) {   // the proof j of the chunk with oo[j] <= x < oo[j + 1]; oo[0] <= x < oo[count]
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (oo[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}
__global__ void __launch_bounds__(256) k_rr_move(RrLane X, uint32_t count, uint64_t first, const uint8_t* __restrict__ proofs, const uint64_t* __restrict__ off,
                                                 const uint64_t* __restrict__ out_off, uint32_t n_new, uint8_t* __restrict__ out) {
    const uint64_t* oo = out_off + first;
    const uint64_t lo = oo[0], hi = oo[count];
    if (hi == lo) return;
    const uintptr_t A = ((uintptr_t)out + lo) & ~(uintptr_t)15;
    const uint64_t units = ((uintptr_t)out + hi - A + 15) >> 4;
    // a workgroup takes RR_SPAN consecutive units at a time (64 KB), so a lane's next unit is 4 KB on and mostly in the proof of its last one
    uint32_t j = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * RR_SPAN; base < units; base += (uint64_t)gridDim.x * RR_SPAN) {
        for (uint32_t k = threadIdx.x; k < RR_SPAN && base + k < units; k += 256) {
            const int64_t d0 = (int64_t)(A + 16 * (base + k) - (uintptr_t)out);   // the unit's place in `out`; the span's first unit may start in front of it
            if (d0 >= (int64_t)lo && (uint64_t)d0 + 16 <= hi) {
                if (!(oo[j] <= (uint64_t)d0 && (uint64_t)d0 < oo[j + 1])) j = rr_find(oo, count, (uint64_t)d0);
                const uint64_t pos = (uint64_t)d0 - oo[j];
                if (pos >= 16 && pos + 16 <= X.head[j]) {
                    const uint8_t* src = proofs + off[first + j] + pos;
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
                const uint32_t jj = rr_find(oo, count, (uint64_t)x);
                const uint64_t pos = (uint64_t)x - oo[jj];
                if (pos >= X.head[jj]) continue;
                uint32_t v = *(const uint32_t*)(proofs + off[first + jj] + pos);
                if (pos == 4) v = bswap32((uint32_t)(oo[jj + 1] - oo[jj]));
                if (pos == 12) v = bswap32(n_new);
                *(uint32_t*)(out + x) = v;
            }
        }
    }
}
void launch_rr_move(hipStream_t s, const RrLane& X, uint32_t count, uint64_t first, const uint8_t* proofs, const uint64_t* off, const uint64_t* out_off, uint32_t n_new,
                    uint8_t* out) {
    const uint32_t blocks = std::min<uint32_t>(4096, std::max<uint32_t>(1, count) * 16);
    hipLaunchKernelGGL(k_rr_move, dim3(blocks), dim3(256), 0, s, X, count, first, proofs, off, out_off, n_new, out);
}
