// Ring membership of a committed value on its own (include/zkattest.h: zk_member_*; gk.ts:94-262): the kernels around the Groth-Kohlweiss machinery that a
// ZKAttest proof otherwise supplies -- the prover's front end (which value, which blinder, the commitment's opening), the ZKM1 header and the verifier's
// header / point validation.  The ring fold, the commitments, the challenge hash, the responses and the verifier's sums are the kernels of the full proof
// (k_scalar.hip, k_gk*.hip, k_tom.hip, k_hash.hip, k_verify.hip), run on a workspace whose layout fields say "no repetitions in front of the GKProof".
#include "member.h"

typedef Fe<ModQ, 1> Sq;
typedef Fe<ModT, 1> St;

// ------------------------------------------------------------------ prover
// One thread per proof.  Draw order of one proof (pedersen.ts:53-58 then gk.ts:117-123): fill 0 commit()'s randomScalar when the engine draws the blinder,
// then r_i, a_i, s_i, t_i, rho_i for i = 0 .. n-1 (W.gk_fill0 = 1); with a caller's blinder the 5 n draws start at fill 0 (W.gk_fill0 = 0).
// Writes: the status, the index the fold kernels read (0 for an index outside the padded ring: they address the ring's tables with it), the blinder, and
// the opening (v, r) of com in list slot 4 n count + p, behind the 4 n membership openings of every proof of the chunk.
__global__ void __launch_bounds__(64) k_m_front(Workspace W, uint32_t count, const uint32_t* __restrict__ which, const uint8_t* __restrict__ blinder, uint64_t first,
                                                uint32_t* which_s) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint32_t w = which[first + p];
    const bool inside = w < W.N;
    int32_t st = inside ? ZK_OK : ZK_E_ARG;
    // fills the proof consumes: its draws plus the rejected ones among them (every modulus is q: flag bit 1)
    const uint32_t ndraw = W.gk_fill0 + 5 * W.n, cnt = W.rng.exc_cnt[p];
    uint32_t rej = 0;
    for (uint32_t i = 0; i < (cnt < RNG_MAX_EXC ? cnt : RNG_MAX_EXC); i++) rej += (W.rng.exc_flags[p * RNG_MAX_EXC + i] >> 1) & 1;
    if (st == ZK_OK && (cnt > RNG_MAX_EXC || (W.rng.mode == 1 && ndraw + rej > W.rng.stride_blocks))) st = ZK_E_RNG_EXHAUSTED;
    Sq r;
    if (blinder) {   // newScalar reduces (group.ts:164-167)
        uint32_t bw[8];
        load_be32(blinder + 32 * (first + p), bw);
        r = fe_from_words256_reduce<ModQ>(bw);
    } else r = rng_draw<ModQ>(W.rng, p, 0);
    W.st[p] = st;
    W.zcnt[p] = 0;
    which_s[p] = inside ? w : 0;
    soa_st(W.gk_blind, p, r);
    soa_st(W.lc.v, 4 * W.n * count + p, soa_ld<ModQ, 1>(W.ring, inside ? w : 0));
    soa_st(W.lc.r, 4 * W.n * count + p, r);
}
void launch_m_front(hipStream_t s, const Workspace& W, uint32_t count, const uint32_t* which, const uint8_t* blinder, uint64_t first, uint32_t* which_s) {
    hipLaunchKernelGGL(k_m_front, dim3((count + 63) / 64), dim3(64), 0, s, W, count, which, blinder, first, which_s);
}
// Everything of a proof's slot that k_gk_respond / k_write_gk_points do not write: the 16 header bytes (W.wire.magic: "ZKM1", or "ZKMB" in a bound call; or zeros over the whole slot where the status is
// not 0), the commitment, the blinder, the status.  One workgroup per proof.  W.out_base[p] = p * size is written here too, before the GKProof's writers run.
// A window of a mixed-ring call (S.sel): entry first + p of the window is proof S.sel[first + p] of the batch -- its slot starts at that proof's place in the
// batch's offsets (out = the batch's buffer), com, blinder and status go to that index: every byte is written once, at its final place.  An entry that is
// not an index of the batch writes nothing, and its status keeps the GKProof's writers from writing too.
__global__ void __launch_bounds__(64) k_m_write_head(Workspace W, uint32_t count, uint64_t first, uint32_t size, uint8_t* out, uint8_t* com, uint8_t* blinder_out,
                                                     int32_t* status, MemberSel S) {
    const uint32_t p = blockIdx.x, t = threadIdx.x;
    const int32_t st = W.st[p];
    uint64_t idx = first + p, base = (uint64_t)p * size;
    if (S.sel) {
        idx = S.sel[first + p];
        if (idx >= S.B) {
            if (t == 0) W.st[p] = ZK_E_ARG, W.out_base[p] = 0;
            return;
        }
        base = S.off[idx];
    }
    uint32_t* slot = (uint32_t*)(out + base);
    if (st != ZK_OK) {
        for (uint32_t i = t; i < size / 4; i += 64) slot[i] = 0;
    } else if (t < 4) {
        slot[t] = t == 0 ? W.wire.magic : t == 1 ? bswap32(size) : t == 2 ? bswap32(W.n) : 0;
    }
    if (t == 0) {
        W.out_base[p] = base;
        status[idx] = st;
        const uint32_t e = 4 * W.n * count + p;
        store_tomcoord_be(com + 72 * idx, soa_ld<ModT, 1>(W.lc.ax, e));
        store_tomcoord_be(com + 72 * idx + 36, soa_ld<ModT, 1>(W.lc.ay, e));
        if (blinder_out) store_scalar_be(blinder_out + 32 * idx, soa_ld<ModQ, 1>(W.gk_blind, p));
    }
}
void launch_m_write_head(hipStream_t s, const Workspace& W, uint32_t count, uint64_t first, uint32_t size, uint8_t* out, uint8_t* com, uint8_t* blinder_out, int32_t* status,
                         const MemberSel& S) {
    hipLaunchKernelGGL(k_m_write_head, dim3(count), dim3(64), 0, s, W, count, first, size, out, com, blinder_out, status, S);
}

// ------------------------------------------------------------------ verifier
ZK_DEV bool m_tom_bytes_valid(const uint8_t* p) {  // edwards.ts:204-209 afterJson: range + curve equation, as k_v_validate checks a ZKA1 proof's points
    uint32_t xw[9], yw[9];
    const uint32_t* q = (const uint32_t*)p;
#pragma unroll
    for (int i = 0; i < 9; i++) xw[i] = bswap32(q[8 - i]), yw[i] = bswap32(q[17 - i]);
    return tom_words_on_curve(xw, yw);
}
// The ZKM1 header (one thread per proof): proofs are `size` bytes apart.  Fills the fields the GK kernels of k_verify.hip read: st, okflags (bit 3: the header's n
// is not the ring's -- verifyMembership returns false, gk.ts:208-218 --, the header's n above it), zcnt = 0.  total_len must be the length n announces.
// The magic is exactly the call's: "ZKMB" in a bound call (V.gk_stmt), "ZKM1" in an unbound one.
// (slot != 0: a window of a mixed-ring call -- off holds the gathered starts of slots that the classing kernel found `slot` bytes long)
__global__ void __launch_bounds__(256) k_mv_header(VWork V, uint32_t count, const uint8_t* proofs, const uint64_t* off, uint64_t first, uint32_t slot) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint64_t o0 = off[first + p], o1 = slot ? o0 + slot : off[first + p + 1];
    const uint32_t* h = (const uint32_t*)(proofs + o0);
    const uint32_t total = bswap32(h[1]), n = bswap32(h[2]);
    int32_t st = ZK_OK;
    uint32_t flags = 0;
    if (h[0] != (V.gk_stmt == GK_STMT_MEMBER ? ZK_MAGIC_ZKMB : ZK_MAGIC_ZKM1) || h[3] != 0 || n > 63 || total != zkm1_size(n)) st = ZK_E_BAD_ENCODING;
    else if (n != V.n) flags = 8 | (n << 16);   // (its total_len is the one ITS n announces; the slot is the ring's size)
    else if (total != o1 - o0) st = ZK_E_BAD_ENCODING;
    V.st[p] = st, V.okflags[p] = flags, V.zcnt[p] = 0;
}
// One thread per point that exists: com, then the 4 n commitments of the announced structure (a proof whose n is not the ring's has its 4 n' points walked by
// the thread of com, as k_v_validate does; the call's slots have the active ring's size, so of a longer proof only what lies inside its slot).
__global__ void __launch_bounds__(256) k_mv_validate(VWork V, uint32_t count, const uint8_t* proofs, const uint64_t* off, uint64_t first, uint32_t slot) {
    const uint32_t per = 1 + 4 * V.n, t = gtid();
    if (t >= count * per) return;
    const uint32_t p = t / per, u = t % per;
    if (V.st[p] != ZK_OK) return;
    const uint8_t* gk = proofs + off[first + p] + ZKM1_HDR;
    const bool other = V.okflags[p] & 8;
    bool ok = true;
    if (u == 0) {
        ok = m_tom_bytes_valid(V.com + 72 * (first + p));
        if (other) {   // no byte outside the proof's slot is read: of a longer structure, the points that lie inside it
            const uint64_t room = ((slot ? slot : off[first + p + 1] - off[first + p]) - ZKM1_HDR) / 72;
            const uint32_t np = 4 * (V.okflags[p] >> 16);
            for (uint32_t k = 0; k < (np < room ? np : (uint32_t)room); k++) ok = ok && m_tom_bytes_valid(gk + 72 * k);
        }
    } else if (!other) ok = m_tom_bytes_valid(gk + 72 * (u - 1));
    if (!ok) atomicCAS(&V.st[p], ZK_OK, ZK_E_BAD_ENCODING);
}
void launch_mv_header_validate(hipStream_t s, const VWork& V, uint32_t count, const uint8_t* proofs, const uint64_t* off, uint64_t first, uint32_t slot) {
    hipLaunchKernelGGL(k_mv_header, dim3((count + 255) / 256), dim3(256), 0, s, V, count, proofs, off, first, slot);
    const uint32_t n = count * (1 + 4 * V.n);
    hipLaunchKernelGGL(k_mv_validate, dim3((n + 255) / 256), dim3(256), 0, s, V, count, proofs, off, first, slot);
}
// offsets of a batch of equally long proofs (the GK kernels take an offset array)
__global__ void __launch_bounds__(256) k_mv_offsets(uint64_t* off, uint64_t B, uint64_t size) {
    const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (i <= B) off[i] = i * size;
}
void launch_mv_offsets(hipStream_t s, uint64_t* off, uint64_t B, uint64_t size) {
    hipLaunchKernelGGL(k_mv_offsets, dim3((uint32_t)((B + 256) / 256)), dim3(256), 0, s, off, B, size);
}
// The verdict (gk.ts:261): the sum of the membership relations -- the fixed-base part (list slot p * 4 n), the groups of the proof's own points, com -- is the
// identity.  k_v_final_memb of a ZKAttest proof below 20 repetitions computes the same sum and reports ZK_E_SECLEVEL; here it IS the answer.
ZK_DEV TomPt m_ld_tom4(const Soa4& a, uint32_t e) {
    TomPt r;
    r.x = soa_ld<ModT, 2>(a.x, e), r.y = soa_ld<ModT, 2>(a.y, e), r.z = soa_ld<ModT, 2>(a.z, e), r.t = soa_ld<ModT, 2>(a.t, e);
    return r;
}
// (S.sel: a window of a mixed-ring call -- the verdict of entry first + p goes to index S.sel[first + p] of the batch, k_lv_scatter's pattern; an entry that is
// no index of the batch writes nothing)
__global__ void __launch_bounds__(64, 2) k_mv_final(Workspace W, VWork V, uint32_t count, uint8_t* ok_out, int32_t* status_out, uint64_t first, MemberSel S) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint64_t idx = S.sel ? S.sel[first + p] : first + p;
    if (S.sel && idx >= S.B) return;
    const int32_t st = V.st[p];
    uint8_t ok = 0;
    if (st == ZK_OK && !(V.okflags[p] & 8)) {
        const uint32_t n = V.n, nq = (n + 1) / 2, e = p * 4 * n;
        TomPt m;   // (X : Y : Z) without T -> (XZ : YZ : XY : Z^2)
        {
            const auto x = soa_ld<ModT, 2>(W.lc.proj.x, e), y = soa_ld<ModT, 2>(W.lc.proj.y, e), z = soa_ld<ModT, 2>(W.lc.proj.z, e);
            m.x = x * z, m.y = y * z, m.t = x * y, m.z = z * z;
        }
        for (uint32_t q = 0; q < nq; q++) m = tom_add(m, m_ld_tom4(V.gk_acc, p * nq + q));
        m = tom_add(m, m_ld_tom4(V.misc_acc, p));
        ok = fe_is_zero(m.x) && fe_eq(m.y, m.z) && !fe_is_zero(m.z);   // edwards.ts:117-125 on the a = 1 image
    }
    ok_out[idx] = ok;
    status_out[idx] = st;
}
void launch_mv_final(hipStream_t s, const Workspace& W, const VWork& V, uint32_t count, uint8_t* ok, int32_t* status, uint64_t first, const MemberSel& S) {
    hipLaunchKernelGGL(k_mv_final, dim3((count + 63) / 64), dim3(64), 0, s, W, V, count, ok, status, first, S);
}
