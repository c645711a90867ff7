// P-256 sums and walks of ONE scalar multiplication on cooperating waves (coop.h): the comb and key-table sums of a call of a few proofs (k_p256.hip:
// k_front_co, k_exp_commit_kt_co) and of a few screened witnesses (k_screen.hip: k_screen_table_co, k_screen_walk_co), and the 65-window walk of a point
// without a table (k_screen_walk_co).  The sums and the walk depend on the arithmetic headers only, so tests/host_arith/host_screen_co.cpp compiles them for
// the host against coop.h's SIMT emulation; the loaders they take their entries through are coop_dev.h's on the device and the few lines below on the host.
#pragma once
#ifdef ZK_HOST_BUILD
#include "rtab.h"   // ktab.h, the comb walks, front_recode
#include "coop.h"
// ---- host emulation of coop_dev.h's loaders (same rows, same residues)
inline CoFe<ModQ, 8> co_load_pfix(const uint32_t* e) {
    const uint32_t zero[NLIMB] = {0};
    return co_load4<ModQ, 8>(e, e + NLIMB, ModQ::one, zero);
}
inline CoFe<ModQ, 8> co_load_ktab(const uint32_t* e, bool neg) {
    const uint32_t zero[NLIMB] = {0};
    uint32_t x[NLIMB], y[NLIMB];
    limbs_from_words<8>(x, e);
    limbs_from_words<8>(y, e + 8);
    CoFe<ModQ, 8> r = co_load4<ModQ, 8>(x, y, ModQ::one, zero);
    if (neg) r.v = co_sel(co_row_is(1), co_carry(co_sub_const<ModQ, 4>() - r.v), r.v);
    return r;
}
inline CoP256 co_p256_identity() {
    CoP256 r;
    r.v.v = co_sel(co_row_is(1), co_limbs(ModQ::one), co_splat(0));
    return r;
}
// lane i <-> p[i]: a wave's register parked in 64 words (LDS on the device)
inline CoU32 co_ld_wave(const uint32_t* p) {
    CoU32 r;
    for (int i = 0; i < 64; i++) r.v[i] = p[i];
    return r;
}
inline void co_st_wave(uint32_t* p, const CoU32& v) {
    for (int i = 0; i < 64; i++) p[i] = v.v[i];
}
#else
#include "rtab.h"
#include "coop_dev.h"
ZK_DEV CoU32 co_ld_wave(const uint32_t* p) { return p[__lane_id()]; }
ZK_DEV void co_st_wave(uint32_t* p, const CoU32& v) { p[__lane_id()] = v; }
#endif

// ---------------------------------------------------------------- a call of a few proofs: the table sums on cooperating waves (coop.h)
// One sum = one workgroup of four waves: wave q adds the entries of a quarter of the comb's windows (and of the key table's) at 1.2 us an addition instead of
// one lane's 5.4-8, the four partial sums meet in LDS.  Same group elements as the one-lane kernels, hence the same affine coordinates and the same bytes
// (tests/test_gpu_prove.py: one-lane against cooperative chains, byte for byte).  ZK_UNIFORM_CF: a zero digit's addition is computed and discarded here too.
ZK_DEV CoP256 co_add_if(bool cond, const CoP256& acc, const CoFe<ModQ, 8>& ent, const CoU32& mj) {
    CoP256 e;
    e.v = ent;
#if ZK_UNIFORM_CF
    const CoP256 s = co_p256_add(acc, e, mj);
    CoP256 r;
    r.v = co_pick((uint32_t)cond, s.v, acc.v);
    return r;
#else
    return cond ? co_p256_add(acc, e, mj) : acc;
#endif
}
// acc + (windows [w0, w0 + per) of k) * B through B's comb (rtab.h: p256_fixed_mul_range)
ZK_DEV CoP256 co_fixed_mul_range(CoP256 acc, const uint32_t* __restrict__ tab, uint32_t kw[8], uint32_t w0, uint32_t per, const CoU32& mj) {
#pragma unroll 1
    for (uint32_t w = 0; w < w0; w++) shr256<PFIX_WIN_BITS>(kw);
#pragma unroll 1
    for (uint32_t w = w0; w < w0 + per && w < PFIX_NWIN; w++) {
        const uint32_t d = kw[0] & (PFIX_WIN_SIZE - 1);
        shr256<PFIX_WIN_BITS>(kw);
        acc = co_add_if(d != 0, acc, co_load_pfix(tab + (size_t)PFIX_ENTRY_WORDS * (w * PFIX_WIN_SIZE + (d ? d : 1))), mj);
    }
    return acc;
}
// ... and through a ring key's table (ktab.h: p256_ktab_mul_range)
ZK_DEV CoP256 co_ktab_mul_range(CoP256 acc, const uint32_t* __restrict__ kt, const uint32_t kw[8], bool neg, uint32_t w0, uint32_t per, const CoU32& mj) {
    KeyDigits kd;
    kd.init();
#pragma unroll
    for (int i = 0; i < 8; i++) kd.w[i] = kw[i];
    uint32_t d;
    bool dn;
#pragma unroll 1
    for (uint32_t w = 0; w < w0; w++) kd.next(d, dn);
#pragma unroll 1
    for (uint32_t w = w0; w < w0 + per && w < KTAB_NWIN; w++) {
        kd.next(d, dn);
        acc = co_add_if(d != 0, acc, co_load_ktab(kt + ((size_t)w * KTAB_ENT + (d ? d - 1 : 0)) * KTAB_ENTRY_WORDS, neg != dn), mj);
    }
    return acc;
}
#ifndef ZK_HOST_BUILD
// the sum of the four waves' points: waves 1..3 park theirs in LDS, wave 0 returns the total (the others return their own)
ZK_DEV CoP256 co_wg4_sum(CoP256 acc, uint32_t (*part)[64], uint32_t q, const CoU32& mj) {
    const uint32_t lane = threadIdx.x & 63u;
    __syncthreads();   // (the buffer may still be read from the sum before)
    if (q) part[q - 1][lane] = acc.v.v;
    __syncthreads();
    if (q) return acc;
#pragma unroll 1
    for (uint32_t k = 0; k < 3; k++) {
        CoP256 o;
        o.v.v = part[k][lane];
        acc = co_p256_add(acc, o, mj);
    }
    return acc;
}
#endif

// ---------------------------------------------------------------- k * P for a point without a table of its own, one wave (rtab.h: front_pk_multiples, front_walk)
// The multiples 1..8 of P as eight parked wave registers (CO_WALK_MULT_WORDS words: LDS on the device, never the global scratch area): one doubling and six
// additions.  Every multiple is parked after a product with one, i.e. below 2 q, so that the walk can negate its Y (4 q - Y) within a point register's bound.
#define CO_WALK_MULT_WORDS (8 * 64)
ZK_DEV void co_front_pk_multiples(uint32_t* mult, const CoP256& base, const CoU32& mj) {
    const auto one = co_const<ModQ>(ModQ::one);
    co_st_wave(mult, co_mul(base.v, one, mj).v);
    CoP256 m = co_p256_dbl(base, mj);
    co_st_wave(mult + 64, co_mul(m.v, one, mj).v);
#pragma unroll 1
    for (uint32_t d = 2; d < 8; d++) {
        m = co_p256_add(m, base, mj);
        co_st_wave(mult + 64 * d, co_mul(m.v, one, mj).v);
    }
}
// The 65 signed 4-bit digits of front_recode top down: four doublings and one addition of +- |d| P per digit, the sum SELECTED, never branched on, when
// the digit is zero (front_walk's rule, whatever ZK_UNIFORM_CF is).  260 doublings and 65 additions in a row.
ZK_DEV CoP256 co_front_walk(const uint32_t* mult /* co_front_pk_multiples */, const uint8_t* dig /*[FRONT_NW]*/, const CoU32& mj) {
    CoP256 acc = co_p256_identity();
    CoFe<ModQ, 0> zero;
    zero.v = co_splat(0);
#pragma unroll 1
    for (int w = FRONT_NW - 1; w >= 0; w--) {
#pragma unroll 1
        for (int i = 0; i < 4; i++) acc = co_p256_dbl(acc, mj);
        const uint32_t db = dig[w], d = db & 15;
        CoFe<ModQ, 2> e;
        e.v = co_ld_wave(mult + 64 * (d ? d - 1 : 0));
        CoP256 ep;
        ep.v = co_pick(co_splat((db & 0x80u) ? 1u : 0u) & co_row_is(1), co_sub(zero, e), e).template as<8>();
        const CoP256 s = co_p256_add(acc, ep, mj);
        acc.v = co_pick(co_splat(d != 0 ? 1u : 0u), s.v, acc.v);
    }
    return acc;
}
