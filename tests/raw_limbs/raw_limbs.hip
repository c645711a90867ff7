// Raw-limb driver for csrc/field.h (one element per lane) and csrc/coop.h (one element per 16-lane row): operands are built DIRECTLY from the limbs of
// the input file -- no fe_to_mont, no conversion of any kind -- so a test can hand the templates the worst case their types admit (tests/test_raw_limbs.py).
// One source, two compilers:
//   g++ -x c++ -std=c++17 -DZK_HOST_BUILD -I zkp-ecdsa_amd/csrc raw_limbs.hip      host executable (coop.h runs through its SIMT emulation)
//   hipcc --offload-arch=gfx950 -std=c++17 -I zkp-ecdsa_amd/csrc raw_limbs.hip     device executable: one thread per one-lane record, one wave per four
//                                                                                 cooperative records (the real DPP / ds_bpermute instructions)
// usage: raw_limbs IN OUT.   Both executables must write the same bytes for the same input.
//
// Vector format (every field a little-endian uint32):
//   header    'RAWL' (0x4c574152), n_one, n_coop, 0
//   n_one  one-lane records of 31 words:      modulus, 0, op, class, a[9], b[9], c[9]
//   n_coop cooperative records of 36 words:   modulus, 1, op, class, a[16], b[16]      (lane j of the row; a run's length is a multiple of 4: one wave)
//   modulus: 0 = ModQ, 1 = ModN, 2 = ModT.  Records with the same (modulus, op, class) that follow each other form a run; a run is one loop / one launch.
// Output: n_one records of 36 words (up to four results of 9 limbs; a boolean is word 0; unused words zero), then n_coop records of 16 words (every lane of the row).
//
// Classes (the K of Fe<M, K> / CoFe<M, K>; `corner` = kmax / KCAP, the largest partner of a KCAP operand):
//   product  P0..P6 (Ka, Kb) = (1,1) (2,2) (4,2) (16,16) (64,64) (128,128: ModQ, ModN only) (KCAP, corner);  c has the magnitude of b
//   sum      the product classes with Ka + Kb <= KCAP, and class 7 = (256, 256)
//   sub      S0..S5 Kb = 1, 3, 4, 7, 127, 255 with Ka = KCAP - C(Kb), the largest the static_assert admits
//   sub2     T0..T3 (Kb, Kc) = (1,1) (2,1) (3,4) (127,128) with Ka = KCAP - C(Kb + Kc)
//   unary    U0..U7 K = 1, 2, 4, 16, 64, 128, 256, 512
// One-lane ops: 0 a * b   1 fe_sqr(x), x = a if Ka^2 <= kmax else b   2/3 fe_mul2<false/true> (a b, a c)   4/5 fe_mul3 (+ c b)   6/7 fe_mul4 (+ b a)
//   8 a * b on Fe<M, 2> (class P1)   9 limbs_mont_mul_rows on the raw limbs   10 a + b (sum)   11 a - b (sub)   12 fe_sub2(a, b, c) (sub2)   13 fe_neg(b) (sub)
//   14 fe_dbl (unary, K <= 256)   15 fe_reduce (unary)   16 fe_canon (U0..U2)   17 fe_is_zero (unary)   18 fe_eq(a, b) (sub)
//   19/20 fe_inv_gcd<M, false/true> (U1)   21 fe_inv_fermat (U1)
// Cooperative ops: 0 co_mul (product)   1 co_add (sum)   2 co_sub (sub)   3 co_addsub, a - b in rows 1, 2 (sub)   4 co_addsub, a - b in rows 0, 3 (sub)
//   5 co_carry on the raw register a   6 co_normalize (unary)   7 co_double (unary, K <= 256)   8 co_triple (U0, U1, U5 with K = 170)
//   9 co_pick(rows 0 and 2: a, else b) (product)   10 co_rows<2, 4, 0, 1> (U1)
#include "coop.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define RL_MAGIC 0x4c574152u
#define RL_ONE_IN 31
#define RL_ONE_OUT 36
#define RL_CO_IN 36
#define RL_CO_OUT 16

template <class M, int K>
ZK_DEV Fe<M, K> rl_ld(const uint32_t* p) {
    Fe<M, K> r;
#pragma unroll
    for (int i = 0; i < NLIMB; i++) r.l[i] = p[i];
    return r;
}
template <class M, int K>
ZK_DEV void rl_st(uint32_t* o, const Fe<M, K>& a) {
#pragma unroll
    for (int i = 0; i < NLIMB; i++) o[i] = a.l[i];
}

template <class M, int OP, int Ka, int Kb, int Kc>
ZK_DEV void rl_one(const uint32_t* in, uint32_t* out) {
    const uint32_t *pa = in + 4, *pb = in + 4 + NLIMB, *pc = in + 4 + 2 * NLIMB;
    constexpr bool BATCH = (OP & 1) != 0;
    if constexpr (OP == 0) rl_st(out, rl_ld<M, Ka>(pa) * rl_ld<M, Kb>(pb));
    else if constexpr (OP == 1) {
        if constexpr ((long)Ka * Ka <= M::kmax) rl_st(out, fe_sqr(rl_ld<M, Ka>(pa)));
        else rl_st(out, fe_sqr(rl_ld<M, Kb>(pb)));
    } else if constexpr (OP == 2 || OP == 3) {
        Fe<M, 2> r0, r1;
        fe_mul2<BATCH>(r0, r1, rl_ld<M, Ka>(pa), rl_ld<M, Kb>(pb), rl_ld<M, Ka>(pa), rl_ld<M, Kc>(pc));
        rl_st(out, r0), rl_st(out + NLIMB, r1);
    } else if constexpr (OP == 4 || OP == 5) {
        Fe<M, 2> r0, r1, r2;
        fe_mul3<BATCH>(r0, r1, r2, rl_ld<M, Ka>(pa), rl_ld<M, Kb>(pb), rl_ld<M, Ka>(pa), rl_ld<M, Kc>(pc), rl_ld<M, Kc>(pc), rl_ld<M, Kb>(pb));
        rl_st(out, r0), rl_st(out + NLIMB, r1), rl_st(out + 2 * NLIMB, r2);
    } else if constexpr (OP == 6 || OP == 7) {
        Fe<M, 2> r0, r1, r2, r3;
        fe_mul4<BATCH>(r0, r1, r2, r3, rl_ld<M, Ka>(pa), rl_ld<M, Kb>(pb), rl_ld<M, Ka>(pa), rl_ld<M, Kc>(pc), rl_ld<M, Kc>(pc), rl_ld<M, Kb>(pb), rl_ld<M, Kb>(pb),
                       rl_ld<M, Ka>(pa));
        rl_st(out, r0), rl_st(out + NLIMB, r1), rl_st(out + 2 * NLIMB, r2), rl_st(out + 3 * NLIMB, r3);
    } else if constexpr (OP == 8) rl_st(out, rl_ld<M, 2>(pa) * rl_ld<M, 2>(pb));
    else if constexpr (OP == 9) {
        static_assert((long)Ka * Kb <= M::kmax, "Montgomery input magnitudes too large");
        Fe<M, 2> r;
        limbs_mont_mul_rows<M>(r.l, rl_ld<M, Ka>(pa).l, rl_ld<M, Kb>(pb).l);
        rl_st(out, r);
    } else if constexpr (OP == 10) rl_st(out, rl_ld<M, Ka>(pa) + rl_ld<M, Kb>(pb));
    else if constexpr (OP == 11) rl_st(out, rl_ld<M, Ka>(pa) - rl_ld<M, Kb>(pb));
    else if constexpr (OP == 12) rl_st(out, fe_sub2(rl_ld<M, Ka>(pa), rl_ld<M, Kb>(pb), rl_ld<M, Kc>(pc)));
    else if constexpr (OP == 13) rl_st(out, fe_neg(rl_ld<M, Kb>(pb)));
    else if constexpr (OP == 14) rl_st(out, fe_dbl(rl_ld<M, Ka>(pa)));
    else if constexpr (OP == 15) rl_st(out, fe_reduce(rl_ld<M, Ka>(pa)));
    else if constexpr (OP == 16) rl_st(out, fe_canon(rl_ld<M, Ka>(pa)));
    else if constexpr (OP == 17) out[0] = fe_is_zero(rl_ld<M, Ka>(pa)) ? 1u : 0u;
    else if constexpr (OP == 18) out[0] = fe_eq(rl_ld<M, Ka>(pa), rl_ld<M, Kb>(pb)) ? 1u : 0u;
    else if constexpr (OP == 19) rl_st(out, fe_inv_gcd<M, false>(rl_ld<M, 2>(pa)));
    else if constexpr (OP == 20) rl_st(out, fe_inv_gcd<M, true>(rl_ld<M, 2>(pa)));
    else rl_st(out, fe_inv_fermat<M>(rl_ld<M, 2>(pa)));
}

template <class M, int OP, int Ka, int Kb>
ZK_DEV CoU32 rl_co(const CoU32& av, const CoU32& bv) {
    CoFe<M, Ka> a;
    CoFe<M, Kb> b;
    a.v = av, b.v = bv;
    const CoU32 row = co_row_index();
    (void)row;
    if constexpr (OP == 0) return co_mul(a, b, co_limbs(M::mod)).v;
    else if constexpr (OP == 1) return co_add(a, b).v;
    else if constexpr (OP == 2) return co_sub(a, b).v;
    else if constexpr (OP == 3) return co_addsub(a, b, co_eq(row, 1) | co_eq(row, 2)).v;
    else if constexpr (OP == 4) return co_addsub(a, b, co_eq(row, 0) | co_eq(row, 3)).v;
    else if constexpr (OP == 5) return co_carry(av);
    else if constexpr (OP == 6) return co_normalize(a).v;
    else if constexpr (OP == 7) return co_double(a).v;
    else if constexpr (OP == 8) return co_triple(a).v;
    else if constexpr (OP == 9) return co_pick(co_eq(row, 0) | co_eq(row, 2), a, b).v;
    else return co_rows<2, 4, 0, 1>(a).v;
}

#ifndef ZK_HOST_BUILD
template <class M, int OP, int Ka, int Kb, int Kc>
__global__ void __launch_bounds__(64) k_rl_one(const uint32_t* in, uint32_t* out, uint32_t first, uint32_t n) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) rl_one<M, OP, Ka, Kb, Kc>(in + (size_t)(first + i) * RL_ONE_IN, out + (size_t)(first + i) * RL_ONE_OUT);
}
// one wave per block: rows 0..3 are records first + 4 * block + (0..3)
template <class M, int OP, int Ka, int Kb>
__global__ void __launch_bounds__(64) k_rl_co(const uint32_t* in, uint32_t* out, uint32_t first) {
    const uint32_t lane = threadIdx.x, rec = first + 4 * blockIdx.x + (lane >> 4), j = lane & 15u;
    const uint32_t* p = in + (size_t)rec * RL_CO_IN + 4;
    out[(size_t)rec * RL_CO_OUT + j] = rl_co<M, OP, Ka, Kb>(p[j], p[16 + j]);
}
#endif

struct RlCtx {
    const uint32_t *one_in, *co_in;   // host: the file; device: device copies
    uint32_t *one_out, *co_out;
};
template <class M, int OP, int Ka, int Kb, int Kc>
static void rl_run_one(const RlCtx& c, uint32_t first, uint32_t n) {
#ifdef ZK_HOST_BUILD
    for (uint32_t i = first; i < first + n; i++) rl_one<M, OP, Ka, Kb, Kc>(c.one_in + (size_t)i * RL_ONE_IN, c.one_out + (size_t)i * RL_ONE_OUT);
#else
    hipLaunchKernelGGL((k_rl_one<M, OP, Ka, Kb, Kc>), dim3((n + 63) / 64), dim3(64), 0, 0, c.one_in, c.one_out, first, n);
#endif
}
template <class M, int OP, int Ka, int Kb>
static void rl_run_co(const RlCtx& c, uint32_t first, uint32_t n) {   // n % 4 == 0 (checked by the caller)
#ifdef ZK_HOST_BUILD
    for (uint32_t w = first; w < first + n; w += 4) {
        CoU32 a, b;
        for (int i = 0; i < 64; i++) {
            const uint32_t* p = c.co_in + (size_t)(w + (i >> 4)) * RL_CO_IN + 4;
            a.v[i] = p[i & 15], b.v[i] = p[16 + (i & 15)];
        }
        const CoU32 r = rl_co<M, OP, Ka, Kb>(a, b);
        for (int i = 0; i < 64; i++) c.co_out[(size_t)(w + (i >> 4)) * RL_CO_OUT + (i & 15)] = r.v[i];
    }
#else
    hipLaunchKernelGGL((k_rl_co<M, OP, Ka, Kb>), dim3(n / 4), dim3(64), 0, 0, c.co_in, c.co_out, first);
#endif
}

// ---- classes -> template arguments.  Every function returns false for a (modulus, op, class) that is not a case.
template <class M>
constexpr int rl_corner() { return M::kmax / KCAP; }
template <class M, int OP, bool COOP, int Ka, int Kb, int Kc = Kb>
static void rl_go(const RlCtx& c, uint32_t first, uint32_t n) {
    if constexpr (COOP) rl_run_co<M, OP, Ka, Kb>(c, first, n);
    else rl_run_one<M, OP, Ka, Kb, Kc>(c, first, n);
}
template <class M, int OP, bool COOP, bool SUM>
static bool rl_product(const RlCtx& c, uint32_t cls, uint32_t first, uint32_t n) {
    switch (cls) {
    case 0: rl_go<M, OP, COOP, 1, 1>(c, first, n); return true;
    case 1: rl_go<M, OP, COOP, 2, 2>(c, first, n); return true;
    case 2: rl_go<M, OP, COOP, 4, 2>(c, first, n); return true;
    case 3: rl_go<M, OP, COOP, 16, 16>(c, first, n); return true;
    case 4: rl_go<M, OP, COOP, 64, 64>(c, first, n); return true;
    case 5:
        if constexpr (SUM || 128L * 128 <= M::kmax) {
            rl_go<M, OP, COOP, 128, 128>(c, first, n);
            return true;
        } else return false;
    case 6:
        if constexpr (!SUM) {
            rl_go<M, OP, COOP, KCAP, rl_corner<M>()>(c, first, n);
            return true;
        } else return false;
    case 7:
        if constexpr (SUM) {
            rl_go<M, OP, COOP, 256, 256>(c, first, n);
            return true;
        } else return false;
    }
    return false;
}
template <class M, int OP, bool COOP>
static bool rl_sub(const RlCtx& c, uint32_t cls, uint32_t first, uint32_t n) {
    switch (cls) {
    case 0: rl_go<M, OP, COOP, KCAP - 4, 1>(c, first, n); return true;
    case 1: rl_go<M, OP, COOP, KCAP - 4, 3>(c, first, n); return true;
    case 2: rl_go<M, OP, COOP, KCAP - 8, 4>(c, first, n); return true;
    case 3: rl_go<M, OP, COOP, KCAP - 8, 7>(c, first, n); return true;
    case 4: rl_go<M, OP, COOP, KCAP - 128, 127>(c, first, n); return true;
    case 5: rl_go<M, OP, COOP, KCAP - 256, 255>(c, first, n); return true;
    }
    return false;
}
template <class M>
static bool rl_sub2(const RlCtx& c, uint32_t cls, uint32_t first, uint32_t n) {
    switch (cls) {
    case 0: rl_run_one<M, 12, KCAP - 4, 1, 1>(c, first, n); return true;
    case 1: rl_run_one<M, 12, KCAP - 4, 2, 1>(c, first, n); return true;
    case 2: rl_run_one<M, 12, KCAP - 8, 3, 4>(c, first, n); return true;
    case 3: rl_run_one<M, 12, KCAP - 256, 127, 128>(c, first, n); return true;
    }
    return false;
}
template <class M, int OP, bool COOP, int KMAX>
static bool rl_unary(const RlCtx& c, uint32_t cls, uint32_t first, uint32_t n) {
    switch (cls) {
    case 0: rl_go<M, OP, COOP, 1, 1>(c, first, n); return true;
    case 1: rl_go<M, OP, COOP, 2, 1>(c, first, n); return true;
    case 2: rl_go<M, OP, COOP, 4, 1>(c, first, n); return true;
    case 3: if constexpr (KMAX >= 16) { rl_go<M, OP, COOP, 16, 1>(c, first, n); return true; } else return false;
    case 4: if constexpr (KMAX >= 64) { rl_go<M, OP, COOP, 64, 1>(c, first, n); return true; } else return false;
    case 5: if constexpr (KMAX >= 128) { rl_go<M, OP, COOP, 128, 1>(c, first, n); return true; } else return false;
    case 6: if constexpr (KMAX >= 256) { rl_go<M, OP, COOP, 256, 1>(c, first, n); return true; } else return false;
    case 7: if constexpr (KMAX >= 512) { rl_go<M, OP, COOP, 512, 1>(c, first, n); return true; } else return false;
    }
    return false;
}
template <class M>
static bool rl_dispatch_one(const RlCtx& c, uint32_t op, uint32_t cls, uint32_t first, uint32_t n) {
    switch (op) {
    case 0: return rl_product<M, 0, false, false>(c, cls, first, n);
    case 1: return rl_product<M, 1, false, false>(c, cls, first, n);
    case 2: return rl_product<M, 2, false, false>(c, cls, first, n);
    case 3: return rl_product<M, 3, false, false>(c, cls, first, n);
    case 4: return rl_product<M, 4, false, false>(c, cls, first, n);
    case 5: return rl_product<M, 5, false, false>(c, cls, first, n);
    case 6: return rl_product<M, 6, false, false>(c, cls, first, n);
    case 7: return rl_product<M, 7, false, false>(c, cls, first, n);
    case 8:
        if (cls != 1) return false;
        rl_run_one<M, 8, 2, 2, 2>(c, first, n);
        return true;
    case 9: return rl_product<M, 9, false, false>(c, cls, first, n);
    case 10: return rl_product<M, 10, false, true>(c, cls, first, n);
    case 11: return rl_sub<M, 11, false>(c, cls, first, n);
    case 12: return rl_sub2<M>(c, cls, first, n);
    case 13: return rl_sub<M, 13, false>(c, cls, first, n);
    case 14: return rl_unary<M, 14, false, 256>(c, cls, first, n);
    case 15: return rl_unary<M, 15, false, 512>(c, cls, first, n);
    case 16: return rl_unary<M, 16, false, 4>(c, cls, first, n);
    case 17: return rl_unary<M, 17, false, 512>(c, cls, first, n);
    case 18: return rl_sub<M, 18, false>(c, cls, first, n);
    case 19: if (cls != 1) return false; rl_run_one<M, 19, 2, 2, 2>(c, first, n); return true;
    case 20: if (cls != 1) return false; rl_run_one<M, 20, 2, 2, 2>(c, first, n); return true;
    case 21: if (cls != 1) return false; rl_run_one<M, 21, 2, 2, 2>(c, first, n); return true;
    }
    return false;
}
template <class M>
static bool rl_dispatch_co(const RlCtx& c, uint32_t op, uint32_t cls, uint32_t first, uint32_t n) {
    switch (op) {
    case 0: return rl_product<M, 0, true, false>(c, cls, first, n);
    case 1: return rl_product<M, 1, true, true>(c, cls, first, n);
    case 2: return rl_sub<M, 2, true>(c, cls, first, n);
    case 3: return rl_sub<M, 3, true>(c, cls, first, n);
    case 4: return rl_sub<M, 4, true>(c, cls, first, n);
    case 5: if (cls != 0) return false; rl_run_co<M, 5, 1, 1>(c, first, n); return true;
    case 6: return rl_unary<M, 6, true, 512>(c, cls, first, n);
    case 7: return rl_unary<M, 7, true, 256>(c, cls, first, n);
    case 8:
        if (cls == 0) rl_run_co<M, 8, 1, 1>(c, first, n);
        else if (cls == 1) rl_run_co<M, 8, 2, 1>(c, first, n);
        else if (cls == 5) rl_run_co<M, 8, 170, 1>(c, first, n);
        else return false;
        return true;
    case 9: return rl_product<M, 9, true, false>(c, cls, first, n);
    case 10: if (cls != 1) return false; rl_run_co<M, 10, 2, 1>(c, first, n); return true;
    }
    return false;
}
static bool rl_dispatch(const RlCtx& c, bool coop, uint32_t mod, uint32_t op, uint32_t cls, uint32_t first, uint32_t n) {
    if (coop && n % 4) return false;
    switch (mod) {
    case 0: return coop ? rl_dispatch_co<ModQ>(c, op, cls, first, n) : rl_dispatch_one<ModQ>(c, op, cls, first, n);
    case 1: return coop ? rl_dispatch_co<ModN>(c, op, cls, first, n) : rl_dispatch_one<ModN>(c, op, cls, first, n);
    case 2: return coop ? rl_dispatch_co<ModT>(c, op, cls, first, n) : rl_dispatch_one<ModT>(c, op, cls, first, n);
    }
    return false;
}
// runs of equal (modulus, op, class) over one section
static bool rl_section(const RlCtx& c, bool coop, const uint32_t* recs, uint32_t count) {
    const size_t stride = coop ? RL_CO_IN : RL_ONE_IN;
    for (uint32_t first = 0; first < count;) {
        const uint32_t* r = recs + first * stride;
        uint32_t n = 1;
        while (first + n < count && memcmp(recs + (first + n) * stride, r, 16) == 0) n++;
        if (r[1] != (coop ? 1u : 0u) || !rl_dispatch(c, coop, r[0], r[2], r[3], first, n)) {
            fprintf(stderr, "raw_limbs: record %u (layout %u): modulus %u op %u class %u over %u records is not a case\n", first, r[1], r[0], r[2], r[3], n);
            return false;
        }
        first += n;
    }
    return true;
}

#ifndef ZK_HOST_BUILD
#define RL_HIP(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "raw_limbs: HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)
#endif

int main(int argc, char** argv) {
    if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fprintf(stderr, "raw_limbs: cannot read %s\n", argv[1]), 2;
    uint32_t hdr[4];
    if (fread(hdr, 4, 4, f) != 4 || hdr[0] != RL_MAGIC) return fprintf(stderr, "raw_limbs: bad header\n"), 2;
    const uint32_t n_one = hdr[1], n_coop = hdr[2];
    if (n_one > (1u << 24) || n_coop > (1u << 24)) return fprintf(stderr, "raw_limbs: too many records\n"), 2;
    std::vector<uint32_t> in((size_t)n_one * RL_ONE_IN + (size_t)n_coop * RL_CO_IN + 1), out((size_t)n_one * RL_ONE_OUT + (size_t)n_coop * RL_CO_OUT + 1, 0u);
    const size_t in_words = in.size() - 1, out_words = out.size() - 1;
    if (fread(in.data(), 4, in_words, f) != in_words || fgetc(f) != EOF) return fprintf(stderr, "raw_limbs: the file's length does not match its header\n"), 2;
    fclose(f);
    const uint32_t *one_recs = in.data(), *co_recs = in.data() + (size_t)n_one * RL_ONE_IN;
    RlCtx c;
#ifdef ZK_HOST_BUILD
    c.one_in = one_recs, c.co_in = co_recs;
    c.one_out = out.data(), c.co_out = out.data() + (size_t)n_one * RL_ONE_OUT;
#else
    uint32_t *d_in = nullptr, *d_out = nullptr;
    RL_HIP(hipMalloc(&d_in, 4 * (in_words + 1)));
    RL_HIP(hipMalloc(&d_out, 4 * (out_words + 1)));
    RL_HIP(hipMemcpy(d_in, in.data(), 4 * in_words, hipMemcpyHostToDevice));
    RL_HIP(hipMemset(d_out, 0, 4 * (out_words + 1)));
    c.one_in = d_in, c.co_in = d_in + (size_t)n_one * RL_ONE_IN;
    c.one_out = d_out, c.co_out = d_out + (size_t)n_one * RL_ONE_OUT;
#endif
    if (!rl_section(c, false, one_recs, n_one) || !rl_section(c, true, co_recs, n_coop)) return 1;
#ifndef ZK_HOST_BUILD
    RL_HIP(hipGetLastError());
    RL_HIP(hipDeviceSynchronize());
    RL_HIP(hipMemcpy(out.data(), d_out, 4 * out_words, hipMemcpyDeviceToHost));
    RL_HIP(hipFree(d_in));
    RL_HIP(hipFree(d_out));
#endif
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 4, out_words, f) != out_words || fclose(f) != 0) return fprintf(stderr, "raw_limbs: cannot write %s\n", argv[2]), 2;
    return 0;
}
