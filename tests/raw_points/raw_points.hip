// Raw-limb driver for the POINT LAWS of csrc/curve.h (one point per lane) and csrc/coop.h (one point per wave, a coordinate per 16-lane row): operands are built
// DIRECTLY from the limbs of the input file -- no fe_to_mont, no from_affine, no conversion of any kind -- and every coordinate of a result leaves exactly as the
// function returned it, so a test can hand the laws the identity, P + (-P), points of small order and every loose representation their types admit
// (tests/raw_points_common.py writes the vectors, tests/test_raw_points.py checks the results).  One source, two compilers:
//   g++ -x c++ -std=c++17 -DZK_HOST_BUILD -I zkp-ecdsa_amd/csrc raw_points.hip     host executable (coop.h runs through its SIMT emulation)
//   hipcc --offload-arch=gfx950 -std=c++17 -I zkp-ecdsa_amd/csrc raw_points.hip    device executable: one thread per one-lane record, one wave per cooperative
//                                                                                 record (the real DPP / ds_bpermute instructions)
// usage: raw_points IN OUT.   Both executables must write the same bytes for the same input.
//
// Vector format (every field a little-endian uint32):
//   header    'RAWP' (0x50574152), n_one, n_coop, 0
//   n_one one-lane records, then n_coop cooperative records:   layout (0 one lane, 1 cooperative) | n << 8, op, class, flags, e[n][9], n <= 8
//   e[k] is a field element of nine limbs; the elements e[n..7] that the file leaves out are zero.  One-lane operands: a P-256 point is three elements X, Y, Z, a Tom-256 point four, X, Y, T, Z; the first operand
//   starts at e[0], the second at e[3] (P-256 one-lane ops: a point, an affine entry x, y or the XYZZ entry) or e[4] (everything else).
//   Cooperative operands: rows 0..3 of the first register are e[0..3], of the second e[4..7] (limb j in lane j of the row, lanes 9..15 zero).
// Output: n_one records of 40 words (up to four result elements of 9 limbs, then four flag words; unused words zero), then n_coop records of 64 words (every lane).
//
// One-lane ops (the magnitude class of every operand is the one the function's signature declares):
//   P-256    0 p256_add   1 p256_add_mixed   2 p256_dbl   3 p256_jdbl (X, Y < 34 q, Z < 10 q)   4 p256_from_jac
//            5 p256_xyzz_sum_step: the sum X < 10 q, Y < 6 q, ZZ, ZZZ in e[0..3], the entry in e[4..5]; flags bit 0 = empty, bit 1 = nz (the digit is not zero);
//              result X, Y, ZZ, ZZZ, flag word 0 = empty, flag word 1 = p256_xyzz_sum_degenerate of the result
//            6 p256_xyzz_sum_point of the sum in e[0..3] (flags bit 0 = empty); flag word 0 = p256_xyzz_sum_degenerate
//            7 p256_select(flags bit 0, e[0..2], e[3..5])
//            8 flag word 0: is the point the identity?  x == 0 && z == 0 && y != 0 on the reduced coordinates  (k_pmsm.hip: k_pm_final; k_verify.hip: k_v_p256_*)
//              flag word 1: is the point at infinity?   fe_is_zero(fe_reduce(z))                               (k_p256.hip: the normalisers; k_verify.hip: k_v_exp_points)
//   Tom-256, a = 1 image (TomModel<TOM_MODEL_A1>) / a = -1 model of the comb tables (TomModel<TOM_MODEL_M1>):
//            9 tom_neg   10 / 16 add_pts   11 tom_dbl   17 add_pts_last
//            12 / 18 first   13 / 19 add   14 / 20 add_last of a table entry in e[4..6]: class 0 through entry(), class 1 through entry_neg(, flags bit 0)
//            21 tom_add_tab(p, ft_neg_sel(X2, neg), Y2, ft_neg_sel(d'T2, neg), Z2) of a Straus table entry in e[4..7], flags bit 0 = neg (k_verify.hip: k_v_straus)
//            15 is the point the identity?  class 0: x == 0 && y == z && z != 0 (k_msm.hip: k_msm_final; k_member.hip; k_verify.hip: tom_is_identity);
//               class 1: fe_is_zero(fe_reduce(x)) && y == z (k_tables.hip: k_tom_order_check)
// Cooperative ops: 0 co_p256_add   1 co_p256_dbl   2 co_p256_jdbl   3 co_p256_from_jac   4 co_tom_add   5 co_tom_dbl   6 co_tom_m1_add
//   7 co_tom_m1_add_tab (second register: the entry)   8 co_tom_m1_to_a1   9 co_p256_z_is_zero (the verdict in every lane)
//   10 co_tom_add_tab (second register: the Straus table entry X2, Y2, d'T2, Z2; flags bit 0 = neg)
//   11 co_p256_z_is_zero(co_p256_add(a, b)): the sum and its test as k_v_exp_points_co chains them
#include "coop.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define RP_MAGIC 0x50574152u
#define RP_IN 76
#define RP_ONE_OUT 40
#define RP_CO_OUT 64
#define RP_ONE_OPS 22
#define RP_CO_OPS 12

template <class M, int K>
ZK_DEV Fe<M, K> rp_ld(const uint32_t* e, int k) {
    Fe<M, K> r;
#pragma unroll
    for (int i = 0; i < NLIMB; i++) r.l[i] = e[k * NLIMB + i];
    return r;
}
template <class M, int K>
ZK_DEV void rp_st(uint32_t* o, int k, const Fe<M, K>& a) {
#pragma unroll
    for (int i = 0; i < NLIMB; i++) o[k * NLIMB + i] = a.l[i];
}
ZK_DEV P256Pt rp_p256(const uint32_t* e, int k) {
    P256Pt r;
    r.x = rp_ld<ModQ, 8>(e, k), r.y = rp_ld<ModQ, 8>(e, k + 1), r.z = rp_ld<ModQ, 8>(e, k + 2);
    return r;
}
ZK_DEV P256Aff rp_p256_aff(const uint32_t* e, int k) {
    P256Aff r;
    r.x = rp_ld<ModQ, 2>(e, k), r.y = rp_ld<ModQ, 2>(e, k + 1);
    return r;
}
ZK_DEV P256Jac rp_p256_jac(const uint32_t* e) {
    P256Jac r;
    r.x = rp_ld<ModQ, 34>(e, 0), r.y = rp_ld<ModQ, 34>(e, 1), r.z = rp_ld<ModQ, 10>(e, 2);
    return r;
}
ZK_DEV P256XyzzSum rp_xyzz(const uint32_t* e, uint32_t flags) {
    P256XyzzSum s;
    s.p.x = rp_ld<ModQ, 10>(e, 0), s.p.y = rp_ld<ModQ, 6>(e, 1), s.p.zz = rp_ld<ModQ, 2>(e, 2), s.p.zzz = rp_ld<ModQ, 2>(e, 3);
    s.empty = (flags & 1u) != 0;
    return s;
}
ZK_DEV void rp_st_p256(uint32_t* o, const P256Pt& p) { rp_st(o, 0, p.x), rp_st(o, 1, p.y), rp_st(o, 2, p.z); }
ZK_DEV TomPt rp_tom(const uint32_t* e, int k, TomPt*) {
    TomPt r;
    r.x = rp_ld<ModT, 2>(e, k), r.y = rp_ld<ModT, 2>(e, k + 1), r.t = rp_ld<ModT, 2>(e, k + 2), r.z = rp_ld<ModT, 2>(e, k + 3);
    return r;
}
ZK_DEV TomM1Pt rp_tom(const uint32_t* e, int k, TomM1Pt*) {
    TomM1Pt r;
    r.x = rp_ld<ModT, 12>(e, k), r.y = rp_ld<ModT, 8>(e, k + 1), r.t = rp_ld<ModT, 2>(e, k + 2), r.z = rp_ld<ModT, 2>(e, k + 3);
    return r;
}
ZK_DEV TomNiels rp_niels(const uint32_t* e) {   // a loaded table entry: three elements < 2 t in the slots of a TomNiels, whatever the model
    TomNiels r;
    r.x = rp_ld<ModT, 2>(e, 4), r.y = rp_ld<ModT, 2>(e, 5), r.dt = rp_ld<ModT, 2>(e, 6);
    return r;
}
template <class P>
ZK_DEV void rp_st_tom(uint32_t* o, const P& p) { rp_st(o, 0, p.x), rp_st(o, 1, p.y), rp_st(o, 2, p.t), rp_st(o, 3, p.z); }

// WHAT: 0 first, 1 add, 2 add_last of a table entry, through the model's interface as the comb kernels use it (k_tom.hip, k_tables.hip)
template <int MODEL, int WHAT>
ZK_DEV void rp_tom_entry(const uint32_t* e, uint32_t cls, uint32_t flags, uint32_t* o) {
    typedef TomModel<MODEL> TM;
    typedef typename TM::Pt Pt;
    const Pt p = rp_tom(e, 0, (Pt*)nullptr);
    const TomNiels q = rp_niels(e);
    if (cls == 0) {
        const auto en = TM::entry(q);
        if constexpr (WHAT == 0) rp_st_tom(o, TM::first(en));
        else if constexpr (WHAT == 1) rp_st_tom(o, TM::add(p, en));
        else rp_st_tom(o, TM::add_last(p, en));
    } else {
        const auto en = TM::entry_neg(q, (flags & 1u) != 0);
        if constexpr (WHAT == 0) rp_st_tom(o, TM::first(en));
        else if constexpr (WHAT == 1) rp_st_tom(o, TM::add(p, en));
        else rp_st_tom(o, TM::add_last(p, en));
    }
}

ZK_DEV void rp_one(const uint32_t* in, uint32_t* o) {
    const uint32_t op = in[1], cls = in[2], flags = in[3];
    const uint32_t* e = in + 4;
    switch (op) {
    case 0: rp_st_p256(o, p256_add(rp_p256(e, 0), rp_p256(e, 3))); break;
    case 1: rp_st_p256(o, p256_add_mixed(rp_p256(e, 0), rp_p256_aff(e, 3))); break;
    case 2: rp_st_p256(o, p256_dbl(rp_p256(e, 0))); break;
    case 3: {
        const P256Jac r = p256_jdbl(rp_p256_jac(e));
        rp_st(o, 0, r.x), rp_st(o, 1, r.y), rp_st(o, 2, r.z);
        break;
    }
    case 4: rp_st_p256(o, p256_from_jac(rp_p256_jac(e))); break;
    case 5: {
        P256XyzzSum s = rp_xyzz(e, flags);
        p256_xyzz_sum_step(s, (flags & 2u) != 0, rp_p256_aff(e, 4));
        rp_st(o, 0, s.p.x), rp_st(o, 1, s.p.y), rp_st(o, 2, s.p.zz), rp_st(o, 3, s.p.zzz);
        o[36] = s.empty ? 1u : 0u, o[37] = p256_xyzz_sum_degenerate(s) ? 1u : 0u;
        break;
    }
    case 6: {
        const P256XyzzSum s = rp_xyzz(e, flags);
        rp_st_p256(o, p256_xyzz_sum_point(s));
        o[36] = p256_xyzz_sum_degenerate(s) ? 1u : 0u;
        break;
    }
    case 7: rp_st_p256(o, p256_select((flags & 1u) != 0, rp_p256(e, 0), rp_p256(e, 3))); break;
    case 8: {   // flag word 0: k_pmsm.hip: k_pm_final, k_verify.hip: k_v_p256_straus_final / k_v_p256_final (weier.ts:117-119);
                // flag word 1: k_verify.hip: k_v_exp_points; k_p256.hip: `Fq2 rz = fe_reduce(acc.z); if (fe_is_zero(rz))` of the normalisers and the table walks
        const P256Pt acc = rp_p256(e, 0);
        o[36] = fe_is_zero(fe_reduce(acc.x)) && fe_is_zero(fe_reduce(acc.z)) && !fe_is_zero(fe_reduce(acc.y)) ? 1u : 0u;
        o[37] = fe_is_zero(fe_reduce(acc.z)) ? 1u : 0u;
        break;
    }
    case 9: rp_st_tom(o, tom_neg(rp_tom(e, 0, (TomPt*)nullptr))); break;
    case 10: rp_st_tom(o, TomModel<TOM_MODEL_A1>::add_pts(rp_tom(e, 0, (TomPt*)nullptr), rp_tom(e, 4, (TomPt*)nullptr))); break;
    case 11: rp_st_tom(o, tom_dbl(rp_tom(e, 0, (TomPt*)nullptr))); break;
    case 12: rp_tom_entry<TOM_MODEL_A1, 0>(e, cls, flags, o); break;
    case 13: rp_tom_entry<TOM_MODEL_A1, 1>(e, cls, flags, o); break;
    case 14: rp_tom_entry<TOM_MODEL_A1, 2>(e, cls, flags, o); break;
    case 15: {
        const TomPt a = rp_tom(e, 0, (TomPt*)nullptr);
        if (cls == 0) o[36] = fe_is_zero(a.x) && fe_eq(a.y, a.z) && !fe_is_zero(a.z) ? 1u : 0u;   // k_msm.hip: k_msm_final; k_member.hip; k_verify.hip: tom_is_identity
        else o[36] = fe_is_zero(fe_reduce(a.x)) && fe_eq(a.y, a.z) ? 1u : 0u;                     // k_tables.hip: k_tom_order_check
        break;
    }
    case 16: rp_st_tom(o, TomModel<TOM_MODEL_M1>::add_pts(rp_tom(e, 0, (TomM1Pt*)nullptr), rp_tom(e, 4, (TomM1Pt*)nullptr))); break;
    case 17: rp_st_tom(o, TomModel<TOM_MODEL_M1>::add_pts_last(rp_tom(e, 0, (TomM1Pt*)nullptr), rp_tom(e, 4, (TomM1Pt*)nullptr))); break;
    case 18: rp_tom_entry<TOM_MODEL_M1, 0>(e, cls, flags, o); break;
    case 19: rp_tom_entry<TOM_MODEL_M1, 1>(e, cls, flags, o); break;
    case 20: rp_tom_entry<TOM_MODEL_M1, 2>(e, cls, flags, o); break;
    case 21: {
        const bool neg = (flags & 1u) != 0;
        rp_st_tom(o, tom_add_tab(rp_tom(e, 0, (TomPt*)nullptr), ft_neg_sel(rp_ld<ModT, 2>(e, 4), neg), rp_ld<ModT, 2>(e, 5), ft_neg_sel(rp_ld<ModT, 2>(e, 6), neg), rp_ld<ModT, 2>(e, 7)));
        break;
    }
    }
}

// a and b: the two registers of the record; the op is the same in every lane of the wave
ZK_DEV CoU32 rp_co(uint32_t op, uint32_t flags, const CoU32& av, const CoU32& bv) {
    switch (op) {
    case 0:
    case 1:
    case 3:
    case 9:
    case 11: {
        const CoU32 mj = co_limbs(ModQ::mod);
        CoP256 a, b;
        a.v.v = av, b.v.v = bv;
        if (op == 0) return co_p256_add(a, b, mj).v.v;
        if (op == 11) return co_splat(co_p256_z_is_zero(co_p256_add(a, b, mj), mj) ? 1u : 0u);
        if (op == 1) return co_p256_dbl(a, mj).v.v;
        if (op == 9) return co_splat(co_p256_z_is_zero(a, mj) ? 1u : 0u);
        CoP256J j;
        j.v.v = av;
        return co_p256_from_jac(j, mj).v.v;
    }
    case 2: {
        CoP256J j;
        j.v.v = av;
        return co_p256_jdbl(j, co_limbs(ModQ::mod)).v.v;
    }
    default: {
        const CoU32 mj = co_limbs(ModT::mod);
        CoTom a, b;
        a.v.v = av, b.v.v = bv;
        if (op == 4) return co_tom_add(a, b, mj).v.v;
        if (op == 5) return co_tom_dbl(a, mj).v.v;
        if (op == 6) return co_tom_m1_add(a, b, mj).v.v;
        if (op == 7) return co_tom_m1_add_tab(a, b.v, mj).v.v;
        if (op == 10) return co_tom_add_tab(a, b.v, (flags & 1u) != 0, mj).v.v;
        return co_tom_m1_to_a1(a, mj).v.v;
    }
    }
}

#ifndef ZK_HOST_BUILD
__global__ void __launch_bounds__(64) k_rp_one(const uint32_t* in, uint32_t* out, uint32_t n) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) rp_one(in + (size_t)i * RP_IN, out + (size_t)i * RP_ONE_OUT);
}
// one wave per block and record
__global__ void __launch_bounds__(64) k_rp_co(const uint32_t* in, uint32_t* out) {
    const uint32_t lane = threadIdx.x, row = lane >> 4, j = lane & 15u;
    const uint32_t* r = in + (size_t)blockIdx.x * RP_IN;
    const uint32_t a = j < NLIMB ? r[4 + row * NLIMB + j] : 0u, b = j < NLIMB ? r[4 + (4 + row) * NLIMB + j] : 0u;
    out[(size_t)blockIdx.x * RP_CO_OUT + lane] = rp_co(r[1], r[3], a, b);
}
#define RP_HIP(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "raw_points: HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)
#endif

int main(int argc, char** argv) {
    if (argc != 3) return fprintf(stderr, "usage: %s IN OUT\n", argv[0]), 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fprintf(stderr, "raw_points: cannot read %s\n", argv[1]), 2;
    uint32_t hdr[4];
    if (fread(hdr, 4, 4, f) != 4 || hdr[0] != RP_MAGIC) return fprintf(stderr, "raw_points: bad header\n"), 2;
    const uint32_t n_one = hdr[1], n_coop = hdr[2];
    if (n_one > (1u << 20) || n_coop > (1u << 20)) return fprintf(stderr, "raw_points: too many records\n"), 2;
    std::vector<uint32_t> in((size_t)(n_one + n_coop) * RP_IN + 1, 0u), out((size_t)n_one * RP_ONE_OUT + (size_t)n_coop * RP_CO_OUT + 1, 0u);
    const size_t out_words = out.size() - 1;
    for (uint32_t i = 0; i < n_one + n_coop; i++) {   // every record is a case before anything runs; in memory a record has all eight elements
        uint32_t* r = in.data() + (size_t)i * RP_IN;
        const uint32_t coop = i < n_one ? 0u : 1u;
        if (fread(r, 4, 4, f) != 4) return fprintf(stderr, "raw_points: the file's length does not match its header\n"), 2;
        const uint32_t nelem = r[0] >> 8;
        r[0] &= 0xffu;
        if (r[0] != coop || nelem > 8 || r[1] >= (coop ? RP_CO_OPS : RP_ONE_OPS) || r[2] > 1 || r[3] > 3)
            return fprintf(stderr, "raw_points: record %u: layout %u op %u class %u flags %u with %u elements is not a case\n", i, r[0], r[1], r[2], r[3], nelem), 1;
        if (fread(r + 4, 4, (size_t)nelem * NLIMB, f) != (size_t)nelem * NLIMB) return fprintf(stderr, "raw_points: the file's length does not match its header\n"), 2;
    }
    if (fgetc(f) != EOF) return fprintf(stderr, "raw_points: the file's length does not match its header\n"), 2;
    fclose(f);
    const uint32_t* co_in = in.data() + (size_t)n_one * RP_IN;
    uint32_t* co_out = out.data() + (size_t)n_one * RP_ONE_OUT;
#ifdef ZK_HOST_BUILD
    for (uint32_t i = 0; i < n_one; i++) rp_one(in.data() + (size_t)i * RP_IN, out.data() + (size_t)i * RP_ONE_OUT);
    for (uint32_t w = 0; w < n_coop; w++) {
        const uint32_t* r = co_in + (size_t)w * RP_IN;
        CoU32 a, b;
        for (int i = 0; i < 64; i++) {
            const int row = i >> 4, j = i & 15;
            a.v[i] = j < NLIMB ? r[4 + row * NLIMB + j] : 0u, b.v[i] = j < NLIMB ? r[4 + (4 + row) * NLIMB + j] : 0u;
        }
        const CoU32 res = rp_co(r[1], r[3], a, b);
        for (int i = 0; i < 64; i++) co_out[(size_t)w * RP_CO_OUT + i] = res.v[i];
    }
#else
    (void)co_in, (void)co_out;
    const size_t in_words = in.size() - 1;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    RP_HIP(hipMalloc(&d_in, 4 * (in_words + 1)));
    RP_HIP(hipMalloc(&d_out, 4 * (out_words + 1)));
    RP_HIP(hipMemcpy(d_in, in.data(), 4 * in_words, hipMemcpyHostToDevice));
    RP_HIP(hipMemset(d_out, 0, 4 * (out_words + 1)));
    if (n_one) hipLaunchKernelGGL(k_rp_one, dim3((n_one + 63) / 64), dim3(64), 0, 0, d_in, d_out, n_one);
    if (n_coop) hipLaunchKernelGGL(k_rp_co, dim3(n_coop), dim3(64), 0, 0, d_in + (size_t)n_one * RP_IN, d_out + (size_t)n_one * RP_ONE_OUT);
    RP_HIP(hipGetLastError());
    RP_HIP(hipDeviceSynchronize());
    RP_HIP(hipMemcpy(out.data(), d_out, 4 * out_words, hipMemcpyDeviceToHost));
    RP_HIP(hipFree(d_in));
    RP_HIP(hipFree(d_out));
#endif
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 4, out_words, f) != out_words || fclose(f) != 0) return fprintf(stderr, "raw_points: cannot write %s\n", argv[2]), 2;
    return 0;
}
