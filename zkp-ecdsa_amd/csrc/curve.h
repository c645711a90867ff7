// Point arithmetic on the two groups of the hot path, one point per lane (gfx950).
//   * P-256 (src/curves/weier.ts): projective (X:Y:Z), a = -3, Renes-Costello-Batina COMPLETE addition and
//     doubling -- the same step sequences the reference uses (weier.ts:133-230), so identity / P = Q inputs behave
//     exactly as in the reference.
//   * Tom-256 (src/curves/edwards.ts): twisted Edwards a*x^2 + y^2 = 1 + d*x^2*y^2 in extended coordinates.  The
//     engine works on the isomorphic curve x'^2 + y^2 = 1 + (d/a) x'^2 y^2 (x' = sqrt(a) x), whose unified
//     Hisil-Wong-Carter-Dawson addition (edwards.ts:161-183 with a = 1) needs no multiplication by a.  a is a
//     square and d/a a non-square mod t (checked in tools/gen_consts.py), so the law is complete.  Only affine
//     coordinates of the original curve ever leave the engine (hash inputs, proof bytes).
#pragma once
#include "field.h"

// Independent products of a point formula in lock-step (field.h: limbs_mont_mul_n) or one after the other; chosen per
// translation unit and per curve with -DZK_BATCH_TOM=0/1, -DZK_BATCH_P256=0/1 (csrc/Makefile).
#ifndef ZK_BATCH_TOM
#define ZK_BATCH_TOM 1
#endif
#ifndef ZK_BATCH_P256
#define ZK_BATCH_P256 1
#endif

typedef Fe<ModQ, 8> Fq8;  // P-256 coordinate: < 8q
typedef Fe<ModQ, 2> Fq2;
typedef Fe<ModT, 2> Ft2;  // Tom coordinate: < 2t
typedef Fe<ModN, 2> Fn2;

struct P256Pt {
    Fq8 x, y, z;
};
struct P256Aff {  // Montgomery affine, canonical not required
    Fq2 x, y;
};
ZK_DEV P256Pt p256_identity() {  // weier.ts:50-52
    P256Pt r;
    r.x = fe_zero<ModQ>().as<8>();
    r.y = fe_one_mont<ModQ>().as<8>();
    r.z = fe_zero<ModQ>().as<8>();
    return r;
}
ZK_DEV P256Pt p256_from_affine(const P256Aff& a) {
    P256Pt r;
    r.x = a.x.as<8>();
    r.y = a.y.as<8>();
    r.z = fe_one_mont<ModQ>().as<8>();
    return r;
}
// weier.ts:176-230 (RCB 2016, Algorithm 4, a = -3): 12M + 2 mult-by-b
ZK_DEV P256Pt p256_add(const P256Pt& p, const P256Pt& q) {
    const auto b = fe_const<ModQ, 1>(P256_B_M);
    Fq2 t0, t1, t2, t3, t4, x3;
    fe_mul3<ZK_BATCH_P256 != 0>(t0, t1, t2, p.x, q.x, p.y, q.y, p.z, q.z);
    fe_mul3<ZK_BATCH_P256 != 0>(t3, t4, x3, p.x + p.y, q.x + q.y, p.y + p.z, q.y + q.z, p.x + p.z, q.x + q.z);
    auto t3b = fe_sub2(t3, t0, t1);
    auto t4b = fe_sub2(t4, t1, t2);
    auto y3 = fe_sub2(x3, t0, t2);
    Fq2 z3, y3b;
    fe_mul2<ZK_BATCH_P256 != 0>(z3, y3b, b, t2, b, y3);
    auto x3b = y3 - z3;
    auto x3c = x3b + (x3b + x3b);
    auto z3b = t1 - x3c;
    auto x3d = t1 + x3c;
    auto t2b = t2 + t2 + t2;
    auto y3c = fe_sub2(y3b, t2b, t0);
    auto y3d = y3c + (y3c + y3c);
    auto t0b = (t0 + t0 + t0) - t2b;
    Fq2 t1b, t2c, m1, m2, m3, m4;
    fe_mul3<ZK_BATCH_P256 != 0>(t1b, t2c, m1, t4b, y3d, t0b, y3d, x3d, z3b);
    fe_mul3<ZK_BATCH_P256 != 0>(m2, m3, m4, t3b, x3d, t4b, z3b, t3b, t0b);
    auto y3e = m1 + t2c;
    auto x3e = m2 - t1b;
    auto z3c = m3 + m4;
    P256Pt r;
    r.x = x3e.template as<8>();
    r.y = y3e.template as<8>();
    r.z = z3c.template as<8>();
    return r;
}
// Same law with q affine (Z2 = 1): RCB Algorithm 5 shape, 11M + 2 mult-by-b.  q must not be the identity.
ZK_DEV P256Pt p256_add_mixed(const P256Pt& p, const P256Aff& q) {
    const auto b = fe_const<ModQ, 1>(P256_B_M);
    Fq2 t0, t1, t3, m4, m5, z3;
    fe_mul3<ZK_BATCH_P256 != 0>(t0, t1, t3, p.x, q.x, p.y, q.y, p.x + p.y, q.x + q.y);
    fe_mul3<ZK_BATCH_P256 != 0>(m4, m5, z3, q.y, p.z, q.x, p.z, b, p.z);
    auto t3b = fe_sub2(t3, t0, t1);
    auto t4b = m4 + p.y;   // (y1+z1)(y2+1) - t1 - z1
    auto y3 = m5 + p.x;    // (x1+z1)(x2+1) - t0 - z1
    auto x3b = y3 - z3;
    auto x3c = x3b + (x3b + x3b);
    auto z3b = t1 - x3c;
    auto x3d = t1 + x3c;
    auto y3b = b * y3;
    auto t2b = p.z + p.z + p.z;
    auto y3c = fe_sub2(y3b, t2b, t0);
    auto y3d = y3c + (y3c + y3c);
    auto t0b = (t0 + t0 + t0) - t2b;
    Fq2 t1b, t2c, m1, m2, m3, m6;
    fe_mul3<ZK_BATCH_P256 != 0>(t1b, t2c, m1, t4b, y3d, t0b, y3d, x3d, z3b);
    fe_mul3<ZK_BATCH_P256 != 0>(m2, m3, m6, t3b, x3d, t4b, z3b, t3b, t0b);
    auto y3e = m1 + t2c;
    auto x3e = m2 - t1b;
    auto z3c = m3 + m6;
    P256Pt r;
    r.x = x3e.template as<8>();
    r.y = y3e.template as<8>();
    r.z = z3c.template as<8>();
    return r;
}
// weier.ts:133-175 (RCB Algorithm 6, a = -3): 8M + 3S incl. 2 mult-by-b
ZK_DEV P256Pt p256_dbl(const P256Pt& p) {
    const auto b = fe_const<ModQ, 1>(P256_B_M);
    Fq2 t0, t1, t2, t3, z3, t0c;
    fe_mul3<ZK_BATCH_P256 != 0>(t0, t1, t2, p.x, p.x, p.y, p.y, p.z, p.z);
    fe_mul3<ZK_BATCH_P256 != 0>(t3, z3, t0c, p.x, p.y, p.x, p.z, p.y, p.z);
    auto t3b = t3 + t3;
    auto z3b = z3 + z3;
    Fq2 bt2, bz3;
    fe_mul2<ZK_BATCH_P256 != 0>(bt2, bz3, b, t2, b, z3b);
    auto y3 = bt2 - z3b;
    auto y3b = y3 + (y3 + y3);
    auto x3 = t1 - y3b;
    auto y3c = t1 + y3b;
    auto t2b = t2 + t2 + t2;
    auto z3c = fe_sub2(bz3, t2b, t0);
    auto z3d = z3c + (z3c + z3c);
    auto t0b = (t0 + t0 + t0) - t2b;
    auto t0d = t0c + t0c;
    Fq2 y3d, x3b, m1, m2, z3e;
    fe_mul3<ZK_BATCH_P256 != 0>(y3d, x3b, m1, x3, y3c, x3, t3b, t0b, z3d);
    fe_mul2<ZK_BATCH_P256 != 0>(m2, z3e, t0d, z3d, t0d, t1);
    auto y3e = y3d + m1;
    auto x3c = x3b - m2;
    auto z3f = (z3e + z3e) + (z3e + z3e);
    P256Pt r;
    r.x = x3c.template as<8>();
    r.y = y3e.template as<8>();
    r.z = z3f.template as<8>();
    return r;
}
// Jacobian doubling for a = -3 (x = X / Z^2, y = Y / Z^3; "dbl-2001-b": 3M + 5S against the 13 products of the complete doubling above).  Only for the
// doubling CHAINS of the per-proof window tables of R (k_rtab_base: 256 doublings in a row, what a single verification waits for longest): their points
// have odd prime order, which is all the formula needs (it is wrong for Y = 0, a point of order 2; the identity (X : Y : 0) stays (0 : Y' : 0), Y' != 0).
// Magnitudes: the lazy subtractions at the end leave X, Y < 34 q and Z < 10 q; as inputs of the next doubling their products stay far inside
// ModQ::kmax ((34 + 10)^2, (34 + 4)(34 + 2)), so the chain needs no reduction of its own.
struct P256Jac {
    Fe<ModQ, 34> x, y;
    Fe<ModQ, 10> z;
};
ZK_DEV P256Jac p256_jac_from(const P256Pt& p) {   // a point with Z = 1 (p256_from_affine) or the identity (0 : 1 : 0): the same triple in both systems
    P256Jac r;
    r.x = p.x.as<34>(), r.y = p.y.as<34>(), r.z = p.z.as<10>();
    return r;
}
ZK_DEV P256Jac p256_jdbl(const P256Jac& p) {
    Fq2 delta, gamma, yz2;
    fe_mul3<ZK_BATCH_P256 != 0>(delta, gamma, yz2, p.z, p.z, p.y, p.y, p.y + p.z, p.y + p.z);
    Fq2 beta, a0, g2;
    fe_mul3<ZK_BATCH_P256 != 0>(beta, a0, g2, p.x, gamma, p.x - delta, p.x + delta, gamma, gamma);
    auto alpha = a0 + (a0 + a0);
    auto b4 = (beta + beta) + (beta + beta);
    auto g4 = (g2 + g2) + (g2 + g2);
    Fq2 al2 = alpha * alpha;
    auto x3 = fe_sub2(al2, b4, b4);
    Fq2 m = alpha * (b4 - x3);
    auto y3 = fe_sub2(m, g4, g4);
    auto z3 = fe_sub2(yz2, gamma, delta);
    P256Jac r;
    r.x = x3, r.y = y3, r.z = z3;
    return r;
}
ZK_DEV P256Pt p256_from_jac(const P256Jac& p) {   // (X : Y : Z) Jacobian -> (X Z : Y : Z^3) homogeneous, the form the complete additions take
    Fq2 z2 = p.z * p.z;
    Fq2 xz, z3;
    fe_mul2<ZK_BATCH_P256 != 0>(xz, z3, p.x, p.z, z2, p.z);
    Fq2 y = fe_reduce(p.y);   // the additions take coordinates < 8 q
    P256Pt r;
    r.x = xz.template as<8>();
    r.y = y.as<8>();
    r.z = z3.template as<8>();
    return r;
}
ZK_DEV P256Pt p256_select(bool c, const P256Pt& a, const P256Pt& b) {
    P256Pt r;
    r.x = fe_select(c, a.x, b.x);
    r.y = fe_select(c, a.y, b.y);
    r.z = fe_select(c, a.z, b.z);
    return r;
}
// A table sum skips the addition of a ZERO digit.  Default build: with a branch -- the lane idles while its neighbours add, which is what keeps the table
// sums at 124-140 registers and three waves per SIMD, but makes control flow depend on digits of secret scalars (nonces, blinders).  -DZK_UNIFORM_CF=1
// (`make uniform`: lib/libzkattest_hip_uniform.so): the addition is always computed, on a valid entry, and discarded by a select; control flow and the
// set of executed instructions no longer depend on secret data (addresses of the table gathers still do: see INTEGRATION.md, "side channels").
#ifndef ZK_UNIFORM_CF
#define ZK_UNIFORM_CF 0
#endif
#if ZK_UNIFORM_CF
#define ZK_ADD_IF(cond, acc, sum_expr)                 \
    do {                                               \
        const bool c__ = (cond);                       \
        const P256Pt s__ = (sum_expr);                 \
        (acc) = p256_select(c__, s__, (acc));          \
    } while (0)
#else
#define ZK_ADD_IF(cond, acc, sum_expr)                 \
    do {                                               \
        if (cond) (acc) = (sum_expr);                  \
    } while (0)
#endif

// XYZZ coordinates (x = X / ZZ, y = Y / ZZZ, ZZ^3 = ZZZ^2) for the SUMS OF AFFINE TABLE ENTRIES of k_exp_commit_kt (rtab.h / ktab.h: the *_xyzz walks): the
// generic mixed addition "madd-2008-s" costs 8 products and 2 squarings against the 13 products of p256_add_mixed.  It is NOT complete: it is wrong when the
// running point is the identity and when the entry has the running point's x (P = 0 below: a doubling, or a sum that is the identity).  The walks never test
// for either per step:
//   * a sum starts EMPTY (P256XyzzSum::empty) and its first entry is copied, so the law never sees the identity as an operand;
//   * ZZ' = ZZ P^2 and ZZZ' = ZZZ P^3: one step with P = 0 leaves ZZ = 0 for the rest of the sum, whatever is added afterwards.  A final ZZ != 0 therefore proves
//     that every step was a generic addition of two points with different x, and ONE zero test of ZZ per stored point decides whether the lane recomputes the sum
//     with the complete law (never on honest inputs; a prover who knows the discrete log of its key can craft scalars that get there).
// Magnitudes: the lazy subtractions leave X < 10 q and Y < 6 q; as operands of the next addition (P = U2 - X < 18 q, R = S2 - Y < 10 q, Q - X' < 18 q) every
// product stays far inside ModQ::kmax (18 * 18, 10 * 18), so a chain of additions needs no reduction of its own.
struct P256Xyzz {
    Fe<ModQ, 10> x;
    Fe<ModQ, 6> y;
    Fq2 zz, zzz;
};
ZK_DEV P256Xyzz p256_xyzz_from_affine(const P256Aff& a) {
    P256Xyzz r;
    r.x = a.x.as<10>(), r.y = a.y.as<6>();
    r.zz = fe_one_mont<ModQ>().as<2>(), r.zzz = fe_one_mont<ModQ>().as<2>();
    return r;
}
// the two squarings of the addition below: the squaring form (45 + 81 multiply-adds) where the translation unit computes its products one after the other,
// the lock-step pair (field.h: limbs_mont_mul_n) where it batches them
template <int Ka, int Kb>
ZK_DEV void p256_sqr2(Fq2& r0, Fq2& r1, const Fe<ModQ, Ka>& a, const Fe<ModQ, Kb>& b) {
#if ZK_BATCH_P256 && !defined(ZK_HOST_BUILD)
    fe_mul2<true>(r0, r1, a, a, b, b);
#else
    r0 = fe_sqr(a), r1 = fe_sqr(b);
#endif
}
// p + q, q affine and not the identity, p not the identity, x(p) != x(q): four lock-step groups, 2 + 2 + 3 + 3 products
ZK_DEV P256Xyzz p256_xyzz_madd(const P256Xyzz& p, const P256Aff& q) {
    Fq2 u2, s2;
    fe_mul2<ZK_BATCH_P256 != 0>(u2, s2, q.x, p.zz, q.y, p.zzz);
    auto P = u2 - p.x;
    auto R = s2 - p.y;
    Fq2 pp, rr;
    Fq2 ppp, Q;
    P256Xyzz r;
    p256_sqr2(pp, rr, P, R);
    fe_mul3<ZK_BATCH_P256 != 0>(ppp, Q, r.zz, P, pp, p.x, pp, p.zz, pp);
    auto x3 = fe_sub2(rr, ppp, Q + Q);
    Fq2 m1, m2;
    fe_mul3<ZK_BATCH_P256 != 0>(m1, m2, r.zzz, R, Q - x3, p.y, ppp, p.zzz, ppp);
    r.x = x3;
    r.y = m1 - m2;
    return r;
}
// (X : Y : ZZ : ZZZ) -> (X ZZZ : Y ZZ : ZZ ZZZ) homogeneous, the form the stores, the normaliser and k_t1 take: 3 products
ZK_DEV P256Pt p256_from_xyzz(const P256Xyzz& p) {
    Fq2 x, y, z;
    fe_mul3<ZK_BATCH_P256 != 0>(x, y, z, p.x, p.zzz, p.y, p.zz, p.zz, p.zzz);
    P256Pt r;
    r.x = x.as<8>(), r.y = y.as<8>(), r.z = z.as<8>();
    return r;
}
ZK_DEV P256Xyzz p256_xyzz_select(bool c, const P256Xyzz& a, const P256Xyzz& b) {
    P256Xyzz r;
    r.x = fe_select(c, a.x, b.x), r.y = fe_select(c, a.y, b.y);
    r.zz = fe_select(c, a.zz, b.zz), r.zzz = fe_select(c, a.zzz, b.zzz);
    return r;
}
// A sum of table entries under way.  empty: nothing added yet (p is then all zeros and never read as a point).
struct P256XyzzSum {
    P256Xyzz p;
    bool empty;
};
ZK_DEV P256XyzzSum p256_xyzz_sum_empty() {
    P256XyzzSum s;
    s.p.x = fe_zero<ModQ>().as<10>(), s.p.y = fe_zero<ModQ>().as<6>();
    s.p.zz = fe_zero<ModQ>().as<2>(), s.p.zzz = fe_zero<ModQ>().as<2>();
    s.empty = true;
    return s;
}
// one step of a table walk: the entry e of a NON-ZERO digit (nz) joins the sum -- copied into an empty sum, added otherwise; a zero digit changes nothing.
// Default build: the caller branches on nz (and loads e inside the branch); -DZK_UNIFORM_CF=1: computed on a valid entry and discarded by select, like ZK_ADD_IF.
ZK_DEV void p256_xyzz_sum_step(P256XyzzSum& s, bool nz, const P256Aff& e) {
#if ZK_UNIFORM_CF
    const P256Xyzz a = p256_xyzz_madd(s.p, e), c = p256_xyzz_from_affine(e);
    s.p = p256_xyzz_select(nz, p256_xyzz_select(s.empty, c, a), s.p);
    s.empty = s.empty && !nz;
#else
    if (nz) {
        if (s.empty) s.p = p256_xyzz_from_affine(e);
        else s.p = p256_xyzz_madd(s.p, e);
        s.empty = false;
    }
#endif
}
// did the sum meet an exceptional pair?  (the canonical zero test of ZZ, once per stored point)
ZK_DEV bool p256_xyzz_sum_degenerate(const P256XyzzSum& s) { return !s.empty && fe_is_zero(s.p.zz); }
// the sum as a homogeneous point; an empty sum is the identity (0 : 1 : 0).  Meaningless where p256_xyzz_sum_degenerate.
ZK_DEV P256Pt p256_xyzz_sum_point(const P256XyzzSum& s) { return p256_select(s.empty, p256_identity(), p256_from_xyzz(s.p)); }

// y^2 == x^3 - 3x + b  (weier.ts:56-70 with Z = 1)
ZK_DEV bool p256_on_curve(const P256Aff& a) {
    const auto b = fe_const<ModQ, 1>(P256_B_M);
    auto y2 = a.y * a.y;
    auto x2 = a.x * a.x;
    auto x3 = x2 * a.x;
    auto rhs = (x3 + b) - (a.x + a.x + a.x);
    return fe_eq(y2, rhs);
}

// ECDSA's last step without a field inversion: is x(R) mod n == r for R = (X : Y : Z) and a canonical r in [1, n)?  x = X / Z lies in [0, p) and
// n < p < 2 n, so x mod n == r exactly when x == r or -- only where r + n < p, the wrap case R.x in [n, p) -- x == r + n: X == r Z or X == (r + n) Z mod p.
// The identity (Z == 0) has no x-coordinate: false.  Device and host (tests/host_arith/host_screen.cpp).
ZK_DEV bool p256_x_is_r_mod_n(const P256Pt& R, const Fe<ModN, 1>& r) {
    Fe<ModQ, 1> r0;
    Fe<ModQ, 2> r1;   // r + n as a plain integer < 2 n < 2^257
#pragma unroll
    for (int i = 0; i < NLIMB; i++) r0.l[i] = r.l[i], r1.l[i] = r.l[i] + ModN::mod[i];
    limbs_normalize(r1.l);
    const bool wrap = !limbs_geq_mod<ModQ>(r1.l);   // r + n < p
    const Fq2 z = fe_reduce(R.z);
    const bool eq0 = fe_eq(R.x, fe_to_mont(r0) * z), eq1 = fe_eq(R.x, fe_to_mont(r1) * z);
    return !fe_is_zero(z) && (eq0 || (wrap && eq1));
}

// ---------------------------------------------------------------- Tom-256 on the a = 1 image
struct TomPt {  // extended (X:Y:T:Z), Montgomery
    Ft2 x, y, t, z;
};
template <int KX>
struct TomNielsT {  // affine precomputed: x, y, (d/a)*x*y; x and dt may carry a looser bound (negated entries)
    Fe<ModT, KX> x;
    Ft2 y;
    Fe<ModT, KX> dt;
};
typedef TomNielsT<2> TomNiels;
// -P of a table entry when neg (signed comb digits): (-x, y, -dt) with -v = 4t - v < 4t
ZK_DEV TomNielsT<4> tom_niels_neg_sel(const TomNiels& q, bool neg) {
    TomNielsT<4> r;
#pragma unroll
    for (int i = 0; i < NLIMB; i++) {
        r.x.l[i] = neg ? ModT::sub4[i] - q.x.l[i] : q.x.l[i];
        r.dt.l[i] = neg ? ModT::sub4[i] - q.dt.l[i] : q.dt.l[i];
    }
    limbs_normalize(r.x.l);
    limbs_normalize(r.dt.l);
    r.y = q.y;
    return r;
}
ZK_DEV TomPt tom_identity() {  // edwards.ts:46-48
    TomPt r;
    r.x = fe_zero<ModT>().as<2>();
    r.y = fe_one_mont<ModT>().as<2>();
    r.t = fe_zero<ModT>().as<2>();
    r.z = fe_one_mont<ModT>().as<2>();
    return r;
}
// edwards.ts:161-183 with a = 1 and Z2 = 1, d*T2 precomputed: 8M, as two lock-step groups of four independent products
template <int KX>
ZK_DEV TomPt tom_add_niels(const TomPt& p, const TomNielsT<KX>& q) {
    Ft2 A, B, C, P4;
    fe_mul4<ZK_BATCH_TOM != 0>(A, B, C, P4, p.x, q.x, p.y, q.y, p.t, q.dt, p.x + p.y, q.x + q.y);
    auto E = fe_sub2(P4, A, B);
    auto F = p.z - C;
    auto G = p.z + C;
    auto H = B - A;
    TomPt r;
    fe_mul4<ZK_BATCH_TOM != 0>(r.x, r.y, r.t, r.z, E, F, G, H, E, H, F, G);
    return r;
}
// the same addition when the result only has to be ADDED TO NOTHING ELSE (last step of a comb): no T3, 7M
template <int KX>
ZK_DEV TomPt tom_add_niels_last(const TomPt& p, const TomNielsT<KX>& q) {
    Ft2 A, B, C, P4;
    fe_mul4<ZK_BATCH_TOM != 0>(A, B, C, P4, p.x, q.x, p.y, q.y, p.t, q.dt, p.x + p.y, q.x + q.y);
    auto E = fe_sub2(P4, A, B);
    auto F = p.z - C;
    auto G = p.z + C;
    auto H = B - A;
    TomPt r;
    fe_mul3<ZK_BATCH_TOM != 0>(r.x, r.y, r.z, E, F, G, H, F, G);
    r.t = fe_zero<ModT>().as<2>();
    return r;
}
// identity + q: the niels entry as an extended point (X, Y, T = XY, Z = 1), 1M instead of the 8M of an addition
template <int KX>
ZK_DEV TomPt tom_from_niels(const TomNielsT<KX>& q) {
    TomPt r;
    if constexpr (KX == 2) r.x = q.x;
    else r.x = fe_reduce(q.x);  // a (possibly negated) entry with the looser bound: one extra product
    r.y = q.y;
    r.t = q.x * q.y;
    r.z = fe_one_mont<ModT>().as<2>();
    return r;
}
// general unified addition (both extended): 9M + 1 mult-by-d'
ZK_DEV TomPt tom_add(const TomPt& p, const TomPt& q) {
    const auto d1 = fe_const<ModT, 1>(TOM_D1_M);
    Ft2 A, B, C0, D, P4;
    fe_mul4<ZK_BATCH_TOM != 0>(A, B, C0, D, p.x, q.x, p.y, q.y, p.t, q.t, p.z, q.z);
    Ft2 C;
    fe_mul2<ZK_BATCH_TOM != 0>(C, P4, C0, d1, p.x + p.y, q.x + q.y);
    auto E = fe_sub2(P4, A, B);
    auto F = D - C;
    auto G = D + C;
    auto H = B - A;
    TomPt r;
    fe_mul4<ZK_BATCH_TOM != 0>(r.x, r.y, r.t, r.z, E, F, G, H, E, H, F, G);
    return r;
}
// addition with an entry (X2, Y2, d'T2, Z2) of the verifier's Straus tables (k_verify.hip: st_tab, k_v_straus): 9 modmuls
template <int KX>
ZK_DEV TomPt tom_add_tab(const TomPt& p, const Fe<ModT, KX>& x2, const Ft2& y2, const Fe<ModT, KX>& dt2, const Ft2& z2) {
    auto A = p.x * x2;
    auto B = p.y * y2;
    auto C = p.t * dt2;
    auto D = p.z * z2;
    auto E = ((p.x + p.y) * (x2 + y2) - A) - B;
    auto F = D - C;
    auto G = D + C;
    auto H = B - A;
    TomPt r;
    r.x = E * F, r.y = G * H, r.t = E * H, r.z = F * G;
    return r;
}
// -v for a coordinate < 2t: 4t - v < 4t ... kept below 4t, which the products of tom_add_tab accept (2 * 4 <= kmax)
ZK_DEV Fe<ModT, 4> ft_neg_sel(const Ft2& v, bool neg) {
    Fe<ModT, 4> r;
#pragma unroll
    for (int i = 0; i < NLIMB; i++) r.l[i] = neg ? ModT::sub4[i] - v.l[i] : v.l[i];
    limbs_normalize(r.l);
    return r;
}
// edwards.ts:141-160 with a = 1: 4S + 4M
ZK_DEV TomPt tom_dbl(const TomPt& p) {
    Ft2 A, B, Cz, S;
    auto xy = p.x + p.y;
    fe_mul4<ZK_BATCH_TOM != 0>(A, B, Cz, S, p.x, p.x, p.y, p.y, p.z, p.z, xy, xy);
    auto C = Cz + Cz;
    auto E = fe_sub2(S, A, B);
    auto G = A + B;
    auto F = G - C;
    auto H = A - B;
    TomPt r;
    fe_mul4<ZK_BATCH_TOM != 0>(r.x, r.y, r.t, r.z, E, F, G, H, E, H, F, G);
    return r;
}
ZK_DEV TomPt tom_neg(const TomPt& p) {  // edwards.ts:136-140
    TomPt r;
    r.x = fe_reduce(fe_neg(p.x));
    r.y = p.y;
    r.t = fe_reduce(fe_neg(p.t));
    r.z = p.z;
    return r;
}
// Is (x, y) -- plain 9-word coordinates -- a point of a*x^2 + y^2 = 1 + d*x^2*y^2 with both coordinates < t (edwards.ts:52-65, 74-77: what
// deserialising a point checks)?  Validation only needs the verdict, so the coordinates are NOT taken to the Montgomery domain: every Montgomery
// product of plain operands divides by R once, u = x^2/R, v = y^2/R, w = u*v/R = x^2 y^2/R^3, and the equation is compared scaled by 1/R:
// u * (aR)/R + v  ==  w * (dR^3)/R + 1/R.  Five products instead of the seven of tom_from_affine_words (the verifier's validation pass
// runs it on ~1 600 points per proof).
ZK_DEV bool tom_words_on_curve(const uint32_t xw[9], const uint32_t yw[9]) {
    if (words_geq<9>(xw, ModT::mod32) || words_geq<9>(yw, ModT::mod32)) return false;
    const auto x = fe_from_words<ModT, 9>(xw), y = fe_from_words<ModT, 9>(yw);
    const auto u = x * x, v = y * y;
    const auto lhs = u * fe_const<ModT, 1>(TOM_A_M) + v;
    const auto rhs = (u * v) * fe_const<ModT, 1>(TOM_D_R3) + fe_const<ModT, 1>(TOM_RINV);
    return fe_eq(lhs, rhs);
}
// original-curve affine (plain 9-word x, y) -> a=1 image, extended Montgomery.  Returns false if a coordinate is
// >= t (edwards.ts:74-77) or the point is off the curve a*x^2 + y^2 = 1 + d*x^2*y^2 (edwards.ts:52-65).
ZK_DEV bool tom_from_affine_words(TomPt& r, const uint32_t xw[9], const uint32_t yw[9]) {
    if (words_geq<9>(xw, ModT::mod32) || words_geq<9>(yw, ModT::mod32)) return false;
    auto x = fe_to_mont(fe_from_words<ModT, 9>(xw));
    auto y = fe_to_mont(fe_from_words<ModT, 9>(yw));
    auto x2 = x * x, y2 = y * y;
    auto lhs = fe_const<ModT, 1>(TOM_A_M) * x2 + y2;
    auto rhs = fe_const<ModT, 1>(TOM_D_M) * (x2 * y2) + fe_one_mont<ModT>();
    bool ok = fe_eq(lhs, rhs);
    r.x = x * fe_const<ModT, 1>(TOM_S_M);
    r.y = y;
    r.t = r.x * r.y;
    r.z = fe_one_mont<ModT>().as<2>();
    return ok;
}

// ---------------------------------------------------------------- Tom-256 on the a = -1 model: the fixed-base comb tables of g and h ONLY
// (x', y) on the a = 1 image  ->  (x'', y') = (s2 * x', 1 / y), s2^2 = -d/a:  -x''^2 + y'^2 = 1 + d2 x''^2 y'^2, d2 = -a/d.  A group isomorphism away from
// the two points with y = 0 (order 4); it fixes the identity.  On this model E = X1 y2 + Y1 x2 and H = Y1 y2 + X1 x2 come out of (Y1 - X1)(y2 - x2) and
// (Y1 + X1)(y2 + x2) alone ("madd-2008-hwcd-3"), so the addition of a table entry costs 7 products instead of 8.  -1 is a non-square and d2 a square mod t
// (tools/gen_consts.py), so the law is complete only on points of ODD order: the exceptional pairs differ by a point of even order.  Multiples of bases
// with q * g = q * h = identity (checked when the parameters are set, api.hip) never form such a pair; every sum over points taken from a proof stays
// on the a = 1 law above.  The LAST step of a sum maps back -- x' = X3 / (s2 Z3), y = Z3 / Y3, i.e. the triple (E H / s2 : F G : G H) -- so the
// normaliser and everything behind it see the a = 1 image as before.
struct TomM1Pt {  // extended (X:Y:T:Z); the bounds are those of the first step of a sum (tom_m1_from_niels), every addition returns coordinates < 2t
    Fe<ModT, 12> x;
    Fe<ModT, 8> y;
    Ft2 t, z;
};
template <int KT>
struct TomM1NielsT {  // y' - x'', y' + x'', 2 d2 x'' y'; the identity entry is (1, 1, 0)
    Ft2 ym, yp;
    Fe<ModT, KT> t2;
};
// a loaded table entry (three field elements, in the slots of a TomNiels) as it is used; neg: -P swaps the first two and negates the third
ZK_DEV TomM1NielsT<2> tom_m1_niels(const TomNiels& q) {
    TomM1NielsT<2> r;
    r.ym = q.x, r.yp = q.y, r.t2 = q.dt;
    return r;
}
ZK_DEV TomM1NielsT<4> tom_m1_niels_neg_sel(const TomNiels& q, bool neg) {
    TomM1NielsT<4> r;
    r.ym = fe_select(neg, q.y, q.x);
    r.yp = fe_select(neg, q.x, q.y);
#pragma unroll
    for (int i = 0; i < NLIMB; i++) r.t2.l[i] = neg ? ModT::sub4[i] - q.dt.l[i] : q.dt.l[i];
    limbs_normalize(r.t2.l);
    return r;
}
ZK_DEV TomM1Pt tom_m1_identity() {
    TomM1Pt r;
    r.x = fe_zero<ModT>().as<12>();
    r.y = fe_one_mont<ModT>().as<8>();
    r.t = fe_zero<ModT>().as<2>();
    r.z = fe_one_mont<ModT>().as<2>();
    return r;
}
// E F, G H, E H, F G
template <int KE, int KF, int KG, int KH>
ZK_DEV TomM1Pt tom_m1_finish(const Fe<ModT, KE>& E, const Fe<ModT, KF>& F, const Fe<ModT, KG>& G, const Fe<ModT, KH>& H) {
    Ft2 x, y;
    TomM1Pt r;
    fe_mul4<ZK_BATCH_TOM != 0>(x, y, r.t, r.z, E, F, G, H, E, H, F, G);
    r.x = x.as<12>(), r.y = y.as<8>();
    return r;
}
// the sum is final: x, y, z of the result hold the a = 1 image's projective triple (E H / s2 : F G : G H), t is zero
template <int KE, int KF, int KG, int KH>
ZK_DEV TomM1Pt tom_m1_finish_last(const Fe<ModT, KE>& E, const Fe<ModT, KF>& F, const Fe<ModT, KG>& G, const Fe<ModT, KH>& H) {
    Ft2 eh, y;
    TomM1Pt r;
    fe_mul3<ZK_BATCH_TOM != 0>(eh, y, r.z, E, H, F, G, G, H);
    r.x = (eh * fe_const<ModT, 1>(TOM_M1_SINV_M)).as<12>();
    r.y = y.as<8>();
    r.t = fe_zero<ModT>().as<2>();
    return r;
}
// mixed addition of a table entry: 3 + 4 lock-step products
template <bool LAST, int KT>
ZK_DEV TomM1Pt tom_m1_add_niels_t(const TomM1Pt& p, const TomM1NielsT<KT>& q) {
    Ft2 A, B, C;
    fe_mul3<ZK_BATCH_TOM != 0>(A, B, C, p.y - p.x, q.ym, p.y + p.x, q.yp, p.t, q.t2);
    auto D = p.z + p.z;
    auto E = B - A;
    auto F = D - C;
    auto G = D + C;
    auto H = B + A;
    if constexpr (LAST) return tom_m1_finish_last(E, F, G, H);
    else return tom_m1_finish(E, F, G, H);
}
template <int KT>
ZK_DEV TomM1Pt tom_m1_add_niels(const TomM1Pt& p, const TomM1NielsT<KT>& q) { return tom_m1_add_niels_t<false>(p, q); }
template <int KT>
ZK_DEV TomM1Pt tom_m1_add_niels_last(const TomM1Pt& p, const TomM1NielsT<KT>& q) { return tom_m1_add_niels_t<true>(p, q); }
// identity + q, scaled by 4: X = 2 (yp - ym), Y = 2 (yp + ym), T = (yp - ym)(yp + ym), Z = 4: 1 product
template <int KT>
ZK_DEV TomM1Pt tom_m1_from_niels(const TomM1NielsT<KT>& q) {
    auto dm = q.yp - q.ym;
    auto dp = q.yp + q.ym;
    TomM1Pt r;
    r.x = dm + dm;
    r.y = dp + dp;
    r.t = dm * dp;
    r.z = fe_const<ModT, 1>(TOM_FOUR_M).as<2>();
    return r;
}
// general addition of two extended points (partial sums of the wide kernel): 8 products and one by 2 d2
template <bool LAST>
ZK_DEV TomM1Pt tom_m1_add_t(const TomM1Pt& p, const TomM1Pt& q) {
    Ft2 A, B, C0, D0;
    fe_mul4<ZK_BATCH_TOM != 0>(A, B, C0, D0, p.y - p.x, q.y - q.x, p.y + p.x, q.y + q.x, p.t, q.t, p.z, q.z);
    Ft2 C = C0 * fe_const<ModT, 1>(TOM_M1_2D2_M);
    auto D = D0 + D0;
    auto E = B - A;
    auto F = D - C;
    auto G = D + C;
    auto H = B + A;
    if constexpr (LAST) return tom_m1_finish_last(E, F, G, H);
    else return tom_m1_finish(E, F, G, H);
}

// The two models behind one interface: the comb kernels (k_tom.hip) and the table builder (k_tables.hip) are templates over MODEL.
//   Pt: accumulator;  entry / entry_neg: a loaded table entry as used (signed combs negate it on load);  first: identity + entry;  add: + entry;
//   add_last: + entry where the sum is final: x, y, z of the result are the a = 1 image's projective triple (what the lists and the normaliser take);
//   add_pts / add_pts_last: the same for two accumulators.
#define TOM_MODEL_A1 0
#define TOM_MODEL_M1 1
template <int MODEL>
struct TomModel;
template <>
struct TomModel<TOM_MODEL_A1> {
    typedef TomPt Pt;
    static ZK_DEV Pt identity() { return tom_identity(); }
    static ZK_DEV TomNiels entry(const TomNiels& q) { return q; }
    static ZK_DEV TomNielsT<4> entry_neg(const TomNiels& q, bool neg) { return tom_niels_neg_sel(q, neg); }
    template <class E>
    static ZK_DEV Pt first(const E& e) { return tom_from_niels(e); }
    template <class E>
    static ZK_DEV Pt add(const Pt& p, const E& e) { return tom_add_niels(p, e); }
    template <class E>
    static ZK_DEV Pt add_last(const Pt& p, const E& e) { return tom_add_niels_last(p, e); }
    static ZK_DEV Pt add_pts(const Pt& p, const Pt& q) { return tom_add(p, q); }
    static ZK_DEV Pt add_pts_last(const Pt& p, const Pt& q) { return tom_add(p, q); }
};
template <>
struct TomModel<TOM_MODEL_M1> {
    typedef TomM1Pt Pt;
    static ZK_DEV Pt identity() { return tom_m1_identity(); }
    static ZK_DEV TomM1NielsT<2> entry(const TomNiels& q) { return tom_m1_niels(q); }
    static ZK_DEV TomM1NielsT<4> entry_neg(const TomNiels& q, bool neg) { return tom_m1_niels_neg_sel(q, neg); }
    template <class E>
    static ZK_DEV Pt first(const E& e) { return tom_m1_from_niels(e); }
    template <class E>
    static ZK_DEV Pt add(const Pt& p, const E& e) { return tom_m1_add_niels(p, e); }
    template <class E>
    static ZK_DEV Pt add_last(const Pt& p, const E& e) { return tom_m1_add_niels_last(p, e); }
    static ZK_DEV Pt add_pts(const Pt& p, const Pt& q) { return tom_m1_add_t<false>(p, q); }
    static ZK_DEV Pt add_pts_last(const Pt& p, const Pt& q) { return tom_m1_add_t<true>(p, q); }
};
