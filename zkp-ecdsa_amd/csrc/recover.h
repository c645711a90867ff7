// Key recovery from a signature (include/zkattest.h: zk_recover_batch; kernels: k_recover.hip): the three steps that are arithmetic and nothing else, on the
// field and curve headers only, so that tests/host_arith/host_recover.cpp compiles them for the host.
//   rec_candidate_x, rec_lift_x   the candidate nonce point of a pass: x = r (pass 0) or r + n (pass 1, only where r + n < p), y the EVEN root of x^3 - 3x + b
//   rec_tail     A = u1 G, Bp = u2 R -> Q0 = A + Bp (R's even root), Q1 = A - Bp (the odd one), canonical affine through ONE shared inversion; an identity is marked
//   rec_select   the winner among up to four looked-up candidates: lowest ring index, ties to the lowest candidate number
#pragma once
#include "curve.h"

#define REC_NCAND 4
#define REC_NONE 0xFFFFFFFFu   // (ZK_WHICH_NONE: this header does not see zkattest.h in the host build)

// x of pass `pass` as a canonical field element; false where the pass has no x-candidate (r + n >= p).  rw: r in [1, n) as 8 little-endian words.
ZK_DEV bool rec_candidate_x(const uint32_t rw[8], uint32_t pass, Fe<ModQ, 1>& x) {
    uint32_t xw[8];
    uint64_t carry = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t v = (uint64_t)rw[i] + (pass ? ModN::mod32[i] : 0u) + carry;
        xw[i] = (uint32_t)v, carry = v >> 32;
    }
    limbs_from_words<8>(x.l, xw);
    return !carry && !words_geq<8>(xw, ModQ::mod32);
}
// The lift in three steps, so that the square root in the middle can run in one lane (fe_pow_words) or on a cooperating wave (coop.h: co_pow_words):
// v = x^3 - 3x + b in Montgomery form, reduced ...
ZK_DEV Fq2 rec_lift_v(const Fe<ModQ, 1>& xp) {
    const auto b = fe_const<ModQ, 1>(P256_B_M);
    const Fq2 x = fe_to_mont(xp);
    const auto x2 = x * x;
    const auto x3 = x2 * x;
    return fe_reduce((x3 + b) - (x + x + x));
}
// ... y = v^((p + 1) / 4), a root exactly where v is a square ...
ZK_DEV Fq2 rec_lift_root(const Fq2& v) { return fe_pow_words<ModQ>(v, ModQ::exp_sqrt); }
// ... and the point (x, even y) in Montgomery form; false where y^2 != v: x^3 - 3x + b is no square mod p
ZK_DEV bool rec_lift_point(const Fe<ModQ, 1>& xp, const Fq2& v, const Fq2& y, P256Aff& R) {
    if (!fe_eq(y * y, v)) return false;
    const Fe<ModQ, 1> yp = fe_from_mont(y);
    const Fe<ModQ, 1> ye = (yp.l[0] & 1u) ? fe_sub_mod(fe_zero<ModQ>(), yp) : yp;   // p is odd: exactly one of y, p - y is even (y = 0 is its own negative)
    R.x = fe_to_mont(xp), R.y = fe_to_mont(ye);
    return true;
}
// the three in one lane
ZK_DEV bool rec_lift_x(const Fe<ModQ, 1>& xp, P256Aff& R) {
    const Fq2 v = rec_lift_v(xp);
    return rec_lift_point(xp, v, rec_lift_root(v), R);
}

struct RecPair {
    Fe<ModQ, 1> x[2], y[2];   // canonical plain affine coordinates of Q0 = A + Bp and Q1 = A - Bp; (0, 0) for an identity
    bool ident[2];
};
// One inversion for both: 1 / (Z0 Z1), with a zero Z replaced by one so that an identity does not take its sibling with it.  LOCKSTEP: field.h, fe_inv_gcd.
template <bool LOCKSTEP>
ZK_DEV void rec_pair_affine(const P256Pt& Q0, const P256Pt& Q1, RecPair& o) {
    Fq2 z0 = fe_reduce(Q0.z), z1 = fe_reduce(Q1.z);
    o.ident[0] = fe_is_zero(z0), o.ident[1] = fe_is_zero(z1);
    z0 = fe_select(o.ident[0], fe_one_mont<ModQ>().template as<2>(), z0);
    z1 = fe_select(o.ident[1], fe_one_mont<ModQ>().template as<2>(), z1);
    Fe<ModQ, 1> one = fe_zero<ModQ>();
    one.l[0] = 1;
    const Fq2 inv = fe_inv<ModQ, LOCKSTEP>(z0 * z1) * one;   // plain domain from here: the affine coordinates come out plain (k_p256_normalize)
    const Fq2 i0 = inv * z1, i1 = inv * z0;
    o.x[0] = fe_canon(Q0.x * i0), o.y[0] = fe_canon(Q0.y * i0);
    o.x[1] = fe_canon(Q1.x * i1), o.y[1] = fe_canon(Q1.y * i1);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        o.x[k] = fe_select(o.ident[k], fe_zero<ModQ>(), o.x[k]);
        o.y[k] = fe_select(o.ident[k], fe_zero<ModQ>(), o.y[k]);
    }
}
template <bool LOCKSTEP>
ZK_DEV void rec_tail(const P256Pt& A, const P256Pt& Bp, RecPair& o) {
    P256Pt nB = Bp;
    nB.y = fe_neg(fe_reduce(Bp.y)).template as<8>();
    rec_pair_affine<LOCKSTEP>(p256_add(A, Bp), p256_add(A, nB), o);   // the complete law: A = +-Bp, A = identity, Bp = identity need no case of their own
}

// idx[c]: the lowest ring index of candidate c's x, REC_NONE where the candidate does not exist or is not in the ring.  Returns the winning c, or REC_NCAND.
ZK_DEV uint32_t rec_select(const uint32_t idx[REC_NCAND]) {
    uint32_t best = REC_NONE, win = REC_NCAND;
#pragma unroll
    for (uint32_t c = 0; c < REC_NCAND; c++)
        if (idx[c] < best) best = idx[c], win = c;   // strictly lower: a tie stays with the lower c
    return win;
}
