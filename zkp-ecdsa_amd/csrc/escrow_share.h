// Threshold opening of escrow tags (include/zkattest.h: zk_auditors_*, zk_ctx_set_auditors): t of n auditors, each with a Shamir share a_j of the auditor
// secret a, open a ZKT1 tag together.  A share "ZKS1" is auditor j's partial opening D = a_j E1 with a Chaum-Pedersen proof that D was made with the secret
// behind A_j = a_j g; t of them combine to 4 (E2 - sum lambda_j D_j), the point zk_rings_escrow_open_batch looks up.  The "ZKS1" layout and the arithmetic
// the engine did not have: the Lagrange coefficients mod q and the joint ladder sum lambda_j D_j.  Device functions that also compile for the host CPU under
// ZK_HOST_BUILD (tests/host_arith/host_escrow_share.cpp).
#pragma once
#include "escrow.h"
#include "distinct.h"

// "ZKS1": 16 header bytes ("ZKS1" | total_len = 264 | j | 0), D, U1, U2 (72 bytes each), s (32 bytes)
#define ZKS1_HDR 16
#define ZKS1_SIZE 264
#define ZKS1_WORDS (ZKS1_SIZE / 4)
#define ZK_MAGIC_ZKS1 0x31534b5au
#define ZKS1_PT(k) (ZKS1_HDR + 72 * (k))   // 0..2: D, U1, U2
#define ZKS1_S (ZKS1_HDR + 216)
#define ZKS1_MSG_POINTS 5   // hashPoints([A_j, E1, D, U1, U2]): 5 x 67 = 335 bytes ...
#define ZKS1_MSG_BLOCKS 6   // ... and SHA-256's padding
#define ZK_AUDITORS_MAX 16

// The response, plain canonical: s = k - c a_j mod q
ZK_DEV Fe<ModQ, 1> share_respond(const Fe<ModQ, 1>& k, const uint32_t c3[3], const Fe<ModQ, 1>& aj) { return link_respond(k, c3, aj); }
ZK_DEV Fe<ModQ, 1> share_small(uint32_t v) {   // an index as a scalar
    const uint32_t w[8] = {v, 0, 0, 0, 0, 0, 0, 0};
    Fe<ModQ, 1> r;
    limbs_from_words<8>(r.l, w);
    return r;
}
// The Lagrange coefficient of idx[s] among the t different indices idx[0 .. t-1] for the value at `at`: prod_{m != s} (idx[m] - at) / (idx[m] - idx[s]) mod q,
// plain canonical.  at = 0 gives the lambda of a combine; zk_ctx_set_auditors also asks for at = m > t.  Indices are public.
ZK_DEV Fe<ModQ, 1> share_lagrange(const uint32_t* idx, uint32_t t, uint32_t s, uint32_t at) {
    Fe<ModQ, 1> num = share_small(1), den = share_small(1);
    const Fe<ModQ, 1> js = share_small(idx[s]), x0 = share_small(at);
    for (uint32_t m = 0; m < t; m++) {
        if (m == s) continue;
        const Fe<ModQ, 1> im = share_small(idx[m]);
        num = fe_mul_mod(num, fe_sub_mod(im, x0)), den = fe_mul_mod(den, fe_sub_mod(im, js));
    }
    return fe_mul_mod(num, dist_inverse(den));
}
// Horner's rule at the point j: coef[0] + coef[1] j + ... + coef[t-1] j^(t-1) mod q, all plain canonical (the dealer's shares).
// coef(i) hands out coefficient i: the kernel draws it where it is needed instead of keeping an array.
template <class Coef>
ZK_DEV Fe<ModQ, 1> share_eval(Coef coef, uint32_t t, uint32_t j) {
    const Fe<ModQ, 1> x = share_small(j);
    Fe<ModQ, 1> v = coef(t - 1);
    for (uint32_t i = t - 1; i > 0; i--) v = fe_add_mod(fe_mul_mod(v, x), coef(i - 1));
    return v;
}

// ------------------------------------------------------------------ sum_s lambda_s D_s for t points out of shares
// A lane's t addends (x, y, d' x y) with Z = 1 lie in memory the caller owns, 27 words each, word w of addend s at p[(27 s + w) * stride]: held in registers
// they would be a table indexed at run time.  `stride` is the lanes' count, so that the lanes of a wave read neighbouring words.
struct ShareTab {
    uint32_t* p;
    size_t stride;
};
ZK_DEV void share_tab_put(const ShareTab& T, uint32_t s, const TomPt& d) {
    const TomNiels e = link_niels(d);
    uint32_t* q = T.p + 27 * (size_t)s * T.stride;
#pragma unroll
    for (int l = 0; l < NLIMB; l++) q[l * T.stride] = e.x.l[l], q[(9 + l) * T.stride] = e.y.l[l], q[(18 + l) * T.stride] = e.dt.l[l];
}
ZK_DEV TomNiels share_tab_get(const ShareTab& T, uint32_t s) {
    TomNiels e;
    const uint32_t* q = T.p + 27 * (size_t)s * T.stride;
#pragma unroll
    for (int l = 0; l < NLIMB; l++) e.x.l[l] = q[l * T.stride], e.y.l[l] = q[(9 + l) * T.stride], e.dt.l[l] = q[(18 + l) * T.stride];
    return e;
}
// One joint ladder, left to right over the 256 bits of every coefficient (lam: t x eight little-endian words): one doubling per bit, shared by the t terms,
// and one mixed addition per set bit of a coefficient -- 256 doublings and about 128 t additions.  It branches on the bits: the coefficients are public,
// and where every lane of a wave reads the same `lam` the branches are wave-uniform.  A D may carry a component of order 2 or 4 and partial sums may pass
// through the identity: everything stays on the a = 1 law, which is complete, and starts from the identity.
ZK_DEV TomPt share_joint_ladder(const ShareTab& T, const uint32_t* lam, uint32_t t) {
    TomPt acc = tom_identity();
#pragma unroll 1
    for (int w = 7; w >= 0; w--) {
#pragma unroll 1
        for (int i = 31; i >= 0; i--) {
            acc = tom_dbl(acc);
#pragma unroll 1
            for (uint32_t s = 0; s < t; s++)
                if ((lam[8 * s + w] >> i) & 1) acc = tom_add_niels(acc, share_tab_get(T, s));
        }
    }
    return acc;
}
// What t shares open a tag to: 4 (E2 - sum lambda_j D_j); the factor 4 for the reason it is in escrow_open_point
ZK_DEV TomPt share_combine_point(const TomPt& e2, const TomPt& sum) { return tom_dbl(tom_dbl(tom_add(e2, tom_neg(sum)))); }

#if !defined(ZK_HOST_BUILD)
// ------------------------------------------------------------------ a lane's arena (api_escrow_share.hip carves it, k_escrow_share.hip's kernels read it); C = tags per chunk
// The list's slots for a chunk of `count` tags.  Share: p = U1 (k, 0) on the (g, h) combs; count + p = D, 2 count + p = U2, projective from the ladder.
// Verifier: p = (s, 0) on the combs.
#define SHR_SLOTS 3
struct ShareLane : SigmaLane {   // L [SHR_SLOTS C], one draw, ZKS1_MSG_BLOCKS message blocks
    uint32_t* kw;         // [C][8] share: k as words (the masked ladder reads them); verifier: s reduced (dist_ladder2 reads them)
    DistQuad* tab;       // [C][DIST_TAB_QUADS] verifier: the addends of relation 2's chain
    uint32_t* rel;        // [C][2] verifier: the two relations as their lanes found them
};
#define SHR_RNG_BLOCKS (1 + RNG_MAX_EXC)
#define SPLIT_RNG_BLOCKS (ZK_AUDITORS_MAX - 1 + RNG_MAX_EXC)
struct ShareProveIo {     // device pointers of a share call, indexed by the tag's place in the batch
    const uint8_t* tags;
    uint8_t* out;
    int32_t* status;
};
struct ShareVerifyIo {
    const uint8_t *tags, *shares;
    uint8_t* ok;
    int32_t* status;
};
struct ShareSecret {      // the call's share secret, staged once: a_j mod q as words and the index j
    const uint32_t* a8;
    uint32_t j;
};
struct ShareCombineIo {   // a combine call: slot s of `shares` (B shares) belongs to auditors[s]
    const uint8_t *tags, *shares;
    const uint32_t* auditors;   // [t] on the device
    uint64_t B;
    uint32_t t;
};
void launch_share_front(hipStream_t s, const ShareLane& K, uint32_t count, uint64_t first, const ShareProveIo& io);
void launch_share_ladder(hipStream_t s, const ShareLane& K, const ShareSecret& A, uint32_t count, uint64_t first, const ShareProveIo& io);
void launch_share_msg(hipStream_t s, const ShareLane& K, const uint32_t* keys_w /*[n][18]*/, uint32_t j, uint32_t count, uint64_t first, const ShareProveIo& io);
void launch_share_respond(hipStream_t s, const ShareLane& K, const ShareSecret& A, uint32_t count, uint64_t first, const ShareProveIo& io);
void launch_share_parse(hipStream_t s, const ShareLane& K, const uint32_t* keys_w, uint32_t n, uint32_t count, uint64_t first, const ShareVerifyIo& io);
void launch_share_relations(hipStream_t s, const ShareLane& K, const uint32_t* keys_w, uint32_t count, uint64_t first, const ShareVerifyIo& io);
void launch_share_verdict(hipStream_t s, const ShareLane& K, uint32_t count, uint64_t first, const ShareVerifyIo& io);
// lam[i][s][8]: the coefficient of idx[s] for the value at at[i], i < evals (one thread each)
void launch_share_lagrange(hipStream_t s, const uint32_t* idx, uint32_t t, const uint32_t* at, uint32_t evals, uint32_t* lam);
// One lane per tag: the tag's and the t shares' headers, E1, E2 and every D; the joint ladder over tab; 4 (E2 - sum) as the projective triple b of O.T
void launch_share_combine(hipStream_t s, const EscrowOpen& O, const ShareCombineIo& io, const uint32_t* lam, uint32_t* tab, uint32_t count, uint64_t first, uint32_t* index,
                          int32_t* status);
// zk_ctx_set_auditors: lane i < evals walks sum_s lam[i][s] key[s] over the first t keys (72 bytes each) into the projective triple i of L
void launch_share_interpolate(hipStream_t s, const uint8_t* keys72, uint32_t t, const uint32_t* lam, uint32_t evals, uint32_t* tab, const TomList& L);
// zk_auditors_split_key: the secret reduced and the t - 1 draws of "proof" 0 as f's coefficients; a_j = f(j) as the opening (a_j, 0) of slot j - 1 and as 32
// big-endian bytes; flag[0] = 1 where the RNG does not hold the draws
void launch_share_split(hipStream_t s, const RngCtx& rng, const uint8_t* secret, uint32_t t, uint32_t n, const TomList& L, uint8_t* shares_be32, uint32_t* flag);
// api_escrow.hip: what the combine shares with the single-auditor opening
struct zk_ctx;
struct Ring;
void escrow_secret_point(zk_ctx* c, hipStream_t s, const uint8_t* d_secret, const TomList& S, uint32_t* a8, uint8_t* d_ag);
size_t escrow_open_carve(EscrowOpen& O, uint8_t* base, uint64_t B, uint32_t slab);
EscIndexRing escrow_index_desc(const Ring& R, uint64_t nkeys);
zk_status escrow_index_build(zk_ctx* c, Ring& R);
#endif
