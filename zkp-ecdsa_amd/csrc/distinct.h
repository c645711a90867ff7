// Distinct-key proofs (include/zkattest.h: zk_distinct_*): "two Tom-256 commitments hide DIFFERENT keys" as one MultProof (mult.ts:93-175) over
// Cx = C1 - C2, Cy = commit(1 / (x1 - x2)), Cz = g.  The "ZKD1" layout and the arithmetic the engine did not have -- relation 5 of aggregateMult,
// t_x Cy + c C_4 - A_4_2 = O, which multiplies a point out of a proof by a full 256-bit scalar -- plus the seven responses of proveMult, which the
// PointAdd respond kernel (k_scalar.hip: mult_respond) takes from here too.  Device functions that also compile for the host CPU under ZK_HOST_BUILD
// (tests/host_arith/host_distinct.cpp).
#pragma once
#include "link.h"

// "ZKD1": 16 header bytes ("ZKD1" | total_len = 744 | 0 | 0), C_w (72 bytes), then a MultProof as it lies inside ZKA1: C_4, A_x, A_y, A_z, A_4_1, A_4_2
// (72 bytes each), t_x, t_y, t_z, t_rx, t_ry, t_rz, t_r4 (32 bytes each)
#define ZKD1_HDR 16
#define ZKD1_SIZE 744
#define ZKD1_WORDS (ZKD1_SIZE / 4)
#define ZK_MAGIC_ZKD1 0x31444b5au
#define ZKD1_CW ZKD1_HDR
#define ZKD1_PT(k) (ZKD1_HDR + 72 + 72 * (k))   // 0..5: C_4, A_x, A_y, A_z, A_4_1, A_4_2
#define ZKD1_SC(k) (ZKD1_HDR + 72 + 432 + 32 * (k))   // 0..6: t_x, t_y, t_z, t_rx, t_ry, t_rz, t_r4
#define ZKD1_MSG_POINTS 9    // hashPoints([Cx, Cy, Cz, C_4, A_x, A_y, A_z, A_4_1, A_4_2]): 9 x 67 = 603 bytes ...
#define ZKD1_MSG_BLOCKS 10   // ... and SHA-256's padding

// The seven responses of proveMult (mult.ts:122-130), all plain canonical: t[i] = k[i] - c v_i mod q over v = (x, y, z, r_x, r_y, r_z, r_4 = x r_y) with
// k = (k_x, k_y, k_z, s_x, s_y, s_z, s_4), the nonces and the blinders of A_x, A_y, A_z, A_4_1.
ZK_DEV void mult_responses(Fe<ModQ, 1> t[7], const uint32_t* c3, const Fe<ModQ, 1> k[7], const Fe<ModQ, 1>& x, const Fe<ModQ, 1>& y, const Fe<ModQ, 1>& z,
                           const Fe<ModQ, 1>& rx, const Fe<ModQ, 1>& ry, const Fe<ModQ, 1>& rz) {
    const uint32_t w[8] = {c3[0], c3[1], c3[2], 0, 0, 0, 0, 0};
    Fe<ModQ, 1> c;
    limbs_from_words<8>(c.l, w);
    const auto cm = fe_to_mont(c);
    const Fe<ModQ, 1> r4 = fe_mul_mod(x, ry);
    t[0] = fe_sub_mod(k[0], fe_canon(cm * x));
    t[1] = fe_sub_mod(k[1], fe_canon(cm * y));
    t[2] = fe_sub_mod(k[2], fe_canon(cm * z));
    t[3] = fe_sub_mod(k[3], fe_canon(cm * rx));
    t[4] = fe_sub_mod(k[4], fe_canon(cm * ry));
    t[5] = fe_sub_mod(k[5], fe_canon(cm * rz));
    t[6] = fe_sub_mod(k[6], fe_canon(cm * r4));
}
// 1 / d mod q, plain canonical in and out; 0 for d = 0 (fe_inv's rule).  The rounds of fe_inv are fixed in the uniform build: d is a witness.
ZK_DEV Fe<ModQ, 1> dist_inverse(const Fe<ModQ, 1>& d) {
    Fe<ModQ, 1> one = fe_zero<ModQ>();
    one.l[0] = 1;
    return fe_canon(fe_inv<ModQ>(fe_to_mont(d)) * one);   // a Montgomery product with the plain 1 leaves the Montgomery domain
}
// Cx = C1 - C2, one complete addition: the identity for C1 = C2, which is a legal point here
ZK_DEV TomPt dist_sub(const TomPt& c1, const TomPt& c2) { return tom_add(c1, tom_neg(c2)); }

// ------------------------------------------------------------------ t * Cy + c * C4 for a 256-bit t and the 80-bit challenge
// The three addends Cy, C4 and Cy + C4 as the addition takes them, (X, Y, d' T, Z), 36 words each: they lie in memory the caller owns, one 16-byte aligned
// area of DIST_TAB_QUADS quads per chain, and the chain reads the one its two bits select.  Held in registers they would be a table indexed at run time.
struct alignas(16) DistQuad {
    uint32_t w[4];
};
#define DIST_TAB_QUADS 27
ZK_DEV void dist_tab_put(DistQuad* tab, int k, const TomPt& p) {
    const Ft2 dt = p.t * fe_const<ModT, 1>(TOM_D1_M);
    uint32_t w[36];
#pragma unroll
    for (int l = 0; l < NLIMB; l++) w[l] = p.x.l[l], w[9 + l] = p.y.l[l], w[18 + l] = dt.l[l], w[27 + l] = p.z.l[l];
#pragma unroll
    for (int i = 0; i < 9; i++) tab[9 * k + i] = DistQuad{{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]}};
}
ZK_DEV TomPt dist_tab_add(const TomPt& acc, const DistQuad* tab, uint32_t k) {
    uint32_t w[36];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const DistQuad q = tab[9 * k + i];
        w[4 * i] = q.w[0], w[4 * i + 1] = q.w[1], w[4 * i + 2] = q.w[2], w[4 * i + 3] = q.w[3];
    }
    Ft2 x, y, dt, z;
#pragma unroll
    for (int l = 0; l < NLIMB; l++) x.l[l] = w[l], y.l[l] = w[9 + l], dt.l[l] = w[18 + l], z.l[l] = w[27 + l];
    return tom_add_tab(acc, x, y, dt, z);
}
// Left to right over the 256 bits of t (t8: eight little-endian words) and, in the low 80, of c: one doubling per bit and one addition wherever either
// scalar has a set bit -- 256 doublings, about 130 to 260 additions.  It branches on the bits: both scalars are public (a response of the proof, the
// verifier's hash).  t8 and c3 are read one word at a time, so they too should lie in memory.  The bases come out of a proof, nobody has checked their
// order and Cy + C4 may be the identity: everything stays on the a = 1 law, which is complete, and starts from the identity like any other point.
ZK_DEV TomPt dist_ladder2(const TomPt& cy, const uint32_t* t8, const TomPt& c4, const uint32_t* c3, DistQuad* tab) {
    dist_tab_put(tab, 0, cy), dist_tab_put(tab, 1, c4), dist_tab_put(tab, 2, tom_add(cy, c4));
    TomPt acc = tom_identity();
#pragma unroll 1
    for (int w = 7; w >= 0; w--) {
        uint32_t tw = t8[w], cw = w > 2 ? 0 : w == 2 ? c3[2] & 0xffffu : c3[w];
#pragma unroll 1
        for (int i = 0; i < 32; i++) {
            acc = tom_dbl(acc);
            const uint32_t sel = (tw >> 31) | ((cw >> 31) << 1);
            if (sel) acc = dist_tab_add(acc, tab, sel - 1);
            tw <<= 1, cw <<= 1;
        }
    }
    return acc;
}
// Relation 5 of aggregateMult (mult.ts:166-170), exactly: t_x Cy + c C_4 - A_4_2 = O
ZK_DEV bool dist_relation5(const TomPt& cy, const uint32_t* t8, const TomPt& c4, const uint32_t* c3, const TomPt& a42, DistQuad* tab) {
    return link_is_identity(tom_add(dist_ladder2(cy, t8, c4, c3, tab), tom_neg(a42)));
}
// Relation 3, whose base is g: the parser's successor folds c into the comb opening, so what is left is ((t_z + c) g + t_rz h) - A_z = O
ZK_DEV bool dist_relation3(const TomPt& D, const TomPt& az) { return link_is_identity(tom_add(D, tom_neg(az))); }

#if !defined(ZK_HOST_BUILD)
// ------------------------------------------------------------------ a lane's arena (api_distinct.hip carves it, k_distinct.hip's kernels read it); C = proofs per chunk
// The list's slots for a chunk of `count` proofs.
// Prover: 2 p, 2 p + 1 = (A_z, A_4_1) of proof p (k_z under s_z, s_4: the pair form); 2 count + 7 p + k = C_w (w, r_w), C_4 (1, d r_w), A_x (k_x, s_x),
// A_y (k_y, s_y), A_4_2 (k_x w, k_x r_w), the two openings the caller claims (x1, r1), (x2, r2); 9 count + p = Cx = C1 - C2, projective from the front end.
// Verifier: 4 p + k = (t_x, t_rx), (t_y, t_ry), (t_z + c, t_rz), (t_z, t_r4); 4 count + p = Cx.
#define DIST_SLOTS 10
#define DIST_SINGLES 7
struct DistLane : SigmaLane {   // L [DIST_SLOTS C], eight draws, ZKD1_MSG_BLOCKS message blocks
    uint32_t* cw;         // [C][36] com1 (x, y), com2 (x, y) as the caller states them, nine little-endian words each
    uint32_t* tw;        // [C][8] verifier: t_x reduced, as words (dist_ladder2 reads them from memory)
    DistQuad* tab;        // [C][DIST_TAB_QUADS] verifier: the addends of relation 5's chain
    uint32_t* rel;        // [C][3] verifier: relations 1, 2 and 4 as the short ladders found them
};
#define DIST_RNG_BLOCKS (8 + RNG_MAX_EXC)   // r_w, k_x, k_y, k_z, s_x, s_y, s_z, s_4 and a margin: rejected fills shift later draws
struct DistProveIo {      // device pointers of a prove call, indexed by the proof's place in the batch
    const uint8_t *key1, *com1, *blinder1, *key2, *com2, *blinder2;
    uint8_t* out;
    int32_t* status;
};
typedef LinkVerifyIo DistVerifyIo;   // com1, com2, proofs, ok, status
void launch_dist_front(hipStream_t s, const DistLane& K, uint32_t count, uint64_t first, const DistProveIo& io);
void launch_dist_opening_msg(hipStream_t s, const DevParams& P, const DistLane& K, uint32_t count);   // behind the normaliser: the opening compare, the challenge's message
void launch_dist_respond(hipStream_t s, const DistLane& K, uint32_t count, uint64_t first, const DistProveIo& io);
void launch_dist_parse(hipStream_t s, const DevParams& P, const DistLane& K, uint32_t count, uint64_t first, const DistVerifyIo& io);
void launch_dist_cx_msg(hipStream_t s, const DistLane& K, uint32_t count);   // behind the normaliser: Cx into the challenge's message
void launch_dist_fold(hipStream_t s, const DistLane& K, uint32_t count);     // behind the hash: t_z + c into relation 3's opening
void launch_dist_short(hipStream_t s, const DistLane& K, uint32_t count, uint64_t first, const DistVerifyIo& io);
void launch_dist_long(hipStream_t s, const DistLane& K, uint32_t count, uint64_t first, const DistVerifyIo& io);
#endif
