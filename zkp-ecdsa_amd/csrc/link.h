// Link proofs (include/zkattest.h: zk_link_*; equality.ts:60-116 on its own): the "ZKL1" layout and the arithmetic the engine did not have -- the verifier's
// c * C for a base the CALLER supplies and the 80-bit challenge -- plus the relation built on it and the prover's responses.  Device functions that also
// compile for the host CPU under ZK_HOST_BUILD (tests/host_arith/host_link.cpp).
#pragma once
#include "curve.h"

// "ZKL1": 16 header bytes ("ZKL1" | total_len = 256 | 0 | 0), then an EqualityProof as it lies inside ZKA1: A_1, A_2 (72 bytes each), t_x, t_r1, t_r2
#define ZKL1_HDR 16
#define ZKL1_SIZE 256
#define ZK_MAGIC_ZKL1 0x314c4b5au
#define ZKL1_A1 ZKL1_HDR
#define ZKL1_A2 (ZKL1_HDR + 72)
#define ZKL1_TX (ZKL1_HDR + 144)
#define ZKL1_MSG_BLOCKS 5   // hashPoints of four Tom-256 points: 4 x 67 bytes and SHA-256's padding

// A point with Z = 1 on the a = 1 image as the entry the mixed addition takes: (x, y, d' x y)
ZK_DEV TomNiels link_niels(const TomPt& p) {
    TomNiels e;
    e.x = p.x, e.y = p.y;
    e.dt = p.t * fe_const<ModT, 1>(TOM_D1_M);
    return e;
}
// c * base, c = c3[0] + 2^32 c3[1] + 2^64 c3[2] < 2^80, base with Z = 1.  Left to right over the challenge's bits, one doubling per bit behind the first
// set one and one mixed addition per set bit: at most 79 doublings and 79 additions.  It branches on the bits: they are public (the verifier's hash).
// The base comes out of a proof or from the caller, so it may have a component of even order: everything stays on the a = 1 law, which is complete
// (curve.h: the a = -1 model's 7-product addition is complete on points of odd order only, which nobody has checked here).
ZK_DEV TomPt link_ladder(const TomPt& base, const uint32_t c3[3]) {
    const TomNiels nb = link_niels(base);
    TomPt acc = tom_identity();
    bool started = false;
#pragma unroll
    for (int w = 2; w >= 0; w--) {
        uint32_t word = w == 2 ? c3[2] << 16 : c3[w];
#pragma unroll 1
        for (int i = w == 2 ? 16 : 32; i > 0; i--) {
            if (started) acc = tom_dbl(acc);
            if (word >> 31) {
                acc = started ? tom_add_niels(acc, nb) : base;
                started = true;
            }
            word <<= 1;
        }
    }
    return acc;
}
ZK_DEV bool link_is_identity(const TomPt& m) { return fe_is_zero(m.x) && fe_eq(m.y, m.z) && !fe_is_zero(m.z); }   // edwards.ts:117-125 on the a = 1 image
// One relation of verifyEquality (equality.ts:94-116), exactly: (t_x g + t_r h) + c C - A = O, with D = t_x g + t_r h from the comb tables
ZK_DEV bool link_relation(const TomPt& C, const uint32_t c3[3], const TomPt& D, const TomPt& A) {
    TomPt m = tom_add(link_ladder(C, c3), D);
    m = tom_add(m, tom_neg(A));
    return link_is_identity(m);
}
// (X : Y : Z) of the a = 1 image, as the commitment kernels leave it, with its T: (XZ : YZ : XY : Z^2)
ZK_DEV TomPt link_from_triple(const Ft2& x, const Ft2& y, const Ft2& z) {
    TomPt m;
    m.x = x * z, m.y = y * z, m.t = x * y, m.z = z * z;
    return m;
}
// A response of proveEquality (equality.ts:70-76): k - c v mod q, all plain canonical (k_scalar.hip: eq_respond's arithmetic)
ZK_DEV Fe<ModQ, 1> link_respond(const Fe<ModQ, 1>& k, const uint32_t c3[3], const Fe<ModQ, 1>& v) {
    const uint32_t w[8] = {c3[0], c3[1], c3[2] & 0xffffu, 0, 0, 0, 0, 0};
    Fe<ModQ, 1> c;
    limbs_from_words<8>(c.l, w);
    return fe_sub_mod(k, fe_canon(fe_to_mont(c) * v));
}

#if !defined(ZK_HOST_BUILD)
#include "engine.h"
// ------------------------------------------------------------------ bytes of a call -> words, points and scalars (k_link.hip, k_distinct.hip)
// 72 bytes (two 36-byte big-endian coordinates, 4-byte aligned) -> 18 little-endian words; true where both are below the field prime and on the curve
ZK_DEV bool lk_load_point(const uint8_t* p, uint32_t w[18]) {
    const uint32_t* q = (const uint32_t*)p;
#pragma unroll
    for (int i = 0; i < 9; i++) w[i] = bswap32(q[8 - i]), w[9 + i] = bswap32(q[17 - i]);
    return tom_words_on_curve(w, w + 9);
}
ZK_DEV Fe<ModQ, 1> lk_load_scalar(const uint8_t* p) {   // newScalar reduces (group.ts:164-167)
    uint32_t w[8];
    load_be32(p, w);
    return fe_from_words256_reduce<ModQ>(w);
}
// one point of the challenge's message: 04 || x (33 bytes) || y (33 bytes), from nine little-endian words per coordinate
ZK_DEV void lk_put_point(uint8_t* m, const uint32_t* xw, const uint32_t* yw) {
    m[0] = 4;
#pragma unroll
    for (int i = 0; i < 33; i++) m[1 + i] = (uint8_t)(xw[(32 - i) >> 2] >> (8 * ((32 - i) & 3))), m[34 + i] = (uint8_t)(yw[(32 - i) >> 2] >> (8 * ((32 - i) & 3)));
}
ZK_DEV TomPt lk_point_from_words(const uint32_t w[18]) {
    TomPt r;
    (void)tom_from_affine_words(r, w, w + 9);
    return r;
}
// ------------------------------------------------------------------ a lane's arena (api_link.hip carves it, k_link.hip's kernels read it); C = proofs per chunk
// The list's slots for a chunk of `count` proofs -- prover: 2 p, 2 p + 1 = (A_1, A_2) of proof p (k under s1, s2), 2 count + 2 p, + 1 = the openings the
// caller claims (x under r1, r2); verifier: 2 p, 2 p + 1 = t_x g + t_r1 h, t_x g + t_r2 h.
#define LINK_SLOTS 4
struct LinkLane : SigmaLane {   // L [LINK_SLOTS C], three draws, ZKL1_MSG_BLOCKS message blocks
    uint32_t* cw;         // [C][36] com1 (x, y), com2 (x, y) as the caller states them, nine little-endian words each
};
#define LINK_RNG_BLOCKS (3 + RNG_MAX_EXC)   // k, s1, s2 and a margin: rejected fills shift later draws
struct LinkProveIo {      // device pointers of a prove call, indexed by the proof's place in the batch
    const uint8_t *key, *com1, *blinder1, *com2, *blinder2;
    uint8_t* out;
    int32_t* status;
};
struct LinkVerifyIo {
    const uint8_t *com1, *com2, *proofs;
    uint8_t* ok;
    int32_t* status;
};
void launch_link_front(hipStream_t s, const LinkLane& K, uint32_t count, uint64_t first, const LinkProveIo& io);
void launch_link_opening_msg(hipStream_t s, const LinkLane& K, uint32_t count);   // behind the normaliser: the opening compare, then the challenge's message
void launch_link_respond(hipStream_t s, const LinkLane& K, uint32_t count, uint64_t first, const LinkProveIo& io);
void launch_link_parse(hipStream_t s, const LinkLane& K, uint32_t count, uint64_t first, const LinkVerifyIo& io);
void launch_link_ladder(hipStream_t s, const LinkLane& K, uint32_t count, uint64_t first, const LinkVerifyIo& io);
void launch_link_keycoms(hipStream_t s, uint64_t B, const uint8_t* proofs, const uint64_t* off, const Wire& wire, uint8_t* com, int32_t* status);
#endif
