// TEST HARNESS (not product code): the arithmetic of the key recovery (zkp-ecdsa_amd/csrc/recover.h: rec_candidate_x, rec_lift_x, rec_tail, rec_select -- what k_recover.hip's
// kernels call) compiled for the host CPU with g++ -DZK_HOST_BUILD, beside host_screen.cpp.  Built and driven by tests/test_recover_host.py.
#define ZK_HOST_BUILD 1
#include "recover.h"

static void be_to_words(const uint8_t* p, uint32_t w[8]) {
    for (int i = 0; i < 8; i++) w[i] = 0;
    for (int i = 0; i < 32; i++) {
        int bi = 31 - i;
        w[bi / 4] |= (uint32_t)p[i] << (8 * (bi % 4));
    }
}
static void fe_to_be(const Fe<ModQ, 1>& a, uint8_t* p) {
    uint32_t w[8];
    words_from_limbs<8>(w, a.l);
    for (int i = 0; i < 32; i++) p[i] = (uint8_t)(w[(31 - i) / 4] >> (8 * ((31 - i) % 4)));
}
static Fq8 mont_of(const uint8_t* p) {
    uint32_t w[8];
    be_to_words(p, w);
    return fe_to_mont(fe_from_words256_reduce<ModQ>(w)).as<8>();
}
// r: 32 bytes in [1, n).  Returns 0: the pass has no x-candidate, 1: x does not lift, 2: lifted, xy = the point with even y (plain, big-endian).
extern "C" int ha_rec_lift(const uint8_t* r32, uint32_t pass, uint8_t* xy64) {
    uint32_t rw[8];
    be_to_words(r32, rw);
    Fe<ModQ, 1> x;
    if (!rec_candidate_x(rw, pass, x)) return 0;
    P256Aff R;
    if (!rec_lift_x(x, R)) return 1;
    fe_to_be(fe_from_mont(R.x), xy64), fe_to_be(fe_from_mont(R.y), xy64 + 32);
    return 2;
}
// A, Bp: projective points as 3 x 32 big-endian plain coordinates (any representative).  out: Q0 = A + Bp, Q1 = A - Bp as 2 x 64 bytes; returns the
// identity marks (bit k: Q_k is the identity).
extern "C" int ha_rec_tail(const uint8_t* A96, const uint8_t* B96, uint8_t* out128) {
    P256Pt A, Bp;
    A.x = mont_of(A96), A.y = mont_of(A96 + 32), A.z = mont_of(A96 + 64);
    Bp.x = mont_of(B96), Bp.y = mont_of(B96 + 32), Bp.z = mont_of(B96 + 64);
    RecPair o;
    rec_tail<false>(A, Bp, o);
    for (int k = 0; k < 2; k++) fe_to_be(o.x[k], out128 + 64 * k), fe_to_be(o.y[k], out128 + 64 * k + 32);
    return (o.ident[0] ? 1 : 0) | (o.ident[1] ? 2 : 0);
}
extern "C" uint32_t ha_rec_select(const uint32_t* idx4) { return rec_select(idx4); }
