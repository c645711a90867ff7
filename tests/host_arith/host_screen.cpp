// TEST HARNESS (not product code): the last step of the witness screen's ECDSA check (zkp-ecdsa_amd/csrc/curve.h: p256_x_is_r_mod_n, what k_screen_walk
// calls) compiled for the host CPU with g++ -DZK_HOST_BUILD, beside host_arith.cpp.  Built and driven by tests/test_screen_host.py.
#define ZK_HOST_BUILD 1
#include "curve.h"

static void be_to_words(const uint8_t* p, int nbytes, uint32_t* w, int nw) {
    for (int i = 0; i < nw; i++) w[i] = 0;
    for (int i = 0; i < nbytes; i++) {
        int bi = nbytes - 1 - i;
        w[bi / 4] |= (uint32_t)p[i] << (8 * (bi % 4));
    }
}
// X, Z: 32-byte big-endian plain coordinates of a projective point (any representative below 2^256); r: 32 bytes, in [1, n).  Returns 1 / 0.
extern "C" int ha_x_is_r_mod_n(const uint8_t* X32, const uint8_t* Z32, const uint8_t* r32) {
    uint32_t xw[8], zw[8], rw[8];
    be_to_words(X32, 32, xw, 8), be_to_words(Z32, 32, zw, 8), be_to_words(r32, 32, rw, 8);
    P256Pt R;
    R.x = fe_to_mont(fe_from_words256_reduce<ModQ>(xw)).as<8>();
    R.y = fe_one_mont<ModQ>().as<8>();
    R.z = fe_to_mont(fe_from_words256_reduce<ModQ>(zw)).as<8>();
    Fe<ModN, 1> r;
    limbs_from_words<8>(r.l, rw);
    return p256_x_is_r_mod_n(R, r) ? 1 : 0;
}
