// TEST HARNESS (not product code): the distinct-key proofs' arithmetic (zkp-ecdsa_amd/csrc/distinct.h: dist_ladder2, dist_relation5, dist_sub, dist_inverse,
// mult_responses) compiled for the host CPU with g++ -DZK_HOST_BUILD, beside host_link.cpp.  Built as a shared library and driven against the oracle by
// tests/test_distinct_host.py; with -DHOST_DISTINCT_MAIN it is a program of its own (a self-check of the joint ladder against two plain double-and-adds,
// of relation 5 with an honest A_4_2 and one a g away, of C - C and of d * (1 / d)), so that the same source runs under -fsanitize=address,undefined.
#define ZK_HOST_BUILD 1
#include <cstdio>
#include <cstring>
#include "distinct.h"

static void words_to_be(const uint32_t* w, int nw, uint8_t* out) {
    for (int i = 0; i < nw; i++) {
        uint32_t v = __builtin_bswap32(w[nw - 1 - i]);
        memcpy(out + 4 * i, &v, 4);
    }
}
static void be_to_words(const uint8_t* p, int nbytes, uint32_t* w, int nw) {
    for (int i = 0; i < nw; i++) w[i] = 0;
    for (int i = 0; i < nbytes; i++) {
        int bi = nbytes - 1 - i;
        w[bi / 4] |= (uint32_t)p[i] << (8 * (bi % 4));
    }
}
static bool tom_load(TomPt& r, const uint8_t* xy72) {
    uint32_t xw[9], yw[9];
    be_to_words(xy72, 36, xw, 9), be_to_words(xy72 + 36, 36, yw, 9);
    return tom_from_affine_words(r, xw, yw);
}
// extended point of the a = 1 image -> original-curve affine bytes (what k_tom_normalize computes)
static void tom_store(const TomPt& p, uint8_t* out72) {
    Ft2 zi = fe_inv<ModT>(fe_reduce(p.z));
    auto x = fe_from_mont((p.x * zi) * fe_const<ModT, 1>(TOM_SINV_M));
    auto y = fe_from_mont(p.y * zi);
    uint32_t w[9];
    words_from_limbs<9>(w, x.l);
    words_to_be(w, 9, out72);
    words_from_limbs<9>(w, y.l);
    words_to_be(w, 9, out72 + 36);
}
static void chal_load(const uint8_t* c10, uint32_t c3[3]) { be_to_words(c10, 10, c3, 3); }
static Fe<ModQ, 1> scalar_load(const uint8_t* be32) {
    uint32_t w[8];
    be_to_words(be32, 32, w, 8);
    return fe_from_words256_reduce<ModQ>(w);
}
static void scalar_store(const Fe<ModQ, 1>& s, uint8_t* out32) {
    uint32_t w[8];
    words_from_limbs<8>(w, s.l);
    words_to_be(w, 8, out32);
}
// out[i] = t[i] * Cy[i] + c[i] * C4[i] (dist_ladder2), affine; t is reduced mod q as the parser reduces a response
extern "C" int hd_ladder2(uint64_t count, const uint8_t* t32, const uint8_t* c10, const uint8_t* cy72, const uint8_t* c472, uint8_t* out72) {
    for (uint64_t i = 0; i < count; i++) {
        TomPt Cy, C4;
        uint32_t c3[3], t8[8];
        DistQuad tab[DIST_TAB_QUADS];
        if (!tom_load(Cy, cy72 + 72 * i) || !tom_load(C4, c472 + 72 * i)) return 1;
        chal_load(c10 + 10 * i, c3);
        words_from_limbs<8>(t8, scalar_load(t32 + 32 * i).l);
        tom_store(dist_ladder2(Cy, t8, C4, c3, tab), out72 + 72 * i);
    }
    return 0;
}
// ok[i] = dist_relation5(Cy, t_x, C4, c, A_4_2)
extern "C" int hd_relation5(uint64_t count, const uint8_t* t32, const uint8_t* c10, const uint8_t* cy72, const uint8_t* c472, const uint8_t* a72, uint8_t* ok) {
    for (uint64_t i = 0; i < count; i++) {
        TomPt Cy, C4, A;
        uint32_t c3[3], t8[8];
        DistQuad tab[DIST_TAB_QUADS];
        if (!tom_load(Cy, cy72 + 72 * i) || !tom_load(C4, c472 + 72 * i) || !tom_load(A, a72 + 72 * i)) return 1;
        chal_load(c10 + 10 * i, c3);
        words_from_limbs<8>(t8, scalar_load(t32 + 32 * i).l);
        ok[i] = dist_relation5(Cy, t8, C4, c3, A, tab) ? 1 : 0;
    }
    return 0;
}
// out[i] = C1[i] - C2[i] (dist_sub), affine
extern "C" int hd_sub(uint64_t count, const uint8_t* c1_72, const uint8_t* c2_72, uint8_t* out72) {
    for (uint64_t i = 0; i < count; i++) {
        TomPt A, B;
        if (!tom_load(A, c1_72 + 72 * i) || !tom_load(B, c2_72 + 72 * i)) return 1;
        tom_store(dist_sub(A, B), out72 + 72 * i);
    }
    return 0;
}
extern "C" int hd_inverse(uint64_t count, const uint8_t* d32, uint8_t* out32) {
    for (uint64_t i = 0; i < count; i++) scalar_store(dist_inverse(scalar_load(d32 + 32 * i)), out32 + 32 * i);
    return 0;
}
// the seven responses of one proveMult: k224 = k_x, k_y, k_z, s_x, s_y, s_z, s_4; v192 = x, y, z, r_x, r_y, r_z
extern "C" int hd_responses(uint64_t count, const uint8_t* c10, const uint8_t* k224, const uint8_t* v192, uint8_t* out224) {
    for (uint64_t i = 0; i < count; i++) {
        uint32_t c3[3];
        chal_load(c10 + 10 * i, c3);
        Fe<ModQ, 1> k[7], v[6], t[7];
        for (int j = 0; j < 7; j++) k[j] = scalar_load(k224 + 224 * i + 32 * j);
        for (int j = 0; j < 6; j++) v[j] = scalar_load(v192 + 192 * i + 32 * j);
        mult_responses(t, c3, k, v[0], v[1], v[2], v[3], v[4], v[5]);
        for (int j = 0; j < 7; j++) scalar_store(t[j], out224 + 224 * i + 32 * j);
    }
    return 0;
}

#ifdef HOST_DISTINCT_MAIN
// k * P by a plain double-and-add on the general addition (the self-check's own reference)
static TomPt plain_mul(const TomPt& P, const uint32_t* w, int nbits) {
    TomPt acc = tom_identity();
    for (int i = nbits - 1; i >= 0; i--) {
        acc = tom_dbl(acc);
        if ((w[i >> 5] >> (i & 31)) & 1) acc = tom_add(acc, P);
    }
    return acc;
}
// Tom-256's generator (instances.ts:38-54) as 36-byte big-endian coordinates
static const char* GEN_X = "000000007907055d0a7d4abc3eafdc25d431d9659fbe007ee2d8ddc4e906206ea9ba4fdb";
static const char* GEN_Y = "00000000be231cb9f9bf18319c9f081141559b0a33dddccd2221f0464a9cd57081b01a01";
static void hex_to(const char* h, uint8_t* out, int n) {
    for (int i = 0; i < n; i++) {
        unsigned v;
        sscanf(h + 2 * i, "%2x", &v);
        out[i] = (uint8_t)v;
    }
}
static TomPt affine(const TomPt& p) {   // the same point with Z = 1, as a proof's bytes give it
    uint8_t t72[72];
    TomPt r;
    tom_store(p, t72), tom_load(r, t72);
    return r;
}
int main() {
    uint8_t g72[72];
    hex_to(GEN_X, g72, 36), hex_to(GEN_Y, g72 + 36, 36);
    TomPt G;
    if (!tom_load(G, g72)) return printf("generator not on the curve\n"), 1;
    const uint32_t k7[8] = {0x9e3779b9u, 0x7f4a7c15u, 0xf39cc060u, 0x5cedc834u, 0x1082276bu, 0xf3a27251u, 0xf86c6a11u, 0x0d1a5b3cu};
    const TomPt Cy = affine(plain_mul(G, k7, 256)), C4 = affine(tom_dbl(tom_add(Cy, G))), O = affine(tom_identity());
    const uint32_t ts[6][8] = {{0, 0, 0, 0, 0, 0, 0, 0}, {1, 0, 0, 0, 0, 0, 0, 0}, {2, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0x80000000u},
                               {0xfffffffeu, 0xffffffffu, 0xffffffffu, 0, 0, 0, 1, 0xffffffffu},   // q - 1
                               {0x12345678u, 0x9abcdef0u, 0x0fedcba9u, 0x87654321u, 0xdeadbeefu, 0x01234567u, 0x89abcdefu, 0x7fffffffu}};
    const uint32_t cs[5][3] = {{0, 0, 0}, {1, 0, 0}, {0, 0, 0x8000}, {0xffffffffu, 0xffffffffu, 0xffff}, {0x12345678u, 0x9abcdef0u, 0x0fed}};
    struct {
        const TomPt *y, *c4;
    } pairs[5] = {{&Cy, &C4}, {&Cy, &Cy}, {&O, &C4}, {&Cy, &O}, {&Cy, nullptr /* -Cy: the precomputed sum is the identity */}};
    const TomPt negCy = affine(tom_neg(Cy));
    int bad = 0;
    for (auto& pr : pairs)
        for (auto& t : ts)
            for (auto& c : cs) {
                const TomPt& b4 = pr.c4 ? *pr.c4 : negCy;
                DistQuad tab[DIST_TAB_QUADS];
                uint8_t a[72], b[72];
                tom_store(dist_ladder2(*pr.y, t, b4, c, tab), a);
                const TomPt want = tom_add(plain_mul(*pr.y, t, 256), plain_mul(b4, c, 80));
                tom_store(want, b);
                if (memcmp(a, b, 72)) bad++, printf("joint ladder differs\n");
                if (!dist_relation5(*pr.y, t, b4, c, affine(want), tab)) bad++, printf("honest relation 5 refused\n");
                if (dist_relation5(*pr.y, t, b4, c, affine(tom_add(want, G)), tab)) bad++, printf("relation 5 accepted an A_4_2 one g away\n");
            }
    {   // C - C is the identity, (0, 1); d * (1 / d) = 1, 1 / 0 = 0
        uint8_t a[72], o[72] = {0};
        o[71] = 1;
        tom_store(dist_sub(Cy, Cy), a);
        if (memcmp(a, o, 72)) bad++, printf("C - C is not (0, 1)\n");
        const Fe<ModQ, 1> d = fe_from_words256_reduce<ModQ>(ts[5]);
        const Fe<ModQ, 1> p = fe_mul_mod(d, dist_inverse(d));
        uint32_t w[8];
        words_from_limbs<8>(w, p.l);
        if (w[0] != 1 || w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) bad++, printf("d * (1 / d) is not 1\n");
        if (!fe_is_zero(dist_inverse(fe_zero<ModQ>()))) bad++, printf("1 / 0 is not 0\n");
    }
    if (bad) printf("host_distinct: %d failures\n", bad);
    else printf("host_distinct: ok\n");
    return bad ? 1 : 0;
}
#endif
