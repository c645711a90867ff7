// TEST HARNESS (not product code): the link proofs' arithmetic (zkp-ecdsa_amd/csrc/link.h: link_ladder, link_relation, link_from_triple, link_respond)
// compiled for the host CPU with g++ -DZK_HOST_BUILD, beside host_arith.cpp.  Built as a shared library and driven against the oracle by
// tests/test_link_host.py; with -DHOST_LINK_MAIN it is a program of its own (a self-check of the ladder against a plain double-and-add and of the relation
// with an honest and an off-by-one A), so that the same source runs under -fsanitize=address,undefined.
#define ZK_HOST_BUILD 1
#include <cstdio>
#include <cstring>
#include "link.h"

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
// k * P for a 256-bit k by a plain double-and-add on the general addition (the test's own reference for the comb part and the self-check)
static TomPt plain_mul(const TomPt& P, const uint32_t* w, int nbits) {
    TomPt acc = tom_identity();
    for (int i = nbits - 1; i >= 0; i--) {
        acc = tom_dbl(acc);
        if ((w[i >> 5] >> (i & 31)) & 1) acc = tom_add(acc, P);
    }
    return acc;
}

// out[i] = c[i] * base[i] (link_ladder), affine
extern "C" int hl_ladder(uint64_t count, const uint8_t* c10, const uint8_t* base72, uint8_t* out72) {
    for (uint64_t i = 0; i < count; i++) {
        TomPt B;
        uint32_t c3[3];
        if (!tom_load(B, base72 + 72 * i)) return 1;
        chal_load(c10 + 10 * i, c3);
        tom_store(link_ladder(B, c3), out72 + 72 * i);
    }
    return 0;
}
// ok[i] = link_relation(C, c, D, A) with D = t_x g + t_r h handed over as the commitment kernels leave it: a projective triple without T
extern "C" int hl_relation(uint64_t count, const uint8_t* g72, const uint8_t* h72, const uint8_t* c10, const uint8_t* C72, const uint8_t* tx32, const uint8_t* tr32,
                           const uint8_t* A72, uint8_t* ok) {
    TomPt G, H;
    if (!tom_load(G, g72) || !tom_load(H, h72)) return 1;
    for (uint64_t i = 0; i < count; i++) {
        TomPt C, A;
        if (!tom_load(C, C72 + 72 * i) || !tom_load(A, A72 + 72 * i)) return 1;
        uint32_t c3[3], w[8];
        chal_load(c10 + 10 * i, c3);
        words_from_limbs<8>(w, scalar_load(tx32 + 32 * i).l);
        TomPt D = plain_mul(G, w, 256);
        words_from_limbs<8>(w, scalar_load(tr32 + 32 * i).l);
        D = tom_add(D, plain_mul(H, w, 256));   // (an extended point with Z != 1: its T is dropped and rebuilt)
        ok[i] = link_relation(C, c3, link_from_triple(D.x, D.y, D.z), A) ? 1 : 0;
    }
    return 0;
}
extern "C" int hl_respond(uint64_t count, const uint8_t* k32, const uint8_t* c10, const uint8_t* v32, uint8_t* out32) {
    for (uint64_t i = 0; i < count; i++) {
        uint32_t c3[3], w[8];
        chal_load(c10 + 10 * i, c3);
        words_from_limbs<8>(w, link_respond(scalar_load(k32 + 32 * i), c3, scalar_load(v32 + 32 * i)).l);
        words_to_be(w, 8, out32 + 32 * i);
    }
    return 0;
}

#ifdef HOST_LINK_MAIN
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
int main() {
    uint8_t g72[72];
    hex_to(GEN_X, g72, 36), hex_to(GEN_Y, g72 + 36, 36);
    TomPt G;
    if (!tom_load(G, g72)) return printf("generator not on the curve\n"), 1;
    const uint32_t k7[8] = {0x9e3779b9u, 0x7f4a7c15u, 0xf39cc060u, 0x5cedc834u, 0x1082276bu, 0xf3a27251u, 0xf86c6a11u, 0x0d1a5b3cu};
    TomPt C, H;   // two more bases, with Z = 1 as the ladder takes them
    {
        uint8_t t72[72];
        const TomPt c0 = plain_mul(G, k7, 256);
        tom_store(c0, t72), tom_load(C, t72);
        tom_store(tom_dbl(tom_add(c0, G)), t72), tom_load(H, t72);
    }
    const uint32_t cs[8][3] = {{0, 0, 0}, {1, 0, 0}, {2, 0, 0}, {0, 0, 0x8000}, {0xffffffffu, 0xffffffffu, 0xffff}, {0x55555555u, 0x55555555u, 0x5555},
                               {0xaaaaaaaau, 0xaaaaaaaau, 0xaaaa}, {0x12345678u, 0x9abcdef0u, 0x0fed}};
    int bad = 0;
    const TomPt* bases[3] = {&C, &H, &G};
    for (int i = 0; i < 8; i++)
        for (const TomPt* base : bases) {
            uint8_t a[72], b[72];
            tom_store(link_ladder(*base, cs[i]), a);
            const uint32_t w[3] = {cs[i][0], cs[i][1], cs[i][2]};
            tom_store(plain_mul(*base, w, 80), b);
            if (memcmp(a, b, 72)) bad++, printf("ladder differs for challenge %d\n", i);
            // the relation: D + c base - A with A = D + c base, then with A one G further
            const TomPt D = tom_add(tom_dbl(H), G), A = tom_add(D, plain_mul(*base, w, 80));
            uint8_t a72[72];
            tom_store(A, a72);
            TomPt Aa;
            tom_load(Aa, a72);
            if (!link_relation(*base, cs[i], link_from_triple(D.x, D.y, D.z), Aa)) bad++, printf("honest relation refused for challenge %d\n", i);
            tom_store(tom_add(A, G), a72);
            tom_load(Aa, a72);
            if (link_relation(*base, cs[i], link_from_triple(D.x, D.y, D.z), Aa)) bad++, printf("relation accepted an A one g away for challenge %d\n", i);
        }
    if (bad) printf("host_link: %d failures\n", bad);
    else printf("host_link: ok\n");
    return bad ? 1 : 0;
}
#endif
