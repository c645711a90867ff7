// TEST HARNESS (not product code): the escrow tags' arithmetic (zkp-ecdsa_amd/csrc/escrow.h: escrow_ladder, escrow_open_point, escrow_responses and the ZKT1
// layout constants) compiled for the host CPU with g++ -DZK_HOST_BUILD, beside host_link.cpp.  Built as a shared library and driven against the Python
// statement by tests/test_escrow_host.py; with -DHOST_ESCROW_MAIN it is a program of its own (the masked ladder against a plain double-and-add, the opening
// rule with and without components of small order, and the ladder, the responses and the opening against values of the Python statement), so that the same
// source runs under -fsanitize=address,undefined.
#define ZK_HOST_BUILD 1
#include <cstdio>
#include <cstring>
#include "escrow.h"

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
static Fe<ModQ, 1> scalar_load(const uint8_t* be32) {
    uint32_t w[8];
    be_to_words(be32, 32, w, 8);
    return fe_from_words256_reduce<ModQ>(w);
}

extern "C" int he_layout(uint32_t out[8]) {
    out[0] = ZKT1_SIZE, out[1] = ZKT1_HDR, out[2] = ZK_MAGIC_ZKT1, out[3] = ZKT1_PT(0), out[4] = ZKT1_PT(4), out[5] = ZKT1_SC(0), out[6] = ZKT1_SC(2) + 32, out[7] = ZKT1_MSG_BLOCKS;
    return 0;
}
// out[i] = a[i] * base[i] (escrow_ladder) for a 256-bit a taken as it stands (NOT reduced), affine
extern "C" int he_ladder(uint64_t count, const uint8_t* a32, const uint8_t* base72, uint8_t* out72) {
    for (uint64_t i = 0; i < count; i++) {
        TomPt B;
        uint32_t a8[8];
        if (!tom_load(B, base72 + 72 * i)) return 1;
        be_to_words(a32 + 32 * i, 32, a8, 8);
        tom_store(escrow_ladder(B, a8), out72 + 72 * i);
    }
    return 0;
}
// out[i] = 4 (E2[i] - a[i] E1[i]) (escrow_open_point), affine
extern "C" int he_open(uint64_t count, const uint8_t* a32, const uint8_t* e1_72, const uint8_t* e2_72, uint8_t* out72) {
    for (uint64_t i = 0; i < count; i++) {
        TomPt E1, E2;
        uint32_t a8[8];
        if (!tom_load(E1, e1_72 + 72 * i) || !tom_load(E2, e2_72 + 72 * i)) return 1;
        be_to_words(a32 + 32 * i, 32, a8, 8);
        tom_store(escrow_open_point(E1, E2, a8), out72 + 72 * i);
    }
    return 0;
}
// out[i] = (t_x, t_r, t_rho) of escrow_responses for c[i], nonces k[i][3] = (k_x, k_r, k_rho) and values v[i][3] = (x, r, rho)
extern "C" int he_respond(uint64_t count, const uint8_t* c10, const uint8_t* k96, const uint8_t* v96, uint8_t* out96) {
    for (uint64_t i = 0; i < count; i++) {
        uint32_t c3[3], w[8];
        be_to_words(c10 + 10 * i, 10, c3, 3);
        Fe<ModQ, 1> t[3];
        escrow_responses(t, c3, scalar_load(k96 + 96 * i), scalar_load(k96 + 96 * i + 32), scalar_load(k96 + 96 * i + 64), scalar_load(v96 + 96 * i),
                         scalar_load(v96 + 96 * i + 32), scalar_load(v96 + 96 * i + 64));
        for (int j = 0; j < 3; j++) {
            words_from_limbs<8>(w, t[j].l);
            words_to_be(w, 8, out96 + 96 * i + 32 * j);
        }
    }
    return 0;
}

#ifdef HOST_ESCROW_MAIN
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
// k * P for a 256-bit k by a plain double-and-add on the general addition (the self-check's own reference)
static TomPt plain_mul(const TomPt& P, const uint32_t* w, int nbits) {
    TomPt acc = tom_identity();
    for (int i = nbits - 1; i >= 0; i--) {
        acc = tom_dbl(acc);
        if ((w[i >> 5] >> (i & 31)) & 1) acc = tom_add(acc, P);
    }
    return acc;
}
static TomPt z1(const TomPt& p) {   // the same point with Z = 1, as the ladder takes its base
    uint8_t t72[72];
    TomPt r;
    tom_store(p, t72), tom_load(r, t72);
    return r;
}
// Values of the Python statement (tests/escrow_common.py over the oracle's points: a plain double-and-add of Point.add, Scalar.sub / mul, times4), so that the
// sanitized run checks the ladder, the responses and the opening rule against them too.  Bases: g, and g + (the point of order 4 with y = 0).  Scalars: q - 1,
// q (the sum reaches the identity at the last bit) and a fixed 255-bit a.
static const char* PY_Q1 = "ffffffff00000001000000000000000000000000fffffffffffffffffffffffe";
static const char* PY_Q = "ffffffff00000001000000000000000000000000ffffffffffffffffffffffff";
static const char* PY_A = "7edcba9889abcdef01234567deadbeef876543210fedcba99abcdef012345678";
static const char* PY_GP4 = "000000014436c3b92215251d31cb59c40c919b1b6d0f40074a7b57533bc66b92d80f880400000001aa4c05f0aedbcc579fe21d8edeb522488868a0f723d74cfb620687d922a824b9";
static const char* PY_LADDER[3][2] = {   // [scalar q - 1, q, a][base g, g + P4]
    {"0000000386f8fa9ef582b547c15023da2bce269d0e7a2bfa74f3723488361d14128d83d400000000be231cb9f9bf18319c9f081141559b0a33dddccd2221f0464a9cd57081b01a01",
     "000000007907055d0a7d4abc3eafdc25d431d9659fbe007ee2d8ddc4e906206ea9ba4fdb0000000341dce3420640e7d26360f7eebeaa64f87a5a4fac35aa5fb3269f68123a97b9ae"},
    {"000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000000001",
     "0000000186056fe258184edf35b110d74d3f897810b94567ec8ff04a32c683d009b72de7000000000000000000000000000000000000000000000000000000000000000000000000"},
    {"00000000284ccdc7ee787a729e2c620502b207ec1877bc1ca53f2893d32f37abf439f695000000034c67dc044e9016e06f9ec7c0b5e0e50b003208e844f8f89b18aa9a265f475de7",
     "00000000284ccdc7ee787a729e2c620502b207ec1877bc1ca53f2893d32f37abf439f695000000034c67dc044e9016e06f9ec7c0b5e0e50b003208e844f8f89b18aa9a265f475de7"}};
// responses k - c v mod q for c = 0x0fed9abcdef012345678, k = (q - 1, 5, a), v = (q - 1, 2^256 - 1, 0x1234)
static const char* PY_RESP_V[3] = {PY_Q1, "ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff", "0000000000000000000000000000000000000000000000000000000000001234"};
static const char* PY_RESP_K1 = "0000000000000000000000000000000000000000000000000000000000000005";
static const char* PY_RESP[3] = {"000000000000000000000000000000000000000000000fed9abcdef012345677", "edcbb974acf1356900000fed9abceeddacf13568fffffffffffff01265432114",
                                 "7edcba9889abcdef01234567deadbeef876543210ecbda84e4b2b4e4b17e5618"};
// the opening rule for A = a g, x = 0xabcdef, rho = 0x1357924680: E1 = rho g + (the point of order 2), E2 = x g + rho A + (the point of order 4); 4 x g
static const char* PY_E1 = "000000035bbe7a758695384de0382e0936cdbead83b035112092372c69e59ccb60cfed6000000000c59473b8a52337a8fe23b64a6a30891346f546d7ea0f4771a09049bba3f868d2";
static const char* PY_E2 = "00000003e0a034be258d99798cb8d4da37984b62ef5f774235a5c3d0d5f0e956baa630d100000000b8915d1aaddbe3b9ab2203ca71ad1c9da0de843b4d5a163355c5a85df69406c2";
static const char* PY_OPEN = "0000000146557b84dbe36a39ff85958357971c442993f96196695b7bda6038ff9984d65b00000002ec7d99fb8750b9c1ec8057fe2c6bde445647b5fe1c67761992a72a3afc1468ba";
static int python_vectors() {
    int bad = 0;
    uint8_t base72[2][72], s32[32], want[72], got[96];
    hex_to(GEN_X, base72[0], 36), hex_to(GEN_Y, base72[0] + 36, 36), hex_to(PY_GP4, base72[1], 72);
    const char* scalars[3] = {PY_Q1, PY_Q, PY_A};
    for (int i = 0; i < 3; i++)
        for (int b = 0; b < 2; b++) {
            hex_to(scalars[i], s32, 32), hex_to(PY_LADDER[i][b], want, 72);
            if (he_ladder(1, s32, base72[b], got) || memcmp(got, want, 72)) bad++, printf("ladder differs from the Python value for scalar %d, base %d\n", i, b);
        }
    uint8_t c10[10], k96[96], v96[96];
    hex_to("0fed9abcdef012345678", c10, 10);
    hex_to(PY_Q1, k96, 32), hex_to(PY_RESP_K1, k96 + 32, 32), hex_to(PY_A, k96 + 64, 32);
    for (int j = 0; j < 3; j++) hex_to(PY_RESP_V[j], v96 + 32 * j, 32);
    he_respond(1, c10, k96, v96, got);
    for (int j = 0; j < 3; j++) {
        hex_to(PY_RESP[j], s32, 32);
        if (memcmp(got + 32 * j, s32, 32)) bad++, printf("response %d differs from the Python value\n", j);
    }
    uint8_t e1[72], e2[72];
    hex_to(PY_A, s32, 32), hex_to(PY_E1, e1, 72), hex_to(PY_E2, e2, 72), hex_to(PY_OPEN, want, 72);
    if (he_open(1, s32, e1, e2, got) || memcmp(got, want, 72)) bad++, printf("opening differs from the Python value\n");
    return bad;
}
int main() {
    static_assert(ZKT1_SIZE == 472 && ZKT1_SC(2) + 32 == ZKT1_SIZE && ZKT1_PT(4) + 72 == ZKT1_SC(0) && 7 * 67 + 9 <= ZKT1_MSG_BLOCKS * 64, "ZKT1 layout");
    uint8_t g72[72];
    hex_to(GEN_X, g72, 36), hex_to(GEN_Y, g72 + 36, 36);
    TomPt G;
    if (!tom_load(G, g72)) return printf("generator not on the curve\n"), 1;
    // (0, -1) has order 2 on the a = 1 image as on the curve; (1, 0) has order 4 there
    TomPt P2 = tom_identity(), P4 = tom_identity();
    P2.y = fe_reduce(fe_neg(P2.y));
    P4.x = P4.y, P4.y = fe_zero<ModT>().as<2>();
    const uint32_t k7[8] = {0x9e3779b9u, 0x7f4a7c15u, 0xf39cc060u, 0x5cedc834u, 0x1082276bu, 0xf3a27251u, 0xf86c6a11u, 0x0d1a5b3cu};
    const TomPt C = z1(plain_mul(G, k7, 256));
    const TomPt bases[4] = {G, C, z1(tom_add(C, P4)), z1(tom_add(G, P2))};
    const uint32_t as[6][8] = {{0, 0, 0, 0, 0, 0, 0, 0}, {1, 0, 0, 0, 0, 0, 0, 0}, {2, 0, 0, 0, 0, 0, 0, 0}, {1, 0, 0, 0, 0, 0, 0, 0x80000000u},
                               {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                               {0x12345678u, 0x9abcdef0u, 0x0fedcba9u, 0x87654321u, 0xdeadbeefu, 0x01234567u, 0x89abcdefu, 0x7edcba98u}};
    int bad = 0;
    for (int i = 0; i < 6; i++)
        for (int b = 0; b < 4; b++) {
            uint8_t x[72], y[72];
            tom_store(escrow_ladder(bases[b], as[i]), x);
            tom_store(plain_mul(bases[b], as[i], 256), y);
            if (memcmp(x, y, 72)) bad++, printf("ladder differs for scalar %d, base %d\n", i, b);
        }
    // the opening rule: E1 = rho g, E2 = C + rho (a g) opens to 4 C, with and without a component of small order on E1 and E2
    const uint32_t* a = as[5];
    const uint32_t rho[8] = {0x0badcafeu, 0x11111111u, 0x22222222u, 0x33333333u, 0x44444444u, 0x55555555u, 0x66666666u, 0x07777777u};
    const TomPt A = z1(plain_mul(G, a, 256)), E1 = plain_mul(G, rho, 256), E2 = tom_add(C, plain_mul(A, rho, 256));
    uint8_t want[72], got[72];
    tom_store(tom_dbl(tom_dbl(C)), want);
    const TomPt* small[3] = {nullptr, &P2, &P4};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const TomPt e1 = z1(small[i] ? tom_add(E1, *small[i]) : E1), e2 = z1(small[j] ? tom_add(E2, *small[j]) : E2);
            tom_store(escrow_open_point(e1, e2, a), got);
            if (memcmp(want, got, 72)) bad++, printf("opening differs with small-order components %d, %d\n", i, j);
        }
    tom_store(escrow_open_point(z1(E1), z1(tom_add(E2, G)), a), got);
    if (!memcmp(want, got, 72)) bad++, printf("a tag of another key opened to this one\n");
    bad += python_vectors();
    if (bad) printf("host_escrow: %d failures\n", bad);
    else printf("host_escrow: ok\n");
    return bad ? 1 : 0;
}
#endif
