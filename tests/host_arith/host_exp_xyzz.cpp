// TEST HARNESS (not product code): the XYZZ table sums of the Exp commit phase (zkp-ecdsa_amd/csrc/curve.h: p256_xyzz_madd and the sum helpers; rtab.h / ktab.h:
// the *_xyzz walks) compiled for the host CPU with g++ -DZK_HOST_BUILD -DPFIX_WIN_BITS=8 -- a comb narrow enough for its tables to be built here -- next to the
// complete-law walks they replace in k_exp_commit_kt.  Built and driven by tests/test_exp_xyzz_host.py; with -DHOST_EXP_XYZZ_MAIN it is a stand-alone program (the
// sanitizer build: g++ -fsanitize=address,undefined) that runs a fixed set of sums, the crafted collisions among them, and compares the two paths.
#define ZK_HOST_BUILD 1
#include <cstdio>
#include <cstring>
#include <vector>
#include "rtab.h"   // curve.h, ktab.h, the fixed-base comb walks

static void be_to_words(const uint8_t* p, int nbytes, uint32_t* w, int nw) {
    for (int i = 0; i < nw; i++) w[i] = 0;
    for (int i = 0; i < nbytes; i++) {
        int bi = nbytes - 1 - i;
        w[bi / 4] |= (uint32_t)p[i] << (8 * (bi % 4));
    }
}
static void words_to_be(const uint32_t* w, int nw, uint8_t* out) {
    for (int i = 0; i < nw; i++) {
        uint32_t v = __builtin_bswap32(w[nw - 1 - i]);
        memcpy(out + 4 * i, &v, 4);
    }
}
static bool p256_load(P256Aff& a, const uint8_t* xy64) {
    uint32_t xw[8], yw[8];
    be_to_words(xy64, 32, xw, 8), be_to_words(xy64 + 32, 32, yw, 8);
    a.x = fe_to_mont(fe_from_words<ModQ, 8>(xw));
    a.y = fe_to_mont(fe_from_words<ModQ, 8>(yw));
    return p256_on_curve(a);
}
static void p256_store(const P256Pt& p, uint8_t* out64) {  // identity -> 64 zero bytes
    Fq2 z = fe_reduce(p.z);
    if (fe_is_zero(z)) {
        memset(out64, 0, 64);
        return;
    }
    Fq2 zi = fe_inv<ModQ>(z);
    uint32_t w[9];
    words_from_limbs<9>(w, fe_from_mont(p.x * zi).l);
    words_to_be(w, 8, out64);
    words_from_limbs<9>(w, fe_from_mont(p.y * zi).l);
    words_to_be(w, 8, out64 + 32);
}
static P256Aff to_affine(const P256Pt& p) {
    Fq2 zi = fe_inv<ModQ>(fe_reduce(p.z));
    P256Aff a;
    a.x = p.x * zi, a.y = p.y * zi;
    return a;
}

// the three tables: G's and h's combs (every d * 2^(PFIX_WIN_BITS w) * B, d = 1 .. 2^PFIX_WIN_BITS - 1, Montgomery limbs) and one key's table as k_ktab.hip builds it
static std::vector<uint32_t> g_tab_G, g_tab_H, g_tab_K;
static void build_comb(std::vector<uint32_t>& tab, const P256Aff& B) {
    tab.assign(PFIX_TAB_WORDS, 0);
    P256Pt base = p256_from_affine(B);
    for (uint32_t w = 0; w < PFIX_NWIN; w++) {
        P256Pt acc = base;
        for (uint32_t d = 1; d < PFIX_WIN_SIZE; d++) {
            if (d > 1) acc = p256_add(acc, base);
            const P256Aff a = to_affine(acc);
            uint32_t* e = tab.data() + (size_t)PFIX_ENTRY_WORDS * (w * PFIX_WIN_SIZE + d);
            for (int l = 0; l < 9; l++) e[l] = a.x.l[l], e[9 + l] = a.y.l[l];
        }
        for (uint32_t k = 0; k < PFIX_WIN_BITS; k++) base = p256_dbl(base);
    }
}
extern "C" int hx_init(const uint8_t* g64, const uint8_t* h64, const uint8_t* key64) {
    P256Aff G, H, K;
    if (!p256_load(G, g64) || !p256_load(H, h64) || !p256_load(K, key64)) return -1;
    build_comb(g_tab_G, G), build_comb(g_tab_H, H);
    g_tab_K.assign(KTAB_KEY_WORDS, 0);
    P256Pt base = p256_from_affine(K);
    for (uint32_t w = 0; w < KTAB_NWIN; w++) {
        P256Pt acc = base;
        for (uint32_t d = 1; d <= KTAB_ENT; d++) {
            if (d > 1) acc = p256_add(acc, base);
            const P256Aff a = to_affine(acc);
            st_ktab(g_tab_K.data() + ((size_t)w * KTAB_ENT + d - 1) * KTAB_ENTRY_WORDS, fe_canon(a.x), fe_canon(a.y));
        }
        for (uint32_t k = 0; k < KTAB_BITS; k++) base = p256_dbl(base);
    }
    return 0;
}
// Sum i of gkb96 = g || k || b (big-endian, < 2^256): T = g G + k (+- key), A = T + b h the way k_exp_commit_kt's lanes take them (k_p256.hip: exp_kt_sums) -- one XYZZ
// chain, one zero test of ZZ per stored point, both points again with the complete law where a test fires -- and through the complete-law walks alone.
// out256: T, A of the first, T, A of the second (64 bytes each, the identity as zeros).  fell: 0, or 1 (T) | 2 (A).
extern "C" int hx_sums(uint64_t count, const uint8_t* gkb96, int neg, uint8_t* out256, uint32_t* fell) {
    if (g_tab_K.empty()) return -1;
    for (uint64_t i = 0; i < count; i++) {
        uint32_t gw[8], kw[8], bw[8], f = 0;
        uint8_t* o = out256 + 256 * i;
        auto scal = [&]() { be_to_words(gkb96 + 96 * i, 32, gw, 8), be_to_words(gkb96 + 96 * i + 32, 32, kw, 8), be_to_words(gkb96 + 96 * i + 64, 32, bw, 8); };
        scal();
        P256XyzzSum s = p256_xyzz_sum_empty();
        p256_fixed_mul_acc_xyzz(s, g_tab_G.data(), gw);
        p256_ktab_mul_acc_xyzz(s, g_tab_K.data(), kw, neg != 0);
        if (p256_xyzz_sum_degenerate(s)) f = 1;
        else p256_store(p256_xyzz_sum_point(s), o);
        p256_fixed_mul_acc_xyzz(s, g_tab_H.data(), bw);
        if (p256_xyzz_sum_degenerate(s)) f |= 2;
        else p256_store(p256_xyzz_sum_point(s), o + 64);
        scal();
        const P256Pt T = p256_ktab_mul_acc(p256_fixed_mul(g_tab_G.data(), gw), g_tab_K.data(), kw, neg != 0);
        const P256Pt A = p256_fixed_mul_acc(T, g_tab_H.data(), bw);
        if (f) p256_store(T, o), p256_store(A, o + 64);
        p256_store(T, o + 128), p256_store(A, o + 192);
        fell[i] = f;
    }
    return 0;
}
// p[0] + p[1] + ... + p[n - 1] as a bare chain of p256_xyzz_madd from the copy of p[0]; returns 1 if ZZ came out zero (out64 is then meaningless), -1 for a bad point
extern "C" int hx_chain(uint64_t n, const uint8_t* pts64, uint8_t* out64) {
    P256XyzzSum s = p256_xyzz_sum_empty();
    for (uint64_t i = 0; i < n; i++) {
        P256Aff a;
        if (!p256_load(a, pts64 + 64 * i)) return -1;
        p256_xyzz_sum_step(s, true, a);
    }
    if (p256_xyzz_sum_degenerate(s)) return 1;
    p256_store(p256_xyzz_sum_point(s), out64);
    return 0;
}

#ifdef HOST_EXP_XYZZ_MAIN
// Stand-alone run for the sanitizer build.  G is the curve's generator; h = 5 G and key = 7 G (multiples by the complete law here), so that the collisions can be
// crafted without any other arithmetic: sk = 7, hs = 5.
static void put_u64(uint8_t* be32, uint64_t v) {
    memset(be32, 0, 32);
    for (int i = 0; i < 8; i++) be32[31 - i] = (uint8_t)(v >> (8 * i));
}
int main() {
    static const uint8_t G64[64] = {0x6B, 0x17, 0xD1, 0xF2, 0xE1, 0x2C, 0x42, 0x47, 0xF8, 0xBC, 0xE6, 0xE5, 0x63, 0xA4, 0x40, 0xF2, 0x77, 0x03, 0x7D, 0x81, 0x2D, 0xEB,
                                    0x33, 0xA0, 0xF4, 0xA1, 0x39, 0x45, 0xD8, 0x98, 0xC2, 0x96, 0x4F, 0xE3, 0x42, 0xE2, 0xFE, 0x1A, 0x7F, 0x9B, 0x8E, 0xE7, 0xEB, 0x4A,
                                    0x7C, 0x0F, 0x9E, 0x16, 0x2B, 0xCE, 0x33, 0x57, 0x6B, 0x31, 0x5E, 0xCE, 0xCB, 0xB6, 0x40, 0x68, 0x37, 0xBF, 0x51, 0xF5};
    P256Aff G;
    if (!p256_load(G, G64)) return 2;
    P256Pt m = p256_from_affine(G), h = m, key = m;
    for (int i = 1; i < 5; i++) h = p256_add(h, m);
    for (int i = 1; i < 7; i++) key = p256_add(key, m);
    uint8_t h64[64], k64[64];
    p256_store(h, h64), p256_store(key, k64);
    if (hx_init(G64, h64, k64)) return 3;
    // (g, k, b, expected fell): plain sums, empty parts, and sk = 7, hs = 5: g = 3 * 7 with k = 3 (the G-sum IS the key's first entry: a doubling), T = 2 * 5 G
    // with b = 2 (T is h's first entry), g = 15, k = 0, b = 253 and its like stay generic
    const uint64_t cases[][4] = {{123456789, 987654321, 55555, 0}, {0, 0, 0, 0}, {0, 9, 0, 0}, {4, 0, 0, 0}, {0, 0, 77, 0}, {21, 3, 9, 3}, {3, 1, 2, 2}, {10, 0, 2, 2},
                                 {15, 0, 253, 0}, {0x8080808080808080ull, 0x8181818181818080ull, 0xffffffffffffffffull, 0}};
    const int n = sizeof(cases) / sizeof(cases[0]);
    std::vector<uint8_t> gkb(96 * n), out(256 * n);
    std::vector<uint32_t> fell(n);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++) put_u64(gkb.data() + 96 * i + 32 * j, cases[i][j]);
    int bad = 0;
    for (int neg = 0; neg < 2; neg++) {
        if (hx_sums(n, gkb.data(), neg, out.data(), fell.data())) return 4;
        for (int i = 0; i < n; i++) {
            if (memcmp(out.data() + 256 * i, out.data() + 256 * i + 128, 128)) bad++, printf("case %d neg %d: the two paths differ\n", i, neg);
            if (!neg && fell[i] != cases[i][3]) bad++, printf("case %d: fell %u, expected %u\n", i, fell[i], (unsigned)cases[i][3]);
        }
    }
    printf(bad ? "FAILED\n" : "host_exp_xyzz ok: %d sums x 2\n", n);
    return bad ? 1 : 0;
}
#endif
