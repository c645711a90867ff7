// TEST HARNESS (not product code): the witness screen's point arithmetic on cooperating waves (zkp-ecdsa_amd/csrc/coop_sums.h: co_front_pk_multiples,
// co_front_walk, co_fixed_mul_range, co_ktab_mul_range -- what k_screen_walk_co and k_screen_table_co run) compiled for the host CPU against coop.h's SIMT
// emulation, g++ -DZK_HOST_BUILD -DPFIX_WIN_BITS=8 (a comb narrow enough for its table to be built here).  A stand-alone program: it reads
//     G <xy>      the generator, 64 bytes as hex
//     K <xy>      a public key
//     C <u1> <u2> a pair of scalars, 32 bytes each as hex (any number of them, after G and K)
// from standard input and prints, per pair, the affine points (hex, the identity as zeros)
//     walk  u2 * K by the 65-window walk over the parked multiples 1..8 of K
//     kt+   u2 * K through K's table, the four waves' ranges of k_screen_table_co added up;  kt-  the same with the table's base point negated
//     g4    u1 * G through G's comb, four ranges (k_screen_table_co);  g3  three ranges (k_screen_walk_co's waves 1..3)
//     R     g3 + walk, joined by one cooperative addition as the walk kernel ends
// Driven by tests/test_screen_co_host.py, which compares every line with the oracle.
#define ZK_HOST_BUILD 1
#include <cstdio>
#include <cstring>
#include <vector>
#include "coop_sums.h"

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
static P256Aff to_affine(const P256Pt& p) {
    Fq2 zi = fe_inv<ModQ>(fe_reduce(p.z));
    P256Aff a;
    a.x = p.x * zi, a.y = p.y * zi;
    return a;
}
static void print_point(const char* tag, const CoP256& c) {
    P256Pt p;
    co_store4(c.v, p.x.l, p.y.l, p.z.l, nullptr);
    uint8_t out[64];
    memset(out, 0, 64);
    if (!fe_is_zero(fe_reduce(p.z))) {
        const P256Aff a = to_affine(p);
        uint32_t w[9];
        words_from_limbs<9>(w, fe_from_mont(a.x).l);
        words_to_be(w, 8, out);
        words_from_limbs<9>(w, fe_from_mont(a.y).l);
        words_to_be(w, 8, out + 32);
    }
    printf("%s ", tag);
    for (int i = 0; i < 64; i++) printf("%02x", out[i]);
    printf("\n");
}
static bool hex_bytes(const char* s, uint8_t* out, int n) {
    if ((int)strlen(s) != 2 * n) return false;
    for (int i = 0; i < n; i++) {
        unsigned v;
        if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}
// G's comb (every d * 2^(PFIX_WIN_BITS w) * G, Montgomery limbs) and K's table as k_ktab.hip builds it
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
static void build_ktab(std::vector<uint32_t>& tab, const P256Aff& K) {
    tab.assign(KTAB_KEY_WORDS, 0);
    P256Pt base = p256_from_affine(K);
    for (uint32_t w = 0; w < KTAB_NWIN; w++) {
        P256Pt acc = base;
        for (uint32_t d = 1; d <= KTAB_ENT; d++) {
            if (d > 1) acc = p256_add(acc, base);
            const P256Aff a = to_affine(acc);
            st_ktab(tab.data() + ((size_t)w * KTAB_ENT + d - 1) * KTAB_ENTRY_WORDS, fe_canon(a.x), fe_canon(a.y));
        }
        for (uint32_t k = 0; k < KTAB_BITS; k++) base = p256_dbl(base);
    }
}
// the sum of `parts` waves' ranges, added up in wave order as co_wg4_sum and k_screen_walk_co's wave 1 do
template <class Range>
static CoP256 sum_ranges(uint32_t parts, const CoU32& mj, const Range& range) {
    CoP256 total = range(0);
    for (uint32_t q = 1; q < parts; q++) total = co_p256_add(total, range(q), mj);
    return total;
}

int main() {
    std::vector<uint32_t> comb, ktab, mult(CO_WALK_MULT_WORDS);
    P256Aff G, K;
    bool have_g = false, have_k = false;
    const CoU32 mj = co_limbs(ModQ::mod);
    char tag[8], a[160], b[160];
    int n = 0;
    for (;;) {
        const int got = scanf("%7s %159s", tag, a);
        if (got != 2) break;
        uint8_t xy[64], u1b[32], u2b[32];
        if (tag[0] == 'G' || tag[0] == 'K') {
            if (!hex_bytes(a, xy, 64)) return 2;
            if (tag[0] == 'G') {
                if (!p256_load(G, xy)) return 3;
                build_comb(comb, G), have_g = true;
            } else {
                if (!p256_load(K, xy)) return 3;
                build_ktab(ktab, K), have_k = true;
                uint32_t e[2 * NLIMB];   // K as k_screen_front leaves it in the witness's area: nine Montgomery limbs of x, nine of y
                for (int l = 0; l < NLIMB; l++) e[l] = K.x.l[l], e[NLIMB + l] = K.y.l[l];
                CoP256 base;
                base.v = co_load_pfix(e);
                co_front_pk_multiples(mult.data(), base, mj);
            }
            continue;
        }
        if (tag[0] != 'C' || !have_g || !have_k || scanf("%159s", b) != 1 || !hex_bytes(a, u1b, 32) || !hex_bytes(b, u2b, 32)) return 4;
        uint32_t u1[8], u2[8], kw[8];
        be_to_words(u1b, 32, u1, 8), be_to_words(u2b, 32, u2, 8);
        uint8_t dig[FRONT_NW];
        memcpy(kw, u2, sizeof kw);
        front_recode(kw, dig);
        const CoP256 walk = co_front_walk(mult.data(), dig, mj);
        print_point("walk", walk);
        constexpr uint32_t kper = (KTAB_NWIN + 3) / 4, g4per = (PFIX_NWIN + 3) / 4, g3per = (PFIX_NWIN + 2) / 3;
        for (int neg = 0; neg < 2; neg++)
            print_point(neg ? "kt-" : "kt+", sum_ranges(4, mj, [&](uint32_t q) { return co_ktab_mul_range(co_p256_identity(), ktab.data(), u2, neg != 0, q * kper, kper, mj); }));
        const auto comb_range = [&](uint32_t per) {
            return [&, per](uint32_t q) {
                memcpy(kw, u1, sizeof kw);
                return co_fixed_mul_range(co_p256_identity(), comb.data(), kw, q * per, per, mj);
            };
        };
        print_point("g4", sum_ranges(4, mj, comb_range(g4per)));
        const CoP256 g3 = sum_ranges(3, mj, comb_range(g3per));
        print_point("g3", g3);
        print_point("R", co_p256_add(g3, walk, mj));
        n++;
    }
    printf("done %d\n", n);
    return 0;
}
