// TEST HARNESS (not product code): the a = -1 model of the Tom-256 fixed-base comb tables (zkp-ecdsa_amd/csrc/curve.h: TomModel<TOM_MODEL_M1>, coop.h:
// co_tom_m1_*) compiled for the host CPU with g++ -DZK_HOST_BUILD, beside host_arith.cpp.  Table entries are made here the way k_tables.hip's composer makes
// them (from an extended point of the a = 1 image with any Z), and whole comb sums run in the three shapes the kernels of k_tom.hip use: one lane
// (first / add / add_last), four partial sums joined by general additions (k_tom_commit_wide), and rows of a wave (k_tom_commit_co).  Every result leaves
// as the a = 1 image's projective triple and is normalised like k_tom_normalize does.  Built and driven by tests/test_tom_m1_host.py.
#define ZK_HOST_BUILD 1
#include <cstring>
#include "curve.h"
#include "coop.h"
#include "comb_digits.h"

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
// projective triple of the a = 1 image -> original-curve affine bytes (k_tom_normalize); a zero Z gives 72 bytes of 0xee
template <int KX, int KY, int KZ>
static void store_triple(const Fe<ModT, KX>& X, const Fe<ModT, KY>& Y, const Fe<ModT, KZ>& Z, uint8_t* out72) {
    Ft2 z = fe_reduce(Z);
    if (fe_is_zero(z)) {
        memset(out72, 0xee, 72);
        return;
    }
    Ft2 zi = fe_inv<ModT>(z);
    auto x = fe_from_mont((X * zi) * fe_const<ModT, 1>(TOM_SINV_M));
    auto y = fe_from_mont(Y * zi);
    uint32_t w[9];
    words_from_limbs<9>(w, x.l);
    words_to_be(w, 9, out72);
    words_from_limbs<9>(w, y.l);
    words_to_be(w, 9, out72 + 36);
}
// the composer's entry of k_tables.hip (MODEL = TOM_MODEL_M1): x'' = s2 X / Z, y' = Z / Y through one inversion of Y Z
static TomNiels m1_entry_of(const TomPt& s) {
    Ft2 wi = fe_inv<ModT>(s.y * s.z);
    Ft2 zz = s.z * s.z, sxy = (s.x * s.y) * fe_const<ModT, 1>(TOM_M1_S_M);
    TomNiels e;
    e.x = (zz - sxy) * wi, e.y = (zz + sxy) * wi;
    e.dt = ((e.y - e.x) * (e.y + e.x)) * fe_const<ModT, 1>(TOM_M1_D2H_M);
    return e;
}
static TomNiels a1_entry_of(const TomPt& s) {
    Ft2 zi = fe_inv<ModT>(s.z);
    TomNiels e;
    e.x = s.x * zi, e.y = s.y * zi;
    e.dt = (e.x * e.y) * fe_const<ModT, 1>(TOM_D1_M);
    return e;
}
template <int MODEL>
static TomNiels entry_of(const TomPt& s) {
    if constexpr (MODEL == TOM_MODEL_M1) return m1_entry_of(s);
    else return a1_entry_of(s);
}
static void fe_words(const Ft2& a, uint8_t* out36) {
    uint32_t w[9];
    words_from_limbs<9>(w, fe_from_mont(a).l);
    words_to_be(w, 9, out36);
}
// the three field elements of P's entry, plain canonical values: 108 bytes per point
extern "C" int ha_m1_entry(uint64_t count, const uint8_t* xy72, uint8_t* out108) {
    for (uint64_t i = 0; i < count; i++) {
        TomPt P;
        if (!tom_load(P, xy72 + 72 * i)) return 1;
        const TomNiels e = m1_entry_of(tom_dbl(tom_dbl(P)));   // an extended point with Z != 1: the entry of 4 P
        fe_words(e.x, out108 + 108 * i), fe_words(e.y, out108 + 108 * i + 36), fe_words(e.dt, out108 + 108 * i + 72);
    }
    return 0;
}
// one product of the model per call: op 0: P + Q (first + add_last);  1: P + Q - R (first, add, negated entry + add_last);  2: P + Q through the general
// addition of two accumulators (add_pts_last);  3: (P + Q) + (Q + R) through add_pts, then + identity entry through add_last
extern "C" int ha_m1_combo(int op, uint64_t count, const uint8_t* p72, const uint8_t* q72, const uint8_t* r72, uint8_t* out72) {
    typedef TomModel<TOM_MODEL_M1> TM;
    for (uint64_t i = 0; i < count; i++) {
        TomPt P, Q, R;
        if (!tom_load(P, p72 + 72 * i) || !tom_load(Q, q72 + 72 * i) || !tom_load(R, r72 + 72 * i)) return 1;
        const TomNiels eP = m1_entry_of(P), eQ = m1_entry_of(Q), eR = m1_entry_of(R), e0 = m1_entry_of(tom_identity());
        TM::Pt acc;
        if (op == 0) acc = TM::add_last(TM::first(TM::entry(eP)), TM::entry(eQ));
        else if (op == 1) acc = TM::add_last(TM::add(TM::first(TM::entry_neg(eP, false)), TM::entry(eQ)), TM::entry_neg(eR, true));
        else if (op == 2) acc = TM::add_pts_last(TM::first(TM::entry(eP)), TM::add(TM::identity(), TM::entry(eQ)));
        else acc = TM::add_last(TM::add_pts(TM::add(TM::first(TM::entry(eP)), TM::entry(eQ)), TM::add(TM::first(TM::entry(eQ)), TM::entry(eR))), TM::entry(e0));
        store_triple(acc.x, acc.y, acc.z, out72 + 72 * i);
    }
    return 0;
}

// ---------------------------------------------------------------- whole comb sums v * g + r * h
struct Base {
    TomPt win[32];   // 2^(bits w) P
};
static void base_init(Base& b, const TomPt& P, uint32_t bits, uint32_t nwin) {
    TomPt p = P;
    for (uint32_t w = 0; w < nwin; w++) {
        b.win[w] = p;
        for (uint32_t i = 0; i < bits; i++) p = tom_dbl(p);
    }
}
template <int MODEL>
static TomNiels comb_entry(const Base& b, uint32_t w, uint32_t d, uint32_t bits) {   // entry[w][d] = d * 2^(bits w) P
    TomPt acc = tom_identity();
    for (int k = (int)bits - 1; k >= 0; k--) {
        acc = tom_dbl(acc);
        if ((d >> k) & 1) acc = tom_add(acc, b.win[w]);
    }
    return entry_of<MODEL>(acc);
}
static CoTom co_from(const TomNiels& e, const uint32_t (&row3)[NLIMB]) {
    CoTom c;
    c.v = co_load4<ModT, 2>(e.x.l, e.y.l, e.dt.l, row3);
    return c;
}
// shape 0: one lane (k_tom_commit / tom_comb_acc);  1: four partial sums and two rounds of general additions (k_tom_commit_wide);  2: rows of a wave, four partial
// sums joined one after the other (k_tom_commit_co).  bits: 8..24 (unsigned digits).
template <int MODEL>
static int comb_commit(int shape, uint32_t bits, const TomPt& G, const TomPt& H, uint64_t count, const uint8_t* v32, const uint8_t* r32, uint8_t* out72) {
    typedef TomModel<MODEL> TM;
    const uint32_t nwin = (256 + bits - 1) / bits;
    if (nwin > 32 || bits > 24) return 2;
    static Base bg, bh;
    base_init(bg, G, bits, nwin), base_init(bh, H, bits, nwin);
    for (uint64_t i = 0; i < count; i++) {
        uint32_t dv[32], dr[32];
        {
            CombDigits a, b;
            a.init(bits), b.init(bits);
            be_to_words(v32 + 32 * i, 32, a.w, 8), be_to_words(r32 + 32 * i, 32, b.w, 8);
            bool sg;
            for (uint32_t w = 0; w < nwin; w++) a.next(dv[w], sg), b.next(dr[w], sg);
        }
        if (shape == 0) {
            typename TM::Pt acc = TM::identity();
            for (uint32_t w = 0; w < nwin; w++) {
                const auto cg = TM::entry(comb_entry<MODEL>(bg, w, dv[w], bits));
                acc = w == 0 ? TM::first(cg) : TM::add(acc, cg);
                const auto ch = TM::entry(comb_entry<MODEL>(bh, w, dr[w], bits));
                acc = w + 1 == nwin ? TM::add_last(acc, ch) : TM::add(acc, ch);
            }
            store_triple(acc.x, acc.y, acc.z, out72 + 72 * i);
        } else if (shape == 1) {
            const uint32_t per = (nwin + 3) / 4;
            typename TM::Pt part[4];
            for (uint32_t p = 0; p < 4; p++) {
                part[p] = TM::identity();
                for (int pass = 0; pass < 2; pass++)
                    for (uint32_t j = 0; j < per; j++) {
                        const uint32_t w = p * per + j;
                        const bool in = w < nwin;   // windows past the last one add entry 0 of window 0, the identity
                        part[p] = TM::add(part[p], TM::entry(comb_entry<MODEL>(pass ? bh : bg, in ? w : 0, in ? (pass ? dr[w] : dv[w]) : 0, bits)));
                    }
            }
            const auto s01 = TM::add_pts(part[0], part[1]), s23 = TM::add_pts(part[2], part[3]);
            const auto acc = TM::add_pts_last(s01, s23);
            store_triple(acc.x, acc.y, acc.z, out72 + 72 * i);
        } else {
            if (MODEL != TOM_MODEL_M1) return 3;
            const CoU32 mj = co_limbs(ModT::mod);
            const uint32_t per = (nwin + 3) / 4;
            TomNiels idn;
            idn.x = fe_zero<ModT>().as<2>(), idn.y = fe_one_mont<ModT>().as<2>(), idn.dt = fe_zero<ModT>().as<2>();
            CoTom sum;
            for (uint32_t p = 0; p < 4; p++) {
                CoTom acc = co_from(idn, ModT::one);   // (0 : 1 : 0 : 1)
                for (int pass = 0; pass < 2; pass++)
                    for (uint32_t w = p * per; w < p * per + per && w < nwin; w++)
                        acc = co_tom_m1_add_tab(acc, co_from(comb_entry<TOM_MODEL_M1>(pass ? bh : bg, w, pass ? dr[w] : dv[w], bits), TOM_TWO_M).v, mj);
                sum = p ? co_tom_m1_add(sum, acc, mj) : acc;
            }
            sum = co_tom_m1_to_a1(sum, mj);
            Ft2 X, Y, T, Z;
            co_store4(sum.v, X.l, Y.l, T.l, Z.l);
            store_triple(X, Y, Z, out72 + 72 * i);
        }
    }
    return 0;
}
extern "C" int ha_m1_comb(int model, int shape, uint32_t bits, const uint8_t* g72, const uint8_t* h72, uint64_t count, const uint8_t* v32, const uint8_t* r32, uint8_t* out72) {
    TomPt G, H;
    if (!tom_load(G, g72) || !tom_load(H, h72)) return 1;
    return model ? comb_commit<TOM_MODEL_M1>(shape, bits, G, H, count, v32, r32, out72) : comb_commit<TOM_MODEL_A1>(shape, bits, G, H, count, v32, r32, out72);
}
