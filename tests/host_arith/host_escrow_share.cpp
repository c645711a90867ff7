// TEST HARNESS (not product code): the threshold opening's arithmetic (zkp-ecdsa_amd/csrc/escrow_share.h: the ZKS1 layout constants, share_respond,
// share_lagrange, share_eval, share_joint_ladder, share_combine_point) compiled for the host CPU with g++ -DZK_HOST_BUILD, beside host_escrow.cpp.  A program
// of its own, so that it runs under -fsanitize=address,undefined: tests/test_escrow_threshold_host.py writes vectors of the Python statement
// (tests/escrow_threshold_common.py) into a file, one case per line, and the program checks every line:
//     layout   size hdr magic pt0 pt2 s blocks                (decimal)
//     respond  c(10) k(32) a_j(32) want(32)                   (hex, big-endian)
//     lagrange at(1) idx(t) want(32 t)
//     eval     j(1) coef(32 t) want(32)
//     combine  idx(t) E2(72) D(72 t) want(72)                 4 (E2 - sum lambda_j D_j), affine
#define ZK_HOST_BUILD 1
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "escrow_share.h"

typedef std::vector<uint8_t> Bytes;
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
static void scalar_store(const Fe<ModQ, 1>& v, uint8_t* be32) {
    uint32_t w[8];
    words_from_limbs<8>(w, v.l);
    words_to_be(w, 8, be32);
}
static bool unhex(const std::string& h, Bytes& out) {
    if (h.size() % 2) return false;
    out.resize(h.size() / 2);
    for (size_t i = 0; i < out.size(); i++) {
        unsigned v;
        if (sscanf(h.c_str() + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}

static bool check_layout(std::istringstream& in) {
    const unsigned long have[7] = {ZKS1_SIZE, ZKS1_HDR, ZK_MAGIC_ZKS1, ZKS1_PT(0), ZKS1_PT(2), ZKS1_S, ZKS1_MSG_BLOCKS};
    for (unsigned long h : have) {
        unsigned long want;
        if (!(in >> want) || want != h) return false;
    }
    return true;
}
static bool check_respond(const std::vector<Bytes>& a) {
    if (a.size() != 4 || a[0].size() != 10 || a[1].size() != 32 || a[2].size() != 32 || a[3].size() != 32) return false;
    uint32_t c3[3];
    be_to_words(a[0].data(), 10, c3, 3);
    uint8_t got[32];
    scalar_store(share_respond(scalar_load(a[1].data()), c3, scalar_load(a[2].data())), got);
    return !memcmp(got, a[3].data(), 32);
}
static bool check_lagrange(const std::vector<Bytes>& a) {
    if (a.size() != 3 || a[0].size() != 1 || a[1].empty() || a[1].size() > ZK_AUDITORS_MAX || a[2].size() != 32 * a[1].size()) return false;
    const uint32_t t = (uint32_t)a[1].size();
    std::vector<uint32_t> idx(a[1].begin(), a[1].end());
    for (uint32_t s = 0; s < t; s++) {
        uint8_t got[32];
        scalar_store(share_lagrange(idx.data(), t, s, a[0][0]), got);
        if (memcmp(got, a[2].data() + 32 * s, 32)) return false;
    }
    return true;
}
static bool check_eval(const std::vector<Bytes>& a) {
    if (a.size() != 3 || a[0].size() != 1 || a[1].empty() || a[1].size() % 32 || a[2].size() != 32) return false;
    const uint32_t t = (uint32_t)(a[1].size() / 32);
    uint8_t got[32];
    scalar_store(share_eval([&](uint32_t i) { return scalar_load(a[1].data() + 32 * i); }, t, a[0][0]), got);
    return !memcmp(got, a[2].data(), 32);
}
static bool check_combine(const std::vector<Bytes>& a) {
    if (a.size() != 4 || a[0].empty() || a[0].size() > ZK_AUDITORS_MAX || a[1].size() != 72 || a[2].size() != 72 * a[0].size() || a[3].size() != 72) return false;
    const uint32_t t = (uint32_t)a[0].size();
    std::vector<uint32_t> idx(a[0].begin(), a[0].end()), lam(8 * t), tab(27 * t);
    const ShareTab T{tab.data(), 1};
    TomPt e2, d;
    if (!tom_load(e2, a[1].data())) return false;
    for (uint32_t s = 0; s < t; s++) {
        if (!tom_load(d, a[2].data() + 72 * s)) return false;
        share_tab_put(T, s, d);
        words_from_limbs<8>(lam.data() + 8 * s, share_lagrange(idx.data(), t, s, 0).l);
    }
    uint8_t got[72];
    tom_store(share_combine_point(e2, share_joint_ladder(T, lam.data(), t)), got);
    return !memcmp(got, a[3].data(), 72);
}

int main(int argc, char** argv) {
    static_assert(ZKS1_SIZE == 264 && ZKS1_S + 32 == ZKS1_SIZE && ZKS1_PT(2) + 72 == ZKS1_S && ZKS1_MSG_POINTS * 67 + 9 <= ZKS1_MSG_BLOCKS * 64, "ZKS1 layout");
    if (argc != 2) return printf("usage: host_escrow_share VECTORS\n"), 2;
    std::ifstream f(argv[1]);
    if (!f) return printf("cannot read %s\n", argv[1]), 2;
    std::string line;
    int n = 0, bad = 0, kinds[5] = {};
    while (std::getline(f, line)) {
        std::istringstream in(line);
        std::string kind, tok;
        if (!(in >> kind)) continue;
        n++;
        bool ok = false;
        if (kind == "layout") ok = check_layout(in), kinds[0]++;
        else {
            std::vector<Bytes> a;
            bool parsed = true;
            while (in >> tok) {
                a.emplace_back();
                parsed = unhex(tok, a.back()) && parsed;
            }
            if (kind == "respond") ok = parsed && check_respond(a), kinds[1]++;
            else if (kind == "lagrange") ok = parsed && check_lagrange(a), kinds[2]++;
            else if (kind == "eval") ok = parsed && check_eval(a), kinds[3]++;
            else if (kind == "combine") ok = parsed && check_combine(a), kinds[4]++;
        }
        if (!ok) bad++, printf("line %d (%s) differs from the Python statement\n", n, kind.c_str());
    }
    for (int k : kinds)
        if (!k) bad++, printf("a kind of vector is missing\n");
    if (bad) printf("host_escrow_share: %d failures\n", bad);
    else printf("host_escrow_share: ok (%d vectors)\n", n);
    return bad ? 1 : 0;
}
