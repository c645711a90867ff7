// TEST HARNESS (not product code): the quorum proofs' plan (zkp-ecdsa_amd/csrc/quorum_plan.h: zkq_rank, zkq_unrank, zkq_pairs, zkq_max_size, zkq_size,
// zkq_header, zkq_walk) compiled for the host CPU with plain g++.  Built as a shared library and driven by tests/test_quorum_host.py; with
// -DHOST_QUORUM_MAIN it is a program of its own (the pair order for every k, the sizes, the header walk over hand-made bundles that end exactly at the end
// of their allocation), so that the same source runs under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "quorum_plan.h"

extern "C" {
uint32_t hq_pairs(uint32_t k) { return zkq_pairs(k); }
uint32_t hq_rank(uint32_t k, uint32_t i, uint32_t j) { return zkq_rank(k, i, j); }
void hq_unrank(uint32_t k, uint32_t p, uint32_t* ij) { zkq_unrank(k, p, ij[0], ij[1]); }
uint64_t hq_max_size(uint32_t k, uint64_t proof_max) { return zkq_max_size(k, proof_max); }
uint64_t hq_size(uint32_t k, uint64_t att_bytes) { return zkq_size(k, att_bytes); }
void hq_header(uint32_t total, uint32_t k, uint8_t* out16) {
    uint32_t hw[4];
    zkq_header(hw, total, k);
    memcpy(out16, hw, 16);
}
// -> 1 / 0; m_off: k + 1 entries
int hq_walk(const uint8_t* bundles, uint64_t o0, uint64_t o1, uint32_t k, int packed, uint64_t* m_off) { return zkq_walk(bundles, o0, o1, k, wire_make(packed != 0), m_off) ? 1 : 0; }
uint32_t hq_min_member(int packed, uint32_t n) {   // the shortest proof rr_head accepts for n index bits
    const Wire w = wire_make(packed != 0);
    return w.fixed + w.gk_n * n + 32;
}
}

#ifdef HOST_QUORUM_MAIN
#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) {                                                \
            printf("host_quorum: FAILED %s (line %d)\n", #x, __LINE__); \
            return 1;                                              \
        }                                                          \
    } while (0)
// a bundle of k members of the given lengths (headers only; the rest zero) in an allocation of exactly its size
static std::vector<uint8_t> bundle(uint32_t k, const std::vector<uint32_t>& lens, bool packed, uint32_t n) {
    uint64_t att = 0;
    for (uint32_t l : lens) att += l;
    std::vector<uint8_t> b(zkq_size(k, att), 0);
    hq_header((uint32_t)b.size(), k, b.data());
    size_t pos = ZKQ1_HDR;
    for (uint32_t l : lens) {
        const uint32_t hw[4] = {wire_make(packed).magic, __builtin_bswap32(l), __builtin_bswap32(20u), __builtin_bswap32(n)};
        memcpy(b.data() + pos, hw, 16);
        pos += l;
    }
    return b;
}
int main() {
    for (uint32_t k = 0; k <= 18; k++) {
        const uint32_t P = zkq_pairs(k);
        CHECK(P == (k >= 2 && k <= 16 ? k * (k - 1) / 2 : 0));
        uint32_t p = 0;
        for (uint32_t i = 0; i < k && P; i++)
            for (uint32_t j = i + 1; j < k; j++, p++) {
                uint32_t a, b;
                zkq_unrank(k, p, a, b);
                CHECK(a == i && b == j && zkq_rank(k, i, j) == p);
            }
        CHECK(p == P);
    }
    CHECK(zkq_max_size(3, 1000) == 16 + 3000 + 3 * 744 && zkq_max_size(1, 1000) == 0 && zkq_max_size(17, 1000) == 0 && zkq_max_size(3, 0) == 0);
    for (int packed = 0; packed < 2; packed++) {
        const uint32_t n = 3, m = hq_min_member(packed, n);
        uint64_t off[4];
        std::vector<uint8_t> b = bundle(3, {m, m + 8, m + 4}, packed, n);
        CHECK(zkq_walk(b.data(), 0, b.size(), 3, wire_make(packed), off));
        CHECK(off[0] == 16 && off[1] == 16 + m && off[2] == 16 + 2 * m + 8 && off[3] == b.size() - 3 * 744);
        CHECK(zkq_walk(b.data(), 0, b.size(), 3, wire_make(packed), nullptr));
        CHECK(!zkq_walk(b.data(), 0, b.size(), 3, wire_make(!packed), off));      // the other layout's magic
        CHECK(!zkq_walk(b.data(), 0, b.size(), 2, wire_make(packed), off) && !zkq_walk(b.data(), 0, b.size(), 4, wire_make(packed), off));
        CHECK(!zkq_walk(b.data(), 0, b.size() - 1, 3, wire_make(packed), off));   // one byte short
        CHECK(!zkq_walk(b.data(), 0, b.size() - 4, 3, wire_make(packed), off));
        CHECK(!zkq_walk(b.data(), 4, b.size(), 3, wire_make(packed), off));
        {   // an inner total_len that overruns: the last member claims the pairs' bytes and more
            std::vector<uint8_t> c = b;
            const uint32_t len = __builtin_bswap32((uint32_t)(c.size()));
            memcpy(c.data() + off[2] + 4, &len, 4);
            CHECK(!zkq_walk(c.data(), 0, c.size(), 3, wire_make(packed), off));
        }
        {   // an inner total_len that is no multiple of 4, made up by the next member
            std::vector<uint8_t> c = bundle(3, {m + 2, m + 2, m + 4}, packed, n);
            CHECK(!zkq_walk(c.data(), 0, c.size(), 3, wire_make(packed), off));
        }
        {   // a member too short for the GKProof its n announces
            std::vector<uint8_t> c = bundle(3, {m, m - 4, m}, packed, n);
            CHECK(!zkq_walk(c.data(), 0, c.size(), 3, wire_make(packed), off));
        }
        {   // nothing but the header and the pairs: the walk stops at the first member without reading past the slot
            std::vector<uint8_t> c = bundle(2, {}, packed, n);
            CHECK(c.size() == 16 + 744 && !zkq_walk(c.data(), 0, c.size(), 2, wire_make(packed), off));
            std::vector<uint8_t> d(16);
            hq_header(16, 2, d.data());
            CHECK(!zkq_walk(d.data(), 0, 16, 2, wire_make(packed), off) && !zkq_walk(d.data(), 0, 12, 2, wire_make(packed), off));
        }
    }
    printf("host_quorum: ok\n");
    return 0;
}
#endif
