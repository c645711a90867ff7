// TEST HARNESS (not product code): the resident point index (zkp-ecdsa_amd/csrc/escrow_index.h: the slot function, esc_index_insert, esc_index_lookup)
// compiled for the host CPU with g++ -DZK_HOST_BUILD, where the two atomics are their one-thread statements.  Built as a shared library and driven against
// the Python restatement by tests/test_escrow_index_host.py; with -DHOST_ESCROW_INDEX_MAIN it is a program of its own (the slot function against values
// computed in Python, and insert-then-lookup over synthetic points against a brute-force scan: a cluster that wraps from the last slot to slot 0, equal
// points at several indices under every insertion order, a table at its fullest allowed load, absent points, stale entries behind the key count), so that
// the same source runs under -fsanitize=address,undefined.
#define ZK_HOST_BUILD 1
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>
#include "escrow_index.h"

// A table over caller-owned points.  pts: [18][cap] limb-major; nkeys <= cap; order: the sequence in which the keys are inserted (a permutation of 0 .. nkeys-1).
struct HostIndex {
    std::vector<uint32_t> slots;
    EscIndexRing R;
    HostIndex(const uint32_t* pts, uint32_t nkeys, const uint32_t* order) : slots(2 * (size_t)esc_index_cap(nkeys), ESC_INDEX_EMPTY) {
        R.id = 0, R.nkeys = nkeys, R.mask = (uint32_t)slots.size() - 1, R.pts = pts, R.slots = slots.data();
        for (uint32_t k = 0; k < nkeys; k++) esc_index_insert(R, order ? order[k] : k);
    }
};

extern "C" uint32_t hei_cap(uint64_t nkeys) { return esc_index_cap(nkeys); }
extern "C" uint32_t hei_hash(uint32_t w0, uint32_t w1) { return esc_index_hash(w0, w1); }
extern "C" uint32_t hei_home(uint32_t l0, uint32_t l1, uint32_t l2, uint32_t mask) { return esc_index_home(l0, l1, l2, mask); }
// builds the table over pts ([18][cap(nkeys)]) in the given order, copies the slots out, and looks up nq points q ([nq][18]: x limbs, y limbs)
extern "C" int hei_build_lookup(const uint32_t* pts, uint32_t nkeys, const uint32_t* order, uint32_t* slots_out, const uint32_t* q, uint32_t nq, uint32_t* found) {
    HostIndex H(pts, nkeys, order);
    if (slots_out) memcpy(slots_out, H.slots.data(), 4 * H.slots.size());
    for (uint32_t i = 0; i < nq; i++) found[i] = esc_index_lookup(H.R, q + 18 * (size_t)i, q + 18 * (size_t)i + 9);
    return 0;
}

#ifdef HOST_ESCROW_INDEX_MAIN
// (l0, l1, l2 of x, the hash, the home slot in tables of 4, 16 and 2^21 slots) computed by tests/escrow_index_common.py for x = 0, 1, 2^64 - 1, 2^32,
// 2^30 - 1, 2^30, 2^60 + 2^31, 2^270 - 1 (only bits 0..63 count: the same slot as 2^64 - 1) and eight random 270-bit values
static const uint32_t PY_SLOTS[16][7] = {
    {0x00000000u, 0x00000000u, 0x00000000u, 0x00000000u, 0u, 0u, 0u},
    {0x00000001u, 0x00000000u, 0x00000000u, 0x481e425eu, 2u, 14u, 1983070u},
    {0x3fffffffu, 0x3fffffffu, 0x0000000fu, 0xa4f0dc37u, 3u, 7u, 1104951u},
    {0x00000000u, 0x00000004u, 0x00000000u, 0xf0c7f383u, 3u, 3u, 521091u},
    {0x3fffffffu, 0x00000000u, 0x00000000u, 0x532969acu, 0u, 12u, 616876u},
    {0x00000000u, 0x00000001u, 0x00000000u, 0xeb8a1c6au, 2u, 10u, 662634u},
    {0x00000000u, 0x00000002u, 0x00000001u, 0x70aa754fu, 3u, 15u, 685391u},
    {0x3fffffffu, 0x3fffffffu, 0x3fffffffu, 0xa4f0dc37u, 3u, 7u, 1104951u},
    {0x1cc99396u, 0x0bb59bffu, 0x26ae768fu, 0x5ddbf83cu, 0u, 12u, 1833020u},
    {0x066de486u, 0x3d591949u, 0x3faac572u, 0x96fefabcu, 0u, 12u, 2030268u},
    {0x12e4016eu, 0x0d75f4eeu, 0x003031ecu, 0x29f0f86eu, 2u, 14u, 1112174u},
    {0x2e09e4b8u, 0x18faf0e0u, 0x307a2235u, 0xba35e257u, 3u, 7u, 1434199u},
    {0x2b195b47u, 0x0453c9fau, 0x3d43e94au, 0x37d84baau, 2u, 10u, 1592234u},
    {0x01090aeeu, 0x069f8db8u, 0x029392b5u, 0x1d131ca4u, 0u, 4u, 1252516u},
    {0x24ffc604u, 0x1d518531u, 0x22162b36u, 0xe9b962cbu, 3u, 11u, 1663691u},
    {0x0f4c6fc3u, 0x3084f04au, 0x098d7d67u, 0x8611f236u, 2u, 6u, 1176118u},
};
struct Pt {
    uint32_t l[18];
    bool operator==(const Pt& o) const { return !memcmp(l, o.l, sizeof l); }
};
static uint32_t g_lcg = 12345;
static uint32_t rnd30() {
    g_lcg = g_lcg * 1664525u + 1013904223u;
    return (g_lcg >> 2) & 0x3fffffffu;
}
// a synthetic point whose home slot in a table of mask + 1 slots is `slot` (any slot for mask = 0xffffffff), distinct for distinct tags
static Pt make_point(uint32_t slot, uint32_t mask, uint32_t tag) {
    Pt p;
    for (int i = 0; i < 18; i++) p.l[i] = rnd30();
    p.l[17] = tag;
    if (mask != 0xffffffffu)
        while (esc_index_home(p.l[0], p.l[1], p.l[2], mask) != slot) p.l[0] = (p.l[0] + 1) & 0x3fffffffu;
    return p;
}
static std::vector<uint32_t> limb_major(const std::vector<Pt>& v, uint32_t cap) {   // [18][cap], exactly: the sanitizer sees every read past an entry
    std::vector<uint32_t> m(18 * (size_t)cap, 0);
    for (size_t i = 0; i < v.size(); i++)
        for (int l = 0; l < 18; l++) m[(size_t)l * cap + i] = v[i].l[l];
    return m;
}
static uint32_t brute(const std::vector<Pt>& v, uint32_t nkeys, const Pt& q) {
    for (uint32_t i = 0; i < nkeys; i++)
        if (v[i] == q) return i;
    return ESC_INDEX_EMPTY;
}
// every key and every extra query against the brute-force scan, for the table built in `order`; also: every distinct point owns exactly one slot
static int check(const char* what, const std::vector<Pt>& v, uint32_t nkeys, const uint32_t* order, const std::vector<Pt>& extra, std::vector<uint32_t>* slots_out = nullptr) {
    const uint32_t cap = esc_index_cap(nkeys);
    const std::vector<uint32_t> pts = limb_major(v, cap);
    HostIndex H(pts.data(), nkeys, order);
    int bad = 0;
    std::vector<Pt> qs(v.begin(), v.end());
    qs.insert(qs.end(), extra.begin(), extra.end());
    for (const Pt& q : qs)
        if (esc_index_lookup(H.R, q.l, q.l + 9) != brute(v, nkeys, q)) bad++;
    uint32_t used = 0, distinct = 0;
    for (uint32_t s : H.slots)
        if (s != ESC_INDEX_EMPTY) {
            used++;
            if (s >= nkeys || brute(v, nkeys, v[s]) != s) bad++;   // a slot holds the LOWEST index of its point
        }
    for (uint32_t i = 0; i < nkeys; i++) distinct += brute(v, nkeys, v[i]) == i;
    if (used != distinct) bad++;
    if (bad) printf("%s: %d mismatches\n", what, bad);
    if (slots_out) *slots_out = H.slots;
    return bad;
}
int main() {
    int bad = 0;
    for (const auto& r : PY_SLOTS) {
        const uint32_t w0 = r[0] | (r[1] << 30), w1 = (r[1] >> 2) | (r[2] << 28);
        if (esc_index_hash(w0, w1) != r[3] || esc_index_home(r[0], r[1], r[2], 3) != r[4] || esc_index_home(r[0], r[1], r[2], 15) != r[5] ||
            esc_index_home(r[0], r[1], r[2], (1u << 21) - 1) != r[6])
            bad++, printf("slot function differs from the Python value for x limbs %08x %08x %08x\n", r[0], r[1], r[2]);
    }
    if (esc_index_cap(2) != 2 || esc_index_cap(5) != 8 || esc_index_cap(256) != 256 || esc_index_cap(257) != 512 || esc_index_cap(600) != 1024) bad++, printf("esc_index_cap\n");

    // 1. a cluster that wraps: 8 keys, 16 slots, four distinct points at home slot 15, one at 14, one at 0, two at 7.  Whatever the order, slots 14, 15, 0 .. 3
    // are taken and 4 is empty; an absent point at home 15 walks 15, 0, 1, 2, 3 and ends at the empty slot 4.
    {
        std::vector<Pt> v = {make_point(15, 15, 0), make_point(7, 15, 1), make_point(15, 15, 2), make_point(14, 15, 3),
                             make_point(15, 15, 4), make_point(0, 15, 5), make_point(15, 15, 6), make_point(7, 15, 7)};
        const std::vector<Pt> absent = {make_point(15, 15, 100), make_point(14, 15, 101), make_point(0, 15, 102), make_point(7, 15, 103), make_point(9, 15, 104)};
        uint32_t order[8] = {0, 1, 2, 3, 4, 5, 6, 7};
        int orders = 0;
        do {   // every insertion order: 8! tables
            std::vector<uint32_t> slots;
            bad += check("wrap cluster", v, 8, order, absent, &slots);
            for (uint32_t s : {14u, 15u, 0u, 1u, 2u, 3u, 7u, 8u})
                if (slots[s] == ESC_INDEX_EMPTY) bad++;
            if (slots[4] != ESC_INDEX_EMPTY || slots[9] != ESC_INDEX_EMPTY) bad++;
            orders++;
        } while (std::next_permutation(order, order + 8));
        if (orders != 40320) bad++;
    }
    // 2. equal points at several indices: the lowest index wins under every insertion order tried (all 5040 of 7 keys); the copies share the wrapped cluster
    {
        std::vector<Pt> v = {make_point(15, 15, 0), make_point(15, 15, 1), make_point(15, 15, 2), make_point(3, 15, 3)};
        v.push_back(v[1]), v.push_back(v[3]), v.push_back(v[1]);   // 4 = 1, 5 = 3, 6 = 1
        uint32_t order[7] = {0, 1, 2, 3, 4, 5, 6};
        do bad += check("equal points", v, 7, order, {make_point(15, 15, 200)});
        while (std::next_permutation(order, order + 7));
        const std::vector<uint32_t> pts = limb_major(v, 8);
        const uint32_t rev[7] = {6, 5, 4, 3, 2, 1, 0};
        HostIndex H(pts.data(), 7, rev);
        if (esc_index_lookup(H.R, v[6].l, v[6].l + 9) != 1 || esc_index_lookup(H.R, v[5].l, v[5].l + 9) != 3) bad++, printf("the lowest index did not win\n");
    }
    // 3. the fullest allowed load: nkeys = entries, so half the slots are taken -- 2 keys in 4 slots, 8 in 16 (all at one home slot: the longest cluster), 256 in 512
    {
        std::vector<Pt> two = {make_point(3, 3, 0), make_point(3, 3, 1)};
        bad += check("2 keys", two, 2, nullptr, {make_point(3, 3, 2), make_point(0, 3, 3)});
        std::vector<Pt> eight;
        for (uint32_t i = 0; i < 8; i++) eight.push_back(make_point(12, 15, i));
        bad += check("8 keys at one home slot", eight, 8, nullptr, {make_point(12, 15, 50), make_point(11, 15, 51), make_point(4, 15, 52)});
        std::vector<Pt> many, absent;
        for (uint32_t i = 0; i < 256; i++) many.push_back(make_point(0, 0xffffffffu, i));
        for (uint32_t i = 0; i < 256; i++) absent.push_back(make_point(0, 0xffffffffu, 1000 + i));
        std::vector<uint32_t> order(256);
        for (uint32_t i = 0; i < 256; i++) order[i] = (i * 77 + 5) & 255;
        bad += check("256 keys", many, 256, order.data(), absent);
    }
    // 4. 600 keys in 1024 entries with repeats, a shuffled order; the entries behind the key count hold points that must never match
    {
        std::vector<Pt> v;
        for (uint32_t i = 0; i < 600; i++) v.push_back(i % 7 == 3 && i > 50 ? v[i - 50] : make_point(0, 0xffffffffu, i));
        std::vector<Pt> stale;
        for (uint32_t i = 600; i < 1024; i++) stale.push_back(make_point(0, 0xffffffffu, i));
        std::vector<Pt> all = v;
        all.insert(all.end(), stale.begin(), stale.end());
        std::vector<uint32_t> order(600);
        for (uint32_t i = 0; i < 600; i++) order[i] = (i * 7 + 3) % 600;
        bad += check("600 keys", all, 600, order.data(), stale);
        // a stale index in a slot (no insertion writes one) is stepped over, not followed
        const std::vector<uint32_t> pts = limb_major(all, 1024);
        HostIndex H(pts.data(), 600, nullptr);
        const uint32_t s = esc_index_home(stale[0].l[0], stale[0].l[1], stale[0].l[2], H.R.mask);
        H.slots[s] = 600;
        if (esc_index_lookup(H.R, stale[0].l, stale[0].l + 9) != ESC_INDEX_EMPTY) bad++, printf("an entry behind the key count matched\n");
        H.slots[s] = 0x7fffffffu;
        if (esc_index_lookup(H.R, stale[0].l, stale[0].l + 9) != ESC_INDEX_EMPTY) bad++, printf("an index outside the points was followed\n");
    }
    // 5. a full table (never built: the load is at most 1/2) still ends every probe sequence: the loops are bounded by the slot count
    {
        std::vector<Pt> v = {make_point(1, 3, 0), make_point(2, 3, 1)};
        const std::vector<uint32_t> pts = limb_major(v, 2);
        HostIndex H(pts.data(), 2, nullptr);
        for (uint32_t& s : H.slots) s = 0;
        const Pt q = make_point(2, 3, 9);
        if (esc_index_lookup(H.R, q.l, q.l + 9) != ESC_INDEX_EMPTY) bad++, printf("full table\n");
        esc_index_insert(H.R, 1);   // no empty slot and no equal occupant: returns after one round
    }
    if (bad) printf("host_escrow_index: %d failures\n", bad);
    else printf("host_escrow_index: ok\n");
    return bad ? 1 : 0;
}
#endif
