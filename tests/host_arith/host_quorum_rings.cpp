// TEST HARNESS (not product code): the capacity rule of the quorum calls with one ring id per member (zkp-ecdsa_amd/csrc/quorum_plan.h: QuorumRings,
// zkq_ring_entry, zkq_capacity_rings, zkq_max_size_rings) compiled for the host CPU with plain g++ -- the function the kernel (k_quorum.hip: k_q_caps) and
// the host-pointer call (api_quorum.hip) both run.  A program of its own (tests/test_quorum_rings_host.py builds it with -fsanitize=address,undefined): the
// id arrays are heap allocations of exactly k entries, so a read past the k-th id is an error the sanitizer reports.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "quorum_plan.h"

#define CHECK(x)                                                         \
    do {                                                                 \
        if (!(x)) {                                                      \
            printf("host_quorum_rings: FAILED %s (line %d)\n", #x, __LINE__); \
            return 1;                                                    \
        }                                                                \
    } while (0)

static QuorumRings table(const std::vector<uint32_t>& id, const std::vector<uint32_t>& resident, const std::vector<uint32_t>& proof_max) {
    QuorumRings R{};
    R.count = (uint32_t)id.size();
    for (uint32_t r = 0; r < R.count; r++) R.id[r] = id[r], R.resident[r] = resident[r], R.proof_max[r] = proof_max[r];
    return R;
}
static uint64_t cap(const QuorumRings& R, const std::vector<uint32_t>& ids, uint32_t* used = nullptr) {
    return zkq_capacity_rings(R, (uint32_t)ids.size(), ids.data(), used);
}
static uint64_t fixed(uint32_t k) { return 16 + 744ull * (k * (k - 1) / 2); }

int main() {
    // three entries: rings 7 and 3 resident with different sizes, ring 9 known but not resident (no keys, or no params)
    const QuorumRings R = table({7, 3, 9}, {1, 1, 0}, {1000, 5000, 77});
    CHECK(zkq_ring_entry(R, 7) == 0 && zkq_ring_entry(R, 3) == 1 && zkq_ring_entry(R, 9) == ZKQ_RINGS && zkq_ring_entry(R, 0) == ZKQ_RINGS);
    // k = 2 and k = 16, mixed and with all ids equal
    uint32_t used = 0;
    CHECK(cap(R, {7, 3}, &used) == fixed(2) + 6000 && used == 3);
    used = 0;
    CHECK(cap(R, {3, 3}, &used) == fixed(2) + 10000 && used == 2);
    CHECK(zkq_max_size_rings(R, 2, std::vector<uint32_t>{7, 3}.data()) == fixed(2) + 6000);
    {
        std::vector<uint32_t> ids(16), same(16, 7);
        for (uint32_t i = 0; i < 16; i++) ids[i] = i % 2 ? 3 : 7;
        used = 0;
        CHECK(cap(R, ids, &used) == fixed(16) + 8 * 6000 && fixed(16) == 16 + 744 * 120 && used == 3);
        used = 0;
        CHECK(cap(R, same, &used) == fixed(16) + 16 * 1000 && used == 1);
        CHECK(cap(R, same) == zkq_max_size(16, 1000));   // all ids equal: the one-ring rule
        CHECK(zkq_max_size_rings(R, 16, ids.data()) == cap(R, ids));
        ids[15] = 9;   // the last id not resident: counts 0 in the slot, and the max size is 0
        used = 0;
        CHECK(cap(R, ids, &used) == fixed(16) + 8 * 1000 + 7 * 5000 && used == 3 && zkq_max_size_rings(R, 16, ids.data()) == 0);
    }
    // one id missing: unknown, or known and not resident, at every place of a quorum of three
    for (uint32_t at = 0; at < 3; at++)
        for (uint32_t gone : {9u, 12345u, 0xffffffffu}) {
            std::vector<uint32_t> ids = {7, 3, 7};
            const uint32_t lost = R.proof_max[zkq_ring_entry(R, ids[at])];
            ids[at] = gone;
            CHECK(cap(R, ids) == fixed(3) + 7000 - lost && zkq_max_size_rings(R, 3, ids.data()) == 0);
        }
    used = 0;
    CHECK(cap(R, {9, 12345}, &used) == fixed(2) && used == 0);
    // k outside 2..16: no slot
    CHECK(cap(R, {7}) == 0 && cap(R, std::vector<uint32_t>(17, 7)) == 0 && zkq_capacity_rings(R, 0, nullptr, nullptr) == 0);
    CHECK(zkq_max_size_rings(R, 1, std::vector<uint32_t>{7}.data()) == 0 && zkq_max_size_rings(R, 17, std::vector<uint32_t>(17, 7).data()) == 0);
    // sums near 2^32 per slot: sixteen members of a ring whose largest proof takes 2^32 - 1 bytes
    {
        const QuorumRings big = table({1, 2}, {1, 1}, {0xffffffffu, 0x10000000u});
        CHECK(cap(big, {1, 2}) == fixed(2) + 0xffffffffull + 0x10000000ull);          // just above 2^32
        CHECK(cap(big, std::vector<uint32_t>(16, 2)) == fixed(16) + 0x100000000ull);   // 16 x 2^28 = 2^32 exactly, plus the fixed part
        CHECK(cap(big, std::vector<uint32_t>(16, 1)) == fixed(16) + 16 * 0xffffffffull);
        CHECK(cap(big, std::vector<uint32_t>(15, 2)) == fixed(15) + 0xf0000000ull && cap(big, std::vector<uint32_t>(15, 2)) < 0x100000000ull);
    }
    // a full table of sixteen entries: the last one is found, an id behind it is not; a resident ring with no size (no params) gives max size 0
    {
        QuorumRings full{};
        full.count = ZKQ_RINGS;
        for (uint32_t r = 0; r < ZKQ_RINGS; r++) full.id[r] = 100 + r, full.resident[r] = 1, full.proof_max[r] = 10 * (r + 1);
        used = 0;
        CHECK(cap(full, {115, 100}, &used) == fixed(2) + 170 && used == 0x8001u && zkq_ring_entry(full, 116) == ZKQ_RINGS);
        full.proof_max[3] = 0;
        CHECK(zkq_max_size_rings(full, 2, std::vector<uint32_t>{103, 100}.data()) == 0 && cap(full, {103, 100}) == fixed(2) + 10);
    }
    printf("host_quorum_rings: ok\n");
    return 0;
}
