// csrc/member_plan.h on the host: the index arithmetic of a mixed-ring membership call, against a direct restatement.  Over a seeded sweep of class mixes --
// empty classes, classes of one proof, batches of the census workgroup's size and one proof either side of it, ids that are not resident --: the size of
// every class, the offsets of every proof (zero-length slots for ids that are not resident), the offsets as the device computes them (a workgroup's first
// offset from the per-class counts of the workgroups before it, then a scan inside the workgroup), the window cuts (every proof of a class exactly once, in
// order, no window above the cap), the out_cap decision and the verifier's slot rule.  Built with the sanitizers by tests/test_member_rings_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "member_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            failures++;                        \
            fprintf(stderr, "FAIL %s: ", name); \
            fprintf(stderr, __VA_ARGS__);      \
            fprintf(stderr, "\n");             \
        }                                      \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t below) {   // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) % below);
}
static uint64_t size_of_n(uint32_t n) { return 16 + 288ull * n + 32ull * (3 * n + 1); }   // include/zkattest.h

// one mix: `rings` resident rings of the given n, ids[b] in 0 .. rings-1 for ring b's id 100 + 7 r, or any other value for an id that is not resident
static void run(const char* name, const std::vector<uint32_t>& ns, const std::vector<uint32_t>& ids, uint32_t chunk, uint32_t lanes) {
    const uint64_t B = ids.size();
    MrRings R;
    mr_rings_clear(R);
    for (size_t r = 0; r < ns.size(); r++) mr_rings_add(R, 100 + 7 * (uint32_t)r, ns[r]);
    CHECK(R.count == ns.size() && R.size[MR_UNKNOWN] == 0 && R.size[MR_BAD] == 0, "%u rings", R.count);
    // ---- direct restatement: class, size and offset of every proof
    std::vector<uint32_t> want_cls(B);
    std::vector<uint64_t> want_off(B + 1, 0);
    std::vector<std::vector<uint32_t>> members(MR_CLASSES);
    for (uint64_t b = 0; b < B; b++) {
        uint32_t k = MR_UNKNOWN;
        for (size_t r = 0; r < ns.size(); r++)
            if (ids[b] == 100 + 7 * r) k = (uint32_t)r;
        want_cls[b] = k;
        members[k].push_back((uint32_t)b);
        want_off[b + 1] = want_off[b] + (k == MR_UNKNOWN ? 0 : size_of_n(ns[k]));
    }
    for (size_t r = 0; r < ns.size(); r++) CHECK(R.size[r] == size_of_n(ns[r]), "ring %zu: size %u", r, R.size[r]);
    // ---- the host plan
    std::vector<uint8_t> cls(B + 1, 0xee);
    std::vector<uint64_t> off(B + 2, ~0ull);
    uint32_t cnt[MR_CLASSES];
    mr_plan_host(R, B, ids.data(), cls.data(), cnt, off.data());
    CHECK(cls[B] == 0xee && off[B + 1] == ~0ull, "the plan wrote past its arrays");
    for (uint64_t b = 0; b < B; b++) CHECK(cls[b] == want_cls[b] && off[b] == want_off[b], "proof %llu: class %u at %llu", (unsigned long long)b, cls[b], (unsigned long long)off[b]);
    CHECK(off[B] == want_off[B], "total %llu, not %llu", (unsigned long long)off[B], (unsigned long long)want_off[B]);
    for (uint32_t k = 0; k < MR_CLASSES; k++) CHECK(cnt[k] == members[k].size(), "class %u: %u proofs", k, cnt[k]);
    CHECK(mr_bytes(cnt, R) == want_off[B], "mr_bytes of the totals");
    // ---- the device's way: per workgroup of MR_BLOCK proofs, the per-class counts of the workgroups before it give its first offset
    {
        uint32_t before[MR_CLASSES] = {};
        for (uint64_t b0 = 0; b0 < B; b0 += MR_BLOCK) {
            uint64_t run_ = mr_bytes(before, R);
            for (uint64_t b = b0; b < B && b < b0 + MR_BLOCK; b++) {
                CHECK(run_ == want_off[b], "workgroup %llu: proof %llu at %llu", (unsigned long long)(b0 / MR_BLOCK), (unsigned long long)b, (unsigned long long)run_);
                run_ += R.size[cls[b]];
                before[cls[b]]++;
            }
        }
    }
    // ---- the out_cap decision
    CHECK(mr_fits(want_off[B], want_off[B]) && mr_fits(want_off[B], want_off[B] + 1) && mr_fits(want_off[B], ~0ull), "a buffer that holds the batch is refused");
    if (want_off[B]) CHECK(!mr_fits(want_off[B], want_off[B] - 1) && !mr_fits(want_off[B], 0), "a buffer one byte short is accepted");
    // ---- the fast path's condition
    {
        uint32_t used = 0, last = MR_CLASSES;
        for (size_t r = 0; r < ns.size(); r++)
            if (!members[r].empty()) used++, last = (uint32_t)r;
        const uint32_t want = used == 1 && members[MR_UNKNOWN].empty() ? last : MR_CLASSES;
        CHECK(mr_single_class(cnt, R) == want, "single class %u, not %u", mr_single_class(cnt, R), want);
        uint32_t c2[MR_CLASSES];
        for (uint32_t k = 0; k < MR_CLASSES; k++) c2[k] = cnt[k];
        c2[MR_BAD] = 1;
        CHECK(mr_single_class(c2, R) == MR_CLASSES, "a refused slot beside one class still takes the one-ring path");
    }
    // ---- windows: every proof of every class exactly once, in order; no window above the cap; the cap is min(2 x chunk x lanes, the largest class)
    const uint32_t cap = mr_window_cap(chunk, lanes, cnt, R);
    uint32_t most = 1;
    for (size_t r = 0; r < ns.size(); r++) most = std::max<uint32_t>(most, (uint32_t)members[r].size());
    CHECK(cap >= 1 && cap == std::min<uint64_t>(2ull * chunk * lanes, most), "cap %u for chunk %u, lanes %u, largest class %u", cap, chunk, lanes, most);
    std::vector<uint32_t> seen(B, 0);
    for (size_t r = 0; r < ns.size(); r++) {
        const uint32_t n = cnt[r], nw = mr_window_count(n, cap);
        uint32_t next = 0;
        for (uint32_t w = 0; w < nw; w++) {
            uint32_t first, c;
            mr_window(n, cap, w, &first, &c);
            CHECK(first == next && c >= 1 && c <= cap && first + c <= n, "class %zu window %u: [%u, +%u) of %u", r, w, first, c, n);
            for (uint32_t j = first; j < first + c && j < n; j++) seen[members[r][j]]++;
            next = first + c;
        }
        CHECK(next == n, "class %zu: windows end at %u of %u", r, next, n);
        uint32_t first, c;
        mr_window(n, cap, nw, &first, &c);   // one past the last window: empty, inside the class
        CHECK(first == n && c == 0, "class %zu: a window past the last one holds %u proofs from %u", r, c, first);
    }
    for (uint64_t b = 0; b < B; b++) CHECK(seen[b] == (want_cls[b] < MR_SLOTS ? 1u : 0u), "proof %llu entered %u windows", (unsigned long long)b, seen[b]);
    printf("%-34s B %6llu, %2zu rings, %10llu bytes, cap %u\n", name, (unsigned long long)B, ns.size(), (unsigned long long)want_off[B], cap);
}

int main() {
    const char* name = "slot rule";
    // the verifier's slot rule
    CHECK(mr_slot_ok(0, 1200, 1200, 1200) && mr_slot_ok(1200, 2400, 3600, 1200), "an honest slot is refused");
    CHECK(!mr_slot_ok(0, 1196, 1200, 1200) && !mr_slot_ok(0, 1204, 2400, 1200), "a slot of another length");
    CHECK(!mr_slot_ok(2, 1202, 2400, 1200) && !mr_slot_ok(1201, 2401, 2404, 1200), "a misaligned slot");
    CHECK(!mr_slot_ok(1200, 0, 1200, 1200) && !mr_slot_ok(~0ull - 1199 + 1, 0, ~0ull, 1200), "a slot whose end lies before its start");
    CHECK(!mr_slot_ok(1200, 2400, 2399, 1200) && !mr_slot_ok(0, 1200, 0, 1200), "a slot that ends behind the batch");
    CHECK(zkm1_size(3) == 1200 && zkm1_size(5) == 1968 && zkm1_size(9) == 3504 && zkm1_size(16) == size_of_n(16), "ZKM1 sizes");
    const std::vector<uint32_t> three = {3, 9, 5};
    auto cyc = [&](uint64_t B, uint32_t rings, uint32_t unknown_every) {
        std::vector<uint32_t> ids(B);
        for (uint64_t b = 0; b < B; b++) ids[b] = unknown_every && b % unknown_every == unknown_every - 1 ? 5 : 100 + 7 * (uint32_t)(b % rings);
        return ids;
    };
    run("empty batch", three, {}, 4096, 2);
    run("one proof", three, {107}, 4096, 2);
    run("24 interleaved, one unknown", three, cyc(24, 3, 14), 4096, 2);
    run("24 at the smallest chunk, 1 lane", three, cyc(24, 3, 14), 1, 1);
    run("24 at the smallest chunk, 2 lanes", three, cyc(24, 3, 14), 1, 2);
    run("unknown ids only", three, std::vector<uint32_t>(40, 5), 4096, 2);
    run("one class", three, std::vector<uint32_t>(300, 114), 128, 2);
    run("no resident ring", {}, cyc(10, 3, 0), 4096, 2);
    for (uint64_t B : {MR_BLOCK - 1, MR_BLOCK, MR_BLOCK + 1, 2 * MR_BLOCK - 1, 2 * MR_BLOCK, 2 * MR_BLOCK + 1}) {
        std::vector<uint32_t> ids(B, 100);   // one class of B - 1 proofs, one class of one proof at the end; the middle class stays empty
        ids[B - 1] = 114;
        char label[64];
        snprintf(label, sizeof label, "census block edge, B = %llu", (unsigned long long)B);
        run(label, three, ids, 64, 2);
    }
    {   // sixteen rings, every n the context can build for a small ring
        std::vector<uint32_t> ns;
        for (uint32_t r = 0; r < MR_SLOTS; r++) ns.push_back(1 + r);
        run("sixteen rings", ns, cyc(1000, 16, 9), 16, 3);
    }
    for (int it = 0; it < 200; it++) {   // the seeded sweep
        const uint32_t rings = 1 + rnd(MR_SLOTS);
        std::vector<uint32_t> ns;
        for (uint32_t r = 0; r < rings; r++) ns.push_back(1 + rnd(20));
        const uint64_t B = rnd(4) == 0 ? (uint64_t)MR_BLOCK * (1 + rnd(3)) + rnd(3) - 1 : rnd(1500);
        const uint32_t live = 1 + rnd(rings), unknown_pct = rnd(3) == 0 ? 0 : rnd(60);   // rings above `live` stay empty
        std::vector<uint32_t> ids(B);
        for (auto& v : ids) v = rnd(100) < unknown_pct ? 100 + 7 * rnd(live) + 1 + rnd(5) : 100 + 7 * rnd(live);
        char label[64];
        snprintf(label, sizeof label, "sweep %d", it);
        run(label, ns, ids, 1 + rnd(300), 1 + rnd(4));
    }
    if (failures) return fprintf(stderr, "%d checks failed\n", failures), 1;
    printf("member rings plan ok\n");
    return 0;
}
