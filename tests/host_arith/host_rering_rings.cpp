// csrc/rering_plan.h on the host: the plan of a mixed-ring re-ring call, against a direct restatement.  Batches of synthetic proof headers -- several
// secLevels, so heads of different lengths; several source n; broken headers; ids that are not resident; indices outside the destination ring -- over fixed
// shapes (empty classes, classes of one proof, unknown ids only, batches of the census workgroup's size and one proof either side of it) and a seeded sweep
// of 200 mixes: every proof's class, status and slot (rules 1-3 in their order), the offsets, the offsets as the device derives them (per workgroup sums, a
// scan inside the workgroup), the out_cap / in-place / overlap decisions and the window cuts.  Built with the sanitizers by tests/test_rering_rings_host.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rering_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                        \
    do {                                        \
        if (!(cond)) {                          \
            failures++;                         \
            fprintf(stderr, "FAIL %s: ", name); \
            fprintf(stderr, __VA_ARGS__);       \
            fprintf(stderr, "\n");              \
        }                                       \
    } while (0)

static uint64_t rng_state = 0x243f6a8885a308d3ull;
static uint32_t rnd(uint32_t below) {   // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) % below);
}
// include/zkattest.h, restated: ZKA1 (tc = 36) and ZKA1P (tc = 33)
static uint64_t gk_size(uint32_t n, uint32_t tc) { return (uint64_t)n * (8 * tc + 96) + 32; }
static uint64_t head_size(uint32_t sec, uint32_t z, uint32_t tc) {
    const uint64_t fixed = 32 + 128 + 4 * tc, rep = 64 + 4 * tc + 128, mult = 12 * tc + 224, eq = 4 * tc + 96;
    return fixed + rep * sec + (8 * tc + 4 * mult + 2 * eq) * z;
}
static void be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24), p[1] = (uint8_t)(v >> 16), p[2] = (uint8_t)(v >> 8), p[3] = (uint8_t)v; }

enum Break { FINE, MAGIC, TOTAL, BIG_N, SHORT, MISALIGNED_LEN };
struct Spec {
    uint32_t sec, z, n_old, id, which;
    Break brk;
};
struct RingSpec {
    uint32_t id, n;
};

static void run(const char* name, bool packed, const std::vector<RingSpec>& rings, const std::vector<Spec>& specs, uint32_t chunk, uint32_t lanes) {
    const uint64_t B = specs.size();
    const uint32_t tc = packed ? 33 : 36;
    const Wire wire = wire_make(packed);
    RrRings R;
    rrr_rings_clear(R);
    for (const RingSpec& r : rings) rrr_rings_add(R, r.id, r.n, 1ull << r.n);
    CHECK(R.m.count == rings.size(), "%u rings", R.m.count);
    // ---- the batch: headers only (16 bytes of the 32-byte header matter), the rest of every slot stays zero
    std::vector<uint64_t> off(B + 1, 0);
    std::vector<uint32_t> ids(B), which(B);
    std::vector<uint64_t> slot_len(B);
    for (uint64_t b = 0; b < B; b++) {
        const Spec& s = specs[b];
        uint64_t len = head_size(s.sec, s.z, tc) + gk_size(s.n_old, tc);
        if (s.brk == SHORT) len = 16;
        if (s.brk == MISALIGNED_LEN) len += 2;
        slot_len[b] = len, off[b + 1] = off[b] + len, ids[b] = s.id, which[b] = s.which;
    }
    std::vector<uint8_t> blob(off[B] + 1, 0);
    for (uint64_t b = 0; b < B; b++) {
        const Spec& s = specs[b];
        uint8_t* p = blob.data() + off[b];
        if (slot_len[b] < 16) continue;
        memcpy(p, packed ? "ZK1P" : "ZKA1", 4);
        if (s.brk == MAGIC) p[3] ^= 1;
        be32(p + 4, (uint32_t)slot_len[b] + (s.brk == TOTAL ? 4 : 0));
        be32(p + 8, s.sec);
        be32(p + 12, s.brk == BIG_N ? 64 : s.n_old);
    }
    // ---- direct restatement: rules 1-3 in their order
    std::vector<uint32_t> want_cls(B), want_len(B), want_head(B);
    std::vector<int32_t> want_st(B);
    std::vector<uint64_t> want_off(B + 1, 0);
    std::vector<std::vector<uint32_t>> members(MR_CLASSES);
    uint64_t want_other = 0, want_in = 0;
    for (uint64_t b = 0; b < B; b++) {
        const Spec& s = specs[b];
        int ring = -1;
        for (size_t r = 0; r < rings.size(); r++)
            if (rings[r].id == s.id) ring = (int)r;
        const bool aligned = !(off[b] & 3);
        uint32_t cls, len = 0, head = 0;
        int32_t st;
        if (ring < 0) cls = RRR_ARG, st = ZK_E_ARG;
        else if (s.brk != FINE || !aligned) cls = RRR_ENC, st = ZK_E_BAD_ENCODING;
        else if (s.which >= (1ull << rings[ring].n)) cls = RRR_ARG, st = ZK_E_ARG;
        else {
            cls = (uint32_t)ring, st = ZK_OK, head = (uint32_t)head_size(s.sec, s.z, tc), len = head + (uint32_t)gk_size(rings[ring].n, tc);
            want_other += s.n_old != rings[ring].n;
        }
        if (ring >= 0 && aligned && !(slot_len[b] & 3) && slot_len[b] >= 32) want_in = std::max(want_in, off[b + 1]);
        want_cls[b] = cls, want_len[b] = len, want_head[b] = head, want_st[b] = st;
        members[cls].push_back((uint32_t)b);
        want_off[b + 1] = want_off[b] + len;
    }
    // ---- per proof, then the host plan
    for (uint64_t b = 0; b < B; b++) {
        const RrPlan p = rrr_plan_proof(R, wire, blob.data(), off[b], off[b + 1], ids[b], which[b]);
        CHECK(p.cls == want_cls[b] && p.len == want_len[b] && p.head == want_head[b], "proof %llu: class %u, slot %u, head %u (want %u, %u, %u)", (unsigned long long)b, p.cls, p.len,
              p.head, want_cls[b], want_len[b], want_head[b]);
        CHECK(rrr_class_status(p.cls) == want_st[b], "proof %llu: status %d, not %d", (unsigned long long)b, rrr_class_status(p.cls), want_st[b]);
    }
    std::vector<uint8_t> cls(B + 1, 0xee);
    std::vector<uint64_t> poff(B + 2, ~0ull);
    const RrBatch t = rrr_plan_host(R, wire, B, blob.data(), off.data(), ids.data(), which.data(), cls.data(), poff.data());
    CHECK(cls[B] == 0xee && poff[B + 1] == ~0ull, "the plan wrote past its arrays");
    for (uint64_t b = 0; b < B; b++) CHECK(cls[b] == want_cls[b] && poff[b] == want_off[b], "proof %llu: class %u at %llu", (unsigned long long)b, cls[b], (unsigned long long)poff[b]);
    CHECK(poff[B] == want_off[B] && t.bytes == want_off[B], "total %llu, not %llu", (unsigned long long)t.bytes, (unsigned long long)want_off[B]);
    CHECK(t.other == want_other && t.in_bytes == want_in, "other %llu (want %llu), input bytes %llu (want %llu)", (unsigned long long)t.other, (unsigned long long)want_other,
          (unsigned long long)t.in_bytes, (unsigned long long)want_in);
    for (uint32_t k = 0; k < MR_CLASSES; k++) CHECK(t.cnt[k] == members[k].size(), "class %u: %u proofs", k, t.cnt[k]);
    const RrBatch t2 = rrr_plan_host(R, wire, B, blob.data(), off.data(), ids.data(), which.data(), nullptr, nullptr);
    CHECK(t2.bytes == t.bytes && t2.other == t.other && t2.in_bytes == t.in_bytes, "the plan without arrays differs");
    // ---- the device's way: per workgroup of MR_BLOCK proofs the sum of its slots, the exclusive prefix over the workgroups, a scan inside the workgroup
    {
        std::vector<uint64_t> blk((B + MR_BLOCK - 1) / MR_BLOCK + 1, 0);
        for (uint64_t b = 0; b < B; b++) blk[b / MR_BLOCK] += rrr_plan_proof(R, wire, blob.data(), off[b], off[b + 1], ids[b], which[b]).len;
        uint64_t run_ = 0;
        for (auto& v : blk) {
            const uint64_t x = v;
            v = run_, run_ += x;
        }
        for (uint64_t b0 = 0; b0 < B; b0 += MR_BLOCK) {
            uint64_t at = blk[b0 / MR_BLOCK];
            for (uint64_t b = b0; b < B && b < b0 + MR_BLOCK; b++) {
                CHECK(at == want_off[b], "workgroup %llu: proof %llu at %llu", (unsigned long long)(b0 / MR_BLOCK), (unsigned long long)b, (unsigned long long)at);
                at += want_len[b];
            }
        }
        CHECK(blk.back() == want_off[B], "the workgroups' total");
    }
    // ---- the decisions: out_cap exact, in place, overlap
    {
        const uint8_t* in = blob.data();
        std::vector<uint8_t> other_buf(16);
        const uint8_t* far = other_buf.data();   // (only compared, never dereferenced: rrr_decide reads no byte)
        const uint64_t need = want_off[B], in_end = off[B];
        const bool apart = far + need <= in || in + in_end <= far;
        if (apart) {
            CHECK(rrr_decide(in, far, need, need, want_other, in_end) == ZK_OK && rrr_decide(in, far, ~0ull, need, want_other, in_end) == ZK_OK, "a buffer that holds the batch is refused");
            if (need) CHECK(rrr_decide(in, far, need - 1, need, want_other, in_end) == ZK_E_BUFFER && rrr_decide(in, far, 0, need, want_other, in_end) == ZK_E_BUFFER, "a buffer one byte short");
        }
        // in place: allowed exactly when no proof changes size; out_cap against proof_off[B]
        CHECK(rrr_decide(in, in, in_end, need, want_other, in_end) == (want_other ? ZK_E_ARG : ZK_OK), "in place with %llu proofs of another n", (unsigned long long)want_other);
        if (in_end) CHECK(rrr_decide(in, in, in_end - 1, need, 0, in_end) == ZK_E_BUFFER, "in place, one byte short");
        CHECK(rrr_decide(in, in, in_end, need, 1, in_end) == ZK_E_ARG && rrr_decide(in, in, 0, need, 1, in_end) == ZK_E_ARG, "in place: the size rule comes before out_cap");
        // any other overlap: out inside the input, the input inside out, out's end touching the input's start is none
        if (in_end > 64 && need) {
            CHECK(rrr_decide(in, in + 64, ~0ull, need, 0, in_end) == ZK_E_ARG, "out 64 bytes into proofs");
            CHECK(rrr_decide(in + 64, in, ~0ull, need + 65, 0, in_end - 64) == ZK_E_ARG, "proofs 64 bytes into out");
            CHECK(rrr_decide(in, in + in_end, ~0ull, need, 0, in_end) == ZK_OK, "out directly behind proofs");
            CHECK(rrr_decide(in + need, in, ~0ull, need, 0, in_end - std::min(need, in_end)) == ZK_OK, "out directly in front of proofs");
            CHECK(rrr_decide(in, in + 64, 0, need, 0, in_end) == ZK_E_ARG, "overlap comes before out_cap");
        }
    }
    // ---- the fast path's condition and the windows
    {
        uint32_t used = 0, last = MR_CLASSES;
        for (size_t r = 0; r < rings.size(); r++)
            if (!members[r].empty()) used++, last = (uint32_t)r;
        const uint32_t want = used == 1 && members[RRR_ARG].empty() && members[RRR_ENC].empty() ? last : MR_CLASSES;
        CHECK(mr_single_class(t.cnt, R.m) == want, "single class %u, not %u", mr_single_class(t.cnt, R.m), want);
    }
    const uint32_t cap = mr_window_cap(chunk, lanes, t.cnt, R.m);
    uint32_t most = 1;
    for (size_t r = 0; r < rings.size(); r++) most = std::max<uint32_t>(most, (uint32_t)members[r].size());
    CHECK(cap >= 1 && cap == std::min<uint64_t>(2ull * chunk * lanes, most), "cap %u for chunk %u, lanes %u, largest class %u", cap, chunk, lanes, most);
    std::vector<uint32_t> seen(B, 0);
    uint32_t windows = 0;
    for (size_t r = 0; r < rings.size(); r++) {
        const uint32_t n = t.cnt[r], nw = mr_window_count(n, cap);
        uint32_t next = 0;
        for (uint32_t w = 0; w < nw; w++, windows++) {
            uint32_t first, c;
            mr_window(n, cap, w, &first, &c);
            CHECK(first == next && c >= 1 && c <= cap && first + c <= n, "class %zu window %u: [%u, +%u) of %u", r, w, first, c, n);
            for (uint32_t j = first; j < first + c && j < n; j++) seen[members[r][j]]++;
            next = first + c;
        }
        CHECK(next == n, "class %zu: windows end at %u of %u", r, next, n);
    }
    for (uint64_t b = 0; b < B; b++) CHECK(seen[b] == (want_cls[b] < MR_SLOTS ? 1u : 0u), "proof %llu entered %u windows", (unsigned long long)b, seen[b]);
    printf("%-36s B %5llu, %2zu rings, %9llu bytes, %3llu of another n, cap %u, %u windows\n", name, (unsigned long long)B, rings.size(), (unsigned long long)want_off[B],
           (unsigned long long)want_other, cap, windows);
}

int main() {
    const char* name = "header rule";
    {   // rr_head on its own
        const Wire w = wire_make(false);
        std::vector<uint8_t> p(head_size(1, 0, 36) + gk_size(3, 36), 0);
        memcpy(p.data(), "ZKA1", 4), be32(p.data() + 4, (uint32_t)p.size()), be32(p.data() + 8, 1), be32(p.data() + 12, 3);
        const RrHead h = rr_head(p.data(), 0, p.size(), w);
        CHECK(h.ok && h.n == 3 && h.head == head_size(1, 0, 36) && h.total == p.size(), "an honest header: head %u", h.head);
        CHECK(!rr_head(p.data(), 0, p.size() - 4, w).ok && !rr_head(p.data(), 2, p.size() + 2, w).ok && !rr_head(p.data(), 8, 0, w).ok, "a slot that is not the header's");
        CHECK(!rr_head(p.data(), 0, p.size(), wire_make(true)).ok, "the other layout's magic");
        be32(p.data() + 12, 40);   // an n whose GKProof alone is longer than the proof
        CHECK(!rr_head(p.data(), 0, p.size(), w).ok, "total_len below head + GKProof");
    }
    const std::vector<RingSpec> three = {{100, 3}, {107, 5}, {114, 3}};
    const uint32_t secs[3] = {20, 80, 128};
    auto good = [&](uint64_t b, uint32_t id, uint32_t n_old) { return Spec{secs[b % 3], (uint32_t)(b % 5), n_old, id, (uint32_t)(b % 8), FINE}; };
    auto cyc = [&](uint64_t B, uint32_t unknown_every) {
        std::vector<Spec> v;
        for (uint64_t b = 0; b < B; b++) v.push_back(good(b, unknown_every && b % unknown_every == unknown_every - 1 ? 5 : three[b % 3].id, 3));
        return v;
    };
    run("empty batch", false, three, {}, 4096, 2);
    run("one proof", false, three, {good(0, 107, 3)}, 4096, 2);
    run("10 interleaved, mixed secLevels", false, three, cyc(10, 0), 4096, 2);
    run("10 interleaved, packed", true, three, cyc(10, 0), 4096, 2);
    run("24, one unknown, smallest chunk", false, three, cyc(24, 14), 1, 1);
    run("24, one unknown, 2 lanes", false, three, cyc(24, 14), 1, 2);
    {
        std::vector<Spec> v;
        for (uint64_t b = 0; b < 40; b++) v.push_back(good(b, 5, 3));
        run("unknown ids only", false, three, v, 4096, 2);
        run("no resident ring", false, {}, v, 4096, 2);
    }
    {   // every refusal between good neighbours; an unknown id beats a broken header, a broken header beats an index outside the ring
        std::vector<Spec> v = cyc(12, 0);
        v[1].brk = MAGIC, v[3].brk = TOTAL, v[5].brk = BIG_N, v[7].which = 8 /* ring 107 holds 32 */, v[8].which = 8 /* ring 114 holds 8 */, v[9].which = 32;
        v[10] = Spec{20, 0, 3, 5, 99, MAGIC}, v[11] = Spec{20, 0, 3, 100, 99, TOTAL};
        run("refusals between good neighbours", false, three, v, 4096, 2);
        v[4].brk = MISALIGNED_LEN;   // every slot behind it starts misaligned
        run("a slot of odd length", false, three, v, 4096, 2);
        v[4].brk = SHORT;
        run("a slot shorter than a header", false, three, v, 4096, 2);
    }
    {   // in place: every proof already has its ring's n, then one that does not
        std::vector<Spec> v;
        for (uint64_t b = 0; b < 9; b++) v.push_back(good(b, three[b % 3].id, three[b % 3].n));
        run("in place, equal n", false, three, v, 2, 2);
        v[4].n_old = 3;   // bound for the ring of n = 5
        run("in place, one proof of another n", false, three, v, 2, 2);
    }
    {
        std::vector<Spec> v;
        for (uint64_t b = 0; b < 300; b++) v.push_back(good(b, 114, 5));
        run("one class", false, three, v, 128, 2);
    }
    for (uint64_t B : {MR_BLOCK - 1, MR_BLOCK, MR_BLOCK + 1, 2 * MR_BLOCK - 1, 2 * MR_BLOCK, 2 * MR_BLOCK + 1}) {
        std::vector<Spec> v;
        for (uint64_t b = 0; b < B; b++) v.push_back(good(b, 100, 3));   // one class of B - 1 proofs, one of one proof at the end; the middle ring stays empty
        v[B - 1].id = 114;
        char label[64];
        snprintf(label, sizeof label, "census block edge, B = %llu", (unsigned long long)B);
        run(label, false, three, v, 64, 2);
    }
    for (int it = 0; it < 200; it++) {   // the seeded sweep
        const uint32_t nr = 1 + rnd(MR_SLOTS);
        std::vector<RingSpec> rings;
        for (uint32_t r = 0; r < nr; r++) rings.push_back({100 + 7 * r, 1 + rnd(20)});
        const uint64_t B = rnd(4) == 0 ? (uint64_t)MR_BLOCK * (1 + rnd(2)) + rnd(3) - 1 : rnd(400);
        const uint32_t live = 1 + rnd(nr), unknown_pct = rnd(3) == 0 ? 0 : rnd(50), broken_pct = rnd(3) == 0 ? 0 : rnd(30), same_n = rnd(3) == 0;
        std::vector<Spec> v(B);
        for (auto& s : v) {
            const uint32_t r = rnd(live);
            s.sec = secs[rnd(3)], s.z = rnd(s.sec + 1), s.id = rnd(100) < unknown_pct ? rings[r].id + 1 + rnd(5) : rings[r].id;
            s.n_old = same_n ? rings[r].n : 1 + rnd(20);
            s.which = rnd(10) == 0 ? (1u << rings[r].n) + rnd(3) : rnd(1u << rings[r].n);
            s.brk = rnd(100) < broken_pct ? (Break)(1 + rnd(5)) : FINE;
        }
        char label[64];
        snprintf(label, sizeof label, "sweep %d", it);
        run(label, rnd(2) != 0, rings, v, 1 + rnd(100), 1 + rnd(4));
    }
    if (failures) return fprintf(stderr, "%d checks failed\n", failures), 1;
    printf("rering rings plan ok\n");
    return 0;
}
