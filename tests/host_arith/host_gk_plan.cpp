// csrc/gk_plan.h on the host, with no HIP anywhere: the plans of the ring fold's buffers against (1) a restatement of the expressions the carvers and
// launchers spelled out before the header existed, literals and all, and (2) a walk of both launchers' passes -- the prover's tile pass, every finish pass
// with its ping-pong, or the per-level fallback of rings of fewer than 8 keys (k_scalar.hip: launch_gk_scalars_fold); the verifier's tile pass and finish
// passes with and without table E (k_verify.hip: launch_v_gk_total) -- in which every source and destination fits the planned capacity of its buffer.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include "gk_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            failures++;                   \
            fprintf(stderr, "FAIL: ");    \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
        }                                 \
    } while (0)

// ---- the expressions as they stood in api.hip: carve, api_member.hip: mcarve, api_verify.hip: vcarve and engine.h
static size_t old_finish_lds(uint32_t T, uint32_t g) { return sizeof(uint32_t) * 9 * ((size_t)g * (T + 1) + (size_t)(g / 2) * (T + 2)); }
static uint32_t old_finish_gsz(uint32_t T, uint32_t ntiles) {
    uint32_t g = ntiles < 64 ? ntiles : 64;
    while (g > 2 && old_finish_lds(T, g) > 60 * 1024) g >>= 1;
    return g;
}
static void plans_match_the_old_expressions(uint32_t C, uint32_t n, uint64_t N, bool etab) {
    const uint64_t g = std::max<uint64_t>(1, std::min<uint64_t>(C, ((uint64_t)1 << 16) / N));
    const uint32_t T = etab ? 8 : std::min<uint32_t>(n, 12);
    const uint64_t tile_elems = (uint64_t)(T + 1) * C * (N >> T);
    const uint64_t bufA = std::max<uint64_t>(g * N, tile_elems);
    const uint64_t bufB = std::max<uint64_t>(g * N, (uint64_t)(n + 1) * C * std::max<uint64_t>(1, (N >> T) / old_finish_gsz(T, (uint32_t)(N >> T))));
    const GkProvePlan p = gk_prove_plan(C, n, N, etab);
    CHECK(p.group == g && p.T == T && p.ntiles == N >> T && p.bufA == bufA && p.bufB == bufB, "prover plan C=%u n=%u etab=%d: group %u/%llu T %u/%u bufA %llu/%llu bufB %llu/%llu", C, n,
          etab, p.group, (unsigned long long)g, p.T, T, (unsigned long long)p.bufA, (unsigned long long)bufA, (unsigned long long)p.bufB, (unsigned long long)bufB);
    for (uint32_t t = 1; t <= 21; t++)
        for (uint32_t nt = 1; nt <= 8192; nt *= 2)
            CHECK(gk_finish_gsz(t, nt) == old_finish_gsz(t, nt) && gk_finish_lds(t, nt) == old_finish_lds(t, nt), "finish group T=%u ntiles=%u", t, nt);
    if (etab) return;   // (the verifier sizes by n alone)
    const uint32_t VT = n >= 9 && n <= 20 ? 8 : std::min<uint32_t>(n, 13);
    const GkVerifyPlan v = gk_verify_plan(C, n, N);
    CHECK(v.T == VT && v.res == (uint64_t)C * (N >> VT) && v.res2 == (uint64_t)C * std::max<uint64_t>(1, (N >> VT) / 512), "verifier plan C=%u n=%u: T %u/%u res %llu res2 %llu", C, n,
          v.T, VT, (unsigned long long)v.res, (unsigned long long)v.res2);
    CHECK(gk_etab_range(n) == (n >= 9 && n <= 20), "table range n=%u", n);
}

// ---- launch_gk_scalars_fold, a chunk of `count` <= C proofs
static void prover_passes_fit(uint32_t C, uint32_t n, uint64_t N, bool etab, uint32_t count) {
    const GkProvePlan p = gk_prove_plan(C, n, N, etab);
    if (n < 3) {   // one kernel per level: `group` proofs x N elements in A, then N/2 in B, ...
        CHECK(p.group >= 1 && p.group <= std::max<uint32_t>(C, 1), "fallback group %u of C=%u", p.group, C);
        const uint64_t cap = (uint64_t)p.group * N;
        CHECK(cap <= p.bufA && cap <= p.bufB, "fallback C=%u n=%u: %llu elements in %llu / %llu", C, n, (unsigned long long)cap, (unsigned long long)p.bufA, (unsigned long long)p.bufB);
        for (uint32_t first = 0; first < count; first += p.group) {
            const uint32_t G = std::min(count - first, p.group);
            for (uint32_t j = 0; j < n; j++) CHECK((uint64_t)G * (N >> j) <= cap && (uint64_t)G * (N >> (j + 1)) <= cap, "fallback level %u", j);
        }
        return;
    }
    uint32_t T = p.T, ntiles = p.ntiles;
    CHECK(T <= n && (etab || T <= GK_TMAX) && ((uint64_t)ntiles << T) == N, "tile C=%u n=%u etab=%d: T=%u ntiles=%u", C, n, etab, T, ntiles);
    uint64_t src_cap = p.bufA, dst_cap = p.bufB;
    CHECK((uint64_t)(T + 1) * C * ntiles <= src_cap, "tile pass C=%u n=%u etab=%d", C, n, etab);   // res: stride (T+1) C ntiles, rows of proofs < count
    while (ntiles > 1) {
        const uint32_t gsz = gk_finish_gsz(T, ntiles), ngroups = ntiles / gsz;
        uint32_t lv = 0;
        while ((1u << lv) < gsz) lv++;
        CHECK(gsz >= 2 && ngroups * gsz == ntiles && (1u << lv) == gsz, "finish C=%u n=%u etab=%d: group %u of %u tiles", C, n, etab, gsz, ntiles);
        CHECK(gsz == 2 || gk_finish_lds(T, gsz) <= 60 * 1024, "finish LDS T=%u gsz=%u", T, gsz);
        CHECK((uint64_t)(T + 1) * C * ntiles <= src_cap, "finish source C=%u n=%u etab=%d T=%u: %llu in %llu", C, n, etab, T, (unsigned long long)(T + 1) * C * ntiles, (unsigned long long)src_cap);
        CHECK((uint64_t)(T + lv + 1) * C * ngroups <= dst_cap, "finish destination C=%u n=%u etab=%d T=%u: %llu in %llu", C, n, etab, T, (unsigned long long)(T + lv + 1) * C * ngroups,
              (unsigned long long)dst_cap);
        std::swap(src_cap, dst_cap);
        T += lv, ntiles = ngroups;
    }
    CHECK(T == n, "C=%u n=%u etab=%d: the passes fold %u index bits", C, n, etab, T);   // n + 1 coefficients per proof land in gk_coef
}

// ---- launch_v_gk_total: sized by n, launched by the table pointer
static void verifier_passes_fit(uint32_t C, uint32_t n, uint64_t N, bool etab, uint32_t count) {
    if (n < 3) return;   // k_v_gk_small: one thread per proof, no buffer
    const GkVerifyPlan v = gk_verify_plan(C, n, N);
    uint32_t T = vgk_tile(n, etab);
    uint64_t ntiles = N >> T;
    CHECK(T <= n && T >= v.T, "verifier tile C=%u n=%u etab=%d: launches at %u, sized for %u", C, n, etab, T, v.T);
    uint64_t src_cap = v.res, dst_cap = v.res2;
    if (ntiles > 1) CHECK(count * ntiles <= src_cap, "verifier tile pass C=%u n=%u etab=%d", C, n, etab);
    while (ntiles > 1) {
        const uint32_t gsz = vgk_finish_gsz((uint32_t)ntiles);
        const uint64_t ngroups = ntiles / gsz;
        uint32_t lv = 0;
        while ((1u << lv) < gsz) lv++;
        CHECK(gsz >= 2 && gsz <= 512 && ngroups * gsz == ntiles && (1u << lv) == gsz, "verifier finish C=%u n=%u etab=%d: group %u of %llu", C, n, etab, gsz, (unsigned long long)ntiles);
        CHECK(count * ntiles <= src_cap, "verifier finish source C=%u n=%u etab=%d", C, n, etab);
        if (ngroups > 1) CHECK(count * ngroups <= dst_cap, "verifier finish destination C=%u n=%u etab=%d: %llu in %llu", C, n, etab, (unsigned long long)(count * ngroups), (unsigned long long)dst_cap);
        std::swap(src_cap, dst_cap);
        T += lv, ntiles = ngroups;
    }
    CHECK(T == n, "verifier C=%u n=%u etab=%d: the passes fold %u index bits", C, n, etab, T);
}

int main() {
    const uint32_t ns[] = {1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 20, 21}, Cs[] = {1, 15, 16, 17, 4096};
    int shapes = 0;
    for (uint32_t n : ns)
        for (uint32_t C : Cs)
            for (int etab = 0; etab <= (n >= 9 && n <= 20 ? 1 : 0); etab++) {   // a ring has a table E only in this range (api.hip: build_ring)
                const uint64_t N = (uint64_t)1 << n;
                plans_match_the_old_expressions(C, n, N, etab != 0);
                for (uint32_t count : {C, (C + 1) / 2}) prover_passes_fit(C, n, N, etab != 0, count), verifier_passes_fit(C, n, N, etab != 0, count);
                shapes++;
            }
    for (uint32_t sec : {1u, 20u, 80u, 128u}) {
        const size_t blocks = (2 * 67 + (size_t)sec * (65 + 2 * 67) + 9 + 63) / 64;
        CHECK(exph_blocks(sec) == blocks && exph_msg_bytes(sec) == 2 * 67 + sec * (65 + 2 * 67), "Exp message sec=%u: %u blocks, %zu spelled out", sec, exph_blocks(sec), blocks);
    }
    printf("%d shapes: plans as before, every pass of both folds inside its buffers\n", shapes);
    if (failures) return 1;
    printf("gk plan ok\n");
    return 0;
}
