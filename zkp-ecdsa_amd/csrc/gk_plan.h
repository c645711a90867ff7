// Geometry of the ring fold (GK phase): which tile exponent a launch uses and how many elements each of its buffers must hold.  The launchers
// (k_scalar.hip: launch_gk_scalars_fold; k_verify.hip: launch_v_gk_total) and the carvers of every arena that holds a fold's buffers (ctx.h: carve_gk_*)
// take these numbers from here and nowhere else.  An element is one field value of 9 limbs (36 bytes of an Soa).  Nothing here knows HIP: plain g++
// compiles it (tests/host_arith/host_gk_plan.cpp, which walks both launchers' passes against the planned capacities).
#pragma once
#include <stddef.h>
#include "wire.h"   // ZK_HD

#define GK_BLOCK_T 8      // a ring with table E folds its 8 low index bits through the table: one value (polynomial) per 256 keys (k_gk.hip)
#define GK_ETAB_MINN 9    // rings of 2^9 .. 2^20 keys get a table E when they are built (api.hip)
#define GK_ETAB_MAXN 20
#define GKM_MINN 12       // ... and from 2^12 keys on the digit planes of the matrix-pipe fold (k_gk_mfma.hip)
#define GK_TMAX 12        // prover's plain tile: 256 lanes x 16 elements (k_scalar.hip: k_gk_tile)
#define GK_FIN_GMAX 64    // prover's finish pass: polynomials per workgroup, fewer where their dynamic LDS would pass GK_FIN_LDS_MAX (k_gk_finish)
#define GK_FIN_LDS_MAX (60 * 1024)
#define GK_LEVEL_ELEMS (1u << 16)   // rings of fewer than 8 keys: elements one pass of the per-level fallback holds in each ping-pong buffer (k_gk_level)
#define VGK_T 13          // verifier's plain tile: 256 lanes x 32 elements (k_verify.hip: k_v_gk_tile)
#define VGK_FIN 512u      // verifier's finish pass: tile values per workgroup (k_v_gk_finish)

static inline bool gk_etab_range(uint32_t n) { return n >= GK_ETAB_MINN && n <= GK_ETAB_MAXN; }

// ---- prover
// dynamic LDS of one k_gk_finish workgroup over g polynomials of T+1 coefficients: plane A g x (T+1) elements, plane B g/2 x (T+2)
static inline size_t gk_finish_lds(uint32_t T, uint32_t g) { return sizeof(uint32_t) * 9 * ((size_t)g * (T + 1) + (size_t)(g / 2) * (T + 2)); }
static inline uint32_t gk_finish_gsz(uint32_t T, uint32_t ntiles) {
    uint32_t g = ntiles < GK_FIN_GMAX ? ntiles : GK_FIN_GMAX;
    while (g > 2 && gk_finish_lds(T, g) > GK_FIN_LDS_MAX) g >>= 1;
    return g;
}
// n >= 3: the tile pass leaves (T+1) coefficients x ntiles polynomials per proof in gk_bufA, and the finish passes ping-pong between gk_bufB and gk_bufA
// until one polynomial of n+1 coefficients is left (the first pass's output is the largest).  n < 3: one kernel per level on `group` proofs at a time,
// group x N elements in either buffer.
struct GkProvePlan {
    uint32_t group;        // proofs per pass of the per-level fallback
    uint32_t T, ntiles;    // tile exponent and tiles per proof
    uint64_t bufA, bufB;   // elements
};
static inline GkProvePlan gk_prove_plan(uint32_t C, uint32_t n, uint64_t N, bool has_etab) {
    GkProvePlan p;
    const uint64_t fit = GK_LEVEL_ELEMS / N, group = fit > C ? C : fit < 1 ? 1 : fit;
    p.group = (uint32_t)group;
    p.T = has_etab ? GK_BLOCK_T : n < GK_TMAX ? n : GK_TMAX;
    p.ntiles = (uint32_t)(N >> p.T);
    const uint32_t ngroups = p.ntiles / gk_finish_gsz(p.T, p.ntiles);
    const uint64_t level = group * N, tiles = (uint64_t)(p.T + 1) * C * p.ntiles, finish = (uint64_t)(n + 1) * C * (ngroups ? ngroups : 1);
    p.bufA = level > tiles ? level : tiles;
    p.bufB = level > finish ? level : finish;
    return p;
}

// ---- verifier
// The launcher takes the table path where the bound ring HAS a table (its pointer); the carver cannot know that -- a lane's arena outlives the ring it was
// carved for -- and sizes for the table path wherever n allows a table.  A ring in that range without one (ZKATTEST_GK_TABLE=0, or the table shed) launches
// with the larger plain tile: fewer, never more, elements than planned.
static inline uint32_t vgk_tile(uint32_t n, bool block) { return block ? GK_BLOCK_T : n < VGK_T ? n : VGK_T; }
static inline uint32_t vgk_finish_gsz(uint32_t ntiles) { return ntiles < VGK_FIN ? ntiles : VGK_FIN; }
struct GkVerifyPlan {
    uint32_t T;           // the tile exponent the buffers are sized for
    uint64_t res, res2;   // elements: one value per tile and proof, then one per finish group
};
static inline GkVerifyPlan gk_verify_plan(uint32_t C, uint32_t n, uint64_t N) {
    GkVerifyPlan p;
    p.T = vgk_tile(n, gk_etab_range(n));
    const uint64_t ntiles = N >> p.T, ngroups = ntiles / VGK_FIN;
    p.res = C * ntiles;
    p.res2 = C * (ngroups ? ngroups : 1);
    return p;
}

// ---- the Exp challenge's message (k_hash.hip: k_exph_*; its buffers are carved beside the fold's): the padded message of hashPoints(Px, Py, A_0, Tx_0,
// Ty_0, ...) -- two Tom points (67 bytes each), then per repetition a P-256 point (65) and two Tom points -- and its length in 64-byte blocks
ZK_HD static inline uint32_t exph_msg_bytes(uint32_t sec) { return 2 * 67 + sec * (65 + 2 * 67); }
ZK_HD static inline uint32_t exph_blocks(uint32_t sec) { return (exph_msg_bytes(sec) + 9 + 63) / 64; }
