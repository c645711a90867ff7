// Escrow tags (include/zkattest.h: zk_escrow_*, zk_ctx_set_auditor): exponential ElGamal of a committed key x under an auditor's key A = a g,
// (E1, E2) = (rho g, x g + rho A), with a sigma proof that E2 carries the x of C = x g + r h.  The "ZKT1" layout, the three responses, and the arithmetic the
// engine did not have: a * P for a 256-bit SECRET a and a point P out of a tag, and the opening rule 4 (E2 - a E1).  Device functions that also compile for
// the host CPU under ZK_HOST_BUILD (tests/host_arith/host_escrow.cpp).
#pragma once
#include "link.h"
#include "escrow_index.h"

// "ZKT1": 16 header bytes ("ZKT1" | total_len = 472 | 0 | 0), E1, E2, T1, T2, T3 (72 bytes each), t_x, t_r, t_rho (32 bytes each)
#define ZKT1_HDR 16
#define ZKT1_SIZE 472
#define ZKT1_WORDS (ZKT1_SIZE / 4)
#define ZK_MAGIC_ZKT1 0x31544b5au
#define ZKT1_PT(k) (ZKT1_HDR + 72 * (k))          // 0..4: E1, E2, T1, T2, T3
#define ZKT1_SC(k) (ZKT1_HDR + 360 + 32 * (k))    // 0..2: t_x, t_r, t_rho
#define ZKT1_MSG_POINTS 7   // hashPoints([C, E1, E2, A, T1, T2, T3]): 7 x 67 = 469 bytes ...
#define ZKT1_MSG_BLOCKS 8   // ... and SHA-256's padding

// The three responses, all plain canonical: t_x = k_x - c x, t_r = k_r - c r, t_rho = k_rho - c rho mod q
ZK_DEV void escrow_responses(Fe<ModQ, 1> t[3], const uint32_t c3[3], const Fe<ModQ, 1>& kx, const Fe<ModQ, 1>& kr, const Fe<ModQ, 1>& krho, const Fe<ModQ, 1>& x,
                             const Fe<ModQ, 1>& r, const Fe<ModQ, 1>& rho) {
    t[0] = link_respond(kx, c3, x), t[1] = link_respond(kr, c3, r), t[2] = link_respond(krho, c3, rho);
}
// a * base for a 256-bit a (a8: eight little-endian words) and a base with Z = 1 out of a tag.  a is the auditor's secret: left to right over its bits, one
// doubling and one mixed addition per bit, the addend chosen between the base and the identity's entry (0, 1, 0) by a mask over the limbs -- no branch and no
// address depends on a bit, in every build; the two candidates are values, not a table (a private array indexed at run time would be scratch).  256 doublings
// and 256 additions.  The base may carry a component of order 2 or 4 and the sum may pass through the identity (a >= q): everything stays on the a = 1 law,
// which is complete, and starts from the identity.
ZK_DEV TomPt escrow_ladder(const TomPt& base, const uint32_t* a8) {
    const TomNiels nb = link_niels(base);
    const Ft2 one = fe_one_mont<ModT>().as<2>();
    TomPt acc = tom_identity();
#pragma unroll 1
    for (int w = 7; w >= 0; w--) {
        uint32_t word = a8[w];
#pragma unroll 1
        for (int i = 0; i < 32; i++) {
            acc = tom_dbl(acc);
            const uint32_t m = 0u - (word >> 31);
            TomNiels e;
#pragma unroll
            for (int l = 0; l < NLIMB; l++) e.x.l[l] = nb.x.l[l] & m, e.y.l[l] = (nb.y.l[l] & m) | (one.l[l] & ~m), e.dt.l[l] = nb.dt.l[l] & m;
            acc = tom_add_niels(acc, e);
            word <<= 1;
        }
    }
    return acc;
}
// What a tag opens to: 4 (E2 - a E1).  The factor 4 kills whatever component of order 2 or 4 a prover left in E1 or E2, so that the prime-order parts decide
// -- they are rho g and x g + rho A by the tag's relations -- and the result is 4 x g.
ZK_DEV TomPt escrow_open_point(const TomPt& e1, const TomPt& e2, const uint32_t* a8) {
    const TomPt m = tom_add(e2, tom_neg(escrow_ladder(e1, a8)));
    return tom_dbl(tom_dbl(m));
}

#if !defined(ZK_HOST_BUILD)
// ------------------------------------------------------------------ a lane's arena (api_escrow.hip carves it, k_escrow.hip's kernels read it); C = tags per chunk
// The list's slots for a chunk of `count` tags.
// Prover: 4 p + k on (g, h) = E1 (rho, 0), T1 (k_x, k_r), T2 (k_rho, 0), the opening the caller claims (x, r); 4 count + 2 p + k on (g, A) = E2 (x, rho),
// T3 (k_x, k_rho).  Verifier: 2 p + k on (g, h) = (t_x, t_r), (t_rho, 0); 2 count + p on (g, A) = (t_x, t_rho).
#define ESC_SLOTS 6
struct EscrowLane : SigmaLane {   // L [ESC_SLOTS C], four draws, ZKT1_MSG_BLOCKS message blocks
    uint32_t* cw;         // [C][18] com (x, y) as the caller states it, nine little-endian words each
    uint32_t* rel;       // [C][3] verifier: the three relations as their lanes found them
};
#define ESC_RNG_BLOCKS (4 + RNG_MAX_EXC)   // rho, k_x, k_r, k_rho and a margin: rejected fills shift later draws
struct EscrowKey {        // (a kernel argument) the auditor's key as the caller stated it, nine little-endian words per coordinate
    uint32_t w[18];
};
struct EscrowProveIo {    // device pointers of a prove call, indexed by the tag's place in the batch
    const uint8_t *key, *com, *blinder;
    uint8_t* out;
    int32_t* status;
};
struct EscrowVerifyIo {
    const uint8_t *com, *tags;
    uint8_t* ok;
    int32_t* status;
};
// An open call's buffers: the tags' points 4 (E2 - a E1) in one list over the whole batch, a slab of the ring's points 4 y_i g in another
struct EscrowOpen {
    TomList T;            // [B]
    TomList S;            // [1] (a, 0), whose commitment is compared with the auditor's key
    uint32_t* a8;         // [8] a mod q as words
    int32_t* st;          // [B]
    TomList Rg;           // [ESC_RING_SLAB]
    uint8_t* ag;          // [72] a g as bytes
};
#define ESC_RING_SLAB (1u << 18)
void launch_escrow_check_key(hipStream_t s, const uint8_t* d_xy72, uint32_t* d_words18, int32_t* d_res /* [2]: encoding sound, identity */);
void launch_escrow_front(hipStream_t s, const EscrowLane& K, uint32_t count, uint64_t first, const EscrowProveIo& io);
void launch_escrow_opening_msg(hipStream_t s, const EscrowLane& K, const EscrowKey& A, uint32_t count);   // behind the normaliser: the opening compare, the challenge's message
void launch_escrow_respond(hipStream_t s, const EscrowLane& K, uint32_t count, uint64_t first, const EscrowProveIo& io);
void launch_escrow_parse(hipStream_t s, const EscrowLane& K, const EscrowKey& A, uint32_t count, uint64_t first, const EscrowVerifyIo& io);
void launch_escrow_relations(hipStream_t s, const EscrowLane& K, uint32_t count, uint64_t first, const EscrowVerifyIo& io);
void launch_escrow_verdict(hipStream_t s, const EscrowLane& K, uint32_t count, uint64_t first, const EscrowVerifyIo& io);
void launch_escrow_stage_secret(hipStream_t s, const uint8_t* d_secret, const TomList& L, uint32_t slot, uint32_t* a8);
void launch_escrow_open_points(hipStream_t s, const EscrowOpen& O, uint32_t count, uint64_t first, const uint8_t* tags, uint32_t* index, int32_t* status);
void launch_escrow_ring_scalars(hipStream_t s, const Soa& ring, uint64_t i0, uint32_t n, const TomList& L);
void launch_escrow_times4(hipStream_t s, const TomList& L, uint32_t n);   // the projective triples of slots 0 .. n - 1, doubled twice in place
void launch_escrow_match(hipStream_t s, const EscrowOpen& O, uint64_t B, uint64_t i0, uint32_t n, uint32_t* index);
// k_escrow_index.hip: the resident point index (escrow_index.h)
void launch_escrow_index_insert(hipStream_t s, const EscIndexRing& R);   // the slots hold ESC_INDEX_EMPTY, the points of the keys below R.nkeys are in place
void launch_escrow_index_lookup(hipStream_t s, const EscIndexSet& S, const EscrowOpen& O, uint64_t B, const uint32_t* ring_ids, uint32_t* ring_out, uint32_t* index,
                                int32_t* status);   // behind launch_escrow_open_points and the normaliser of O.T
void launch_escrow_index_gather(hipStream_t s, const Soa& ring, const uint32_t* ent, uint32_t n, const TomList& L);
void launch_escrow_index_scatter(hipStream_t s, const TomList& L, const uint32_t* ent, uint32_t n, uint32_t* pts, uint32_t cap);
#endif
