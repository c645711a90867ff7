// Ring membership on its own (k_member.hip, api_member.hip): the launch wrappers (the ZKM1 layout is in wire.h) of the kernels around the shared GK machinery,
// and of the classing, offsets and gather kernels of the mixed-ring forms (k_member_rings.hip; the plan's arithmetic is member_plan.h's).
#pragma once
#include "sigma.h"   // jobs.h (ctx.h, engine.h, MaybeScope) and the chunk RNG: the member lanes' chunk front at the end
#include "member_plan.h"
// Where a window of a mixed-ring call puts its results: window entry j is proof sel[j] of a batch of B, whose slot starts at off[sel[j]] (prover).
// sel == nullptr: a one-ring call -- entry j is proof first + j, slots are `size` bytes apart.
struct MemberSel {
    const uint32_t* sel = nullptr;
    const uint64_t* off = nullptr;
    uint64_t B = 0;
};
void launch_m_front(hipStream_t s, const Workspace& W, uint32_t count, const uint32_t* which, const uint8_t* blinder, uint64_t first, uint32_t* which_s);
void launch_m_write_head(hipStream_t s, const Workspace& W, uint32_t count, uint64_t first, uint32_t size, uint8_t* out, uint8_t* com, uint8_t* blinder_out, int32_t* status,
                         const MemberSel& S = MemberSel{});
// slot != 0: every slot is `slot` bytes long (a window's gathered offsets have no successor to measure against)
void launch_mv_header_validate(hipStream_t s, const VWork& V, uint32_t count, const uint8_t* proofs, const uint64_t* off, uint64_t first, uint32_t slot = 0);
void launch_mv_offsets(hipStream_t s, uint64_t* off, uint64_t B, uint64_t size);
void launch_mv_final(hipStream_t s, const Workspace& W, const VWork& V, uint32_t count, uint8_t* ok, int32_t* status, uint64_t first, const MemberSel& S = MemberSel{});
// k_member_rings.hip
void launch_mr_class(hipStream_t s, uint64_t B, const uint32_t* ring_ids, const MrRings& R, const uint64_t* proof_off, uint8_t* cls, uint32_t* blk_cnt, uint32_t* out,
                     uint8_t* ok, int32_t* status);
void launch_mr_perm(hipStream_t s, uint64_t B, const uint8_t* cls, const uint32_t* blk_base, const uint32_t* out, uint32_t* perm);
void launch_mr_offsets(hipStream_t s, uint64_t B, const uint8_t* cls, const uint32_t* blk_base, const MrRings& R, uint64_t* out_off, uint8_t* com, uint8_t* blinder_out,
                       int32_t* status);
// context != nullptr (a bound call): the window also collects its proofs' 32 context bytes, entry j = context of proof sel[j]
void launch_mr_pgather(hipStream_t s, uint32_t n, uint64_t B, const uint32_t* sel, const uint32_t* which, const uint8_t* blinder, const uint8_t* seeds, const uint8_t* context,
                       uint32_t* w_which, uint8_t* w_blinder, uint8_t* w_seeds, uint8_t* w_context);
void launch_mr_vgather(hipStream_t s, uint32_t n, uint64_t B, const uint32_t* sel, const uint64_t* proof_off, const uint8_t* com, const uint8_t* seeds, const uint8_t* context,
                       uint64_t* w_off, uint8_t* w_com, uint8_t* w_seeds, uint8_t* w_context);

// ------------------------------------------------------------------ the member lanes (api_member.hip; api_rering.hip runs its chunks on them too)
zk_status ensure_member_lanes(zk_ctx* c, uint32_t C, uint32_t nlanes);   // api_member.hip
// 32-byte RNG blocks a chunk lays out per proof: fill 0 (com's blinder) where the engine draws it, the 5 n draws of the proof, and a margin -- rejected fills shift later draws
static inline uint32_t member_rng_blocks(uint32_t n, uint32_t fill0) { return fill0 + 5 * n + RNG_MAX_EXC; }
// A chunk's RNG on its lane (W.gk_fill0 is set): proofs first .. first + cnt of `rng`, whose data is a device pointer; the prepass; then, in seed mode, the
// chunk reads the fills the prepass wrote.
static inline void member_chunk_rng(zk_ctx* c, bool timed, hipStream_t s, Workspace& W, const zk_rng& rng, uint64_t first, uint32_t cnt) {
    sigma_chunk_rng(c, timed, s, W.rng, W.rng_fill, rng, first, cnt, member_rng_blocks(W.n, W.gk_fill0));
}
// A chunk's commitments: `front` (the caller's front end: launch_m_front / launch_rr_front) and the fold's scalars, then the 4 n membership commitments of
// every proof and every proof's com -- list C -- committed and normalised.  Returns what the fold read, for launch_gk_respond.
template <class Front>
static inline ChunkIn member_chunk_commit(zk_ctx* c, bool timed, hipStream_t s, Workspace& W, zk_ctx::MemberLane& L, uint32_t cnt, Front&& front) {
    const ChunkIn in{nullptr, nullptr, nullptr, L.which_s, cnt};
    const uint32_t nc = cnt * (4 * W.n + 1);
    {
        MaybeScope t(timed, c, "gk_fold", s);
        front();
        launch_gk_scalars_fold(s, W, in, L.gk_am);
        launch_gk_cd_scalars(s, W, cnt);
    }
    {
        MaybeScope t(timed, c, "tom_commit", s);
        launch_tom_commit(s, c->P, W.lc, nc, 1, 1);
    }
    {
        MaybeScope t(timed, c, "tom_normalize", s);
        launch_tom_normalize(s, W.lc, nc, 0, 1, 1);
    }
    return in;
}
