// Re-ring proofs (include/zkattest.h: zk_proof_rering_batch; k_rering.hip, api_rering.hip): a ZKA1 proof's GKProof section is replaced by a fresh one for the
// active ring, every other byte is kept.  The membership prover runs as it is on a member lane (api_member.hip) whose writers point into the ZKA1 proof; this
// header has what is new: the rule that says where a proof's GKProof section lies, a lane's per-proof arrays and the launch wrappers of the kernels around it.
#pragma once
#include "engine.h"
#include "rering_plan.h"   // RrHead, rr_head: what a proof's header says; the plan of the mixed-ring form

// a lane's per-proof arrays beside its member workspace; nothing here is witness-derived (keyXcom and R are public parts of the proofs)
struct RrLane {
    uint32_t* kx;      // [C][18] keyXcom as the proof states it: x, then y, nine little-endian words each
    uint32_t* head;    // [C] bytes in front of the proof's GKProof section (0 where the proof failed in the front end)
    uint32_t* flags;   // [C] bit 0: the RNG stream is too short for the proof's draws
    uint64_t* len;     // [C] the new proof's length, 0 for a failed proof
    Soa Rx, Ry;        // [C] R as the hardened statement hashes it (plain, reduced)
    Soa kax, kay;      // [2 C] list A as k_gk_hash reads it at W.sec = 0: slot 2 p = keyXcom
};
#define RR_CENSUS_WORDS 4   // u64: bytes the output needs at most, well-formed proofs whose n is not the ring's, proof_off[B]
void launch_rr_census(hipStream_t s, uint64_t B, const uint8_t* proofs, const uint64_t* off, const uint32_t* which, const Wire& wire, uint32_t n, uint32_t N,
                      unsigned long long* cnt);
// keyXcom's blinders: draw 1 of proofs [first, first + count) behind the prepass; *exhausted |= 1 where a proof's stream is too short for it (32 zero bytes then)
void launch_rr_blinders(hipStream_t s, const RngCtx& g, uint32_t count, uint64_t first, uint8_t* out, uint32_t* exhausted);
void launch_rr_front(hipStream_t s, const Workspace& W, const RrLane& X, uint32_t count, uint64_t first, const uint8_t* proofs, const uint64_t* off, const uint32_t* which,
                     const uint8_t* blinder, uint32_t* which_s);
void launch_rr_compare(hipStream_t s, const Workspace& W, const RrLane& X, uint32_t count, uint64_t first, int32_t* status);
// out_off[first + 1 ..] from the chunk's lengths behind out_off[first] (0 for the first chunk), and where each proof's new GKProof section starts
void launch_rr_scan(hipStream_t s, const Workspace& W, const RrLane& X, uint32_t count, uint64_t first, uint64_t* out_off);
// in place: out_off = proof_off
void launch_rr_place(hipStream_t s, const Workspace& W, const RrLane& X, uint32_t count, uint64_t first, uint64_t B, const uint64_t* off, uint64_t* out_off);
void launch_rr_move(hipStream_t s, const RrLane& X, uint32_t count, uint64_t first, const uint8_t* proofs, const uint64_t* off, const uint64_t* out_off, uint32_t n_new,
                    uint8_t* out);

// ------------------------------------------------------------------ one destination ring id per proof (k_rering_rings.hip; the plan is rering_plan.h's)
// The census' arrays over the whole batch, and what the host reads back in ONE copy: RRR_HEAD_BYTES of counters followed by k_part_scan's 2 x MR_CLASSES words
// (proofs per class, where each class starts in the permutation).
struct RrCensus {
    uint64_t* cnt;        // [4] the slots' bytes (= out_off[B]), proofs that pass rules 1-3 with another n than their ring's, proof_off[B], 0
    uint32_t* cls_tot;    // [2 x MR_CLASSES] directly behind cnt
    uint8_t* cls;         // [B]
    uint32_t *len, *head; // [B] the output slot's length and the bytes in front of the GKProof section, 0 for a refusal
    uint32_t* blk_cnt;    // [blocks][MR_CLASSES] per workgroup of MR_BLOCK proofs: proofs per class, then (k_part_scan) those of the workgroups before it
    uint64_t* blk_bytes;  // [blocks + 1] ... the bytes of its slots, then (k_rrr_totals) of the workgroups before it
    uint64_t* blk_other;  // [blocks] ... its proofs of another n
    uint32_t* perm;       // [B]
};
#define RRR_HEAD_BYTES 32
#define RRR_READBACK (RRR_HEAD_BYTES + 4 * 2 * MR_CLASSES)
void launch_rrr_census(hipStream_t s, uint64_t B, const uint8_t* proofs, const uint64_t* off, const uint32_t* which, const uint32_t* ids, const Wire& wire, const RrRings& R,
                       const RrCensus& X);
// out_off (in place: a copy of proof_off) and the statuses of rules 1-3
void launch_rrr_offsets(hipStream_t s, uint64_t B, const RrCensus& X, const uint64_t* proof_off, bool in_place, uint64_t* out_off, int32_t* status);
void launch_rrr_perm(hipStream_t s, uint64_t B, const RrCensus& X);
// every head of the batch to its place in one launch over [0, out_off[B]): k_rr_move's method with the per-proof n of the destination ring
void launch_rrr_move(hipStream_t s, uint64_t B, const RrCensus& X, const RrRings& R, const uint8_t* proofs, const uint64_t* off, const uint64_t* out_off, uint8_t* out);
// behind the windows: zero bytes in the slot of every proof whose final status is not ZK_OK (rules 4 and 5; the slots of rules 1-3 are empty)
void launch_rrr_blank(hipStream_t s, uint64_t B, const uint64_t* out_off, const int32_t* status, uint8_t* out);
// The sel-indexed forms of launch_rr_front / _compare / _place: window entry first + p is proof sel[first + p] of a batch of B (sel == nullptr: proof first + p).
// which / blinder are the window's gathered arrays (entry first + p), proofs / off / out_off / status the batch's.
void launch_rrr_front(hipStream_t s, const Workspace& W, const RrLane& X, uint32_t count, uint64_t first, const uint32_t* sel, uint64_t B, const uint8_t* proofs,
                      const uint64_t* off, const uint32_t* which, const uint8_t* blinder, uint32_t* which_s);
void launch_rrr_compare(hipStream_t s, const Workspace& W, const RrLane& X, uint32_t count, uint64_t first, const uint32_t* sel, uint64_t B, int32_t* status);
void launch_rrr_place(hipStream_t s, const Workspace& W, const RrLane& X, uint32_t count, uint64_t first, const uint32_t* sel, uint64_t B, const uint64_t* out_off);
