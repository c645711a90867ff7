// Re-ring proofs (include/zkattest.h: zk_proof_rering_batch; k_rering.hip, api_rering.hip): a ZKA1 proof's GKProof section is replaced by a fresh one for the
// active ring, every other byte is kept.  The membership prover runs as it is on a member lane (api_member.hip) whose writers point into the ZKA1 proof; this
// header has what is new: the rule that says where a proof's GKProof section lies, a lane's per-proof arrays and the launch wrappers of the kernels around it.
#pragma once
#include "engine.h"

// What the header of the proof in slot [o0, o1) says, read from its first 16 bytes alone: the bytes in front of its GKProof section (`head`) and its n, or
// ok = false where the slot is ZK_E_BAD_ENCODING for this call -- offsets that do not ascend or are not 4-byte aligned, a slot whose length is no multiple of 4 (no proof of either layout has one) or too short for a header, a
// wrong magic, a total_len that is not the slot's length, n > 63, a total_len smaller than the fixed head plus the GKProof its n announces.
struct RrHead {
    bool ok;
    uint32_t n, total, head;
};
ZK_HD static inline bool rr_slot_readable(uint64_t o0, uint64_t o1) { return o1 >= o0 && !(o0 & 3) && !((o1 - o0) & 3) && o1 - o0 >= ZK_HDR && o1 - o0 <= 0xffffffffull; }   // else no byte of it is read
ZK_HD static inline RrHead rr_head(const uint8_t* proofs, uint64_t o0, uint64_t o1, const Wire& w) {
    RrHead h{false, 0, 0, 0};
    if (!rr_slot_readable(o0, o1)) return h;
    uint32_t hw[4];
    __builtin_memcpy(hw, proofs + o0, 16);
    h.total = __builtin_bswap32(hw[1]), h.n = __builtin_bswap32(hw[3]);
    if (hw[0] != w.magic || h.total != o1 - o0 || h.n > 63) return h;
    const uint32_t gk = w.gk_n * h.n + 32;
    if (h.total < w.fixed + gk) return h;
    h.head = h.total - gk;
    h.ok = true;
    return h;
}
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
