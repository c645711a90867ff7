// Re-ring calls (include/zkattest.h: zk_proof_rering_batch, zk_proof_rering_batch_rings): what a proof's header says, and the plan of the mixed-ring form --
// every proof's class and output length from its header, its destination ring and its index alone (rules 1-3 of the contract, in that order), the batch's
// offsets, the out_cap / in-place / overlap decisions and the window cuts (member_plan.h: mr_window*).  The census and offsets kernels (k_rering_rings.hip)
// and the host layer (api_rering.hip: the host-pointer form plans here before anything is uploaded) share these functions.  Nothing here knows HIP: plain
// g++ compiles it (tests/host_arith/host_rering_rings.cpp).
#pragma once
#include "../../include/zkattest.h"
#include "member_plan.h"

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

// ------------------------------------------------------------------ one destination ring id per proof
// A proof's class: the slot of its destination ring, or one of the two refusals that are settled before anything is proved (a zero-length slot).  They
// take member_plan.h's two spare classes, so its counts, single-class test and windows apply as they are.
#define RRR_ARG MR_UNKNOWN   // rule 1 (the id is not resident) or rule 3 (which_new >= N of its ring): ZK_E_ARG
#define RRR_ENC MR_BAD       // rule 2 (rr_head refuses header or slot): ZK_E_BAD_ENCODING
struct RrRings {   // (a kernel argument) the resident rings in slot order; m.size is unused here (a re-ringed proof's length also follows from its head)
    MrRings m;
    uint32_t n[MR_SLOTS];
    uint64_t N[MR_SLOTS];
};
ZK_HD static inline void rrr_rings_clear(RrRings& r) {
    mr_rings_clear(r.m);
    for (uint32_t s = 0; s < MR_SLOTS; s++) r.n[s] = 0, r.N[s] = 0;
}
ZK_HD static inline void rrr_rings_add(RrRings& r, uint32_t id, uint32_t n, uint64_t N) {
    if (r.m.count < MR_SLOTS) r.n[r.m.count] = n, r.N[r.m.count] = N, mr_rings_add(r.m, id, n);
}
ZK_HD static inline int32_t rrr_class_status(uint32_t cls) { return cls < MR_SLOTS ? ZK_OK : cls == RRR_ENC ? ZK_E_BAD_ENCODING : ZK_E_ARG; }
struct RrPlan {
    uint32_t cls;     // ring slot | RRR_ARG | RRR_ENC
    uint32_t head;    // bytes in front of the GKProof section (0 for a refusal)
    uint32_t len;     // the output slot: head + gk(n of the destination ring), 0 for a refusal
    uint32_t other;   // 1: passes rules 1-3 with another n than its destination ring's (the in-place form refuses the call)
};
// Rules 1-3, the first that matches: no byte of a proof whose id is not resident is read, and of no proof a byte beyond its header.
ZK_HD static inline RrPlan rrr_plan_proof(const RrRings& r, const Wire& w, const uint8_t* proofs, uint64_t o0, uint64_t o1, uint32_t id, uint32_t which) {
    RrPlan p{RRR_ARG, 0, 0, 0};
    const uint32_t k = mr_class_of_id(r.m, id);
    if (k >= MR_SLOTS) return p;
    const RrHead h = rr_head(proofs, o0, o1, w);
    if (!h.ok) {
        p.cls = RRR_ENC;
        return p;
    }
    if (which >= r.N[k]) return p;
    p.cls = k, p.head = h.head, p.len = h.head + w.gk_n * r.n[k] + 32, p.other = h.n != r.n[k];
    return p;
}
// The call's decisions, from the census' figures alone and before a byte of out, out_off or the statuses is written: `bytes` = the sum of the slots
// (= out_off[B]), `other` = proofs that pass rules 1-3 with another n than their ring's, in_end = proof_off[B].
ZK_HD static inline zk_status rrr_decide(const uint8_t* proofs, const uint8_t* out, uint64_t out_cap, uint64_t bytes, uint64_t other, uint64_t in_end) {
    const bool in_place = out == proofs;
    if (in_place && other) return ZK_E_ARG;
    if (!in_place && out < proofs + in_end && proofs < out + bytes) return ZK_E_ARG;
    if ((in_place ? in_end : bytes) > out_cap) return ZK_E_BUFFER;
    return ZK_OK;
}
// host-pointer calls: the whole batch in one pass, what the census and the offsets kernel give.  cls, off: B (+ 1) entries or nullptr.
struct RrBatch {
    uint32_t cnt[MR_CLASSES];   // proofs per class
    uint64_t bytes;             // the sum of the slots = out_off[B]
    uint64_t other;             // proofs that pass rules 1-3 with another n than their ring's
    uint64_t in_bytes;          // the end of the last input slot a byte of which is read (a resident id, a readable slot)
};
static inline RrBatch rrr_plan_host(const RrRings& r, const Wire& w, uint64_t B, const uint8_t* proofs, const uint64_t* proof_off, const uint32_t* ids, const uint32_t* which,
                                    uint8_t* cls, uint64_t* off) {
    RrBatch t{};
    for (uint64_t b = 0; b < B; b++) {
        const RrPlan p = rrr_plan_proof(r, w, proofs, proof_off[b], proof_off[b + 1], ids[b], which[b]);
        if (mr_class_of_id(r.m, ids[b]) < MR_SLOTS && rr_slot_readable(proof_off[b], proof_off[b + 1]) && proof_off[b + 1] > t.in_bytes) t.in_bytes = proof_off[b + 1];
        if (cls) cls[b] = (uint8_t)p.cls;
        if (off) off[b] = t.bytes;
        t.cnt[p.cls]++, t.bytes += p.len, t.other += p.other;
    }
    if (off) off[B] = t.bytes;
    return t;
}
