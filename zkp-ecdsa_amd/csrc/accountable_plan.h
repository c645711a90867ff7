// Accountable attestations (include/zkattest.h: zk_accountable_*): the one statement of a "ZKC1" bundle's sizes, its header words and its slot walk.  The
// kernels (k_accountable.hip) and the host layer (api_accountable.hip) share these functions.  Nothing here knows HIP: plain g++ compiles it
// (tests/host_arith/host_accountable.cpp).
#pragma once
#include "rering_plan.h"
#include "quorum_plan.h"   // QuorumRings, zkq_ring_entry: what a `_rings` call knows of the context's rings

#define ZKC1_HDR 16
#define ZK_MAGIC_ZKC1 0x31434b5au   // "ZKC1" as a little-endian word
#define ZKC_TAG_BYTES 472u          // a ZKT1 tag (escrow.h: ZKT1_SIZE)
#define ZKC_TAG_MAGIC 0x31544b5au   // "ZKT1" (escrow.h: ZK_MAGIC_ZKT1)

// zk_accountable_proof_max_size: the header, one attestation of at most `proof_max` bytes (zk_proof_max_size), the tag
ZK_HD static inline uint64_t zkc_max_size(uint64_t proof_max) { return proof_max ? ZKC1_HDR + proof_max + ZKC_TAG_BYTES : 0; }
// The `_rings` forms (one resident ring id per bundle).  zkc_capacity_rings: the slot of a bundle that proves over ring `id` -- zk_rings_accountable_proof_max_size
// of that ring, 0 for an id that names no resident ring (or one whose proof_max is 0: no params).  `used` (may be NULL) collects the entries the ids name, as a
// bit set.  A call's out_cap is held against the sum of its bundles' slots; the sum is taken by zkc_capacity_add, which stays at 2^64 - 1 once it is passed:
// a total that cannot be represented is refused as "too small", never wrapped into a small one.
ZK_HD static inline uint64_t zkc_capacity_rings(const QuorumRings& R, uint32_t id, uint32_t* used) {
    const uint32_t r = zkq_ring_entry(R, id);
    if (r == ZKQ_RINGS || !R.proof_max[r]) return 0;
    if (used) *used |= 1u << r;
    return zkc_max_size(R.proof_max[r]);
}
ZK_HD static inline uint64_t zkc_capacity_add(uint64_t sum, uint64_t cap) { return sum + cap < sum ? ~0ull : sum + cap; }
// the sum over a list of ids (the host form's loop; the kernel adds its lanes' slots with atomics, behind zkc_capacity_fits)
ZK_HD static inline uint64_t zkc_capacity_total(const QuorumRings& R, uint64_t B, const uint32_t* ids, uint32_t* used) {
    uint64_t total = 0;
    for (uint64_t b = 0; b < B; b++) total = zkc_capacity_add(total, zkc_capacity_rings(R, ids[b], used));
    return total;
}
// true where B slots of the largest resident ring still fit 64 bits: then no sum over B ids can pass 2^64 - 1, whatever they name
ZK_HD static inline bool zkc_capacity_fits(const QuorumRings& R, uint64_t B) {
    uint64_t most = 0;
    for (uint32_t r = 0; r < R.count && r < ZKQ_RINGS; r++)
        if (R.resident[r] && zkc_max_size(R.proof_max[r]) > most) most = zkc_max_size(R.proof_max[r]);
    return !most || B <= ~0ull / most;
}
// a bundle whose attestation takes att_bytes
ZK_HD static inline uint64_t zkc_size(uint64_t att_bytes) { return ZKC1_HDR + att_bytes + ZKC_TAG_BYTES; }
ZK_HD static inline void zkc_header(uint32_t hw[4], uint32_t total) {   // the 16 header bytes as four words in memory order
    hw[0] = ZK_MAGIC_ZKC1, hw[1] = __builtin_bswap32(total), hw[2] = 0, hw[3] = 0;
}
// What a call may need of the slot [o0, o1) before a byte of it is read: the attestation's bytes if the walk accepts it, else 0 -- from the offsets alone
// (split's att_cap and the verifier's staging are held against the sum of these)
ZK_HD static inline uint64_t zkc_slot_att_bytes(uint64_t o0, uint64_t o1) {
    return rr_slot_readable(o0, o1) && o1 - o0 >= ZKC1_HDR + ZK_HDR + ZKC_TAG_BYTES ? o1 - o0 - ZKC1_HDR - ZKC_TAG_BYTES : 0;
}

// The walk of the bundle in slot [o0, o1): true where the slot passes the encoding rules of zk_accountable_verify_batch -- offsets that ascend and are
// 4-byte aligned, a length that is a multiple of 4, the magic, total_len = the slot's length, two zero reserved words, and one inner header (rr_head's rules
// for the wire layout `w`) that walks from byte 16 exactly to total_len - 472.  att[0..1], where given, receive where the attestation starts and where the
// tag starts (from `bundles`).  16 bytes of the bundle and 16 of the inner header are read, nothing outside the slot.
ZK_HD static inline bool zkc_walk(const uint8_t* bundles, uint64_t o0, uint64_t o1, const Wire& w, uint64_t* att) {
    if (!zkc_slot_att_bytes(o0, o1)) return false;
    uint32_t hw[4];
    __builtin_memcpy(hw, bundles + o0, 16);
    if (hw[0] != ZK_MAGIC_ZKC1 || __builtin_bswap32(hw[1]) != o1 - o0 || hw[2] != 0 || hw[3] != 0) return false;
    const uint64_t pos = o0 + ZKC1_HDR, end = o1 - ZKC_TAG_BYTES;
    if (!rr_head(bundles, pos, end, w).ok) return false;   // (its total_len must be end - pos: one word more or less is refused)
    if (att) att[0] = pos, att[1] = end;
    return true;
}
// zk_accountable_join_batch: the proof in slot [o0, o1) by rr_head's rules and the 16 header bytes of its tag ("ZKT1" | 472 | 0 | 0); the bundle's length, or 0
// where join refuses.  No byte of the tag beyond its header is read, and none of the proof beyond its own.
ZK_HD static inline uint64_t zkc_join_len(const uint8_t* proofs, uint64_t o0, uint64_t o1, const uint8_t* tag, const Wire& w) {
    if (!rr_head(proofs, o0, o1, w).ok || zkc_size(o1 - o0) > 0xffffffffull) return 0;
    uint32_t tw[4];
    __builtin_memcpy(tw, tag, 16);
    if (tw[0] != ZKC_TAG_MAGIC || __builtin_bswap32(tw[1]) != ZKC_TAG_BYTES || tw[2] != 0 || tw[3] != 0) return 0;
    return zkc_size(o1 - o0);
}
