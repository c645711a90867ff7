// Quorum proofs (include/zkattest.h: zk_quorum_*): the one statement of a "ZKQ1" bundle's pair order, its size rules and its header walk.  The kernels
// (k_quorum.hip) and the host layer (api_quorum.hip) share these functions.  Nothing here knows HIP: plain g++ compiles it (tests/host_arith/host_quorum.cpp).
#pragma once
#include "rering_plan.h"

#define ZKQ1_HDR 16
#define ZK_MAGIC_ZKQ1 0x31514b5au   // "ZKQ1" as a little-endian word
#define ZKQ_KMIN 2u
#define ZKQ_KMAX 16u
#define ZKQ_PAIR_BYTES 744u         // a ZKD1 proof (distinct.h: ZKD1_SIZE)

ZK_HD static inline bool zkq_k_ok(uint32_t k) { return k >= ZKQ_KMIN && k <= ZKQ_KMAX; }
// pairs of a quorum of k members, 0 for a k outside 2..16
ZK_HD static inline uint32_t zkq_pairs(uint32_t k) { return zkq_k_ok(k) ? k * (k - 1) / 2 : 0; }
// The pair order is Engine.distinct_pairs' lexicographic one: (0,1), (0,2), ..., (0,k-1), (1,2), ..., (k-2,k-1).  Row i holds k - 1 - i pairs.
ZK_HD static inline uint32_t zkq_rank(uint32_t k, uint32_t i, uint32_t j) { return i * (2 * k - i - 1) / 2 + (j - i - 1); }   // 0 <= i < j < k
ZK_HD static inline void zkq_unrank(uint32_t k, uint32_t p, uint32_t& i, uint32_t& j) {   // 0 <= p < zkq_pairs(k): a short loop over the rows, no table
    uint32_t row = 0, r = p;
    while (row + 2 < k && r >= k - 1 - row) r -= k - 1 - row, row++;
    i = row, j = row + 1 + r;
}
// zk_quorum_proof_max_size: the header, k attestations of at most `proof_max` bytes (zk_proof_max_size), the pairs' proofs
ZK_HD static inline uint64_t zkq_max_size(uint32_t k, uint64_t proof_max) {
    return zkq_k_ok(k) && proof_max ? ZKQ1_HDR + (uint64_t)k * proof_max + (uint64_t)zkq_pairs(k) * ZKQ_PAIR_BYTES : 0;
}
// The `_rings` forms (one resident ring id per member): what a call knows of the context's rings, and the capacity a quorum's slot needs.  At most ZKQ_RINGS
// entries (ZK_MAX_RINGS); an entry with resident = 0, like an id that has no entry, names no ring.
#define ZKQ_RINGS 16u
struct QuorumRings {   // (a kernel argument)
    uint32_t count;
    uint32_t id[ZKQ_RINGS], resident[ZKQ_RINGS], proof_max[ZKQ_RINGS];   // proof_max: zk_ring_proof_max_size of the ring
};
// the entry of `id`, ZKQ_RINGS where it names no resident ring
ZK_HD static inline uint32_t zkq_ring_entry(const QuorumRings& R, uint32_t id) {
    for (uint32_t r = 0; r < R.count && r < ZKQ_RINGS; r++)
        if (R.resident[r] && R.id[r] == id) return r;
    return ZKQ_RINGS;
}
// The slot of a quorum whose member i proves over ring ids[i]: the header, every member's ring's largest proof (0 for an id that is not resident), the pairs'
// proofs.  0 for a k outside 2..16.  `used` (may be NULL) collects the entries the ids name, as a bit set.  The sum cannot wrap: 16 proofs of < 2^32 bytes.
ZK_HD static inline uint64_t zkq_capacity_rings(const QuorumRings& R, uint32_t k, const uint32_t* ids, uint32_t* used) {
    if (!zkq_k_ok(k)) return 0;
    uint64_t cap = ZKQ1_HDR + (uint64_t)zkq_pairs(k) * ZKQ_PAIR_BYTES;
    for (uint32_t i = 0; i < k; i++) {
        const uint32_t r = zkq_ring_entry(R, ids[i]);
        if (r == ZKQ_RINGS) continue;
        cap += R.proof_max[r];
        if (used) *used |= 1u << r;
    }
    return cap;
}
// zk_rings_quorum_proof_max_size: the same sum, but 0 as soon as one id is not resident
ZK_HD static inline uint64_t zkq_max_size_rings(const QuorumRings& R, uint32_t k, const uint32_t* ids) {
    if (!zkq_k_ok(k)) return 0;
    for (uint32_t i = 0; i < k; i++)
        if (zkq_ring_entry(R, ids[i]) == ZKQ_RINGS || !R.proof_max[zkq_ring_entry(R, ids[i])]) return 0;
    return zkq_capacity_rings(R, k, ids, nullptr);
}
// a bundle whose k attestations take att_bytes
ZK_HD static inline uint64_t zkq_size(uint32_t k, uint64_t att_bytes) { return ZKQ1_HDR + att_bytes + (uint64_t)zkq_pairs(k) * ZKQ_PAIR_BYTES; }
ZK_HD static inline void zkq_header(uint32_t hw[4], uint32_t total, uint32_t k) {   // the 16 header bytes as four words in memory order
    hw[0] = ZK_MAGIC_ZKQ1, hw[1] = __builtin_bswap32(total), hw[2] = __builtin_bswap32(k), hw[3] = 0;
}

// The header walk of the bundle in slot [o0, o1) for a call of k members per quorum: true where the slot passes the encoding rules of zk_quorum_verify_batch --
// offsets that ascend and are 4-byte aligned, a length that is a multiple of 4, the magic, total_len = the slot's length, the header's k = the call's, a zero
// reserved word, and k inner headers (rr_head's rules for the wire layout `w`) that walk from byte 16 exactly to total_len - 744 P.  m_off, where given,
// receives the members' k + 1 offsets (from `bundles`; m_off[k] = where the pairs' proofs start).  No byte outside the slot is read, and of a member no byte
// beyond its first 16.
ZK_HD static inline bool zkq_walk(const uint8_t* bundles, uint64_t o0, uint64_t o1, uint32_t k, const Wire& w, uint64_t* m_off) {
    if (!zkq_k_ok(k) || o1 < o0 || (o0 & 3) || ((o1 - o0) & 3) || o1 - o0 < ZKQ1_HDR || o1 - o0 > 0xffffffffull) return false;
    uint32_t hw[4];
    __builtin_memcpy(hw, bundles + o0, 16);
    if (hw[0] != ZK_MAGIC_ZKQ1 || __builtin_bswap32(hw[1]) != o1 - o0 || __builtin_bswap32(hw[2]) != k || hw[3] != 0) return false;
    const uint64_t tail = (uint64_t)zkq_pairs(k) * ZKQ_PAIR_BYTES;
    if (o1 - o0 < ZKQ1_HDR + tail) return false;
    const uint64_t end = o1 - tail;
    uint64_t pos = o0 + ZKQ1_HDR;
    for (uint32_t i = 0; i < k; i++) {
        if (end - pos < ZK_HDR) return false;
        uint32_t len_be;
        __builtin_memcpy(&len_be, bundles + pos + 4, 4);
        const uint64_t len = __builtin_bswap32(len_be);
        if (len > end - pos || !rr_head(bundles, pos, pos + len, w).ok) return false;
        if (m_off) m_off[i] = pos;
        pos += len;
    }
    if (pos != end) return false;
    if (m_off) m_off[k] = end;
    return true;
}
