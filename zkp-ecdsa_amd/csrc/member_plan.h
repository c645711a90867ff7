// Mixed-ring membership calls (include/zkattest.h: zk_member_*_batch_rings): the index arithmetic of a call's plan.  A ZKM1 proof's size depends on its
// ring's n alone, so the class of every proof -- the slot of its ring, MR_UNKNOWN for an id that is not resident, MR_BAD for a slot the verifier refuses by
// its geometry -- fixes every proof's place in the output before anything is proved.  The classing and offsets kernels (k_member_rings.hip) and the host
// layer (api_member.hip) share these functions.  Nothing here knows HIP: plain g++ compiles it (tests/host_arith/host_member_rings.cpp).
#pragma once
#include "wire.h"

#define MR_BLOCK 256                // proofs per workgroup of the classing kernel
#define MR_SLOTS 16                 // resident rings of a context (ZK_MAX_RINGS)
#define MR_UNKNOWN MR_SLOTS         // the id is not resident: ZK_E_ARG, a zero-length slot
#define MR_BAD (MR_SLOTS + 1)       // verifier only: the slot's length, alignment or order refuses the proof (ZK_E_BAD_ENCODING, no byte of it is read)
#define MR_CLASSES (MR_SLOTS + 2)

struct MrRings {   // (a kernel argument) the resident rings in slot order: id and ZKM1 size; size[MR_UNKNOWN] = size[MR_BAD] = 0
    uint32_t count;
    uint32_t id[MR_SLOTS];
    uint32_t size[MR_CLASSES];
};
ZK_HD static inline void mr_rings_clear(MrRings& r) {
    r.count = 0;
    for (uint32_t s = 0; s < MR_SLOTS; s++) r.id[s] = 0;
    for (uint32_t s = 0; s < MR_CLASSES; s++) r.size[s] = 0;
}
ZK_HD static inline void mr_rings_add(MrRings& r, uint32_t id, uint32_t n) {
    if (r.count < MR_SLOTS) r.id[r.count] = id, r.size[r.count] = (uint32_t)zkm1_size(n), r.count++;
}
ZK_HD static inline uint32_t mr_class_of_id(const MrRings& r, uint32_t id) {
    uint32_t k = MR_UNKNOWN;
    for (uint32_t s = 0; s < MR_SLOTS; s++)
        if (s < r.count && r.id[s] == id) k = s;
    return k;
}
// the verifier's slot [o0, o1) of a batch whose bytes end at o_end, for a ring whose proofs take `size` bytes
ZK_HD static inline bool mr_slot_ok(uint64_t o0, uint64_t o1, uint64_t o_end, uint32_t size) { return o1 >= o0 && o1 <= o_end && !(o0 & 3) && o1 - o0 == size; }
// bytes of cnt[k] proofs of every class k: a batch's total, or (cnt = how many proofs of each class lie before a workgroup) that workgroup's first offset
ZK_HD static inline uint64_t mr_bytes(const uint32_t* cnt /*[MR_CLASSES]*/, const MrRings& r) {
    uint64_t sum = 0;
    for (uint32_t k = 0; k < MR_CLASSES; k++) sum += (uint64_t)cnt[k] * r.size[k];
    return sum;
}
static inline bool mr_fits(uint64_t total, uint64_t out_cap) { return total <= out_cap; }
// host-pointer calls: classes, per-class counts and offsets of a whole batch in one pass (off[B] = the bytes of the batch)
static inline void mr_plan_host(const MrRings& r, uint64_t B, const uint32_t* ids, uint8_t* cls /*B or nullptr*/, uint32_t* cnt /*[MR_CLASSES]*/, uint64_t* off /*B+1 or nullptr*/) {
    uint64_t run = 0;
    for (uint32_t k = 0; k < MR_CLASSES; k++) cnt[k] = 0;
    for (uint64_t b = 0; b < B; b++) {
        const uint32_t k = mr_class_of_id(r, ids[b]);
        if (cls) cls[b] = (uint8_t)k;
        if (off) off[b] = run;
        cnt[k]++, run += r.size[k];
    }
    if (off) off[B] = run;
}
// one resident class and nothing else: the class whose ring the one-ring pipeline runs on, MR_CLASSES otherwise
static inline uint32_t mr_single_class(const uint32_t* cnt, const MrRings& r) {
    uint32_t used = 0, last = MR_CLASSES;
    for (uint32_t k = 0; k < r.count; k++)
        if (cnt[k]) used++, last = k;
    return used == 1 && !cnt[MR_UNKNOWN] && !cnt[MR_BAD] ? last : MR_CLASSES;
}
// windows: at most 2 x chunk x lanes proofs of one ring at a time, no more than the largest class holds
static inline uint32_t mr_window_cap(uint32_t chunk, uint32_t lanes, const uint32_t* cnt, const MrRings& r) {
    uint32_t most = 1;
    for (uint32_t k = 0; k < r.count; k++)
        if (cnt[k] > most) most = cnt[k];
    const uint64_t cap = 2ull * (chunk ? chunk : 1) * (lanes ? lanes : 1);
    return (uint32_t)(cap < most ? cap : most);
}
static inline uint32_t mr_window_count(uint32_t n, uint32_t cap) { return (n + cap - 1) / cap; }
// window w of a class of n proofs: its first place in the class's `sel` list and how many proofs it takes
static inline void mr_window(uint32_t n, uint32_t cap, uint32_t w, uint32_t* first, uint32_t* cnt) {
    const uint64_t f = (uint64_t)w * cap;
    *first = (uint32_t)(f < n ? f : n);
    *cnt = n - *first < cap ? n - *first : cap;
}
