// The resident point index of a ring (include/zkattest.h: zk_rings_escrow_open_batch): the ring's points 4 y_i g and an open-addressed table of key indices
// over them, so that an escrow tag's point 4 (E2 - a E1) is looked up in a few probes whatever the ring's size.  Public data: it depends on g and the ring
// only.  This header is the ONE definition of the layout, the slot function, the insertion and the lookup: the kernels (k_escrow_index.hip) and the host test
// (tests/host_arith/host_escrow_index.cpp, under ZK_HOST_BUILD) compile it, tests/escrow_index_common.py restates the slot function.
//
// Layout.  A ring of nkeys keys has cap = the least power of two >= nkeys entries of points (the ring's padded size: it does not change while
// zk_ctx_update_ring patches in place) and 2 cap slots.  Points: 18 limbs of 30 bits per entry, limb-major -- limb l of entry i at pts[l * cap + i], l = 0..8
// the affine x, 9..17 the affine y, plain canonical, as the normaliser writes them: 72 bytes per entry.  Only entries below nkeys are ever inserted or read.
// Slots: u32 key indices, ESC_INDEX_EMPTY = 0xffffffff for an empty one.
//
// Slot function.  w0, w1 = the two low 32-bit words of the canonical x (bits 0..31 and 32..63);
//     h = w0 * 0x9e3779b1 + w1 * 0x85ebca6b;  h ^= h >> 16;  h *= 0xc2b2ae35;  h ^= h >> 13     (all mod 2^32)
// and the point's home slot is h & (slots - 1).  Probing is linear with wrap-around, bounded by the slot count.
//
// Insertion (one lane per key, any order, concurrently): compare-and-swap on the empty value; where the occupant is the same point, the minimum of the two
// indices stays and the lane stops; otherwise the next slot.  An occupied slot never changes its POINT, and every lane of a point walks the same sequence from
// the same home slot, so every distinct point owns exactly one slot and that slot ends up with the point's lowest index.  Which slot of a cluster a point
// owns depends on the order of the lanes; no lookup result does.  The load is at most 1/2, so every probe sequence ends at an empty slot.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "zkdev.h"

#define ESC_INDEX_EMPTY 0xffffffffu
#define ESC_INDEX_LIMBS 18   // limbs per point: x then y

struct EscIndexRing {        // (part of a kernel argument) one resident ring's index
    uint32_t id;
    uint32_t nkeys;          // entries below it are real keys
    uint32_t mask;           // slots - 1; the points' stride is (mask + 1) / 2
    const uint32_t* pts;
    uint32_t* slots;
};
#define ESC_INDEX_MAX_RINGS 16
struct EscIndexSet {         // (a kernel argument) the resident rings' indexes in ascending id order
    EscIndexRing r[ESC_INDEX_MAX_RINGS];
    uint32_t count;
};

ZK_HOSTDEV uint32_t esc_index_cap(uint64_t nkeys) {   // entries of points; twice as many slots
    uint32_t cap = 1;
    while (cap < nkeys) cap <<= 1;
    return cap;
}
ZK_HOSTDEV uint32_t esc_index_hash(uint32_t w0, uint32_t w1) {
    uint32_t h = w0 * 0x9e3779b1u + w1 * 0x85ebca6bu;
    h ^= h >> 16;
    h *= 0xc2b2ae35u;
    h ^= h >> 13;
    return h;
}
// the home slot from the three low limbs of x (30 bits each): the words are put together as words_from_limbs puts them
ZK_HOSTDEV uint32_t esc_index_home(uint32_t l0, uint32_t l1, uint32_t l2, uint32_t mask) {
    return esc_index_hash(l0 | (l1 << 30), (l1 >> 2) | (l2 << 28)) & mask;
}

#if defined(ZK_HOST_BUILD)   // one thread: the atomics are what they say
inline uint32_t esc_index_cas(uint32_t* p, uint32_t expect, uint32_t v) {
    const uint32_t old = *p;
    if (old == expect) *p = v;
    return old;
}
inline void esc_index_min(uint32_t* p, uint32_t v) {
    if (v < *p) *p = v;
}
#else
ZK_DEV uint32_t esc_index_cas(uint32_t* p, uint32_t expect, uint32_t v) { return atomicCAS(p, expect, v); }
ZK_DEV void esc_index_min(uint32_t* p, uint32_t v) { (void)atomicMin(p, v); }
#endif

ZK_DEV bool esc_index_same(const EscIndexRing& R, uint32_t i, uint32_t j) {
    const uint32_t cap = (R.mask + 1) >> 1;
    uint32_t diff = 0;
#pragma unroll 1
    for (uint32_t l = 0; l < ESC_INDEX_LIMBS; l++) diff |= R.pts[(size_t)l * cap + i] ^ R.pts[(size_t)l * cap + j];
    return diff == 0;
}
// key i < R.nkeys into the slots
ZK_DEV void esc_index_insert(const EscIndexRing& R, uint32_t i) {
    const uint32_t cap = (R.mask + 1) >> 1;
    uint32_t s = esc_index_home(R.pts[i], R.pts[(size_t)cap + i], R.pts[2 * (size_t)cap + i], R.mask);
#pragma unroll 1
    for (uint32_t probe = 0; probe <= R.mask; probe++, s = (s + 1) & R.mask) {
        const uint32_t old = esc_index_cas(R.slots + s, ESC_INDEX_EMPTY, i);
        if (old == ESC_INDEX_EMPTY) return;
        if (old < R.nkeys && esc_index_same(R, old, i)) {
            esc_index_min(R.slots + s, i);
            return;
        }
    }
}
// the lowest index below R.nkeys whose point is (x, y) -- nine canonical limbs each --, ESC_INDEX_EMPTY for none.  An index that is not below nkeys (none is
// ever inserted) is stepped over, so that no table contents make the lookup read outside the points.
ZK_DEV uint32_t esc_index_lookup(const EscIndexRing& R, const uint32_t x[9], const uint32_t y[9]) {
    const uint32_t cap = (R.mask + 1) >> 1;
    uint32_t s = esc_index_home(x[0], x[1], x[2], R.mask);
#pragma unroll 1
    for (uint32_t probe = 0; probe <= R.mask; probe++, s = (s + 1) & R.mask) {
        const uint32_t i = R.slots[s];
        if (i == ESC_INDEX_EMPTY) return ESC_INDEX_EMPTY;
        if (i >= R.nkeys || R.pts[i] != x[0]) continue;   // the low limb of x screens before the other seventeen are compared
        uint32_t diff = 0;
#pragma unroll
        for (int l = 1; l < 9; l++) diff |= R.pts[(size_t)l * cap + i] ^ x[l];
#pragma unroll
        for (int l = 0; l < 9; l++) diff |= R.pts[(size_t)(9 + l) * cap + i] ^ y[l];
        if (!diff) return i;
    }
    return ESC_INDEX_EMPTY;
}
