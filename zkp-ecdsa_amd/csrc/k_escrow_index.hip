// The resident point index of a ring (escrow_index.h; include/zkattest.h: zk_rings_escrow_open_batch): the insertion of a ring's points into its slots, the
// lookup of a batch of tags' points in the rings their ids name, and the two copies zk_ctx_update_ring's patch needs around the point builders.  The points
// themselves come from k_escrow.hip's and k_tom.hip's kernels.  No field arithmetic here: everything compares canonical limbs.
#include "escrow.h"

// One lane per key below R.nkeys (escrow_index.h: esc_index_insert).  The slots were filled with ESC_INDEX_EMPTY before.
__global__ void __launch_bounds__(256) k_escrow_index_insert(EscIndexRing R) {
    const uint32_t i = gtid();
    if (i >= R.nkeys) return;
    esc_index_insert(R, i);
}
void launch_escrow_index_insert(hipStream_t s, const EscIndexRing& R) {
    if (R.nkeys) hipLaunchKernelGGL(k_escrow_index_insert, dim3((R.nkeys + 255) / 256), dim3(256), 0, s, R);
}
// One lane per tag, behind the ladder and the normaliser: the tag's point 4 (E2 - a E1) looked up in the ring its id names, or in every resident ring in
// ascending id order.  The descriptors are a kernel argument and the loop over them is uniform, so a lane's ring costs no read-back, census or permutation.
// Status: ZK_E_ARG for an id that is neither resident nor ZK_ESCROW_RING_ANY, else what the ladder's kernel decided; both outputs stay "none" unless the
// status is 0 and a ring holds the point.
__global__ void __launch_bounds__(256) k_escrow_index_lookup(EscIndexSet S, EscrowOpen O, uint64_t B, const uint32_t* ring_ids, uint32_t* ring_out, uint32_t* index,
                                                             int32_t* status) {
    const uint64_t b = gtid();
    if (b >= B) return;
    const uint32_t want = ring_ids[b];
    const int32_t st = O.st[b];
    const bool any = want == ZK_ESCROW_RING_ANY;
    bool known = any;
    uint32_t x[9], y[9];
#pragma unroll
    for (int l = 0; l < 9; l++) x[l] = O.T.ax.p[(size_t)l * O.T.ax.stride + b], y[l] = O.T.ay.p[(size_t)l * O.T.ay.stride + b];
    uint32_t found = ESC_INDEX_EMPTY, ring = ESC_INDEX_EMPTY;
#pragma unroll 1
    for (uint32_t d = 0; d < S.count; d++) {
        const bool mine = want == S.r[d].id;
        known = known || mine;
        if (st != ZK_OK || found != ESC_INDEX_EMPTY || !(mine || any)) continue;
        const uint32_t i = esc_index_lookup(S.r[d], x, y);
        if (i != ESC_INDEX_EMPTY) found = i, ring = S.r[d].id;
    }
    status[b] = known ? st : ZK_E_ARG;
    ring_out[b] = known ? ring : ESC_INDEX_EMPTY;
    index[b] = known ? found : ESC_INDEX_EMPTY;
}
void launch_escrow_index_lookup(hipStream_t s, const EscIndexSet& S, const EscrowOpen& O, uint64_t B, const uint32_t* ring_ids, uint32_t* ring_out, uint32_t* index,
                                int32_t* status) {
    hipLaunchKernelGGL(k_escrow_index_lookup, dim3((uint32_t)((B + 255) / 256)), dim3(256), 0, s, S, O, B, ring_ids, ring_out, index, status);
}
// zk_ctx_update_ring's patch: the ring's entries ent[0 .. n-1] as the openings (y, 0) of slots 0 .. n - 1 ...
__global__ void __launch_bounds__(256) k_escrow_index_gather(Soa ring, const uint32_t* ent, uint32_t n, TomList L) {
    const uint32_t j = gtid();
    if (j >= n) return;
    const uint32_t e = ent[j] < ring.stride ? ent[j] : 0;   // (the host's entries are below the padded size)
    soa_st(L.v, j, soa_ld<ModQ, 1>(ring, e)), soa_st(L.r, j, fe_zero<ModQ>());
}
void launch_escrow_index_gather(hipStream_t s, const Soa& ring, const uint32_t* ent, uint32_t n, const TomList& L) {
    hipLaunchKernelGGL(k_escrow_index_gather, dim3((n + 255) / 256), dim3(256), 0, s, ring, ent, n, L);
}
// ... and their normalised points from slots 0 .. n - 1 into entries ent[0 .. n-1] of the resident points (cap entries; the caller's entries are below it)
__global__ void __launch_bounds__(256) k_escrow_index_scatter(TomList L, const uint32_t* ent, uint32_t n, uint32_t* pts, uint32_t cap) {
    const uint32_t j = gtid();
    if (j >= n) return;
    const uint32_t e = ent[j];
    if (e >= cap) return;
#pragma unroll
    for (int l = 0; l < 9; l++) pts[(size_t)l * cap + e] = L.ax.p[(size_t)l * L.ax.stride + j], pts[(size_t)(9 + l) * cap + e] = L.ay.p[(size_t)l * L.ay.stride + j];
}
void launch_escrow_index_scatter(hipStream_t s, const TomList& L, const uint32_t* ent, uint32_t n, uint32_t* pts, uint32_t cap) {
    hipLaunchKernelGGL(k_escrow_index_scatter, dim3((n + 255) / 256), dim3(256), 0, s, L, ent, n, pts, cap);
}
