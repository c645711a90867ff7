// In-place update of a resident ring (zk_ctx_update_ring, api.hip): the kernels that have no counterpart in the full build.
//
// Every table of a ring is indexed by key or by block of 256 keys, so a change of k keys in b blocks rewrites k limbs, k per-key tables, b columns of table E and
// of the two digit tables, b leaves and the root.  The tables themselves are rebuilt by the SAME kernels as the full build, handed an index list (k_gk.hip,
// k_gk_mfma.hip, k_ktab.hip, k_hash.hip: launch_*_list); what is left for this file is moving the new keys in:
//   k_ring_scatter      ring[entry[i]] = the uploaded key src[i], reduced exactly like k_ring_load, or a copy of ring entry 0 (padding of a ring whose key 0 stays)
//   k_ktab_copy_entry0  the per-key table of a padding entry is the table of entry 0: copied once entry 0's is final instead of recomputed
//   k_ring_export       ring entries -> 32-byte integers, and k_keys_scatter the new keys over them: the key list of a rebuild when the padded size changes
#include "engine.h"

__global__ void __launch_bounds__(256) k_ring_scatter(const uint8_t* __restrict__ keys, const uint32_t* __restrict__ entry, const uint32_t* __restrict__ src, uint32_t count,
                                                      Soa ring) {
    uint32_t i = gtid();
    if (i >= count) return;
    const uint32_t e = entry[i], k = src[i];
    if (e >= ring.stride) return;
    if (k == ZK_RU_FROM_ENTRY0) {   // (entry 0 is then not in the list: nobody writes what this lane reads)
        soa_st(ring, e, soa_ld<ModQ, 1>(ring, 0));
        return;
    }
    uint32_t w[8];
    load_be32(keys + 32 * (size_t)k, w);
    soa_st(ring, e, fe_from_words256_reduce<ModQ>(w));
}
void launch_ring_scatter(hipStream_t s, const uint8_t* d_keys_be32, const uint32_t* d_entry, const uint32_t* d_src, uint32_t count, const Soa& ring) {
    if (count) hipLaunchKernelGGL(k_ring_scatter, dim3((count + 255) / 256), dim3(256), 0, s, d_keys_be32, d_entry, d_src, count, ring);
}

#define RU_KEY_VEC ((uint32_t)(KTAB_KEY_WORDS / 4))   // 16-byte vectors of one key's table
#define RU_KEY_WGS (RU_KEY_VEC / 256)
static_assert(RU_KEY_VEC % 256 == 0, "a key's table is a whole number of 256-lane vector rows");
__global__ void __launch_bounds__(256) k_ktab_copy_entry0(const uint32_t* __restrict__ entry, uint32_t count, uint32_t* ktab, uint8_t* ok) {
    const uint32_t i = blockIdx.x / RU_KEY_WGS, v = (blockIdx.x % RU_KEY_WGS) * 256 + threadIdx.x;
    if (i >= count) return;
    const uint32_t e = entry[i];
    if (e == 0) return;
    const uint8_t good = ok[0];
    if (v == 0) ok[e] = good;
    if (!good) return;   // entry 0 owns no table (its value is no x-coordinate): neither do its copies
    const uint4* from = (const uint4*)ktab;
    uint4* to = (uint4*)(ktab + (size_t)e * KTAB_KEY_WORDS);
    to[v] = from[v];
}
void launch_ktab_copy_entry0(hipStream_t s, const uint32_t* d_entry, uint32_t count, uint32_t* ktab, uint8_t* ok) {
    if (count) hipLaunchKernelGGL(k_ktab_copy_entry0, dim3(count * RU_KEY_WGS), dim3(256), 0, s, d_entry, count, ktab, ok);
}

__global__ void __launch_bounds__(256) k_ring_export(Soa ring, uint64_t count, uint8_t* out) {
    uint64_t i = gtid();
    if (i >= count) return;
    store_scalar_be(out + 32 * i, soa_ld<ModQ, 1>(ring, (uint32_t)i));
}
void launch_ring_export(hipStream_t s, const Soa& ring, uint64_t count, uint8_t* d_keys_be32) {
    if (count) hipLaunchKernelGGL(k_ring_export, dim3((uint32_t)((count + 255) / 256)), dim3(256), 0, s, ring, count, d_keys_be32);
}
__global__ void __launch_bounds__(256) k_keys_scatter(const uint8_t* __restrict__ keys, const uint32_t* __restrict__ entry, const uint32_t* __restrict__ src, uint32_t count,
                                                      uint8_t* out) {
    uint32_t t = gtid();
    if (t >= count * 8) return;
    const uint32_t i = t >> 3, w = t & 7;
    const uint8_t* from = keys + 32 * (size_t)src[i] + 4 * w;
    uint8_t* to = out + 32 * (size_t)entry[i] + 4 * w;
    for (int b = 0; b < 4; b++) to[b] = from[b];
}
void launch_keys_scatter(hipStream_t s, const uint8_t* d_keys_be32, const uint32_t* d_entry, const uint32_t* d_src, uint32_t count, uint8_t* d_out_be32) {
    if (count) hipLaunchKernelGGL(k_keys_scatter, dim3((count * 8 + 255) / 256), dim3(256), 0, s, d_keys_be32, d_entry, d_src, count, d_out_be32);
}
