// Witness screen (include/zkattest.h: zk_screen_batch): where is the signer's key in the ring, and does the ECDSA signature verify?
//
// The prover's front end (k_p256.hip: k_front*) recovers R = u1 G + u2 pk like the reference (src/zkpAttestList.ts:124-131, "First we do a signature
// verification to recover R") and, like it, never compares R.x with r.  The screen makes that comparison, for a few dozen point additions per witness:
//   k_screen_init     which_out, flags and the scratch of a chunk before the first ring's pass
//   k_screen_lookup   find mode: blocks of 256 witnesses against LDS tiles of limb 0 of the ring's resident limbs; a limb-0 hit is compared at full width
//                     and the lowest index kept (atomicMin over the ring segments of a witness block)
//   k_screen_front    key check, signature range, lookup verdict, the scalars u1 = z / s, u2 = r / s mod n (ONE inversion, of s), the choice of the path
//   k_screen_table    u1 * G by the fixed-base comb; off the key-table path also 1..8 times pk
//   k_screen_walk     u2 * pk through the key's table (33 gathered additions) or the 65-window walk, R, and X == r Z (curve.h: p256_x_is_r_mod_n)
// The three ECDSA kernels are split like k_front / k_front_table / k_front_walk so that no live set exceeds 256 registers; between them the values live in
// the witness's scratch area.  The table sums and the walk are the prover's own device functions (rtab.h, ktab.h): ZK_ADD_IF / p256_select, so the uniform
// build has no digit-dependent skip here either.  Branches below depend on the public key, the ring and the range of (r, s) only.
// A chunk of at most ZK_SCREEN_CO_MAX witnesses (engine.h) takes the last two on cooperating waves instead, one workgroup per witness:
//   k_screen_table_co key-table path: four waves sum a quarter of the windows of G's comb and of the key's table each
//   k_screen_walk_co  walk path: wave 0 builds 1..8 times pk in LDS and walks u2's digits while waves 1..3 sum u1 * G from the comb
// Both end with the verdict of k_screen_walk, taken by one lane on the normalised rows of R.
#include <algorithm>
#include "rtab.h"
#include "coop_sums.h"   // the sums and the walk of a chunk of a few witnesses on cooperating waves (k_screen_table_co, k_screen_walk_co)

ZK_DEV bool scr_mine(const ScreenIn& in, const ScreenRing& G, uint32_t b) { return b < in.count && (!in.ids || in.ids[b] == G.id); }
ZK_DEV bool scr_ring_is(const ScreenRing& G, uint32_t i, const Fe<ModQ, 1>& x) {
    bool same = true;
#pragma unroll
    for (int l = 0; l < NLIMB; l++) same = same && G.ring.p[(size_t)l * G.ring.stride + i] == x.l[l];
    return same;
}

__global__ void __launch_bounds__(256) k_screen_init(ScreenIn in, uint32_t* scratch) {
    const uint32_t b = gtid();
    if (b >= in.count) return;
    in.which_out[b] = ZK_WHICH_NONE;   // the lookup's atomicMin starts from it; a witness whose ring is not resident keeps it
    in.flags[b] = in.ids ? ZK_SCREEN_RING_NOT_RESIDENT : 0;   // a pass of the witness's ring replaces it
    scr_area(scratch, b)[SCR_USE] = SCR_SKIP;
}

// blockIdx.x: 256 witnesses; blockIdx.y: a segment of seg_tiles tiles of the ring's caller keys [0, nkeys) -- the padding is never searched
__global__ void __launch_bounds__(256) k_screen_lookup(ScreenRing G, ScreenIn in, uint32_t seg_tiles) {
    __shared__ __align__(16) uint32_t tile[SCR_TILE];
    const uint32_t b = gtid();
    const bool live = scr_mine(in, G, b);
    Fe<ModQ, 1> x = fe_zero<ModQ>();
    uint32_t x0 = SCR_NO_X;
    if (live) {
        uint32_t xw[8];
        load_be32(in.pk + 64 * (size_t)b, xw);
        x = fe_from_words256_reduce<ModQ>(xw);   // keyToInt's value: pk.x mod p
        x0 = x.l[0];
    }
    if (!__syncthreads_or(live)) return;
    uint32_t best = ZK_WHICH_NONE;
#pragma unroll 1
    for (uint32_t t = blockIdx.y * seg_tiles; t < (blockIdx.y + 1) * seg_tiles; t++) {
        const uint32_t base = t * SCR_TILE;
        if (base >= G.nkeys) break;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < SCR_TILE; i += 256) tile[i] = base + i < G.nkeys ? G.ring.p[base + i] : SCR_PAD;
        __syncthreads();
        const uint4* t4 = (const uint4*)tile;
#pragma unroll 4
        for (uint32_t j = 0; j < SCR_TILE / 4; j++) {
            const uint4 v = t4[j];   // every lane reads the same address: one broadcast per four keys
            if (v.x == x0 || v.y == x0 || v.z == x0 || v.w == x0) {
                const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    const uint32_t i = base + 4 * j + k;   // ascending: the first full match is the segment's lowest
                    if (vv[k] == x0 && i < best && scr_ring_is(G, i, x)) best = i;
                }
            }
        }
    }
    if (best != ZK_WHICH_NONE) atomicMin(&in.which_out[b], best);
}

__global__ void __launch_bounds__(64, 2) k_screen_front(ScreenRing G, ScreenIn in, uint32_t* scratch) {
    const uint32_t b = gtid();
    if (!scr_mine(in, G, b)) return;
    uint32_t xw[8], yw[8], zw[8], rw[8], sw[8];
    load_be32(in.pk + 64 * (size_t)b, xw);
    load_be32(in.pk + 64 * (size_t)b + 32, yw);
    load_be32(in.msg + 32 * (size_t)b, zw);
    load_be32(in.sig + 64 * (size_t)b, rw);
    load_be32(in.sig + 64 * (size_t)b + 32, sw);
    uint32_t fl = 0;
    // deserializePoint (weier.ts:74-89), the prover's own key check (k_front)
    const Fe<ModQ, 1> pkx = fe_from_words256_reduce<ModQ>(xw), pky = fe_from_words256_reduce<ModQ>(yw);
    P256Aff pk;
    pk.x = fe_to_mont(pkx), pk.y = fe_to_mont(pky);
    if (!p256_on_curve(pk)) fl |= ZK_SCREEN_KEY_NOT_ON_CURVE;
    // FIPS 186: r, s in [1, n - 1] as 256-bit integers (the prover reduces them mod n instead)
    uint32_t ro = 0, so = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) ro |= rw[i], so |= sw[i];
    if (!ro || !so || words_geq<8>(rw, ModN::mod32) || words_geq<8>(sw, ModN::mod32)) fl |= ZK_SCREEN_SIG_RANGE;
    // the lookup's verdict: find mode left the lowest index or ZK_WHICH_NONE in which_out; check mode compares the named entry (padding included)
    const uint32_t wo = in.which ? in.which[b] : in.which_out[b];
    if (in.which) in.which_out[b] = wo;
    const bool in_ring = in.which ? (wo < G.N && scr_ring_is(G, wo, pkx)) : wo != ZK_WHICH_NONE;
    if (!in_ring) fl |= ZK_SCREEN_NOT_IN_RING;
    in.flags[b] = fl;
    if (fl & (ZK_SCREEN_KEY_NOT_ON_CURVE | ZK_SCREEN_SIG_RANGE)) return;   // (the area keeps SCR_SKIP)
    // u1 = z / s, u2 = r / s mod n (zkpAttestList.ts:119-127); s != 0 here
    const Fn2 z = fe_to_mont(fe_from_words256_reduce<ModN>(zw));
    const Fn2 r = fe_to_mont(fe_from_words256_reduce<ModN>(rw));
    const Fn2 sinv = fe_inv<ModN>(fe_to_mont(fe_from_words256_reduce<ModN>(sw)));
    const Fe<ModN, 1> u1 = fe_from_mont(sinv * z), u2 = fe_from_mont(sinv * r);
    uint32_t* area = scr_area(scratch, b);
    uint32_t use = 0;
    const uint32_t* kt = nullptr;
    if (G.ktab && in_ring && G.ktab_ok[wo]) {   // the key's table was built for one of the two roots: + / - by pk.y
        kt = G.ktab + (size_t)wo * KTAB_KEY_WORDS;
        use = fe_eq(pk.y, ld_ktab(kt).y) ? 1 : 2;
    }
    words_from_limbs<8>(area + SCR_U1, u1.l);
    uint32_t u2w[8];
    words_from_limbs<8>(u2w, u2.l);
#pragma unroll
    for (int i = 0; i < 8; i++) area[SCR_U2 + i] = u2w[i];
    front_recode(u2w, (uint8_t*)(area + SCR_DIG));
#pragma unroll
    for (int l = 0; l < NLIMB; l++) area[SCR_PK + l] = pk.x.l[l], area[SCR_PK + NLIMB + l] = pk.y.l[l];
    *(const uint32_t**)(area + SCR_KT) = kt;
    area[SCR_USE] = use;
}

__global__ void __launch_bounds__(64, 2) k_screen_table(DevParams P, uint32_t count, uint32_t* scratch) {
    const uint32_t b = gtid();
    if (b >= count) return;
    uint32_t* area = scr_area(scratch, b);
    const uint32_t use = area[SCR_USE];
    if (use == SCR_SKIP) return;
    if (!use) {
        P256Aff pk;
#pragma unroll
        for (int l = 0; l < NLIMB; l++) pk.x.l[l] = area[SCR_PK + l], pk.y.l[l] = area[SCR_PK + NLIMB + l];
        front_pk_multiples(area, pk);
    }
    uint32_t kw[8];
#pragma unroll
    for (int i = 0; i < 8; i++) kw[i] = area[SCR_U1 + i];
    st_rtab(area + 8 * RTAB_ENTRY_WORDS, p256_fixed_mul(P.pfix_G, kw));
}

__global__ void __launch_bounds__(64, 2) k_screen_walk(ScreenIn in, uint32_t* scratch) {
    const uint32_t b = gtid();
    if (b >= in.count) return;
    const uint32_t* area = scr_area(scratch, b);
    const uint32_t use = area[SCR_USE];
    if (use == SCR_SKIP) return;
    P256Pt R;
    if (use) {
        uint32_t kw[8];
#pragma unroll
        for (int i = 0; i < 8; i++) kw[i] = area[SCR_U2 + i];
        R = p256_ktab_mul_acc(ld_rtab(area + 8 * RTAB_ENTRY_WORDS), *(const uint32_t* const*)(area + SCR_KT), kw, use == 2);
    } else {
        const P256Pt acc = front_walk(area, (const uint8_t*)(area + SCR_DIG));   // (u1 * G is loaded behind the walk: it would sit in 27 registers through it)
        R = p256_add(ld_rtab(area + 8 * RTAB_ENTRY_WORDS), acc);
    }
    uint32_t rw[8];
    load_be32(in.sig + 64 * (size_t)b, rw);
    Fe<ModN, 1> r;   // in [1, n): k_screen_front checked the range
    limbs_from_words<8>(r.l, rw);
    if (!p256_x_is_r_mod_n(R, r)) in.flags[b] |= ZK_SCREEN_SIG_INVALID;
}

// ---------------------------------------------------------------- a chunk of a few witnesses: the point arithmetic on cooperating waves (coop.h, coop_sums.h)
// One workgroup of four waves per witness; k_screen_init / lookup / front have run as for any chunk and the workgroup reads their results from the witness's
// area.  Same group element R as the one-lane kernels (other projective coordinates), hence the same verdict; nothing witness-derived leaves the area and LDS.
// the verdict both paths end with (k_screen_walk's last lines): wave 0 hands the exact limbs of R's rows to its lane 0
ZK_DEV void scr_co_verdict(const CoP256& R, uint32_t* rsum /* LDS, 64 words */, const ScreenIn& in, uint32_t b) {
    const uint32_t lane = threadIdx.x & 63u;
    rsum[lane] = co_normalize(R.v).v;
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    if (lane) return;
    P256Pt Rp;
#pragma unroll
    for (int l = 0; l < NLIMB; l++) Rp.x.l[l] = rsum[l], Rp.y.l[l] = rsum[16 + l], Rp.z.l[l] = rsum[32 + l];
    uint32_t rw[8];
    load_be32(in.sig + 64 * (size_t)b, rw);
    Fe<ModN, 1> r;   // in [1, n): k_screen_front checked the range
    limbs_from_words<8>(r.l, rw);
    if (!p256_x_is_r_mod_n(Rp, r)) in.flags[b] |= ZK_SCREEN_SIG_INVALID;   // R = identity: Z reduces to zero, no x-coordinate
}
// use 1 / 2: R = u1 G + u2 pk, wave q takes windows [4 q, 4 q + 4) of G's comb and [9 q, 9 q + 9) of the key's table (k_front_co's waves 0..3)
__global__ void __launch_bounds__(256) k_screen_table_co(DevParams P, ScreenIn in, uint32_t* scratch) {
    __shared__ uint32_t part[3][64];
    __shared__ uint32_t rsum[64];
    const uint32_t b = blockIdx.x, q = threadIdx.x >> 6;
    const uint32_t* area = scr_area(scratch, b);
    const uint32_t use = area[SCR_USE];
    if (use != 1 && use != 2) return;   // (uniform for the workgroup)
    const CoU32 mj = co_limbs(ModQ::mod);
    uint32_t kw[8];
#pragma unroll
    for (int i = 0; i < 8; i++) kw[i] = area[SCR_U1 + i];
    constexpr uint32_t gper = (PFIX_NWIN + 3) / 4, kper = (KTAB_NWIN + 3) / 4;
    CoP256 acc = co_fixed_mul_range(co_p256_identity(), P.pfix_G, kw, q * gper, gper, mj);
#pragma unroll
    for (int i = 0; i < 8; i++) kw[i] = area[SCR_U2 + i];
    acc = co_ktab_mul_range(acc, *(const uint32_t* const*)(area + SCR_KT), kw, use == 2, q * kper, kper, mj);
    acc = co_wg4_sum(acc, part, q, mj);
    if (q) return;
    scr_co_verdict(acc, rsum, in, b);
}
// use 0: wave 0 owns the chain -- 1..8 times pk (LDS), the 65 digits of u2 --; waves 1..3 sum u1 * G from the comb meanwhile (five windows each), wave 1
// adds the three parts up, and ONE addition joins the two behind the walk
__global__ void __launch_bounds__(256) k_screen_walk_co(DevParams P, ScreenIn in, uint32_t* scratch) {
    __shared__ uint32_t mult[CO_WALK_MULT_WORDS];
    __shared__ uint32_t part[2][64];
    __shared__ uint32_t u1g[64];
    __shared__ uint32_t rsum[64];
    const uint32_t b = blockIdx.x, q = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t* area = scr_area(scratch, b);
    if (area[SCR_USE] != 0) return;   // (uniform for the workgroup)
    const CoU32 mj = co_limbs(ModQ::mod);
    CoP256 acc;
    if (!q) {
        CoP256 pk;
        pk.v = co_load_pfix(area + SCR_PK);   // the comb entries' format: nine Montgomery limbs of x, nine of y
        co_front_pk_multiples(mult, pk, mj);
    } else {
        uint32_t kw[8];
#pragma unroll
        for (int i = 0; i < 8; i++) kw[i] = area[SCR_U1 + i];
        constexpr uint32_t gper = (PFIX_NWIN + 2) / 3;
        acc = co_fixed_mul_range(co_p256_identity(), P.pfix_G, kw, (q - 1) * gper, gper, mj);
        if (q > 1) part[q - 2][lane] = acc.v.v;
    }
    __syncthreads();
    if (!q) acc = co_front_walk(mult, (const uint8_t*)(area + SCR_DIG), mj);
    else if (q == 1) {
#pragma unroll 1
        for (uint32_t k = 0; k < 2; k++) {
            CoP256 o;
            o.v.v = part[k][lane];
            acc = co_p256_add(acc, o, mj);
        }
        u1g[lane] = acc.v.v;
    }
    __syncthreads();
    if (q) return;
    CoP256 g;
    g.v.v = u1g[lane];
    scr_co_verdict(co_p256_add(g, acc, mj), rsum, in, b);
}

void launch_screen_init(hipStream_t s, const ScreenIn& in, uint32_t* scratch) {
    hipLaunchKernelGGL(k_screen_init, dim3((in.count + 255) / 256), dim3(256), 0, s, in, scratch);
}
// one ring's pass over the chunk: the lookup (find mode only) ...
void launch_screen_lookup(hipStream_t s, const ScreenRing& G, const ScreenIn& in) {
    if (in.which) return;
    // enough workgroups for the GPU whatever the number of witnesses: a witness block's share of the ring is cut into up to 65 535 segments
    const uint32_t wblocks = (in.count + 255) / 256, tiles = (G.nkeys + SCR_TILE - 1) / SCR_TILE;
    uint32_t nseg = std::min<uint32_t>(std::min<uint32_t>(tiles, 65535u), (2048 + wblocks - 1) / wblocks);
    const uint32_t seg_tiles = (tiles + nseg - 1) / nseg;
    nseg = (tiles + seg_tiles - 1) / seg_tiles;
    hipLaunchKernelGGL(k_screen_lookup, dim3(wblocks, nseg), dim3(256), 0, s, G, in, seg_tiles);
}
// ... and the front end of the ring's witnesses
void launch_screen_front(hipStream_t s, const ScreenRing& G, const ScreenIn& in, uint32_t* scratch) {
    hipLaunchKernelGGL(k_screen_front, dim3((in.count + 63) / 64), dim3(64), 0, s, G, in, scratch);
}
// the point arithmetic of the whole chunk, after every ring's pass: a chunk of a few witnesses on cooperating waves, four per witness whatever its path
void launch_screen_ecdsa(hipStream_t s, const DevParams& P, const ScreenIn& in, uint32_t* scratch) {
    if (in.count <= ZK_SCREEN_CO_MAX && !zk_one_lane_chains()) {
        g_coop_chains.fetch_add((uint64_t)in.count * 4, std::memory_order_relaxed);
        hipLaunchKernelGGL(k_screen_table_co, dim3(in.count), dim3(256), 0, s, P, in, scratch);
        hipLaunchKernelGGL(k_screen_walk_co, dim3(in.count), dim3(256), 0, s, P, in, scratch);
        return;
    }
    hipLaunchKernelGGL(k_screen_table, dim3((in.count + 63) / 64), dim3(64), 0, s, P, in.count, scratch);
    hipLaunchKernelGGL(k_screen_walk, dim3((in.count + 63) / 64), dim3(64), 0, s, in, scratch);
}
