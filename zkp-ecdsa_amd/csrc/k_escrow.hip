// Escrow tags (include/zkattest.h: zk_escrow_*): the kernels around the shared machinery -- the commitments are k_tom.hip's, over the context's (g, h) combs
// and the auditor's (g, A) set, the challenge hash k_hash.hip's message path (launch_sha_msgs), the arithmetic escrow.h's and link.h's.  The prover's front
// end (validation, the four draws, the openings), the opening compare and the challenge's message behind the normaliser, the responses with the 472-byte
// writer; the verifier's parser, its three relation lanes per tag and the verdict; the auditor's ladder, the ring's points 4 y_i g and the match.
#include "escrow.h"

typedef Fe<ModQ, 1> Sq;
typedef Fe<ModT, 1> St;

ZK_DEV void esc_put_padding(uint8_t* m) {   // behind the 469 message bytes: 0x80, zeros, the bit length
    m[469] = 0x80;
#pragma unroll
    for (int i = 470; i < 510; i++) m[i] = 0;
    m[510] = (uint8_t)((469 * 8) >> 8), m[511] = (uint8_t)(469 * 8);
}
ZK_DEV void esc_put_slot(uint8_t* m, const TomList& L, uint32_t e) {   // a normalised slot of the list as a point of the message
    uint32_t w[18];
    words_from_limbs<9>(w, soa_ld<ModT, 1>(L.ax, e).l);
    words_from_limbs<9>(w + 9, soa_ld<ModT, 1>(L.ay, e).l);
    lk_put_point(m, w, w + 9);
}
// the list slot of a tag's point k (E1, E2, T1, T2, T3) in a prover chunk of `count` tags
ZK_DEV uint32_t esc_point_slot(uint32_t count, uint32_t p, uint32_t k) {
    return k == 0 ? 4 * p : k == 1 ? 4 * count + 2 * p : k == 2 ? 4 * p + 1 : k == 3 ? 4 * p + 2 : 4 * count + 2 * p + 1;
}

// ------------------------------------------------------------------ prover
// One thread per tag.  Draws under the randomness contract: 0 rho, 1 k_x, 2 k_r, 3 k_rho, all mod q.  Writes the status of the commitment's encoding, the RNG
// flag, the commitment's words and the six openings of the chunk's list.
__global__ void __launch_bounds__(64) k_escrow_front(EscrowLane K, uint32_t count, uint64_t first, EscrowProveIo io) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint64_t b = first + p;
    uint32_t cw[18];
    const bool ok = lk_load_point(io.com + 72 * b, cw);
#pragma unroll
    for (int i = 0; i < 18; i++) K.cw[18 * p + i] = cw[i];
    K.st[p] = ok ? ZK_OK : ZK_E_BAD_ENCODING;
    // fills the tag consumes: its four draws plus the rejected ones among them (k_link_front's rule)
    const uint32_t cnt = K.rng.exc_cnt[p];
    uint32_t rej = 0;
    for (uint32_t i = 0; i < (cnt < RNG_MAX_EXC ? cnt : RNG_MAX_EXC); i++) rej += (K.rng.exc_flags[p * RNG_MAX_EXC + i] >> 1) & 1;
    K.flags[p] = cnt > RNG_MAX_EXC || (K.rng.mode == 1 && 4 + rej > K.rng.stride_blocks);
    const Sq zero = fe_zero<ModQ>();
    const Sq rho = rng_draw<ModQ>(K.rng, p, 0), kx = rng_draw<ModQ>(K.rng, p, 1), kr = rng_draw<ModQ>(K.rng, p, 2), krho = rng_draw<ModQ>(K.rng, p, 3);
    const Sq x = lk_load_scalar(io.key + 32 * b), r = lk_load_scalar(io.blinder + 32 * b);
    soa_st(K.L.v, 4 * p, rho), soa_st(K.L.r, 4 * p, zero);
    soa_st(K.L.v, 4 * p + 1, kx), soa_st(K.L.r, 4 * p + 1, kr);
    soa_st(K.L.v, 4 * p + 2, krho), soa_st(K.L.r, 4 * p + 2, zero);
    soa_st(K.L.v, 4 * p + 3, x), soa_st(K.L.r, 4 * p + 3, r);
    const uint32_t e = 4 * count + 2 * p;
    soa_st(K.L.v, e, x), soa_st(K.L.r, e, rho);
    soa_st(K.L.v, e + 1, kx), soa_st(K.L.r, e + 1, krho);
}
void launch_escrow_front(hipStream_t s, const EscrowLane& K, uint32_t count, uint64_t first, const EscrowProveIo& io) {
    hipLaunchKernelGGL(k_escrow_front, dim3((count + 63) / 64), dim3(64), 0, s, K, count, first, io);
}
// Behind the normaliser, one thread per tag.  The opening x g + r h (canonical) against the commitment as the caller states it, word for word, then the RNG;
// and the padded message of hashPoints([C, E1, E2, A, T1, T2, T3]).
__global__ void __launch_bounds__(64) k_escrow_opening_msg(EscrowLane K, EscrowKey A, uint32_t count) {
    const uint32_t p = gtid();
    if (p >= count) return;
    uint32_t w[18];
    uint8_t* m = K.msg + (size_t)p * ZKT1_MSG_BLOCKS * 64;
    uint32_t diff = 0;
    words_from_limbs<9>(w, soa_ld<ModT, 1>(K.L.ax, 4 * p + 3).l);
    words_from_limbs<9>(w + 9, soa_ld<ModT, 1>(K.L.ay, 4 * p + 3).l);
#pragma unroll
    for (int i = 0; i < 18; i++) diff |= w[i] ^ K.cw[18 * p + i];
#pragma unroll
    for (int i = 0; i < 18; i++) w[i] = K.cw[18 * p + i];
    lk_put_point(m, w, w + 9);
    esc_put_slot(m + 67, K.L, esc_point_slot(count, p, 0));
    esc_put_slot(m + 67 * 2, K.L, esc_point_slot(count, p, 1));
    lk_put_point(m + 67 * 3, A.w, A.w + 9);
#pragma unroll 1
    for (int k = 2; k < 5; k++) esc_put_slot(m + 67 * (k + 2), K.L, esc_point_slot(count, p, k));
    esc_put_padding(m);
    if (K.st[p] == ZK_OK) K.st[p] = diff ? ZK_E_OPENING : (K.flags[p] & 1) ? ZK_E_RNG_EXHAUSTED : ZK_OK;
}
void launch_escrow_opening_msg(hipStream_t s, const EscrowLane& K, const EscrowKey& A, uint32_t count) {
    hipLaunchKernelGGL(k_escrow_opening_msg, dim3((count + 63) / 64), dim3(64), 0, s, K, A, count);
}
// One workgroup of 128 threads per tag, one 32-bit word of the slot each (118 of them): the header, the five points (lanes 1..10 make a coordinate each), the
// responses (lanes 11..13 one each).  A failed tag's slot is 118 zero words.  Every byte of the slot is written once.
__global__ void __launch_bounds__(128) k_escrow_respond(EscrowLane K, uint32_t count, uint64_t first, EscrowProveIo io) {
    __shared__ uint32_t sl[128];
    const uint32_t p = blockIdx.x, t = threadIdx.x;
    const int32_t st = K.st[p];
    if (st == ZK_OK) {
        if (t == 0) sl[0] = ZK_MAGIC_ZKT1, sl[1] = bswap32(ZKT1_SIZE), sl[2] = 0, sl[3] = 0;
        else if (t < 11) {
            const uint32_t e = esc_point_slot(count, p, (t - 1) >> 1);
            uint32_t w[9];
            words_from_limbs<9>(w, soa_ld<ModT, 1>((t - 1) & 1 ? K.L.ay : K.L.ax, e).l);
#pragma unroll
            for (int i = 0; i < 9; i++) sl[4 + 9 * (t - 1) + i] = bswap32(w[8 - i]);
        } else if (t < 14) {
            const uint32_t j = t - 11;   // 0: t_x = k_x - c x; 1: t_r = k_r - c r; 2: t_rho = k_rho - c rho
            const Sq k = j == 0 ? soa_ld<ModQ, 1>(K.L.v, 4 * p + 1) : j == 1 ? soa_ld<ModQ, 1>(K.L.r, 4 * p + 1) : soa_ld<ModQ, 1>(K.L.v, 4 * p + 2);
            const Sq v = j == 0 ? soa_ld<ModQ, 1>(K.L.v, 4 * p + 3) : j == 1 ? soa_ld<ModQ, 1>(K.L.r, 4 * p + 3) : soa_ld<ModQ, 1>(K.L.v, 4 * p);
            uint32_t w[8];
            words_from_limbs<8>(w, link_respond(k, K.chal + 4 * p, v).l);
#pragma unroll
            for (int i = 0; i < 8; i++) sl[94 + 8 * j + i] = bswap32(w[7 - i]);
        }
    }
    __syncthreads();
    if (t < ZKT1_WORDS) ((uint32_t*)(io.out + (first + p) * ZKT1_SIZE))[t] = st == ZK_OK ? sl[t] : 0;
    if (t == 0) io.status[first + p] = st;
}
void launch_escrow_respond(hipStream_t s, const EscrowLane& K, uint32_t count, uint64_t first, const EscrowProveIo& io) {
    hipLaunchKernelGGL(k_escrow_respond, dim3(count), dim3(128), 0, s, K, count, first, io);
}

// ------------------------------------------------------------------ verifier
// One thread per tag: the header, the six points' encoding (range and curve equation), the scalars reduced as the Scalar constructor reduces them, the comb
// parts' openings and the challenge's message.
__global__ void __launch_bounds__(64) k_escrow_parse(EscrowLane K, EscrowKey A, uint32_t count, uint64_t first, EscrowVerifyIo io) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint64_t b = first + p;
    const uint8_t* pr = io.tags + b * ZKT1_SIZE;
    const uint32_t* h = (const uint32_t*)pr;
    bool ok = h[0] == ZK_MAGIC_ZKT1 && h[1] == bswap32(ZKT1_SIZE) && h[2] == 0 && h[3] == 0;
    uint8_t* m = K.msg + (size_t)p * ZKT1_MSG_BLOCKS * 64;
    uint32_t w[18];
#pragma unroll 1
    for (int j = 0; j < 6; j++) {   // C, E1, E2, then T1, T2, T3 behind A
        const uint8_t* src = j == 0 ? io.com + 72 * b : pr + ZKT1_PT(j - 1);
        ok = lk_load_point(src, w) && ok;
        lk_put_point(m + 67 * (j < 3 ? j : j + 1), w, w + 9);
    }
    lk_put_point(m + 67 * 3, A.w, A.w + 9);
    esc_put_padding(m);
    K.st[p] = ok ? ZK_OK : ZK_E_BAD_ENCODING;
    const Sq tx = lk_load_scalar(pr + ZKT1_SC(0)), tr = lk_load_scalar(pr + ZKT1_SC(1)), trho = lk_load_scalar(pr + ZKT1_SC(2));
    soa_st(K.L.v, 2 * p, tx), soa_st(K.L.r, 2 * p, tr);
    soa_st(K.L.v, 2 * p + 1, trho), soa_st(K.L.r, 2 * p + 1, fe_zero<ModQ>());
    soa_st(K.L.v, 2 * count + p, tx), soa_st(K.L.r, 2 * count + p, trho);
}
void launch_escrow_parse(hipStream_t s, const EscrowLane& K, const EscrowKey& A, uint32_t count, uint64_t first, const EscrowVerifyIo& io) {
    hipLaunchKernelGGL(k_escrow_parse, dim3((count + 63) / 64), dim3(64), 0, s, K, A, count, first, io);
}
// One lane per (tag, relation), lane 3 p + j (link.h: link_relation, its comb part from the list):
//   0: (t_x g + t_r h) + c C - T1 = O      1: (t_rho g) + c E1 - T2 = O      2: (t_x g + t_rho A) + c E2 - T3 = O
__global__ void __launch_bounds__(64) k_escrow_relations(EscrowLane K, uint32_t count, uint64_t first, EscrowVerifyIo io) {
    const uint32_t t = gtid();
    if (t >= 3 * count) return;
    const uint32_t p = t / 3, j = t - 3 * p;
    const uint64_t b = first + p;
    bool rel = false;
    if (K.st[p] == ZK_OK) {
        const uint8_t* pr = io.tags + b * ZKT1_SIZE;
        uint32_t w[18];
        (void)lk_load_point(j == 0 ? io.com + 72 * b : pr + ZKT1_PT(j - 1), w);
        const TomPt base = lk_point_from_words(w);
        (void)lk_load_point(pr + ZKT1_PT(2 + j), w);
        const TomPt T = lk_point_from_words(w);
        const uint32_t e = j == 2 ? 2 * count + p : 2 * p + j;
        const TomPt D = link_from_triple(soa_ld<ModT, 2>(K.L.proj.x, e), soa_ld<ModT, 2>(K.L.proj.y, e), soa_ld<ModT, 2>(K.L.proj.z, e));
        rel = link_relation(base, K.chal + 4 * p, D, T);
    }
    K.rel[t] = rel ? 1 : 0;
}
void launch_escrow_relations(hipStream_t s, const EscrowLane& K, uint32_t count, uint64_t first, const EscrowVerifyIo& io) {
    hipLaunchKernelGGL(k_escrow_relations, dim3((3 * count + 63) / 64), dim3(64), 0, s, K, count, first, io);
}
__global__ void __launch_bounds__(256) k_escrow_verdict(EscrowLane K, uint32_t count, uint64_t first, EscrowVerifyIo io) {   // the AND of a tag's three relations
    const uint32_t p = gtid();
    if (p >= count) return;
    io.ok[first + p] = (K.rel[3 * p] & K.rel[3 * p + 1] & K.rel[3 * p + 2] & 1) ? 1 : 0;
    io.status[first + p] = K.st[p];
}
void launch_escrow_verdict(hipStream_t s, const EscrowLane& K, uint32_t count, uint64_t first, const EscrowVerifyIo& io) {
    hipLaunchKernelGGL(k_escrow_verdict, dim3((count + 255) / 256), dim3(256), 0, s, K, count, first, io);
}

// ------------------------------------------------------------------ the auditor's key
// One thread: the key's encoding (res[0]: both coordinates below the field prime and on the curve), whether it is the identity (res[1]), and its eighteen
// little-endian words as the table builder and the order check take them
__global__ void k_escrow_check_key(const uint8_t* xy72, uint32_t* words18, int32_t* res) {
    if (gtid() != 0) return;
    uint32_t w[18];
    const bool ok = lk_load_point(xy72, w);
    uint32_t rest = w[9] ^ 1u;
#pragma unroll
    for (int i = 0; i < 18; i++) {
        words18[i] = w[i];
        if (i != 9) rest |= w[i];
    }
    res[0] = ok ? 1 : 0, res[1] = rest == 0 ? 1 : 0;
}
void launch_escrow_check_key(hipStream_t s, const uint8_t* d_xy72, uint32_t* d_words18, int32_t* d_res) {
    hipLaunchKernelGGL(k_escrow_check_key, dim3(1), dim3(64), 0, s, d_xy72, d_words18, d_res);
}

// ------------------------------------------------------------------ opening
// One thread: the secret reduced mod q as the opening (a, 0) of list slot `slot` and, where asked for, as the eight words the ladder reads
__global__ void k_escrow_stage_secret(const uint8_t* secret, TomList L, uint32_t slot, uint32_t* a8) {
    if (gtid() != 0) return;
    const Sq a = lk_load_scalar(secret);
    soa_st(L.v, slot, a), soa_st(L.r, slot, fe_zero<ModQ>());
    if (a8) {
        uint32_t w[8];
        words_from_limbs<8>(w, a.l);
#pragma unroll
        for (int i = 0; i < 8; i++) a8[i] = w[i];
    }
}
void launch_escrow_stage_secret(hipStream_t s, const uint8_t* d_secret, const TomList& L, uint32_t slot, uint32_t* a8) {
    hipLaunchKernelGGL(k_escrow_stage_secret, dim3(1), dim3(64), 0, s, d_secret, L, slot, a8);
}
// One lane per tag: the header, E1 and E2 (anything else in the slot is the verifier's business), a E1 through the masked ladder, 4 (E2 - a E1) as a
// projective triple of the tags' list.  A refused tag leaves the identity there, status 10, and the match skips it; every index starts as "none".
__global__ void __launch_bounds__(64) k_escrow_open_points(EscrowOpen O, uint32_t count, uint64_t first, const uint8_t* tags, uint32_t* index, int32_t* status) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint64_t b = first + p;
    const uint8_t* pr = tags + b * ZKT1_SIZE;
    const uint32_t* h = (const uint32_t*)pr;
    bool ok = h[0] == ZK_MAGIC_ZKT1 && h[1] == bswap32(ZKT1_SIZE) && h[2] == 0 && h[3] == 0;
    uint32_t w[18];
    ok = lk_load_point(pr + ZKT1_PT(0), w) && ok;
    TomPt e1 = lk_point_from_words(w);
    ok = lk_load_point(pr + ZKT1_PT(1), w) && ok;
    TomPt e2 = lk_point_from_words(w);
    if (!ok) e1 = tom_identity(), e2 = tom_identity();   // (the ladder runs all the same: the lanes of a wave stay together)
    const TomPt m = escrow_open_point(e1, e2, O.a8);
    soa_st(O.T.proj.x, (uint32_t)b, m.x), soa_st(O.T.proj.y, (uint32_t)b, m.y), soa_st(O.T.proj.z, (uint32_t)b, m.z);
    O.st[b] = ok ? ZK_OK : ZK_E_BAD_ENCODING;
    status[b] = ok ? ZK_OK : ZK_E_BAD_ENCODING;
    index[b] = 0xffffffffu;
}
void launch_escrow_open_points(hipStream_t s, const EscrowOpen& O, uint32_t count, uint64_t first, const uint8_t* tags, uint32_t* index, int32_t* status) {
    hipLaunchKernelGGL(k_escrow_open_points, dim3((count + 63) / 64), dim3(64), 0, s, O, count, first, tags, index, status);
}
// The ring's keys i0 .. i0 + n - 1 as the openings (y_i, 0) of slots 0 .. n - 1
__global__ void __launch_bounds__(256) k_escrow_ring_scalars(Soa ring, uint64_t i0, uint32_t n, TomList L) {
    const uint32_t i = gtid();
    if (i >= n) return;
    soa_st(L.v, i, soa_ld<ModQ, 1>(ring, (uint32_t)(i0 + i))), soa_st(L.r, i, fe_zero<ModQ>());
}
void launch_escrow_ring_scalars(hipStream_t s, const Soa& ring, uint64_t i0, uint32_t n, const TomList& L) {
    hipLaunchKernelGGL(k_escrow_ring_scalars, dim3((n + 255) / 256), dim3(256), 0, s, ring, i0, n, L);
}
__global__ void __launch_bounds__(64) k_escrow_times4(TomList L, uint32_t n) {
    const uint32_t i = gtid();
    if (i >= n) return;
    const TomPt m = tom_dbl(tom_dbl(link_from_triple(soa_ld<ModT, 2>(L.proj.x, i), soa_ld<ModT, 2>(L.proj.y, i), soa_ld<ModT, 2>(L.proj.z, i))));
    soa_st(L.proj.x, i, m.x), soa_st(L.proj.y, i, m.y), soa_st(L.proj.z, i, m.z);
}
void launch_escrow_times4(hipStream_t s, const TomList& L, uint32_t n) { hipLaunchKernelGGL(k_escrow_times4, dim3((n + 63) / 64), dim3(64), 0, s, L, n); }
// One lane per tag over a slab of the ring's points (keys i0 .. i0 + n - 1, all real keys: the caller stops at the ring's key count).  The slabs come in
// ascending order and a lane stops at its first match, so the index is the lowest.  A key's low limb of x screens before the other seventeen are compared;
// every lane of a wave reads the same key, so the slab streams through the scalar cache.  The points are public.
__global__ void __launch_bounds__(256) k_escrow_match(EscrowOpen O, uint64_t B, uint64_t i0, uint32_t n, uint32_t* index) {
    const uint64_t b = gtid();
    if (b >= B) return;
    if (O.st[b] != ZK_OK || index[b] != 0xffffffffu) return;
    const St x = soa_ld<ModT, 1>(O.T.ax, (uint32_t)b), y = soa_ld<ModT, 1>(O.T.ay, (uint32_t)b);
    const uint32_t* rx = O.Rg.ax.p;
#pragma unroll 1
    for (uint32_t i = 0; i < n; i++) {
        if (rx[i] != x.l[0]) continue;
        const St kx = soa_ld<ModT, 1>(O.Rg.ax, i), ky = soa_ld<ModT, 1>(O.Rg.ay, i);
        uint32_t diff = 0;
#pragma unroll
        for (int l = 0; l < NLIMB; l++) diff |= (kx.l[l] ^ x.l[l]) | (ky.l[l] ^ y.l[l]);
        if (!diff) {
            index[b] = (uint32_t)(i0 + i);
            return;
        }
    }
}
void launch_escrow_match(hipStream_t s, const EscrowOpen& O, uint64_t B, uint64_t i0, uint32_t n, uint32_t* index) {
    hipLaunchKernelGGL(k_escrow_match, dim3((uint32_t)((B + 255) / 256)), dim3(256), 0, s, O, B, i0, n, index);
}
