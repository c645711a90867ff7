// Distinct-key proofs (include/zkattest.h: zk_distinct_*): one MultProof (mult.ts:93-175) over Cx = C1 - C2, Cy = C_w = commit(1 / (x1 - x2)), Cz = g.  The
// kernels around the shared machinery -- every commitment is a fixed-base one through k_tom.hip's comb kernels, Cx goes through its normaliser, the challenge
// hash is k_hash.hip's message path (launch_sha_msgs), the arithmetic is distinct.h's and link.h's: the prover's front end (validation, d and its inverse, the
// eight draws, the openings, Cx), the opening compare and the challenge's message behind the normaliser, the responses with the 744-byte writer; the verifier's
// parser, Cx into the message, c into relation 3's opening, the three short ladders (relations 1, 2, 4) and, in a kernel of its own, relation 5's 256-bit chain.
#include "distinct.h"

typedef Fe<ModQ, 1> Sq;

ZK_DEV void dist_put_padding(uint8_t* m) {   // behind the 603 message bytes: 0x80, zeros, the bit length
    m[603] = 0x80;
#pragma unroll
    for (int i = 604; i < 638; i++) m[i] = 0;
    m[638] = (uint8_t)((603 * 8) >> 8), m[639] = (uint8_t)(603 * 8);
}
ZK_DEV void dist_put_slot(uint8_t* m, const TomList& L, uint32_t slot) {   // a normalised slot of the list as a point of the message
    uint32_t w[18];
    words_from_limbs<9>(w, soa_ld<ModT, 1>(L.ax, slot).l);
    words_from_limbs<9>(w + 9, soa_ld<ModT, 1>(L.ay, slot).l);
    lk_put_point(m, w, w + 9);
}
ZK_DEV void dist_put_g(uint8_t* m, const DevParams& P) {
    uint32_t w[18];
    words_from_limbs<9>(w, P.tom_g_aff);
    words_from_limbs<9>(w + 9, P.tom_g_aff + 9);
    lk_put_point(m, w, w + 9);
}
ZK_DEV void dist_store_proj(const TomList& L, uint32_t slot, const TomPt& p) { soa_st(L.proj.x, slot, p.x), soa_st(L.proj.y, slot, p.y), soa_st(L.proj.z, slot, p.z); }
// Cx = C1 - C2 from the commitments' words where both are points of the curve, else the identity: the slot goes through a normaliser that shares one
// inversion among a workgroup's points, and a failed proof touches no neighbour
ZK_DEV TomPt dist_cx(bool ok, const uint32_t cw[36]) {
    TomPt cx = tom_identity();
    if (ok) cx = dist_sub(lk_point_from_words(cw), lk_point_from_words(cw + 18));
    return cx;
}
ZK_DEV Sq dist_one() {
    Sq one = fe_zero<ModQ>();
    one.l[0] = 1;
    return one;
}

// ------------------------------------------------------------------ prover
// One thread per proof.  Draws (pedersen.ts:53-58, mult.ts:105-113 under the randomness contract), all mod q: 0 r_w, 1..3 k_x, k_y, k_z, 4..7 the blinders of
// A_x, A_y, A_z, A_4_1.  Writes the status of the commitments' encoding and of d = x1 - x2, the RNG flag, the commitments' words, Cx and the nine openings.
__global__ void __launch_bounds__(64) k_dist_front(DistLane K, uint32_t count, uint64_t first, DistProveIo io) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint64_t b = first + p;
    uint32_t cw[36];
    const bool ok1 = lk_load_point(io.com1 + 72 * b, cw), ok2 = lk_load_point(io.com2 + 72 * b, cw + 18);
#pragma unroll
    for (int i = 0; i < 36; i++) K.cw[36 * p + i] = cw[i];
    dist_store_proj(K.L, DIST_SLOTS * count - count + p, dist_cx(ok1 && ok2, cw));
    // fills the proof consumes: its eight draws plus the rejected ones among them (k_m_front's rule)
    const uint32_t cnt = K.rng.exc_cnt[p];
    uint32_t rej = 0;
    for (uint32_t i = 0; i < (cnt < RNG_MAX_EXC ? cnt : RNG_MAX_EXC); i++) rej += (K.rng.exc_flags[p * RNG_MAX_EXC + i] >> 1) & 1;
    K.flags[p] = cnt > RNG_MAX_EXC || (K.rng.mode == 1 && 8 + rej > K.rng.stride_blocks);
    const Sq x1 = lk_load_scalar(io.key1 + 32 * b), x2 = lk_load_scalar(io.key2 + 32 * b);
    const Sq d = fe_sub_mod(x1, x2);
    K.st[p] = !(ok1 && ok2) ? ZK_E_BAD_ENCODING : fe_is_zero(d) ? ZK_E_ARG : ZK_OK;   // x1 = x2 mod q: the statement is false
    const Sq w = dist_inverse(d), rw = rng_draw<ModQ>(K.rng, p, 0), kx = rng_draw<ModQ>(K.rng, p, 1), kz = rng_draw<ModQ>(K.rng, p, 3);
    soa_st(K.L.v, 2 * p, kz), soa_st(K.L.r, 2 * p, rng_draw<ModQ>(K.rng, p, 6));       // A_z
    soa_st(K.L.v, 2 * p + 1, kz), soa_st(K.L.r, 2 * p + 1, rng_draw<ModQ>(K.rng, p, 7));   // A_4_1
    const uint32_t e = 2 * count + DIST_SINGLES * p;
    soa_st(K.L.v, e, w), soa_st(K.L.r, e, rw);                                          // C_w
    soa_st(K.L.v, e + 1, dist_one()), soa_st(K.L.r, e + 1, fe_mul_mod(d, rw));          // C_4 = d C_w = g + d r_w h
    soa_st(K.L.v, e + 2, kx), soa_st(K.L.r, e + 2, rng_draw<ModQ>(K.rng, p, 4));        // A_x
    soa_st(K.L.v, e + 3, rng_draw<ModQ>(K.rng, p, 2)), soa_st(K.L.r, e + 3, rng_draw<ModQ>(K.rng, p, 5));   // A_y
    soa_st(K.L.v, e + 4, fe_mul_mod(kx, w)), soa_st(K.L.r, e + 4, fe_mul_mod(kx, rw));  // A_4_2 = k_x C_w
    soa_st(K.L.v, e + 5, x1), soa_st(K.L.r, e + 5, lk_load_scalar(io.blinder1 + 32 * b));
    soa_st(K.L.v, e + 6, x2), soa_st(K.L.r, e + 6, lk_load_scalar(io.blinder2 + 32 * b));
}
void launch_dist_front(hipStream_t s, const DistLane& K, uint32_t count, uint64_t first, const DistProveIo& io) {
    hipLaunchKernelGGL(k_dist_front, dim3((count + 63) / 64), dim3(64), 0, s, K, count, first, io);
}
// the list slot of point k of a proof's seven: C_w, C_4, A_x, A_y, A_z, A_4_1, A_4_2
ZK_DEV uint32_t dist_point_slot(uint32_t count, uint32_t p, uint32_t k) {
    const uint32_t e = 2 * count + DIST_SINGLES * p;
    return k < 4 ? e + k : k == 6 ? e + 4 : 2 * p + (k - 4);
}
// Behind the normaliser, one thread per proof.  The openings x1 g + r1 h, x2 g + r2 h (canonical) against the commitments as the caller states them, word for
// word (k_rr_compare's rule), then the RNG; and the padded message of hashPoints([Cx, C_w, g, C_4, A_x, A_y, A_z, A_4_1, A_4_2]).
__global__ void __launch_bounds__(64) k_dist_opening_msg(DevParams P, DistLane K, uint32_t count) {
    const uint32_t p = gtid();
    if (p >= count) return;
    uint8_t* m = K.msg + (size_t)p * ZKD1_MSG_BLOCKS * 64;
    uint32_t diff = 0;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const uint32_t e = 2 * count + DIST_SINGLES * p + 5 + j;
        uint32_t w[18];
        words_from_limbs<9>(w, soa_ld<ModT, 1>(K.L.ax, e).l);
        words_from_limbs<9>(w + 9, soa_ld<ModT, 1>(K.L.ay, e).l);
#pragma unroll
        for (int i = 0; i < 18; i++) diff |= w[i] ^ K.cw[36 * p + 18 * j + i];
    }
    dist_put_slot(m, K.L, DIST_SLOTS * count - count + p);
    dist_put_slot(m + 67, K.L, dist_point_slot(count, p, 0));
    dist_put_g(m + 134, P);
#pragma unroll 1
    for (uint32_t k = 1; k < 7; k++) dist_put_slot(m + 67 * (2 + k), K.L, dist_point_slot(count, p, k));
    dist_put_padding(m);
    if (K.st[p] == ZK_OK) K.st[p] = diff ? ZK_E_OPENING : (K.flags[p] & 1) ? ZK_E_RNG_EXHAUSTED : ZK_OK;
}
void launch_dist_opening_msg(hipStream_t s, const DevParams& P, const DistLane& K, uint32_t count) {
    hipLaunchKernelGGL(k_dist_opening_msg, dim3((count + 63) / 64), dim3(64), 0, s, P, K, count);
}
// One workgroup of 64 threads per proof builds the slot's 186 words in LDS: lanes 0..13 a coordinate of the seven points each, lane 14 the seven responses
// (distinct.h: mult_responses with x = d, y = w, z = 1 under the blinders r1 - r2, r_w, 0), lane 15 the header.  Then every lane writes three words (two for the
// last lanes).  A failed proof's slot is 186 zero words.  Every byte of the slot is written once.
__global__ void __launch_bounds__(64) k_dist_respond(DistLane K, uint32_t count, uint64_t first, DistProveIo io) {
    __shared__ uint32_t sl[ZKD1_WORDS];
    const uint32_t p = blockIdx.x, t = threadIdx.x;
    const int32_t st = K.st[p];
    if (st == ZK_OK) {
        if (t < 14) {
            uint32_t w[9];
            words_from_limbs<9>(w, soa_ld<ModT, 1>(t & 1 ? K.L.ay : K.L.ax, dist_point_slot(count, p, t >> 1)).l);
#pragma unroll
            for (int i = 0; i < 9; i++) sl[4 + 9 * t + i] = bswap32(w[8 - i]);
        } else if (t == 14) {
            const uint32_t e = 2 * count + DIST_SINGLES * p;
            auto v = [&](uint32_t slot) { return soa_ld<ModQ, 1>(K.L.v, slot); };
            auto r = [&](uint32_t slot) { return soa_ld<ModQ, 1>(K.L.r, slot); };
            const Sq k[7] = {v(e + 2), v(e + 3), v(2 * p), r(e + 2), r(e + 3), r(2 * p), r(2 * p + 1)};
            Sq resp[7];
            mult_responses(resp, K.chal + 4 * p, k, fe_sub_mod(v(e + 5), v(e + 6)), v(e), dist_one(), fe_sub_mod(r(e + 5), r(e + 6)), r(e), fe_zero<ModQ>());
#pragma unroll
            for (int j = 0; j < 7; j++) {
                uint32_t w[8];
                words_from_limbs<8>(w, resp[j].l);
#pragma unroll
                for (int i = 0; i < 8; i++) sl[130 + 8 * j + i] = bswap32(w[7 - i]);
            }
        } else if (t == 15) sl[0] = ZK_MAGIC_ZKD1, sl[1] = bswap32(ZKD1_SIZE), sl[2] = 0, sl[3] = 0;
    }
    __syncthreads();
    uint32_t* o = (uint32_t*)(io.out + (first + p) * ZKD1_SIZE);
    for (uint32_t i = t; i < ZKD1_WORDS; i += 64) o[i] = st == ZK_OK ? sl[i] : 0;
    if (t == 0) io.status[first + p] = st;
}
void launch_dist_respond(hipStream_t s, const DistLane& K, uint32_t count, uint64_t first, const DistProveIo& io) {
    hipLaunchKernelGGL(k_dist_respond, dim3(count), dim3(64), 0, s, K, count, first, io);
}

// ------------------------------------------------------------------ verifier
// One thread per proof: the header, the nine points' encoding (edwards.ts:204-209: range and curve equation), the scalars reduced as the Scalar constructor
// reduces them (what zk_verify_batch does with a MultProof's scalars inside ZKA1), the comb parts' openings, t_x as words for relation 5's chain, Cx as the
// normaliser takes it, and the challenge's message but for Cx.
__global__ void __launch_bounds__(64) k_dist_parse(DevParams P, DistLane K, uint32_t count, uint64_t first, DistVerifyIo io) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint64_t b = first + p;
    const uint8_t* pr = io.proofs + b * ZKD1_SIZE;
    const uint32_t* h = (const uint32_t*)pr;
    bool ok = h[0] == ZK_MAGIC_ZKD1 && h[1] == bswap32(ZKD1_SIZE) && h[2] == 0 && h[3] == 0;
    uint8_t* m = K.msg + (size_t)p * ZKD1_MSG_BLOCKS * 64;
    {
        uint32_t cw[36];
        const bool ok1 = lk_load_point(io.com1 + 72 * b, cw), ok2 = lk_load_point(io.com2 + 72 * b, cw + 18);
        dist_store_proj(K.L, 4 * count + p, dist_cx(ok1 && ok2, cw));
        ok = ok && ok1 && ok2;
    }
    uint32_t w[18];
#pragma unroll 1
    for (int j = 0; j < 7; j++) {   // C_w, then the MultProof's six: places 1, 3..8 of the message
        ok = lk_load_point(pr + ZKD1_CW + 72 * j, w) && ok;
        lk_put_point(m + 67 * (j ? j + 2 : 1), w, w + 9);
    }
    dist_put_g(m + 134, P);
    dist_put_padding(m);
    K.st[p] = ok ? ZK_OK : ZK_E_BAD_ENCODING;
    const Sq tx = lk_load_scalar(pr + ZKD1_SC(0)), tz = lk_load_scalar(pr + ZKD1_SC(2));
    uint32_t t8[8];
    words_from_limbs<8>(t8, tx.l);
#pragma unroll
    for (int i = 0; i < 8; i++) K.tw[8 * p + i] = t8[i];
    soa_st(K.L.v, 4 * p, tx), soa_st(K.L.r, 4 * p, lk_load_scalar(pr + ZKD1_SC(3)));
    soa_st(K.L.v, 4 * p + 1, lk_load_scalar(pr + ZKD1_SC(1))), soa_st(K.L.r, 4 * p + 1, lk_load_scalar(pr + ZKD1_SC(4)));
    soa_st(K.L.v, 4 * p + 2, tz), soa_st(K.L.r, 4 * p + 2, lk_load_scalar(pr + ZKD1_SC(5)));
    soa_st(K.L.v, 4 * p + 3, tz), soa_st(K.L.r, 4 * p + 3, lk_load_scalar(pr + ZKD1_SC(6)));
}
void launch_dist_parse(hipStream_t s, const DevParams& P, const DistLane& K, uint32_t count, uint64_t first, const DistVerifyIo& io) {
    hipLaunchKernelGGL(k_dist_parse, dim3((count + 63) / 64), dim3(64), 0, s, P, K, count, first, io);
}
__global__ void __launch_bounds__(64) k_dist_cx_msg(DistLane K, uint32_t count) {
    const uint32_t p = gtid();
    if (p >= count) return;
    dist_put_slot(K.msg + (size_t)p * ZKD1_MSG_BLOCKS * 64, K.L, 4 * count + p);
}
void launch_dist_cx_msg(hipStream_t s, const DistLane& K, uint32_t count) { hipLaunchKernelGGL(k_dist_cx_msg, dim3((count + 63) / 64), dim3(64), 0, s, K, count); }
// Relation 3's base is g, so its c Cz joins the comb part: (t_z + c) g + t_rz h, one modular addition instead of a fourth ladder
__global__ void __launch_bounds__(64) k_dist_fold(DistLane K, uint32_t count) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint32_t* c3 = K.chal + 4 * p;
    const uint32_t w[8] = {c3[0], c3[1], c3[2] & 0xffffu, 0, 0, 0, 0, 0};
    Sq c;
    limbs_from_words<8>(c.l, w);
    soa_st(K.L.v, 4 * p + 2, fe_add_mod(soa_ld<ModQ, 1>(K.L.v, 4 * p + 2), c));
}
void launch_dist_fold(hipStream_t s, const DistLane& K, uint32_t count) { hipLaunchKernelGGL(k_dist_fold, dim3((count + 63) / 64), dim3(64), 0, s, K, count); }
ZK_DEV TomPt dist_proof_point(const uint8_t* src) {
    uint32_t w[18];
    (void)lk_load_point(src, w);
    return lk_point_from_words(w);
}
ZK_DEV TomPt dist_comb_part(const TomList& L, uint32_t slot) { return link_from_triple(soa_ld<ModT, 2>(L.proj.x, slot), soa_ld<ModT, 2>(L.proj.y, slot), soa_ld<ModT, 2>(L.proj.z, slot)); }
// One lane per (proof, short relation): lane 3 p + j checks relation 1, 2 or 4 of aggregateMult (mult.ts:152-165) -- t g + t_r h + c C - A = O over
// (Cx, A_x), (C_w, A_y), (C_4, A_4_1) with the comb part from list slot 4 p + 0, 1, 3 (link.h: link_relation) -- and leaves its verdict for k_dist_long.
// Cx is the normalised slot 4 count + p; it may be the identity.
__global__ void __launch_bounds__(64) k_dist_short(DistLane K, uint32_t count, uint64_t first, DistVerifyIo io) {
    const uint32_t t = gtid();
    if (t >= 3 * count) return;
    const uint32_t p = t / 3, j = t % 3;
    const uint8_t* pr = io.proofs + (first + p) * ZKD1_SIZE;
    bool rel = false;
    if (K.st[p] == ZK_OK) {
        TomPt C;
        if (j == 0) {
            uint32_t w[18];
            words_from_limbs<9>(w, soa_ld<ModT, 1>(K.L.ax, 4 * count + p).l);
            words_from_limbs<9>(w + 9, soa_ld<ModT, 1>(K.L.ay, 4 * count + p).l);
            C = lk_point_from_words(w);
        } else C = dist_proof_point(pr + (j == 1 ? ZKD1_CW : ZKD1_PT(0)));
        const TomPt A = dist_proof_point(pr + ZKD1_PT(j == 2 ? 4 : 1 + j));
        rel = link_relation(C, K.chal + 4 * p, dist_comb_part(K.L, 4 * p + (j == 2 ? 3 : j)), A);
    }
    K.rel[t] = rel;
}
void launch_dist_short(hipStream_t s, const DistLane& K, uint32_t count, uint64_t first, const DistVerifyIo& io) {
    hipLaunchKernelGGL(k_dist_short, dim3((3 * count + 63) / 64), dim3(64), 0, s, K, count, first, io);
}
// One lane per proof, behind k_dist_short on the same stream: relation 5, t_x C_w + c C_4 - A_4_2 = O (distinct.h: dist_ladder2, about three short ladders
// long, hence waves of its own), relation 3 from its comb part alone, and the verdict: the AND of the five.
__global__ void __launch_bounds__(64) k_dist_long(DistLane K, uint32_t count, uint64_t first, DistVerifyIo io) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint64_t b = first + p;
    const uint8_t* pr = io.proofs + b * ZKD1_SIZE;
    const int32_t st = K.st[p];
    bool ok = false;
    if (st == ZK_OK) {
        ok = K.rel[3 * p] && K.rel[3 * p + 1] && K.rel[3 * p + 2];
        ok = dist_relation3(dist_comb_part(K.L, 4 * p + 2), dist_proof_point(pr + ZKD1_PT(3))) && ok;
        ok = dist_relation5(dist_proof_point(pr + ZKD1_CW), K.tw + 8 * p, dist_proof_point(pr + ZKD1_PT(0)), K.chal + 4 * p, dist_proof_point(pr + ZKD1_PT(5)),
                            K.tab + (size_t)DIST_TAB_QUADS * p) && ok;
    }
    io.ok[b] = ok ? 1 : 0, io.status[b] = st;
}
void launch_dist_long(hipStream_t s, const DistLane& K, uint32_t count, uint64_t first, const DistVerifyIo& io) {
    hipLaunchKernelGGL(k_dist_long, dim3((count + 63) / 64), dim3(64), 0, s, K, count, first, io);
}
