// Threshold opening of escrow tags (include/zkattest.h: zk_auditors_*): the kernels around the shared machinery -- U1 = k g and s g are k_tom.hip's over the
// context's (g, h) combs, the challenge hash k_hash.hip's message path, the masked ladder escrow.h's, the two-base public ladder distinct.h's, the arithmetic
// escrow_share.h's.  An auditor's front end, its two masked ladders per tag and the 264-byte writer; the share verifier's parser, its two relation lanes per
// share and the verdict; the Lagrange coefficients, the combine's joint ladder, and the dealer's split.
#include "escrow_share.h"

typedef Fe<ModQ, 1> Sq;

ZK_DEV bool shr_tag_header(const uint8_t* tag) {
    const uint32_t* h = (const uint32_t*)tag;
    return h[0] == ZK_MAGIC_ZKT1 && h[1] == bswap32(ZKT1_SIZE) && h[2] == 0 && h[3] == 0;
}
ZK_DEV void shr_put_padding(uint8_t* m) {   // behind the 335 message bytes: 0x80, zeros, the bit length
    m[335] = 0x80;
#pragma unroll
    for (int i = 336; i < 382; i++) m[i] = 0;
    m[382] = (uint8_t)((335 * 8) >> 8), m[383] = (uint8_t)(335 * 8);
}
ZK_DEV void shr_put_slot(uint8_t* m, const TomList& L, uint32_t e) {   // a normalised slot of the list as a point of the message
    uint32_t w[18];
    words_from_limbs<9>(w, soa_ld<ModT, 1>(L.ax, e).l);
    words_from_limbs<9>(w + 9, soa_ld<ModT, 1>(L.ay, e).l);
    lk_put_point(m, w, w + 9);
}
ZK_DEV void shr_put_triple(const Soa3& P, uint32_t e, const TomPt& m) { soa_st(P.x, e, m.x), soa_st(P.y, e, m.y), soa_st(P.z, e, m.z); }
// the list slot of a share's point k (D, U1, U2) in a chunk of `count` tags
ZK_DEV uint32_t shr_point_slot(uint32_t count, uint32_t p, uint32_t k) { return k == 0 ? count + p : k == 1 ? p : 2 * count + p; }

// ------------------------------------------------------------------ an auditor's share
// One thread per tag.  The tag's header and E1; the draw under the randomness contract: fill 0 is k, mod q; its opening (k, 0) and its words.
__global__ void __launch_bounds__(64) k_share_front(ShareLane K, uint32_t count, uint64_t first, ShareProveIo io) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint8_t* tag = io.tags + (first + p) * ZKT1_SIZE;
    uint32_t w[18];
    const bool ok = lk_load_point(tag + ZKT1_PT(0), w) && shr_tag_header(tag);
    K.st[p] = ok ? ZK_OK : ZK_E_BAD_ENCODING;
    const uint32_t cnt = K.rng.exc_cnt[p];   // fills the share consumes: its draw plus the rejected ones before it (k_link_front's rule)
    uint32_t rej = 0;
    for (uint32_t i = 0; i < (cnt < RNG_MAX_EXC ? cnt : RNG_MAX_EXC); i++) rej += (K.rng.exc_flags[p * RNG_MAX_EXC + i] >> 1) & 1;
    K.flags[p] = cnt > RNG_MAX_EXC || (K.rng.mode == 1 && 1 + rej > K.rng.stride_blocks);
    const Sq k = rng_draw<ModQ>(K.rng, p, 0);
    soa_st(K.L.v, p, k), soa_st(K.L.r, p, fe_zero<ModQ>());
    uint32_t k8[8];
    words_from_limbs<8>(k8, k.l);
#pragma unroll
    for (int i = 0; i < 8; i++) K.kw[8 * p + i] = k8[i];
}
void launch_share_front(hipStream_t s, const ShareLane& K, uint32_t count, uint64_t first, const ShareProveIo& io) {
    hipLaunchKernelGGL(k_share_front, dim3((count + 63) / 64), dim3(64), 0, s, K, count, first, io);
}
// One lane per (ladder, tag): lanes 0 .. count - 1 walk D = a_j E1, lanes count .. 2 count - 1 walk U2 = k E1, both through escrow_ladder -- no branch and no
// address depends on a bit of a_j or k (a lane's scalar lies where its index says).  A refused tag walks the identity.
__global__ void __launch_bounds__(64) k_share_ladder(ShareLane K, ShareSecret A, uint32_t count, uint64_t first, ShareProveIo io) {
    const uint32_t t = gtid();
    if (t >= 2 * count) return;
    const uint32_t which = t >= count ? 1 : 0, p = t - which * count;
    uint32_t w[18];
    (void)lk_load_point(io.tags + (first + p) * ZKT1_SIZE + ZKT1_PT(0), w);
    TomPt e1 = lk_point_from_words(w);
    if (K.st[p] != ZK_OK) e1 = tom_identity();
    shr_put_triple(K.L.proj, (1 + which) * count + p, escrow_ladder(e1, which ? K.kw + 8 * p : A.a8));
}
void launch_share_ladder(hipStream_t s, const ShareLane& K, const ShareSecret& A, uint32_t count, uint64_t first, const ShareProveIo& io) {
    hipLaunchKernelGGL(k_share_ladder, dim3((2 * count + 63) / 64), dim3(64), 0, s, K, A, count, first, io);
}
// Behind the normaliser, one thread per tag: the padded message of hashPoints([A_j, E1, D, U1, U2]), then the RNG's verdict
__global__ void __launch_bounds__(64) k_share_msg(ShareLane K, const uint32_t* keys_w, uint32_t j, uint32_t count, uint64_t first, ShareProveIo io) {
    const uint32_t p = gtid();
    if (p >= count) return;
    uint8_t* m = K.msg + (size_t)p * ZKS1_MSG_BLOCKS * 64;
    uint32_t w[18];
#pragma unroll
    for (int i = 0; i < 18; i++) w[i] = keys_w[18 * (j - 1) + i];
    lk_put_point(m, w, w + 9);
    (void)lk_load_point(io.tags + (first + p) * ZKT1_SIZE + ZKT1_PT(0), w);
    lk_put_point(m + 67, w, w + 9);
#pragma unroll 1
    for (uint32_t k = 0; k < 3; k++) shr_put_slot(m + 67 * (2 + k), K.L, shr_point_slot(count, p, k));
    shr_put_padding(m);
    if (K.st[p] == ZK_OK && (K.flags[p] & 1)) K.st[p] = ZK_E_RNG_EXHAUSTED;
}
void launch_share_msg(hipStream_t s, const ShareLane& K, const uint32_t* keys_w, uint32_t j, uint32_t count, uint64_t first, const ShareProveIo& io) {
    hipLaunchKernelGGL(k_share_msg, dim3((count + 63) / 64), dim3(64), 0, s, K, keys_w, j, count, first, io);
}
// One workgroup of 128 threads per tag, one 32-bit word of the slot each (66 of them): the header, the three points (lanes 1..6 make a coordinate each), the
// response (lane 7).  A failed share's slot is 66 zero words.  Every byte of the slot is written once.
__global__ void __launch_bounds__(128) k_share_respond(ShareLane K, ShareSecret A, uint32_t count, uint64_t first, ShareProveIo io) {
    __shared__ uint32_t sl[128];
    const uint32_t p = blockIdx.x, t = threadIdx.x;
    const int32_t st = K.st[p];
    if (st == ZK_OK) {
        if (t == 0) sl[0] = ZK_MAGIC_ZKS1, sl[1] = bswap32(ZKS1_SIZE), sl[2] = bswap32(A.j), sl[3] = 0;
        else if (t < 7) {
            const uint32_t e = shr_point_slot(count, p, (t - 1) >> 1);
            uint32_t w[9];
            words_from_limbs<9>(w, soa_ld<ModT, 1>((t - 1) & 1 ? K.L.ay : K.L.ax, e).l);
#pragma unroll
            for (int i = 0; i < 9; i++) sl[4 + 9 * (t - 1) + i] = bswap32(w[8 - i]);
        } else if (t == 7) {
            uint32_t w[8];
#pragma unroll
            for (int i = 0; i < 8; i++) w[i] = A.a8[i];
            Sq aj;
            limbs_from_words<8>(aj.l, w);
            words_from_limbs<8>(w, share_respond(soa_ld<ModQ, 1>(K.L.v, p), K.chal + 4 * p, aj).l);
#pragma unroll
            for (int i = 0; i < 8; i++) sl[ZKS1_S / 4 + i] = bswap32(w[7 - i]);
        }
    }
    __syncthreads();
    if (t < ZKS1_WORDS) ((uint32_t*)(io.out + (first + p) * ZKS1_SIZE))[t] = st == ZK_OK ? sl[t] : 0;
    if (t == 0) io.status[first + p] = st;
}
void launch_share_respond(hipStream_t s, const ShareLane& K, const ShareSecret& A, uint32_t count, uint64_t first, const ShareProveIo& io) {
    hipLaunchKernelGGL(k_share_respond, dim3(count), dim3(128), 0, s, K, A, count, first, io);
}

// ------------------------------------------------------------------ the share verifier
ZK_DEV bool shr_share_header(const uint8_t* sh, uint32_t& j) {   // everything but the range of j
    const uint32_t* h = (const uint32_t*)sh;
    j = bswap32(h[2]);
    return h[0] == ZK_MAGIC_ZKS1 && h[1] == bswap32(ZKS1_SIZE) && h[3] == 0;
}
// One thread per share: both headers, j in 1..n, the four points' encoding, s reduced as the Scalar constructor reduces it (its comb opening and its words),
// and the challenge's message.
__global__ void __launch_bounds__(64) k_share_parse(ShareLane K, const uint32_t* keys_w, uint32_t n, uint32_t count, uint64_t first, ShareVerifyIo io) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint64_t b = first + p;
    const uint8_t *tag = io.tags + b * ZKT1_SIZE, *sh = io.shares + b * ZKS1_SIZE;
    uint32_t j;
    bool ok = shr_share_header(sh, j) && j >= 1 && j <= n && shr_tag_header(tag);
    const uint32_t jj = j >= 1 && j <= n ? j - 1 : 0;
    uint8_t* m = K.msg + (size_t)p * ZKS1_MSG_BLOCKS * 64;
    uint32_t w[18];
#pragma unroll
    for (int i = 0; i < 18; i++) w[i] = keys_w[18 * jj + i];
    lk_put_point(m, w, w + 9);
#pragma unroll 1
    for (int k = 0; k < 4; k++) {   // E1, D, U1, U2
        ok = lk_load_point(k == 0 ? tag + ZKT1_PT(0) : sh + ZKS1_PT(k - 1), w) && ok;
        lk_put_point(m + 67 * (1 + k), w, w + 9);
    }
    shr_put_padding(m);
    K.st[p] = ok ? ZK_OK : ZK_E_BAD_ENCODING;
    const Sq s = lk_load_scalar(sh + ZKS1_S);
    soa_st(K.L.v, p, s), soa_st(K.L.r, p, fe_zero<ModQ>());
    uint32_t s8[8];
    words_from_limbs<8>(s8, s.l);
#pragma unroll
    for (int i = 0; i < 8; i++) K.kw[8 * p + i] = s8[i];
}
void launch_share_parse(hipStream_t s, const ShareLane& K, const uint32_t* keys_w, uint32_t n, uint32_t count, uint64_t first, const ShareVerifyIo& io) {
    hipLaunchKernelGGL(k_share_parse, dim3((count + 63) / 64), dim3(64), 0, s, K, keys_w, n, count, first, io);
}
// One lane per (relation, share), all values public.  Lanes 0 .. count - 1: s E1 + c D - U2 = O through the two-base ladder (distinct.h: dist_relation5's
// shape); lanes count .. 2 count - 1: (s g) + c A_j - U1 = O (link.h: link_relation, its comb part from the list).
__global__ void __launch_bounds__(64) k_share_relations(ShareLane K, const uint32_t* keys_w, uint32_t count, uint64_t first, ShareVerifyIo io) {
    const uint32_t t = gtid();
    if (t >= 2 * count) return;
    const uint32_t which = t >= count ? 1 : 0, p = t - which * count;
    const uint64_t b = first + p;
    bool rel = false;
    if (K.st[p] == ZK_OK) {
        const uint8_t *tag = io.tags + b * ZKT1_SIZE, *sh = io.shares + b * ZKS1_SIZE;
        uint32_t w[18];
        if (which == 0) {
            (void)lk_load_point(tag + ZKT1_PT(0), w);
            const TomPt e1 = lk_point_from_words(w);
            (void)lk_load_point(sh + ZKS1_PT(0), w);
            const TomPt d = lk_point_from_words(w);
            (void)lk_load_point(sh + ZKS1_PT(2), w);
            rel = dist_relation5(e1, K.kw + 8 * p, d, K.chal + 4 * p, lk_point_from_words(w), K.tab + (size_t)p * DIST_TAB_QUADS);
        } else {
            uint32_t j;
            (void)shr_share_header(sh, j);
#pragma unroll
            for (int i = 0; i < 18; i++) w[i] = keys_w[18 * (j - 1) + i];
            const TomPt aj = lk_point_from_words(w);
            (void)lk_load_point(sh + ZKS1_PT(1), w);
            const TomPt sg = link_from_triple(soa_ld<ModT, 2>(K.L.proj.x, p), soa_ld<ModT, 2>(K.L.proj.y, p), soa_ld<ModT, 2>(K.L.proj.z, p));
            rel = link_relation(aj, K.chal + 4 * p, sg, lk_point_from_words(w));
        }
    }
    K.rel[t] = rel ? 1 : 0;
}
void launch_share_relations(hipStream_t s, const ShareLane& K, const uint32_t* keys_w, uint32_t count, uint64_t first, const ShareVerifyIo& io) {
    hipLaunchKernelGGL(k_share_relations, dim3((2 * count + 63) / 64), dim3(64), 0, s, K, keys_w, count, first, io);
}
__global__ void __launch_bounds__(256) k_share_verdict(ShareLane K, uint32_t count, uint64_t first, ShareVerifyIo io) {   // the AND of a share's two relations
    const uint32_t p = gtid();
    if (p >= count) return;
    io.ok[first + p] = (K.rel[p] & K.rel[count + p] & 1) ? 1 : 0;
    io.status[first + p] = K.st[p];
}
void launch_share_verdict(hipStream_t s, const ShareLane& K, uint32_t count, uint64_t first, const ShareVerifyIo& io) {
    hipLaunchKernelGGL(k_share_verdict, dim3((count + 255) / 256), dim3(256), 0, s, K, count, first, io);
}

// ------------------------------------------------------------------ combine
// One thread per value: the t coefficients for the value at at[i] (nullptr: at 0), eight little-endian words each
__global__ void __launch_bounds__(64) k_share_lagrange(const uint32_t* idx, uint32_t t, const uint32_t* at, uint32_t evals, uint32_t* lam) {
    const uint32_t i = gtid();
    if (i >= evals) return;
#pragma unroll 1
    for (uint32_t s = 0; s < t; s++) {
        uint32_t w[8];
        words_from_limbs<8>(w, share_lagrange(idx, t, s, at ? at[i] : 0).l);
#pragma unroll
        for (int k = 0; k < 8; k++) lam[8 * ((size_t)i * t + s) + k] = w[k];
    }
}
void launch_share_lagrange(hipStream_t s, const uint32_t* idx, uint32_t t, const uint32_t* at, uint32_t evals, uint32_t* lam) {
    hipLaunchKernelGGL(k_share_lagrange, dim3((evals + 63) / 64), dim3(64), 0, s, idx, t, at, evals, lam);
}
// One lane per tag: the tag's header, E1 and E2, every slot's share header (its j is the slot's auditor) and D; then sum lambda_j D_j as one joint ladder
// over the lane's addends in `tab` (count lanes wide), whose branches on the coefficients' bits are the same for every lane; 4 (E2 - sum) as the
// projective triple of the tags' list.  A refused tag walks identities and leaves the identity there, status 10, and the lookup skips it.
__global__ void __launch_bounds__(64) k_share_combine(EscrowOpen O, ShareCombineIo io, const uint32_t* lam, uint32_t* tab, uint32_t count, uint64_t first, uint32_t* index,
                                                      int32_t* status) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint64_t b = first + p;
    const uint8_t* tag = io.tags + b * ZKT1_SIZE;
    uint32_t w[18];
    bool ok = shr_tag_header(tag);
    ok = lk_load_point(tag + ZKT1_PT(0), w) && ok;
    ok = lk_load_point(tag + ZKT1_PT(1), w) && ok;
    TomPt e2 = lk_point_from_words(w);
#pragma unroll 1
    for (uint32_t s = 0; s < io.t; s++) {
        const uint8_t* sh = io.shares + ((uint64_t)s * io.B + b) * ZKS1_SIZE;
        uint32_t j;
        ok = shr_share_header(sh, j) && j == io.auditors[s] && ok;
        ok = lk_load_point(sh + ZKS1_PT(0), w) && ok;
    }
    if (!ok) e2 = tom_identity();
    const ShareTab T{tab + p, count};
#pragma unroll 1
    for (uint32_t s = 0; s < io.t; s++) {
        (void)lk_load_point(io.shares + ((uint64_t)s * io.B + b) * ZKS1_SIZE + ZKS1_PT(0), w);
        TomPt d = lk_point_from_words(w);
        if (!ok) d = tom_identity();
        share_tab_put(T, s, d);
    }
    shr_put_triple(O.T.proj, (uint32_t)b, share_combine_point(e2, share_joint_ladder(T, lam, io.t)));
    O.st[b] = ok ? ZK_OK : ZK_E_BAD_ENCODING;
    status[b] = ok ? ZK_OK : ZK_E_BAD_ENCODING;
    index[b] = 0xffffffffu;
}
void launch_share_combine(hipStream_t s, const EscrowOpen& O, const ShareCombineIo& io, const uint32_t* lam, uint32_t* tab, uint32_t count, uint64_t first, uint32_t* index,
                          int32_t* status) {
    hipLaunchKernelGGL(k_share_combine, dim3((count + 63) / 64), dim3(64), 0, s, O, io, lam, tab, count, first, index, status);
}
// zk_ctx_set_auditors' consistency check: lane i interpolates the first t keys (validated before) at its value through the combine's ladder
__global__ void __launch_bounds__(64) k_share_interpolate(const uint8_t* keys72, uint32_t t, const uint32_t* lam, uint32_t evals, uint32_t* tab, TomList L) {
    const uint32_t i = gtid();
    if (i >= evals) return;
    const ShareTab T{tab + i, evals};
#pragma unroll 1
    for (uint32_t s = 0; s < t; s++) {
        uint32_t w[18];
        (void)lk_load_point(keys72 + 72 * s, w);
        share_tab_put(T, s, lk_point_from_words(w));
    }
    shr_put_triple(L.proj, i, share_joint_ladder(T, lam + 8 * (size_t)i * t, t));
}
void launch_share_interpolate(hipStream_t s, const uint8_t* keys72, uint32_t t, const uint32_t* lam, uint32_t evals, uint32_t* tab, const TomList& L) {
    hipLaunchKernelGGL(k_share_interpolate, dim3((evals + 63) / 64), dim3(64), 0, s, keys72, t, lam, evals, tab, L);
}

// ------------------------------------------------------------------ the dealer
// One thread per share j = 1..n: f(j) by Horner's rule, every coefficient drawn where it is needed (the draws are random-access; nothing is kept in an array).
// Lane 0 alone judges the RNG while every lane writes its share: where the flag comes out set, what the lanes wrote is meaningless, stays in the witness-flagged
// arena, and the host copies none of it out before it wipes the arena.
__global__ void __launch_bounds__(64) k_share_split(RngCtx rng, const uint8_t* secret, uint32_t t, uint32_t n, TomList L, uint8_t* shares_be32, uint32_t* flag) {
    const uint32_t i = gtid();
    if (i >= n) return;
    if (i == 0) {
        const uint32_t cnt = rng.exc_cnt[0];
        uint32_t rej = 0;
        for (uint32_t e = 0; e < (cnt < RNG_MAX_EXC ? cnt : RNG_MAX_EXC); e++) rej += (rng.exc_flags[e] >> 1) & 1;
        flag[0] = cnt > RNG_MAX_EXC || (rng.mode == 1 && t - 1 + rej > rng.stride_blocks);
    }
    const Sq a = share_eval([&](uint32_t k) { return k == 0 ? lk_load_scalar(secret) : rng_draw<ModQ>(rng, 0, k - 1); }, t, i + 1);
    soa_st(L.v, i, a), soa_st(L.r, i, fe_zero<ModQ>());
    uint32_t w[8];
    words_from_limbs<8>(w, a.l);
#pragma unroll
    for (int k = 0; k < 8; k++) ((uint32_t*)shares_be32)[8 * i + k] = bswap32(w[7 - k]);
}
void launch_share_split(hipStream_t s, const RngCtx& rng, const uint8_t* secret, uint32_t t, uint32_t n, const TomList& L, uint8_t* shares_be32, uint32_t* flag) {
    hipLaunchKernelGGL(k_share_split, dim3(1), dim3(64), 0, s, rng, secret, t, n, L, shares_be32, flag);
}
