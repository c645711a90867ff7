// Link proofs (include/zkattest.h: zk_link_*, zk_proof_key_commitments): proveEquality / verifyEquality (equality.ts:60-116) for two commitments the caller
// brings, outside any ZKAttest proof.  The kernels around the shared machinery -- the commitments are k_tom.hip's pair form, the challenge hash k_hash.hip's
// message path (launch_sha_msgs), the arithmetic link.h's: the prover's front end (validation, the three draws, the openings), the opening compare and the
// challenge's message behind the normaliser, the responses with the 256-byte writer; the verifier's parser and its ladder; the keyXcom extractor.
#include "link.h"
#include "rering_plan.h"   // rr_head: where a ZKA1 / ZK1P proof's header and slot are sound

typedef Fe<ModQ, 1> Sq;
typedef Fe<ModT, 1> St;

ZK_DEV void lk_put_padding(uint8_t* m) {   // behind the 268 message bytes: 0x80, zeros, the bit length
    m[268] = 0x80;
#pragma unroll
    for (int i = 269; i < 318; i++) m[i] = 0;
    m[318] = (uint8_t)((268 * 8) >> 8), m[319] = (uint8_t)(268 * 8);
}

// ------------------------------------------------------------------ prover
// One thread per proof.  Draws (equality.ts:62-64 under the randomness contract): 0 k, 1 s1, 2 s2, all mod q.  Writes the status of the commitments' encoding,
// the RNG flag, the commitments' words and the four openings of the chunk's list.
__global__ void __launch_bounds__(64) k_link_front(LinkLane K, uint32_t count, uint64_t first, LinkProveIo io) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint64_t b = first + p;
    uint32_t cw[36];
    const bool ok1 = lk_load_point(io.com1 + 72 * b, cw), ok2 = lk_load_point(io.com2 + 72 * b, cw + 18);
#pragma unroll
    for (int i = 0; i < 36; i++) K.cw[36 * p + i] = cw[i];
    K.st[p] = ok1 && ok2 ? ZK_OK : ZK_E_BAD_ENCODING;
    // fills the proof consumes: its three draws plus the rejected ones among them (k_m_front's rule)
    const uint32_t cnt = K.rng.exc_cnt[p];
    uint32_t rej = 0;
    for (uint32_t i = 0; i < (cnt < RNG_MAX_EXC ? cnt : RNG_MAX_EXC); i++) rej += (K.rng.exc_flags[p * RNG_MAX_EXC + i] >> 1) & 1;
    K.flags[p] = cnt > RNG_MAX_EXC || (K.rng.mode == 1 && 3 + rej > K.rng.stride_blocks);
    const Sq k = rng_draw<ModQ>(K.rng, p, 0), x = lk_load_scalar(io.key + 32 * b);
    soa_st(K.L.v, 2 * p, k), soa_st(K.L.r, 2 * p, rng_draw<ModQ>(K.rng, p, 1));
    soa_st(K.L.v, 2 * p + 1, k), soa_st(K.L.r, 2 * p + 1, rng_draw<ModQ>(K.rng, p, 2));
    const uint32_t e = 2 * count + 2 * p;
    soa_st(K.L.v, e, x), soa_st(K.L.r, e, lk_load_scalar(io.blinder1 + 32 * b));
    soa_st(K.L.v, e + 1, x), soa_st(K.L.r, e + 1, lk_load_scalar(io.blinder2 + 32 * b));
}
void launch_link_front(hipStream_t s, const LinkLane& K, uint32_t count, uint64_t first, const LinkProveIo& io) {
    hipLaunchKernelGGL(k_link_front, dim3((count + 63) / 64), dim3(64), 0, s, K, count, first, io);
}
// Behind the normaliser, one thread per proof.  The openings x g + r1 h, x g + r2 h (canonical) against the commitments as the caller states them, word for
// word (k_rr_compare's rule), then the RNG; and the padded message of hashPoints([C1, C2, A1, A2]).
__global__ void __launch_bounds__(64) k_link_opening_msg(LinkLane K, uint32_t count) {
    const uint32_t p = gtid();
    if (p >= count) return;
    uint32_t w[18];
    uint8_t* m = K.msg + (size_t)p * ZKL1_MSG_BLOCKS * 64;
    uint32_t diff = 0;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const uint32_t e = 2 * count + 2 * p + j;
        words_from_limbs<9>(w, soa_ld<ModT, 1>(K.L.ax, e).l);
        words_from_limbs<9>(w + 9, soa_ld<ModT, 1>(K.L.ay, e).l);
#pragma unroll
        for (int i = 0; i < 18; i++) diff |= w[i] ^ K.cw[36 * p + 18 * j + i];
#pragma unroll
        for (int i = 0; i < 18; i++) w[i] = K.cw[36 * p + 18 * j + i];
        lk_put_point(m + 67 * j, w, w + 9);
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        words_from_limbs<9>(w, soa_ld<ModT, 1>(K.L.ax, 2 * p + j).l);
        words_from_limbs<9>(w + 9, soa_ld<ModT, 1>(K.L.ay, 2 * p + j).l);
        lk_put_point(m + 67 * (2 + j), w, w + 9);
    }
    lk_put_padding(m);
    if (K.st[p] == ZK_OK) K.st[p] = diff ? ZK_E_OPENING : (K.flags[p] & 1) ? ZK_E_RNG_EXHAUSTED : ZK_OK;
}
void launch_link_opening_msg(hipStream_t s, const LinkLane& K, uint32_t count) {
    hipLaunchKernelGGL(k_link_opening_msg, dim3((count + 63) / 64), dim3(64), 0, s, K, count);
}
// One workgroup of 64 threads per proof, one 32-bit word of the slot each: the header, A_1, A_2 (lanes 1..4 make a coordinate each), the responses (lanes 5..7
// one each).  A failed proof's slot is 64 zero words.  Every byte of the slot is written once.
__global__ void __launch_bounds__(64) k_link_respond(LinkLane K, uint32_t count, uint64_t first, LinkProveIo io) {
    __shared__ uint32_t sl[64];
    const uint32_t p = blockIdx.x, t = threadIdx.x;
    const int32_t st = K.st[p];
    if (st == ZK_OK) {
        if (t == 0) sl[0] = ZK_MAGIC_ZKL1, sl[1] = bswap32(ZKL1_SIZE), sl[2] = 0, sl[3] = 0;
        else if (t < 5) {
            const uint32_t e = 2 * p + ((t - 1) >> 1);
            uint32_t w[9];
            words_from_limbs<9>(w, soa_ld<ModT, 1>((t - 1) & 1 ? K.L.ay : K.L.ax, e).l);
#pragma unroll
            for (int i = 0; i < 9; i++) sl[4 + 9 * (t - 1) + i] = bswap32(w[8 - i]);
        } else if (t < 8) {
            const uint32_t j = t - 5;   // 0: t_x = k - c x; 1, 2: t_r = s - c r
            const uint32_t e = 2 * count + 2 * p;
            const Sq k = j == 0 ? soa_ld<ModQ, 1>(K.L.v, 2 * p) : soa_ld<ModQ, 1>(K.L.r, 2 * p + j - 1);
            const Sq v = j == 0 ? soa_ld<ModQ, 1>(K.L.v, e) : soa_ld<ModQ, 1>(K.L.r, e + j - 1);
            uint32_t w[8];
            words_from_limbs<8>(w, link_respond(k, K.chal + 4 * p, v).l);
#pragma unroll
            for (int i = 0; i < 8; i++) sl[40 + 8 * j + i] = bswap32(w[7 - i]);
        }
    }
    __syncthreads();
    ((uint32_t*)(io.out + (first + p) * ZKL1_SIZE))[t] = st == ZK_OK ? sl[t] : 0;
    if (t == 0) io.status[first + p] = st;
}
void launch_link_respond(hipStream_t s, const LinkLane& K, uint32_t count, uint64_t first, const LinkProveIo& io) {
    hipLaunchKernelGGL(k_link_respond, dim3(count), dim3(64), 0, s, K, count, first, io);
}

// ------------------------------------------------------------------ verifier
// One thread per proof: the header, the four points' encoding (edwards.ts:204-209: range and curve equation), the scalars reduced as the Scalar constructor
// reduces them (what zk_verify_batch does with an EqualityProof's scalars inside ZKA1), the comb parts' openings and the challenge's message.
__global__ void __launch_bounds__(64) k_link_parse(LinkLane K, uint32_t count, uint64_t first, LinkVerifyIo io) {
    const uint32_t p = gtid();
    if (p >= count) return;
    const uint64_t b = first + p;
    const uint8_t* pr = io.proofs + b * ZKL1_SIZE;
    const uint32_t* h = (const uint32_t*)pr;
    bool ok = h[0] == ZK_MAGIC_ZKL1 && h[1] == bswap32(ZKL1_SIZE) && h[2] == 0 && h[3] == 0;
    uint8_t* m = K.msg + (size_t)p * ZKL1_MSG_BLOCKS * 64;
    uint32_t w[18];
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        const uint8_t* src = j == 0 ? io.com1 + 72 * b : j == 1 ? io.com2 + 72 * b : pr + ZKL1_A1 + 72 * (j - 2);
        ok = lk_load_point(src, w) && ok;
        lk_put_point(m + 67 * j, w, w + 9);
    }
    lk_put_padding(m);
    K.st[p] = ok ? ZK_OK : ZK_E_BAD_ENCODING;
    const Sq tx = lk_load_scalar(pr + ZKL1_TX);
    soa_st(K.L.v, 2 * p, tx), soa_st(K.L.r, 2 * p, lk_load_scalar(pr + ZKL1_TX + 32));
    soa_st(K.L.v, 2 * p + 1, tx), soa_st(K.L.r, 2 * p + 1, lk_load_scalar(pr + ZKL1_TX + 64));
}
void launch_link_parse(hipStream_t s, const LinkLane& K, uint32_t count, uint64_t first, const LinkVerifyIo& io) {
    hipLaunchKernelGGL(k_link_parse, dim3((count + 63) / 64), dim3(64), 0, s, K, count, first, io);
}
// One lane per (proof, relation): lane 2 p + j checks t_x g + t_rj h + c C_j - A_j = O (link.h: link_relation), its comb part from list slot 2 p + j.  The two
// lanes of a proof are neighbours in a wave; ok is the AND of both, written with the status by the even lane.  Lanes past the chunk mirror its last lane so
// that the exchange finds every lane of the wave.
__global__ void __launch_bounds__(64) k_link_ladder(LinkLane K, uint32_t count, uint64_t first, LinkVerifyIo io) {
    const uint32_t t0 = gtid();
    const bool live = t0 < 2 * count;
    const uint32_t t = live ? t0 : 2 * count - 1, p = t >> 1, j = t & 1;
    const uint64_t b = first + p;
    const int32_t st = K.st[p];
    bool rel = false;
    if (st == ZK_OK) {
        uint32_t w[18];
        (void)lk_load_point((j ? io.com2 : io.com1) + 72 * b, w);
        const TomPt C = lk_point_from_words(w);
        (void)lk_load_point(io.proofs + b * ZKL1_SIZE + (j ? ZKL1_A2 : ZKL1_A1), w);
        const TomPt A = lk_point_from_words(w);
        const TomPt D = link_from_triple(soa_ld<ModT, 2>(K.L.proj.x, t), soa_ld<ModT, 2>(K.L.proj.y, t), soa_ld<ModT, 2>(K.L.proj.z, t));
        rel = link_relation(C, K.chal + 4 * p, D, A);
    }
    const bool other = __shfl_xor((int)rel, 1, 64) != 0;
    if (live && j == 0) io.ok[b] = rel && other ? 1 : 0, io.status[b] = st;
}
void launch_link_ladder(hipStream_t s, const LinkLane& K, uint32_t count, uint64_t first, const LinkVerifyIo& io) {
    hipLaunchKernelGGL(k_link_ladder, dim3((2 * count + 63) / 64), dim3(64), 0, s, K, count, first, io);
}

// ------------------------------------------------------------------ keyXcom of a ZKA1 / ZK1P proof
// One thread per proof.  rr_head's rules (zk_proof_rering_batch's: the slot readable and as long as the header says, the magic the context's wire layout's, room
// for the fixed part and the GKProof section); then the two coordinates behind R and comS1, widened to 36 bytes.  No curve check; a refused slot gives 72 zero bytes.
__global__ void __launch_bounds__(256) k_link_keycoms(uint64_t B, const uint8_t* __restrict__ proofs, const uint64_t* __restrict__ off, Wire wire, uint8_t* __restrict__ com,
                                                      int32_t* __restrict__ status) {
    const uint64_t b = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint64_t o0 = off[b];
    const RrHead h = rr_head(proofs, o0, off[b + 1], wire);
    uint32_t w[18];
#pragma unroll
    for (int i = 0; i < 18; i++) w[i] = 0;
    if (h.ok) {
        const uint8_t* kx = proofs + o0 + ZK_HDR + 128;
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int i = 0; i < 36; i++)
                if ((uint32_t)i < wire.tc) w[9 * c + (i >> 2)] |= (uint32_t)kx[wire.tc * c + wire.tc - 1 - i] << (8 * (i & 3));
    }
    uint32_t* o = (uint32_t*)(com + 72 * b);
#pragma unroll
    for (int i = 0; i < 9; i++) o[i] = bswap32(w[8 - i]), o[9 + i] = bswap32(w[17 - i]);
    status[b] = h.ok ? ZK_OK : ZK_E_BAD_ENCODING;
}
void launch_link_keycoms(hipStream_t s, uint64_t B, const uint8_t* proofs, const uint64_t* off, const Wire& wire, uint8_t* com, int32_t* status) {
    hipLaunchKernelGGL(k_link_keycoms, dim3((uint32_t)((B + 255) / 256)), dim3(256), 0, s, B, proofs, off, wire, com, status);
}
