// Key recovery (include/zkattest.h: zk_recover_batch): the signer's key from (msgHash, signature) alone, and its place in the ring.
//
// A P-256 signature (r, s) over z determines its signer up to four candidates Q = (s R - z G) / r, one per curve point R whose x is r mod n: x = r or
// r + n (the latter only where r + n < p), y even or odd.  The reference has no counterpart: its prover takes the key from the caller
// (src/zkpAttestList.ts:104-118).  Per chunk and pass (pass 0: x = r, pass 1: x = r + n):
//   k_recover_front   pass 0: the chunk's initial state, ring residency, the range of (r, s); both: the lift of x to R with even y (recover.h: rec_candidate_x, rec_lift_x),
//                     u1 = -z / r, u2 = s / r mod n (ONE inversion, of r), u2's digits -- all in the screen's scratch-area layout with R in pk's place
//   k_recover_table   u1 * G by the fixed-base comb and 1..8 times R (k_screen_table's body on the walk path)
//   k_recover_tail    Bp = u2 * R by the prover's 65-window walk, Q0 = A + Bp and Q1 = A - Bp -- ONE walk for both parities --, canonical affine through one
//                     shared inversion (recover.h: rec_tail), the two 64-byte records and their pseudo-witness ids
// then the screen's own lookup (k_screen.hip: k_screen_lookup, unchanged) over the up to four candidates of every witness as pseudo-witnesses, and
//   k_recover_select  lowest index, ties to the lowest candidate (recover.h: rec_select): pk_xy_out, which_out, flags.
// The kernels are split like the screen's so that no live set exceeds 256 registers.  The walk and the comb sum are the prover's device functions
// (rtab.h: ZK_ADD_IF / p256_select): no digit-dependent skip in the uniform build.  Branches depend on the range of (r, s), on whether r lifts -- R is
// public in every proof -- and, in the lookup, on the candidate keys.  In pass 1 a workgroup without a witness whose r + n < p leaves at once: every
// workgroup outside adversarial inputs (r < p - n has probability 2^-128).
// A chunk of at most ZK_SCREEN_CO_MAX witnesses takes the square root and the point arithmetic on cooperating waves instead (below): k_recover_front_co,
// k_recover_walk_co; ZKATTEST_ONE_LANE_CHAINS keeps every chunk on the one-lane kernels.
#include "rtab.h"
#include "coop_sums.h"   // the walk and the comb sum of a chunk of a few witnesses on cooperating waves
#include "recover.h"

// the front end before the lift: pass 0 writes the chunk's initial state (`writer`: one lane per witness does).  Returns whether the pass has an x-candidate.
ZK_DEV bool rec_front_begin(const RecoverIn& in, const RecoverBuf& buf, const RingSlots& rs, uint32_t pass, uint32_t b, bool writer, uint32_t rw[8], uint32_t& st, Fe<ModQ, 1>& x) {
    load_be32(in.sig + 64 * (size_t)b, rw);
    if (!pass) {
        bool resident = !in.ids;
        if (in.ids)
            for (uint32_t k = 0; k < rs.count; k++) resident = resident || rs.id[k] == in.ids[b];
        uint32_t sw[8], ro = 0, so = 0;
        load_be32(in.sig + 64 * (size_t)b + 32, sw);
#pragma unroll
        for (int i = 0; i < 8; i++) ro |= rw[i], so |= sw[i];
        // FIPS 186: r, s in [1, n - 1] as 256-bit integers
        st = !resident ? REC_ST_NORING : (!ro || !so || words_geq<8>(rw, ModN::mod32) || words_geq<8>(sw, ModN::mod32)) ? REC_ST_RANGE : 0u;
        if (writer) {
#pragma unroll 1
            for (uint32_t c = 0; c < REC_NCAND; c++) buf.cand_ids[c * in.count + b] = REC_NO_RING, buf.cand_which[c * in.count + b] = ZK_WHICH_NONE;
            scr_area(buf.scratch, b)[SCR_USE] = SCR_SKIP;
            buf.state[b] = st;
        }
    } else st = buf.state[b];
    return !(st & (REC_ST_RANGE | REC_ST_NORING)) && rec_candidate_x(rw, pass, x);
}
// ... and behind it: the state, the scalars and the area of a witness whose x lifted to R (one lane)
ZK_DEV void rec_front_finish(const RecoverIn& in, const RecoverBuf& buf, uint32_t pass, uint32_t b, uint32_t st, const uint32_t rw[8], const P256Aff& R) {
    buf.state[b] = st | (pass ? REC_ST_LIFT1 : REC_ST_LIFT0);
    uint32_t zw[8], sw[8];
    load_be32(in.msg + 32 * (size_t)b, zw);
    load_be32(in.sig + 64 * (size_t)b + 32, sw);
    // u1 = -z / r, u2 = s / r mod n with z = truncateToN(msg_hash) as the prover and the screen take it; r != 0 here
    const Fn2 z = fe_to_mont(fe_from_words256_reduce<ModN>(zw));
    const Fn2 s = fe_to_mont(fe_from_words256_reduce<ModN>(sw));
    const Fn2 rinv = fe_inv<ModN>(fe_to_mont(fe_from_words256_reduce<ModN>(rw)));
    const Fe<ModN, 1> u1 = fe_from_mont(rinv * fe_neg(z)), u2 = fe_from_mont(rinv * s);
    uint32_t* area = scr_area(buf.scratch, b);
    words_from_limbs<8>(area + SCR_U1, u1.l);
    uint32_t u2w[8];
    words_from_limbs<8>(u2w, u2.l);
#pragma unroll
    for (int i = 0; i < 8; i++) area[SCR_U2 + i] = u2w[i];
    front_recode(u2w, (uint8_t*)(area + SCR_DIG));
#pragma unroll
    for (int l = 0; l < NLIMB; l++) area[SCR_PK + l] = R.x.l[l], area[SCR_PK + NLIMB + l] = R.y.l[l];
    *(const uint32_t**)(area + SCR_KT) = nullptr;
    area[SCR_USE] = 0;
}
__global__ void __launch_bounds__(64, 2) k_recover_front(RecoverIn in, RecoverBuf buf, RingSlots rs, uint32_t pass) {
    const uint32_t b = gtid();
    uint32_t rw[8], st = 0;
    Fe<ModQ, 1> x;
    const bool want = b < in.count && rec_front_begin(in, buf, rs, pass, b, true, rw, st, x);
    if (pass && !__syncthreads_or(want)) return;
    if (!want) return;
    P256Aff R;
    if (!rec_lift_x(x, R)) return;
    rec_front_finish(in, buf, pass, b, st, rw, R);
}

__global__ void __launch_bounds__(64, 2) k_recover_table(DevParams P, uint32_t count, uint32_t* scratch) {
    const uint32_t b = gtid();
    if (b >= count) return;
    uint32_t* area = scr_area(scratch, b);
    if (area[SCR_USE] != 0) return;
    P256Aff R;
#pragma unroll
    for (int l = 0; l < NLIMB; l++) R.x.l[l] = area[SCR_PK + l], R.y.l[l] = area[SCR_PK + NLIMB + l];
    front_pk_multiples(area, R);
    uint32_t kw[8];
#pragma unroll
    for (int i = 0; i < 8; i++) kw[i] = area[SCR_U1 + i];
    st_rtab(area + 8 * RTAB_ENTRY_WORDS, p256_fixed_mul(P.pfix_G, kw));
}

// the two records of a pass and the ids of their pseudo-witnesses; an identity is no key: its slot keeps REC_NO_RING and the lookup passes it by
ZK_DEV void rec_store_pair(const RecoverIn& in, const RecoverBuf& buf, uint32_t b, uint32_t pass, const RecPair& o) {
#pragma unroll
    for (uint32_t k = 0; k < 2; k++) {
        if (o.ident[k]) continue;
        const uint32_t slot = (2 * pass + k) * in.count + b;
        store_scalar_be(buf.cand + 64 * (size_t)slot, o.x[k]);
        store_scalar_be(buf.cand + 64 * (size_t)slot + 32, o.y[k]);
        buf.cand_ids[slot] = in.ids ? in.ids[b] : in.plain_id;
    }
}
__global__ void __launch_bounds__(64, 2) k_recover_tail(RecoverIn in, RecoverBuf buf, uint32_t pass) {
    const uint32_t b = gtid();
    if (b >= in.count) return;
    uint32_t* area = scr_area(buf.scratch, b);
    if (area[SCR_USE] != 0) return;
    const P256Pt Bp = front_walk(area, (const uint8_t*)(area + SCR_DIG));   // (u1 * G is loaded behind the walk, as in k_screen_walk)
    RecPair o;
    rec_tail<true>(ld_rtab(area + 8 * RTAB_ENTRY_WORDS), Bp, o);
    rec_store_pair(in, buf, b, pass, o);
    area[SCR_USE] = SCR_SKIP;   // consumed: the next pass starts from an idle chunk
}

__global__ void __launch_bounds__(256) k_recover_select(RecoverIn in, RecoverBuf buf) {
    const uint32_t b = gtid();
    if (b >= in.count) return;
    const uint32_t st = buf.state[b];
    uint32_t idx[REC_NCAND], win = REC_NCAND, fl;
#pragma unroll
    for (uint32_t c = 0; c < REC_NCAND; c++) idx[c] = buf.cand_which[c * in.count + b];
    if (st & REC_ST_NORING) fl = ZK_RECOVER_RING_NOT_RESIDENT;
    else if (st & REC_ST_RANGE) fl = ZK_RECOVER_SIG_RANGE;
    else {
        win = rec_select(idx);
        fl = win < REC_NCAND ? 0u : (ZK_RECOVER_NOT_IN_RING | ((st & (REC_ST_LIFT0 | REC_ST_LIFT1)) ? 0u : ZK_RECOVER_NO_POINT));
    }
    const uint32_t* src = (const uint32_t*)(buf.cand + 64 * (size_t)((win < REC_NCAND ? win : 0) * in.count + b));
    uint32_t* dst = (uint32_t*)(in.pk_out + 64 * (size_t)b);
#pragma unroll
    for (int i = 0; i < 16; i++) dst[i] = win < REC_NCAND ? src[i] : 0u;
    in.which_out[b] = win < REC_NCAND ? idx[win] : ZK_WHICH_NONE;
    in.flags[b] = fl;
}

// ---------------------------------------------------------------- a chunk of a few witnesses: the square root and the point arithmetic on cooperating waves
// At most ZK_SCREEN_CO_MAX witnesses, as for the screen (k_screen.hip: k_screen_walk_co).  Same group elements as the one-lane kernels and the same one-lane
// endings on exact limbs (recover.h: rec_lift_point, rec_pair_affine), hence the same canonical bytes.  Nothing witness-derived leaves the area and LDS.
// One wave per witness: the lift's v^((p+1)/4) by co_pow_words (every row raises the same v), the rest of the front end in lane 0.
__global__ void __launch_bounds__(64) k_recover_front_co(RecoverIn in, RecoverBuf buf, RingSlots rs, uint32_t pass) {
    __shared__ uint32_t vl[16], yl[16];
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    uint32_t rw[8], st = 0;
    Fe<ModQ, 1> x;
    if (!rec_front_begin(in, buf, rs, pass, b, lane == 0, rw, st, x)) return;   // (uniform for the wave)
    const Fq2 v = rec_lift_v(x);
    if (lane < NLIMB) vl[lane] = v.l[lane];
    __syncthreads();
    const CoU32 mj = co_limbs(ModQ::mod);
    const CoFe<ModQ, 2> cy = co_pow_words<ModQ>(co_load4<ModQ, 2>(vl, vl, vl, vl), ModQ::exp_sqrt, mj);
    co_store4(cy, yl, nullptr, nullptr, nullptr);
    __syncthreads();
    if (lane) return;
    Fq2 y;
#pragma unroll
    for (int l = 0; l < NLIMB; l++) y.l[l] = yl[l];
    P256Aff R;
    if (!rec_lift_point(x, v, y, R)) return;
    rec_front_finish(in, buf, pass, b, st, rw, R);
}
// One workgroup of four waves per witness, k_screen_walk_co's plan: wave 0 holds 1..8 times R in LDS and walks u2's digits while waves 1..3 sum u1 * G from the
// comb; the ending is A +- Bp, co_normalize, and the shared inversion of rec_pair_affine in lane 0 of wave 0.
__global__ void __launch_bounds__(256) k_recover_walk_co(DevParams P, RecoverIn in, RecoverBuf buf, uint32_t pass) {
    __shared__ uint32_t mult[CO_WALK_MULT_WORDS];
    __shared__ uint32_t part[2][64];
    __shared__ uint32_t u1g[64];
    __shared__ uint32_t qs[2][64];
    const uint32_t b = blockIdx.x, q = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t* area = scr_area(buf.scratch, b);
    if (area[SCR_USE] != 0) return;   // (uniform for the workgroup)
    const CoU32 mj = co_limbs(ModQ::mod);
    CoP256 acc;
    if (!q) {
        CoP256 R;
        R.v = co_load_pfix(area + SCR_PK);
        co_front_pk_multiples(mult, R, mj);
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
    CoP256 A, Bp, nB;
    A.v.v = u1g[lane];
    const CoFe<ModQ, 2> bp = co_mul(acc.v, co_const<ModQ>(ModQ::one), mj);   // below 2 q, so that 4 q - Y stays within a point register's bound (co_front_walk)
    CoFe<ModQ, 0> zero;
    zero.v = co_splat(0);
    Bp.v = bp.template as<8>();
    nB.v = co_pick(co_row_is(1), co_sub(zero, bp), bp).template as<8>();
    qs[0][lane] = co_normalize(co_p256_add(A, Bp, mj).v).v;
    qs[1][lane] = co_normalize(co_p256_add(A, nB, mj).v).v;
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    if (lane) return;
    P256Pt Q[2];
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
        for (int l = 0; l < NLIMB; l++) Q[k].x.l[l] = qs[k][l], Q[k].y.l[l] = qs[k][16 + l], Q[k].z.l[l] = qs[k][32 + l];
    RecPair o;
    rec_pair_affine<false>(Q[0], Q[1], o);
    rec_store_pair(in, buf, b, pass, o);
    area[SCR_USE] = SCR_SKIP;
}

static bool recover_co(const RecoverIn& in) { return in.count <= ZK_SCREEN_CO_MAX && !zk_one_lane_chains(); }
void launch_recover_lift(hipStream_t s, const RecoverIn& in, const RecoverBuf& buf, const RingSlots& rs, uint32_t pass) {
    if (recover_co(in)) hipLaunchKernelGGL(k_recover_front_co, dim3(in.count), dim3(64), 0, s, in, buf, rs, pass);
    else hipLaunchKernelGGL(k_recover_front, dim3((in.count + 63) / 64), dim3(64), 0, s, in, buf, rs, pass);
}
void launch_recover_points(hipStream_t s, const DevParams& P, const RecoverIn& in, const RecoverBuf& buf, uint32_t pass) {
    if (recover_co(in)) {   // four chains per witness and pass, as the screen counts them (zk_test_counter 4)
        g_coop_chains.fetch_add((uint64_t)in.count * 4, std::memory_order_relaxed);
        hipLaunchKernelGGL(k_recover_walk_co, dim3(in.count), dim3(256), 0, s, P, in, buf, pass);
        return;
    }
    hipLaunchKernelGGL(k_recover_table, dim3((in.count + 63) / 64), dim3(64), 0, s, P, in.count, buf.scratch);
    hipLaunchKernelGGL(k_recover_tail, dim3((in.count + 63) / 64), dim3(64), 0, s, in, buf, pass);
}
void launch_recover_select(hipStream_t s, const RecoverIn& in, const RecoverBuf& buf) {
    hipLaunchKernelGGL(k_recover_select, dim3((in.count + 255) / 256), dim3(256), 0, s, in, buf);
}
