// zk_ctx_set_auditor / zk_escrow_keygen / zk_escrow_prove_batch / zk_escrow_verify_batch / zk_escrow_open_batch (include/zkattest.h): escrow tags "ZKT1" --
// exponential ElGamal of a committed key under an auditor's key with a sigma proof that ties it to the commitment, and the auditor's opening against the
// active ring.  Host-side pipeline; the kernels of its own are in k_escrow.hip, the commitments are k_tom.hip's over the context's (g, h) combs and the
// auditor's (g, A) set, the challenge hash k_hash.hip's message path.  The chunks run on the context's lanes (their streams are the prover lanes'), every
// lane's arena carved from one witness-flagged buffer.
#include "ctx.h"
#include "sigma.h"
#include "escrow_share.h"
#include "accountable.h"

#define ZK_AUDITOR_BITS 16   // comb width of the (g, A) set: 0.13 GB per base (24 bits: 23 GB); a tag's bytes do not depend on it

// ------------------------------------------------------------------ the auditor's key
void escrow_drop_auditor(zk_ctx* c) {
    if (c->PA.tom_tab_h) (void)hipFree(c->PA.tom_tab_h);
    if (c->aud_tab_g) (void)hipFree(c->aud_tab_g);
    c->PA = DevParams{};
    c->aud_tab_g = nullptr, c->auditor_set = false;
    c->auditors_t = 0, c->auditors_n = 0;   // the share keys were checked against this key (zk_ctx_set_auditors)
}
extern "C" zk_status zk_ctx_set_auditor(zk_ctx* c, const uint8_t auditor_xy72[72]) {
    if (!c || !auditor_xy72) return ZK_E_ARG;
    if (c->stream_busy) return busy_refusal(c);
    if (!c->params_set) return ZK_E_BUFFER;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DevBuf d;   // 72 bytes of the key, its 18 words, g's 18 words, the kernel's two verdicts, the order check's two
    HIPCHK(c, hipMalloc(&d.p, 512));
    uint8_t* const d_xy = d.as<uint8_t>();
    uint32_t* const d_w = (uint32_t*)(d_xy + 128);
    uint32_t* const d_g = d_w + 32;
    int32_t* const d_res = (int32_t*)(d_g + 32);
    HIPCHK(c, hipMemcpyAsync(d_xy, auditor_xy72, 72, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(d_g, c->tom_g_w, 72, hipMemcpyHostToDevice, s));
    launch_escrow_check_key(s, d_xy, d_w, d_res);
    launch_tom_order_check(s, d_w, d_w, d_res + 2);
    int32_t res[4] = {0, 0, 0, 0};
    uint32_t aw[18];
    HIPCHK(c, hipMemcpyAsync(res, d_res, 16, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(aw, d_w, 72, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (!res[0]) return ZK_E_BAD_ENCODING;
    if (res[1] || !res[2]) {
        c->err = "the auditor's key is the identity or has a component outside the group of prime order";
        return ZK_E_ARG;
    }
    // from here on the previous key is gone: a failure below leaves the context without an auditor
    escrow_drop_auditor(c);
    const bool share = c->tom_bits == ZK_AUDITOR_BITS;
    HIPCHK(c, hipMalloc(&c->PA.tom_tab_h, sizeof(uint32_t) * tom_tab_words(ZK_AUDITOR_BITS)));
    if (!share) HIPCHK(c, hipMalloc(&c->aud_tab_g, sizeof(uint32_t) * tom_tab_words(ZK_AUDITOR_BITS)));
    c->PA.tom_tab_g = share ? c->P.tom_tab_g : c->aud_tab_g;
    c->PA.tom_bits = ZK_AUDITOR_BITS;
    c->PA.tom_model = c->P.tom_model;   // A has odd order, so it may live on whichever model g's table is on
    c->PA.sec = c->P.sec;
    memcpy(c->PA.tom_g_aff, c->P.tom_g_aff, sizeof c->PA.tom_g_aff);
    int32_t one = 1, ok = 0;
    HIPCHK(c, hipMemcpyAsync(c->d_flag, &one, 4, hipMemcpyHostToDevice, s));
    if (!share) launch_build_tom_table(s, d_g, ZK_AUDITOR_BITS, c->PA.tom_model, c->aud_tab_g, c->tab_scratch, c->d_flag);
    launch_build_tom_table(s, d_w, ZK_AUDITOR_BITS, c->PA.tom_model, c->PA.tom_tab_h, c->tab_scratch, c->d_flag);
    hipError_t e = hipMemcpyAsync(&ok, c->d_flag, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess || !ok) escrow_drop_auditor(c);
    HIPCHK(c, e);
    if (!ok) return ZK_E_POINT_NOT_IN_GROUP;
    memcpy(c->aud_w, aw, sizeof aw), memcpy(c->aud_xy, auditor_xy72, 72);
    c->auditor_set = true;
    return ZK_OK;
}

static zk_status escrow_refusal(zk_ctx* c, uint64_t B) {   // of every call that needs the auditor's key
    if (zk_status zs = sigma_refusal(c, B)) return zs;
    if (!c->auditor_set) {
        c->err = "no auditor key is set (zk_ctx_set_auditor)";
        return ZK_E_BUFFER;
    }
    return ZK_OK;
}
extern "C" uint64_t zk_escrow_tag_size(void) { return ZKT1_SIZE; }

// a * g for the secret at d_secret through one comb walk: S[0] = (a, 0), its affine bytes at d_ag; a8 (nullable) receives a mod q as words
void escrow_secret_point(zk_ctx* c, hipStream_t s, const uint8_t* d_secret, const TomList& S, uint32_t* a8, uint8_t* d_ag) {
    launch_escrow_stage_secret(s, d_secret, S, 0, a8);
    launch_tom_commit(s, c->P, S, 1, 1, 1);
    launch_tom_normalize(s, S, 1, 0, 1, 1);
    launch_affine_to_bytes(s, S.ax, S.ay, 1, 1, d_ag);
}
struct EscrowKeygen {
    uint8_t *secret, *ag;
    TomList S;
};
static size_t escrow_keygen_layout(EscrowKeygen& G, uint8_t* base) {
    SoaCarver k(base);
    G.secret = (uint8_t*)k.take(32), G.ag = (uint8_t*)k.take(72), G.S = k.list(1);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_escrow_keygen(zk_ctx* c, const uint8_t secret_be32[32], uint8_t auditor_xy72[72]) {
    if (!c || !secret_be32 || !auditor_xy72) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = sigma_refusal(c, 1)) return zs;
    EscrowKeygen G;
    if (zk_status zs = lay_out(c, B_et, [&](uint8_t* base) { return escrow_keygen_layout(G, base); })) return zs;
    if (zk_status zs = upload_or_wipe(c, {{G.secret, secret_be32, 32}})) return zs;   // the staged secret lies in a witness-flagged buffer
    escrow_secret_point(c, c->stream, G.secret, G.S, nullptr, G.ag);
    uint8_t ag[72];
    if (zk_status zs = download_or_wipe(c, {{G.ag, ag, 72}})) return zs;
    wipe_witness(c);   // one key per call: nothing of it stays behind
    bool ident = ag[71] == 1;
    for (int i = 0; i < 71; i++) ident = ident && ag[i] == 0;
    if (ident) {
        c->err = "the secret is 0 mod q";
        return ZK_E_ARG;
    }
    memcpy(auditor_xy72, ag, 72);
    return ZK_OK;
}

// ------------------------------------------------------------------ lanes
static void escrow_carve(SoaCarver& k, EscrowLane& X, uint32_t C) {
    X = EscrowLane{};
    sigma_carve_core(k, X, C, ESC_SLOTS, ESC_RNG_BLOCKS, ZKT1_MSG_BLOCKS);
    X.cw = (uint32_t*)k.take(4 * 18 * (size_t)C);
    X.rel = (uint32_t*)k.take(12 * (size_t)C);
}
typedef SigmaRun<EscrowLane> EscrowRun;
static EscrowKey escrow_key(const zk_ctx* c) {
    EscrowKey A;
    memcpy(A.w, c->aud_w, sizeof A.w);
    return A;
}

// ------------------------------------------------------------------ prover
static zk_status escrow_prove_device(zk_ctx* c, uint64_t B, const EscrowProveIo& io, const zk_rng& rng, uint64_t out_cap) {
    zk_status gate;
    if (sigma_prove_gate(c, B, rng, out_cap, ZKT1_SIZE, gate, escrow_refusal)) return gate;
    if (!words_aligned({io.com, io.key, io.blinder, io.out, io.status, rng.data})) return ZK_E_ARG;
    timing_begin(c);   // (behind every refusal: a call that runs nothing leaves the last call's record as it is)
    EscrowRun R;
    if (zk_status zs = sigma_plan(c, B, B_et, R, escrow_carve)) return zs;
    const bool timed = zk_timed(c, B);
    const EscrowKey A = escrow_key(c);
    return sigma_run_chunks(c, R, true, [&](EscrowLane& K, hipStream_t s, uint32_t cnt, uint64_t first) {
        sigma_chunk_rng(c, timed, s, K.rng, K.rng_fill, rng, first, cnt, ESC_RNG_BLOCKS);
        {
            MaybeScope t(timed, c, "escrow_front", s);
            launch_escrow_front(s, K, cnt, first, io);
        }
        {
            MaybeScope t(timed, c, "tom_commit", s);
            launch_tom_commit(s, c->P, K.L, 4 * cnt, 1, 1);                          // E1, T1, T2 and the claimed opening on (g, h)
            launch_tom_commit(s, c->PA, tom_list_from(K.L, 4 * cnt), 2 * cnt, 1, 1);   // E2, T3 on (g, A)
        }
        {
            MaybeScope t(timed, c, "tom_normalize", s);
            launch_tom_normalize(s, K.L, ESC_SLOTS * cnt, 0, 1, 1);
        }
        {
            MaybeScope t(timed, c, "hash", s);
            launch_escrow_opening_msg(s, K, A, cnt);
            launch_sigma_hash(s, K, cnt, ZKT1_MSG_BLOCKS);
        }
        {
            MaybeScope t(timed, c, "escrow_respond", s);
            launch_escrow_respond(s, K, cnt, first, io);
        }
    });
}
extern "C" zk_status zk_escrow_prove_batch_device(zk_ctx* c, uint64_t B, const void* d_key, const void* d_com, const void* d_blinder, const zk_rng* rng, void* d_out,
                                                  uint64_t out_cap, void* d_status) {
    if (!c || !rng || (B && (!d_key || !d_com || !d_blinder || !rng->data || !d_out || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const zk_status zs = escrow_prove_device(c, B, {(const uint8_t*)d_key, (const uint8_t*)d_com, (const uint8_t*)d_blinder, (uint8_t*)d_out, (int32_t*)d_status}, *rng, out_cap);
    if (zs && c->params_set && !c->stream_busy) wipe_witness(c);
    return zs;
}
// zk_escrow_prove_batch_device's pipeline for api_accountable.hip (accountable.h)
zk_status zkc_escrow_prove(zk_ctx* c, uint64_t B, const uint8_t* key, const uint8_t* com, const uint8_t* blinder, const zk_rng& rng, uint8_t* out, int32_t* status) {
    return escrow_prove_device(c, B, {key, com, blinder, out, status}, rng, B * ZKT1_SIZE);
}
// Host pointers: key, blinder and seeds through the context's witness-flagged input buffer, the tags through its output staging buffer.
struct EscrowProveIn {
    uint8_t *key, *com, *blinder, *rng;
    int32_t* st;
};
static size_t escrow_prove_in_layout(EscrowProveIn& I, uint8_t* base, size_t B, size_t rng_bytes) {
    Carver k(base);
    I.key = (uint8_t*)k.take(32 * B), I.com = (uint8_t*)k.take(72 * B), I.blinder = (uint8_t*)k.take(32 * B);
    I.rng = (uint8_t*)k.take(rng_bytes ? rng_bytes : 32), I.st = (int32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_escrow_prove_batch(zk_ctx* c, uint64_t B, const uint8_t* key, const uint8_t* com, const uint8_t* blinder, const zk_rng* rng, uint8_t* out,
                                           uint64_t out_cap, int32_t* status) {
    if (!c || !rng || (B && (!key || !com || !blinder || !rng->data || !out || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    zk_status gate;
    if (sigma_prove_gate(c, B, *rng, out_cap, ZKT1_SIZE, gate, escrow_refusal)) return gate;
    EscrowProveIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return escrow_prove_in_layout(I, base, B, rng_bytes(rng, B)); })) return zs;
    if (zk_status zs = reserve(c, B_io, B * ZKT1_SIZE)) return zs;
    uint8_t* const d_out = (uint8_t*)c->buf[B_io].p;
    // from the first upload on, key, blinder and seeds lie in the input buffer: every failure below zeroes them
    if (zk_status zs = upload_or_wipe(c, {{I.key, key, 32 * B}, {I.com, com, 72 * B}, {I.blinder, blinder, 32 * B}, {I.rng, rng->data, rng_bytes(rng, B)}})) return zs;
    if (zk_status zs = escrow_prove_device(c, B, {I.key, I.com, I.blinder, d_out, I.st}, zk_rng{rng->mode, I.rng, rng->stride_blocks}, B * ZKT1_SIZE)) {
        wipe_witness(c);
        return zs;
    }
    return download_or_wipe(c, {{d_out, out, B * ZKT1_SIZE}, {I.st, status, 4 * B}});
}

// ------------------------------------------------------------------ verifier
static zk_status escrow_verify_device(zk_ctx* c, uint64_t B, const EscrowVerifyIo& io) {
    if (zk_status zs = escrow_refusal(c, B)) return zs;
    if (B == 0) return ZK_OK;
    if (!words_aligned({io.com, io.tags, io.status})) return ZK_E_ARG;
    timing_begin(c);
    EscrowRun R;
    if (zk_status zs = sigma_plan(c, B, B_et, R, escrow_carve)) return zs;
    const bool timed = zk_timed(c, B);
    const EscrowKey A = escrow_key(c);
    return sigma_run_chunks(c, R, false, [&](const EscrowLane& K, hipStream_t s, uint32_t cnt, uint64_t first) {
        {
            MaybeScope t(timed, c, "escrow_parse", s);
            launch_escrow_parse(s, K, A, cnt, first, io);
            launch_sigma_hash(s, K, cnt, ZKT1_MSG_BLOCKS);
        }
        {
            MaybeScope t(timed, c, "tom_commit", s);
            launch_tom_commit(s, c->P, K.L, 2 * cnt, 1, 1);                      // t_x g + t_r h, t_rho g
            launch_tom_commit(s, c->PA, tom_list_from(K.L, 2 * cnt), cnt, 1, 1);   // t_x g + t_rho A
        }
        {
            MaybeScope t(timed, c, "escrow_ladder", s);
            launch_escrow_relations(s, K, cnt, first, io);
            launch_escrow_verdict(s, K, cnt, first, io);
        }
    });
}
extern "C" zk_status zk_escrow_verify_batch_device(zk_ctx* c, uint64_t B, const void* d_com, const void* d_tags, void* d_ok, void* d_status) {
    if (!c || (B && (!d_com || !d_tags || !d_ok || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return escrow_verify_device(c, B, {(const uint8_t*)d_com, (const uint8_t*)d_tags, (uint8_t*)d_ok, (int32_t*)d_status});
}
// zk_escrow_verify_batch_device's pipeline for api_accountable.hip (accountable.h)
zk_status zkc_escrow_verify(zk_ctx* c, uint64_t B, const uint8_t* com, const uint8_t* tags, uint8_t* ok, int32_t* status) {
    return escrow_verify_device(c, B, {com, tags, ok, status});
}
struct EscrowVerifyIn {   // no witness is staged: a failing copy returns as it is
    uint8_t *com, *ok;
    int32_t* st;
};
static size_t escrow_verify_in_layout(EscrowVerifyIn& I, uint8_t* base, size_t B) {
    Carver k(base);
    I.com = (uint8_t*)k.take(72 * B), I.ok = (uint8_t*)k.take(B), I.st = (int32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_escrow_verify_batch(zk_ctx* c, uint64_t B, const uint8_t* com, const uint8_t* tags, uint8_t* ok, int32_t* status) {
    if (!c || (B && (!com || !tags || !ok || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = escrow_refusal(c, B)) return zs;
    if (B == 0) return ZK_OK;
    EscrowVerifyIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return escrow_verify_in_layout(I, base, B); })) return zs;
    if (zk_status zs = reserve(c, B_io, B * ZKT1_SIZE)) return zs;
    uint8_t* const d_tags = (uint8_t*)c->buf[B_io].p;
    if (zk_status zs = upload_rows(c, {{I.com, com, 72 * B}, {d_tags, tags, B * ZKT1_SIZE}})) return zs;
    if (zk_status zs = escrow_verify_device(c, B, {I.com, d_tags, I.ok, I.st})) return zs;
    return download_rows(c, {{I.ok, ok, B}, {I.st, status, 4 * B}});
}

// ------------------------------------------------------------------ opening
size_t escrow_open_carve(EscrowOpen& O, uint8_t* base, uint64_t B, uint32_t slab) {
    SoaCarver k(base);
    O = EscrowOpen{};
    O.S = k.list(1);
    O.a8 = (uint32_t*)k.take(32);
    O.ag = (uint8_t*)k.take(72);
    O.T = k.list(B);
    O.st = (int32_t*)k.take(4 * B);
    O.Rg = k.list(slab);
    return k.off + ZK_LAYOUT_TAIL;
}
// The auditor's side.  1. a g against the context's key, once; 2. one lane per tag: 4 (E2 - a E1), normalised; 3. per slab of the active ring's real keys:
// 4 y_i g through the comb, normalised; 4. the match.  The ring's point table is rebuilt by every call.
static zk_status escrow_open_device(zk_ctx* c, uint64_t B, const uint8_t* d_secret, const uint8_t* d_tags, uint32_t* d_index, int32_t* d_status) {
    if (zk_status zs = escrow_refusal(c, B)) return zs;
    if (!c->ring->N) {
        c->err = "no ring is active";
        return ZK_E_BUFFER;
    }
    if (B == 0) return ZK_OK;
    if (!words_aligned({d_secret, d_tags, d_index, d_status})) return ZK_E_ARG;
    timing_begin(c);
    const uint64_t nkeys = c->ring->nkeys;
    const uint32_t slab = (uint32_t)std::min<uint64_t>(nkeys, ESC_RING_SLAB);
    EscrowOpen O;
    if (zk_status zs = lay_out(c, B_et, [&](uint8_t* base) { return escrow_open_carve(O, base, B, slab); })) return zs;
    const bool timed = zk_timed(c, B);
    hipStream_t s0 = c->stream;
    {
        MaybeScope t(timed, c, "escrow_open", s0);
        escrow_secret_point(c, s0, d_secret, O.S, O.a8, O.ag);
    }
    uint8_t ag[72];
    if (zk_status zs = download_or_wipe(c, {{O.ag, ag, 72}})) return zs;   // (a blocking copy: the staged secret is in place for every lane behind it)
    if (memcmp(ag, c->aud_xy, 72) != 0) {
        wipe_witness(c);
        timing_end(c);   // the key check ran: the call's record is its "escrow_open" family alone
        c->err = "the secret does not belong to the context's auditor key";
        return ZK_E_OPENING;
    }
    const uint32_t C = (uint32_t)std::min<uint64_t>(c->chunk, B);
    const std::vector<ChunkPlan> plan = make_chunk_plan(B, C, 1, false);
    const uint32_t NL = (uint32_t)std::min<size_t>(std::min<uint32_t>(c->lanes, ZK_MAX_LANES), plan.size());
    for (uint64_t k = 0; k < plan.size(); k++) {
        hipStream_t s = c->pl[k % NL].stream;
        MaybeScope t(timed, c, "escrow_ladder", s);
        launch_escrow_open_points(s, O, plan[k].cnt, plan[k].first, d_tags, d_index, d_status);
    }
    hipError_t e = drain_lanes(c, NL);
    if (e == hipSuccess) {
        {
            MaybeScope t(timed, c, "tom_normalize", s0);
            launch_tom_normalize(s0, O.T, (uint32_t)B, 0, 1, 1);
        }
        const Soa ring = {c->ring->ring_mem, (uint32_t)c->ring->N};
        for (uint64_t i0 = 0; i0 < nkeys; i0 += slab) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(slab, nkeys - i0);
            {
                MaybeScope t(timed, c, "escrow_ring_points", s0);
                launch_escrow_ring_scalars(s0, ring, i0, n, O.Rg);
                launch_tom_commit(s0, c->P, O.Rg, n, 1, 1);
                launch_escrow_times4(s0, O.Rg, n);
                launch_tom_normalize(s0, O.Rg, n, 0, 1, 1);
            }
            {
                MaybeScope t(timed, c, "escrow_match", s0);
                launch_escrow_match(s0, O, B, i0, n, d_index);
            }
        }
        e = hipStreamSynchronize(s0);
    }
    if (e != hipSuccess) wipe_witness(c);   // a failed call leaves neither a nor a E1 behind
    HIPCHK(c, e);
    HIPCHK(c, hipGetLastError());
    timing_end(c);
    return ZK_OK;
}
extern "C" zk_status zk_escrow_open_batch_device(zk_ctx* c, uint64_t B, const void* d_secret, const void* d_tags, void* d_index, void* d_status) {
    if (!c || !d_secret || (B && (!d_tags || !d_index || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const zk_status zs = escrow_open_device(c, B, (const uint8_t*)d_secret, (const uint8_t*)d_tags, (uint32_t*)d_index, (int32_t*)d_status);
    if (zs && zs != ZK_E_OPENING && c->params_set && !c->stream_busy) wipe_witness(c);
    return zs;
}
struct EscrowOpenIn {
    uint8_t* secret;
    uint32_t* index;
    int32_t* st;
};
static size_t escrow_open_in_layout(EscrowOpenIn& I, uint8_t* base, size_t B) {
    Carver k(base);
    I.secret = (uint8_t*)k.take(32), I.index = (uint32_t*)k.take(4 * B), I.st = (int32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_escrow_open_batch(zk_ctx* c, uint64_t B, const uint8_t secret_be32[32], const uint8_t* tags, uint32_t* index_u32, int32_t* status) {
    if (!c || !secret_be32 || (B && (!tags || !index_u32 || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = escrow_refusal(c, B)) return zs;
    if (!c->ring->N) {
        c->err = "no ring is active";
        return ZK_E_BUFFER;
    }
    if (B == 0) return ZK_OK;
    EscrowOpenIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return escrow_open_in_layout(I, base, B); })) return zs;
    if (zk_status zs = reserve(c, B_io, B * ZKT1_SIZE)) return zs;
    uint8_t* const d_tags = (uint8_t*)c->buf[B_io].p;
    // from the first upload on the secret lies in the input buffer: every failure below zeroes it
    if (zk_status zs = upload_or_wipe(c, {{I.secret, secret_be32, 32}, {d_tags, tags, B * ZKT1_SIZE}})) return zs;
    if (zk_status zs = escrow_open_device(c, B, I.secret, d_tags, I.index, I.st)) {
        wipe_witness(c);
        return zs;
    }
    return download_or_wipe(c, {{I.index, index_u32, 4 * B}, {I.st, status, 4 * B}});
}

// ------------------------------------------------------------------ the resident point index and the opening against any resident ring
// (escrow_index.h; kernels: k_escrow_index.hip).  A ring's points 4 y_i g and the table of key indices over them are public data of (g, the ring): not
// witness-flagged, kept from one call to the next, patched by zk_ctx_update_ring's in-place path, dropped by every rebuild of the ring and by
// zk_ctx_set_params.  A ring of nkeys >= 2 keys has esc_index_cap(nkeys) == N entries.
static_assert(ESC_INDEX_MAX_RINGS >= ZK_MAX_RINGS, "one descriptor per resident ring");
#define ESC_INDEX_SLAB (1u << 16)   // keys whose points are computed at a time: 252 bytes of temporary memory each
void escrow_index_drop(Ring& R) {
    hipFree(R.esc_pts), hipFree(R.esc_slots);
    R.esc_pts = nullptr, R.esc_slots = nullptr;
}
EscIndexRing escrow_index_desc(const Ring& R, uint64_t nkeys) {
    EscIndexRing D{};
    D.id = R.id, D.nkeys = (uint32_t)nkeys, D.mask = 2 * (uint32_t)R.N - 1, D.pts = R.esc_pts, D.slots = R.esc_slots;
    return D;
}
static size_t escrow_index_tmp_layout(TomList& L, uint8_t* base, uint32_t slab) {
    SoaCarver k(base);
    L = k.list(slab);
    return k.off + ZK_LAYOUT_TAIL;
}
static hipError_t escrow_index_tmp(DevBuf& d, TomList& L, uint32_t slab) {
    const hipError_t e = hipMalloc(&d.p, escrow_index_tmp_layout(L, nullptr, slab));
    if (e == hipSuccess) escrow_index_tmp_layout(L, d.as<uint8_t>(), slab);
    return e;
}
static void escrow_index_refill(hipStream_t s, const Ring& R, uint64_t nkeys) {   // every slot empty, then one lane per key
    (void)hipMemsetAsync(R.esc_slots, 0xff, 8 * R.N, s);
    launch_escrow_index_insert(s, escrow_index_desc(R, nkeys));
}
// slots 0 .. n - 1 of L hold the openings (y, 0): their points 4 y g, normalised into L.ax, L.ay
static void escrow_index_points(zk_ctx* c, hipStream_t s, const TomList& L, uint32_t n) {
    launch_tom_commit(s, c->P, L, n, 1, 1);
    launch_escrow_times4(s, L, n);
    launch_tom_normalize(s, L, n, 0, 1, 1);
}
zk_status escrow_index_build(zk_ctx* c, Ring& R) {
    hipStream_t s = c->stream;
    const uint32_t slab = (uint32_t)std::min<uint64_t>(R.nkeys, ESC_INDEX_SLAB), cap = (uint32_t)R.N;
    DevBuf tmp;
    TomList L;
    if (hipMalloc(&R.esc_pts, 72 * R.N) != hipSuccess || hipMalloc(&R.esc_slots, 8 * R.N) != hipSuccess || escrow_index_tmp(tmp, L, slab) != hipSuccess) {
        (void)hipGetLastError();
        escrow_index_drop(R);
        c->err = "the point index of a resident ring could not be allocated";
        return ZK_E_DEVICE;
    }
    const Soa ring = {R.ring_mem, cap};
    for (uint64_t i0 = 0; i0 < R.nkeys; i0 += slab) {   // the normaliser writes each slab where it stays
        const uint32_t n = (uint32_t)std::min<uint64_t>(slab, R.nkeys - i0);
        TomList V = L;
        V.ax = Soa{R.esc_pts + i0, cap}, V.ay = Soa{R.esc_pts + 9 * (size_t)cap + i0, cap};
        launch_escrow_ring_scalars(s, ring, i0, n, V);
        escrow_index_points(c, s, V, n);
    }
    escrow_index_refill(s, R, R.nkeys);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) escrow_index_drop(R);
    HIPCHK(c, e);
    return ZK_OK;
}
hipError_t escrow_index_patch(zk_ctx* c, Ring& R, const uint32_t* d_ent, uint32_t real, uint64_t nkeys) {
    hipStream_t s = c->stream;
    DevBuf tmp;
    TomList L;
    const uint32_t slab = std::min<uint32_t>(real, ESC_INDEX_SLAB);
    if (real && escrow_index_tmp(tmp, L, slab) != hipSuccess) {
        (void)hipGetLastError();
        escrow_index_drop(R);
        return hipSuccess;
    }
    const Soa ring = {R.ring_mem, (uint32_t)R.N};
    for (uint32_t j0 = 0; j0 < real; j0 += slab) {
        const uint32_t n = std::min<uint32_t>(slab, real - j0);
        launch_escrow_index_gather(s, ring, d_ent + j0, n, L);
        escrow_index_points(c, s, L, n);
        launch_escrow_index_scatter(s, L, d_ent + j0, n, R.esc_pts, (uint32_t)R.N);
    }
    escrow_index_refill(s, R, nkeys);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : hipStreamSynchronize(s);   // (the temporary list goes with this scope)
}

// The auditor's side over the resident rings.  1. the index of every resident ring that lacks one; 2. a g against the context's key, once; 3. one lane per
// tag: 4 (E2 - a E1), normalised (zk_escrow_open_batch's kernels); 4. one lane per tag: the lookup in the ring its id names.  The active ring is not read.
static zk_status rings_escrow_open_device(zk_ctx* c, uint64_t B, const uint8_t* d_secret, const uint8_t* d_tags, const uint32_t* d_ids, uint32_t* d_ring_out, uint32_t* d_index,
                                          int32_t* d_status) {
    if (zk_status zs = escrow_refusal(c, B)) return zs;
    if (B == 0) return ZK_OK;
    if (!words_aligned({d_secret, d_tags, d_ids, d_ring_out, d_index, d_status})) return ZK_E_ARG;
    timing_begin(c);
    const bool timed = zk_timed(c, B);
    hipStream_t s0 = c->stream;
    Ring* rs[ZK_MAX_RINGS];
    uint32_t nr = 0;
    for (auto& R : c->rings)
        if (R.live && R.N) rs[nr++] = &R;
    std::sort(rs, rs + nr, [](const Ring* a, const Ring* b) { return a->id < b->id; });
    EscIndexSet S{};
    for (uint32_t k = 0; k < nr; k++) {
        if (!rs[k]->esc_pts) {
            MaybeScope t(timed, c, "escrow_index_build", s0);
            if (zk_status zs = escrow_index_build(c, *rs[k])) return zs;
        }
        S.r[S.count++] = escrow_index_desc(*rs[k], rs[k]->nkeys);
    }
    EscrowOpen O;
    if (zk_status zs = lay_out(c, B_et, [&](uint8_t* base) { return escrow_open_carve(O, base, B, 0); })) return zs;
    {
        MaybeScope t(timed, c, "escrow_open", s0);
        escrow_secret_point(c, s0, d_secret, O.S, O.a8, O.ag);
    }
    uint8_t ag[72];
    if (zk_status zs = download_or_wipe(c, {{O.ag, ag, 72}})) return zs;   // (a blocking copy: the staged secret is in place for every lane behind it)
    if (memcmp(ag, c->aud_xy, 72) != 0) {
        wipe_witness(c);
        timing_end(c);
        c->err = "the secret does not belong to the context's auditor key";
        return ZK_E_OPENING;
    }
    const uint32_t C = (uint32_t)std::min<uint64_t>(c->chunk, B);
    const std::vector<ChunkPlan> plan = make_chunk_plan(B, C, 1, false);
    const uint32_t NL = (uint32_t)std::min<size_t>(std::min<uint32_t>(c->lanes, ZK_MAX_LANES), plan.size());
    for (uint64_t k = 0; k < plan.size(); k++) {
        hipStream_t s = c->pl[k % NL].stream;
        MaybeScope t(timed, c, "escrow_ladder", s);
        launch_escrow_open_points(s, O, plan[k].cnt, plan[k].first, d_tags, d_index, d_status);
    }
    hipError_t e = drain_lanes(c, NL);
    if (e == hipSuccess) {
        {
            MaybeScope t(timed, c, "tom_normalize", s0);
            launch_tom_normalize(s0, O.T, (uint32_t)B, 0, 1, 1);
        }
        {
            MaybeScope t(timed, c, "escrow_lookup", s0);
            launch_escrow_index_lookup(s0, S, O, B, d_ids, d_ring_out, d_index, d_status);
        }
        e = hipStreamSynchronize(s0);
    }
    if (e != hipSuccess) wipe_witness(c);   // a failed call leaves neither a nor a E1 behind
    HIPCHK(c, e);
    HIPCHK(c, hipGetLastError());
    timing_end(c);
    return ZK_OK;
}
extern "C" zk_status zk_rings_escrow_open_batch_device(zk_ctx* c, uint64_t B, const void* d_secret, const void* d_tags, const void* d_ring_ids, void* d_ring_out, void* d_index,
                                                       void* d_status) {
    if (!c || !d_secret || (B && (!d_tags || !d_ring_ids || !d_ring_out || !d_index || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const zk_status zs = rings_escrow_open_device(c, B, (const uint8_t*)d_secret, (const uint8_t*)d_tags, (const uint32_t*)d_ring_ids, (uint32_t*)d_ring_out, (uint32_t*)d_index,
                                                  (int32_t*)d_status);
    if (zs && zs != ZK_E_OPENING && c->params_set && !c->stream_busy) wipe_witness(c);
    return zs;
}
zk_status zkc_rings_escrow_open(zk_ctx* c, uint64_t B, const uint8_t* secret, const uint8_t* tags, const uint32_t* ids, uint32_t* ring_out, uint32_t* index, int32_t* status) {
    return rings_escrow_open_device(c, B, secret, tags, ids, ring_out, index, status);
}
struct RingsEscrowOpenIn {
    uint8_t* secret;
    uint32_t *ids, *ring, *index;
    int32_t* st;
};
static size_t rings_escrow_open_in_layout(RingsEscrowOpenIn& I, uint8_t* base, size_t B) {
    Carver k(base);
    I.secret = (uint8_t*)k.take(32), I.ids = (uint32_t*)k.take(4 * B), I.ring = (uint32_t*)k.take(4 * B), I.index = (uint32_t*)k.take(4 * B), I.st = (int32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_rings_escrow_open_batch(zk_ctx* c, uint64_t B, const uint8_t secret_be32[32], const uint8_t* tags, const uint32_t* ring_ids, uint32_t* ring_out_u32,
                                                uint32_t* index_u32, int32_t* status) {
    if (!c || !secret_be32 || (B && (!tags || !ring_ids || !ring_out_u32 || !index_u32 || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = escrow_refusal(c, B)) return zs;
    if (B == 0) return ZK_OK;
    RingsEscrowOpenIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return rings_escrow_open_in_layout(I, base, B); })) return zs;
    if (zk_status zs = reserve(c, B_io, B * ZKT1_SIZE)) return zs;
    uint8_t* const d_tags = (uint8_t*)c->buf[B_io].p;
    // from the first upload on the secret lies in the input buffer: every failure below zeroes it
    if (zk_status zs = upload_or_wipe(c, {{I.secret, secret_be32, 32}, {I.ids, ring_ids, 4 * B}, {d_tags, tags, B * ZKT1_SIZE}})) return zs;
    if (zk_status zs = rings_escrow_open_device(c, B, I.secret, d_tags, I.ids, I.ring, I.index, I.st)) {
        wipe_witness(c);
        return zs;
    }
    return download_or_wipe(c, {{I.ring, ring_out_u32, 4 * B}, {I.index, index_u32, 4 * B}, {I.st, status, 4 * B}});
}
