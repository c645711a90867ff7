// zk_link_prove_batch / zk_link_verify_batch / zk_proof_key_commitments (include/zkattest.h): proveEquality / verifyEquality (equality.ts:60-116) for two
// Tom-256 commitments the caller brings -- "these two commitments open to the same key" -- and the extractor that hands a verifier the keyXcom of a ZKA1 proof.
// Host-side pipeline; the kernels of its own are in k_link.hip, the commitments are k_tom.hip's pair form, the challenge hash k_hash.hip's message path.
// No ring takes part.  The chunks run on the context's lanes (their streams are the prover lanes'), every lane's arena carved from one witness-flagged buffer.
#include "ctx.h"
#include "sigma.h"
#include "link.h"
#include "rering_plan.h"   // rr_head: the header and slot rules of zk_proof_rering_batch

static void link_carve(SoaCarver& k, LinkLane& X, uint32_t C) {
    X = LinkLane{};
    sigma_carve_core(k, X, C, LINK_SLOTS, LINK_RNG_BLOCKS, ZKL1_MSG_BLOCKS);
    X.cw = (uint32_t*)k.take(4 * 36 * (size_t)C);
}
extern "C" uint64_t zk_link_proof_size(void) { return ZKL1_SIZE; }
typedef SigmaRun<LinkLane> LinkRun;

// ------------------------------------------------------------------ prover
static zk_status link_prove_device(zk_ctx* c, uint64_t B, const LinkProveIo& io, const zk_rng& rng, uint64_t out_cap) {
    zk_status gate;
    if (sigma_prove_gate(c, B, rng, out_cap, ZKL1_SIZE, gate)) return gate;
    if (!words_aligned({io.com1, io.com2, io.key, io.blinder1, io.blinder2, io.out, io.status, rng.data})) return ZK_E_ARG;
    timing_begin(c);   // (behind every refusal: a call that runs nothing leaves the last call's record as it is)
    LinkRun R;
    if (zk_status zs = sigma_plan(c, B, B_lk, R, link_carve)) return zs;
    const bool timed = zk_timed(c, B);
    return sigma_run_chunks(c, R, true, [&](LinkLane& K, hipStream_t s, uint32_t cnt, uint64_t first) {
        sigma_chunk_rng(c, timed, s, K.rng, K.rng_fill, rng, first, cnt, LINK_RNG_BLOCKS);
        {
            MaybeScope t(timed, c, "tom_commit", s);
            launch_link_front(s, K, cnt, first, io);
            launch_tom_commit_pair_slots(s, c->P, K.L, 2 * cnt);   // (k g + s1 h, k g + s2 h), then (x g + r1 h, x g + r2 h)
        }
        {
            MaybeScope t(timed, c, "tom_normalize", s);
            launch_tom_normalize(s, K.L, LINK_SLOTS * cnt, 0, 1, 1);
        }
        {
            MaybeScope t(timed, c, "hash", s);
            launch_link_opening_msg(s, K, cnt);
            launch_sigma_hash(s, K, cnt, ZKL1_MSG_BLOCKS);
        }
        {
            MaybeScope t(timed, c, "link_respond", s);
            launch_link_respond(s, K, cnt, first, io);
        }
    });
}
extern "C" zk_status zk_link_prove_batch_device(zk_ctx* c, uint64_t B, const void* d_key, const void* d_com1, const void* d_blinder1, const void* d_com2, const void* d_blinder2,
                                                const zk_rng* rng, void* d_out, uint64_t out_cap, void* d_status) {
    if (!c || !rng || (B && (!d_key || !d_com1 || !d_blinder1 || !d_com2 || !d_blinder2 || !rng->data || !d_out || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const zk_status zs = link_prove_device(c, B, {(const uint8_t*)d_key, (const uint8_t*)d_com1, (const uint8_t*)d_blinder1, (const uint8_t*)d_com2, (const uint8_t*)d_blinder2,
                                                  (uint8_t*)d_out, (int32_t*)d_status}, *rng, out_cap);
    if (zs && c->params_set && !c->stream_busy) wipe_witness(c);
    return zs;
}
// Host pointers: keys, blinders and seeds through the context's witness-flagged input buffer, the proofs through its output staging buffer.
struct LinkProveIn {
    uint8_t *key, *com1, *blinder1, *com2, *blinder2, *rng;
    int32_t* st;
};
static size_t link_prove_in_layout(LinkProveIn& I, uint8_t* base, size_t B, size_t rng_bytes) {
    Carver k(base);
    I.key = (uint8_t*)k.take(32 * B), I.com1 = (uint8_t*)k.take(72 * B), I.blinder1 = (uint8_t*)k.take(32 * B), I.com2 = (uint8_t*)k.take(72 * B);
    I.blinder2 = (uint8_t*)k.take(32 * B), I.rng = (uint8_t*)k.take(rng_bytes ? rng_bytes : 32), I.st = (int32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_link_prove_batch(zk_ctx* c, uint64_t B, const uint8_t* key, const uint8_t* com1, const uint8_t* blinder1, const uint8_t* com2, const uint8_t* blinder2,
                                         const zk_rng* rng, uint8_t* out, uint64_t out_cap, int32_t* status) {
    if (!c || !rng || (B && (!key || !com1 || !blinder1 || !com2 || !blinder2 || !rng->data || !out || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    zk_status gate;
    if (sigma_prove_gate(c, B, *rng, out_cap, ZKL1_SIZE, gate)) return gate;
    LinkProveIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return link_prove_in_layout(I, base, B, rng_bytes(rng, B)); })) return zs;
    if (zk_status zs = reserve(c, B_io, B * ZKL1_SIZE)) return zs;
    uint8_t* const d_out = (uint8_t*)c->buf[B_io].p;
    // from the first upload on, keys, blinders and seeds lie in the input buffer: every failure below zeroes them
    if (zk_status zs = upload_or_wipe(c, {{I.key, key, 32 * B}, {I.com1, com1, 72 * B}, {I.blinder1, blinder1, 32 * B}, {I.com2, com2, 72 * B}, {I.blinder2, blinder2, 32 * B},
                                          {I.rng, rng->data, rng_bytes(rng, B)}}))
        return zs;
    if (zk_status zs = link_prove_device(c, B, {I.key, I.com1, I.blinder1, I.com2, I.blinder2, d_out, I.st}, zk_rng{rng->mode, I.rng, rng->stride_blocks}, B * ZKL1_SIZE)) {
        wipe_witness(c);
        return zs;
    }
    return download_or_wipe(c, {{d_out, out, B * ZKL1_SIZE}, {I.st, status, 4 * B}});
}

// ------------------------------------------------------------------ verifier
static zk_status link_verify_device(zk_ctx* c, uint64_t B, const LinkVerifyIo& io) {
    if (zk_status zs = sigma_refusal(c, B)) return zs;
    if (B == 0) return ZK_OK;
    if (!words_aligned({io.com1, io.com2, io.proofs, io.status})) return ZK_E_ARG;
    timing_begin(c);
    LinkRun R;
    if (zk_status zs = sigma_plan(c, B, B_lk, R, link_carve)) return zs;
    const bool timed = zk_timed(c, B);
    return sigma_run_chunks(c, R, false, [&](const LinkLane& K, hipStream_t s, uint32_t cnt, uint64_t first) {
        {
            MaybeScope t(timed, c, "link_parse", s);
            launch_link_parse(s, K, cnt, first, io);
            launch_sigma_hash(s, K, cnt, ZKL1_MSG_BLOCKS);
        }
        {
            MaybeScope t(timed, c, "tom_commit", s);
            launch_tom_commit_pair_slots(s, c->P, K.L, cnt);   // t_x g + t_r1 h, t_x g + t_r2 h
        }
        {
            MaybeScope t(timed, c, "link_ladder", s);
            launch_link_ladder(s, K, cnt, first, io);
        }
    });
}
extern "C" zk_status zk_link_verify_batch_device(zk_ctx* c, uint64_t B, const void* d_com1, const void* d_com2, const void* d_proofs, void* d_ok, void* d_status) {
    if (!c || (B && (!d_com1 || !d_com2 || !d_proofs || !d_ok || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return link_verify_device(c, B, {(const uint8_t*)d_com1, (const uint8_t*)d_com2, (const uint8_t*)d_proofs, (uint8_t*)d_ok, (int32_t*)d_status});
}
struct LinkVerifyIn {   // no witness is staged: a failing copy returns as it is
    uint8_t *com1, *com2, *ok;
    int32_t* st;
};
static size_t link_verify_in_layout(LinkVerifyIn& I, uint8_t* base, size_t B) {
    Carver k(base);
    I.com1 = (uint8_t*)k.take(72 * B), I.com2 = (uint8_t*)k.take(72 * B), I.ok = (uint8_t*)k.take(B), I.st = (int32_t*)k.take(4 * B);
    return k.off + ZK_LAYOUT_TAIL;
}
extern "C" zk_status zk_link_verify_batch(zk_ctx* c, uint64_t B, const uint8_t* com1, const uint8_t* com2, const uint8_t* proofs, uint8_t* ok, int32_t* status) {
    if (!c || (B && (!com1 || !com2 || !proofs || !ok || !status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (zk_status zs = sigma_refusal(c, B)) return zs;
    if (B == 0) return ZK_OK;
    LinkVerifyIn I;
    if (zk_status zs = lay_out(c, B_in, [&](uint8_t* base) { return link_verify_in_layout(I, base, B); })) return zs;
    if (zk_status zs = reserve(c, B_io, B * ZKL1_SIZE)) return zs;
    uint8_t* const d_proofs = (uint8_t*)c->buf[B_io].p;
    if (zk_status zs = upload_rows(c, {{I.com1, com1, 72 * B}, {I.com2, com2, 72 * B}, {d_proofs, proofs, B * ZKL1_SIZE}})) return zs;
    if (zk_status zs = link_verify_device(c, B, {I.com1, I.com2, d_proofs, I.ok, I.st})) return zs;
    return download_rows(c, {{I.ok, ok, B}, {I.st, status, 4 * B}});
}

// ------------------------------------------------------------------ keyXcom of ZKA1 / ZK1P proofs
static zk_status key_commitments_device(zk_ctx* c, uint64_t B, const uint8_t* d_proofs, const uint64_t* d_off, uint8_t* d_com, int32_t* d_status) {
    if (zk_status zs = sigma_refusal(c, B)) return zs;
    if (B == 0) return ZK_OK;
    if (!words_aligned({d_proofs, d_off, d_com, d_status}) || ((uintptr_t)d_off & 7)) return ZK_E_ARG;
    launch_link_keycoms(c->stream, B, d_proofs, d_off, wire_make(c->wire != 0), d_com, d_status);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    return ZK_OK;
}
extern "C" zk_status zk_proof_key_commitments_device(zk_ctx* c, uint64_t B, const void* d_proofs, const void* d_proof_off, void* d_com, void* d_status) {
    if (!c || (B && (!d_proofs || !d_proof_off || !d_com || !d_status))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return key_commitments_device(c, B, (const uint8_t*)d_proofs, (const uint64_t*)d_proof_off, (uint8_t*)d_com, (int32_t*)d_status);
}
// Host pointers: nothing but the header and the two coordinates of a slot is looked at, so the work stays on the host (rr_head is the device's rule, compiled here)
extern "C" zk_status zk_proof_key_commitments(zk_ctx* c, uint64_t B, const uint8_t* proofs, const uint64_t* proof_off, uint8_t* com, int32_t* status) {
    if (!c || (B && (!proofs || !proof_off || !com || !status))) return ZK_E_ARG;
    if (zk_status zs = sigma_refusal(c, B)) return zs;
    const Wire w = wire_make(c->wire != 0);
    for (uint64_t b = 0; b < B; b++) {
        uint8_t* o = com + 72 * b;
        memset(o, 0, 72);
        const RrHead h = rr_head(proofs, proof_off[b], proof_off[b + 1], w);
        status[b] = h.ok ? ZK_OK : ZK_E_BAD_ENCODING;
        if (!h.ok) continue;
        const uint8_t* kx = proofs + proof_off[b] + ZK_HDR + 128;
        memcpy(o + 36 - w.tc, kx, w.tc), memcpy(o + 72 - w.tc, kx + w.tc, w.tc);
    }
    return ZK_OK;
}
