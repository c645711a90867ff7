// Host side of the key recovery (include/zkattest.h: zk_recover_batch; kernels: k_recover.hip and the screen's lookup, k_screen.hip).
//
// A call runs in chunks of ZK_RECOVER_CHUNK witnesses on the context's main stream, like the screen.  Per chunk: two passes of lift -> points (x = r, then
// x = r + n, whose workgroups leave at once outside adversarial inputs; nothing is read back to decide), the screen's lookup over the candidate buffer as
// up to 4 x count pseudo-witnesses -- once for the active ring, or once per resident ring for the _rings forms --, and the selection.  Nothing of the
// prover's, the verifier's or the screen's state is touched: the only memory is c->buf[B_rec], allocated by the first call.
#include "jobs.h"   // ctx.h, MaybeScope
#include "recover.h"   // REC_NCAND

#define ZK_RECOVER_CHUNK 16384u
// c->buf[B_rec]: the chunk's buffers, then (host-pointer forms) its inputs and results
struct RecoverStage {
    RecoverBuf buf;
    uint8_t *msg, *sig, *pk_out;
    uint32_t *ids, *which_out, *flags;
};
static size_t recover_carve(RecoverStage& S, uint8_t* base) {
    Carver k(base);
    const size_t C = ZK_RECOVER_CHUNK;
    S.buf.scratch = (uint32_t*)k.take(C * SCR_AREA_WORDS * 4);
    S.buf.cand = (uint8_t*)k.take(REC_NCAND * C * 64);
    S.buf.cand_ids = (uint32_t*)k.take(REC_NCAND * C * 4), S.buf.cand_which = (uint32_t*)k.take(REC_NCAND * C * 4), S.buf.state = (uint32_t*)k.take(C * 4);
    S.msg = (uint8_t*)k.take(32 * C), S.sig = (uint8_t*)k.take(64 * C), S.pk_out = (uint8_t*)k.take(64 * C);
    S.ids = (uint32_t*)k.take(4 * C), S.which_out = (uint32_t*)k.take(4 * C), S.flags = (uint32_t*)k.take(4 * C);
    return k.off + 256;
}
static zk_status recover_prepare(zk_ctx* c, bool rings, RecoverStage& S) {
    if (!c->params_set || (!rings && !c->ring->N)) return ZK_E_BUFFER;
    if (c->stream_busy) return busy_refusal(c);
    return lay_out(c, B_rec, [&](uint8_t* base) { return recover_carve(S, base); });
}
static ScreenRing recover_ring(const Ring& R) {   // (the lookup reads the limbs only)
    ScreenRing G;
    G.ring = Soa{R.ring_mem, (uint32_t)R.N}, G.N = (uint32_t)R.N, G.nkeys = (uint32_t)R.nkeys, G.id = R.id, G.ktab = nullptr, G.ktab_ok = nullptr;
    return G;
}
// one chunk, device pointers; everything is enqueued on c->stream
static void recover_chunk(zk_ctx* c, RecoverIn in, const RecoverBuf& buf, bool timed) {
    RingSlots rs{};
    for (const Ring& R : c->rings)
        if (R.live) rs.id[rs.count++] = R.id;
    in.plain_id = c->ring->id;
    for (uint32_t pass = 0; pass < 2; pass++) {
        {
            MaybeScope t(timed, c, "recover_lift", c->stream);
            launch_recover_lift(c->stream, in, buf, rs, pass);
        }
        MaybeScope t(timed, c, "recover_points", c->stream);
        launch_recover_points(c->stream, c->P, in, buf, pass);
    }
    {
        MaybeScope t(timed, c, "recover_lookup", c->stream);
        ScreenIn L{};   // the candidates as pseudo-witnesses of the screen's find mode: pk = the records, ids = the ring of an existing candidate or an id no ring has
        L.pk = buf.cand, L.ids = buf.cand_ids, L.which_out = buf.cand_which, L.count = REC_NCAND * in.count;
        if (in.ids) {   // (every resident ring makes a pass, whether the chunk names it or not: no census, no read-back; DESIGN.md 5b')
            for (const Ring& R : c->rings)
                if (R.live) launch_screen_lookup(c->stream, recover_ring(R), L);
        } else launch_screen_lookup(c->stream, recover_ring(*c->ring), L);
    }
    launch_recover_select(c->stream, in, buf);   // (outside the timed families: a few loads and stores per witness)
}
// a failed call leaves no u1, u2, candidate key or staged signature behind
static zk_status recover_fail(zk_ctx* c, hipError_t e, const char* what) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s failed: %s (api_recover.hip)", what, hipGetErrorString(e));
    c->err = buf;
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemset(c->buf[B_rec].p, 0, c->buf[B_rec].bytes);
    (void)hipGetLastError();
    return ZK_E_DEVICE;
}
static zk_status recover_device(zk_ctx* c, uint64_t B, const uint8_t* d_msg, const uint8_t* d_sig, const uint32_t* d_ids, bool rings, uint8_t* d_pk_out, uint32_t* d_which_out,
                                uint32_t* d_flags) {
    RecoverStage S;
    zk_status zs = recover_prepare(c, rings, S);
    if (zs || !B) return zs;
    const bool timed = zk_timed(c, B);
    timing_begin(c);
    for (uint64_t first = 0; first < B; first += ZK_RECOVER_CHUNK) {
        RecoverIn in{};
        in.msg = d_msg + 32 * first, in.sig = d_sig + 64 * first, in.ids = rings ? d_ids + first : nullptr;
        in.pk_out = d_pk_out + 64 * first, in.which_out = d_which_out + first, in.flags = d_flags + first, in.count = (uint32_t)std::min<uint64_t>(ZK_RECOVER_CHUNK, B - first);
        recover_chunk(c, in, S.buf, timed);
    }
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return recover_fail(c, e, "the recovery's kernels");
    timing_end(c);
    return ZK_OK;
}
static zk_status recover_host(zk_ctx* c, uint64_t B, const uint8_t* msg, const uint8_t* sig, const uint32_t* ids, bool rings, uint8_t* pk_out, uint32_t* which_out, uint32_t* flags) {
    RecoverStage S;
    zk_status zs = recover_prepare(c, rings, S);
    if (zs || !B) return zs;
    const bool timed = zk_timed(c, B);
    timing_begin(c);
    for (uint64_t first = 0; first < B; first += ZK_RECOVER_CHUNK) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(ZK_RECOVER_CHUNK, B - first);
        hipError_t e = hipMemcpyAsync(S.msg, msg + 32 * first, 32 * (size_t)cnt, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(S.sig, sig + 64 * first, 64 * (size_t)cnt, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && rings) e = hipMemcpyAsync(S.ids, ids + first, 4 * (size_t)cnt, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return recover_fail(c, e, "the copy of the recovery's inputs");
        RecoverIn in{};
        in.msg = S.msg, in.sig = S.sig, in.ids = rings ? S.ids : nullptr, in.pk_out = S.pk_out, in.which_out = S.which_out, in.flags = S.flags, in.count = cnt;
        recover_chunk(c, in, S.buf, timed);
        e = hipMemcpyAsync(pk_out + 64 * first, S.pk_out, 64 * (size_t)cnt, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(which_out + first, S.which_out, 4 * (size_t)cnt, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(flags + first, S.flags, 4 * (size_t)cnt, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // the staging area is reused by the next chunk
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) return recover_fail(c, e, "a chunk of the recovery");
    }
    timing_end(c);
    return ZK_OK;
}

extern "C" zk_status zk_recover_batch_device(zk_ctx* c, uint64_t B, const void* d_msg, const void* d_sig, void* d_pk_out, void* d_which_out, void* d_flags) {
    if (!c || !d_pk_out || !d_which_out || !d_flags || (B && (!d_msg || !d_sig))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return recover_device(c, B, (const uint8_t*)d_msg, (const uint8_t*)d_sig, nullptr, false, (uint8_t*)d_pk_out, (uint32_t*)d_which_out, (uint32_t*)d_flags);
}
extern "C" zk_status zk_recover_batch_rings_device(zk_ctx* c, uint64_t B, const void* d_msg, const void* d_sig, const void* d_ids, void* d_pk_out, void* d_which_out, void* d_flags) {
    if (!c || !d_pk_out || !d_which_out || !d_flags || (B && (!d_msg || !d_sig || !d_ids))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return recover_device(c, B, (const uint8_t*)d_msg, (const uint8_t*)d_sig, (const uint32_t*)d_ids, true, (uint8_t*)d_pk_out, (uint32_t*)d_which_out, (uint32_t*)d_flags);
}
extern "C" zk_status zk_recover_batch(zk_ctx* c, uint64_t B, const uint8_t* msg, const uint8_t* sig, uint8_t* pk_out, uint32_t* which_out, uint32_t* flags) {
    if (!c || !pk_out || !which_out || !flags || (B && (!msg || !sig))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return recover_host(c, B, msg, sig, nullptr, false, pk_out, which_out, flags);
}
extern "C" zk_status zk_recover_batch_rings(zk_ctx* c, uint64_t B, const uint8_t* msg, const uint8_t* sig, const uint32_t* ring_ids, uint8_t* pk_out, uint32_t* which_out,
                                            uint32_t* flags) {
    if (!c || !pk_out || !which_out || !flags || (B && (!msg || !sig || !ring_ids))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return recover_host(c, B, msg, sig, ring_ids, true, pk_out, which_out, flags);
}
