// Host side of the witness screen (include/zkattest.h: zk_screen_batch; kernels: k_screen.hip).
//
// A call runs in chunks of ZK_SCREEN_CHUNK witnesses on the context's main stream.  Per chunk: which_out / flags / the scratch areas are initialised, every
// ring of the call makes one pass (the lookup in find mode, then the front end of the ring's witnesses: checks, scalars, the choice of the path), and the
// point arithmetic runs once over the whole chunk.  The plain forms have one ring, the active one; the _rings forms pass over every resident ring -- at
// most ZK_MAX_RINGS -- with the witnesses of the other rings idle (a workgroup without a witness of the ring leaves at once), which needs no census of
// the ids and no read-back.  Nothing of the prover's or verifier's state is touched: the only memory is c->buf[B_scr], allocated by the first call.
#include "jobs.h"   // ctx.h, MaybeScope

#define ZK_SCREEN_CHUNK 16384u
// c->buf[B_scr]: the scratch areas, then (host-pointer forms) the chunk's inputs and results
struct ScreenStage {
    uint32_t* scratch;
    uint8_t *msg, *sig, *pk;
    uint32_t *which, *ids, *which_out, *flags;
};
static size_t screen_carve(ScreenStage& S, uint8_t* base) {
    Carver k(base);
    const size_t C = ZK_SCREEN_CHUNK;
    S.scratch = (uint32_t*)k.take(C * SCR_AREA_WORDS * 4);
    S.msg = (uint8_t*)k.take(32 * C), S.sig = (uint8_t*)k.take(64 * C), S.pk = (uint8_t*)k.take(64 * C);
    S.which = (uint32_t*)k.take(4 * C), S.ids = (uint32_t*)k.take(4 * C), S.which_out = (uint32_t*)k.take(4 * C), S.flags = (uint32_t*)k.take(4 * C);
    return k.off + 256;
}
static zk_status screen_prepare(zk_ctx* c, bool rings, ScreenStage& S) {
    if (!c->params_set || (!rings && !c->ring->N)) return ZK_E_BUFFER;
    if (c->stream_busy) return busy_refusal(c);
    return lay_out(c, B_scr, [&](uint8_t* base) { return screen_carve(S, base); });
}
static ScreenRing screen_ring(const Ring& R) {
    ScreenRing G;
    G.ring = Soa{R.ring_mem, (uint32_t)R.N}, G.N = (uint32_t)R.N, G.nkeys = (uint32_t)R.nkeys, G.id = R.id, G.ktab = R.ktab, G.ktab_ok = R.ktab_ok;
    return G;
}
// one chunk, device pointers; everything is enqueued on c->stream
static void screen_chunk(zk_ctx* c, const ScreenIn& in, uint32_t* scratch, bool timed) {
    {
        MaybeScope t(timed, c, "screen_lookup", c->stream);
        launch_screen_init(c->stream, in, scratch);
        if (in.ids) {
            for (const Ring& R : c->rings)
                if (R.live) launch_screen_lookup(c->stream, screen_ring(R), in);
        } else launch_screen_lookup(c->stream, screen_ring(*c->ring), in);
    }
    MaybeScope t(timed, c, "screen_ecdsa", c->stream);
    if (in.ids) {
        for (const Ring& R : c->rings)
            if (R.live) launch_screen_front(c->stream, screen_ring(R), in, scratch);
    } else launch_screen_front(c->stream, screen_ring(*c->ring), in, scratch);
    launch_screen_ecdsa(c->stream, c->P, in, scratch);
}
// a failed call leaves no u1, u2 or staged signature behind
static zk_status screen_fail(zk_ctx* c, hipError_t e, const char* what) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s failed: %s (api_screen.hip)", what, hipGetErrorString(e));
    c->err = buf;
    (void)hipStreamSynchronize(c->stream);
    (void)hipMemset(c->buf[B_scr].p, 0, c->buf[B_scr].bytes);
    (void)hipGetLastError();
    return ZK_E_DEVICE;
}
static zk_status screen_device(zk_ctx* c, uint64_t B, const uint8_t* d_msg, const uint8_t* d_sig, const uint8_t* d_pk, const uint32_t* d_which, const uint32_t* d_ids, bool rings,
                               uint32_t* d_which_out, uint32_t* d_flags) {
    ScreenStage S;
    zk_status zs = screen_prepare(c, rings, S);
    if (zs || !B) return zs;
    const bool timed = zk_timed(c, B);
    timing_begin(c);
    for (uint64_t first = 0; first < B; first += ZK_SCREEN_CHUNK) {
        ScreenIn in;
        in.msg = d_msg + 32 * first, in.sig = d_sig + 64 * first, in.pk = d_pk + 64 * first, in.which = d_which ? d_which + first : nullptr, in.ids = rings ? d_ids + first : nullptr;
        in.which_out = d_which_out + first, in.flags = d_flags + first, in.count = (uint32_t)std::min<uint64_t>(ZK_SCREEN_CHUNK, B - first);
        screen_chunk(c, in, S.scratch, timed);
    }
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return screen_fail(c, e, "the screen's kernels");
    timing_end(c);
    return ZK_OK;
}
static zk_status screen_host(zk_ctx* c, uint64_t B, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk, const uint32_t* which, const uint32_t* ids, bool rings,
                             uint32_t* which_out, uint32_t* flags) {
    ScreenStage S;
    zk_status zs = screen_prepare(c, rings, S);
    if (zs || !B) return zs;
    const bool timed = zk_timed(c, B);
    timing_begin(c);
    for (uint64_t first = 0; first < B; first += ZK_SCREEN_CHUNK) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(ZK_SCREEN_CHUNK, B - first);
        hipError_t e = hipMemcpyAsync(S.msg, msg + 32 * first, 32 * (size_t)cnt, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(S.sig, sig + 64 * first, 64 * (size_t)cnt, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(S.pk, pk + 64 * first, 64 * (size_t)cnt, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && which) e = hipMemcpyAsync(S.which, which + first, 4 * (size_t)cnt, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && rings) e = hipMemcpyAsync(S.ids, ids + first, 4 * (size_t)cnt, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return screen_fail(c, e, "the copy of the screen's inputs");
        ScreenIn in;
        in.msg = S.msg, in.sig = S.sig, in.pk = S.pk, in.which = which ? S.which : nullptr, in.ids = rings ? S.ids : nullptr, in.which_out = S.which_out, in.flags = S.flags, in.count = cnt;
        screen_chunk(c, in, S.scratch, timed);
        e = hipMemcpyAsync(which_out + first, S.which_out, 4 * (size_t)cnt, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(flags + first, S.flags, 4 * (size_t)cnt, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // the staging area is reused by the next chunk
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) return screen_fail(c, e, "a chunk of the screen");
    }
    timing_end(c);
    return ZK_OK;
}

extern "C" zk_status zk_screen_batch_device(zk_ctx* c, uint64_t B, const void* d_msg, const void* d_sig, const void* d_pk, const void* d_which, void* d_which_out, void* d_flags) {
    if (!c || !d_which_out || !d_flags || (B && (!d_msg || !d_sig || !d_pk))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return screen_device(c, B, (const uint8_t*)d_msg, (const uint8_t*)d_sig, (const uint8_t*)d_pk, (const uint32_t*)d_which, nullptr, false, (uint32_t*)d_which_out, (uint32_t*)d_flags);
}
extern "C" zk_status zk_screen_batch_rings_device(zk_ctx* c, uint64_t B, const void* d_msg, const void* d_sig, const void* d_pk, const void* d_which, const void* d_ids,
                                                  void* d_which_out, void* d_flags) {
    if (!c || !d_which_out || !d_flags || (B && (!d_msg || !d_sig || !d_pk || !d_ids))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return screen_device(c, B, (const uint8_t*)d_msg, (const uint8_t*)d_sig, (const uint8_t*)d_pk, (const uint32_t*)d_which, (const uint32_t*)d_ids, true, (uint32_t*)d_which_out,
                         (uint32_t*)d_flags);
}
extern "C" zk_status zk_screen_batch(zk_ctx* c, uint64_t B, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk, const uint32_t* which, uint32_t* which_out, uint32_t* flags) {
    if (!c || !which_out || !flags || (B && (!msg || !sig || !pk))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return screen_host(c, B, msg, sig, pk, which, nullptr, false, which_out, flags);
}
extern "C" zk_status zk_screen_batch_rings(zk_ctx* c, uint64_t B, const uint8_t* msg, const uint8_t* sig, const uint8_t* pk, const uint32_t* which, const uint32_t* ring_ids,
                                           uint32_t* which_out, uint32_t* flags) {
    if (!c || !which_out || !flags || (B && (!msg || !sig || !pk || !ring_ids))) return ZK_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    return screen_host(c, B, msg, sig, pk, which, ring_ids, true, which_out, flags);
}
