/* N-API addon over the C ABI (include/zkattest.h): the binding a maintainer of the reference would put behind
 * src/zkpAttestList.ts.  Plain C, N-API version 3 (the header of the Node in this image):
 *
 *   gcc -shared -fPIC -O2 -I/usr/include/node -I../../include zkattest_napi.c -o zkattest.node \
 *       -L../../zkp-ecdsa_amd/lib -lzkattest_hip -Wl,-rpath,<abs path of zkp-ecdsa_amd/lib>
 *
 * One handle = one zk_pool = the listed GPUs of this node (one GPU: a pool of one).  A handle runs one batch at a time: the
 * synchronous calls finish before they return, the *Async calls run on a libuv worker thread and mark the handle busy
 * until their Promise settles; a second call on a busy handle, any call on a destroyed one, and destroying a busy one
 * throw instead of touching freed memory.  The garbage collector destroys a handle nobody closed.  proveSubmit / verifySubmit
 * are the streamed form: several batches of one handle in flight (zk_pool_prove_submit / _wait), one Promise per batch.
 * Large proof buffers are page-locked (zk_host_alloc) and handed to JavaScript as external Buffers, so the engine moves
 * the proof bytes by DMA under its kernels and nothing is copied on the way out. */
#define NAPI_VERSION 3
#include <math.h>
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "zkattest.h"

#define NAPI_OK(call)                                                 \
    do {                                                              \
        if ((call) != napi_ok) {                                      \
            napi_throw_error(env, NULL, "N-API call failed: " #call); \
            return NULL;                                              \
        }                                                             \
    } while (0)
#define PINNED_MIN ((size_t)32 << 20) /* proof buffers from this size on are page-locked */

struct Job;
typedef struct {
    zk_pool *pool;
    int busy, closed;
    int orphaned; /* the external was finalized (environment teardown) while a batch was still running: job_complete frees it */
    uint32_t sec;
    /* streamed batches (proveSubmit / verifySubmit): jobs in submission order, at most `inflight` of them submitted to the engine */
    struct Job *sq_head, *sq_tail;
    int sq_submitted, sq_running;
    uint32_t inflight;
} Handle;

static napi_value throw_text(napi_env env, zk_status st, const char *detail) {
    char msg[640];
    snprintf(msg, sizeof msg, "%s%s%s", zk_strerror(st), detail && detail[0] ? ": " : "", detail ? detail : "");
    napi_throw_error(env, NULL, msg); /* the reference's error texts: 'point not in group', 'T[i] is at infinity', ... */
    return NULL;
}
/* a NULL pool asks the library why the last zk_pool_create of this thread failed */
static napi_value throw_status(napi_env env, Handle *h, zk_status st) { return throw_text(env, st, zk_pool_last_error(h ? h->pool : NULL)); }
static int get_args(napi_env env, napi_callback_info info, size_t want, napi_value *argv) {
    size_t argc = want;
    if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < want) {
        napi_throw_type_error(env, NULL, "wrong number of arguments");
        return 0;
    }
    return 1;
}
/* the handle behind an external; refuses destroyed and (unless allow_busy) busy ones */
static Handle *get_handle(napi_env env, napi_value v, int allow_busy) {
    void *p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p) {
        napi_throw_type_error(env, NULL, "expected an engine handle");
        return NULL;
    }
    Handle *h = p;
    if (h->closed || !h->pool) {
        napi_throw_error(env, NULL, "the engine has been destroyed");
        return NULL;
    }
    if (h->busy && !allow_busy) {
        napi_throw_error(env, NULL, "the engine is busy with an asynchronous batch (one batch at a time per engine)");
        return NULL;
    }
    return h;
}
static void handle_release(Handle *h) {
    if (h->pool) zk_pool_destroy(h->pool);
    free(h);
}
/* The worker thread of a running batch still uses h->pool and job_complete still writes h->busy: a busy handle outlives its
 * external and is released by job_complete. */
static void handle_finalize(napi_env env, void *data, void *hint) {
    Handle *h = data;
    if (h->busy) h->orphaned = 1;
    else handle_release(h);
}
/* Buffer or typed array -> pointer + byte length (NULL for null/undefined) */
static int get_bytes(napi_env env, napi_value v, uint8_t **p, size_t *len) {
    napi_valuetype t;
    *p = NULL, *len = 0;
    if (napi_typeof(env, v, &t) != napi_ok) return 0;
    if (t == napi_null || t == napi_undefined) return 1;
    bool is = false;
    if (napi_is_buffer(env, v, &is) == napi_ok && is) return napi_get_buffer_info(env, v, (void **)p, len) == napi_ok;
    if (napi_is_typedarray(env, v, &is) == napi_ok && is) {
        napi_typedarray_type ty;
        size_t n, off;
        napi_value ab;
        void *data;
        if (napi_get_typedarray_info(env, v, &ty, &n, &data, &ab, &off) != napi_ok) return 0;
        size_t w = ty == napi_uint8_array || ty == napi_int8_array || ty == napi_uint8_clamped_array ? 1
                   : ty == napi_uint16_array || ty == napi_int16_array                              ? 2
                   : ty == napi_uint32_array || ty == napi_int32_array || ty == napi_float32_array ? 4
                                                                                                    : 8;
        *p = (uint8_t *)data, *len = n * w;
        return 1;
    }
    napi_throw_type_error(env, NULL, "expected a Buffer or typed array");
    return 0;
}
static napi_value new_buffer(napi_env env, const void *src, size_t len) {
    napi_value b;
    void *dst;
    if (napi_create_buffer_copy(env, len, len ? src : "", &dst, &b) != napi_ok) return NULL;
    return b;
}
static void set_prop(napi_env env, napi_value obj, const char *name, napi_value v) {
    if (v) napi_set_named_property(env, obj, name, v);
}
static void *xmalloc(napi_env env, size_t n) {
    void *p = malloc(n ? n : 1);
    if (!p && env) napi_throw_error(env, NULL, "out of memory");
    return p;
}
/* proof buffers: page-locked from PINNED_MIN on */
typedef struct {
    uint8_t *p;
    size_t cap;
    int pinned;
} Slab;
static int slab_alloc(Slab *s, size_t cap) {
    s->cap = cap ? cap : 1, s->pinned = 0, s->p = NULL;
    if (s->cap >= PINNED_MIN) {
        s->p = zk_host_alloc(s->cap);
        s->pinned = s->p != NULL;
    }
    if (!s->p) s->p = malloc(s->cap);
    return s->p != NULL;
}
static void slab_free(Slab *s) {
    if (s->p) {
        if (s->pinned) zk_host_free(s->p);
        else free(s->p);
    }
    s->p = NULL;
}
static void slab_finalize(napi_env env, void *data, void *hint) {
    if (hint) zk_host_free(data);
    else free(data);
}
/* hands the slab to JavaScript as a Buffer of `len` bytes (ownership moves to the Buffer) */
static napi_value slab_to_buffer(napi_env env, Slab *s, size_t len) {
    napi_value b = NULL;
    if (napi_create_external_buffer(env, len, s->p, slab_finalize, s->pinned ? (void *)1 : NULL, &b) != napi_ok) {
        slab_free(s);
        return NULL;
    }
    s->p = NULL;
    return b;
}

static napi_value CreatePool(napi_env env, napi_callback_info info) { /* (deviceIds: Int32Array | Buffer of i32) -> handle */
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return NULL;
    uint8_t *ids;
    size_t li;
    if (!get_bytes(env, argv[0], &ids, &li)) return NULL;
    if (!ids || li < 4 || li % 4) {
        napi_throw_type_error(env, NULL, "createPool: an Int32Array of device ids");
        return NULL;
    }
    Handle *h = calloc(1, sizeof *h);
    if (!h) return throw_text(env, ZK_E_BUFFER, "out of memory");
    h->sec = 80;
    zk_status st = zk_pool_create((const int *)ids, (int)(li / 4), &h->pool);
    if (st != ZK_OK) {
        napi_value r = throw_status(env, h, st);
        if (h->pool) zk_pool_destroy(h->pool);
        free(h);
        return r;
    }
    napi_value ext;
    if (napi_create_external(env, h, handle_finalize, NULL, &ext) != napi_ok) {
        zk_pool_destroy(h->pool), free(h);
        napi_throw_error(env, NULL, "could not create the handle");
        return NULL;
    }
    return ext;
}
static napi_value DestroyPool(napi_env env, napi_callback_info info) { /* idempotent; throws while an async batch is running */
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return NULL;
    void *p = NULL;
    if (napi_get_value_external(env, argv[0], &p) != napi_ok || !p) return NULL;
    Handle *h = p;
    if (h->closed) return NULL;
    if (h->busy) {
        napi_throw_error(env, NULL, "cannot destroy an engine while an asynchronous batch is running on it");
        return NULL;
    }
    h->closed = 1;
    zk_pool_destroy(h->pool);
    h->pool = NULL;
    return NULL;
}
static napi_value PoolInfo(napi_env env, napi_callback_info info) { /* (h) -> {devices, ringTransport, proofMaxSize} */
    napi_value argv[1], o, v;
    if (!get_args(env, info, 1, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 1);
    if (!h) return NULL;
    NAPI_OK(napi_create_object(env, &o));
    NAPI_OK(napi_create_int32(env, zk_pool_size(h->pool), &v));
    set_prop(env, o, "devices", v);
    NAPI_OK(napi_create_string_utf8(env, zk_pool_ring_transport(h->pool), NAPI_AUTO_LENGTH, &v));
    set_prop(env, o, "ringTransport", v);
    NAPI_OK(napi_create_double(env, (double)zk_proof_max_size(zk_pool_ctx(h->pool, 0)), &v));
    set_prop(env, o, "proofMaxSize", v);
    return o;
}
/* (h, name, value): per-device settings applied to every device of the pool */
static napi_value SetOption(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    if (!h) return NULL;
    char name[32];
    size_t ln;
    uint32_t val;
    NAPI_OK(napi_get_value_string_utf8(env, argv[1], name, sizeof name, &ln));
    NAPI_OK(napi_get_value_uint32(env, argv[2], &val));
    if (!strcmp(name, "inflight")) { /* streamed jobs inside the engine at a time (proveSubmit / verifySubmit); the addon's own knob */
        if (val < 1 || val > 8) return throw_text(env, ZK_E_ARG, name);
        h->inflight = val;
        return NULL;
    }
    for (int i = 0; i < zk_pool_size(h->pool); i++) {
        zk_ctx *c = zk_pool_ctx(h->pool, i);
        zk_status st = !strcmp(name, "chunk")         ? zk_ctx_set_chunk(c, val)
                       : !strcmp(name, "lanes")       ? zk_ctx_set_lanes(c, val)
                       : !strcmp(name, "combBits")    ? zk_ctx_set_comb_bits(c, val)
                       : !strcmp(name, "hostTaper")   ? zk_ctx_set_host_taper(c, val)
                       : !strcmp(name, "batchVerify") ? zk_ctx_set_batch_verify(c, val)
                       : !strcmp(name, "mode")        ? zk_ctx_set_mode(c, val)
                       : !strcmp(name, "slice")       ? zk_ctx_set_slice(c, val)
                       : !strcmp(name, "ringFold")    ? zk_ctx_set_ring_fold(c, val)
                       : !strcmp(name, "verifyGroups") ? zk_ctx_set_verify_groups(c, val)
                       : !strcmp(name, "wire")        ? zk_ctx_set_wire(c, val)
                       : !strcmp(name, "verifyLevel") ? zk_ctx_set_verify_level(c, val) /* 0: the context's secLevel, 1: every proof's own */
                       : !strcmp(name, "verifyReps")  ? zk_ctx_set_verify_reps(c, val) /* 0: the 20 sampled repetitions, 1: every repetition of every proof */
                       : !strcmp(name, "wipe")        ? zk_ctx_wipe(c) /* value ignored: zero the witness-derived device memory of every context now */
                                                      : ZK_E_ARG;
        if (st != ZK_OK) return throw_text(env, st, name);
    }
    return NULL;
}
static napi_value SetParams(napi_env env, napi_callback_info info) { /* (h, nistH 64, tomG 72, tomH 72, secLevel) */
    napi_value argv[5];
    if (!get_args(env, info, 5, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *a, *b, *c;
    size_t la, lb, lc;
    uint32_t sec;
    if (!h || !get_bytes(env, argv[1], &a, &la) || !get_bytes(env, argv[2], &b, &lb) || !get_bytes(env, argv[3], &c, &lc)) return NULL;
    NAPI_OK(napi_get_value_uint32(env, argv[4], &sec));
    if (la != 64 || lb != 72 || lc != 72) {
        napi_throw_range_error(env, NULL, "params: h_NIST is 64 bytes, g and h of Tom-256 are 72 bytes (affine, big-endian)");
        return NULL;
    }
    zk_status st = zk_pool_set_params(h->pool, a, b, c, sec);
    if (st == ZK_OK) h->sec = sec;
    return st == ZK_OK ? NULL : throw_status(env, h, st);
}
static napi_value SetRing(napi_env env, napi_callback_info info) { /* (h, keys: n x 32 bytes) -> transport */
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *k;
    size_t lk;
    if (!h || !get_bytes(env, argv[1], &k, &lk)) return NULL;
    zk_status st = zk_pool_set_ring(h->pool, k, lk / 32);
    if (st != ZK_OK) return throw_status(env, h, st);
    napi_value v;
    NAPI_OK(napi_create_string_utf8(env, zk_pool_ring_transport(h->pool), NAPI_AUTO_LENGTH, &v));
    return v;
}
static napi_value SynthParams(napi_env env, napi_callback_info info) { /* (h, seed) -> {nistH, tomG, tomH} */
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint32_t seed;
    if (!h) return NULL;
    NAPI_OK(napi_get_value_uint32(env, argv[1], &seed));
    uint8_t a[64], b[72], c[72];
    zk_ctx *ctx = zk_pool_ctx(h->pool, 0);
    zk_status st = zk_synth_params(ctx, seed, a, b, c);
    if (st != ZK_OK) return throw_text(env, st, zk_last_error(ctx));
    napi_value o;
    NAPI_OK(napi_create_object(env, &o));
    set_prop(env, o, "nistH", new_buffer(env, a, 64)), set_prop(env, o, "tomG", new_buffer(env, b, 72)), set_prop(env, o, "tomH", new_buffer(env, c, 72));
    return o;
}
static napi_value SynthWorkload(napi_env env, napi_callback_info info) { /* (h, seed, nKeys, B) -> {ring, msg, sig, pk, which, seeds} */
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint32_t seed, nk, B;
    if (!h) return NULL;
    NAPI_OK(napi_get_value_uint32(env, argv[1], &seed));
    NAPI_OK(napi_get_value_uint32(env, argv[2], &nk));
    NAPI_OK(napi_get_value_uint32(env, argv[3], &B));
    uint8_t *ring = malloc(32 * (size_t)nk + 1), *msg = malloc(32 * (size_t)B + 1), *sig = malloc(64 * (size_t)B + 1), *pk = malloc(64 * (size_t)B + 1),
            *seeds = malloc(32 * (size_t)B + 1);
    uint32_t *which = malloc(4 * (size_t)B + 4);
    napi_value o = NULL;
    zk_ctx *ctx = zk_pool_ctx(h->pool, 0);
    zk_status st = ring && msg && sig && pk && seeds && which ? zk_synth_workload(ctx, seed, nk, B, ring, msg, sig, pk, which, seeds) : ZK_E_BUFFER;
    if (st == ZK_OK && napi_create_object(env, &o) == napi_ok) {
        set_prop(env, o, "ring", new_buffer(env, ring, 32 * (size_t)nk)), set_prop(env, o, "msg", new_buffer(env, msg, 32 * (size_t)B));
        set_prop(env, o, "sig", new_buffer(env, sig, 64 * (size_t)B)), set_prop(env, o, "pk", new_buffer(env, pk, 64 * (size_t)B));
        set_prop(env, o, "which", new_buffer(env, which, 4 * (size_t)B)), set_prop(env, o, "seeds", new_buffer(env, seeds, 32 * (size_t)B));
    }
    free(ring), free(msg), free(sig), free(pk), free(seeds), free(which);
    return st == ZK_OK ? o : throw_text(env, st, zk_last_error(ctx));
}

/* ---- batches.  A Job owns copies of the small inputs; the (large) proof input of a verification is referenced, not copied. */
typedef struct Job {
    int verify, async;
    Handle *h;
    size_t B;
    uint8_t *msg, *sig, *pk, *seeds;
    const uint8_t *proofs_in;
    napi_ref proofs_ref, h_ref; /* an asynchronous job keeps the proof bytes and the handle alive */
    uint32_t *which;
    Slab out;
    uint64_t worst_cap, *off, *len;
    int32_t *status;
    uint8_t *ok;
    uint32_t *ring_ids; /* verifyBatchRings, proveBatchRings: one resident ring id per proof */
    zk_status rc;
    char err[384];
    napi_deferred deferred;
    napi_async_work work;
    /* streamed form */
    struct Job *next;
    int stream, submitted, op; /* op of the running step: 0 = submit, 1 = wait */
    zk_pool_job *pj;
    napi_ref out_ref; /* the caller's page-locked output Buffer */
    uint8_t *out_ext;
    size_t out_ext_cap;
} Job;
static uint8_t *dup_bytes(const uint8_t *p, size_t n) {
    uint8_t *q = malloc(n ? n : 1);
    if (q && p && n) memcpy(q, p, n);
    return q;
}
static void job_free(napi_env env, Job *j) {
    if (j->proofs_ref && env) napi_delete_reference(env, j->proofs_ref);
    if (j->h_ref && env) napi_delete_reference(env, j->h_ref);
    if (j->out_ref && env) napi_delete_reference(env, j->out_ref);
    slab_free(&j->out);
    free(j->msg), free(j->sig), free(j->pk), free(j->seeds), free(j->which), free(j->off), free(j->len), free(j->status), free(j->ok), free(j->ring_ids);
    free(j);
}
/* output capacity for B proofs over G devices: mean + 8 sigma of the zero-bit repetitions per shard, at most the worst case */
static void prove_caps(Handle *h, size_t B, uint64_t mx, uint64_t *cap, uint64_t *worst) {
    uint64_t G = (uint64_t)zk_pool_size(h->pool), m = (B + G - 1) / G;
    uint64_t w = ((mx * (m ? m : 1) + 511) & ~(uint64_t)255) * G;
    double mean = (double)m * ((double)mx - 3392.0 * h->sec / 2.0), dev = 8.0 * 3392.0 * sqrt((double)m * h->sec / 4.0);
    uint64_t c = (((uint64_t)(mean + dev) + mx + 511) & ~(uint64_t)255) * G;
    *worst = w, *cap = c < w ? c : w;
}
static void job_execute(napi_env env, void *data) { /* worker thread (or inline for the synchronous calls): no N-API calls here */
    Job *j = data;
    zk_pool *p = j->h->pool;
    if (j->verify && j->ring_ids) {
        j->rc = zk_pool_verify_batch_rings(p, j->B, j->msg, j->proofs_in, j->off, j->len, j->ring_ids, j->seeds, j->ok, j->status);
    } else if (j->verify) {
        j->rc = zk_pool_verify_batch(p, j->B, j->msg, j->proofs_in, j->off, j->len, j->seeds, j->ok, j->status);
    } else {
        zk_rng rng = {ZK_RNG_SEED, j->seeds, 0};
        for (int pass = 0; pass < 2; pass++) {
            if (j->ring_ids)
                j->rc = zk_pool_prove_batch_rings(p, j->B, j->msg, j->sig, j->pk, j->which, j->ring_ids, &rng, j->out.p, j->out.cap, j->off, j->len, j->status);
            else j->rc = zk_pool_prove_batch(p, j->B, j->msg, j->sig, j->pk, j->which, &rng, j->out.p, j->out.cap, j->off, j->len, j->status);
            if (j->rc != ZK_E_BUFFER || j->out.cap >= j->worst_cap) break;
            slab_free(&j->out); /* 8 sigma were not enough: worst-case buffer */
            if (!slab_alloc(&j->out, j->worst_cap)) break;
        }
    }
    if (j->rc != ZK_OK) snprintf(j->err, sizeof j->err, "%s: %s", zk_strerror(j->rc), zk_pool_last_error(p));
}
static napi_value job_result(napi_env env, Job *j) {
    napi_value v;
    if (napi_create_object(env, &v) != napi_ok) return NULL;
    if (j->verify) {
        set_prop(env, v, "ok", new_buffer(env, j->ok, j->B));
    } else {
        uint64_t end = 0;
        for (size_t b = 0; b < j->B; b++)
            if (j->off[b] + j->len[b] > end) end = j->off[b] + j->len[b];
        set_prop(env, v, "proofs", slab_to_buffer(env, &j->out, (size_t)end));
        set_prop(env, v, "offsets", new_buffer(env, j->off, 8 * j->B)), set_prop(env, v, "lengths", new_buffer(env, j->len, 8 * j->B));
    }
    set_prop(env, v, "status", new_buffer(env, j->status, 4 * j->B));
    return v;
}
static void job_complete(napi_env env, napi_status status, void *data) { /* main thread */
    Job *j = data;
    j->h->busy = 0;
    if (j->h->orphaned) { /* finalized meanwhile: nobody can reach the handle any more */
        handle_release(j->h);
        j->h = NULL;
    }
    napi_value v = status == napi_ok && j->rc == ZK_OK ? job_result(env, j) : NULL;
    if (v) {
        napi_resolve_deferred(env, j->deferred, v);
    } else {
        napi_value msg, e;
        napi_create_string_utf8(env, j->rc != ZK_OK ? j->err : "asynchronous batch failed", NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, NULL, msg, &e);
        napi_reject_deferred(env, j->deferred, e);
    }
    napi_delete_async_work(env, j->work);
    job_free(env, j);
}
static napi_value job_run(napi_env env, Job *j, const char *name) {
    if (!j->async) {
        job_execute(env, j);
        napi_value v = j->rc == ZK_OK ? job_result(env, j) : NULL;
        if (!v) {
            if (j->rc != ZK_OK) napi_throw_error(env, NULL, j->err);
            else napi_throw_error(env, NULL, "could not build the result");
        }
        job_free(env, j);
        return v;
    }
    napi_value promise, rn;
    if (napi_create_promise(env, &j->deferred, &promise) != napi_ok || napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &rn) != napi_ok ||
        napi_create_async_work(env, NULL, rn, job_execute, job_complete, j, &j->work) != napi_ok) {
        job_free(env, j);
        napi_throw_error(env, NULL, "could not queue the batch");
        return NULL;
    }
    j->h->busy = 1;
    if (napi_queue_async_work(env, j->work) != napi_ok) {
        j->h->busy = 0;
        napi_delete_async_work(env, j->work);
        job_free(env, j);
        napi_throw_error(env, NULL, "could not queue the batch");
        return NULL;
    }
    return promise;
}
/* (h, msg Bx32, sig Bx64, pk Bx64, which Bx4 (u32 LE), seeds Bx32)
 *   -> {proofs: Buffer, offsets: B u64 LE, lengths: B u64 LE, status: B i32}   proof b = proofs[offsets[b] .. offsets[b] + lengths[b])
 * rings: (h, msg, sig, pk, which, ringIds (B u32 LE), seeds) -- zk_pool_prove_batch_rings: which[b] indexes ring ringIds[b] */
static napi_value prove_common(napi_env env, napi_callback_info info, int async, int rings) {
    napi_value argv[7];
    if (!get_args(env, info, rings ? 7 : 6, argv)) return NULL;
    uint8_t *ids = NULL;
    size_t lid = 0;
    if (rings) {
        if (!get_bytes(env, argv[5], &ids, &lid)) return NULL;
        argv[5] = argv[6];
    }
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *msg, *sig, *pk, *which, *seeds;
    size_t lm, ls, lp, lw, lse;
    if (!h || !get_bytes(env, argv[1], &msg, &lm) || !get_bytes(env, argv[2], &sig, &ls) || !get_bytes(env, argv[3], &pk, &lp) ||
        !get_bytes(env, argv[4], &which, &lw) || !get_bytes(env, argv[5], &seeds, &lse))
        return NULL;
    size_t B = lm / 32;
    if (!B || lm != 32 * B || ls != 64 * B || lp != 64 * B || lw != 4 * B || lse != 32 * B || (rings && (!ids || lid != 4 * B))) {
        napi_throw_range_error(env, NULL, "proveBatch: per proof 32-byte msgHash, 64-byte signature, 64-byte public key, u32 index, 32-byte seed");
        return NULL;
    }
    Job *j = calloc(1, sizeof *j);
    if (!j) return throw_text(env, ZK_E_BUFFER, "out of memory");
    j->h = h, j->B = B, j->async = async;
    j->msg = dup_bytes(msg, lm), j->sig = dup_bytes(sig, ls), j->pk = dup_bytes(pk, lp), j->seeds = dup_bytes(seeds, lse);
    j->which = (uint32_t *)dup_bytes(which, lw);
    j->ring_ids = rings ? (uint32_t *)dup_bytes(ids, lid) : NULL;
    uint64_t cap, mx = zk_proof_max_size(zk_pool_ctx(h->pool, 0));
    if (rings) { /* the largest proof over the resident rings the batch names; the active ring plays no part */
        mx = 32;
        for (size_t b = 0; j->ring_ids && b < B; b++) {
            uint64_t m = !b || j->ring_ids[b] != j->ring_ids[b - 1] ? zk_ring_proof_max_size(zk_pool_ctx(h->pool, 0), j->ring_ids[b]) : 0;
            if (m > mx) mx = m;
        }
    }
    prove_caps(h, B, mx, &cap, &j->worst_cap);
    j->off = malloc(8 * B), j->len = malloc(8 * B), j->status = malloc(4 * B);
    if (!j->msg || !j->sig || !j->pk || !j->seeds || !j->which || !j->off || !j->len || !j->status || (rings && !j->ring_ids) || !slab_alloc(&j->out, cap)) {
        job_free(env, j);
        return throw_text(env, ZK_E_BUFFER, "out of memory");
    }
    if (async && napi_create_reference(env, argv[0], 1, &j->h_ref) != napi_ok) {
        job_free(env, j);
        return throw_text(env, ZK_E_BUFFER, "could not reference the handle");
    }
    return job_run(env, j, "zkattest.proveBatch");
}
static napi_value ProveBatch(napi_env env, napi_callback_info info) { return prove_common(env, info, 0, 0); }
static napi_value ProveBatchAsync(napi_env env, napi_callback_info info) { return prove_common(env, info, 1, 0); }
static napi_value ProveBatchRings(napi_env env, napi_callback_info info) { return prove_common(env, info, 0, 1); }
static napi_value ProveBatchRingsAsync(napi_env env, napi_callback_info info) { return prove_common(env, info, 1, 1); }
/* (h, msg Bx32, proofs, offsets (B u64 LE), lengths (B u64 LE), seeds Bx32 | null) -> {ok: B bytes, status: B i32}
 * rings: (h, msg, proofs, offsets, lengths, ringIds (B u32 LE), seeds | null) -- zk_pool_verify_batch_rings */
static napi_value verify_common(napi_env env, napi_callback_info info, int async, int rings) {
    napi_value argv[7];
    if (!get_args(env, info, rings ? 7 : 6, argv)) return NULL;
    uint8_t *ids = NULL;
    size_t lid = 0;
    if (rings) {
        if (!get_bytes(env, argv[5], &ids, &lid)) return NULL;
        argv[5] = argv[6];
    }
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *msg, *proofs, *offs, *lens, *seeds;
    size_t lm, lp, lo, ll, ls;
    if (!h || !get_bytes(env, argv[1], &msg, &lm) || !get_bytes(env, argv[2], &proofs, &lp) || !get_bytes(env, argv[3], &offs, &lo) ||
        !get_bytes(env, argv[4], &lens, &ll) || !get_bytes(env, argv[5], &seeds, &ls))
        return NULL;
    size_t B = lm / 32;
    if (!B || lm != 32 * B || lo != 8 * B || ll != 8 * B || (seeds && ls != 32 * B) || !proofs || (rings && lid != 4 * B)) {
        napi_throw_range_error(env, NULL, "verifyBatch: B message hashes, B offsets, B lengths, B seeds or null");
        return NULL;
    }
    Job *j = calloc(1, sizeof *j);
    if (!j) return throw_text(env, ZK_E_BUFFER, "out of memory");
    j->verify = 1, j->h = h, j->B = B, j->async = async;
    j->msg = dup_bytes(msg, lm), j->off = (uint64_t *)dup_bytes(offs, lo), j->len = (uint64_t *)dup_bytes(lens, ll);
    j->seeds = seeds ? dup_bytes(seeds, ls) : NULL;
    j->ok = malloc(B), j->status = malloc(4 * B);
    j->ring_ids = rings ? (uint32_t *)dup_bytes(ids, lid) : NULL;
    j->proofs_in = proofs;
    int okk = j->msg && j->off && j->len && j->ok && j->status && (!seeds || j->seeds) && (!rings || j->ring_ids);
    for (size_t b = 0; okk && b < B; b++) okk = j->off[b] <= lp && j->len[b] <= lp - j->off[b];
    if (okk && async) okk = napi_create_reference(env, argv[2], 1, &j->proofs_ref) == napi_ok && napi_create_reference(env, argv[0], 1, &j->h_ref) == napi_ok;
    if (!okk) {
        job_free(env, j);
        napi_throw_range_error(env, NULL, "verifyBatch: out of memory, or offsets / lengths beyond the proof buffer");
        return NULL;
    }
    return job_run(env, j, "zkattest.verifyBatch");
}
static napi_value VerifyBatch(napi_env env, napi_callback_info info) { return verify_common(env, info, 0, 0); }
static napi_value VerifyBatchAsync(napi_env env, napi_callback_info info) { return verify_common(env, info, 1, 0); }
static napi_value VerifyBatchRings(napi_env env, napi_callback_info info) { return verify_common(env, info, 0, 1); }
static napi_value VerifyBatchRingsAsync(napi_env env, napi_callback_info info) { return verify_common(env, info, 1, 1); }
/* ---- resident rings (zk_pool_add_ring / use_ring / drop_ring, zk_ring_info of the first shard) */
static napi_value AddRing(napi_env env, napi_callback_info info) { /* (h, keys: n x 32 bytes) -> ring id */
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *k;
    size_t lk;
    if (!h || !get_bytes(env, argv[1], &k, &lk)) return NULL;
    uint32_t id = 0;
    zk_status st = zk_pool_add_ring(h->pool, k, lk / 32, &id);
    if (st != ZK_OK) return throw_status(env, h, st);
    napi_value v;
    NAPI_OK(napi_create_uint32(env, id, &v));
    return v;
}
static napi_value UpdateRing(napi_env env, napi_callback_info info) { /* (h, ring id, indices: count x u64 LE, keys: count x 32 bytes, nKeys): zk_pool_update_ring */
    napi_value argv[5];
    if (!get_args(env, info, 5, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *ib, *k;
    size_t li, lk;
    uint32_t id;
    double nk;
    if (!h || !get_bytes(env, argv[2], &ib, &li) || !get_bytes(env, argv[3], &k, &lk)) return NULL;
    if (napi_get_value_uint32(env, argv[1], &id) != napi_ok || napi_get_value_double(env, argv[4], &nk) != napi_ok || nk < 0 || nk > 9007199254740992.0) {
        napi_throw_type_error(env, NULL, "expected a ring id and a key count");
        return NULL;
    }
    if (li % 8 || lk != li * 4) {
        napi_throw_range_error(env, NULL, "updateRing: one 64-bit index and one 32-byte key per change");
        return NULL;
    }
    const size_t count = li / 8;
    uint64_t *idx = (uint64_t *)malloc(li ? li : 8); /* (a Buffer's bytes need not be 8-byte aligned) */
    if (!idx) {
        napi_throw_range_error(env, NULL, "updateRing: out of memory");
        return NULL;
    }
    memcpy(idx, ib, li);
    zk_status st = zk_pool_update_ring(h->pool, id, count, idx, k, (uint64_t)nk);
    free(idx);
    return st == ZK_OK ? NULL : throw_status(env, h, st);
}
static napi_value ring_call(napi_env env, napi_callback_info info, zk_status (*f)(zk_pool *, uint32_t)) { /* (h, ring id) */
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint32_t id;
    if (!h) return NULL;
    if (napi_get_value_uint32(env, argv[1], &id) != napi_ok) {
        napi_throw_type_error(env, NULL, "expected a ring id");
        return NULL;
    }
    zk_status st = f(h->pool, id);
    return st == ZK_OK ? NULL : throw_status(env, h, st);
}
static napi_value UseRing(napi_env env, napi_callback_info info) { return ring_call(env, info, zk_pool_use_ring); }
static napi_value DropRing(napi_env env, napi_callback_info info) { return ring_call(env, info, zk_pool_drop_ring); }
static napi_value RingInfo(napi_env env, napi_callback_info info) { /* (h, ring id) -> {nKeys, logN, flags, generation} */
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint32_t id, logn = 0, flags = 0;
    uint64_t nk = 0, gen = 0;
    if (!h) return NULL;
    if (napi_get_value_uint32(env, argv[1], &id) != napi_ok) {
        napi_throw_type_error(env, NULL, "expected a ring id");
        return NULL;
    }
    zk_status st = zk_ring_info(zk_pool_ctx(h->pool, 0), id, &nk, &logn, &flags, &gen);
    if (st != ZK_OK) return throw_text(env, st, "no resident ring has this id");
    napi_value v, a, b, c, d;
    NAPI_OK(napi_create_object(env, &v));
    NAPI_OK(napi_create_double(env, (double)nk, &a));
    NAPI_OK(napi_create_uint32(env, logn, &b));
    NAPI_OK(napi_create_uint32(env, flags, &c));
    NAPI_OK(napi_create_double(env, (double)gen, &d));
    set_prop(env, v, "nKeys", a), set_prop(env, v, "logN", b), set_prop(env, v, "flags", c), set_prop(env, v, "generation", d);
    return v;
}

/* ---- streamed batches: several jobs of one handle in flight (zk_pool_prove_submit / _wait).
 * proveSubmit / verifySubmit return a Promise at once and append the job to the handle's queue.  The engine wants one caller at a
 * time and its waits in submission order, so every engine call of the queue -- a submit or a wait -- is ONE libuv work item, and the
 * next one is chosen on the main thread when it completes: submit the oldest job not yet submitted while fewer than `inflight`
 * (setOption 'inflight', default 3) are inside the engine, otherwise wait for the oldest.  With three jobs queued the engine sees
 * submit(0) submit(1) submit(2) wait(0) submit(3) wait(1) ...  A handle with queued jobs is busy for every other call. */
static void stream_kick(napi_env env, Handle *h);
static void stream_execute(napi_env env, void *data) { /* worker thread: no N-API calls */
    Job *j = data;
    zk_pool *p = j->h->pool;
    if (j->op == 0) {
        if (j->verify) {
            j->rc = zk_pool_verify_submit(p, j->B, j->msg, j->proofs_in, j->off, j->len, j->seeds, j->ok, j->status, &j->pj);
        } else {
            zk_rng rng = {ZK_RNG_SEED, j->seeds, 0};
            j->rc = zk_pool_prove_submit(p, j->B, j->msg, j->sig, j->pk, j->which, &rng, j->out_ext, j->out_ext_cap, j->off, j->len, j->status, &j->pj);
        }
    } else {
        j->rc = j->verify ? zk_pool_verify_wait(p, j->pj) : zk_pool_prove_wait(p, j->pj);
    }
    if (j->rc != ZK_OK) snprintf(j->err, sizeof j->err, "%s: %s", zk_strerror(j->rc), zk_pool_last_error(p));
}
static napi_value stream_result(napi_env env, Job *j) {
    napi_value v, out = NULL;
    if (napi_create_object(env, &v) != napi_ok) return NULL;
    if (j->verify) {
        set_prop(env, v, "ok", new_buffer(env, j->ok, j->B));
    } else {
        uint64_t end = 0;
        for (size_t b = 0; b < j->B; b++)
            if (j->off[b] + j->len[b] > end) end = j->off[b] + j->len[b];
        napi_value used;
        if (napi_get_reference_value(env, j->out_ref, &out) != napi_ok || napi_create_double(env, (double)end, &used) != napi_ok) return NULL;
        set_prop(env, v, "proofs", out), set_prop(env, v, "used", used);
        set_prop(env, v, "offsets", new_buffer(env, j->off, 8 * j->B)), set_prop(env, v, "lengths", new_buffer(env, j->len, 8 * j->B));
    }
    set_prop(env, v, "status", new_buffer(env, j->status, 4 * j->B));
    return v;
}
static void stream_settle(napi_env env, Job *j, int ok) {
    napi_value v = ok ? stream_result(env, j) : NULL;
    if (v) {
        napi_resolve_deferred(env, j->deferred, v);
    } else {
        napi_value msg, e;
        napi_create_string_utf8(env, j->rc != ZK_OK ? j->err : "streamed batch failed", NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, NULL, msg, &e);
        napi_reject_deferred(env, j->deferred, e);
    }
    job_free(env, j);
}
static void stream_unlink(Handle *h, Job *j) {
    Job **pp = &h->sq_head, *prev = NULL;
    while (*pp && *pp != j) prev = *pp, pp = &(*pp)->next;
    if (*pp) *pp = j->next;
    if (h->sq_tail == j) h->sq_tail = prev;
}
static void stream_complete(napi_env env, napi_status status, void *data) { /* main thread */
    Job *j = data;
    Handle *h = j->h;
    h->sq_running = 0;
    napi_delete_async_work(env, j->work);
    int ok = status == napi_ok && j->rc == ZK_OK;
    if (j->op == 0 && ok) {
        j->submitted = 1, h->sq_submitted++;
    } else { /* a finished wait, or a submit the engine refused: the job leaves the queue */
        if (j->op == 1) h->sq_submitted--;
        stream_unlink(h, j);
        stream_settle(env, j, ok);
    }
    if (!h->sq_head) {
        h->busy = 0;
        if (h->orphaned) {
            handle_release(h);
            return;
        }
    }
    stream_kick(env, h);
}
static void stream_kick(napi_env env, Handle *h) {
    while (!h->sq_running && h->sq_head) {
        Job *u = h->sq_head;
        while (u && u->submitted) u = u->next;
        Job *j = u && (uint32_t)h->sq_submitted < (h->inflight ? h->inflight : 3) ? u : h->sq_head;
        j->op = j == u ? 0 : 1;
        napi_value rn;
        if (napi_create_string_utf8(env, "zkattest.stream", NAPI_AUTO_LENGTH, &rn) == napi_ok &&
            napi_create_async_work(env, NULL, rn, stream_execute, stream_complete, j, &j->work) == napi_ok) {
            if (napi_queue_async_work(env, j->work) == napi_ok) {
                h->sq_running = 1;
                return;
            }
            napi_delete_async_work(env, j->work);
        }
        /* could not queue: a job that is inside the engine has to be waited for here, the others are dropped */
        if (j->submitted) {
            j->rc = j->verify ? zk_pool_verify_wait(h->pool, j->pj) : zk_pool_prove_wait(h->pool, j->pj);
            h->sq_submitted--;
        }
        snprintf(j->err, sizeof j->err, "could not queue the streamed batch");
        j->rc = j->rc == ZK_OK ? ZK_E_BUFFER : j->rc;
        stream_unlink(h, j);
        stream_settle(env, j, 0);
    }
    if (!h->sq_head) h->busy = 0;
}
static napi_value stream_enqueue(napi_env env, Job *j, napi_value hv) {
    napi_value promise;
    Handle *h = j->h;
    if (napi_create_reference(env, hv, 1, &j->h_ref) != napi_ok || napi_create_promise(env, &j->deferred, &promise) != napi_ok) {
        job_free(env, j);
        return throw_text(env, ZK_E_BUFFER, "could not queue the streamed batch");
    }
    j->stream = 1;
    if (h->sq_tail) h->sq_tail->next = j;
    else h->sq_head = j;
    h->sq_tail = j;
    h->busy = 1;
    stream_kick(env, h);
    return promise;
}
/* a handle that is busy with streamed jobs accepts more of them; one that runs an exclusive batch does not */
static Handle *get_stream_handle(napi_env env, napi_value v) {
    Handle *h = get_handle(env, v, 1);
    if (h && h->busy && !h->sq_head) {
        napi_throw_error(env, NULL, "the engine is busy with an asynchronous batch (one batch at a time per engine)");
        return NULL;
    }
    return h;
}
/* (h, msg Bx32, sig Bx64, pk Bx64, which Bx4, seeds Bx32, out: page-locked Buffer from hostAlloc)
 *   -> Promise<{proofs: out, used: bytes, offsets, lengths, status}>; `out` belongs to the job until its Promise settles */
static napi_value ProveSubmit(napi_env env, napi_callback_info info) {
    napi_value argv[7];
    if (!get_args(env, info, 7, argv)) return NULL;
    Handle *h = get_stream_handle(env, argv[0]);
    uint8_t *msg, *sig, *pk, *which, *seeds, *out;
    size_t lm, ls, lp, lw, lse, lo;
    if (!h || !get_bytes(env, argv[1], &msg, &lm) || !get_bytes(env, argv[2], &sig, &ls) || !get_bytes(env, argv[3], &pk, &lp) ||
        !get_bytes(env, argv[4], &which, &lw) || !get_bytes(env, argv[5], &seeds, &lse) || !get_bytes(env, argv[6], &out, &lo))
        return NULL;
    size_t B = lm / 32;
    if (!B || lm != 32 * B || ls != 64 * B || lp != 64 * B || lw != 4 * B || lse != 32 * B || !out) {
        napi_throw_range_error(env, NULL, "proveSubmit: per proof 32-byte msgHash, 64-byte signature, 64-byte public key, u32 index, 32-byte seed; a page-locked output Buffer");
        return NULL;
    }
    Job *j = calloc(1, sizeof *j);
    if (!j) return throw_text(env, ZK_E_BUFFER, "out of memory");
    j->h = h, j->B = B, j->async = 1, j->out_ext = out, j->out_ext_cap = lo;
    j->msg = dup_bytes(msg, lm), j->sig = dup_bytes(sig, ls), j->pk = dup_bytes(pk, lp), j->seeds = dup_bytes(seeds, lse);
    j->which = (uint32_t *)dup_bytes(which, lw);
    j->off = malloc(8 * B), j->len = malloc(8 * B), j->status = malloc(4 * B);
    if (!j->msg || !j->sig || !j->pk || !j->seeds || !j->which || !j->off || !j->len || !j->status ||
        napi_create_reference(env, argv[6], 1, &j->out_ref) != napi_ok) {
        job_free(env, j);
        return throw_text(env, ZK_E_BUFFER, "out of memory");
    }
    return stream_enqueue(env, j, argv[0]);
}
/* (h, msg Bx32, proofs: page-locked Buffer, offsets, lengths, seeds | null) -> Promise<{ok, status}> */
static napi_value VerifySubmit(napi_env env, napi_callback_info info) {
    napi_value argv[6];
    if (!get_args(env, info, 6, argv)) return NULL;
    Handle *h = get_stream_handle(env, argv[0]);
    uint8_t *msg, *proofs, *offs, *lens, *seeds;
    size_t lm, lp, lo, ll, ls;
    if (!h || !get_bytes(env, argv[1], &msg, &lm) || !get_bytes(env, argv[2], &proofs, &lp) || !get_bytes(env, argv[3], &offs, &lo) ||
        !get_bytes(env, argv[4], &lens, &ll) || !get_bytes(env, argv[5], &seeds, &ls))
        return NULL;
    size_t B = lm / 32;
    if (!B || lm != 32 * B || lo != 8 * B || ll != 8 * B || (seeds && ls != 32 * B) || !proofs) {
        napi_throw_range_error(env, NULL, "verifySubmit: B message hashes, B offsets, B lengths, B seeds or null");
        return NULL;
    }
    Job *j = calloc(1, sizeof *j);
    if (!j) return throw_text(env, ZK_E_BUFFER, "out of memory");
    j->verify = 1, j->h = h, j->B = B, j->async = 1;
    j->msg = dup_bytes(msg, lm), j->off = (uint64_t *)dup_bytes(offs, lo), j->len = (uint64_t *)dup_bytes(lens, ll);
    j->seeds = seeds ? dup_bytes(seeds, ls) : NULL;
    j->ok = malloc(B), j->status = malloc(4 * B);
    j->proofs_in = proofs;
    int okk = j->msg && j->off && j->len && j->ok && j->status && (!seeds || j->seeds);
    for (size_t b = 0; okk && b < B; b++) okk = j->off[b] <= lp && j->len[b] <= lp - j->off[b];
    if (okk) okk = napi_create_reference(env, argv[2], 1, &j->proofs_ref) == napi_ok;
    if (!okk) {
        job_free(env, j);
        napi_throw_range_error(env, NULL, "verifySubmit: out of memory, or offsets / lengths beyond the proof buffer");
        return NULL;
    }
    return stream_enqueue(env, j, argv[0]);
}

static napi_value HostAlloc(napi_env env, napi_callback_info info) { /* (bytes) -> page-locked Buffer (zk_host_alloc) */
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return NULL;
    double n;
    NAPI_OK(napi_get_value_double(env, argv[0], &n));
    if (!(n >= 1) || n > 1e12) {
        napi_throw_range_error(env, NULL, "hostAlloc: size in bytes");
        return NULL;
    }
    void *p = zk_host_alloc((size_t)n);
    if (!p) return throw_text(env, ZK_E_BUFFER, "zk_host_alloc failed");
    napi_value b;
    if (napi_create_external_buffer(env, (size_t)n, p, slab_finalize, (void *)1, &b) != napi_ok) {
        zk_host_free(p);
        napi_throw_error(env, NULL, "could not wrap the page-locked buffer");
        return NULL;
    }
    return b;
}
static napi_value HardenedH(napi_env env, napi_callback_info info) { /* (tag: Buffer) -> {nistH, tomH}   zk_hardened_h: host-only */
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return NULL;
    uint8_t *tag;
    size_t lt;
    if (!get_bytes(env, argv[0], &tag, &lt)) return NULL;
    uint8_t a[64], b[72];
    zk_status st = zk_hardened_h(tag, lt, a, b);
    if (st != ZK_OK) return throw_text(env, st, "");
    napi_value o;
    NAPI_OK(napi_create_object(env, &o));
    set_prop(env, o, "nistH", new_buffer(env, a, 64)), set_prop(env, o, "tomH", new_buffer(env, b, 72));
    return o;
}
static napi_value ProofToJson(napi_env env, napi_callback_info info) { /* (proof: Buffer) -> string   (writeJson, src/serde.ts:34-36) */
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return NULL;
    uint8_t *p;
    size_t lp;
    if (!get_bytes(env, argv[0], &p, &lp)) return NULL;
    uint64_t n = 0, cap = 5 * (uint64_t)lp + 4096;   /* the text is ~3.5x the binary proof: one conversion in the common case */
    char *s = xmalloc(env, cap + 1);
    if (!s) return NULL;
    zk_status st = zk_proof_to_json(p, lp, s, cap, &n);
    if (st == ZK_E_BUFFER) {
        free(s);
        s = xmalloc(env, n + 1);
        if (!s) return NULL;
        st = zk_proof_to_json(p, lp, s, n, &n);
    }
    napi_value r = NULL;
    if (st == ZK_OK) napi_create_string_utf8(env, s, n, &r);
    free(s);
    return st == ZK_OK ? r : throw_text(env, st, "");
}
static napi_value ProofFromJson(napi_env env, napi_callback_info info) { /* (text: string) -> Buffer   (readJson, src/serde.ts:21-32) */
    napi_value argv[1];
    if (!get_args(env, info, 1, argv)) return NULL;
    size_t len = 0;
    NAPI_OK(napi_get_value_string_utf8(env, argv[0], NULL, 0, &len));
    if (len > ((size_t)64 << 20)) return throw_text(env, ZK_E_BAD_ENCODING, "JSON text too long");
    char *s = xmalloc(env, len + 1);
    if (!s) return NULL;
    if (napi_get_value_string_utf8(env, argv[0], s, len + 1, &len) != napi_ok) {
        free(s);
        napi_throw_type_error(env, NULL, "expected a string");
        return NULL;
    }
    uint64_t n = 0, cap = len / 2 + 64;   /* at least two hex digits per byte: the binary proof is shorter than half the text */
    napi_value r = NULL;
    uint8_t *b = malloc(cap + 1);
    zk_status st = b ? zk_proof_from_json(s, len, b, cap, &n) : ZK_E_BUFFER;
    if (b && st == ZK_E_BUFFER && n > cap) {
        free(b);
        b = malloc(n + 1);
        st = b ? zk_proof_from_json(s, len, b, n, &n) : ZK_E_BUFFER;
    }
    if (st == ZK_OK) r = new_buffer(env, b, n);
    free(b);
    free(s);
    return st == ZK_OK && r ? r : throw_text(env, st ? st : ZK_E_BUFFER, "");
}
static napi_value KeysToInts(napi_env env, napi_callback_info info) { /* (h, pk: n x 64 bytes) -> {keys: n x 32, status}  (keyToInt) */
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *pk;
    size_t lp;
    if (!h || !get_bytes(env, argv[1], &pk, &lp)) return NULL;
    size_t n = lp / 64;
    uint8_t *keys = malloc(32 * n + 1);
    int32_t *status = malloc(4 * n + 4);
    zk_ctx *ctx = zk_pool_ctx(h->pool, 0);
    zk_status st = keys && status ? zk_keys_to_ints(ctx, n, pk, keys, status) : ZK_E_BUFFER;
    napi_value o = NULL;
    if (st == ZK_OK && napi_create_object(env, &o) == napi_ok) set_prop(env, o, "keys", new_buffer(env, keys, 32 * n)), set_prop(env, o, "status", new_buffer(env, status, 4 * n));
    free(keys), free(status);
    return st == ZK_OK ? o : throw_text(env, st, zk_last_error(ctx));
}

/* ---- whole batches of proofs <-> JSON texts on every host core (zk_proofs_to_json_batch / zk_proofs_from_json_batch), off the event
 * loop: (blob: Buffer, offsets: Buffer of n + 1 u64 LE, threads) -> Promise<{ blob, offsets, status }>.  `to` = 1: ZKA1 -> JSON. */
typedef struct {
    int to;
    uint64_t n;
    uint8_t *in;
    uint64_t *in_off;
    uint32_t threads;
    uint8_t *out;
    uint64_t out_cap, *out_off;
    int32_t *status;
    zk_status rc;
    napi_ref in_ref, off_ref;
    napi_deferred deferred;
    napi_async_work work;
} JsonJob;
static void json_job_free(napi_env env, JsonJob *j) {
    if (j->in_ref) napi_delete_reference(env, j->in_ref);
    if (j->off_ref) napi_delete_reference(env, j->off_ref);
    free(j->out), free(j->out_off), free(j->status), free(j);
}
static void json_execute(napi_env env, void *data) { /* worker thread: no N-API calls */
    JsonJob *j = data;
    for (int pass = 0; pass < 2; pass++) {
        j->rc = j->to ? zk_proofs_to_json_batch(j->n, j->in, j->in_off, (char *)j->out, j->out_cap, j->out_off, j->status, j->threads)
                      : zk_proofs_from_json_batch(j->n, (const char *)j->in, j->in_off, j->out, j->out_cap, j->out_off, j->status, j->threads);
        if (j->rc != ZK_E_BUFFER) break;
        free(j->out);                       /* the offsets are complete: come back with the exact size */
        j->out_cap = j->out_off[j->n] + 64;
        j->out = malloc(j->out_cap);
        if (!j->out) break;
    }
}
static void json_complete(napi_env env, napi_status status, void *data) { /* main thread */
    JsonJob *j = data;
    napi_value v = NULL, b = NULL;
    if (status == napi_ok && j->rc == ZK_OK && napi_create_object(env, &v) == napi_ok) {
        uint64_t len = j->out_off[j->n];
        if (napi_create_external_buffer(env, (size_t)len, j->out, slab_finalize, NULL, &b) == napi_ok) j->out = NULL; /* ownership moved */
        else b = new_buffer(env, j->out, (size_t)len);
        set_prop(env, v, "blob", b);
        set_prop(env, v, "offsets", new_buffer(env, j->out_off, 8 * (j->n + 1)));
        set_prop(env, v, "status", new_buffer(env, j->status, 4 * j->n));
        napi_resolve_deferred(env, j->deferred, v);
    } else {
        napi_value msg, e;
        napi_create_string_utf8(env, "batch JSON conversion failed", NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, NULL, msg, &e);
        napi_reject_deferred(env, j->deferred, e);
    }
    napi_delete_async_work(env, j->work);
    json_job_free(env, j);
}
static napi_value json_batch(napi_env env, napi_callback_info info, int to) {
    napi_value argv[3], promise, rn;
    if (!get_args(env, info, 3, argv)) return NULL;
    uint8_t *in, *off;
    size_t li, lo;
    uint32_t threads = 0;
    if (!get_bytes(env, argv[0], &in, &li) || !get_bytes(env, argv[1], &off, &lo) || napi_get_value_uint32(env, argv[2], &threads) != napi_ok || lo < 8 || lo % 8) {
        napi_throw_type_error(env, NULL, "expected (blob: Buffer, offsets: Buffer of n + 1 u64, threads: number)");
        return NULL;
    }
    JsonJob *j = calloc(1, sizeof *j);
    if (!j) return throw_text(env, ZK_E_BUFFER, "out of memory");
    j->to = to, j->n = lo / 8 - 1, j->in = in, j->in_off = (uint64_t *)off, j->threads = threads;
    if (j->in_off[j->n] > li) {
        free(j);
        napi_throw_range_error(env, NULL, "offsets run past the blob");
        return NULL;
    }
    j->out_cap = to ? 4 * (uint64_t)li + 4096 * (j->n + 1) : (uint64_t)li / 3 + 64 * (j->n + 1);
    j->out = malloc(j->out_cap), j->out_off = malloc(8 * (j->n + 1)), j->status = malloc(4 * (j->n ? j->n : 1));
    if (!j->out || !j->out_off || !j->status || napi_create_reference(env, argv[0], 1, &j->in_ref) != napi_ok ||
        napi_create_reference(env, argv[1], 1, &j->off_ref) != napi_ok || napi_create_promise(env, &j->deferred, &promise) != napi_ok ||
        napi_create_string_utf8(env, to ? "zkattest:toJsonBatch" : "zkattest:fromJsonBatch", NAPI_AUTO_LENGTH, &rn) != napi_ok ||
        napi_create_async_work(env, NULL, rn, json_execute, json_complete, j, &j->work) != napi_ok || napi_queue_async_work(env, j->work) != napi_ok) {
        json_job_free(env, j);
        napi_throw_error(env, NULL, "could not queue the conversion");
        return NULL;
    }
    return promise;
}
static napi_value ProofsToJsonBatch(napi_env env, napi_callback_info info) { return json_batch(env, info, 1); }
static napi_value ProofsFromJsonBatch(napi_env env, napi_callback_info info) { return json_batch(env, info, 0); }

/* (h, msg, sig, pk, which: B u32 LE or null, ringIds: B u32 LE) -> {which: B u32 LE, flags: B u32 LE}: zk_screen_batch_rings on the pool's first context (the
 * screen has no pool form: it costs a few dozen point additions per witness and reads the resident rings, which every shard holds under the same ids) */
static napi_value ScreenBatchRings(napi_env env, napi_callback_info info) {
    napi_value argv[6];
    if (!get_args(env, info, 6, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *msg, *sig, *pk, *wb, *ib;
    size_t lm, ls, lp, lw, li;
    if (!h || !get_bytes(env, argv[1], &msg, &lm) || !get_bytes(env, argv[2], &sig, &ls) || !get_bytes(env, argv[3], &pk, &lp) || !get_bytes(env, argv[4], &wb, &lw) ||
        !get_bytes(env, argv[5], &ib, &li))
        return NULL;
    const size_t B = lm / 32;
    if (lm % 32 || ls != 64 * B || lp != 64 * B || (wb && lw != 4 * B) || li != 4 * B) {
        napi_throw_range_error(env, NULL, "screenBatchRings: 32 bytes of hash, 64 of signature, 64 of key and one ring id per witness (and one index each, or null)");
        return NULL;
    }
    /* (a Buffer's bytes need not be 4-byte aligned) */
    uint32_t *buf = (uint32_t *)xmalloc(env, 16 * B);
    if (!buf) return NULL;
    uint32_t *which = buf, *ids = buf + B, *wo = buf + 2 * B, *fl = buf + 3 * B;
    if (wb) memcpy(which, wb, 4 * B);
    if (B) memcpy(ids, ib, 4 * B);
    zk_status st = zk_screen_batch_rings(zk_pool_ctx(h->pool, 0), B, msg, sig, pk, wb ? which : NULL, ids, wo, fl);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(zk_pool_ctx(h->pool, 0)));
    else if (napi_create_object(env, &v) == napi_ok) set_prop(env, v, "which", new_buffer(env, wo, 4 * B)), set_prop(env, v, "flags", new_buffer(env, fl, 4 * B));
    free(buf);
    return v;
}

/* (h, msg, sig, ringIds: B u32 LE) -> {pk: B x 64 (zeros where flags != 0), which: B u32 LE, flags: B u32 LE}: zk_recover_batch_rings on the pool's first
 * context, like the screen (no pool form) */
static napi_value RecoverBatchRings(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *msg, *sig, *ib;
    size_t lm, ls, li;
    if (!h || !get_bytes(env, argv[1], &msg, &lm) || !get_bytes(env, argv[2], &sig, &ls) || !get_bytes(env, argv[3], &ib, &li)) return NULL;
    const size_t B = lm / 32;
    if (lm % 32 || ls != 64 * B || li != 4 * B) {
        napi_throw_range_error(env, NULL, "recoverBatchRings: 32 bytes of hash, 64 of signature and one ring id per witness");
        return NULL;
    }
    /* (a Buffer's bytes need not be 4-byte aligned) */
    uint32_t *buf = (uint32_t *)xmalloc(env, 12 * B + 64 * B + 4);
    if (!buf) return NULL;
    uint32_t *ids = buf, *wo = buf + B, *fl = buf + 2 * B;
    uint8_t *pk = (uint8_t *)(buf + 3 * B);
    if (B) memcpy(ids, ib, 4 * B);
    zk_status st = zk_recover_batch_rings(zk_pool_ctx(h->pool, 0), B, msg, sig, ids, pk, wo, fl);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(zk_pool_ctx(h->pool, 0)));
    else if (napi_create_object(env, &v) == napi_ok)
        set_prop(env, v, "pk", new_buffer(env, pk, 64 * B)), set_prop(env, v, "which", new_buffer(env, wo, 4 * B)), set_prop(env, v, "flags", new_buffer(env, fl, 4 * B));
    free(buf);
    return v;
}

/* Ring membership on its own (include/zkattest.h: zk_member_*), on the pool's first context like the screen (no pool form); the active ring is the facade's.
 * (h) -> bytes of one ZKM1 proof over the active ring */
static napi_value MemberProofSize(napi_env env, napi_callback_info info) {
    napi_value argv[1], v = NULL;
    if (!get_args(env, info, 1, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    if (!h) return NULL;
    napi_create_double(env, (double)zk_member_proof_size(zk_pool_ctx(h->pool, 0)), &v);
    return v;
}
/* The bound forms ("ZKMB", zk_member_*_bound) take one more argument behind the unbound call's: context, B x 32 bytes.  A missing or misfitting context is a
 * RangeError here; the C ABI never sees a NULL context from this addon. */
static int get_context(napi_env env, napi_value v, size_t B, uint8_t **ctx, const char *what) {
    static uint8_t none[32];   /* B = 0: an empty Buffer may have no address; the call reads no byte of it */
    size_t lc;
    if (!get_bytes(env, v, ctx, &lc)) return 0;
    if (lc != 32 * B || (B && !*ctx)) {
        napi_throw_range_error(env, NULL, what);
        return 0;
    }
    if (!*ctx) *ctx = none;
    return 1;
}
/* (h, which: B u32 LE, blinders: B x 32 or null, seeds: B x 32[, context: B x 32]) -> {proofs: B x size (zeros where status != 0), coms: B x 72, blinders: B x 32,
 * status: B i32 LE} */
static napi_value member_prove(napi_env env, napi_callback_info info, int bound) {
    napi_value argv[5];
    if (!get_args(env, info, bound ? 5 : 4, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *wb, *bl, *seeds, *ctx = NULL;
    size_t lw, lb, ls;
    if (!h || !get_bytes(env, argv[1], &wb, &lw) || !get_bytes(env, argv[2], &bl, &lb) || !get_bytes(env, argv[3], &seeds, &ls)) return NULL;
    const size_t B = lw / 4;
    if (lw % 4 || (bl && lb != 32 * B) || ls != 32 * B) {
        napi_throw_range_error(env, NULL, "memberProveBatch: one u32 index and 32 seed bytes per proof (and 32 blinder bytes each, or null)");
        return NULL;
    }
    if (bound && !get_context(env, argv[4], B, &ctx, "memberProveBatchBound: 32 context bytes per proof")) return NULL;
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    const uint64_t size = zk_member_proof_size(c);
    uint8_t *buf = (uint8_t *)xmalloc(env, (size + 72 + 32 + 8) * B + 8);   /* (a Buffer's bytes need not be 4-byte aligned: the indices are copied) */
    if (!buf) return NULL;
    uint32_t *which = (uint32_t *)buf;
    int32_t *status = (int32_t *)(buf + 4 * B);
    uint8_t *out = buf + 8 * B, *com = out + size * B, *bo = com + 72 * B;
    if (B) memcpy(which, wb, 4 * B);
    zk_rng rng = {ZK_RNG_SEED, seeds, 0};
    zk_status st = bound ? zk_member_prove_batch_bound(c, B, which, ctx, bl, &rng, com, bo, out, size * B, status)
                         : zk_member_prove_batch(c, B, which, bl, &rng, com, bo, out, size * B, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) {
        set_prop(env, v, "proofs", new_buffer(env, out, size * B)), set_prop(env, v, "coms", new_buffer(env, com, 72 * B));
        set_prop(env, v, "blinders", new_buffer(env, bo, 32 * B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    }
    memset(buf, 0, (size + 72 + 32 + 8) * B + 8);   /* the blinders */
    free(buf);
    return v;
}
static napi_value MemberProveBatch(napi_env env, napi_callback_info info) { return member_prove(env, info, 0); }
static napi_value MemberProveBatchBound(napi_env env, napi_callback_info info) { return member_prove(env, info, 1); }
/* (h, coms: B x 72, proofs: B x size[, context: B x 32]) -> {ok: B bytes, status: B i32 LE} */
static napi_value member_verify(napi_env env, napi_callback_info info, int bound) {
    napi_value argv[4];
    if (!get_args(env, info, bound ? 4 : 3, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *com, *proofs, *ctx = NULL;
    size_t lc, lp;
    if (!h || !get_bytes(env, argv[1], &com, &lc) || !get_bytes(env, argv[2], &proofs, &lp)) return NULL;
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    const uint64_t size = zk_member_proof_size(c);
    const size_t B = lc / 72;
    if (lc % 72 || !size || lp != size * B) {
        napi_throw_range_error(env, NULL, "memberVerifyBatch: one 72-byte commitment and one proof of the active ring's size per entry");
        return NULL;
    }
    if (bound && !get_context(env, argv[3], B, &ctx, "memberVerifyBatchBound: 32 context bytes per proof")) return NULL;
    uint8_t *buf = (uint8_t *)xmalloc(env, 5 * B + 8);
    if (!buf) return NULL;
    int32_t *status = (int32_t *)buf;
    uint8_t *ok = buf + 4 * B;
    zk_status st = bound ? zk_member_verify_batch_bound(c, B, com, ctx, proofs, NULL, ok, status) : zk_member_verify_batch(c, B, com, proofs, NULL, ok, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) set_prop(env, v, "ok", new_buffer(env, ok, B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}
static napi_value MemberVerifyBatch(napi_env env, napi_callback_info info) { return member_verify(env, info, 0); }
static napi_value MemberVerifyBatchBound(napi_env env, napi_callback_info info) { return member_verify(env, info, 1); }

/* ... with one resident ring id per entry (zk_member_*_batch_rings); the active ring plays no part.
 * (h, ring id) -> bytes of one ZKM1 proof over that resident ring, 0 for an id that is not resident */
static napi_value MemberProofSizeRing(napi_env env, napi_callback_info info) {
    napi_value argv[2], v = NULL;
    if (!get_args(env, info, 2, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint32_t id = 0;
    if (!h || napi_get_value_uint32(env, argv[1], &id) != napi_ok) return NULL;
    napi_create_double(env, (double)zk_member_proof_size_ring(zk_pool_ctx(h->pool, 0), id), &v);
    return v;
}
/* (h, which: B u32 LE, ring ids: B u32 LE, blinders: B x 32 or null, seeds: B x 32[, context: B x 32]) -> {proofs: the batch's bytes back to back, off: B+1 u64 LE,
 * coms: B x 72, blinders: B x 32, status: B i32 LE} */
static napi_value member_prove_rings(napi_env env, napi_callback_info info, int bound) {
    napi_value argv[6];
    if (!get_args(env, info, bound ? 6 : 5, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *wb, *ib, *bl, *seeds, *ctx = NULL;
    size_t lw, li, lb, ls;
    if (!h || !get_bytes(env, argv[1], &wb, &lw) || !get_bytes(env, argv[2], &ib, &li) || !get_bytes(env, argv[3], &bl, &lb) || !get_bytes(env, argv[4], &seeds, &ls)) return NULL;
    const size_t B = lw / 4;
    if (lw % 4 || li != lw || (bl && lb != 32 * B) || ls != 32 * B) {
        napi_throw_range_error(env, NULL, "memberProveBatchRings: one u32 index, one u32 ring id and 32 seed bytes per proof (and 32 blinder bytes each, or null)");
        return NULL;
    }
    if (bound && !get_context(env, argv[5], B, &ctx, "memberProveBatchRingsBound: 32 context bytes per proof")) return NULL;
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    uint64_t total = 0;   /* (a Buffer's bytes need not be 4-byte aligned: indices and ids are copied) */
    for (size_t b = 0; b < B; b++) {
        uint32_t id;
        memcpy(&id, ib + 4 * b, 4);
        total += zk_member_proof_size_ring(c, id);
    }
    const size_t bytes = 8 * (B + 1) + (72 + 32 + 12) * B + total + 8;
    uint8_t *buf = (uint8_t *)xmalloc(env, bytes);
    if (!buf) return NULL;
    uint64_t *off = (uint64_t *)buf;
    uint32_t *which = (uint32_t *)(buf + 8 * (B + 1)), *ids = which + B;
    int32_t *status = (int32_t *)(ids + B);
    uint8_t *com = (uint8_t *)(status + B), *bo = com + 72 * B, *out = bo + 32 * B;
    if (B) memcpy(which, wb, 4 * B), memcpy(ids, ib, 4 * B);
    zk_rng rng = {ZK_RNG_SEED, seeds, 0};
    zk_status st = bound ? zk_member_prove_batch_rings_bound(c, B, which, ctx, ids, bl, &rng, com, bo, out, total, off, status)
                         : zk_member_prove_batch_rings(c, B, which, ids, bl, &rng, com, bo, out, total, off, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) {
        set_prop(env, v, "proofs", new_buffer(env, out, off[B])), set_prop(env, v, "off", new_buffer(env, off, 8 * (B + 1))), set_prop(env, v, "coms", new_buffer(env, com, 72 * B));
        set_prop(env, v, "blinders", new_buffer(env, bo, 32 * B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    }
    memset(buf, 0, bytes);   /* the blinders */
    free(buf);
    return v;
}
static napi_value MemberProveBatchRings(napi_env env, napi_callback_info info) { return member_prove_rings(env, info, 0); }
static napi_value MemberProveBatchRingsBound(napi_env env, napi_callback_info info) { return member_prove_rings(env, info, 1); }
/* (h, coms: B x 72, proofs: the batch's bytes, off: B+1 u64 LE, ring ids: B u32 LE[, context: B x 32]) -> {ok: B bytes, status: B i32 LE} */
static napi_value member_verify_rings(napi_env env, napi_callback_info info, int bound) {
    napi_value argv[6];
    if (!get_args(env, info, bound ? 6 : 5, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *com, *proofs, *ob, *ib, *ctx = NULL;
    size_t lc, lp, lo, li;
    if (!h || !get_bytes(env, argv[1], &com, &lc) || !get_bytes(env, argv[2], &proofs, &lp) || !get_bytes(env, argv[3], &ob, &lo) || !get_bytes(env, argv[4], &ib, &li)) return NULL;
    const size_t B = lc / 72;
    uint64_t last = 0;
    if (lo == 8 * (B + 1)) memcpy(&last, ob + 8 * B, 8);
    if (lc % 72 || lo != 8 * (B + 1) || li != 4 * B || last != lp) {
        napi_throw_range_error(env, NULL, "memberVerifyBatchRings: one 72-byte commitment and one ring id per entry, B + 1 offsets that end at the proofs' length");
        return NULL;
    }
    if (bound && !get_context(env, argv[5], B, &ctx, "memberVerifyBatchRingsBound: 32 context bytes per proof")) return NULL;
    uint8_t *buf = (uint8_t *)xmalloc(env, 8 * (B + 1) + 9 * B + lp + 8);
    if (!buf) return NULL;
    uint64_t *off = (uint64_t *)buf;
    uint32_t *ids = (uint32_t *)(buf + 8 * (B + 1));
    int32_t *status = (int32_t *)(ids + B);
    uint8_t *ok = (uint8_t *)(status + B), *pr = ok + B + (4 - B % 4) % 4;   /* (the slots' alignment is judged from offset 0: a copy that starts on a word) */
    memcpy(off, ob, 8 * (B + 1));
    if (B) memcpy(ids, ib, 4 * B);
    if (lp) memcpy(pr, proofs, lp);
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    zk_status st = bound ? zk_member_verify_batch_rings_bound(c, B, com, ctx, pr, off, ids, NULL, ok, status)
                         : zk_member_verify_batch_rings(c, B, com, pr, off, ids, NULL, ok, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) set_prop(env, v, "ok", new_buffer(env, ok, B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}
static napi_value MemberVerifyBatchRings(napi_env env, napi_callback_info info) { return member_verify_rings(env, info, 0); }
static napi_value MemberVerifyBatchRingsBound(napi_env env, napi_callback_info info) { return member_verify_rings(env, info, 1); }

/* Re-ring (include/zkattest.h: zk_prove_key_blinders, zk_proof_rering_batch), on the pool's first context like the member calls; the target is the ACTIVE ring,
 * which the facade made so.  (h, seeds: B x 32) -> blinders: B x 32, keyXcom's blinder of the proof made from each seed */
static napi_value KeyBlinders(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *seeds;
    size_t ls;
    if (!h || !get_bytes(env, argv[1], &seeds, &ls)) return NULL;
    const size_t B = ls / 32;
    if (ls % 32) {
        napi_throw_range_error(env, NULL, "keyBlinders: 32 seed bytes per proof");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    uint8_t *out = (uint8_t *)xmalloc(env, 32 * B + 8);
    if (!out) return NULL;
    zk_rng rng = {ZK_RNG_SEED, seeds, 0};
    zk_status st = zk_prove_key_blinders(c, B, &rng, out);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else v = new_buffer(env, out, 32 * B);
    memset(out, 0, 32 * B + 8);
    free(out);
    return v;
}
/* (h, msg: B x 32, proofs: the B proofs back to back, off: (B + 1) u64 LE, whichNew: B u32 LE, blinders: B x 32, seeds: B x 32 -- FRESH) ->
 * {proofs: the re-ringed proofs back to back, off: (B + 1) u64 LE, status: B i32 LE} */
static napi_value ReringBatch(napi_env env, napi_callback_info info) {
    napi_value argv[7];
    if (!get_args(env, info, 7, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *msg, *blob, *ob, *wb, *bl, *seeds;
    size_t lm, lp, lo, lw, lb, ls;
    if (!h || !get_bytes(env, argv[1], &msg, &lm) || !get_bytes(env, argv[2], &blob, &lp) || !get_bytes(env, argv[3], &ob, &lo) || !get_bytes(env, argv[4], &wb, &lw) ||
        !get_bytes(env, argv[5], &bl, &lb) || !get_bytes(env, argv[6], &seeds, &ls))
        return NULL;
    const size_t B = lw / 4;
    if (lw % 4 || lm != 32 * B || lb != 32 * B || ls != 32 * B || lo != 8 * (B + 1)) {
        napi_throw_range_error(env, NULL, "reringBatch: per proof 32 message bytes, one u32 index, 32 blinder bytes and 32 seed bytes; B + 1 offsets");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    const uint64_t cap = lp + B * zk_member_proof_size(c);   /* every head as it is plus a new GKProof section */
    const size_t small = 8 * (B + 1) * 2 + 8 * B;
    uint8_t *buf = (uint8_t *)xmalloc(env, small + cap + 8);   /* (a Buffer's bytes need not be aligned: offsets and indices are copied) */
    if (!buf) return NULL;
    uint64_t *off = (uint64_t *)buf, *out_off = off + (B + 1);
    uint32_t *which = (uint32_t *)(out_off + (B + 1));
    int32_t *status = (int32_t *)(which + B);
    uint8_t *out = buf + small;
    memcpy(off, ob, 8 * (B + 1));
    if (B) memcpy(which, wb, 4 * B);
    zk_rng rng = {ZK_RNG_SEED, seeds, 0};
    zk_status st = zk_proof_rering_batch(c, B, msg, blob, off, which, bl, &rng, out, cap, out_off, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) {
        set_prop(env, v, "proofs", new_buffer(env, out, (size_t)out_off[B])), set_prop(env, v, "off", new_buffer(env, out_off, 8 * (B + 1)));
        set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    }
    free(buf);
    return v;
}

/* zk_proof_rering_batch_rings: (h, msg: B x 32, proofs: the B proofs back to back, off: (B + 1) u64 LE, whichNew: B u32 LE, ringIds: B u32 LE -- resident rings,
 * blinders: B x 32, seeds: B x 32 -- FRESH) -> {proofs: every slot back to back (a proof that failed behind the header checks keeps a slot of zero bytes),
 * off: (B + 1) u64 LE, status: B i32 LE}.  The active ring is neither read nor changed. */
static napi_value ReringBatchRings(napi_env env, napi_callback_info info) {
    napi_value argv[8];
    if (!get_args(env, info, 8, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *msg, *blob, *ob, *wb, *ib, *bl, *seeds;
    size_t lm, lp, lo, lw, li, lb, ls;
    if (!h || !get_bytes(env, argv[1], &msg, &lm) || !get_bytes(env, argv[2], &blob, &lp) || !get_bytes(env, argv[3], &ob, &lo) || !get_bytes(env, argv[4], &wb, &lw) ||
        !get_bytes(env, argv[5], &ib, &li) || !get_bytes(env, argv[6], &bl, &lb) || !get_bytes(env, argv[7], &seeds, &ls))
        return NULL;
    const size_t B = lw / 4;
    if (lw % 4 || li != 4 * B || lm != 32 * B || lb != 32 * B || ls != 32 * B || lo != 8 * (B + 1)) {
        napi_throw_range_error(env, NULL, "reringBatchRings: per proof 32 message bytes, one u32 index, one u32 ring id, 32 blinder bytes and 32 seed bytes; B + 1 offsets");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    const size_t small = 8 * (B + 1) * 2 + 12 * B;
    uint32_t *ids_tmp = (uint32_t *)xmalloc(env, 4 * B + 8);
    if (!ids_tmp) return NULL;
    if (B) memcpy(ids_tmp, ib, 4 * B);
    uint64_t cap = lp;   /* every head as it is plus a new GKProof section of its destination ring's size */
    for (size_t b = 0; b < B; b++) cap += zk_member_proof_size_ring(c, ids_tmp[b]);
    uint8_t *buf = (uint8_t *)xmalloc(env, small + cap + 8);   /* (a Buffer's bytes need not be aligned: offsets, indices and ids are copied) */
    if (!buf) {
        free(ids_tmp);
        return NULL;
    }
    uint64_t *off = (uint64_t *)buf, *out_off = off + (B + 1);
    uint32_t *which = (uint32_t *)(out_off + (B + 1)), *ids = which + B;
    int32_t *status = (int32_t *)(ids + B);
    uint8_t *out = buf + small;
    memcpy(off, ob, 8 * (B + 1));
    if (B) memcpy(which, wb, 4 * B), memcpy(ids, ids_tmp, 4 * B);
    free(ids_tmp);
    zk_rng rng = {ZK_RNG_SEED, seeds, 0};
    zk_status st = zk_proof_rering_batch_rings(c, B, msg, blob, off, which, ids, bl, &rng, out, cap, out_off, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) {
        set_prop(env, v, "proofs", new_buffer(env, out, (size_t)out_off[B])), set_prop(env, v, "off", new_buffer(env, out_off, 8 * (B + 1)));
        set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    }
    free(buf);
    return v;
}

/* Link proofs (include/zkattest.h: zk_link_*, zk_proof_key_commitments), on the pool's first context like the member calls; no ring takes part.
 * (h, keys: B x 32, com1: B x 72, blinder1: B x 32, com2: B x 72, blinder2: B x 32, seeds: B x 32 -- FRESH) -> {proofs: B x 256 (zeros where status != 0),
 * status: B i32 LE} */
static napi_value LinkProveBatch(napi_env env, napi_callback_info info) {
    napi_value argv[7];
    if (!get_args(env, info, 7, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *key, *c1, *b1, *c2, *b2, *seeds;
    size_t lk, lc1, lb1, lc2, lb2, ls;
    if (!h || !get_bytes(env, argv[1], &key, &lk) || !get_bytes(env, argv[2], &c1, &lc1) || !get_bytes(env, argv[3], &b1, &lb1) || !get_bytes(env, argv[4], &c2, &lc2) ||
        !get_bytes(env, argv[5], &b2, &lb2) || !get_bytes(env, argv[6], &seeds, &ls))
        return NULL;
    const size_t B = lk / 32;
    if (lk % 32 || lc1 != 72 * B || lb1 != 32 * B || lc2 != 72 * B || lb2 != 32 * B || ls != 32 * B) {
        napi_throw_range_error(env, NULL, "linkProveBatch: per proof a 32-byte key, two 72-byte commitments, two 32-byte blinders and 32 seed bytes");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    const uint64_t size = zk_link_proof_size();
    uint8_t *buf = (uint8_t *)xmalloc(env, (size + 4) * B + 8);
    if (!buf) return NULL;
    int32_t *status = (int32_t *)buf;
    uint8_t *out = buf + 4 * B;
    zk_rng rng = {ZK_RNG_SEED, seeds, 0};
    zk_status st = zk_link_prove_batch(c, B, key, c1, b1, c2, b2, &rng, out, size * B, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) set_prop(env, v, "proofs", new_buffer(env, out, size * B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}
/* (h, com1: B x 72, com2: B x 72, proofs: B x 256) -> {ok: B bytes, status: B i32 LE} */
static napi_value LinkVerifyBatch(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *c1, *c2, *proofs;
    size_t lc1, lc2, lp;
    if (!h || !get_bytes(env, argv[1], &c1, &lc1) || !get_bytes(env, argv[2], &c2, &lc2) || !get_bytes(env, argv[3], &proofs, &lp)) return NULL;
    const size_t B = lc1 / 72;
    if (lc1 % 72 || lc2 != 72 * B || lp != zk_link_proof_size() * B) {
        napi_throw_range_error(env, NULL, "linkVerifyBatch: two 72-byte commitments and one 256-byte proof per entry");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    uint8_t *buf = (uint8_t *)xmalloc(env, 5 * B + 8);
    if (!buf) return NULL;
    int32_t *status = (int32_t *)buf;
    uint8_t *ok = buf + 4 * B;
    zk_status st = zk_link_verify_batch(c, B, c1, c2, proofs, ok, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) set_prop(env, v, "ok", new_buffer(env, ok, B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}
/* Escrow tags (include/zkattest.h: zk_ctx_set_auditor, zk_escrow_*), on the pool's first context like the link calls; only the opening reads the active ring.
 * (h, auditor: 72) -> undefined */
static napi_value SetAuditor(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *key;
    size_t lk;
    if (!h || !get_bytes(env, argv[1], &key, &lk)) return NULL;
    if (lk != 72) {
        napi_throw_range_error(env, NULL, "setAuditor: a 72-byte Tom-256 point");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    zk_status st = zk_ctx_set_auditor(c, key);
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    return NULL;
}
/* (h, secret: 32) -> the auditor's key a g: 72 bytes */
static napi_value EscrowKeygen(napi_env env, napi_callback_info info) {
    napi_value argv[2];
    if (!get_args(env, info, 2, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *secret, key[72];
    size_t ls;
    if (!h || !get_bytes(env, argv[1], &secret, &ls)) return NULL;
    if (ls != 32) {
        napi_throw_range_error(env, NULL, "escrowKeygen: a 32-byte secret");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    zk_status st = zk_escrow_keygen(c, secret, key);
    if (st != ZK_OK) {
        throw_text(env, st, zk_last_error(c));
        return NULL;
    }
    return new_buffer(env, key, 72);
}
/* (h, keys: B x 32, com: B x 72, blinder: B x 32, seeds: B x 32 -- FRESH) -> {tags: B x 472 (zeros where status != 0), status: B i32 LE} */
static napi_value EscrowProveBatch(napi_env env, napi_callback_info info) {
    napi_value argv[5];
    if (!get_args(env, info, 5, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *key, *com, *bl, *seeds;
    size_t lk, lc, lb, ls;
    if (!h || !get_bytes(env, argv[1], &key, &lk) || !get_bytes(env, argv[2], &com, &lc) || !get_bytes(env, argv[3], &bl, &lb) || !get_bytes(env, argv[4], &seeds, &ls)) return NULL;
    const size_t B = lk / 32;
    if (lk % 32 || lc != 72 * B || lb != 32 * B || ls != 32 * B) {
        napi_throw_range_error(env, NULL, "escrowProveBatch: per tag a 32-byte key, a 72-byte commitment, a 32-byte blinder and 32 seed bytes");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    const uint64_t size = zk_escrow_tag_size();
    uint8_t *buf = (uint8_t *)xmalloc(env, (size + 4) * B + 8);
    if (!buf) return NULL;
    int32_t *status = (int32_t *)buf;
    uint8_t *out = buf + 4 * B;
    zk_rng rng = {ZK_RNG_SEED, seeds, 0};
    zk_status st = zk_escrow_prove_batch(c, B, key, com, bl, &rng, out, size * B, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) set_prop(env, v, "tags", new_buffer(env, out, size * B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}
/* (h, com: B x 72, tags: B x 472) -> {ok: B bytes, status: B i32 LE} */
static napi_value EscrowVerifyBatch(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *com, *tags;
    size_t lc, lt;
    if (!h || !get_bytes(env, argv[1], &com, &lc) || !get_bytes(env, argv[2], &tags, &lt)) return NULL;
    const size_t B = lc / 72;
    if (lc % 72 || lt != zk_escrow_tag_size() * B) {
        napi_throw_range_error(env, NULL, "escrowVerifyBatch: one 72-byte commitment and one 472-byte tag per entry");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    uint8_t *buf = (uint8_t *)xmalloc(env, 5 * B + 8);
    if (!buf) return NULL;
    int32_t *status = (int32_t *)buf;
    uint8_t *ok = buf + 4 * B;
    zk_status st = zk_escrow_verify_batch(c, B, com, tags, ok, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) set_prop(env, v, "ok", new_buffer(env, ok, B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}
/* (h, secret: 32, tags: B x 472) -> {index: B u32 LE (0xffffffff: nobody), status: B i32 LE}, against the ACTIVE ring */
static napi_value EscrowOpenBatch(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *secret, *tags;
    size_t ls, lt;
    if (!h || !get_bytes(env, argv[1], &secret, &ls) || !get_bytes(env, argv[2], &tags, &lt)) return NULL;
    const size_t B = lt / zk_escrow_tag_size();
    if (ls != 32 || lt != zk_escrow_tag_size() * B) {
        napi_throw_range_error(env, NULL, "escrowOpenBatch: a 32-byte secret and 472-byte tags");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    uint8_t *buf = (uint8_t *)xmalloc(env, 8 * B + 8);
    if (!buf) return NULL;
    int32_t *status = (int32_t *)buf;
    uint32_t *index = (uint32_t *)(buf + 4 * B);
    zk_status st = zk_escrow_open_batch(c, B, secret, tags, index, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) set_prop(env, v, "index", new_buffer(env, index, 4 * B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}
/* (h, secret: 32, tags: B x 472, ringIds: B u32 LE, 0xffffffff = any resident ring) -> {ring: B u32 LE, index: B u32 LE (0xffffffff: nobody), status: B i32 LE}:
 * zk_rings_escrow_open_batch, through the rings' resident point indexes; the active ring is not involved */
static napi_value EscrowOpenBatchRings(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *secret, *tags, *ids;
    size_t ls, lt, li;
    if (!h || !get_bytes(env, argv[1], &secret, &ls) || !get_bytes(env, argv[2], &tags, &lt) || !get_bytes(env, argv[3], &ids, &li)) return NULL;
    const size_t B = lt / zk_escrow_tag_size();
    if (ls != 32 || lt != zk_escrow_tag_size() * B || li != 4 * B) {
        napi_throw_range_error(env, NULL, "ringsEscrowOpenBatch: a 32-byte secret, 472-byte tags and one u32 ring id per tag");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    uint8_t *buf = (uint8_t *)xmalloc(env, 16 * B + 8);
    if (!buf) return NULL;
    int32_t *status = (int32_t *)buf;
    uint32_t *index = (uint32_t *)(buf + 4 * B), *ring = (uint32_t *)(buf + 8 * B), *idw = (uint32_t *)(buf + 12 * B);
    memcpy(idw, ids, 4 * B);   /* (a Buffer's bytes need not be 4-byte aligned) */
    zk_status st = zk_rings_escrow_open_batch(c, B, secret, tags, idw, ring, index, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok)
        set_prop(env, v, "ring", new_buffer(env, ring, 4 * B)), set_prop(env, v, "index", new_buffer(env, index, 4 * B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}
/* Threshold opening (include/zkattest.h: zk_auditors_*, zk_ctx_set_auditors), on the pool's first context like the escrow calls.
 * (h, secret: 32, t, n, seed: 32 -- FRESH) -> {shares: n x 32, keys: n x 72}: the dealer's split */
static napi_value AuditorsSplitKey(napi_env env, napi_callback_info info) {
    napi_value argv[5];
    if (!get_args(env, info, 5, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *secret, *seed;
    size_t ls, ld;
    uint32_t t, n;
    if (!h || !get_bytes(env, argv[1], &secret, &ls) || !get_bytes(env, argv[4], &seed, &ld)) return NULL;
    NAPI_OK(napi_get_value_uint32(env, argv[2], &t));
    NAPI_OK(napi_get_value_uint32(env, argv[3], &n));
    if (ls != 32 || ld != 32 || n > 16) {
        napi_throw_range_error(env, NULL, "auditorsSplitKey: a 32-byte secret, 1 <= t <= n <= 16 and a 32-byte seed");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    uint8_t shares[32 * 16], keys[72 * 16];
    zk_rng rng = {ZK_RNG_SEED, seed, 0};
    zk_status st = zk_auditors_split_key(c, secret, t, n, &rng, shares, keys);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) set_prop(env, v, "shares", new_buffer(env, shares, 32 * (size_t)n)), set_prop(env, v, "keys", new_buffer(env, keys, 72 * (size_t)n));
    for (volatile uint8_t *p = shares; p < shares + sizeof shares; p++) *p = 0;
    return v;
}
/* (h, t, keys: n x 72) -> undefined: the share keys, checked against the auditor's key */
static napi_value AuditorsSetKeys(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *keys;
    size_t lk;
    uint32_t t;
    if (!h || !get_bytes(env, argv[2], &keys, &lk)) return NULL;
    NAPI_OK(napi_get_value_uint32(env, argv[1], &t));
    if (lk % 72 || lk == 0 || lk > 72 * 16) {
        napi_throw_range_error(env, NULL, "auditorsSetKeys: 1 to 16 Tom-256 points of 72 bytes");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    zk_status st = zk_ctx_set_auditors(c, t, (uint32_t)(lk / 72), keys);
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    return NULL;
}
/* (h, j, shareSecret: 32, tags: B x 472, seeds: B x 32 -- FRESH) -> {shares: B x 264 (zeros where status != 0), status: B i32 LE} */
static napi_value AuditorsShareBatch(napi_env env, napi_callback_info info) {
    napi_value argv[5];
    if (!get_args(env, info, 5, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *secret, *tags, *seeds;
    size_t ls, lt, ld;
    uint32_t j;
    if (!h || !get_bytes(env, argv[2], &secret, &ls) || !get_bytes(env, argv[3], &tags, &lt) || !get_bytes(env, argv[4], &seeds, &ld)) return NULL;
    NAPI_OK(napi_get_value_uint32(env, argv[1], &j));
    const size_t B = lt / zk_escrow_tag_size();
    if (ls != 32 || lt != zk_escrow_tag_size() * B || ld != 32 * B) {
        napi_throw_range_error(env, NULL, "auditorsShareBatch: a 32-byte share secret, 472-byte tags and 32 seed bytes per tag");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    const uint64_t size = zk_auditors_share_size();
    uint8_t *buf = (uint8_t *)xmalloc(env, (size + 4) * B + 8);
    if (!buf) return NULL;
    int32_t *status = (int32_t *)buf;
    uint8_t *out = buf + 4 * B;
    zk_rng rng = {ZK_RNG_SEED, seeds, 0};
    zk_status st = zk_auditors_share_batch(c, B, j, secret, tags, &rng, out, size * B, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) set_prop(env, v, "shares", new_buffer(env, out, size * B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}
/* (h, tags: B x 472, shares: B x 264) -> {ok: B bytes, status: B i32 LE} */
static napi_value AuditorsShareVerifyBatch(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *tags, *shares;
    size_t lt, ls;
    if (!h || !get_bytes(env, argv[1], &tags, &lt) || !get_bytes(env, argv[2], &shares, &ls)) return NULL;
    const size_t B = lt / zk_escrow_tag_size();
    if (lt != zk_escrow_tag_size() * B || ls != zk_auditors_share_size() * B) {
        napi_throw_range_error(env, NULL, "auditorsShareVerifyBatch: one 472-byte tag and one 264-byte share per entry");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    uint8_t *buf = (uint8_t *)xmalloc(env, 5 * B + 8);
    if (!buf) return NULL;
    int32_t *status = (int32_t *)buf;
    uint8_t *ok = buf + 4 * B;
    zk_status st = zk_auditors_share_verify_batch(c, B, tags, shares, ok, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) set_prop(env, v, "ok", new_buffer(env, ok, B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}
/* (h, auditors: t u32 LE, tags: B x 472, shares: t x B x 264 slot-major, ringIds: B u32 LE, 0xffffffff = any resident ring) -> {ring: B u32 LE, index: B u32 LE
 * (0xffffffff: nobody), status: B i32 LE}; the active ring is not involved */
static napi_value AuditorsCombineBatch(napi_env env, napi_callback_info info) {
    napi_value argv[5];
    if (!get_args(env, info, 5, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *aud, *tags, *shares, *ids;
    size_t la, lt, ls, li;
    if (!h || !get_bytes(env, argv[1], &aud, &la) || !get_bytes(env, argv[2], &tags, &lt) || !get_bytes(env, argv[3], &shares, &ls) || !get_bytes(env, argv[4], &ids, &li)) return NULL;
    const size_t B = lt / zk_escrow_tag_size(), t = la / 4;
    if (la % 4 || t < 1 || t > 16 || lt != zk_escrow_tag_size() * B || ls != zk_auditors_share_size() * B * t || li != 4 * B) {
        napi_throw_range_error(env, NULL, "auditorsCombineBatch: 1 to 16 u32 auditors, 472-byte tags, one 264-byte share per auditor and tag, one u32 ring id per tag");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    uint8_t *buf = (uint8_t *)xmalloc(env, 16 * B + 64 + 8);
    if (!buf) return NULL;
    uint32_t *audw = (uint32_t *)buf;   /* (a Buffer's bytes need not be 4-byte aligned) */
    int32_t *status = (int32_t *)(buf + 64);
    uint32_t *index = (uint32_t *)(buf + 64 + 4 * B), *ring = (uint32_t *)(buf + 64 + 8 * B), *idw = (uint32_t *)(buf + 64 + 12 * B);
    memcpy(audw, aud, la), memcpy(idw, ids, 4 * B);
    zk_status st = zk_auditors_combine_batch(c, B, (uint32_t)t, audw, tags, shares, idw, ring, index, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok)
        set_prop(env, v, "ring", new_buffer(env, ring, 4 * B)), set_prop(env, v, "index", new_buffer(env, index, 4 * B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}
/* Distinct-key proofs (include/zkattest.h: zk_distinct_*), on the pool's first context like the link calls; no ring takes part.
 * (h, key1: B x 32, com1: B x 72, blinder1: B x 32, key2: B x 32, com2: B x 72, blinder2: B x 32, seeds: B x 32 -- FRESH) -> {proofs: B x 744 (zeros where
 * status != 0), status: B i32 LE} */
static napi_value DistinctProveBatch(napi_env env, napi_callback_info info) {
    napi_value argv[8];
    if (!get_args(env, info, 8, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *k1, *c1, *b1, *k2, *c2, *b2, *seeds;
    size_t lk1, lc1, lb1, lk2, lc2, lb2, ls;
    if (!h || !get_bytes(env, argv[1], &k1, &lk1) || !get_bytes(env, argv[2], &c1, &lc1) || !get_bytes(env, argv[3], &b1, &lb1) || !get_bytes(env, argv[4], &k2, &lk2) ||
        !get_bytes(env, argv[5], &c2, &lc2) || !get_bytes(env, argv[6], &b2, &lb2) || !get_bytes(env, argv[7], &seeds, &ls))
        return NULL;
    const size_t B = lk1 / 32;
    if (lk1 % 32 || lc1 != 72 * B || lb1 != 32 * B || lk2 != 32 * B || lc2 != 72 * B || lb2 != 32 * B || ls != 32 * B) {
        napi_throw_range_error(env, NULL, "distinctProveBatch: per proof two 32-byte keys, two 72-byte commitments, two 32-byte blinders and 32 seed bytes");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    const uint64_t size = zk_distinct_proof_size();
    uint8_t *buf = (uint8_t *)xmalloc(env, (size + 4) * B + 8);
    if (!buf) return NULL;
    int32_t *status = (int32_t *)buf;
    uint8_t *out = buf + 4 * B;
    zk_rng rng = {ZK_RNG_SEED, seeds, 0};
    zk_status st = zk_distinct_prove_batch(c, B, k1, c1, b1, k2, c2, b2, &rng, out, size * B, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) set_prop(env, v, "proofs", new_buffer(env, out, size * B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}
/* (h, com1: B x 72, com2: B x 72, proofs: B x 744) -> {ok: B bytes, status: B i32 LE} */
static napi_value DistinctVerifyBatch(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *c1, *c2, *proofs;
    size_t lc1, lc2, lp;
    if (!h || !get_bytes(env, argv[1], &c1, &lc1) || !get_bytes(env, argv[2], &c2, &lc2) || !get_bytes(env, argv[3], &proofs, &lp)) return NULL;
    const size_t B = lc1 / 72;
    if (lc1 % 72 || lc2 != 72 * B || lp != zk_distinct_proof_size() * B) {
        napi_throw_range_error(env, NULL, "distinctVerifyBatch: two 72-byte commitments and one 744-byte proof per entry");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    uint8_t *buf = (uint8_t *)xmalloc(env, 5 * B + 8);
    if (!buf) return NULL;
    int32_t *status = (int32_t *)buf;
    uint8_t *ok = buf + 4 * B;
    zk_status st = zk_distinct_verify_batch(c, B, c1, c2, proofs, ok, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) set_prop(env, v, "ok", new_buffer(env, ok, B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}
/* Quorum proofs (include/zkattest.h: zk_quorum_*), on the pool's first context with its ACTIVE ring.
 * (h, k, msg: Qk x 32, sig: Qk x 64, pk: Qk x 64, which: Qk u32 LE, seeds: Qk x 32, pairSeeds: Q k (k - 1) / 2 x 32 -- both FRESH and independent of each other)
 * -> {bundles: the successful quorums' ZKQ1 bundles back to back, off: (Q + 1) u64 LE, status: Q i32 LE, memberStatus: Qk i32 LE} */
static napi_value quorum_prove(napi_env env, napi_callback_info info, int rings) {
    napi_value argv[9];
    if (!get_args(env, info, 8 + rings, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint32_t k = 0;
    uint8_t *msg, *sig, *pk, *which, *seeds, *pseeds, *idb = NULL;
    size_t lm, ls, lp, lw, lsd, lps, li = 0;
    if (!h || napi_get_value_uint32(env, argv[1], &k) != napi_ok || !get_bytes(env, argv[2], &msg, &lm) || !get_bytes(env, argv[3], &sig, &ls) || !get_bytes(env, argv[4], &pk, &lp) ||
        !get_bytes(env, argv[5], &which, &lw) || (rings && !get_bytes(env, argv[6], &idb, &li)) || !get_bytes(env, argv[6 + rings], &seeds, &lsd) ||
        !get_bytes(env, argv[7 + rings], &pseeds, &lps))
        return NULL;
    const uint64_t P = zk_quorum_pair_count(k);
    const size_t n = lm / 32, Q = P ? n / k : 0;
    if (!P || lm % 32 || n != Q * k || ls != 64 * n || lp != 64 * n || lw != 4 * n || (rings && li != 4 * n) || lsd != 32 * n || lps != 32 * Q * P) {
        napi_throw_range_error(env, NULL, rings ? "ringsQuorumProveBatch: 2 <= k <= 16; per member a 32-byte hash, a 64-byte signature, a 64-byte key, a u32 index, a u32 ring id and 32 seed bytes; 32 seed bytes per pair"
                                                : "quorumProveBatch: 2 <= k <= 16; per member a 32-byte hash, a 64-byte signature, a 64-byte key, a u32 index and 32 seed bytes; 32 seed bytes per pair");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    uint32_t *ids = NULL;   /* (a Buffer's bytes need not be aligned) */
    uint64_t cap = rings ? Q * (16 + 744 * P) : zk_quorum_proof_max_size(c, k) * Q;
    if (rings) {
        ids = (uint32_t *)xmalloc(env, 4 * n + 4);
        if (!ids) return NULL;
        memcpy(ids, idb, 4 * n);
        for (size_t m = 0; m < n; m++) cap += zk_ring_proof_max_size(c, ids[m]);   /* the call's exact capacity rule */
    }
    uint8_t *buf = (uint8_t *)xmalloc(env, 8 * (Q + 1) + 4 * Q + 4 * n + cap + 8);
    if (!buf) {
        free(ids);
        return NULL;
    }
    uint64_t *off = (uint64_t *)buf;
    int32_t *status = (int32_t *)(buf + 8 * (Q + 1)), *mstatus = status + Q;
    uint8_t *out = (uint8_t *)(mstatus + n);
    uint32_t *w = (uint32_t *)xmalloc(env, 4 * n + 4);   /* (a Buffer's bytes need not be aligned) */
    if (!w) {
        free(buf);
        free(ids);
        return NULL;
    }
    memcpy(w, which, 4 * n);
    zk_rng rng = {ZK_RNG_SEED, seeds, 0}, rng_pairs = {ZK_RNG_SEED, pseeds, 0};
    zk_status st = rings ? zk_rings_quorum_prove_batch(c, Q, k, msg, sig, pk, w, ids, &rng, &rng_pairs, out, cap, off, status, mstatus)
                         : zk_quorum_prove_batch(c, Q, k, msg, sig, pk, w, &rng, &rng_pairs, out, cap, off, status, mstatus);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok)
        set_prop(env, v, "bundles", new_buffer(env, out, off[Q])), set_prop(env, v, "off", new_buffer(env, off, 8 * (Q + 1))), set_prop(env, v, "status", new_buffer(env, status, 4 * Q)),
            set_prop(env, v, "memberStatus", new_buffer(env, mstatus, 4 * n));
    free(w);
    free(ids);
    free(buf);
    return v;
}
static napi_value QuorumProveBatch(napi_env env, napi_callback_info info) { return quorum_prove(env, info, 0); }
/* zk_rings_quorum_prove_batch: the same with ids: Qk u32 LE (one RESIDENT ring id per member) behind which; the active ring plays no part */
static napi_value QuorumProveBatchRings(napi_env env, napi_callback_info info) { return quorum_prove(env, info, 1); }
/* (h, k, msg: Qk x 32, bundles: back to back, off: (Q + 1) u64 LE) -> {ok: Q bytes, status: Q i32 LE, firstBad: Q u32 LE} */
static napi_value quorum_verify(napi_env env, napi_callback_info info, int rings) {
    napi_value argv[6];
    if (!get_args(env, info, 5 + rings, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint32_t k = 0;
    uint8_t *msg, *blob, *ob, *idb = NULL;
    size_t lm, lb, lo, li = 0;
    if (!h || napi_get_value_uint32(env, argv[1], &k) != napi_ok || !get_bytes(env, argv[2], &msg, &lm) || !get_bytes(env, argv[3], &blob, &lb) || !get_bytes(env, argv[4], &ob, &lo) ||
        (rings && !get_bytes(env, argv[5], &idb, &li)))
        return NULL;
    const size_t Q = lo >= 8 ? lo / 8 - 1 : 0;
    if (!zk_quorum_pair_count(k) || lo < 8 || lo % 8 || lm != 32 * Q * k || (rings && li != 4 * Q * k)) {
        napi_throw_range_error(env, NULL, rings ? "ringsQuorumVerifyBatch: 2 <= k <= 16, (Q + 1) u64 offsets, k 32-byte hashes and k u32 ring ids per bundle"
                                                : "quorumVerifyBatch: 2 <= k <= 16, (Q + 1) u64 offsets and k 32-byte hashes per bundle");
        return NULL;
    }
    uint8_t *buf = (uint8_t *)xmalloc(env, 8 * (Q + 1) + 9 * Q + 4 * Q * k + 8);
    if (!buf) return NULL;
    uint64_t *off = (uint64_t *)buf;
    memcpy(off, ob, 8 * (Q + 1));
    for (size_t q = 0; q <= Q; q++)
        if (off[q] > lb) {   /* no slot may reach past the Buffer */
            free(buf);
            napi_throw_range_error(env, NULL, "quorumVerifyBatch: an offset lies behind the bundles");
            return NULL;
        }
    int32_t *status = (int32_t *)(buf + 8 * (Q + 1));
    uint32_t *bad = (uint32_t *)(status + Q);
    uint32_t *ids = bad + Q;   /* (a Buffer's bytes need not be aligned) */
    uint8_t *ok = (uint8_t *)(ids + Q * k);
    if (rings) memcpy(ids, idb, 4 * Q * k);
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    zk_status st = rings ? zk_rings_quorum_verify_batch(c, Q, k, msg, blob, off, ids, NULL, ok, status, bad) : zk_quorum_verify_batch(c, Q, k, msg, blob, off, NULL, ok, status, bad);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok)
        set_prop(env, v, "ok", new_buffer(env, ok, Q)), set_prop(env, v, "status", new_buffer(env, status, 4 * Q)), set_prop(env, v, "firstBad", new_buffer(env, bad, 4 * Q));
    free(buf);
    return v;
}
static napi_value QuorumVerifyBatch(napi_env env, napi_callback_info info) { return quorum_verify(env, info, 0); }
/* zk_rings_quorum_verify_batch: the same with ids: Qk u32 LE (one RESIDENT ring id per member) behind off */
static napi_value QuorumVerifyBatchRings(napi_env env, napi_callback_info info) { return quorum_verify(env, info, 1); }
/* Accountable attestations (include/zkattest.h: zk_accountable_*), on the pool's first context with its ACTIVE ring and its auditor key.
 * (h, msg: B x 32, sig: B x 64, pk: B x 64, which: B u32 LE, seeds: B x 32, tagSeeds: B x 32 -- both FRESH and independent of each other)
 * -> {bundles: the successful ZKC1 bundles back to back, off: (B + 1) u64 LE, status: B i32 LE, partStatus: 2B i32 LE (attestation, tag)} */
static napi_value AccountableProveBatch(napi_env env, napi_callback_info info) {
    napi_value argv[7];
    if (!get_args(env, info, 7, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *msg, *sig, *pk, *which, *seeds, *tseeds;
    size_t lm, ls, lp, lw, lsd, lts;
    if (!h || !get_bytes(env, argv[1], &msg, &lm) || !get_bytes(env, argv[2], &sig, &ls) || !get_bytes(env, argv[3], &pk, &lp) || !get_bytes(env, argv[4], &which, &lw) ||
        !get_bytes(env, argv[5], &seeds, &lsd) || !get_bytes(env, argv[6], &tseeds, &lts))
        return NULL;
    const size_t B = lm / 32;
    if (lm % 32 || ls != 64 * B || lp != 64 * B || lw != 4 * B || lsd != 32 * B || lts != 32 * B) {
        napi_throw_range_error(env, NULL, "accountableProveBatch: per bundle a 32-byte hash, a 64-byte signature, a 64-byte key, a u32 index, 32 seed bytes and 32 tag seed bytes");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    const uint64_t cap = zk_accountable_proof_max_size(c) * B;
    uint8_t *buf = (uint8_t *)xmalloc(env, 8 * (B + 1) + 16 * B + cap + 8);
    if (!buf) return NULL;
    uint64_t *off = (uint64_t *)buf;
    int32_t *status = (int32_t *)(buf + 8 * (B + 1)), *pstatus = status + B;
    uint32_t *w = (uint32_t *)(pstatus + 2 * B);   /* (a Buffer's bytes need not be aligned) */
    uint8_t *out = (uint8_t *)(w + B);
    memcpy(w, which, 4 * B);
    zk_rng rng = {ZK_RNG_SEED, seeds, 0}, rng_tags = {ZK_RNG_SEED, tseeds, 0};
    zk_status st = zk_accountable_prove_batch(c, B, msg, sig, pk, w, &rng, &rng_tags, out, cap, off, status, pstatus);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok)
        set_prop(env, v, "bundles", new_buffer(env, out, off[B])), set_prop(env, v, "off", new_buffer(env, off, 8 * (B + 1))), set_prop(env, v, "status", new_buffer(env, status, 4 * B)),
            set_prop(env, v, "partStatus", new_buffer(env, pstatus, 8 * B));
    free(buf);
    return v;
}
/* (B + 1) u64 LE offsets out of a Buffer into aligned memory; no slot may reach past `limit` bytes.  -> 0 after a thrown RangeError */
static int accountable_offsets(napi_env env, const uint8_t *ob, size_t B, size_t limit, uint64_t *off, const char *what) {
    memcpy(off, ob, 8 * (B + 1));
    for (size_t b = 0; b <= B; b++)
        if (off[b] > limit) {
            napi_throw_range_error(env, NULL, what);
            return 0;
        }
    return 1;
}
/* (h, msg: B x 32, bundles: back to back, off: (B + 1) u64 LE) -> {ok: B bytes, status: B i32 LE, firstBad: B u32 LE (0 attestation, 1 tag, 0xFFFFFFFF ok)} */
static napi_value AccountableVerifyBatch(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *msg, *blob, *ob;
    size_t lm, lb, lo;
    if (!h || !get_bytes(env, argv[1], &msg, &lm) || !get_bytes(env, argv[2], &blob, &lb) || !get_bytes(env, argv[3], &ob, &lo)) return NULL;
    const size_t B = lo >= 8 ? lo / 8 - 1 : 0;
    if (lo < 8 || lo % 8 || lm != 32 * B) {
        napi_throw_range_error(env, NULL, "accountableVerifyBatch: (B + 1) u64 offsets and one 32-byte hash per bundle");
        return NULL;
    }
    uint8_t *buf = (uint8_t *)xmalloc(env, 8 * (B + 1) + 9 * B + 8);
    if (!buf) return NULL;
    uint64_t *off = (uint64_t *)buf;
    if (!accountable_offsets(env, ob, B, lb, off, "accountableVerifyBatch: an offset lies behind the bundles")) {
        free(buf);
        return NULL;
    }
    int32_t *status = (int32_t *)(buf + 8 * (B + 1));
    uint32_t *bad = (uint32_t *)(status + B);
    uint8_t *ok = (uint8_t *)(bad + B);
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    zk_status st = zk_accountable_verify_batch(c, B, msg, blob, off, NULL, ok, status, bad);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok)
        set_prop(env, v, "ok", new_buffer(env, ok, B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B)), set_prop(env, v, "firstBad", new_buffer(env, bad, 4 * B));
    free(buf);
    return v;
}
/* Accountable attestations over several resident rings (include/zkattest_rings_accountable.h: zk_rings_accountable_*): one ring id per bundle, the pool's
 * first context, no active ring involved.
 * (h, msg, sig, pk, which: B u32 LE, ringIds: B u32 LE, seeds, tagSeeds) -> what accountableProveBatch returns */
static napi_value AccountableProveBatchRings(napi_env env, napi_callback_info info) {
    napi_value argv[8];
    if (!get_args(env, info, 8, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *msg, *sig, *pk, *which, *ids, *seeds, *tseeds;
    size_t lm, ls, lp, lw, li, lsd, lts;
    if (!h || !get_bytes(env, argv[1], &msg, &lm) || !get_bytes(env, argv[2], &sig, &ls) || !get_bytes(env, argv[3], &pk, &lp) || !get_bytes(env, argv[4], &which, &lw) ||
        !get_bytes(env, argv[5], &ids, &li) || !get_bytes(env, argv[6], &seeds, &lsd) || !get_bytes(env, argv[7], &tseeds, &lts))
        return NULL;
    const size_t B = lm / 32;
    if (lm % 32 || ls != 64 * B || lp != 64 * B || lw != 4 * B || li != 4 * B || lsd != 32 * B || lts != 32 * B) {
        napi_throw_range_error(env, NULL, "accountableProveBatchRings: per bundle a 32-byte hash, a 64-byte signature, a 64-byte key, a u32 index, a u32 ring id, 32 seed bytes and 32 tag seed bytes");
        return NULL;
    }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    uint64_t cap = 0;   /* the call's own rule: the sum of the rings' maxima, 0 for an id that is not resident */
    for (size_t b = 0; b < B; b++) {
        uint32_t id;
        memcpy(&id, ids + 4 * b, 4);
        cap += zk_rings_accountable_proof_max_size(c, id);
    }
    uint8_t *buf = (uint8_t *)xmalloc(env, 8 * (B + 1) + 20 * B + cap + 8);
    if (!buf) return NULL;
    uint64_t *off = (uint64_t *)buf;
    int32_t *status = (int32_t *)(buf + 8 * (B + 1)), *pstatus = status + B;
    uint32_t *w = (uint32_t *)(pstatus + 2 * B), *idw = w + B;   /* (a Buffer's bytes need not be aligned) */
    uint8_t *out = (uint8_t *)(idw + B);
    memcpy(w, which, 4 * B), memcpy(idw, ids, 4 * B);
    zk_rng rng = {ZK_RNG_SEED, seeds, 0}, rng_tags = {ZK_RNG_SEED, tseeds, 0};
    zk_status st = zk_rings_accountable_prove_batch(c, B, msg, sig, pk, w, idw, &rng, &rng_tags, out, cap, off, status, pstatus);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok)
        set_prop(env, v, "bundles", new_buffer(env, out, off[B])), set_prop(env, v, "off", new_buffer(env, off, 8 * (B + 1))), set_prop(env, v, "status", new_buffer(env, status, 4 * B)),
            set_prop(env, v, "partStatus", new_buffer(env, pstatus, 8 * B));
    free(buf);
    return v;
}
/* (h, msg: B x 32, bundles: back to back, off: (B + 1) u64 LE, ringIds: B u32 LE) -> what accountableVerifyBatch returns */
static napi_value AccountableVerifyBatchRings(napi_env env, napi_callback_info info) {
    napi_value argv[5];
    if (!get_args(env, info, 5, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *msg, *blob, *ob, *ids;
    size_t lm, lb, lo, li;
    if (!h || !get_bytes(env, argv[1], &msg, &lm) || !get_bytes(env, argv[2], &blob, &lb) || !get_bytes(env, argv[3], &ob, &lo) || !get_bytes(env, argv[4], &ids, &li)) return NULL;
    const size_t B = lo >= 8 ? lo / 8 - 1 : 0;
    if (lo < 8 || lo % 8 || lm != 32 * B || li != 4 * B) {
        napi_throw_range_error(env, NULL, "accountableVerifyBatchRings: (B + 1) u64 offsets, one 32-byte hash and one u32 ring id per bundle");
        return NULL;
    }
    uint8_t *buf = (uint8_t *)xmalloc(env, 8 * (B + 1) + 13 * B + 8);
    if (!buf) return NULL;
    uint64_t *off = (uint64_t *)buf;
    if (!accountable_offsets(env, ob, B, lb, off, "accountableVerifyBatchRings: an offset lies behind the bundles")) {
        free(buf);
        return NULL;
    }
    int32_t *status = (int32_t *)(buf + 8 * (B + 1));
    uint32_t *bad = (uint32_t *)(status + B), *idw = bad + B;
    uint8_t *ok = (uint8_t *)(idw + B);
    memcpy(idw, ids, 4 * B);
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    zk_status st = zk_rings_accountable_verify_batch(c, B, msg, blob, off, idw, NULL, ok, status, bad);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok)
        set_prop(env, v, "ok", new_buffer(env, ok, B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B)), set_prop(env, v, "firstBad", new_buffer(env, bad, 4 * B));
    free(buf);
    return v;
}
/* (h, secret: 32, bundles: back to back, off: (B + 1) u64 LE, ringIds: B u32 LE, 0xffffffff = any resident ring) -> what ringsEscrowOpenBatch returns: the
 * auditor's call straight on bundles.  It does not verify. */
static napi_value AccountableOpenBatchRings(napi_env env, napi_callback_info info) {
    napi_value argv[5];
    if (!get_args(env, info, 5, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *secret, *blob, *ob, *ids;
    size_t ls, lb, lo, li;
    if (!h || !get_bytes(env, argv[1], &secret, &ls) || !get_bytes(env, argv[2], &blob, &lb) || !get_bytes(env, argv[3], &ob, &lo) || !get_bytes(env, argv[4], &ids, &li)) return NULL;
    const size_t B = lo >= 8 ? lo / 8 - 1 : 0;
    if (ls != 32 || lo < 8 || lo % 8 || li != 4 * B) {
        napi_throw_range_error(env, NULL, "accountableOpenBatchRings: a 32-byte secret, (B + 1) u64 offsets and one u32 ring id per bundle");
        return NULL;
    }
    uint8_t *buf = (uint8_t *)xmalloc(env, 8 * (B + 1) + 16 * B + 8);
    if (!buf) return NULL;
    uint64_t *off = (uint64_t *)buf;
    if (!accountable_offsets(env, ob, B, lb, off, "accountableOpenBatchRings: an offset lies behind the bundles")) {
        free(buf);
        return NULL;
    }
    int32_t *status = (int32_t *)(buf + 8 * (B + 1));
    uint32_t *index = (uint32_t *)(status + B), *ring = index + B, *idw = ring + B;
    memcpy(idw, ids, 4 * B);
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    zk_status st = zk_rings_accountable_open_batch(c, B, secret, blob, off, idw, ring, index, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok)
        set_prop(env, v, "ring", new_buffer(env, ring, 4 * B)), set_prop(env, v, "index", new_buffer(env, index, 4 * B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}
/* zk_accountable_split_batch: (h, bundles: back to back, off: (B + 1) u64 LE) -> {attestations: back to back, off: (B + 1) u64 LE, tags: B x 472, status: B i32 LE} */
static napi_value AccountableSplitBatch(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *blob, *ob;
    size_t lb, lo;
    if (!h || !get_bytes(env, argv[1], &blob, &lb) || !get_bytes(env, argv[2], &ob, &lo)) return NULL;
    if (lo < 8 || lo % 8) {
        napi_throw_range_error(env, NULL, "accountableSplitBatch: B + 1 offsets of 8 bytes");
        return NULL;
    }
    const size_t B = lo / 8 - 1;
    uint8_t *buf = (uint8_t *)xmalloc(env, 16 * (B + 1) + 4 * B + 472 * B + lb + 8);
    if (!buf) return NULL;
    uint64_t *off = (uint64_t *)buf, *aoff = off + (B + 1);
    if (!accountable_offsets(env, ob, B, lb, off, "accountableSplitBatch: an offset lies behind the bundles")) {
        free(buf);
        return NULL;
    }
    int32_t *status = (int32_t *)(aoff + (B + 1));
    uint8_t *tags = (uint8_t *)(status + B), *att = tags + 472 * B;
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    zk_status st = zk_accountable_split_batch(c, B, blob, off, att, lb, aoff, tags, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok)
        set_prop(env, v, "attestations", new_buffer(env, att, aoff[B])), set_prop(env, v, "off", new_buffer(env, aoff, 8 * (B + 1))), set_prop(env, v, "tags", new_buffer(env, tags, 472 * B)),
            set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}
/* zk_accountable_join_batch: (h, proofs: back to back, off: (B + 1) u64 LE, tags: B x 472) -> {bundles: the accepted ones back to back, off: (B + 1) u64 LE, status: B i32 LE} */
static napi_value AccountableJoinBatch(napi_env env, napi_callback_info info) {
    napi_value argv[4];
    if (!get_args(env, info, 4, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *blob, *ob, *tags;
    size_t lb, lo, lt;
    if (!h || !get_bytes(env, argv[1], &blob, &lb) || !get_bytes(env, argv[2], &ob, &lo) || !get_bytes(env, argv[3], &tags, &lt)) return NULL;
    const size_t B = lo >= 8 ? lo / 8 - 1 : 0;
    if (lo < 8 || lo % 8 || lt != 472 * B) {
        napi_throw_range_error(env, NULL, "accountableJoinBatch: (B + 1) u64 offsets and one 472-byte tag per proof");
        return NULL;
    }
    const uint64_t cap = lb + 488 * B;
    uint8_t *buf = (uint8_t *)xmalloc(env, 16 * (B + 1) + 4 * B + cap + 8);
    if (!buf) return NULL;
    uint64_t *off = (uint64_t *)buf, *ooff = off + (B + 1);
    if (!accountable_offsets(env, ob, B, lb, off, "accountableJoinBatch: an offset lies behind the proofs' bytes")) {
        free(buf);
        return NULL;
    }
    int32_t *status = (int32_t *)(ooff + (B + 1));
    uint8_t *out = (uint8_t *)(status + B);
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    zk_status st = zk_accountable_join_batch(c, B, blob, off, tags, out, cap, ooff, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok)
        set_prop(env, v, "bundles", new_buffer(env, out, ooff[B])), set_prop(env, v, "off", new_buffer(env, ooff, 8 * (B + 1))), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}
/* zk_proof_key_commitments: (h, proofs: the B proofs back to back in the context's wire layout, off: (B + 1) u64 LE) -> {coms: B x 72 (zeros where status != 0),
 * status: B i32 LE} */
static napi_value KeyCommitments(napi_env env, napi_callback_info info) {
    napi_value argv[3];
    if (!get_args(env, info, 3, argv)) return NULL;
    Handle *h = get_handle(env, argv[0], 0);
    uint8_t *blob, *ob;
    size_t lp, lo;
    if (!h || !get_bytes(env, argv[1], &blob, &lp) || !get_bytes(env, argv[2], &ob, &lo)) return NULL;
    if (lo < 8 || lo % 8) {
        napi_throw_range_error(env, NULL, "keyCommitments: B + 1 offsets of 8 bytes");
        return NULL;
    }
    const size_t B = lo / 8 - 1;
    uint8_t *buf = (uint8_t *)xmalloc(env, 8 * (B + 1) + (72 + 4) * B + lp + 8);   /* (a Buffer's bytes need not be aligned: offsets and proofs are copied) */
    if (!buf) return NULL;
    uint64_t *off = (uint64_t *)buf;
    int32_t *status = (int32_t *)(off + (B + 1));
    uint8_t *com = (uint8_t *)(status + B), *pr = com + 72 * B;
    memcpy(off, ob, 8 * (B + 1));
    if (lp) memcpy(pr, blob, lp);
    for (size_t b = 0; b <= B; b++)
        if (off[b] > lp) {   /* no slot may reach past the bytes that were handed over */
            free(buf);
            napi_throw_range_error(env, NULL, "keyCommitments: an offset lies behind the proofs' bytes");
            return NULL;
        }
    zk_ctx *c = zk_pool_ctx(h->pool, 0);
    zk_status st = zk_proof_key_commitments(c, B, pr, off, com, status);
    napi_value v = NULL;
    if (st != ZK_OK) throw_text(env, st, zk_last_error(c));
    else if (napi_create_object(env, &v) == napi_ok) set_prop(env, v, "coms", new_buffer(env, com, 72 * B)), set_prop(env, v, "status", new_buffer(env, status, 4 * B));
    free(buf);
    return v;
}

static napi_value Init(napi_env env, napi_value exports) {
    static const struct {
        const char *name;
        napi_callback fn;
    } fns[] = {{"createPool", CreatePool},       {"destroyPool", DestroyPool},       {"poolInfo", PoolInfo},       {"setOption", SetOption},
               {"setParams", SetParams},         {"setRing", SetRing},               {"synthParams", SynthParams}, {"synthWorkload", SynthWorkload},
               {"proveBatch", ProveBatch},       {"verifyBatch", VerifyBatch},       {"proveBatchAsync", ProveBatchAsync},
               {"verifyBatchAsync", VerifyBatchAsync}, {"proofToJson", ProofToJson}, {"proofFromJson", ProofFromJson},
               {"keysToInts", KeysToInts},       {"hostAlloc", HostAlloc},           {"hardenedH", HardenedH},
               {"proofsToJsonBatch", ProofsToJsonBatch}, {"proofsFromJsonBatch", ProofsFromJsonBatch},
               {"proveSubmit", ProveSubmit},     {"verifySubmit", VerifySubmit},
               {"addRing", AddRing},             {"useRing", UseRing},               {"dropRing", DropRing},           {"updateRing", UpdateRing},       {"ringInfo", RingInfo},
               {"verifyBatchRings", VerifyBatchRings}, {"verifyBatchRingsAsync", VerifyBatchRingsAsync},
               {"proveBatchRings", ProveBatchRings},   {"proveBatchRingsAsync", ProveBatchRingsAsync},
               {"screenBatchRings", ScreenBatchRings},
               {"recoverBatchRings", RecoverBatchRings},
               {"memberProofSize", MemberProofSize},   {"memberProveBatch", MemberProveBatch}, {"memberVerifyBatch", MemberVerifyBatch},
               {"memberProofSizeRing", MemberProofSizeRing}, {"memberProveBatchRings", MemberProveBatchRings}, {"memberVerifyBatchRings", MemberVerifyBatchRings},
               {"memberProveBatchBound", MemberProveBatchBound}, {"memberVerifyBatchBound", MemberVerifyBatchBound},
               {"memberProveBatchRingsBound", MemberProveBatchRingsBound}, {"memberVerifyBatchRingsBound", MemberVerifyBatchRingsBound},
               {"keyBlinders", KeyBlinders},     {"reringBatch", ReringBatch},     {"reringBatchRings", ReringBatchRings},
               {"linkProveBatch", LinkProveBatch}, {"linkVerifyBatch", LinkVerifyBatch}, {"keyCommitments", KeyCommitments},
               {"distinctProveBatch", DistinctProveBatch}, {"distinctVerifyBatch", DistinctVerifyBatch},
               {"setAuditor", SetAuditor},       {"escrowKeygen", EscrowKeygen},   {"escrowProveBatch", EscrowProveBatch},
               {"escrowVerifyBatch", EscrowVerifyBatch}, {"escrowOpenBatch", EscrowOpenBatch},
               {"quorumProveBatch", QuorumProveBatch}, {"quorumVerifyBatch", QuorumVerifyBatch},
               {"ringsQuorumProveBatch", QuorumProveBatchRings}, {"ringsQuorumVerifyBatch", QuorumVerifyBatchRings},
               {"ringsEscrowOpenBatch", EscrowOpenBatchRings},
               {"auditorsSplitKey", AuditorsSplitKey}, {"auditorsSetKeys", AuditorsSetKeys}, {"auditorsShareBatch", AuditorsShareBatch},
               {"auditorsShareVerifyBatch", AuditorsShareVerifyBatch}, {"auditorsCombineBatch", AuditorsCombineBatch},
               {"accountableProveBatch", AccountableProveBatch}, {"accountableVerifyBatch", AccountableVerifyBatch},
               {"accountableSplitBatch", AccountableSplitBatch}, {"accountableJoinBatch", AccountableJoinBatch},
               {"accountableProveBatchRings", AccountableProveBatchRings}, {"accountableVerifyBatchRings", AccountableVerifyBatchRings},
               {"accountableOpenBatchRings", AccountableOpenBatchRings}};
    for (size_t i = 0; i < sizeof fns / sizeof fns[0]; i++) {
        napi_value f;
        if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok) return NULL;
        napi_set_named_property(env, exports, fns[i].name, f);
    }
    return exports;
}
NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
