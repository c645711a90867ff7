"""not-gpu: the resident-ring ABI (include/zkattest.h: zk_ctx_add_ring, zk_verify_batch_rings, zk_pool_add_ring) is declared, exported and
bound in Python, the N-API typings declare it, and every entry point refuses a NULL context or pool with ZK_E_ARG (no device is touched)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZK_E_ARG = 14
NEW = ['zk_ctx_add_ring', 'zk_ctx_add_ring_device', 'zk_ctx_use_ring', 'zk_ctx_drop_ring', 'zk_ring_info', 'zk_verify_batch_rings',
       'zk_verify_batch_rings_device', 'zk_pool_add_ring', 'zk_pool_use_ring', 'zk_pool_drop_ring', 'zk_pool_verify_batch_rings']


def _lib():
    import zkp_ecdsa_amd as Z
    if not os.path.exists(Z.LIB_PATH):
        Z.build()
    return Z, Z.lib()


def test_new_symbols_declared_exported_and_listed():
    Z, L = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'zkattest.h')).read()
    declared = set(re.findall(r'\b(zk_[a-z0-9_]+)\s*\(', hdr))
    for s in NEW:
        assert s in declared, s
        assert s in Z.SYMBOLS, s
        assert hasattr(L, s), s
    assert re.search(r'#define ZK_MAX_RINGS 16\b', hdr)


def test_engine_and_pool_methods_exist():
    import zkp_ecdsa_amd as Z
    for m in ('add_ring', 'add_ring_device', 'use_ring', 'drop_ring', 'ring_info', 'verify_batch_rings', 'verify_batch_rings_device'):
        assert callable(getattr(Z.Engine, m, None)), m
    for m in ('add_ring', 'use_ring', 'drop_ring', 'ring_info', 'verify_batch_rings'):
        assert callable(getattr(Z.Pool, m, None)), m
    assert (Z.RING_TABLE_E, Z.RING_DIGIT_PLANES, Z.RING_TABLE_E_DIGITS, Z.RING_KEY_TABLES, Z.RING_ACTIVE) == (1, 2, 4, 8, 16)


def test_typings_declare_the_ring_calls():
    dts = open(os.path.join(ROOT, 'bindings', 'napi', 'zkattest.d.ts')).read()
    assert re.search(r'export function verifySignatureLists\(', dts)
    for m in ('addRing', 'useRing', 'dropRing', 'ringInfo', 'verifyBatchRings', 'verifyBatchRingsAsync'):
        assert re.search(r'\b%s\(' % m, dts), m


def test_null_context_and_pool_are_refused():
    _, L = _lib()
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    rid, nk, ln, fl, gen = u32(), u64(), u32(), u32(), u64()
    keys = bytes(64)
    ids = (u32 * 1)()
    ok, st = (C.c_uint8 * 1)(), (C.c_int32 * 1)()
    off = (u64 * 2)(0, 4)
    assert L.zk_ctx_add_ring(vp(), keys, u64(2), C.byref(rid)) == ZK_E_ARG
    assert L.zk_ctx_add_ring_device(vp(), vp(), u64(2), C.byref(rid)) == ZK_E_ARG
    assert L.zk_ctx_use_ring(vp(), u32(0)) == ZK_E_ARG
    assert L.zk_ctx_drop_ring(vp(), u32(0)) == ZK_E_ARG
    assert L.zk_ring_info(vp(), u32(0), C.byref(nk), C.byref(ln), C.byref(fl), C.byref(gen)) == ZK_E_ARG
    assert L.zk_verify_batch_rings(vp(), u64(1), bytes(32), bytes(4), off, ids, None, ok, st) == ZK_E_ARG
    assert L.zk_verify_batch_rings_device(vp(), u64(1), vp(1), vp(1), vp(1), vp(1), vp(), vp(1), vp(1)) == ZK_E_ARG
    assert L.zk_pool_add_ring(vp(), keys, u64(2), C.byref(rid)) == ZK_E_ARG
    assert L.zk_pool_use_ring(vp(), u32(0)) == ZK_E_ARG
    assert L.zk_pool_drop_ring(vp(), u32(0)) == ZK_E_ARG
    ln2 = (u64 * 1)(4)
    off1 = (u64 * 1)(0)
    assert L.zk_pool_verify_batch_rings(vp(), u64(1), bytes(32), bytes(4), off1, ln2, ids, None, ok, st) == ZK_E_ARG
