"""not-gpu: the ring-update ABI (include/zkattest.h: zk_ctx_update_ring, zk_pool_update_ring) is declared, exported and bound in Python, the N-API typings
declare updateRing, the two new work counters are documented, the table checksum hook stays out of the product library, and both entry points refuse a NULL
context or pool with ZK_E_ARG (no device is touched)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZK_E_ARG = 14
NEW = ['zk_ctx_update_ring', 'zk_pool_update_ring']


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
    assert re.search(r'\* 5 = per-key tables', hdr) and re.search(r'\* 6 = 256-key blocks', hdr)
    # the checksum hook is described in the header but belongs to the test build alone
    assert 'zk_test_ring_checksum' in hdr and 'zk_test_ring_checksum' not in declared
    assert not hasattr(L, 'zk_test_ring_checksum')


def test_engine_and_pool_methods_exist():
    import zkp_ecdsa_amd as Z
    assert callable(getattr(Z.Engine, 'update_ring', None))
    assert callable(getattr(Z.Pool, 'update_ring', None))


def test_changes_are_a_dict_or_a_list_applied_in_order():
    import zkp_ecdsa_amd   # noqa: F401 (the shim that makes the package importable)
    from zkp_ecdsa_amd import _native as N
    a, b = bytes([1]) * 32, bytes([2]) * 32
    cnt, idx, keys = N._ring_changes({5: a, 2: b})
    assert (cnt, list(idx), keys) == (2, [5, 2], a + b)
    cnt, idx, keys = N._ring_changes([(7, a), (7, b)])
    assert (cnt, list(idx), keys) == (2, [7, 7], a + b)
    assert N._ring_changes([]) == (0, None, None)


def test_typings_and_facade_declare_the_update():
    dts = open(os.path.join(ROOT, 'bindings', 'napi', 'zkattest.d.ts')).read()
    assert re.search(r'\bupdateRing\(', dts)
    assert 'ringDelta' in dts
    js = open(os.path.join(ROOT, 'bindings', 'napi', 'zkattest.js')).read()
    assert 'updateRing' in js and 'ringDelta' in js
    assert 'updateRing' in open(os.path.join(ROOT, 'bindings', 'napi', 'zkattest_napi.c')).read()


def test_null_context_and_pool_are_refused():
    _, L = _lib()
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    idx = (u64 * 1)(0)
    assert L.zk_ctx_update_ring(vp(), u32(0), u64(1), idx, bytes(32), u64(2)) == ZK_E_ARG
    assert L.zk_pool_update_ring(vp(), u32(0), u64(1), idx, bytes(32), u64(2)) == ZK_E_ARG
