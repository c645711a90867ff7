"""not-gpu: the mixed-ring prove ABI (include/zkattest.h: zk_prove_batch_rings, zk_prove_batch_rings_device, zk_pool_prove_batch_rings) is declared
with the argument lists the Python binding calls it with, exported by all three builds of the library and bound in Python; the N-API typings declare
the facade call; the test-hook setter exists in the test build only; and every entry point refuses NULL arguments with ZK_E_ARG before any device
is touched."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZK_E_ARG = 14
NEW = ['zk_prove_batch_rings', 'zk_prove_batch_rings_device', 'zk_pool_prove_batch_rings']


def _lib():
    import zkp_ecdsa_amd as Z
    if not os.path.exists(Z.LIB_PATH):
        Z.build()
    return Z, Z.lib()


def _header():
    return open(os.path.join(ROOT, 'include', 'zkattest.h')).read()


def _prototype(hdr, name):
    """the parameter list of `name`'s declaration, comments removed, as a list of parameter texts"""
    m = re.search(r'\bzk_status %s\((.*?)\);' % name, hdr, re.S)
    assert m, name
    text = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    return [' '.join(p.split()) for p in text.split(',')]


def test_new_symbols_declared_exported_and_listed():
    Z, L = _lib()
    declared = set(re.findall(r'\b(zk_[a-z0-9_]+)\s*\(', _header()))
    for s in NEW:
        assert s in declared, s
        assert s in Z.SYMBOLS, s
        assert hasattr(L, s), s
    # the size bound of a proof over a ring that need not be active (what the bindings size `out` with)
    assert 'zk_ring_proof_max_size' in declared and 'zk_ring_proof_max_size' in Z.SYMBOLS
    assert L.zk_ring_proof_max_size(C.c_void_p(), C.c_uint32(0)) == 0


@pytest.mark.parametrize('name', ['libzkattest_hip.so', 'libzkattest_hip_uniform.so', 'libzkattest_hip_testhooks.so'])
def test_every_build_exports_the_calls(name):
    Z, _ = _lib()
    path = os.path.join(os.path.dirname(Z.LIB_PATH), name)
    assert os.path.exists(path), 'not built: ' + name
    L = C.CDLL(path)
    for s in NEW:
        assert hasattr(L, s), (name, s)
    # the setter that forces small segments is a test hook: the product builds do not export it
    assert hasattr(L, 'zk_test_set_prove_segment') == (name == 'libzkattest_hip_testhooks.so')


def test_header_and_ctypes_prototypes_agree():
    """parameter by parameter: a pointer in the header is a pointer type in the binding, uint64_t is c_uint64"""
    Z, L = _lib()
    hdr = _header()
    for name in NEW:
        params = _prototype(hdr, name)
        argtypes = getattr(L, name).argtypes
        assert argtypes is not None and len(argtypes) == len(params), (name, params)
        for p, a in zip(params, argtypes):
            if '*' in p:
                assert a in (C.c_void_p, C.c_char_p) or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert p.startswith('uint64_t ') and a is C.c_uint64, (name, p, a)
        assert getattr(L, name).restype is C.c_int
    assert [p.split()[-1].lstrip('*') for p in _prototype(hdr, 'zk_prove_batch_rings')] == [
        'ctx', 'B', 'msg_hash', 'sig', 'pk_xy', 'which', 'ring_ids', 'rng', 'out', 'out_cap', 'out_off', 'per_proof_status']
    # zk_prove_batch_device + d_ring_ids, zk_pool_prove_batch + ring_ids: the one-ring calls' shapes with the ids behind `which`
    for one, mixed in (('zk_prove_batch_device', 'zk_prove_batch_rings_device'), ('zk_pool_prove_batch', 'zk_pool_prove_batch_rings'), ('zk_prove_batch', 'zk_prove_batch_rings')):
        a, b = _prototype(hdr, one), _prototype(hdr, mixed)
        assert b[:6] == a[:6] and b[7:] == a[6:] and 'ring_ids' in b[6], (one, mixed)


def test_engine_and_pool_methods_exist_and_counters_are_documented():
    import zkp_ecdsa_amd as Z
    for m in ('prove_batch_rings', 'prove_batch_rings_device'):
        assert callable(getattr(Z.Engine, m, None)), m
    assert callable(getattr(Z.Pool, 'prove_batch_rings', None))
    hdr = _header()
    assert re.search(r'\* 7 = segments', hdr) and re.search(r'\* 8 = windows', hdr) and re.search(r'\* 9 = bytes of the staging buffer', hdr)
    assert 'zk_test_set_prove_segment' in hdr


def test_typings_and_facade_declare_the_call():
    dts = open(os.path.join(ROOT, 'bindings', 'napi', 'zkattest.d.ts')).read()
    assert re.search(r'export function proveSignatureLists\(', dts)
    assert re.search(r'\bproveBatchRings\(', dts)
    js = open(os.path.join(ROOT, 'bindings', 'napi', 'zkattest.js')).read()
    assert re.search(r'\bproveSignatureLists\b', js)
    assert os.path.exists(os.path.join(ROOT, 'bindings', 'napi', 'prove_rings_check.js'))


def test_null_arguments_are_refused():
    Z, L = _lib()
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    rng = Z.ZkRng(0, C.cast(C.create_string_buffer(32), vp), 0)
    w, ids = (u32 * 1)(), (u32 * 1)()
    off, ln, st = (u64 * 2)(), (u64 * 1)(), (C.c_int32 * 1)()
    out = C.create_string_buffer(64)
    b32, b64 = bytes(32), bytes(64)
    # no context / no pool
    assert L.zk_prove_batch_rings(vp(), u64(1), b32, b64, b64, w, ids, C.byref(rng), out, u64(64), off, st) == ZK_E_ARG
    assert L.zk_prove_batch_rings_device(vp(), u64(1), vp(1), vp(1), vp(1), vp(1), vp(1), C.byref(rng), vp(1), u64(64), vp(1), vp(1)) == ZK_E_ARG
    assert L.zk_pool_prove_batch_rings(vp(), u64(1), b32, b64, b64, w, ids, C.byref(rng), out, u64(64), off, ln, st) == ZK_E_ARG
    assert L.zk_prove_batch_rings(vp(), u64(0), None, None, None, None, None, None, None, u64(0), None, None) == ZK_E_ARG
