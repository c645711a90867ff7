"""not-gpu: the mixed-ring membership ABI (include/zkattest.h: zk_member_proof_size_ring, zk_member_prove_batch_rings, zk_member_verify_batch_rings and their
_device forms) is declared with the argument lists the Python binding calls it with, exported by all three builds of the library and bound in Python; the
header no longer lists _rings forms as missing; the facade exports the two key-list functions and the typings name them; every entry point refuses what it can
refuse before any device is touched."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAPI = os.path.join(ROOT, 'bindings', 'napi')
ZK_E_ARG = 14
CALLS = ['zk_member_prove_batch_rings', 'zk_member_prove_batch_rings_device', 'zk_member_verify_batch_rings', 'zk_member_verify_batch_rings_device']
NEW = ['zk_member_proof_size_ring'] + CALLS


def _lib():
    import zkp_ecdsa_amd as Z
    if not os.path.exists(Z.LIB_PATH):
        Z.build()
    return Z, Z.lib()


def _header():
    return open(os.path.join(ROOT, 'include', 'zkattest.h')).read()


def _prototype(hdr, name):
    m = re.search(r'\bzk_status %s\((.*?)\);' % name, hdr, re.S)
    assert m, name
    text = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    return [' '.join(p.split()) for p in text.split(',')]


def test_symbols_declared_exported_and_listed():
    Z, L = _lib()
    hdr = _header()
    declared = set(re.findall(r'\b(zk_[a-z0-9_]+)\s*\(', hdr))
    for s in NEW:
        assert s in declared, s
        assert s in Z.SYMBOLS, s
        assert hasattr(L, s), s
    assert re.search(r'\buint64_t zk_member_proof_size_ring\(const zk_ctx \*ctx, uint32_t ring\);', hdr)
    assert re.search(r'\buint64_t zk_member_proof_size\(const zk_ctx \*ctx\);', hdr)
    # the membership block's list of what is not provided: the _rings forms have left it, the others stay
    m = re.search(r'Not provided: ([^\n]*?)\. \*/\s*uint64_t zk_member_proof_size\(', hdr)
    assert m, 'the membership block ends with its "Not provided" line'
    assert '_rings' not in m.group(1)
    for kept in ('submit / wait', 'zk_pool_*', 'JSON', 'packed'):
        assert kept in m.group(1), kept
    assert re.search(r'\b13 = windows that mixed-ring membership calls', hdr)


@pytest.mark.parametrize('name', ['libzkattest_hip.so', 'libzkattest_hip_uniform.so', 'libzkattest_hip_testhooks.so'])
def test_every_build_exports_the_calls(name):
    Z, _ = _lib()
    path = os.path.join(os.path.dirname(Z.LIB_PATH), name)
    assert os.path.exists(path), 'not built: ' + name
    L = C.CDLL(path)
    for s in NEW:
        assert hasattr(L, s), (name, s)


def test_header_and_ctypes_prototypes_agree():
    Z, L = _lib()
    hdr = _header()
    for name in CALLS:
        params = _prototype(hdr, name)
        argtypes = getattr(L, name).argtypes
        assert argtypes is not None and len(argtypes) == len(params), (name, params)
        for p, a in zip(params, argtypes):
            if '*' in p:
                assert a in (C.c_void_p, C.c_char_p) or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert p.startswith('uint64_t ') and a is C.c_uint64, (name, p, a)
    assert [p.split()[-1].lstrip('*') for p in _prototype(hdr, 'zk_member_prove_batch_rings')] == [
        'ctx', 'B', 'which', 'ring_ids', 'blinder_be32', 'rng', 'com_xy72', 'blinder_out', 'out', 'out_cap', 'out_off', 'per_proof_status']
    assert [p.split()[-1].lstrip('*') for p in _prototype(hdr, 'zk_member_verify_batch_rings')] == [
        'ctx', 'B', 'com_xy72', 'proofs', 'proof_off', 'ring_ids', 'verifier_seeds', 'ok', 'per_proof_status']
    assert L.zk_member_proof_size_ring.restype is C.c_uint64 and list(L.zk_member_proof_size_ring.argtypes) == [C.c_void_p, C.c_uint32]


def test_engine_methods_exist():
    import inspect
    Z, _ = _lib()
    for m in ('member_prove_batch_rings', 'member_prove_batch_rings_device', 'member_verify_batch_rings', 'member_verify_batch_rings_device'):
        assert callable(getattr(Z.Engine, m, None)), m
    assert list(inspect.signature(Z.Engine.member_proof_size).parameters) == ['self', 'ring']
    assert inspect.signature(Z.Engine.member_proof_size).parameters['ring'].default is None   # None: the active ring, as before
    sig = inspect.signature(Z.Engine.member_prove_batch_rings).parameters
    assert list(sig)[:8] == ['self', 'which', 'ring_ids', 'blinders', 'seeds', 'streams', 'stream_blocks', 'want_blinders']
    assert list(inspect.signature(Z.Engine.member_verify_batch_rings).parameters)[:5] == ['self', 'coms', 'proofs', 'ring_ids', 'vseeds']


def test_facade_exports_and_typings():
    js = open(os.path.join(NAPI, 'zkattest.js')).read()
    dts = open(os.path.join(NAPI, 'zkattest.d.ts')).read()
    exports = js[js.rindex('module.exports'):]
    for name in ('proveMembershipLists', 'verifyMembershipLists'):
        assert re.search(r'\b%s\b' % name, exports), name
        assert re.search(r'export function %s\(' % name, dts), name
    assert os.path.exists(os.path.join(NAPI, 'member_rings_check.js'))


def test_arguments_are_refused_before_any_device_is_touched():
    Z, L = _lib()
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    rng = Z.ZkRng(0, C.cast(C.create_string_buffer(32), vp), 0)
    w, ids, st, off = (u32 * 1)(), (u32 * 1)(), (C.c_int32 * 1)(), (u64 * 2)()
    com, out, ok = C.create_string_buffer(72), C.create_string_buffer(1200), C.create_string_buffer(1)
    assert L.zk_member_proof_size_ring(vp(), u32(0)) == 0   # no context: no ring
    assert L.zk_member_prove_batch_rings(vp(), u64(1), w, ids, None, C.byref(rng), com, None, out, u64(1200), off, st) == ZK_E_ARG
    assert L.zk_member_prove_batch_rings_device(vp(), u64(1), vp(1), vp(1), None, C.byref(rng), vp(1), None, vp(1), u64(1200), vp(1), vp(1)) == ZK_E_ARG
    assert L.zk_member_verify_batch_rings(vp(), u64(1), bytes(72), bytes(1200), off, ids, None, ok, st) == ZK_E_ARG
    assert L.zk_member_verify_batch_rings_device(vp(), u64(1), vp(1), vp(1), vp(1), vp(1), None, vp(1), vp(1)) == ZK_E_ARG
