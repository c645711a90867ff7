"""not-gpu: the ABI of the quorum calls with one ring id per member (include/zkattest.h: zk_rings_quorum_proof_max_size, zk_rings_quorum_prove_batch,
zk_rings_quorum_verify_batch and their _device forms) is declared with the argument lists the Python binding calls it with, exported by all three builds of
the library, listed in SYMBOLS and bound in Python; every entry point refuses what it can refuse before any device is touched; the header states the contract."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZK_E_ARG = 14
CALLS = ['zk_rings_quorum_prove_batch', 'zk_rings_quorum_prove_batch_device', 'zk_rings_quorum_verify_batch', 'zk_rings_quorum_verify_batch_device']
NEW = ['zk_rings_quorum_proof_max_size'] + CALLS


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


def test_header_symbols_and_native_name_the_same_calls():
    Z, L = _lib()
    hdr = _header()
    assert set(re.findall(r'\b(zk_rings_quorum_[a-z_]+)\s*\(', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S))) == set(NEW)
    assert re.search(r'\buint64_t zk_rings_quorum_proof_max_size\(const zk_ctx \*ctx, uint32_t k, const uint32_t \*ring_ids\s*(/\*k\*/)?\);', hdr)
    assert {s for s in Z.SYMBOLS if s.startswith('zk_rings_quorum_')} == set(NEW)
    for s in NEW:
        assert hasattr(L, s), s
    assert L.zk_rings_quorum_proof_max_size.restype is C.c_uint64


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
            elif p.startswith('uint32_t '):
                assert a is C.c_uint32, (name, p, a)
            else:
                assert p.startswith('uint64_t ') and a is C.c_uint64, (name, p, a)
    names = lambda n: [p.split()[-1].lstrip('*') for p in _prototype(hdr, n)]
    # the one-ring argument lists with ring_ids behind which / bundle_off
    assert names('zk_rings_quorum_prove_batch') == ['ctx', 'Q', 'k', 'msg_hash', 'sig', 'pk_xy', 'which', 'ring_ids', 'rng', 'rng_pairs', 'out', 'out_cap', 'out_off',
                                                    'per_quorum_status', 'per_member_status']
    assert names('zk_rings_quorum_verify_batch') == ['ctx', 'Q', 'k', 'msg_hash', 'bundles', 'bundle_off', 'ring_ids', 'verifier_seeds', 'ok', 'per_quorum_status', 'first_bad']
    one = lambda n: [p for p in names(n) if 'ring_ids' not in p]
    for n in ('zk_quorum_prove_batch', 'zk_quorum_prove_batch_device', 'zk_quorum_verify_batch', 'zk_quorum_verify_batch_device'):
        assert one(n.replace('zk_quorum_', 'zk_rings_quorum_')) == names(n), n


def test_python_signatures():
    Z, _ = _lib()
    sig = lambda m: list(inspect.signature(getattr(Z.Engine, m)).parameters)
    assert sig('quorum_proof_max_size_rings') == ['self', 'k', 'ring_ids']
    assert sig('quorum_prove_batch_rings')[:9] == ['self', 'k', 'msg', 'sig', 'pk', 'which', 'ring_ids', 'seeds', 'pair_seeds']
    assert sig('quorum_verify_batch_rings')[:6] == ['self', 'k', 'msg', 'bundles', 'ring_ids', 'verifier_seeds']
    assert inspect.signature(Z.Engine.quorum_verify_batch_rings).parameters['verifier_seeds'].default is None
    for m in ('quorum_prove_batch_rings_device', 'quorum_verify_batch_rings_device'):
        assert callable(getattr(Z.Engine, m, None)), m


def test_header_states_the_contract():
    hdr = _header()
    for text in ('The wire format\n * is ZKQ1, unchanged', 'k different KEYS mod q', 'hardened mode each hashes the digest of its own ring',
                 'ZK_E_ARG for an id that is not resident', 'The active ring is neither read nor changed', 'a member\n *   whose id is not resident counting 0',
                 'one kernel, one read-back', '"quorum_caps"', 'Still not provided: submit / wait forms, zk_pool_* forms, JSON, a caller-context binding',
                 'zk_rings_quorum_proof_max_size(ctx, k, ring_ids) = 16 + the sum of zk_ring_proof_max_size(ctx, ring_ids[i]) over the k members + 744 P'):
        assert text in hdr, text
    assert 'what the\n * zk_quorum_* calls above do not provide' in hdr   # the one-ring block keeps its "Not provided: one ring id per member"
    for doc in ('README.md', 'INTEGRATION.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'zk_rings_quorum_prove_batch' in text and 'Not provided: one ring id per member' not in text, doc


def test_arguments_are_refused_before_any_device_is_touched():
    """the argument checks in their order: a NULL context or required pointer first (nothing else is looked at), Q = 0 needs no array"""
    Z, L = _lib()
    vp, u64 = C.c_void_p, C.c_uint64
    rng = Z.ZkRng(0, C.cast(C.create_string_buffer(64), vp), 0)
    st = (C.c_int32 * 2)()
    ids = (C.c_uint32 * 2)()
    off = (C.c_uint64 * 2)()
    out, ok = C.create_string_buffer(64), C.create_string_buffer(1)
    assert L.zk_rings_quorum_proof_max_size(None, 2, ids) == 0
    assert L.zk_rings_quorum_prove_batch(vp(), u64(1), 2, bytes(64), bytes(128), bytes(128), st, ids, C.byref(rng), C.byref(rng), out, u64(64), off, st, None) == ZK_E_ARG
    assert L.zk_rings_quorum_prove_batch(vp(), u64(0), 2, None, None, None, None, None, C.byref(rng), C.byref(rng), None, u64(0), off, None, None) == ZK_E_ARG
    assert L.zk_rings_quorum_prove_batch_device(vp(), u64(1), 2, vp(4), vp(4), vp(4), vp(4), vp(4), C.byref(rng), C.byref(rng), vp(4), u64(64), vp(8), vp(4), None) == ZK_E_ARG
    assert L.zk_rings_quorum_verify_batch(vp(), u64(1), 2, bytes(64), bytes(64), off, ids, None, ok, st, None) == ZK_E_ARG
    assert L.zk_rings_quorum_verify_batch_device(vp(), u64(1), 2, vp(4), vp(4), vp(8), vp(4), None, vp(4), vp(4), None) == ZK_E_ARG
