"""not-gpu: the quorum ABI (include/zkattest.h: zk_quorum_pair_count, zk_quorum_proof_max_size, zk_quorum_prove_batch, zk_quorum_verify_batch and their
_device forms) is declared with the argument lists the Python binding calls it with, exported by all three builds of the library, listed in SYMBOLS, bound in
Python and named by the N-API typings; zk_quorum_pair_count counts the pairs; and every entry point refuses what it can refuse before any device is touched."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZK_E_ARG = 14
CALLS = ['zk_quorum_prove_batch', 'zk_quorum_prove_batch_device', 'zk_quorum_verify_batch', 'zk_quorum_verify_batch_device']
NEW = ['zk_quorum_pair_count', 'zk_quorum_proof_max_size'] + CALLS


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


def test_header_symbols_native_and_typings_name_the_same_calls():
    Z, L = _lib()
    hdr = _header()
    assert set(re.findall(r'\b(zk_quorum_[a-z_]+)\s*\(', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S))) == set(NEW)
    assert re.search(r'\buint64_t zk_quorum_pair_count\(uint32_t k\);', hdr) and re.search(r'\buint64_t zk_quorum_proof_max_size\(const zk_ctx \*ctx, uint32_t k\);', hdr)
    assert {s for s in Z.SYMBOLS if s.startswith('zk_quorum_')} == set(NEW)
    for s in NEW:
        assert hasattr(L, s), s
    napi = os.path.join(ROOT, 'bindings', 'napi')
    dts, addon = open(os.path.join(napi, 'zkattest.d.ts')).read(), open(os.path.join(napi, 'zkattest_napi.c')).read()
    engine = dts[dts.index('export class Engine {'):]
    names = {'zk_quorum_prove_batch': ('quorumProveBatch', 'proveQuorum'), 'zk_quorum_verify_batch': ('quorumVerifyBatch', 'verifyQuorum')}
    for sym, (method, facade) in names.items():
        assert re.search(r'^    %s\(' % method, engine, re.M), method
        assert re.search(r'\{"%s", \w+\}' % method, addon) and re.search(r'\b%s\(' % sym, addon), sym
        assert re.search(r'^export function %s\(' % facade, dts, re.M), facade
    assert set(re.findall(r'^    (quorum[A-Za-z]+)\(', engine, re.M)) == {m for m, _ in names.values()}
    assert re.search(r'^export class QuorumProof \{', dts, re.M)
    for m in ('quorum_pair_count', 'quorum_proof_max_size', 'quorum_prove_batch', 'quorum_prove_batch_device', 'quorum_verify_batch', 'quorum_verify_batch_device'):
        assert callable(getattr(Z.Engine, m, None)), m


def test_pair_count_values():
    Z, L = _lib()
    assert L.zk_quorum_pair_count.restype is C.c_uint64 and L.zk_quorum_proof_max_size.restype is C.c_uint64
    for k in range(0, 20):
        want = k * (k - 1) // 2 if 2 <= k <= 16 else 0
        assert L.zk_quorum_pair_count(k) == want == (len(Z.Engine.distinct_pairs(k)) if 2 <= k <= 16 else 0), k
    assert L.zk_quorum_pair_count(16) == 120 and L.zk_quorum_pair_count(0xFFFFFFFF) == 0
    assert L.zk_quorum_proof_max_size(None, 3) == 0


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
    assert [p.split()[-1].lstrip('*') for p in _prototype(hdr, 'zk_quorum_prove_batch')] == [
        'ctx', 'Q', 'k', 'msg_hash', 'sig', 'pk_xy', 'which', 'rng', 'rng_pairs', 'out', 'out_cap', 'out_off', 'per_quorum_status', 'per_member_status']
    assert [p.split()[-1].lstrip('*') for p in _prototype(hdr, 'zk_quorum_verify_batch')] == [
        'ctx', 'Q', 'k', 'msg_hash', 'bundles', 'bundle_off', 'verifier_seeds', 'ok', 'per_quorum_status', 'first_bad']


def test_header_states_the_contract():
    hdr = _header()
    assert re.search(r'header 16 B : "ZKQ1" \| total_len u32 big-endian \| k u32 big-endian \| 0 u32', hdr)
    for text in ('rng_pairs must be independent of rng', 'its attestations come from different signers', 'in that direction',
                 'Not provided: one ring id per member, submit / wait forms, zk_pool_* forms, JSON, a caller-context binding',
                 '"quorum_blinders"', '"quorum_gather"', '"quorum_layout"', '"quorum_walk"', '"quorum_verdict"', 'zk_quorum_proof_max_size(ctx, k) = 16 + k zk_proof_max_size(ctx) + 744 P'):
        assert text in hdr, text


def test_arguments_are_refused_before_any_device_is_touched():
    Z, L = _lib()
    vp, u64 = C.c_void_p, C.c_uint64
    rng = Z.ZkRng(0, C.cast(C.create_string_buffer(64), vp), 0)
    st = (C.c_int32 * 2)()
    off = (C.c_uint64 * 2)()
    out, ok = C.create_string_buffer(64), C.create_string_buffer(1)
    assert L.zk_quorum_prove_batch(vp(), u64(1), 2, bytes(64), bytes(128), bytes(128), st, C.byref(rng), C.byref(rng), out, u64(64), off, st, None) == ZK_E_ARG
    assert L.zk_quorum_prove_batch_device(vp(), u64(1), 2, vp(4), vp(4), vp(4), vp(4), C.byref(rng), C.byref(rng), vp(4), u64(64), vp(8), vp(4), None) == ZK_E_ARG
    assert L.zk_quorum_verify_batch(vp(), u64(1), 2, bytes(64), bytes(64), off, None, ok, st, None) == ZK_E_ARG
    assert L.zk_quorum_verify_batch_device(vp(), u64(1), 2, vp(4), vp(4), vp(8), None, vp(4), vp(4), None) == ZK_E_ARG
