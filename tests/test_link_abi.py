"""not-gpu: the link-proof ABI (include/zkattest.h: zk_link_proof_size, zk_link_prove_batch, zk_link_verify_batch, zk_proof_key_commitments and their _device
forms) is declared with the argument lists the Python binding calls it with, exported by all three builds of the library and bound in Python; a ZKL1 proof
is 256 bytes in the library and in its layout header; and every entry point refuses what it can refuse before any device is touched."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZK_E_ARG = 14
CALLS = ['zk_link_prove_batch', 'zk_link_prove_batch_device', 'zk_link_verify_batch', 'zk_link_verify_batch_device', 'zk_proof_key_commitments',
         'zk_proof_key_commitments_device']
NEW = ['zk_link_proof_size'] + CALLS


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
    declared = set(re.findall(r'\b(zk_[a-z0-9_]+)\s*\(', _header()))
    for s in NEW:
        assert s in declared, s
        assert s in Z.SYMBOLS, s
        assert hasattr(L, s), s
    assert re.search(r'\buint64_t zk_link_proof_size\(void\);', _header())


def test_header_symbols_and_typings_name_the_same_calls():
    """header <-> SYMBOLS <-> zkattest.d.ts: every host-pointer call of the header is listed in SYMBOLS, and the typings declare the Engine method and the facade
    functions that reach it through an addon entry point calling exactly that symbol"""
    Z, _ = _lib()
    hdr = _header()
    napi = os.path.join(ROOT, 'bindings', 'napi')
    dts, addon = open(os.path.join(napi, 'zkattest.d.ts')).read(), open(os.path.join(napi, 'zkattest_napi.c')).read()
    engine = dts[dts.index('export class Engine {'):]
    names = {'zk_link_prove_batch': ('linkProveBatch', ['proveSameKey', 'proveSameKeys']), 'zk_link_verify_batch': ('linkVerifyBatch', ['verifySameKey', 'verifySameKeys']),
             'zk_proof_key_commitments': ('keyCommitments', ['keyCommitment', 'keyCommitments'])}
    header_calls = set(re.findall(r'\bzk_status (zk_link_[a-z_]+|zk_proof_key_commitments[a-z_]*)\(', hdr))
    assert header_calls == set(CALLS)
    assert {c for c in header_calls if not c.endswith('_device')} == set(names)
    for sym, (method, facade) in names.items():
        assert sym in Z.SYMBOLS and sym + '_device' in Z.SYMBOLS, sym
        assert re.search(r'^    %s\(' % method, engine, re.M), method
        assert re.search(r'\{"%s", \w+\}' % method, addon) and re.search(r'\b%s\(' % sym, addon), sym
        for f in facade:
            assert re.search(r'^export function %s\(' % f, dts, re.M), f
    # and nothing link-related in the typings or in SYMBOLS that the header does not have
    assert set(re.findall(r'^    (link[A-Za-z]+|keyCommitments)\(', engine, re.M)) == {m for m, _ in names.values()}
    assert {s for s in Z.SYMBOLS if s.startswith('zk_link_') or s.startswith('zk_proof_key_commitments')} == set(NEW)
    assert re.search(r'^export class LinkProof \{', dts, re.M)


def test_link_proof_size_is_256():
    Z, L = _lib()
    assert L.zk_link_proof_size.restype is C.c_uint64 and L.zk_link_proof_size() == 256


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
    assert [p.split()[-1].lstrip('*') for p in _prototype(hdr, 'zk_link_prove_batch')] == [
        'ctx', 'B', 'key_be32', 'com1_xy72', 'blinder1_be32', 'com2_xy72', 'blinder2_be32', 'rng', 'out', 'out_cap', 'per_proof_status']
    assert [p.split()[-1].lstrip('*') for p in _prototype(hdr, 'zk_link_verify_batch')] == ['ctx', 'B', 'com1_xy72', 'com2_xy72', 'proofs', 'ok', 'per_proof_status']
    assert [p.split()[-1].lstrip('*') for p in _prototype(hdr, 'zk_proof_key_commitments')] == ['ctx', 'B', 'proofs', 'proof_off', 'com_xy72', 'per_proof_status']
    for m in ('link_proof_size', 'link_prove_batch', 'link_prove_batch_device', 'link_verify_batch', 'link_verify_batch_device', 'proof_key_commitments',
              'proof_key_commitments_device'):
        assert callable(getattr(Z.Engine, m, None)), m


def test_header_states_the_contract():
    hdr = _header()
    assert re.search(r'header 16 B : "ZKL1" \| total_len u32 big-endian \(= 256\) \| 0 u32 \| 0 u32', hdr)
    for text in ('zk_link_prove_batch: the key and a', 'REDUCED mod q', 'there is no verifier_seeds argument', 'deliberately makes the two proofs linkable',
                 'rng must be independent of the seeds', '"link_respond"', '"link_ladder"', '"link_parse"'):
        assert text in hdr, text


def test_layout_header_agrees(tmp_path):
    """csrc/link.h is the one definition of the ZKL1 layout (host and device code include it)"""
    src = tmp_path / 'size.cpp'
    src.write_text('#define ZK_HOST_BUILD 1\n#include "link.h"\n#include <cstdio>\nint main() { printf("%u %u %x %u %u %u\\n", (unsigned)ZKL1_SIZE, (unsigned)ZKL1_HDR, '
                   '(unsigned)ZK_MAGIC_ZKL1, (unsigned)ZKL1_A1, (unsigned)ZKL1_A2, (unsigned)ZKL1_TX); }\n')
    exe = str(tmp_path / 'size')
    subprocess.check_call(['g++', '-std=c++17', '-Wno-unknown-pragmas', '-I', os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc'), str(src), '-o', exe])
    assert subprocess.check_output([exe]).decode().strip() == '256 16 %x 16 88 160' % int.from_bytes(b'ZKL1', 'little')


def test_arguments_are_refused_before_any_device_is_touched():
    Z, L = _lib()
    vp, u64 = C.c_void_p, C.c_uint64
    rng = Z.ZkRng(0, C.cast(C.create_string_buffer(32), vp), 0)
    st, off = (C.c_int32 * 1)(), (C.c_uint64 * 2)(0, 64)
    out, ok, com = C.create_string_buffer(256), C.create_string_buffer(1), C.create_string_buffer(72)
    assert L.zk_link_prove_batch(vp(), u64(1), bytes(32), bytes(72), bytes(32), bytes(72), bytes(32), C.byref(rng), out, u64(256), st) == ZK_E_ARG
    assert L.zk_link_prove_batch_device(vp(), u64(1), vp(4), vp(4), vp(4), vp(4), vp(4), C.byref(rng), vp(4), u64(256), vp(4)) == ZK_E_ARG
    assert L.zk_link_verify_batch(vp(), u64(1), bytes(72), bytes(72), bytes(256), ok, st) == ZK_E_ARG
    assert L.zk_link_verify_batch_device(vp(), u64(1), vp(4), vp(4), vp(4), vp(4), vp(4)) == ZK_E_ARG
    assert L.zk_proof_key_commitments(vp(), u64(1), bytes(64), off, com, st) == ZK_E_ARG
    assert L.zk_proof_key_commitments_device(vp(), u64(1), vp(4), vp(8), vp(4), vp(4)) == ZK_E_ARG
    assert L.zk_link_prove_batch(vp(), u64(0), None, None, None, None, None, None, None, u64(0), None) == ZK_E_ARG
