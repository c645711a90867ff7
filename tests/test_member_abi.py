"""not-gpu: the membership ABI (include/zkattest.h: zk_member_proof_size, zk_member_prove_batch, zk_member_verify_batch and their _device forms) is declared
with the argument lists the Python binding calls it with, exported by all three builds of the library and bound in Python; the ZKM1 size formula of the
library's own layout header holds for n = 1..20; and every entry point refuses what it can refuse before any device is touched."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZK_E_ARG = 14
CALLS = ['zk_member_prove_batch', 'zk_member_prove_batch_device', 'zk_member_verify_batch', 'zk_member_verify_batch_device']
NEW = ['zk_member_proof_size'] + CALLS


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
    assert re.search(r'\buint64_t zk_member_proof_size\(const zk_ctx \*ctx\);', _header())


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
    assert [p.split()[-1].lstrip('*') for p in _prototype(hdr, 'zk_member_prove_batch')] == [
        'ctx', 'B', 'which', 'blinder_be32', 'rng', 'com_xy72', 'blinder_out', 'out', 'out_cap', 'per_proof_status']
    assert [p.split()[-1].lstrip('*') for p in _prototype(hdr, 'zk_member_verify_batch')] == [
        'ctx', 'B', 'com_xy72', 'proofs', 'verifier_seeds', 'ok', 'per_proof_status']
    assert L.zk_member_proof_size.restype is C.c_uint64
    for m in ('member_proof_size', 'member_prove_batch', 'member_prove_batch_device', 'member_verify_batch', 'member_verify_batch_device'):
        assert callable(getattr(Z.Engine, m, None)), m


def test_zkm1_is_documented_next_to_zka1():
    hdr = _header()
    a, m = hdr.index('"ZKA1" layout'), hdr.index('"ZKM1" layout')
    assert a < m < hdr.index('#ifndef ZKATTEST_H')
    assert re.search(r'header 16 B : "ZKM1" \| total_len u32 \| n = log2\(padded ring\) u32 \| 0 u32', hdr)


def test_size_formula_of_the_layout_header(tmp_path):
    """csrc/wire.h is the one definition of the ZKM1 size (host and device code include it): 16 + 288 n + 32 (3 n + 1) for n = 1..20, 6192 at n = 16"""
    src = tmp_path / 'size.cpp'
    src.write_text('#include "wire.h"\n#include <cstdio>\nint main() { for (unsigned n = 1; n <= 20; n++) printf("%llu\\n", (unsigned long long)zkm1_size(n));'
                   ' printf("%u %x\\n", (unsigned)ZKM1_HDR, (unsigned)ZK_MAGIC_ZKM1); }\n')
    exe = str(tmp_path / 'size')
    subprocess.check_call(['g++', '-std=c++17', '-I', os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc'), str(src), '-o', exe])
    lines = subprocess.check_output([exe]).decode().split('\n')
    assert [int(x) for x in lines[:20]] == [16 + 288 * n + 32 * (3 * n + 1) for n in range(1, 21)]
    assert int(lines[15]) == 6192
    assert lines[20] == '16 %x' % int.from_bytes(b'ZKM1', 'little')


def test_arguments_are_refused_before_any_device_is_touched():
    Z, L = _lib()
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    rng = Z.ZkRng(0, C.cast(C.create_string_buffer(32), vp), 0)
    w, st = (u32 * 1)(), (C.c_int32 * 1)()
    com, out, ok = C.create_string_buffer(72), C.create_string_buffer(1200), C.create_string_buffer(1)
    assert L.zk_member_proof_size(vp()) == 0   # no context: no ring
    assert L.zk_member_prove_batch(vp(), u64(1), w, None, C.byref(rng), com, None, out, u64(1200), st) == ZK_E_ARG
    assert L.zk_member_prove_batch_device(vp(), u64(1), vp(1), None, C.byref(rng), vp(1), None, vp(1), u64(1200), vp(1)) == ZK_E_ARG
    assert L.zk_member_verify_batch(vp(), u64(1), bytes(72), bytes(1200), None, ok, st) == ZK_E_ARG
    assert L.zk_member_verify_batch_device(vp(), u64(1), vp(1), vp(1), None, vp(1), vp(1)) == ZK_E_ARG
    assert L.zk_member_prove_batch(vp(), u64(0), None, None, None, None, None, None, u64(0), None) == ZK_E_ARG
