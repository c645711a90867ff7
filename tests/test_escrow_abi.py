"""not-gpu: the escrow-tag ABI (include/zkattest.h: zk_ctx_set_auditor, zk_escrow_keygen, zk_escrow_tag_size, zk_escrow_prove_batch, zk_escrow_verify_batch,
zk_escrow_open_batch and their _device forms) is declared with the argument lists the Python binding calls it with, exported by all three builds of the
library and bound in Python; a ZKT1 tag is 472 bytes in the library and in its layout header; the header states the contract; and every entry point refuses
what it can refuse before any device is touched."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZK_E_ARG = 14
CALLS = ['zk_ctx_set_auditor', 'zk_escrow_keygen', 'zk_escrow_prove_batch', 'zk_escrow_prove_batch_device', 'zk_escrow_verify_batch', 'zk_escrow_verify_batch_device',
         'zk_escrow_open_batch', 'zk_escrow_open_batch_device']
NEW = ['zk_escrow_tag_size'] + CALLS


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
    assert re.search(r'\buint64_t zk_escrow_tag_size\(void\);', hdr)
    assert set(re.findall(r'\b(?:zk_status|uint64_t) (zk_escrow_[a-z_]+)\(', hdr)) == set(NEW) - {'zk_ctx_set_auditor'}
    assert {s for s in Z.SYMBOLS if s.startswith('zk_escrow_')} == set(NEW) - {'zk_ctx_set_auditor'}


def test_header_symbols_and_typings_name_the_same_calls():
    """header <-> SYMBOLS <-> zkattest.d.ts: every host-pointer call of the header is listed in SYMBOLS, and the typings declare the Engine method and the facade
    functions that reach it through an addon entry point calling exactly that symbol"""
    Z, _ = _lib()
    napi = os.path.join(ROOT, 'bindings', 'napi')
    dts, addon = open(os.path.join(napi, 'zkattest.d.ts')).read(), open(os.path.join(napi, 'zkattest_napi.c')).read()
    engine = dts[dts.index('export class Engine {'):]
    names = {'zk_ctx_set_auditor': ('setAuditor', []), 'zk_escrow_keygen': ('escrowKeygen', ['escrowAuditorKey']),
             'zk_escrow_prove_batch': ('escrowProveBatch', ['proveEscrowTag', 'proveEscrowTags']),
             'zk_escrow_verify_batch': ('escrowVerifyBatch', ['verifyEscrowTag', 'verifyEscrowTags']), 'zk_escrow_open_batch': ('escrowOpenBatch', ['openEscrowTags'])}
    assert {c for c in CALLS if not c.endswith('_device')} == set(names)
    for sym, (method, facade) in names.items():
        assert sym in Z.SYMBOLS, sym
        assert re.search(r'^    %s\(' % method, engine, re.M), method
        assert re.search(r'\{"%s", \w+\}' % method, addon) and re.search(r'\b%s\(' % sym, addon), sym
        for f in facade:
            assert re.search(r'^export function %s\(' % f, dts, re.M), f
    assert set(re.findall(r'^    (escrow[A-Za-z]+|setAuditor)\(', engine, re.M)) == {m for m, _ in names.values()}
    assert re.search(r'^export class EscrowTag \{', dts, re.M)


def test_tag_size_is_472():
    Z, L = _lib()
    assert L.zk_escrow_tag_size.restype is C.c_uint64 and L.zk_escrow_tag_size() == 472


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
            if '*' in p or '[' in p:
                assert a in (C.c_void_p, C.c_char_p) or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert p.startswith('uint64_t ') and a is C.c_uint64, (name, p, a)
    def names(call):
        return [re.sub(r'\[\d+\]$', '', p.split()[-1].lstrip('*')) for p in _prototype(hdr, call)]
    assert names('zk_ctx_set_auditor') == ['ctx', 'auditor_xy72']
    assert names('zk_escrow_keygen') == ['ctx', 'secret_be32', 'auditor_xy72']
    assert names('zk_escrow_prove_batch') == ['ctx', 'B', 'key_be32', 'com_xy72', 'blinder_be32', 'rng', 'out', 'out_cap', 'per_tag_status']
    assert names('zk_escrow_verify_batch') == ['ctx', 'B', 'com_xy72', 'tags', 'ok', 'per_tag_status']
    assert names('zk_escrow_open_batch') == ['ctx', 'B', 'secret_be32', 'tags', 'index_u32', 'per_tag_status']
    for m in ('set_auditor', 'escrow_keygen', 'escrow_tag_size', 'escrow_prove_batch', 'escrow_prove_batch_device', 'escrow_verify_batch', 'escrow_verify_batch_device',
              'escrow_open_batch', 'escrow_open_batch_device'):
        assert callable(getattr(Z.Engine, m, None)), m


def test_header_states_the_contract():
    hdr = _header()
    assert re.search(r'header 16 B : "ZKT1" \| total_len u32 big-endian \(= 472\) \| 0 u32 \| 0 u32', hdr)
    for text in ('c = hashPoints([C, E1, E2, A, T1, T2, T3])', 'fill 0 is rho, 1 k_x, 2 k_r,', 'REDUCED mod q, not refused', 'no verifier_seeds argument',
                 '4 y_i g = 4 E2 - a (4 E1)', 'The factor 4 is part of the rule', 'It is bound to C and to A, not to a message or a ring', 'Opening does not verify',
                 "rng must be independent of the seeds C's proof was made with", 'Anyone who knows a can open every tag made for A', 'zk_ctx_set_params drops it',
                 '"escrow_front"', '"escrow_respond"', '"escrow_parse"', '"escrow_ladder"', '"escrow_open"', '"escrow_ring_points"', '"escrow_match"',
                 'Not provided: submit / wait, zk_pool_*, JSON.', 'is rebuilt by every call'):
        assert text in hdr, text


def test_layout_header_agrees(tmp_path):
    """csrc/escrow.h is the one definition of the ZKT1 layout (host and device code include it)"""
    src = tmp_path / 'size.cpp'
    src.write_text('#define ZK_HOST_BUILD 1\n#include "escrow.h"\n#include <cstdio>\nint main() { printf("%u %u %x %u %u %u %u %u\\n", (unsigned)ZKT1_SIZE, (unsigned)ZKT1_HDR, '
                   '(unsigned)ZK_MAGIC_ZKT1, (unsigned)ZKT1_PT(0), (unsigned)ZKT1_PT(4), (unsigned)ZKT1_SC(0), (unsigned)ZKT1_SC(2), (unsigned)ZKT1_MSG_BLOCKS); }\n')
    exe = str(tmp_path / 'size')
    subprocess.check_call(['g++', '-std=c++17', '-Wno-unknown-pragmas', '-I', os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc'), str(src), '-o', exe])
    assert subprocess.check_output([exe]).decode().strip() == '472 16 %x 16 304 376 440 8' % int.from_bytes(b'ZKT1', 'little')


def test_arguments_are_refused_before_any_device_is_touched():
    Z, L = _lib()
    vp, u64 = C.c_void_p, C.c_uint64
    rng = Z.ZkRng(0, C.cast(C.create_string_buffer(32), vp), 0)
    st, idx = (C.c_int32 * 1)(), (C.c_uint32 * 1)()
    out, ok, key = C.create_string_buffer(472), C.create_string_buffer(1), C.create_string_buffer(72)
    assert L.zk_ctx_set_auditor(vp(), bytes(72)) == ZK_E_ARG
    assert L.zk_escrow_keygen(vp(), bytes(32), key) == ZK_E_ARG
    assert L.zk_escrow_prove_batch(vp(), u64(1), bytes(32), bytes(72), bytes(32), C.byref(rng), out, u64(472), st) == ZK_E_ARG
    assert L.zk_escrow_prove_batch_device(vp(), u64(1), vp(4), vp(4), vp(4), C.byref(rng), vp(4), u64(472), vp(4)) == ZK_E_ARG
    assert L.zk_escrow_verify_batch(vp(), u64(1), bytes(72), bytes(472), ok, st) == ZK_E_ARG
    assert L.zk_escrow_verify_batch_device(vp(), u64(1), vp(4), vp(4), vp(4), vp(4)) == ZK_E_ARG
    assert L.zk_escrow_open_batch(vp(), u64(1), bytes(32), bytes(472), idx, st) == ZK_E_ARG
    assert L.zk_escrow_open_batch_device(vp(), u64(1), vp(4), vp(4), vp(4), vp(4)) == ZK_E_ARG
    assert L.zk_escrow_prove_batch(vp(), u64(0), None, None, None, None, None, u64(0), None) == ZK_E_ARG
