"""not-gpu: the ABI of the opening against any resident ring (include/zkattest.h: zk_rings_escrow_open_batch and its _device form, ZK_ESCROW_RING_ANY) is
declared with the argument lists the Python binding calls it with, exported by all three builds of the library, bound in Python and in the N-API typings; the
header states the contract; and the entry points refuse a NULL context before any device is touched."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZK_E_ARG = 14
CALLS = ['zk_rings_escrow_open_batch', 'zk_rings_escrow_open_batch_device']


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
    for s in CALLS:
        assert s in declared and s in Z.SYMBOLS and hasattr(L, s), s
    assert {s for s in Z.SYMBOLS if 'escrow' in s and s.startswith('zk_rings_')} == set(CALLS)
    assert re.search(r'^#define ZK_ESCROW_RING_ANY 0xffffffffu$', hdr, re.M) and Z.ESCROW_RING_ANY == 0xffffffff


def test_header_symbols_and_typings_name_the_same_calls():
    Z, _ = _lib()
    napi = os.path.join(ROOT, 'bindings', 'napi')
    dts, addon = open(os.path.join(napi, 'zkattest.d.ts')).read(), open(os.path.join(napi, 'zkattest_napi.c')).read()
    engine = dts[dts.index('export class Engine {'):]
    assert re.search(r'^    ringsEscrowOpenBatch\(', engine, re.M)
    assert re.search(r'\{"ringsEscrowOpenBatch", \w+\}', addon) and re.search(r'\bzk_rings_escrow_open_batch\(', addon)
    assert len(re.findall(r'^export function openEscrowTags\(', dts, re.M)) == 2   # the one-ring form and the one with a key list per tag


@pytest.mark.parametrize('name', ['libzkattest_hip.so', 'libzkattest_hip_uniform.so', 'libzkattest_hip_testhooks.so'])
def test_every_build_exports_the_calls(name):
    Z, _ = _lib()
    path = os.path.join(os.path.dirname(Z.LIB_PATH), name)
    assert os.path.exists(path), 'not built: ' + name
    L = C.CDLL(path)
    for s in CALLS:
        assert hasattr(L, s), (name, s)


def test_header_and_ctypes_prototypes_agree():
    Z, L = _lib()
    hdr = _header()
    for name in CALLS:
        params = _prototype(hdr, name)
        argtypes = getattr(L, name).argtypes
        assert argtypes is not None and len(argtypes) == len(params) == 8, (name, params)
        for p, a in zip(params, argtypes):
            if '*' in p or '[' in p:
                assert a in (C.c_void_p, C.c_char_p) or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert p.startswith('uint64_t ') and a is C.c_uint64, (name, p, a)
    names = [re.sub(r'\[\d+\]$', '', p.split()[-1].lstrip('*')) for p in _prototype(hdr, CALLS[0])]
    assert names == ['ctx', 'B', 'secret_be32', 'tags', 'ring_ids', 'ring_out_u32', 'index_u32', 'per_tag_status']
    for m in ('escrow_open_batch_rings', 'escrow_open_batch_rings_device'):
        assert callable(getattr(Z.Engine, m, None)), m


def test_header_states_the_contract():
    hdr = ' '.join(_header().split())
    for text in ('ZK_ESCROW_RING_ANY: the resident rings are then searched in ascending id order', 'The ACTIVE ring is neither read nor changed',
                 '"no active ring" is no refusal', 'ZK_E_ARG when ring_ids[b] is neither resident nor ZK_ESCROW_RING_ANY (before the tag\'s bytes are judged)',
                 'ring_out and index are both 0xffffffff unless the status is 0 and a match exists', 'h = w0 * 0x9e3779b1 + w1 * 0x85ebca6b',
                 'slot = h & (slots - 1)', 'linear probing with wrap-around', 'zk_ctx_set_params drop it', 'no tombstones',
                 '"escrow_index_build"', '"escrow_lookup"', 'Not provided: pool, streamed and JSON forms.',
                 'is rebuilt by every call'):   # (zk_escrow_open_batch keeps its code path and its documentation)
        assert text in hdr, text


def test_a_null_context_is_refused_before_any_device_is_touched():
    Z, L = _lib()
    vp, u64 = C.c_void_p, C.c_uint64
    ids, ring, idx, st = (C.c_uint32 * 1)(), (C.c_uint32 * 1)(), (C.c_uint32 * 1)(), (C.c_int32 * 1)()
    assert L.zk_rings_escrow_open_batch(vp(), u64(1), bytes(32), bytes(472), ids, ring, idx, st) == ZK_E_ARG
    assert L.zk_rings_escrow_open_batch_device(vp(), u64(1), vp(4), vp(4), vp(4), vp(4), vp(4), vp(4)) == ZK_E_ARG
    assert L.zk_rings_escrow_open_batch(vp(), u64(0), None, None, None, None, None, None) == ZK_E_ARG
