"""not-gpu: the bound-membership ABI (include/zkattest.h: the eight zk_member_*_bound entry points) is declared with the argument lists the Python binding
calls it with -- the unbound call's list with `context` after `which` (prove) or after com_xy72 (verify) --, exported by all three builds of the library and
bound in Python, where Engine's member calls take context / d_context keywords; the header documents "ZKMB", the statement's bytes and what a ring update
does to old proofs; the "ZKMB" magic and the statement's length are the layout headers'; a NULL context is refused before any device is touched."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZK_E_ARG = 14
BASE = ['zk_member_prove_batch', 'zk_member_prove_batch_device', 'zk_member_verify_batch', 'zk_member_verify_batch_device',
        'zk_member_prove_batch_rings', 'zk_member_prove_batch_rings_device', 'zk_member_verify_batch_rings', 'zk_member_verify_batch_rings_device']


def _bound(name):
    return name[:-len('_device')] + '_bound_device' if name.endswith('_device') else name + '_bound'


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
    for s in map(_bound, BASE):
        assert s in declared and s in Z.SYMBOLS and hasattr(L, s), s


@pytest.mark.parametrize('name', ['libzkattest_hip.so', 'libzkattest_hip_uniform.so', 'libzkattest_hip_testhooks.so'])
def test_every_build_exports_the_calls(name):
    Z, _ = _lib()
    path = os.path.join(os.path.dirname(Z.LIB_PATH), name)
    assert os.path.exists(path), 'not built: ' + name
    L = C.CDLL(path)
    for s in map(_bound, BASE):
        assert hasattr(L, s), (name, s)


def test_a_bound_prototype_is_the_unbound_one_with_the_context_in_its_place():
    Z, L = _lib()
    hdr = _header()
    for base in BASE:
        name, dev = _bound(base), base.endswith('_device')
        old, new = _prototype(hdr, base), _prototype(hdr, name)
        after = ('d_which' if dev else 'which') if 'prove' in base else ('d_com_xy72' if dev else 'com_xy72')
        at = [p.split()[-1].lstrip('*') for p in old].index(after) + 1
        want = old[:at] + ['const void *d_context' if dev else 'const uint8_t *context'] + old[at:]
        assert new == want, (name, new)
        argtypes = getattr(L, name).argtypes
        assert argtypes is not None and len(argtypes) == len(new) == len(getattr(L, base).argtypes) + 1, name
        for p, a in zip(new, argtypes):
            if '*' in p:
                assert a in (C.c_void_p, C.c_char_p) or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert p.startswith('uint64_t ') and a is C.c_uint64, (name, p, a)


def test_engine_keywords():
    Z, _ = _lib()
    for m in ('member_prove_batch', 'member_verify_batch', 'member_prove_batch_rings', 'member_verify_batch_rings'):
        p = inspect.signature(getattr(Z.Engine, m)).parameters
        assert 'context' in p and p['context'].default is None, m
        p = inspect.signature(getattr(Z.Engine, m + '_device')).parameters
        assert 'd_context' in p and p['d_context'].default is None, m


def test_header_documents_the_statement_and_the_ring_update():
    hdr = _header()
    assert hdr.index('"ZKM1" layout') < hdr.index('"ZKMB"') < hdr.index('#ifndef ZKATTEST_H')
    sec = hdr[hdr.index('Bound membership proofs, "ZKMB"'):hdr.index('zk_status zk_member_prove_batch_bound(')]
    for needle in ('"ZKAttest-GK-member-v1" (21 bytes', 'ring digest (32', 'context_b (32)', '04 || com_b.x (33', '152 bytes', 'zk_ctx_update_ring', 'no longer verifies',
                   'ZK_MODE_HARDENED', 'context == NULL: ZK_E_ARG', 'ZK_E_BAD_ENCODING'):
        assert needle in sec, needle
    assert 'there is no statement to bind' not in hdr
    unbound = hdr[hdr.index('ring membership of a committed value on its own'):hdr.index('uint64_t zk_member_proof_size(const zk_ctx *ctx);')]
    assert 'Not provided' in unbound and '_bound' in unbound


def test_magic_and_statement_length_of_the_layout_headers(tmp_path):
    src = tmp_path / 'bound.cpp'
    src.write_text('#define ZK_HOST_BUILD 1\n#include "wire.h"\n#include "sha256.h"\n#include <cstdio>\nint main() { printf("%x %x %u %u %u %s\\n", (unsigned)ZK_MAGIC_ZKMB,'
                   ' (unsigned)ZK_MAGIC_ZKM1, gk_stmt_bytes(GK_STMT_MEMBER), gk_hash_len(16, GK_STMT_MEMBER), gk_hash_blocks(3, GK_STMT_MEMBER), GK_MEMBER_TAG); }\n')
    exe = str(tmp_path / 'bound')
    subprocess.check_call(['g++', '-std=c++17', '-I', os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc'), str(src), '-o', exe])
    out = subprocess.check_output([exe]).decode().split()
    assert out == ['%x' % int.from_bytes(b'ZKMB', 'little'), '%x' % int.from_bytes(b'ZKM1', 'little'), '152', str(268 * 16 + 152), '16', 'ZKAttest-GK-member-v1']


def test_arguments_are_refused_before_any_device_is_touched():
    Z, L = _lib()
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    rng = Z.ZkRng(0, C.cast(C.create_string_buffer(32), vp), 0)
    w, st, off = (u32 * 1)(), (C.c_int32 * 1)(), (u64 * 2)()
    com, out, ok = C.create_string_buffer(72), C.create_string_buffer(1200), C.create_string_buffer(1)
    ctx32 = bytes(32)
    # no context handle
    assert L.zk_member_prove_batch_bound(vp(), u64(1), w, ctx32, None, C.byref(rng), com, None, out, u64(1200), st) == ZK_E_ARG
    assert L.zk_member_prove_batch_bound_device(vp(), u64(1), vp(1), vp(1), None, C.byref(rng), vp(1), None, vp(1), u64(1200), vp(1)) == ZK_E_ARG
    assert L.zk_member_verify_batch_bound(vp(), u64(1), bytes(72), ctx32, bytes(1200), None, ok, st) == ZK_E_ARG
    assert L.zk_member_verify_batch_bound_device(vp(), u64(1), vp(1), vp(1), vp(1), None, vp(1), vp(1)) == ZK_E_ARG
    assert L.zk_member_prove_batch_rings_bound(vp(), u64(1), w, ctx32, w, None, C.byref(rng), com, None, out, u64(1200), off, st) == ZK_E_ARG
    assert L.zk_member_prove_batch_rings_bound_device(vp(), u64(1), vp(1), vp(1), vp(1), None, C.byref(rng), vp(1), None, vp(1), u64(1200), vp(1), vp(1)) == ZK_E_ARG
    assert L.zk_member_verify_batch_rings_bound(vp(), u64(1), bytes(72), ctx32, bytes(1200), off, w, None, ok, st) == ZK_E_ARG
    assert L.zk_member_verify_batch_rings_bound_device(vp(), u64(1), vp(1), vp(1), vp(1), vp(1), vp(1), None, vp(1), vp(1)) == ZK_E_ARG
