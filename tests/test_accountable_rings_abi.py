"""not-gpu: the ABI of the accountable attestations over several rings (zk_rings_accountable_*) is declared -- in include/zkattest_rings_accountable.h, the part
of include/zkattest.h that is a file of its own -- with the argument lists the Python binding calls it with, exported by all three builds of the library and
bound in Python; the header states the contract; the entry points refuse what they can before any device is touched; the new kernels own no scratch."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZK_E_ARG = 14
CALLS = {'zk_rings_accountable_prove_batch': 14, 'zk_rings_accountable_prove_batch_device': 14, 'zk_rings_accountable_verify_batch': 10,
         'zk_rings_accountable_verify_batch_device': 10, 'zk_rings_accountable_open_batch': 9, 'zk_rings_accountable_open_batch_device': 9}
SIZE = 'zk_rings_accountable_proof_max_size'
METHODS = ['ring_accountable_proof_max_size', 'accountable_prove_batch_rings', 'accountable_prove_batch_rings_device', 'accountable_verify_batch_rings',
           'accountable_verify_batch_rings_device', 'accountable_open_batch_rings', 'accountable_open_batch_rings_device']


def _lib():
    import zkp_ecdsa_amd as Z
    if not os.path.exists(Z.LIB_PATH):
        Z.build()
    return Z, Z.lib()


def _header():
    return open(os.path.join(ROOT, 'include', 'zkattest_rings_accountable.h')).read()


def _prototype(hdr, name):
    m = re.search(r'\bzk_status %s\((.*?)\);' % name, hdr, re.S)
    assert m, name
    text = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    return [' '.join(p.split()) for p in text.split(',')]


def test_symbols_declared_exported_listed_and_bound():
    Z, L = _lib()
    hdr = _header()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(zk_[a-z0-9_]+)\s*\(', code))
    assert declared == set(CALLS) | {SIZE}
    assert set(Z._native.RINGS_ACCOUNTABLE_SYMBOLS) == declared
    for s in declared:
        assert hasattr(L, s), s
    assert re.search(r'^uint64_t zk_rings_accountable_proof_max_size\(const zk_ctx \*ctx, uint32_t ring_id\);', hdr, re.M)
    for m in METHODS:
        assert callable(getattr(Z.Engine, m, None)), m
    # zkattest.h brings the file in, behind its ZKC1 section and inside its extern "C" block
    main = open(os.path.join(ROOT, 'include', 'zkattest.h')).read()
    at = main.index('#include "zkattest_rings_accountable.h"')
    assert main.index('zk_accountable_join_batch_device(') < at < main.rindex('#ifdef __cplusplus')


@pytest.mark.skipif(shutil.which('gcc') is None, reason='no gcc')
def test_a_c_program_that_includes_zkattest_h_sees_the_declarations(tmp_path):
    src = tmp_path / 'use.c'
    src.write_text('#include "zkattest.h"\n'
                   'typedef zk_status (*open_fn)(zk_ctx *, uint64_t, const uint8_t *, const uint8_t *, const uint64_t *, const uint32_t *, uint32_t *, uint32_t *, int32_t *);\n'
                   'open_fn f = zk_rings_accountable_open_batch;\n'
                   'uint64_t (*g)(const zk_ctx *, uint32_t) = zk_rings_accountable_proof_max_size;\n')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I' + os.path.join(ROOT, 'include'), '-c', str(src), '-o', str(tmp_path / 'use.o')])


@pytest.mark.parametrize('name', ['libzkattest_hip.so', 'libzkattest_hip_uniform.so', 'libzkattest_hip_testhooks.so'])
def test_every_build_exports_the_calls(name):
    Z, _ = _lib()
    path = os.path.join(os.path.dirname(Z.LIB_PATH), name)
    assert os.path.exists(path), 'not built: ' + name
    L = C.CDLL(path)
    for s in CALLS:
        assert hasattr(L, s), (name, s)
    L.zk_rings_accountable_proof_max_size.restype = C.c_uint64
    L.zk_rings_accountable_proof_max_size.argtypes = [C.c_void_p, C.c_uint32]
    assert L.zk_rings_accountable_proof_max_size(None, 0) == 0


def test_header_and_ctypes_prototypes_agree():
    Z, L = _lib()
    hdr = _header()
    for name, count in CALLS.items():
        params = _prototype(hdr, name)
        argtypes = getattr(L, name).argtypes
        assert argtypes is not None and len(argtypes) == len(params) == count, (name, params)
        for p, a in zip(params, argtypes):
            if '*' in p or '[' in p:
                assert a in (C.c_void_p, C.c_char_p) or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert p.startswith('uint64_t ') and a is C.c_uint64, (name, p, a)
    names = lambda n: [re.sub(r'\[\d+\]$', '', p.split()[-1].lstrip('*')) for p in _prototype(hdr, n)]
    assert names('zk_rings_accountable_prove_batch') == ['ctx', 'B', 'msg_hash', 'sig', 'pk_xy', 'which', 'ring_ids', 'rng', 'rng_tags', 'out', 'out_cap', 'out_off',
                                                         'per_proof_status', 'per_part_status']
    assert names('zk_rings_accountable_verify_batch') == ['ctx', 'B', 'msg_hash', 'bundles', 'bundle_off', 'ring_ids', 'verifier_seeds', 'ok', 'per_proof_status', 'first_bad']
    assert names('zk_rings_accountable_open_batch') == ['ctx', 'B', 'secret_be32', 'bundles', 'bundle_off', 'ring_ids', 'ring_out_u32', 'index_u32', 'per_proof_status']
    for n in ('prove', 'verify', 'open'):
        assert len(names('zk_rings_accountable_%s_batch_device' % n)) == len(names('zk_rings_accountable_%s_batch' % n))
    # the one-ring calls' lists with ring_ids put in: behind `which` (prover), behind the offsets (verifier)
    one = open(os.path.join(ROOT, 'include', 'zkattest.h')).read()
    for n, at in (('prove', 6), ('verify', 5)):
        ring = [re.sub(r'\[\d+\]$', '', p.split()[-1].lstrip('*')) for p in _prototype(one, 'zk_accountable_%s_batch' % n)]
        assert names('zk_rings_accountable_%s_batch' % n) == ring[:at] + ['ring_ids'] + ring[at:]


def test_header_states_the_contract():
    hdr = ' '.join(re.sub(r'^ \*', '', l) for l in _header().splitlines())
    hdr = ' '.join(hdr.split())
    for text in ('zk_rings_accountable_proof_max_size(ctx, ring_id) = 16 + zk_ring_proof_max_size(ctx, ring_id) + 472',
                 'the ZKC1 header, the proof zk_prove_batch_rings makes for row b with ring_ids[b]',
                 'com = that proof\'s keyXcom and blinder = what zk_prove_key_blinders gives for row b',
                 'in hardened mode each proof hashes its own ring\'s digest', 'which[b] indexes the padded size of ring ring_ids[b]',
                 'ZK_E_ARG for an id that is not resident', 'When all ids name one ring, every output equals zk_accountable_prove_batch\'s with that ring active',
                 'out_cap is decided exactly from the ids, before a byte of any output is written', 'a non-resident id contributes 0',
                 'the largest ring NAMED, not the largest resident', 'verified exactly as zk_verify_batch_rings verifies it with ring_ids[b]',
                 'the tag exactly as zk_escrow_verify_batch does against the attestation\'s keyXcom',
                 'ZK_E_ARG for an id that is neither resident nor ZK_ESCROW_RING_ANY, before the bundle\'s bytes are judged',
                 'exactly what zk_accountable_split_batch followed by zk_rings_escrow_open_batch gives on the same inputs',
                 'only the tags are moved, 472 B per bundle', 'ZK_E_OPENING, with nothing written', 'OPENING DOES NOT VERIFY',
                 'the ACTIVE ring is neither read nor changed, and a context with no active ring is not refused',
                 'for B >= 2^32 and while streamed jobs are queued', 'B = 0 is ZK_OK with out_off[0] = 0', 'in this context\'s HBM, 4-byte aligned, else ZK_E_ARG',
                 '"accountable_caps"', 'Not provided: threshold share calls on bundles (split first), tags inside ZKQ1 bundles',
                 'rng_tags must be independent of rng'):
        assert text in hdr, text


def test_refusals_before_any_device_is_touched():
    Z, L = _lib()
    vp, u64 = C.c_void_p, C.c_uint64
    seed = C.create_string_buffer(32)
    rng = Z.ZkRng(0, C.cast(seed, vp), 0)
    out, off, st, ok = C.create_string_buffer(4096), (u64 * 2)(), (C.c_int32 * 2)(), (C.c_uint8 * 1)()
    w = (C.c_uint32 * 1)()
    assert L.zk_rings_accountable_proof_max_size(vp(), 0) == 0
    assert L.zk_rings_accountable_prove_batch(vp(), u64(1), bytes(32), bytes(64), bytes(64), w, w, C.byref(rng), C.byref(rng), out, u64(4096), off, st, None) == ZK_E_ARG
    assert L.zk_rings_accountable_prove_batch_device(vp(), u64(1), vp(4), vp(4), vp(4), vp(4), vp(4), C.byref(rng), C.byref(rng), vp(4), u64(4096), vp(4), vp(4), None) == ZK_E_ARG
    assert L.zk_rings_accountable_verify_batch(vp(), u64(1), bytes(32), bytes(1024), off, w, None, ok, st, None) == ZK_E_ARG
    assert L.zk_rings_accountable_verify_batch_device(vp(), u64(1), vp(4), vp(4), vp(4), vp(4), None, vp(4), vp(4), None) == ZK_E_ARG
    assert L.zk_rings_accountable_open_batch(vp(), u64(1), bytes(32), bytes(1024), off, w, w, w, st) == ZK_E_ARG
    assert L.zk_rings_accountable_open_batch_device(vp(), u64(1), vp(4), vp(4), vp(4), vp(4), vp(4), vp(4), vp(4)) == ZK_E_ARG
    assert L.zk_rings_accountable_prove_batch(vp(), u64(0), None, None, None, None, None, None, None, None, u64(0), None, None, None) == ZK_E_ARG


def test_new_kernels_report_no_scratch_and_no_spills():
    Z, _ = _lib()
    spec = importlib.util.spec_from_file_location('kernel_meta', os.path.join(ROOT, 'tools', 'kernel_meta.py'))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    ks = {n: k for n, k in km.kernels(Z.LIB_PATH).items() if 'k_acc_caps' in n or 'k_acc_fold_open' in n}
    assert any('k_acc_caps' in n for n in ks) and any('k_acc_fold_open' in n for n in ks), list(ks)
    for n, k in ks.items():
        assert k['scratch'] == 0 and k['agpr'] == 0 and k['vgpr_spill'] == 0 and k['vgpr'] <= 64 and k['waves_per_simd'] >= 2, (n, k)
