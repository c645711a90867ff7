"""not-gpu: the ABI of the accountable attestations (include/zkattest.h: zk_accountable_*) is declared with the argument lists the Python binding calls it
with, exported by all three builds of the library and bound in Python; the header states the contract; the entry points refuse a NULL context before any
device is touched; and the new kernels, read from the code object's metadata, own no scratch and spill nothing."""
import ctypes as C
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZK_E_ARG = 14
CALLS = {'zk_accountable_prove_batch': 13, 'zk_accountable_prove_batch_device': 13, 'zk_accountable_verify_batch': 9, 'zk_accountable_verify_batch_device': 9,
         'zk_accountable_split_batch': 9, 'zk_accountable_split_batch_device': 9, 'zk_accountable_join_batch': 9, 'zk_accountable_join_batch_device': 9}
METHODS = ['accountable_proof_max_size', 'accountable_prove_batch', 'accountable_prove_batch_device', 'accountable_verify_batch', 'accountable_verify_batch_device',
           'accountable_split', 'accountable_split_device', 'accountable_join', 'accountable_join_device']


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


def test_symbols_declared_exported_listed_and_bound():
    Z, L = _lib()
    hdr = _header()
    declared = set(re.findall(r'\b(zk_[a-z0-9_]+)\s*\(', hdr))
    for s in list(CALLS) + ['zk_accountable_proof_max_size']:
        assert s in declared and s in Z.SYMBOLS and hasattr(L, s), s
    assert {s for s in Z.SYMBOLS if s.startswith('zk_accountable_')} == set(CALLS) | {'zk_accountable_proof_max_size'}
    assert re.search(r'^uint64_t zk_accountable_proof_max_size\(const zk_ctx \*ctx\);', hdr, re.M)
    for m in METHODS:
        assert callable(getattr(Z.Engine, m, None)), m
    # the sets the escrow, threshold and quorum ABI tests pin are what they were: everything the header declares with "accountable" in its name is one of ours
    assert {s for s in declared if 'accountable' in s} == set(CALLS) | {'zk_accountable_proof_max_size'}
    assert {s for s in declared if s.startswith('zk_quorum_')} == {'zk_quorum_pair_count', 'zk_quorum_proof_max_size', 'zk_quorum_prove_batch', 'zk_quorum_prove_batch_device',
                                                                   'zk_quorum_verify_batch', 'zk_quorum_verify_batch_device'}
    assert {s for s in declared if s.startswith('zk_escrow_')} == {s for s in Z.SYMBOLS if s.startswith('zk_escrow_')}
    assert {s for s in declared if s.startswith('zk_auditors_')} == {s for s in Z.SYMBOLS if s.startswith('zk_auditors_')}


@pytest.mark.parametrize('name', ['libzkattest_hip.so', 'libzkattest_hip_uniform.so', 'libzkattest_hip_testhooks.so'])
def test_every_build_exports_the_calls(name):
    Z, _ = _lib()
    path = os.path.join(os.path.dirname(Z.LIB_PATH), name)
    assert os.path.exists(path), 'not built: ' + name
    L = C.CDLL(path)
    for s in CALLS:
        assert hasattr(L, s), (name, s)
    L.zk_accountable_proof_max_size.restype = C.c_uint64
    L.zk_accountable_proof_max_size.argtypes = [C.c_void_p]
    assert L.zk_accountable_proof_max_size(None) == 0


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
    assert names('zk_accountable_prove_batch') == ['ctx', 'B', 'msg_hash', 'sig', 'pk_xy', 'which', 'rng', 'rng_tags', 'out', 'out_cap', 'out_off', 'per_proof_status',
                                                   'per_part_status']
    assert names('zk_accountable_verify_batch') == ['ctx', 'B', 'msg_hash', 'bundles', 'bundle_off', 'verifier_seeds', 'ok', 'per_proof_status', 'first_bad']
    assert names('zk_accountable_split_batch') == ['ctx', 'B', 'bundles', 'bundle_off', 'att_out', 'att_cap', 'att_off', 'tags_out', 'per_proof_status']
    assert names('zk_accountable_join_batch') == ['ctx', 'B', 'proofs', 'proof_off', 'tags', 'out', 'out_cap', 'out_off', 'per_proof_status']
    for n in ('prove', 'verify', 'split', 'join'):
        assert len(names('zk_accountable_%s_batch_device' % n)) == len(names('zk_accountable_%s_batch' % n))


def test_header_states_the_contract():
    hdr = ' '.join(re.sub(r'^ \*', '', l) for l in _header().splitlines())
    hdr = ' '.join(hdr.split())
    for text in ('Wire format "ZKC1" (a bundle)', '"ZKC1" | total_len u32 big-endian | 0 u32 | 0 u32',
                 'one ZKT1 tag, exactly as zk_escrow_prove_batch writes it, for C = the keyXcom inside that attestation',
                 'C is not repeated, so a tag can only be checked against the attestation it travels with',
                 'zk_accountable_proof_max_size(ctx) = 16 + zk_proof_max_size(ctx) + 472',
                 'with key = pk_xy[64 b : 64 b + 32], com = that proof\'s keyXcom and blinder = what zk_prove_key_blinders gives for row b',
                 'in both protocol modes and wire layouts, whatever the comb width or build',
                 'the first non-zero one of the attestation\'s status, then the tag\'s',
                 'A failed bundle gets an empty slot (out_off[b + 1] = out_off[b]), the bundles behind it close up, no neighbour\'s byte changes',
                 'ZK_E_BUFFER, before a byte of any output is written: out_cap < B zk_accountable_proof_max_size, no params, no active ring, no auditor key',
                 'ZK_E_BAD_ENCODING with ok 0 and first_bad 0, no byte outside the slot read',
                 'that does not walk from byte 16 exactly to total_len - 472',
                 'the attestation is verified exactly as zk_verify_batch verifies it',
                 'the tag exactly as zk_escrow_verify_batch does against the attestation\'s keyXcom',
                 'first_bad (may be NULL) is 0 for the attestation, 1 for the tag and 0xFFFFFFFF where ok = 1',
                 'are pure layout: they prove nothing and check no curve',
                 'an empty attestation slot and 472 zero bytes', 'join(split(x)) = x and split(join(p, t)) = (p, t)',
                 'A tag is bound to keyXcom and A, not to the ring', 'split, zk_proof_rering_batch, join',
                 'for B >= 2^32 and while streamed jobs are queued', 'B = 0 is ZK_OK with out_off[0] = 0',
                 'in this context\'s HBM, 4-byte aligned, else ZK_E_ARG', 'is zeroed by zk_ctx_wipe, zk_ctx_destroy and a failed call',
                 '"accountable_blinders"', '"accountable_layout"', '"accountable_walk"', '"accountable_verdict"',
                 'Not provided: one ring id per proof, tags inside ZKQ1 bundles, submit / wait, zk_pool_* and JSON forms, opening straight from bundles (split first), a caller-context binding.',
                 'rng_tags must be independent of rng'):
        assert text in hdr, text


def test_a_null_context_is_refused_before_any_device_is_touched():
    Z, L = _lib()
    vp, u64 = C.c_void_p, C.c_uint64
    seed = C.create_string_buffer(32)
    rng = Z.ZkRng(0, C.cast(seed, vp), 0)
    out, off, st, ok = C.create_string_buffer(4096), (u64 * 2)(), (C.c_int32 * 2)(), (C.c_uint8 * 1)()
    w = (C.c_uint32 * 1)()
    assert L.zk_accountable_proof_max_size(vp()) == 0
    assert L.zk_accountable_prove_batch(vp(), u64(1), bytes(32), bytes(64), bytes(64), w, C.byref(rng), C.byref(rng), out, u64(4096), off, st, None) == ZK_E_ARG
    assert L.zk_accountable_prove_batch_device(vp(), u64(1), vp(4), vp(4), vp(4), vp(4), C.byref(rng), C.byref(rng), vp(4), u64(4096), vp(4), vp(4), None) == ZK_E_ARG
    assert L.zk_accountable_verify_batch(vp(), u64(1), bytes(32), bytes(1024), off, None, ok, st, None) == ZK_E_ARG
    assert L.zk_accountable_verify_batch_device(vp(), u64(1), vp(4), vp(4), vp(4), None, vp(4), vp(4), None) == ZK_E_ARG
    assert L.zk_accountable_split_batch(vp(), u64(1), bytes(1024), off, out, u64(4096), off, out, st) == ZK_E_ARG
    assert L.zk_accountable_split_batch_device(vp(), u64(1), vp(4), vp(4), vp(4), u64(4096), vp(4), vp(4), vp(4)) == ZK_E_ARG
    assert L.zk_accountable_join_batch(vp(), u64(1), bytes(1024), off, bytes(472), out, u64(4096), off, st) == ZK_E_ARG
    assert L.zk_accountable_join_batch_device(vp(), u64(1), vp(4), vp(4), vp(4), vp(4), u64(4096), vp(4), vp(4)) == ZK_E_ARG
    assert L.zk_accountable_prove_batch(vp(), u64(0), None, None, None, None, None, None, None, u64(0), None, None, None) == ZK_E_ARG


def test_new_kernels_report_no_scratch_and_no_spills():
    Z, _ = _lib()
    spec = importlib.util.spec_from_file_location('kernel_meta', os.path.join(ROOT, 'tools', 'kernel_meta.py'))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    ks = {n: k for n, k in km.kernels(Z.LIB_PATH).items() if 'k_acc_' in n}
    for want in ('k_acc_keys', 'k_acc_fold_prove', 'k_acc_place', 'k_acc_walk', 'k_acc_verdict'):
        assert any(want in n for n in ks), want
    for n, k in ks.items():
        assert k['scratch'] == 0 and k['agpr'] == 0 and k['vgpr_spill'] == 0 and k['vgpr'] <= 256 and k['waves_per_simd'] >= 2, (n, k)
