"""not-gpu: the ABI of the threshold opening (include/zkattest.h: zk_auditors_*, zk_ctx_set_auditors) is declared with the argument lists the Python binding
calls it with, exported by all three builds of the library and bound in Python; the share size is 264; the header states the contract; and the entry points
refuse a NULL context before any device is touched; and the new kernels, read from the code object's metadata, own no scratch and spill nothing."""
import ctypes as C
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZK_E_ARG = 14
CALLS = {'zk_auditors_split_key': 7, 'zk_ctx_set_auditors': 4, 'zk_auditors_share_batch': 9, 'zk_auditors_share_batch_device': 9,
         'zk_auditors_share_verify_batch': 6, 'zk_auditors_share_verify_batch_device': 6, 'zk_auditors_combine_batch': 10, 'zk_auditors_combine_batch_device': 10}
METHODS = ['auditors_split_key', 'set_auditors', 'auditors_share_size', 'auditors_share_batch', 'auditors_share_batch_device', 'auditors_share_verify_batch',
           'auditors_share_verify_batch_device', 'auditors_combine_batch', 'auditors_combine_batch_device']


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
    for s in list(CALLS) + ['zk_auditors_share_size']:
        assert s in declared and s in Z.SYMBOLS and hasattr(L, s), s
    assert {s for s in Z.SYMBOLS if s.startswith('zk_auditors_')} == set(CALLS) - {'zk_ctx_set_auditors'} | {'zk_auditors_share_size'}
    assert re.search(r'^uint64_t zk_auditors_share_size\(void\);', hdr, re.M)
    for m in METHODS:
        assert callable(getattr(Z.Engine, m, None)), m
    # nothing new matches the names the single-auditor ABI tests pin
    assert not [s for s in CALLS if s.startswith('zk_escrow_') or (s.startswith('zk_rings_') and 'escrow' in s)]


@pytest.mark.parametrize('name', ['libzkattest_hip.so', 'libzkattest_hip_uniform.so', 'libzkattest_hip_testhooks.so'])
def test_every_build_exports_the_calls_and_the_size_is_264(name):
    Z, _ = _lib()
    path = os.path.join(os.path.dirname(Z.LIB_PATH), name)
    assert os.path.exists(path), 'not built: ' + name
    L = C.CDLL(path)
    for s in CALLS:
        assert hasattr(L, s), (name, s)
    L.zk_auditors_share_size.restype = C.c_uint64
    assert L.zk_auditors_share_size() == 264


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
            elif p.startswith('uint64_t '):
                assert a is C.c_uint64, (name, p, a)
            else:
                assert p.startswith('uint32_t ') and a is C.c_uint32, (name, p, a)
    names = lambda n: [re.sub(r'\[\d+\]$', '', p.split()[-1].lstrip('*')) for p in _prototype(hdr, n)]
    assert names('zk_auditors_split_key') == ['ctx', 'secret_be32', 't', 'n', 'rng', 'shares_be32', 'share_keys_xy72']
    assert names('zk_ctx_set_auditors') == ['ctx', 't', 'n', 'share_keys_xy72']
    assert names('zk_auditors_share_batch') == ['ctx', 'B', 'j', 'share_secret_be32', 'tags', 'rng', 'out', 'out_cap', 'per_tag_status']
    assert names('zk_auditors_share_verify_batch') == ['ctx', 'B', 'tags', 'shares', 'ok', 'per_share_status']
    assert names('zk_auditors_combine_batch') == ['ctx', 'B', 't', 'auditors_u32', 'tags', 'shares', 'ring_ids', 'ring_out_u32', 'index_u32', 'per_tag_status']
    assert L.zk_auditors_share_size() == 264


def test_header_states_the_contract():
    hdr = ' '.join(re.sub(r'^ \*', '', l) for l in _header().splitlines())
    hdr = ' '.join(hdr.split())
    for text in ('Wire format "ZKS1", 264 bytes', '"ZKS1" | total_len u32 big-endian (= 264) | j u32 big-endian | 0 u32',
                 'c = hashPoints([A_j, E1, D, U1, U2])', 's = k - c a_j', 'lambda_j = prod_{m in S, m != j} m / (m - j)', 'M = 4 (E2 - sum_{j in S} lambda_j D_j)',
                 'fills 0 .. t-2', 'zk_ctx_set_auditors refuses its key', 'The dealer sees a: distributed key generation is not provided',
                 'It needs an auditor key (zk_ctx_set_auditor), else ZK_E_BUFFER', 'A mismatch is ZK_E_OPENING, and nothing is kept',
                 'zk_ctx_set_auditor and zk_ctx_set_params drop the set',
                 'ZK_E_BUFFER without an auditor set; ZK_E_ARG for j outside 1..n; ZK_E_OPENING with nothing written when a_j g is not A_j; ZK_E_BUFFER for out_cap < 264 B',
                 'A failed share is 264 zero bytes and touches no neighbour', 'no branch and no address depends on a bit of a_j or k, in every build',
                 'U1 comes from the (g, h) comb with r = 0', 'nor the mode (h plays no part), nor the uniform build', 'A scalar s >= q is REDUCED, not refused',
                 'there is no verifier randomness', 'ZK_E_ARG when t is not the context\'s threshold, or when auditors holds a 0, a value above n, or a duplicate',
                 'the ACTIVE ring is neither read nor changed, and missing point indexes are built first',
                 'j != auditors[s] included', 'The lambda_j are computed once per call; they are public', 'its branches on the bits of lambda are wave-uniform',
                 'Combining does not verify, as opening does not', 'A share reveals a_j E1 for that tag only',
                 '"share_front"', '"share_ladder"', '"share_respond"', '"share_parse"', '"share_relations"', '"combine_ladder"',
                 'Not provided: distributed key generation, resharing, pool, streamed and JSON forms.'):
        assert text in hdr, text


def test_a_null_context_is_refused_before_any_device_is_touched():
    Z, L = _lib()
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    seed = C.create_string_buffer(32)
    rng = Z.ZkRng(0, C.cast(seed, vp), 0)
    out, st, ok = C.create_string_buffer(264), (C.c_int32 * 1)(), (C.c_uint8 * 1)()
    ids, ring, idx, aud = (u32 * 1)(), (u32 * 1)(), (u32 * 1)(), (u32 * 2)(1, 2)
    assert L.zk_auditors_split_key(vp(), bytes(32), u32(2), u32(3), C.byref(rng), C.create_string_buffer(96), C.create_string_buffer(216)) == ZK_E_ARG
    assert L.zk_ctx_set_auditors(vp(), u32(2), u32(3), bytes(216)) == ZK_E_ARG
    assert L.zk_auditors_share_batch(vp(), u64(1), u32(1), bytes(32), bytes(472), C.byref(rng), out, u64(264), st) == ZK_E_ARG
    assert L.zk_auditors_share_batch_device(vp(), u64(1), u32(1), vp(4), vp(4), C.byref(rng), vp(4), u64(264), vp(4)) == ZK_E_ARG
    assert L.zk_auditors_share_verify_batch(vp(), u64(1), bytes(472), bytes(264), ok, st) == ZK_E_ARG
    assert L.zk_auditors_share_verify_batch_device(vp(), u64(1), vp(4), vp(4), vp(4), vp(4)) == ZK_E_ARG
    assert L.zk_auditors_combine_batch(vp(), u64(1), u32(2), aud, bytes(472), bytes(528), ids, ring, idx, st) == ZK_E_ARG
    assert L.zk_auditors_combine_batch_device(vp(), u64(1), u32(2), vp(4), vp(4), vp(4), vp(4), vp(4), vp(4), vp(4)) == ZK_E_ARG
    assert L.zk_auditors_combine_batch(vp(), u64(0), u32(2), None, None, None, None, None, None, None) == ZK_E_ARG


def test_new_kernels_report_no_scratch_and_no_spills():
    Z, _ = _lib()
    spec = importlib.util.spec_from_file_location('kernel_meta', os.path.join(ROOT, 'tools', 'kernel_meta.py'))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    ks = {n: k for n, k in km.kernels(Z.LIB_PATH).items() if 'k_share_' in n}
    for want in ('k_share_front', 'k_share_ladder', 'k_share_msg', 'k_share_respond', 'k_share_parse', 'k_share_relations', 'k_share_verdict', 'k_share_lagrange',
                 'k_share_combine', 'k_share_interpolate', 'k_share_split'):
        assert any(want in n for n in ks), want
    for n, k in ks.items():
        assert k['scratch'] == 0 and k['agpr'] == 0 and k['vgpr_spill'] == 0 and k['vgpr'] <= 256 and k['waves_per_simd'] >= 2, (n, k)
