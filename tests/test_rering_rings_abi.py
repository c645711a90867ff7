"""Re-ring proofs with one destination ring id per proof, CPU tier: the two entry points are declared in include/zkattest.h with the contract beside the
one-ring call's, exported by both built libraries (the product one and the one with data-independent control flow) and bound by the Python mirror."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ['zk_proof_rering_batch_rings', 'zk_proof_rering_batch_rings_device']


def test_header_declares_the_entry_points_and_the_contract():
    h = open(os.path.join(ROOT, 'include', 'zkattest.h')).read()
    for s in SYMS:
        assert re.search(r'\bzk_status %s\(zk_ctx \*' % s, h), s
    assert 'Not provided: _rings' not in h and 'Not provided: streamed and zk_pool_* forms.' in h
    doc = h[h.index(' * zk_proof_rering_batch_rings:'):h.index(' * Two warnings.')]
    for phrase in ('neither read nor changed', 'KEEPS its slot, filled with zero bytes', 'out_cap < out_off[B]', 'ONE read-back', '"m_gather"', 'which_new[b] >= N of ITS ring'):
        assert phrase in doc, phrase


@pytest.mark.parametrize('name', ['libzkattest_hip.so', 'libzkattest_hip_uniform.so'])
def test_both_libraries_export_the_entry_points(name):
    import zkp_ecdsa_amd as Z
    L = C.CDLL(os.path.join(os.path.dirname(Z.LIB_PATH), name))
    for s in SYMS:
        assert hasattr(L, s), s
        assert s in Z.SYMBOLS


def test_engine_has_the_methods():
    import zkp_ecdsa_amd as Z
    for m in ('rering_batch_rings', 'rering_batch_rings_device'):
        assert callable(getattr(Z.Engine, m))
    for s in SYMS:
        assert getattr(Z.lib(), s).argtypes is not None and len(getattr(Z.lib(), s).argtypes) == 13
