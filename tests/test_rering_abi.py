"""Re-ring proofs, CPU tier: the new entry points are declared in include/zkattest.h, exported by the built library and bound by the Python mirror."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ['zk_prove_key_blinders', 'zk_prove_key_blinders_device', 'zk_proof_rering_batch', 'zk_proof_rering_batch_device']


def _header():
    return open(os.path.join(ROOT, 'include', 'zkattest.h')).read()


def test_header_declares_the_entry_points_and_the_status():
    h = _header()
    for s in SYMS:
        assert re.search(r'\bzk_status %s\(zk_ctx \*' % s, h), s
    assert re.search(r'\bZK_E_OPENING = 16\b', h)
    # the enum is extended: no existing value moved
    for name, val in [('ZK_OK', 0), ('ZK_E_BAD_ENCODING', 10), ('ZK_E_RNG_EXHAUSTED', 11), ('ZK_E_BUFFER', 12), ('ZK_E_ARG', 14), ('ZK_E_DEVICE', 15)]:
        assert re.search(r'\b%s = %d\b' % (name, val), h), name
    # the two warnings a caller must read
    assert 'INTERSECTION' in h and 'fresh and independent' in h


def test_library_exports_the_entry_points():
    import zkp_ecdsa_amd as Z
    L = C.CDLL(Z.LIB_PATH)
    for s in SYMS:
        assert hasattr(L, s), s
        assert s in Z.SYMBOLS


def test_strerror_knows_the_new_status():
    import zkp_ecdsa_amd as Z
    L = Z.lib()
    unknown = L.zk_strerror(99)
    assert L.zk_strerror(16) != unknown and L.zk_strerror(16)
    assert Z.STATUS_TEXT[16] == L.zk_strerror(16).decode()


def test_engine_has_the_methods():
    import zkp_ecdsa_amd as Z
    for m in ('prove_key_blinders', 'rering_batch', 'prove_key_blinders_device', 'rering_batch_device'):
        assert callable(getattr(Z.Engine, m))
