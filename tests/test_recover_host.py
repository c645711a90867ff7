"""CPU tier of the key recovery (include/zkattest.h: zk_recover_batch).  Its arithmetic -- the lift of r to a curve point, the tail A +- Bp with one shared
inversion, the selection rule (csrc/recover.h) -- compiled for the host (tests/host_arith/host_recover.cpp) against Python integers and the model of
tests/recover_common.py; and the Python binding's surface against the header."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import pytest

import recover_common as RC
import zkattest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, N = RC.P, RC.N_ORD
NONE = RC.NONE


@pytest.fixture(scope='module')
def ha(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    out = tmp_path_factory.mktemp('host_recover') / 'libhost_recover.so'
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-shared', '-fPIC', '-Wall', '-Werror', '-Wno-unknown-pragmas',
                           '-I' + os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host_arith', 'host_recover.cpp'), '-o', str(out)])
    lib = C.CDLL(str(out))
    lib.ha_rec_select.restype = C.c_uint32
    return lib


def lift(ha, r, pass_):
    out = C.create_string_buffer(64)
    rc = ha.ha_rec_lift(RC.be(r), pass_, out)
    return rc, (int.from_bytes(out.raw[:32], 'big'), int.from_bytes(out.raw[32:], 'big')) if rc == 2 else None


def check_lift(ha, r, pass_):
    x = r + pass_ * N
    rc, pt = lift(ha, r, pass_)
    if x >= P:
        assert rc == 0, (r, pass_)
        return rc
    exp = RC.lift(x)
    if exp is None:
        assert rc == 1, (r, pass_)
    else:
        assert rc == 2 and pt == exp and pt[1] % 2 == 0 and (pt[1] * pt[1] - (x ** 3 - 3 * x + RC.B_COEF)) % P == 0, (r, pass_)
    return rc


def test_lift(ha):
    rnd = random.Random(20261019)
    seen = set()
    for _ in range(300):
        seen.add(check_lift(ha, rnd.randrange(1, N), 0))
    assert seen == {1, 2}   # about half of all x are on the curve
    smallest_off = next(x for x in range(1, 1000) if RC.lift(x) is None)
    assert check_lift(ha, smallest_off, 0) == 1
    # x with v = x^3 - 3x + b = 0 would be a point of order 2; P-256 has prime order, so there is none (searched below 2^16: nothing to test)
    assert next((x for x in range(1 << 16) if (x ** 3 - 3 * x + RC.B_COEF) % P == 0), None) is None
    # the second x-candidate: x = n + 3 is on the curve (the screen's wrap point); the edges of r + n < p
    assert check_lift(ha, 3, 1) == 2 and RC.lift(N + 3) is not None
    assert check_lift(ha, P - N - 1, 1) in (1, 2)       # r + n = p - 1: the largest x there is
    assert check_lift(ha, P - N, 1) == 0                # r + n = p: no candidate, and not x = 0
    assert check_lift(ha, P - N + 5, 1) == 0
    assert check_lift(ha, N - 1, 1) == 0                # r + n > 2^256: the carry out of eight words
    for _ in range(40):                                 # random r below p - n: pass 1 exists
        r = rnd.randrange(1, P - N)
        assert check_lift(ha, r, 1) in (1, 2)


def proj(pt, rnd):
    """a random projective representative of an affine point or of the identity (None), as 96 bytes"""
    if pt is None:
        return RC.be(0) + RC.be(rnd.randrange(1, P)) + RC.be(0)
    Z = rnd.randrange(1, P)
    return RC.be(pt[0] * Z % P) + RC.be(pt[1] * Z % P) + RC.be(Z)


def aff(pt):
    a = pt.toAffine()
    return a if a else None


def tail(ha, A, Bp, rnd):
    out = C.create_string_buffer(128)
    marks = ha.ha_rec_tail(proj(A, rnd), proj(Bp, rnd), out)
    res = []
    for k in range(2):
        raw = out.raw[64 * k:64 * k + 64]
        res.append(None if marks >> k & 1 else (int.from_bytes(raw[:32], 'big'), int.from_bytes(raw[32:], 'big')))
        if marks >> k & 1:
            assert raw == bytes(64)
    return res


def ref_pair(A, Bp):
    def pt(a):
        return R.p256.identity() if a is None else R.WeierstrassPoint(R.p256, a[0], a[1])
    return [aff(pt(A).add(pt(Bp))), aff(pt(A).add(pt(Bp).neg()))]


def test_tail(ha):
    rnd = random.Random(7)
    G, sc = R.p256.generator(), R.p256.newScalar
    pts = [aff(G.mul(sc(rnd.randrange(1, N)))) for _ in range(12)]
    for i in range(0, 12, 2):
        A, Bp = pts[i], pts[i + 1]
        assert tail(ha, A, Bp, rnd) == ref_pair(A, Bp)
    A = pts[0]
    negA = (A[0], P - A[1])
    # A = Bp: Q1 is the identity and Q0 = 2A must still be exact; A = -Bp: the other way round
    same, opp = ref_pair(A, A), ref_pair(A, negA)
    assert same[0] is not None and same[1] is None and opp[0] is None and opp[1] == same[0]
    assert tail(ha, A, A, rnd) == same
    assert tail(ha, A, negA, rnd) == opp
    # A = identity: Q0 = Bp, Q1 = -Bp; Bp = identity: both are A; both the identity: both marked
    assert tail(ha, None, A, rnd) == [A, negA]
    assert tail(ha, A, None, rnd) == [A, A]
    assert tail(ha, None, None, rnd) == [None, None]


def test_select_rule(ha):
    def sel(*idx):
        return ha.ha_rec_select((C.c_uint32 * 4)(*idx))
    assert sel(NONE, NONE, NONE, NONE) == 4
    assert sel(5, NONE, NONE, NONE) == 0 and sel(NONE, 5, NONE, NONE) == 1 and sel(NONE, NONE, 5, NONE) == 2 and sel(NONE, NONE, NONE, 0) == 3
    assert sel(9, 3, NONE, NONE) == 1 and sel(3, 9, NONE, NONE) == 0          # the lowest index wins, whatever c
    assert sel(7, 7, NONE, NONE) == 0 and sel(NONE, 7, 7, 7) == 1              # ties go to the lowest c
    assert sel(8, 7, 7, 6) == 3 and sel(0, 0, 0, 0) == 0 and sel(NONE, 2, 1, 1) == 2
    assert sel(0xFFFFFFFE, NONE, NONE, NONE) == 0                              # the largest index there can be still beats "none"


def test_python_surface_matches_the_header():
    import zkp_ecdsa_amd as Z
    hdr = open(os.path.join(ROOT, 'include', 'zkattest.h')).read()
    vals = {k: int(v, 0) for k, v in re.findall(r'\b(ZK_RECOVER_[A-Z_]+)\s*=\s*(\w+)', hdr)}
    assert vals == {'ZK_RECOVER_SIG_RANGE': Z.RECOVER_SIG_RANGE, 'ZK_RECOVER_NOT_IN_RING': Z.RECOVER_NOT_IN_RING,
                    'ZK_RECOVER_RING_NOT_RESIDENT': Z.RECOVER_RING_NOT_RESIDENT, 'ZK_RECOVER_NO_POINT': Z.RECOVER_NO_POINT}
    assert sorted(vals.values()) == [2, 8, 16, 32]
    assert (Z.RECOVER_SIG_RANGE, Z.RECOVER_NOT_IN_RING, Z.RECOVER_RING_NOT_RESIDENT) == (Z.SCREEN_SIG_RANGE, Z.SCREEN_NOT_IN_RING, Z.SCREEN_RING_NOT_RESIDENT)
    assert (RC.SIG_RANGE, RC.NOT_IN_RING, RC.RING_NOT_RESIDENT, RC.NO_POINT) == (2, 8, 16, 32)
    assert callable(Z.Engine.recover_batch) and callable(Z.Engine.recover_batch_device)
    for s in ('zk_recover_batch', 'zk_recover_batch_device', 'zk_recover_batch_rings', 'zk_recover_batch_rings_device'):
        assert s in Z.SYMBOLS and re.search(r'\b%s\s*\(' % s, hdr)


def test_model_on_a_reference_signature():
    """A self-check of the MODEL, not of the engine (it passes without the feature): against the reference's own verifier, a signature made with a known key
    is recovered to that key.  The GPU tests take every expected value from this model."""
    rnd = random.Random(11)
    G, sc = R.p256.generator(), R.p256.newScalar
    for _ in range(6):
        d, k = rnd.randrange(1, N), rnd.randrange(1, N)
        msg = rnd.randbytes(32)
        z = R.truncateToN(int.from_bytes(msg, 'big'), N)
        Rx = aff(G.mul(sc(k)))[0]
        r = Rx % N
        s = pow(k, -1, N) * (z + r * d) % N
        sig = RC.be(r) + RC.be(s)
        Q = aff(G.mul(sc(d)))
        assert R.ecdsa_verify(b'\x04' + RC.be(Q[0]) + RC.be(Q[1]), msg, sig)
        ring = [rnd.randrange(P) for _ in range(5)] + [Q[0]]
        assert RC.model(msg, sig, ring) == (RC.be(Q[0]) + RC.be(Q[1]), 5, 0)
        assert RC.model(msg, sig, ring[:5]) == (bytes(64), NONE, RC.NOT_IN_RING)
        assert RC.model(msg, RC.be(0) + RC.be(s), ring) == (bytes(64), NONE, RC.SIG_RANGE)
