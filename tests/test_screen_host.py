"""CPU tier of the witness screen (include/zkattest.h: zk_screen_batch).  The comparison that ends its ECDSA check -- x(R) mod n == r on a projective R,
without an inversion (csrc/curve.h: p256_x_is_r_mod_n) -- compiled for the host (tests/host_arith/host_screen.cpp) against Python integers; and the
Python binding's surface against the header."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2 ** 256 - 2 ** 224 + 2 ** 192 + 2 ** 96 - 1
N = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551


@pytest.fixture(scope='module')
def ha(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    out = tmp_path_factory.mktemp('host_screen') / 'libhost_screen.so'
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-shared', '-fPIC', '-Wall', '-Werror', '-Wno-unknown-pragmas',
                           '-I' + os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host_arith', 'host_screen.cpp'), '-o', str(out)])
    return C.CDLL(str(out))


def ask(ha, X, Z, r):
    return ha.ha_x_is_r_mod_n(X.to_bytes(32, 'big'), Z.to_bytes(32, 'big'), r.to_bytes(32, 'big'))


def test_x_is_r_mod_n_on_random_projective_points(ha):
    rnd = random.Random(20261017)
    for _ in range(300):
        x, Z = rnd.randrange(P), rnd.randrange(1, P)
        X = x * Z % P
        r = x % N
        if r:
            assert ask(ha, X, Z, r) == 1, (x, Z)
        other = rnd.randrange(1, N)
        assert ask(ha, X, Z, other) == (1 if other == r else 0)
        near = (r + rnd.choice([1, N - 1])) % N   # off by one either way
        if near:
            assert ask(ha, X, Z, near) == 0
        assert ask(ha, X, 0, r or 1) == 0         # Z = 0: the identity has no x


def test_x_is_r_mod_n_wrap(ha):
    """x in [n, p): x mod n = x - n; the issue's point x = n + 3 with r = 3, and the edges of the range"""
    rnd = random.Random(3)
    for x, r in ((N + 3, 3), (N + 1, 1), (P - 1, P - 1 - N)):
        for _ in range(20):
            Z = rnd.randrange(1, P)
            assert ask(ha, x * Z % P, Z, r) == 1
            assert ask(ha, x * Z % P, Z, r + 1) == 0
        assert ask(ha, x % P, 0, r) == 0
    # r + n >= p: no second candidate; x = r + n - p (what a careless reduction of r + n mod p would accept) must fail
    r = P - N + 5
    for _ in range(20):
        Z = rnd.randrange(1, P)
        assert ask(ha, r * Z % P, Z, r) == 1
        assert ask(ha, (r + N - P) * Z % P, Z, r) == 0
    assert ask(ha, (P - N) * 7 % P, 7, P - N) == 1 and ask(ha, 0, 7, P - N) == 0   # r + n == p exactly: x = 0 is not r mod n


def test_python_surface_matches_the_header():
    import zkp_ecdsa_amd as Z
    hdr = open(os.path.join(ROOT, 'include', 'zkattest.h')).read()
    vals = {k: int(v, 0) for k, v in re.findall(r'\b(ZK_SCREEN_[A-Z_]+)\s*=\s*(\w+)', hdr)}
    assert vals == {'ZK_SCREEN_KEY_NOT_ON_CURVE': Z.SCREEN_KEY_NOT_ON_CURVE, 'ZK_SCREEN_SIG_RANGE': Z.SCREEN_SIG_RANGE, 'ZK_SCREEN_SIG_INVALID': Z.SCREEN_SIG_INVALID,
                    'ZK_SCREEN_NOT_IN_RING': Z.SCREEN_NOT_IN_RING, 'ZK_SCREEN_RING_NOT_RESIDENT': Z.SCREEN_RING_NOT_RESIDENT}
    assert sorted(vals.values()) == [1, 2, 4, 8, 16]
    none = re.search(r'#define\s+ZK_WHICH_NONE\s+(\w+?)u?\s', hdr)
    assert int(none.group(1), 0) == Z.WHICH_NONE == 0xFFFFFFFF
    assert callable(Z.Engine.screen_batch) and callable(Z.Engine.screen_batch_device)
    for s in ('zk_screen_batch', 'zk_screen_batch_device', 'zk_screen_batch_rings', 'zk_screen_batch_rings_device'):
        assert s in Z.SYMBOLS and re.search(r'\b%s\s*\(' % s, hdr)
