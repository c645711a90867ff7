"""not-gpu: the distinct-key proofs' arithmetic (zkp-ecdsa_amd/csrc/distinct.h) compiled for the host CPU (tests/host_arith/host_distinct.cpp) against the
oracle's Point.mul, add and neg and its proveMult: the joint ladder t Cy + c C_4 for bases out of a proof (equal, opposite, the identity, a point of order 2),
the whole relation 5 with A_4_2 honest and one unit away, Cx = C1 - C2, 1 / d, the seven responses; and the same source as a program of its own under the
address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

import zkattest_ref as R
from test_link_host import CHALLENGES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = R.tomEdwards256
q = G.order
SRC = os.path.join(ROOT, 'tests', 'host_arith', 'host_distinct.cpp')
FLAGS = ['-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-I' + os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')]

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')

# t as a proof carries it (32 bytes; the parser reduces mod q): the edge values and 8 seeded ones
TS = [0, 1, 2, q - 1, 1 << 255, (1 << 256) - 1] + [random.Random(701 + i).getrandbits(256) for i in range(8)]
CS = CHALLENGES[:7] + CHALLENGES[7:11]


@pytest.fixture(scope='module')
def hd(tmp_path_factory):
    out = tmp_path_factory.mktemp('host_distinct') / 'libhost_distinct.so'
    subprocess.check_call(['g++', '-O1', '-shared', '-fPIC'] + FLAGS + [SRC, '-o', str(out)])
    return C.CDLL(str(out))


def xy(pt):
    x, y = pt.toAffine()
    return x.to_bytes(36, 'big') + y.to_bytes(36, 'big')


def sc(v):
    return G.newScalar(v)


def be32(v):
    return v.to_bytes(32, 'big')


@pytest.fixture(scope='module')
def pts():
    rnd = random.Random(711)
    g = G.generator()
    h = g.mul(sc(rnd.randrange(1, q)))
    com = lambda: g.mul(sc(rnd.randrange(q))).add(h.mul(sc(rnd.randrange(q))))
    return g, h, com(), com()


def _order2():
    """(0, -1): the point of order 2"""
    pt = G.deserializePoint(b'\x04' + (0).to_bytes(33, 'big') + (G.p - 1).to_bytes(33, 'big'))
    assert not pt.isIdentity() and pt.add(pt).isIdentity()
    return pt


def _base_pairs(pts):
    g, h, a, b = pts
    O = G.identity()
    return [(a, b), (a, a), (a, a.neg()), (O, b), (a, O), (_order2(), b)]


def test_ladder2_against_point_mul(hd, pts):
    assert len(TS) == 14 and len(set(CS)) == 11
    rows = []
    pairs = _base_pairs(pts)
    for i, t in enumerate(TS):
        for j, c in enumerate(CS):
            # every base pair with the edge scalars; the seeded ones walk through the pairs
            for k, (cy, c4) in enumerate(pairs):
                if (i < 6 and j < 7) or (i + j) % len(pairs) == k:
                    rows.append((t, c, cy, c4))
    n = len(rows)
    out = C.create_string_buffer(72 * n)
    assert hd.hd_ladder2(C.c_uint64(n), b''.join(be32(r[0]) for r in rows), b''.join(r[1].to_bytes(10, 'big') for r in rows), b''.join(xy(r[2]) for r in rows),
                         b''.join(xy(r[3]) for r in rows), out) == 0
    memo = {}
    def mul(pt, k):
        key = (xy(pt), k)
        if key not in memo:
            memo[key] = pt.mul(sc(k))
        return memo[key]
    for i, (t, c, cy, c4) in enumerate(rows):
        assert out.raw[72 * i:72 * i + 72] == xy(mul(cy, t % q).add(mul(c4, c))), (i, hex(t), hex(c))


def test_relation5_honest_and_one_unit_away(hd, pts):
    g, h, a, b = pts
    rnd = random.Random(713)
    rows = []   # (t_x, c, Cy, C4, A_4_2, want)
    for c in CS:
        # an honest MultProof's values: Cy = commit(y, ry), C4 = x Cy, A_4_2 = k_x Cy, t_x = k_x - c x
        x, y, ry, kx = (rnd.randrange(q) for _ in range(4))
        Cy = g.mul(sc(y)).add(h.mul(sc(ry)))
        C4, A = Cy.mul(sc(x)), Cy.mul(sc(kx))
        tx = (kx - c * x) % q
        rows += [(tx, c, Cy, C4, A, 1), (tx, c, Cy, C4, A.add(g), 0), (tx, c, Cy, C4, A.add(g.neg()), 0), ((tx + 1) % q, c, Cy, C4, A, 0)]
    n = len(rows)
    ok = C.create_string_buffer(n)
    assert hd.hd_relation5(C.c_uint64(n), b''.join(be32(r[0]) for r in rows), b''.join(r[1].to_bytes(10, 'big') for r in rows), b''.join(xy(r[2]) for r in rows),
                           b''.join(xy(r[3]) for r in rows), b''.join(xy(r[4]) for r in rows), ok) == 0
    for i, (tx, c, Cy, C4, A, want) in enumerate(rows):
        assert Cy.mul(sc(tx)).add(C4.mul(sc(c))).add(A.neg()).isIdentity() == bool(want), i   # the oracle's own verdict
        assert ok.raw[i] == want, (i, hex(c))


def test_cx_is_c1_minus_c2(hd, pts):
    g, h, a, b = pts
    rows = [(a, b), (b, a), (a, a), (a, G.identity()), (G.identity(), a), (a, a.neg())]
    out = C.create_string_buffer(72 * len(rows))
    assert hd.hd_sub(C.c_uint64(len(rows)), b''.join(xy(r[0]) for r in rows), b''.join(xy(r[1]) for r in rows), out) == 0
    for i, (c1, c2) in enumerate(rows):
        assert out.raw[72 * i:72 * i + 72] == xy(c1.sub(c2)), i
    assert out.raw[144:216] == (0).to_bytes(36, 'big') + (1).to_bytes(36, 'big')   # C1 = C2: the identity serialises as (0, 1)


def test_inverse(hd):
    rnd = random.Random(717)
    ds = [1, q - 1, 2] + [rnd.randrange(1, q) for _ in range(5)]
    out = C.create_string_buffer(32 * len(ds))
    assert hd.hd_inverse(C.c_uint64(len(ds)), b''.join(map(be32, ds)), out) == 0
    for i, d in enumerate(ds):
        assert int.from_bytes(out.raw[32 * i:32 * i + 32], 'big') == pow(d, -1, q), i


def test_responses_against_prove_mult(hd, pts, monkeypatch):
    g, h, a, b = pts
    pp = R.PedersenParams(G, g, h)
    rnd = random.Random(719)
    n = 6
    cs, ks, vs, want = [], [], [], []
    for i in range(n):
        x, y, rx, ry, rz = (rnd.randrange(q) for _ in range(5))
        if i == 0:
            y, rz = pow(x, -1, q), 0   # the distinct-key prover's shape: z = 1 under the blinder 0
        z = x * y % q
        com = lambda v, r: R.Commitment(g.mul(sc(v)).add(h.mul(sc(r))), sc(r))
        draws = [rnd.randrange(q) for _ in range(7)]
        seen = []
        monkeypatch.setattr(R, 'hashPoints', lambda pts_, suffix=b'', _h=R.hashPoints: seen.append(_h(pts_, suffix)) or seen[-1])
        pi = R.proveMult(pp, x, y, z, com(x, rx), com(y, ry), com(z, rz), R.StreamRng([be32(d) for d in draws]))
        monkeypatch.undo()
        cs.append(seen[0]), ks.append(draws), vs.append([x, y, z, rx, ry, rz])
        want.append([getattr(pi, f).k for f in R.MultProof.FIELDS_S])
    out = C.create_string_buffer(224 * n)
    assert hd.hd_responses(C.c_uint64(n), b''.join(c.to_bytes(10, 'big') for c in cs), b''.join(be32(k) for row in ks for k in row),
                           b''.join(be32(v) for row in vs for v in row), out) == 0
    for i in range(n):
        got = [int.from_bytes(out.raw[224 * i + 32 * j:224 * i + 32 * j + 32], 'big') for j in range(7)]
        assert got == want[i], i


def test_program_of_its_own_under_the_sanitizers(tmp_path):
    exe = tmp_path / 'host_distinct'
    subprocess.check_call(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DHOST_DISTINCT_MAIN'] + FLAGS + [SRC, '-o', str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and 'host_distinct: ok' in r.stdout, r.stdout + r.stderr
