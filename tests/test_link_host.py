"""not-gpu: the link proofs' arithmetic (zkp-ecdsa_amd/csrc/link.h) compiled for the host CPU (tests/host_arith/host_link.cpp) against the oracle's Point.mul,
add and neg: the 80-bit ladder c * C for caller-supplied bases, the whole relation t_x g + t_r h + c C - A = O with A honest and one unit away, the
responses k - c v mod q; and the same source as a program of its own under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

import zkattest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = R.tomEdwards256
q = G.order
SRC = os.path.join(ROOT, 'tests', 'host_arith', 'host_link.cpp')
FLAGS = ['-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-I' + os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')]

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')

CHALLENGES = [0, 1, 2, 1 << 79, (1 << 80) - 1, int('55' * 10, 16), int('aa' * 10, 16)] + [random.Random(601 + i).getrandbits(80) for i in range(16)]


@pytest.fixture(scope='module')
def hl(tmp_path_factory):
    out = tmp_path_factory.mktemp('host_link') / 'libhost_link.so'
    subprocess.check_call(['g++', '-O1', '-shared', '-fPIC'] + FLAGS + [SRC, '-o', str(out)])
    return C.CDLL(str(out))


def xy(pt):
    x, y = pt.toAffine()
    return x.to_bytes(36, 'big') + y.to_bytes(36, 'big')


def sc(v):
    return G.newScalar(v)


@pytest.fixture(scope='module')
def pts():
    rnd = random.Random(611)
    g = G.generator()
    h = g.mul(sc(rnd.randrange(1, q)))
    com = g.mul(sc(rnd.randrange(q))).add(h.mul(sc(rnd.randrange(q))))
    return g, h, com


def test_ladder_against_point_mul(hl, pts):
    g, h, com = pts
    assert len(set(CHALLENGES)) == 7 + 16 and all(0 <= c < 1 << 80 for c in CHALLENGES)
    bases = [h, com, G.identity(), g]
    cs, bs = [], []
    for c in CHALLENGES:
        for b in bases:
            cs.append(c), bs.append(b)
    n = len(cs)
    out = C.create_string_buffer(72 * n)
    assert hl.hl_ladder(C.c_uint64(n), b''.join(c.to_bytes(10, 'big') for c in cs), b''.join(map(xy, bs)), out) == 0
    for i in range(n):
        assert out.raw[72 * i:72 * i + 72] == xy(bs[i].mul(sc(cs[i]))), (hex(cs[i]), i % len(bases))


def test_whole_relation_honest_and_one_unit_away(hl, pts):
    g, h, com = pts
    rnd = random.Random(613)
    rows = []   # (c, C, t_x, t_r, A, want)
    for c in CHALLENGES:
        # a seeded commitment; the identity (x = r = 0); h itself (x = 0, r = 1); one commitment used for both relations (C1 = C2, r1 = r2)
        x0, r0 = rnd.randrange(q), rnd.randrange(q)
        openings = [(x0, r0), (0, 0), (0, 1), (x0, r0)]
        for x, r in openings:
            Cpt = g.mul(sc(x)).add(h.mul(sc(r)))
            k, s = rnd.randrange(q), rnd.randrange(q)
            A = g.mul(sc(k)).add(h.mul(sc(s)))
            tx, tr = (k - c * x) % q, (s - c * r) % q
            rows.append((c, Cpt, tx, tr, A, 1))
            rows.append((c, Cpt, tx, tr, A.add(g), 0))
            rows.append((c, Cpt, tx, tr, A.add(g.neg()), 0))
            rows.append((c, Cpt, tx, (tr + 1) % q, A, 0))
    n = len(rows)
    ok = C.create_string_buffer(n)
    assert hl.hl_relation(C.c_uint64(n), xy(g), xy(h), b''.join(r[0].to_bytes(10, 'big') for r in rows), b''.join(xy(r[1]) for r in rows),
                          b''.join(r[2].to_bytes(32, 'big') for r in rows), b''.join(r[3].to_bytes(32, 'big') for r in rows), b''.join(xy(r[4]) for r in rows), ok) == 0
    # the oracle's own verdict for every row, from Point.mul / add / neg
    for i, (c, Cpt, tx, tr, A, want) in enumerate(rows):
        if i % 16 < 4:   # (the oracle's sum for a sample of the rows: it is slow)
            assert g.mul(sc(tx)).add(h.mul(sc(tr))).add(Cpt.mul(sc(c))).add(A.neg()).isIdentity() == bool(want), i
        assert ok.raw[i] == want, (i, hex(c))


def test_responses(hl):
    rnd = random.Random(617)
    ks = [0, 1, q - 1, rnd.randrange(q), rnd.randrange(q)]
    vs = [0, 1, q - 1, rnd.randrange(q), q + 5, (1 << 256) - 1]   # values at or above q are reduced as newScalar reduces them
    rows = [(k, c, v) for k in ks for c in CHALLENGES[:7] + CHALLENGES[7:10] for v in vs]
    n = len(rows)
    out = C.create_string_buffer(32 * n)
    assert hl.hl_respond(C.c_uint64(n), b''.join(k.to_bytes(32, 'big') for k, _, _ in rows), b''.join(c.to_bytes(10, 'big') for _, c, _ in rows),
                         b''.join(v.to_bytes(32, 'big') for _, _, v in rows), out) == 0
    for i, (k, c, v) in enumerate(rows):
        assert int.from_bytes(out.raw[32 * i:32 * i + 32], 'big') == sc(k).sub(sc(c).mul(sc(v))).k, i


def test_program_of_its_own_under_the_sanitizers(tmp_path):
    exe = tmp_path / 'host_link'
    subprocess.check_call(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DHOST_LINK_MAIN'] + FLAGS + [SRC, '-o', str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and 'host_link: ok' in r.stdout, r.stdout + r.stderr
