"""not-gpu: the escrow tags' arithmetic (zkp-ecdsa_amd/csrc/escrow.h) compiled for the host CPU (tests/host_arith/host_escrow.cpp) against the Python
statement (tests/escrow_common.py): the layout constants, the three responses, the masked 256-bit ladder a * P against Point.mul for bases with and without a
component of small order and for a sum that passes through the identity, the opening rule 4 (E2 - a E1); the Python statement's own self-check (its tags
verify, open to the planted index, and every mutant is refused); and the same source as a program of its own under the address and undefined-behaviour
sanitizers."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

import escrow_common as EC

R = EC.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = EC.TOM
q = G.order
SRC = os.path.join(ROOT, 'tests', 'host_arith', 'host_escrow.cpp')
FLAGS = ['-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-I' + os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')]

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')

SCALARS = [1, 2, q - 1, (1 << 255) + 1, random.Random(701).getrandbits(256)]


@pytest.fixture(scope='module')
def he(tmp_path_factory):
    out = tmp_path_factory.mktemp('host_escrow') / 'libhost_escrow.so'
    subprocess.check_call(['g++', '-O1', '-shared', '-fPIC'] + FLAGS + [SRC, '-o', str(out)])
    return C.CDLL(str(out))


def xy(pt):
    return R._tp(pt)


def mul_plain(P, k):
    """k * P for an integer k taken as it stands (Point.mul reduces its scalar mod q, which is wrong for a point outside the prime-order group)"""
    acc = G.identity()
    for i in reversed(range(k.bit_length())):
        acc = acc.add(acc)
        if (k >> i) & 1:
            acc = acc.add(P)
    return acc


@pytest.fixture(scope='module')
def world():
    rnd = random.Random(711)
    g = G.generator()
    h = g.mul(EC.sc(rnd.randrange(1, q)))
    pp = R.PedersenParams(G, g, h)
    a = rnd.randrange(1, q)
    return pp, a, EC.keygen(pp, a), rnd


def test_layout_constants(he):
    out = (C.c_uint32 * 8)()
    assert he.he_layout(out) == 0
    assert list(out) == [EC.SIZE, 16, int.from_bytes(b'ZKT1', 'little'), EC.PT[0], EC.PT[4], EC.SC[0], EC.SIZE, 8]
    assert EC.PT[4] + 72 == EC.SC[0] and EC.SC[2] + 32 == EC.SIZE and 7 * 67 + 1 + 8 <= 8 * 64


def test_masked_ladder_against_the_python_multiplication(he, world):
    pp, a, A, rnd = world
    P2, P4 = EC.small_order_points()
    ordinary = pp.g.mul(EC.sc(rnd.randrange(1, q))).add(pp.h)
    bases = [ordinary, ordinary.add(P4), ordinary.add(P2), pp.g]
    rows = [(k, b) for k in SCALARS for b in bases]
    rows.append((q, ordinary))        # the sum passes through the identity: q * P = O on a prime-order point, reached at the last bit
    rows.append((q + 1, ordinary))    # ... and goes on from there
    n = len(rows)
    out = C.create_string_buffer(72 * n)
    assert he.he_ladder(C.c_uint64(n), b''.join(k.to_bytes(32, 'big') for k, _ in rows), b''.join(xy(b) for _, b in rows), out) == 0
    for i, (k, b) in enumerate(rows):
        assert out.raw[72 * i:72 * i + 72] == xy(mul_plain(b, k)), (hex(k), i)
    assert out.raw[72 * (n - 2):72 * (n - 1)] == xy(G.identity()) and out.raw[72 * (n - 1):] == xy(ordinary)
    # on the prime-order group the plain multiplication is Point.mul
    assert xy(mul_plain(ordinary, SCALARS[4])) == xy(ordinary.mul(EC.sc(SCALARS[4])))


def test_responses_against_the_python_statement(he):
    rnd = random.Random(717)
    cs = [0, 1, (1 << 80) - 1] + [rnd.getrandbits(80) for _ in range(5)]
    vals = [0, 1, q - 1, q + 5, (1 << 256) - 1, rnd.randrange(q)]   # values at or above q are reduced as newScalar reduces them
    rows = [(c, [rnd.choice(vals) for _ in range(3)], [rnd.choice(vals) for _ in range(3)]) for c in cs for _ in range(6)]
    n = len(rows)
    out = C.create_string_buffer(96 * n)
    assert he.he_respond(C.c_uint64(n), b''.join(c.to_bytes(10, 'big') for c, _, _ in rows), b''.join(EC.be32(k) for _, k, _ in rows),
                         b''.join(EC.be32(v) for _, _, v in rows), out) == 0
    for i, (c, k, v) in enumerate(rows):
        for j in range(3):
            assert int.from_bytes(out.raw[96 * i + 32 * j:96 * i + 32 * j + 32], 'big') == EC.sc(k[j]).sub(EC.sc(c).mul(EC.sc(v[j]))).k, (i, j)


def test_opening_rule_with_components_of_small_order(he, world):
    pp, a, A, rnd = world
    P2, P4 = EC.small_order_points()
    x, rho = rnd.randrange(q), rnd.randrange(q)
    E1, E2 = pp.g.mul(EC.sc(rho)), EC.commit2(pp.g, x, A, rho)
    want = xy(EC.times4(pp.g.mul(EC.sc(x))))
    small = [None, P2, P4, P4.add(P2)]
    rows = [(E1.add(s) if s else E1, E2.add(t) if t else E2) for s in small for t in small]
    n = len(rows)
    out = C.create_string_buffer(72 * n)
    assert he.he_open(C.c_uint64(n), a.to_bytes(32, 'big') * n, b''.join(xy(e1) for e1, _ in rows), b''.join(xy(e2) for _, e2 in rows), out) == 0
    for i in range(n):
        assert out.raw[72 * i:72 * i + 72] == want, i
    # the Python statement computes the same point from the tag's bytes
    t = EC.to_bytes(rows[5][0], rows[5][1], pp.g, pp.g, pp.g, EC.sc(0), EC.sc(0), EC.sc(0))
    assert EC.open_point(a, t) == want
    # without the factor 4 the small-order component would decide: E2 + P2 - a E1 is not x g
    assert xy(E2.add(P2).add(E1.mul(EC.sc(a)).neg())) != xy(pp.g.mul(EC.sc(x)))


def test_python_statement_checks_itself(world):
    pp, a, A, rnd = world
    ring = [rnd.randrange(q) for _ in range(6)]
    ring[4] = ring[1]                      # one key at two indices: the lower one is the answer
    table = EC.ring_points(pp, ring)
    xs, rs, seeds = EC.workload(b'self', 3)
    planted = [1, 5, 0]
    for b in range(3):
        x = ring[planted[b]]
        c72 = xy(EC.commit2(pp.g, x, pp.h, rs[b]))
        t = EC.prove(pp, A, x, c72, rs[b], R.SeedRng(seeds[32 * b:32 * b + 32]))
        assert len(t) == EC.SIZE and EC.verify(pp, A, c72, t) == (1, 0)
        assert EC.open_tag(a, t, table) == (planted[b], 0)
        assert EC.verify(pp, EC.keygen(pp, a + 1), c72, t) == (0, 0)       # another auditor's key
        other_c = xy(EC.commit2(pp.g, x + 1, pp.h, rs[b]))
        rows = EC.mutants(t, c72, xy(pp.h), other_c)
        assert len(rows) >= 14
        for name, c, m in rows[1:]:
            ok, st = EC.verify(pp, A, c, m)
            if name.endswith('+ q'):
                assert (ok, st) == (1, 0), name
            else:
                assert ok == 0, name
                assert st == (10 if name in ('magic', 'total_len', 'reserved', 'off-curve coordinate') else 0), name
    # a response with room for + q below 2^256: a commitment with blinder 0 has t_r = k_r, and the stream hands a small k_r in
    blocks = [EC.tag(b'small', 0), EC.tag(b'small', 1), (0x1234567 + (1 << 200)).to_bytes(32, 'big'), EC.tag(b'small', 3)]
    c0 = xy(pp.g.mul(EC.sc(ring[2])))
    t = EC.prove(pp, A, ring[2], c0, 0, R.StreamRng(blocks))
    plus_q = [m for name, _, m in EC.mutants(t, c0, xy(pp.h), xy(pp.h)) if name == 't_r + q']
    assert len(plus_q) == 1 and plus_q[0] != t and EC.verify(pp, A, c0, plus_q[0]) == (1, 0) and EC.open_tag(a, plus_q[0], table) == (2, 0)
    # a key outside the ring; a damaged header
    c72 = xy(EC.commit2(pp.g, xs[0], pp.h, rs[0]))
    t = EC.prove(pp, A, xs[0], c72, rs[0], R.SeedRng(seeds[:32]))
    assert EC.open_tag(a, t, table) == (EC.NONE, 0) and EC.open_tag(a, b'ZKT2' + t[4:], table) == (EC.NONE, 10)


def test_program_of_its_own_under_the_sanitizers(tmp_path):
    exe = tmp_path / 'host_escrow'
    subprocess.check_call(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DHOST_ESCROW_MAIN'] + FLAGS + [SRC, '-o', str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and 'host_escrow: ok' in r.stdout, r.stdout + r.stderr
