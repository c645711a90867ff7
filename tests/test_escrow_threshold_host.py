"""not-gpu: the threshold opening's Python statement (tests/escrow_threshold_common.py) checks itself -- shares of (t, n) = (1, 1), (2, 3), (3, 5) and
(16, 16) verify and combine, over every t-subset at (2, 3) and three subsets elsewhere, to what the undivided secret opens; every mutant is refused; the
interpolation check refuses one replaced A_j -- and the engine's arithmetic (zkp-ecdsa_amd/csrc/escrow_share.h) compiled for the host CPU
(tests/host_arith/host_escrow_share.cpp), a program of its own under the address and undefined-behaviour sanitizers, agrees with vectors of the statement:
the layout, the response, the Lagrange coefficients, the dealer's polynomial, and the combined point for the sixteen small-order variants of (E1, E2) and a
D_j + P4."""
import itertools
import os
import random
import shutil
import subprocess

import pytest

import escrow_common as EC
import escrow_threshold_common as TC

R = EC.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = EC.TOM
q = G.order
SRC = os.path.join(ROOT, 'tests', 'host_arith', 'host_escrow_share.cpp')
FLAGS = ['-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-I' + os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')]
SHAPES = [(1, 1), (2, 3), (3, 5), (16, 16)]


def xy(pt):
    return R._tp(pt)


def subsets(t, n):
    """every t-subset at (2, 3) -- in both orders --; elsewhere the first t, the last t and a scattered one, not in ascending order"""
    if (t, n) == (2, 3):
        return [list(s) for s in itertools.permutations(range(1, n + 1), t)]
    rnd = random.Random(100 * t + n)
    scattered = rnd.sample(range(1, n + 1), t)
    return [list(range(1, t + 1)), list(range(n - t + 1, n + 1))[::-1], scattered]


@pytest.fixture(scope='module')
def world():
    rnd = random.Random(811)
    g = G.generator()
    h = g.mul(EC.sc(rnd.randrange(1, q)))
    pp = R.PedersenParams(G, g, h)
    a = rnd.randrange(1, q)
    A = EC.keygen(pp, a)
    ring = [rnd.randrange(q) for _ in range(5)]
    x, r = ring[3], rnd.randrange(q)
    c72 = xy(EC.commit2(pp.g, x, pp.h, r))
    tag = EC.prove(pp, A, x, c72, r, R.SeedRng(EC.tag(b'thr-host', 0)))
    other = EC.prove(pp, A, ring[1], xy(EC.commit2(pp.g, ring[1], pp.h, r)), r, R.SeedRng(EC.tag(b'thr-host', 1)))
    assert EC.verify(pp, A, c72, tag) == (1, 0)
    return pp, a, A, ring, tag, other, rnd


@pytest.mark.parametrize('t,n', SHAPES)
def test_python_statement_checks_itself(world, t, n):
    pp, a, A, ring, tag, other, rnd = world
    tables = {7: EC.ring_points(pp, ring)}
    want = (7, 3, 0)
    assert EC.open_tag(a, tag, tables[7]) == (3, 0)
    shares, keys = TC.split(pp, a + q, t, n, R.SeedRng(EC.tag(b'split', 16 * t + n)))   # the secret is reduced
    assert len(shares) == n and TC.keys_consistent(A, t, keys)
    assert t > 1 or shares == [a]
    sh = [TC.share(pp, j, shares[j - 1], keys[j - 1], tag, R.SeedRng(EC.tag(b'share', j)))[0] for j in range(1, n + 1)]
    for j in range(1, n + 1):
        assert len(sh[j - 1]) == TC.SIZE and TC.verify(pp, keys, tag, sh[j - 1]) == (1, 0)
    for S in subsets(t, n):
        assert TC.combine(n, S, tag, [sh[j - 1] for j in S], 7, tables) == want, S
        assert TC.combine(n, S, tag, [sh[j - 1] for j in S], TC.ANY, tables) == want
    S = subsets(t, n)[-1]
    assert TC.combine(n, S, tag, [sh[j - 1] for j in S], 8, tables) == (TC.NONE, TC.NONE, TC.E_ARG)
    assert TC.combine(n, S, b'ZKT2' + tag[4:], [sh[j - 1] for j in S], 7, tables) == (TC.NONE, TC.NONE, TC.E_BAD)
    if n > 1:
        # one replaced A_j: the interpolation check refuses the set, wherever the key sits
        for j in {1, t, n}:
            bad = list(keys)
            bad[j - 1] = keys[j - 1].add(pp.g)
            assert not TC.keys_consistent(A, t, bad), j
        assert not TC.keys_consistent(A.add(pp.g), t, keys)


def test_mutants_of_a_share(world):
    pp, a, A, ring, tag, other, rnd = world
    t, n = 2, 3
    shares, keys = TC.split(pp, a, t, n, R.SeedRng(EC.tag(b'split', 99)))
    sh, st = TC.share(pp, 2, shares[1], keys[1], tag, R.SeedRng(EC.tag(b'mut', 0)))
    assert st == 0
    rows = TC.mutants(sh, tag, xy(pp.h), other, n)
    assert len(rows) >= 14
    for name, tg, m in rows[1:]:
        ok, st = TC.verify(pp, keys, tg, m)
        assert ok == 0 and name != 's + q', name
        assert st == (10 if name in ('magic', 'total_len', 'reserved', 'j := 0', 'j := n + 1', 'off-curve coordinate', 'a damaged tag header') else 0), name
    # s + q: a response with room below 2^256 needs s < 2^224.  With the share secret 1 (key g) and the stream's k = 2^100, s = k - c lies just below 2^100
    small = TC.share(pp, 1, 1, pp.g, tag, R.StreamRng([(1 << 100).to_bytes(32, 'big')]))[0]
    plus_q = [m for name, _, m in TC.mutants(small, tag, xy(pp.h), other, 2) if name == 's + q']
    assert len(plus_q) == 1 and plus_q[0] != small and TC.verify(pp, [pp.g], tag, small) == TC.verify(pp, [pp.g], tag, plus_q[0]) == (1, 0)
    # a D replaced by another valid point: the combine answers status 0 and no member; a D_j + P4 changes nothing
    P2, P4 = EC.small_order_points()
    tables = {1: EC.ring_points(pp, ring)}
    s1 = TC.share(pp, 1, shares[0], keys[0], tag, R.SeedRng(EC.tag(b'mut', 1)))[0]
    wrong = sh[:16] + xy(pp.h) + sh[88:]
    assert TC.combine(n, [2, 1], tag, [wrong, s1], 1, tables) == (TC.NONE, TC.NONE, 0) and TC.verify(pp, keys, tag, wrong) == (0, 0)
    plus = sh[:16] + xy(EC.point(sh[16:88]).add(P4)) + sh[88:]
    assert TC.combine(n, [2, 1], tag, [plus, s1], 1, tables) == (1, 3, 0)
    assert TC.combine(n, [1, 2], tag, [plus, s1], 1, tables) == (TC.NONE, TC.NONE, TC.E_BAD)   # a slot's share names another auditor
    # a refused tag: 264 zero bytes
    assert TC.share(pp, 1, shares[0], keys[0], b'ZKT2' + tag[4:], R.SeedRng(bytes(32))) == (bytes(264), 10)


def _hex(*parts):
    return ' '.join(p.hex() for p in parts)


def vectors(world):
    pp, a, A, ring, tag, other, rnd = world
    lines = ['layout %d 16 %d %d %d %d 6' % (TC.SIZE, int.from_bytes(b'ZKS1', 'little'), TC.PT[0], TC.PT[2], TC.S_OFF)]
    vals = [0, 1, q - 1, q + 5, (1 << 256) - 1, rnd.randrange(q)]   # values at or above q are reduced as newScalar reduces them
    for c in [0, 1, (1 << 80) - 1] + [rnd.getrandbits(80) for _ in range(4)]:
        for _ in range(4):
            k, v = rnd.choice(vals), rnd.choice(vals)
            lines.append('respond ' + _hex(c.to_bytes(10, 'big'), EC.be32([k]), EC.be32([v]), EC.be32([EC.sc(k).sub(EC.sc(c).mul(EC.sc(v))).k])))
    for t, n in SHAPES:
        for S in subsets(t, n):
            for at in {0, n, min(n + 1, 16)} - (set(S) if t > 1 else set()) | {0}:
                lines.append('lagrange ' + _hex(bytes([at]), bytes(S), EC.be32(TC.lagrange(S, at))))
        coef = [rnd.choice(vals) % q for _ in range(t)]
        for j in (1, n):
            lines.append('eval ' + _hex(bytes([j]), EC.be32(coef), EC.be32([sum(c * pow(j, i, q) for i, c in enumerate(coef)) % q])))
    # the combined point: E1 = rho g and E2 = x g + rho A with every pair of small-order components, D_j = a_j E1 (and one D_j + P4): 4 x g throughout
    P2, P4 = EC.small_order_points()
    small = [None, P2, P4, P4.add(P2)]
    x, rho = rnd.randrange(q), rnd.randrange(q)
    E1, E2 = pp.g.mul(EC.sc(rho)), EC.commit2(pp.g, x, A, rho)
    want = xy(EC.times4(pp.g.mul(EC.sc(x))))
    shares, keys = TC.split(pp, a, 3, 5, R.SeedRng(EC.tag(b'split', 35)))
    S = [5, 2, 3]
    for s1 in small:
        for s2 in small:
            e1, e2 = (E1.add(s1) if s1 else E1), (E2.add(s2) if s2 else E2)
            Ds = [TC.mul_plain(e1, shares[j - 1]) for j in S]
            lines.append('combine ' + _hex(bytes(S), xy(e2), b''.join(xy(D) for D in Ds), want))
    Ds = [TC.mul_plain(E1.add(P4), shares[j - 1]) for j in S]
    Ds[1] = Ds[1].add(P4)
    lines.append('combine ' + _hex(bytes(S), xy(E2.add(P2)), b''.join(xy(D) for D in Ds), want))
    for t, n in SHAPES:   # ... and every shape's subsets on plain points
        sh, _ = TC.split(pp, a, t, n, R.SeedRng(EC.tag(b'split', 200 + n)))
        for S in subsets(t, n):
            lines.append('combine ' + _hex(bytes(S), xy(E2), b''.join(xy(E1.mul(EC.sc(sh[j - 1]))) for j in S), want))
    return lines


@pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')
def test_program_of_its_own_under_the_sanitizers(world, tmp_path):
    exe, vec = tmp_path / 'host_escrow_share', tmp_path / 'vectors.txt'
    lines = vectors(world)
    assert sum(l.startswith("combine") for l in lines) == 16 + 1 + 6 + 3 * 3
    vec.write_text('\n'.join(lines) + '\n')
    subprocess.check_call(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + FLAGS + [SRC, '-o', str(exe)])
    r = subprocess.run([str(exe), str(vec)], capture_output=True, text=True)
    assert r.returncode == 0 and 'host_escrow_share: ok (%d vectors)' % len(lines) in r.stdout, r.stdout + r.stderr
    # the program notices a wrong vector: one flipped byte of a combine's expected point
    bad = lines[:-1] + [lines[-1][:-2] + ('00' if lines[-1][-2:] != '00' else '01')]
    vec.write_text('\n'.join(bad) + '\n')
    r = subprocess.run([str(exe), str(vec)], capture_output=True, text=True)
    assert r.returncode == 1 and 'line %d (combine) differs' % len(lines) in r.stdout, r.stdout + r.stderr

