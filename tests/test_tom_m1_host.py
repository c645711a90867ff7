"""not-gpu: the source of the a = -1 comb-table model (zkp-ecdsa_amd/csrc/curve.h: TomModel, coop.h: co_tom_m1_*) compiled for the host CPU
(tests/host_arith/host_arith_m1.cpp) against the oracle: table entries as the composer of k_tables.hip writes them, single additions in every form, and
whole comb sums v * g + r * h in the shapes of the one-lane, wide and cooperative kernels of k_tom.hip."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

import zkattest_ref as R
from test_tom_m1_model import D2, S2, RA, inv, t

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = R.tomEdwards256
q = G.order

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')


@pytest.fixture(scope='module')
def ha(tmp_path_factory):
    out = tmp_path_factory.mktemp('host_arith_m1') / 'libhost_arith_m1.so'
    subprocess.check_call(['g++', '-O1', '-std=c++17', '-shared', '-fPIC', '-Wall', '-Werror', '-Wno-unknown-pragmas',
                           '-I' + os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host_arith', 'host_arith_m1.cpp'), '-o', str(out)])
    return C.CDLL(str(out))


def xy(pt):
    x, y = pt.toAffine()
    return x.to_bytes(36, 'big') + y.to_bytes(36, 'big')


def bases(seed, n):
    rnd = random.Random(seed)
    return [G.generator().mul(G.newScalar(rnd.randrange(1, q))) for _ in range(n)]


def test_entries_as_the_table_builder_writes_them(ha):
    ps = bases(41, 6) + [G.identity()]
    out = C.create_string_buffer(108 * len(ps))
    assert ha.ha_m1_entry(C.c_uint64(len(ps)), b''.join(map(xy, ps)), out) == 0
    for i, P in enumerate(ps):
        x, y = P.dbl().dbl().toAffine()
        xm, ym = S2 * RA * x % t, inv(y)
        want = [(ym - xm) % t, (ym + xm) % t, 2 * D2 * xm * ym % t]
        assert [int.from_bytes(out.raw[108 * i + 36 * k:108 * i + 36 * k + 36], 'big') for k in range(3)] == want, i
    assert out.raw[108 * 6:] == (1).to_bytes(36, 'big') * 2 + bytes(36)        # the identity entry (1, 1, 0)


def test_products_of_the_model_on_the_host(ha):
    b = bases(43, 6)
    idn = G.identity()
    P = [b[0], b[1], b[2], b[0], b[3], idn, idn, b[4]]
    Q = [b[1], b[1], b[3], b[0].neg(), idn, b[5], idn, b[4]]
    Rr = [b[2], b[5], b[2].add(b[3]), b[3], b[1], b[5], idn, b[4]]
    n = len(P)
    args = (C.c_uint64(n), b''.join(map(xy, P)), b''.join(map(xy, Q)), b''.join(map(xy, Rr)))
    want = {0: lambda i: P[i].add(Q[i]), 1: lambda i: P[i].add(Q[i]).sub(Rr[i]), 2: lambda i: P[i].add(Q[i]),
            3: lambda i: P[i].add(Q[i]).add(Q[i].add(Rr[i]))}
    for op, f in want.items():
        out = C.create_string_buffer(72 * n)
        assert ha.ha_m1_combo(op, *args, out) == 0
        for i in range(n):
            assert out.raw[72 * i:72 * i + 72] == xy(f(i)), (op, i)


@pytest.mark.parametrize('bits', [8, 16, 24])
def test_whole_comb_sums_in_the_shapes_of_the_kernels(ha, bits):
    rnd = random.Random(47 + bits)
    g = G.generator()
    h = g.mul(G.newScalar(rnd.randrange(1, q)))
    one_window = 0x5a5a5a << (bits * 3)
    sc = [0, 1, q - 1, one_window & ((1 << 256) - 1), rnd.randrange(q), rnd.randrange(1 << 256)]
    vs, rs = [], []
    for v in sc:
        for r in sc[:4] + [rnd.randrange(q)]:
            vs.append(v), rs.append(r)
    n = len(vs)
    vb, rb = b''.join(v.to_bytes(32, 'big') for v in vs), b''.join(r.to_bytes(32, 'big') for r in rs)
    want = [xy(g.mul(G.newScalar(v % q)).add(h.mul(G.newScalar(r % q)))) for v, r in zip(vs, rs)]
    for model, shape in ((1, 0), (1, 1), (1, 2), (0, 0), (0, 1)):
        out = C.create_string_buffer(72 * n)
        assert ha.ha_m1_comb(model, shape, bits, xy(g), xy(h), C.c_uint64(n), vb, rb, out) == 0
        for i in range(n):
            assert out.raw[72 * i:72 * i + 72] == want[i], (model, shape, i, hex(vs[i]), hex(rs[i]))
