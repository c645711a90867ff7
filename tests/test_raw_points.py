"""The point laws of csrc/curve.h and csrc/coop.h on raw limbs: exceptional points and loose coordinates, on the host and on the device.

tests/test_host_arith.py builds every operand from canonical affine bytes and reads every result through an inversion and fe_canon, which maps 0, q, 2 q and 3 q to the
same bytes; tools/coop_bench.hip runs chains from random points.  Neither can see a law or a predicate that is right mod M but outside the representation the next step
assumes -- the cooperative verifier once compared a Z that was 2 q with {0, q}.  tests/raw_points/raw_points.hip builds P256Pt / TomPt / TomM1Pt / CoP256 / CoTom ...
straight from limbs; tests/raw_points_common.py writes the vectors from Python integers (O + O, O + P, P + O, P + P through the addition law, P + (-P), P + Q, dbl(O),
the P-256 point with x = 0, every Tom-256 point of order 1, 2 and 4 on both models, table entries of the identity and of the order-2 point; every case with coordinates
at v and v + k M, zeros at every multiple of M the class admits, projective operands scaled by 1, M - 1 and a random factor; 32 random pairs per op in canonical and
loose form) and checks every raw result: the model's point by cross-products mod M, X Y == T Z, limbs and values inside the declared class, every identity predicate the
kernels evaluate against the value mod M.  No tolerance anywhere.  The verifier's Straus sums are among the ops: tom_add_tab with ft_neg_sel (curve.h) and
co_tom_add_tab (coop.h) take entries of every small-order point and both signs, where -0 arrives as 4 t."""
import os
import shutil
import subprocess
import time

import pytest

import raw_points_common as C
import zkattest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'raw_points', 'raw_points.hip')


def _gxx(out, *flags, opt='-O1'):
    subprocess.check_call(['g++', '-x', 'c++', opt, '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-DZK_HOST_BUILD', *flags, '-I' + CSRC, SRC, '-o', str(out)])
    return str(out)


@pytest.fixture(scope='module')
def case(tmp_path_factory):
    """the vector file, the host executable and its output: made once"""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    d = tmp_path_factory.mktemp('raw_points')
    n_one, n_co = C.write_vectors(d / 'vectors.bin')
    exe = _gxx(d / 'raw_points_host')
    res = subprocess.run([exe, str(d / 'vectors.bin'), str(d / 'host.out')], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    host = open(d / 'host.out', 'rb').read()
    return dict(dir=d, n=(n_one, n_co), host=host, bad=C.check_output(host, n_one, n_co))


PAIRS = {'O+O', 'O+P', 'P+O', 'P+P', 'P+-P', 'P+Q', 'random'}
ENTRY = {'O+Q', 'Q+Q', '-Q+Q', 'random'}


def test_vector_file_holds_every_op_pair_class_and_representation(case):
    recs, table = C.records()
    n_one, n_co = case['n']
    size = os.path.getsize(case['dir'] / 'vectors.bin')
    per = {k: sum(1 for r in recs if (r.coop, (C.CO_OPS if r.coop else C.ONE_OPS)[r.op]) == k) for k in table}
    print('records: %d one-lane, %d cooperative, %d bytes; per op: %s' % (n_one, n_co, size, sorted(per.items())))
    print('small-order points: a = 1 image %s; a = -1 model %s' % (sorted(C.SMALL['A1']), sorted(C.SMALL['M1'])))
    assert size < 1000000
    # every op of the driver, none left out
    assert {n for c, n in table if not c} == set(C.ONE_OPS) and {n for c, n in table if c} == set(C.CO_OPS)
    assert all(24 <= n <= 400 for n in per.values()), per
    # the file itself, parsed again from its bytes as the driver parses it: record for record the generator's (layout, op, class, flags) and operands, so the
    # table below, which the generator filled record by record, describes what the executables were given
    f_one, f_co, frecs = C.read_vectors(case['dir'] / 'vectors.bin')
    assert (f_one, f_co) == (n_one, n_co) == (sum(1 for r in recs if not r.coop), sum(1 for r in recs if r.coop)) and len(frecs) == len(recs)
    seen, fper = {}, {}
    for (layout, op, cls, flags, elems), r in zip(frecs, recs):
        assert (layout, op, cls, flags, elems) == (r.coop, r.op, r.cls, r.flags, r.elems)
        name = (C.CO_OPS if layout else C.ONE_OPS)[op]
        fper[(layout, name)] = fper.get((layout, name), 0) + 1
        seen.setdefault((layout, name), {}).setdefault(r.pair, set()).add(r.rep)
    assert seen == table and fper == per and all(frecs[i][0] <= frecs[i + 1][0] for i in range(len(frecs) - 1))
    # pair classes per law
    for k in ((0, 'p256_add'), (1, 'co_p256_add')):
        assert PAIRS | {'X0+X0', 'X0+-X0', 'X0+P', 'O+X0'} <= set(table[k])
    for k, small in (((0, 'tom_add'), 'A1'), ((1, 'co_tom_add'), 'A1'), ((0, 'tom_m1_add'), 'M1'), ((0, 'tom_m1_add_last'), 'M1'), ((1, 'co_tom_m1_add'), 'M1')):
        s = C.SMALL[small]
        want = {'%s+%s' % (a, b) for a in s for b in s} | {'%s+%s' % (a, x) for a in s for x in ('P', '-P')} | {'P+P', 'P+-P', 'P+Q', 'P+O', 'random'}
        assert want <= set(table[k]), (k, want - set(table[k]))
    for k in ((0, 'p256_dbl'), (1, 'co_p256_dbl'), (0, 'p256_jdbl'), (1, 'co_p256_jdbl'), (0, 'p256_from_jac'), (1, 'co_p256_from_jac')):
        assert {'dbl(O)', 'dbl(P)', 'dbl(X0)', 'random'} <= set(table[k])
    for k in ((0, 'tom_dbl'), (1, 'co_tom_dbl')):
        assert {'dbl(O)', 'dbl(S2)', 'dbl(S4+)', 'dbl(S4-)', 'dbl(P)', 'random'} <= set(table[k])
    assert ENTRY | {'O+X0', 'X0+X0', '-X0+X0'} <= set(table[(0, 'p256_add_mixed')])
    for n in ('tom_add_niels', 'tom_add_niels_last', 'tom_m1_add_niels', 'tom_m1_add_niels_last'):
        assert ENTRY | {'O+e(O)', 'O+e(S2)', 'Q+e(O)', 'S2+e(S2)'} <= set(table[(0, n)])
        reps = set().union(*table[(0, n)].values())
        assert {'canon/entry', 'canon/entry_neg(0)', 'canon/entry_neg(1)'} <= reps
    for k in ((0, 'tom_add_tab'), (1, 'co_tom_add_tab')):   # the Straus entries of every small-order point and a generic one, under every accumulator, both signs
        s = ['S2', 'S4+', 'S4-']
        assert {'%s+%s' % (a, e) for a in ['O', 'Q', '-Q'] + s for e in ['Q', 'e(O)'] + ['e(%s)' % x for x in s]} | {'random'} <= set(table[k])
        assert all({'canon/neg=0', 'canon/neg=1'} <= reps for pair, reps in table[k].items() if pair != 'random')
        assert {'zero*1/neg=0', 'zero*1/neg=1'} <= set().union(*table[k].values())
    assert set(table[(1, 'co_p256_add+z_is_zero')]) == set(table[(1, 'co_p256_add')])
    assert {'empty+e', 'P+Q', 'Q+Q', '-Q+Q', 'degenerate+Q', 'random'} <= set(table[(0, 'p256_xyzz_sum_step')])
    # representation classes: every exceptional case in canonical, loose and mixed form, a zero coordinate at 0 and M (one lane) / at every multiple (cooperative);
    # every random pair canonical and loose
    for (coop, name), cases in table.items():
        if name == 'co_p256_z_is_zero':
            continue
        for pair, reps in cases.items():
            base = {x.split('/')[0] for x in reps}
            if pair == 'random':
                assert base == {'canon', 'rand-loose'}, (name, pair, reps)
            else:
                assert {'canon', 'loose', 'mixed'} <= base, (name, pair, reps)
    assert {'zero*%d' % k for k in range(1, 8)} <= table[(1, 'co_p256_add')]['O+O'] and {'zero*%d' % k for k in range(1, 10)} <= table[(1, 'co_p256_jdbl')]['dbl(O)']
    assert 'zero*1' in table[(0, 'p256_add')]['O+O'] and 'zero*1' in table[(0, 'tom_add')]['O+O'] and 'zero*1' in table[(1, 'co_tom_add')]['S2+S4+']
    assert sum(1 for r in recs if r.pair == 'random' and r.coop == 0 and r.op == 0) == 64
    # the cooperative Z test: Z at every multiple of q below 8 q, the alpha = 0 shape (Z = 2 q under an identity's X and Y) among them
    z = table[(1, 'co_p256_z_is_zero')]
    assert {'Z=%dq' % k for k in (0, 1, 3, 4, 5, 6, 7)} | {'alpha=0 shape', 'Z=kq+-1', 'random'} <= set(z)
    a0 = [r for r in recs if r.pair == 'alpha=0 shape']
    assert len(a0) == 1 and a0[0].elems[2] == 2 * C.Q and a0[0].elems[0] == 0 and a0[0].want == 1


def test_adding_two_identities_leaves_the_z_that_the_alpha_zero_vector_documents(case):
    """co_p256_add(O, O) on canonical limbs returns Z = 2 q exactly (two products of q each): the representation the hand-built 'alpha=0 shape' vector of the
    predicate stands for.  If the law comes to leave another multiple this fails and the vector moves with it; the chained op co_p256_add+z_is_zero covers the pair
    whatever the multiple is."""
    recs, _ = C.records()
    n_one, n_co = case['n']
    import numpy as np
    out = np.frombuffer(case['host'], np.uint32)[n_one * C.ONE_OUT:].reshape(n_co, C.CO_OUT)
    hit = [i for i, r in enumerate(recs) if r.coop and C.CO_OPS[r.op] == 'co_p256_add' and r.pair == 'O+O' and r.rep == 'canon']
    assert len(hit) == 1
    rows = out[hit[0] - n_one].tolist()
    assert C.val(rows[32:41]) == 2 * C.Q and C.val(rows[0:9]) % C.Q == 0


def test_python_model_agrees_with_the_oracles_scalar_multiplication():
    """the model alone: the oracle's laws with the constants of the two Tom-256 models derived here, and P-256"""
    # the maps are group isomorphisms: k * (image of g) is the image of k * g
    ref = R.tomEdwards256
    for k in (1, 2, 3, 0xdeadbeef, ref.order - 1):
        x, y = C.taff(ref.generator().mul(ref.newScalar(k)))
        assert C.taff(C.A1.generator().mul(C.A1.newScalar(k))) == (C._s * x % C.T, y)
        assert C.taff(C.M1.generator().mul(C.M1.newScalar(k))) == (C.S2 * C._s * x % C.T, pow(y, -1, C.T))
    for name, G in C.GROUPS.items():
        g = G.generator()
        for k1, k2 in ((5, 7), (C._tscal[0], C._tscal[1]), (3, G.order - 3)):
            assert g.mul(G.newScalar(k1)).add(g.mul(G.newScalar(k2))).eq(g.mul(G.newScalar((k1 + k2) % G.order)))
            assert g.mul(G.newScalar(k1)).dbl().eq(g.mul(G.newScalar(2 * k1 % G.order)))
        assert g.mul(G.newScalar(G.order - 1)).add(g).eq(G.identity())
        small = {n: C.tpt(G, xy) for n, xy in C.SMALL[name].items()}
        order = {'O': 1, 'S2': 2, 'S4+': 4, 'S4-': 4}
        for n, S in small.items():
            for k in range(1, 5):      # k * S by repeated addition, by doubling and by the oracle's window walk
                acc = small['O']
                for _ in range(k):
                    acc = acc.add(S)
                assert acc.eq(S.mul(G.newScalar(k))) and (k != 2 or acc.eq(S.dbl()))
                assert acc.eq(small['O']) == (k % order[n] == 0), (name, n, k)
            P = C.tpt(G, C.TPTS[name][64])
            assert S.add(P).add(P.neg()).eq(S) and S.add(P).eq(P.add(S))
    G = R.p256
    g = G.generator()
    for k1, k2 in ((5, 7), (C._scal[0], C._scal[1]), (3, G.order - 3)):
        assert g.mul(G.newScalar(k1)).add(g.mul(G.newScalar(k2))).eq(g.mul(G.newScalar((k1 + k2) % G.order)))
        assert g.mul(G.newScalar(k1)).dbl().eq(g.mul(G.newScalar(2 * k1 % G.order)))
    x0 = C.wpt(C.X0)
    assert G.isOnGroup(x0) and x0.add(C.wpt(C.wneg(C.X0))).isIdentity() and x0.add(x0).eq(x0.dbl()) and x0.mul(G.newScalar(G.order)).isIdentity()


def test_point_laws_return_the_models_point_inside_their_class_on_the_host(case):
    """results by cross-products mod M (X Y == T Z for extended coordinates; the identity as the identity), every limb <= LIMB_MASK and every value below K M for
    the K of the declared return type"""
    bad = [b for b in case['bad'] if 'predicate' not in b and 'verdict' not in b]
    assert not bad, '%d records:\n%s' % (len(bad), '\n'.join(bad[:40]))


def test_identity_predicates_answer_for_the_value_mod_m_in_every_representation_on_the_host(case):
    bad = [b for b in case['bad'] if 'predicate' in b or 'verdict' in b]
    assert not bad, '%d records:\n%s' % (len(bad), '\n'.join(bad[:40]))


def test_host_build_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(case):
    """the stand-alone host program again with -fsanitize=address,undefined on the whole vector file: no report, the same bytes"""
    d = case['dir']
    exe = _gxx(d / 'raw_points_san', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', opt='-O0')
    res = subprocess.run([exe, str(d / 'vectors.bin'), str(d / 'san.out')], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and not res.stderr.strip(), res.stderr[-4000:]
    assert open(d / 'san.out', 'rb').read() == case['host']


@pytest.mark.gpu
def test_point_laws_on_raw_limbs_on_the_device_equal_the_host(case):
    """raw_points.hip compiled with hipcc for gfx950: one thread per one-lane record, one wave per cooperative record -- the identity, P + (-P), small-order points and
    loose coordinates on the real DPP / ds_bpermute instructions, and co_p256_z_is_zero's wave ballot.  The device writes the bytes the host build writes."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    d = case['dir']
    exe = d / 'raw_points_dev'
    t0 = time.time()
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-Wno-unused-value', '-Wno-unused-result', '-I' + CSRC, SRC, '-o', str(exe)], timeout=600)
    t1 = time.time()
    res = subprocess.run([str(exe), str(d / 'vectors.bin'), str(d / 'dev.out')], capture_output=True, text=True, timeout=120)
    print('raw_points device build: hipcc %.1f s, run %.1f s' % (t1 - t0, time.time() - t1))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    dev = open(d / 'dev.out', 'rb').read()
    if dev != case['host']:
        bad = C.check_output(dev, *case['n'])      # names the records that break a promise
        assert not bad, '\n'.join(bad[:40])
    assert dev == case['host']
