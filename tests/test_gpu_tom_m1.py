"""gpu: the comb tables of g and h on the a = -1 model (curve.h: TomModel; 7 products per table addition) give the oracle's commitments byte for byte through every
kernel that reads them -- one lane, list B with its pairs, four lanes, cooperating waves, the verifier's compacted list -- at an unsigned width below and at
the default, and at the signed width 25; a context whose h is NOT of odd order keeps the a = 1 tables and still gives the oracle's bytes."""
import random

import pytest

pytestmark = pytest.mark.gpu

LB_COMMITS = 34
SHAPES = {1: 'one lane', 2: 'list B', 3: 'four lanes', 4: 'cooperating waves', 5: 'compacted list'}


def scalars(bits):
    import zkattest_ref as R
    q = R.tomEdwards256.order
    nwin = ((257 if bits > 24 else 256) + bits - 1) // bits
    one_window = (0x9d3b71 & ((1 << bits) - 1)) << (bits * (nwin // 2))     # a single non-zero window in the middle
    rnd = random.Random(bits)
    vals = [0, 1, q - 1, one_window % q, 1 << (bits * (nwin - 1)), rnd.randrange(q)]
    return [(v, r) for v in vals for r in vals]


def commit_all_shapes(e, octx, bits):
    pairs = scalars(bits)
    want = {}
    for v, r in pairs:
        want[(v, r)] = octx.tom_commit(v, r)
    vs, rs = [p[0] for p in pairs], [p[1] for p in pairs]
    ran = []
    for shape in SHAPES:
        if shape in (3, 4) and bits > 24:
            continue                      # signed digits keep one lane (k_tom.hip)
        if shape == 2:                    # list B of len(pairs) items: slot = k * items + item, every slot of an item commits to the item's (v, r)
            got = e.test_tom_commit_shape(2, vs * LB_COMMITS, rs * LB_COMMITS)
            for k in range(LB_COMMITS):
                for i, p in enumerate(pairs):
                    assert got[k * len(pairs) + i] == want[p], (bits, 'list B', k, p)
        else:
            got = e.test_tom_commit_shape(shape, vs, rs)
            for p, g in zip(pairs, got):
                assert g == want[p], (bits, SHAPES[shape], p)
        ran.append(shape)
    return ran


@pytest.mark.parametrize('bits', [16, 24, 25])
def test_commitments_through_every_comb_kernel_on_the_new_model(bits):
    import coracle as CO
    import zkp_ecdsa_amd as Z
    e = Z.Engine(0)
    raw = e.synth_params(91)
    e.set_comb_bits(bits)
    assert e.test_counter(10) == (1 << 64) - 1          # no tables yet
    e.set_params(*raw, 80)
    assert e.test_counter(10) == 1                       # honest parameters: both bases of odd order, the a = -1 model
    octx = CO.OracleCtx(*raw, 80)
    coop0 = e.test_counter(4)
    ran = commit_all_shapes(e, octx, bits)
    assert ran == ([1, 2, 5] if bits > 24 else [1, 2, 3, 4, 5])
    if bits <= 24:
        assert e.test_counter(4) > coop0                 # the cooperative kernel ran
    e.close()


def test_a_base_of_even_order_keeps_the_a1_tables_and_the_oracles_bytes():
    """h + (1 / sqrt(a), 0) lies on the curve but outside the subgroup of order q: q * h' != identity, so the context must build and use the a = 1 tables
    (whose law is complete on the whole curve) -- the reference has no such check and its bytes are what counts."""
    import coracle as CO
    import zkattest_ref as R
    import zkp_ecdsa_amd as Z
    G = R.tomEdwards256
    t = G.p
    ra = pow(G.a, (t + 1) // 4, t)
    assert ra * ra % t == G.a
    T4 = R.TEdwardsPoint(G, pow(ra, -1, t), 0)
    assert G.isOnGroup(T4) and T4.dbl().dbl().isIdentity() and not T4.dbl().isIdentity()
    e = Z.Engine(0)
    nh, tg, th = e.synth_params(92)
    h = R.TEdwardsPoint(G, int.from_bytes(th[:36], 'big'), int.from_bytes(th[36:], 'big'))
    assert G.isOnGroup(h)
    x, y = h.add(T4).toAffine()
    th2 = x.to_bytes(36, 'big') + y.to_bytes(36, 'big')
    for bits in (16, 25):
        e.set_comb_bits(bits)
        e.set_params(nh, tg, th2, 80)
        assert e.test_counter(10) == 0
        octx = CO.OracleCtx(nh, tg, th2, 80)
        commit_all_shapes(e, octx, bits)
    # the same with g moved instead, and back to honest parameters on the same context
    g = R.TEdwardsPoint(G, int.from_bytes(tg[:36], 'big'), int.from_bytes(tg[36:], 'big'))
    x, y = g.add(T4.dbl()).toAffine()                      # + the point of order 2
    tg2 = x.to_bytes(36, 'big') + y.to_bytes(36, 'big')
    e.set_comb_bits(16)
    e.set_params(nh, tg2, th, 80)
    assert e.test_counter(10) == 0
    commit_all_shapes(e, CO.OracleCtx(nh, tg2, th, 80), 16)
    e.set_params(nh, tg, th, 80)
    assert e.test_counter(10) == 1
    commit_all_shapes(e, CO.OracleCtx(nh, tg, th, 80), 16)
    e.close()
