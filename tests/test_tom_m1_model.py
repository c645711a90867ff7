"""not-gpu: the a = -1 model of the Tom-256 fixed-base comb tables (zkp-ecdsa_amd/csrc/curve.h) in plain integers against the
oracle's Tom-256 arithmetic (oracle/zkattest_ref.py: TEdwardsPoint): the map, the table-entry form, the 7-product addition, the 1-product first step and
the last step that returns to the a = 1 image -- and the pair of points for which the model's law has NO answer, which is why a context whose g or h is
not of odd order keeps the a = 1 tables (api.hip: zk_ctx_set_params)."""
import os
import random
import re

import zkattest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = R.tomEdwards256
t, a, d, q = G.p, G.a, G.d, G.order


def inv(x):
    return pow(x, -1, t)


def sqrt(x):
    r = pow(x, (t + 1) // 4, t)
    assert r * r % t == x % t, 'not a square'
    return r


def is_square(x):
    return pow(x % t, (t - 1) // 2, t) == 1


RA = sqrt(a)                # the a = 1 image: x' = sqrt(a) x, d1 = d / a
D1 = d * inv(a) % t
S2 = sqrt(-D1 % t)          # the model: x'' = s2 x', y' = 1 / y
D2 = -inv(D1) % t


def to_model(P):
    x, y = P.toAffine()
    return S2 * RA * x % t, inv(y)


def entry(P):               # (y' - x'', y' + x'', 2 d2 x'' y')
    x, y = to_model(P)
    return (y - x) % t, (y + x) % t, 2 * D2 * x * y % t


def entry_neg(e):           # -P: swap the first two, negate the third
    return e[1], e[0], -e[2] % t


def first(e):               # identity + entry, scaled by 4: one product
    ym, yp, _ = e
    return 2 * (yp - ym) % t, 2 * (yp + ym) % t, (yp - ym) * (yp + ym) % t, 4


def efgh(p, e):
    X, Y, T, Z = p
    ym, yp, t2 = e
    A, B, C, D = (Y - X) * ym % t, (Y + X) * yp % t, T * t2 % t, 2 * Z % t      # 3 products
    return (B - A) % t, (D - C) % t, (D + C) % t, (B + A) % t


def add(p, e):              # 7 products
    E, F, Gg, H = efgh(p, e)
    return E * F % t, Gg * H % t, E * H % t, F * Gg % t


def add_last(p, e):         # 7 products: the a = 1 image's projective triple (E H / s2 : F G : G H)
    E, F, Gg, H = efgh(p, e)
    return E * H * inv(S2) % t, F * Gg % t, Gg * H % t


def add_points(p, r):       # general addition of two extended points: 8 products and one by 2 d2
    X1, Y1, T1, Z1 = p
    X2, Y2, T2, Z2 = r
    A, B, C, D = (Y1 - X1) * (Y2 - X2) % t, (Y1 + X1) * (Y2 + X2) % t, T1 * T2 * 2 * D2 % t, 2 * Z1 * Z2 % t
    E, F, Gg, H = (B - A) % t, (D - C) % t, (D + C) % t, (B + A) % t
    return E * F % t, Gg * H % t, E * H % t, F * Gg % t


def image_to_original(tr):  # (X : Y : Z) on the a = 1 image -> affine on the reference's curve (k_tom_normalize)
    X, Y, Z = tr
    assert Z % t, 'zero denominator'
    return X * inv(Z) * inv(RA) % t, Y * inv(Z) % t


def model_to_original(p):
    X, Y, T, Z = p
    return image_to_original((T * inv(S2) % t, Z, Y))   # x' = X / (s2 Z) = T / (s2 Y), y = Z / Y


def pts(seed, n):
    rnd = random.Random(seed)
    g = G.generator()
    h = g.mul(G.newScalar(rnd.randrange(1, q)))
    return [(g if i & 1 else h).mul(G.newScalar(rnd.randrange(1, q))) for i in range(n)]


def times(k, P):            # k * P for a plain integer k (a Scalar would reduce it mod q)
    acc = G.identity()
    for b in bin(k)[2:]:
        acc = acc.dbl()
        if b == '1':
            acc = acc.add(P)
    return acc


def test_the_constants_of_the_model_and_the_facts_they_rest_on():
    assert t % 4 == 3 and not is_square(-1)
    assert is_square(a) and not is_square(D1) and is_square(-D1) and is_square(D2)
    assert times(q, G.generator()).isIdentity() and not times(q - 1, G.generator()).isIdentity()
    # the generated header carries these values (Montgomery form, radix 2^30, R = 2^270)
    src = open(os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc', 'consts_gen.h')).read()

    def const(name):
        m = re.search(r'%s\[9\] = \{([^}]*)\}' % name, src)
        limbs = [int(x.strip().rstrip('u'), 16) for x in m.group(1).split(',')]
        return sum(l << (30 * i) for i, l in enumerate(limbs)) * inv(1 << 270) % t
    assert const('TOM_M1_S_M') in (S2, t - S2)
    s2 = const('TOM_M1_S_M')
    assert const('TOM_M1_SINV_M') == inv(s2)
    assert const('TOM_M1_D2_M') == D2 and const('TOM_M1_2D2_M') == 2 * D2 % t and const('TOM_M1_D2H_M') == D2 * inv(2) % t
    assert const('TOM_TWO_M') == 2 and const('TOM_FOUR_M') == 4
    assert s2 == S2, 'this test and tools/gen_consts.py take the same root of -d/a'


def test_the_map_lands_on_the_model_curve_and_fixes_the_identity():
    for P in pts(1, 12) + [G.identity()]:
        x, y = to_model(P)
        assert (-x * x + y * y - 1 - D2 * x * x * y * y) % t == 0
    assert to_model(G.identity()) == (0, 1) and entry(G.identity()) == (1, 1, 0)


def test_seven_product_addition_first_step_and_last_step_against_the_reference():
    ps = pts(2, 24)
    idn = G.identity()
    cases = [(ps[i], ps[i + 1]) for i in range(0, 24, 2)]
    cases += [(ps[0], ps[0]), (ps[1], ps[1].neg()), (ps[2], idn), (idn, ps[3]), (idn, idn)]   # P + P, P + (-P), P + identity, identity + P, identity + identity
    for P, Q in cases:
        want = P.add(Q).toAffine()
        acc = first(entry(P))
        assert model_to_original(acc) == P.toAffine()
        assert model_to_original(add(acc, entry(Q))) == want
        assert image_to_original(add_last(acc, entry(Q))) == want                              # the last-step triple
        assert image_to_original(add_last(acc, entry_neg(entry(Q.neg())))) == want             # a negated entry
        assert model_to_original(add_points(acc, first(entry(Q)))) == want                     # two accumulators
    # a chain as a comb sum runs it: first, adds, last
    acc, ref = first(entry(ps[0])), ps[0]
    for P in ps[1:9]:
        acc, ref = add(acc, entry(P)), ref.add(P)
    assert image_to_original(add_last(acc, entry(ps[9]))) == ref.add(ps[9]).toAffine()


def test_a_base_outside_the_odd_order_subgroup_breaks_the_model_but_not_the_reference():
    """The curve has order 4 q; (1 / sqrt(a), 0) has order 4.  P and P + T4 differ by a point of even order: the model's law meets a zero denominator
    (Z3 = F G = 0) where the reference's law, complete on the whole curve, answers.  Multiples of a base g + T4 form such pairs, hence the set-up check."""
    T4 = R.TEdwardsPoint(G, inv(RA), 0)
    assert G.isOnGroup(T4) and not T4.dbl().isIdentity() and T4.dbl().dbl().isIdentity()
    assert not times(q, T4).isIdentity()                  # what the device check of zk_ctx_set_params sees for such a base
    for P in pts(3, 4):
        Q = P.add(T4)
        assert G.isOnGroup(Q) and not times(q, Q).isIdentity() and times(q, P).isIdentity()
        s = add(first(entry(P)), entry(Q))
        assert s[3] == 0                                             # zero denominator: no affine point behind it
        ref = P.add(Q)
        assert G.isOnGroup(ref) and ref.z % t != 0 and ref.eq(P.dbl().add(T4))
