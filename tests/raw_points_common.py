"""Vectors and the plain-integer model for tests/raw_points/raw_points.hip (tests/test_raw_points.py).

Everything is derived here from the curve constants of oracle/zkattest_ref.py: the a = 1 image of Tom-256 (x' = sqrt(a) x, d1 = d / a), the a = -1 model of the comb
tables (x'' = s2 x', y' = 1 / y, s2^2 = -d1, d2 = -1 / d1), their generators, their points of order 1, 2 and 4, the P-256 point with x = 0.  The model of a law is the
oracle's own class (WeierstrassPoint / TEdwardsPoint: the reference's step sequences on plain ints) instantiated with those constants.  A record carries its operands
as raw integers (Montgomery residue + k * M: the representation), the model's answer, and two tags: the pair class and the representation class."""
import random

import numpy as np

import zkattest_ref as R

W, NL, MASK, NEAR = 30, 9, (1 << 30) - 1, 3
RR = 1 << (W * NL)
Q, T = R.p256.p, R.tomEdwards256.p
MAGIC, REC_IN, ONE_OUT, CO_OUT = 0x50574152, 76, 40, 64


def limbs(v):
    return tuple((v >> (W * i)) & MASK for i in range(NL - 1)) + (v >> (W * (NL - 1)),)


def val(l):
    return sum(int(x) << (W * i) for i, x in enumerate(l))


def sqrt_3mod4(v, p):
    """the root v^((p + 1) / 4) (what tools/gen_consts.py takes), None where Euler's criterion says v is no square"""
    assert p % 4 == 3
    if v % p and pow(v, (p - 1) // 2, p) != 1:
        return None
    r = pow(v, (p + 1) // 4, p)
    assert r * r % p == v % p
    return r


# ---- the two Tom-256 models of the engine
_ref = R.tomEdwards256
_s = sqrt_3mod4(_ref.a, T)
assert _s is not None, 'a must be a square: the a = 1 image exists'
D1 = _ref.d * pow(_ref.a, -1, T) % T
S2 = sqrt_3mod4(-D1 % T, T)
assert S2 is not None, '-d/a must be a square: the a = -1 model exists'
D2 = -pow(D1, -1, T) % T
A1 = R.TEdwards('tom a=1', T, 1, D1, _ref.order, (_s * _ref.gen[0] % T, _ref.gen[1]))
M1 = R.TEdwards('tom a=-1', T, T - 1, D2, _ref.order, (S2 * _s * _ref.gen[0] % T, pow(_ref.gen[1], -1, T)))


def small_order_points(G):
    """every affine point of order 1, 2 and 4 of a x^2 + y^2 = 1 + d x^2 y^2: the identity, (0, -1), and (+-a^(-1/2), 0) where a is a square (Euler's criterion)"""
    pts = {'O': (0, 1), 'S2': (0, G.p - 1)}
    r = sqrt_3mod4(pow(G.a, -1, G.p), G.p)
    if r is not None:
        pts['S4+'], pts['S4-'] = (r, 0), (G.p - r, 0)
    for x, y in pts.values():
        assert G.isOnGroup(R.TEdwardsPoint(G, x, y, x * y % G.p, 1))
    return pts


SMALL = {'A1': small_order_points(A1), 'M1': small_order_points(M1)}
# the outcome found, asserted so that a case cannot vanish silently: a = 1 is a square, a = -1 is not (t = 3 mod 4)
assert sorted(SMALL['A1']) == ['O', 'S2', 'S4+', 'S4-'] and sorted(SMALL['M1']) == ['O', 'S2']

_b_root = sqrt_3mod4(R.p256.b, Q)
assert _b_root is not None, 'b must be a square: P-256 has a point with x = 0'
X0 = (0, _b_root)


def tpt(G, xy):
    return R.TEdwardsPoint(G, xy[0], xy[1], xy[0] * xy[1] % G.p, 1)


def wpt(xy):
    return R.p256.identity() if xy is None else R.WeierstrassPoint(R.p256, xy[0], xy[1], 1)


def waff(P):
    """affine (x, y) of a P-256 point, None for the identity"""
    if P.z % Q == 0:
        assert P.x % Q == 0 and P.y % Q
        return None
    zi = pow(P.z, -1, Q)
    return (P.x * zi % Q, P.y * zi % Q)


def taff(P):
    zi = pow(P.z, -1, P.group.p)
    return (P.x * zi % P.group.p, P.y * zi % P.group.p)


def wneg(xy):
    return None if xy is None else (xy[0], -xy[1] % Q)


def tneg(xy):
    return (-xy[0] % T, xy[1])


_rnd = random.Random('raw points')
_scal = [_rnd.randrange(1, R.p256.order) for _ in range(66)]
WPTS = [waff(R.p256.generator().mul(R.p256.newScalar(k))) for k in _scal]
_tscal = [_rnd.randrange(1, _ref.order) for _ in range(66)]
TPTS = {'A1': [taff(A1.generator().mul(A1.newScalar(k))) for k in _tscal], 'M1': [taff(M1.generator().mul(M1.newScalar(k))) for k in _tscal]}
GROUPS = {'A1': A1, 'M1': M1}

# ---- operations: name, layout, op number
ONE_OPS = ['p256_add', 'p256_add_mixed', 'p256_dbl', 'p256_jdbl', 'p256_from_jac', 'p256_xyzz_sum_step', 'p256_xyzz_sum_point', 'p256_select', 'p256_is_identity / z_is_zero',
           'tom_neg', 'tom_add', 'tom_dbl', 'tom_from_niels', 'tom_add_niels', 'tom_add_niels_last', 'tom_is_identity', 'tom_m1_add', 'tom_m1_add_last',
           'tom_m1_from_niels', 'tom_m1_add_niels', 'tom_m1_add_niels_last', 'tom_add_tab']
CO_OPS = ['co_p256_add', 'co_p256_dbl', 'co_p256_jdbl', 'co_p256_from_jac', 'co_tom_add', 'co_tom_dbl', 'co_tom_m1_add', 'co_tom_m1_add_tab', 'co_tom_m1_to_a1', 'co_p256_z_is_zero',
          'co_tom_add_tab', 'co_p256_add+z_is_zero']
# the K of every result coordinate, from the declared return type
OUT_K = {'p256': (8, 8, 8), 'jac': (34, 34, 10), 'xyzz': (10, 6, 2, 2), 'tom': (2, 2, 2, 2), 'm1': (12, 8, 2, 2), 'co_p256': (8, 8, 8), 'co_jac': (10, 10, 10, 10), 'co_tom': (2, 2, 2, 2)}


class Rec:
    __slots__ = ('coop', 'op', 'cls', 'flags', 'elems', 'pair', 'rep', 'kind', 'want', 'outk')

    def __init__(self, coop, op, cls, flags, elems, pair, rep, kind, want, outk):
        self.coop, self.op, self.cls, self.flags, self.elems, self.pair, self.rep, self.kind, self.want, self.outk = coop, op, cls, flags, elems, pair, rep, kind, want, outk


def mont(v, M):
    return v * RR % M


def enc(M, reals, ks, mode, zk=0):
    """raw integers of real values: Montgomery residue + k M.  mode: canon k = 0, plus k = 1, loose k = K - 1; a residue 0 takes k = min(zk, K - 1) in mode canon"""
    out = []
    for r, K in zip(reals, ks):
        m = mont(r % M, M)
        if mode == 'canon':
            k = min(zk, K - 1) if m == 0 else 0
        elif mode == 'plus':
            k = min(1, K - 1)
        else:
            k = K - 1
        out.append(m + k * M)
        assert out[-1] < K * M
    return out


# representation classes of an operand pair: (lambda of p, mode of p, lambda of q, mode of q); 'rnd' is one seeded value per record.  Affine operands have no lambda.
REPS = {'canon': (1, 'canon', 1, 'canon'), 'loose': (-1, 'loose', 'rnd', 'plus'), 'mixed': ('rnd', 'plus', -1, 'loose'), 'rand-loose': ('rnd', 'loose', 'rnd', 'loose')}


def lam(spec, M, rnd):
    return 1 if spec == 1 else M - 1 if spec == -1 else rnd.randrange(2, M - 1)


def scale(M, coords, l, weights):
    return [c * pow(l, w, M) % M for c, w in zip(coords, weights)]


class Gen:
    def __init__(self):
        self.recs = []
        self.table = {}      # (coop, op name) -> {pair class: set of representation classes}: what the vector file must hold
        self.rnd = random.Random('raw points representations')

    def add(self, coop, name, cls, flags, elems, pair, rep, kind, want, outk):
        if not coop and kind != 'bool' and rep.startswith('zero*') and not rep.startswith('zero*1'):
            return    # a law's one-lane operand takes a zero as 0 and as M; the cooperative operands and the predicates run over every multiple below K M
        op = (CO_OPS if coop else ONE_OPS).index(name)
        elems = list(elems) + [0] * (8 - len(elems))
        self.recs.append(Rec(coop, op, cls, flags, elems, pair, rep, kind, want, outk))
        self.table.setdefault((coop, name), {}).setdefault(pair, set()).add(rep)

    def reps(self, M, has_zero, kmax, random_case):
        """the representation classes of one case: (name, lambda p, mode p, lambda q, mode q, zero k); kmax: a zero coordinate runs over k M, k < kmax"""
        if random_case:
            names = ['canon', 'rand-loose']
        else:
            names = ['canon', 'loose', 'mixed']
        out = [(n,) + tuple(lam(s, M, self.rnd) if i % 2 == 0 else s for i, s in enumerate(REPS[n])) + (0,) for n in names]
        if has_zero and not random_case:
            out += [('zero*%d' % k, 1, 'canon', 1, 'canon', k) for k in range(1, kmax)]
        return out


# ---------------------------------------------------------------- P-256
def p256_pairs():
    P, Qq = WPTS[64], WPTS[65]
    cases = [('O+O', None, None), ('O+P', None, P), ('P+O', P, None), ('P+P', P, P), ('P+-P', P, wneg(P)), ('P+Q', P, Qq),
             ('X0+X0', X0, X0), ('X0+-X0', X0, wneg(X0)), ('X0+P', X0, P), ('O+X0', None, X0)]
    return cases, [('random', WPTS[2 * i], WPTS[2 * i + 1]) for i in range(32)]


def hom(xy):
    return [0, 1, 0] if xy is None else [xy[0], xy[1], 1]


def gen_p256(g):
    cases, rand = p256_pairs()
    for coop in (0, 1):
        for pair, p, q in cases + rand:
            want = wpt(p).add(wpt(q))
            has_zero = p is None or q is None or p[0] == 0 or q[0] == 0
            for rep, lp, mp, lq, mq, zk in g.reps(Q, has_zero, 8, pair == 'random'):
                e = enc(Q, scale(Q, hom(p), lp, (1, 1, 1)), (8, 8, 8), mp, zk)
                f = enc(Q, scale(Q, hom(q), lq, (1, 1, 1)), (8, 8, 8), mq, zk)
                if coop:
                    g.add(1, 'co_p256_add', 0, 0, e + [0] + f, pair, rep, 'proj3', (want.x, want.y, want.z), OUT_K['co_p256'])
                    # the sum and its Z test chained, as k_v_exp_points_co runs them: O + O is what alpha = 0 leaves there
                    g.add(1, 'co_p256_add+z_is_zero', 0, 0, e + [0] + f, pair, rep, 'bool', int(want.z % Q == 0), ())
                else:
                    g.add(0, 'p256_add', 0, 0, e + f, pair, rep, 'proj3', (want.x, want.y, want.z), OUT_K['p256'])
                    if pair in ('P+Q', 'O+P', 'random'):
                        for c in ((0, 1) if pair != 'random' else (len(g.recs) % 2,)):
                            g.add(0, 'p256_select', 0, c, e + f, pair, rep + '/c=%d' % c, 'same', (f, e)[c], OUT_K['p256'])
    # mixed addition: the accumulator at O, Q, -Q, a generic point; the entry generic and with x = 0
    P, Qq = WPTS[64], WPTS[65]
    mixed = [('O+Q', None, Qq), ('Q+Q', Qq, Qq), ('-Q+Q', wneg(Qq), Qq), ('P+Q', P, Qq), ('O+X0', None, X0), ('X0+X0', X0, X0), ('-X0+X0', wneg(X0), X0), ('P+X0', P, X0)]
    for pair, p, q in mixed + [('random', WPTS[2 * i], WPTS[2 * i + 1]) for i in range(32)]:
        want = wpt(p).add(wpt(q))
        for rep, lp, mp, lq, mq, zk in g.reps(Q, p is None or p[0] == 0 or q[0] == 0, 8, pair == 'random'):
            e = enc(Q, scale(Q, hom(p), lp, (1, 1, 1)), (8, 8, 8), mp, zk)
            f = enc(Q, list(q), (2, 2), 'loose' if mq != 'canon' else 'canon', zk)
            g.add(0, 'p256_add_mixed', 0, 0, e + f, pair, rep, 'proj3', (want.x, want.y, want.z), OUT_K['p256'])
    # doublings; the identity predicates on the same operands and on points that are NOT the identity with some coordinates zero
    dbl = [('dbl(O)', None), ('dbl(P)', P), ('dbl(X0)', X0)] + [('random', WPTS[i]) for i in range(32)]
    for pair, p in dbl:
        want = wpt(p).dbl()
        for rep, lp, mp, _, _, zk in g.reps(Q, p is None or p[0] == 0, 8, pair == 'random'):
            e = enc(Q, scale(Q, hom(p), lp, (1, 1, 1)), (8, 8, 8), mp, zk)
            g.add(0, 'p256_dbl', 0, 0, e, pair, rep, 'proj3', (want.x, want.y, want.z), OUT_K['p256'])
            g.add(1, 'co_p256_dbl', 0, 0, e, pair, rep, 'proj3', (want.x, want.y, want.z), OUT_K['co_p256'])
    preds = [('O', [0, 1, 0]), ('(0:0:0)', [0, 0, 0]), ('(1:1:0)', [1, 1, 0]), ('X0', [0, X0[1], 1]), ('P', hom(P))] + [('random', hom(WPTS[i])) for i in range(32)]
    for pair, c in preds:
        for rep, lp, mp, _, _, zk in g.reps(Q, 0 in c, 8, pair == 'random'):
            e = enc(Q, scale(Q, c, lp, (1, 1, 1)), (8, 8, 8), mp, zk)
            g.add(0, 'p256_is_identity / z_is_zero', 0, 0, e, pair, rep, 'bool', (int(c[0] == 0 and c[2] == 0 and c[1] != 0), int(c[2] == 0)), ())
    # the cooperative Z test: Z (class 8) at every multiple of q below 8 q, under an identity's X and Y and under unrelated ones; Z = 2 q under (0 : Y) is what adding
    # two identities leaves (alpha = 0); Z one off a multiple of q
    for k in range(8):
        for pair, x, y in (('alpha=0 shape' if k == 2 else 'Z=%dq' % k, 0, mont(1, Q) + (k % 2) * Q), ('Z=%dq, X != 0' % k, mont(P[0], Q) + Q, mont(P[1], Q))):
            g.add(1, 'co_p256_z_is_zero', 0, 0, [x, y, k * Q], pair, 'zero*%d' % k, 'bool', 1, ())
        for dlt in (1, -1):
            if 0 <= k * Q + dlt:
                g.add(1, 'co_p256_z_is_zero', 0, 0, [0, mont(1, Q), k * Q + dlt], 'Z=kq+-1', 'k=%d%+d' % (k, dlt), 'bool', 0, ())
    g.add(1, 'co_p256_z_is_zero', 0, 0, [0, mont(1, Q), 8 * Q - 1], 'Z=kq+-1', 'k=8-1', 'bool', 0, ())
    for i in range(32):
        for rep, mode in (('canon', 'canon'), ('rand-loose', 'loose')):
            g.add(1, 'co_p256_z_is_zero', 0, 0, enc(Q, scale(Q, hom(WPTS[i]), g.rnd.randrange(2, Q), (1, 1, 1)), (8, 8, 8), mode), 'random', rep, 'bool', 0, ())
    # Jacobian chains (x = X / Z^2, y = Y / Z^3): points of odd order and the identity (X : Y : 0); cooperative: ZZ = Z^2 in row 3
    for pair, p in [('dbl(O)', None), ('dbl(P)', P), ('dbl(X0)', X0)] + [('random', WPTS[i]) for i in range(32)]:
        want = waff(wpt(p).dbl())
        for rep, lp, mp, _, _, zk in g.reps(Q, p is None or p[0] == 0, 10, pair == 'random'):
            c = scale(Q, hom(p) + ([0] if p is None else [1]), lp, (2, 3, 1, 2))
            g.add(0, 'p256_jdbl', 0, 0, enc(Q, c[:3], (34, 34, 10), mp, zk), pair, rep, 'jac', want, OUT_K['jac'])
            g.add(0, 'p256_from_jac', 0, 0, enc(Q, c[:3], (34, 34, 10), mp, zk), pair, rep, 'proj3', tuple(hom(p)), OUT_K['p256'])
            g.add(1, 'co_p256_jdbl', 0, 0, enc(Q, c, (10, 10, 10, 10), mp, zk), pair, rep, 'jac', want, OUT_K['co_jac'])
            g.add(1, 'co_p256_from_jac', 0, 0, enc(Q, c, (10, 10, 10, 10), mp, zk), pair, rep, 'proj3', tuple(hom(p)), OUT_K['co_p256'])
    # XYZZ sums of table entries (x = X / ZZ, y = Y / ZZZ).  The law is incomplete by design: an entry with the sum's x leaves ZZ = 0, which the predicate must see
    xy = [('empty+e', None, Qq, 3), ('empty, zero digit', None, Qq, 1), ('P, zero digit', P, Qq, 0), ('P+Q', P, Qq, 2), ('Q+Q', Qq, Qq, 2), ('-Q+Q', wneg(Qq), Qq, 2),
          ('X0+X0', X0, X0, 2), ('-X0+X0', wneg(X0), X0, 2), ('P+X0', P, X0, 2), ('degenerate+Q', 'deg', Qq, 2)]
    for pair, p, q, flags in xy + [('random', WPTS[2 * i], WPTS[2 * i + 1], 2) for i in range(32)]:
        for rep, lp, mp, _, mq, zk in g.reps(Q, p is None or p == 'deg' or p[0] == 0 or q[0] == 0, 2, pair == 'random'):
            if p is None:
                st = [0, 0, 0, 0]
            elif p == 'deg':
                st = [P[0], P[1], 0, 0]
            else:
                st = scale(Q, [p[0], p[1], 1, 1], lp, (2, 3, 2, 3))
            e = enc(Q, st, (10, 6, 2, 2), mp if p is not None else 'canon', zk)
            f = enc(Q, list(q), (2, 2), 'loose' if mq != 'canon' else 'canon', zk)
            if flags & 2 == 0:
                want = ('same', e, flags & 1)
            elif flags & 1:
                want = ('point', q, 0)
            elif p == 'deg' or p[0] == q[0]:
                want = ('degenerate', None, 0)
            else:
                want = ('point', waff(wpt(p).add(wpt(q))), 0)
            g.add(0, 'p256_xyzz_sum_step', 0, flags, e + f, pair, rep, 'xyzz', want, OUT_K['xyzz'])
            deg = p == 'deg'
            g.add(0, 'p256_xyzz_sum_point', 0, flags & 1, e, pair, rep, 'xyzz_point', (tuple(hom(None if p is None else (0, 0) if deg else p)), int(deg)), OUT_K['p256'])


# ---------------------------------------------------------------- Tom-256, both models
def ext(xy):
    return [xy[0], xy[1], xy[0] * xy[1] % T, 1]


def tom_pairs(model):
    pts, small = TPTS[model], SMALL[model]
    P, Qq = pts[64], pts[65]
    cases = [('%s+%s' % (a, b), small[a], small[b]) for a in small for b in small]
    for a in small:
        cases += [('%s+P' % a, small[a], P), ('%s+-P' % a, small[a], tneg(P)), ('P+%s' % a, P, small[a])]
    cases += [('P+P', P, P), ('P+-P', P, tneg(P)), ('P+Q', P, Qq)]
    return cases, [('random', pts[2 * i], pts[2 * i + 1]) for i in range(32)]


def a1_triple_of_m1(S):
    """a point of the a = -1 model (projective) as the a = 1 image's projective triple: x' = X / (s2 Z), y = Z / Y"""
    return (S.x * S.y * pow(S2, -1, T) % T, S.z * S.z % T, S.z * S.y % T)


def niels(model, xy):
    x, y = xy
    return [x, y, D1 * x * y % T] if model == 'A1' else [(y - x) % T, (y + x) % T, 2 * D2 * x * y % T]


def gen_tom(g, model):
    G = GROUPS[model]
    m1 = model == 'M1'
    ks = (12, 8, 2, 2) if m1 else (2, 2, 2, 2)
    outk = OUT_K['m1' if m1 else 'tom']
    cases, rand = tom_pairs(model)
    for pair, p, q in cases + rand:
        S = tpt(G, p).add(tpt(G, q))
        has_zero = 0 in p or 0 in q
        for rep, lp, mp, lq, mq, zk in g.reps(T, has_zero, 2, pair == 'random'):
            e1, f1 = scale(T, ext(p), lp, (1, 1, 1, 1)), scale(T, ext(q), lq, (1, 1, 1, 1))
            e, f = enc(T, e1, ks, mp, zk), enc(T, f1, ks, mq, zk)
            g.add(0, 'tom_m1_add' if m1 else 'tom_add', 0, 0, e + f, pair, rep, 'ext4', (S.x, S.y, S.z), outk)
            g.add(1, 'co_tom_m1_add' if m1 else 'co_tom_add', 0, 0, enc(T, e1, (2, 2, 2, 2), mp, zk) + enc(T, f1, (2, 2, 2, 2), mq, zk), pair, rep, 'ext4', (S.x, S.y, S.z), OUT_K['co_tom'])
            if m1:
                g.add(0, 'tom_m1_add_last', 0, 0, e + f, pair, rep, 'ext3', a1_triple_of_m1(S), outk)
    pts, small = TPTS[model], SMALL[model]
    P, Qq = pts[64], pts[65]
    if not m1:
        # the verifier's Straus sums (k_v_straus, k_v_straus_co): an entry is an extended point (X2 : Y2 : d1 T2 : Z2) built from proof-supplied points, negated on load
        # (one lane: 4 t - v, so -0 is 4 t; cooperative: co_sub of the rows).  Accumulator at O, Q, -Q and every small-order point; entries of every small-order
        # point and a generic one; both signs on the canonical form, in turn elsewhere
        accs = [('O', small['O']), ('Q', Qq), ('-Q', tneg(Qq))] + [(a, small[a]) for a in small if a != 'O']
        ents = [('Q', Qq)] + [('e(%s)' % a, small[a]) for a in small]
        turn = 0
        for pair, p, q in [('%s+%s' % (an, en), a, e) for an, a in accs for en, e in ents] + [('random', pts[2 * i], pts[2 * i + 1]) for i in range(32)]:
            for rep, lp, mp, lq, mq, zk in g.reps(T, 0 in p or 0 in q, 2, pair == 'random'):
                e = enc(T, scale(T, ext(p), lp, (1, 1, 1, 1)), (2, 2, 2, 2), mp, zk)
                qe = scale(T, ext(q), lq, (1, 1, 1, 1))
                f = enc(T, [qe[0], qe[1], D1 * qe[2] % T, qe[3]], (2, 2, 2, 2), mq, zk)
                signs = (0, 1)
                if rep != 'canon' or pair == 'random':
                    turn += 1
                    signs = (turn % 2,)
                for neg in signs:
                    S = tpt(G, p).add(tpt(G, tneg(q) if neg else q))
                    r = '%s/neg=%d' % (rep, neg)
                    g.add(0, 'tom_add_tab', 0, neg, e + f, pair, r, 'ext4', (S.x, S.y, S.z), outk)
                    g.add(1, 'co_tom_add_tab', 0, neg, e + f, pair, r, 'ext4', (S.x, S.y, S.z), OUT_K['co_tom'])
    # one operand: doubling and negation (a = 1 image), the identity predicates (a = 1 image: what the kernels test), the way back from the a = -1 model
    unary = [('dbl(%s)' % a, small[a]) for a in small] + [('dbl(P)', P)] + [('random', pts[i]) for i in range(32)]
    for pair, p in unary:
        for rep, lp, mp, _, _, zk in g.reps(T, 0 in p, 2, pair == 'random'):
            e1 = scale(T, ext(p), lp, (1, 1, 1, 1))
            e = enc(T, e1, (2, 2, 2, 2), mp, zk)
            if not m1:
                D, N = tpt(G, p).dbl(), tpt(G, p).neg()
                g.add(0, 'tom_dbl', 0, 0, e, pair, rep, 'ext4', (D.x, D.y, D.z), outk)
                g.add(1, 'co_tom_dbl', 0, 0, e, pair, rep, 'ext4', (D.x, D.y, D.z), OUT_K['co_tom'])
                g.add(0, 'tom_neg', 0, 0, e, pair, rep, 'ext4', (N.x, N.y, N.z), outk)
                for cls in ((0, 1) if pair != 'random' else (len(g.recs) % 2,)):
                    g.add(0, 'tom_is_identity', cls, 0, e, pair, rep + '/site %d' % cls, 'bool', int(p == (0, 1)), ())
            else:
                g.add(1, 'co_tom_m1_to_a1', 0, 0, e, pair, rep, 'rows013', a1_triple_of_m1(tpt(G, p)), OUT_K['co_tom'])
    if not m1:   # quadruples that are no point at all: the predicate answers for the value mod t, coordinate by coordinate
        for pair, c, w0, w1 in (('(0:0:0:0)', [0, 0, 0, 0], 0, 1), ('(0:1:0:2)', [0, 1, 0, 2], 0, 0)):
            for rep, lp, mp, _, _, zk in g.reps(T, True, 2, False):
                for cls, w in ((0, w0), (1, w1)):
                    g.add(0, 'tom_is_identity', cls, 0, enc(T, c, (2, 2, 2, 2), mp, zk), pair, rep + '/site %d' % cls, 'bool', w, ())
    # table entries: the accumulator at O, Q, -Q and the point of order 2 (a generic one: the random pairs); the entry generic, the identity's and the order-2 point's
    accs = [('O', small['O']), ('Q', Qq), ('-Q', tneg(Qq)), ('S2', small['S2'])]
    ents = [('Q', Qq), ('e(O)', small['O']), ('e(S2)', small['S2'])]
    entry_cases = [('%s+%s' % (an, en), a, e) for an, a in accs for en, e in ents] + [('random', pts[2 * i], pts[2 * i + 1]) for i in range(32)]
    names = ('tom_m1_from_niels', 'tom_m1_add_niels', 'tom_m1_add_niels_last') if m1 else ('tom_from_niels', 'tom_add_niels', 'tom_add_niels_last')
    turn = 0
    for pair, p, q in entry_cases:
        for rep, lp, mp, _, mq, zk in g.reps(T, 0 in p or 0 in q, 2, pair == 'random'):
            e = enc(T, scale(T, ext(p), lp, (1, 1, 1, 1)), ks, mp, zk)
            # the three ways an entry is loaded: all of them on the canonical form of an exceptional case, in turn elsewhere
            ways = ((0, 0), (1, 0), (1, 1))
            if rep != 'canon' or pair == 'random':
                turn += 1
                ways = (ways[turn % 3],)
            f = enc(T, niels(model, q), (2, 2, 2), 'loose' if mq != 'canon' else 'canon', zk)
            if m1:   # cooperative: the entry's rows and the constant 2
                S = tpt(G, p).add(tpt(G, q))
                g.add(1, 'co_tom_m1_add_tab', 0, 0, enc(T, scale(T, ext(p), lp, (1, 1, 1, 1)), (2, 2, 2, 2), mp, zk) + f + enc(T, [2], (2,), 'loose' if mq != 'canon' else 'canon'),
                      pair, rep, 'ext4', (S.x, S.y, S.z), OUT_K['co_tom'])
            for cls, neg in ways:
                qq = tneg(q) if neg else q
                S, F = tpt(G, p).add(tpt(G, qq)), tpt(G, qq)
                r = '%s/entry%s' % (rep, ('', '_neg(0)', '_neg(1)')[cls + neg])
                g.add(0, names[1], cls, neg, e + f, pair, r, 'ext4', (S.x, S.y, S.z), outk)
                g.add(0, names[2], cls, neg, e + f, pair, r, 'ext3', a1_triple_of_m1(S) if m1 else (S.x, S.y, S.z), outk)
                if pair.startswith('O+') or pair == 'random':
                    g.add(0, names[0], cls, neg, [0, 0, 0, 0] + f, pair, r, 'ext4', (F.x, F.y, F.z), outk)


_cache = []


def records():
    """(records, table): made once"""
    if not _cache:
        g = Gen()
        gen_p256(g)
        gen_tom(g, 'A1')
        gen_tom(g, 'M1')
        g.recs.sort(key=lambda r: r.coop)      # stable: one-lane records first
        _cache.append((g.recs, g.table))
    return _cache[0]


def write_vectors(path):
    """a record: layout | n << 8, op, class, flags, then its first n elements (the elements behind the last one that is not zero are left out: the driver reads zero)"""
    recs, _ = records()
    words = []
    for r in recs:
        n = max([k + 1 for k, v in enumerate(r.elems) if v] or [0])
        words += [r.coop | (n << 8), r.op, r.cls, r.flags]
        for v in r.elems[:n]:
            words += limbs(v)
    n_one = sum(1 for r in recs if not r.coop)
    with open(path, 'wb') as f:
        f.write(np.array([MAGIC, n_one, len(recs) - n_one, 0] + words, np.uint32).tobytes())
    return n_one, len(recs) - n_one


def read_vectors(path):
    """the records of a vector file as the driver reads them: (layout, op, class, flags, the eight elements as integers)"""
    w = np.fromfile(path, np.uint32).tolist()
    assert w[0] == MAGIC and w[3] == 0
    out, pos = [], 4
    for _ in range(w[1] + w[2]):
        n = w[pos] >> 8
        assert n <= 8
        elems = [val(w[pos + 4 + 9 * k:pos + 13 + 9 * k]) for k in range(n)] + [0] * (8 - n)
        out.append((w[pos] & 255, w[pos + 1], w[pos + 2], w[pos + 3], elems))
        pos += 4 + 9 * n
    assert pos == len(w)
    return w[1], w[2], out


# ---------------------------------------------------------------- checking an output file
def _parallel(M, u, w):
    """u and w name the same projective point: every 2 x 2 minor vanishes mod M and u is not the zero vector"""
    n = len(u)
    return any(x % M for x in u) and any(x % M for x in w) and all((u[i] * w[j] - u[j] * w[i]) % M == 0 for i in range(n) for j in range(i + 1, n))


def check_record(r, o):
    """one record's output words against the model; returns None or what is wrong"""
    M = Q if (r.coop and r.op in (0, 1, 2, 3, 9, 11)) or (not r.coop and r.op < 9) else T
    rinv = pow(RR, -1, M)
    if r.kind == 'bool':
        want = r.want if isinstance(r.want, tuple) else (r.want,)
        got = (o[0],) if r.coop else tuple(o[36:36 + len(want)])
        if r.coop and any(x != got[0] for x in o):
            return 'the verdict differs between lanes'
        if not r.coop and (any(o[:36]) or any(o[36 + len(want):])):
            return 'stray output words'
        return None if got == want else 'predicate says %s, the value mod M says %s' % (got, want)
    n = len(r.outk)
    if r.coop:
        rows = [o[16 * i:16 * i + 16] for i in range(4)]
        if any(any(row[9:]) for row in rows):
            return 'lanes 9..15 are not zero'
        ls, cap = [row[:9] for row in rows], MASK + NEAR
        if r.kind == 'proj3':
            n = 3
        used = [0, 1, 3] if r.kind == 'rows013' else list(range(n))
    else:
        ls, cap, used = [o[9 * i:9 * i + 9] for i in range(4)], MASK, list(range(n))
        if any(any(ls[i]) for i in range(n, 4)):
            return 'stray output words'
    vs = [val(l) for l in ls]
    for i in used:
        k = r.outk[i if not r.kind == 'rows013' else 0]
        if max(ls[i][:8]) > cap or vs[i] >= k * M:
            return 'coordinate %d leaves its class: limbs %s, value / M = %.3f, K = %d' % (i, [hex(x) for x in ls[i]], vs[i] / M, k)
    if r.kind == 'same':
        return None if vs[:3] == list(r.want) and not any(o[36:]) else 'not the selected operand'
    c = [v * rinv % M for v in vs]        # out of the Montgomery domain
    if r.kind == 'proj3':
        return None if _parallel(M, c[:3], r.want) else 'not the model\'s point'
    if r.kind == 'ext4':
        if (c[0] * c[1] - c[2] * c[3]) % M:
            return 'X Y != T Z'
        return None if c[3] and _parallel(M, (c[0], c[1], c[3]), r.want) else 'not the model\'s point'
    if r.kind == 'ext3':
        if vs[2] != 0:
            return 'T of a final sum is not zero'
        return None if c[3] and _parallel(M, (c[0], c[1], c[3]), r.want) else 'not the model\'s point'
    if r.kind == 'rows013':
        return None if _parallel(M, (c[0], c[1], c[3]), r.want) else 'not the model\'s point'
    if r.kind == 'jac':
        X, Y, Z = c[:3]
        if r.coop and (c[3] - Z * Z) % M:
            return 'ZZ != Z^2'
        if r.want is None:
            return None if X == 0 and Z == 0 and Y else 'not the identity (0 : Y : 0)'
        return None if Z and (X - r.want[0] * Z * Z) % M == 0 and (Y - r.want[1] * Z ** 3) % M == 0 else 'not the model\'s point'
    if r.kind == 'xyzz':
        what, p, empty = r.want
        X, Y, ZZ, ZZZ = c
        if o[36] != empty or any(o[38:]):
            return 'wrong empty flag'
        if what == 'same':
            return None if vs == r.elems[:4] and o[37] == int(not empty and ZZ == 0) else 'a zero digit changed the sum'
        if what == 'degenerate':
            return None if ZZ == 0 and o[37] == 1 else 'an exceptional pair left ZZ = %x, degenerate = %d' % (ZZ, o[37])
        if o[37] != 0 or ZZ == 0:
            return 'a generic sum is called degenerate'
        return None if (X - p[0] * ZZ) % M == 0 and (Y - p[1] * ZZZ) % M == 0 and (ZZ ** 3 - ZZZ ** 2) % M == 0 else 'not the model\'s point'
    if r.kind == 'xyzz_point':
        want, deg = r.want
        if o[36] != deg or any(o[37:]):
            return 'degenerate flag'
        if deg:
            return None if c[2] == 0 else 'Z of a degenerate sum'
        return None if _parallel(M, c[:3], want) else 'not the model\'s point'
    return 'unknown kind'


def check_output(raw, n_one, n_co):
    recs, _ = records()
    words = np.frombuffer(raw, np.uint32)
    assert len(words) == n_one * ONE_OUT + n_co * CO_OUT
    o1 = words[:n_one * ONE_OUT].reshape(n_one, ONE_OUT).tolist()
    o2 = words[n_one * ONE_OUT:].reshape(n_co, CO_OUT).tolist()
    bad = []
    for i, r in enumerate(recs):
        err = check_record(r, o2[i - n_one] if r.coop else o1[i])
        if err:
            bad.append('%s [%s] [%s] class %d flags %d: %s' % ((CO_OPS if r.coop else ONE_OPS)[r.op], r.pair, r.rep, r.cls, r.flags, err))
    return bad
