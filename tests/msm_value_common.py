"""Shared by tests/test_msm_value_model.py (no GPU) and tests/test_gpu_msm_value.py: crafted term sets for the verifier's two cross-proof bucket passes
(csrc/k_msm.hip, Tom-256; csrc/k_pmsm.hip, P-256) and their sums by plain integers.

Every table point is a known multiple a_j of the base (g of the Tom-256 parameters, G of P-256), on Tom-256 optionally plus e_j times the point of order 4,
so every sum the passes compute is ONE integer (mod the group order, the small-order part mod 4) and the expected point is ONE fixed-base multiplication by
the oracle.  Nothing here is computed by the engine.

    Tom-256:  Tw[w][grp] = ( sum_{live terms of grp} digit_w(s_i) a_i 2^(C w) mod q ) g          total[grp] = sum_w Tw[w][grp] + cg g + ch h
    P-256:    Tw[w][grp] = ( sum_{terms of grp} digit_w(s_i) a_i mod n ) G                       (k_pm_reduce leaves the 2^(C w) to k_pm_final)

A term is live when its proof is below `count` and (Tom-256 only) its scalar is not zero.  Constants restated from the kernels: see below.
"""
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
import zkattest_ref as R   # noqa: E402

TOM = R.tomEdwards256
Q = TOM.order          # scalars of the Tom-256 pass
PN = R.p256.order      # scalars of the P-256 pass
NONE = 0xffffffff      # point index of the identity entry (Tom-256 only)
PARAM_SEED = 5

# restated from csrc/engine.h, k_msm.hip and k_pmsm.hip
VK, V_SLOT_TERMS = 20, 36
TOM_SHAPE = {8: (16, 16), 64: (13, 20)}     # groups -> (C, windows): ceil(256 / C) windows, 2^19 (group, digit) keys per window
P_SHAPE = {8: (13, 11), 64: (10, 14)}       # groups -> (C, windows): ceil(134 / C) windows
MSM_NBG = 1 << 19
MSM_SLICE, MSM_NSLICE, MSM_BIG_MAX = 2048, 128, 4096
PM_BIG, PM_BIG_MAX = 64, 2048
M64 = (1 << 64) - 1


def tom_big(nlive):
    """k_msm_bucket: a bucket with MORE terms than this is oversized"""
    return 8 * ((nlive + MSM_NBG - 1) // MSM_NBG) + 64


def to_words(v):
    return [(v >> (64 * i)) & M64 for i in range(4)]


def from_words(w):
    return sum(int(w[i]) << (64 * i) for i in range(4))


def digits(sc, C, w):
    """digit w (C bits) of the scalars sc[..., 4] (little-endian 64-bit words), as the kernels cut it: bits [C w, C (w + 1)) of the 256-bit value"""
    k, sh = divmod(C * w, 64)
    if k >= 4:
        return np.zeros(sc.shape[:-1], dtype=np.int64)
    d = sc[..., k] >> np.uint64(sh)
    if sh + C > 64 and k + 1 < 4:
        d = d | (sc[..., k + 1] << np.uint64(64 - sh))
    return (d & np.uint64((1 << C) - 1)).astype(np.int64)


class Case:
    """One call of a hook: terms per (proof slot, local slot), the table's multipliers, and what the case claims about itself."""

    def __init__(self, curve, name, groups, cap, count, nq=1):
        self.curve, self.name, self.groups, self.cap, self.count, self.nq = curve, name, groups, cap, count, nq
        self.C, self.nw = (TOM_SHAPE if curve == 'tom' else P_SHAPE)[groups]
        self.mod = Q if curve == 'tom' else PN
        self.T = VK * V_SLOT_TERMS + 8 * nq + 3 if curve == 'tom' else VK + 1
        self.gsz = -(-count // groups) if count else 1
        self.table = []                                   # (a_j, e_j): a_j base + e_j P4
        self.sc = np.zeros((cap, self.T, 4), dtype=np.uint64)
        self.idx = np.zeros((cap, self.T), dtype=np.uint32)
        self.coef = [(0, 0, 0, 0)] * count                # Tom-256: mg, mh, eg, eh per live proof
        self.cur = {}
        self.claims = {}                                  # 'oversized': n, 'sizes': {(w, grp, digit): n}, 'live': n, 'beyond': 0 / 1, 'flags': {grp: 0 / 1}

    # ---- layout
    def group_range(self, g):
        p0 = min(g * self.gsz, self.count)
        return p0, min(self.count, p0 + self.gsz)

    def alloc(self, g, n, cl=False):
        """the next n free local slots of group g: Tom-256 any slot; P-256 the A slots (u < 20) or, cl, the Clambda slots (u = 20)"""
        p0, p1 = self.group_range(g)
        per = self.T if self.curve == 'tom' else (1 if cl else VK)
        s0 = self.cur.get((g, cl), 0)
        assert s0 + n <= (p1 - p0) * per, (self.name, g, s0, n, (p1 - p0) * per)
        self.cur[(g, cl)] = s0 + n
        s = np.arange(s0, s0 + n)
        return p0 + s // per, (np.full(n, VK) if self.curve == 'p256' and cl else s % per)

    def put(self, g, scalars, idxs, cl=False):
        """terms (scalar, table index) into the next free slots of group g"""
        n = len(idxs)
        if isinstance(scalars, int):
            scalars = [scalars] * n
        p, u = self.alloc(g, n, cl)
        uniq = {}
        for v in scalars:
            if v not in uniq:
                assert 0 <= v < self.mod, (self.name, v)
                uniq[v] = to_words(v)
        self.sc[p, u] = np.array([uniq[v] for v in scalars], dtype=np.uint64)
        self.idx[p, u] = np.asarray(idxs, dtype=np.uint32)

    def point(self, a, e=0):
        self.table.append((a % self.mod, e % 4))
        return len(self.table) - 1

    def term_ids(self):
        """[cap, T]: the pass's id of every (proof slot, local slot) -- include/zkattest.h: zk_test_msm_sum, zk_test_pmsm_sum"""
        p = np.arange(self.cap, dtype=np.int64)[:, None]
        u = np.arange(self.T, dtype=np.int64)[None, :]
        cap, nq = self.cap, self.nq
        if self.curve == 'p256':
            return np.where(u < VK, VK * p + u, VK * cap + p)
        n0, n1 = VK * V_SLOT_TERMS * cap, 8 * nq * cap
        v, m = u - VK * V_SLOT_TERMS, u - VK * V_SLOT_TERMS - 8 * nq
        return np.where(u < VK * V_SLOT_TERMS, (u // VK) * (VK * cap) + VK * p + u % VK,
                        np.where(m < 0, n0 + (v // nq) * (nq * cap) + nq * p + v % nq, n0 + n1 + m * cap + p))

    def hook_arrays(self):
        """(term_idx uint32[nterms], term_sc uint8[nterms, 32] big-endian) in term-id order"""
        ids = self.term_ids().ravel()
        n = self.cap * self.T
        assert len(np.unique(ids)) == n and ids.min() == 0 and ids.max() == n - 1
        idx = np.empty(n, dtype=np.uint32)
        idx[ids] = self.idx.ravel()
        be = np.empty((n, 4), dtype='>u8')
        be[ids] = self.sc.reshape(n, 4)[:, ::-1]
        return idx, np.ascontiguousarray(be).view(np.uint8).reshape(n, 32)

    # ---- the reference
    def live(self):
        """(proof, local slot) of the live terms, their scalars' words, table indices and groups"""
        m = np.zeros((self.cap, self.T), dtype=bool)
        m[:self.count] = True
        if self.curve == 'tom':
            m &= (self.sc != 0).any(-1)
        p, u = np.nonzero(m)
        return p, u, self.sc[p, u], self.idx[p, u].astype(np.int64), p // self.gsz

    def window_sums(self):
        """A[w][grp], E[w][grp]: the coefficient of the base (mod the group order; Tom-256: times 2^(C w)) and of P4 (mod 4) in Tw[w][grp]"""
        _, _, sc, idx, grp = self.live()
        nt = len(self.table)
        idx = np.where(idx >= nt, nt, idx)
        A = [[0] * self.groups for _ in range(self.nw)]
        E = [[0] * self.groups for _ in range(self.nw)]
        for w in range(self.nw):
            d = digits(sc, self.C, w)
            cnt = np.bincount(grp * (nt + 1) + idx, weights=d.astype(np.float64), minlength=self.groups * (nt + 1))
            assert cnt.max(initial=0) < 2.0 ** 52   # exact in a double
            cnt = cnt.reshape(self.groups, nt + 1)
            scale = 1 << (self.C * w) if self.curve == 'tom' else 1
            for g in range(self.groups):
                for j in np.nonzero(cnt[g, :nt])[0]:
                    a, e = self.table[j]
                    A[w][g] += int(cnt[g, j]) * a
                    E[w][g] += int(cnt[g, j]) * e
                A[w][g] = A[w][g] * scale % self.mod
                E[w][g] = E[w][g] * scale % 4
        return A, E

    def direct_totals(self):
        """sum s_i a_i (mod the order) and sum s_i e_i (mod 4) per group, term by term over the whole scalars (P-256: cut to the windows' bits, as k_pm_pack cuts)"""
        _, _, sc, idx, grp = self.live()
        A, E = [0] * self.groups, [0] * self.groups
        cut = (1 << (self.C * self.nw)) - 1
        for k in range(len(idx)):
            if idx[k] < len(self.table):
                a, e = self.table[idx[k]]
                s = from_words(sc[k]) & cut
                A[grp[k]] += s * a
                E[grp[k]] += s * e
        return [v % self.mod for v in A], [v % 4 for v in E]

    def bucket_sizes(self):
        """sizes[w]: terms per (group << C | digit) key of window w (digit 0 takes no part), as the passes group them"""
        _, _, sc, _, grp = self.live()
        out = []
        for w in range(self.nw):
            d = digits(sc, self.C, w)
            sel = d > 0
            out.append(np.bincount((grp[sel] << self.C) | d[sel], minlength=self.groups << self.C))
        return out

    def n_live(self):
        return len(self.live()[0])

    def big(self):
        return tom_big(self.n_live()) if self.curve == 'tom' else PM_BIG

    def n_oversized(self):
        big = self.big()
        return int(sum((s > big).sum() for s in self.bucket_sizes()))

    def beyond(self):
        """P-256: 1 if a scalar of a live proof has a bit at or above windows x C (k_pm_pack: counters[1])"""
        sc = self.sc[:self.count].reshape(-1, 4)
        top = self.C * self.nw
        k, sh = divmod(top, 64)
        hit = (sc[:, k] >> np.uint64(sh)) != 0
        for j in range(k + 1, 4):
            hit |= sc[:, j] != 0
        return int(hit.any())

    def fixed_sums(self):
        """Tom-256: (cg, ch) per group -- the sums of mg + eg and of mh + eh over the group's proofs (k_msm_coef)"""
        out = []
        for g in range(self.groups):
            p0, p1 = self.group_range(g)
            out.append((sum(self.coef[p][0] + self.coef[p][2] for p in range(p0, p1)) % Q, sum(self.coef[p][1] + self.coef[p][3] for p in range(p0, p1)) % Q))
        return out

    def totals(self):
        """Tom-256: per group (coefficient of g, of h, of P4) of windows + fixed-base part; the pass's flag is 1 iff that point is the identity"""
        A, E = self.window_sums()
        fx = self.fixed_sums()
        return [((sum(A[w][g] for w in range(self.nw)) + fx[g][0]) % Q, fx[g][1], sum(E[w][g] for w in range(self.nw)) % 4) for g in range(self.groups)]


# ---------------------------------------------------------------- the oracle's points
class Oracle:
    """expected points: one fixed-base multiplication by the C oracle per point; the small-order part added with the Python reference's complete addition"""

    def __init__(self, nist_h64, tom_g72, tom_h72):
        import coracle as CO
        import escrow_common as EC
        self.CO = CO
        self.octx = CO.OracleCtx(nist_h64, tom_g72, tom_h72, 80)
        self.P4 = EC.small_order_points()[1]
        self.cache = {}

    def tom(self, a, e=0, r=0):
        """a g + r h + e P4 as 72 bytes; the identity as zero bytes"""
        key = (a % Q, e % 4, r % Q)
        if key not in self.cache:
            b = self.octx.tom_commit(key[0], key[2])
            x, y = int.from_bytes(b[:36], 'big'), int.from_bytes(b[36:], 'big')
            if key[1]:
                pt = R.TEdwardsPoint(TOM, x, y)
                for _ in range(key[1]):
                    pt = pt.add(self.P4)
                x, y = pt.toAffine()
            self.cache[key] = bytes(72) if (x, y) == (0, 1) else x.to_bytes(36, 'big') + y.to_bytes(36, 'big')
        return self.cache[key]

    def p256(self, a):
        key = ('p', a % PN)
        if key not in self.cache:
            self.cache[key] = (self.CO.p256_mul(key[1]) if key[1] else None) or bytes(64)
        return self.cache[key]

    def table(self, case):
        return [self.tom(a, e) if case.curve == 'tom' else self.p256(a) for a, e in case.table]

    def expected_tw(self, case):
        A, E = case.window_sums()
        f = (lambda a, e: self.tom(a, e)) if case.curve == 'tom' else (lambda a, e: self.p256(a))
        return [[f(A[w][g], E[w][g]) for g in range(case.groups)] for w in range(case.nw)]

    def expected_one(self, case):
        return [self.tom(cg, 0, ch) for cg, ch in case.fixed_sums()]

    def expected_flags(self, case):
        return [1 if self.tom(a, e, r) == bytes(72) else 0 for a, r, e in case.totals()]


def oracle_from_reference_params():
    """the oracle over the synthetic parameters of seed PARAM_SEED, from the Python reference alone (no GPU)"""
    p = R.synth_params(PARAM_SEED, 80)

    def xy(pt, w):
        x, y = pt.toAffine()
        return x.to_bytes(w, 'big') + y.to_bytes(w, 'big')
    return Oracle(xy(p.NistGroup.h, 32), xy(p.ProofGroup.g, 36), xy(p.ProofGroup.h, 36))


# ---------------------------------------------------------------- generators
def _rand_table(case, rnd, n):
    return [case.point(rnd.randrange(1, case.mod)) for _ in range(n)]


def _single(case, w, d):
    """the scalar whose only non-zero digit is d in window w"""
    v = d << (case.C * w)
    assert v < case.mod and (case.curve == 'tom' or v < 1 << (case.C * case.nw))
    return v


def _fill_bucket(case, rnd, g, w, d, n, tab, cl=False):
    """n terms of random table points into bucket (w, digit d) of group g; claims its size"""
    case.put(g, _single(case, w, d), [tab[rnd.randrange(len(tab))] for _ in range(n)], cl)
    key = (w, g, d)
    case.claims.setdefault('sizes', {})[key] = case.claims.get('sizes', {}).get(key, 0) + n


def _rand_coef(case, rnd):
    case.coef = [tuple(rnd.randrange(1, Q) for _ in range(4)) for _ in range(case.count)]


def tom_random_ragged(groups):
    """1: count = 37 of cap 48, uniform scalars, 64 points; the dead slots 37..47 hold non-zero scalars and valid points; at 64 groups 27 groups are empty"""
    rnd = random.Random(101 + groups)
    c = Case('tom', 'random_ragged', groups, 48, 37)
    tab = _rand_table(c, rnd, 64)
    c.sc[:] = np.array([to_words(rnd.randrange(1, Q)) for _ in range(c.cap * c.T)], dtype=np.uint64).reshape(c.cap, c.T, 4)
    c.idx[:] = np.array([tab[rnd.randrange(64)] for _ in range(c.cap * c.T)], dtype=np.uint32).reshape(c.cap, c.T)
    _rand_coef(c, rnd)
    c.claims.update(live=37 * c.T, oversized=0, empty_groups=[g for g in range(groups) if g * c.gsz >= 37])
    return c


def tom_digit_extremes(groups):
    """2: 0, 1, q - 1, 2^255 - 1, and per window 1 << C w and (2^C - 1) << C w cut to the top window's width; a zero scalar is not live"""
    rnd = random.Random(202 + groups)
    c = Case('tom', 'digit_extremes', groups, 16, 16)
    tab = _rand_table(c, rnd, 16)
    vals = [0, 1, Q - 1, (1 << 255) - 1]
    for w in range(c.nw):
        vals += [1 << (c.C * w), (((1 << c.C) - 1) << (c.C * w)) & ((1 << 256) - 1)]
    assert all(v < Q for v in vals)
    nz = 0
    for g in range(min(groups, 16)):
        # every value in every live group, walking through the three term lists: the slots, the membership terms and the three per proof
        p0, p1 = c.group_range(g)
        per = (p1 - p0) * c.T
        rep = max(1, min(3, per // len(vals)))
        c.put(g, vals * rep, [tab[rnd.randrange(16)] for _ in range(rep * len(vals))])
        nz += rep * (len(vals) - 1)
        rest = per - c.cur[(g, False)]
        tail = [vals[(7 * k + g) % len(vals)] for k in range(rest)]   # ... to the group's last slot: the misc terms are at the end of a proof's slots
        c.put(g, tail, [tab[rnd.randrange(16)] for _ in range(rest)])
        nz += sum(1 for v in tail if v)
    _rand_coef(c, rnd)
    c.claims.update(live=nz, oversized=None)
    return c


def _collision_patterns(c, rnd):
    P, Q_ = rnd.randrange(1, c.mod), rnd.randrange(1, c.mod)
    iP, iN, iQ = c.point(P), c.point(-P), c.point(Q_)
    ident = NONE if c.curve == 'tom' else None
    small = [[iP, iP], [iP, iN], [iP, iN, iQ], [ident, iP, ident], [iP, iP, iP]]
    large = [[iP] * 300, [iP, iN] * 150, [iP, iN] * 150 + [iQ], [ident] * 100 + [iP] * 200, [iP, iP, iP] * 99]
    if ident is None:   # an affine table has no identity entry
        small[3], large[3] = [iP, iQ, iN, iN], [iP, iQ, iN, iN] * 75
    return small, large


def tom_collisions(groups):
    """3: P + P, P - P, P - P + Q, identity entries with P, 3 P in one bucket -- once among a few terms (k_msm_bucket's lane), once filling an oversized
    bucket of 297..301 terms so that equal and opposite points meet in a lane of k_msm_bucket_big and in its tree"""
    rnd = random.Random(303 + groups)
    c = Case('tom', 'collisions', groups, 2 * groups, 2 * groups)
    small, large = _collision_patterns(c, rnd)
    for k in range(5):
        g = (3 * k + 1) % groups
        c.put(g, _single(c, 3, 5 + k), small[k])
        rnd.shuffle(large[k])
        c.put(g, _single(c, c.nw - 1, 9 + k), large[k])
        c.claims.setdefault('sizes', {}).update({(3, g, 5 + k): len(small[k]), (c.nw - 1, g, 9 + k): len(large[k])})
    _rand_coef(c, rnd)
    c.claims.update(live=sum(len(s) + len(b) for s, b in zip(small, large)), oversized=5)
    return c


def tom_slice_edges(groups):
    """4: one group holds buckets of exactly big, big + 1, MSM_SLICE, MSM_SLICE + 1 and (8 groups) MSM_NSLICE * MSM_SLICE + 300 terms: the threshold, a
    second slice of one term beside 126 empty ones, and the wrap of the slice loop.  8 groups: count = 9 120, so a group's 1 140 proofs also take
    k_msm_coef's strided sum beyond 256.  64 groups: the four smaller buckets (the wrap needs 262 444 terms in ONE group, 23 k proofs at 64 groups)."""
    rnd = random.Random(404 + groups)
    count = 9120 if groups == 8 else 448
    c = Case('tom', 'slice_edges', groups, count, count)
    tab = _rand_table(c, rnd, 64)
    big = 72                                   # 8 x ceil(live / 2^19) + 64 for at most 2^19 live terms; checked against the reference's count
    sizes = [big, big + 1, MSM_SLICE, MSM_SLICE + 1] + ([MSM_NSLICE * MSM_SLICE + 300] if groups == 8 else [])
    g = 3
    for k, n in enumerate(sizes):
        _fill_bucket(c, rnd, g, (5 * k + 2) % c.nw, 1000 + 77 * k, n, tab)
    for gg in range(groups):                   # a few ordinary terms everywhere
        for _ in range(20):
            _fill_bucket(c, rnd, gg, rnd.randrange(c.nw - 1), rnd.randrange(1, 1 << c.C), 1, tab)
    _rand_coef(c, rnd)
    c.claims.update(live=sum(sizes) + 20 * groups, oversized=len(sizes) - 1, big=big)
    return c


def tom_list_overflow(groups):
    """5: 4 100 oversized buckets (MSM_BIG_MAX = 4 096 fit the list) of big + 1 terms each over windows, groups and digits, a few hundred ordinary terms beside"""
    rnd = random.Random(505 + groups)
    nover, big = MSM_BIG_MAX + 4, 72
    per_group = -(-nover // groups)
    count = groups * -(-(per_group * (big + 1) + 64) // (VK * V_SLOT_TERMS + 8 + 3))
    c = Case('tom', 'list_overflow', groups, count, count)
    tab = _rand_table(c, rnd, 32)
    for k in range(nover):
        g, j = k % groups, k // groups
        _fill_bucket(c, rnd, g, j % c.nw, 1 + (j // c.nw) * 3 + (g % 3), big + 1, tab)   # (top window: digits stay below its 2^8 / 2^9 values)
    for gg in range(groups):
        for _ in range(40):
            _fill_bucket(c, rnd, gg, rnd.randrange(c.nw - 1), rnd.randrange(1 << (c.C - 1), 1 << c.C), 1, tab)
    _rand_coef(c, rnd)
    c.claims.update(live=nover * (big + 1) + 40 * groups, oversized=nover, big=big)
    return c


def tom_flags(groups, off_by_one=True):
    """6: group 0: many random terms whose total with the fixed-base part is 0 by construction (flag 1); group 1: the same with one scalar off by one
    (flag 0); groups 2, 3: the total is exactly the point of order 2 / of order 4 (flag 0: x = 0, y = -z and y = 0); group 4: four times the point of order
    4, the identity (flag 1); group 5: no terms, fixed-base coefficients that cancel (flag 1)"""
    rnd = random.Random(606 + groups)
    gsz = 8 if groups == 8 else 3
    c = Case('tom', 'flags', groups, groups * gsz, groups * gsz)
    tab = _rand_table(c, rnd, 32)
    comp_a = rnd.randrange(1, Q)
    comp = c.point(comp_a)
    a4 = rnd.randrange(1, Q)
    with4 = c.point(a4, 1)                     # a4 g + P4
    coef = [(0, 0, 0, 0)] * c.count
    flags = {}

    def close(g, extra=0):
        """the compensating term: scalar s with s comp_a = -(sum of the group so far + cg), then + extra"""
        tot = sum(from_words(c.sc[p, u]) * c.table[c.idx[p, u]][0] for p in range(*c.group_range(g)) for u in range(c.T) if c.sc[p, u].any())
        p0, p1 = c.group_range(g)
        cg = sum(coef[p][0] + coef[p][2] for p in range(p0, p1))
        s = -(tot + cg) * pow(comp_a, -1, Q) % Q
        c.put(g, [(s + extra) % Q], [comp])

    for g in (0, 1):
        c.put(g, [rnd.randrange(1, Q) for _ in range(1500)], [tab[rnd.randrange(32)] for _ in range(1500)])
        for p in range(*c.group_range(g)):
            r = rnd.randrange(1, Q)
            coef[p] = (rnd.randrange(1, Q), r, rnd.randrange(1, Q), Q - r)   # mh + eh = 0 mod q
        close(g, extra=g)
        flags[g] = 1 - g
    for g, k in ((2, 2), (3, 1), (4, 4)):      # k (a4 g + P4) + compensation = k P4
        c.put(g, [rnd.randrange(1, Q) for _ in range(200)], [tab[rnd.randrange(32)] for _ in range(200)])
        c.put(g, [k], [with4])
        close(g)
        flags[g] = 1 if k == 4 else 0
    p0, _ = c.group_range(5)
    r = rnd.randrange(1, Q)
    coef[p0], coef[p0 + 1] = (r, 5, 7, Q - 9), (Q - r, 4, Q - 7, 0)
    flags[5] = 1
    c.coef = coef
    c.claims.update(live=2 * 1501 + 3 * 202, oversized=None, flags=flags)
    return c


TOM_CASES = {'random_ragged': tom_random_ragged, 'digit_extremes': tom_digit_extremes, 'collisions': tom_collisions, 'slice_edges': tom_slice_edges,
             'list_overflow': tom_list_overflow, 'flags': tom_flags}


def _p_rand_terms(c, rnd, tab, bound_a=1 << 128, bound_sl=1 << 134):
    n = c.cap * VK
    c.sc[:, :VK] = np.array([to_words(rnd.randrange(1, bound_a)) for _ in range(n)], dtype=np.uint64).reshape(c.cap, VK, 4)
    c.sc[:, VK] = np.array([to_words(rnd.randrange(1, bound_sl)) for _ in range(c.cap)], dtype=np.uint64)
    c.idx[:] = np.array([tab[rnd.randrange(len(tab))] for _ in range(c.cap * c.T)], dtype=np.uint32).reshape(c.cap, c.T)


def p_random_ragged(groups):
    """1: count = 37 of cap 48: A scalars below 2^128, SL below 2^134, garbage in the dead slots; the top windows see only SL's few high bits"""
    rnd = random.Random(1101 + groups)
    c = Case('p256', 'random_ragged', groups, 48, 37)
    _p_rand_terms(c, rnd, _rand_table(c, rnd, 64))
    c.claims.update(live=37 * 21, oversized=None, beyond=0, empty_groups=[g for g in range(groups) if g * c.gsz >= 37])
    return c


def p_digit_extremes(groups):
    """2: per window 1 << C w and (2^C - 1) << C w, 0, 1, 2^128 - 1 in the A terms; the windows above bit 128 through SL"""
    rnd = random.Random(1202 + groups)
    c = Case('p256', 'digit_extremes', groups, 16, 16)
    tab = _rand_table(c, rnd, 16)
    top = c.C * c.nw
    va = [0, 1, (1 << 128) - 1] + [v for w in range(c.nw) for v in (1 << (c.C * w), ((1 << c.C) - 1) << (c.C * w)) if v < 1 << 128]
    vs = [v & ((1 << top) - 1) for w in range(c.nw) for v in (1 << (c.C * w), ((1 << c.C) - 1) << (c.C * w))]
    for g in range(min(groups, 16)):
        p0, p1 = c.group_range(g)
        na, ns = (p1 - p0) * VK, p1 - p0
        c.put(g, [va[(k + 5 * g) % len(va)] for k in range(na)], [tab[rnd.randrange(16)] for _ in range(na)])
        c.put(g, [vs[(k + 3 * g) % len(vs)] for k in range(ns)], [tab[rnd.randrange(16)] for _ in range(ns)], cl=True)
    c.claims.update(live=16 * 21, oversized=None, beyond=0)
    return c


def p_collisions(groups):
    """3: P + P, P - P, P - P + Q, P + Q - P - P, 3 P through the mixed complete addition: among a few terms and filling an oversized bucket (k_pm_big)"""
    rnd = random.Random(1303 + groups)
    count = 16 * groups
    c = Case('p256', 'collisions', groups, count, count)
    small, large = _collision_patterns(c, rnd)
    for k in range(5):
        g = (3 * k + 1) % groups
        c.put(g, _single(c, 2, 5 + k), small[k])
        rnd.shuffle(large[k])
        c.put(g, _single(c, 7, 9 + k), large[k])
        c.claims.setdefault('sizes', {}).update({(2, g, 5 + k): len(small[k]), (7, g, 9 + k): len(large[k])})
    c.claims.update(live=count * 21, oversized=5, beyond=0)
    return c


def p_big_edges(groups):
    """4: buckets of exactly PM_BIG, PM_BIG + 1, 256, 257 and 1 000 terms in one group: the threshold and the 256-thread stride of k_pm_big"""
    rnd = random.Random(1404 + groups)
    count = 96 * groups
    c = Case('p256', 'big_edges', groups, count, count)
    tab = _rand_table(c, rnd, 64)
    sizes = [PM_BIG, PM_BIG + 1, 256, 257, 1000]
    for k, n in enumerate(sizes):
        _fill_bucket(c, rnd, 3, (2 * k + 1) % 9, 100 + 77 * k, n, tab)
    for gg in range(groups):
        for _ in range(20):
            _fill_bucket(c, rnd, gg, rnd.randrange(9), rnd.randrange(1, 1 << c.C), 1, tab)
    c.claims.update(live=count * 21, oversized=4, beyond=0)
    return c


def p_list_overflow(groups):
    """5: 2 052 oversized buckets (PM_BIG_MAX = 2 048 fit the list) of PM_BIG + 1 terms each, ordinary terms beside them"""
    rnd = random.Random(1505 + groups)
    nover = PM_BIG_MAX + 4
    per_group = -(-nover // groups)
    count = groups * -(-(per_group * (PM_BIG + 1) + 64) // VK)
    c = Case('p256', 'list_overflow', groups, count, count)
    tab = _rand_table(c, rnd, 32)
    nwa = 128 // c.C                           # windows that lie wholly below bit 128: single-digit scalars there are A scalars
    for k in range(nover):
        g, j = k % groups, k // groups
        _fill_bucket(c, rnd, g, j % nwa, 1 + j // nwa, PM_BIG + 1, tab)
    for gg in range(groups):
        for _ in range(40):
            _fill_bucket(c, rnd, gg, rnd.randrange(nwa), rnd.randrange(1 << (c.C - 1), 1 << c.C), 1, tab)
    c.claims.update(live=count * 21, oversized=nover, beyond=0)
    return c


def p_bounds(groups, over=False):
    """7: SL = 2^133 - 1 and SL = 2^(windows C) - 1, the largest value k_pm_pack admits; `over`: one more scalar, 2^(windows C), sets counters[1]"""
    rnd = random.Random(1707 + groups)
    c = Case('p256', 'bounds_over' if over else 'bounds', groups, 2 * groups, 2 * groups)
    tab = _rand_table(c, rnd, 16)
    _p_rand_terms(c, rnd, tab)
    top = c.C * c.nw
    c.sc[0, VK] = to_words((1 << 133) - 1)
    c.sc[3, VK] = to_words((1 << top) - 1)
    c.sc[c.count - 1, 7] = to_words((1 << top) - 1)
    if over:
        c.sc[5, VK] = to_words(1 << top)
    c.claims.update(live=c.count * 21, oversized=None, beyond=1 if over else 0)
    return c


P_CASES = {'random_ragged': p_random_ragged, 'digit_extremes': p_digit_extremes, 'collisions': p_collisions, 'big_edges': p_big_edges,
           'list_overflow': p_list_overflow, 'bounds': p_bounds, 'bounds_over': lambda groups: p_bounds(groups, True)}

_cases = {}


def case(curve, name, groups):
    """the case, built once per process and left unchanged"""
    key = (curve, name, groups)
    if key not in _cases:
        _cases[key] = (TOM_CASES if curve == 'tom' else P_CASES)[name](groups)
    return _cases[key]


# ---------------------------------------------------------------- running a case on an engine
def run_tom(eng, orc, c):
    """zk_test_msm_sum on case c; asserts every Tw, the fixed-base point, the flags, the live terms and that the oversized counter is the reference's"""
    idx, sc = c.hook_arrays()
    tw, one, flags, live, over = eng.test_msm_sum(c.groups, c.cap, c.count, c.nq, orc.table(c), idx, sc, c.coef)
    exp_tw, exp_over = orc.expected_tw(c), c.n_oversized()
    print('%s/%d: live %d (reference %d), oversized %d (reference %d), big %d' % (c.name, c.groups, live, c.n_live(), over, exp_over, c.big()))
    assert live == c.n_live()
    assert over == exp_over
    bad = [(w, g) for w in range(c.nw) for g in range(c.groups) if tw[w][g] != exp_tw[w][g]]
    assert not bad, ('Tw differs at (window, group)', bad[:20], len(bad))
    assert one == orc.expected_one(c)
    assert flags == orc.expected_flags(c)
    return tw, flags


def run_p256(eng, orc, c):
    """zk_test_pmsm_sum on case c; asserts every Tw, counters[1] and that counters[2] is the reference's count"""
    idx, sc = c.hook_arrays()
    tw, flags, beyond, over = eng.test_pmsm_sum(c.groups, c.cap, c.count, orc.table(c), idx, sc)
    exp_tw, exp_over = orc.expected_tw(c), c.n_oversized()
    print('%s/%d: beyond %d (reference %d), oversized %d (reference %d)' % (c.name, c.groups, beyond, c.beyond(), over, exp_over))
    assert beyond == c.beyond()
    assert over == exp_over
    bad = [(w, g) for w in range(c.nw) for g in range(c.groups) if tw[w][g] != exp_tw[w][g]]
    assert not bad, ('Tw differs at (window, group)', bad[:20], len(bad))
    return tw, flags
