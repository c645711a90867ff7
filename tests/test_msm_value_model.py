"""not-gpu: the integer reference of tests/msm_value_common.py held to itself on every crafted input of tests/test_gpu_msm_value.py -- digits reassemble
the scalars, the window sums add up to the term-by-term totals, and every case has the property it is named for (so many oversized buckets, a bucket of so
many terms), counted by the reference alone with the kernels' thresholds as restated there."""
import pytest

import msm_value_common as MV

TOM = [(n, g) for n in MV.TOM_CASES for g in (8, 64)]
P256 = [(n, g) for n in MV.P_CASES for g in (8, 64)]


def check_reference(c):
    p, u, sc, idx, grp = c.live()
    # the digits reassemble the scalars (P-256: the bits the windows cover)
    top = c.C * c.nw
    for k in list(range(0, len(p), max(1, len(p) // 500))) + [len(p) - 1]:
        s = MV.from_words(sc[k])
        assert sum(int(MV.digits(sc[k], c.C, w)) << (c.C * w) for w in range(c.nw)) == s & ((1 << top) - 1)
        assert c.curve == 'p256' or top >= 256
    assert all(int(MV.digits(sc, c.C, w).max(initial=0)) < 1 << c.C for w in range(c.nw))
    # window sums against the totals term by term
    A, E = c.window_sums()
    dA, dE = c.direct_totals()
    for g in range(c.groups):
        if c.curve == 'tom':
            assert sum(A[w][g] for w in range(c.nw)) % c.mod == dA[g] and sum(E[w][g] for w in range(c.nw)) % 4 == dE[g]
        else:
            assert sum(A[w][g] << (c.C * w) for w in range(c.nw)) % c.mod == dA[g]
    # what the case claims
    sizes = c.bucket_sizes()
    cl = c.claims
    if c.curve == 'tom':
        assert c.n_live() == cl['live'] and (p < c.count).all()
        assert int(sum(s.sum() for s in sizes)) == sum(int((MV.digits(sc, c.C, w) > 0).sum()) for w in range(c.nw))
    if 'big' in cl:
        assert c.big() == cl['big']
    if cl.get('oversized') is not None:
        assert c.n_oversized() == cl['oversized']
    for (w, g, d), n in cl.get('sizes', {}).items():
        assert sizes[w][(g << c.C) | d] == n, (w, g, d)
    for g in cl.get('empty_groups', []):
        assert not (grp == g).any() and all(A[w][g] == 0 for w in range(c.nw))
    if c.curve == 'p256':
        assert c.beyond() == cl['beyond']
    return sizes


@pytest.mark.parametrize('name,groups', TOM)
def test_tom_case_meets_its_conditions(name, groups):
    c = MV.case('tom', name, groups)
    sizes = check_reference(c)
    big = c.big()
    if name == 'random_ragged':
        assert c.count == 37 and c.cap == 48 and len(c.table) == 64 and (c.sc[37:] != 0).any(-1).all()     # garbage in the dead slots
        assert len(c.claims['empty_groups']) == (27 if groups == 64 else 0)
    if name == 'digit_extremes':
        vals = {MV.from_words(w) for w in c.sc[:c.count].reshape(-1, 4)[::1]}
        assert {0, 1, MV.Q - 1, (1 << 255) - 1} <= vals
        assert all(1 << (c.C * w) in vals and ((((1 << c.C) - 1) << (c.C * w)) & ((1 << 256) - 1)) in vals for w in range(c.nw))
        assert all(int(s.max()) > 0 for s in sizes) and int(sizes[c.nw - 1].argmax()) & ((1 << c.C) - 1) < 1 << (256 - c.C * (c.nw - 1))
    if name == 'collisions':
        assert c.n_oversized() == 5   # (all five in the top window)
        assert sorted(int(v) for v in sizes[c.nw - 1][sizes[c.nw - 1] > big]) == [297, 300, 300, 300, 301]
    if name == 'slice_edges':
        allsz = sorted(int(v) for s in sizes for v in s[s >= big])
        assert allsz == [big, big + 1, MV.MSM_SLICE, MV.MSM_SLICE + 1] + ([MV.MSM_NSLICE * MV.MSM_SLICE + 300] if groups == 8 else [])
        assert c.n_oversized() == len(allsz) - 1                       # a bucket of exactly `big` terms is not oversized
        assert groups != 8 or (c.count == 9120 and c.gsz == 1140 > 256 and all(all(v != 0 for v in t) for t in c.coef))
    if name == 'list_overflow':
        assert c.n_oversized() > MV.MSM_BIG_MAX and c.n_live() <= MV.MSM_NBG
        over = [int(v) for s in sizes for v in s[s > big]]
        assert set(over) == {big + 1}
        assert sum(1 for s in sizes if (s > big).any()) == c.nw and len({int(k) >> c.C for s in sizes for k in (s > big).nonzero()[0]}) == groups
        assert sum(int(((s > 0) & (s <= big)).sum()) for s in sizes) >= 300     # ordinary buckets beside them
    if name == 'flags':
        tot = c.totals()
        assert tot[0] == (0, 0, 0) and tot[1][1:] == (0, 0) and tot[1][0] != 0
        assert tot[2] == (0, 0, 2) and tot[3] == (0, 0, 1) and tot[4] == (0, 0, 0) and tot[5] == (0, 0, 0)


@pytest.mark.parametrize('name,groups', P256)
def test_p256_case_meets_its_conditions(name, groups):
    c = MV.case('p256', name, groups)
    sizes = check_reference(c)
    a_max = max(MV.from_words(w) for w in c.sc[:c.count, :MV.VK].reshape(-1, 4)[::7])
    assert a_max < 1 << 128 or name.startswith('bounds')
    if name == 'random_ragged':
        assert c.count == 37 and c.cap == 48 and (c.sc[37:] != 0).any(-1).all()
    if name == 'collisions':
        assert sorted(int(v) for v in sizes[7][sizes[7] > MV.PM_BIG]) == [297, 300, 300, 300, 301]
    if name == 'big_edges':
        allsz = sorted(int(v) for s in sizes for v in s[s >= MV.PM_BIG])
        assert allsz == [MV.PM_BIG, MV.PM_BIG + 1, 256, 257, 1000]
    if name == 'list_overflow':
        assert c.n_oversized() > MV.PM_BIG_MAX and {int(v) for s in sizes for v in s[s > MV.PM_BIG]} == {MV.PM_BIG + 1}
    if name.startswith('bounds'):
        top = c.C * c.nw
        sl = [MV.from_words(w) for w in c.sc[:c.count, MV.VK]]
        assert (1 << 133) - 1 in sl and (1 << top) - 1 in sl and ((1 << top) in sl) == (name == 'bounds_over')
        assert top >= 134 and c.beyond() == (1 if name == 'bounds_over' else 0)


def test_expected_points_add_up():
    """the expected Tw of a group, added as points, are the expected total: the reference's integers and the oracle's points say the same"""
    import zkattest_ref as R
    orc = MV.oracle_from_reference_params()

    def pt(b):
        return R.TEdwardsPoint(MV.TOM, 0, 1) if b == bytes(72) else R.TEdwardsPoint(MV.TOM, int.from_bytes(b[:36], 'big'), int.from_bytes(b[36:], 'big'))
    for name in ('random_ragged', 'flags'):
        c = MV.case('tom', name, 8)
        tw, one, flags, tot = orc.expected_tw(c), orc.expected_one(c), orc.expected_flags(c), c.totals()
        for g in range(c.groups):
            acc = pt(one[g])
            for w in range(c.nw):
                acc = acc.add(pt(tw[w][g]))
            assert acc.eq(pt(orc.tom(tot[g][0], tot[g][2], tot[g][1]))) and acc.isIdentity() == bool(flags[g])
        if name == 'flags':
            assert [flags[g] for g in range(6)] == [c.claims['flags'][g] for g in range(6)] == [1, 0, 0, 0, 1, 1]
    # the table's points are what their multipliers say: P and -P, and the small-order component
    c = MV.case('tom', 'collisions', 8)
    tab = [pt(b) for b in orc.table(c)]
    assert tab[0].add(tab[1]).isIdentity() and not tab[0].add(tab[0]).isIdentity()
    c = MV.case('tom', 'flags', 8)
    a4, e4 = c.table[-1]
    assert e4 == 1 and pt(orc.tom(a4, 1)).add(pt(orc.tom(MV.Q - a4))).eq(orc.P4)
    pc = MV.case('p256', 'collisions', 8)
    t = orc.table(pc)
    assert t[0][:32] == t[1][:32] and int.from_bytes(t[0][32:], 'big') + int.from_bytes(t[1][32:], 'big') == R.p256.p
