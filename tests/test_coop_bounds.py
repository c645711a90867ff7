"""CPU checks of the bounds the lane-cooperative field arithmetic (zkp-ecdsa_amd/csrc/coop.h) relies on: interval arithmetic over the generated constants, no GPU,
in the style of test_field_bounds.py.  A CoFe<M, K> holds a value < K*M in limbs that are only NEARLY normalised (limbs 0..7 <= 2^30 - 1 + CO_NEAR); the comments of
coop.h claim that this never overflows a 32-bit lane or a 64-bit accumulator.  These tests compute the worst case of every claim from the constants."""
import os
import re

from test_field_bounds import KCAP, MASK, NL, W, _consts, _top, _val

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COOP = open(os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc', 'coop.h')).read()
CO_NEAR = int(re.search(r'#define CO_NEAR (\d+)u', COOP).group(1))
FULL = MASK + CO_NEAR
KS = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]
CARRY_MAX = ((1 << 32) - 1) >> W          # what one parallel carry step can hand to the next limb


def _worst(K, M):
    """limb-wise upper bound of a CoFe<M, K>"""
    return [FULL] * (NL - 1) + [_top(K, M)]


def test_a_carry_step_and_a_product_stay_nearly_normalised():
    """co_carry: limbs < 2^32 in, low part + at most 3 out -- CO_NEAR must cover it, and the top limb must have room for what limb 7 hands up."""
    assert CARRY_MAX <= CO_NEAR
    for name, d in _consts().items():
        assert _top(KCAP, _val(d['mod'])) + CARRY_MAX < 1 << 32


def test_montgomery_rounds_stay_within_the_column_budget():
    """co_mont_round, nine times: t += a_i * b_j;  t += m * M_j (m < 2^30);  t = (t >> 30) + lo30(t of the lane above).  Worst case per lane over every magnitude pair the
    static_assert admits: the accumulator stays below 2^61 + 2^34 (the comment's budget; 2^64 is the hard limit), the part a lane hands to the next limb at the end
    (co_hi30) is at most CO_NEAR, and the top lane ends below 2^30 with nothing left to hand to lane 9."""
    worst = 0
    for name, d in _consts().items():
        M, N = _val(d['mod']), d['mod']
        for Ka in KS:
            for Kb in KS:
                if Ka * Kb > d['kmax']:
                    continue
                A, B = _worst(Ka, M), _worst(Kb, M)
                U = [0] * NL                                            # lanes 9..15: b = 0 and M_j = 0, so t stays 0 there
                for i in range(NL):
                    assert all(u < (1 << 32) + (1 << 30) for u in U)   # "t < 2^32 + 2^30 before a round"
                    U = [U[j] + A[i] * B[j] + MASK * N[j] for j in range(NL)]
                    assert all(u < (1 << 61) + (1 << 34) for u in U), (name, Ka, Kb, i, max(U).bit_length())
                    worst = max(worst, max(U))
                    U = [(U[j] >> W) + (min(MASK, U[j + 1]) if j + 1 < NL else 0) for j in range(NL)]
                assert all((u >> W) <= CO_NEAR for u in U[:NL - 1]), (name, Ka, Kb, [u >> W for u in U])
                assert U[NL - 1] + CO_NEAR < 1 << W, (name, Ka, Kb)       # limb 8 = lo30(t_8) + hi30(t_7) < 2^30 and hi30(t_8) = 0: nothing leaves lane 8
    assert worst > 1 << 61                                              # the budget is what the comment says, not a loose one


def test_sums_and_differences_fit_a_lane_in_every_limb_top_limb_included():
    """co_add: a + b;  co_sub / co_addsub: a + S - b with S = C*M in the twice-lent form of co_sub_const, for every (Ka, C) the static_asserts admit
    (Ka + C <= KCAP, Kb < C) -- no limb underflows or overflows 32 bits, and the carry step that follows has room in the top limb."""
    for name, d in _consts().items():
        M = _val(d['mod'])
        for Ka in KS:
            for Kb in KS:
                if Ka + Kb <= KCAP:
                    s = [x + y for x, y in zip(_worst(Ka, M), _worst(Kb, M))]
                    assert all(x < 1 << 32 for x in s) and s[NL - 1] + CARRY_MAX < 1 << 32
        lend = [1 << W] + [MASK] * (NL - 2) + [-1]
        for C in (4, 8, 16, 32, 64, 128, 256):
            S = [x + y for x, y in zip(d['sub%d' % C], lend)]
            assert _val(S) == C * M and all(0 <= x < 1 << 32 for x in S)
            b = _worst(C - 1, M)                                      # the largest subtrahend SubC sends to this constant
            assert all(S[i] >= b[i] for i in range(NL)), (name, C, [hex(x) for x in S])
            a = _worst(KCAP - C, M)                                   # the largest minuend
            assert all(a[i] + S[i] < 1 << 32 for i in range(NL)), (name, C)
            assert a[NL - 1] + S[NL - 1] + CARRY_MAX < 1 << 32
            # the compile-time form of the same two top-limb facts (co_sub_consts_fit): tops bounded by K * (M_8 + 1)
            m8 = d['mod'][NL - 1] + 1
            assert _top(C - 1, M) <= (C - 1) * m8 and _top(KCAP, M) <= KCAP * m8
            assert d['sub%d' % C][NL - 1] >= 1 + (C - 1) * m8 and d['sub%d' % C][NL - 1] + KCAP * m8 + CO_NEAR < 1 << 32


def test_the_static_assert_of_coop_h_looks_at_the_top_limb():
    body = re.search(r'constexpr bool co_sub_consts_fit\(\) \{(.*?)\n\}', COOP, re.S).group(1)
    assert 'NLIMB - 1]' in body and 'KCAP' in body


def test_double_and_triple_fit_a_lane_before_the_carry_step():
    """co_double / co_triple: a + a (+ a) in every limb, then one carry step; 2K, 3K <= KCAP"""
    for name, d in _consts().items():
        M = _val(d['mod'])
        for n in (2, 3):
            assert n * FULL < 1 << 32
            assert n * _top(KCAP // n, M) + CARRY_MAX < 1 << 32
            assert (n * FULL >> W) <= CO_NEAR
