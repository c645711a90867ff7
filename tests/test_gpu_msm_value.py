"""-m gpu: the verifier's two cross-proof bucket passes BY VALUE.  zk_test_msm_sum / zk_test_pmsm_sum run the production launch sequences (run_msm;
pmsm_prepare and pmsm_sums) on crafted terms; every window sum Tw[w][grp], the groups' fixed-base points, the flags and the counters are compared, byte for
byte, with the integer reference of tests/msm_value_common.py and ONE fixed-base multiplication by the oracle per point.  Each case also asserts that the
pass saw exactly as many oversized buckets as the reference counts, so a case cannot silently miss the path it is for.  tests/test_msm_value_model.py holds
the reference and the cases' claims to themselves without a GPU.

The cases (both shapes of each pass):
  random_ragged   count = 37 of cap 48: dead slots with garbage, empty groups at 64 groups
  digit_extremes  0, 1, q - 1, 2^255 - 1, one digit / all ones in every window, the narrow top window
  collisions      P + P, P - P, P - P + Q, identity entries, 3 P inside one bucket -- in a lane's walk and filling an oversized bucket
  slice_edges     Tom-256: buckets of big, big + 1, 2 048, 2 049 and 128 x 2 048 + 300 terms; 1 140 proofs per group in k_msm_coef    (P-256: big_edges)
  list_overflow   more oversized buckets than the list holds (4 096 / 2 048): the rest is summed by the ordinary lanes after all
  flags           Tom-256: totals that are the identity, off by one, the point of order 2, a point of order 4
  bounds          P-256: SL = 2^133 - 1 and the largest scalar k_pm_pack admits; one beyond it sets counters[1]
The last reduction of the Tom-256 pass runs on cooperating waves here and in one lane in a child process (ZKATTEST_ONE_LANE_CHAINS, read once per process)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

import msm_value_common as MV


@pytest.fixture(scope='module')
def ctx():
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    raw = eng.synth_params(MV.PARAM_SEED)
    eng.set_params(*raw, 80)
    yield eng, MV.Oracle(*raw)
    eng.close()


@pytest.mark.parametrize('groups', [8, 64])
@pytest.mark.parametrize('name', list(MV.TOM_CASES))
def test_tom_pass_by_value(ctx, name, groups):
    eng, orc = ctx
    c = MV.case('tom', name, groups)
    tw, flags = MV.run_tom(eng, orc, c)
    if name == 'random_ragged':
        for g in c.claims['empty_groups']:   # no live proof: every window the identity, and the verdict 1
            assert flags[g] == 1 and all(tw[w][g] == bytes(72) for w in range(c.nw))
    if name == 'flags':
        assert flags[:6] == [1, 0, 0, 0, 1, 1]   # zero by construction; off by one; order 2; order 4; 4 P4; cancelling fixed-base coefficients only
    if name == 'list_overflow':
        assert c.n_oversized() > MV.MSM_BIG_MAX


@pytest.mark.parametrize('groups', [8, 64])
@pytest.mark.parametrize('name', list(MV.P_CASES))
def test_p256_pass_by_value(ctx, name, groups):
    eng, orc = ctx
    c = MV.case('p256', name, groups)
    _, flags = MV.run_p256(eng, orc, c)
    if name == 'bounds_over':
        # A scalar beyond the windows would be cut off silently, so the pass (k_pm_final) clears EVERY group's flag when counters[1] is set, and the caller
        # (api_verify.hip) sends every proof of the chunk through the per-proof P-256 sums.
        assert flags == [0] * groups


def test_tom_last_reduction_in_one_lane():
    """the same values from k_msm_red_last (one lane per (window, group)) as from the cooperating waves above"""
    env = dict(os.environ, ZKATTEST_ONE_LANE_CHAINS='1')
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'msm_value_one_lane.py')], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, (out.stdout.decode()[-2000:], out.stderr.decode()[-2000:])
    rec = json.loads(out.stdout.decode().strip().splitlines()[-1])
    assert rec['one_lane'] is True and rec['ok'] == [[n, g] for n in ('random_ragged', 'digit_extremes', 'collisions', 'flags') for g in (8, 64)]
