"""-m gpu: the witness screen on calls of a few witnesses (include/zkattest.h: zk_screen_batch) -- a chunk of at most ZK_SCREEN_CO_MAX witnesses runs its point
arithmetic on cooperating waves (k_screen.hip: k_screen_table_co, k_screen_walk_co), counted by zk_test_counter 4 at four chains per witness.  Every expected
value comes from the model of tests/test_gpu_screen.py (the oracle's ecdsa_verify and the ring as a Python list); the witnesses made by hand -- every path in one
call, R = identity, signatures with prescribed u1, u2 -- are built in tests/screen_small_check.py.  Two contexts, with and without per-key tables."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

import screen_small_check as SC
from test_gpu_screen import INVALID, KEY, NONE, NOT_IN_RING, NOT_RESIDENT, RANGE, expect, model, screen, screen_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CO_MAX = int(re.search(r'#define ZK_SCREEN_CO_MAX (\d+)u', open(os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc', 'engine.h')).read()).group(1))
CHUNK = 16384


@pytest.fixture(scope='module')
def ctx():
    c = SC.contexts()
    yield c
    for e in c['engs'].values():
        e.close()


def counted(ctx, fn):
    """fn() and what it added to the process-wide count of chains handed to cooperating waves"""
    e = ctx['engs']['kt']
    c0 = e.test_counter(4)
    res = fn()
    return res, e.test_counter(4) - c0


def on_ring(ctx, ring, wits, which=None, want_chains=None):
    """the host form of both contexts on one resident ring -> the common answer; every call must add 4 chains per witness (or want_chains)"""
    out = []
    for name, e in ctx['engs'].items():
        e.use_ring(ctx['ids'][name][ring])
        res, d = counted(ctx, lambda: screen(e, wits, which))
        assert d == (4 * len(wits) if want_chains is None else want_chains), (name, d)
        out.append(res)
    assert out[0] == out[1], 'the contexts with and without key tables disagree'
    return out[0]


# ---------------------------------------------------------------- 1. the cooperative path is taken and agrees with the model
@pytest.mark.parametrize('B', [1, 3, 8])
def test_small_calls_take_the_cooperative_path_and_agree_with_the_model(ctx, B):
    wits = ctx['wa'][:B]
    exp = expect(wits, ctx['rings']['A'])
    assert exp == (list(range(B)), [0] * B)
    assert on_ring(ctx, 'A', wits) == exp
    for name, e in ctx['engs'].items():
        res, d = counted(ctx, lambda: screen_device(e, wits))
        assert res == exp and d == 4 * B, (name, res, d)


# ---------------------------------------------------------------- 2. every path in one call
def test_path_mix_in_one_call(ctx):
    mix, M = SC.path_mix(ctx), ctx['rings']['M']
    names, wits = list(mix), list(mix.values())
    exp = expect(wits, M)
    fl, wo = dict(zip(names, exp[1])), dict(zip(names, exp[0]))
    assert fl['identity, key in ring'] == INVALID and fl['identity, key not in ring'] == INVALID | NOT_IN_RING, fl   # R = identity has no x-coordinate
    assert fl['member'] == fl['member 2'] == fl['wrap'] == 0 and fl['-pk'] == INVALID and fl['not in ring'] == NOT_IN_RING, fl
    assert fl['off curve'] & KEY and fl['r = 0'] == RANGE, fl
    assert (wo['member'], wo['-pk'], wo['wrap'], wo['identity, key in ring'], wo['member 2'], wo['not in ring']) == (2, 2, 3, 6, 5, NONE), wo
    assert len(wits) == 9 and on_ring(ctx, 'M', wits) == exp
    five = [mix[k] for k in SC.MIX5]
    assert on_ring(ctx, 'M', five) == expect(five, M)
    for name, e in ctx['engs'].items():
        assert screen_device(e, wits) == exp, name
    which = [2, 2, 0, 2, 2, 3, 6, 6, 5]   # check mode: the same paths, the key of 'identity, key not in ring' is not at 6
    assert on_ring(ctx, 'M', wits, which) == expect(wits, M, which)


# ---------------------------------------------------------------- 3. chosen scalars
def test_chosen_scalars(ctx):
    """u2 at the extremes of the walk's and the key table's signed digits, u1 with empty comb windows: a wrong carry, a slip in the top window or a wrong sign
    in the walk or in a wave's range turns a valid signature into INVALID"""
    cases = SC.chosen_scalars(ctx)
    assert len(cases) >= 50 and {c[2] for c in cases} == {True, False}, len(cases)
    wits = [c[3] for c in cases]
    exp = expect(wits, ctx['rings']['M'])
    assert exp == ([4 if c[2] else NONE for c in cases], [0 if c[2] else NOT_IN_RING for c in cases])
    got = on_ring(ctx, 'M', wits)
    bad = [(hex(c[0]), hex(c[1]), c[2], g) for c, g, w in zip(cases, got[1], exp[1]) if g != w]
    assert not bad and got == exp, bad
    one = [on_ring(ctx, 'M', [w])[1][0] for w in wits[::5]]   # ... and a few of them alone in their call
    assert one == exp[1][::5]


# ---------------------------------------------------------------- 4. the threshold and the chunk boundary
@pytest.mark.parametrize('B,chains', [(CO_MAX, 4 * CO_MAX), (CO_MAX + 1, 0), (CHUNK + 3, 12)])
def test_threshold_and_chunk_boundary(ctx, B, chains):
    """at most ZK_SCREEN_CO_MAX witnesses in a chunk: cooperative; one more: the one-lane kernels; 16 384 + 3: the decision is taken per chunk"""
    assert CO_MAX + 1 <= CHUNK
    wa = ctx['wa']
    wits = [wa[i % 8] for i in range(B)]
    exp = expect(wits, ctx['rings']['A'])
    assert exp == ([i % 8 for i in range(B)], [0] * B)
    assert on_ring(ctx, 'A', wits, want_chains=chains) == exp


# ---------------------------------------------------------------- 5. the rings forms
def test_rings_forms(ctx):
    mix = SC.path_mix(ctx)
    wits = [ctx['wa'][1], mix['identity, key in ring'], ctx['wb'][9], mix['-pk'], ctx['wb'][3], mix['wrap']]
    names = ['A', 'M', 'B', 'A', 'A', 'M']
    for name, e in ctx['engs'].items():
        ids = [ctx['ids'][name][k] for k in names]
        exp = [model(w, ctx['rings'][k]) for w, k in zip(wits, names)]
        assert exp == [(1, 0), (6, INVALID), (9, 0), (2, INVALID), (NONE, NOT_IN_RING), (3, 0)]
        want = ([a for a, _ in exp], [b for _, b in exp])
        res, d = counted(ctx, lambda: screen(e, wits, ring_ids=ids))
        assert res == want and d == 4 * 6, (name, res, d)   # the point arithmetic runs once per chunk, not once per ring
        res, d = counted(ctx, lambda: screen_device(e, wits, ring_ids=ids))
        assert res == want and d == 4 * 6, (name, res, d)
        ids[4] = 999   # not resident: bit 16 alone, find and check mode
        exp[4] = (NONE, NOT_RESIDENT)
        assert screen(e, wits, ring_ids=ids) == ([a for a, _ in exp], [b for _, b in exp]), name
        which = [1, 6, 8, 2, 0, 2]
        exp_c = [model(w, ctx['rings'][k], which[i]) for i, (w, k) in enumerate(zip(wits, names))]
        exp_c[4] = (NONE, NOT_RESIDENT)
        assert [b for _, b in exp_c] == [0, INVALID, NOT_IN_RING, INVALID, NOT_RESIDENT, NOT_IN_RING]
        assert screen(e, wits, which=which, ring_ids=ids) == ([a for a, _ in exp_c], [b for _, b in exp_c]), name
        assert screen_device(e, wits, which=which, ring_ids=ids) == ([a for a, _ in exp_c], [b for _, b in exp_c]), name


# ---------------------------------------------------------------- 6. no stray writes
@pytest.mark.parametrize('B', [1, 5])
def test_no_write_past_the_outputs(ctx, B):
    import torch
    dev = 'cuda:0'
    mix = SC.path_mix(ctx)
    wits = [mix[k] for k in SC.MIX5][:B]
    exp = expect(wits, ctx['rings']['M'])
    d_msg, d_sig, d_pk = (torch.frombuffer(bytearray(b''.join(w[i] for w in wits)), dtype=torch.uint8).to(dev) for i in range(3))
    for name, e in ctx['engs'].items():
        e.use_ring(ctx['ids'][name]['M'])
        d_wo = torch.full((B + 4,), 7, dtype=torch.int32, device=dev)
        d_fl = torch.full((B + 4,), 7, dtype=torch.int32, device=dev)
        e.screen_batch_device(B, d_msg.data_ptr(), d_sig.data_ptr(), d_pk.data_ptr(), None, d_wo.data_ptr(), d_fl.data_ptr())
        torch.cuda.synchronize()
        wo, fl = [x & NONE for x in d_wo.cpu().tolist()], [x & NONE for x in d_fl.cpu().tolist()]
        assert (wo[:B], fl[:B]) == exp, name
        assert wo[B:] == [7] * 4 and fl[B:] == [7] * 4, (name, wo, fl)


# ---------------------------------------------------------------- 7. the same answers three ways
def test_cooperative_one_lane_and_uniform_builds_answer_alike():
    import zkp_ecdsa_amd as Z
    uni = os.path.join(os.path.dirname(Z.LIB_PATH), 'libzkattest_hip_uniform.so')
    runs = [('default', {}), ('one lane', {'ZKATTEST_ONE_LANE_CHAINS': '1'})]
    if os.path.exists(uni):
        runs.append(('uniform', {'ZKATTEST_LIB': uni}))
    env0 = {k: v for k, v in os.environ.items() if k != 'ZKATTEST_ONE_LANE_CHAINS'}
    recs = {}
    for tag, extra in runs:
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'screen_small_check.py')], env=dict(env0, **extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert out.returncode == 0, (tag, out.stderr.decode()[-2000:])
        recs[tag] = json.loads(out.stdout.decode().strip().splitlines()[-1])
    d = recs['default']
    assert d['coop'] == 4 * d['witnesses'] and recs['one lane']['coop'] == 0, (d['coop'], recs['one lane']['coop'])
    assert recs['one lane']['answers'] == d['answers']
    flags = [f for ans in d['answers'] for f in ans[1]]
    assert flags.count(0) >= 50 and sum(1 for f in flags if f & INVALID) >= 8
    if 'uniform' not in recs:
        pytest.skip('the uniform build is not there (make -C zkp-ecdsa_amd/csrc uniform); the default and the one-lane answers agree')
    assert recs['uniform']['lib'].endswith('_uniform.so') and recs['uniform']['answers'] == d['answers'] and recs['uniform']['coop'] == d['coop']
