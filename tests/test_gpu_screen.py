"""-m gpu: the witness screen (include/zkattest.h: zk_screen_batch) -- the signer's index in the ring and the ECDSA verdict before a proof is paid for.
Every expected value comes from the small model below, built from oracle/zkattest_ref.py (ecdsa_verify, p256.deserializePoint, truncateToN through
ecdsa_verify) and the ring as a Python list; the engine is never compared with itself.  Two contexts, with and without per-key tables, must agree."""
import ctypes as C
import functools
import random

import pytest

pytestmark = pytest.mark.gpu

import zkattest_ref as R

S = 7331
P, N_ORD = R.p256.p, R.p256.order
NONE = 0xFFFFFFFF
KEY, RANGE, INVALID, NOT_IN_RING, NOT_RESIDENT = 1, 2, 4, 8, 16
ZK_E_BUFFER, ZK_E_ARG = 12, 14


# ---------------------------------------------------------------- the model
@functools.lru_cache(maxsize=None)
def model_sig(msg, sig, pk):
    """bits 1, 2, 4 of one witness"""
    fl = 0
    try:
        R.p256.deserializePoint(b'\x04' + pk)
    except ValueError:
        fl |= KEY
    r, s = int.from_bytes(sig[:32], 'big'), int.from_bytes(sig[32:], 'big')
    if not (1 <= r < N_ORD and 1 <= s < N_ORD):
        fl |= RANGE
    if not fl and not R.ecdsa_verify(b'\x04' + pk, msg, sig):
        fl |= INVALID
    return fl


def model(wit, ring, which=None):
    """ring: the caller's keys as a list of integers -> (which_out, flags) of the witness (msg, sig, pk)"""
    msg, sig, pk = wit
    x = int.from_bytes(pk[:32], 'big') % P
    n_pad = 1 << max(1, (len(ring) - 1).bit_length())
    if which is None:
        wo = next((i for i, k in enumerate(ring) if k == x), NONE)
        miss = wo == NONE
    else:
        wo = which
        miss = which >= n_pad or (ring[which] if which < len(ring) else ring[0]) != x
    return wo, model_sig(msg, sig, pk) | (NOT_IN_RING if miss else 0)


def expect(wits, ring, which=None):
    res = [model(w, ring, None if which is None else which[i]) for i, w in enumerate(wits)]
    return [a for a, _ in res], [b for _, b in res]


# ---------------------------------------------------------------- helpers
def ints(ring_bytes):
    return [int.from_bytes(ring_bytes[32 * i:32 * i + 32], 'big') for i in range(len(ring_bytes) // 32)]


def ring_bytes(ring):
    return b''.join(k.to_bytes(32, 'big') for k in ring)


def wits_of(W, count=None):
    _, msg, sig, pk, which, _ = W
    return [(msg[32 * b:32 * b + 32], sig[64 * b:64 * b + 64], pk[64 * b:64 * b + 64]) for b in range(len(which) if count is None else count)]


def screen(eng, wits, which=None, ring_ids=None):
    return eng.screen_batch(b''.join(w[0] for w in wits), b''.join(w[1] for w in wits), b''.join(w[2] for w in wits), which=which, ring_ids=ring_ids)


def screen_device(eng, wits, which=None, ring_ids=None):
    import torch
    dev = 'cuda:0'
    B = len(wits)

    def up(parts):
        return torch.frombuffer(bytearray(b''.join(parts)), dtype=torch.uint8).to(dev)

    def u32(v):
        return torch.tensor([x if x < 2 ** 31 else x - 2 ** 32 for x in v], dtype=torch.int32).to(dev)
    d_msg, d_sig, d_pk = up(w[0] for w in wits), up(w[1] for w in wits), up(w[2] for w in wits)
    d_w = u32(which) if which is not None else None
    d_ids = u32(ring_ids) if ring_ids is not None else None
    d_wo = torch.full((B,), 7, dtype=torch.int32, device=dev)
    d_fl = torch.full((B,), 7, dtype=torch.int32, device=dev)
    eng.screen_batch_device(B, d_msg.data_ptr(), d_sig.data_ptr(), d_pk.data_ptr(), d_w.data_ptr() if d_w is not None else None, d_wo.data_ptr(), d_fl.data_ptr(),
                            d_ring_ids=d_ids.data_ptr() if d_ids is not None else None)
    torch.cuda.synchronize()
    return [x & NONE for x in d_wo.cpu().tolist()], [x & NONE for x in d_fl.cpu().tolist()]


def flip(b, bit):
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


def neg_pk(pk):
    return pk[:32] + ((P - int.from_bytes(pk[32:], 'big')) % P).to_bytes(32, 'big')


def be(v):
    return v.to_bytes(32, 'big')


def named_mutants(w, other):
    """the issue's list for one valid witness w = (msg, sig, pk); other: another ring member's witness"""
    msg, sig, pk = w
    r, s = sig[:32], sig[32:]
    return {
        'msg bit': (flip(msg, 13), sig, pk), 'r bit': (msg, flip(r, 5) + s, pk), 's bit': (msg, r + flip(s, 201), pk),
        '-pk': (msg, sig, neg_pk(pk)), 'other member': (msg, sig, other[2]), 'off curve': (msg, sig, flip(pk, 300)),
        'r = 0': (msg, be(0) + s, pk), 's = 0': (msg, r + be(0), pk), 'r = n': (msg, be(N_ORD) + s, pk), 's = n': (msg, r + be(N_ORD), pk),
    }


def random_mutant(rnd, w):
    msg, sig, pk = w
    f = rnd.randrange(4)
    if f == 0:
        return (flip(msg, rnd.randrange(256)), sig, pk)
    if f == 1:
        return (msg, flip(sig, rnd.randrange(512)), pk)
    if f == 2:
        return (msg, sig, flip(pk, rnd.randrange(512)))
    return w   # the field is rewritten with its own value: a valid witness


def sqrt_p(v):
    y = pow(v, (P + 1) // 4, P)
    return y if y * y % P == v % P else None


def curve_y(x):
    return sqrt_p((x * x * x - 3 * x + R.p256.b) % P)


# ---------------------------------------------------------------- the contexts
RINGS = {'A': 8, 'B': 1000, 'C': 5000}


@pytest.fixture(scope='module')
def ctx():
    """Two contexts at secLevel 20 -- per-key tables on and off -- with rings A, B, C and the edge ring E resident; the workloads, the rings as lists"""
    import zkp_ecdsa_amd as Z
    engs = {}
    for name, kt in (('kt', 1), ('nokt', 0)):
        e = Z.Engine(0)
        e.set_key_tables(kt)
        e.set_params(*e.synth_params(S), 20)
        engs[name] = e
    e = engs['kt']
    # every synthetic witness has a key of its own, planted at ring[b mod n_keys]: a workload is all valid only while B <= n_keys
    W = {k: e.synth_workload(S + i, n, {'A': 8, 'B': 65, 'C': 257}[k]) for i, (k, n) in enumerate(sorted(RINGS.items()))}
    rings = {k: ints(W[k][0]) for k in W}
    # the edge ring: C with witness 1's key moved to the last index, witness 2's key at two other indices, witness 3's key gone, and a small x at 5
    wc = wits_of(W['C'], 8)
    xs = [int.from_bytes(w[2][:32], 'big') for w in wc]
    E = list(rings['C'])
    rnd = random.Random(S)
    for i in (1, 2, 3):
        E[i] = rnd.randrange(P)
    E[4999] = xs[1]
    E[77] = E[3000] = xs[2]
    small = next(x for x in range(1, 100) if curve_y(x) is not None and x < 2 ** 256 - P)
    E[5] = small
    rings['E'] = E
    # the wrap case: P0 with x = n + 3, r = 3, pk = r^-1 (s P0 - z G); its x goes into ring A at index 3
    G, sc = R.p256.generator(), R.p256.newScalar
    y0 = curve_y(N_ORD + 3)
    assert y0 is not None
    P0 = R.WeierstrassPoint(R.p256, N_ORD + 3, y0)
    msgw, sw = W['A'][1][:32], 0x1234567890abcdef1234567890abcdef
    z = R.truncateToN(int.from_bytes(msgw, 'big'), N_ORD)
    pkw = P0.mul(sc(sw)).add(G.mul(sc((N_ORD - z) % N_ORD))).mul(sc(pow(3, -1, N_ORD)))
    xw, yw = pkw.toAffine()
    Wr = list(rings['A'])
    Wr[3] = xw
    rings['W'] = Wr
    wrap = (msgw, be(3) + be(sw), be(xw) + be(yw))
    ids = {}
    for name, e in engs.items():
        ids[name] = {k: e.add_ring(ring_bytes(rings[k])) for k in ('A', 'B', 'C', 'E', 'W')}
    yield {'engs': engs, 'W': W, 'rings': rings, 'ids': ids, 'small': small, 'wrap': wrap}
    for e in engs.values():
        e.close()


def both(ctx, ring, wits, which=None):
    """the host entry point of both contexts on one resident ring (made active) -> the common answer"""
    out = []
    for name, e in ctx['engs'].items():
        e.use_ring(ctx['ids'][name][ring])
        out.append(screen(e, wits, which))
    assert out[0] == out[1], 'the contexts with and without key tables disagree'
    return out[0]


# ---------------------------------------------------------------- 1. valid witnesses, find mode
@pytest.mark.parametrize('B', [1, 65, 257])
def test_valid_witnesses_find_mode(ctx, B):
    wits = wits_of(ctx['W']['C'], B)
    exp = expect(wits, ctx['rings']['C'])
    assert exp == (ctx['W']['C'][4][:B], [0] * B)   # the model itself: every synthetic witness is valid and sits at the workload's index
    assert both(ctx, 'C', wits) == exp
    for name, e in ctx['engs'].items():
        assert screen_device(e, wits) == exp, name
    if B == 65:   # the small rings: 8 witnesses over the 8 keys of A, 65 over the first 65 of B's 1 000
        for k in ('A', 'B'):
            wk = wits_of(ctx['W'][k])
            assert both(ctx, k, wk) == (ctx['W'][k][4], [0] * len(wk)) == expect(wk, ctx['rings'][k])


# ---------------------------------------------------------------- 2. lookup edges on the 5 000-key ring
def test_lookup_edges(ctx):
    E, wc = ctx['rings']['E'], wits_of(ctx['W']['C'], 8)
    small = ctx['small']
    shifted = (wc[0][0], wc[0][1], be(small + P) + be(curve_y(small)))   # x-bytes x + p: the same ring value as x
    plain = (wc[0][0], wc[0][1], be(small) + be(curve_y(small)))
    wits = [wc[0], wc[1], wc[2], wc[3], shifted, plain]
    exp = expect(wits, E)
    assert exp[0] == [0, 4999, 77, NONE, 5, 5] and exp[1][:4] == [0, 0, 0, NOT_IN_RING] and exp[1][4] == exp[1][5] == INVALID
    assert both(ctx, 'E', wits) == exp
    for name, e in ctx['engs'].items():
        assert screen_device(e, wits) == exp, name
    # check mode: correct, correct at the last index, wrong, in the padding for the owner of keys[0], in the padding for somebody else, >= N
    cw = [wc[0], wc[1], wc[0], wc[0], wc[1], wc[0], wc[2], wc[2]]
    which = [0, 4999, 10, 5000, 8191, 8192, 3000, NONE]
    exp = expect(cw, E, which)
    assert exp == (which, [0, 0, NOT_IN_RING, 0, NOT_IN_RING, NOT_IN_RING, 0, NOT_IN_RING])
    assert both(ctx, 'E', cw, which) == exp
    for name, e in ctx['engs'].items():
        assert screen_device(e, cw, which) == exp, name


# ---------------------------------------------------------------- 3. ECDSA mutants
def test_named_mutants(ctx):
    wa = wits_of(ctx['W']['A'], 8)
    muts = named_mutants(wa[2], wa[5])
    names, wits = list(muts), list(muts.values())
    exp = expect(wits, ctx['rings']['A'])
    byname = dict(zip(names, exp[1]))
    assert byname['-pk'] == INVALID and byname['other member'] == INVALID and byname['off curve'] & KEY, byname
    assert all(byname[k] == RANGE for k in ('r = 0', 's = 0', 'r = n', 's = n')) and byname['msg bit'] == byname['s bit'] == INVALID, byname
    assert exp[0][names.index('-pk')] == 2 and exp[0][names.index('other member')] == 5
    assert both(ctx, 'A', wits) == exp
    assert both(ctx, 'A', wits, [2] * len(wits)) == expect(wits, ctx['rings']['A'], [2] * len(wits))


def test_random_mutant_sweep(ctx):
    rnd = random.Random(S + 1)
    wb = wits_of(ctx['W']['B'])
    wits = [random_mutant(rnd, wb[i % len(wb)]) for i in range(240)]
    exp = expect(wits, ctx['rings']['B'])
    good, bad = sum(1 for f in exp[1] if f == 0), sum(1 for f in exp[1] if f & INVALID)
    assert good >= 20 and bad >= 20, (good, bad)   # the model gives both verdicts: the sweep is not one-sided
    assert both(ctx, 'B', wits) == exp


# ---------------------------------------------------------------- 4. the wrap case R.x in [n, p)
def test_wrap_case(ctx):
    msg, sig, pk = ctx['wrap']
    assert R.ecdsa_verify(b'\x04' + pk, msg, sig)
    over = (msg, be(N_ORD + 3) + sig[32:], pk)   # the same r written as n + 3: out of range for the screen, the same witness for the prover
    exp = expect([ctx['wrap'], over], ctx['rings']['W'])
    assert exp == ([3, 3], [0, RANGE])
    assert both(ctx, 'W', [ctx['wrap'], over]) == exp


# ---------------------------------------------------------------- 5. flags == 0 means the proof verifies
def test_screen_predicts_the_verifier(ctx):
    eng, rid = ctx['engs']['kt'], ctx['ids']['kt']['A']
    seeds = ctx['W']['B'][5]
    wa = wits_of(ctx['W']['A']) * 3   # 24 witnesses over the ring's 8 signers
    wits = list(wa)
    muts = named_mutants(wa[3], wa[6])
    for i, k in enumerate(['msg bit', 's bit', '-pk', 'other member', 'off curve']):
        wits[2 * i + 1] = muts[k]
    wits[11] = (wa[11][0], wa[11][1], wits_of(ctx['W']['B'], 1)[0][2])                        # a key that is not in the ring
    for i, b in enumerate((13, 15, 17, 19, 21, 23)):
        m = named_mutants(wa[b], wa[(b + 1) % 8])
        wits[b] = m[['msg bit', '-pk', 's bit', 'other member', 'msg bit', '-pk'][i]]
    eng.use_ring(rid)
    wo, fl = screen(eng, wits)
    assert (wo, fl) == expect(wits, ctx['rings']['A']) and sum(1 for f in fl if f) == 12
    proofs, st = eng.prove_batch(b''.join(w[0] for w in wits), b''.join(w[1] for w in wits), b''.join(w[2] for w in wits), [0 if w == NONE else w for w in wo], seeds=seeds[:32 * 24])
    made = [b for b in range(24) if proofs[b] is not None]
    ok, _ = eng.verify_batch(b''.join(wits[b][0] for b in made), [proofs[b] for b in made])
    verdict = [0] * 24
    for b, o in zip(made, ok):
        verdict[b] = o
    assert verdict == [1 if f == 0 else 0 for f in fl], (verdict, fl, st)


# ---------------------------------------------------------------- 6. rings
def test_mixed_rings_and_unknown_id(ctx):
    wits, names = [], []
    for i in range(60):
        k = 'ABC'[i % 3]
        ws = wits_of(ctx['W'][k])
        w = ws[(i // 3) % len(ws)]
        wits.append(w if i % 5 else (flip(w[0], i), w[1], w[2]))
        names.append(k)
    for name, e in ctx['engs'].items():
        ids = [ctx['ids'][name][k] for k in names]
        exp_wo, exp_fl = [], []
        for w, k in zip(wits, names):
            a, b = model(w, ctx['rings'][k])
            exp_wo.append(a), exp_fl.append(b)
        per_ring = ([None] * 60, [None] * 60)
        for k in 'ABC':
            idx = [i for i in range(60) if names[i] == k]
            e.use_ring(ctx['ids'][name][k])
            a, b = screen(e, [wits[i] for i in idx])
            for j, i in enumerate(idx):
                per_ring[0][i], per_ring[1][i] = a[j], b[j]
        assert per_ring == (exp_wo, exp_fl), name
        assert screen(e, wits, ring_ids=ids) == (exp_wo, exp_fl), name
        assert screen_device(e, wits, ring_ids=ids) == (exp_wo, exp_fl), name
        ids[7] = ids[20] = 999   # not resident: bit 16 alone
        exp_wo[7] = exp_wo[20] = NONE
        exp_fl[7] = exp_fl[20] = NOT_RESIDENT
        assert screen(e, wits, ring_ids=ids) == (exp_wo, exp_fl), name
        which = [w if w != NONE else 3 for w in exp_wo]   # check mode through the rings form
        exp_c = [model(w, ctx['rings'][k], which[i]) for i, (w, k) in enumerate(zip(wits, names))]
        exp_c[7] = exp_c[20] = (NONE, NOT_RESIDENT)
        assert screen(e, wits, which=which, ring_ids=ids) == ([a for a, _ in exp_c], [b for _, b in exp_c]), name


def test_screen_after_update_ring(ctx):
    wa, wb = wits_of(ctx['W']['A'], 8), wits_of(ctx['W']['B'], 8)
    for name, e in ctx['engs'].items():
        rid = e.add_ring(ctx['W']['A'][0])
        assert screen(e, [wa[2], wb[5]], ring_ids=[rid, rid]) == ([2, NONE], [0, NOT_IN_RING])
        e.update_ring(rid, {2: wb[5][2][:32]})
        ring = list(ctx['rings']['A'])
        ring[2] = int.from_bytes(wb[5][2][:32], 'big')
        exp = expect([wa[2], wb[5]], ring)
        assert exp == ([NONE, 2], [NOT_IN_RING, 0])
        assert screen(e, [wa[2], wb[5]], ring_ids=[rid, rid]) == exp, name
        e.drop_ring(rid)


# ---------------------------------------------------------------- 7. call-level statuses
def test_call_level_statuses(ctx):
    import zkp_ecdsa_amd as Z
    w = wits_of(ctx['W']['A'], 4)
    e = Z.Engine(0)
    try:
        for kw in ({}, {'ring_ids': [0] * 4}):
            with pytest.raises(Z.ZkError) as ei:   # before zk_ctx_set_params
                screen(e, w, **kw)
            assert ei.value.status == ZK_E_BUFFER
        e.set_params(*e.synth_params(S), 20)
        with pytest.raises(Z.ZkError) as ei:       # no active ring
            screen(e, w)
        assert ei.value.status == ZK_E_BUFFER
        assert screen(e, w, ring_ids=[5] * 4) == ([NONE] * 4, [NOT_RESIDENT] * 4)   # the rings form needs none
        rid = e.add_ring(ctx['W']['A'][0])
        e.use_ring(rid)
        assert screen(e, []) == ([], []) and screen(e, [], ring_ids=[]) == ([], [])   # B = 0
        msg, sig, pk = (b''.join(x[i] for x in w) for i in range(3))
        out = (C.c_uint32 * 4)()
        L, h = e.L, e.h
        assert L.zk_screen_batch(h, 4, msg, sig, pk, None, None, out) == ZK_E_ARG
        assert L.zk_screen_batch(h, 4, msg, sig, pk, None, out, None) == ZK_E_ARG
        assert L.zk_screen_batch(h, 4, None, sig, pk, None, out, out) == ZK_E_ARG
        assert L.zk_screen_batch_rings(h, 4, msg, sig, pk, None, None, out, out) == ZK_E_ARG
        assert L.zk_screen_batch_device(h, 4, None, None, None, None, None, None) == ZK_E_ARG
        assert L.zk_screen_batch_rings_device(h, 4, None, None, None, None, None, None, None) == ZK_E_ARG
        _, m, s, p, which, seeds = ctx['W']['A']
        buf = Z.PinnedBuffer(e.proof_max_size() * 2)
        t = e.prove_submit(m[:64], s[:128], p[:128], which[:2], seeds[:64], buf)   # a streamed job is queued
        with pytest.raises(Z.ZkError) as ei:
            screen(e, w)
        assert ei.value.status == ZK_E_ARG
        with pytest.raises(Z.ZkError) as ei:
            screen(e, w, ring_ids=[rid] * 4)
        assert ei.value.status == ZK_E_ARG
        _, st = e.prove_wait(t)
        assert list(st) == [0, 0]
        assert screen(e, w) == ([0, 1, 2, 3], [0] * 4)
        buf.free()
    finally:
        e.close()


# ---------------------------------------------------------------- 8. the prover is not disturbed
def test_screen_between_prove_calls(ctx):
    eng = ctx['engs']['kt']
    eng.use_ring(ctx['ids']['kt']['A'])
    _, msg, sig, pk, which, seeds = ctx['W']['A']
    args = (msg[:32 * 6], sig[:64 * 6], pk[:64 * 6], which[:6])
    first = eng.prove_batch(*args, seeds=seeds[:32 * 6])
    assert screen(eng, wits_of(ctx['W']['A']) * 5) == (which * 5, [0] * 40)
    assert screen(eng, wits_of(ctx['W']['B'], 9), ring_ids=[ctx['ids']['kt']['B']] * 9) == (list(range(9)), [0] * 9)
    assert eng.prove_batch(*args, seeds=seeds[:32 * 6]) == first and first[1] == [0] * 6


# ---------------------------------------------------------------- the uniform build
def test_uniform_build_gives_the_same_flags():
    import json
    import os
    import subprocess
    import sys
    import zkp_ecdsa_amd as Z
    uni = os.path.join(os.path.dirname(Z.LIB_PATH), 'libzkattest_hip_uniform.so')
    if not os.path.exists(uni):
        pytest.skip('the uniform build is not there (make -C zkp-ecdsa_amd/csrc uniform)')
    recs = []
    for lib in (Z.LIB_PATH, uni):
        out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'screen_uniform_check.py')], env=dict(os.environ, ZKATTEST_LIB=lib),
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        recs.append(json.loads(out.stdout.decode().strip().splitlines()[-1]))
    assert recs[1]['lib'].endswith('_uniform.so') and recs[0]['answers'] == recs[1]['answers']
    flags = [f for ans in recs[0]['answers'] for f in ans[1]]
    assert flags.count(0) >= 16 and any(f & INVALID for f in flags)
