"""-m gpu: key recovery (include/zkattest.h: zk_recover_batch) -- the signer's key from (msgHash, signature) alone and its index in the ring.  Every
expected value comes from the model of tests/recover_common.py (oracle/zkattest_ref.py and Python integers); the engine is never compared with itself.
Two contexts, with and without per-key tables, must agree.

A chunk of at most ZK_SCREEN_CO_MAX witnesses runs on cooperating waves, so most calls below take that path; the one-lane kernels are held to the same
bytes by the child-process comparison (tests/recover_small_check.py, ZKATTEST_ONE_LANE_CHAINS) and by the calls of more than 4 096 witnesses."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

import recover_common as RC
import zkattest_ref as R

S = 7331
P, N_ORD = RC.P, RC.N_ORD
NONE = RC.NONE
RANGE, NOT_IN_RING, NOT_RESIDENT, NO_POINT = RC.SIG_RANGE, RC.NOT_IN_RING, RC.RING_NOT_RESIDENT, RC.NO_POINT
ZK_E_BUFFER, ZK_E_ARG = 12, 14
be = RC.be


# ---------------------------------------------------------------- helpers
def ints(ring_bytes):
    return [int.from_bytes(ring_bytes[32 * i:32 * i + 32], 'big') for i in range(len(ring_bytes) // 32)]


def ring_bytes(ring):
    return b''.join(k.to_bytes(32, 'big') for k in ring)


def wits_of(W, count=None):
    """(msg, sig) pairs of a synthetic workload"""
    _, msg, sig, _, which, _ = W
    return [(msg[32 * b:32 * b + 32], sig[64 * b:64 * b + 64]) for b in range(len(which) if count is None else count)]


def keys_of(W, count=None):
    _, _, _, pk, which, _ = W
    return [pk[64 * b:64 * b + 64] for b in range(len(which) if count is None else count)]


def recover(eng, wits, ring_ids=None):
    return eng.recover_batch(b''.join(w[0] for w in wits), b''.join(w[1] for w in wits), ring_ids=ring_ids)


def recover_device(eng, wits, ring_ids=None):
    import torch
    dev = 'cuda:0'
    B = len(wits)
    d_msg = torch.frombuffer(bytearray(b''.join(w[0] for w in wits)), dtype=torch.uint8).to(dev)
    d_sig = torch.frombuffer(bytearray(b''.join(w[1] for w in wits)), dtype=torch.uint8).to(dev)
    d_ids = torch.tensor([x if x < 2 ** 31 else x - 2 ** 32 for x in ring_ids], dtype=torch.int32).to(dev) if ring_ids is not None else None
    d_pk = torch.full((64 * B,), 7, dtype=torch.uint8, device=dev)
    d_wo = torch.full((B,), 7, dtype=torch.int32, device=dev)
    d_fl = torch.full((B,), 7, dtype=torch.int32, device=dev)
    eng.recover_batch_device(B, d_msg.data_ptr(), d_sig.data_ptr(), d_pk.data_ptr(), d_wo.data_ptr(), d_fl.data_ptr(), d_ring_ids=d_ids.data_ptr() if d_ids is not None else None)
    torch.cuda.synchronize()
    raw, fl = bytes(d_pk.cpu().numpy().tobytes()), [x & NONE for x in d_fl.cpu().tolist()]
    for b in range(B):   # the device form writes 64 zero bytes where there is no key
        assert fl[b] == 0 or raw[64 * b:64 * b + 64] == bytes(64)
    return [raw[64 * b:64 * b + 64] if fl[b] == 0 else None for b in range(B)], [x & NONE for x in d_wo.cpu().tolist()], fl


def flip(b, bit):
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


def aff(pt):
    a = pt.toAffine()
    return a if a else None


def nonce_point_is_odd(msg, sig, pk):
    """parity of y(R) for R = (z / s) G + (r / s) pk: the candidate number (mod 2) under which pk is recovered"""
    r, s = int.from_bytes(sig[:32], 'big'), int.from_bytes(sig[32:], 'big')
    z, w = R.truncateToN(int.from_bytes(msg, 'big'), N_ORD), pow(s, -1, N_ORD)
    X = R.p256.generator().dblmul(R.p256.newScalar(z * w), R.p256.deserializePoint(b'\x04' + pk), R.p256.newScalar(r * w))
    return X.toAffine()[1] & 1


def sign(d, k, msg):
    """an ECDSA signature with key d and nonce k (no low-s rule): (sig, R = k G affine)"""
    Rp = aff(R.p256.generator().mul(R.p256.newScalar(k)))
    z, r = R.truncateToN(int.from_bytes(msg, 'big'), N_ORD), Rp[0] % N_ORD
    return be(r) + be(pow(k, -1, N_ORD) * (z + r * d) % N_ORD), Rp


# ---------------------------------------------------------------- the contexts
RINGS = {'A': 8, 'B': 1000, 'C': 5000}


def contexts():
    """Two contexts at secLevel 20 -- per-key tables on and off -- with rings A, B, C and the edge rings resident; the workloads, the rings as lists"""
    import zkp_ecdsa_amd as Z
    engs = {}
    for name, kt in (('kt', 1), ('nokt', 0)):
        e = Z.Engine(0)
        e.set_key_tables(kt)
        e.set_params(*e.synth_params(S), 20)
        engs[name] = e
    e = engs['kt']
    W = {k: e.synth_workload(S + i, n, {'A': 8, 'B': 65, 'C': 257}[k]) for i, (k, n) in enumerate(sorted(RINGS.items()))}
    rings = {k: ints(W[k][0]) for k in W}
    G, sc = R.p256.generator(), R.p256.newScalar
    rnd = random.Random(S)
    wc, kc = wits_of(W['C'], 8), keys_of(W['C'], 8)
    xs = [int.from_bytes(k[:32], 'big') for k in kc]
    # the edge ring: C with witness 1's key moved to the last index, witness 2's key at two other indices, witness 3's key gone
    E = list(rings['C'])
    for i in (1, 2, 3):
        E[i] = rnd.randrange(P)
    E[4999] = xs[1]
    E[77] = E[3000] = xs[2]
    # ... witness 4: the x of its OTHER candidate of the same x(R) (the non-signer's) planted below the signer's index 4
    c4 = dict(RC.candidates(*wc[4]))
    own4 = next(c for c, Q in c4.items() if Q is not None and Q[0] == xs[4])
    other4 = c4[own4 ^ 1]
    E[0] = other4[0]   # (witness 0 loses its key: it is not used with this ring)
    # ... z = 0 mod n: msg_hash = the bytes of n, key d, nonce k; Q0 = -Q1 share one x, planted at 10
    d, k = rnd.randrange(1, N_ORD), rnd.randrange(1, N_ORD)
    zmsg = be(N_ORD)
    zsig, _ = sign(d, k, zmsg)
    zQ = aff(G.mul(sc(d)))
    E[10] = zQ[0]
    # ... an identity candidate: R = k G, s = z / k makes Q = (s R - z G) / r the identity under R's own parity; the sibling is (-2 z / r) G, planted at 11
    k2 = rnd.randrange(1, N_ORD)
    imsg = wc[5][0]
    zi = R.truncateToN(int.from_bytes(imsg, 'big'), N_ORD)
    R2 = aff(G.mul(sc(k2)))
    r2 = R2[0] % N_ORD
    isig = be(r2) + be(zi * pow(k2, -1, N_ORD) % N_ORD)
    sib = aff(G.mul(sc((-2 * zi * pow(r2, -1, N_ORD)) % N_ORD)))
    E[11] = sib[0]
    rings['E'] = E
    # the wrap case of the screen's test: P0 with x = n + 3, r = 3, pk = r^-1 (s P0 - z G); its x goes into ring A at index 3
    y0 = RC.lift(N_ORD + 3)[1]
    P0 = R.WeierstrassPoint(R.p256, N_ORD + 3, y0)
    msgw, sw = W['A'][1][:32], 0x1234567890abcdef1234567890abcdef
    z = R.truncateToN(int.from_bytes(msgw, 'big'), N_ORD)
    pkw = P0.mul(sc(sw)).add(G.mul(sc((N_ORD - z) % N_ORD))).mul(sc(pow(3, -1, N_ORD)))
    xw, yw = pkw.toAffine()
    Wr = list(rings['A'])
    Wr[3] = xw
    rings['W'] = Wr
    edge = {'wrap': (msgw, be(3) + be(sw)), 'wrap_pk': be(xw) + be(yw), 'other4': be(other4[0]) + be(other4[1]), 'zero_z': (zmsg, zsig), 'zero_z_x': zQ[0],
            'ident': (imsg, isig), 'ident_sib': be(sib[0]) + be(sib[1])}
    ids = {}
    for name, e in engs.items():
        ids[name] = {k: e.add_ring(ring_bytes(rings[k])) for k in ('A', 'B', 'C', 'E', 'W')}
    return {'engs': engs, 'W': W, 'rings': rings, 'ids': ids, 'edge': edge}


@pytest.fixture(scope='module')
def ctx():
    c = contexts()
    yield c
    for e in c['engs'].values():
        e.close()


def edge_list_large(ctx):
    """the edge witnesses of ring E: the last index; the lowest of two; a key that is gone; the non-signer's candidate at the lower index; z = 0 mod n; an
    identity candidate; a valid witness, its message bit flip and its s bit flip"""
    ed, wc = ctx['edge'], wits_of(ctx['W']['C'], 8)
    return [wc[1], wc[2], wc[3], wc[4], ed['zero_z'], ed['ident'], wc[6], (flip(wc[6][0], 13), wc[6][1]), (wc[6][0], flip(wc[6][1], 256 + 201))]


def edge_list_small(ctx):
    """the edge witnesses of ring W: the wrap witness; an r with no curve point and r + n >= p; r = 0, s = 0, r = n, s = n; a valid witness"""
    wa = wits_of(ctx['W']['A'], 8)
    msg, sig = wa[2]
    r, s = sig[:32], sig[32:]
    rnd = random.Random(S + 2)
    nopoint = next(x for x in (rnd.randrange(P - N_ORD, N_ORD) for _ in range(64)) if RC.lift(x) is None)
    return [ctx['edge']['wrap'], (msg, be(nopoint) + s), (msg, be(0) + s), (msg, r + be(0)), (msg, be(N_ORD) + s), (msg, r + be(N_ORD)), wa[5]]


def both(ctx, ring, wits):
    """the host entry point of both contexts on one resident ring (made active) -> the common answer"""
    out = []
    for name, e in ctx['engs'].items():
        e.use_ring(ctx['ids'][name][ring])
        out.append(recover(e, wits))
    assert out[0] == out[1], 'the contexts with and without key tables disagree'
    return out[0]


# ---------------------------------------------------------------- 1. valid witnesses
@pytest.mark.parametrize('B', [1, 65, 257])
def test_valid_witnesses(ctx, B):
    W = ctx['W']['C']
    wits, keys = wits_of(W, B), keys_of(W, B)
    exp = (keys, W[4][:B], [0] * B)   # the workload's own key bytes and index
    assert RC.expect(wits[:16], ctx['rings']['C']) == tuple(x[:16] for x in exp)
    assert both(ctx, 'C', wits) == exp
    for name, e in ctx['engs'].items():
        assert recover_device(e, wits) == exp, name
    if B == 257:   # both parity paths are exercised: c = 0 (A + Bp) and c = 1 (A - Bp) each win often
        odd = sum(nonce_point_is_odd(m, s, k) for (m, s), k in zip(wits, keys))
        assert odd >= 32 and B - odd >= 32, odd
    if B == 65:    # the small rings: 8 witnesses over the 8 keys of A, 65 over the first 65 of B's 1 000
        for k in ('A', 'B'):
            Wk = ctx['W'][k]
            assert both(ctx, k, wits_of(Wk)) == (keys_of(Wk), Wk[4], [0] * len(Wk[4]))


def test_more_than_a_small_chunk(ctx):
    """4 096 + 3 valid witnesses in one call, against the workload's keys"""
    eng = ctx['engs']['nokt']   # (no per-key tables to build for the extra ring)
    Wb = eng.synth_workload(S + 9, 5000, 4099)
    rid = eng.add_ring(Wb[0])
    try:
        assert recover(eng, wits_of(Wb), ring_ids=[rid] * 4099) == (keys_of(Wb), Wb[4], [0] * 4099)
    finally:
        eng.drop_ring(rid)


def test_more_than_one_chunk(ctx):
    """16 384 + 5 witnesses in one call, host and device forms: the chunk loop's offsets, the staging area's reuse, and the per-chunk choice of the path
    (the last five run on cooperating waves: 4 chains per witness and pass, two passes)"""
    eng = ctx['engs']['nokt']
    eng.use_ring(ctx['ids']['nokt']['A'])
    wa, ka = wits_of(ctx['W']['A']), keys_of(ctx['W']['A'])
    B = 16384 + 5
    wits = [wa[(3 * i + i // 8) % 8] for i in range(B)]
    exp = ([ka[(3 * i + i // 8) % 8] for i in range(B)], [(3 * i + i // 8) % 8 for i in range(B)], [0] * B)
    assert RC.expect(wits[16380:16388], ctx['rings']['A']) == tuple(x[16380:16388] for x in exp)
    c0 = eng.test_counter(4)
    assert recover(eng, wits) == exp
    assert recover_device(eng, wits) == exp
    assert eng.test_counter(4) - c0 == (0 if os.environ.get('ZKATTEST_ONE_LANE_CHAINS') is not None else 2 * 2 * 4 * 5)


# ---------------------------------------------------------------- 2. edges
def test_edges_on_the_large_ring(ctx):
    E, ed = ctx['rings']['E'], ctx['edge']
    kc = keys_of(ctx['W']['C'], 8)
    wits = edge_list_large(ctx)
    exp = RC.expect(wits, E)
    # the last index; the lowest of two; a key that is gone; the non-signer's candidate at the lower index wins; tie -> c = 0; the identity's sibling, exactly
    assert exp[1] == [4999, 77, NONE, 0, 10, 11, 6, NONE, NONE]
    assert exp[2] == [0, 0, NOT_IN_RING, 0, 0, 0, 0, NOT_IN_RING, NOT_IN_RING]
    assert exp[0][:4] == [kc[1], kc[2], None, ed['other4']] and exp[0][5] == ed['ident_sib'] and exp[0][6:] == [kc[6], None, None]
    c0 = dict(RC.candidates(*ed['zero_z']))[0]
    assert exp[0][4] == be(c0[0]) + be(c0[1]) and c0[0] == ed['zero_z_x']
    ident = dict(RC.candidates(*ed['ident']))
    assert sorted(Q is None for Q in (ident[0], ident[1])) == [False, True]   # exactly one of the pair is the identity
    assert both(ctx, 'E', wits) == exp
    for name, e in ctx['engs'].items():
        assert recover_device(e, wits) == exp, name


def test_wrap_range_and_no_point(ctx):
    ed = ctx['edge']
    wits = edge_list_small(ctx)
    exp = RC.expect(wits, ctx['rings']['W'])
    assert exp == ([ed['wrap_pk'], None, None, None, None, None, keys_of(ctx['W']['A'], 8)[5]], [3, NONE, NONE, NONE, NONE, NONE, 5],
                   [0, NO_POINT | NOT_IN_RING, RANGE, RANGE, RANGE, RANGE, 0])
    assert {c for c, _ in RC.candidates(*ed['wrap'])} >= {2, 3}   # found only through the r + n pair
    assert RC.winner_c(*ed['wrap'], ctx['rings']['W']) in (2, 3)
    assert both(ctx, 'W', wits) == exp
    for name, e in ctx['engs'].items():
        assert recover_device(e, wits) == exp, name


# ---------------------------------------------------------------- 3. both paths
def test_cooperative_and_one_lane_paths_give_the_same_bytes():
    runs = [('default', {}), ('one lane', {'ZKATTEST_ONE_LANE_CHAINS': '1'})]
    env0 = {k: v for k, v in os.environ.items() if k != 'ZKATTEST_ONE_LANE_CHAINS'}
    recs = {}
    for tag, extra in runs:
        out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'recover_small_check.py')], env=dict(env0, **extra),
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert out.returncode == 0, (tag, out.stderr.decode()[-2000:])
        recs[tag] = json.loads(out.stdout.decode().strip().splitlines()[-1])
    d, o = recs['default'], recs['one lane']
    assert d['answers'] == o['answers'] and d['big'] == o['big'] == 'ok'
    assert d['coop'] == 2 * 4 * d['witnesses'] and o['coop'] == 0, (d['coop'], o['coop'], d['witnesses'])   # 4 per witness per pass, two passes, cooperative run only
    assert d['big_coop'] == o['big_coop'] == 0   # 4 096 + 3 witnesses in one chunk: the one-lane kernels
    flags = [f for ans in d['answers'] for f in ans[2]]
    assert d['witnesses'] == 65 + 9 + 7 and flags.count(0) >= 65 + 6 + 2 and RANGE in flags and NO_POINT | NOT_IN_RING in flags


# ---------------------------------------------------------------- 4. the chain: flags == 0 <=> the screen agrees <=> the proof verifies
def test_recover_screen_prove_verify(ctx):
    eng, rid = ctx['engs']['kt'], ctx['ids']['kt']['A']
    seeds = ctx['W']['B'][5]
    wa = wits_of(ctx['W']['A']) * 3   # 24 witnesses over the ring's 8 signers
    wits = list(wa)
    for i, b in enumerate(range(1, 24, 2)):   # 12 mutants
        m, s = wa[b]
        wits[b] = [(flip(m, 7 + i), s), (m, flip(s, 256 + 3 * i)), (m, flip(s, 5 * i)), (m, be(0) + s[32:])][i % 4]
    eng.use_ring(rid)
    pks, wo, fl = recover(eng, wits)
    assert (pks, wo, fl) == RC.expect(wits, ctx['rings']['A']) and sum(1 for f in fl if f) == 12
    msg, sig = b''.join(w[0] for w in wits), b''.join(w[1] for w in wits)
    pk = b''.join(p if p is not None else bytes(64) for p in pks)
    swo, sfl = eng.screen_batch(msg, sig, pk)
    for b in range(24):
        assert (fl[b] == 0) == ((swo[b], sfl[b]) == (wo[b], 0)), b
    proofs, st = eng.prove_batch(msg, sig, pk, [0 if w == NONE else w for w in wo], seeds=seeds[:32 * 24])
    made = [b for b in range(24) if proofs[b] is not None]
    ok, _ = eng.verify_batch(b''.join(wits[b][0] for b in made), [proofs[b] for b in made])
    verdict = [0] * 24
    for b, o in zip(made, ok):
        verdict[b] = o
    assert verdict == [1 if f == 0 else 0 for f in fl], (verdict, fl, st)


# ---------------------------------------------------------------- 5. rings
def test_mixed_rings_and_unknown_id(ctx):
    wits, names = [], []
    for i in range(60):
        k = 'ABC'[i % 3]
        ws = wits_of(ctx['W'][k])
        w = ws[(i // 3) % len(ws)]
        wits.append(w if i % 5 else (flip(w[0], i), w[1]))
        names.append(k)
    exp = [RC.model(m, s, ctx['rings'][k]) for (m, s), k in zip(wits, names)]
    exp = ([pk if f == 0 else None for pk, _, f in exp], [w for _, w, _ in exp], [f for _, _, f in exp])
    assert exp[2].count(0) == 48
    for name, e in ctx['engs'].items():
        ids = [ctx['ids'][name][k] for k in names]
        per_ring = ([None] * 60, [None] * 60, [None] * 60)
        for k in 'ABC':
            idx = [i for i in range(60) if names[i] == k]
            e.use_ring(ctx['ids'][name][k])
            res = recover(e, [wits[i] for i in idx])
            for j, i in enumerate(idx):
                for t in range(3):
                    per_ring[t][i] = res[t][j]
        assert per_ring == exp, name
        assert recover(e, wits, ring_ids=ids) == exp, name
        assert recover_device(e, wits, ring_ids=ids) == exp, name
        ids[7] = ids[20] = 999   # not resident: bit 16 alone
        unk = tuple(list(x) for x in exp)
        for b in (7, 20):
            unk[0][b], unk[1][b], unk[2][b] = None, NONE, NOT_RESIDENT
        assert recover(e, wits, ring_ids=ids) == unk, name
        assert recover_device(e, wits, ring_ids=ids) == unk, name


def test_recover_after_update_ring(ctx):
    wa, wb = wits_of(ctx['W']['A'], 8), wits_of(ctx['W']['B'], 8)
    ka, kb = keys_of(ctx['W']['A'], 8), keys_of(ctx['W']['B'], 8)
    for name, e in ctx['engs'].items():
        rid = e.add_ring(ctx['W']['A'][0])
        assert recover(e, [wa[2], wb[5]], ring_ids=[rid, rid]) == ([ka[2], None], [2, NONE], [0, NOT_IN_RING])
        e.update_ring(rid, {2: kb[5][:32]})
        ring = list(ctx['rings']['A'])
        ring[2] = int.from_bytes(kb[5][:32], 'big')
        exp = RC.expect([wa[2], wb[5]], ring)
        assert exp == ([None, kb[5]], [NONE, 2], [NOT_IN_RING, 0])
        assert recover(e, [wa[2], wb[5]], ring_ids=[rid, rid]) == exp, name
        e.drop_ring(rid)


# ---------------------------------------------------------------- 6. call-level statuses
def test_call_level_statuses(ctx):
    import zkp_ecdsa_amd as Z
    w = wits_of(ctx['W']['A'], 4)
    e = Z.Engine(0)
    try:
        for kw in ({}, {'ring_ids': [0] * 4}):
            with pytest.raises(Z.ZkError) as ei:   # before zk_ctx_set_params
                recover(e, w, **kw)
            assert ei.value.status == ZK_E_BUFFER
        e.set_params(*e.synth_params(S), 20)
        with pytest.raises(Z.ZkError) as ei:       # no active ring
            recover(e, w)
        assert ei.value.status == ZK_E_BUFFER
        assert recover(e, w, ring_ids=[5] * 4) == ([None] * 4, [NONE] * 4, [NOT_RESIDENT] * 4)   # the rings form needs none
        rid = e.add_ring(ctx['W']['A'][0])
        e.use_ring(rid)
        assert recover(e, []) == ([], [], []) and recover(e, [], ring_ids=[]) == ([], [], [])   # B = 0
        msg, sig = (b''.join(x[i] for x in w) for i in range(2))
        out = (C.c_uint32 * 4)()
        pk = (C.c_uint8 * 256)()
        L, h = e.L, e.h
        assert L.zk_recover_batch(h, 4, msg, sig, None, out, out) == ZK_E_ARG
        assert L.zk_recover_batch(h, 4, msg, sig, pk, None, out) == ZK_E_ARG
        assert L.zk_recover_batch(h, 4, msg, sig, pk, out, None) == ZK_E_ARG
        assert L.zk_recover_batch(h, 4, None, sig, pk, out, out) == ZK_E_ARG
        assert L.zk_recover_batch_rings(h, 4, msg, sig, None, pk, out, out) == ZK_E_ARG
        assert L.zk_recover_batch_device(h, 4, None, None, None, None, None) == ZK_E_ARG
        assert L.zk_recover_batch_rings_device(h, 4, None, None, None, None, None, None) == ZK_E_ARG
        _, m, s, p, which, seeds = ctx['W']['A']
        buf = Z.PinnedBuffer(e.proof_max_size() * 2)
        t = e.prove_submit(m[:64], s[:128], p[:128], which[:2], seeds[:64], buf)   # a streamed job is queued
        with pytest.raises(Z.ZkError) as ei:
            recover(e, w)
        assert ei.value.status == ZK_E_ARG
        with pytest.raises(Z.ZkError) as ei:
            recover(e, w, ring_ids=[rid] * 4)
        assert ei.value.status == ZK_E_ARG
        _, st = e.prove_wait(t)
        assert list(st) == [0, 0]
        assert recover(e, w) == (keys_of(ctx['W']['A'], 4), [0, 1, 2, 3], [0] * 4)
        buf.free()
    finally:
        e.close()


# ---------------------------------------------------------------- 7. the prover is not disturbed
def test_recover_between_prove_calls(ctx):
    eng = ctx['engs']['kt']
    eng.use_ring(ctx['ids']['kt']['A'])
    _, msg, sig, pk, which, seeds = ctx['W']['A']
    args = (msg[:32 * 6], sig[:64 * 6], pk[:64 * 6], which[:6])
    first = eng.prove_batch(*args, seeds=seeds[:32 * 6])
    assert recover(eng, wits_of(ctx['W']['A']) * 5) == (keys_of(ctx['W']['A']) * 5, which * 5, [0] * 40)
    assert recover(eng, wits_of(ctx['W']['B'], 9), ring_ids=[ctx['ids']['kt']['B']] * 9) == (keys_of(ctx['W']['B'], 9), list(range(9)), [0] * 9)
    assert eng.prove_batch(*args, seeds=seeds[:32 * 6]) == first and first[1] == [0] * 6


# ---------------------------------------------------------------- 8. the uniform build
def test_uniform_build_gives_the_same_answers():
    import zkp_ecdsa_amd as Z
    uni = os.path.join(os.path.dirname(Z.LIB_PATH), 'libzkattest_hip_uniform.so')
    if not os.path.exists(uni):
        pytest.skip('the uniform build is not there (make -C zkp-ecdsa_amd/csrc uniform)')
    recs = []
    for lib in (Z.LIB_PATH, uni):
        out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'recover_uniform_check.py')], env=dict(os.environ, ZKATTEST_LIB=lib),
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert out.returncode == 0, out.stderr.decode()[-2000:]
        recs.append(json.loads(out.stdout.decode().strip().splitlines()[-1]))
    a, b = recs
    assert b['lib'].endswith('_uniform.so') and (a['pk'], a['which'], a['flags']) == (b['pk'], b['which'], b['flags'])
    bad = {3: NOT_IN_RING, 5: NOT_IN_RING, 8: RANGE}
    assert a['flags'] == [bad.get(i, 0) for i in range(24)]
    assert all(a['pk'][i] == a['own'][i] and a['which'][i] == a['own_which'][i] for i in range(24) if i not in bad)
