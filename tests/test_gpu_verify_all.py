"""-m gpu: the exhaustive verify mode (include/zkattest.h: zk_ctx_set_verify_reps).  ZK_VERIFY_REPS_ALL checks every repetition of a proof in
ceil(sec / 20) passes over the sampled verifier's pipeline; its answers are those of the model in tests/verify_all_common.py -- the Python
restatement's verifySignatureList with secparam = the proof's repetition count and the repetitions walked in ascending order -- through every
blocking entry point, both wire layouts, per-proof levels, the batched passes and the pool.  The default mode keeps the sampled verifier's answers."""
import hashlib

import pytest

pytestmark = pytest.mark.gpu

import verify_all_common as VA
from zka1_mutants import P256_N, TOM_Q, PADD, REP_HEAD, Layout, _flip, _put, _set_len

S, NKEYS, N = 5150, 8, 3
E_T_INF, E_T1_INF, E_PARAMS, E_SECLEVEL, E_BAD, E_ARG = 3, 4, 8, 9, 10, 14


def _vseeds(n, tag):
    return b''.join(hashlib.sha256(tag + i.to_bytes(4, 'big')).digest() for i in range(n))


_CACHE = {}


def _world():
    """parameters and the ring every test verifies over (the keys of a synthetic workload of 4 signers)"""
    if 'world' not in _CACHE:
        import zkp_ecdsa_amd as Z
        e = Z.Engine(0)
        nh, tg, th = e.synth_params(S)
        ring = e.synth_workload(S, NKEYS, 4)[0]
        e.close()
        _CACHE['world'] = (nh, tg, th, ring, [int.from_bytes(ring[32 * i:32 * i + 32], 'big') for i in range(NKEYS)])
    return _CACHE['world']


def _proofs(level):
    """(message hashes, 4 honest engine-made proofs) at `level`, made once per module and never changed"""
    if level not in _CACHE:
        import zkp_ecdsa_amd as Z
        nh, tg, th, _, _ = _world()
        eng = Z.Engine(0)
        ring, msg, sig, pk, which, seeds = eng.synth_workload(S, NKEYS, 4)
        eng.set_params(nh, tg, th, level)
        eng.set_ring(ring, NKEYS)
        proofs, st = eng.prove_batch(msg, sig, pk, which, seeds=seeds)
        assert st == [0] * 4, (level, st)
        eng.close()
        _CACHE[level] = (msg, proofs)
    return _CACHE[level]


def _engine(sec, reps_all=True, per_proof=False):
    import zkp_ecdsa_amd as Z
    nh, tg, th, ring, _ = _world()
    eng = Z.Engine(0)
    eng.set_params(nh, tg, th, sec)
    eng.set_ring(ring, NKEYS)
    eng.set_verify_level(per_proof)
    eng.set_verify_reps(reps_all)
    return eng


def _oracle(sec):
    import coracle as CO
    nh, tg, th, ring, _ = _world()
    octx = CO.OracleCtx(nh, tg, th, sec)
    octx.set_ring(ring, NKEYS)
    return octx


def _model(sec, msgs, plist, vs):
    nh, tg, th, _, keys = _world()
    r = [VA.model(VA.params_of(nh, tg, th, sec), keys, msgs[32 * i:32 * i + 32], p, vs[32 * i:32 * i + 32]) for i, p in enumerate(plist)]
    return [a for a, _ in r], [b for _, b in r]


def _break(p, sec, i, tom=False):
    """beta1 (a one-bit repetition) or z2 (a zero-bit one) of repetition i incremented: the repetition's P-256 relation fails, nothing else changes.
    tom: beta2 or r1 instead, the blinder of a Tom-256 commitment -- a Tom-256 relation fails."""
    return VA.bump_scalar(p, Layout(p, N, sec).rep_scalars(i)[2 if tom else 1], TOM_Q if tom else P256_N)


def _flip_header_bit(p, sec, i):
    """Header challenge bit i flipped with the layout kept consistent -- a PointAdd proof taken out of repetition i, or a copy of another repetition's put in --
    so that everything deserialises and the recomputed challenge, which hashes A, Tx and Ty only, disagrees with the header at repetition i alone."""
    lay = Layout(p, N, sec)
    at = lay.rep[i] + REP_HEAD
    if i in lay.zero_reps:
        q = p[:at] + p[at + PADD:]
    else:
        z = lay.rep[lay.zero_reps[0]] + REP_HEAD
        q = p[:at] + p[z:z + PADD] + p[at:]
    return _set_len(_put(q, 16, (lay.bits ^ (1 << i)).to_bytes(16, 'big')))


def _identity_at(p, sec, i, msg32, j):
    """-> (proof, status): repetition i's point made the identity.  A one-bit repetition: alpha = 0, 'T is at infinity'.  A zero-bit one: z = -z1 / k makes
    z R + Q the identity, 'T1 is at infinity' (R = +-k G with the synthetic signer's nonce k, Q = z1 G), as tests/zka1_mutants.py plants it."""
    import coracle as CO
    import zkattest_ref as R
    lay = Layout(p, N, sec)
    if i in lay.one_reps:
        return _put(p, lay.rep[i] + 208, bytes(32)), E_T_INF
    k = R.fromBytes(R.synth_tag(b'nonce', S, j)) % (P256_N - 1) + 1
    sign = 1 if CO.p256_mul(k)[32:] == p[64:96] else -1
    r = int.from_bytes(p[32:64], 'big') % P256_N
    z1 = pow(r, -1, P256_N) * (int.from_bytes(msg32, 'big') % P256_N) % P256_N
    zbad = (-sign * z1 * pow(k, -1, P256_N)) % P256_N
    return _put(p, lay.rep[i] + 208, zbad.to_bytes(32, 'big')), E_T1_INF


def _off(plist):
    import ctypes as C
    off = (C.c_uint64 * (len(plist) + 1))()
    o = 0
    for b, p in enumerate(plist):
        off[b] = o
        o += len(p)
    off[len(plist)] = o
    return off


def _device(eng, msgs, plist, vs):
    import torch
    B = len(plist)
    dev = 'cuda:0'
    d_msg = torch.frombuffer(bytearray(msgs), dtype=torch.uint8).to(dev)
    d_pr = torch.frombuffer(bytearray(b''.join(plist)), dtype=torch.uint8).to(dev)
    d_off = torch.tensor(list(_off(plist)), dtype=torch.int64).to(dev)
    d_vs = torch.frombuffer(bytearray(vs), dtype=torch.uint8).to(dev)
    d_ok = torch.zeros(B, dtype=torch.uint8, device=dev)
    d_st = torch.full((B,), -1, dtype=torch.int32, device=dev)
    eng.verify_batch_device(B, d_msg.data_ptr(), d_pr.data_ptr(), d_off.data_ptr(), d_vs.data_ptr(), d_ok.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    return d_ok.cpu().tolist(), d_st.cpu().tolist()


@pytest.mark.parametrize('r,seed', VA.MISSED, ids=['rep%d' % r for r, _ in VA.MISSED])
def test_a_broken_repetition_the_sample_misses(r, seed):
    """One repetition out of 80 broken, under a committed verifier seed whose 20 sampled repetitions do not hold it (tests/test_verify_all_host.py): the sampled
    verifier accepts, as the oracle does, and the exhaustive one rejects -- with the broken repetition in each of the four passes."""
    msg, p = _proofs(80)
    broken = [_break(p[0], 80, r)]
    assert r not in VA.sampled_indices(seed, N, 80)
    eng = _engine(80, reps_all=False)
    assert eng.verify_batch(msg[:32], broken, vseeds=seed) == ([1], [0]) == _oracle(80).verify_batch(msg[:32], broken, vseeds=seed)
    eng.set_verify_reps(True)
    assert eng.verify_batch(msg[:32], broken, vseeds=seed) == ([0], [0])
    assert eng.verify_batch(msg[:32], [p[0]], vseeds=seed) == ([1], [0])
    eng.close()


@pytest.mark.parametrize('sec,passes', [(20, 1), (21, 2), (40, 2), (41, 3), (80, 4)])
def test_valid_proofs_stay_valid(sec, passes):
    """Batches of 1, 3 and 300 honest proofs (300: the batched bucket pass at the default min_chunk) at levels on both sides of a multiple of 20, and the passes
    each call runs (zk_test_counter 12)."""
    msg, p = _proofs(sec)
    eng = _engine(sec)
    for B in (1, 3, 300):
        msgs = b''.join(msg[32 * (i % 4):32 * (i % 4) + 32] for i in range(B))
        c12, c2 = eng.test_counter(12), eng.test_counter(2)
        assert eng.verify_batch(msgs, [p[i % 4] for i in range(B)], vseeds=_vseeds(B, b'valid')) == ([1] * B, [0] * B), (sec, B)
        assert eng.test_counter(12) - c12 == passes, (sec, B)
        assert (eng.test_counter(2) > c2) == (B == 300)
    eng.close()


def _model_batch(sec):
    """12 proofs at `sec`: honest ones, one repetition broken at the edges of the passes, header bits that disagree with the challenge, a structural and a
    membership mutant, an exception behind a broken repetition, another message."""
    msg, p = _proofs(sec)
    lay = Layout(p[2], N, sec)
    items = [(0, p[0]), (1, p[1]),
             (0, _break(p[0], sec, 0)), (1, _break(p[1], sec, 19)), (2, _break(p[2], sec, 20)), (3, _break(p[3], sec, sec - 1)),
             (0, _flip_header_bit(_flip_header_bit(p[0], sec, 5), sec, sec - 1)), (1, _flip_header_bit(p[1], sec, sec - 1)),
             (2, _flip(p[2], 40, 4)),                            # R.x: off the curve
             (2, _flip(p[2], lay.gk_scalars()[0] + 31, 1)),      # a response of the membership proof
             (3, _flip_header_bit(_break(p[3], sec, 20), sec, sec - 1)),
             (0, p[3])]
    return b''.join(msg[32 * j:32 * j + 32] for j, _ in items), [b for _, b in items]


@pytest.mark.parametrize('sec', [21, 41])
def test_engine_equals_model_through_every_blocking_entry_point(sec):
    import zkp_ecdsa_amd as Z
    msgs, plist = _model_batch(sec)
    B = len(plist)
    vs = _vseeds(B, b'model%d' % sec)
    want = _model(sec, msgs, plist, vs)
    assert want == ([1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, E_PARAMS, E_PARAMS, E_BAD, 0, E_PARAMS, 0]), want
    eng = _engine(sec)
    assert eng.verify_batch(msgs, plist, vseeds=vs) == want
    assert _device(eng, msgs, plist, vs) == want
    _, _, _, ring, _ = _world()
    ids = [eng.add_ring(ring, NKEYS), eng.add_ring(ring, NKEYS)]
    assert eng.verify_batch_rings(msgs, plist, [ids[i % 2] for i in range(B)], vseeds=vs) == want
    # ZKA1P: the proofs the packed layout carries as they are
    keep = []
    for i, q in enumerate(plist):
        try:
            if Z.unpack_proof(Z.pack_proof(q)) == q:
                keep.append(i)
        except Z.ZkError:
            pass
    assert len(keep) >= 10, keep
    eng.set_wire(True)
    sel = lambda a, w: b''.join(a[w * i:w * i + w] for i in keep)
    packed = [Z.pack_proof(plist[i]) for i in keep]
    got = eng.verify_batch(sel(msgs, 32), packed, vseeds=sel(vs, 32))
    assert got == ([want[0][i] for i in keep], [want[1][i] for i in keep])
    assert _device(eng, sel(msgs, 32), packed, sel(vs, 32)) == got
    eng.close()


def test_the_lowest_repetition_that_throws_gives_the_status():
    """secLevel 41, passes over 0..19, 20..39 and 21..40: an identity at repetition 25 with a header bit that disagrees at 40, and the two swapped."""
    sec = 41
    msg, p = _proofs(sec)
    a, st_a = _identity_at(p[1], sec, 25, msg[32:64], 1)
    a = _flip_header_bit(a, sec, 40)
    b, st_b = _identity_at(p[1], sec, 40, msg[32:64], 1)
    b = _flip_header_bit(b, sec, 25)
    msgs, plist, vs = msg[32:64] * 2, [a, b], _vseeds(2, b'order')
    want = ([0, 0], [st_a, E_PARAMS])
    assert st_a in (E_T_INF, E_T1_INF) and st_b in (E_T_INF, E_T1_INF)
    assert _model(sec, msgs, plist, vs) == want
    eng = _engine(sec)
    assert eng.verify_batch(msgs, plist, vseeds=vs) == want
    assert _device(eng, msgs, plist, vs) == want
    # ... and the identity alone, in the last pass only
    c, st_c = _identity_at(p[1], sec, 40, msg[32:64], 1)
    assert eng.verify_batch(msg[32:64], [c], vseeds=vs[:32]) == ([0], [st_c]) == _model(sec, msg[32:64], [c], vs[:32])
    eng.close()


def test_per_proof_levels_run_their_own_passes():
    m7, p7 = _proofs(7)
    m21, p21 = _proofs(21)
    m80, p80 = _proofs(80)
    eng = _engine(80, per_proof=True)
    plist = [p7[0], p21[0], p80[0], _break(p80[1], 80, 60), p21[1], p7[1]]
    msgs = m7[:32] + m21[:32] + m80[:32] + m80[32:64] + m21[32:64] + m7[32:64]
    vs = _vseeds(6, b'levels')
    c12 = eng.test_counter(12)
    want = ([0, 1, 1, 0, 1, 0], [E_SECLEVEL, 0, 0, 0, 0, E_SECLEVEL])
    assert eng.verify_batch(msgs, plist, vseeds=vs) == want
    assert eng.test_counter(12) - c12 == 1 + 2 + 4
    assert _device(eng, msgs, plist, vs) == want
    eng.close()


def test_batched_passes_and_their_fallback(monkeypatch):
    """41 proofs at secLevel 41 in chunks of 16 with both cross-proof passes on (the means of tests/test_gpu_mutants_batched.py): two broken proofs among 39
    honest ones are the only ones rejected, and the group of the one whose Tom-256 relation fails went through the per-proof sums."""
    sec = 41
    msg, p = _proofs(sec)
    monkeypatch.setenv('ZKATTEST_P256_BATCH', '1')      # read in zk_ctx_create
    eng = _engine(sec)
    monkeypatch.delenv('ZKATTEST_P256_BATCH')
    eng.set_timing(1)
    eng.set_batch_verify(1), eng.set_chunk(16), eng.set_lanes(2)
    B, bad = 41, 22
    plist = [p[i % 4] for i in range(B)]
    plist[bad] = _break(plist[bad], sec, 40, tom=True)   # seen by the last pass only; a Tom-256 relation: its group fails the bucket pass
    plist[3] = _break(plist[3], sec, 2)                  # ... and a P-256 relation, seen by the first
    msgs = b''.join(msg[32 * (i % 4):32 * (i % 4) + 32] for i in range(B))
    c0, c2, c3, c12 = (eng.test_counter(k) for k in (0, 2, 3, 12))
    ok, st = eng.verify_batch(msgs, plist, vseeds=_vseeds(B, b'batched'))
    assert st == [0] * B and ok == [0 if i in (3, bad) else 1 for i in range(B)]
    assert eng.test_counter(0) > c0, 'the per-proof fallback did not run'
    assert eng.test_counter(2) > c2 and eng.test_counter(3) > c3, 'the cross-proof passes did not run'
    assert eng.test_counter(12) - c12 == 3
    fam = eng.last_timing()[1]
    assert 'v_merge' in fam and 'v_msm_tom' in fam and 'v_msm_p256' in fam, fam
    eng.close()


def test_rules():
    import zkp_ecdsa_amd as Z
    msg, p = _proofs(80)
    r, seed = VA.MISSED[2]
    plist = [p[0], _break(p[1], 80, r), p[2][:48] + bytes([p[2][48] ^ 1]) + p[2][49:], p[3][:-4]]
    vs = seed * 4
    eng = _engine(80)
    pin = Z.PinnedBuffer(len(b''.join(p)))
    pin.view[:len(b''.join(p))] = b''.join(p)
    with pytest.raises(Z.ZkError) as e:                      # no streamed variant
        eng.verify_submit(msg, pin, _off(p), 4, vseeds=vs)
    assert e.value.status == E_ARG
    all_ = eng.verify_batch(msg, plist, vseeds=vs)
    assert all_ == ([1, 0, 0, 0], [0, 0, E_BAD, E_BAD])
    eng.set_verify_reps(False)                               # back to the sampled verifier: the oracle's answers
    assert eng.verify_batch(msg, plist, vseeds=vs) == _oracle(80).verify_batch(msg, plist, vseeds=vs) == ([1, 1, 0, 0], [0, 0, E_BAD, E_BAD])
    t = eng.verify_submit(msg, pin, _off(p), 4, vseeds=vs)
    assert eng.L.zk_ctx_set_verify_reps(eng.h, 1) == E_ARG   # streamed jobs queued
    assert [list(x) for x in eng.verify_wait(t)] == [[1] * 4, [0] * 4]
    assert eng.L.zk_ctx_set_verify_reps(eng.h, 1) == 0
    pin.free()
    eng.close()


def test_pool_of_two_contexts():
    import zkp_ecdsa_amd as Z
    nh, tg, th, ring, _ = _world()
    msg, p = _proofs(80)
    r, seed = VA.MISSED[3]
    plist = [p[0], _break(p[1], 80, r), p[2], _break(p[3], 80, r)]
    pool = Z.Pool([0, 0])
    pool.set_params(nh, tg, th, 80)
    pool.set_ring(ring, NKEYS)
    assert pool.verify_batch(msg, plist, vseeds=seed * 4) == ([1] * 4, [0] * 4)
    pool.set_verify_reps(True)
    assert pool.verify_batch(msg, plist, vseeds=seed * 4) == ([1, 0, 1, 0], [0] * 4)
    assert pool.L.zk_pool_set_verify_reps(pool.h, 2) == E_ARG
    pool.close()
