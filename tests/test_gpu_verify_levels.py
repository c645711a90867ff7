"""-m gpu: per-proof verify levels (include/zkattest.h: zk_ctx_set_verify_level).  In ZK_VERIFY_LEVEL_PER_PROOF the engine verifies every proof
at its own header's secLevel, as the reference's verifySignatureList does (src/zkpAttestList.ts:147-184, src/exp/exp.ts:233-262) and as the
oracle does: engine (ok, status) == oracle (ok, status) with fixed verifier seeds, through every entry point, on batches that mix levels.  The
default mode keeps today's answers (a proof of another level than the context's: ZK_E_BAD_ENCODING)."""
import hashlib
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu

from zka1_mutants import mutants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, NKEYS = 4711, 8
LEVELS = (20, 33, 80, 96, 128)


def _vseeds(n, tag):
    return b''.join(hashlib.sha256(tag + i.to_bytes(4, 'big')).digest() for i in range(n))


_CACHE = {}


def _proofs(level, B=4, S_=S, nkeys=NKEYS):
    """B honest proofs made by the engine at `level` (cached per module)."""
    key = (level, B, S_, nkeys)
    if key not in _CACHE:
        import zkp_ecdsa_amd as Z
        eng = Z.Engine(0)
        nh, tg, th = eng.synth_params(S_)
        ring, msg, sig, pk, which, seeds = eng.synth_workload(S_, nkeys, B)
        eng.set_params(nh, tg, th, level)
        eng.set_ring(ring, nkeys)
        proofs, st = eng.prove_batch(msg, sig, pk, which, seeds=seeds)
        assert st == [0] * B, (level, st)
        eng.close()
        _CACHE[key] = (msg, proofs)
    return _CACHE[key]


def _engine(sec, per_proof=True):
    import coracle as CO
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    nh, tg, th = eng.synth_params(S)
    ring = eng.synth_workload(S, NKEYS, 4)[0]   # the ring _proofs proves over (its keys depend on B)
    eng.set_params(nh, tg, th, sec)
    eng.set_ring(ring, NKEYS)
    if per_proof:
        eng.set_verify_level(True)
    octx = CO.OracleCtx(nh, tg, th, sec)
    octx.set_ring(ring, NKEYS)
    return eng, octx


def _mixed(levels, per_level):
    """Interleaved batch: proof i is at levels[i % len(levels)], copies of each level's honest proofs."""
    made = {l: _proofs(l) for l in levels}
    msgs, plist = [], []
    for i in range(per_level * len(levels)):
        l = levels[i % len(levels)]
        m, p = made[l]
        k = (i // len(levels)) % len(p)
        msgs.append(m[32 * k:32 * k + 32])
        plist.append(p[k])
    return b''.join(msgs), plist


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
    off = _off(plist)
    dev = 'cuda:0'
    d_msg = torch.frombuffer(bytearray(msgs), dtype=torch.uint8).to(dev)
    d_pr = torch.frombuffer(bytearray(b''.join(plist)), dtype=torch.uint8).to(dev)
    d_off = torch.tensor(list(off), dtype=torch.int64).to(dev)
    d_vs = torch.frombuffer(bytearray(vs), dtype=torch.uint8).to(dev)
    d_ok = torch.zeros(B, dtype=torch.uint8, device=dev)
    d_st = torch.full((B,), -1, dtype=torch.int32, device=dev)
    eng.verify_batch_device(B, d_msg.data_ptr(), d_pr.data_ptr(), d_off.data_ptr(), d_vs.data_ptr(), d_ok.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    return d_ok.cpu().tolist(), d_st.cpu().tolist()


def _pinned(plist):
    import zkp_ecdsa_amd as Z
    raw = b''.join(plist)
    pin = Z.PinnedBuffer(max(len(raw), 64))
    pin.view[:len(raw)] = raw
    return pin


def _every_entry_point(eng, msgs, plist, vs):
    """{entry point: (ok, status)} for one batch."""
    import zkp_ecdsa_amd as Z
    B = len(plist)
    r = {'verify_batch': eng.verify_batch(msgs, plist, vseeds=vs)}
    pin = _pinned(plist)
    off = _off(plist)
    _, ok, st = eng.verify_batch_host_raw(msgs, pin, off, B, vseeds=vs)
    r['page_locked'] = (list(ok), list(st))
    r['device'] = _device(eng, msgs, plist, vs)
    t = eng.verify_submit(msgs, pin, off, B, vseeds=vs)
    ok, st = eng.verify_wait(t)
    r['submit_wait'] = (list(ok), list(st))
    pin.free()
    return r


@pytest.mark.parametrize('per_level', [4, 52])
def test_mixed_levels_through_every_entry_point_equal_the_oracle(per_level):
    """A context at 80 in per-proof mode: an interleaved batch at 20, 33, 80, 96 and 128 is accepted like the oracle accepts it, through
    zk_verify_batch (pageable and page-locked), zk_verify_batch_device and submit / wait.  per_level 52: 260 proofs, so that the level windows
    of 52 proofs run the small-call kernels; the 256-per-chunk batched check is covered by the homogeneous-window test below."""
    eng, octx = _engine(80)
    msgs, plist = _mixed(LEVELS, per_level)
    vs = _vseeds(len(plist), b'mix%d' % per_level)
    o = octx.verify_batch(msgs, plist, nthreads=16, vseeds=vs)
    assert o == ([1] * len(plist), [0] * len(plist))
    for name, g in _every_entry_point(eng, msgs, plist, vs).items():
        assert g == o, name
    eng.close()


def test_batched_check_inside_level_windows():
    """Two levels with 256 proofs each: every level window is a chunk that takes the chunk-wide batched Tom-256 check (>= 256 proofs),
    one forged proof per level is found, the rest passes -- as the oracle says."""
    eng, octx = _engine(80)
    msgs, plist = _mixed((33, 96), 256)
    plist = list(plist)
    for i in (17, 300):   # one proof of each level: a flipped response byte
        p = plist[i]
        plist[i] = p[:-9] + bytes([p[-9] ^ 1]) + p[-8:]
    vs = _vseeds(len(plist), b'big')
    before = eng.test_counter(2)
    g = eng.verify_batch(msgs, plist, vseeds=vs)
    assert eng.test_counter(2) > before, 'the batched check did not run'
    o = octx.verify_batch(msgs, plist, nthreads=16, vseeds=vs)
    assert g == o
    assert g[0].count(0) == 2 and g[0][17] == 0 and g[0][300] == 0
    eng.close()


def test_pool_of_one_device_verifies_mixed_levels():
    import coracle as CO
    import zkp_ecdsa_amd as Z
    pool = Z.Pool([0])
    e = Z.Engine(0)
    nh, tg, th = e.synth_params(S)
    ring = e.synth_workload(S, NKEYS, 4)[0]
    e.close()
    pool.set_params(nh, tg, th, 80)
    pool.set_ring(ring, NKEYS)
    pool.set_verify_level(True)
    msgs, plist = _mixed(LEVELS, 3)
    vs = _vseeds(len(plist), b'pool')
    octx = CO.OracleCtx(nh, tg, th, 80)
    octx.set_ring(ring, NKEYS)
    o = octx.verify_batch(msgs, plist, nthreads=16, vseeds=vs)
    assert pool.verify_batch(msgs, plist, vseeds=vs) == o == ([1] * 15, [0] * 15)
    pool.close()


def test_default_mode_keeps_refusing_other_levels():
    """Only the mode changes the answer: the same mixed batch in the default mode gives ZK_E_BAD_ENCODING to every proof that is not at 80."""
    eng, octx = _engine(80, per_proof=False)
    msgs, plist = _mixed(LEVELS, 2)
    vs = _vseeds(len(plist), b'def')
    want = ([1 if LEVELS[i % 5] == 80 else 0 for i in range(10)], [0 if LEVELS[i % 5] == 80 else 10 for i in range(10)])
    assert eng.verify_batch(msgs, plist, vseeds=vs) == want
    assert _device(eng, msgs, plist, vs) == want
    eng.set_verify_level(True)
    assert eng.verify_batch(msgs, plist, vseeds=vs) == ([1] * 10, [0] * 10)
    eng.set_verify_level(False)
    assert eng.verify_batch(msgs, plist, vseeds=vs) == want
    eng.close()


def _zero_rep_proof(p, n):
    """The 0-repetition proof of an honest one: header (sec 0, no challenge bits), R, comS1, keyXcom, keyYcom, then the GKProof."""
    gk_len = n * (4 * 72 + 96) + 32
    q = p[:8] + (0).to_bytes(4, 'big') + p[12:16] + bytes(16) + p[32:304] + p[len(p) - gk_len:]
    return q[:4] + len(q).to_bytes(4, 'big') + q[8:]


def test_context_at_seclevel_7():
    """A context set to 7 in per-proof mode verifies 80-repetition proofs; a 7-repetition proof whose membership holds gets 'security level
    not achieved' (9); one over another ring gets ok 0 / status 0; a hand-built 0-repetition proof gets 9; a default-mode context at 7 refuses."""
    import zkp_ecdsa_amd as Z
    eng, octx = _engine(7)
    m80, p80 = _proofs(80)
    m7, p7 = _proofs(7)
    m7o, p7o = _proofs(7, S_=S + 1)   # another ring (other synthetic keys)
    p0 = _zero_rep_proof(p80[0], 3)
    msgs = m80[:64] + m7[:64] + m7o[:32] + m80[:32]
    plist = [p80[0], p80[1], p7[0], p7[1], p7o[0], p0]
    vs = _vseeds(len(plist), b'seven')
    o = octx.verify_batch(msgs, plist, nthreads=8, vseeds=vs)
    assert o == ([1, 1, 0, 0, 0, 0], [0, 0, 9, 9, 0, 9]), o
    for name, g in _every_entry_point(eng, msgs, plist, vs).items():
        assert g == o, name
    # each kind alone (one level per call: the single-level path, below 20 the membership-only pipeline)
    for sel in ([0, 1], [2, 3, 4], [5]):
        ms = b''.join(msgs[32 * i:32 * i + 32] for i in sel)
        pl = [plist[i] for i in sel]
        v = b''.join(vs[32 * i:32 * i + 32] for i in sel)
        assert eng.verify_batch(ms, pl, vseeds=v) == ([o[0][i] for i in sel], [o[1][i] for i in sel])
        assert _device(eng, ms, pl, v) == ([o[0][i] for i in sel], [o[1][i] for i in sel])
    eng.set_verify_level(False)
    with pytest.raises(Z.ZkError):
        eng.verify_batch(msgs, plist, vseeds=vs)
    eng.close()


def _level_mutants(p, level, n, rnd_tag):
    """A few mutants of a proof at `level`: header secLevel and n, challenge bits above the level, a flipped point, a flipped scalar, truncation."""
    put = lambda b, pos, d: b[:pos] + d + b[pos + len(d):]
    out = [('honest', p)]
    for v in (level - 1, level + 1, 0, 129, 200):
        out.append(('hdr-sec=%d' % v, put(p, 8, v.to_bytes(4, 'big'))))
    for v in (n - 1, n + 1, 64):
        out.append(('hdr-n=%d' % v, put(p, 12, v.to_bytes(4, 'big'))))
    if level < 128:
        bits = int.from_bytes(p[16:32], 'big') | (1 << level)
        out.append(('bit-above', put(p, 16, bits.to_bytes(16, 'big'))))
    out.append(('R-x', put(p, 40, bytes([p[40] ^ 4]))))
    out.append(('keyXcom', put(p, 200, bytes([p[200] ^ 1]))))
    out.append(('last-scalar', p[:-9] + bytes([p[-9] ^ 1]) + p[-8:]))
    out.append(('first-rep-A', put(p, 310, bytes([p[310] ^ 2]))))
    cut = p[:-4]
    out.append(('short', cut[:4] + len(cut).to_bytes(4, 'big') + cut[8:]))
    return out


@pytest.mark.parametrize('packed', [False, True])
def test_mutant_sweep_over_a_mixed_batch(packed):
    """zka1_mutants at 80 (header sec / n mutants included: they announce other levels) next to hand-made mutants at 20, 33 and 128, in one
    batch, both wire layouts: engine == oracle for every proof."""
    import zkp_ecdsa_amd as Z
    eng, octx = _engine(80)
    m80, p80 = _proofs(80)
    items = [(n, j, b) for (n, j, b) in mutants(p80[:2], 3, S, S)[:160]]
    for lvl in (20, 33, 128):
        m, p = _proofs(lvl)
        for name, b in _level_mutants(p[0], lvl, 3, lvl):
            items.append(('%d/%s' % (lvl, name), ('lv', lvl), b))
    names = [it[0] for it in items]
    msgs = b''.join(m80[32 * it[1]:32 * it[1] + 32] if not isinstance(it[1], tuple) else _proofs(it[1][1])[0][:32] for it in items)
    plist = [it[2] for it in items]
    assert all(len(p) % 4 == 0 for p in plist)
    if packed:   # the mutants the packed layout can carry as they are (a ZKA1 padding byte, for one, has no packed form)
        keep = [i for i, p in enumerate(plist) if _pack(p) is not None]
        names, plist = [names[i] for i in keep], [plist[i] for i in keep]
        msgs = b''.join(msgs[32 * i:32 * i + 32] for i in keep)
    vs = _vseeds(len(plist), b'mut')
    o = octx.verify_batch(msgs, plist, nthreads=16, vseeds=vs)
    if packed:
        eng.set_wire(True)
        plist = [_pack(p) for p in plist]
    g = eng.verify_batch(msgs, plist, vseeds=vs)
    bad = [(names[i], (g[0][i], g[1][i]), (o[0][i], o[1][i])) for i in range(len(plist)) if (g[0][i], g[1][i]) != (o[0][i], o[1][i])]
    assert not bad, bad[:12]
    assert _device(eng, msgs, plist, vs) == g
    assert {(1, 0), (0, 0), (0, 10)} <= set(zip(*g))
    eng.close()


def _pack(p):
    """ZKA1 -> ZKA1P, or None where the proof does not survive the round trip ZKA1 -> ZKA1P -> ZKA1 byte for byte."""
    import zkp_ecdsa_amd as Z
    try:
        q = Z.pack_proof(p)
        return q if Z.unpack_proof(q) == p else None
    except Z.ZkError:
        return None


def test_single_level_batch_is_bit_identical_in_both_modes():
    """A batch at the context's own level, honest and tampered (the cases of tests/test_gpu_verify.py): the same ok and status in both modes."""
    eng, octx = _engine(80, per_proof=False)
    m, p = _proofs(80)
    msgs = m + m
    plist = list(p) + list(p)
    plist[4] = p[0][:-9] + bytes([p[0][-9] ^ 1]) + p[0][-8:]                  # a response scalar
    plist[5] = p[1][:48] + bytes([p[1][48] ^ 1]) + p[1][49:]                  # R
    plist[6] = p[2][:16] + bytes([p[2][16] ^ 0x80]) + p[2][17:]               # a challenge bit
    plist[7] = p[3][:-4]                                                      # truncated
    msgs = msgs[:32 * 3] + bytes(32) + msgs[32 * 4:]                          # another message for proof 3
    vs = _vseeds(len(plist), b'same')
    a = eng.verify_batch(msgs, plist, vseeds=vs)
    ad = _device(eng, msgs, plist, vs)
    eng.set_verify_level(True)
    b = eng.verify_batch(msgs, plist, vseeds=vs)
    bd = _device(eng, msgs, plist, vs)
    assert a == b == ad == bd == octx.verify_batch(msgs, plist, nthreads=8, vseeds=vs)
    assert a[0] == [1, 1, 1, 0, 0, 0, 0, 0]
    eng.close()


def test_timing_shows_the_partition_only_on_a_mixed_batch():
    import zkp_ecdsa_amd as Z
    eng, _ = _engine(80)
    eng.set_timing(1)
    msgs, plist = _mixed((33, 80), 4)
    vs = _vseeds(len(plist), b't')
    assert eng.verify_batch(msgs, plist, vseeds=vs) == ([1] * 8, [0] * 8)
    _, fam = eng.last_timing()
    assert 'v_levels' in fam and 'v_hash' in fam, fam
    m, p = _proofs(96)
    assert eng.verify_batch(m, p, vseeds=_vseeds(4, b'u')) == ([1] * 4, [0] * 4)
    _, fam = eng.last_timing()
    assert 'v_levels' not in fam and 'v_hash' in fam, fam
    eng.close()


def test_hardened_mode_mixed_levels_match_the_restatement():
    """Proofs made in hardened mode at 20 and 33, verified together by a hardened context at 80 in per-proof mode, against the Python
    restatement's verifySignatureList(..., hardened=True) the way tests/test_hardened.py checks it; another message fails in both."""
    import zkattest_ref as R
    import zkp_ecdsa_amd as Z
    e = Z.Engine(0)
    nh, th = Z.hardened_h(b'levels')
    _, tg, _ = e.synth_params(S)
    ring, msg, sig, pk, which, seeds = e.synth_workload(S, NKEYS, 2)
    e.set_mode(Z.MODE_HARDENED)
    e.set_ring(ring, NKEYS)
    made = {}
    for lvl in (20, 33):
        e.set_params(nh, tg, th, lvl)
        e.set_ring(ring, NKEYS)
        made[lvl], st = e.prove_batch(msg, sig, pk, which, seeds=seeds)
        assert st == [0, 0]
    e.set_params(nh, tg, th, 80)
    e.set_ring(ring, NKEYS)
    e.set_verify_level(True)
    other = hashlib.sha256(b'other').digest()
    msgs = msg[:32] + msg[32:64] + msg[:32] + other
    plist = [made[20][0], made[33][1], made[33][0], made[20][1]]
    keys = [int.from_bytes(ring[32 * i:32 * i + 32], 'big') for i in range(NKEYS)]
    g = R.tomEdwards256.generator()
    want = []
    for b, p in enumerate(plist):
        lvl = int.from_bytes(p[8:12], 'big')
        params = R.SystemParametersList(
            R.PedersenParams(R.p256, R.p256.generator(), R.WeierstrassPoint(R.p256, int.from_bytes(nh[:32], 'big'), int.from_bytes(nh[32:], 'big'), 1)),
            R.PedersenParams(R.tomEdwards256, g, R.TEdwardsPoint(R.tomEdwards256, int.from_bytes(th[:36], 'big'), int.from_bytes(th[36:], 'big'))), lvl)
        want.append(1 if R.verifySignatureList(params, msgs[32 * b:32 * b + 32], keys, R.proof_from_bytes(p), hardened=True) else 0)
    assert want == [1, 1, 1, 0]
    vs = _vseeds(4, b'hard')
    assert e.verify_batch(msgs, plist, vseeds=vs) == (want, [0] * 4)
    assert _device(e, msgs, plist, vs) == (want, [0] * 4)
    e.set_mode(Z.MODE_REFERENCE)   # the statement is not hashed: membership fails for every hardened proof
    assert e.verify_batch(msgs, plist, vseeds=vs) == ([0] * 4, [0] * 4)
    e.close()


def test_setter_rules():
    import zkp_ecdsa_amd as Z
    eng, _ = _engine(80, per_proof=False)
    assert eng.L.zk_ctx_set_verify_level(eng.h, 2) == 14
    m, p = _proofs(80)
    pin = _pinned(p)
    t = eng.verify_submit(m, pin, _off(p), 4, vseeds=_vseeds(4, b's'))
    assert eng.L.zk_ctx_set_verify_level(eng.h, 1) == 14   # streamed jobs queued
    assert [list(x) for x in eng.verify_wait(t)] == [[1] * 4, [0] * 4]
    assert eng.L.zk_ctx_set_verify_level(eng.h, 1) == 0
    pin.free()
    eng.close()


def test_facade_set_verify_level(tmp_path):
    """bindings/napi: setVerifyLevel('proof') makes verifySignatureList return true for a proof made under generateParamsList(128) when it is
    called with params at 80 over the same groups (the reference returns true for that call); 'context' keeps 'error deserializing'.
    Skipped as tests/test_napi_binding.py skips."""
    napi = os.path.join(ROOT, 'bindings', 'napi')
    if not (shutil.which('node') and shutil.which('gcc') and os.path.exists('/usr/include/node/node_api.h')):
        pytest.skip('node / gcc / node_api.h not available')
    out = str(tmp_path / 'zkattest.node')
    subprocess.check_call(['make', '-s', '-C', napi, 'OUT=' + out])
    env = dict(os.environ, ZKATTEST_NODE=out)
    r = subprocess.run(['node', 'verify_level_check.js'], cwd=napi, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'context: false' in r.stdout and 'proof: true' in r.stdout, r.stdout
