"""gpu: ring membership of a committed value on its own (include/zkattest.h: zk_member_*; "ZKM1" proofs) against the Python restatement of the reference's
commit / proveMembership / verifyMembership (oracle/zkattest_ref.py) with the contract's RNG per proof: byte parity of proofs, commitments and blinders on
both paths of the ring fold (a ring of 5 values: plain fold; a ring of 300: table E and padding), with engine-drawn and caller blinders, host and device
pointers, one-proof calls, rejected fills, every chunk / lane / fold / build setting; the verifier against mutants of every field; the ring lifecycle; wiping."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import member_common as M

pytestmark = pytest.mark.gpu
ZK_E_BAD_ENCODING, ZK_E_RNG_EXHAUSTED, ZK_E_ARG = 10, 11, 14
FIXED300 = [0, 1, 127, 128, 255, 256, 298, 299]   # first / last of a chunk of 128, of a 256-key block of table E, the last keys; 298, 299 are ring entries, 300.. padding


@pytest.fixture(scope='module')
def env():
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    nh, tg, th = eng.synth_params(M.PARAM_SEED)
    eng.set_params(nh, tg, th, 80)
    e = {'Z': Z, 'eng': eng, 'params': M.oracle_params(tg, th)}
    e['r5'] = eng.add_ring(M.ring_bytes(M.RING5), 5)
    e['r300'] = eng.add_ring(M.ring_bytes(M.RING300), 300)
    yield e
    eng.close()


@pytest.fixture(scope='module')
def ring5_ref(env):
    """the oracle's proofs for which = 0..7 of the 5-value ring, engine-drawn blinders (commit then proveMembership on one SeedRng): computed once"""
    seeds = M.seeds_for(b'r5', 9)
    return seeds, [M.oracle_prove(env['params'], M.RING5, w, M.R.SeedRng(seeds[32 * w:32 * w + 32])) for w in range(8)]


@pytest.fixture(scope='module')
def ring300_run(env):
    """the engine's 300 proofs of the 300-value ring at chunk 128 (three chunks on two lanes), shared by the tests that compare against them"""
    eng = env['eng']
    eng.use_ring(env['r300'])
    eng.set_chunk(128)
    seeds = M.seeds_for(b'r300', 300)
    out = eng.member_prove_batch(list(range(300)), seeds=seeds)
    eng.set_chunk(4096)
    assert out[3] == [0] * 300
    return seeds, out


def test_size_follows_the_active_ring(env):
    eng = env['eng']
    eng.use_ring(env['r5'])
    assert eng.member_proof_size() == M.proof_size(3) == 1200
    eng.use_ring(env['r300'])
    assert eng.member_proof_size() == M.proof_size(9) == 3504


def test_ring5_engine_drawn_blinders_match_the_oracle(env, ring5_ref):
    eng = env['eng']
    eng.use_ring(env['r5'])
    seeds, ref = ring5_ref
    which = list(range(8)) + [8]   # 5..7: padding indices; 8: outside the padded ring
    proofs, coms, blinders, st = eng.member_prove_batch(which, seeds=seeds)
    assert st == [0] * 8 + [ZK_E_ARG]
    for w in range(8):
        assert (proofs[w], coms[w], blinders[w]) == ref[w], w
        assert M.oracle_verify(env['params'], M.RING5, coms[w], proofs[w]), w
    assert proofs[8] is None and eng.member_last_raw[8 * 1200:] == bytes(1200)   # a zeroed slot; its neighbours are the oracle's bytes (above)
    ok, vst = eng.member_verify_batch(coms[:8], proofs[:8])
    assert ok == [1] * 8 and vst == [0] * 8


def test_ring5_caller_blinders_match_the_oracle_host_and_device(env):
    import torch
    eng = env['eng']
    eng.use_ring(env['r5'])
    seeds = M.seeds_for(b'r5b', 8)
    bl = [int.from_bytes(M.tag(b'blind', w), 'big') % M.Q for w in range(8)]
    bl[3] = M.Q + 12345   # >= q: reduced as newScalar does (q + 12345 < 2^256)
    assert bl[3] < 2 ** 256
    blb = b''.join(b.to_bytes(32, 'big') for b in bl)
    ref = [M.oracle_prove(env['params'], M.RING5, w, M.R.SeedRng(seeds[32 * w:32 * w + 32]), blinder=bl[w]) for w in range(8)]
    proofs, coms, blinders, st = eng.member_prove_batch(list(range(8)), blinders=blb, seeds=seeds)
    assert st == [0] * 8
    for w in range(8):
        assert (proofs[w], coms[w], blinders[w]) == ref[w], w
    # the device-pointer forms: same bytes, same verdicts
    dev = torch.device('cuda:0')

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d_w = torch.arange(8, dtype=torch.int32, device=dev)
    d_bl, d_seeds = up(blb), up(seeds)
    d_com, d_bo = torch.zeros(8 * 72, dtype=torch.uint8, device=dev), torch.zeros(8 * 32, dtype=torch.uint8, device=dev)
    d_out, d_st = torch.full((8 * 1200,), 7, dtype=torch.uint8, device=dev), torch.full((8,), 7, dtype=torch.int32, device=dev)
    eng.member_prove_batch_device(8, d_w.data_ptr(), d_bl.data_ptr(), d_seeds.data_ptr(), d_com.data_ptr(), d_bo.data_ptr(), d_out.data_ptr(), 8 * 1200, d_st.data_ptr())
    torch.cuda.synchronize()
    assert bytes(d_out.cpu().numpy()) == b''.join(proofs) and bytes(d_com.cpu().numpy()) == b''.join(coms)
    assert bytes(d_bo.cpu().numpy()) == b''.join(blinders) and d_st.cpu().tolist() == [0] * 8
    d_ok, d_vst = torch.full((8,), 7, dtype=torch.uint8, device=dev), torch.full((8,), 7, dtype=torch.int32, device=dev)
    eng.member_verify_batch_device(8, d_com.data_ptr(), d_out.data_ptr(), None, d_ok.data_ptr(), d_vst.data_ptr())
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [1] * 8 and d_vst.cpu().tolist() == [0] * 8
    with pytest.raises(env['Z'].ZkError) as ei:   # out_cap one byte short
        eng.member_prove_batch_device(8, d_w.data_ptr(), d_bl.data_ptr(), d_seeds.data_ptr(), d_com.data_ptr(), d_bo.data_ptr(), d_out.data_ptr(), 8 * 1200 - 1, d_st.data_ptr())
    assert ei.value.status == 12


def test_ring300_fixed_indices_match_the_oracle_and_all_verify(env, ring300_run):
    eng = env['eng']
    seeds, (proofs, coms, blinders, st) = ring300_run
    for w in FIXED300:
        ref = M.oracle_prove(env['params'], M.RING300, w, M.R.SeedRng(seeds[32 * w:32 * w + 32]))
        assert (proofs[w], coms[w], blinders[w]) == ref, w
        assert M.oracle_verify(env['params'], M.RING300, coms[w], proofs[w]), w
    eng.use_ring(env['r300'])
    eng.set_chunk(128)
    ok, vst = eng.member_verify_batch(coms, proofs, vseeds=M.seeds_for(b'v300', 300))
    eng.set_chunk(4096)
    assert ok == [1] * 300 and vst == [0] * 300


def test_ring300_bytes_do_not_depend_on_the_plan_or_the_build(env, ring300_run):
    eng, Z = env['eng'], env['Z']
    seeds, base = ring300_run
    eng.use_ring(env['r300'])
    which = list(range(300))

    def run():
        out = eng.member_prove_batch(which, seeds=seeds)
        assert out[3] == [0] * 300
        return out
    assert run() == base   # the default chunk: one chunk of 300
    eng.set_chunk(128)
    try:
        for lanes in (1, 3):
            eng.set_lanes(lanes)
            assert run() == base, lanes
        eng.set_lanes(2)
        for fold in (0, 1):
            eng.set_ring_fold(fold)
            assert run() == base, fold
            ok, _ = eng.member_verify_batch(base[1][:40], base[0][:40])
            assert ok == [1] * 40, fold
    finally:
        eng.set_ring_fold(1), eng.set_lanes(2), eng.set_chunk(4096)
    uni = os.path.join(os.path.dirname(Z.LIB_PATH), 'libzkattest_hip_uniform.so')
    assert os.path.exists(uni), 'the uniform build is not there (make -C zkp-ecdsa_amd/csrc uniform)'
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'member_uniform_check.py')], env=dict(os.environ, ZKATTEST_LIB=uni),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    rec = json.loads(out.stdout.decode().strip().splitlines()[-1])
    assert rec['lib'].endswith('_uniform.so') and rec['sha256'] == hashlib.sha256(b''.join(base[0]) + b''.join(base[1])).hexdigest()


def test_one_proof_calls_on_both_rings(env, ring5_ref, ring300_run):
    eng = env['eng']
    seeds5, ref5 = ring5_ref
    eng.use_ring(env['r5'])
    proofs, coms, blinders, st = eng.member_prove_batch([6], seeds=seeds5[32 * 6:32 * 7])
    assert st == [0] and (proofs[0], coms[0], blinders[0]) == ref5[6]
    assert eng.member_verify_batch(coms, proofs) == ([1], [0])
    seeds300, base = ring300_run
    eng.use_ring(env['r300'])
    proofs, coms, blinders, st = eng.member_prove_batch([298], seeds=seeds300[32 * 298:32 * 299])
    assert st == [0] and (proofs[0], coms[0], blinders[0]) == (base[0][298], base[1][298], base[2][298])   # (== the oracle's: test_ring300_fixed_indices_...)
    assert eng.member_verify_batch(coms, proofs) == ([1], [0])


def test_stream_rng_with_rejected_fills(env):
    eng = env['eng']
    eng.use_ring(env['r5'])
    src = M.R.SeedRng(M.tag(b'stream', 0))
    fills = [src.fill(32) for _ in range(16)]   # 1 + 5 n draws
    blocks = [b'\xff' * 32] + fills[:7] + [b'\xff' * 32] + fills[7:]   # the blinder's first fill and a mid-proof fill are rejected (>= q)
    ref = M.oracle_prove(env['params'], M.RING5, 4, M.R.StreamRng(blocks))
    proofs, coms, blinders, st = eng.member_prove_batch([4], streams=b''.join(blocks), stream_blocks=18)
    assert st == [0] and (proofs[0], coms[0], blinders[0]) == ref
    assert blinders[0] == fills[0]
    proofs, coms, _, st = eng.member_prove_batch([4], streams=b''.join(blocks[:17]), stream_blocks=17)
    assert st == [ZK_E_RNG_EXHAUSTED] and proofs == [None] and eng.member_last_raw == bytes(1200)
    # caller's blinder: the 5 n draws start at fill 0
    bl = 987654321
    ref = M.oracle_prove(env['params'], M.RING5, 1, M.R.StreamRng(blocks[1:]), blinder=bl)
    proofs, coms, blinders, st = eng.member_prove_batch([1], blinders=bl.to_bytes(32, 'big'), streams=b''.join(blocks[1:17]), stream_blocks=16)
    assert st == [0] and (proofs[0], coms[0], blinders[0]) == ref


def _mutants(env, ring5_ref, big_proof):
    """(name, com, proof, expectation): expectation 'oracle' = deserialises, compare with the oracle's verdict (which must be False); 'bad' = ZK_E_BAD_ENCODING"""
    _, ref = ring5_ref
    n, S = 3, 1200
    T = M.TOM.p
    cases = []

    def base(k):
        return bytearray(ref[k % 5][0]), ref[k % 5][1]

    def flip(buf, pos, bit=1):
        buf[pos] ^= bit
        return buf
    k = 0
    sc0 = 16 + 288 * n
    for cls, name in enumerate(('f', 'za', 'zb')):
        for i in range(n):
            for byte in (0, 31):
                p, cm = base(k)
                cases.append(('%s[%d] byte %d' % (name, i, byte), cm, bytes(flip(p, sc0 + 32 * (cls * n + i) + byte)), 'oracle'))
                k += 1
    for byte in (0, 9, 20, 31):
        p, cm = base(k)
        cases.append(('zd byte %d' % byte, cm, bytes(flip(p, sc0 + 32 * 3 * n + byte, 0x40 if byte else 1)), 'oracle'))
        k += 1
    for j in range(2):   # com commits to a value outside the ring, same blinder
        p, cm = base(j)
        bl = int.from_bytes(ref[j][2], 'big')
        other = M.R._tp(M.R.gk_commit(env['params'], (M.RING5[j] + 1 + j) % M.Q, bl))
        cases.append(('com to a value outside the ring %d' % j, other, bytes(p), 'oracle'))

    def pt(k_):
        return 16 + 72 * k_
    for a, b in ((0, 1), (3 * n, 3 * n + 2), (1, 3 * n + 1)):   # cl_0 <-> cl_1, cd_0 <-> cd_2, cl_1 <-> cd_1
        p, cm = base(k)
        p[pt(a):pt(a) + 72], p[pt(b):pt(b) + 72] = p[pt(b):pt(b) + 72], p[pt(a):pt(a) + 72]
        cases.append(('points %d and %d swapped' % (a, b), cm, bytes(p), 'oracle'))
        k += 1
    cases.append(('a proof of the 300-value ring (n = 9), cut to the slot', big_proof[1], big_proof[0][:S], 'wrong n'))
    # ---- what does not deserialise
    hdr = [('magic byte %d' % i, i, 0x20) for i in range(4)] + [('total_len byte %d' % i, 4 + i, 1 << i) for i in (1, 2, 3)] + [('reserved byte %d' % i, 12 + i, 1) for i in (0, 3)]
    for name, pos, bit in hdr:
        p, cm = base(k)
        cases.append((name, cm, bytes(flip(p, pos, bit)), 'bad'))
        k += 1
    p, cm = base(k)
    p[8:12] = (64).to_bytes(4, 'big')
    p[4:8] = M.proof_size(64).to_bytes(4, 'big')
    cases.append(('n = 64', cm, bytes(p), 'bad'))
    p, cm = base(k + 1)
    p[8:12] = (2).to_bytes(4, 'big')
    cases.append(('n = 2 with the length of n = 3', cm, bytes(p), 'bad'))
    for q in range(4 * n):   # every point of the structure: y changed -> off the curve
        p, cm = base(q)
        flip(p, pt(q) + 71)
        x, y = int.from_bytes(p[pt(q):pt(q) + 36], 'big'), int.from_bytes(p[pt(q) + 36:pt(q) + 72], 'big')
        assert not M.TOM.isOnGroup(M.R.TEdwardsPoint(M.TOM, x, y, x * y % T, 1))
        cases.append(('point %d off its curve' % q, cm, bytes(p), 'bad'))
    for q, coord in ((0, 0), (n, 1), (2 * n + 1, 0), (4 * n - 1, 1)):   # x + t or y + t: on the curve mod t, not canonical
        p, cm = base(q)
        o = pt(q) + 36 * coord
        v = int.from_bytes(p[o:o + 36], 'big') + T
        p[o:o + 36] = v.to_bytes(36, 'big')
        cases.append(('point %d coordinate %d non-canonical' % (q, coord), cm, bytes(p), 'bad'))
    for q in (2, 3 * n):   # a padding byte of the 36-byte coordinate set
        p, cm = base(q)
        flip(p, pt(q), 0x80)
        cases.append(('point %d padding byte' % q, cm, bytes(p), 'bad'))
    for j, pos in ((0, 71), (1, 35)):
        p, cm = base(j)
        cm = bytes(flip(bytearray(cm), pos))
        cases.append(('com off its curve (byte %d)' % pos, cm, bytes(p), 'bad'))
    p, cm = base(2)
    cm = (int.from_bytes(cm[:36], 'big') + T).to_bytes(36, 'big') + cm[36:]
    cases.append(('com non-canonical', cm, bytes(p), 'bad'))
    return cases


def test_verifier_rejects_every_mutant_and_accepts_every_control(env, ring5_ref, ring300_run):
    eng = env['eng']
    _, ref = ring5_ref
    _, base300 = ring300_run
    cases = _mutants(env, ring5_ref, (base300[0][7], base300[1][7]))
    assert 60 <= len(cases) <= 70, len(cases)
    for name, cm, p, exp in cases:   # the oracle's verdict on what deserialises: every one of them is a forgery
        if exp == 'oracle':
            assert M.oracle_verify(env['params'], M.RING5, cm, p) is False, name
    controls = [0, len(cases) // 3, 2 * len(cases) // 3, len(cases)]   # untouched proofs between the mutants
    coms, proofs, want = [], [], []
    for i in range(len(cases) + 1):
        if i in controls:
            coms.append(ref[i % 8][1]), proofs.append(ref[i % 8][0]), want.append((1, 0, 'control'))
        if i < len(cases):
            name, cm, p, exp = cases[i]
            coms.append(cm), proofs.append(p), want.append((0, ZK_E_BAD_ENCODING if exp == 'bad' else 0, name))
    eng.use_ring(env['r5'])
    for rnd in range(3):
        ok, st = eng.member_verify_batch(coms, proofs, vseeds=M.seeds_for(b'vm%d' % rnd, len(proofs)))
        for i, (wok, wst, name) in enumerate(want):
            assert (ok[i], st[i]) == (wok, wst), (rnd, name, ok[i], st[i])
    ok, st = eng.member_verify_batch(coms, proofs)   # the engine's own seeds
    assert [(o, s) for o, s in zip(ok, st)] == [(w[0], w[1]) for w in want]


def test_ring_lifecycle(env):
    eng = env['eng']
    vals = M.ring_values(b'life', 5)
    rid = eng.add_ring(M.ring_bytes(vals), 5)
    try:
        eng.use_ring(rid)
        seeds = M.seeds_for(b'life', 2)
        old_p, old_c, _, st = eng.member_prove_batch([2, 3], seeds=seeds)
        assert st == [0, 0] and eng.member_verify_batch(old_c, old_p) == ([1, 1], [0, 0])
        new = (vals[2] + 99) % M.Q
        eng.update_ring(rid, {2: new.to_bytes(32, 'big')})
        new_p, new_c, _, st = eng.member_prove_batch([2, 3], seeds=seeds)
        assert st == [0, 0]
        ref = M.oracle_prove(env['params'], vals[:2] + [new] + vals[3:], 2, M.R.SeedRng(seeds[:32]))
        assert (new_p[0], new_c[0]) == ref[:2]
        assert new_p[1] != old_p[1] and new_c[1] == old_c[1]   # index 3's value is unchanged, the ring it is shown to be in is not
        # the proofs for the new ring verify; the ones made before the update -- for the old value at index 2, and for index 3 over the old ring -- do not
        assert eng.member_verify_batch(new_c + old_c, new_p + old_p) == ([1, 1, 0, 0], [0, 0, 0, 0])
        eng.use_ring(env['r300'])   # another resident ring: the size and the verdicts follow the active one
        assert eng.member_proof_size() == 3504
        p300, c300, _, st = eng.member_prove_batch([299], seeds=seeds[:32])
        assert st == [0] and len(p300[0]) == 3504 and eng.member_verify_batch(c300, p300) == ([1], [0])
        eng.use_ring(rid)
        assert eng.member_proof_size() == 1200
        assert eng.member_verify_batch(new_c + [c300[0]], new_p + [p300[0][:1200]]) == ([1, 1, 0], [0, 0, 0])
    finally:
        eng.use_ring(env['r5'])   # the active ring cannot be dropped
        eng.drop_ring(rid)


def test_wipe_then_the_same_call_gives_the_same_bytes(env, ring5_ref):
    eng = env['eng']
    eng.use_ring(env['r5'])
    seeds, _ = ring5_ref
    a = eng.member_prove_batch(list(range(8)), seeds=seeds[:256])
    eng.wipe()
    b = eng.member_prove_batch(list(range(8)), seeds=seeds[:256])
    assert a == b and a[3] == [0] * 8
    assert eng.member_verify_batch(b[1], b[0]) == ([1] * 8, [0] * 8)


def test_hardened_mode_refuses_the_calls(env):
    eng, Z = env['eng'], env['Z']
    eng.use_ring(env['r5'])
    eng.set_mode(Z.MODE_HARDENED)
    try:
        with pytest.raises(Z.ZkError) as ei:
            eng.member_prove_batch([0], seeds=bytes(32))
        assert ei.value.status == ZK_E_ARG
        with pytest.raises(Z.ZkError) as ei:
            eng.member_verify_batch([bytes(72)], [bytes(1200)])
        assert ei.value.status == ZK_E_ARG
    finally:
        eng.set_mode(Z.MODE_REFERENCE)
