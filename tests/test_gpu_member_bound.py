"""gpu: bound membership proofs, "ZKMB" (include/zkattest.h: zk_member_*_bound) -- the challenge hashes ring digest, caller context and com behind the 4 n
points -- against the Python oracle's proveMembership / verifyMembership with statement=S_b (tests/member_bound_common.py).

Rings of 2, 4 (3 real keys), 8, 256, 512 (300 real keys) and 4 096 keys: n = 1, 2, 3, 8, 9, 12 -- the plain fold, the two small sizes whose padding spills
into an extra SHA-256 block (n = 3, n = 8), the first table-E size and the first matrix-core size.  Three proofs per ring with distinct contexts, one of them
for the padding copy of keys[0] where the ring is padded, engine-drawn and caller blinders; the oracle's side is computed once per module."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import member_bound_common as MB

M = MB.M
pytestmark = pytest.mark.gpu
ZK_E_BAD_ENCODING, ZK_E_ARG = 10, 14
RINGS, LOG2, MODES, inputs = MB.RINGS, MB.LOG2, MB.MODES, MB.inputs


@pytest.fixture(scope='module')
def env():
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    nh, tg, th = eng.synth_params(M.PARAM_SEED)
    eng.set_params(nh, tg, th, 80)
    e = {'Z': Z, 'eng': eng, 'params': M.oracle_params(tg, th), 'vals': {}, 'rid': {}}
    for name, (count, _) in RINGS.items():
        e['vals'][name] = M.ring_values(name.encode(), count)
        e['rid'][name] = eng.add_ring(M.ring_bytes(e['vals'][name]), count)
    yield e
    eng.close()


@pytest.fixture(scope='module')
def ref(env):
    """the oracle: ref[name][mode] = three (proof, com, blinder) with statement=S_b"""
    out = {}
    for name in RINGS:
        which, ctx, seeds, bl = inputs(name)
        out[name] = {}
        for mode in MODES:
            out[name][mode] = [MB.oracle_prove(env['params'], env['vals'][name], which[b], M.R.SeedRng(seeds[32 * b:32 * b + 32]), ctx[b],
                                               blinder=bl[b] if mode == 'caller' else None) for b in range(3)]
    return out


def prove(eng, name, mode, bound=True):
    which, ctx, seeds, bl = inputs(name)
    blb = b''.join(b.to_bytes(32, 'big') for b in bl) if mode == 'caller' else None
    return eng.member_prove_batch(which, blinders=blb, seeds=seeds, context=ctx if bound else None)


@pytest.fixture(scope='module')
def run(env):
    """the engine's bound proofs of every ring, both blinder modes (reference mode)"""
    eng, out = env['eng'], {}
    for name in RINGS:
        eng.use_ring(env['rid'][name])
        out[name] = {mode: prove(eng, name, mode) for mode in MODES}
    return out


@pytest.mark.parametrize('name', list(RINGS))
def test_bytes_are_the_oracles(env, ref, run, name):
    eng = env['eng']
    eng.use_ring(env['rid'][name])
    assert eng.member_proof_size() == M.proof_size(LOG2[name])
    for mode in MODES:
        proofs, coms, blinders, st = run[name][mode]
        assert st == [0, 0, 0], (mode, st)
        for b in range(3):
            assert proofs[b][:4] == b'ZKMB' and len(proofs[b]) == M.proof_size(LOG2[name])
            assert (proofs[b], coms[b], blinders[b]) == ref[name][mode][b], (mode, b)


@pytest.mark.parametrize('name', list(RINGS))
def test_verdicts_follow_context_com_and_magic(env, ref, run, name):
    eng, Z = env['eng'], env['Z']
    eng.use_ring(env['rid'][name])
    _, ctx, _, _ = inputs(name)
    vals = env['vals'][name]
    for mode in MODES:
        proofs, coms, _, _ = run[name][mode]
        assert eng.member_verify_batch(coms, proofs, context=ctx) == ([1, 1, 1], [0, 0, 0]), mode
        assert all(MB.oracle_verify(env['params'], vals, coms[b], proofs[b], ctx[b]) for b in range(3)), mode
    proofs, coms, _, _ = run[name]['drawn']
    flipped = [bytes([ctx[0][0] ^ 1]) + ctx[0][1:], ctx[1][:31] + bytes([ctx[1][31] ^ 0x80]), ctx[2][:13] + bytes([ctx[2][13] ^ 0x10]) + ctx[2][14:]]
    assert eng.member_verify_batch(coms, proofs, context=flipped) == ([0, 0, 0], [0, 0, 0])
    assert not MB.oracle_verify(env['params'], vals, coms[0], proofs[0], flipped[0])
    assert eng.member_verify_batch(coms, proofs, context=[ctx[1], ctx[2], ctx[0]]) == ([0, 0, 0], [0, 0, 0])   # another proof's context
    # com swapped with a neighbour's (proofs 0 and 1 are about different values); the third is a control
    assert eng.member_verify_batch([coms[1], coms[0], coms[2]], proofs, context=ctx) == ([0, 0, 1], [0, 0, 0])
    # the other magic is a wrong magic, in both directions
    zkm1 = prove(eng, name, 'drawn', bound=False)
    assert zkm1[3] == [0, 0, 0] and all(p[:4] == b'ZKM1' for p in zkm1[0])
    assert eng.member_verify_batch(zkm1[1], zkm1[0], context=ctx) == ([0, 0, 0], [ZK_E_BAD_ENCODING] * 3)
    assert eng.member_verify_batch(coms, proofs) == ([0, 0, 0], [ZK_E_BAD_ENCODING] * 3)
    relabelled = [b'ZKMB' + p[4:] for p in zkm1[0]]   # a ZKM1 transcript under the bound magic: the challenge is another one
    assert eng.member_verify_batch(zkm1[1], relabelled, context=ctx) == ([0, 0, 0], [0, 0, 0])


@pytest.mark.parametrize('name', list(RINGS))
def test_unbound_calls_return_what_they_returned(env, name):
    eng = env['eng']
    eng.use_ring(env['rid'][name])
    which, _, seeds, bl = inputs(name)
    for mode in MODES:
        proofs, coms, blinders, st = prove(eng, name, mode, bound=False)
        assert st == [0, 0, 0]
        for b in range(3):
            want = M.oracle_prove(env['params'], env['vals'][name], which[b], M.R.SeedRng(seeds[32 * b:32 * b + 32]), blinder=bl[b] if mode == 'caller' else None)
            assert (proofs[b], coms[b], blinders[b]) == want, (mode, b)
        assert eng.member_verify_batch(coms, proofs) == ([1, 1, 1], [0, 0, 0])


def test_update_ring_changes_the_digest_every_bound_proof_hashes(env, ref):
    eng = env['eng']
    vals = list(env['vals']['k8'])
    rid = eng.add_ring(M.ring_bytes(vals), 8)
    try:
        eng.use_ring(rid)
        which, ctx, seeds, _ = inputs('k8')   # indices 0, 5, 7
        old = prove(eng, 'k8', 'drawn')
        assert [(old[0][b], old[1][b], old[2][b]) for b in range(3)] == ref['k8']['drawn']   # same keys, same bytes as the first 8-key ring
        assert eng.member_verify_batch(old[1], old[0], context=ctx) == ([1, 1, 1], [0, 0, 0])
        new_vals = vals[:3] + [(vals[3] + 77) % M.Q] + vals[4:]   # key 3 is none of the proofs'
        eng.update_ring(rid, {3: new_vals[3].to_bytes(32, 'big')})
        assert eng.member_verify_batch(old[1], old[0], context=ctx) == ([0, 0, 0], [0, 0, 0])
        assert not any(MB.oracle_verify(env['params'], new_vals, old[1][b], old[0][b], ctx[b]) for b in range(3))
        new = prove(eng, 'k8', 'drawn')
        for b in range(3):
            want = MB.oracle_prove(env['params'], new_vals, which[b], M.R.SeedRng(seeds[32 * b:32 * b + 32]), ctx[b])
            assert (new[0][b], new[1][b], new[2][b]) == want, b
        assert new[1] == old[1] and all(new[0][b] != old[0][b] for b in range(3))   # the same commitments, shown to be in another ring
        assert eng.member_verify_batch(new[1], new[0], context=ctx) == ([1, 1, 1], [0, 0, 0])
    finally:
        eng.use_ring(env['rid']['k8'])
        eng.drop_ring(rid)


def test_hardened_mode_runs_the_bound_calls_and_still_refuses_the_unbound_ones(env, run):
    eng, Z = env['eng'], env['Z']
    eng.set_mode(Z.MODE_HARDENED)
    try:
        for name in ('k8', 'k300'):
            eng.use_ring(env['rid'][name])
            _, ctx, _, _ = inputs(name)
            for mode in MODES:
                got = prove(eng, name, mode)
                assert got == run[name][mode], (name, mode)
                assert eng.member_verify_batch(got[1], got[0], context=ctx) == ([1, 1, 1], [0, 0, 0])
            with pytest.raises(Z.ZkError) as ei:
                prove(eng, name, 'drawn', bound=False)
            assert ei.value.status == ZK_E_ARG
            with pytest.raises(Z.ZkError) as ei:
                eng.member_verify_batch(run[name]['drawn'][1], run[name]['drawn'][0])
            assert ei.value.status == ZK_E_ARG
        ids = [env['rid']['k8'], env['rid']['k300']]
        with pytest.raises(Z.ZkError) as ei:
            eng.member_prove_batch_rings([0, 0], ids, seeds=bytes(64))
        assert ei.value.status == ZK_E_ARG
        p, cm, _, st = eng.member_prove_batch_rings([0, 0], ids, seeds=bytes(64), context=bytes(64))
        assert st == [0, 0] and eng.member_verify_batch_rings(cm, p, ids, context=bytes(64)) == ([1, 1], [0, 0])
    finally:
        eng.set_mode(Z.MODE_REFERENCE)


def test_null_context_is_an_argument_error(env):
    eng, L = env['eng'], env['Z'].lib()
    eng.use_ring(env['rid']['k8'])
    ok, st = (C.c_uint8 * 1)(), (C.c_int32 * 1)()
    assert L.zk_member_verify_batch_bound(eng.h, 1, bytes(72), None, bytes(1200), None, ok, st) == ZK_E_ARG
    assert L.zk_member_verify_batch_bound(eng.h, 0, None, None, None, None, ok, st) == ZK_E_ARG
    assert L.zk_member_verify_batch_bound(eng.h, 0, None, bytes(32), None, None, ok, st) == 0


def test_rings_form_hashes_each_proofs_own_ring(env):
    eng = env['eng']
    a, big = env['rid']['k8'], env['rid']['k300']
    other_vals = M.ring_values(b'k8-other', 8)
    other_vals[2] = env['vals']['k8'][2]   # key 2 is in both 8-key rings
    other = eng.add_ring(M.ring_bytes(other_vals), 8)
    try:
        unknown = max(a, big, other) + 1000
        ids = [a, big, a, unknown, big, other, a, big]   # 7 proofs interleaved over the two rings (one of them over the second 8-key ring) + one id that is not resident
        which = [2, 299, 7, 0, 511, 2, 0, 1]
        B = len(ids)
        ctx = [MB.context_for(b'rings', b) for b in range(B)]
        seeds = M.seeds_for(b'bound-rings', B)
        windows = eng.test_counter(13)
        proofs, coms, blinders, st = eng.member_prove_batch_rings(which, ids, seeds=seeds, context=ctx)
        assert eng.test_counter(13) - windows == 3   # one window per ring
        assert st == [0, 0, 0, ZK_E_ARG, 0, 0, 0, 0] and proofs[3] is None and coms[3] == bytes(72) and blinders[3] == bytes(32)
        off, raw = eng.member_last_off, eng.member_last_raw   # (the one-ring calls below overwrite the engine's copies)
        assert off[4] == off[3]
        ok, vst = eng.member_verify_batch_rings(coms, raw, ids, offsets=off, context=ctx)
        assert ok == [1, 1, 1, 0, 1, 1, 1, 1] and vst == [0, 0, 0, ZK_E_ARG, 0, 0, 0, 0]
        for rid in (a, big, other):   # slot, com, status and verdict of the one-ring bound call with that ring active
            sel = [b for b in range(B) if ids[b] == rid]
            eng.use_ring(rid)
            one = eng.member_prove_batch([which[b] for b in sel], seeds=b''.join(seeds[32 * b:32 * b + 32] for b in sel), context=[ctx[b] for b in sel])
            assert one[3] == [0] * len(sel)
            assert (one[0], one[1], one[2]) == ([proofs[b] for b in sel], [coms[b] for b in sel], [blinders[b] for b in sel]), rid
            assert eng.member_verify_batch(one[1], one[0], context=[ctx[b] for b in sel]) == ([1] * len(sel), [0] * len(sel))
        # proofs 0 (ring a) and 5 (ring `other`) are about the same value at the same index of two rings of equal size: each verifies under its own ring's id only
        swapped = list(ids)
        swapped[0], swapped[5] = other, a
        ok, vst = eng.member_verify_batch_rings(coms, raw, swapped, offsets=off, context=ctx)
        assert ok == [0, 1, 1, 0, 1, 0, 1, 1] and vst == [0, 0, 0, ZK_E_ARG, 0, 0, 0, 0]
        assert MB.oracle_verify(env['params'], env['vals']['k8'], coms[0], proofs[0], ctx[0])
        assert not MB.oracle_verify(env['params'], other_vals, coms[0], proofs[0], ctx[0])
        # a wrong context in one window entry fails that entry alone
        bad = list(ctx)
        bad[4] = ctx[1]
        ok, _ = eng.member_verify_batch_rings(coms, raw, ids, offsets=off, context=bad)
        assert ok == [1, 1, 1, 0, 0, 1, 1, 1]
    finally:
        eng.use_ring(a)
        eng.drop_ring(other)


@pytest.mark.parametrize('name', ['k8', 'k300'])
def test_device_pointer_forms_give_the_same_bytes_and_verdicts(env, run, name):
    import torch
    eng = env['eng']
    rid = env['rid'][name]
    eng.use_ring(rid)
    which, ctx, seeds, bl = inputs(name)
    size = M.proof_size(LOG2[name])
    dev = torch.device('cuda:0')

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    proofs, coms, blinders, _ = run[name]['caller']
    d_w = torch.tensor(which, dtype=torch.int32, device=dev)
    d_ctx, d_bl, d_seeds = up(b''.join(ctx)), up(b''.join(b.to_bytes(32, 'big') for b in bl)), up(seeds)
    d_com, d_bo = torch.zeros(3 * 72, dtype=torch.uint8, device=dev), torch.zeros(3 * 32, dtype=torch.uint8, device=dev)
    d_out, d_st = torch.full((3 * size,), 7, dtype=torch.uint8, device=dev), torch.full((3,), 7, dtype=torch.int32, device=dev)
    eng.member_prove_batch_device(3, d_w.data_ptr(), d_bl.data_ptr(), d_seeds.data_ptr(), d_com.data_ptr(), d_bo.data_ptr(), d_out.data_ptr(), 3 * size, d_st.data_ptr(),
                                  d_context=d_ctx.data_ptr())
    torch.cuda.synchronize()
    assert bytes(d_out.cpu().numpy()) == b''.join(proofs) and bytes(d_com.cpu().numpy()) == b''.join(coms)
    assert bytes(d_bo.cpu().numpy()) == b''.join(blinders) and d_st.cpu().tolist() == [0, 0, 0]
    d_ok, d_vst = torch.full((3,), 7, dtype=torch.uint8, device=dev), torch.full((3,), 7, dtype=torch.int32, device=dev)
    eng.member_verify_batch_device(3, d_com.data_ptr(), d_out.data_ptr(), None, d_ok.data_ptr(), d_vst.data_ptr(), d_context=d_ctx.data_ptr())
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [1, 1, 1] and d_vst.cpu().tolist() == [0, 0, 0]
    d_bad = up(b''.join([ctx[0], ctx[2], ctx[2]]))
    eng.member_verify_batch_device(3, d_com.data_ptr(), d_out.data_ptr(), None, d_ok.data_ptr(), d_vst.data_ptr(), d_context=d_bad.data_ptr())
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [1, 0, 1] and d_vst.cpu().tolist() == [0, 0, 0]
    # the _rings device forms on the same inputs (one ring: the caller's buffers as they are)
    d_ids = torch.full((3,), rid, dtype=torch.int32, device=dev)
    d_off = torch.zeros(4, dtype=torch.int64, device=dev)
    d_out2, d_com2 = torch.full((3 * size,), 7, dtype=torch.uint8, device=dev), torch.zeros(3 * 72, dtype=torch.uint8, device=dev)
    eng.member_prove_batch_rings_device(3, d_w.data_ptr(), d_ids.data_ptr(), d_bl.data_ptr(), d_seeds.data_ptr(), d_com2.data_ptr(), d_bo.data_ptr(), d_out2.data_ptr(), 3 * size,
                                        d_off.data_ptr(), d_st.data_ptr(), d_context=d_ctx.data_ptr())
    torch.cuda.synchronize()
    assert bytes(d_out2.cpu().numpy()) == b''.join(proofs) and bytes(d_com2.cpu().numpy()) == b''.join(coms) and d_off.cpu().tolist() == [0, size, 2 * size, 3 * size]
    eng.member_verify_batch_rings_device(3, d_com2.data_ptr(), d_out2.data_ptr(), d_off.data_ptr(), d_ids.data_ptr(), None, d_ok.data_ptr(), d_vst.data_ptr(),
                                         d_context=d_bad.data_ptr())
    torch.cuda.synchronize()
    assert d_ok.cpu().tolist() == [1, 0, 1] and d_vst.cpu().tolist() == [0, 0, 0]


def test_uniform_build_gives_the_same_bytes(env, run):
    Z = env['Z']
    uni = os.path.join(os.path.dirname(Z.LIB_PATH), 'libzkattest_hip_uniform.so')
    assert os.path.exists(uni), 'the uniform build is not there (make -C zkp-ecdsa_amd/csrc uniform)'
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'member_bound_uniform_check.py')], env=dict(os.environ, ZKATTEST_LIB=uni),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    rec = json.loads(out.stdout.decode().strip().splitlines()[-1])
    want = hashlib.sha256(b''.join(b''.join(run['k8'][mode][0]) + b''.join(run['k8'][mode][1]) + b''.join(run['k8'][mode][2]) for mode in MODES)).hexdigest()
    assert rec['lib'].endswith('_uniform.so') and rec['sha256'] == want and rec['verdicts'] == [[1, 1, 1], [0, 0, 0]]
