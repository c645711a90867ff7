"""gpu: the host layer of the membership and re-ring calls (csrc/api_member.hip, csrc/api_rering.hip) seen from outside -- what a change of its plumbing
must leave alone.  The NULL checks of the 16 zk_member_* entry points (bound / unbound, one ring / _rings, host / _device), argument by argument; the timed
families each kind of call puts on the streams (zk_last_timing), chunks of 2, 2, 1 over two lanes; and a mixed-ring call with every optional input at once
-- bound, caller blinders, ZK_RNG_STREAM, blinders out -- through two windows per ring, against the one-ring bound calls.  Rings of 5 and 17 values
(n = 3, 5) as in test_gpu_member_rings.py, secLevel 20; the re-ring calls move five ZKA1 proofs between two rings of 5 keys."""
import ctypes as C
import os
import struct
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import member_common as M

pytestmark = pytest.mark.gpu
ZK_OK, ZK_E_ARG = 0, 14
RING17 = M.ring_values(b'ring17', 17)
WINDOWS = 13   # zk_test_counter: windows of mixed-ring membership calls
SIZE5, SIZE17 = 1200, 1968


@pytest.fixture(scope='module')
def env():
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    nh, tg, th = eng.synth_params(M.PARAM_SEED)
    eng.set_params(nh, tg, th, 20)
    e = {'Z': Z, 'eng': eng}
    e['r5'] = eng.add_ring(M.ring_bytes(M.RING5), 5)
    e['r17'] = eng.add_ring(M.ring_bytes(RING17), 17)
    assert [eng.member_proof_size(r) for r in (e['r5'], e['r17'])] == [SIZE5, SIZE17]
    # re-ring: five ZKA1 proofs over ring A (5 keys, signer b's key at which[b]) and ring B with A's keys in reverse order
    ringA, e['msg'], sig, pk, e['whichA'], seeds = eng.synth_workload(77, 5, 5)
    e['rA'] = eng.add_ring(ringA, 5)
    e['rB'] = eng.add_ring(b''.join(ringA[32 * (4 - i):32 * (5 - i)] for i in range(5)), 5)
    eng.use_ring(e['rA'])
    e['zka1'], st = eng.prove_batch(e['msg'], sig, pk, e['whichA'], seeds=seeds)
    assert st == [0] * 5
    e['key_blinders'] = eng.prove_key_blinders(seeds=seeds)
    yield e
    eng.close()


# ---------------------------------------------------------------- 1: the NULL matrix
PROVE = ('which', 'context', 'blinder', 'rng', 'com', 'blinder_out', 'out', 'out_cap', 'status')
PROVE_RINGS = ('which', 'context', 'ids', 'blinder', 'rng', 'com', 'blinder_out', 'out', 'out_cap', 'out_off', 'status')
VERIFY = ('com', 'context', 'proofs', 'vseeds', 'ok', 'status')
VERIFY_RINGS = ('com', 'context', 'proofs', 'proof_off', 'ids', 'vseeds', 'ok', 'status')
OPTIONAL = ('blinder', 'blinder_out', 'vseeds')
ALWAYS = ('rng', 'context', 'out_off')   # required whatever B is (context: the bound forms, out_off: the rings prove forms)
ENTRY_POINTS = [(side, rings, bound, device) for side in ('prove', 'verify') for rings in (False, True) for bound in (False, True) for device in (False, True)]


def _params(side, rings, bound):
    names = {('prove', False): PROVE, ('prove', True): PROVE_RINGS, ('verify', False): VERIFY, ('verify', True): VERIFY_RINGS}[(side, rings)]
    return [p for p in names if bound or p != 'context']


def _name(side, rings, bound, device):
    return 'zk_member_%s_batch%s%s%s' % (side, '_rings' if rings else '', '_bound' if bound else '', '_device' if device else '')


def _buffers(env, device):
    """one valid value per parameter name for B = 2 (proof 0 over the 5-value ring, proof 1 over the 17-value ring's id in the rings forms); the second
    dict keeps them alive and readable"""
    raw = {'which': struct.pack('<2I', 0, 1), 'ids': struct.pack('<2I', env['r5'], env['r17']), 'context': M.tag(b'args-ctx', 0) + M.tag(b'args-ctx', 1),
           'blinder': (7).to_bytes(32, 'big') + (9).to_bytes(32, 'big'), 'seeds': M.seeds_for(b'args', 2), 'com': bytes(144), 'blinder_out': bytes(64), 'out': bytes(4096),
           'out_off': b'\x5a' * 24, 'status': bytes(8), 'proofs': bytes(4096), 'proof_off': struct.pack('<3Q', 0, SIZE5, SIZE5 + SIZE17), 'vseeds': M.seeds_for(b'args-v', 2),
           'ok': bytes(2)}
    if device:
        import torch
        keep = {k: torch.frombuffer(bytearray(v), dtype=torch.uint8).to('cuda:0') for k, v in raw.items()}
        torch.cuda.synchronize()
        val = {k: t.data_ptr() for k, t in keep.items()}
    else:
        keep = {k: C.create_string_buffer(v, len(v)) for k, v in raw.items()}
        val = dict(keep)
    val['out_cap'] = 4096
    return val, keep


def _call(env, entry, val, B, drop=None):
    """the entry point on `val` with parameter `drop` NULL ('c': the context, 'rng.data': the RNG's data pointer)"""
    Z, eng = env['Z'], env['eng']
    side, rings, bound, device = entry
    seeds = val.get('seeds')
    data = None if drop == 'rng.data' or seeds is None else seeds if device else C.cast(seeds, C.c_void_p)
    rng = Z.ZkRng(0, data, 0)
    args = []
    for p in _params(side, rings, bound):
        if p == drop:
            args.append(None)
        elif p == 'rng':
            args.append(C.byref(rng))
        else:
            args.append(val.get(p, 0 if p == 'out_cap' else None))
    return getattr(eng.L, _name(*entry))(None if drop == 'c' else eng.h, B, *args)


def _out_off(entry, keep):
    """the three offset words as they lie in the out_off buffer"""
    if entry[3]:
        import torch
        torch.cuda.synchronize()
        return struct.unpack('<3Q', bytes(keep['out_off'].cpu().numpy()))
    return struct.unpack('<3Q', keep['out_off'].raw)


@pytest.mark.parametrize('entry', ENTRY_POINTS, ids=lambda e: _name(*e))
def test_null_matrix(env, entry):
    eng = env['eng']
    side, rings, bound, device = entry
    eng.use_ring(env['r5'])
    params = _params(side, rings, bound)
    val, keep = _buffers(env, device)
    # B = 2: every pointer but the optional ones is required
    assert _call(env, entry, val, 2) == ZK_OK
    for p in ['c'] + [p for p in params if p not in OPTIONAL and p != 'out_cap'] + (['rng.data'] if side == 'prove' else []):
        assert _call(env, entry, val, 2, drop=p) == ZK_E_ARG, p
    for p in params:
        if p in OPTIONAL:
            assert _call(env, entry, val, 2, drop=p) == ZK_OK, p
    # B = 0: the context, the RNG (not its data), the bound forms' context and the rings prove forms' out_off -- which gets its one offset
    val, keep = _buffers(env, device)   # fresh ones: the B = 2 calls above have written their offsets into out_off
    val0 = {p: val[p] for p in params if p in ALWAYS and p != 'rng'}
    untouched = struct.unpack('<Q', b'\x5a' * 8)[0]
    if side == 'prove' and rings:
        assert _out_off(entry, keep) == (untouched,) * 3
    assert _call(env, entry, val0, 0) == ZK_OK
    if side == 'prove' and rings:
        assert _out_off(entry, keep) == (0, untouched, untouched)
    for p in ['c'] + [p for p in params if p in ALWAYS]:
        assert _call(env, entry, val0, 0, drop=p) == ZK_E_ARG, p


# ---------------------------------------------------------------- 2: the timed families of every kind of call
PROVER = ['gk_fold', 'hash', 'respond_write', 'rng_prepass', 'tom_commit', 'tom_normalize']
VERIFIER = ['v_gk_total', 'v_parse_validate', 'v_sums']
FAMILIES = {
    'prove': PROVER, 'verify': VERIFIER,
    'mixed prove': sorted(PROVER + ['m_class', 'm_gather']), 'mixed verify': sorted(VERIFIER + ['m_class', 'm_gather']),
    'one-class prove': PROVER, 'one-class verify': VERIFIER,   # host pointers: classed on the host, then the one-ring call
    'one-class prove device': sorted(PROVER + ['m_class']), 'one-class verify device': sorted(VERIFIER + ['m_class']),
    'rering': sorted(PROVER + ['rr_census', 'rr_offsets', 'rr_move']), 'rering in place': sorted(PROVER + ['rr_census', 'rr_offsets']),
}


def _families(eng):
    """the names zk_last_timing lists for the last call, as listed (a name listed twice stays twice)"""
    total, names, ms = C.c_float(), (C.c_char_p * 32)(), (C.c_float * 32)()
    n = eng.L.zk_last_timing(eng.h, C.byref(total), names, ms, 32)
    return sorted(names[i].decode() for i in range(n))


def test_timing_families(env):
    import torch
    eng = env['eng']
    r5, r17 = env['r5'], env['r17']
    seeds = M.seeds_for(b'fam', 5)
    got = {}
    eng.set_timing(1), eng.set_chunk(2), eng.set_lanes(2)
    try:
        eng.use_ring(r5)
        p, cm, _, st = eng.member_prove_batch([0, 1, 2, 3, 4], seeds=seeds)
        got['prove'] = _families(eng)
        assert st == [0] * 5 and eng.member_verify_batch(cm, p) == ([1] * 5, [0] * 5)
        got['verify'] = _families(eng)
        ids = [r5, r17, r5, r17, r5]
        p, cm, _, st = eng.member_prove_batch_rings([0, 1, 2, 3, 4], ids, seeds=seeds)
        got['mixed prove'] = _families(eng)
        assert st == [0] * 5 and eng.member_verify_batch_rings(cm, p, ids) == ([1] * 5, [0] * 5)
        got['mixed verify'] = _families(eng)
        p, cm, _, st = eng.member_prove_batch_rings([0, 1, 2, 3, 4], [r17] * 5, seeds=seeds)
        got['one-class prove'] = _families(eng)
        assert st == [0] * 5 and eng.member_verify_batch_rings(cm, p, [r17] * 5) == ([1] * 5, [0] * 5)
        got['one-class verify'] = _families(eng)
        d = {k: torch.frombuffer(bytearray(v), dtype=torch.uint8).to('cuda:0') for k, v in (
            ('which', struct.pack('<5I', 0, 1, 2, 3, 4)), ('ids', struct.pack('<5I', *[r17] * 5)), ('seeds', seeds), ('com', bytes(72 * 5)), ('out', bytes(SIZE17 * 5)),
            ('off', bytes(48)), ('st', bytes(20)), ('ok', bytes(5)))}
        eng.member_prove_batch_rings_device(5, d['which'].data_ptr(), d['ids'].data_ptr(), None, d['seeds'].data_ptr(), d['com'].data_ptr(), None, d['out'].data_ptr(), SIZE17 * 5,
                                            d['off'].data_ptr(), d['st'].data_ptr())
        got['one-class prove device'] = _families(eng)
        eng.member_verify_batch_rings_device(5, d['com'].data_ptr(), d['out'].data_ptr(), d['off'].data_ptr(), d['ids'].data_ptr(), None, d['ok'].data_ptr(), d['st'].data_ptr())
        got['one-class verify device'] = _families(eng)
        torch.cuda.synchronize()
        assert bytes(d['out'].cpu().numpy()) == b''.join(p) and d['ok'].cpu().tolist() == [1] * 5
        eng.use_ring(env['rB'])
        idxB = [4 - w for w in env['whichA']]
        fresh = M.seeds_for(b'fam-fresh', 5)
        out, st = eng.rering_batch(env['msg'], env['zka1'], idxB, env['key_blinders'], seeds=fresh)
        got['rering'] = _families(eng)
        assert st == [0] * 5
        out2, st = eng.rering_batch(env['msg'], env['zka1'], idxB, env['key_blinders'], seeds=fresh, in_place=True)
        got['rering in place'] = _families(eng)
        assert st == [0] * 5 and out2 == out and eng.verify_batch(env['msg'], out) == ([1] * 5, [0] * 5)
    finally:
        eng.set_timing(2), eng.set_chunk(4096), eng.set_lanes(2)
    print('families:', got)
    assert got == FAMILIES


# ---------------------------------------------------------------- 3: every optional input at once, through windows
NB = 40   # stream blocks per proof: the 5 n = 25 draws of the larger ring, and room for rejected ones
WINDOWS_PER_CALL = 4


def test_every_optional_input_through_windows(env):
    import torch
    eng = env['eng']
    r5, r17 = env['r5'], env['r17']
    B = 24
    ids = [r5 if b % 2 == 0 else r17 for b in range(B)]
    which = [(b // 2) % 8 if b % 2 == 0 else (5 * (b // 2) + 3) % 32 for b in range(B)]
    ctx = [M.tag(b'win-ctx', b) for b in range(B)]
    blinders = b''.join((int.from_bytes(M.tag(b'win-bl', b), 'big') % M.Q).to_bytes(32, 'big') for b in range(B))
    rows = []
    for b in range(B):
        src = M.R.SeedRng(M.tag(b'win-stream', b))
        rows.append(b''.join(src.fill(32) for _ in range(NB)))
    streams = b''.join(rows)
    vseeds = M.seeds_for(b'win-v', B)
    sizes = [SIZE5 if r == r5 else SIZE17 for r in ids]
    off = [sum(sizes[:b]) for b in range(B + 1)]
    eng.set_chunk(2), eng.set_lanes(2)
    try:
        # the one-ring bound calls, ring by ring
        ref = [None] * B
        for r in (r5, r17):
            idx = [b for b in range(B) if ids[b] == r]
            eng.use_ring(r)
            w0 = eng.test_counter(WINDOWS)
            one = eng.member_prove_batch([which[b] for b in idx], blinders=b''.join(blinders[32 * b:32 * b + 32] for b in idx), streams=b''.join(rows[b] for b in idx),
                                         stream_blocks=NB, context=[ctx[b] for b in idx])
            assert eng.test_counter(WINDOWS) == w0 and one[3] == [0] * 12
            for k, b in enumerate(idx):
                ref[b] = tuple(col[k] for col in one)
        assert all(x[0][:4] == b'ZKMB' and x[2] == blinders[32 * b:32 * b + 32] for b, x in enumerate(ref))
        # host pointers
        w0 = eng.test_counter(WINDOWS)
        got = eng.member_prove_batch_rings(which, ids, blinders=blinders, streams=streams, stream_blocks=NB, context=ctx)
        windows = eng.test_counter(WINDOWS) - w0
        print('windows per mixed prove call:', windows)
        assert [tuple(col[b] for col in got) for b in range(B)] == ref
        assert eng.member_last_off == off
        raw = eng.member_last_raw
        assert windows == WINDOWS_PER_CALL
        # device pointers
        def up(b):
            return torch.frombuffer(bytearray(b), dtype=torch.uint8).to('cuda:0')

        def fill(n):
            return torch.full((n,), 0x5a, dtype=torch.uint8, device='cuda:0')
        d_which, d_ids, d_ctx = up(struct.pack('<24I', *which)), up(struct.pack('<24I', *ids)), up(b''.join(ctx))
        d_bl, d_rng, d_vs = up(blinders), up(streams), up(vseeds)
        d_com, d_bo, d_out, d_off, d_st = fill(72 * B), fill(32 * B), fill(off[B]), fill(8 * (B + 1)), fill(4 * B)
        w0 = eng.test_counter(WINDOWS)
        eng.member_prove_batch_rings_device(B, d_which.data_ptr(), d_ids.data_ptr(), d_bl.data_ptr(), d_rng.data_ptr(), d_com.data_ptr(), d_bo.data_ptr(), d_out.data_ptr(), off[B],
                                            d_off.data_ptr(), d_st.data_ptr(), mode=1, stride_blocks=NB, d_context=d_ctx.data_ptr())
        torch.cuda.synchronize()
        assert eng.test_counter(WINDOWS) - w0 == WINDOWS_PER_CALL
        assert bytes(d_out.cpu().numpy()) == raw and bytes(d_com.cpu().numpy()) == b''.join(got[1]) and bytes(d_bo.cpu().numpy()) == b''.join(got[2])
        assert list(struct.unpack('<25Q', bytes(d_off.cpu().numpy()))) == off and bytes(d_st.cpu().numpy()) == bytes(4 * B)
        # the verifier: caller seeds, every proof accepted; a flipped context byte rejects that proof and no other
        w0 = eng.test_counter(WINDOWS)
        assert eng.member_verify_batch_rings(got[1], raw, ids, vseeds=vseeds, offsets=off, context=ctx) == ([1] * B, [0] * B)
        vwindows = eng.test_counter(WINDOWS) - w0
        print('windows per mixed verify call:', vwindows)
        assert vwindows == WINDOWS_PER_CALL
        flipped = {3: 0, 10: 31, 17: 13, 22: 7}
        bad = [c if b not in flipped else c[:flipped[b]] + bytes([c[flipped[b]] ^ 0x10]) + c[flipped[b] + 1:] for b, c in enumerate(ctx)]
        want = [0 if b in flipped else 1 for b in range(B)]
        assert eng.member_verify_batch_rings(got[1], raw, ids, vseeds=vseeds, offsets=off, context=bad) == (want, [0] * B)
        d_ok, d_vst, d_bad = fill(B), fill(4 * B), up(b''.join(bad))
        for d_c, ok in ((d_ctx, [1] * B), (d_bad, want)):
            eng.member_verify_batch_rings_device(B, d_com.data_ptr(), d_out.data_ptr(), d_off.data_ptr(), d_ids.data_ptr(), d_vs.data_ptr(), d_ok.data_ptr(), d_vst.data_ptr(),
                                                 d_context=d_c.data_ptr())
            torch.cuda.synchronize()
            assert d_ok.cpu().tolist() == ok and bytes(d_vst.cpu().numpy()) == bytes(4 * B)
    finally:
        eng.set_chunk(4096), eng.set_lanes(2)
