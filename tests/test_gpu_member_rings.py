"""gpu: membership proofs with one resident ring id per proof (include/zkattest.h: zk_member_prove_batch_rings / zk_member_verify_batch_rings).  The
contract is parity: every (proof, com, blinder, status) and every (ok, status) of a mixed batch is what the one-ring entry point gives for that input with
that ring active -- checked for every proof of every batch here, and against the Python oracle (member_common) for four proofs per ring.  Three rings of
different n (5, 17 and 300 values: n = 3, 5, 9) and a second ring of 5 values; host and device pointers; engine-drawn and caller blinders, seed and stream
RNG; the window plan at its smallest chunk; a census workgroup's edge; the verifier's refusals by slot geometry; the call-level refusals; wiping."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import member_common as M

pytestmark = pytest.mark.gpu
ZK_E_BAD_ENCODING, ZK_E_BUFFER, ZK_E_ARG = 10, 12, 14
RING17 = M.ring_values(b'ring17', 17)    # N = 32, n = 5
RING5B = M.ring_values(b'ring5b', 5)     # a second ring of n = 3
UNKNOWN = 0x7fff0000                     # an id no context hands out
WINDOWS = 13                             # zk_test_counter: windows of mixed-ring membership calls


@pytest.fixture(scope='module')
def env():
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    nh, tg, th = eng.synth_params(M.PARAM_SEED)
    eng.set_params(nh, tg, th, 80)
    e = {'Z': Z, 'eng': eng, 'params': M.oracle_params(tg, th)}
    e['r5'] = eng.add_ring(M.ring_bytes(M.RING5), 5)
    e['r300'] = eng.add_ring(M.ring_bytes(M.RING300), 300)
    e['r17'] = eng.add_ring(M.ring_bytes(RING17), 17)
    e['r5b'] = eng.add_ring(M.ring_bytes(RING5B), 5)
    e['values'] = {e['r5']: M.RING5, e['r300']: M.RING300, e['r17']: RING17, e['r5b']: RING5B}
    e['size'] = {e['r5']: 1200, e['r300']: 3504, e['r17']: 1968, e['r5b']: 1200, UNKNOWN: 0}
    yield e
    eng.close()


def _shape24(env):
    """B = 24: ids cycle over the three rings, index 13 carries an id that is not resident.  Per ring, in order: the first key, the last key, a padding
    index, an index >= N, then keys 1, 2, ..."""
    per = {env['r5']: [0, 4, 5, 8, 1, 2, 3, 6], env['r17']: [0, 16, 17, 32, 1, 2, 3, 31], env['r300']: [0, 299, 300, 512, 1, 2, 3, 511]}
    cyc, seen, ids, which = [env['r5'], env['r300'], env['r17']], {}, [], []
    for b in range(24):
        r = cyc[b % 3]
        j = seen.get(r, 0)
        seen[r] = j + 1
        ids.append(UNKNOWN if b == 13 else r), which.append(per[r][j])
    return ids, which


def _per_ring(env, ids, which, run):
    """the one-ring entry point, ring by ring: run(ring id, batch indices) -> a tuple of per-proof lists; returns the per-proof tuples in batch order (None
    where the id is not resident)"""
    eng, got = env['eng'], [None] * len(ids)
    for r in sorted(set(ids) - {UNKNOWN}):
        idx = [b for b in range(len(ids)) if ids[b] == r]
        eng.use_ring(r)
        out = run(r, idx)
        for k, b in enumerate(idx):
            got[b] = tuple(col[k] for col in out)
    return got


def _cut(buf, idx, w):
    return b''.join(buf[w * b:w * (b + 1)] for b in idx)


def _check_against_one_ring(env, ids, which, got, seeds=None, blinders=None, streams=None, stream_blocks=0):
    eng = env['eng']
    ref = _per_ring(env, ids, which, lambda r, idx: eng.member_prove_batch(
        [which[b] for b in idx], blinders=_cut(blinders, idx, 32) if blinders is not None else None, seeds=_cut(seeds, idx, 32) if seeds is not None else None,
        streams=_cut(streams, idx, 32 * stream_blocks) if streams is not None else None, stream_blocks=stream_blocks))
    proofs, coms, bl, st = got
    for b in range(len(ids)):
        if ids[b] == UNKNOWN:
            assert (proofs[b], coms[b], bl[b], st[b]) == (None, bytes(72), bytes(32), ZK_E_ARG), b
        else:
            assert (proofs[b], coms[b], bl[b], st[b]) == ref[b], b
    return ref


@pytest.fixture(scope='module')
def batch24(env):
    """the interleaved batch, proved on a context on which no ring has been made active yet; shared by the prover's and the verifier's tests"""
    eng, Z = env['eng'], env['Z']
    assert not any(eng.ring_info(r)['flags'] & Z.RING_ACTIVE for r in env['values'])
    ids, which = _shape24(env)
    seeds = M.seeds_for(b'mr24', 24)
    w0 = eng.test_counter(WINDOWS)
    got = eng.member_prove_batch_rings(which, ids, seeds=seeds)
    return {'ids': ids, 'which': which, 'seeds': seeds, 'got': got, 'off': list(eng.member_last_off), 'raw': eng.member_last_raw, 'windows': eng.test_counter(WINDOWS) - w0}


def test_interleaved_batch_equals_the_one_ring_calls_and_the_oracle(env, batch24):
    eng, Z = env['eng'], env['Z']
    ids, which, seeds, got, off = (batch24[k] for k in ('ids', 'which', 'seeds', 'got', 'off'))
    proofs, coms, bl, st = got
    assert batch24['windows'] == 3   # one window per ring at the default plan
    # layout: the prefix sum of the sizes, an empty slot for the id that is not resident, zeroed slots where the status is not 0
    assert [eng.member_proof_size(r) for r in (env['r5'], env['r17'], env['r300'], UNKNOWN)] == [1200, 1968, 3504, 0]
    run = 0
    for b in range(24):
        assert off[b] == run, b
        run += env['size'][ids[b]]
    assert off[24] == run == len(batch24['raw'])
    assert st[13] == ZK_E_ARG and off[14] == off[13] and coms[13] == bytes(72) and bl[13] == bytes(32)
    for b in range(24):
        want = ZK_E_ARG if ids[b] == UNKNOWN or which[b] >= 2 ** (len(env['values'][ids[b]]) - 1).bit_length() else 0
        assert st[b] == want, b
        if st[b]:
            assert proofs[b] is None and batch24['raw'][off[b]:off[b + 1]] == bytes(off[b + 1] - off[b])
    assert sum(1 for s in st if s == ZK_E_ARG) == 4
    _check_against_one_ring(env, ids, which, got, seeds=seeds)
    # the oracle: the first key, the last key, a padding index and one more key of every ring
    done = {}
    for b in range(24):
        r = ids[b]
        if r == UNKNOWN or st[b] or done.get(r, 0) == 4:
            continue
        done[r] = done.get(r, 0) + 1
        ref = M.oracle_prove(env['params'], env['values'][r], which[b], M.R.SeedRng(seeds[32 * b:32 * b + 32]))
        assert (proofs[b], coms[b], bl[b]) == ref, b
        assert M.oracle_verify(env['params'], env['values'][r], coms[b], proofs[b]), b
    assert done == {env['r5']: 4, env['r17']: 4, env['r300']: 4}
    # with a ring active: the same bytes, and the active ring is neither changed nor rebuilt
    eng.use_ring(env['r17'])
    info = {r: eng.ring_info(r) for r in env['values']}
    assert eng.member_prove_batch_rings(which, ids, seeds=seeds) == got
    assert {r: eng.ring_info(r) for r in env['values']} == info and info[env['r17']]['flags'] & Z.RING_ACTIVE
    assert eng.member_proof_size() == 1968


def test_caller_blinders_and_stream_mode(env, batch24):
    eng = env['eng']
    ids, which = batch24['ids'], batch24['which']
    bl = [int.from_bytes(M.tag(b'mrblind', b), 'big') % M.Q for b in range(24)]
    bl[4] = M.Q + 777   # >= q: reduced as newScalar does
    blb = b''.join(v.to_bytes(32, 'big') for v in bl)
    seeds = M.seeds_for(b'mr24b', 24)
    got = eng.member_prove_batch_rings(which, ids, blinders=blb, seeds=seeds)
    _check_against_one_ring(env, ids, which, got, seeds=seeds, blinders=blb)
    assert got[2][4] == (777).to_bytes(32, 'big') and got[2][5] == blb[32 * 5:32 * 6]
    ref = M.oracle_prove(env['params'], M.RING300, which[4], M.R.SeedRng(seeds[32 * 4:32 * 5]), blinder=bl[4])
    assert ids[4] == env['r300'] and (got[0][4], got[1][4], got[2][4]) == ref
    # ZK_RNG_STREAM: one row of 56 fills per proof (1 + 5 n = 46 for the largest ring, and room for rejected ones)
    nb = 56
    rows = []
    for b in range(24):
        src = M.R.SeedRng(M.tag(b'mrstream', b))
        rows.append(b''.join(src.fill(32) for _ in range(nb)))
    streams = b''.join(rows)
    for blinders in (None, blb):
        got = eng.member_prove_batch_rings(which, ids, blinders=blinders, streams=streams, stream_blocks=nb)
        _check_against_one_ring(env, ids, which, got, blinders=blinders, streams=streams, stream_blocks=nb)
        assert sum(1 for s in got[3] if s == 0) == 20


def test_window_plan_does_not_change_a_byte(env, batch24):
    eng = env['eng']
    ids, which, seeds, got = (batch24[k] for k in ('ids', 'which', 'seeds', 'got'))
    eng.set_chunk(1)   # the smallest chunk: windows of 2 x lanes proofs
    try:
        for lanes in (1, 2):
            eng.set_lanes(lanes)
            w0 = eng.test_counter(WINDOWS)
            assert eng.member_prove_batch_rings(which, ids, seeds=seeds) == got, lanes
            assert eng.member_last_off == batch24['off']
            assert eng.test_counter(WINDOWS) - w0 == sum(-(-n // (2 * lanes)) for n in (8, 8, 7)) > 3, lanes
            ok, vst = eng.member_verify_batch_rings(got[1], batch24['raw'], ids, offsets=batch24['off'], vseeds=M.seeds_for(b'mrv', 24))
            assert ok == [1 if s == 0 else 0 for s in got[3]], lanes
    finally:
        eng.set_lanes(2), eng.set_chunk(4096)


def test_census_workgroup_edge_one_class_unknown_only_and_empty(env):
    eng = env['eng']
    # 257 proofs: 256 of the 5-value ring fill one census workgroup, the one proof of the 17-value ring stands alone in the second
    ids = [env['r5']] * 256 + [env['r17']]
    which = [b % 8 for b in range(256)] + [16]
    seeds = M.seeds_for(b'mr257', 257)
    w0 = eng.test_counter(WINDOWS)
    got = eng.member_prove_batch_rings(which, ids, seeds=seeds)
    assert eng.test_counter(WINDOWS) - w0 == 2 and got[3] == [0] * 257
    assert eng.member_last_off == [1200 * b for b in range(257)] + [1200 * 256 + 1968]
    _check_against_one_ring(env, ids, which, got, seeds=seeds)
    ok, vst = eng.member_verify_batch_rings(got[1], got[0], ids)
    assert ok == [1] * 257 and vst == [0] * 257
    # one class: the one-ring pipeline, no window
    w0 = eng.test_counter(WINDOWS)
    one = eng.member_prove_batch_rings(which[:9], [env['r5']] * 9, seeds=seeds[:32 * 9])
    assert tuple(col[:9] for col in got) == one and eng.member_last_off == [1200 * b for b in range(10)]
    assert eng.member_verify_batch_rings(one[1], one[0], [env['r5']] * 9) == ([1] * 9, [0] * 9)
    assert eng.test_counter(WINDOWS) == w0
    # ids that are not resident only; an empty batch
    none = eng.member_prove_batch_rings([0, 1, 2], [UNKNOWN, UNKNOWN + 1, UNKNOWN], seeds=seeds[:96])
    assert none == ([None] * 3, [bytes(72)] * 3, [bytes(32)] * 3, [ZK_E_ARG] * 3) and eng.member_last_off == [0] * 4
    assert eng.member_verify_batch_rings([bytes(72)] * 3, [b''] * 3, [UNKNOWN] * 3) == ([0] * 3, [ZK_E_ARG] * 3)
    assert eng.member_prove_batch_rings([], []) == ([], [], [], []) and eng.member_last_off == [0]
    assert eng.member_verify_batch_rings([], [], []) == ([], [])


def test_device_forms_write_every_output_byte_and_nothing_else(env, batch24):
    import torch
    eng, Z = env['eng'], env['Z']
    ids, which, seeds, got, off, raw = (batch24[k] for k in ('ids', 'which', 'seeds', 'got', 'off', 'raw'))
    dev = torch.device('cuda:0')

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def fill(n, dtype=torch.uint8):
        return torch.full((n,), 0x5a, dtype=dtype, device=dev)
    d_w = torch.tensor(which, dtype=torch.int32, device=dev)
    d_ids = torch.tensor(ids, dtype=torch.int32, device=dev)
    d_seeds = up(seeds)
    total, tail = off[24], 4096
    for cap in (total - 1, total):
        d_com, d_bo, d_out, d_st, d_off = fill(72 * 24), fill(32 * 24), fill(total + tail), fill(24, torch.int32), fill(25, torch.int64)
        args = (24, d_w.data_ptr(), d_ids.data_ptr(), None, d_seeds.data_ptr(), d_com.data_ptr(), d_bo.data_ptr(), d_out.data_ptr(), cap, d_off.data_ptr(), d_st.data_ptr())
        if cap < total:   # one byte short: refused before anything is written
            with pytest.raises(Z.ZkError) as ei:
                eng.member_prove_batch_rings_device(*args)
            assert ei.value.status == ZK_E_BUFFER
            torch.cuda.synchronize()
            for t in (d_com, d_bo, d_out):
                assert bytes(t.cpu().numpy()) == b'\x5a' * t.numel()
            assert d_st.cpu().tolist() == [0x5a] * 24 and d_off.cpu().tolist() == [0x5a] * 25
            continue
        eng.member_prove_batch_rings_device(*args)
        torch.cuda.synchronize()
        out = bytes(d_out.cpu().numpy())
        assert out[:total] == raw and out[total:] == b'\x5a' * tail
        assert bytes(d_com.cpu().numpy()) == b''.join(got[1]) and bytes(d_bo.cpu().numpy()) == b''.join(got[2])
        assert d_st.cpu().tolist() == got[3] and d_off.cpu().tolist() == off
        d_ok, d_vst = fill(24), fill(24, torch.int32)
        eng.member_verify_batch_rings_device(24, d_com.data_ptr(), d_out.data_ptr(), d_off.data_ptr(), d_ids.data_ptr(), None, d_ok.data_ptr(), d_vst.data_ptr())
        torch.cuda.synchronize()
        assert d_ok.cpu().tolist() == [1 if s == 0 else 0 for s in got[3]]
        assert d_vst.cpu().tolist() == [ZK_E_ARG if i == UNKNOWN else ZK_E_BAD_ENCODING if s else 0 for i, s in zip(ids, got[3])]


def test_verifier_gives_the_one_ring_verdicts(env, batch24):
    eng = env['eng']
    ids, got, off, raw = (batch24[k] for k in ('ids', 'got', 'off', 'raw'))
    coms = list(got[1])
    slots = [raw[off[b]:off[b + 1]] for b in range(24)]   # (a zeroed slot where the prover's status is not 0)

    def one_ring(ids_, coms_, slots_, vseeds=None):
        return _per_ring(env, ids_, None, lambda r, idx: eng.member_verify_batch(
            [coms_[b] for b in idx], [slots_[b] for b in idx], vseeds=_cut(vseeds, idx, 32) if vseeds is not None else None))
    vseeds = M.seeds_for(b'mrv24', 24)
    want = one_ring(ids, coms, slots, vseeds)
    want[13] = (0, ZK_E_ARG)
    for vs in (vseeds, None):   # explicit seeds, the engine's own
        ok, st = eng.member_verify_batch_rings(coms, raw, ids, offsets=off, vseeds=vs)
        assert list(zip(ok, st)) == want
    assert sum(ok) == 20 and sorted(set(want)) == [(0, ZK_E_BAD_ENCODING), (0, ZK_E_ARG), (1, 0)]
    # mutants, one per honest proof: a byte of a point, of a scalar, of n, of the magic, of com -- each the one-ring (ok, status)
    good = [b for b in range(24) if got[3][b] == 0]
    m_coms, m_slots, names = list(coms), list(slots), {}
    kinds = ('point', 'scalar', 'n', 'magic', 'com')
    for k, b in enumerate(good[:15]):
        kind = kinds[k % 5]
        n = (len(slots[b]) - 48) // 384
        p, cm = bytearray(slots[b]), bytearray(coms[b])
        if kind == 'point':
            p[16 + 72 * (k % (4 * n)) + 71] ^= 1
        elif kind == 'scalar':
            p[16 + 288 * n + 32 * (k % (3 * n + 1)) + 31] ^= 1
        elif kind == 'n':
            p[11] ^= 1
        elif kind == 'magic':
            p[2] ^= 0x20
        else:
            cm[71] ^= 1
        m_coms[b], m_slots[b], names[b] = bytes(cm), bytes(p), kind
    want = one_ring(ids, m_coms, m_slots, vseeds)
    want[13] = (0, ZK_E_ARG)
    ok, st = eng.member_verify_batch_rings(m_coms, m_slots, ids, vseeds=vseeds)
    assert list(zip(ok, st)) == want
    for b, kind in names.items():
        assert want[b][0] == 0, (b, kind)
    assert {want[b] for b, kind in names.items() if kind == 'scalar'} == {(0, 0)} and {want[b] for b, kind in names.items() if kind == 'magic'} == {(0, ZK_E_BAD_ENCODING)}
    assert all(want[b] == (1, 0) for b in good[15:])


def test_verifier_refuses_by_slot_geometry_and_by_ring(env, batch24):
    eng = env['eng']
    ids, got, off, raw = (batch24[k] for k in ('ids', 'got', 'off', 'raw'))
    r5, r5b, r17 = env['r5'], env['r5b'], env['r17']
    b5 = [b for b in range(24) if ids[b] == r5 and got[3][b] == 0][:2]
    b17 = next(b for b in range(24) if ids[b] == r17 and got[3][b] == 0)
    (pa, ca), (pb, cb), (pc, cc) = ((got[0][b], got[1][b]) for b in (b5[0], b5[1], b17))
    # a proof of the 5-value ring under the 17-value ring's id: the slot is not that ring's size; under another ring of the same n: the relations fail
    ok, st = eng.member_verify_batch_rings([ca, ca, ca, cc, cc], [pa, pa, pa, pc, pc], [r5, r17, r5b, r17, r5])
    assert list(zip(ok, st)) == [(1, 0), (0, ZK_E_BAD_ENCODING), (0, 0), (1, 0), (0, ZK_E_BAD_ENCODING)]
    eng.use_ring(r5b)   # (the one-ring verdict for it)
    assert eng.member_verify_batch([ca], [pa]) == ([0], [0])
    # a misaligned slot and a decreasing offset; ids that are not resident take up the odd bytes between the aligned slots
    blob = bytes(2) + pa + bytes(2) + pb
    offsets = [0, 2, 1202, 1204, 2404, 1204, 2404]
    assert len(blob) == 2404
    ok, st = eng.member_verify_batch_rings([bytes(72), ca, bytes(72), cb, cb, cb], blob, [UNKNOWN, r5, UNKNOWN, r5, r5, r5], offsets=offsets)
    assert list(zip(ok, st)) == [(0, ZK_E_ARG), (0, ZK_E_BAD_ENCODING), (0, ZK_E_ARG), (1, 0), (0, ZK_E_BAD_ENCODING), (1, 0)]
    # an end behind the batch's end, a slot one word short or long
    blob = pa + pb + pa
    cases = [([0, 1200, 3600, 3600], [(1, 0), (0, ZK_E_BAD_ENCODING), (0, ZK_E_BAD_ENCODING)]),
             ([0, 1200, 2396, 3600], [(1, 0), (0, ZK_E_BAD_ENCODING), (0, ZK_E_BAD_ENCODING)]),
             ([0, 1200, 2400, 3600], [(1, 0), (1, 0), (1, 0)])]
    for offsets, want in cases:
        ok, st = eng.member_verify_batch_rings([ca, cb, ca], blob, [r5] * 3, offsets=offsets)
        assert list(zip(ok, st)) == want, offsets
    offsets = (C.c_uint64 * 4)(0, 1200, 4800, 3600)   # proof_off[b + 1] > proof_off[B]
    ok, st, idv = (C.c_uint8 * 3)(), (C.c_int32 * 3)(), (C.c_uint32 * 3)(r5, r5, r5)
    assert eng.L.zk_member_verify_batch_rings(eng.h, 3, ca + cb + ca, blob, offsets, idv, None, ok, st) == 0
    assert list(zip(ok, st)) == [(1, 0), (0, ZK_E_BAD_ENCODING), (0, ZK_E_BAD_ENCODING)]


def test_refusals_and_wipe(env, batch24):
    Z = env['Z']
    eng = env['eng']
    ids, which, seeds, got = (batch24[k] for k in ('ids', 'which', 'seeds', 'got'))
    # a mixed call leaves gathered seeds behind; zk_ctx_wipe zeroes them with everything else that is witness-derived
    assert eng.member_prove_batch_rings(which, ids, seeds=seeds) == got
    assert eng.test_counter(11) > 0
    eng.wipe()
    assert eng.test_counter(11) == 0
    assert eng.member_prove_batch_rings(which, ids, seeds=seeds) == got
    eng.set_mode(Z.MODE_HARDENED)
    try:
        with pytest.raises(Z.ZkError) as ei:
            eng.member_prove_batch_rings(which, ids, seeds=seeds)
        assert ei.value.status == ZK_E_ARG
        with pytest.raises(Z.ZkError) as ei:
            eng.member_verify_batch_rings(got[1], batch24['raw'], ids, offsets=batch24['off'])
        assert ei.value.status == ZK_E_ARG
    finally:
        eng.set_mode(Z.MODE_REFERENCE)
    # NULL arguments
    L, h = eng.L, eng.h
    w, idv, st, off = (C.c_uint32 * 2)(0, 1), (C.c_uint32 * 2)(env['r5'], env['r17']), (C.c_int32 * 2)(), (C.c_uint64 * 3)()
    data = C.create_string_buffer(64)
    rng = Z.ZkRng(0, C.cast(data, C.c_void_p), 0)
    com, out, ok = C.create_string_buffer(144), C.create_string_buffer(4096), (C.c_uint8 * 2)()
    assert L.zk_member_prove_batch_rings(h, 2, w, idv, None, C.byref(rng), com, None, out, 4096, off, st) == 0
    assert L.zk_member_prove_batch_rings(h, 2, w, None, None, C.byref(rng), com, None, out, 4096, off, st) == ZK_E_ARG
    assert L.zk_member_prove_batch_rings(h, 2, None, idv, None, C.byref(rng), com, None, out, 4096, off, st) == ZK_E_ARG
    assert L.zk_member_prove_batch_rings(h, 2, w, idv, None, None, com, None, out, 4096, off, st) == ZK_E_ARG
    assert L.zk_member_prove_batch_rings(h, 2, w, idv, None, C.byref(rng), com, None, out, 4096, None, st) == ZK_E_ARG
    assert L.zk_member_prove_batch_rings(h, 2, w, idv, None, C.byref(rng), com, None, out, 3167, off, st) == ZK_E_BUFFER
    assert L.zk_member_prove_batch_rings_device(h, 2, None, None, None, C.byref(rng), None, None, None, 0, None, None) == ZK_E_ARG
    assert L.zk_member_verify_batch_rings(h, 2, com.raw, out.raw, off, None, None, ok, st) == ZK_E_ARG
    assert L.zk_member_verify_batch_rings(h, 2, com.raw, out.raw, None, idv, None, ok, st) == ZK_E_ARG
    assert L.zk_member_verify_batch_rings_device(h, 2, None, None, None, None, None, None, None) == ZK_E_ARG
    assert L.zk_member_proof_size_ring(None, env['r5']) == 0
    # before zk_ctx_set_params; while a streamed job is queued
    e2 = Z.Engine(0)
    try:
        with pytest.raises(Z.ZkError) as ei:
            e2.member_prove_batch_rings([0], [0], seeds=bytes(32), cap=4096)
        assert ei.value.status == ZK_E_BUFFER
        nh, tg, th = e2.synth_params(M.PARAM_SEED)
        e2.set_params(nh, tg, th, 20)
        ring, msg, sig, pk, wh, sd = e2.synth_workload(7, 8, 2)
        rid = e2.add_ring(ring, 8)
        e2.use_ring(rid)
        p, cm, _, s = e2.member_prove_batch_rings([1, 2], [rid, rid], seeds=seeds[:64])
        assert s == [0, 0]
        buf = Z.PinnedBuffer(e2.proof_max_size() * 2)
        t = e2.prove_submit(msg, sig, pk, wh, sd, buf)
        with pytest.raises(Z.ZkError) as ei:
            e2.member_prove_batch_rings([1, 2], [rid, rid], seeds=seeds[:64])
        assert ei.value.status == ZK_E_ARG and 'streamed' in str(ei.value)
        with pytest.raises(Z.ZkError) as ei:
            e2.member_verify_batch_rings(cm, p, [rid, rid])
        assert ei.value.status == ZK_E_ARG
        _, pst = e2.prove_wait(t)
        assert list(pst) == [0, 0]
        assert e2.member_verify_batch_rings(cm, p, [rid, rid]) == ([1, 1], [0, 0])
        buf.free()
    finally:
        e2.close()
