"""-m gpu: mixed-ring proving (include/zkattest.h: zk_prove_batch_rings).  A batch whose proofs name different resident rings gets, proof by proof,
the bytes and the status of zk_prove_batch with that proof's ring active -- and of the oracle's prover -- through the host and the device entry
points, in seed and stream mode, in ZKA1P and in hardened mode, through a pool, with and without per-key tables; the output goes unchanged through
zk_verify_batch_rings.  The active ring plays no part and stays as it was."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

S = 6262
RINGS = {'A': 8, 'B': 1000, 'C': 5000}   # n = 3; n = 10 (table E); n = 13 (table E and digit planes): the shapes of test_gpu_rings.py
ZK_E_RNG_EXHAUSTED, ZK_E_BUFFER, ZK_E_ARG = 11, 12, 14
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vseeds(n, tag):
    return b''.join(hashlib.sha256(tag + i.to_bytes(4, 'big')).digest() for i in range(n))


def _params(eng, sec=80):
    nh, tg, th = eng.synth_params(S)
    eng.set_params(nh, tg, th, sec)
    return nh, tg, th


def _cols(items):
    """items: (msg32, sig64, pk64, which, seed32, ring id, ring name or None) -> the arrays of a prove call"""
    return (b''.join(it[0] for it in items), b''.join(it[1] for it in items), b''.join(it[2] for it in items), [it[3] for it in items],
            b''.join(it[4] for it in items), [it[5] for it in items])


def _item(W, i, rid, name):
    ring, msg, sig, pk, which, seeds = W
    return (msg[32 * i:32 * i + 32], sig[64 * i:64 * i + 64], pk[64 * i:64 * i + 64], which[i], seeds[32 * i:32 * i + 32], rid, name)


def _per_ring(eng, items, resident, prove=None):
    """What zk_prove_batch answers for every input with its ring active (ZK_E_ARG and no proof for an id that is not resident); the active ring is
    restored."""
    proofs, st = [None] * len(items), [ZK_E_ARG] * len(items)
    active = [r for r in resident if eng.ring_info(r)['flags'] & 16]
    for r in resident:
        idx = [i for i, it in enumerate(items) if it[5] == r]
        if not idx:
            continue
        eng.use_ring(r)
        msg, sig, pk, which, seeds, _ = _cols([items[i] for i in idx])
        p, s = prove(msg, sig, pk, which, seeds) if prove else eng.prove_batch(msg, sig, pk, which, seeds=seeds)
        for j, i in enumerate(idx):
            proofs[i], st[i] = p[j], s[j]
    if active:
        eng.use_ring(active[0])
    return proofs, st


def _device(eng, items, cap, mode=0, streams=None, stream_blocks=0):
    """zk_prove_batch_rings_device on torch buffers -> (proofs, statuses, offsets)"""
    import torch
    msg, sig, pk, which, seeds, ids = _cols(items)
    B, dev = len(items), 'cuda:0'
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d_msg, d_sig, d_pk, d_rng = up(msg), up(sig), up(pk), up(seeds if streams is None else streams)
    d_which = torch.tensor(which, dtype=torch.int64).to(torch.int32).to(dev)
    d_ids = torch.tensor(ids, dtype=torch.int64).to(torch.int32).to(dev)
    d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_off = torch.full((B + 1,), -1, dtype=torch.int64, device=dev)
    d_st = torch.full((B,), -1, dtype=torch.int32, device=dev)
    eng.prove_batch_rings_device(B, d_msg.data_ptr(), d_sig.data_ptr(), d_pk.data_ptr(), d_which.data_ptr(), d_ids.data_ptr(), d_rng.data_ptr(), d_out.data_ptr(), cap,
                                 d_off.data_ptr(), d_st.data_ptr(), mode=mode, stride_blocks=stream_blocks)
    torch.cuda.synchronize()
    off, st = d_off.cpu().tolist(), d_st.cpu().tolist()
    raw = bytes(d_out[:off[B]].cpu().numpy().tobytes())
    return [raw[off[b]:off[b + 1]] if st[b] == 0 else None for b in range(B)], st, off


@pytest.fixture(scope='module')
def setup():
    """One context with A, B and C resident (B active), one synthetic workload of 4 signatures per ring, and the oracle context of every ring."""
    import coracle as CO
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    params = _params(eng)
    W = {k: eng.synth_workload(S + i, n, 4) for i, (k, n) in enumerate(sorted(RINGS.items()))}
    ids = {k: eng.add_ring(W[k][0], RINGS[k]) for k in sorted(RINGS)}
    eng.use_ring(ids['B'])
    orc = {}
    for k in RINGS:
        orc[k] = CO.OracleCtx(*params, 80)
        orc[k].set_ring(W[k][0], RINGS[k])
    yield Z, eng, params, W, ids, orc
    eng.close()


def _mixed_items(setup):
    Z, eng, params, W, ids, orc = setup
    dropped = eng.add_ring(W['A'][0], 8)
    eng.drop_ring(dropped)
    items = [_item(W[k], i, ids[k], k) for i in range(4) for k in ('A', 'B', 'C')]
    items.append(_item(W['B'], 0, 999, None))            # an id that never existed
    items.append(_item(W['A'], 2, dropped, None))        # a dropped id
    a = _item(W['A'], 1, ids['A'], 'A')
    items.append(a[:3] + (4000,) + a[4:])                # `which` past the 8-key ring's padding: the one-ring call's per-proof ZK_E_ARG
    c = _item(W['C'], 1, ids['C'], 'C')
    items.append(c[:3] + (4000,) + c[4:])                # the same index is inside the 5000-key ring (not the signer's entry: the proof is made, and is no member's)
    b = _item(W['B'], 3, ids['B'], 'B')
    items.append(b[:2] + (b[2][:63] + bytes([b[2][63] ^ 1]),) + b[3:])   # a key that is off the curve
    return items


def test_mixed_batch_equals_per_ring_calls_and_the_oracle(setup):
    Z, eng, params, W, ids, orc = setup
    items = _mixed_items(setup)
    resident = list(ids.values())
    want = _per_ring(eng, items, resident)
    assert want[1][:12] == [0] * 12 and want[1][12:15] == [ZK_E_ARG] * 3 and want[1][15] == 0 and want[1][16] not in (0, ZK_E_ARG), want[1]
    seg, win = eng.test_counter(7), eng.test_counter(8)
    msg, sig, pk, which, seeds, rids = _cols(items)
    got = eng.prove_batch_rings(msg, sig, pk, which, rids, seeds=seeds)
    assert got[1] == want[1]
    assert got[0] == want[0]
    assert (eng.test_counter(7), eng.test_counter(8)) == (seg + 1, win + 3)   # one segment, one window per ring
    cap = sum(len(p) for p in want[0] if p)
    dp, dst, off = _device(eng, items, cap + 64)
    assert (dp, dst) == want
    assert off[0] == 0 and off[-1] == cap
    assert [off[b + 1] - off[b] for b in range(len(items))] == [len(p) if p else 0 for p in want[0]]   # back to back in index order, empty where a status is set
    assert eng.ring_info(ids['B'])['flags'] & Z.RING_ACTIVE   # the active ring is as it was
    for k in RINGS:   # two proofs per ring against the oracle's prover
        idx = [i for i, it in enumerate(items) if it[6] == k][:2]
        m, s_, p_, w_, sd, _ = _cols([items[i] for i in idx])
        exp, est = orc[k].prove_batch(m, s_, p_, w_, seeds=sd, nthreads=2)
        assert est == [0, 0] and exp == [got[0][i] for i in idx], k


def test_output_goes_unchanged_through_verify_batch_rings(setup):
    Z, eng, params, W, ids, orc = setup
    items = _mixed_items(setup)
    msg, sig, pk, which, seeds, rids = _cols(items)
    proofs, st = eng.prove_batch_rings(msg, sig, pk, which, rids, seeds=seeds)
    plist = [p or b'' for p in proofs]
    vs = _vseeds(len(items), b'rt')
    ok, vst = eng.verify_batch_rings(msg, plist, rids, vseeds=vs)
    assert ok[:12] == [1] * 12 and vst[:12] == [0] * 12   # every honest proof verifies under its own ring
    assert ok[12:15] == [0] * 3 and ok[15] == 0 and ok[16] == 0   # no proof; a proof for an entry that is not the signer's; no proof
    for k in RINGS:
        idx = [i for i, it in enumerate(items) if it[6] == k and proofs[i]]
        o = orc[k].verify_batch(b''.join(items[i][0] for i in idx), [proofs[i] for i in idx], nthreads=8, vseeds=b''.join(vs[32 * i:32 * i + 32] for i in idx))
        assert o == ([ok[i] for i in idx], [vst[i] for i in idx]), k


def test_one_class_is_the_plain_call(setup):
    Z, eng, params, W, ids, orc = setup
    ring, msg, sig, pk, which, seeds = W['C']
    eng.use_ring(ids['C'])
    want = eng.prove_batch(msg, sig, pk, which, seeds=seeds)
    eng.use_ring(ids['B'])
    seg, win = eng.test_counter(7), eng.test_counter(8)
    assert eng.prove_batch_rings(msg, sig, pk, which, [ids['C']] * 4, seeds=seeds) == want
    items = [_item(W['C'], i, ids['C'], 'C') for i in range(4)]
    dp, dst, off = _device(eng, items, sum(len(p) for p in want[0]))
    assert (dp, dst) == want
    assert (eng.test_counter(7), eng.test_counter(8)) == (seg, win)   # nothing staged, no window
    assert eng.ring_info(ids['B'])['flags'] & Z.RING_ACTIVE


def test_segments_and_windows_are_cut():
    """chunk 256, one lane, two rings x 520 proofs interleaved, in the test build (the only one that can force a small segment): see
    tests/prove_rings_cut_check.py."""
    import zkp_ecdsa_amd as Z
    th = os.path.join(os.path.dirname(Z.LIB_PATH), 'libzkattest_hip_testhooks.so')
    assert os.path.exists(th), 'the test-hooks build is not there (make -C zkp-ecdsa_amd/csrc testhooks)'
    assert not hasattr(Z.lib(), 'zk_test_set_prove_segment')   # the product library has no such setter
    env = dict(os.environ)
    env['ZKATTEST_LIB'] = th
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'prove_rings_cut_check.py')], env=env, capture_output=True, text=True, timeout=900)
    print(res.stdout[-3000:])
    assert res.returncode == 0 and 'prove_rings_cut_check ok' in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]


def test_stream_mode(setup):
    Z, eng, params, W, ids, orc = setup
    items = [_item(W[k], i, ids[k], k) for i in range(2) for k in ('C', 'A', 'B')] + [_item(W['A'], 3, 4242, None)]
    nblk = 3 + 44 * 80 + 5 * 13 + 64   # enough blocks for the largest ring of the batch
    streams = [b''.join(hashlib.sha256(it[4] + k.to_bytes(8, 'big')).digest() for k in range(nblk)) for it in items]
    by_seed = {it[4]: i for i, it in enumerate(items)}
    msg, sig, pk, which, seeds, rids = _cols(items)
    for blocks in (nblk, 100):   # 100 blocks: every stream runs out -- ZK_E_RNG_EXHAUSTED as in the one-ring call, ZK_E_ARG for the unknown id all the same

        def prove(m, s_, p_, w_, sd):   # the per-ring reference: every input with its own stream
            rows = [streams[by_seed[sd[32 * j:32 * j + 32]]][:32 * blocks] for j in range(len(w_))]
            return eng.prove_batch(m, s_, p_, w_, streams=b''.join(rows), stream_blocks=blocks)

        want = _per_ring(eng, items, list(ids.values()), prove=prove)
        rows = b''.join(r[:32 * blocks] for r in streams)
        got = eng.prove_batch_rings(msg, sig, pk, which, rids, streams=rows, stream_blocks=blocks)
        assert got == want
        assert got[1] == ([0] * 6 if blocks == nblk else [ZK_E_RNG_EXHAUSTED] * 6) + [ZK_E_ARG], got[1]
        cap = sum(len(p) for p in want[0] if p)
        dp, dst, off = _device(eng, items, cap + 64, mode=1, streams=rows, stream_blocks=blocks)
        assert (dp, dst) == want
        if blocks == nblk:   # the seed contract's own stream IS the seed contract
            assert got == eng.prove_batch_rings(msg, sig, pk, which, rids, seeds=seeds)


def test_packed_wire(setup):
    Z, eng, params, W, ids, orc = setup
    items = [_item(W[k], i, ids[k], k) for i in range(2) for k in ('B', 'C', 'A')]
    msg, sig, pk, which, seeds, rids = _cols(items)
    plain = eng.prove_batch_rings(msg, sig, pk, which, rids, seeds=seeds)
    eng.set_wire(True)
    try:
        want = _per_ring(eng, items, list(ids.values()))
        got = eng.prove_batch_rings(msg, sig, pk, which, rids, seeds=seeds)
        assert got == want and got[1] == [0] * 6
        assert got[0] == [Z.pack_proof(p) for p in plain[0]]
        assert eng.verify_batch_rings(msg, got[0], rids, vseeds=_vseeds(6, b'pk')) == ([1] * 6, [0] * 6)
        dp, dst, off = _device(eng, items, sum(len(p) for p in got[0]))
        assert (dp, dst) == want
    finally:
        eng.set_wire(False)


def test_hardened_mode_each_ring_with_its_own_digest():
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    nh, th = Z.hardened_h(b'prove rings')
    _, tg, _ = eng.synth_params(S)
    eng.set_params(nh, tg, th, 80)
    eng.set_mode(Z.MODE_HARDENED)
    W = eng.synth_workload(S, 8, 4)
    ring2 = W[0][:32 * 7] + hashlib.sha256(b'other key').digest()   # A': the last key differs (signers 0..3 are members of both)
    a, a2 = eng.add_ring(W[0], 8), eng.add_ring(ring2, 8)
    items = [_item(W, i, (a, a2)[i & 1], None) for i in range(4)]
    want = _per_ring(eng, items, [a, a2])
    msg, sig, pk, which, seeds, rids = _cols(items)
    got = eng.prove_batch_rings(msg, sig, pk, which, rids, seeds=seeds)   # (no ring is active on this context)
    assert got == want and got[1] == [0] * 4
    vs = _vseeds(4, b'h')
    assert eng.verify_batch_rings(msg, got[0], rids, vseeds=vs) == ([1] * 4, [0] * 4)                  # under its own ring
    assert eng.verify_batch_rings(msg, got[0], [a2, a, a2, a], vseeds=vs)[0] == [0] * 4               # and under no other: the digest is in the challenge
    eng.close()


def test_output_capacity(setup):
    Z, eng, params, W, ids, orc = setup
    items = [_item(W[k], i, ids[k], k) for i in range(2) for k in ('A', 'C')]
    msg, sig, pk, which, seeds, rids = _cols(items)
    want = eng.prove_batch_rings(msg, sig, pk, which, rids, seeds=seeds)
    exact = sum(len(p) for p in want[0])
    with pytest.raises(Z.ZkError) as e:
        eng.prove_batch_rings(msg, sig, pk, which, rids, seeds=seeds, cap=exact - 1)
    assert e.value.status == ZK_E_BUFFER
    assert eng.prove_batch_rings(msg, sig, pk, which, rids, seeds=seeds, cap=exact) == want
    with pytest.raises(Z.ZkError) as e:
        _device(eng, items, exact - 1)
    assert e.value.status == ZK_E_BUFFER
    assert _device(eng, items, exact)[:2] == want
    pinned = Z.PinnedBuffer(exact)   # a page-locked `out`: the segment's bytes cross by DMA
    assert eng.prove_batch_rings(msg, sig, pk, which, rids, seeds=seeds, out=pinned) == want
    pinned.free()


def test_pool_of_two_contexts_on_device_0(setup):
    Z, eng, params, W, ids, orc = setup
    pool = Z.Pool([0, 0])
    pool.set_params(*params, 80)
    pid = {k: pool.add_ring(W[k][0], RINGS[k]) for k in ('A', 'B')}
    items = [_item(W[k], i, pid[k], k) for i in range(4) for k in ('A', 'B')] + [_item(W['A'], 0, 77, None)]
    msg, sig, pk, which, seeds, rids = _cols(items)
    got = pool.prove_batch_rings(msg, sig, pk, which, rids, seeds=seeds)
    single = eng.prove_batch_rings(msg, sig, pk, which, [{pid['A']: ids['A'], pid['B']: ids['B']}.get(r, 77) for r in rids], seeds=seeds)
    assert got == single
    assert got[1] == [0] * 8 + [ZK_E_ARG]
    pool.close()


def test_key_tables_off_beside_on_and_no_active_ring():
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    _params(eng)
    W = eng.synth_workload(S, 1000, 4)
    ring, msg, sig, pk, which, seeds = W
    with_t = eng.add_ring(ring, 1000)
    eng.set_key_tables(False)
    without = eng.add_ring(ring, 1000)
    assert eng.ring_info(with_t)['flags'] & Z.RING_KEY_TABLES and not eng.ring_info(without)['flags'] & Z.RING_KEY_TABLES
    with pytest.raises(Z.ZkError) as e:   # no ring is active: the one-ring call has nothing to prove over
        eng.prove_batch(msg, sig, pk, which, seeds=seeds)
    assert e.value.status == ZK_E_BUFFER
    a = eng.prove_batch_rings(msg, sig, pk, which, [with_t, without, with_t, without], seeds=seeds)
    b = eng.prove_batch_rings(msg, sig, pk, which, [without, with_t, without, with_t], seeds=seeds)
    assert a == b and a[1] == [0] * 4
    assert not any(eng.ring_info(r)['flags'] & Z.RING_ACTIVE for r in (with_t, without))
    eng.use_ring(with_t)
    assert eng.prove_batch(msg, sig, pk, which, seeds=seeds) == a
    eng.close()
