"""-m gpu: resident rings and mixed-ring verification (include/zkattest.h: zk_ctx_add_ring, zk_verify_batch_rings).  Several rings stay built on
one context; switching between them rebuilds nothing and proves exactly what a context that was handed that ring with zk_ctx_set_ring proves.
A batch whose proofs name different rings gets, proof by proof, the (ok, status) of zk_verify_batch with that proof's ring active -- and of
the oracle -- through the host and the device entry points, with per-proof levels, in ZKA1P and in hardened mode."""
import ctypes as C
import hashlib

import pytest

pytestmark = pytest.mark.gpu

from zka1_mutants import mutants

S = 5150
RINGS = {'A': 8, 'B': 1000, 'C': 5000}   # n = 3; n = 10 (table E); n = 13 (table E and digit planes)
ZK_E_ARG = 14


def _vseeds(n, tag):
    return b''.join(hashlib.sha256(tag + i.to_bytes(4, 'big')).digest() for i in range(n))


def _params(eng, sec=80):
    nh, tg, th = eng.synth_params(S)
    eng.set_params(nh, tg, th, sec)
    return nh, tg, th


def _workloads(eng, B=4):
    """{name: (ring, msg, sig, pk, which, seeds)}: one synthetic workload per ring (its keys depend on the seed, the key count and B)."""
    return {k: eng.synth_workload(S + i, n, B) for i, (k, n) in enumerate(sorted(RINGS.items()))}


def _oracle(params, ring, nkeys, sec=80):
    import coracle as CO
    o = CO.OracleCtx(*params, sec)
    o.set_ring(ring, nkeys)
    return o


def _off(plist):
    off = (C.c_uint64 * (len(plist) + 1))()
    o = 0
    for b, p in enumerate(plist):
        off[b] = o
        o += len(p)
    off[len(plist)] = o
    return off


def _device(eng, msgs, plist, ids, vs):
    import torch
    B = len(plist)
    dev = 'cuda:0'
    d_msg = torch.frombuffer(bytearray(msgs), dtype=torch.uint8).to(dev)
    d_pr = torch.frombuffer(bytearray(b''.join(plist)), dtype=torch.uint8).to(dev)
    d_off = torch.tensor(list(_off(plist)), dtype=torch.int64).to(dev)
    d_ids = torch.tensor(list(ids), dtype=torch.int32).to(dev)
    d_vs = torch.frombuffer(bytearray(vs), dtype=torch.uint8).to(dev)
    d_ok = torch.zeros(B, dtype=torch.uint8, device=dev)
    d_st = torch.full((B,), -1, dtype=torch.int32, device=dev)
    eng.verify_batch_rings_device(B, d_msg.data_ptr(), d_pr.data_ptr(), d_off.data_ptr(), d_ids.data_ptr(), d_vs.data_ptr(), d_ok.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    return d_ok.cpu().tolist(), d_st.cpu().tolist()


def _per_ring(eng, msgs, plist, ids, vs, resident):
    """What zk_verify_batch answers for every proof with its ring active (ZK_E_ARG for an id that is not resident); the active ring is restored."""
    ok, st = [0] * len(plist), [ZK_E_ARG] * len(plist)
    active = [r for r in resident if eng.ring_info(r)['flags'] & 16]
    for r in resident:
        idx = [i for i, x in enumerate(ids) if x == r]
        if not idx:
            continue
        eng.use_ring(r)
        o, s = eng.verify_batch(b''.join(msgs[32 * i:32 * i + 32] for i in idx), [plist[i] for i in idx], vseeds=b''.join(vs[32 * i:32 * i + 32] for i in idx))
        for j, i in enumerate(idx):
            ok[i], st[i] = o[j], s[j]
    if active:
        eng.use_ring(active[0])
    return ok, st


@pytest.fixture(scope='module')
def setup():
    """One context with A, B and C resident, their honest proofs (4 each, made after use_ring), and the oracle context of every ring."""
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    params = _params(eng)
    W = _workloads(eng)
    ids = {k: eng.add_ring(W[k][0], RINGS[k]) for k in sorted(RINGS)}
    proofs = {}
    for k in ('A', 'B', 'C', 'A'):   # alternating: a ring that was active before is used again, nothing is rebuilt
        eng.use_ring(ids[k])
        ring, msg, sig, pk, which, seeds = W[k]
        p, st = eng.prove_batch(msg, sig, pk, which, seeds=seeds)
        assert st == [0] * 4, (k, st)
        if k in proofs:
            assert p == proofs[k], k
        proofs[k] = p
    orc = {k: _oracle(params, W[k][0], RINGS[k]) for k in RINGS}
    yield Z, eng, params, W, ids, proofs, orc
    eng.close()


def test_resident_rings_prove_like_set_ring(setup):
    Z, eng, params, W, ids, proofs, orc = setup
    for k in sorted(RINGS):
        fresh = Z.Engine(0)
        _params(fresh)
        ring, msg, sig, pk, which, seeds = W[k]
        fresh.set_ring(ring, RINGS[k])
        p, st = fresh.prove_batch(msg, sig, pk, which, seeds=seeds)
        assert st == [0] * 4 and p == proofs[k], k
        fresh.close()
    ring, msg, sig, pk, which, seeds = W['A']   # a sample against the oracle's prover
    exp, est = orc['A'].prove_batch(msg[:64], sig[:128], pk[:128], which[:2], seeds=seeds[:64], nthreads=2)
    assert exp == proofs['A'][:2]
    for k in ('B', 'C'):
        ring, msg, sig, pk, which, seeds = W[k]
        assert orc[k].verify_batch(msg, proofs[k], nthreads=4, vseeds=_vseeds(4, b'o')) == ([1] * 4, [0] * 4), k


def test_switching_never_rebuilds_and_ids_are_not_reused(setup):
    Z, eng, params, W, ids, proofs, orc = setup
    info = {k: eng.ring_info(ids[k]) for k in RINGS}
    assert {k: (v['n_keys'], v['log_n']) for k, v in info.items()} == {'A': (8, 3), 'B': (1000, 10), 'C': (5000, 13)}
    assert info['B']['flags'] & Z.RING_TABLE_E and info['C']['flags'] & Z.RING_DIGIT_PLANES
    for k in ('B', 'C', 'A', 'B'):
        eng.use_ring(ids[k])
        assert eng.ring_info(ids[k])['flags'] & Z.RING_ACTIVE
    assert {k: eng.ring_info(ids[k])['generation'] for k in RINGS} == {k: v['generation'] for k, v in info.items()}
    eng.set_ring(W['B'][0], RINGS['B'])   # rebuilds the active ring (B) in place, under its id
    after = {k: eng.ring_info(ids[k])['generation'] for k in RINGS}
    assert after == {k: info[k]['generation'] + (k == 'B') for k in RINGS}
    with pytest.raises(Z.ZkError) as e:
        eng.drop_ring(ids['B'])   # the active ring
    assert e.value.status == ZK_E_ARG
    extra = eng.add_ring(W['A'][0], RINGS['A'])
    assert extra not in ids.values()
    eng.drop_ring(extra)
    for call in (lambda: eng.use_ring(extra), lambda: eng.drop_ring(extra), lambda: eng.ring_info(extra), lambda: eng.use_ring(12345)):
        with pytest.raises(Z.ZkError) as e:
            call()
        assert e.value.status == ZK_E_ARG
    again = eng.add_ring(W['A'][0], RINGS['A'])
    assert again not in ids.values() and again != extra
    eng.drop_ring(again)
    eng.use_ring(ids['A'])


def _mixed_batch(setup):
    Z, eng, params, W, ids, proofs, orc = setup
    alt = eng.synth_workload(S + 77, 8, 4)[0]   # another ring of 8 keys: same n as A
    alt_id = eng.add_ring(alt, 8)
    dropped = eng.add_ring(alt, 8)
    eng.drop_ring(dropped)
    items = []   # (message, proof, ring id, oracle ring or None)
    for i in range(4):
        for k in ('A', 'B', 'C'):
            items.append((W[k][1][32 * i:32 * i + 32], proofs[k][i], ids[k], k))
    items.append((W['A'][1][:32], proofs['A'][0], alt_id, None))          # wrong ring, same n
    items.append((W['A'][1][:32], proofs['A'][1], ids['C'], 'C'))         # wrong ring, another n
    items.append((W['C'][1][:32], proofs['C'][0], ids['A'], 'A'))
    items.append((W['B'][1][:32], proofs['B'][0], 999, None))            # unknown id
    items.append((W['A'][1][:32], proofs['A'][2], dropped, None))         # dropped id
    for name, j, b in mutants(proofs['A'][:2], 3, S, S)[:60]:
        items.append((W['A'][1][32 * j:32 * j + 32], b, ids['A'], 'A'))
    return alt_id, items


def _check(setup, items, alt_id, vs, oracle_ok=True):
    Z, eng, params, W, ids, proofs, orc = setup
    msgs = b''.join(it[0] for it in items)
    plist = [it[1] for it in items]
    rids = [it[2] for it in items]
    resident = list(ids.values()) + [alt_id]
    want = _per_ring(eng, msgs, plist, rids, vs, resident)
    got = eng.verify_batch_rings(msgs, plist, rids, vseeds=vs)
    assert got == want
    assert _device(eng, msgs, plist, rids, vs) == want
    if oracle_ok:
        for k in RINGS:
            idx = [i for i, it in enumerate(items) if it[3] == k and it[2] in resident]
            o = orc[k].verify_batch(b''.join(items[i][0] for i in idx), [plist[i] for i in idx], nthreads=16, vseeds=b''.join(vs[32 * i:32 * i + 32] for i in idx))
            assert o == ([want[0][i] for i in idx], [want[1][i] for i in idx]), k
    return want


def test_mixed_batch_equals_per_ring_calls_and_the_oracle(setup):
    Z, eng, params, W, ids, proofs, orc = setup
    alt_id, items = _mixed_batch(setup)
    vs = _vseeds(len(items), b'mix')
    ok, st = _check(setup, items, alt_id, vs)
    assert ok[:12] == [1] * 12
    assert (ok[12:17], st[15:17]) == ([0] * 5, [ZK_E_ARG] * 2)
    assert {(1, 0), (0, 0), (0, 10)} <= set(zip(ok, st))
    # one ring, all ids equal: the usual pipeline with that ring bound, identical to zk_verify_batch with it active
    eng.use_ring(ids['A'])
    one = eng.verify_batch_rings(W['C'][1], proofs['C'], [ids['C']] * 4, vseeds=vs[:128])
    assert one == ([1] * 4, [0] * 4)
    assert eng.ring_info(ids['A'])['flags'] & Z.RING_ACTIVE
    eng.drop_ring(alt_id)


@pytest.mark.parametrize('variant', ['levels', 'packed'])
def test_mixed_batch_with_levels_and_packed_wire(setup, variant):
    Z, eng, params, W, ids, proofs, orc = setup
    alt_id = eng.add_ring(eng.synth_workload(S + 77, 8, 4)[0], 8)
    items = []
    if variant == 'levels':
        made = {}
        for lvl in (20, 128):   # 80: the fixture's proofs
            eng.set_params(*params, lvl)
            for k in RINGS:
                eng.use_ring(ids[k])
                ring, msg, sig, pk, which, seeds = W[k]
                p, st = eng.prove_batch(msg, sig, pk, which, seeds=seeds)
                assert st == [0] * 4
                made[(k, lvl)] = p
        eng.set_params(*params, 80)
        eng.set_verify_level(True)
        for i in range(2):
            for lvl in (20, 80, 128):
                for k in ('A', 'B', 'C'):
                    p = proofs[k][i] if lvl == 80 else made[(k, lvl)][i]
                    items.append((W[k][1][32 * i:32 * i + 32], p, ids[k], k))
        items.append((W['B'][1][:32], made[('B', 20)][0], ids['A'], 'A'))
        items.append((W['B'][1][:32], made[('B', 128)][0], 4242, None))
    else:
        eng.set_wire(True)
        for i in range(4):
            for k in ('C', 'A', 'B'):
                items.append((W[k][1][32 * i:32 * i + 32], Z.pack_proof(proofs[k][i]), ids[k], None))
        items.append((W['A'][1][:32], Z.pack_proof(proofs['A'][3]), alt_id, None))
        items.append((W['A'][1][:32], Z.pack_proof(proofs['A'][3]), 31337, None))
    vs = _vseeds(len(items), variant.encode())
    ok, st = _check(setup, items, alt_id, vs, oracle_ok=variant == 'levels')
    if variant == 'levels':
        assert ok == [1] * 18 + [0, 0] and st[-2:] == [0, ZK_E_ARG]
        eng.set_verify_level(False)
    else:
        assert ok == [1] * 12 + [0, 0] and st[-1] == ZK_E_ARG
        eng.set_wire(False)
    eng.drop_ring(alt_id)


def test_hardened_mode_each_ring_with_its_own_digest():
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    nh, th = Z.hardened_h(b'rings')
    _, tg, _ = eng.synth_params(S)
    eng.set_params(nh, tg, th, 80)
    eng.set_mode(Z.MODE_HARDENED)
    ring, msg, sig, pk, which, seeds = eng.synth_workload(S, 8, 4)
    ring2 = ring[:32 * 7] + hashlib.sha256(b'other key').digest()   # A': one key differs
    a = eng.add_ring(ring, 8)
    a2 = eng.add_ring(ring2, 8)
    eng.use_ring(a)
    p, st = eng.prove_batch(msg, sig, pk, which, seeds=seeds)
    assert st == [0] * 4
    ids = [a, a2, a, a2]
    vs = _vseeds(4, b'h')
    got = eng.verify_batch_rings(msg, p, ids, vseeds=vs)
    assert got == _per_ring(eng, msg, p, ids, vs, [a, a2])
    assert got[0] == [1, 0, 1, 0]   # membership over A' fails for every proof
    assert _device(eng, msg, p, ids, vs) == got
    eng.close()


def test_windows_are_cut_and_the_batched_check_runs():
    """chunk 256, one lane: windows of at most 512 proofs, two classes of 520 proofs each -- every class is cut into two windows, and the chunks of
    256 take the batched Tom-256 check (zk_test_counter 2 counts its terms)."""
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    _params(eng)
    eng.set_chunk(256)
    eng.set_lanes(1)
    B = 520
    made, ids = {}, {}
    for k, n in (('A', 600), ('B', 2100)):   # (a synthetic workload's signers are ring members up to the ring's size)
        W = eng.synth_workload(S + 11 + n, n, B)
        ids[k] = eng.add_ring(W[0], n)
        eng.use_ring(ids[k])
        p, st = eng.prove_batch(*W[1:5], seeds=W[5])
        assert st == [0] * B
        made[k] = (W[1], p)
    msgs, plist, rids = [], [], []
    for i in range(B):
        for k in ('A', 'B'):
            msgs.append(made[k][0][32 * i:32 * i + 32])
            plist.append(made[k][1][i])
            rids.append(ids[k])
    plist[5] = plist[5][:-9] + bytes([plist[5][-9] ^ 1]) + plist[5][-8:]
    msgs = b''.join(msgs)
    vs = _vseeds(len(plist), b'win')
    terms = eng.test_counter(2)
    got = eng.verify_batch_rings(msgs, plist, rids, vseeds=vs)
    assert eng.test_counter(2) > terms
    want = [1] * len(plist)
    want[5] = 0
    assert got[0] == want
    assert got == _per_ring(eng, msgs, plist, rids, vs, list(ids.values()))
    assert _device(eng, msgs, plist, rids, vs) == got
    eng.close()


def test_pool_of_two_contexts_on_device_0():
    import zkp_ecdsa_amd as Z
    pool = Z.Pool([0, 0])
    nh, tg, th = pool.engine(0).synth_params(S)
    pool.set_params(nh, tg, th, 80)
    eng = pool.engine(0)
    W = {k: eng.synth_workload(S + n, n, 4) for k, n in (('A', 8), ('B', 1000))}
    ids = {k: pool.add_ring(W[k][0], n) for k, n in (('A', 8), ('B', 1000))}
    assert ids['A'] != ids['B']
    for i in range(2):
        assert pool.engine(i).ring_info(ids['B'])['n_keys'] == 1000
    msgs, plist, rids = [], [], []
    for k in ('A', 'B'):
        pool.use_ring(ids[k])
        p, st = pool.prove_batch(*W[k][1:5], seeds=W[k][5])
        assert st == [0] * 4
        for i in range(4):
            msgs.append(W[k][1][32 * i:32 * i + 32])
            plist.append(p[i])
            rids.append(ids[k])
    plist.append(plist[0])
    msgs.append(msgs[0])
    rids.append(77)
    msgs = b''.join(msgs)
    vs = _vseeds(len(plist), b'pool')
    got = pool.verify_batch_rings(msgs, plist, rids, vseeds=vs)
    assert got == ([1] * 8 + [0], [0] * 8 + [ZK_E_ARG])
    assert got == eng.verify_batch_rings(msgs, plist, rids, vseeds=vs)
    with pytest.raises(Z.ZkError):
        pool.drop_ring(ids['B'])   # active
    pool.use_ring(ids['A'])
    pool.drop_ring(ids['B'])
    pool.close()


def test_key_tables_off_before_add_ring():
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    _params(eng)
    ring, msg, sig, pk, which, seeds = eng.synth_workload(S, 1000, 4)
    with_t = eng.add_ring(ring, 1000)
    eng.set_key_tables(False)
    without = eng.add_ring(ring, 1000)
    assert eng.ring_info(with_t)['flags'] & Z.RING_KEY_TABLES
    assert not eng.ring_info(without)['flags'] & Z.RING_KEY_TABLES
    out = []
    for r in (with_t, without):
        eng.use_ring(r)
        p, st = eng.prove_batch(msg, sig, pk, which, seeds=seeds)
        assert st == [0] * 4
        out.append(p)
    assert out[0] == out[1]
    eng.close()
