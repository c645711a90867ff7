"""-m gpu: zk_proof_rering_batch_rings -- re-ring with one resident destination ring id per proof.  The contract is parity: where a proof succeeds, its bytes
are what zk_proof_rering_batch writes for that input alone with its ring active and the same seed (checked for every proof of every batch, and against the
oracle splice for one proof per n); the layout is fixed by ids and headers alone, so a proof that fails its opening or its RNG stream keeps a slot of zero
bytes.  Five proofs made on ring A (8 keys) at secLevel 20 with 16-bit combs; rings B, B2 (8 keys, n = 3) and C (20 keys, n = 5) resident, A active.
Helpers: tests/rering_rings_common.py."""
import hashlib
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rering_rings_common as K
from rering_rings_common import E_ARG, E_BAD, E_BUF, E_OPENING, E_RNG, UNKNOWN, gk_size

pytestmark = pytest.mark.gpu
WINDOWS = 13   # zk_test_counter: windows of mixed-ring membership and re-ring calls
CYCLE = ['B', 'C', 'B2', 'C', 'B', 'C', 'B2', 'C', 'B', 'C']


@pytest.fixture(scope='module')
def X():
    x = K.make_fixture()
    # the parity batch, shared: 10 inputs interleaved B, C, B2, C, B, ... with ring A active
    x.bt10 = K.batch(x, CYCLE, b'p10')
    x.digest0 = x.eng.ring_digest()
    x.got10 = K.rings_call(x, x.bt10)
    x.ref10 = K.one_ring(x, x.bt10)
    yield x
    x.eng.close()


def _slot(x, bt, j):
    """the slot of input j where it passes rules 1-3: its head plus a GKProof section of its destination ring's n"""
    return len(bt['proofs'][j]) - gk_size(3) + gk_size(x.n[bt['rings'][j]])


def _patch(p, at, word):
    return p[:at] + word.to_bytes(4, 'big') + p[at + 4:]


def test_parity(X):
    x, eng, bt = X, X.eng, X.bt10
    out, st, off, raw = x.got10
    assert st == [0] * 10 and x.ref10[1] == [0] * 10
    assert out == x.ref10[0]                                     # every proof: the one-ring call's bytes for that input with its ring active
    for j in (0, 1):                                             # one n = 3, one n = 5: the oracle splice
        r = bt['rings'][j]
        assert out[j] == K.oracle_splice(x, bt['proofs'][j], bt['blinders'][j], bt['which'][j], x.keys[r], bt['seeds'][32 * j:32 * j + 32]), j
        assert int.from_bytes(out[j][12:16], 'big') == x.n[r] and int.from_bytes(out[j][4:8], 'big') == len(out[j])
    assert off == [sum(_slot(x, bt, i) for i in range(j)) for j in range(11)] and raw == b''.join(out)
    vs = b''.join(K.h(b'vs', j) for j in range(10))
    assert eng.verify_batch_rings(bt['msg'], out, bt['ids'], vseeds=vs) == ([1] * 10, [0] * 10)
    assert eng.verify_batch_rings(bt['msg'], bt['proofs'], bt['ids'], vseeds=vs)[0] == [0] * 10   # the originals are proofs for none of the targets
    # the active ring is neither read nor changed
    assert eng.ring_info(x.idA)['flags'] & x.Z.RING_ACTIVE and eng.ring_digest() == x.digest0
    assert not any(eng.ring_info(r)['flags'] & x.Z.RING_ACTIVE for r in x.id.values())
    # the device form: the same bytes
    rc, draw, ooff, dst = K.dev(x, bt)
    assert rc == 0 and dst == [0] * 10 and ooff == off and draw[:off[10]] == raw and draw[off[10]:] == b'\x5a' * (len(draw) - off[10])


def test_statuses_between_good_neighbours(X):
    x = X
    bt = K.batch(x, ['B', 'B', 'C', 'B', 'B2', 'B', 'C', 'C', 'B', 'C'], b'st10')
    bt['ids'][1] = UNKNOWN                                       # rule 1
    bt['proofs'][3] = _patch(bt['proofs'][3], 4, len(bt['proofs'][3]) + 4)   # rule 2: a patched header word
    bt['which'][5] = 12                                          # rule 3: ring B holds 8
    bt['which'][6] = 12                                          # ring C holds 32: a legal index with another proof's key -> the opening fails
    assert bt['which'][9] == 12 and bt['rings'][9] == 'C'         # ... and input 9 (proof 4) takes the same index, where its own key lies: it succeeds
    bl = bytearray(bt['blinders'][8])
    bl[31] ^= 1
    bt['blinders'][8] = bytes(bl)                                # rule 4: a wrong blinder
    want = [0, E_ARG, 0, E_BAD, 0, E_ARG, E_OPENING, 0, E_OPENING, 0]
    out, st, off, raw = K.rings_call(x, bt)
    assert st == want
    lens = [0 if want[j] in (E_ARG, E_BAD) else _slot(x, bt, j) for j in range(10)]
    assert off == [sum(lens[:j]) for j in range(11)] and len(raw) == off[10]
    for j in (6, 8):                                             # a reserved slot, all zero bytes
        assert out[j] is None and lens[j] > 0 and raw[off[j]:off[j + 1]] == bytes(lens[j])
    good = [j for j in range(10) if want[j] == 0]
    clean = K.rings_call(x, K.pick(bt, good))
    assert clean[1] == [0] * len(good) and [out[j] for j in good] == clean[0]   # every neighbour: its bytes in a batch without the bad ones
    assert x.eng.verify_batch_rings(K.pick(bt, good)['msg'], clean[0], K.pick(bt, good)['ids']) == ([1] * len(good), [0] * len(good))
    assert x.eng.verify_batch_rings(bt['msg'][32 * 6:32 * 7], [raw[off[6]:off[7]]], [bt['ids'][6]]) == ([0], [E_BAD])   # a zeroed slot to a verifier
    # ZK_RNG_STREAM: 25 blocks per proof hold the 15 draws of n = 3 and exactly the 25 of n = 5; the first block of input 1 (bound for C) is a rejected fill
    sb = K.batch(x, ['B', 'C', 'B2', 'C'], b'stream')
    blocks = 25
    streams = bytearray(b''.join(hashlib.sha256(sb['seeds'][32 * j:32 * j + 32] + k.to_bytes(8, 'big')).digest() for j in range(4) for k in range(blocks)))
    ref = K.rings_call(x, sb)
    got = K.rings_call(x, sb, streams=bytes(streams), stream_blocks=blocks)
    assert ref[1] == [0] * 4 and got[:3] == ref[:3]
    streams[32 * blocks:32 * blocks + 32] = b'\xff' * 32
    out, st, off, raw = K.rings_call(x, sb, streams=bytes(streams), stream_blocks=blocks)
    assert st == [0, E_RNG, 0, 0] and off == ref[2] and raw[off[1]:off[2]] == bytes(_slot(x, sb, 1))
    assert [out[j] for j in (0, 2, 3)] == [ref[0][j] for j in (0, 2, 3)]


def test_buffer_rule(X):
    x = X
    bt = K.batch(x, ['B', 'C', 'B2', 'C', 'B'], b'buf')
    bt['blinders'][1] = bytes(32)                                # fails its opening: its slot is reserved all the same
    need = sum(_slot(x, bt, j) for j in range(5))
    rc, raw, ooff, dst = K.dev(x, bt, cap=need - 1)
    assert rc == E_BUF
    assert raw == b'\x5a' * len(raw) and all(v == 0x5a5a5a5a5a5a5a5a for v in ooff) and all(v == 0x5a5a5a5a for v in dst)
    rc, raw, ooff, dst = K.dev(x, bt, cap=need)
    assert rc == 0 and dst == [0, E_OPENING, 0, 0, 0] and ooff[5] == need and raw[need:] == b'\x5a' * (len(raw) - need)
    ref, rst = K.one_ring(x, bt)
    for j in range(5):
        assert raw[ooff[j]:ooff[j + 1]] == (ref[j] if j != 1 else bytes(_slot(x, bt, 1))), j


def test_in_place(X):
    x, eng = X, X.eng
    first = K.batch(x, ['B', 'B2', 'B', 'B2', 'B'], b'ip1')
    made, st, off1, _ = K.rings_call(x, first)
    assert st == [0] * 5
    swapped = K.batch(x, ['B2', 'B', 'B2', 'B', 'B2'], b'ip2', proofs=made)
    want, wst = K.one_ring(x, swapped)
    assert wst == [0] * 5
    bad = dict(swapped, blinders=list(swapped['blinders']))
    bad['blinders'][3] = bytes(31) + b'\x01'
    rc, raw, ooff, dst = K.dev(x, bad, in_place=True)
    exp = list(want)
    exp[3] = made[3]                                             # a failed proof keeps its bytes
    assert rc == 0 and dst == [0, 0, 0, E_OPENING, 0] and ooff == off1 and raw == b''.join(exp)
    for j in range(5):
        assert exp[j][:-gk_size(3)] == made[j][:-gk_size(3)]     # heads byte-identical
    ok = [j for j in range(5) if j != 3]
    assert eng.verify_batch_rings(K.pick(swapped, ok)['msg'], [exp[j] for j in ok], K.pick(swapped, ok)['ids']) == ([1] * 4, [0] * 4)
    inp, st, off, _ = K.rings_call(x, swapped, in_place=True)   # the host-pointer form's in-place path
    assert st == [0] * 5 and inp == want and off == off1
    # one n = 3 proof bound for C: ZK_E_ARG, nothing written
    mixed = dict(swapped, ids=list(swapped['ids']), which=list(swapped['which']))
    mixed['ids'][2], mixed['which'][2] = x.id['C'], x.idx['C'][2]
    rc, raw, ooff, dst = K.dev(x, mixed, in_place=True)
    assert rc == E_ARG and raw == b''.join(made) and all(v == 0x5a5a5a5a for v in dst) and all(v == 0x5a5a5a5a5a5a5a5a for v in ooff)
    with pytest.raises(x.Z.ZkError) as ei:
        K.rings_call(x, mixed, in_place=True)
    assert ei.value.status == E_ARG
    # a partial overlap: out 64 bytes into proofs
    rc, raw, ooff, dst = K.dev(x, swapped, out_shift=64)
    assert rc == E_ARG and raw[:len(b''.join(made))] == b''.join(made) and all(v == 0x5a5a5a5a for v in dst)


def test_hardened_mode(X):
    x, eng = X, X.eng
    bt = K.batch(x, ['B', 'C', 'B2', 'C', 'B2', 'B'], b'hard')
    eng.set_mode(x.Z.MODE_HARDENED)
    try:
        out, st, off, raw = K.rings_call(x, bt)
        ref, rst = K.one_ring(x, bt)
        assert st == [0] * 6 and rst == [0] * 6 and out == ref
        assert eng.verify_batch_rings(bt['msg'], out, bt['ids']) == ([1] * 6, [0] * 6)
        ids = list(bt['ids'])
        ids[0], ids[2] = ids[2], ids[0]                          # B <-> B2: equal sizes, another digest (and other keys)
        assert eng.verify_batch_rings(bt['msg'], out, ids)[0] == [0, 1, 0, 1, 1, 1]
    finally:
        eng.set_mode(x.Z.MODE_REFERENCE)
    assert eng.verify_batch_rings(bt['msg'], out, bt['ids'])[0] == [0] * 6   # (the statement is part of the challenge)


def test_packed_wire(X):
    x, eng = X, X.eng
    bt = K.batch(x, ['B', 'C', 'B2', 'C', 'B'], b'packed')
    eng.set_wire(True)
    try:
        bt['proofs'] = [x.Z.pack_proof(p) for p in bt['proofs']]
        out, st, off, raw = K.rings_call(x, bt)
        ref, rst = K.one_ring(x, bt)
        assert st == [0] * 5 and rst == [0] * 5 and out == ref
        assert [len(out[j]) - len(bt['proofs'][j]) for j in range(5)] == [gk_size(x.n[r], 33) - gk_size(3, 33) for r in bt['rings']]
        assert eng.verify_batch_rings(bt['msg'], out, bt['ids']) == ([1] * 5, [0] * 5)
    finally:
        eng.set_wire(False)


def test_windows(X):
    x, eng = X, X.eng
    rings = ['B', 'C', 'B', 'B2', 'B', 'C', 'B', 'B2', 'B', 'C', 'B', 'B2', 'B', 'C', 'B', 'B']   # 9 for B, 4 for C, 3 for B2
    bt = K.batch(x, rings, b'win16')
    bt['blinders'][6] = bytes(32)                                # one failed proof in the middle of B's class
    w0 = eng.test_counter(WINDOWS)
    base = K.rings_call(x, bt)
    assert base[1] == [0] * 6 + [E_OPENING] + [0] * 9 and eng.test_counter(WINDOWS) - w0 == 3
    eng.set_chunk(1)                                             # the smallest chunk: windows of 2 x lanes proofs
    try:
        for lanes in (1, 2):
            eng.set_lanes(lanes)
            w0 = eng.test_counter(WINDOWS)
            assert K.rings_call(x, bt) == base, lanes
            cap = 2 * lanes
            assert eng.test_counter(WINDOWS) - w0 == sum(-(-n // cap) for n in (9, 4, 3)) and -(-9 // cap) >= 3 and 9 % cap, lanes
    finally:
        eng.set_lanes(2), eng.set_chunk(4096)
    good = [j for j in range(16) if j != 6]
    assert eng.verify_batch_rings(K.pick(bt, good)['msg'], [base[0][j] for j in good], K.pick(bt, good)['ids']) == ([1] * 15, [0] * 15)


def test_census_edge(X):
    x, eng = X, X.eng
    bt = K.batch(x, [('B', 'C', 'B2')[j % 3] for j in range(256)] + ['C'], b'edge257')
    rc, raw, ooff, dst = K.dev(x, bt)
    assert rc == 0 and dst == [0] * 257
    assert ooff == [sum(_slot(x, bt, i) for i in range(j)) for j in range(258)]
    got = [raw[ooff[j]:ooff[j + 1]] for j in range(257)]
    try:                                                         # engine against engine: the one-ring device calls grouped by ring
        for r in ('B', 'B2', 'C'):
            sel = [j for j in range(257) if bt['rings'][j] == r]
            eng.use_ring(x.id[r])
            rc1, raw1, off1, st1 = K.dev(x, K.pick(bt, sel), call='one')
            assert rc1 == 0 and st1 == [0] * len(sel)
            assert [raw1[off1[k]:off1[k + 1]] for k in range(len(sel))] == [got[j] for j in sel], r
    finally:
        eng.use_ring(x.idA)
    assert eng.verify_batch_rings(bt['msg'], got, bt['ids']) == ([1] * 257, [0] * 257)


def test_one_class(X):
    x, eng = X, X.eng
    bt = K.batch(x, ['B'] * 7, b'one')
    w0 = eng.test_counter(WINDOWS)
    out, st, off, raw = K.rings_call(x, bt)
    assert st == [0] * 7 and eng.test_counter(WINDOWS) == w0     # the caller's arrays, no window
    assert eng.ring_info(x.idA)['flags'] & x.Z.RING_ACTIVE
    assert (out, st) == K.one_ring(x, bt)
    # the call's rule holds without a mix too: a failed proof keeps a zeroed slot
    bt['blinders'][2] = bytes(32)
    out2, st2, off2, raw2 = K.rings_call(x, bt)
    assert st2 == [0, 0, E_OPENING, 0, 0, 0, 0] and off2 == off and raw2[off[2]:off[3]] == bytes(off[3] - off[2])
    assert [out2[j] for j in range(7) if j != 2] == [out[j] for j in range(7) if j != 2]


def test_call_level(X):
    import ctypes as C
    x, eng, Z = X, X.eng, X.Z
    L, hnd = eng.L, eng.h
    bt = K.pick(x.bt10, [0, 1])
    out_off = (C.c_uint64 * 3)(7, 7, 7)
    rng = Z.ZkRng(0, C.cast(C.create_string_buffer(bt['seeds'], 64), C.c_void_p), 0)
    assert L.zk_proof_rering_batch_rings(hnd, 0, None, None, out_off, None, None, None, C.byref(rng), None, 0, out_off, None) == 0 and out_off[0] == 0
    blob = b''.join(bt['proofs'])
    off = (C.c_uint64 * 3)(0, len(bt['proofs'][0]), len(blob))
    w, ids, st = (C.c_uint32 * 2)(*bt['which']), (C.c_uint32 * 2)(*bt['ids']), (C.c_int32 * 2)()
    out = C.create_string_buffer(2 * len(blob))
    args = [hnd, 2, bt['msg'], blob, off, w, ids, b''.join(bt['blinders']), C.byref(rng), out, len(out), out_off, st]
    assert L.zk_proof_rering_batch_rings(*args) == 0 and list(st) == [0, 0] and out.raw[:out_off[2]] == b''.join(x.got10[0][:2])
    for k in (2, 3, 4, 5, 6, 7, 8, 9, 11, 12):                   # every pointer: NULL is ZK_E_ARG
        a = list(args)
        a[k] = None
        assert L.zk_proof_rering_batch_rings(*a) == E_ARG, k
    assert L.zk_proof_rering_batch_rings_device(hnd, 2, None, None, None, None, None, None, C.byref(rng), None, 0, None, None) == E_ARG
    # a failed call and zk_ctx_wipe leave no gathered blinder, seed or stream row behind
    assert eng.test_counter(11) > 0
    with pytest.raises(Z.ZkError) as ei:
        K.rings_call(x, x.bt10, cap=16)
    assert ei.value.status == E_BUF and eng.test_counter(11) == 0
    assert K.rings_call(x, x.bt10) == x.got10 and eng.test_counter(11) > 0
    eng.wipe()
    assert eng.test_counter(11) == 0
    # a second context: no params; params but no resident ring (every proof rule 1); queued streamed jobs
    e2 = Z.Engine(0)
    try:
        with pytest.raises(Z.ZkError) as ei:
            e2.rering_batch_rings(bt['msg'], bt['proofs'], bt['which'], bt['ids'], bt['blinders'], seeds=bt['seeds'], cap=1 << 16)
        assert ei.value.status == E_BUF
        e2.set_comb_bits(16)
        e2.set_params(*x.par, K.SEC)
        none, st = e2.rering_batch_rings(bt['msg'], bt['proofs'], bt['which'], bt['ids'], bt['blinders'], seeds=bt['seeds'], cap=1 << 16)
        assert st == [E_ARG, E_ARG] and none == [None, None] and e2.rering_last_off == [0, 0, 0]
        ring, msg, sig, pk, wh, sd = e2.synth_workload(K.S, 8, 2)
        e2.set_ring(ring, 8)
        buf = Z.PinnedBuffer(e2.proof_max_size() * 2)
        t = e2.prove_submit(msg, sig, pk, wh, sd, buf)
        with pytest.raises(Z.ZkError) as ei:
            e2.rering_batch_rings(bt['msg'], bt['proofs'], bt['which'], bt['ids'], bt['blinders'], seeds=bt['seeds'], cap=1 << 16)
        assert ei.value.status == E_ARG and 'streamed' in str(ei.value)
        e2.prove_wait(t)
    finally:
        e2.close()
