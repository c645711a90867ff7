"""-m gpu: zk_rings_quorum_prove_batch / zk_rings_quorum_verify_batch -- ZKQ1 bundles whose members sit in different resident rings.  The expected bytes are the
recipe's with the `_rings` calls: the 16-byte header, then what prove_batch_rings, prove_key_blinders, proof_key_commitments and distinct_prove_batch give on
the same rows.  secLevel 20 and 16-bit combs as tests/test_gpu_quorum.py.  Two resident rings of different padded size: A (16 keys) and B (64 keys), one
witness per key for A's 16 keys and B's first 16; A's key SHARED is also enrolled in B at index 63.  No ring is active on X.eng; ring A is active on X.act."""
import os
import random
import struct

import pytest

pytestmark = pytest.mark.gpu

SEC, S, NA, NB, NW = 20, 77, 16, 64, 16
SHARED, SHARED_AT = 5, 63   # witness of ring A whose key ring B holds too, and where
PAIR = 744
E_BAD, E_RNG, E_BUF, E_ARG = 10, 11, 12, 14
NONE = 0xFFFFFFFF
GONE = 999                  # an id that is not resident


class Ctx:
    pass


def _engine(x, mode=None, packed=False, par=None, active=None):
    eng = x.Z.Engine(0)
    eng.set_comb_bits(16)
    par = par or x.par
    eng.set_params(par[0], par[1], par[2], SEC)
    if mode is not None:
        eng.set_mode(mode)
    if packed:
        eng.set_wire(1)
    ids = {'A': eng.add_ring(x.ring['A'], NA), 'B': eng.add_ring(x.ring['B'], NB)}
    if x.ids is None:
        x.ids = ids
    assert ids == x.ids   # ids count up alike in every context: one id table serves all engines of this file
    if active:
        eng.use_ring(ids[active])
    return eng


@pytest.fixture(scope='module')
def X():
    import distinct_common as DC
    import zkp_ecdsa_amd as Z
    x = Ctx()
    x.Z, x.DC = Z, DC
    probe = Z.Engine(0)
    x.par = probe.synth_params(S)
    wl = {'A': probe.synth_workload(S, NA, NW), 'B': probe.synth_workload(S + 1, NB, NW)}
    probe.close()
    x.ring = {'A': wl['A'][0], 'B': wl['B'][0]}
    x.wit = {r: [(wl[r][1][32 * b:32 * b + 32], wl[r][2][64 * b:64 * b + 64], wl[r][3][64 * b:64 * b + 64], wl[r][4][b]) for b in range(NW)] for r in 'AB'}
    assert len({w[2] for r in 'AB' for w in x.wit[r]}) == 2 * NW and all(w[3] != SHARED_AT for w in x.wit['B'])   # 32 different keys
    x.ring['B'] = x.ring['B'][:32 * SHARED_AT] + x.wit['A'][SHARED][2][:32] + x.ring['B'][32 * SHARED_AT + 32:]
    x.ids = None
    x.eng = _engine(x)
    x.act = _engine(x, active='A')
    assert x.eng.ring_proof_max_size(x.ids['A']) < x.eng.ring_proof_max_size(x.ids['B'])
    assert not any(x.eng.ring_info(r)['flags'] & Z.RING_ACTIVE for r in x.ids.values())
    yield x
    x.eng.close(), x.act.close()


def _header(total, k):
    return b'ZKQ1' + struct.pack('>III', total, k, 0)


def _rows(x, members):
    """members: (ring, witness) or (ring, witness, ring shown in) -> msg, sig, pk, which, ring ids"""
    msg, sig, pk, which, ids = b'', b'', b'', [], []
    for m in members:
        w = x.wit[m[0]][m[1]]
        shown = m[2] if len(m) > 2 else m[0]
        assert shown == m[0] or (m[0], m[1], shown) == ('A', SHARED, 'B')
        msg, sig, pk = msg + w[0], sig + w[1], pk + w[2]
        which.append(w[3] if shown == m[0] else SHARED_AT)
        ids.append(x.ids[shown])
    return msg, sig, pk, which, ids


def _quorum(q, k, ring=None):
    """k different signers, interleaved over the two rings (or all of `ring`)"""
    return [(ring or 'AB'[(q + i) % 2], (q + i) % NW) for i in range(k)]


def _workload(x, Q, k, name, ring=None):
    P = k * (k - 1) // 2
    return _rows(x, sum((_quorum(q, k, ring) for q in range(Q)), [])) + (x.DC.seeds_for(b'att' + name, Q * k), x.DC.seeds_for(b'pair' + name, Q * P))


def _blinders(eng, seeds):
    bl = eng.prove_key_blinders(seeds=seeds)
    return [bl[32 * b:32 * b + 32] for b in range(len(seeds) // 32)] if isinstance(bl, (bytes, bytearray)) else list(bl)


def _recipe(eng, k, msg, sig, pk, which, ids, seeds, pair_seeds):
    """the `_rings` calls and the header: what a user of a sharded registry builds today"""
    n = len(which)
    Q, P = n // k, k * (k - 1) // 2
    proofs, st = eng.prove_batch_rings(msg, sig, pk, which, ids, seeds=seeds)
    assert list(st) == [0] * n
    bl = _blinders(eng, seeds)
    kx, st = eng.proof_key_commitments(proofs)
    assert st == [0] * n
    key = [pk[64 * m:64 * m + 32] for m in range(n)]
    first = [q * k + i for q in range(Q) for i, _ in eng.distinct_pairs(k)]
    second = [q * k + j for q in range(Q) for _, j in eng.distinct_pairs(k)]
    dp, st = eng.distinct_prove_batch([key[m] for m in first], [kx[m] for m in first], [bl[m] for m in first], [key[m] for m in second], [kx[m] for m in second],
                                      [bl[m] for m in second], seeds=pair_seeds)
    assert st == [0] * (Q * P)
    out = []
    for q in range(Q):
        body = b''.join(proofs[q * k:q * k + k]) + b''.join(dp[q * P:q * P + P])
        out.append(_header(16 + len(body), k) + body)
    return out


def _members(bundle, k):
    P = k * (k - 1) // 2
    pos, out = 16, []
    for _ in range(k):
        ln = int.from_bytes(bundle[pos + 4:pos + 8], 'big')
        out.append(bundle[pos:pos + ln])
        pos += ln
    assert pos == len(bundle) - PAIR * P
    return out, [bundle[pos + PAIR * p:pos + PAIR * p + PAIR] for p in range(P)]


def _honest(x, Q, k, name, eng=None, ring=None):
    w = _workload(x, Q, k, name, ring)
    bundles, st, mst = (eng or x.eng).quorum_prove_batch_rings(k, *w)
    assert st == [0] * Q and mst == [0] * (Q * k)
    return w, bundles


def _flip(b, at):
    return b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]


def _cap(x, k, ids):
    P = k * (k - 1) // 2
    size = {x.ids['A']: x.eng.ring_proof_max_size(x.ids['A']), x.ids['B']: x.eng.ring_proof_max_size(x.ids['B'])}
    return sum(size.get(i, 0) for i in ids) + (len(ids) // k) * (16 + PAIR * P)


# ------------------------------------------------------------------ 1. the bytes are the recipe's
@pytest.mark.parametrize('Q,k', [(5, 3), (3, 2), (2, 5)])
def test_bundles_equal_the_recipe(X, Q, k):
    w, bundles = _honest(X, Q, k, b'rings%d' % k)
    assert set(w[4][:k]) == set(X.ids.values())   # both rings inside one quorum
    assert bundles == _recipe(X.eng, k, *w)
    assert X.eng.quorum_verify_batch_rings(k, w[0], bundles, w[4]) == ([1] * Q, [0] * Q, [NONE] * Q)


@pytest.mark.parametrize('variant', ['hardened', 'packed'])
def test_bundles_equal_the_recipe_in_hardened_mode_and_in_the_packed_layout(X, variant):
    Z, Q, k = X.Z, 5, 3
    if variant == 'hardened':
        nh, th = Z.hardened_h(b'quorum')
        eng = _engine(X, mode=Z.MODE_HARDENED, par=(nh, X.par[1], th))
    else:
        eng = _engine(X, packed=True)
    try:
        w, bundles = _honest(X, Q, k, b'rings3', eng)
        assert bundles == _recipe(eng, k, *w)
        assert bundles != _honest(X, Q, k, b'rings3')[1]
        assert bundles[0][16:20] == (b'ZK1P' if variant == 'packed' else b'ZKA1')
        assert eng.quorum_verify_batch_rings(k, w[0], bundles, w[4]) == ([1] * Q, [0] * Q, [NONE] * Q)
        assert X.eng.quorum_verify_batch_rings(k, w[0], bundles, w[4])[0] == [0] * Q   # another h, another layout
    finally:
        eng.close()


# ------------------------------------------------------------------ 2., 3. one ring id throughout; the active ring
@pytest.mark.parametrize('ring', ['A', 'B'])
def test_one_ring_id_throughout_equals_the_one_ring_call(X, ring):
    """quorum 1 repeats a signer: the statuses agree as well as the bytes; then the verdicts on a tampered and a re-headed bundle"""
    Q, k = 3, 3
    members = _quorum(0, k, ring) + [(ring, 4), (ring, 7), (ring, 4)] + _quorum(2, k, ring)
    w = _rows(X, members) + (X.DC.seeds_for(b'att-one', Q * k), X.DC.seeds_for(b'pair-one', Q * 3))
    one = w[:4] + w[5:]
    X.act.use_ring(X.ids[ring])
    try:
        want = X.act.quorum_prove_batch(k, *one)
        assert want[1] == [0, E_ARG, 0] and want[2] == [0] * 9
        forged = [want[0][0], _flip(want[0][2], 200), _header(len(want[0][2]), k + 1) + want[0][2][16:]]
        msg = w[0][:96] + w[0][192:] + w[0][192:]
        want_v = X.act.quorum_verify_batch(k, msg, forged)
        assert want_v[0] == [1, 0, 0]
    finally:
        X.act.use_ring(X.ids['A'])
    digest = X.act.ring_digest()
    for eng in (X.act, X.eng):   # ring A active (another ring when ring = 'B'), and none
        assert eng.quorum_prove_batch_rings(k, *w) == want
        assert eng.quorum_verify_batch_rings(k, msg, forged, [X.ids[ring]] * 9) == want_v
    assert X.act.ring_digest() == digest and X.act.ring_info(X.ids['A'])['flags'] & X.Z.RING_ACTIVE
    assert not any(X.eng.ring_info(r)['flags'] & X.Z.RING_ACTIVE for r in X.ids.values())


def test_the_active_ring_is_untouched_by_a_mixed_call(X):
    Q, k = 2, 3
    w, bundles = _honest(X, Q, k, b'active')   # on the context with no active ring
    digest = X.act.ring_digest()
    got, st, _ = X.act.quorum_prove_batch_rings(k, *w)
    assert st == [0] * Q and got == bundles
    assert X.act.quorum_verify_batch_rings(k, w[0], bundles, w[4])[0] == [1] * Q
    assert X.act.ring_digest() == digest
    assert X.act.ring_info(X.ids['A'])['flags'] & X.Z.RING_ACTIVE and not X.act.ring_info(X.ids['B'])['flags'] & X.Z.RING_ACTIVE


# ------------------------------------------------------------------ 4., 5. the prover's statuses
def _three(x, middle, name):
    """quorums 0 and 2 honest and mixed, `middle` the members of quorum 1; call(sel) proves the selected quorums under their own seeds"""
    rows = [_rows(x, _quorum(0, 3)), middle, _rows(x, _quorum(3, 3))]
    seeds, pair_seeds = x.DC.seeds_for(b'att' + name, 9), x.DC.seeds_for(b'pair' + name, 9)
    cat = lambda i, sel: sum((rows[q][i] for q in sel), []) if i >= 3 else b''.join(rows[q][i] for q in sel)
    sub = lambda a, sel: b''.join(a[96 * q:96 * q + 96] for q in sel)
    call = lambda sel: x.eng.quorum_prove_batch_rings(3, *[cat(i, sel) for i in range(5)], seeds=sub(seeds, sel), pair_seeds=sub(pair_seeds, sel))
    return call, sub(seeds, [1])


def test_the_same_key_through_two_rings_is_refused(X):
    middle = _rows(X, [('A', SHARED), ('B', 2), ('A', SHARED, 'B')])
    assert middle[4] == [X.ids['A'], X.ids['B'], X.ids['B']] and middle[3][2] == SHARED_AT
    call, seeds = _three(X, middle, b'shared')
    bundles, st, mst = call([0, 1, 2])
    assert st == [0, E_ARG, 0] and mst == [0] * 9 and bundles[1] is None
    alone, st2, _ = call([0, 2])
    assert st2 == [0, 0] and [bundles[0], bundles[2]] == alone
    # the recipe cannot be completed either: both attestations exist and verify, the distinct-key proof of pair (0, 2) does not
    proofs, pst = X.eng.prove_batch_rings(*middle, seeds=seeds)
    assert list(pst) == [0] * 3 and X.eng.verify_batch_rings(middle[0], proofs, middle[4]) == ([1] * 3, [0] * 3)
    bl, (kx, _) = _blinders(X.eng, seeds), X.eng.proof_key_commitments(proofs)
    key = middle[2][:32]
    assert key == middle[2][128:160]
    dp, dst = X.eng.distinct_prove_batch([key], [kx[0]], [bl[0]], [key], [kx[2]], [bl[2]], seeds=X.DC.seeds_for(b'pair-shared', 1))
    assert dst == [E_ARG] and dp == [None]


def test_a_non_resident_id_in_the_prover(X):
    msg, sig, pk, which, ids = _rows(X, [('A', 8), ('B', 9), ('A', 10)])
    middle = (msg, sig, pk, which, [ids[0], GONE, ids[2]])
    call, seeds = _three(X, middle, b'gone')
    bundles, st, mst = call([0, 1, 2])
    assert st == [0, E_ARG, 0] and mst == [0, 0, 0, 0, E_ARG, 0, 0, 0, 0] and bundles[1] is None
    assert mst[3:6] == list(X.eng.prove_batch_rings(*middle, seeds=seeds)[1])
    alone, st2, _ = call([0, 2])
    assert st2 == [0, 0] and [bundles[0], bundles[2]] == alone
    # every id of a call unknown: nothing to stage, every quorum refused
    none = X.eng.quorum_prove_batch_rings(3, msg, sig, pk, which, [GONE] * 3, seeds=seeds, pair_seeds=seeds)
    assert none == ([None], [E_ARG], [E_ARG] * 3)


# ------------------------------------------------------------------ 6., 7., 11. the verifier
@pytest.fixture(scope='module')
def H(X):
    """three honest quorums of three: rings ABA, BAB, ABA"""
    h = Ctx()
    h.k, h.Q = 3, 3
    h.w, h.bundles = _honest(X, h.Q, h.k, b'verify')
    assert h.w[4] == [X.ids[r] for r in 'ABABABABA']
    return h


def test_a_non_resident_id_in_the_verifier(X, H):
    ids = list(H.w[4])
    ids[3 + 2] = GONE
    assert X.eng.quorum_verify_batch_rings(H.k, H.w[0], H.bundles, ids) == ([1, 0, 1], [0, E_ARG, 0], [NONE, 2, NONE])
    assert X.eng.quorum_verify_batch_rings(H.k, H.w[0], H.bundles, H.w[4], want_first_bad=False) == ([1] * 3, [0] * 3, None)
    assert X.eng.quorum_verify_batch_rings(H.k, H.w[0], H.bundles, H.w[4], verifier_seeds=X.DC.seeds_for(b'vseeds', 9))[0] == [1] * 3


@pytest.mark.parametrize('first', [0, 1])
def test_the_wrong_ring_told_to_the_verifier(X, H, first):
    """members `first` and `first + 1` of quorum 1 sit in different rings: with their ids swapped neither key is in the ring named for it"""
    ids = list(H.w[4])
    ids[3 + first], ids[3 + first + 1] = ids[3 + first + 1], ids[3 + first]
    assert ids != H.w[4]
    ok, st, bad = X.eng.quorum_verify_batch_rings(H.k, H.w[0], H.bundles, ids)
    members, _ = _members(H.bundles[1], H.k)
    mok, mst = X.eng.verify_batch_rings(H.w[0][96:192], members, ids[3:6])
    print('verify_batch_rings on the members of quorum 1 with ids %s: ok %s status %s' % (ids[3:6], list(mok), list(mst)))
    assert list(mok)[first] == 0
    assert ok == [1, 0, 1] and bad == [NONE, first, NONE] and st == [0, next((s for s in mst if s), 0), 0]


def test_byte_flips_name_the_member_or_the_pair(X, H):
    k, msg, b = H.k, H.w[0], H.bundles[1]   # members in rings B, A, B
    rnd = random.Random(21)
    members, pairs = _members(b, k)
    starts = [16 + sum(len(m) for m in members[:j]) for j in range(k)]
    assert [m[12:16] for m in members] == [b'\x00\x00\x00\x06', b'\x00\x00\x00\x04', b'\x00\x00\x00\x06']   # the inner headers' n: rings B, A, B
    cases = [(starts[j] + rnd.randrange(32, len(members[j])), j) for j in range(k)]
    cases += [(len(b) - PAIR * (len(pairs) - p) + 600, k + p) for p in range(len(pairs))]
    for at, bad in cases:
        got = X.eng.quorum_verify_batch_rings(k, msg, [H.bundles[0], _flip(b, at), H.bundles[2]], H.w[4])
        assert got[0] == [1, 0, 1] and got[2] == [NONE, bad, NONE], (at, bad, got)
        if bad < k:   # the member's own verdict by the mixed-ring verifier
            m = _flip(members[bad], at - starts[bad])
            assert X.eng.verify_batch_rings(msg[32 * (k + bad):32 * (k + bad + 1)], [m], [H.w[4][k + bad]]) == ([0], [got[1][1]])


# ------------------------------------------------------------------ 8. capacity
def test_capacity_is_exact(X, H):
    import ctypes as C
    k, Q = H.k, H.Q
    ida, idb = X.ids['A'], X.ids['B']
    sa, sb = X.eng.ring_proof_max_size(ida), X.eng.ring_proof_max_size(idb)
    assert X.eng.quorum_proof_max_size_rings(3, [ida, idb, ida]) == 16 + 2 * sa + sb + 3 * PAIR
    assert X.eng.quorum_proof_max_size_rings(2, [idb, idb]) == 16 + 2 * sb + PAIR
    assert X.eng.quorum_proof_max_size_rings(16, [ida, idb] * 8) == 16 + 8 * (sa + sb) + 120 * PAIR
    assert X.eng.quorum_proof_max_size_rings(3, [ida, GONE, ida]) == 0
    assert X.eng.quorum_proof_max_size_rings(1, [ida]) == 0 and X.eng.quorum_proof_max_size_rings(17, [ida] * 17) == 0
    L, n, P = X.eng.L, Q * k, 3
    need = _cap(X, k, H.w[4])
    assert need == Q * (16 + 3 * PAIR) + 5 * sa + 4 * sb
    out = C.create_string_buffer(b'\x5a' * need, need)
    off = (C.c_uint64 * (Q + 1))(*([0x5a5a5a5a] * (Q + 1)))
    st = (C.c_int32 * Q)(*([0x5a5a] * Q))
    mst = (C.c_int32 * n)(*([0x5a5a] * n))
    which, ids = (C.c_uint32 * n)(*H.w[3]), (C.c_uint32 * n)(*H.w[4])
    r1, keep1 = X.eng._rng(n, H.w[5], None, 0)
    r2, keep2 = X.eng._rng(Q * P, H.w[6], None, 0)
    call = lambda cap, ids_, m: L.zk_rings_quorum_prove_batch(X.eng.h, Q, k, H.w[0], H.w[1], H.w[2], which, ids_, C.byref(r1), C.byref(r2), out, cap, off, st, m)
    assert call(need - 1, ids, mst) == E_BUF
    assert out.raw == b'\x5a' * need and list(off) == [0x5a5a5a5a] * (Q + 1) and list(st) == [0x5a5a] * Q and list(mst) == [0x5a5a] * n
    assert call(need, ids, None) == 0   # per_member_status NULL
    assert [out.raw[off[q]:off[q + 1]] for q in range(Q)] == H.bundles and list(st) == [0] * Q
    # a member whose id is not resident counts 0: the sum without ring B's share for member 1
    gone = (C.c_uint32 * n)(*([H.w[4][0], GONE] + H.w[4][2:]))
    assert call(need - sb - 1, gone, mst) == E_BUF
    assert call(need - sb, gone, mst) == 0 and list(st) == [E_ARG, 0, 0] and off[1] == 0
    assert [out.raw[off[q]:off[q + 1]] for q in (1, 2)] == H.bundles[1:]
    # NULL for a required pointer; k outside 2..16; Q = 0; no params
    assert call(need, None, mst) == E_ARG
    assert L.zk_rings_quorum_verify_batch(X.eng.h, Q, k, H.w[0], b''.join(H.bundles), off, None, None, out, st, None) == E_ARG
    for bad_k in (0, 1, 17):
        with pytest.raises(X.Z.ZkError) as e:
            X.eng.quorum_verify_batch_rings(bad_k, H.w[0][:32 * bad_k * 3], H.bundles, [ida] * (3 * bad_k))
        assert e.value.status == E_ARG
    assert X.eng.quorum_prove_batch_rings(k, b'', b'', b'', [], []) == ([], [], [])
    assert X.eng.quorum_verify_batch_rings(k, b'', [], []) == ([], [], [])
    bare = X.Z.Engine(0)
    try:
        assert bare.quorum_proof_max_size_rings(3, [0, 0, 0]) == 0
        with pytest.raises(X.Z.ZkError) as e:
            bare.quorum_verify_batch_rings(k, H.w[0], H.bundles, H.w[4])
        assert e.value.status == E_BUF
    finally:
        bare.close()


# ------------------------------------------------------------------ 9., 10. window edges; the device forms; wipe
@pytest.fixture(scope='module')
def W(X):
    eng = _engine(X)
    yield eng
    eng.close()


@pytest.mark.parametrize('Q,k,chunk,lanes', [(5, 3, 4, 2), (23, 3, 8, 1)])
def test_windows_of_both_rings(X, W, Q, k, chunk, lanes):
    """windows of two quorums (chunk 4 x 2 lanes: 8 members) whose members sit in both rings; 69 members and 69 pairs cross a wave"""
    w, bundles = _honest(X, Q, k, b'window%d' % Q)
    W.set_chunk(chunk), W.set_lanes(lanes)
    try:
        got, st, mst = W.quorum_prove_batch_rings(k, *w)
        assert st == [0] * Q and mst == [0] * (Q * k) and got == bundles
        assert W.quorum_verify_batch_rings(k, w[0], bundles, w[4]) == ([1] * Q, [0] * Q, [NONE] * Q)
        ids = list(w[4])
        ids[-1] = GONE   # the last member of the last window
        assert W.quorum_verify_batch_rings(k, w[0], bundles, ids) == ([1] * (Q - 1) + [0], [0] * (Q - 1) + [E_ARG], [NONE] * (Q - 1) + [k - 1])
    finally:
        W.set_chunk(4096), W.set_lanes(2)


def _up(b, tail=16):
    import torch
    return torch.frombuffer(bytearray(bytes(b) + bytes(tail)), dtype=torch.uint8).to(torch.device('cuda:0'))


def test_device_forms_on_torch_buffers(X, H):
    import numpy as np
    import torch
    k, Q = H.k, H.Q
    msg, sig, pk, which, ids, seeds, pair_seeds = H.w
    cap = _cap(X, k, ids)
    u32 = lambda v: struct.pack('<%dI' % len(v), *v)
    d = [_up(msg), _up(sig), _up(pk), _up(u32(which)), _up(u32(ids)), _up(seeds), _up(pair_seeds)]
    ptr = [t.data_ptr() for t in d]
    fill = lambda nbytes: torch.full((nbytes,), 0x5a, dtype=torch.uint8, device='cuda:0')
    d_out, d_off, d_st, d_mst = fill(cap + 64), fill(8 * (Q + 1) + 16), fill(4 * Q + 16), fill(4 * Q * k + 16)
    torch.cuda.synchronize()
    with pytest.raises(X.Z.ZkError) as e:   # one byte short: refused from the ids alone, nothing written
        X.eng.quorum_prove_batch_rings_device(Q, k, *ptr, d_out.data_ptr(), cap - 1, d_off.data_ptr(), d_st.data_ptr(), d_mst.data_ptr())
    assert e.value.status == E_BUF
    for t in (d_out, d_off, d_st, d_mst):
        assert bytes(t.cpu().numpy()) == b'\x5a' * t.numel()
    X.eng.quorum_prove_batch_rings_device(Q, k, *ptr, d_out.data_ptr(), cap, d_off.data_ptr(), d_st.data_ptr(), d_mst.data_ptr())
    torch.cuda.synchronize()
    off = np.frombuffer(bytes(d_off.cpu().numpy())[:8 * (Q + 1)], dtype=np.uint64)
    out = bytes(d_out.cpu().numpy())
    assert [out[int(off[q]):int(off[q + 1])] for q in range(Q)] == H.bundles
    assert out[int(off[Q]):int(off[Q]) + 64] == b'\x5a' * 64 and out[cap:] == b'\x5a' * 64
    assert bytes(d_st.cpu().numpy()) == bytes(4 * Q) + b'\x5a' * 16 and bytes(d_mst.cpu().numpy()) == bytes(4 * Q * k) + b'\x5a' * 16
    assert bytes(d_off.cpu().numpy())[8 * (Q + 1):] == b'\x5a' * 16
    # the verifier on device buffers: a tampered pair, a tampered header, an id that is not resident
    bundles = [H.bundles[0], _flip(H.bundles[1], len(H.bundles[1]) - 100), _header(len(H.bundles[2]), k + 1) + H.bundles[2][16:]]
    vids = [GONE] + ids[1:]
    host = X.eng.quorum_verify_batch_rings(k, msg, bundles, vids)
    assert host == ([0, 0, 0], [E_ARG, 0, E_BAD], [0, k + 2, 0])
    offs = [0]
    for b in bundles:
        offs.append(offs[-1] + len(b))
    d_b, d_boff, d_seeds, d_vids = _up(b''.join(bundles), 0), _up(struct.pack('<%dQ' % (Q + 1), *offs), 0), _up(X.DC.seeds_for(b'dv', Q * k), 0), _up(u32(vids))
    for vs, fb in ((None, True), (d_seeds.data_ptr(), False)):
        d_ok, d_vst, d_bad = fill(Q + 8), fill(4 * Q + 16), fill(4 * Q + 16)
        torch.cuda.synchronize()
        X.eng.quorum_verify_batch_rings_device(Q, k, ptr[0], d_b.data_ptr(), d_boff.data_ptr(), d_vids.data_ptr(), vs, d_ok.data_ptr(), d_vst.data_ptr(),
                                               d_bad.data_ptr() if fb else None)
        torch.cuda.synchronize()
        ok, vst, bad = bytes(d_ok.cpu().numpy()), bytes(d_vst.cpu().numpy()), bytes(d_bad.cpu().numpy())
        assert list(ok[:Q]) == host[0] and ok[Q:] == b'\x5a' * 8
        assert list(np.frombuffer(vst[:4 * Q], dtype=np.int32)) == host[1] and vst[4 * Q:] == b'\x5a' * 16
        assert bad == (struct.pack('<%dI' % Q, *host[2]) + b'\x5a' * 16 if fb else b'\x5a' * (4 * Q + 16))
    # misaligned pointers are refused: the ids of either call, another array of either call
    for shift in ({4: 2}, {0: 1}):
        p2 = [p + shift.get(i, 0) for i, p in enumerate(ptr)]
        with pytest.raises(X.Z.ZkError) as e:
            X.eng.quorum_prove_batch_rings_device(Q, k, *p2, d_out.data_ptr(), cap, d_off.data_ptr(), d_st.data_ptr(), d_mst.data_ptr())
        assert e.value.status == E_ARG
    for m, i in ((1, 0), (0, 2)):
        with pytest.raises(X.Z.ZkError) as e:
            X.eng.quorum_verify_batch_rings_device(Q, k, ptr[0] + m, d_b.data_ptr(), d_boff.data_ptr(), d_vids.data_ptr() + i, None, d_ok.data_ptr(), d_vst.data_ptr(), None)
        assert e.value.status == E_ARG
    # Q = 0: ZK_OK, out_off[0] = 0, nothing else touched
    d_off0 = fill(24)
    torch.cuda.synchronize()
    X.eng.quorum_prove_batch_rings_device(0, k, None, None, None, None, None, ptr[5], ptr[6], None, 0, d_off0.data_ptr(), None, None)
    X.eng.quorum_verify_batch_rings_device(0, k, None, None, None, None, None, None, None, None)
    torch.cuda.synchronize()
    assert bytes(d_off0.cpu().numpy()) == bytes(8) + b'\x5a' * 16


def test_timing_families(X, H):
    X.eng.set_timing(1)
    try:
        X.eng.quorum_prove_batch_rings(H.k, *H.w)
        names = set(X.eng.last_timing()[1])
        assert {'quorum_blinders', 'quorum_gather', 'quorum_layout', 'distinct_respond'} <= names, names
        X.eng.quorum_verify_batch_rings(H.k, H.w[0], H.bundles, H.w[4])
        names = set(X.eng.last_timing()[1])
        assert {'quorum_walk', 'quorum_verdict', 'distinct_parse', 'distinct_short', 'distinct_long'} <= names, names
        import torch
        msg, sig, pk, which, ids, seeds, pair_seeds = H.w
        u32 = lambda v: struct.pack('<%dI' % len(v), *v)
        d = [_up(a) for a in (msg, sig, pk, u32(which), u32(ids), seeds, pair_seeds)]
        cap = _cap(X, H.k, ids)
        res = [torch.zeros(n, dtype=torch.uint8, device='cuda:0') for n in (cap + 64, 8 * (H.Q + 1), 4 * H.Q)]
        torch.cuda.synchronize()
        X.eng.quorum_prove_batch_rings_device(H.Q, H.k, *[t.data_ptr() for t in d], res[0].data_ptr(), cap, res[1].data_ptr(), res[2].data_ptr(), None)
        assert 'quorum_caps' in X.eng.last_timing()[1]
    finally:
        X.eng.set_timing(0)


def test_wipe_and_a_failed_call_leave_no_nonzero_word(X, H, W):
    """zk_test_counter 11 counts the nonzero words of every witness-flagged buffer: the quorum staging, the staged inputs, the mixed-ring prover's windows"""
    assert W.quorum_prove_batch_rings(H.k, *H.w)[0] == H.bundles
    assert 0 < W.test_counter(11) < 1 << 63
    W.wipe()
    assert W.test_counter(11) == 0
    assert W.quorum_prove_batch_rings(H.k, *H.w)[0] == H.bundles
    assert W.test_counter(11) > 0
    with pytest.raises(X.Z.ZkError) as e:   # a failed call wipes by itself
        W.quorum_prove_batch_rings(H.k, *H.w, cap=1000)
    assert e.value.status == E_BUF and W.test_counter(11) == 0
    assert W.quorum_prove_batch_rings(H.k, *H.w)[0] == H.bundles
    # the device form: a call refused behind the capacity kernel (a misaligned array) wipes as well
    import torch
    msg, sig, pk, which, ids, seeds, pair_seeds = H.w
    u32 = lambda v: struct.pack('<%dI' % len(v), *v)
    d = [_up(a) for a in (msg, sig, pk, u32(which), u32(ids), seeds, pair_seeds)]
    cap = _cap(X, H.k, ids)
    res = [torch.zeros(n, dtype=torch.uint8, device='cuda:0') for n in (cap + 64, 8 * (H.Q + 1), 4 * H.Q)]
    torch.cuda.synchronize()
    ptr = [t.data_ptr() for t in d]
    W.quorum_prove_batch_rings_device(H.Q, H.k, *ptr, res[0].data_ptr(), cap, res[1].data_ptr(), res[2].data_ptr(), None)
    assert W.test_counter(11) > 0
    with pytest.raises(X.Z.ZkError) as e:
        W.quorum_prove_batch_rings_device(H.Q, H.k, ptr[0] + 1, *ptr[1:], res[0].data_ptr(), cap, res[1].data_ptr(), res[2].data_ptr(), None)
    assert e.value.status == E_ARG and W.test_counter(11) == 0
