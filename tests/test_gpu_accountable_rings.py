"""-m gpu: zk_rings_accountable_prove_batch / _verify_batch / _open_batch -- ZKC1 bundles over several resident rings, one ring id per bundle, no active ring.
The expected bytes are the recipe's with the `_rings` calls: the 16-byte header, then what prove_batch_rings, prove_key_blinders, proof_key_commitments and
escrow_prove_batch give on the same rows; the expected verdicts are split + verify_batch_rings + escrow_verify_batch's; the expected openings are split +
escrow_open_batch_rings'.  Shapes as tests/test_gpu_quorum_rings.py: secLevel 20, 16-bit combs, two resident rings A (16 keys) and B (64 keys), 16 witnesses
each, A's key SHARED also enrolled in B at index 63.  No ring is active on X.eng; ring A is active on X.act.  The auditor's key comes from escrow_keygen."""
import hashlib
import struct

import pytest

pytestmark = pytest.mark.gpu

SEC, S, NA, NB, NW = 20, 77, 16, 64, 16
SHARED, SHARED_AT = 5, 63
TAG = 472
E_BAD, E_RNG, E_BUF, E_ARG, E_OPENING = 10, 11, 12, 14, 16
NONE = 0xFFFFFFFF
ANY = 0xFFFFFFFF            # ZK_ESCROW_RING_ANY
GONE = 999                  # an id that is not resident
ATT_BLOCKS = 2048


class Ctx:
    pass


def _engine(x, mode=None, packed=False, par=None, active=None, auditor=True):
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
    assert ids == x.ids
    if active:
        eng.use_ring(ids[active])
    if auditor:
        eng.set_auditor(eng.escrow_keygen(x.a32))
    return eng


@pytest.fixture(scope='module')
def X():
    import accountable_common as AC
    import distinct_common as DC
    import zkp_ecdsa_amd as Z
    x = Ctx()
    x.Z, x.DC, x.AC = Z, DC, AC
    probe = Z.Engine(0)
    x.par = probe.synth_params(S)
    wl = {'A': probe.synth_workload(S, NA, NW), 'B': probe.synth_workload(S + 1, NB, NW)}
    probe.close()
    x.ring = {'A': wl['A'][0], 'B': wl['B'][0]}
    x.wit = {r: [(wl[r][1][32 * b:32 * b + 32], wl[r][2][64 * b:64 * b + 64], wl[r][3][64 * b:64 * b + 64], wl[r][4][b]) for b in range(NW)] for r in 'AB'}
    assert len({w[2] for r in 'AB' for w in x.wit[r]}) == 2 * NW and all(w[3] != SHARED_AT for w in x.wit['B'])
    x.ring['B'] = x.ring['B'][:32 * SHARED_AT] + x.wit['A'][SHARED][2][:32] + x.ring['B'][32 * SHARED_AT + 32:]
    x.a32 = hashlib.sha256(b'accountable-rings auditor').digest()
    x.ids = None
    x.eng = _engine(x)
    x.act = _engine(x, active='A')
    x.size = {i: x.eng.ring_accountable_proof_max_size(i) for i in x.ids.values()}
    assert x.size[x.ids['A']] == 16 + x.eng.ring_proof_max_size(x.ids['A']) + TAG < x.size[x.ids['B']] == 16 + x.eng.ring_proof_max_size(x.ids['B']) + TAG
    assert x.eng.ring_accountable_proof_max_size(GONE) == 0
    assert not any(x.eng.ring_info(r)['flags'] & Z.RING_ACTIVE for r in x.ids.values())
    yield x
    x.eng.close(), x.act.close()


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


def _mixed(B, ring=None):
    """B witnesses interleaved over the two rings (or all of `ring`); beyond 32 the same witnesses again under fresh seeds"""
    return [(ring or 'AB'[b % 2], (b // (1 if ring else 2)) % NW) for b in range(B)]


def _blocks(seeds, b, n):
    return [hashlib.sha256(seeds[32 * b:32 * b + 32] + k.to_bytes(8, 'big')).digest() for k in range(n)]


def _recipe(x, eng, msg, sig, pk, which, ids, att_rng, tag_rng):
    """the `_rings` prover, the three existing calls and the header: what a user of a sharded registry builds today"""
    B = len(which)
    proofs, ast = eng.prove_batch_rings(msg, sig, pk, which, ids, **att_rng)
    assert list(ast) == [0] * B
    bl = eng.prove_key_blinders(**att_rng)
    kx, kst = eng.proof_key_commitments(proofs)
    assert kst == [0] * B
    tags, tst = eng.escrow_prove_batch([pk[64 * b:64 * b + 32] for b in range(B)], kx, bl, **tag_rng)
    assert tst == [0] * B
    return [x.AC.bundle(proofs[b], tags[b]) for b in range(B)]


def _verify_recipe(x, eng, msg, bundles, ids, packed=0, vseeds=None):
    """split (tests/accountable_common.py's) + verify_batch_rings + proof_key_commitments + escrow_verify_batch -> (ok, status, first_bad)"""
    att, tags, sst = x.AC.split(bundles, packed)
    live = [b for b in range(len(bundles)) if sst[b] == 0]
    ok, st, bad = [0] * len(bundles), [E_BAD] * len(bundles), [0] * len(bundles)
    if live:
        a_ok, a_st = eng.verify_batch_rings(b''.join(msg[32 * b:32 * b + 32] for b in live), [att[b] for b in live], [ids[b] for b in live],
                                            None if vseeds is None else b''.join(vseeds[32 * b:32 * b + 32] for b in live))
        kx, _ = eng.proof_key_commitments([att[b] for b in live])
        t_ok, t_st = eng.escrow_verify_batch(kx, [tags[b] for b in live])
        for i, b in enumerate(live):
            a_bad, t_bad = not a_ok[i] or a_st[i] != 0, not t_ok[i] or t_st[i] != 0
            ok[b], st[b], bad[b] = int(not a_bad and not t_bad), a_st[i] or t_st[i], 0 if a_bad else 1 if t_bad else NONE
    return ok, st, bad


def _flags(x, eng):
    return [eng.ring_info(r)['flags'] for r in x.ids.values()]


@pytest.fixture(scope='module')
def H(X):
    """six honest bundles over rings A B A B A B, the shared key last but one (shown in A), shared and left unchanged"""
    h = Ctx()
    h.members = [('A', 1), ('B', 2), ('A', 3), ('B', 4), ('A', SHARED), ('B', 6)]
    h.w = _rows(X, h.members)
    h.B = len(h.members)
    h.seeds, h.tag_seeds = X.DC.seeds_for(b'accr-att', h.B), X.DC.seeds_for(b'accr-tag', h.B)
    flags = _flags(X, X.eng)
    h.bundles, h.st, h.pst = X.eng.accountable_prove_batch_rings(*h.w, seeds=h.seeds, tag_seeds=h.tag_seeds)
    assert h.st == [0] * h.B and h.pst == [(0, 0)] * h.B and _flags(X, X.eng) == flags
    return h


# ------------------------------------------------------------------ 1. the bytes are the recipe's
@pytest.mark.parametrize('B,mode,packed,stream,chunk', [(65, 0, False, False, 4), (3, 1, True, False, None), (3, 0, False, True, None), (1, 1, False, False, None),
                                                        (3, 0, True, True, None), (1, 0, True, False, None), (3, 1, False, False, None), (1, 0, False, False, None),
                                                        (1, 1, True, False, None), (3, 1, False, True, None), (3, 0, False, False, None)])
def test_bundles_equal_the_recipe(X, B, mode, packed, stream, chunk):
    Z = X.Z
    if mode:
        nh, th = Z.hardened_h(b'accountable-rings')
        eng = _engine(X, mode=Z.MODE_HARDENED, packed=packed, par=(nh, X.par[1], th))
    elif packed or chunk:
        eng = _engine(X, packed=packed)
    else:
        eng = X.eng
    try:
        if chunk:
            eng.set_chunk(chunk)   # windows of chunk x lanes bundles: both rings inside every window
        w = _rows(X, _mixed(B))
        assert B < 2 or set(w[4][:2]) == set(X.ids.values())
        name = b'r%d%d%d%d' % (B, mode, packed, stream)
        seeds, tag_seeds = X.DC.seeds_for(b'att' + name, B), X.DC.seeds_for(b'tag' + name, B)
        if stream:
            att_rng = {'streams': b''.join(b''.join(_blocks(seeds, b, ATT_BLOCKS)) for b in range(B)), 'stream_blocks': ATT_BLOCKS}
            tag_rng = {'streams': b''.join(b''.join(_blocks(tag_seeds, b, 4)) for b in range(B)), 'stream_blocks': 4}
            got = eng.accountable_prove_batch_rings(*w, streams=att_rng['streams'], stream_blocks=ATT_BLOCKS, tag_streams=tag_rng['streams'], tag_stream_blocks=4)
            assert eng.accountable_prove_batch_rings(*w, seeds=seeds, tag_seeds=tag_seeds)[0] == got[0]   # block k of a stream = sha256(seed | k)
        else:
            att_rng, tag_rng = {'seeds': seeds}, {'seeds': tag_seeds}
            got = eng.accountable_prove_batch_rings(*w, seeds=seeds, tag_seeds=tag_seeds)
        bundles, st, pst = got
        assert st == [0] * B and pst == [(0, 0)] * B
        want = _recipe(X, eng, *w, att_rng, tag_rng)
        for b in range(B):
            assert bundles[b] == want[b], b
        raw, off = eng.accountable_last_raw
        assert raw == b''.join(bundles) and off[0] == 0 and off[B] == len(raw)
        assert eng.accountable_verify_batch_rings(w[0], bundles, w[4]) == ([1] * B, [0] * B, [NONE] * B)
        assert eng.accountable_verify_batch_rings(w[0], bundles, w[4], want_first_bad=False) == ([1] * B, [0] * B, None)
        ring, idx, ost = eng.accountable_open_batch_rings(X.a32, bundles, w[4])
        assert (ring, idx, ost) == (w[4], w[3], [0] * B)
    finally:
        if eng is not X.eng:
            eng.close()


# ------------------------------------------------------------------ 2. one ring named
def test_one_ring_named_equals_the_one_ring_calls(X):
    B = 5
    w = _rows(X, _mixed(B, 'A'))
    ids = w[4]
    seeds, tag_seeds = X.DC.seeds_for(b'one-att', B), X.DC.seeds_for(b'one-tag', B)
    ff = b'\xff' * 32
    tag_rows = [_blocks(tag_seeds, b, 4) for b in range(B)]
    tag_rows[2] = [ff] + tag_rows[2][:3]   # bundle 2's tag runs out of randomness: statuses and closing up agree too
    tag_streams = b''.join(b''.join(r) for r in tag_rows)
    want = X.act.accountable_prove_batch(*w[:4], seeds=seeds, tag_streams=tag_streams, tag_stream_blocks=4)
    want_raw = X.act.accountable_last_raw
    assert want[1] == [0, 0, E_RNG, 0, 0]
    live = [b for b in want[0] if b is not None]
    forged = [live[0], live[1][:-9] + bytes([live[1][-9] ^ 1]) + live[1][-8:], live[2][:-4], live[3][:200] + bytes([live[3][200] ^ 1]) + live[3][201:]]
    msg = b''.join(w[0][32 * b:32 * b + 32] for b in (0, 1, 3, 4))
    want_v = X.act.accountable_verify_batch(msg, forged)
    assert want_v[0] == [1, 0, 0, 0] and want_v[2] == [NONE, 1, 0, 0]
    for eng in (X.act, X.eng):   # ring A active, and none
        flags = _flags(X, eng)
        assert eng.accountable_prove_batch_rings(*w, seeds=seeds, tag_streams=tag_streams, tag_stream_blocks=4) == want
        assert eng.accountable_last_raw == want_raw
        assert eng.accountable_verify_batch_rings(msg, forged, ids[:4]) == want_v
        assert _flags(X, eng) == flags
    assert X.act.ring_info(X.ids['A'])['flags'] & X.Z.RING_ACTIVE


# ------------------------------------------------------------------ 3. statuses
def test_prover_statuses(X, H):
    eng = X.eng
    # a non-resident id: ZK_E_ARG, an empty slot, the neighbours' bytes unchanged
    ids = list(H.w[4])
    ids[2] = GONE
    got, st, pst = eng.accountable_prove_batch_rings(*H.w[:4], ids, seeds=H.seeds, tag_seeds=H.tag_seeds)
    assert st == [0, 0, E_ARG, 0, 0, 0] and pst[2][0] == E_ARG and [p for i, p in enumerate(pst) if i != 2] == [(0, 0)] * 5
    assert st[2] == list(eng.prove_batch_rings(*H.w[:4], ids, seeds=H.seeds)[1])[2]
    assert got == H.bundles[:2] + [None] + H.bundles[3:]
    raw, off = eng.accountable_last_raw
    assert off[2] == off[3] and raw == b''.join(b for b in got if b)
    # a tag stream one block short: ZK_E_RNG_EXHAUSTED in the tag's part status only
    tag_rows = [_blocks(H.tag_seeds, b, 4) for b in range(H.B)]
    tag_rows[4] = [b'\xff' * 32] + tag_rows[4][:3]
    got, st, pst = eng.accountable_prove_batch_rings(*H.w, seeds=H.seeds, tag_streams=b''.join(b''.join(r) for r in tag_rows), tag_stream_blocks=4)
    assert st == [0, 0, 0, 0, E_RNG, 0] and pst == [(0, 0)] * 4 + [(0, E_RNG), (0, 0)]
    assert got == H.bundles[:4] + [None, H.bundles[5]]
    # which beyond the ring's padded size: the inner call's status (16 is inside ring B's padded size, outside ring A's)
    which = list(H.w[3])
    which[0] = NA
    inner = list(eng.prove_batch_rings(H.w[0], H.w[1], H.w[2], which, H.w[4], seeds=H.seeds)[1])
    assert inner[0] != 0 and inner[1:] == [0] * 5
    got, st, pst = eng.accountable_prove_batch_rings(H.w[0], H.w[1], H.w[2], which, H.w[4], seeds=H.seeds, tag_seeds=H.tag_seeds)
    assert st == inner and pst[0][0] == inner[0] and got == [None] + H.bundles[1:]
    # every id of a call unknown: nothing to stage, every bundle refused
    none = eng.accountable_prove_batch_rings(*H.w[:4], [GONE] * H.B, seeds=H.seeds, tag_seeds=H.tag_seeds)
    assert none[0] == [None] * H.B and none[1] == [E_ARG] * H.B


# ------------------------------------------------------------------ 4. capacity
def test_capacity_is_exact_host_form(X, H):
    eng, B = X.eng, H.B
    need = sum(X.size[i] for i in H.w[4])
    assert need == 3 * X.size[X.ids['A']] + 3 * X.size[X.ids['B']]
    pat = lambda n, width: [int.from_bytes(b'\x5a' * width, 'little')] * n
    with pytest.raises(X.Z.ZkError) as e:
        eng.accountable_prove_batch_rings(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds, cap=need - 1, fill=0x5a)
    out, off, st, pst = eng.accountable_last_outputs
    assert e.value.status == E_BUF and out == b'\x5a' * need and off == pat(B + 1, 8) and st == pat(B, 4)[:B] and pst == pat(2 * B, 4)
    assert eng.accountable_prove_batch_rings(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds, cap=need, fill=0x5a)[0] == H.bundles
    # an id that is not resident counts 0
    ids = [GONE] + H.w[4][1:]
    with pytest.raises(X.Z.ZkError) as e:
        eng.accountable_prove_batch_rings(*H.w[:4], ids, seeds=H.seeds, tag_seeds=H.tag_seeds, cap=need - X.size[X.ids['A']] - 1)
    assert e.value.status == E_BUF
    got = eng.accountable_prove_batch_rings(*H.w[:4], ids, seeds=H.seeds, tag_seeds=H.tag_seeds, cap=need - X.size[X.ids['A']])
    assert got[0] == [None] + H.bundles[1:] and got[1] == [E_ARG] + [0] * 5
    # an all-A batch succeeds in a buffer smaller than B x the B-ring maximum (the binding hands the call exactly the rule's sum)
    w = _rows(X, _mixed(4, 'A'))
    assert 4 * X.size[X.ids['A']] < 4 * X.size[X.ids['B']]
    assert eng.accountable_prove_batch_rings(*w, cap=4 * X.size[X.ids['A']])[1] == [0] * 4
    # call level: B = 0; NULL ids; no params; no auditor
    assert eng.accountable_prove_batch_rings(b'', b'', b'', [], []) == ([], [], [])
    assert eng.accountable_last_raw == (b'', [0])
    assert eng.accountable_verify_batch_rings(b'', [], []) == ([], [], [])
    assert eng.accountable_open_batch_rings(X.a32, [], []) == ([], [], [])
    import ctypes as C
    r1, k1 = eng._rng(B, H.seeds, None, 0)
    r2, k2 = eng._rng(B, H.tag_seeds, None, 0)
    out, off, st = C.create_string_buffer(need), (C.c_uint64 * (B + 1))(), (C.c_int32 * B)()
    which = (C.c_uint32 * B)(*H.w[3])
    assert eng.L.zk_rings_accountable_prove_batch(eng.h, B, H.w[0], H.w[1], H.w[2], which, None, C.byref(r1), C.byref(r2), out, need, off, st, None) == E_ARG
    assert eng.L.zk_rings_accountable_prove_batch(eng.h, 1 << 32, H.w[0], H.w[1], H.w[2], which, which, C.byref(r1), C.byref(r2), out, need, off, st, None) == E_ARG
    bare = X.Z.Engine(0)
    plain = _engine(X, auditor=False)
    try:
        assert bare.ring_accountable_proof_max_size(0) == 0
        for eng2 in (bare, plain):
            with pytest.raises(X.Z.ZkError) as e:
                eng2.accountable_verify_batch_rings(H.w[0], H.bundles, H.w[4])
            assert e.value.status == E_BUF
            with pytest.raises(X.Z.ZkError) as e:
                eng2.accountable_open_batch_rings(X.a32, H.bundles, H.w[4])
            assert e.value.status == E_BUF
        with pytest.raises(X.Z.ZkError) as e:
            plain.accountable_prove_batch_rings(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds, cap=need)
        assert e.value.status == E_BUF
    finally:
        bare.close(), plain.close()


def _up(b, tail=16):
    import torch
    return torch.frombuffer(bytearray(bytes(b) + bytes(tail)), dtype=torch.uint8).to(torch.device('cuda:0'))


def test_capacity_is_exact_device_form_and_the_device_verifier_and_opener(X, H):
    import numpy as np
    import torch
    eng, B = X.eng, H.B
    msg, sig, pk, which, ids = H.w
    need = sum(X.size[i] for i in ids)
    u32 = lambda v: struct.pack('<%dI' % len(v), *v)
    d = [_up(msg), _up(sig), _up(pk), _up(u32(which)), _up(u32(ids)), _up(H.seeds), _up(H.tag_seeds)]
    ptr = [t.data_ptr() for t in d]
    fill = lambda nbytes: torch.full((nbytes,), 0x5a, dtype=torch.uint8, device='cuda:0')
    d_out, d_off, d_st, d_pst = fill(need + 64), fill(8 * (B + 1) + 16), fill(4 * B + 16), fill(8 * B + 16)
    torch.cuda.synchronize()
    with pytest.raises(X.Z.ZkError) as e:   # one byte short: refused from the ids alone, nothing written
        eng.accountable_prove_batch_rings_device(B, *ptr, d_out.data_ptr(), need - 1, d_off.data_ptr(), d_st.data_ptr(), d_pst.data_ptr())
    assert e.value.status == E_BUF
    for t in (d_out, d_off, d_st, d_pst):
        assert bytes(t.cpu().numpy()) == b'\x5a' * t.numel()
    eng.set_timing(1)
    try:
        eng.accountable_prove_batch_rings_device(B, *ptr, d_out.data_ptr(), need, d_off.data_ptr(), d_st.data_ptr(), d_pst.data_ptr())
        names = set(eng.last_timing()[1])
        assert {'accountable_caps', 'accountable_blinders', 'accountable_layout'} <= names, names
    finally:
        eng.set_timing(0)
    torch.cuda.synchronize()
    off = np.frombuffer(bytes(d_off.cpu().numpy())[:8 * (B + 1)], dtype=np.uint64)
    out = bytes(d_out.cpu().numpy())
    assert [out[int(off[b]):int(off[b + 1])] for b in range(B)] == H.bundles
    assert out[int(off[B]):int(off[B]) + 64] == b'\x5a' * 64 and out[need:] == b'\x5a' * 64
    assert bytes(d_st.cpu().numpy()) == bytes(4 * B) + b'\x5a' * 16 and bytes(d_pst.cpu().numpy()) == bytes(8 * B) + b'\x5a' * 16
    # an all-A batch in a buffer smaller than B x the B-ring maximum: the read-back names ring A alone
    wa = _rows(X, _mixed(4, 'A'))
    da = [_up(wa[0]), _up(wa[1]), _up(wa[2]), _up(u32(wa[3])), _up(u32(wa[4])), _up(H.seeds[:128]), _up(H.tag_seeds[:128])]
    cap_a = 4 * X.size[X.ids['A']]
    a_out, a_off, a_st = fill(cap_a), fill(8 * 5), fill(16)
    torch.cuda.synchronize()
    eng.accountable_prove_batch_rings_device(4, *[t.data_ptr() for t in da], a_out.data_ptr(), cap_a, a_off.data_ptr(), a_st.data_ptr(), None)
    torch.cuda.synchronize()
    assert bytes(a_st.cpu().numpy()) == bytes(16)
    # the verifier and the opener on device buffers: a tampered tag, a truncated slot, an id that is not resident
    bundles = list(H.bundles)
    bundles[1] = bundles[1][:-9] + bytes([bundles[1][-9] ^ 1]) + bundles[1][-8:]
    bundles[3] = bundles[3][:-4]
    vids = [GONE] + ids[1:]
    host = eng.accountable_verify_batch_rings(msg, bundles, vids)
    assert host == ([0, 0, 1, 0, 1, 1], [E_ARG, 0, 0, E_BAD, 0, 0], [0, 1, NONE, 0, NONE, NONE])
    host_open = eng.accountable_open_batch_rings(X.a32, bundles, vids)
    assert host_open[2] == [E_ARG, 0, 0, E_BAD, 0, 0] and host_open[0][2] == ids[2] and host_open[1][3] == NONE
    offs = [0]
    for b in bundles:
        offs.append(offs[-1] + len(b))
    d_b, d_boff, d_vids, d_secret = _up(b''.join(bundles), 0), _up(struct.pack('<%dQ' % (B + 1), *offs), 0), _up(u32(vids)), _up(X.a32)
    d_ok, d_vst, d_bad = fill(B + 10), fill(4 * B + 16), fill(4 * B + 16)
    d_ring, d_idx, d_ost = fill(4 * B + 16), fill(4 * B + 16), fill(4 * B + 16)
    torch.cuda.synchronize()
    eng.accountable_verify_batch_rings_device(B, ptr[0], d_b.data_ptr(), d_boff.data_ptr(), d_vids.data_ptr(), None, d_ok.data_ptr(), d_vst.data_ptr(), d_bad.data_ptr())
    eng.accountable_open_batch_rings_device(B, d_secret.data_ptr(), d_b.data_ptr(), d_boff.data_ptr(), d_vids.data_ptr(), d_ring.data_ptr(), d_idx.data_ptr(), d_ost.data_ptr())
    torch.cuda.synchronize()
    ok, vst, bad = bytes(d_ok.cpu().numpy()), bytes(d_vst.cpu().numpy()), bytes(d_bad.cpu().numpy())
    assert list(ok[:B]) == host[0] and ok[B:] == b'\x5a' * 10
    assert list(np.frombuffer(vst[:4 * B], dtype=np.int32)) == host[1] and vst[4 * B:] == b'\x5a' * 16
    assert bad == struct.pack('<%dI' % B, *host[2]) + b'\x5a' * 16
    for t, want in ((d_ring, host_open[0]), (d_idx, host_open[1])):
        assert bytes(t.cpu().numpy()) == struct.pack('<%dI' % B, *want) + b'\x5a' * 16
    assert bytes(d_ost.cpu().numpy()) == struct.pack('<%di' % B, *host_open[2]) + b'\x5a' * 16
    # misaligned ids are refused by all three; B = 0 is ZK_OK with out_off[0] = 0
    for call in (lambda: eng.accountable_prove_batch_rings_device(B, *ptr[:4], ptr[4] + 2, *ptr[5:], d_out.data_ptr(), need, d_off.data_ptr(), d_st.data_ptr(), None),
                 lambda: eng.accountable_verify_batch_rings_device(B, ptr[0], d_b.data_ptr(), d_boff.data_ptr(), d_vids.data_ptr() + 2, None, d_ok.data_ptr(), d_vst.data_ptr()),
                 lambda: eng.accountable_open_batch_rings_device(B, d_secret.data_ptr(), d_b.data_ptr(), d_boff.data_ptr(), d_vids.data_ptr() + 2, d_ring.data_ptr(),
                                                                 d_idx.data_ptr(), d_ost.data_ptr())):
        with pytest.raises(X.Z.ZkError) as e:
            call()
        assert e.value.status == E_ARG
    d_off0 = fill(24)
    torch.cuda.synchronize()
    eng.accountable_prove_batch_rings_device(0, None, None, None, None, None, ptr[5], ptr[6], None, 0, d_off0.data_ptr(), None, None)
    eng.accountable_verify_batch_rings_device(0, None, None, None, None, None, None, None, None)
    eng.accountable_open_batch_rings_device(0, d_secret.data_ptr(), None, None, None, None, None, None)
    torch.cuda.synchronize()
    assert bytes(d_off0.cpu().numpy()) == bytes(8) + b'\x5a' * 16


# ------------------------------------------------------------------ 5. the verifier
def test_verifier_equals_the_recipe(X, H):
    eng, B, msg, ids = X.eng, H.B, H.w[0], H.w[4]
    flags = _flags(X, eng)
    swapped = list(H.bundles)   # bundles 0 and 2 (both ring A) with their tags exchanged
    swapped[0], swapped[2] = H.bundles[0][:-TAG] + H.bundles[2][-TAG:], H.bundles[2][:-TAG] + H.bundles[0][-TAG:]
    other = list(ids)           # bundle 1 told to be in the other ring
    other[1] = X.ids['A']
    gone = list(ids)
    gone[3] = GONE
    cut = list(H.bundles)
    cut[5] = cut[5][:-4]
    vseeds = X.DC.seeds_for(b'accr-vs', B)
    for bundles, vids, vs, want in ((H.bundles, ids, None, ([1] * B, [0] * B, [NONE] * B)),
                                    (swapped, ids, None, ([0, 1, 0, 1, 1, 1], None, [1, NONE, 1, NONE, NONE, NONE])),
                                    (H.bundles, other, None, ([1, 0, 1, 1, 1, 1], None, [NONE, 0, NONE, NONE, NONE, NONE])),
                                    (H.bundles, gone, None, ([1, 1, 1, 0, 1, 1], [0, 0, 0, E_ARG, 0, 0], [NONE, NONE, NONE, 0, NONE, NONE])),
                                    (cut, ids, None, ([1, 1, 1, 1, 1, 0], [0, 0, 0, 0, 0, E_BAD], [NONE, NONE, NONE, NONE, NONE, 0])),
                                    (swapped, ids, vseeds, None)):
        got = eng.accountable_verify_batch_rings(msg, bundles, vids, vs)
        assert got == _verify_recipe(X, eng, msg, bundles, vids, 0, vs)
        if want:
            assert got[0] == want[0] and got[2] == want[2] and (want[1] is None or got[1] == want[1])
    assert _flags(X, eng) == flags


# ------------------------------------------------------------------ 6. the open
def test_open_equals_split_and_the_rings_opener(X, H):
    eng, B, ids, which = X.eng, H.B, H.w[4], H.w[3]
    flags = _flags(X, eng)
    assert eng.accountable_open_batch_rings(X.a32, H.bundles, ids) == (ids, which, [0] * B)
    # ANY finds the ring; the shared key (bundle 4, shown in A) is answered with the lower id
    low = min(X.ids.values())
    want_ring = [i if b != 4 else low for b, i in enumerate(ids)]
    want_idx = [w if b != 4 or low == X.ids['A'] else SHARED_AT for b, w in enumerate(which)]
    assert eng.accountable_open_batch_rings(X.a32, H.bundles, [ANY] * B) == (want_ring, want_idx, [0] * B)
    # refused bundles, ids of every kind, the other ring's id: what split + escrow_open_batch_rings gives
    bundles = list(H.bundles)
    bundles[0] = b'ZKC2' + bundles[0][4:]
    bundles[3] = bundles[3][:-4]
    bundles[5] = bundles[5][:-TAG] + b'ZKT2' + bundles[5][-TAG + 4:]   # the walk accepts it, the tag's header is refused
    oids = [GONE, X.ids['A'], ANY, ANY, X.ids['B'], ids[5]]
    att, tags, sst = eng.accountable_split(bundles)
    assert sst == [E_BAD, 0, 0, E_BAD, 0, 0] and (att, tags, sst) == X.AC.split(bundles, 0)
    want = eng.escrow_open_batch_rings(X.a32, tags, oids)
    got = eng.accountable_open_batch_rings(X.a32, bundles, oids)
    assert got == want
    assert got[2] == [E_ARG, 0, 0, E_BAD, 0, E_BAD]
    assert got[0] == [NONE, NONE, ids[2], NONE, X.ids['B'], NONE] and got[1] == [NONE, NONE, which[2], NONE, SHARED_AT, NONE]
    # a wrong secret: ZK_E_OPENING, nothing written
    wrong = hashlib.sha256(b'not the auditor').digest()
    with pytest.raises(X.Z.ZkError) as e:
        eng.accountable_open_batch_rings(wrong, H.bundles, ids, fill=0x5a)
    assert e.value.status == E_OPENING
    assert eng.accountable_last_outputs == ([0x5a5a5a5a] * B, [0x5a5a5a5a] * B, [0x5a5a5a5a] * B)
    assert eng.accountable_open_batch_rings(X.a32, H.bundles, ids)[2] == [0] * B   # the context is usable again
    assert _flags(X, eng) == flags
    # windows of one bundle (chunk 1 x 1 lane): six windows, each with its own walk, opener and fold
    win = _engine(X)
    try:
        win.set_chunk(1), win.set_lanes(1)
        assert win.accountable_open_batch_rings(X.a32, bundles, oids) == want
        assert win.accountable_verify_batch_rings(H.w[0], H.bundles, ids)[0] == [1] * B
    finally:
        win.close()


# ------------------------------------------------------------------ 7. round trip through a ring update and a re-ring
def test_round_trip_through_update_and_rering(X, H):
    eng = _engine(X)
    try:
        B, (msg, sig, pk, which, ids) = H.B, H.w
        bundles, st, _ = eng.accountable_prove_batch_rings(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds)
        assert st == [0] * B and bundles == H.bundles
        unused = 40   # a key of ring B that no witness and no shared entry uses
        assert unused not in which and unused != SHARED_AT
        eng.update_ring(X.ids['B'], [(unused, hashlib.sha256(b'a new member').digest())])
        stale = eng.accountable_verify_batch_rings(msg, bundles, ids)[0]
        print('verdicts of the old bundles against the updated ring B:', stale)
        assert [stale[b] for b in (0, 2, 4)] == [1, 1, 1]   # ring A did not change
        att, tags, sst = eng.accountable_split(bundles)
        assert sst == [0] * B
        moved, mst = eng.rering_batch_rings(msg, att, which, ids, eng.prove_key_blinders(seeds=H.seeds), seeds=X.DC.seeds_for(b'accr-move', B))
        assert mst == [0] * B
        joined, jst = eng.accountable_join(list(moved), tags)
        assert jst == [0] * B
        assert eng.accountable_verify_batch_rings(msg, joined, ids) == ([1] * B, [0] * B, [NONE] * B)
        assert eng.accountable_open_batch_rings(X.a32, joined, ids) == (ids, which, [0] * B)
    finally:
        eng.close()


def test_device_open_with_a_wrong_secret_writes_nothing_in_any_window(X, H):
    """B = 6 bundles in windows of 2 (chunk 1 x 2 lanes): the opener refuses the secret in the first window, before the first fold, so no word of the caller's
    three device arrays changes -- neither the first window's nor a later one's; the right secret then fills them"""
    import torch
    eng = _engine(X)
    try:
        eng.set_chunk(1), eng.set_lanes(2)
        B, ids, which = H.B, H.w[4], H.w[3]
        offs = [0]
        for b in H.bundles:
            offs.append(offs[-1] + len(b))
        u32 = lambda v: struct.pack('<%dI' % len(v), *v)
        d_b, d_off, d_ids = _up(b''.join(H.bundles), 0), _up(struct.pack('<%dQ' % (B + 1), *offs), 0), _up(u32(ids))
        d_wrong, d_right = _up(hashlib.sha256(b'not the auditor').digest()), _up(X.a32)
        outs = [torch.full((4 * B + 16,), 0x5a, dtype=torch.uint8, device='cuda:0') for _ in range(3)]
        torch.cuda.synchronize()
        with pytest.raises(X.Z.ZkError) as e:
            eng.accountable_open_batch_rings_device(B, d_wrong.data_ptr(), d_b.data_ptr(), d_off.data_ptr(), d_ids.data_ptr(), *[t.data_ptr() for t in outs])
        torch.cuda.synchronize()
        assert e.value.status == E_OPENING
        for t in outs:
            assert bytes(t.cpu().numpy()) == b'\x5a' * t.numel()
        eng.accountable_open_batch_rings_device(B, d_right.data_ptr(), d_b.data_ptr(), d_off.data_ptr(), d_ids.data_ptr(), *[t.data_ptr() for t in outs])
        torch.cuda.synchronize()
        got = [bytes(t.cpu().numpy()) for t in outs]
        assert got == [u32(ids) + b'\x5a' * 16, u32(which) + b'\x5a' * 16, bytes(4 * B) + b'\x5a' * 16]
    finally:
        eng.close()


def test_wipe_and_a_failed_call_leave_no_nonzero_word(X, H):
    """zk_test_counter 11 counts the nonzero words of every witness-flagged buffer"""
    eng = _engine(X)
    try:
        assert eng.accountable_prove_batch_rings(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds)[0] == H.bundles
        assert 0 < eng.test_counter(11) < 1 << 63
        eng.wipe()
        assert eng.test_counter(11) == 0
        assert eng.accountable_prove_batch_rings(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds)[0] == H.bundles
        with pytest.raises(X.Z.ZkError) as e:
            eng.accountable_prove_batch_rings(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds, cap=1000)
        assert e.value.status == E_BUF and eng.test_counter(11) == 0
        assert eng.accountable_open_batch_rings(X.a32, H.bundles, H.w[4])[2] == [0] * H.B
        eng.wipe()
        assert eng.test_counter(11) == 0
    finally:
        eng.close()
