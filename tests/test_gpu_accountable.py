"""-m gpu: zk_accountable_prove_batch / zk_accountable_verify_batch / zk_accountable_split_batch / zk_accountable_join_batch ("ZKC1").  The expected bytes are
the recipe's (INTEGRATION.md "Accountable attestations"): the 16-byte header, then what prove_batch, prove_key_blinders, proof_key_commitments and
escrow_prove_batch give on the same rows; one bundle's attestation is also checked against the C oracle and its tag against tests/escrow_common.py.  The
layout (walk, split, join) is tests/accountable_common.py's.  secLevel 20, 16-bit combs, a ring of 8 keys from synth_workload, an auditor from escrow_keygen."""
import hashlib
import os
import struct
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEC, S, NKEYS, NW = 20, 77, 8, 8   # synth_workload gives witness b its own key at ring index b mod NKEYS: one witness per member
E_BAD, E_RNG, E_BUF, E_ARG = 10, 11, 12, 14
NONE = 0xFFFFFFFF
TAG = 472
ATT_BLOCKS = 2048   # blocks of an attestation's explicit stream: block k = sha256(seed | k), what the seed mode draws


class Ctx:
    pass


def _engine(x, mode=None, packed=False, auditor=True, ring=True):
    eng = x.Z.Engine(0)
    eng.set_comb_bits(16)
    eng.set_params(x.par[0], x.par[1], x.par[2], SEC)
    if mode is not None:
        eng.set_mode(mode)
    if packed:
        eng.set_wire(1)
    if ring:
        eng.set_ring(x.ring, NKEYS)
    if auditor:
        eng.set_auditor(x.A72)
    return eng


def _rows(x, idx):
    cut = lambda a, w: b''.join(a[w * b:w * b + w] for b in idx)
    return cut(x.msg, 32), cut(x.sig, 64), cut(x.pk, 64), [x.which[b] for b in idx]


def _blocks(seeds, b, n):
    return [hashlib.sha256(seeds[32 * b:32 * b + 32] + k.to_bytes(8, 'big')).digest() for k in range(n)]


def _recipe(x, eng, msg, sig, pk, which, att_rng, tag_rng):
    """the four existing calls and the header: what a user builds today.  att_rng / tag_rng: keyword arguments (seeds=..., or streams=... and stream_blocks=...)
    -> (bundles; (attestation status, tag status) pairs; proofs; keyXcoms; tags)"""
    B = len(which)
    proofs, ast = eng.prove_batch(msg, sig, pk, which, **att_rng)
    assert ast == [0] * B
    bl = eng.prove_key_blinders(**att_rng)
    kx, kst = eng.proof_key_commitments(proofs)
    assert kst == [0] * B
    tags, tst = eng.escrow_prove_batch([pk[64 * b:64 * b + 32] for b in range(B)], kx, bl, **tag_rng)
    assert tst == [0] * B
    out = [x.AC.bundle(proofs[b], tags[b]) for b in range(B)]
    return out, list(zip(ast, tst)), proofs, kx, tags


def _verify_recipe(x, eng, msg, bundles, vseeds=None):
    """verify_batch + proof_key_commitments + escrow_verify_batch on the split parts (tests/accountable_common.py's split) -> (ok, status, first_bad)"""
    att, tags, sst = x.AC.split(bundles, x.packed_of(eng))
    live = [b for b in range(len(bundles)) if sst[b] == 0]
    ok, st, bad = [0] * len(bundles), [E_BAD] * len(bundles), [0] * len(bundles)
    if live:
        a_ok, a_st = eng.verify_batch(b''.join(msg[32 * b:32 * b + 32] for b in live), [att[b] for b in live],
                                      None if vseeds is None else b''.join(vseeds[32 * b:32 * b + 32] for b in live))
        kx, _ = eng.proof_key_commitments([att[b] for b in live])
        t_ok, t_st = eng.escrow_verify_batch(kx, [tags[b] for b in live])
        for i, b in enumerate(live):
            a_bad, t_bad = not a_ok[i] or a_st[i] != 0, not t_ok[i] or t_st[i] != 0
            ok[b], st[b], bad[b] = int(not a_bad and not t_bad), a_st[i] or t_st[i], 0 if a_bad else 1 if t_bad else NONE
    return ok, st, bad


@pytest.fixture(scope='module')
def X():
    import accountable_common as AC
    import escrow_common as EC
    import zkp_ecdsa_amd as Z
    x = Ctx()
    x.Z, x.AC, x.EC, x.R = Z, AC, EC, EC.R
    probe = Z.Engine(0)
    x.par = probe.synth_params(S)
    x.ring, x.msg, x.sig, x.pk, x.which, _ = probe.synth_workload(S, NKEYS, NW)
    probe.close()
    x.pp = EC.MC.oracle_params(x.par[1], x.par[2])
    x.a = int.from_bytes(EC.tag(b'acc-auditor', 0), 'big')
    x.a32 = x.a.to_bytes(32, 'big')
    x.A = EC.keygen(x.pp, x.a)
    x.A72 = x.R._tp(x.A)
    x.packed = {}
    x.packed_of = lambda eng: x.packed.get(id(eng), 0)
    x.eng = _engine(x)
    assert x.eng.escrow_keygen(x.a32) == x.A72
    yield x
    x.eng.close()


@pytest.fixture(scope='module')
def H(X):
    """three honest bundles of the reference mode in the ZKA1 layout and the recipe's parts, shared and left unchanged"""
    h = Ctx()
    h.idx = [1, 4, 6]
    h.w = _rows(X, h.idx)
    h.seeds, h.tag_seeds = X.EC.seeds_for(b'acc-att', 3), X.EC.seeds_for(b'acc-tag', 3)
    h.want, h.parts, h.proofs, h.kx, h.tags = _recipe(X, X.eng, *h.w, {'seeds': h.seeds}, {'seeds': h.tag_seeds})
    h.bundles, h.st, h.pst = X.eng.accountable_prove_batch(*h.w, seeds=h.seeds, tag_seeds=h.tag_seeds)
    return h


# ------------------------------------------------------------------ 1. the bytes are the recipe's
@pytest.mark.parametrize('B,mode,packed,stream,chunk', [(65, 0, False, False, 4), (3, 1, True, False, None), (3, 0, False, True, None), (1, 1, False, False, None),
                                                        (3, 0, True, True, None), (1, 0, True, False, None)])
def test_bundles_equal_the_recipe(X, B, mode, packed, stream, chunk):
    eng = X.eng if (mode, packed, chunk) == (0, False, None) else _engine(X, mode, packed)
    X.packed[id(eng)] = int(packed)
    try:
        if chunk:
            eng.set_chunk(chunk)
        assert eng.accountable_proof_max_size() == 16 + eng.proof_max_size() + TAG == X.AC.max_size(eng.proof_max_size())
        w = _rows(X, [b % NW for b in range(B)])   # beyond 8 bundles: the same witnesses again under fresh seeds
        name = b'r%d%d%d%d' % (B, mode, packed, stream)
        seeds, tag_seeds = X.EC.seeds_for(b'att' + name, B), X.EC.seeds_for(b'tag' + name, B)
        if stream:
            att_rng = {'streams': b''.join(b''.join(_blocks(seeds, b, ATT_BLOCKS)) for b in range(B)), 'stream_blocks': ATT_BLOCKS}
            tag_rng = {'streams': b''.join(b''.join(_blocks(tag_seeds, b, 4)) for b in range(B)), 'stream_blocks': 4}
            got = eng.accountable_prove_batch(*w, streams=att_rng['streams'], stream_blocks=ATT_BLOCKS, tag_streams=tag_rng['streams'], tag_stream_blocks=4)
            seeded = eng.accountable_prove_batch(*w, seeds=seeds, tag_seeds=tag_seeds)
            assert seeded[0] == got[0]   # block k of a stream = sha256(seed | k): the seed mode's draws
        else:
            att_rng, tag_rng = {'seeds': seeds}, {'seeds': tag_seeds}
            got = eng.accountable_prove_batch(*w, seeds=seeds, tag_seeds=tag_seeds)
        bundles, st, pst = got
        assert st == [0] * B and pst == [(0, 0)] * B
        want = _recipe(X, eng, *w, att_rng, tag_rng)[0]
        for b in range(B):
            assert bundles[b] == want[b], b
        raw, off = eng.accountable_last_raw
        assert raw == b''.join(bundles) and off[0] == 0 and off[B] == len(raw)
        vseeds = X.EC.seeds_for(b'vs' + name, B)
        assert eng.accountable_verify_batch(w[0], bundles, vseeds) == ([1] * B, [0] * B, [NONE] * B)
        assert eng.accountable_verify_batch(w[0], bundles, want_first_bad=False) == ([1] * B, [0] * B, None)
    finally:
        if eng is not X.eng:
            eng.close()


def test_one_bundle_equals_the_oracle_and_the_python_statement(X, H):
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import coracle as CO
    EC = X.EC
    assert H.st == [0] * 3 and H.bundles == H.want
    octx = CO.OracleCtx(X.par[0], X.par[1], X.par[2], SEC)
    octx.set_ring(X.ring, NKEYS)
    att, est = octx.prove_batch(*H.w, seeds=H.seeds, nthreads=2)
    assert est == [0] * 3
    b = 1
    bundle = H.bundles[b]
    assert bundle[:16] == X.AC.header(len(bundle)) and bundle[16:-TAG] == att[b]
    assert octx.verify_batch(H.w[0][32 * b:32 * b + 32], [bundle[16:-TAG]], nthreads=1) == ([1], [0])
    bl = X.eng.prove_key_blinders(seeds=H.seeds)
    key, r = int.from_bytes(H.w[2][64 * b:64 * b + 32], 'big'), int.from_bytes(bl[b], 'big')
    assert X.eng.test_tom_commit([key], [r]) == [H.kx[b]]   # the blinder opens the oracle's keyXcom
    assert bundle[-TAG:] == EC.prove(X.pp, X.A, key, H.kx[b], r, X.R.SeedRng(H.tag_seeds[32 * b:32 * b + 32]))
    assert EC.verify(X.pp, X.A, H.kx[b], bundle[-TAG:]) == (1, 0)


# ------------------------------------------------------------------ 2. closing up
def test_a_failed_part_leaves_an_empty_slot_and_the_neighbours_close_up(X, H):
    """A call has ONE stride for all its rows, so a single row cannot be given fewer blocks than its neighbours.  The middle attestation's row is therefore a
    full-length stream of 0xff blocks, every one of which the rejection sampling refuses: the row runs out of randomness exactly as a short one does, and the
    status is compared with what zk_prove_batch gives on the same streams.  The tag's row uses the escrow tests' device: block 0 rejected, so four blocks do not
    hold the four draws."""
    eng = X.eng
    ff = b'\xff' * 32
    # (a) the middle attestation's stream holds only rejected blocks: an attestation failure
    att_rows = [b''.join(_blocks(H.seeds, b, ATT_BLOCKS)) for b in range(3)]
    att_rows[1] = ff * ATT_BLOCKS
    att_rng = {'streams': b''.join(att_rows), 'stream_blocks': ATT_BLOCKS}
    got, st, pst = eng.accountable_prove_batch(*H.w, streams=att_rng['streams'], stream_blocks=ATT_BLOCKS, tag_seeds=H.tag_seeds)
    ref_st = eng.prove_batch(*H.w, **att_rng)[1]
    assert ref_st[1] != 0 and ref_st[0] == ref_st[2] == 0
    assert st == [0, ref_st[1], 0] and pst[0] == pst[2] == (0, 0) and pst[1][0] == ref_st[1]
    assert got == [H.bundles[0], None, H.bundles[2]]
    raw, off = eng.accountable_last_raw
    assert off == [0, len(H.bundles[0]), len(H.bundles[0]), len(H.bundles[0]) + len(H.bundles[2])] and raw == H.bundles[0] + H.bundles[2]
    # (b) the middle tag's stream: block 0 rejected, so four blocks do not hold the four draws
    tag_rows = [_blocks(H.tag_seeds, b, 4) for b in range(3)]
    tag_rows[1] = [ff] + tag_rows[1][:3]
    got, st, pst = eng.accountable_prove_batch(*H.w, seeds=H.seeds, tag_streams=b''.join(b''.join(r) for r in tag_rows), tag_stream_blocks=4)
    assert st == [0, E_RNG, 0] and pst == [(0, 0), (0, E_RNG), (0, 0)]
    assert got == [H.bundles[0], None, H.bundles[2]]
    raw, off = eng.accountable_last_raw
    assert off == [0, len(H.bundles[0]), len(H.bundles[0]), len(H.bundles[0]) + len(H.bundles[2])] and raw == H.bundles[0] + H.bundles[2]


def _dev_prove(x, eng, h, cap=None, misalign=0, part=True):
    """zk_accountable_prove_batch_device on torch buffers -> (0 or the ZkError's status, out, offsets, statuses, part statuses as the call left them)"""
    import torch
    B = len(h.w[3])
    full = max(eng.accountable_proof_max_size(), 16 + 65536 + TAG) * B
    d = [_up(h.w[0]), _up(h.w[1]), _up(h.w[2]), _up(struct.pack('<%dI' % B, *h.w[3])), _up(h.seeds), _up(h.tag_seeds)]
    outs = [torch.full((n,), 0x5a, dtype=torch.uint8, device='cuda:0') for n in (full + 64, 8 * (B + 1) + 16, 4 * B + 16, 8 * B + 16)]
    torch.cuda.synchronize()
    rc = 0
    try:
        eng.accountable_prove_batch_device(B, d[0].data_ptr() + misalign, *[t.data_ptr() for t in d[1:]], outs[0].data_ptr(), full if cap is None else cap, outs[1].data_ptr(),
                                           outs[2].data_ptr(), outs[3].data_ptr() if part else None)
    except x.Z.ZkError as e:
        rc = e.status
    torch.cuda.synchronize()
    return (rc,) + tuple(bytes(t.cpu().numpy()) for t in outs)


def _up(b, tail=16):
    import torch
    return torch.frombuffer(bytearray(bytes(b) + bytes(tail)), dtype=torch.uint8).to(torch.device('cuda:0'))


def _untouched(res):
    return all(r == b'\x5a' * len(r) for r in res[1:])


def test_prover_refusals_write_nothing(X, H):
    Z = X.Z
    need = X.eng.accountable_proof_max_size() * 3
    res = _dev_prove(X, X.eng, H, cap=need - 1)
    assert res[0] == E_BUF and _untouched(res)
    with pytest.raises(Z.ZkError) as e:
        X.eng.accountable_prove_batch(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds, cap=need - 1)
    assert e.value.status == E_BUF
    assert X.eng.accountable_prove_batch(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds, cap=need)[0] == H.bundles
    for kw in ({'auditor': False}, {'ring': False}):
        eng = _engine(X, **kw)
        try:
            if not kw.get('ring', True):
                assert eng.accountable_proof_max_size() == 0
            res = _dev_prove(X, eng, H)
            assert res[0] == E_BUF and _untouched(res), kw
            with pytest.raises(Z.ZkError) as e:
                eng.accountable_prove_batch(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds, cap=1 << 22)
            assert e.value.status == E_BUF
            with pytest.raises(Z.ZkError) as e:
                eng.accountable_verify_batch(H.w[0], H.bundles)
            assert e.value.status == E_BUF
        finally:
            eng.close()
    eng = Z.Engine(0)   # no params
    try:
        assert eng.accountable_proof_max_size() == 0
        with pytest.raises(Z.ZkError) as e:
            eng.accountable_prove_batch(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds, cap=1 << 22)
        assert e.value.status == E_BUF
    finally:
        eng.close()
    # B = 0; NULL for a required pointer
    assert X.eng.accountable_prove_batch(b'', b'', b'', []) == ([], [], [])
    assert X.eng.accountable_verify_batch(b'', []) == ([], [], [])
    assert X.eng.accountable_split([]) == ([], [], []) and X.eng.accountable_join([], []) == ([], [])
    import ctypes as C
    off, st = (C.c_uint64 * 4)(), (C.c_int32 * 3)()
    r1, _k1 = X.eng._rng(3, H.seeds, None, 0)
    which = (C.c_uint32 * 3)(*H.w[3])
    out = C.create_string_buffer(need)
    assert X.eng.L.zk_accountable_prove_batch(X.eng.h, 3, H.w[0], H.w[1], H.w[2], which, C.byref(r1), None, out, need, off, st, None) == E_ARG
    assert X.eng.L.zk_accountable_verify_batch(X.eng.h, 3, H.w[0], b''.join(H.bundles), None, None, out, st, None) == E_ARG


# ------------------------------------------------------------------ 3. the verifier names the part
def _flip(b, at):
    return b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]


def test_the_verifier_names_the_part(X, H):
    eng, AC = X.eng, X.AC
    msg = H.w[0]
    b0, b1, b2 = H.bundles
    # a flipped byte in the attestation (a response byte), in t_rho; tags swapped between two honest bundles; a tag under another auditor key
    other = _engine(X, auditor=False)
    try:
        other.set_auditor(other.escrow_keygen((X.a + 1).to_bytes(32, 'big')))
        foreign = other.accountable_prove_batch(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds)[0]
        assert other.accountable_verify_batch(msg, foreign)[0] == [1, 1, 1]
    finally:
        other.close()
    assert [f[:-TAG] for f in foreign] == [b[:-TAG] for b in H.bundles]   # the attestation does not depend on the auditor
    cases = [[_flip(b0, len(b0) - TAG - 9), b1, b2], [b0, _flip(b1, len(b1) - 5), b2], [b0[:-TAG] + b2[-TAG:], b1, b2[:-TAG] + b0[-TAG:]],
             [b0, foreign[1], b2]]
    want = [([0, 1, 1], [0, NONE, NONE]), ([1, 0, 1], [NONE, 1, NONE]), ([0, 1, 0], [1, NONE, 1]), ([1, 0, 1], [NONE, 1, NONE])]
    for bundles, (ok, bad) in zip(cases, want):
        got = eng.accountable_verify_batch(msg, bundles)
        assert (got[0], got[2]) == (ok, bad), (got, ok, bad)
        assert got == _verify_recipe(X, eng, msg, bundles)
    flipped = cases[0][0]
    assert eng.accountable_verify_batch(msg[:32], [flipped])[1] == eng.verify_batch(msg[:32], [flipped[16:-TAG]])[1]
    # every header error and each inner-length case: ZK_E_BAD_ENCODING, first_bad 0; the good neighbours stay good
    bad = AC.bad_vectors(b1, len(b1) - 16 - TAG)
    for name, v in bad:
        got = eng.accountable_verify_batch(msg, [b0, v, b2])
        if len(v) % 4:   # the slot behind it starts at an offset that is no multiple of 4: refused by the same rule
            assert got == ([1, 0, 0], [0, E_BAD, E_BAD], [NONE, 0, 0]), name
        else:
            assert got == ([1, 0, 1], [0, E_BAD, 0], [NONE, 0, NONE]), name
    many = [v for _, v in bad]
    got = eng.accountable_verify_batch(msg[32:64] * len(many), many)
    assert got == ([0] * len(many), [E_BAD] * len(many), [0] * len(many)) == _verify_recipe(X, eng, msg[32:64] * len(many), many)
    # offsets that are not aligned or do not ascend, on one blob
    blob = b0 + b1 + b2
    o1, o2 = len(b0), len(b0) + len(b1)
    assert eng.accountable_verify_batch(msg, None, blob=blob, offsets=[0, o1 + 2, o2, len(blob)])[1] == [E_BAD, E_BAD, 0]
    assert eng.accountable_verify_batch(msg, None, blob=blob, offsets=[0, o2, o1, len(blob)])[1] == [E_BAD, E_BAD, E_BAD]


def test_nothing_outside_a_slot_is_read(X, H):
    """the device form on a buffer that ends with the last slot's last readable byte: the last bundle is cut inside its tag (the header says so too), and what
    lies behind the slot is a guard pattern that would pass as the rest of the tag -- the verdict is the walk's, from the slot alone"""
    import numpy as np
    import torch
    b0, b1, _ = H.bundles
    cut = X.AC.put32(b1[:-100], 4, len(b1) - 100)
    blob = b0 + cut
    offs = [0, len(b0), len(blob)]
    d_b = _up(blob + b1[-100:], 0)   # behind the slot: the bytes a reader that overruns would want
    d_off, d_msg = _up(struct.pack('<3Q', *offs), 0), _up(H.w[0][:64], 0)
    d_ok = torch.full((2 + 6,), 0x5a, dtype=torch.uint8, device='cuda:0')
    d_st = torch.full((8 + 16,), 0x5a, dtype=torch.uint8, device='cuda:0')
    d_bad = torch.full((8 + 16,), 0x5a, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    X.eng.accountable_verify_batch_device(2, d_msg.data_ptr(), d_b.data_ptr(), d_off.data_ptr(), None, d_ok.data_ptr(), d_st.data_ptr(), d_bad.data_ptr())
    torch.cuda.synchronize()
    assert bytes(d_ok.cpu().numpy()) == bytes([1, 0]) + b'\x5a' * 6
    assert list(np.frombuffer(bytes(d_st.cpu().numpy())[:8], dtype=np.int32)) == [0, E_BAD]
    assert list(np.frombuffer(bytes(d_bad.cpu().numpy())[:8], dtype=np.uint32)) == [NONE, 0]
    assert bytes(d_b.cpu().numpy()) == blob + b1[-100:]


# ------------------------------------------------------------------ 4. split and join
def test_split_and_join_round_trips(X, H):
    eng, AC = X.eng, X.AC
    att, tags, st = eng.accountable_split(H.bundles)
    assert (att, tags, st) == AC.split(H.bundles, 0) and att == H.proofs and tags == H.tags and st == [0] * 3
    assert eng.accountable_last_raw == (b''.join(att), [0, len(att[0]), len(att[0]) + len(att[1]), sum(map(len, att))])
    assert eng.accountable_join(att, tags) == (H.bundles, [0] * 3) == AC.join(att, tags, 0)
    assert eng.accountable_split(eng.accountable_join(H.proofs, H.tags)[0])[:2] == (H.proofs, H.tags)
    # a refused bundle: an empty slot and zero tag bytes, the neighbours close up
    for name, v in AC.bad_vectors(H.bundles[1], len(H.proofs[1])):
        got = eng.accountable_split([H.bundles[0], v, H.bundles[2]])
        if len(v) % 4:   # the slot behind it starts at an offset that is no multiple of 4: refused by the same rule
            assert got == ([H.proofs[0], b'', b''], [H.tags[0], bytes(TAG), bytes(TAG)], [0, E_BAD, E_BAD]), name
            continue
        assert got == ([H.proofs[0], b'', H.proofs[2]], [H.tags[0], bytes(TAG), H.tags[2]], [0, E_BAD, 0]), name
        assert eng.accountable_last_raw[0] == H.proofs[0] + H.proofs[2]
    # join refuses a bad proof header and a bad tag header
    bad_tag = b'ZKT2' + H.tags[0][4:]
    proofs, tags2 = [H.proofs[0], H.proofs[1][:-4], H.proofs[2]], [bad_tag, H.tags[1], H.tags[2]]
    assert eng.accountable_join(proofs, tags2) == ([None, None, H.bundles[2]], [E_BAD, E_BAD, 0]) == AC.join(proofs, tags2, 0)
    assert eng.accountable_last_raw == (H.bundles[2], [0, 0, 0, len(H.bundles[2])])
    # capacities, from the offsets alone
    for call in (lambda: eng.accountable_split(H.bundles, cap=sum(map(len, H.proofs)) - 1), lambda: eng.accountable_join(H.proofs, H.tags, cap=sum(map(len, H.bundles)) - 1)):
        with pytest.raises(X.Z.ZkError) as e:
            call()
        assert e.value.status == E_BUF
    assert eng.accountable_split(H.bundles, cap=sum(map(len, H.proofs)))[0] == H.proofs
    assert eng.accountable_join(H.proofs, H.tags, cap=sum(map(len, H.bundles)))[0] == H.bundles


def test_split_tags_open_alone_and_through_a_threshold(X, H):
    eng = _engine(X)
    try:
        _, tags, _ = eng.accountable_split(H.bundles)
        assert eng.escrow_open_batch(X.a32, tags) == (H.w[3], [0] * 3)
        shares, keys = eng.auditors_split_key(X.a32, 2, 3, seed=X.EC.tag(b'acc-split', 0))
        eng.set_auditors(2, keys)
        sh = {}
        for j in (1, 3):
            sh[j], st = eng.auditors_share_batch(j, shares[j - 1], tags, seeds=X.EC.seeds_for(b'acc-sh%d' % j, 3))
            assert st == [0] * 3 and eng.auditors_share_verify_batch(tags, sh[j]) == ([1] * 3, [0] * 3)
        rings, idx, st = eng.auditors_combine_batch([1, 3], tags, [sh[1], sh[3]], [X.Z.ESCROW_RING_ANY] * 3)
        assert (idx, st) == (H.w[3], [0] * 3)
    finally:
        eng.close()


def test_split_rering_join_keeps_the_tag(X, H):
    eng = _engine(X)
    try:
        bl = eng.prove_key_blinders(seeds=H.seeds)
        att, tags, _ = eng.accountable_split(H.bundles)
        new = [bytes([0]) + hashlib.sha256(b'acc-new-key%d' % i).digest()[:31] for i in range(4)]
        eng.update_ring(0, [(NKEYS + i, k) for i, k in enumerate(new)], NKEYS + 4)   # 12 keys: one index bit more, the old keys where they were
        moved, st = eng.rering_batch(H.w[0], att, H.w[3], bl, seeds=X.EC.seeds_for(b'acc-rr', 3))
        assert st == [0] * 3 and all(len(m) > len(a) for m, a in zip(moved, att))
        joined, st = eng.accountable_join(moved, tags)
        assert st == [0] * 3 and [j[-TAG:] for j in joined] == H.tags
        assert eng.accountable_verify_batch(H.w[0], joined) == ([1] * 3, [0] * 3, [NONE] * 3)
        assert eng.accountable_verify_batch(H.w[0], H.bundles)[0] == [0] * 3   # the old bundles name the old ring
        assert eng.escrow_open_batch(X.a32, eng.accountable_split(joined)[1]) == (H.w[3], [0] * 3)
    finally:
        eng.close()


# ------------------------------------------------------------------ 5. the device forms
def test_device_forms_on_torch_buffers(X, H):
    import numpy as np
    import torch
    B = 3
    rc, out, off, st, pst = _dev_prove(X, X.eng, H)
    off = np.frombuffer(off[:8 * (B + 1)], dtype=np.uint64)
    assert rc == 0 and [out[int(off[b]):int(off[b + 1])] for b in range(B)] == H.bundles and int(off[0]) == 0
    assert out[int(off[B]):] == b'\x5a' * (len(out) - int(off[B])) and st == bytes(4 * B) + b'\x5a' * 16 and pst == bytes(8 * B) + b'\x5a' * 16
    assert _dev_prove(X, X.eng, H, part=False)[4] == b'\x5a' * (8 * B + 16)
    res = _dev_prove(X, X.eng, H, misalign=1)
    assert res[0] == E_ARG and _untouched(res)
    # the verifier, split and join on device buffers equal the host forms
    bundles = [H.bundles[0], _flip(H.bundles[1], len(H.bundles[1]) - 5), X.AC.put32(H.bundles[2], 8, 1)]
    host = X.eng.accountable_verify_batch(H.w[0], bundles)
    assert host == ([1, 0, 0], [0, 0, E_BAD], [NONE, 1, 0])
    blob = b''.join(bundles)
    offs = [0]
    for b in bundles:
        offs.append(offs[-1] + len(b))
    d_msg, d_b, d_boff, d_seeds = _up(H.w[0]), _up(blob, 0), _up(struct.pack('<%dQ' % (B + 1), *offs), 0), _up(X.EC.seeds_for(b'acc-dv', B), 0)
    fill = lambda n: torch.full((n,), 0x5a, dtype=torch.uint8, device='cuda:0')
    for vs, fb in ((None, True), (d_seeds.data_ptr(), False)):
        d_ok, d_vst, d_bad = fill(B + 8), fill(4 * B + 16), fill(4 * B + 16)
        torch.cuda.synchronize()
        X.eng.accountable_verify_batch_device(B, d_msg.data_ptr(), d_b.data_ptr(), d_boff.data_ptr(), vs, d_ok.data_ptr(), d_vst.data_ptr(), d_bad.data_ptr() if fb else None)
        torch.cuda.synchronize()
        ok, vst, bad = bytes(d_ok.cpu().numpy()), bytes(d_vst.cpu().numpy()), bytes(d_bad.cpu().numpy())
        assert list(ok[:B]) == host[0] and ok[B:] == b'\x5a' * 8
        assert list(np.frombuffer(vst[:4 * B], dtype=np.int32)) == host[1] and vst[4 * B:] == b'\x5a' * 16
        assert bad == (struct.pack('<%dI' % B, *host[2]) + b'\x5a' * 16 if fb else b'\x5a' * (4 * B + 16))
    with pytest.raises(X.Z.ZkError) as e:
        X.eng.accountable_verify_batch_device(B, d_msg.data_ptr(), d_b.data_ptr() + 2, d_boff.data_ptr(), None, d_ok.data_ptr(), d_vst.data_ptr(), None)
    assert e.value.status == E_ARG
    h_att, h_tags, h_st = X.eng.accountable_split(bundles)
    d_att, d_aoff, d_tags, d_sst = fill(len(blob) + 64), fill(8 * (B + 1) + 16), fill(TAG * B + 64), fill(4 * B + 16)
    torch.cuda.synchronize()
    X.eng.accountable_split_device(B, d_b.data_ptr(), d_boff.data_ptr(), d_att.data_ptr(), len(blob), d_aoff.data_ptr(), d_tags.data_ptr(), d_sst.data_ptr())
    torch.cuda.synchronize()
    aoff = [int(v) for v in np.frombuffer(bytes(d_aoff.cpu().numpy())[:8 * (B + 1)], dtype=np.uint64)]
    att, tg = bytes(d_att.cpu().numpy()), bytes(d_tags.cpu().numpy())
    assert [att[aoff[b]:aoff[b + 1]] for b in range(B)] == h_att and att[aoff[B]:] == b'\x5a' * (len(att) - aoff[B])
    assert tg == b''.join(h_tags) + b'\x5a' * 64 and list(np.frombuffer(bytes(d_sst.cpu().numpy())[:4 * B], dtype=np.int32)) == h_st == [0, 0, E_BAD]
    with pytest.raises(X.Z.ZkError) as e:
        X.eng.accountable_split_device(B, d_b.data_ptr(), d_boff.data_ptr(), d_att.data_ptr() + 1, len(blob), d_aoff.data_ptr(), d_tags.data_ptr(), d_sst.data_ptr())
    assert e.value.status == E_ARG
    # join on the split's own buffers gives the accepted bundles back, closed up
    d_out, d_ooff, d_jst = fill(len(blob) + 64), fill(8 * (B + 1) + 16), fill(4 * B + 16)
    torch.cuda.synchronize()
    X.eng.accountable_join_device(B, d_att.data_ptr(), d_aoff.data_ptr(), d_tags.data_ptr(), d_out.data_ptr(), len(blob), d_ooff.data_ptr(), d_jst.data_ptr())
    torch.cuda.synchronize()
    ooff = [int(v) for v in np.frombuffer(bytes(d_ooff.cpu().numpy())[:8 * (B + 1)], dtype=np.uint64)]
    out = bytes(d_out.cpu().numpy())
    assert [out[ooff[b]:ooff[b + 1]] for b in range(B)] == [bundles[0], bundles[1], b''] and out[ooff[B]:] == b'\x5a' * (len(out) - ooff[B])
    assert list(np.frombuffer(bytes(d_jst.cpu().numpy())[:4 * B], dtype=np.int32)) == [0, 0, E_BAD]
    with pytest.raises(X.Z.ZkError) as e:
        X.eng.accountable_join_device(B, d_att.data_ptr(), d_aoff.data_ptr(), d_tags.data_ptr(), d_out.data_ptr() + 3, len(blob), d_ooff.data_ptr(), d_jst.data_ptr())
    assert e.value.status == E_ARG


def test_wipe_and_a_failed_call_leave_no_nonzero_word(X, H):
    """zk_test_counter 11 counts the nonzero words of every witness-flagged buffer, the accountable staging (gathered keys and blinders) among them; it sums
    them all, so the staging entry is not isolated.  The failed call here is refused for out_cap before anything is staged: what the test shows is that a failed
    call leaves nothing of the call before it either, not that a call failing between two pipelines clears its own window (that path is wipe_witness too)."""
    eng = _engine(X)
    try:
        assert eng.accountable_prove_batch(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds)[0] == H.bundles
        assert 0 < eng.test_counter(11) < 1 << 63
        eng.wipe()
        assert eng.test_counter(11) == 0
        assert eng.accountable_prove_batch(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds)[0] == H.bundles
        assert eng.test_counter(11) > 0
        with pytest.raises(X.Z.ZkError) as e:   # a failed call wipes by itself
            eng.accountable_prove_batch(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds, cap=1000)
        assert e.value.status == E_BUF and eng.test_counter(11) == 0
        assert eng.accountable_prove_batch(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds)[0] == H.bundles
    finally:
        eng.close()


# ------------------------------------------------------------------ 6. timing families
def test_last_timing_lists_the_new_families(X, H):
    import ctypes as C

    def names():
        total, nm, ms = C.c_float(), (C.c_char_p * 64)(), (C.c_float * 64)()
        n = X.eng.L.zk_last_timing(X.eng.h, C.byref(total), nm, ms, 64)
        return {nm[i].decode() for i in range(min(n, 64))}

    X.eng.set_timing(1)
    try:
        X.eng.accountable_prove_batch(*H.w, seeds=H.seeds, tag_seeds=H.tag_seeds)
        got = names()
        assert {'accountable_blinders', 'accountable_layout', 'escrow_front', 'escrow_respond', 'tom_commit', 'hash'} <= got, got
        X.eng.accountable_verify_batch(H.w[0], H.bundles)
        got = names()
        assert {'accountable_walk', 'accountable_verdict', 'escrow_parse', 'escrow_ladder'} <= got, got
    finally:
        X.eng.set_timing(0)
