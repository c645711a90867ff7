"""-m gpu: zk_auditors_* -- t of n auditors open escrow tags through verifiable shares "ZKS1".  The split's and the shares' bytes, the share verifier's verdicts
and statuses are the Python statement's (tests/escrow_threshold_common.py); the combine's answers are zk_rings_escrow_open_batch's with the undivided secret
on the same tags and ring ids.  secLevel 20, 12-bit context combs, chunks of 64 tags on 2 lanes; rings of 257, 5 and 2 keys resident; B in {1, 3, 65}."""
import hashlib
import itertools
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

SEC = 20
E_BAD, E_RNG, E_BUFFER, E_ARG, E_OPENING = 10, 11, 12, 14, 16
NONE = ANY = 0xffffffff
NB = 65


class Ctx:
    pass


def _engine(Z, par, A72=None, bits=12, mode=None):
    eng = Z.Engine(0)
    eng.set_comb_bits(bits)
    eng.set_params(*par, SEC)
    if mode is not None:
        eng.set_mode(mode)
    eng.set_chunk(64)
    eng.set_lanes(2)
    if A72:
        eng.set_auditor(A72)
    return eng


def _tags(x, eng, name, keys):
    _, r, seeds = x.EC.workload(name, len(keys))
    c = eng.test_tom_commit(keys, r)
    tags, st = eng.escrow_prove_batch(x.EC.be32(keys), c, x.EC.be32(r), seeds=seeds)
    assert st == [0] * len(keys)
    return tags


def _subsets(t, n):
    if (t, n) == (2, 3):
        return [list(s) for s in itertools.permutations(range(1, n + 1), t)]
    scattered = {(3, 5): [5, 2, 3], (16, 16): [(7 * i) % 16 + 1 for i in range(16)], (1, 1): [1]}[(t, n)]
    return [list(range(1, t + 1)), list(range(n - t + 1, n + 1))[::-1], scattered]


def _split(x, eng, t, n):
    """the engine's split of x.a with the shape's seed, installed as the context's set -> (shares, keys)"""
    shares, keys = eng.auditors_split_key(x.a32, t, n, seed=x.EC.tag(b'split-seed', 10 * t + n))
    eng.set_auditors(t, keys)
    return shares, keys


def _shares(x, eng, shares, tags, js=None):
    """{j: the engine's shares of `tags` by auditor j}, seeds by auditor and tag"""
    out = {}
    for j in js or range(1, len(shares) + 1):
        sh, st = eng.auditors_share_batch(j, shares[j - 1], tags, seeds=x.EC.seeds_for(b'sh%d' % j, len(tags)))
        assert st == [0] * len(tags)
        out[j] = sh
    return out


def _statement_share(x, j, shares, keys, tag, b):
    TC = x.TC
    return TC.share(x.pp, j, int.from_bytes(shares[j - 1], 'big'), x.EC.point(keys[j - 1]), tag, x.R.SeedRng(x.EC.seeds_for(b'sh%d' % j, b + 1)[32 * b:]))


@pytest.fixture(scope='module')
def X():
    import escrow_common as EC
    import escrow_threshold_common as TC
    import zkp_ecdsa_amd as Z
    x = Ctx()
    x.Z, x.EC, x.TC, x.R = Z, EC, TC, EC.R
    boot = Z.Engine(0)
    x.par = boot.synth_params(EC.PARAM_SEED)
    boot.close()
    x.pp = EC.MC.oracle_params(x.par[1], x.par[2])
    x.a32 = EC.tag(b'auditor-thr', 0)
    x.a = int.from_bytes(x.a32, 'big') % EC.Q
    x.A72 = x.R._tp(EC.keygen(x.pp, x.a))
    eng = x.eng = _engine(Z, x.par, x.A72)
    x.lists = [EC.scalars(b'thrA', 257), EC.scalars(b'thrB', 5), EC.scalars(b'thrC', 2)]
    x.lists[1][4] = x.lists[0][9]   # one key enrolled in two rings
    x.ids = [eng.add_ring(EC.be32(r), len(r)) for r in x.lists]
    x.outside = EC.scalars(b'thr-outside', 2)
    plan = [(b % 3, [0, len(x.lists[b % 3]) - 1, (53 * b + 7) % len(x.lists[b % 3])][(b // 3) % 3]) for b in range(NB - 3)] + [(0, 9)]
    x.keys = [x.lists[r][i] for r, i in plan] + x.outside
    x.want_ids = [ANY if b % 4 == 3 else x.ids[r] for b, (r, _) in enumerate(plan)] + [ANY, x.ids[0]]
    # tag 0 keeps its place for B = 1; tags 1 and 2 name their rings, tag 3 searches every ring
    assert len(x.keys) == NB
    x.tags = _tags(x, eng, b'thr65', x.keys)
    x.single = lambda tags, ids: eng.escrow_open_batch_rings(x.a32, tags, ids)
    yield x
    eng.close()


# ------------------------------------------------------------------ the split, the shares, the verifier and the combine against the statement and the single auditor
@pytest.mark.parametrize('B', [1, 3, NB])
@pytest.mark.parametrize('t,n', [(2, 3), (3, 5)])
def test_split_shares_verify_and_combine(X, t, n, B):
    eng, EC, TC = X.eng, X.EC, X.TC
    shares, keys = _split(X, eng, t, n)
    want = TC.split_bytes(X.pp, X.a, t, n, X.R.SeedRng(EC.tag(b'split-seed', 10 * t + n)))
    assert (b''.join(shares), b''.join(keys)) == want
    assert eng.test_counter(11) == 0   # the dealer's staging is zero when the call returns
    tags, ids = X.tags[:B], X.want_ids[:B]
    sh = _shares(X, eng, shares, tags)
    for j in range(1, n + 1):
        for b in (range(B) if B <= 3 else (0, 1, 63, 64)):   # (a chunk's first and last tags, and the second chunk's one)
            assert (sh[j][b], 0) == _statement_share(X, j, shares, keys, tags[b], b), (j, b)
        assert eng.auditors_share_verify_batch(tags, sh[j]) == ([1] * B, [0] * B)
    single = X.single(tags, ids)
    assert single[2] == [0] * B and (B < NB or (single[1].count(NONE) == 2 and len(set(single[0])) == 4))
    for S in _subsets(t, n):
        assert eng.auditors_combine_batch(S, tags, [sh[j] for j in S], ids) == single, S
    assert eng.auditors_combine_batch(_subsets(t, n)[0], [], [[]] * t, []) == ([], [], [])


@pytest.mark.parametrize('t,n', [(1, 1), (16, 16)])
def test_the_smallest_and_the_largest_shape(X, t, n):
    eng, EC, TC = X.eng, X.EC, X.TC
    shares, keys = _split(X, eng, t, n)
    assert (b''.join(shares), b''.join(keys)) == TC.split_bytes(X.pp, X.a, t, n, X.R.SeedRng(EC.tag(b'split-seed', 10 * t + n)))
    if t == 1:
        assert shares == [X.a.to_bytes(32, 'big')] and keys == [X.A72]
    tags, ids = X.tags[:3], X.want_ids[:3]
    sh = _shares(X, eng, shares, tags)
    for j in range(1, n + 1):
        assert (sh[j][1], 0) == _statement_share(X, j, shares, keys, tags[1], 1), j
        assert eng.auditors_share_verify_batch(tags, sh[j]) == ([1] * 3, [0] * 3)
    single = X.single(tags, ids)
    for S in _subsets(t, n):
        assert eng.auditors_combine_batch(S, tags, [sh[j] for j in S], ids) == single, S


# ------------------------------------------------------------------ mutants; a wrong D; components of small order
def test_mutants_wrong_d_and_small_order_components(X):
    eng, EC, TC, R = X.eng, X.EC, X.TC, X.R
    t, n = 2, 3
    shares, keys = _split(X, eng, t, n)
    kp = [EC.point(k) for k in keys]
    tags = X.tags[:3]
    sh = _shares(X, eng, shares, tags)
    rows = TC.mutants(sh[2][0], tags[0], X.par[2], tags[1], n)
    got = eng.auditors_share_verify_batch([tg for _, tg, _ in rows], [m for _, _, m in rows])
    want = [TC.verify(X.pp, kp, tg, m) for _, tg, m in rows]
    assert got == ([w[0] for w in want], [w[1] for w in want]), [name for name, _, _ in rows]
    assert got[0][0] == 1 and got[0].count(1) == 1 and got[1].count(E_BAD) == 7 and not any(name == 's + q' for name, _, _ in rows)
    # s + q: a response with room below 2^256 needs s < 2^224.  With the undivided secret 1 (A = g, one auditor) and the stream's k = 2^100, s = k - c lies
    # just below 2^100; the share belongs to the same tag, whose own proof the share verifier does not look at
    one = _engine(X.Z, X.par, X.par[1])
    try:
        s1, k1 = one.auditors_split_key((1).to_bytes(32, 'big'), 1, 1, seed=bytes(32))
        assert s1 == [(1).to_bytes(32, 'big')] and k1 == [X.par[1]]
        one.set_auditors(1, k1)
        small, st = one.auditors_share_batch(1, s1[0], tags[:1], streams=(1 << 100).to_bytes(32, 'big'), stream_blocks=1)
        assert st == [0] and small[0] == TC.share(X.pp, 1, 1, X.pp.g, tags[0], R.StreamRng([(1 << 100).to_bytes(32, 'big')]))[0]
        plus_q = [m for name, _, m in TC.mutants(small[0], tags[0], X.par[2], tags[1], 2) if name == 's + q']
        assert len(plus_q) == 1 and plus_q[0] != small[0] and TC.verify(X.pp, [X.pp.g], tags[0], plus_q[0]) == (1, 0)
        assert one.auditors_share_verify_batch([tags[0]] * 2, [small[0], plus_q[0]]) == ([1, 1], [0, 0])
    finally:
        one.close()
    # one D replaced by another valid point: status 0 and no member, and that share fails its verifier
    ids = X.want_ids[:3]
    single = X.single(tags, ids)
    wrong = [s[:16] + X.par[2] + s[88:] for s in sh[2]]
    assert eng.auditors_combine_batch([2, 3], tags, [wrong, sh[3]], ids) == ([NONE] * 3, [NONE] * 3, [0] * 3)
    assert eng.auditors_share_verify_batch(tags, wrong) == ([0] * 3, [0] * 3)
    # D_j + P4 leaves the answer as it is; a slot whose share names another auditor, or whose D is off the curve, is status 10 for that tag alone
    P2, P4 = EC.small_order_points()
    plus = [s[:16] + R._tp(EC.point(s[16:88]).add(P4)) + s[88:] for s in sh[2]]
    assert eng.auditors_combine_batch([2, 3], tags, [plus, sh[3]], ids) == single
    mixed = [sh[2][0], sh[1][1], sh[2][2][:40] + bytes([sh[2][2][40] ^ 0x40]) + sh[2][2][41:]]
    assert eng.auditors_combine_batch([2, 3], tags, [mixed, sh[3]], ids) == ([single[0][0], NONE, NONE], [single[1][0], NONE, NONE], [0, E_BAD, E_BAD])
    assert TC.combine(n, [2, 3], tags[1], [mixed[1], sh[3][1]], ANY, {}) == (NONE, NONE, E_BAD)
    # tags whose E1 / E2 carry components of small order: the shares are made from them, and the combine gives the single auditor's answer
    def pt_plus(tg, k, S):
        o = EC.PT[k]
        return tg[:o] + R._tp(EC.point(tg[o:o + 72]).add(S)) + tg[o + 72:]
    odd = [pt_plus(tags[0], 1, P4), pt_plus(tags[1], 1, P2), pt_plus(tags[2], 0, P4.add(P2)), pt_plus(pt_plus(tags[0], 0, P4), 1, P4.add(P2))]
    oids = [ids[0], ids[1], ids[2], ANY]
    osh = _shares(X, eng, shares, odd)
    assert (osh[1][2], 0) == _statement_share(X, 1, shares, keys, odd[2], 2)
    want = X.single(odd, oids)
    assert want[2] == [0] * 4 and NONE not in want[1]
    for S in ([1, 2], [3, 1]):
        assert eng.auditors_combine_batch(S, odd, [osh[j] for j in S], oids) == want
    # a refused tag among good ones: 264 zero bytes, status 10, and its neighbours are untouched
    batch = [tags[0], b'ZKT2' + tags[1][4:], tags[2]]
    got, st = eng.auditors_share_batch(2, shares[1], batch, seeds=EC.seeds_for(b'sh2', 3))
    assert st == [0, E_BAD, 0] and got[0] == sh[2][0] and got[2] == sh[2][2] and eng.share_last_raw[264:528] == bytes(264)


# ------------------------------------------------------------------ refusals, in the contract's order
def _status(Z, f, *a, **k):
    try:
        f(*a, **k)
    except Z.ZkError as e:
        return e.status
    return 0


def test_refusals_in_the_contract_order(X):
    Z, EC = X.Z, X.EC
    eng = _engine(Z, X.par)
    try:
        rid = eng.add_ring(EC.be32(X.lists[1]), 5)
        tags = [X.tags[1], X.tags[4]]   # keys 0 and 4 of the ring of 5
        shares, keys = eng.auditors_split_key(X.a32, 2, 3, seed=EC.tag(b'split-seed', 23))   # parameters are all the dealer needs
        assert _status(Z, eng.set_auditors, 2, keys) == E_BUFFER                              # no auditor key
        eng.set_auditor(X.A72)
        # no set: ZK_E_BUFFER before j, the secret and the capacity are looked at
        assert _status(Z, eng.auditors_share_batch, 9, bytes(32), tags, cap=1) == E_BUFFER
        assert _status(Z, eng.auditors_share_verify_batch, tags, [bytes(264)] * 2) == E_BUFFER
        assert _status(Z, eng.auditors_combine_batch, [1, 1], tags, [[bytes(264)] * 2] * 2, [rid] * 2) == E_BUFFER
        # a set with one inconsistent key, with a key off the curve, with the identity; t and n out of range
        bad = list(keys)
        bad[2] = keys[1]
        assert _status(Z, eng.set_auditors, 2, bad) == E_OPENING
        assert _status(Z, eng.set_auditors, 2, [keys[0], keys[1][:35] + bytes([keys[1][35] ^ 1]) + keys[1][36:], keys[2]]) == E_BAD
        assert _status(Z, eng.set_auditors, 2, [keys[0], bytes(71) + b'\x01', keys[2]]) == E_ARG
        assert _status(Z, eng.set_auditors, 4, keys) == E_ARG and _status(Z, eng.set_auditors, 0, keys) == E_ARG
        assert _status(Z, eng.set_auditors, 2, keys * 6) == E_ARG     # n = 18
        assert _status(Z, eng.auditors_share_verify_batch, tags, [bytes(264)] * 2) == E_BUFFER   # nothing was kept
        eng.set_auditors(2, keys)
        # share: j, then the secret (nothing written), then the capacity
        seeds = EC.seeds_for(b'sh1', 2)
        assert _status(Z, eng.auditors_share_batch, 0, shares[0], tags, seeds=seeds, cap=1) == E_ARG
        assert _status(Z, eng.auditors_share_batch, 4, shares[0], tags, seeds=seeds, cap=1) == E_ARG
        assert _status(Z, eng.auditors_share_batch, 1, shares[1], tags, seeds=seeds, cap=1) == E_OPENING
        assert eng.test_counter(11) == 0
        assert _status(Z, eng.auditors_share_batch, 1, shares[0], tags, seeds=seeds, cap=527) == E_BUFFER
        assert eng.test_counter(11) == 0
        sh1, st = eng.auditors_share_batch(1, shares[0], tags, seeds=seeds)
        sh3, st3 = eng.auditors_share_batch(3, shares[2], tags, seeds=EC.seeds_for(b'sh3', 2))
        assert st == st3 == [0, 0]
        # a stream that does not hold the draw: per tag
        got, st = eng.auditors_share_batch(1, shares[0], tags, streams=b'\xff' * 64, stream_blocks=1)   # the one block is rejected
        assert st == [E_RNG, E_RNG] and got == [None, None]
        # combine: t, a 0, a value above n, a duplicate; then a non-resident ring id before a bad tag
        two = [sh1, sh3]
        assert _status(Z, eng.auditors_combine_batch, [1, 3, 2], tags, [sh1, sh3, sh1], [rid] * 2) == E_ARG
        assert _status(Z, eng.auditors_combine_batch, [1], tags, [sh1], [rid] * 2) == E_ARG
        for S in ([0, 3], [1, 4], [3, 3]):
            assert _status(Z, eng.auditors_combine_batch, S, tags, two, [rid] * 2) == E_ARG, S
        damaged = [b'ZKT2' + tags[0][4:], tags[1]]
        ring, idx, st = eng.auditors_combine_batch([1, 3], damaged, two, [rid + 77, rid])
        assert st == [E_ARG, 0] and ring == [NONE, rid] and idx[0] == NONE
        assert eng.auditors_combine_batch([1, 3], damaged, two, [rid, rid + 77])[2] == [E_BAD, E_ARG]
        assert eng.auditors_combine_batch([1, 3], tags, two, [ANY, rid]) == eng.escrow_open_batch_rings(X.a32, tags, [ANY, rid])
        # the split's own refusals
        assert _status(Z, eng.auditors_split_key, X.a32, 3, 2) == E_ARG and _status(Z, eng.auditors_split_key, X.a32, 1, 17) == E_ARG
        assert _status(Z, eng.auditors_split_key, X.a32, 3, 3, stream=bytes(32), stream_blocks=1) == E_RNG
        # zk_ctx_set_auditor drops the set, and so does zk_ctx_set_params
        eng.set_auditor(X.A72)
        assert _status(Z, eng.auditors_share_verify_batch, tags, sh1) == E_BUFFER
        eng.set_auditors(2, keys)
        assert eng.auditors_share_verify_batch(tags, sh1) == ([1, 1], [0, 0])
        eng.set_params(*X.par, SEC)
        assert _status(Z, eng.auditors_share_verify_batch, tags, sh1) == E_BUFFER
    finally:
        eng.close()


# ------------------------------------------------------------------ the device forms
def test_device_forms_equal_the_host_forms(X):
    import numpy as np
    import torch
    eng, EC = X.eng, X.EC
    t, n, B = 3, 5, NB
    shares, keys = _split(X, eng, t, n)
    tags = list(X.tags)
    tags[40] = b'ZKT2' + tags[40][4:]
    ids = list(X.want_ids)
    ids[5] = 4321
    def up(b):
        return torch.frombuffer(bytearray(bytes(b)), dtype=torch.uint8).to(torch.device('cuda:0'))
    def fresh(nbytes):
        return torch.full((nbytes + 16,), 0x5a, dtype=torch.uint8, device='cuda:0')
    d_tags = up(b''.join(tags))
    S = [5, 2, 3]
    host_sh, dev_sh = {}, {}
    for j in S:
        seeds = EC.seeds_for(b'sh%d' % j, B)
        sh, st = eng.auditors_share_batch(j, shares[j - 1], tags, seeds=seeds)
        assert st == [0] * 40 + [E_BAD] + [0] * 24
        host_sh[j] = eng.share_last_raw
        d_sec, d_seeds, d_out, d_st = up(shares[j - 1]), up(seeds), fresh(264 * B), fresh(4 * B)
        torch.cuda.synchronize()
        eng.auditors_share_batch_device(B, j, d_sec.data_ptr(), d_tags.data_ptr(), d_seeds.data_ptr(), d_out.data_ptr(), 264 * B, d_st.data_ptr())
        torch.cuda.synchronize()
        raw = bytes(d_out.cpu().numpy())
        assert raw[:264 * B] == host_sh[j] and raw[264 * B:] == b'\x5a' * 16 and raw[264 * 40:264 * 41] == bytes(264)
        assert list(np.frombuffer(bytes(d_st.cpu().numpy())[:4 * B], dtype=np.int32)) == st
        dev_sh[j] = d_out
        # a wrong share secret writes nothing
        d_out2, d_st2 = fresh(264 * B), fresh(4 * B)
        with pytest.raises(X.Z.ZkError) as e:
            eng.auditors_share_batch_device(B, j, up(shares[j % n]).data_ptr(), d_tags.data_ptr(), d_seeds.data_ptr(), d_out2.data_ptr(), 264 * B, d_st2.data_ptr())
        torch.cuda.synchronize()
        assert e.value.status == E_OPENING and bytes(d_out2.cpu().numpy()) == b'\x5a' * (264 * B + 16) and bytes(d_st2.cpu().numpy()) == b'\x5a' * (4 * B + 16)
    # verify
    rows = [host_sh[5][264 * b:264 * b + 264] for b in range(B)]
    rows[7] = rows[7][:263] + bytes([rows[7][263] ^ 1])   # one bit of s
    host = eng.auditors_share_verify_batch(tags, rows)
    assert host == ([1] * 7 + [0] + [1] * 32 + [0] + [1] * 24, [0] * 40 + [E_BAD] + [0] * 24)
    d_rows, d_ok, d_st = up(b''.join(rows)), fresh(B), fresh(4 * B)
    eng.auditors_share_verify_batch_device(B, d_tags.data_ptr(), d_rows.data_ptr(), d_ok.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    assert list(bytes(d_ok.cpu().numpy())[:B]) == host[0] and bytes(d_ok.cpu().numpy())[B:] == b'\x5a' * 16
    assert list(np.frombuffer(bytes(d_st.cpu().numpy())[:4 * B], dtype=np.int32)) == host[1]
    # combine, slot-major
    host = eng.auditors_combine_batch(S, tags, [[host_sh[j][264 * b:264 * b + 264] for b in range(B)] for j in S], ids)
    assert host[2][5] == E_ARG and host[2][40] == E_BAD and host[2].count(0) == B - 2 and host == X.single(tags, ids)
    d_all = up(b''.join(host_sh[j] for j in S))
    d_aud, d_ids = up(np.array(S, dtype=np.uint32).tobytes()), up(np.array(ids, dtype=np.uint32).tobytes())
    outs = [fresh(4 * B) for _ in range(3)]
    torch.cuda.synchronize()
    eng.auditors_combine_batch_device(B, t, d_aud.data_ptr(), d_tags.data_ptr(), d_all.data_ptr(), d_ids.data_ptr(), *[o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    raw = [bytes(o.cpu().numpy()) for o in outs]
    assert (list(np.frombuffer(raw[0][:4 * B], dtype=np.uint32)), list(np.frombuffer(raw[1][:4 * B], dtype=np.uint32)), list(np.frombuffer(raw[2][:4 * B], dtype=np.int32))) == host
    assert all(r[4 * B:] == b'\x5a' * 16 for r in raw)
    with pytest.raises(X.Z.ZkError) as e:   # a duplicate auditor, read from the device
        eng.auditors_combine_batch_device(B, t, up(np.array([5, 2, 5], dtype=np.uint32).tobytes()).data_ptr(), d_tags.data_ptr(), d_all.data_ptr(), d_ids.data_ptr(),
                                          *[o.data_ptr() for o in outs])
    assert e.value.status == E_ARG
    with pytest.raises(X.Z.ZkError) as e:   # misaligned device pointers
        eng.auditors_share_verify_batch_device(1, 4098, 4096, 4096, 4096)
    assert e.value.status == E_ARG


# ------------------------------------------------------------------ zk_ctx_update_ring, zk_ctx_wipe, the timing names
def test_update_ring_wipe_and_timing_names(X):
    Z, EC = X.Z, X.EC
    eng = _engine(Z, X.par, X.A72)
    try:
        ring = EC.scalars(b'thrU', 257)
        new = EC.scalars(b'thrNew', 2)
        rid = eng.add_ring(EC.be32(ring), 257)
        keys = [ring[0], ring[100], ring[256], new[0], new[1]]
        tags = _tags(X, eng, b'thr-update', keys)
        shares, akeys = eng.auditors_split_key(X.a32, 2, 3, seed=EC.tag(b'split-seed', 23))
        eng.set_auditors(2, akeys)
        eng.set_timing(1)
        sh = _shares(X, eng, shares, tags, js=(1, 3))
        assert set(eng.last_timing()[1]) == {'escrow_open', 'rng_prepass', 'share_front', 'tom_commit', 'share_ladder', 'tom_normalize', 'hash', 'share_respond'}
        assert eng.test_counter(11) > 0
        eng.wipe()
        assert eng.test_counter(11) == 0   # a_j, k, the fills and a_j E1 are gone
        assert eng.auditors_share_verify_batch(tags, sh[3]) == ([1] * 5, [0] * 5)
        assert set(eng.last_timing()[1]) == {'share_parse', 'tom_commit', 'share_relations'}
        two = [sh[3], sh[1]]
        assert eng.auditors_combine_batch([3, 1], tags, two, [rid] * 5) == ([rid] * 3 + [NONE] * 2, [0, 100, 256, NONE, NONE], [0] * 5)
        assert set(eng.last_timing()[1]) == {'escrow_index_build', 'combine_ladder', 'tom_normalize', 'escrow_lookup'}
        eng.update_ring(rid, {0: EC.be32([new[0]]), 100: EC.be32([new[1]])})   # in place: the index is patched, and the combine follows it
        assert eng.auditors_combine_batch([3, 1], tags, two, [ANY] * 5) == ([NONE, NONE, rid, rid, rid], [NONE, NONE, 256, 0, 100], [0] * 5)
        assert set(eng.last_timing()[1]) == {'combine_ladder', 'tom_normalize', 'escrow_lookup'}
        assert eng.escrow_open_batch_rings(X.a32, tags, [ANY] * 5)[1] == [NONE, NONE, 256, 0, 100]
        with pytest.raises(Z.ZkError):   # a wrong share secret: the key check is all that ran
            eng.auditors_share_batch(1, shares[1], tags)
        assert set(eng.last_timing()[1]) == {'escrow_open'} and eng.test_counter(11) == 0
    finally:
        eng.close()


# ------------------------------------------------------------------ the bytes depend on neither the comb widths, nor the mode, nor the build
def test_bytes_do_not_depend_on_comb_width_mode_or_build(X, tmp_path):
    Z, EC = X.Z, X.EC
    tags = X.tags[:5]
    def everything(eng):
        shares, keys = eng.auditors_split_key(X.a32, 3, 5, seed=EC.tag(b'split-seed', 35))
        eng.set_auditors(3, keys)
        h = hashlib.sha256(b''.join(shares) + b''.join(keys))
        for j in range(1, 6):
            sh, st = eng.auditors_share_batch(j, shares[j - 1], tags, seeds=EC.seeds_for(b'sh%d' % j, 5))
            assert st == [0] * 5
            h.update(b''.join(sh))
        return h.hexdigest()
    want = everything(X.eng)   # 12-bit combs
    for bits, mode in ((16, None), (16, Z.MODE_HARDENED)):
        eng = _engine(Z, X.par, None, bits, mode)
        try:
            eng.set_auditor(eng.escrow_keygen(X.a32))
            assert everything(eng) == want, (bits, mode)
        finally:
            eng.close()
    uni = os.path.join(os.path.dirname(Z.LIB_PATH), 'libzkattest_hip_uniform.so')
    assert os.path.exists(uni), 'the uniform build is not there (make -C zkp-ecdsa_amd/csrc uniform)'
    path = tmp_path / 'tags.bin'
    path.write_bytes(b''.join(tags))
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'escrow_threshold_uniform_check.py'), str(path)],
                         env=dict(os.environ, ZKATTEST_LIB=uni), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    rec = json.loads(out.stdout.decode().strip().splitlines()[-1])
    assert rec['lib'].endswith('_uniform.so') and rec['sha256'] == want

