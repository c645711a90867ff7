"""-m gpu: zk_quorum_prove_batch / zk_quorum_verify_batch ("ZKQ1").  The expected bytes are the recipe's (INTEGRATION.md "Counting signers"): the 16-byte
header, then what prove_batch, prove_key_blinders, proof_key_commitments and distinct_prove_batch give on the same rows; one quorum is also checked against the
oracle (the C oracle's proveSignatureList for the attestations, tests/distinct_common.py's proveMult for the pairs).  secLevel 20, 16-bit combs, a ring of 8
keys from synth_workload -- except the quorum of 16 members, which needs 16 different signers and so takes a ring of 32.  The workload has one witness
per ring member, so "signer s again" is the same witness under fresh seeds: another attestation by the same key."""
import hashlib
import os
import random
import struct
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEC, S, NKEYS, NW = 20, 77, 8, 8   # synth_workload gives witness b its own key at ring index b mod NKEYS: one witness per member
PAIR = 744
E_BAD, E_RNG, E_BUF, E_ARG = 10, 11, 12, 14
NONE = 0xFFFFFFFF


class Ctx:
    pass


def _engine(Z, par, ring, nkeys, mode=None, packed=False):
    eng = Z.Engine(0)
    eng.set_comb_bits(16)
    eng.set_params(par[0], par[1], par[2], SEC)
    if mode is not None:
        eng.set_mode(mode)
    if packed:
        eng.set_wire(1)
    eng.set_ring(ring, nkeys)
    return eng


@pytest.fixture(scope='module')
def X():
    import distinct_common as DC
    import zkp_ecdsa_amd as Z
    x = Ctx()
    x.Z, x.DC, x.R = Z, DC, DC.R
    probe = Z.Engine(0)
    x.par = probe.synth_params(S)
    x.ring, x.msg, x.sig, x.pk, x.which, _ = probe.synth_workload(S, NKEYS, NW)
    probe.close()
    x.eng = _engine(Z, x.par, x.ring, NKEYS)
    x.by = {}
    for b, w in enumerate(x.which):
        x.by.setdefault(w, []).append(b)
    x.signers = sorted(x.by)
    assert len(x.signers) >= 5
    yield x
    x.eng.close()


def _header(total, k):
    return b'ZKQ1' + struct.pack('>III', total, k, 0)


def _pick(x, signers, salt=0):
    """one witness per signer -> the rows of msg, sig, pk, which"""
    idx = [x.by[s][salt % len(x.by[s])] for s in signers]
    cut = lambda a, w: b''.join(a[w * b:w * b + w] for b in idx)
    return cut(x.msg, 32), cut(x.sig, 64), cut(x.pk, 64), [x.which[b] for b in idx]


def _workload(x, Q, k, name):
    """Q quorums of k different signers each: quorum q takes signers q, q + 1, ... (mod the signers the workload has)"""
    rows = [_pick(x, [x.signers[(q + i) % len(x.signers)] for i in range(k)], q) for q in range(Q)]
    P = k * (k - 1) // 2
    return (b''.join(r[0] for r in rows), b''.join(r[1] for r in rows), b''.join(r[2] for r in rows), sum((r[3] for r in rows), []),
            x.DC.seeds_for(b'att' + name, Q * k), x.DC.seeds_for(b'pair' + name, Q * P))


def _recipe(eng, k, msg, sig, pk, which, seeds, pair_seeds):
    """the four existing calls and the header: what a user builds today"""
    n = len(which)
    Q, P = n // k, k * (k - 1) // 2
    proofs, st = eng.prove_batch(msg, sig, pk, which, seeds=seeds)
    assert st == [0] * n
    bl = eng.prove_key_blinders(seeds=seeds)
    bl = [bl[32 * b:32 * b + 32] for b in range(n)] if isinstance(bl, (bytes, bytearray)) else list(bl)
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
    return out, proofs, kx, bl, dp


def _members(bundle, k):
    """the k attestations of a bundle and its pairs' proofs, by the inner total_len fields"""
    P = k * (k - 1) // 2
    pos, out = 16, []
    for _ in range(k):
        ln = int.from_bytes(bundle[pos + 4:pos + 8], 'big')
        out.append(bundle[pos:pos + ln])
        pos += ln
    assert pos == len(bundle) - PAIR * P
    return out, [bundle[pos + PAIR * p:pos + PAIR * p + PAIR] for p in range(P)]


def _honest(x, Q, k, name, eng=None):
    w = _workload(x, Q, k, name)
    bundles, st, mst = (eng or x.eng).quorum_prove_batch(k, *w)
    assert st == [0] * Q and mst == [0] * (Q * k)
    return w, bundles


# ------------------------------------------------------------------ 1. the bytes are the recipe's
@pytest.mark.parametrize('Q,k', [(5, 3), (3, 2), (2, 5)])
def test_bundles_equal_the_recipe(X, Q, k):
    eng = X.eng
    assert eng.quorum_pair_count(k) == k * (k - 1) // 2
    assert eng.quorum_proof_max_size(k) == 16 + k * eng.proof_max_size() + PAIR * (k * (k - 1) // 2)
    w, bundles = _honest(X, Q, k, b'recipe%d' % k)
    want = _recipe(eng, k, *w)[0]
    for q in range(Q):
        assert bundles[q] == want[q], q
    assert eng.quorum_verify_batch(k, w[0], bundles) == ([1] * Q, [0] * Q, [NONE] * Q)


def test_one_quorum_of_three_equals_the_oracle(X):
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import coracle as CO
    DC, R, k = X.DC, X.R, 3
    (msg, sig, pk, which, seeds, pair_seeds), (bundle,) = _honest(X, 1, k, b'oracle')
    octx = CO.OracleCtx(X.par[0], X.par[1], X.par[2], SEC)
    octx.set_ring(X.ring, NKEYS)
    att, est = octx.prove_batch(msg, sig, pk, which, seeds=seeds, nthreads=2)
    assert est == [0] * k
    members, pairs = _members(bundle, k)
    assert members == list(att)
    pp = DC.MC.oracle_params(X.par[1], X.par[2])
    kx, _ = X.eng.proof_key_commitments(list(att))
    bl = X.eng.prove_key_blinders(seeds=seeds)
    bl = [bl[32 * b:32 * b + 32] for b in range(k)] if isinstance(bl, (bytes, bytearray)) else list(bl)
    xs, rs = [int.from_bytes(pk[64 * m:64 * m + 32], 'big') for m in range(k)], [int.from_bytes(b, 'big') for b in bl]
    assert X.eng.test_tom_commit(xs, rs) == list(kx)   # the blinders open the oracle's keyXcoms
    for p, (i, j) in enumerate(X.eng.distinct_pairs(k)):
        assert pairs[p] == DC.oracle_prove(pp, xs[i], kx[i], rs[i], xs[j], kx[j], rs[j], R.SeedRng(pair_seeds[32 * p:32 * p + 32])), p
        assert DC.oracle_verify(pp, kx[i], kx[j], pairs[p]) == (1, 0)
    assert octx.verify_batch(msg, members, nthreads=2) == ([1] * k, [0] * k)


@pytest.mark.parametrize('variant', ['hardened', 'packed'])
def test_bundles_equal_the_recipe_in_hardened_mode_and_in_the_packed_layout(X, variant):
    Z, Q, k = X.Z, 5, 3
    if variant == 'hardened':
        nh, th = Z.hardened_h(b'quorum')
        eng = _engine(Z, (nh, X.par[1], th), X.ring, NKEYS, mode=Z.MODE_HARDENED)
    else:
        eng = _engine(Z, X.par, X.ring, NKEYS, packed=True)
    try:
        w, bundles = _honest(X, Q, k, b'recipe3', eng)
        assert bundles == _recipe(eng, k, *w)[0]
        assert bundles != _honest(X, Q, k, b'recipe3')[1]
        assert bundles[0][16:20] == (b'ZK1P' if variant == 'packed' else b'ZKA1')
        assert eng.quorum_verify_batch(k, w[0], bundles) == ([1] * Q, [0] * Q, [NONE] * Q)
        assert X.eng.quorum_verify_batch(k, w[0], bundles)[0] == [0] * Q   # another h, another layout
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. lane and window edges
def test_69_members_and_69_pairs_cross_a_wave(X):
    Q, k = 23, 3
    w, bundles = _honest(X, Q, k, b'wave')
    assert bundles == _recipe(X.eng, k, *w)[0]
    assert X.eng.quorum_verify_batch(k, w[0], bundles) == ([1] * Q, [0] * Q, [NONE] * Q)


def test_one_quorum_of_sixteen(X):
    """120 pairs from one quorum; 16 different signers need more than 8 keys: a ring of 32"""
    Z, k = X.Z, 16
    probe = Z.Engine(0)
    probe.synth_params(S)
    ring, msg, sig, pk, which, _ = probe.synth_workload(S + 1, 32, 32)
    probe.close()
    first = {}
    for b, s in enumerate(which):
        first.setdefault(s, b)
    assert len(first) >= k
    idx = [first[s] for s in sorted(first)[:k]]
    cut = lambda a, n: b''.join(a[n * b:n * b + n] for b in idx)
    w = (cut(msg, 32), cut(sig, 64), cut(pk, 64), [which[b] for b in idx], X.DC.seeds_for(b'att16', k), X.DC.seeds_for(b'pair16', 120))
    eng = _engine(Z, X.par, ring, 32)
    try:
        bundles, st, mst = eng.quorum_prove_batch(k, *w)
        assert st == [0] and mst == [0] * k
        assert bundles == _recipe(eng, k, *w)[0]
        assert eng.quorum_verify_batch(k, w[0], bundles) == ([1], [0], [NONE])
        # the last pair, (14, 15), tampered with
        bad = bundles[0][:-9] + bytes([bundles[0][-9] ^ 1]) + bundles[0][-8:]
        assert eng.quorum_verify_batch(k, w[0], [bad]) == ([0], [0], [k + 119])
    finally:
        eng.close()


def test_quorums_straddle_chunk_edges(X):
    Q, k = 5, 3
    w, bundles = _honest(X, Q, k, b'chunk')
    eng = _engine(X.Z, X.par, X.ring, NKEYS)
    try:
        eng.set_chunk(4)   # windows of two quorums, chunks of four members and of four pairs
        got, st, mst = eng.quorum_prove_batch(k, *w)
        assert st == [0] * Q and got == bundles
        assert eng.quorum_verify_batch(k, w[0], bundles) == ([1] * Q, [0] * Q, [NONE] * Q)
    finally:
        eng.close()


# ------------------------------------------------------------------ 3. the verifier
@pytest.fixture(scope='module')
def H(X):
    """three honest quorums of three"""
    h = Ctx()
    h.k, h.Q = 3, 3
    h.w, h.bundles = _honest(X, h.Q, h.k, b'verify')
    return h


def _flip(b, at):
    return b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]


def test_byte_flips_name_the_member_or_the_pair(X, H):
    sys.path.insert(0, os.path.join(ROOT, 'oracle'))
    import coracle as CO
    k, msg = H.k, H.w[0]
    octx = CO.OracleCtx(X.par[0], X.par[1], X.par[2], SEC)
    octx.set_ring(X.ring, NKEYS)
    rnd = random.Random(20)
    members, pairs = _members(H.bundles[1], k)
    starts = [16 + sum(len(m) for m in members[:j]) for j in range(k)]
    mutants, want = [], []
    for j in range(k):   # a seeded flip inside member j: the oracle's verdict and status for that mutant
        at = rnd.randrange(32, len(members[j]))
        mutants.append(_flip(H.bundles[1], starts[j] + at))
        ok, st = octx.verify_batch(msg[32 * (k + j):32 * (k + j + 1)], [_flip(members[j], at)], nthreads=1)
        assert ok == [0]
        want.append((0, st[0], j))
    for p in range(len(pairs)):   # a flip inside pair p's responses
        mutants.append(_flip(H.bundles[1], len(H.bundles[1]) - PAIR * (len(pairs) - p) + 600))
        want.append((0, 0, k + p))
    for m, (ok, st, bad) in zip(mutants, want):
        got = X.eng.quorum_verify_batch(k, msg, [H.bundles[0], m, H.bundles[2]])
        assert got == ([1, ok, 1], [0, st, 0], [NONE, bad, NONE]), (got, bad)


def test_swapped_members_fail_at_a_pair(X, H):
    """members 0 and 1 swapped in place, their message hashes alongside: every attestation verifies, the proof of pair (0, 1) does not (it is directional)"""
    k, msg = H.k, H.w[0]
    members, pairs = _members(H.bundles[0], k)
    body = members[1] + members[0] + members[2] + b''.join(pairs)
    forged = _header(16 + len(body), k) + body
    msg2 = msg[32:64] + msg[0:32] + msg[64:]
    assert X.eng.verify_batch(msg2[:96], [members[1], members[0], members[2]]) == ([1] * 3, [0] * 3)
    assert X.eng.quorum_verify_batch(k, msg2, [forged] + H.bundles[1:]) == ([0, 1, 1], [0, 0, 0], [k + 0, NONE, NONE])


def test_spliced_attestation_by_the_same_signer_fails_at_its_first_pair(X):
    """member 2 taken from another honest bundle where it is signer 0's attestation again: all three attestations are valid, pair (0, 2) is not"""
    k, s = 3, X.signers
    rows_a, rows_b = _pick(X, [s[0], s[1], s[2]], 0), _pick(X, [s[3], s[4], s[0]], 1)
    cat = lambda i: rows_a[i] + rows_b[i]
    bundles, st, _ = X.eng.quorum_prove_batch(k, cat(0), cat(1), cat(2), cat(3), X.DC.seeds_for(b'att-splice', 6), X.DC.seeds_for(b'pair-splice', 6))
    assert st == [0, 0]
    (a, pa), (b, _) = _members(bundles[0], k), _members(bundles[1], k)
    body = a[0] + a[1] + b[2] + b''.join(pa)
    msg = rows_a[0][:64] + rows_b[0][64:96]
    assert X.eng.verify_batch(msg, [a[0], a[1], b[2]]) == ([1] * 3, [0] * 3)
    assert X.eng.quorum_verify_batch(k, msg, [_header(16 + len(body), k) + body]) == ([0], [0], [k + 1])


def test_header_mutants_fail_by_the_encoding_rules(X, H):
    k, msg, b = H.k, H.w[0], H.bundles[1]
    total = len(b)
    inner = int.from_bytes(b[20:24], 'big')
    mutants = {
        'magic': b'ZKQ2' + b[4:],
        'k + 1': _header(total, k + 1) + b[16:],
        'k - 1': _header(total, k - 1) + b[16:],
        'total_len + 4': _header(total + 4, k) + b[16:],
        'total_len - 4': _header(total - 4, k) + b[16:],
        'reserved': b[:15] + b'\x01' + b[16:],
        'truncated': b[:-4],
        'two bytes short': b[:-2],
        'inner total_len + 4': b[:20] + (inner + 4).to_bytes(4, 'big') + b[24:],
        'inner magic': b[:16] + b'ZK1P' + b[20:],
    }
    for name, m in mutants.items():
        # the bundles lie back to back: behind a slot whose length is no multiple of 4 the next slot's OFFSET is no multiple of 4, which is itself one of
        # the encoding rules -- that neighbour is ZK_E_BAD_ENCODING by its own slot, every other neighbour is unaffected
        behind = (1, 0, NONE) if len(m) % 4 == 0 else (0, E_BAD, 0)
        got = X.eng.quorum_verify_batch(k, msg, [H.bundles[0], m, H.bundles[2]])
        assert got == ([1, 0, behind[0]], [0, E_BAD, behind[1]], [NONE, 0, behind[2]]), (name, got)
    # the same mutant in the last slot: both neighbours in front of it are accepted
    m3 = msg[:96] + msg[192:] + msg[96:192]
    assert X.eng.quorum_verify_batch(k, m3, [H.bundles[0], H.bundles[2], b[:-2]]) == ([1, 1, 0], [0, 0, E_BAD], [NONE, NONE, 0])
    assert X.eng.quorum_verify_batch(k, msg, H.bundles, want_first_bad=False) == ([1] * 3, [0] * 3, None)
    assert X.eng.quorum_verify_batch(k, msg, H.bundles, vseeds=X.DC.seeds_for(b'vseeds', 9))[0] == [1] * 3


# ------------------------------------------------------------------ 4. the prover's statuses
def _three(x, middle, name):
    """quorums 0 and 2 honest, `middle` = (msg, sig, pk, which) of quorum 1"""
    s = x.signers
    rows = [_pick(x, [s[0], s[1], s[2]], 0), middle, _pick(x, [s[2], s[3], s[4]], 1)]
    cat = lambda i, sel: sum((rows[q][i] for q in sel), []) if i == 3 else b''.join(rows[q][i] for q in sel)
    seeds, pair_seeds = x.DC.seeds_for(b'att' + name, 9), x.DC.seeds_for(b'pair' + name, 9)
    sub = lambda a, sel: b''.join(a[96 * q:96 * q + 96] for q in sel)
    call = lambda sel, **kw: x.eng.quorum_prove_batch(3, cat(0, sel), cat(1, sel), cat(2, sel), cat(3, sel), sub(seeds, sel), **kw)
    return call, pair_seeds, sub


def test_a_repeated_signer_is_refused_and_its_neighbours_do_not_notice(X):
    s = X.signers
    rep = _pick(X, [s[5 % len(s)], s[1]], 0)
    again = _pick(X, [s[5 % len(s)]], 1)
    middle = tuple(rep[i] + again[i] for i in range(4))
    call, pair_seeds, sub = _three(X, middle, b'repeat')
    bundles, st, mst = call([0, 1, 2], pair_seeds=pair_seeds)
    assert st == [0, E_ARG, 0] and mst == [0] * 9 and bundles[1] is None
    alone, st2, _ = call([0, 2], pair_seeds=sub(pair_seeds, [0, 2]))
    assert st2 == [0, 0] and [bundles[0], bundles[2]] == alone


@pytest.mark.parametrize('wrong', ['another key', 'outside the ring'])
def test_a_member_with_a_wrong_index_gets_prove_batch_s_status(X, wrong):
    """member 1 of the middle quorum names another ring entry, or none: per_member_status is zk_prove_batch's status for that member, and where it is not 0
    the quorum fails with it.  (zk_prove_batch does not screen witnesses: an index inside the ring that names another key is status 0 there, and the
    attestation it makes does not verify -- the bundle says so at verify time, naming member 1.)"""
    s = X.signers
    msg, sig, pk, which = _pick(X, [s[0], s[3], s[4]], 2)
    other = next(i for i in range(NKEYS) if i != which[1]) if wrong == 'another key' else NKEYS + 3
    middle = (msg, sig, pk, [which[0], other, which[2]])
    try:
        _, want = X.eng.prove_batch(*middle, seeds=X.DC.seeds_for(b'attwhich', 9)[96:192])
    except X.Z.ZkError as e:   # the whole call is refused: so is the quorum call
        with pytest.raises(X.Z.ZkError) as e2:
            _three(X, middle, b'which')[0]([0, 1, 2])
        assert e2.value.status == e.status
        return
    print('zk_prove_batch statuses for the middle quorum (%s): %s' % (wrong, want))
    assert want[0] == 0 and want[2] == 0 and (want[1] != 0 or wrong == 'another key')
    call, pair_seeds, sub = _three(X, middle, b'which')
    bundles, st, mst = call([0, 1, 2], pair_seeds=pair_seeds)
    assert st == [0, want[1], 0] and mst == [0] * 3 + want + [0] * 3 and (bundles[1] is None) == (want[1] != 0)
    alone, _, _ = call([0, 2], pair_seeds=sub(pair_seeds, [0, 2]))
    assert [bundles[0], bundles[2]] == alone
    assert call([0, 1, 2], pair_seeds=pair_seeds, want_member_status=False)[:2] == (bundles, st)
    if want[1] == 0:
        msgs = _three_msgs(X)
        assert X.eng.quorum_verify_batch(3, msgs[0] + msg + msgs[1], bundles) == ([1, 0, 1], [0, 0, 0], [NONE, 1, NONE])


def test_a_pair_stream_one_block_short(X):
    s = X.signers
    call, _, _ = _three(X, _pick(X, [s[1], s[2], s[3]], 3), b'short')
    blk = lambda q, p, j: hashlib.sha256(b'quorum-stream' + bytes([q, p, j])).digest()
    row = lambda q, p: b''.join(b'\xff' * 32 if (q, p, j) == (1, 2, 0) else blk(q, p, j) for j in range(8))   # a rejected fill: pair (1, 2) of quorum 1 needs nine blocks
    streams = lambda sel: b''.join(row(q, p) for q in sel for p in range(3))
    bundles, st, mst = call([0, 1, 2], pair_streams=streams([0, 1, 2]), pair_stream_blocks=8)
    assert st == [0, E_RNG, 0] and mst == [0] * 9 and bundles[1] is None
    alone, st2, _ = call([0, 2], pair_streams=streams([0, 2]), pair_stream_blocks=8)
    assert st2 == [0, 0] and [bundles[0], bundles[2]] == alone
    assert X.eng.quorum_verify_batch(3, b''.join(_three_msgs(X)), alone)[0] == [1, 1]


def _three_msgs(x):
    s = x.signers
    return [_pick(x, [s[0], s[1], s[2]], 0)[0], _pick(x, [s[2], s[3], s[4]], 1)[0]]


# ------------------------------------------------------------------ 5. the device forms
def _up(b, tail=16):
    import torch
    return torch.frombuffer(bytearray(bytes(b) + bytes(tail)), dtype=torch.uint8).to(torch.device('cuda:0'))


def test_device_forms_on_torch_buffers(X, H):
    import numpy as np
    import torch
    k, Q = H.k, H.Q
    msg, sig, pk, which, seeds, pair_seeds = H.w
    cap = X.eng.quorum_proof_max_size(k) * Q
    d = [_up(msg), _up(sig), _up(pk), _up(struct.pack('<%dI' % len(which), *which)), _up(seeds), _up(pair_seeds)]
    d_out = torch.full((cap + 64,), 0x5a, dtype=torch.uint8, device='cuda:0')
    d_off = torch.full((8 * (Q + 1) + 16,), 0x5a, dtype=torch.uint8, device='cuda:0')
    d_st = torch.full((4 * Q + 16,), 0x5a, dtype=torch.uint8, device='cuda:0')
    d_mst = torch.full((4 * Q * k + 16,), 0x5a, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    X.eng.quorum_prove_batch_device(Q, k, *[t.data_ptr() for t in d], d_out.data_ptr(), cap, d_off.data_ptr(), d_st.data_ptr(), d_mst.data_ptr())
    torch.cuda.synchronize()
    off = np.frombuffer(bytes(d_off.cpu().numpy())[:8 * (Q + 1)], dtype=np.uint64)
    out = bytes(d_out.cpu().numpy())
    assert [out[int(off[q]):int(off[q + 1])] for q in range(Q)] == H.bundles
    assert out[int(off[Q]):int(off[Q]) + 64] == b'\x5a' * 64 and out[cap:] == b'\x5a' * 64
    assert bytes(d_st.cpu().numpy()) == bytes(4 * Q) + b'\x5a' * 16 and bytes(d_mst.cpu().numpy()) == bytes(4 * Q * k) + b'\x5a' * 16
    assert bytes(d_off.cpu().numpy())[8 * (Q + 1):] == b'\x5a' * 16
    # the verifier on the prover's buffers, then with a tampered pair and a tampered header; no seeds, then seeds; with and without first_bad
    bundles = [H.bundles[0], _flip(H.bundles[1], len(H.bundles[1]) - 100), _header(len(H.bundles[2]), k + 1) + H.bundles[2][16:]]
    host = X.eng.quorum_verify_batch(k, msg, bundles)
    assert host == ([1, 0, 0], [0, 0, E_BAD], [NONE, k + 2, 0])
    blob = b''.join(bundles)
    offs = [0]
    for b in bundles:
        offs.append(offs[-1] + len(b))
    d_b, d_boff, d_seeds = _up(blob, 0), _up(struct.pack('<%dQ' % (Q + 1), *offs), 0), _up(X.DC.seeds_for(b'dv', Q * k), 0)
    for vs, fb in ((None, True), (d_seeds.data_ptr(), False)):
        d_ok = torch.full((Q + 8,), 0x5a, dtype=torch.uint8, device='cuda:0')
        d_vst = torch.full((4 * Q + 16,), 0x5a, dtype=torch.uint8, device='cuda:0')
        d_bad = torch.full((4 * Q + 16,), 0x5a, dtype=torch.uint8, device='cuda:0')
        torch.cuda.synchronize()
        X.eng.quorum_verify_batch_device(Q, k, d[0].data_ptr(), d_b.data_ptr(), d_boff.data_ptr(), vs, d_ok.data_ptr(), d_vst.data_ptr(), d_bad.data_ptr() if fb else None)
        torch.cuda.synchronize()
        ok, vst, bad = bytes(d_ok.cpu().numpy()), bytes(d_vst.cpu().numpy()), bytes(d_bad.cpu().numpy())
        assert list(ok[:Q]) == host[0] and ok[Q:] == b'\x5a' * 8
        assert list(np.frombuffer(vst[:4 * Q], dtype=np.int32)) == host[1] and vst[4 * Q:] == b'\x5a' * 16
        assert bad == (struct.pack('<%dI' % Q, *host[2]) + b'\x5a' * 16 if fb else b'\x5a' * (4 * Q + 16))
    # a misaligned pointer is refused
    with pytest.raises(X.Z.ZkError) as e:
        X.eng.quorum_verify_batch_device(Q, k, d[0].data_ptr() + 1, d_b.data_ptr(), d_boff.data_ptr(), None, d_ok.data_ptr(), d_vst.data_ptr(), None)
    assert e.value.status == E_ARG


# ------------------------------------------------------------------ 6. call-level rules
def test_call_level_rules(X, H):
    import ctypes as C
    Z, k, Q = X.Z, H.k, H.Q
    msg = H.w[0]
    for bad_k in (1, 17, 0):
        assert X.eng.quorum_pair_count(bad_k) == 0 and X.eng.quorum_proof_max_size(bad_k) == 0
        with pytest.raises(Z.ZkError) as e:
            X.eng.quorum_verify_batch(bad_k, msg, H.bundles)
        assert e.value.status == E_ARG
    assert [X.eng.quorum_pair_count(k_) for k_ in (2, 3, 16)] == [1, 3, 120]
    w1 = tuple(a[:n] for a, n in zip(H.w, (32, 64, 64, 1, 32, 0)))
    w17 = _workload(X, 1, 17, b'k17')
    for bad_k, w in ((1, w1), (17, w17)):
        with pytest.raises(Z.ZkError) as e:
            X.eng.quorum_prove_batch(bad_k, *w, cap=1 << 20)
        assert e.value.status == E_ARG
    # no params; params but no ring
    eng = Z.Engine(0)
    try:
        for step in range(2):
            assert eng.quorum_proof_max_size(k) == 0
            with pytest.raises(Z.ZkError) as e:
                eng.quorum_prove_batch(k, *H.w, cap=1 << 24)
            assert e.value.status == E_BUF
            with pytest.raises(Z.ZkError) as e:
                eng.quorum_verify_batch(k, msg, H.bundles)
            assert e.value.status == E_BUF
            eng.set_params(X.par[0], X.par[1], X.par[2], SEC)
    finally:
        eng.close()
    # Q = 0
    assert X.eng.quorum_prove_batch(k, b'', b'', b'', []) == ([], [], [])
    assert X.eng.quorum_verify_batch(k, b'', []) == ([], [], [])
    # out_cap one byte short: nothing is written
    L, n, P = X.eng.L, Q * k, 3
    need = X.eng.quorum_proof_max_size(k) * Q
    out = C.create_string_buffer(b'\x5a' * need, need)
    off = (C.c_uint64 * (Q + 1))(*([0x5a5a5a5a] * (Q + 1)))
    st = (C.c_int32 * Q)(*([0x5a5a] * Q))
    mst = (C.c_int32 * n)(*([0x5a5a] * n))
    which = (C.c_uint32 * n)(*H.w[3])
    r1, keep1 = X.eng._rng(n, H.w[4], None, 0)
    r2, keep2 = X.eng._rng(Q * P, H.w[5], None, 0)
    rc = L.zk_quorum_prove_batch(X.eng.h, Q, k, H.w[0], H.w[1], H.w[2], which, C.byref(r1), C.byref(r2), out, need - 1, off, st, mst)
    assert rc == E_BUF
    assert out.raw == b'\x5a' * need and list(off) == [0x5a5a5a5a] * (Q + 1) and list(st) == [0x5a5a] * Q and list(mst) == [0x5a5a] * n
    assert L.zk_quorum_prove_batch(X.eng.h, Q, k, H.w[0], H.w[1], H.w[2], which, C.byref(r1), C.byref(r2), out, need, off, st, None) == 0   # per_member_status NULL
    assert [out.raw[off[q]:off[q + 1]] for q in range(Q)] == H.bundles and list(st) == [0] * Q
    # NULL for a required pointer
    assert L.zk_quorum_prove_batch(X.eng.h, Q, k, H.w[0], H.w[1], H.w[2], which, C.byref(r1), None, out, need, off, st, None) == E_ARG
    assert L.zk_quorum_verify_batch(X.eng.h, Q, k, msg, b''.join(H.bundles), None, None, out, st, None) == E_ARG
    # the timing families: the existing ones plus the new kernels'
    X.eng.set_timing(1)
    try:
        X.eng.quorum_prove_batch(k, *H.w)
        names = set(X.eng.last_timing()[1])
        assert {'quorum_blinders', 'quorum_gather', 'quorum_layout', 'distinct_respond', 'tom_commit', 'hash'} <= names, names
        X.eng.quorum_verify_batch(k, msg, H.bundles)
        names = set(X.eng.last_timing()[1])
        assert {'quorum_walk', 'quorum_verdict', 'distinct_parse', 'distinct_short', 'distinct_long'} <= names, names
    finally:
        X.eng.set_timing(0)


# ------------------------------------------------------------------ 7. wipe
def test_wipe_and_a_failed_call_leave_no_nonzero_word(X, H):
    """zk_test_counter 11 counts the nonzero words of every witness-flagged buffer, the quorum staging (gathered keys and blinders) among them"""
    eng = _engine(X.Z, X.par, X.ring, NKEYS)
    try:
        assert eng.quorum_prove_batch(H.k, *H.w)[0] == H.bundles
        assert 0 < eng.test_counter(11) < 1 << 63
        eng.wipe()
        assert eng.test_counter(11) == 0
        assert eng.quorum_prove_batch(H.k, *H.w)[0] == H.bundles
        assert eng.test_counter(11) > 0
        with pytest.raises(X.Z.ZkError) as e:   # a failed call wipes by itself
            eng.quorum_prove_batch(H.k, *H.w, cap=1000)
        assert e.value.status == E_BUF and eng.test_counter(11) == 0
        assert eng.quorum_prove_batch(H.k, *H.w)[0] == H.bundles
    finally:
        eng.close()
