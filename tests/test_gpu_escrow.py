"""-m gpu: zk_ctx_set_auditor / zk_escrow_keygen / zk_escrow_prove_batch / zk_escrow_verify_batch / zk_escrow_open_batch.  The expected bytes, verdicts and
indices are the Python statement's (tests/escrow_common.py).  secLevel 20, 16-bit combs unless a test says otherwise; commitments come from
eng.test_tom_commit."""
import hashlib
import importlib.util
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

SEC = 20
E_BAD, E_RNG, E_BUF, E_ARG, E_OPENING = 10, 11, 12, 14, 16
B67 = 67
NONE = 0xffffffff


class Ctx:
    pass


def _engine(Z, par, bits=16, chunk=64):
    eng = Z.Engine(0)
    eng.set_comb_bits(bits)
    eng.set_params(*par, SEC)
    eng.set_chunk(chunk)   # 67 tags: two chunks, a wave boundary inside the first
    return eng


@pytest.fixture(scope='module')
def X():
    import escrow_common as EC
    import zkp_ecdsa_amd as Z
    x = Ctx()
    x.Z, x.EC, x.R = Z, EC, EC.R
    boot = Z.Engine(0)
    x.par = boot.synth_params(EC.PARAM_SEED)
    boot.close()
    eng = x.eng = _engine(Z, x.par)
    x.pp = EC.MC.oracle_params(x.par[1], x.par[2])
    x.a = int.from_bytes(EC.tag(b'auditor', 0), 'big')   # (not reduced: the engine reduces)
    x.a32 = x.a.to_bytes(32, 'big')
    x.A = EC.keygen(x.pp, x.a)
    x.A72 = x.R._tp(x.A)
    assert eng.escrow_keygen(x.a32) == x.A72
    eng.set_auditor(x.A72)
    # the ring of 300 keys and the 67 tags over planted indices (0, 299 and repeats among them), shared: inputs, the engine's tags, the statement's bytes
    x.ring = EC.MC.RING300
    x.planted = [0, 299, 7, 7, 150] + [(37 * b + 11) % 300 for b in range(5, B67)]
    x.x = [x.ring[i] for i in x.planted]
    _, x.r, x.seeds = EC.workload(b'w67', B67)
    x.c = eng.test_tom_commit(x.x, x.r)
    x.tags, x.st = eng.escrow_prove_batch(EC.be32(x.x), x.c, EC.be32(x.r), seeds=x.seeds)
    x.want = [EC.prove(x.pp, x.A, x.x[b], x.c[b], x.r[b], x.R.SeedRng(x.seeds[32 * b:32 * b + 32])) for b in range(B67)]
    eng.set_ring(EC.MC.ring_bytes(x.ring), 300)
    yield x
    eng.close()


# ------------------------------------------------------------------ 1. prove: bytes
def test_67_tags_equal_the_python_statement(X):
    assert X.eng.escrow_tag_size() == 472
    assert X.st == [0] * B67
    for b in range(B67):
        assert X.tags[b] == X.want[b], b
    one = X.eng.escrow_prove_batch(X.EC.be32(X.x[5:6]), X.c[5:6], X.EC.be32(X.r[5:6]), seeds=X.seeds[160:192])   # B = 1
    assert one == ([X.want[5]], [0])


@pytest.mark.parametrize('bits', [16, 12])
def test_bytes_at_two_comb_widths_and_in_both_rng_modes(X, bits):
    """12-bit context combs: the (g, A) set builds g's table of its own; the stream mode takes the same draws from explicit blocks"""
    EC = X.EC
    eng = X.eng if bits == 16 else _engine(X.Z, X.par, bits)
    try:
        if bits != 16:
            eng.set_auditor(X.A72)
            assert eng.escrow_prove_batch(EC.be32(X.x), X.c, EC.be32(X.r), seeds=X.seeds) == (X.tags, [0] * B67)
        blocks = [[hashlib.sha256(X.seeds[32 * b:32 * b + 32] + k.to_bytes(8, 'big')).digest() for k in range(4)] for b in range(B67)]
        got = eng.escrow_prove_batch(EC.be32(X.x), X.c, EC.be32(X.r), streams=b''.join(b''.join(r) for r in blocks), stream_blocks=4)
        assert got == (X.tags, [0] * B67)
        assert eng.escrow_verify_batch(X.c, X.tags) == ([1] * B67, [0] * B67)
    finally:
        if bits != 16:
            eng.close()


def test_uniform_library_gives_the_same_bytes(X):
    Z = X.Z
    uni = os.path.join(os.path.dirname(Z.LIB_PATH), 'libzkattest_hip_uniform.so')
    assert os.path.exists(uni), 'the uniform build is not there (make -C zkp-ecdsa_amd/csrc uniform)'
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'escrow_uniform_check.py')], env=dict(os.environ, ZKATTEST_LIB=uni),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    rec = json.loads(out.stdout.decode().strip().splitlines()[-1])
    assert rec['lib'].endswith('_uniform.so') and rec['sha256'] == hashlib.sha256(b''.join(X.tags)).hexdigest()
    assert rec['index'] == X.planted


# ------------------------------------------------------------------ 2. prove: refusals
def test_prover_refusals(X):
    eng, EC, Z = X.eng, X.EC, X.Z
    n = 5
    keys, r, c = list(X.x[:n]), list(X.r[:n]), list(X.c[:n])
    r[1] = (r[1] + 1) % EC.Q                                        # a wrong blinder
    c[3] = c[3][:35] + bytes([c[3][35] ^ 1]) + c[3][36:]            # one bit of com's x flipped: off the curve
    tags, st = eng.escrow_prove_batch(EC.be32(keys), c, EC.be32(r), seeds=X.seeds[:32 * n])
    assert st == [0, E_OPENING, 0, E_BAD, 0]
    assert [tags[b] for b in (0, 2, 4)] == [X.tags[b] for b in (0, 2, 4)]
    raw = eng.escrow_last_raw
    assert raw[472:944] == bytes(472) and raw[3 * 472:4 * 472] == bytes(472)
    # a short stream: block 0 rejected (>= q), so four blocks do not hold the four draws; tag 1 has its four
    ff = b'\xff' * 32
    blk = [[hashlib.sha256(b'escrow-stream' + bytes([b, k])).digest() for k in range(5)] for b in range(2)]
    rows = [[ff] + blk[0][:4], blk[1]]
    full, st5 = eng.escrow_prove_batch(EC.be32(X.x[:2]), X.c[:2], EC.be32(X.r[:2]), streams=b''.join(b''.join(w) for w in rows), stream_blocks=5)
    assert st5 == [0, 0]
    for b in range(2):
        assert full[b] == EC.prove(X.pp, X.A, X.x[b], X.c[b], X.r[b], X.R.StreamRng(rows[b])), b
    short, st4 = eng.escrow_prove_batch(EC.be32(X.x[:2]), X.c[:2], EC.be32(X.r[:2]), streams=b''.join(b''.join(w[:4]) for w in rows), stream_blocks=4)
    assert st4 == [E_RNG, 0] and short[1] == full[1] and eng.escrow_last_raw[:472] == bytes(472)
    # out_cap one byte short: ZK_E_BUFFER with nothing written (device form on poisoned buffers)
    rc, out, stw = _dev_prove(X, eng, range(n), cap=472 * n - 1)
    assert rc == E_BUF and out == b'\x5a' * len(out) and stw == b'\x5a' * len(stw)
    with pytest.raises(Z.ZkError) as e:
        eng.escrow_prove_batch(EC.be32(X.x[:n]), X.c[:n], EC.be32(X.r[:n]), seeds=X.seeds[:32 * n], cap=472 * n - 1)
    assert e.value.status == E_BUF
    assert eng.escrow_prove_batch(b'', [], b'', seeds=b'') == ([], [])
    assert eng.escrow_verify_batch([], []) == ([], []) and eng.escrow_open_batch(X.a32, []) == ([], [])


def test_set_auditor_and_the_calls_without_one(X):
    Z, EC = X.Z, X.EC
    P2, _ = EC.small_order_points()
    eng = Z.Engine(0)
    try:
        eng.set_comb_bits(16)
        for call in (lambda: eng.set_auditor(X.A72), lambda: eng.escrow_keygen(X.a32)):   # before zk_ctx_set_params
            with pytest.raises(Z.ZkError) as e:
                call()
            assert e.value.status == E_BUF
        eng.set_params(*X.par, SEC)
        p = EC.TOM.p
        bad = [(X.A72[:71] + bytes([X.A72[71] ^ 1]), E_BAD),                                  # off the curve
               (b'\x01' + X.A72[1:], E_BAD),                                                  # a padding byte set
               (p.to_bytes(36, 'big') + X.A72[36:], E_BAD),                                   # x = p
               (X.R._tp(EC.TOM.identity()), E_ARG),                                           # the identity
               (X.R._tp(X.A.add(P2)), E_ARG)]                                                 # A + (a point of order 2): q A != O
        for key, want in bad:
            with pytest.raises(Z.ZkError) as e:
                eng.set_auditor(key)
            assert e.value.status == want, (key.hex(), want)
        with pytest.raises(Z.ZkError) as e:
            eng.escrow_keygen(EC.Q.to_bytes(32, 'big'))   # a = 0 mod q
        assert e.value.status == E_ARG
        # no auditor: ZK_E_BUFFER with nothing written
        rc, out, stw = _dev_prove(X, eng, range(3))
        assert rc == E_BUF and out == b'\x5a' * len(out) and stw == b'\x5a' * len(stw)
        for call in (lambda: eng.escrow_verify_batch(X.c[:1], X.tags[:1]), lambda: eng.escrow_open_batch(X.a32, X.tags[:1])):
            with pytest.raises(Z.ZkError) as e:
                call()
            assert e.value.status == E_BUF
        # another auditor, then the right one: a second call replaces the key
        a2 = X.a + 1
        eng.set_auditor(eng.escrow_keygen(a2.to_bytes(32, 'big')))
        assert eng.escrow_verify_batch(X.c[:3], X.tags[:3]) == ([0] * 3, [0] * 3)   # a tag made for A gives ok = 0 under A'
        for b in range(3):
            assert EC.verify(X.pp, EC.keygen(X.pp, a2), X.c[b], X.tags[b]) == (0, 0)
        eng.set_auditor(X.A72)
        assert eng.escrow_verify_batch(X.c[:3], X.tags[:3]) == ([1] * 3, [0] * 3)
        eng.set_params(*X.par, SEC)   # drops the key
        with pytest.raises(Z.ZkError) as e:
            eng.escrow_verify_batch(X.c[:1], X.tags[:1])
        assert e.value.status == E_BUF
        eng.set_auditor(X.A72)
        assert eng.escrow_verify_batch(X.c[:1], X.tags[:1]) == ([1], [0])
        with pytest.raises(Z.ZkError) as e:   # an auditor but no active ring
            eng.escrow_open_batch(X.a32, X.tags[:1])
        assert e.value.status == E_BUF
    finally:
        eng.close()


# ------------------------------------------------------------------ 3. verify
def test_verifier_all_67_and_every_mutant_against_the_python_statement(X):
    EC = X.EC
    assert X.eng.escrow_verify_batch(X.c, X.tags) == ([1] * B67, [0] * B67)
    idx = [0, 1, 2, 66]
    others = X.eng.test_tom_commit([(X.x[b] + 1) % EC.Q for b in idx], [X.r[b] for b in idx])
    rows = []
    for k, b in enumerate(idx):
        rows += EC.mutants(X.tags[b], X.c[b], X.c[(b + 1) % B67], others[k])
    # a response with room for + q below 2^256 (q is close to 2^256): a commitment with blinder 0 has t_r = k_r, and the stream hands a small k_r in
    blocks = [EC.tag(b'small', 0), EC.tag(b'small', 1), (0x1234567 + (1 << 200)).to_bytes(32, 'big'), EC.tag(b'small', 3)]
    c0 = X.eng.test_tom_commit(X.x[:1], [0])
    small, st = X.eng.escrow_prove_batch(EC.be32(X.x[:1]), c0, EC.be32([0]), streams=b''.join(blocks), stream_blocks=4)
    assert st == [0] and small[0] == EC.prove(X.pp, X.A, X.x[0], c0[0], 0, X.R.StreamRng(blocks))
    rows += EC.mutants(small[0], c0[0], X.c[1], others[0])
    assert ('t_r + q', c0[0], EC.sc_plus(small[0], 1, EC.Q)) in rows
    names = {r[0] for r in rows}
    assert {'E1 := another point', 'E2 := another point', 'T1 := another point', 'T2 := another point', 'T3 := another point', 't_x + 1', 't_r + 1', 't_rho + 1',
            'a wrong com', 'magic', 'total_len', 'reserved', 'off-curve coordinate'} <= names
    assert any(n.endswith('+ q') for n in names), 'no response of these tags leaves room for + q below 2^256'
    ok, st = X.eng.escrow_verify_batch([r[1] for r in rows], [r[2] for r in rows])
    for i, (name, c, t) in enumerate(rows):   # no mutant is skipped
        want = EC.verify(X.pp, X.A, c, t)
        print(i, name, 'engine', (ok[i], st[i]), 'statement', want)
        assert (ok[i], st[i]) == want, (i, name)
        if name == 'honest' or name.endswith('+ q'):
            assert want == (1, 0), (i, name)
        elif name in ('magic', 'total_len', 'reserved', 'off-curve coordinate'):
            assert want == (0, E_BAD), (i, name)
        else:
            assert want == (0, 0), (i, name)


# ------------------------------------------------------------------ 4. open
def test_open_every_planted_index_and_the_rules_around_it(X):
    eng, EC, R = X.eng, X.EC, X.R
    assert {0, 299} <= set(X.planted) and len(set(X.planted)) < B67
    assert eng.escrow_open_batch(X.a32, X.tags) == (X.planted, [0] * B67)
    table = EC.ring_points(X.pp, X.ring)
    for b in (0, 1, 2, 3, 66):
        assert EC.open_tag(X.a, X.tags[b], table) == (X.planted[b], 0), b
    # a key that is not in the ring; a point of order 2 and of order 4 added to E2; a damaged header
    P2, P4 = EC.small_order_points()
    xo, ro, so = EC.workload(b'outside', 1)
    co = eng.test_tom_commit(xo, ro)
    outside, st = eng.escrow_prove_batch(EC.be32(xo), co, EC.be32(ro), seeds=so)
    assert st == [0]
    def e2_plus(t, S):
        o = EC.PT[1]
        return t[:o] + R._tp(EC.point(t[o:o + 72]).add(S)) + t[o + 72:]
    batch = [outside[0], e2_plus(X.tags[1], P2), e2_plus(X.tags[4], P4), b'ZKT2' + X.tags[2][4:], X.tags[2], e2_plus(X.tags[0], P4.add(P2))]
    want = ([NONE, X.planted[1], X.planted[4], NONE, X.planted[2], X.planted[0]], [0, 0, 0, E_BAD, 0, 0])
    assert eng.escrow_open_batch(X.a32, batch) == want
    assert [EC.open_tag(X.a, t, table) for t in batch] == list(zip(*want))
    # a wrong secret: ZK_E_OPENING at call level, the outputs untouched (device form on poisoned buffers)
    rc, idx, stw = _dev_open(X, eng, ((X.a + 1) % (1 << 256)).to_bytes(32, 'big'), X.tags[:5])
    assert rc == E_OPENING and idx == b'\x5a' * len(idx) and stw == b'\x5a' * len(stw)
    with pytest.raises(X.Z.ZkError) as e:
        eng.escrow_open_batch(((X.a + 1) % (1 << 256)).to_bytes(32, 'big'), X.tags[:5])
    assert e.value.status == E_OPENING


def test_open_a_key_at_two_indices_gives_the_lower(X):
    eng, EC = X.eng, X.EC
    ring = list(X.ring)
    ring[20] = ring[150]   # tag 4 carries ring[150]
    ring[299] = ring[7]    # tags 2 and 3 carry ring[7]; tag 1 carried the old ring[299]
    eng.set_ring(EC.MC.ring_bytes(ring), 300)
    try:
        assert eng.escrow_open_batch(X.a32, X.tags[:5]) == ([0, NONE, 7, 7, 20], [0] * 5)
    finally:
        eng.set_ring(EC.MC.ring_bytes(X.ring), 300)


# ------------------------------------------------------------------ 5. end to end
def test_end_to_end_attestation_tag_verify_open_and_rering(X):
    Z, EC = X.Z, X.EC
    NB, S = 3, 77
    eng = Z.Engine(0)
    try:
        eng.set_comb_bits(16)
        par = eng.synth_params(S)
        eng.set_params(*par, SEC)
        ringA, msg, sig, pk, which, seeds = eng.synth_workload(S, 16, NB)
        keysA = [int.from_bytes(ringA[32 * i:32 * i + 32], 'big') for i in range(16)]
        keysB = [int.from_bytes(EC.tag(b'other', i), 'big') % EC.Q for i in range(40)]
        for i in range(16):
            keysB[2 * i + 5] = keysA[i]
        idA, idB = eng.add_ring(ringA, 16), eng.add_ring(EC.be32(keysB), 40)
        A72 = eng.escrow_keygen(X.a32)
        eng.set_auditor(A72)
        eng.use_ring(idA)
        proofs, st = eng.prove_batch(msg, sig, pk, which, seeds=seeds)
        assert st == [0] * NB
        bl = eng.prove_key_blinders(seeds=seeds)
        kx, st = eng.proof_key_commitments(proofs)
        assert st == [0] * NB
        keys = [keysA[w] for w in which]
        tags, st = eng.escrow_prove_batch(EC.be32(keys), kx, bl, seeds=EC.seeds_for(b'fresh', NB))
        assert st == [0] * NB
        assert eng.verify_batch(msg, proofs) == ([1] * NB, [0] * NB)
        assert eng.escrow_verify_batch(kx, tags) == ([1] * NB, [0] * NB)
        assert eng.escrow_open_batch(X.a32, tags) == (list(which), [0] * NB)
        pp = EC.MC.oracle_params(par[1], par[2])
        for b in range(NB):
            assert EC.verify(pp, EC.keygen(pp, X.a), kx[b], tags[b]) == (1, 0)
        assert eng.escrow_verify_batch([kx[1]], [tags[0]]) == ([0], [0])   # signer 0's tag beside signer 1's attestation
        # the same tags after re-ringing into ring B: keyXcom is kept
        eng.use_ring(idB)
        new_which = [2 * w + 5 for w in which]
        moved, st = eng.rering_batch(msg, proofs, new_which, bl, seeds=EC.seeds_for(b'rering', NB))
        assert st == [0] * NB
        assert eng.verify_batch(msg, moved) == ([1] * NB, [0] * NB)
        assert eng.proof_key_commitments(moved) == (kx, [0] * NB)
        assert eng.escrow_verify_batch(kx, tags) == ([1] * NB, [0] * NB)
        assert eng.escrow_open_batch(X.a32, tags) == (new_which, [0] * NB)
    finally:
        eng.close()


# ------------------------------------------------------------------ 6. the device forms, 7. wipe, timing
def _up(b, tail=16):
    import torch
    return torch.frombuffer(bytearray(bytes(b) + bytes(tail)), dtype=torch.uint8).to(torch.device('cuda:0'))


def _dev_prove(x, eng, idx, cap=None, fill=0x5a):
    """zk_escrow_prove_batch_device on torch buffers -> (0 or the ZkError's status, out as left with 64 bytes behind out_cap, statuses as left)"""
    import torch
    EC = x.EC
    idx = list(idx)
    B = len(idx)
    d = [_up(EC.be32([x.x[b] for b in idx])), _up(b''.join(x.c[b] for b in idx)), _up(EC.be32([x.r[b] for b in idx])), _up(b''.join(x.seeds[32 * b:32 * b + 32] for b in idx))]
    d_out = torch.full((472 * B + 64,), fill, dtype=torch.uint8, device='cuda:0')
    d_st = torch.full((4 * B + 16,), fill, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    rc = 0
    try:
        eng.escrow_prove_batch_device(B, *[t.data_ptr() for t in d], d_out.data_ptr(), 472 * B if cap is None else cap, d_st.data_ptr())
    except x.Z.ZkError as e:
        rc = e.status
    torch.cuda.synchronize()
    return rc, bytes(d_out.cpu().numpy()), bytes(d_st.cpu().numpy())


def _dev_open(x, eng, secret32, tags, fill=0x5a):
    import torch
    B = len(tags)
    d_a, d_t = _up(secret32), _up(b''.join(tags), 0)
    d_idx = torch.full((4 * B + 16,), fill, dtype=torch.uint8, device='cuda:0')
    d_st = torch.full((4 * B + 16,), fill, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    rc = 0
    try:
        eng.escrow_open_batch_device(B, d_a.data_ptr(), d_t.data_ptr(), d_idx.data_ptr(), d_st.data_ptr())
    except x.Z.ZkError as e:
        rc = e.status
    torch.cuda.synchronize()
    return rc, bytes(d_idx.cpu().numpy()), bytes(d_st.cpu().numpy())


def test_device_forms_equal_the_host_forms(X):
    import numpy as np
    import torch
    B = B67
    rc, out, stw = _dev_prove(X, X.eng, range(B))
    assert rc == 0 and out[:472 * B] == b''.join(X.tags) and out[472 * B:] == b'\x5a' * 64
    assert stw[:4 * B] == bytes(4 * B) and stw[4 * B:] == b'\x5a' * 16
    # the verifier and the opening: the batch at the very end of its allocations (no read outside the slots), what lies behind B untouched
    tags = list(X.tags)
    tags[3] = tags[3][:400] + bytes([tags[3][400] ^ 1]) + tags[3][401:]
    tags[66] = b'ZKT2' + tags[66][4:]
    d_t, d_c = _up(b''.join(tags), 0), _up(b''.join(X.c), 0)
    d_ok = torch.full((B + 8,), 0x5a, dtype=torch.uint8, device='cuda:0')
    d_st = torch.full((4 * B + 16,), 0x5a, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    X.eng.escrow_verify_batch_device(B, d_c.data_ptr(), d_t.data_ptr(), d_ok.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    ok, st = bytes(d_ok.cpu().numpy()), np.frombuffer(bytes(d_st.cpu().numpy()), dtype=np.int32)
    host = X.eng.escrow_verify_batch(X.c, tags)
    assert (list(ok[:B]), list(st[:B])) == host and host[0] == [1] * 3 + [0] + [1] * 62 + [0] and host[1] == [0] * 66 + [E_BAD]
    assert ok[B:] == b'\x5a' * 8 and bytes(d_st.cpu().numpy())[4 * B:] == b'\x5a' * 16
    rc, idx, stw = _dev_open(X, X.eng, X.a32, tags)
    assert rc == 0
    host = X.eng.escrow_open_batch(X.a32, tags)
    assert (list(np.frombuffer(idx[:4 * B], dtype=np.uint32)), list(np.frombuffer(stw[:4 * B], dtype=np.int32))) == host
    assert host == (X.planted[:66] + [NONE], [0] * 66 + [E_BAD])   # (the response byte damaged in tag 3 is the verifier's business)
    assert idx[4 * B:] == b'\x5a' * 16 and stw[4 * B:] == b'\x5a' * 16


def test_wipe_and_a_failed_call_leave_no_nonzero_word(X):
    """zk_test_counter 11 counts the nonzero words of every witness-flagged buffer, the escrow arenas (keys, blinders, draws, a, a E1) among them"""
    eng, EC = _engine(X.Z, X.par), X.EC
    try:
        eng.set_auditor(X.A72)
        eng.set_ring(EC.MC.ring_bytes(X.ring), 300)
        assert eng.escrow_prove_batch(EC.be32(X.x[:8]), X.c[:8], EC.be32(X.r[:8]), seeds=X.seeds[:256])[0] == X.tags[:8]
        assert 0 < eng.test_counter(11) < 1 << 63
        eng.wipe()
        assert eng.test_counter(11) == 0
        assert eng.escrow_open_batch(X.a32, X.tags[:8])[0] == X.planted[:8]
        assert eng.test_counter(11) > 0
        eng.wipe()
        assert eng.test_counter(11) == 0
        assert eng.escrow_prove_batch(EC.be32(X.x[:8]), X.c[:8], EC.be32(X.r[:8]), seeds=X.seeds[:256])[0] == X.tags[:8]
        rc, _, _ = _dev_prove(X, eng, range(8), cap=100)   # a failed call wipes by itself
        assert rc == E_BUF and eng.test_counter(11) == 0
        assert eng.escrow_open_batch(X.a32, X.tags[:8])[0] == X.planted[:8]
        with pytest.raises(X.Z.ZkError) as e:   # ... and so does an opening with a wrong secret
            eng.escrow_open_batch(bytes(31) + b'\x05', X.tags[:8])
        assert e.value.status == E_OPENING and eng.test_counter(11) == 0
    finally:
        eng.close()


def test_timing_families(X):
    eng, EC = X.eng, X.EC
    eng.set_timing(1)
    try:
        eng.escrow_prove_batch(EC.be32(X.x[:8]), X.c[:8], EC.be32(X.r[:8]), seeds=X.seeds[:256])
        assert set(eng.last_timing()[1]) == {'rng_prepass', 'escrow_front', 'tom_commit', 'tom_normalize', 'hash', 'escrow_respond'}
        eng.escrow_verify_batch(X.c[:8], X.tags[:8])
        assert set(eng.last_timing()[1]) == {'escrow_parse', 'tom_commit', 'escrow_ladder'}
        eng.escrow_open_batch(X.a32, X.tags[:8])
        assert set(eng.last_timing()[1]) == {'escrow_open', 'escrow_ladder', 'tom_normalize', 'escrow_ring_points', 'escrow_match'}
        with pytest.raises(X.Z.ZkError):   # a wrong secret: the key check is all that ran
            eng.escrow_open_batch(bytes(31) + b'\x05', X.tags[:8])
        assert set(eng.last_timing()[1]) == {'escrow_open'}
    finally:
        eng.set_timing(0)


# ------------------------------------------------------------------ 8. kernel resources
def test_new_kernels_report_no_scratch_and_no_spills(X):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('kernel_meta', os.path.join(root, 'tools', 'kernel_meta.py'))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    ks = {n: k for n, k in km.kernels(X.Z.LIB_PATH).items() if 'k_escrow' in n}
    for want in ('k_escrow_front', 'k_escrow_opening_msg', 'k_escrow_respond', 'k_escrow_parse', 'k_escrow_relations', 'k_escrow_verdict', 'k_escrow_check_key',
                 'k_escrow_stage_secret', 'k_escrow_open_points', 'k_escrow_ring_scalars', 'k_escrow_times4', 'k_escrow_match'):
        assert any(want in n for n in ks), want
    for n, k in ks.items():
        assert k['scratch'] == 0 and k['agpr'] == 0 and k['vgpr_spill'] == 0 and k['vgpr'] <= 256 and k['waves_per_simd'] >= 2, (n, k)
