"""-m gpu: zk_link_prove_batch / zk_link_verify_batch / zk_proof_key_commitments.  The expected bytes are the oracle's proveEquality(ProofGroup, x, Commitment(C1, r1),
Commitment(C2, r2), rng) in the ZKL1 layout, the expected verdicts aggregateEquality into a MultiMult, evaluate().isIdentity() (tests/link_common.py).
secLevel 20, 16-bit combs; commitments come from eng.test_tom_commit unless a test says otherwise."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

SEC = 20
E_BAD, E_RNG, E_BUF, E_ARG, E_OPENING = 10, 11, 12, 14, 16


class Ctx:
    pass


@pytest.fixture(scope='module')
def X():
    import link_common as LC
    import zkp_ecdsa_amd as Z
    x = Ctx()
    x.Z, x.LC, x.R = Z, LC, LC.R
    eng = x.eng = Z.Engine(0)
    eng.set_comb_bits(16)
    x.par = nh, tg, th = eng.synth_params(LC.PARAM_SEED)
    eng.set_params(nh, tg, th, SEC)
    x.pp = LC.MC.oracle_params(tg, th)
    # the 257-proof workload, shared: inputs, the engine's proofs, the oracle's bytes of the five named proofs
    x.B = 257
    x.x, x.r1, x.r2, x.seeds = LC.workload(b'w257', x.B)
    x.c1, x.c2 = eng.test_tom_commit(x.x, x.r1), eng.test_tom_commit(x.x, x.r2)
    x.proofs, x.st = eng.link_prove_batch(LC.be32(x.x), x.c1, LC.be32(x.r1), x.c2, LC.be32(x.r2), seeds=x.seeds)
    yield x
    eng.close()


def _oracle(x, b, rng=None, pp=None):
    return x.LC.oracle_prove(pp or x.pp, x.x[b], x.c1[b], x.r1[b], x.c2[b], x.r2[b], rng or x.R.SeedRng(x.seeds[32 * b:32 * b + 32]))


def _prove(x, eng, idx, **kw):
    LC = x.LC
    return eng.link_prove_batch(LC.be32([x.x[b] for b in idx]), [x.c1[b] for b in idx], LC.be32([x.r1[b] for b in idx]), [x.c2[b] for b in idx],
                                LC.be32([x.r2[b] for b in idx]), **kw)


# ------------------------------------------------------------------ 1. bytes
def test_67_proofs_equal_the_oracle(X):
    assert X.eng.link_proof_size() == 256
    proofs, st = _prove(X, X.eng, range(67), seeds=X.seeds[:32 * 67])   # one full wave and a tail
    assert st == [0] * 67
    for b in range(67):
        assert proofs[b] == _oracle(X, b), b
    assert proofs == X.proofs[:67]   # a proof's bytes do not depend on the batch around it


def test_257_proofs_two_blocks(X):
    assert X.st == [0] * 257
    for b in (0, 63, 64, 255, 256):
        assert X.proofs[b] == _oracle(X, b), b
        assert X.LC.oracle_verify(X.pp, X.c1[b], X.c2[b], X.proofs[b]) == (1, 0)
    assert X.eng.link_verify_batch(X.c1, X.c2, X.proofs) == ([1] * 257, [0] * 257)


def test_bytes_do_not_depend_on_the_plan_or_the_build(X):
    eng, Z = X.eng, X.Z
    eng.set_chunk(100)   # three chunks
    try:
        for lanes in (1, 2):
            eng.set_lanes(lanes)
            assert _prove(X, eng, range(257), seeds=X.seeds) == (X.proofs, [0] * 257), lanes
            assert eng.link_verify_batch(X.c1, X.c2, X.proofs) == ([1] * 257, [0] * 257)
    finally:
        eng.set_lanes(2), eng.set_chunk(4096)
    uni = os.path.join(os.path.dirname(Z.LIB_PATH), 'libzkattest_hip_uniform.so')
    assert os.path.exists(uni), 'the uniform build is not there (make -C zkp-ecdsa_amd/csrc uniform)'
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'link_uniform_check.py')], env=dict(os.environ, ZKATTEST_LIB=uni),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    rec = json.loads(out.stdout.decode().strip().splitlines()[-1])
    assert rec['lib'].endswith('_uniform.so') and rec['sha256'] == hashlib.sha256(b''.join(X.proofs)).hexdigest()


def test_hardened_mode_with_the_hardened_h(X):
    """the same 67 proofs (one full wave and a tail) under ZK_MODE_HARDENED and its h: the bytes are the oracle's for that h"""
    Z, LC = X.Z, X.LC
    nh, th = Z.hardened_h(b'link')
    eng = Z.Engine(0)
    try:
        eng.set_comb_bits(16)
        eng.set_params(nh, X.par[1], th, SEC)
        eng.set_mode(Z.MODE_HARDENED)
        pp = LC.MC.oracle_params(X.par[1], th)
        n = 67
        c1, c2 = eng.test_tom_commit(X.x[:n], X.r1[:n]), eng.test_tom_commit(X.x[:n], X.r2[:n])
        assert c1 != X.c1[:n]
        proofs, st = eng.link_prove_batch(LC.be32(X.x[:n]), c1, LC.be32(X.r1[:n]), c2, LC.be32(X.r2[:n]), seeds=X.seeds[:32 * n])
        assert st == [0] * n
        for b in range(n):
            assert proofs[b] == LC.oracle_prove(pp, X.x[b], c1[b], X.r1[b], c2[b], X.r2[b], X.R.SeedRng(X.seeds[32 * b:32 * b + 32])), b
        assert eng.link_verify_batch(c1, c2, proofs) == ([1] * n, [0] * n)
        assert X.eng.link_verify_batch(c1, c2, proofs)[0] == [0] * n   # the reference-mode h is another one
    finally:
        eng.close()


# ------------------------------------------------------------------ 2. the rejection path
def test_rejected_fills_and_a_short_stream(X):
    R = X.R
    ff = b'\xff' * 32   # >= q
    def blk(b, k):
        return hashlib.sha256(b'link-stream' + bytes([b, k])).digest()
    rows = [[ff, blk(0, 1), blk(0, 2), blk(0, 3)],        # block 0 rejected: k is block 1
            [blk(1, 0), ff, blk(1, 2), blk(1, 3)],        # block 1 rejected: s1 is block 2
            [blk(2, 0), blk(2, 1), blk(2, 2), blk(2, 3)]]
    proofs, st = _prove(X, X.eng, range(3), streams=b''.join(b''.join(r) for r in rows), stream_blocks=4)
    assert st == [0, 0, 0]
    for b in range(3):
        assert proofs[b] == _oracle(X, b, R.StreamRng(rows[b])), b
    # one block short: three blocks where a rejected fill makes four necessary; two blocks for three draws
    proofs3, st3 = _prove(X, X.eng, range(3), streams=b''.join(b''.join(r[:3]) for r in rows), stream_blocks=3)
    assert st3 == [E_RNG, E_RNG, 0] and proofs3[2] == proofs[2]
    assert X.eng.link_last_raw[:512] == bytes(512)
    proofs2, st2 = _prove(X, X.eng, range(3), streams=b''.join(b''.join(r[:2]) for r in rows), stream_blocks=2)
    assert st2 == [E_RNG] * 3 and X.eng.link_last_raw == bytes(768)


# ------------------------------------------------------------------ 3. statuses
def test_prover_statuses(X):
    eng, LC, Z = X.eng, X.LC, X.Z
    q = LC.Q
    n = 6
    keys, r1, r2 = list(X.x[:n]), list(X.r1[:n]), list(X.r2[:n])
    c1, c2 = list(X.c1[:n]), list(X.c2[:n])
    r2[1] = (r2[1] + 1) % q                                             # a wrong blinder2
    c1[2] = c1[2][:35] + bytes([c1[2][35] ^ 1]) + c1[2][36:]            # one bit of com1's x flipped
    xs = 0x1234567 + (1 << 200)                                         # a key for which key + q is still below 2^256
    assert xs + q < 1 << 256
    cs1, cs2 = eng.test_tom_commit([xs], [r1[3]])[0], eng.test_tom_commit([xs], [r2[3]])[0]
    keys[3], c1[3], c2[3] = xs + q, cs1, cs2                            # key + q
    r1[4] = (r1[4] + 1) % q                                             # a wrong blinder1
    seeds = X.seeds[:32 * n]
    proofs, st = eng.link_prove_batch(LC.be32(keys), c1, LC.be32(r1), c2, LC.be32(r2), seeds=seeds)
    assert st == [0, E_OPENING, E_BAD, 0, E_OPENING, 0]
    assert proofs[0] == X.proofs[0] and proofs[5] == X.proofs[5]
    assert proofs[3] == LC.oracle_prove(X.pp, xs, cs1, r1[3], cs2, r2[3], X.R.SeedRng(seeds[96:128]))
    raw = eng.link_last_raw
    assert raw[256:768] == bytes(512) and raw[1024:1280] == bytes(256)
    assert eng.link_prove_batch(LC.be32([xs]), [cs1], LC.be32([r1[3]]), [cs2], LC.be32([r2[3]]), seeds=seeds[96:128]) == ([proofs[3]], [0])
    # out_cap one byte short: ZK_E_BUFFER, out and statuses untouched (device form on poisoned buffers)
    rc, out, stw = _dev_prove(X, range(n), cap=256 * n - 1)
    assert rc == E_BUF and out == b'\x5a' * len(out) and stw == b'\x5a' * len(stw)
    with pytest.raises(Z.ZkError) as e:
        _prove(X, eng, range(n), seeds=X.seeds[:32 * n], cap=256 * n - 1)
    assert e.value.status == E_BUF
    assert eng.link_prove_batch(b'', [], b'', [], b'', seeds=b'') == ([], [])
    assert eng.link_verify_batch([], [], []) == ([], [])
    assert eng.proof_key_commitments([]) == ([], [])


# ------------------------------------------------------------------ 4. the verifier against the oracle
def _mutants(x, b, x1c2):
    """(name, com1, com2, proof) for honest proof b"""
    LC = x.LC
    p, c1, c2 = x.proofs[b], x.c1[b], x.c2[b]
    def sc_plus(k):
        o = 160 + 32 * k
        return p[:o] + ((int.from_bytes(p[o:o + 32], 'big') + 1) % LC.Q).to_bytes(32, 'big') + p[o + 32:]
    A1, A2 = p[16:88], p[88:160]
    return [('honest', c1, c2, p),
            ('magic', c1, c2, b'ZKM1' + p[4:]),
            ('total_len', c1, c2, p[:4] + (255).to_bytes(4, 'big') + p[8:]),
            ('reserved', c1, c2, p[:12] + b'\x00\x00\x00\x01' + p[16:]),
            ('A_1 x byte', c1, c2, p[:16 + 20] + bytes([p[16 + 20] ^ 0x40]) + p[16 + 21:]),
            ('A_1 <-> A_2', c1, c2, p[:16] + A2 + A1 + p[160:]),
            ('A_2 := A_1', c1, c2, p[:88] + A1 + p[160:]),
            ('t_x + 1', c1, c2, sc_plus(0)),
            ('t_r1 + 1', c1, c2, sc_plus(1)),
            ('t_r2 + 1', c1, c2, sc_plus(2)),
            ('com1 <-> com2', c2, c1, p),
            ('com2 := commit(x + 1, r2)', c1, x1c2, p)]


def test_verifier_against_the_oracle(X):
    LC = X.LC
    idx = list(range(8))
    x1c2 = X.eng.test_tom_commit([(X.x[b] + 1) % LC.Q for b in idx], [X.r2[b] for b in idx])
    rows = [m for b in idx for m in _mutants(X, b, x1c2[b])]
    # com1 = com2 with r1 = r2: honest
    same, st = X.eng.link_prove_batch(LC.be32(X.x[:2]), X.c1[:2], LC.be32(X.r1[:2]), X.c1[:2], LC.be32(X.r1[:2]), seeds=X.seeds[:64])
    assert st == [0, 0]
    rows += [('com1 = com2', X.c1[b], X.c1[b], same[b]) for b in range(2)]
    ok, st = X.eng.link_verify_batch([r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])
    for i, (name, c1, c2, p) in enumerate(rows):
        want = LC.oracle_verify(X.pp, c1, c2, p)
        print(i, name, 'engine', (ok[i], st[i]), 'oracle', want)
        assert (ok[i], st[i]) == want, (i, name)
        if name in ('honest', 'com1 = com2'):
            assert want == (1, 0), (i, name)
        elif want[1] == 0:
            assert ok[i] == 0, (i, name)   # every mutant that deserialises is refused
        if name == 'A_1 x byte':
            assert want == (0, E_BAD), i


# ------------------------------------------------------------------ 5. the device forms
def _up(b, tail=16):
    import torch
    return torch.frombuffer(bytearray(bytes(b) + bytes(tail)), dtype=torch.uint8).to(torch.device('cuda:0'))


def _dev_prove(x, idx, cap=None, fill=0x5a):
    """zk_link_prove_batch_device on torch buffers -> (0 or the ZkError's status, out as left with 64 bytes behind out_cap, statuses as left)"""
    import torch
    LC = x.LC
    idx = list(idx)
    B = len(idx)
    d = [_up(LC.be32([x.x[b] for b in idx])), _up(b''.join(x.c1[b] for b in idx)), _up(LC.be32([x.r1[b] for b in idx])), _up(b''.join(x.c2[b] for b in idx)),
         _up(LC.be32([x.r2[b] for b in idx])), _up(b''.join(x.seeds[32 * b:32 * b + 32] for b in idx))]
    d_out = torch.full((256 * B + 64,), fill, dtype=torch.uint8, device='cuda:0')
    d_st = torch.full((4 * B + 16,), fill, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    rc = 0
    try:
        x.eng.link_prove_batch_device(B, *[t.data_ptr() for t in d], d_out.data_ptr(), 256 * B if cap is None else cap, d_st.data_ptr())
    except x.Z.ZkError as e:
        rc = e.status
    torch.cuda.synchronize()
    return rc, bytes(d_out.cpu().numpy()), bytes(d_st.cpu().numpy())


def test_device_forms_on_torch_buffers(X):
    import numpy as np
    import torch
    B = 70
    rc, out, stw = _dev_prove(X, range(B))
    assert rc == 0 and out[:256 * B] == b''.join(X.proofs[:B]) and out[256 * B:] == b'\x5a' * 64
    assert stw[:4 * B] == bytes(4 * B) and stw[4 * B:] == b'\x5a' * 16
    # the verifier: the batch at the very end of its allocations (no read outside the slots), ok[B] and the statuses behind B untouched
    proofs = list(X.proofs[:B])
    proofs[3] = proofs[3][:200] + bytes([proofs[3][200] ^ 1]) + proofs[3][201:]
    proofs[69] = b'ZKL2' + proofs[69][4:]
    d_p, d_c1, d_c2 = _up(b''.join(proofs), 0), _up(b''.join(X.c1[:B]), 0), _up(b''.join(X.c2[:B]), 0)
    d_ok = torch.full((B + 8,), 0x5a, dtype=torch.uint8, device='cuda:0')
    d_st = torch.full((4 * B + 16,), 0x5a, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    X.eng.link_verify_batch_device(B, d_c1.data_ptr(), d_c2.data_ptr(), d_p.data_ptr(), d_ok.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    ok, st = bytes(d_ok.cpu().numpy()), np.frombuffer(bytes(d_st.cpu().numpy()), dtype=np.int32)
    host = X.eng.link_verify_batch(X.c1[:B], X.c2[:B], proofs)
    assert (list(ok[:B]), list(st[:B])) == host and host[0] == [1] * 3 + [0] + [1] * 65 + [0] and host[1] == [0] * 69 + [E_BAD]
    assert ok[B:] == b'\x5a' * 8 and bytes(d_st.cpu().numpy())[4 * B:] == b'\x5a' * 16


# ------------------------------------------------------------------ 6. end to end, 7. zk_proof_key_commitments
@pytest.fixture(scope='module')
def E2E(X):
    """ring A: 8 keys; ring B: 20 keys holding A's keys at 2 a + 4 (the construction of test_gpu_rering.py)"""
    Z, R, LC = X.Z, X.R, X.LC
    e = Ctx()
    NB, S = 4, 77
    eng = e.eng = Z.Engine(0)
    eng.set_comb_bits(16)
    nh, tg, th = eng.synth_params(S)
    eng.set_params(nh, tg, th, SEC)
    e.pp = LC.MC.oracle_params(tg, th)
    ringA, e.msg, sig, pk, e.which, seeds = eng.synth_workload(S, 8, NB)
    keysA = [int.from_bytes(ringA[32 * i:32 * i + 32], 'big') for i in range(8)]
    keysB = [int.from_bytes(LC.tag(b'other', i), 'big') % LC.Q for i in range(20)]
    for a in range(8):
        keysB[2 * a + 4] = keysA[a]
    e.idA = eng.add_ring(ringA, 8)
    e.idB = eng.add_ring(LC.be32(keysB), 20)
    eng.use_ring(e.idA)
    e.proofs, st = eng.prove_batch(e.msg, sig, pk, e.which, seeds=seeds)
    assert st == [0] * NB
    e.blA = eng.prove_key_blinders(seeds=seeds)
    eng.use_ring(e.idB)
    e.mproofs, e.coms, e.blB, st = eng.member_prove_batch([2 * w + 4 for w in e.which], seeds=LC.seeds_for(b'member', NB))
    assert st == [0] * NB
    e.kx = [R._tp(R.proof_from_bytes(p).keyXcom) for p in e.proofs]
    e.keys = [keysA[w] for w in e.which]
    e.links, st = eng.link_prove_batch(LC.be32(e.keys), e.kx, e.blA, e.coms, e.blB, seeds=LC.seeds_for(b'fresh', NB))
    assert st == [0] * NB
    e.NB = NB
    yield e
    eng.close()


def test_end_to_end_attestation_member_link(X, E2E):
    e, eng, Z = E2E, E2E.eng, X.Z
    NB = e.NB
    eng.use_ring(e.idA)
    assert eng.verify_batch(e.msg, e.proofs) == ([1] * NB, [0] * NB)
    assert eng.proof_key_commitments(e.proofs) == (e.kx, [0] * NB)
    eng.set_wire(1)
    try:
        assert eng.proof_key_commitments([Z.pack_proof(p) for p in e.proofs]) == (e.kx, [0] * NB)
    finally:
        eng.set_wire(0)
    eng.use_ring(e.idB)
    assert eng.member_verify_batch(e.coms, e.mproofs) == ([1] * NB, [0] * NB)
    assert eng.link_verify_batch(e.kx, e.coms, e.links) == ([1] * NB, [0] * NB)
    for b in range(NB):
        assert X.LC.oracle_verify(e.pp, e.kx[b], e.coms[b], e.links[b]) == (1, 0)
    # the link made for signer 0, presented with signer 1's attestation
    assert eng.link_verify_batch([e.kx[1]], [e.coms[0]], [e.links[0]]) == ([0], [0])
    assert eng.link_verify_batch([e.kx[0]], [e.coms[1]], [e.links[0]]) == ([0], [0])


def test_key_commitments_statuses_and_device_form(X, E2E):
    import numpy as np
    import torch
    e, eng, Z = E2E, E2E.eng, X.Z
    p = e.proofs
    packed = Z.pack_proof(p[2])
    batch = [p[0], p[1][:-4], b'ZKA2' + p[2][4:], packed, p[3]]   # a truncated slot, a wrong magic, the other layout's magic
    want = ([e.kx[0], bytes(72), bytes(72), bytes(72), e.kx[3]], [0, E_BAD, E_BAD, E_BAD, 0])
    assert eng.proof_key_commitments(batch) == want
    eng.set_wire(1)
    try:
        assert eng.proof_key_commitments([packed, p[0]]) == ([e.kx[2], bytes(72)], [0, E_BAD])
    finally:
        eng.set_wire(0)
    # the device form, the batch at the end of its allocation
    off, o = [], 0
    for b in batch:
        off.append(o)
        o += len(b)
    off.append(o)
    d_p, d_off = _up(b''.join(batch), 0), _up(np.array(off, dtype=np.uint64).tobytes(), 0)
    d_com = torch.full((72 * 5 + 8,), 0x5a, dtype=torch.uint8, device='cuda:0')
    d_st = torch.full((4 * 5 + 8,), 0x5a, dtype=torch.uint8, device='cuda:0')
    torch.cuda.synchronize()
    eng.proof_key_commitments_device(5, d_p.data_ptr(), d_off.data_ptr(), d_com.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    com, st = bytes(d_com.cpu().numpy()), bytes(d_st.cpu().numpy())
    assert [com[72 * b:72 * b + 72] for b in range(5)] == want[0] and com[360:] == b'\x5a' * 8
    assert list(np.frombuffer(st[:20], dtype=np.int32)) == want[1] and st[20:] == b'\x5a' * 8


def test_call_level_rules(X):
    Z = X.Z
    eng = Z.Engine(0)
    try:
        with pytest.raises(Z.ZkError) as e:   # before zk_ctx_set_params
            _prove(X, eng, range(2), seeds=X.seeds[:64])
        assert e.value.status == E_BUF
        with pytest.raises(Z.ZkError) as e:
            eng.link_verify_batch(X.c1[:1], X.c2[:1], X.proofs[:1])
        assert e.value.status == E_BUF
        with pytest.raises(Z.ZkError) as e:
            eng.proof_key_commitments([bytes(64)])
        assert e.value.status == E_BUF
    finally:
        eng.close()
    # timing families of both calls
    X.eng.set_timing(1)
    try:
        _prove(X, X.eng, range(8), seeds=X.seeds[:256])
        assert set(X.eng.last_timing()[1]) == {'rng_prepass', 'tom_commit', 'tom_normalize', 'hash', 'link_respond'}
        X.eng.link_verify_batch(X.c1[:8], X.c2[:8], X.proofs[:8])
        assert set(X.eng.last_timing()[1]) == {'link_parse', 'tom_commit', 'link_ladder'}
    finally:
        X.eng.set_timing(0)
