"""-m gpu: zk_proof_rering_batch / zk_prove_key_blinders.  A ZKA1 proof made on ring A is moved to rings that hold the signers' keys at other indices; the
expected bytes are composed from the oracle: the original proof parsed (proof_from_bytes), proveMembership(ProofGroup, Commitment(keyXcom, blinder), which_new,
new_keys, rng, statement=...) for the section, proof_to_bytes for the splice, the C restatement's verifier for the verdict.  secLevel 20, rings of 8 keys
(n = 3) and 20 keys (n = 5), 16-bit combs."""
import hashlib

import pytest

pytestmark = pytest.mark.gpu

SEC, S, NB = 20, 77, 5
E_BAD, E_RNG, E_BUF, E_ARG, E_OPENING = 10, 11, 12, 14, 16


def _h(t, i):
    return hashlib.sha256(b'rering-test' + t + i.to_bytes(4, 'big')).digest()


def _ring_bytes(vals):
    return b''.join(v.to_bytes(32, 'big') for v in vals)


def _gk_size(n, tc=36):
    return n * (8 * tc + 96) + 32


class Ctx:
    pass


@pytest.fixture(scope='module')
def X():
    import coracle as CO
    import member_common as MC
    import zkattest_ref as R
    import zkp_ecdsa_amd as Z
    x = Ctx()
    x.Z, x.R, x.MC = Z, R, MC
    eng = x.eng = Z.Engine(0)
    eng.set_comb_bits(16)
    x.par = nh, tg, th = eng.synth_params(S)
    eng.set_params(nh, tg, th, SEC)
    ringA, x.msg, sig, pk, x.which, x.seeds = eng.synth_workload(S, 8, NB)   # signer b's key is ring A's entry b
    x.keysA = [int.from_bytes(ringA[32 * i:32 * i + 32], 'big') for i in range(8)]
    # ring B: 8 keys, A's keys 0..4 at 7 - a, three others in front; ring C: 20 keys, all of A's keys at 2 a + 4, others elsewhere
    other = [int.from_bytes(_h(b'other', i), 'big') % MC.Q for i in range(20)]
    x.keysB = other[:3] + [x.keysA[7 - i] for i in range(3, 8)]
    x.keysC = list(other)
    for a in range(8):
        x.keysC[2 * a + 4] = x.keysA[a]
    x.idxB = [7 - w for w in x.which]
    x.idxC = [2 * w + 4 for w in x.which]
    eng.set_ring(ringA, 8)
    x.idA = 0
    x.idB, x.idC = eng.add_ring(_ring_bytes(x.keysB)), eng.add_ring(_ring_bytes(x.keysC))
    x.proofsA, st = eng.prove_batch(x.msg, sig, pk, x.which, seeds=x.seeds)
    assert st == [0] * NB
    x.blinders = eng.prove_key_blinders(seeds=x.seeds)
    x.fresh = b''.join(_h(b'fresh', b) for b in range(NB))
    x.pp = MC.oracle_params(tg, th)
    x.octx = {}
    for name, keys in (('B', x.keysB), ('C', x.keysC)):
        o = CO.OracleCtx(nh, tg, th, SEC)
        o.set_ring(_ring_bytes(keys), len(keys))
        x.octx[name] = o
    # case 1's result, shared: proofs 0..4 moved from A to B
    eng.use_ring(x.idB)
    x.outB, x.stB = eng.rering_batch(x.msg[:32 * NB], x.proofsA[:NB], x.idxB[:NB], x.blinders[:NB], seeds=x.fresh[:32 * NB])
    x.offB = list(eng.rering_last_off)
    yield x
    eng.close()


def _oracle_splice(x, orig, blinder, which_new, keys, seed, statement=None):
    """the oracle's side: the original proof with a GKProof that proveMembership makes over its keyXcom"""
    R, MC = x.R, x.MC
    prf = R.proof_from_bytes(orig)
    com = R.Commitment(prf.keyXcom, MC.TOM.newScalar(int.from_bytes(blinder, 'big')))
    stmt = statement(prf) if statement else b''
    prf.membershipProof = R.proveMembership(x.pp, com, which_new, keys, R.SeedRng(seed), statement=stmt)
    return R.proof_to_bytes(prf)


def _dev(x, msg, proofs, which, blinders, rng_bytes, in_place=False, cap=None, mode=0, stride=0, fill=0x5a):
    """the _device form on torch buffers -> (status or ZkError code, out bytes as left, out_off words as left, statuses as left)"""
    import numpy as np
    import torch
    dev = torch.device('cuda:0')
    B = len(proofs)

    def up(b):
        return torch.frombuffer(bytearray(bytes(b) + bytes(16)), dtype=torch.uint8).to(dev)
    blob = b''.join(proofs)
    off, o = [], 0
    for p in proofs:
        off.append(o)
        o += len(p)
    off.append(o)
    d_in, d_msg, d_bl, d_rng = up(blob), up(msg), up(b''.join(blinders)), up(rng_bytes)
    d_off, d_w = up(np.array(off, dtype=np.uint64).tobytes()), up(np.array(which, dtype=np.uint32).tobytes())
    size = len(blob) + B * 2048
    d_out = d_in if in_place else torch.full((size,), fill, dtype=torch.uint8, device=dev)
    d_ooff, d_st = torch.full((8 * (B + 1),), fill, dtype=torch.uint8, device=dev), torch.full((4 * B,), fill, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc = 0
    try:
        x.eng.rering_batch_device(B, d_msg.data_ptr(), d_in.data_ptr(), d_off.data_ptr(), d_w.data_ptr(), d_bl.data_ptr(), d_rng.data_ptr(), d_out.data_ptr(),
                                  (len(blob) if in_place else size) if cap is None else cap, d_ooff.data_ptr(), d_st.data_ptr(), mode=mode, stride_blocks=stride)
    except x.Z.ZkError as e:
        rc = e.status
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy().tobytes()
    return rc, raw[:len(blob)] if in_place else raw, list(np.frombuffer(d_ooff.cpu().numpy().tobytes(), dtype=np.uint64)), list(np.frombuffer(d_st.cpu().numpy().tobytes(), dtype=np.int32))


def test_parity_with_member_prover_and_oracle(X):
    x, eng = X, X.eng
    assert x.stB == [0] * NB
    n, gk = 3, _gk_size(3)
    eng.use_ring(x.idB)
    mp, coms, _, mst = eng.member_prove_batch(x.idxB[:NB], blinders=b''.join(x.blinders[:NB]), seeds=x.fresh[:32 * NB])
    assert mst == [0] * NB
    for b in range(NB):
        old, new = x.proofsA[b], x.outB[b]
        assert len(new) == len(old) and new[:4] == b'ZKA1'
        assert int.from_bytes(new[4:8], 'big') == len(new) and int.from_bytes(new[12:16], 'big') == n
        assert new[:4] + new[8:12] + new[16:-gk] == old[:4] + old[8:12] + old[16:-gk]          # the head, byte for byte
        assert new[-gk:] == mp[b][16:]                                                         # the section: the member prover's, in full
        assert coms[b] == old[160:232]
        assert new == _oracle_splice(x, old, x.blinders[b], x.idxB[b], x.keysB, x.fresh[32 * b:32 * b + 32])
    assert x.offB == [sum(len(p) for p in x.outB[:b]) for b in range(NB + 1)]
    vs = b''.join(_h(b'vs', b) for b in range(NB))
    assert eng.verify_batch(x.msg[:32 * NB], x.outB, vseeds=vs) == ([1] * NB, [0] * NB)
    assert eng.verify_batch(x.msg[:32 * NB], x.proofsA[:NB], vseeds=vs) == ([0] * NB, [0] * NB)   # the originals are not proofs for B
    assert x.octx['B'].verify_batch(x.msg[:32 * NB], x.outB, nthreads=5) == ([1] * NB, [0] * NB)


def test_size_change_and_buffer(X):
    x, eng = X, X.eng
    msg = x.msg[:32 * NB]
    eng.use_ring(x.idC)
    up, st = eng.rering_batch(msg, x.proofsA[:NB], x.idxC[:NB], x.blinders[:NB], seeds=x.fresh[:32 * NB])   # 3 -> 5
    assert st == [0] * NB
    grow = _gk_size(5) - _gk_size(3)
    assert [len(p) for p in up] == [len(p) + grow for p in x.proofsA[:NB]]
    assert list(eng.rering_last_off) == [sum(len(p) for p in up[:b]) for b in range(NB + 1)]
    for b in range(NB):
        assert int.from_bytes(up[b][4:8], 'big') == len(up[b]) and int.from_bytes(up[b][12:16], 'big') == 5
        assert up[b][16:-_gk_size(5)] == x.proofsA[b][16:-_gk_size(3)]
    assert up[1] == _oracle_splice(x, x.proofsA[1], x.blinders[1], x.idxC[1], x.keysC, x.fresh[32:64])
    assert eng.verify_batch(msg, up) == ([1] * NB, [0] * NB)
    assert x.octx['C'].verify_batch(msg, up, nthreads=5) == ([1] * NB, [0] * NB)
    eng.use_ring(x.idB)
    down, st = eng.rering_batch(msg, up, x.idxB[:NB], x.blinders[:NB], seeds=x.fresh[:32 * NB])             # 5 -> 3: case 1's bytes again
    assert st == [0] * NB and down == x.outB
    assert list(eng.rering_last_off) == x.offB
    # one byte short: ZK_E_BUFFER and nothing written
    eng.use_ring(x.idC)
    need = sum(len(p) for p in up)
    rc, raw, ooff, dst = _dev(x, msg, x.proofsA[:NB], x.idxC[:NB], x.blinders[:NB], x.fresh[:32 * NB], cap=need - 1)
    assert rc == E_BUF
    assert raw == b'\x5a' * len(raw) and all(v == 0x5a5a5a5a5a5a5a5a for v in ooff) and all(v == 0x5a5a5a5a for v in dst)
    rc, raw, ooff, dst = _dev(x, msg, x.proofsA[:NB], x.idxC[:NB], x.blinders[:NB], x.fresh[:32 * NB], cap=need)
    assert rc == 0 and raw[:need] == b''.join(up) and raw[need:] == b'\x5a' * (len(raw) - need) and dst == [0] * NB
    eng.use_ring(x.idB)


def test_after_update_ring_in_place(X):
    x, eng = X, X.eng
    msg = x.msg[:32 * NB]
    eng.use_ring(x.idB)
    newkey = int.from_bytes(_h(b'rotated', 0), 'big') % x.MC.Q
    eng.update_ring(x.idB, {0: newkey.to_bytes(32, 'big')})   # entry 0 is nobody's key in this batch; n stays 3
    keys2 = [newkey] + x.keysB[1:]
    try:
        assert eng.verify_batch(msg, x.outB) == ([0] * NB, [0] * NB)   # (the fold's polynomial is over the whole ring)
        fresh2 = b''.join(_h(b'fresh2', b) for b in range(NB))
        oop, st = eng.rering_batch(msg, x.outB, x.idxB[:NB], x.blinders[:NB], seeds=fresh2)
        assert st == [0] * NB and eng.verify_batch(msg, oop) == ([1] * NB, [0] * NB)
        assert oop[2] == _oracle_splice(x, x.outB[2], x.blinders[2], x.idxB[2], keys2, fresh2[64:96])
        rc, raw, ooff, dst = _dev(x, msg, x.outB, x.idxB[:NB], x.blinders[:NB], fresh2, in_place=True)
        assert rc == 0 and dst == [0] * NB and raw == b''.join(oop) and ooff == x.offB
        inp, st = eng.rering_batch(msg, x.outB, x.idxB[:NB], x.blinders[:NB], seeds=fresh2, in_place=True)   # the Engine's own in-place path
        assert st == [0] * NB and inp == oop
        # in place with a failed proof: it keeps its bytes, the others are re-ringed
        bad = list(x.blinders[:NB])
        bad[3] = bytes(31) + b'\x01'
        rc, raw, ooff, dst = _dev(x, msg, x.outB, x.idxB[:NB], bad, fresh2, in_place=True)
        want = list(oop)
        want[3] = x.outB[3]
        assert rc == 0 and dst == [0, 0, 0, E_OPENING, 0] and raw == b''.join(want) and ooff == x.offB
        # one proof of another n: ZK_E_ARG, the buffer as it was
        eng.use_ring(x.idC)
        c2, st = eng.rering_batch(msg[64:96], [x.proofsA[2]], [x.idxC[2]], [x.blinders[2]], seeds=x.fresh[64:96])
        eng.use_ring(x.idB)
        mixed = x.outB[:2] + c2 + x.outB[3:]
        rc, raw, ooff, dst = _dev(x, msg, mixed, x.idxB[:NB], x.blinders[:NB], fresh2, in_place=True)
        assert rc == E_ARG and raw == b''.join(mixed) and all(v == 0x5a5a5a5a for v in dst)
    finally:
        eng.update_ring(x.idB, {0: x.keysB[0].to_bytes(32, 'big')})
    assert eng.verify_batch(msg, x.outB) == ([1] * NB, [0] * NB)


def _patch(p, at, word):
    return p[:at] + word.to_bytes(4, 'big') + p[at + 4:]


def test_statuses_between_good_neighbours(X):
    x, eng = X, X.eng
    msg, fresh = x.msg[:32 * NB], x.fresh[:32 * NB]
    eng.use_ring(x.idB)

    def run(proofs=None, which=None, blinders=None, expect=None, **kw):
        out, st = eng.rering_batch(msg, proofs or x.proofsA[:NB], which or x.idxB[:NB], blinders or x.blinders[:NB], **(kw or {'seeds': fresh}))
        assert st == expect
        off = list(eng.rering_last_off)
        for b in range(NB):
            if expect[b] == 0:
                assert out[b] == x.outB[b]
            else:
                assert out[b] is None and off[b] == off[b + 1]
        assert off == [sum(len(x.outB[i]) for i in range(b) if expect[i] == 0) for b in range(NB + 1)]
    # the opening: a wrong blinder; an index whose entry is another key (another signer's, and one that is nobody's)
    bl = list(x.blinders[:NB])
    bl[1] = (int.from_bytes(bl[1], 'big') ^ 1).to_bytes(32, 'big')
    w = list(x.idxB[:NB])
    w[3] = x.idxB[2]
    run(which=w, blinders=bl, expect=[0, E_OPENING, 0, E_OPENING, 0])
    w = list(x.idxB[:NB])
    w[1], w[3] = 8, 0
    run(which=w, expect=[0, E_ARG, 0, E_OPENING, 0])
    # the header
    p = list(x.proofsA[:NB])
    ln = len(p[3])
    p[1] = b'ZKA2' + p[1][4:]
    p[3] = _patch(p[3], 4, ln + 4)
    run(proofs=p, expect=[0, E_BAD, 0, E_BAD, 0])
    p = list(x.proofsA[:NB])
    p[1] = _patch(p[1], 4, len(p[1]) - 4)
    p[3] = _patch(p[3], 12, 64)
    run(proofs=p, expect=[0, E_BAD, 0, E_BAD, 0])
    p = list(x.proofsA[:NB])
    p[2] = x.Z.pack_proof(p[2])   # the other layout's magic
    run(proofs=p, expect=[0, 0, E_BAD, 0, 0])
    # a slot with 2 padding bytes behind the proof, whose header agrees with it: no proof's length is odd mod 4.  (It is the last one: a slot behind it would
    # start unaligned and be refused for that.)
    p = list(x.proofsA[:NB])
    p[4] = _patch(p[4], 4, len(p[4]) + 2) + bytes(2)
    run(proofs=p, expect=[0, 0, 0, 0, E_BAD])
    p[1] = _patch(p[1], 4, len(p[1]) + 2) + bytes(2)   # ... as here: everything behind proof 1 is misaligned
    run(proofs=p, expect=[0, E_BAD, E_BAD, E_BAD, E_BAD])
    # ZK_RNG_STREAM: every proof gets exactly its 15 draws; proof 1's first block is a rejected fill, so it would need a 16th
    blocks = 15
    streams = bytearray()
    for b in range(NB):
        streams += b''.join(hashlib.sha256(fresh[32 * b:32 * b + 32] + k.to_bytes(8, 'big')).digest() for k in range(blocks))
    run(streams=bytes(streams), stream_blocks=blocks, expect=[0] * NB)
    streams[32 * blocks:32 * blocks + 32] = b'\xff' * 32
    run(streams=bytes(streams), stream_blocks=blocks, expect=[0, E_RNG, 0, 0, 0])


def test_buffer_rule_and_overlap(X):
    """out_cap is decided from the headers: it must hold every proof that passes the header and index checks, also one that then fails its opening (the
    header says so); a proof that fails those two checks needs no room.  out may equal proofs, it may not overlap it otherwise."""
    import numpy as np
    import torch
    x, eng = X, X.eng
    msg, fresh = x.msg[:32 * NB], x.fresh[:32 * NB]
    eng.use_ring(x.idB)
    bl = list(x.blinders[:NB])
    bl[1] = bytes(32)
    real = sum(len(x.outB[b]) for b in range(NB) if b != 1)
    rc, raw, ooff, dst = _dev(x, msg, x.proofsA[:NB], x.idxB[:NB], bl, fresh, cap=real)
    assert rc == E_BUF and raw == b'\x5a' * len(raw)
    rc, raw, ooff, dst = _dev(x, msg, x.proofsA[:NB], x.idxB[:NB], bl, fresh, cap=real + len(x.outB[1]))
    assert rc == 0 and dst == [0, E_OPENING, 0, 0, 0] and raw[:real] == b''.join(x.outB[b] for b in range(NB) if b != 1) and raw[real:] == b'\x5a' * (len(raw) - real)
    w = list(x.idxB[:NB])
    w[1] = 8   # fails the index check: counted out
    rc, raw, ooff, dst = _dev(x, msg, x.proofsA[:NB], w, x.blinders[:NB], fresh, cap=real)
    assert rc == 0 and dst == [0, E_ARG, 0, 0, 0] and raw[:real] == b''.join(x.outB[b] for b in range(NB) if b != 1)
    # out inside proofs, 64 bytes on: refused, nothing written
    dev = torch.device('cuda:0')
    blob = b''.join(x.proofsA[:NB])
    off = np.cumsum([0] + [len(p) for p in x.proofsA[:NB]]).astype(np.uint64)

    def up(b):
        return torch.frombuffer(bytearray(bytes(b) + bytes(16)), dtype=torch.uint8).to(dev)
    d_buf = up(blob + bytes(len(blob)))
    d_msg, d_bl, d_rng, d_off, d_w = up(msg), up(b''.join(x.blinders[:NB])), up(fresh), up(off.tobytes()), up(np.array(x.idxB[:NB], dtype=np.uint32).tobytes())
    d_ooff, d_st = torch.zeros(8 * (NB + 1), dtype=torch.uint8, device=dev), torch.full((4 * NB,), 0x5a, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(x.Z.ZkError) as ei:
        eng.rering_batch_device(NB, d_msg.data_ptr(), d_buf.data_ptr(), d_off.data_ptr(), d_w.data_ptr(), d_bl.data_ptr(), d_rng.data_ptr(), d_buf.data_ptr() + 64, len(blob),
                                d_ooff.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    assert ei.value.status == E_ARG and d_buf.cpu().numpy().tobytes()[:len(blob)] == blob and set(d_st.cpu().numpy().tobytes()) == {0x5a}


def test_hardened_mode(X):
    x, eng, R = X, X.eng, X.R
    msg, fresh = x.msg[:32 * NB], x.fresh[:32 * NB]
    eng.use_ring(x.idB)
    eng.set_mode(x.Z.MODE_HARDENED)
    try:
        hard, st = eng.rering_batch(msg, x.proofsA[:NB], x.idxB[:NB], x.blinders[:NB], seeds=fresh)
        assert st == [0] * NB
        padded = [v.k for v in R.pad(x.keysB, x.MC.TOM)]
        for b in (0, 4):
            want = _oracle_splice(x, x.proofsA[b], x.blinders[b], x.idxB[b], x.keysB, fresh[32 * b:32 * b + 32],
                                  statement=lambda prf: R.gk_statement(padded, msg[32 * b:32 * b + 32], prf.R, prf.keyXcom))
            assert hard[b] == want
            pts = len(hard[b]) - _gk_size(3) + 4 * 72 * 3
            assert hard[b][:pts] == x.outB[b][:pts] and hard[b][-32:] != x.outB[b][-32:]   # same randomness: same commitments, another challenge
        assert eng.verify_batch(msg, hard) == ([1] * NB, [0] * NB)
        assert eng.verify_batch(bytes(32) + msg[32:], hard)[0] == [0, 1, 1, 1, 1]   # the message is part of the statement
    finally:
        eng.set_mode(x.Z.MODE_REFERENCE)
    assert eng.verify_batch(msg, hard) == ([0] * NB, [0] * NB)


def test_packed_wire(X):
    x, eng = X, X.eng
    msg, fresh = x.msg[:32 * NB], x.fresh[:32 * NB]
    eng.use_ring(x.idB)
    eng.set_wire(True)
    try:
        packed = [x.Z.pack_proof(p) for p in x.proofsA[:NB]]
        out, st = eng.rering_batch(msg, packed, x.idxB[:NB], x.blinders[:NB], seeds=fresh)
        assert st == [0] * NB and out == [x.Z.pack_proof(p) for p in x.outB]
        assert eng.verify_batch(msg, out) == ([1] * NB, [0] * NB)
        _, st = eng.rering_batch(msg, x.proofsA[:NB], x.idxB[:NB], x.blinders[:NB], seeds=fresh)   # ZKA1 input on a ZKA1P context
        assert st == [E_BAD] * NB
        eng.use_ring(x.idC)
        out, st = eng.rering_batch(msg, packed, x.idxC[:NB], x.blinders[:NB], seeds=fresh)           # 3 -> 5 in the packed layout
        assert st == [0] * NB and [len(p) for p in out] == [len(p) + _gk_size(5, 33) - _gk_size(3, 33) for p in packed]
        assert eng.verify_batch(msg, out) == ([1] * NB, [0] * NB)
    finally:
        eng.set_wire(False)
        eng.use_ring(x.idB)


def test_chunks_and_lanes(X):
    x, eng = X, X.eng
    B = 70   # the five proofs fourteen times over, every copy with a seed of its own
    msg = b''.join(x.msg[32 * (b % NB):32 * (b % NB) + 32] for b in range(B))
    proofs, idx, bl = [x.proofsA[b % NB] for b in range(B)], [x.idxC[b % NB] for b in range(B)], [x.blinders[b % NB] for b in range(B)]
    fresh = b''.join(_h(b'fresh70', b) for b in range(B))
    bl[33] = bytes(32)   # one failed proof in the middle: the proofs behind it close up, across chunk borders
    eng.use_ring(x.idC)
    try:
        one, st1 = eng.rering_batch(msg, proofs, idx, bl, seeds=fresh)
        off1 = list(eng.rering_last_off)
        assert st1 == [0] * 33 + [E_OPENING] + [0] * 36
        eng.set_chunk(20)   # 20 + 20 + 20 + 10
        for lanes in (1, 2):
            eng.set_lanes(lanes)
            got, st = eng.rering_batch(msg, proofs, idx, bl, seeds=fresh)
            assert st == st1 and got == one and list(eng.rering_last_off) == off1
        good = [p for p in one if p is not None]
        gm = b''.join(msg[32 * b:32 * b + 32] for b in range(B) if b != 33)
        assert eng.verify_batch(gm, good) == ([1] * 69, [0] * 69)
    finally:
        eng.set_chunk(4096)
        eng.set_lanes(2)
        eng.use_ring(x.idB)


def test_key_blinders(X):
    import torch
    x, eng = X, X.eng
    eng.use_ring(x.idA)
    try:
        coms = eng.test_tom_commit([x.keysA[x.which[b]] for b in range(NB)], [int.from_bytes(x.blinders[b], 'big') for b in range(NB)])
    finally:
        eng.use_ring(x.idB)
    assert coms == [x.proofsA[b][160:232] for b in range(NB)]
    assert x.blinders == [d[0] for d in eng.test_rng_draws(NB, 1, 1, seeds=x.seeds)]
    dev = torch.device('cuda:0')
    d_seeds = torch.frombuffer(bytearray(x.seeds), dtype=torch.uint8).to(dev)
    d_out = torch.zeros(32 * NB, dtype=torch.uint8, device=dev)
    eng.prove_key_blinders_device(NB, d_seeds.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == b''.join(x.blinders)
    # stream mode: the same fills as a stream give the same blinders
    streams = b''.join(hashlib.sha256(x.seeds[32 * b:32 * b + 32] + k.to_bytes(8, 'big')).digest() for b in range(4) for k in range(4))
    assert eng.prove_key_blinders(streams=streams, stream_blocks=4) == x.blinders[:4]
    # a stream that does not hold draw 1 -- one block, or two of which the first is a rejected fill -- is reported, not answered with zeros
    for short, blocks in ((streams[:32] + streams[128:160], 1), (b'\xff' * 32 + streams[32:64] + streams[128:192], 2)):
        with pytest.raises(x.Z.ZkError) as ei:
            eng.prove_key_blinders(streams=short, stream_blocks=blocks)
        assert ei.value.status == E_RNG


def test_wipe(X):
    x, eng = X, X.eng
    eng.use_ring(x.idB)
    out, st = eng.rering_batch(x.msg[:32 * NB], x.proofsA[:NB], x.idxB[:NB], x.blinders[:NB], seeds=x.fresh[:32 * NB])
    assert st == [0] * NB and eng.test_counter(11) > 0
    eng.wipe()
    assert eng.test_counter(11) == 0
