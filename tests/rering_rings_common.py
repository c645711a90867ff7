"""Shared by tests/test_gpu_rering_rings.py: the fixture's rings and proofs (the sizes of tests/test_gpu_rering.py: secLevel 20, 16-bit combs, five proofs made
on ring A of 8 keys; rings B and B2 of 8 keys, n = 3, with A's keys at permuted indices, ring C of 20 keys, n = 5 -- all resident, A active), batches built
from them, the one-ring reference (zk_proof_rering_batch ring by ring) and the _device form on torch buffers."""
import hashlib

SEC, S, NB = 20, 77, 5
E_BAD, E_RNG, E_BUF, E_ARG, E_OPENING = 10, 11, 12, 14, 16
UNKNOWN = 0x7fff0000   # an id no context hands out


def h(t, i):
    return hashlib.sha256(b'rering-rings-test' + t + i.to_bytes(4, 'big')).digest()


def ring_bytes(vals):
    return b''.join(v.to_bytes(32, 'big') for v in vals)


def gk_size(n, tc=36):
    return n * (8 * tc + 96) + 32


class Ctx:
    pass


def make_fixture():
    import coracle  # noqa: F401  (puts the oracle's directory on the path, as tests/test_gpu_rering.py relies on)
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
    keysA = [int.from_bytes(ringA[32 * i:32 * i + 32], 'big') for i in range(8)]
    other = [int.from_bytes(h(b'other', i), 'big') % MC.Q for i in range(20)]
    # B: A's keys 0..4 at 7 - a; B2: at a; C (20 keys): at 2 a + 4
    x.keys = {'B': other[:3] + [keysA[7 - i] for i in range(3, 8)], 'B2': keysA[:5] + other[3:6], 'C': list(other)}
    for a in range(8):
        x.keys['C'][2 * a + 4] = keysA[a]
    x.idx = {'B': [7 - w for w in x.which], 'B2': list(x.which), 'C': [2 * w + 4 for w in x.which]}
    x.n = {'B': 3, 'B2': 3, 'C': 5}
    eng.set_ring(ringA, 8)
    x.idA = 0
    x.id = {name: eng.add_ring(ring_bytes(x.keys[name])) for name in ('B', 'B2', 'C')}
    x.name = {v: k for k, v in x.id.items()}
    x.proofsA, st = eng.prove_batch(x.msg, sig, pk, x.which, seeds=x.seeds)
    assert st == [0] * NB
    x.blinders = eng.prove_key_blinders(seeds=x.seeds)
    x.pp = MC.oracle_params(tg, th)
    return x


def batch(x, rings, tag, proofs=None):
    """len(rings) inputs cycling the five proofs (or `proofs`, a list of five), input j bound for ring rings[j], every input with a fresh seed of its own"""
    src = proofs or x.proofsA
    k = len(rings)
    return {'msg': b''.join(x.msg[32 * (j % NB):32 * (j % NB) + 32] for j in range(k)), 'proofs': [src[j % NB] for j in range(k)],
            'which': [x.idx[rings[j]][j % NB] for j in range(k)], 'ids': [x.id[rings[j]] for j in range(k)], 'blinders': [x.blinders[j % NB] for j in range(k)],
            'seeds': b''.join(h(tag, j) for j in range(k)), 'rings': list(rings)}


def pick(bt, keep):
    """the batch of inputs `keep`, in that order"""
    return {'msg': b''.join(bt['msg'][32 * j:32 * j + 32] for j in keep), 'seeds': b''.join(bt['seeds'][32 * j:32 * j + 32] for j in keep),
            **{k: [bt[k][j] for j in keep] for k in ('proofs', 'which', 'ids', 'blinders', 'rings')}}


def one_ring(x, bt):
    """zk_proof_rering_batch ring by ring, each with its ring active, on the inputs bound for it -> (outputs, statuses) in batch order; A is active again after"""
    eng = x.eng
    out, st = [None] * len(bt['ids']), [None] * len(bt['ids'])
    try:
        for rid in sorted(set(bt['ids']) - {UNKNOWN}):
            sel = [j for j in range(len(bt['ids'])) if bt['ids'][j] == rid]
            sub = pick(bt, sel)
            eng.use_ring(rid)
            o, s = eng.rering_batch(sub['msg'], sub['proofs'], sub['which'], sub['blinders'], seeds=sub['seeds'])
            for k, j in enumerate(sel):
                out[j], st[j] = o[k], s[k]
    finally:
        eng.use_ring(x.idA)
    return out, st


def rings_call(x, bt, **kw):
    kw.setdefault('seeds', bt['seeds'])
    if 'streams' in kw:
        kw.pop('seeds')
    out, st = x.eng.rering_batch_rings(bt['msg'], bt['proofs'], bt['which'], bt['ids'], bt['blinders'], **kw)
    return out, st, list(x.eng.rering_last_off), x.eng.rering_last_raw


def oracle_splice(x, orig, blinder, which_new, keys, seed, statement=None):
    """the oracle's side: the original proof with a GKProof that proveMembership makes over its keyXcom"""
    R, MC = x.R, x.MC
    prf = R.proof_from_bytes(orig)
    com = R.Commitment(prf.keyXcom, MC.TOM.newScalar(int.from_bytes(blinder, 'big')))
    prf.membershipProof = R.proveMembership(x.pp, com, which_new, keys, R.SeedRng(seed), statement=statement(prf) if statement else b'')
    return R.proof_to_bytes(prf)


def dev(x, bt, in_place=False, cap=None, fill=0x5a, out_shift=None, engine=None, call='rings'):
    """the _device form on torch buffers -> (status or ZkError code, out bytes as left, out_off words as left, statuses as left).  out_shift: out = proofs +
    out_shift (a partial overlap).  call='one': zk_proof_rering_batch_device on the same buffers (the ids are not handed over)."""
    import numpy as np
    import torch
    device = torch.device('cuda:0')
    eng = engine or x.eng
    B = len(bt['proofs'])

    def up(b):
        return torch.frombuffer(bytearray(bytes(b) + bytes(16)), dtype=torch.uint8).to(device)
    blob = b''.join(bt['proofs'])
    off = np.cumsum([0] + [len(p) for p in bt['proofs']]).astype(np.uint64)
    d_in = up(blob + (bytes(len(blob)) if out_shift is not None else b''))
    d_msg, d_bl, d_rng = up(bt['msg']), up(b''.join(bt['blinders'])), up(bt['seeds'])
    d_off, d_w, d_ids = up(off.tobytes()), up(np.array(bt['which'], dtype=np.uint32).tobytes()), up(np.array(bt['ids'], dtype=np.uint32).tobytes())
    size = len(blob) + B * 2048
    d_out = d_in if in_place or out_shift is not None else torch.full((size,), fill, dtype=torch.uint8, device=device)
    d_ooff, d_st = torch.full((8 * (B + 1),), fill, dtype=torch.uint8, device=device), torch.full((4 * max(B, 1),), fill, dtype=torch.uint8, device=device)
    torch.cuda.synchronize()
    rc = 0
    out_cap = (len(blob) if in_place or out_shift is not None else size) if cap is None else cap
    try:
        if call == 'rings':
            eng.rering_batch_rings_device(B, d_msg.data_ptr(), d_in.data_ptr(), d_off.data_ptr(), d_w.data_ptr(), d_ids.data_ptr(), d_bl.data_ptr(), d_rng.data_ptr(),
                                          d_out.data_ptr() + (out_shift or 0), out_cap, d_ooff.data_ptr(), d_st.data_ptr())
        else:
            eng.rering_batch_device(B, d_msg.data_ptr(), d_in.data_ptr(), d_off.data_ptr(), d_w.data_ptr(), d_bl.data_ptr(), d_rng.data_ptr(), d_out.data_ptr(), out_cap,
                                    d_ooff.data_ptr(), d_st.data_ptr())
    except x.Z.ZkError as e:
        rc = e.status
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy().tobytes()
    if in_place:
        raw = raw[:len(blob)]
    return rc, raw, [int(v) for v in np.frombuffer(d_ooff.cpu().numpy().tobytes(), dtype=np.uint64)], [int(v) for v in np.frombuffer(d_st.cpu().numpy().tobytes(), dtype=np.int32)][:B]
