"""gpu: the ring fold (GK phase) at the shapes the membership suite does not reach -- that suite proves over rings of 5 and 300 keys (n = 3: the plain tile;
n = 9: table E).  Here: rings of 2 and 4 keys (n = 1, 2: one kernel per level through the ping-pong buffers; the verifier's one-thread fold), 16 keys (n = 4:
the four-level register tile) and 4096 keys (n = 12: the smallest ring whose table path runs on the matrix cores), three proofs each, through the stand-alone
membership calls and through the full prover and verifier.  Every honest proof is accepted, one with a byte of its GK section flipped is refused beside two
accepted neighbours, and where the Python oracle proves the same witness in a few seconds (n <= 4) the membership proofs are its bytes."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import member_common as M

pytestmark = pytest.mark.gpu
RINGS = (2, 4, 16, 4096)
B = 3


@pytest.fixture(scope='module')
def env():
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    nh, tg, th = eng.synth_params(M.PARAM_SEED)
    eng.set_params(nh, tg, th, 80)
    e = {'eng': eng, 'params': M.oracle_params(tg, th), 'rings': {}}
    yield e
    eng.close()


def ring_of(env, nkeys):
    """the resident ring of `nkeys` synthetic keys, made active, with three signatures under keys of it: built by the first test that asks"""
    eng = env['eng']
    if nkeys not in env['rings']:
        # the generator signs proof b with the key of ring slot b mod nkeys, a fresh key per proof: the two-key ring takes its third witness from the first
        S = min(B, nkeys)
        ring, msg, sig, pk, which, _ = eng.synth_workload(M.PARAM_SEED, nkeys, S)
        msg, sig, pk = (b''.join(a[w * (b % S):w * (b % S + 1)] for b in range(B)) for a, w in ((msg, 32), (sig, 64), (pk, 64)))
        which, seeds = [which[b % S] for b in range(B)], M.seeds_for(b'gk%d' % nkeys, B)
        eng.set_key_tables(nkeys < 4096)   # 4096 per-key tables would take the build far beyond the test; the fold does not read them
        try:
            rid = eng.add_ring(ring, nkeys)
        finally:
            eng.set_key_tables(True)
        n = max(1, (nkeys - 1).bit_length())
        values = [int.from_bytes(ring[32 * i:32 * i + 32], 'big') for i in range(nkeys)]
        env['rings'][nkeys] = {'id': rid, 'n': n, 'values': values, 'msg': msg, 'sig': sig, 'pk': pk, 'which': which, 'seeds': seeds}
    r = env['rings'][nkeys]
    eng.use_ring(r['id'])
    return r


def flipped(proof, pos):
    return proof[:pos] + bytes([proof[pos] ^ 1]) + proof[pos + 1:]


@pytest.mark.parametrize('nkeys', RINGS)
def test_membership_proofs_verify_and_a_flipped_gk_byte_is_refused(env, nkeys):
    eng, r = env['eng'], ring_of(env, nkeys)
    n = r['n']
    assert eng.member_proof_size() == M.proof_size(n)
    proofs, coms, _, st = eng.member_prove_batch(r['which'], seeds=r['seeds'])
    assert st == [0] * B
    assert eng.member_verify_batch(coms, proofs) == ([1] * B, [0] * B)
    bad = list(proofs)
    bad[1] = flipped(proofs[1], 16 + 288 * n + 31)   # the low byte of f_0
    assert eng.member_verify_batch(coms, bad)[0] == [1, 0, 1]


@pytest.mark.parametrize('nkeys', RINGS)
def test_full_proofs_verify_and_a_flipped_gk_byte_is_refused(env, nkeys):
    eng, r = env['eng'], ring_of(env, nkeys)
    n = r['n']
    proofs, st = eng.prove_batch(r['msg'], r['sig'], r['pk'], r['which'], seeds=r['seeds'])
    assert st == [0] * B
    assert eng.verify_batch(r['msg'], proofs) == ([1] * B, [0] * B)
    bad = list(proofs)
    bad[2] = flipped(proofs[2], len(proofs[2]) - 32 * (3 * n + 1) + 31)   # the GK section closes the proof: 4 n points, then f, za, zb, zd; f_0's low byte
    assert eng.verify_batch(r['msg'], bad)[0] == [1, 1, 0]


@pytest.mark.parametrize('nkeys', [k for k in RINGS if k <= 16])
def test_membership_proofs_are_the_oracles_bytes(env, nkeys):
    eng, r = env['eng'], ring_of(env, nkeys)
    proofs, coms, blinders, st = eng.member_prove_batch(r['which'], seeds=r['seeds'])
    assert st == [0] * B
    for b in range(B):
        ref = M.oracle_prove(env['params'], r['values'], r['which'][b], M.R.SeedRng(r['seeds'][32 * b:32 * b + 32]))
        assert (proofs[b], coms[b], blinders[b]) == ref, b
