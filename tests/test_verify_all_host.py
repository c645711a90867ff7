"""CPU tier of the exhaustive verify mode (include/zkattest.h: zk_ctx_set_verify_reps): the model the GPU tier compares the engine with
(tests/verify_all_common.py) accepts honest proofs and rejects one broken repetition wherever it sits, the pass rule covers every repetition, the
committed (repetition, verifier seed) pairs of the GPU tier's first test are what they claim to be, and the ABI is declared, exported and bound."""
import ctypes as C
import os
import re

import pytest

import coracle as CO
import zkattest_ref as R
import verify_all_common as VA
from zka1_mutants import P256_N, Layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZK_E_ARG = 14


def _xy(pt, w):
    x, y = pt.toAffine()
    return x.to_bytes(w, 'big') + y.to_bytes(w, 'big')


@pytest.mark.parametrize('sec', [21, 41])
def test_model_accepts_honest_proofs_and_rejects_one_broken_repetition(sec):
    S, nkeys = 616, 4
    params = R.synth_params(S, sec)
    ring = R.synth_ring_fast(S, nkeys)
    msg, sig, pk, which, d, seed = R.synth_proof_input(S, 0, nkeys)
    ring[which] = R.keyToInt(pk)
    c = CO.OracleCtx(_xy(params.NistGroup.h, 32), _xy(params.ProofGroup.g, 36), _xy(params.ProofGroup.h, 36), sec)
    c.set_ring(b''.join(v.to_bytes(32, 'big') for v in ring), nkeys)
    (proof,), st = c.prove_batch(msg, sig, pk[1:], [which], seeds=seed)
    assert st == [0]
    vseed = bytes(range(32))
    assert VA.model(params, ring, msg, proof, vseed) == (1, 0)
    lay = Layout(proof, 2, sec)
    broken = VA.bump_scalar(proof, lay.rep_scalars(sec - 1)[1], P256_N)   # beta1 or z2 of the last repetition
    assert VA.model(params, ring, msg, broken, vseed) == (0, 0)


@pytest.mark.parametrize('sec', [20, 21, 39, 40, 41, 80, 128])
def test_the_passes_cover_every_repetition(sec):
    passes = VA.pass_indices(sec)
    assert len(passes) == -(-sec // 20) and all(len(p) == 20 for p in passes)
    assert all(p == list(range(p[0], p[0] + 20)) for p in passes)
    assert sorted(set().union(*passes)) == list(range(sec))
    assert [p[0] for p in passes] == sorted(p[0] for p in passes)   # ascending: the first pass with an exception holds the lowest repetition that throws


def test_committed_seeds_miss_their_repetition():
    assert [r // 20 for r, _ in VA.MISSED] == [0, 1, 2, 3]
    for r, seed in VA.MISSED:
        idx = VA.sampled_indices(seed, 3, 80)
        assert len(set(idx)) == 20 and r not in idx, (r, sorted(idx))


def _lib():
    import zkp_ecdsa_amd as Z
    if not os.path.exists(Z.LIB_PATH):
        Z.build()
    return Z, Z.lib()


def test_setters_declared_exported_and_bound():
    Z, L = _lib()
    hdr = open(os.path.join(ROOT, 'include', 'zkattest.h')).read()
    declared = set(re.findall(r'\b(zk_[a-z0-9_]+)\s*\(', hdr))
    for s in ('zk_ctx_set_verify_reps', 'zk_pool_set_verify_reps'):
        assert s in declared and s in Z.SYMBOLS and hasattr(L, s), s
    assert re.search(r'ZK_VERIFY_REPS_SAMPLE = 0, ZK_VERIFY_REPS_ALL = 1', hdr)
    assert callable(getattr(Z.Engine, 'set_verify_reps', None)) and callable(getattr(Z.Pool, 'set_verify_reps', None))
    assert L.zk_ctx_set_verify_reps(C.c_void_p(), 1) == ZK_E_ARG and L.zk_pool_set_verify_reps(C.c_void_p(), 1) == ZK_E_ARG
    dts = open(os.path.join(ROOT, 'bindings', 'napi', 'zkattest.d.ts')).read()
    assert re.search(r"export function setVerifyReps\(name: 'sample' \| 'all'\)", dts)


@pytest.mark.gpu
def test_unknown_mode_is_refused():
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    assert eng.L.zk_ctx_set_verify_reps(eng.h, 2) == ZK_E_ARG
    assert eng.L.zk_ctx_set_verify_reps(eng.h, 1) == 0 and eng.L.zk_ctx_set_verify_reps(eng.h, 0) == 0
    eng.close()
