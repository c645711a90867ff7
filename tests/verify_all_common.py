"""The model of the exhaustive verify mode (include/zkattest.h: ZK_VERIFY_REPS_ALL), shared by tests/test_verify_all_host.py (CPU tier) and
tests/test_gpu_verify_all.py (-m gpu): the Python restatement's verifySignatureList with verifyExp(..., secparam = len(proof.expProof), Q) and
the repetitions walked in ascending index order.  The oracle file stays as it is: generateIndices is replaced while the model runs."""
import hashlib

import zkattest_ref as R

VK = 20


def pass_indices(sec):
    """The repetitions every pass of the engine checks: P = ceil(sec / 20) passes, pass r < P - 1 over 20 r .. 20 r + 19, the last one over
    sec - 20 .. sec - 1."""
    assert sec >= VK
    P = (sec + VK - 1) // VK
    return [list(range(VK * r, VK * r + VK)) if r < P - 1 else list(range(sec - VK, sec)) for r in range(P)]


class VerifierRng:
    """verifier-RNG contract (include/zkattest.h): fill k = SHA-256(seed || be64(k))"""

    def __init__(self, seed):
        self.seed, self.k = bytes(seed), 0

    def fill(self, nbytes):
        out = hashlib.sha256(self.seed + self.k.to_bytes(8, 'big')).digest()
        self.k += 1
        return out[:nbytes]


def verify_all(params, msgHash, keys, proof, vrng, hardened=False):
    """oracle/zkattest_ref.py: verifySignatureList, restated, with secparam = the proof's own repetition count and generateIndices = 0 .. limit - 1"""
    ec = R.p256
    groupOrder = ec.order
    z = R.truncateToN(R.fromBytes(msgHash), groupOrder)
    Rp = proof.R
    coordR = Rp.toAffine()
    if not coordR:
        raise ValueError('R is at infinity')
    rinv = R.invMod(coordR[0], groupOrder)
    paramsSigExp = R.PedersenParams(R.p256, Rp, params.NistGroup.h)
    z1 = R.posMod(rinv * z, groupOrder)
    Q = ec.generator().mul(ec.newScalar(z1))
    stmt = R.gk_statement([v.k for v in R.pad(keys, params.ProofGroup.c)], msgHash, Rp, proof.keyXcom) if hardened else b''
    if not R.verifyMembership(params.ProofGroup, proof.keyXcom, keys, proof.membershipProof, vrng, statement=stmt):
        return False
    if len(proof.expProof) < VK:   # the sampled verifier's rule (verifyExp(..., 20, Q): 20 > pi.length)
        raise ValueError('security level not achieved')
    saved = R.generateIndices
    R.generateIndices = lambda indnum, limit, vrng: list(range(limit))
    try:
        return bool(R.verifyExp(paramsSigExp, params.ProofGroup, proof.comS1, proof.keyXcom, proof.keyYcom, proof.expProof, len(proof.expProof), vrng, Q))
    finally:
        R.generateIndices = saved


_CODES = ((3, 'T is at infinity'), (3, 'T[i] is at infinity'), (4, 'T1 is at infinity'), (8, 'params not found'), (9, 'security level'), (7, 'R is at infinity'))


def model(params, keys, msg32, raw, vseed, hardened=False):
    """(ok, status) of the model for one ZKA1 proof, exceptions mapped to the status codes of include/zkattest.h like tests/test_oracle_mutants.py maps them"""
    try:
        proof = R.proof_from_bytes(raw)
    except Exception:
        return 0, 10
    try:
        return (1 if verify_all(params, msg32, keys, proof, VerifierRng(vseed), hardened) else 0), 0
    except ValueError as e:
        for code, text in _CODES:
            if text in str(e):
                return 0, code
        raise


def params_of(nh, tg, th, sec):
    """SystemParametersList from the byte forms the engine's synth_params returns"""
    g = R.tomEdwards256.generator()
    assert g.toAffine()[0].to_bytes(36, 'big') + g.toAffine()[1].to_bytes(36, 'big') == bytes(tg)
    return R.SystemParametersList(
        R.PedersenParams(R.p256, R.p256.generator(), R.WeierstrassPoint(R.p256, int.from_bytes(nh[:32], 'big'), int.from_bytes(nh[32:], 'big'), 1)),
        R.PedersenParams(R.tomEdwards256, g, R.TEdwardsPoint(R.tomEdwards256, int.from_bytes(th[:36], 'big'), int.from_bytes(th[36:], 'big'))), sec)


def bump_scalar(raw, pos, mod):
    """the 32-byte scalar at `pos` incremented mod `mod`"""
    v = (int.from_bytes(raw[pos:pos + 32], 'big') + 1) % mod
    return raw[:pos] + v.to_bytes(32, 'big') + raw[pos + 32:]


def sampled_indices(vseed, n, sec):
    """The 20 repetitions the SAMPLED verifier checks under `vseed` over a ring of 2^n keys: verifyMembership's 2n + 1 randomScalar draws, then
    generateIndices(20, sec) (the verifier-seed contract of include/zkattest.h)."""
    vrng = VerifierRng(vseed)
    for _ in range(2 * n + 1):
        R.tomEdwards256.randomScalar(vrng)
    return R.generateIndices(VK, sec, vrng)[:VK]


# tests/test_gpu_verify_all.py, test 1: (broken repetition r, verifier seed S) with r outside sampled_indices(S, 3, 80) -- one r in each of the four passes
MISSED = ((3, hashlib.sha256(b'verify-all/0').digest()), (27, hashlib.sha256(b'verify-all/1').digest()),
          (45, hashlib.sha256(b'verify-all/0').digest()), (79, hashlib.sha256(b'verify-all/0').digest()))
