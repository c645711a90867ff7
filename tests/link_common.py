"""Shared by tests/test_gpu_link.py and tests/link_uniform_check.py: the seeded openings of a link-proof workload and the Python oracle's side of a ZKL1 proof
(oracle/zkattest_ref.py: proveEquality / aggregateEquality / MultiMult) in its byte layout."""
import hashlib

import member_common as MC

R = MC.R
TOM, Q = MC.TOM, MC.Q
PARAM_SEED = 5
SIZE = 256


def tag(t, i):
    return hashlib.sha256(b'link-test' + t + i.to_bytes(4, 'big')).digest()


def scalars(name, B):
    return [int.from_bytes(tag(name, b), 'big') % Q for b in range(B)]


def seeds_for(name, B):
    return b''.join(tag(b'seed' + name, b) for b in range(B))


def be32(vals):
    return b''.join(v.to_bytes(32, 'big') for v in vals)


def workload(name, B):
    """keys x, blinders r1, r2 and seeds of B link proofs"""
    return scalars(name + b'x', B), scalars(name + b'r1', B), scalars(name + b'r2', B), seeds_for(name, B)


def link_to_bytes(pi):
    return b'ZKL1' + SIZE.to_bytes(4, 'big') + bytes(8) + R._tp(pi.A_1) + R._tp(pi.A_2) + R._sc(pi.t_x) + R._sc(pi.t_r1) + R._sc(pi.t_r2)


def oracle_prove(pp, x, c1_72, r1, c2_72, r2, rng):
    """proveEquality(pp, x, Commitment(C1, r1), Commitment(C2, r2), rng) in the ZKL1 layout"""
    C1, C2 = R.Commitment(MC.tom_point(c1_72), TOM.newScalar(r1)), R.Commitment(MC.tom_point(c2_72), TOM.newScalar(r2))
    return link_to_bytes(R.proveEquality(pp, x, C1, C2, rng))


def _point(b72):
    """deserializePoint's rules (edwards.ts:70-86) on a 72-byte point: the padding bytes zero, both coordinates below p, on the curve"""
    if b72[:3] != bytes(3) or b72[36:39] != bytes(3):
        raise ValueError('a not in range')
    return TOM.deserializePoint(b'\x04' + b72[3:36] + b72[39:])


def oracle_verify(pp, c1_72, c2_72, proof):
    """-> (ok, status): the deserialisation failure (10), or aggregateEquality into a MultiMult, evaluate().isIdentity()"""
    try:
        if proof[:4] != b'ZKL1' or proof[4:8] != SIZE.to_bytes(4, 'big') or proof[8:16] != bytes(8) or len(proof) != SIZE:
            raise ValueError('header')
        C1, C2, A1, A2 = _point(c1_72), _point(c2_72), _point(proof[16:88]), _point(proof[88:160])
    except ValueError:
        return 0, 10
    sc = [TOM.newScalar(int.from_bytes(proof[160 + 32 * k:192 + 32 * k], 'big')) for k in range(3)]
    mm = R.MultiMult(TOM)
    R.aggregateEquality(pp, C1, C2, R.EqualityProof(A1, A2, *sc), mm, R.OsRng(b'link-verifier'))
    return int(mm.evaluate().isIdentity()), 0
