"""Shared by tests/test_gpu_distinct.py and tests/distinct_uniform_check.py: the seeded openings of a distinct-key workload and the Python oracle's side of a ZKD1
proof (oracle/zkattest_ref.py: proveMult / aggregateMult / MultiMult over Cx = C1 - C2, Cy = commit(1 / (x1 - x2)), Cz = g) in its byte layout."""
import hashlib

import link_common as LC
import member_common as MC

R = MC.R
TOM, Q = MC.TOM, MC.Q
PARAM_SEED = 5
SIZE = 744
be32, _point = LC.be32, LC._point
POINTS = ['C_w'] + list(R.MultProof.FIELDS_P)   # the seven points of a proof, 72 bytes each from offset 16
SCALARS = list(R.MultProof.FIELDS_S)            # the seven scalars, 32 bytes each from offset 520


def tag(t, i):
    return hashlib.sha256(b'distinct-test' + t + i.to_bytes(4, 'big')).digest()


def scalars(name, B):
    return [int.from_bytes(tag(name, b), 'big') % Q for b in range(B)]


def seeds_for(name, B):
    return b''.join(tag(b'seed' + name, b) for b in range(B))


def workload(name, B):
    """keys x1, x2, blinders r1, r2 and seeds of B distinct-key proofs"""
    return scalars(name + b'x1', B), scalars(name + b'r1', B), scalars(name + b'x2', B), scalars(name + b'r2', B), seeds_for(name, B)


def header():
    return b'ZKD1' + SIZE.to_bytes(4, 'big') + bytes(8)


def oracle_prove(pp, x1, c1_72, r1, x2, c2_72, r2, rng):
    """Cw = pp.commit(1 / d); proveMult(pp, d, 1 / d, 1, Commitment(C1 - C2, r1 - r2), Cw, Commitment(g, 0)) in the ZKD1 layout, d = x1 - x2"""
    d = (x1 - x2) % Q
    w = pow(d, -1, Q)
    Cd = R.Commitment(MC.tom_point(c1_72).sub(MC.tom_point(c2_72)), TOM.newScalar(r1).sub(TOM.newScalar(r2)))
    Cw = pp.commit(w, rng)
    pi = R.proveMult(pp, d, w, 1, Cd, Cw, R.Commitment(pp.g, TOM.newScalar(0)), rng)
    out = header() + R._tp(Cw.p) + R._mult_bytes(pi)
    assert len(out) == SIZE
    return out


def oracle_verify(pp, c1_72, c2_72, proof):
    """-> (ok, status): the deserialisation failure (10), or aggregateMult into a MultiMult, evaluate().isIdentity()"""
    try:
        if proof[:4] != b'ZKD1' or proof[4:8] != SIZE.to_bytes(4, 'big') or proof[8:16] != bytes(8) or len(proof) != SIZE:
            raise ValueError('header')
        C1, C2 = _point(c1_72), _point(c2_72)
        pts = [_point(proof[16 + 72 * k:88 + 72 * k]) for k in range(7)]
    except ValueError:
        return 0, 10
    sc = [TOM.newScalar(int.from_bytes(proof[520 + 32 * k:552 + 32 * k], 'big')) for k in range(7)]
    mm = R.MultiMult(TOM)
    R.aggregateMult(pp, C1.sub(C2), pts[0], pp.g, R.MultProof(*(pts[1:] + sc)), mm, R.OsRng(b'distinct-verifier'))
    return int(mm.evaluate().isIdentity()), 0
