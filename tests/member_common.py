"""Shared by tests/test_gpu_member.py and tests/member_uniform_check.py: the two test rings, the seeds, and the Python oracle's side of a membership proof
(oracle/zkattest_ref.py: commit / proveMembership / verifyMembership) in the ZKM1 byte layout."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'oracle')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import zkattest_ref as R   # noqa: E402

PARAM_SEED = 5
TOM = R.tomEdwards256
Q = TOM.order


def tag(t, i):
    return hashlib.sha256(b'member-test' + t + i.to_bytes(4, 'big')).digest()


def ring_values(name, count):
    return [int.from_bytes(tag(name, i), 'big') % Q for i in range(count)]


RING5 = ring_values(b'ring5', 5)        # N = 8, n = 3: the plain fold
RING300 = ring_values(b'ring300', 300)  # N = 512, n = 9: table E, 212 padding entries


def ring_bytes(values):
    return b''.join(v.to_bytes(32, 'big') for v in values)


def seeds_for(name, B):
    return b''.join(tag(b'seed' + name, b) for b in range(B))


def proof_size(n):
    return 16 + 288 * n + 32 * (3 * n + 1)


def tom_point(b72):
    x, y = int.from_bytes(b72[:36], 'big'), int.from_bytes(b72[36:], 'big')
    return R.TEdwardsPoint(TOM, x, y, x * y % TOM.p, 1)


def oracle_params(tom_g72, tom_h72):
    return R.PedersenParams(TOM, tom_point(tom_g72), tom_point(tom_h72))


def gk_to_bytes(pi):
    n = len(pi.cl)
    body = b''.join(R._tp(p) for p in pi.cl + pi.ca + pi.cb + pi.cd) + b''.join(R._sc(s) for s in pi.f + pi.za + pi.zb) + R._sc(pi.zd)
    return b'ZKM1' + (16 + len(body)).to_bytes(4, 'big') + n.to_bytes(4, 'big') + bytes(4) + body


def gk_from_bytes(b):
    """a ZKM1 proof that deserialises -> GKProof (scalars reduced as the Scalar constructor does)"""
    n = int.from_bytes(b[8:12], 'big')
    pts = [tom_point(b[16 + 72 * k:16 + 72 * (k + 1)]) for k in range(4 * n)]
    o = 16 + 288 * n
    sc = [TOM.newScalar(int.from_bytes(b[o + 32 * k:o + 32 * (k + 1)], 'big')) for k in range(3 * n + 1)]
    return R.GKProof(pts[:n], pts[n:2 * n], pts[2 * n:3 * n], pts[3 * n:], sc[:n], sc[n:2 * n], sc[2 * n:3 * n], sc[3 * n])


def oracle_prove(params, values, index, rng, blinder=None):
    """commit(values[index]) then proveMembership on ONE rng (blinder None), or a commitment with the caller's blinder and proveMembership alone.
    Returns (proof bytes, com bytes, blinder bytes)."""
    v = R.pad(values, TOM)[index].k
    if blinder is None:
        com = params.commit(v, rng)
    else:
        com = R.Commitment(R.gk_commit(params, v, blinder), TOM.newScalar(blinder))
    pi = R.proveMembership(params, com, index, values, rng)
    return gk_to_bytes(pi), R._tp(com.p), R._sc(com.r)


def oracle_verify(params, values, com72, proof_bytes):
    return bool(R.verifyMembership(params, tom_point(com72), values, gk_from_bytes(proof_bytes), R.OsRng()))
