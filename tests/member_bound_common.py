"""Shared by the bound-membership tests (tests/test_gpu_member_bound.py, tests/member_bound_uniform_check.py, tests/test_member_bound_host.py): the statement
S_b of a "ZKMB" proof (include/zkattest.h: zk_member_*_bound) assembled from the oracle's own parts, and the Python oracle's side of such a proof --
oracle/zkattest_ref.py's proveMembership / verifyMembership with statement=S_b, unchanged, under the RNG contract of tests/member_common.py."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import member_common as M   # noqa: E402

R = M.R
TAG = b'ZKAttest-GK-member-v1'
STATEMENT_BYTES = 21 + 32 + 32 + 67


def context_for(name, b):
    return M.tag(b'context' + name, b)


# name -> (real keys, the three indices proved: first, an inner one, the last of the padded ring -- a padding copy of keys[0] where the ring is padded)
RINGS = {'k2': (2, [0, 1, 1]), 'k3': (3, [0, 2, 3]), 'k8': (8, [0, 5, 7]), 'k256': (256, [0, 128, 255]), 'k300': (300, [1, 299, 511]), 'k4096': (4096, [0, 2049, 4095])}
LOG2 = {'k2': 1, 'k3': 2, 'k8': 3, 'k256': 8, 'k300': 9, 'k4096': 12}
MODES = ('drawn', 'caller')


def inputs(name):
    """which, contexts, seeds, caller blinders of a ring's three proofs"""
    which = RINGS[name][1]
    ctx = [context_for(name.encode(), b) for b in range(3)]
    seeds = M.seeds_for(b'bound' + name.encode(), 3)
    bl = [int.from_bytes(M.tag(b'bblind' + name.encode(), b), 'big') % M.Q for b in range(3)]
    return which, ctx, seeds, bl


def padded(values):
    return [v.k for v in R.pad(values, M.TOM)]


def statement_bytes(digest32, context32, com67):
    assert len(digest32) == 32 and len(context32) == 32 and len(com67) == 67 and com67[0] == 4
    return TAG + digest32 + context32 + com67


def statement(values, context32, com_point):
    """S_b for a proof over `values` (padded here): tag || ring_digest || context || com as hashPoints encodes a point"""
    s = statement_bytes(R.ring_digest(padded(values)), bytes(context32), com_point.toBytes())
    assert len(s) == STATEMENT_BYTES
    return s


def to_zkmb(pi):
    b = M.gk_to_bytes(pi)
    return b'ZKMB' + b[4:]


def oracle_prove(params, values, index, rng, context32, blinder=None):
    """member_common.oracle_prove with the statement: commit (or the caller's blinder), then proveMembership(..., statement=S_b) on the same rng.
    Returns (proof bytes, com bytes, blinder bytes)."""
    v = R.pad(values, M.TOM)[index].k
    if blinder is None:
        com = params.commit(v, rng)
    else:
        com = R.Commitment(R.gk_commit(params, v, blinder), M.TOM.newScalar(blinder))
    pi = R.proveMembership(params, com, index, values, rng, statement=statement(values, context32, com.p))
    return to_zkmb(pi), R._tp(com.p), R._sc(com.r)


def oracle_verify(params, values, com72, proof_bytes, context32):
    assert proof_bytes[:4] == b'ZKMB'
    com = M.tom_point(com72)
    return bool(R.verifyMembership(params, com, values, M.gk_from_bytes(proof_bytes), R.OsRng(), statement=statement(values, context32, com)))
