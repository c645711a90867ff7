"""The model of the key recovery (include/zkattest.h: zk_recover_batch) for tests/test_recover_host.py and tests/test_gpu_recover.py: the candidate
order and the winner rule of the header, literally, on oracle/zkattest_ref.py (p256, WeierstrassPoint, newScalar, truncateToN, ecdsa_verify) and Python
integers.  Every key it returns has passed the reference's ecdsa_verify.  The engine is never compared with itself."""
import zkattest_ref as R

P, N_ORD, B_COEF = R.p256.p, R.p256.order, R.p256.b
NONE = 0xFFFFFFFF
SIG_RANGE, NOT_IN_RING, RING_NOT_RESIDENT, NO_POINT = 2, 8, 16, 32
ZERO64 = bytes(64)


def be(v):
    return v.to_bytes(32, 'big')


def lift(x):
    """(x, even y) on the curve, or None where x^3 - 3x + b is no square mod p"""
    v = (x * x * x - 3 * x + B_COEF) % P
    y = pow(v, (P + 1) // 4, P)
    if y * y % P != v:
        return None
    return (x, y if y % 2 == 0 else P - y)


def candidates(msg, sig):
    """[(c, Q or None)] for the candidates that exist: c as in the header, Q = (x, y) affine integers, None for the identity.  r, s in range."""
    r, s = int.from_bytes(sig[:32], 'big'), int.from_bytes(sig[32:], 'big')
    z = R.truncateToN(int.from_bytes(msg, 'big'), N_ORD)
    rinv = pow(r, -1, N_ORD)
    u1, u2 = (-z * rinv) % N_ORD, (s * rinv) % N_ORD
    A = R.p256.generator().mul(R.p256.newScalar(u1))
    out = []
    for j, x in enumerate((r, r + N_ORD)):
        if x >= P:
            continue
        pt = lift(x)
        if pt is None:
            continue
        for odd in (0, 1):
            y = pt[1] if not odd else (P - pt[1]) % P
            Q = A.add(R.WeierstrassPoint(R.p256, x, y).mul(R.p256.newScalar(u2)))
            aff = Q.toAffine()
            out.append((2 * j + odd, aff if aff else None))
    return out


def model(msg, sig, ring):
    """ring: the caller's keys as integers -> (pk_xy_out, which_out, flags)"""
    r, s = int.from_bytes(sig[:32], 'big'), int.from_bytes(sig[32:], 'big')
    if not (1 <= r < N_ORD and 1 <= s < N_ORD):
        return ZERO64, NONE, SIG_RANGE
    cands = candidates(msg, sig)
    if not cands:
        return ZERO64, NONE, NO_POINT | NOT_IN_RING
    best = None
    for c, Q in cands:   # ascending c: a strictly lower index replaces, so ties stay with the lowest c
        if Q is None:
            continue
        idx = next((i for i, k in enumerate(ring) if k == Q[0]), NONE)
        if idx != NONE and (best is None or idx < best[0]):
            best = (idx, c, Q)
    if best is None:
        return ZERO64, NONE, NOT_IN_RING
    pk = be(best[2][0]) + be(best[2][1])
    assert R.ecdsa_verify(b'\x04' + pk, msg, sig), 'the model returned a key the reference does not verify the signature under'
    return pk, best[0], 0


def winner_c(msg, sig, ring):
    """the candidate number the model's winner has, or None"""
    pk, _, fl = model(msg, sig, ring)
    if fl:
        return None
    return next(c for c, Q in candidates(msg, sig) if Q is not None and be(Q[0]) + be(Q[1]) == pk)


def expect(wits, ring):
    """wits: [(msg, sig)] -> (pk list with None for flags != 0, which list, flags list), the shape Engine.recover_batch returns"""
    res = [model(m, s, ring) for m, s in wits]
    return [pk if fl == 0 else None for pk, _, fl in res], [w for _, w, _ in res], [fl for _, _, fl in res]
