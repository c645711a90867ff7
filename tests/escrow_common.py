"""Shared by the escrow-tag tests (test_escrow_host.py, test_gpu_escrow.py, escrow_uniform_check.py): the Python statement of an escrow tag "ZKT1" -- prove,
verify, open and the bytes -- written from the oracle's primitives (oracle/zkattest_ref.py: Tom-256 points, PedersenParams over (g, h) and over (g, A),
hashPoints, the contract's RNG), and the seeded workloads.  It is the yardstick for every byte the engine writes.

    E1 = rho g   E2 = x g + rho A   T1 = k_x g + k_r h   T2 = k_rho g   T3 = k_x g + k_rho A
    c = hashPoints([C, E1, E2, A, T1, T2, T3])   t_x = k_x - c x   t_r = k_r - c r   t_rho = k_rho - c rho
    draws: fill 0 rho, 1 k_x, 2 k_r, 3 k_rho, all rnd(q)
    open: the lowest i with 4 y_i g = 4 E2 - a (4 E1), or 0xffffffff
"""
import hashlib

import member_common as MC

R = MC.R
TOM, Q = MC.TOM, MC.Q
PARAM_SEED = 5
SIZE = 472
NONE = 0xffffffff
PT = [16 + 72 * k for k in range(5)]     # E1, E2, T1, T2, T3
SC = [376 + 32 * k for k in range(3)]    # t_x, t_r, t_rho


def tag(t, i):
    return hashlib.sha256(b'escrow-test' + t + i.to_bytes(4, 'big')).digest()


def scalars(name, B):
    return [int.from_bytes(tag(name, b), 'big') % Q for b in range(B)]


def seeds_for(name, B):
    return b''.join(tag(b'seed' + name, b) for b in range(B))


def be32(vals):
    return b''.join(v.to_bytes(32, 'big') for v in vals)


def workload(name, B):
    """keys x, blinders r and seeds of B tags"""
    return scalars(name + b'x', B), scalars(name + b'r', B), seeds_for(name, B)


def sc(v):
    return TOM.newScalar(v)


def commit2(base1, v, base2, r):
    """v base1 + r base2"""
    return base2.dblmul(sc(r), base1, sc(v))


def keygen(pp, a):
    return pp.g.mul(sc(a))


def point(b72):
    """deserializePoint's rules (edwards.ts:70-86) on a 72-byte point: the padding bytes zero, both coordinates below p, on the curve"""
    if b72[:3] != bytes(3) or b72[36:39] != bytes(3):
        raise ValueError('a not in range')
    return TOM.deserializePoint(b'\x04' + b72[3:36] + b72[39:])


def small_order_points():
    """(a point of order 2, a point of order 4) of Tom-256: (0, -1) and (1 / sqrt(a), 0)"""
    p, a = TOM.p, TOM.a % TOM.p
    ia = pow(a, -1, p)
    assert p % 4 == 3
    x = pow(ia, (p + 1) // 4, p)
    assert x * x % p == ia, 'a is not a square: no point of order 4 with y = 0'
    P2, P4 = R.TEdwardsPoint(TOM, 0, p - 1, 0, 1), R.TEdwardsPoint(TOM, x, 0, 0, 1)
    assert not P2.isIdentity() and P2.add(P2).isIdentity()
    assert not P4.add(P4).isIdentity() and P4.add(P4).add(P4.add(P4)).isIdentity()
    return P2, P4


def challenge(C, E1, E2, A, T1, T2, T3):
    return R.hashPoints([C, E1, E2, A, T1, T2, T3])


def to_bytes(E1, E2, T1, T2, T3, tx, tr, trho):
    return b'ZKT1' + SIZE.to_bytes(4, 'big') + bytes(8) + b''.join(R._tp(p) for p in (E1, E2, T1, T2, T3)) + b''.join(R._sc(s) for s in (tx, tr, trho))


def prove(pp, A, x, c72, r, rng):
    """the tag for C = x g + r h under auditor key A, C as the caller states it (72 bytes), in the ZKT1 layout"""
    q = TOM.order
    rho, kx, kr, krho = R.rnd(q, rng), R.rnd(q, rng), R.rnd(q, rng), R.rnd(q, rng)
    x, r = x % q, r % q
    C = MC.tom_point(c72)
    E1, E2 = pp.g.mul(sc(rho)), commit2(pp.g, x, A, rho)
    T1, T2, T3 = commit2(pp.g, kx, pp.h, kr), pp.g.mul(sc(krho)), commit2(pp.g, kx, A, krho)
    c = sc(challenge(C, E1, E2, A, T1, T2, T3))
    return to_bytes(E1, E2, T1, T2, T3, sc(kx).sub(c.mul(sc(x))), sc(kr).sub(c.mul(sc(r))), sc(krho).sub(c.mul(sc(rho))))


def verify(pp, A, c72, t):
    """-> (ok, status): the deserialisation failure (10), or whether the three relations hold exactly"""
    try:
        if len(t) != SIZE or t[:4] != b'ZKT1' or t[4:8] != SIZE.to_bytes(4, 'big') or t[8:16] != bytes(8):
            raise ValueError('header')
        C = point(c72)
        E1, E2, T1, T2, T3 = [point(t[o:o + 72]) for o in PT]
    except ValueError:
        return 0, 10
    tx, tr, trho = [sc(int.from_bytes(t[o:o + 32], 'big')) for o in SC]   # the Scalar constructor reduces
    c = sc(challenge(C, E1, E2, A, T1, T2, T3))
    r1 = pp.g.mul(tx).add(pp.h.mul(tr)).add(C.mul(c)).add(T1.neg()).isIdentity()
    r2 = pp.g.mul(trho).add(E1.mul(c)).add(T2.neg()).isIdentity()
    r3 = pp.g.mul(tx).add(A.mul(trho)).add(E2.mul(c)).add(T3.neg()).isIdentity()
    return int(r1 and r2 and r3), 0


def times4(P):
    P2 = P.add(P)
    return P2.add(P2)


def open_point(a, t):
    """4 E2 - a (4 E1) as affine bytes, or None where the header, E1 or E2 do not deserialise"""
    try:
        if len(t) != SIZE or t[:4] != b'ZKT1' or t[4:8] != SIZE.to_bytes(4, 'big') or t[8:16] != bytes(8):
            raise ValueError('header')
        E1, E2 = point(t[PT[0]:PT[0] + 72]), point(t[PT[1]:PT[1] + 72])
    except ValueError:
        return None
    return R._tp(times4(E2).add(times4(E1).mul(sc(a)).neg()))


def ring_points(pp, ring):
    """4 y_i g of every ring key as affine bytes"""
    return [R._tp(times4(pp.g.mul(sc(y)))) for y in ring]


def open_tag(a, t, table):
    """-> (index, status) against ring_points' table"""
    m = open_point(a, t)
    if m is None:
        return NONE, 10
    return (table.index(m) if m in table else NONE), 0


def sc_plus(t, k, d):
    o = SC[k]
    return t[:o] + ((int.from_bytes(t[o:o + 32], 'big') + d) % (1 << 256)).to_bytes(32, 'big') + t[o + 32:]


def mutants(t, c72, other_point72, other_c72):
    """(name, com, tag) for an honest tag t of commitment c72: one mutant per field.  other_point72: another valid point; other_c72: another commitment"""
    names = ['E1', 'E2', 'T1', 'T2', 'T3']
    rows = [('honest', c72, t)]
    rows += [(names[k] + ' := another point', c72, t[:PT[k]] + other_point72 + t[PT[k] + 72:]) for k in range(5)]
    rows += [('%s + 1' % n, c72, sc_plus(t, k, 1)) for k, n in enumerate(('t_x', 't_r', 't_rho'))]
    rows += [('a wrong com', other_c72, t),
             ('magic', c72, b'ZKL1' + t[4:]),
             ('total_len', c72, t[:4] + (471).to_bytes(4, 'big') + t[8:]),
             ('reserved', c72, t[:12] + b'\x00\x00\x00\x01' + t[16:]),
             ('off-curve coordinate', c72, t[:PT[2] + 20] + bytes([t[PT[2] + 20] ^ 0x40]) + t[PT[2] + 21:])]
    for k, n in enumerate(('t_x', 't_r', 't_rho')):
        if int.from_bytes(t[SC[k]:SC[k] + 32], 'big') + Q < 1 << 256:
            rows.append(('%s + q' % n, c72, sc_plus(t, k, Q)))
    return rows
