"""Shared by the threshold-opening tests (test_escrow_threshold_host.py, test_gpu_escrow_threshold.py): the Python statement of the t-of-n opening of an
escrow tag -- the dealer's split, an auditor's share "ZKS1", its verifier, the Lagrange combine and the bytes -- written from the oracle's primitives as
escrow_common.py is (Tom-256 points, hashPoints, rnd, the contract's RNG).  It is the yardstick for every byte and every answer of zk_auditors_*.

    split:   f(X) = a + c_1 X + ... + c_{t-1} X^{t-1}, c_i = rnd(q) (fills 0 .. t-2);  a_j = f(j), A_j = a_j g, j = 1..n
    share:   D = a_j E1, U1 = k g, U2 = k E1, k = rnd(q) (fill 0);  c = hashPoints([A_j, E1, D, U1, U2]);  s = k - c a_j
    verify:  s g + c A_j - U1 = O  and  s E1 + c D - U2 = O
    combine: lambda_j = prod_{m in S, m != j} m / (m - j);  M = 4 (E2 - sum_{j in S} lambda_j D_j), looked up as zk_rings_escrow_open_batch looks up its point
"""
import escrow_common as EC

R = EC.R
TOM, Q = EC.TOM, EC.Q
sc = EC.sc
SIZE = 264
NONE = ANY = 0xffffffff
MAX_N = 16
PT = [16 + 72 * k for k in range(3)]   # D, U1, U2
S_OFF = 232
E_BAD, E_ARG, E_OPENING = 10, 14, 16


def mul_plain(P, k):
    """k * P for an integer k taken as it stands (Point.mul reduces its scalar mod q, which is wrong for a point outside the prime-order group)"""
    acc = TOM.identity()
    for i in reversed(range(k.bit_length())):
        acc = acc.add(acc)
        if (k >> i) & 1:
            acc = acc.add(P)
    return acc


def split(pp, a, t, n, rng):
    """-> (shares a_1..a_n, keys A_1..A_n as points)"""
    assert 1 <= t <= n <= MAX_N
    coef = [a % Q] + [R.rnd(Q, rng) for _ in range(t - 1)]
    shares = []
    for j in range(1, n + 1):
        v = 0
        for c in reversed(coef):
            v = (v * j + c) % Q
        shares.append(v)
    return shares, [pp.g.mul(sc(v)) for v in shares]


def split_bytes(pp, a, t, n, rng):
    """-> (n x 32 bytes of shares, n x 72 bytes of keys), as zk_auditors_split_key writes them"""
    shares, keys = split(pp, a, t, n, rng)
    return EC.be32(shares), b''.join(R._tp(A) for A in keys)


def lagrange(S, at=0):
    """the coefficients of the indices S (all different) for the value at `at`, mod q, in S's order"""
    assert len(set(S)) == len(S)
    out = []
    for j in S:
        num = den = 1
        for m in S:
            if m != j:
                num, den = num * (m - at) % Q, den * (m - j) % Q
        out.append(num * pow(den, -1, Q) % Q)
    return out


def interpolate_points(S, pts, at=0):
    acc = pts[0].mul(sc(0))
    for lam, P in zip(lagrange(S, at), pts):
        acc = acc.add(P.mul(sc(lam)))
    return acc


def keys_consistent(A, t, keys):
    """zk_ctx_set_auditors' check: A_1..A_t interpolate to A at 0 and to A_m at every m > t, compared as bytes"""
    S = list(range(1, t + 1))
    if R._tp(interpolate_points(S, keys[:t], 0)) != R._tp(A):
        return False
    return all(R._tp(interpolate_points(S, keys[:t], m)) == R._tp(keys[m - 1]) for m in range(t + 1, len(keys) + 1))


def tag_points(tag, want=(0, 1)):
    """the tag's header and the points `want` of it (0: E1, 1: E2), or ValueError"""
    if len(tag) != EC.SIZE or tag[:4] != b'ZKT1' or tag[4:8] != EC.SIZE.to_bytes(4, 'big') or tag[8:16] != bytes(8):
        raise ValueError('tag header')
    return [EC.point(tag[EC.PT[k]:EC.PT[k] + 72]) for k in want]


def challenge(Aj, E1, D, U1, U2):
    return R.hashPoints([Aj, E1, D, U1, U2])


def to_bytes(j, D, U1, U2, s):
    return b'ZKS1' + SIZE.to_bytes(4, 'big') + j.to_bytes(4, 'big') + bytes(4) + b''.join(R._tp(p) for p in (D, U1, U2)) + R._sc(s)


def share(pp, j, aj, Aj, tag, rng):
    """auditor j's share of `tag`: (264 bytes, 0), or (264 zero bytes, 10) where the tag's header or E1 do not deserialise"""
    try:
        E1, = tag_points(tag, (0,))
    except ValueError:
        return bytes(SIZE), E_BAD
    k = R.rnd(Q, rng)
    D, U1, U2 = mul_plain(E1, aj % Q), pp.g.mul(sc(k)), mul_plain(E1, k)   # E1 comes out of a tag: it may carry a component of order 2 or 4
    c = sc(challenge(Aj, E1, D, U1, U2))
    return to_bytes(j, D, U1, U2, sc(k).sub(c.mul(sc(aj)))), 0


def parse(sh, n):
    """-> (j, D, U1, U2, s) or ValueError"""
    if len(sh) != SIZE or sh[:4] != b'ZKS1' or sh[4:8] != SIZE.to_bytes(4, 'big') or sh[12:16] != bytes(4):
        raise ValueError('share header')
    j = int.from_bytes(sh[8:12], 'big')
    if not 1 <= j <= n:
        raise ValueError('j')
    D, U1, U2 = [EC.point(sh[o:o + 72]) for o in PT]
    return j, D, U1, U2, sc(int.from_bytes(sh[S_OFF:], 'big'))   # the Scalar constructor reduces


def verify(pp, keys, tag, sh):
    """-> (ok, status) against the tag and the keys A_1..A_n (points)"""
    try:
        j, D, U1, U2, s = parse(sh, len(keys))
        E1, = tag_points(tag, (0,))
    except ValueError:
        return 0, E_BAD
    Aj = keys[j - 1]
    c = sc(challenge(Aj, E1, D, U1, U2))
    r1 = pp.g.mul(s).add(Aj.mul(c)).add(U1.neg()).isIdentity()
    r2 = E1.mul(s).add(D.mul(c)).add(U2.neg()).isIdentity()
    return int(r1 and r2), 0


def combine_point(n, auditors, tag, shares):
    """4 (E2 - sum lambda_j D_j) as affine bytes for the shares of slots 0 .. t-1 (slot s belongs to auditors[s]), or None where something does not
    deserialise: the tag's header, E1, E2, a share's header (j != auditors[s] included) or its D"""
    try:
        E1, E2 = tag_points(tag)
        Ds = []
        for want, sh in zip(auditors, shares):
            if len(sh) != SIZE or sh[:4] != b'ZKS1' or sh[4:8] != SIZE.to_bytes(4, 'big') or sh[12:16] != bytes(4) or int.from_bytes(sh[8:12], 'big') != want:
                raise ValueError('share header')
            Ds.append(EC.point(sh[PT[0]:PT[0] + 72]))
    except ValueError:
        return None
    return R._tp(EC.times4(E2.add(interpolate_points(list(auditors), Ds).neg())))


def combine(n, auditors, tag, shares, ring_id, tables):
    """-> (ring_out, index, status).  tables: {ring id: EC.ring_points' table}, ring_id one of them or ANY"""
    if ring_id != ANY and ring_id not in tables:
        return NONE, NONE, E_ARG
    m = combine_point(n, auditors, tag, shares)
    if m is None:
        return NONE, NONE, E_BAD
    for rid in sorted(tables) if ring_id == ANY else [ring_id]:
        if m in tables[rid]:
            return rid, tables[rid].index(m), 0
    return NONE, NONE, 0


def s_plus(sh, d):
    return sh[:S_OFF] + ((int.from_bytes(sh[S_OFF:], 'big') + d) % (1 << 256)).to_bytes(32, 'big')


def mutants(sh, tag, other_point72, other_tag, n):
    """(name, tag, share) for an honest share of `tag`: one mutant per field, s + q, j changed, the share beside another tag"""
    j = int.from_bytes(sh[8:12], 'big')
    rows = [('honest', tag, sh)]
    rows += [('%s := another point' % nm, tag, sh[:PT[k]] + other_point72 + sh[PT[k] + 72:]) for k, nm in enumerate(('D', 'U1', 'U2'))]
    rows += [('s + 1', tag, s_plus(sh, 1)),
             ('magic', tag, b'ZKT1' + sh[4:]),
             ('total_len', tag, sh[:4] + (263).to_bytes(4, 'big') + sh[8:]),
             ('reserved', tag, sh[:12] + b'\x00\x00\x00\x01' + sh[16:]),
             ('j := another auditor', tag, sh[:8] + (j % n + 1).to_bytes(4, 'big') + sh[12:]),
             ('j := 0', tag, sh[:8] + bytes(4) + sh[12:]),
             ('j := n + 1', tag, sh[:8] + (n + 1).to_bytes(4, 'big') + sh[12:]),
             ('off-curve coordinate', tag, sh[:PT[1] + 20] + bytes([sh[PT[1] + 20] ^ 0x40]) + sh[PT[1] + 21:]),
             ('another tag', other_tag, sh),
             ('a damaged tag header', b'ZKT2' + tag[4:], sh)]
    if int.from_bytes(sh[S_OFF:], 'big') + Q < 1 << 256:
        rows.append(('s + q', tag, s_plus(sh, Q)))
    return rows
