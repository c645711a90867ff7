"""Shared by tests/test_gpu_ring_update.py and tests/ring_update_checksum_check.py: the update scenarios of zk_ctx_update_ring.

Every scenario is (old key list L, changes, new key count) -> new key list L'.  L' is always a prefix of a synthetic workload's ring W (whose signers sit at
W[b], b < B), so valid signatures exist for the keys of L'; L is derived from it by putting other keys ("junk": SHA-256 values, about half of them no
x-coordinate of the curve) where the update will write, by cutting the tail the update appends, or by adding the tail it truncates."""
import hashlib

SIZES = {8: 8, 1000: 304, 5000: 304}   # ring size -> proofs of the synthetic workload (signers at W[0 .. B))


def junk(i):
    return hashlib.sha256(b'ring-update: a key the update replaces %d' % i).digest()


def split(ring):
    ring = bytes(ring)
    return [ring[i:i + 32] for i in range(0, len(ring), 32)]


def padded_size(n):
    N = 2
    while N < n:
        N *= 2
    return N


def scenarios(W):
    """W: list of 32-byte keys.  -> list of (name, L, changes [(index, key)], new_n, L', fast) -- fast: the padded size stays"""
    n = len(W)
    small = n == 8
    interior = (1, 4, 6) if small else (7, 130, 300)   # 3 keys (in blocks 0 and 1 where the ring has two)
    inside = 6 if small else n - 10                    # an append / a truncation that stays inside the padded size
    half = 4 if small else {1000: 500, 5000: 4000}[n]  # ... and one that crosses a power of two
    grow_from = 4 if small else {1000: 500, 5000: 4090}[n]
    out = []

    def repl(pos):
        L = list(W)
        for p in pos:
            L[p] = junk(p)
        return L

    out.append(('interior', repl(interior), [(p, W[p]) for p in interior], n, list(W), True))
    out.append(('key0', repl((0,)), [(0, W[0])], n, list(W), True))
    out.append(('append_inside', W[:inside], [(i, W[i]) for i in range(inside, n)], n, list(W), True))
    out.append(('append_past', W[:grow_from], [(i, W[i]) for i in range(grow_from, n)], n, list(W), False))
    if small:
        out.append(('truncate_inside', list(W), [], inside, W[:inside], True))
    else:
        out.append(('truncate_inside', list(W) + [junk(1000 + i) for i in range(20)], [], n, list(W), True))
    out.append(('truncate_past', list(W), [], half, W[:half], False))
    p, q = interior[0], interior[1]
    out.append(('duplicate', repl((p, q)), [(p, junk(77)), (q, W[q]), (p, W[p])], n, list(W), True))
    for name, L, ch, new_n, Lp, fast in out:   # the scenarios state what they claim
        got = list(L[:new_n]) + [None] * (new_n - len(L))
        for i, k in ch:
            got[i] = k
        assert got == list(Lp) and (padded_size(len(L)) == padded_size(new_n)) == fast, name
    return out


def batch_indices(m, changed, B):
    """proofs of the workload to prove over a list of m keys: which = b for b < min(256, m) (every low-bit slice of table E), and the changed positions past them"""
    idx = list(range(min(256, m, B)))
    idx += [p for p in sorted(set(changed)) if p >= len(idx) and p < min(m, B)]
    return idx


def cut(work, idx, which=None):
    ring, msg, sig, pk, wh, seeds = work
    return (b''.join(msg[32 * i:32 * i + 32] for i in idx), b''.join(sig[64 * i:64 * i + 64] for i in idx), b''.join(pk[64 * i:64 * i + 64] for i in idx),
            [wh[i] for i in idx] if which is None else list(which), b''.join(seeds[32 * i:32 * i + 32] for i in idx))
