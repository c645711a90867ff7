"""Ring keys whose balanced base-256 digits (k_gk_mfma.hip: gkm_digits) sit at their extremes -- not a test module: tests/test_gpu_verify.py and
tests/test_gpu_prove.py put these in place of a synthetic ring's non-signer keys."""
import zkattest_ref as R

Q = R.p256.p
PATTERNS = [bytes.fromhex(h) for h in (
    '00' * 32, '00' * 31 + '01',
    '80' * 32,                                  # every digit -128, carry digit 32 set
    '7f' * 32,                                  # every digit +127
    '7f' * 31 + '80',                           # a carry that ripples through all 32 digits into digit 32
    'ffffffff00000000' + 'ff' * 24,             # the largest value below the prime with ff in every byte the prime allows
    '00' + 'ff' * 31, 'fffffffe' + 'ff' * 28,
    '%064x' % (Q - 1),
    '80' + '00' * 31, '00' * 31 + '80',
    '7f80' * 16, '807f' * 16,
)]
assert all(int.from_bytes(p, 'big') < Q for p in PATTERNS)


def digits(v):
    """the recoding of gkm_digits on a Python integer: 33 digits in [-128, 127], digit 32 the carry"""
    out, carry = [], 0
    for u in range(32):
        t = ((v >> (8 * u)) & 255) + carry
        carry = 1 if t >= 128 else 0
        out.append(t - 256 * carry)
    return out + [carry]


_D = [digits(int.from_bytes(p, 'big')) for p in PATTERNS]
assert any(d[:32] == [-128] * 32 and d[32] == 1 for d in _D) and any(d[:32] == [127] * 32 for d in _D) and any(d[:32].count(-128) == 1 and d[32] == 1 for d in _D)


def extreme_ring(ring, which):
    """ring (32 bytes per key) with every key that no proof signs with replaced: block 0 (with the signers) and the last three 256-key blocks cycle through the
    patterns key by key, every block in between is filled with ONE pattern"""
    nkeys = len(ring) // 32
    keep = set(which)
    out = bytearray(ring)
    last = nkeys // 256 - 3
    for i in range(nkeys):
        if i in keep:
            continue
        blk = i >> 8
        out[32 * i:32 * i + 32] = PATTERNS[(i if blk == 0 or blk >= last else blk - 1) % len(PATTERNS)]
    return bytes(out)
