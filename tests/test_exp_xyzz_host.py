"""not-gpu: the XYZZ table sums of the Exp commit phase (curve.h: p256_xyzz_madd; rtab.h / ktab.h: the *_xyzz walks) compiled for the host CPU
(tests/host_arith/host_exp_xyzz.cpp, g++ -DZK_HOST_BUILD with an 8-bit comb for G and h) against the complete-law walks they replace in k_exp_commit_kt and
against the oracle's P-256 arithmetic: random scalars, empty sums, single digits, the signed-window extremes, and scalars crafted -- the prover knows the
discrete log of its key -- so that a partial sum meets a table entry (a doubling) or its negative (the identity).  The same source with its own main() is the
sanitizer build (-fsanitize=address,undefined), run here as a stand-alone program."""
import ctypes as C
import os
import random
import shutil
import subprocess

import pytest

import zkattest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host_arith', 'host_exp_xyzz.cpp')
FLAGS = ['-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-DPFIX_WIN_BITS=8', '-I' + os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')]

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')

g, n = R.p256, R.p256.order
SK, HS = 0x1F3C5A7E9B2D4F60718293A4B5C6D7E8F9010B2C3D4E5F6A7B8C9DAEBFC0D1E3 % n, 0x2468ACE013579BDF0FEDCBA9876543211234567890ABCDEFFEDCBA0987654321 % n


def _xy(pt):
    c = pt.toAffine()
    return bytes(64) if not c else c[0].to_bytes(32, 'big') + c[1].to_bytes(32, 'big')


def _mul(k):
    return g.generator().mul(g.newScalar(k % n))


@pytest.fixture(scope='module')
def hx(tmp_path_factory):
    out = tmp_path_factory.mktemp('host_exp_xyzz') / 'libhost_exp_xyzz.so'
    subprocess.check_call(['g++', '-O1', '-shared', '-fPIC'] + FLAGS + [SRC, '-o', str(out)])
    lib = C.CDLL(str(out))
    assert lib.hx_init(_xy(g.generator()), _xy(_mul(HS)), _xy(_mul(SK))) == 0
    return lib


def _sums(hx, cases, neg):
    cnt = len(cases)
    out = C.create_string_buffer(256 * cnt)
    fell = (C.c_uint32 * cnt)()
    assert hx.hx_sums(C.c_uint64(cnt), b''.join(x.to_bytes(32, 'big') for c in cases for x in c), neg, out, fell) == 0
    return [out.raw[256 * i:256 * i + 256] for i in range(cnt)], list(fell)


def _check(hx, cases, neg, want_fell):
    outs, fell = _sums(hx, cases, neg)
    sk = -SK if neg else SK
    for i, (gs, ks, bs) in enumerate(cases):
        t = gs + ks * sk
        T, A = _xy(_mul(t)), _xy(_mul(t + bs * HS))
        assert outs[i][0:128] == outs[i][128:256], (i, 'XYZZ sums differ from the complete law')
        assert outs[i][0:64] == T and outs[i][64:128] == A, (i, 'differs from the oracle')
    assert fell == want_fell, fell


def test_random_sums_equal_the_complete_law_and_the_oracle_without_fallback(hx):
    rnd = random.Random(41)
    cases = [(rnd.randrange(n), rnd.randrange(n), rnd.randrange(n)) for _ in range(24)]
    cases += [(rnd.randrange(1 << 256), rnd.randrange(1 << 256), rnd.randrange(1 << 256)) for _ in range(4)]   # the walks take any 256-bit scalar
    for neg in (0, 1):
        _check(hx, cases, neg, [0] * len(cases))


def test_empty_parts_single_digits_and_window_extremes(hx):
    rnd = random.Random(43)
    r = lambda: rnd.randrange(n)
    cases = [(0, 0, 0), (r(), 0, 0), (0, r(), 0), (0, 0, r()), (r(), r(), 0), (r(), 0, r()), (0, r(), r())]            # empty parts; all empty: T = A = identity
    cases += [(5 << 64, 0, 0), (0, 77 << 80, 0), (0, 0, 255 << 248), (0, 128, 0), (0, 129 << 8, 0), (1, 0, 1 << 255)]   # a single non-zero digit (129: -127 and a carry)
    cases += [(r(), int('80' * 32, 16), r()), (r(), int('81' * 32, 16), r()), (r(), int('7f80' * 16, 16), r()), (r(), int('ff' * 31 + '81', 16), r()),
              (int('ff' * 32, 16), int('80' * 31 + '7f', 16), int('ff' * 32, 16))]                                  # key digits at +128 / -127 / -128 + carry, full comb digits
    for neg in (0, 1):
        _check(hx, cases, neg, [0] * len(cases))


def test_crafted_collisions_fall_back_to_the_complete_law(hx):
    """pk = SK * G and h = HS * G with both logarithms known: the G-sum equals the key table's first entry (doubling) or its negative (identity) -> T and A fall
    back (3); T equals the first entry of h's comb or its negative -> A alone falls back (2).  The bytes are the complete law's and the oracle's."""
    rnd = random.Random(47)
    cases, want = [], []
    for _ in range(3):
        k = (rnd.randrange(n) & ~0xff) | rnd.randrange(1, 128)     # first key digit d in 1..127, positive
        d = k & 0xff
        b = rnd.randrange(n)
        cases += [(d * SK % n, k, b), (-d * SK % n, k, b)]
        want += [3, 3]
        b = (rnd.randrange(n) & ~0xff) | rnd.randrange(1, 256)     # first digit e of h's comb
        e = b & 0xff
        k = rnd.randrange(n)
        cases += [((e * HS - k * SK) % n, k, b), ((-e * HS - k * SK) % n, k, b)]
        want += [2, 2]
    cases += [(7 * SK % n, 7, 0), (-7 * SK % n, 7, 0)]            # ... with nothing from h: A = T, the second of them the identity
    want += [3, 3]
    _check(hx, cases, 0, want)


def test_bare_madd_chains(hx):
    rnd = random.Random(53)
    pts = [_mul(rnd.randrange(1, n)) for _ in range(9)]
    for m in (1, 2, 3, 9):
        out = C.create_string_buffer(64)
        assert hx.hx_chain(C.c_uint64(m), b''.join(_xy(p) for p in pts[:m]), out) == 0
        s = pts[0]
        for p in pts[1:m]:
            s = s.add(p)
        assert out.raw == _xy(s), m
    # the same x twice -- P + P, P + (-P) -- leaves ZZ = 0, and it stays 0 whatever follows
    for seq in ([pts[0], pts[0]], [pts[0], pts[0].neg()], [pts[0], pts[1], pts[0].add(pts[1]), pts[2], pts[3]], [pts[0], pts[1], pts[0].add(pts[1]).neg(), pts[2]]):
        assert hx.hx_chain(C.c_uint64(len(seq)), b''.join(_xy(p) for p in seq), C.create_string_buffer(64)) == 1


def test_stand_alone_program_under_the_host_sanitizers(tmp_path):
    exe = tmp_path / 'host_exp_xyzz'
    subprocess.check_call(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DHOST_EXP_XYZZ_MAIN'] + FLAGS + [SRC, '-o', str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and 'host_exp_xyzz ok' in r.stdout, r.stdout + r.stderr
