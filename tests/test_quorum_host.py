"""not-gpu: the quorum proofs' plan (zkp-ecdsa_amd/csrc/quorum_plan.h) compiled for the host CPU (tests/host_arith/host_quorum.cpp): unrank and rank are
inverse for every k in 2..16 and give Engine.distinct_pairs' order, the sizes are the specified ones, and the header walk accepts an exact fit and refuses a
slot one byte short, an inner total_len that overruns or is no multiple of 4 and the other layout's magic; the same source as a program of its own under
the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host_arith', 'host_quorum.cpp')
FLAGS = ['-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-I' + os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')]
PAIR = 744

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')


@pytest.fixture(scope='module')
def hq(tmp_path_factory):
    out = tmp_path_factory.mktemp('host_quorum') / 'libhost_quorum.so'
    subprocess.check_call(['g++', '-O1', '-shared', '-fPIC'] + FLAGS + [SRC, '-o', str(out)])
    L = C.CDLL(str(out))
    L.hq_max_size.restype = L.hq_size.restype = C.c_uint64
    L.hq_max_size.argtypes = L.hq_size.argtypes = [C.c_uint32, C.c_uint64]
    L.hq_walk.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)]
    return L


def test_unrank_and_rank_are_inverse_and_equal_distinct_pairs(hq):
    import zkp_ecdsa_amd as Z
    for k in range(2, 17):
        pairs = Z.Engine.distinct_pairs(k)
        assert hq.hq_pairs(k) == len(pairs) == k * (k - 1) // 2
        for p, (i, j) in enumerate(pairs):
            ij = (C.c_uint32 * 2)()
            hq.hq_unrank(k, p, ij)
            assert (ij[0], ij[1]) == (i, j) and hq.hq_rank(k, i, j) == p, (k, p)
    assert [hq.hq_pairs(k) for k in (0, 1, 17, 100)] == [0, 0, 0, 0] and hq.hq_pairs(16) == 120


def test_sizes(hq):
    for k in (2, 3, 16):
        P = k * (k - 1) // 2
        assert hq.hq_max_size(k, 75000) == 16 + k * 75000 + PAIR * P
        assert hq.hq_size(k, 12344) == 16 + 12344 + PAIR * P
    assert hq.hq_max_size(1, 75000) == 0 and hq.hq_max_size(17, 75000) == 0 and hq.hq_max_size(3, 0) == 0
    out = C.create_string_buffer(16)
    hq.hq_header(0x01020304, 5, out)
    assert out.raw == b'ZKQ1' + bytes([1, 2, 3, 4]) + struct.pack('>II', 5, 0)


def _bundle(hq, k, lens, packed, n=3, magic=None):
    """headers only: the walk reads nothing else"""
    body = b''
    for ln in lens:
        body += (magic or (b'ZK1P' if packed else b'ZKA1')) + struct.pack('>III', ln, 20, n) + bytes(ln - 16)
    body += bytes(PAIR * (k * (k - 1) // 2))
    return b'ZKQ1' + struct.pack('>III', 16 + len(body), k, 0) + body


def _walk(hq, blob, o0, o1, k, packed):
    off = (C.c_uint64 * (k + 1))()
    return hq.hq_walk(blob, o0, o1, k, packed, off), list(off)


@pytest.mark.parametrize('packed', [0, 1])
def test_header_walk(hq, packed):
    k, m = 3, hq.hq_min_member(packed, 3)
    lens = [m, m + 8, m + 4]
    b = _bundle(hq, k, lens, packed)
    # exact fit, alone and between two neighbours
    assert _walk(hq, b, 0, len(b), k, packed) == (1, [16, 16 + m, 16 + 2 * m + 8, len(b) - 3 * PAIR])
    blob = b + b + b
    ok, off = _walk(hq, blob, len(b), 2 * len(b), k, packed)
    assert ok == 1 and off == [len(b) + o for o in (16, 16 + m, 16 + 2 * m + 8, len(b) - 3 * PAIR)]
    # one byte short; a slot that is no multiple of 4; a misaligned start; offsets that do not ascend
    assert _walk(hq, blob, 0, len(b) - 1, k, packed)[0] == 0
    assert _walk(hq, blob, 0, len(b) - 4, k, packed)[0] == 0 and _walk(hq, blob, 0, len(b) + 4, k, packed)[0] == 0
    assert _walk(hq, blob, 2, len(b) + 2, k, packed)[0] == 0 and _walk(hq, blob, len(b), 0, k, packed)[0] == 0
    # the header: magic, k, the reserved word
    assert _walk(hq, b'ZKQ2' + b[4:], 0, len(b), k, packed)[0] == 0
    assert _walk(hq, b, 0, len(b), k + 1, packed)[0] == 0 and _walk(hq, b, 0, len(b), k - 1, packed)[0] == 0
    assert _walk(hq, b[:15] + b'\x01' + b[16:], 0, len(b), k, packed)[0] == 0
    assert _walk(hq, b, 0, len(b), 1, packed)[0] == 0 and _walk(hq, b, 0, len(b), 17, packed)[0] == 0
    # an inner total_len that overruns (the last member claims the pairs too), one that stops short, one that is no multiple of 4
    at = 16 + lens[0] + lens[1] + 4
    assert _walk(hq, b[:at] + struct.pack('>I', lens[2] + 3 * PAIR) + b[at + 4:], 0, len(b), k, packed)[0] == 0
    assert _walk(hq, b[:at] + struct.pack('>I', lens[2] - 4) + b[at + 4:], 0, len(b), k, packed)[0] == 0
    c = _bundle(hq, k, [m + 2, m + 2, m + 4], packed)
    assert _walk(hq, c, 0, len(c), k, packed)[0] == 0
    # the other layout's magic in one member; a member shorter than its n asks for; n above 63
    other = b'ZKA1' if packed else b'ZK1P'
    assert _walk(hq, b[:16] + other + b[20:], 0, len(b), k, packed)[0] == 0
    assert _walk(hq, _bundle(hq, k, lens, packed, magic=other), 0, len(b), k, packed)[0] == 0
    c = _bundle(hq, k, [m, m - 4, m], packed)
    assert _walk(hq, c, 0, len(c), k, packed)[0] == 0
    big = hq.hq_min_member(packed, 64)
    c = _bundle(hq, k, [big, big, big], packed, n=64)
    assert _walk(hq, c, 0, len(c), k, packed)[0] == 0
    # fewer members than k: the walk ends in the pairs' bytes
    c = _bundle(hq, k, lens[:2], packed)
    c = c[:8] + struct.pack('>I', k) + c[12:]
    assert _walk(hq, c, 0, len(c), k, packed)[0] == 0


def test_program_of_its_own_under_the_sanitizers(tmp_path):
    exe = tmp_path / 'host_quorum'
    subprocess.check_call(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DHOST_QUORUM_MAIN'] + FLAGS + [SRC, '-o', str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and 'host_quorum: ok' in r.stdout, r.stdout + r.stderr
