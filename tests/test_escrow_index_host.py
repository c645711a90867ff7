"""not-gpu: the resident point index (zkp-ecdsa_amd/csrc/escrow_index.h) compiled for the host CPU (tests/host_arith/host_escrow_index.cpp) against the
Python restatement (tests/escrow_index_common.py): the slot function on random and extreme x, the vectors the program of its own carries, insert-then-lookup
against a brute-force scan with home slots chosen in Python (a cluster that wraps from the last slot to slot 0, equal points at several indices under several
insertion orders, the fullest allowed load, absent points that end at an empty slot); the header states the function; and the same source as a program of
its own under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import random
import re
import shutil
import subprocess

import pytest

import escrow_index_common as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host_arith', 'host_escrow_index.cpp')
FLAGS = ['-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-I' + os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')]
EXTREME = [0, 1, (1 << 64) - 1, 1 << 32, (1 << 30) - 1, 1 << 30, (1 << 60) | (1 << 31), (1 << 270) - 1]

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')


@pytest.fixture(scope='module')
def hei(tmp_path_factory):
    out = tmp_path_factory.mktemp('host_escrow_index') / 'libhost_escrow_index.so'
    subprocess.check_call(['g++', '-O1', '-shared', '-fPIC'] + FLAGS + [SRC, '-o', str(out)])
    L = C.CDLL(str(out))
    L.hei_cap.argtypes = [C.c_uint64]
    for f in (L.hei_cap, L.hei_hash, L.hei_home):
        f.restype = C.c_uint32
    return L


def _values():
    rnd = random.Random(4242)   # the program's vectors: these eight and the first eight draws
    return EXTREME + [rnd.getrandbits(270) for _ in range(200)]


def test_slot_function_against_the_python_restatement(hei):
    for nkeys, want in ((2, 2), (3, 4), (5, 8), (256, 256), (257, 512), (600, 1024), (1 << 20, 1 << 20)):
        assert hei.hei_cap(nkeys) == want == IC.entries(nkeys) and IC.slots(nkeys) == 2 * want >= 2 * nkeys
    for x in _values():
        l = IC.limbs30(x)
        assert hei.hei_hash(x & IC.M32, (x >> 32) & IC.M32) == IC.hash32(x & IC.M32, (x >> 32) & IC.M32)
        for ns in (4, 16, 1024, 1 << 21):
            assert hei.hei_home(l[0], l[1], l[2], ns - 1) == IC.home(x, ns), (hex(x), ns)
    assert IC.home((1 << 270) - 1, 16) == IC.home((1 << 64) - 1, 16)   # only bits 0..63 of x count
    b72 = (0x0123456789abcdef00112233).to_bytes(36, 'big') + bytes(36)
    assert IC.home_of_point(b72, 1 << 10) == IC.home(0x0123456789abcdef00112233, 1 << 10)


def test_vectors_of_the_program_are_the_python_values():
    src = open(SRC).read()
    rows = re.findall(r'^    \{(0x[0-9a-f]{8})u, (0x[0-9a-f]{8})u, (0x[0-9a-f]{8})u, (0x[0-9a-f]{8})u, (\d+)u, (\d+)u, (\d+)u\},$', src, re.M)
    assert len(rows) == 16
    for x, r in zip(_values()[:16], rows):
        l = IC.limbs30(x)
        assert [int(r[0], 16), int(r[1], 16), int(r[2], 16)] == l[:3]
        assert int(r[3], 16) == IC.hash32(x & IC.M32, (x >> 32) & IC.M32)
        assert [int(r[4]), int(r[5]), int(r[6])] == [IC.home(x, 4), IC.home(x, 16), IC.home(x, 1 << 21)]


def test_header_and_contract_state_the_slot_function():
    for path in (os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc', 'escrow_index.h'), os.path.join(ROOT, 'include', 'zkattest.h')):
        text = ' '.join(open(path).read().split())
        for part in ('h = w0 * 0x9e3779b1 + w1 * 0x85ebca6b', 'h ^= h >> 16', 'h *= 0xc2b2ae35', 'h ^= h >> 13', '0xffffffff'):
            assert part in text, (path, part)


def _point(rnd, slot, nslots, tag):
    """a synthetic point (x, y as integers below 2^270) whose home slot is `slot`"""
    while True:
        x = rnd.getrandbits(270)
        if slot is None or IC.home(x, nslots) == slot:
            return (x, (rnd.getrandbits(240) << 30) | tag)


def _run(hei, pts, nkeys, order, queries):
    """-> (slots, found) of the host build over pts[:entries] inserted in `order`"""
    cap = IC.entries(nkeys)
    assert len(pts) <= cap
    flat = [0] * (18 * cap)
    for i, (x, y) in enumerate(pts):
        for l, v in enumerate(IC.limbs30(x) + IC.limbs30(y)):
            flat[l * cap + i] = v
    q = []
    for x, y in queries:
        q += IC.limbs30(x) + IC.limbs30(y)
    slots, found = (C.c_uint32 * (2 * cap))(), (C.c_uint32 * max(len(queries), 1))()
    assert hei.hei_build_lookup((C.c_uint32 * len(flat))(*flat), nkeys, (C.c_uint32 * nkeys)(*order), slots, (C.c_uint32 * max(len(q), 1))(*q), len(queries), found) == 0
    return list(slots), list(found)[:len(queries)]


def _brute(pts, nkeys, q):
    return pts.index(q) if q in pts[:nkeys] else IC.EMPTY


def test_wrapping_cluster_equal_points_full_load_and_absent_points(hei):
    rnd = random.Random(77)
    # 8 keys, 16 slots: three distinct points and two copies at home slot 15, one point at 14, two elsewhere; the copies' lowest index is 1
    pts = [_point(rnd, 14, 16, 0), _point(rnd, 15, 16, 1), _point(rnd, 15, 16, 2), _point(rnd, 5, 16, 3), _point(rnd, 15, 16, 4)]
    pts += [pts[1], _point(rnd, 0, 16, 6), pts[1]]
    absent = [_point(rnd, 15, 16, 100), _point(rnd, 14, 16, 101), _point(rnd, 0, 16, 102), _point(rnd, 9, 16, 103)]
    tables = set()
    for k in range(40):
        order = list(range(8))
        random.Random(k).shuffle(order)
        slots, found = _run(hei, pts, 8, order, pts + absent)
        assert found == [_brute(pts, 8, q) for q in pts + absent] == [0, 1, 2, 3, 4, 1, 6, 1, IC.EMPTY, IC.EMPTY, IC.EMPTY, IC.EMPTY], order
        # the cluster wraps: 14, 15, 0, 1, 2 are taken (five points: homes 14, 15, 15, 15, 0), 3 is the empty slot an absent point at home 15 ends at
        assert all(slots[s] != IC.EMPTY for s in (14, 15, 0, 1, 2, 5)) and slots[3] == IC.EMPTY and sorted(s for s in slots if s != IC.EMPTY) == [0, 1, 2, 3, 4, 6]
        tables.add(tuple(slots))
    assert len(tables) > 1   # the table's bytes depend on the order of the insertions; no lookup result did
    # the fullest allowed load, every point at ONE home slot: nkeys = entries = 8, the cluster runs 13, 14, 15, 0 .. 4
    pts = [_point(rnd, 13, 16, i) for i in range(8)]
    slots, found = _run(hei, pts, 8, [7, 0, 6, 1, 5, 2, 4, 3], pts + [_point(rnd, 13, 16, 99), _point(rnd, 4, 16, 98), _point(rnd, 5, 16, 97)])
    assert found == list(range(8)) + [IC.EMPTY] * 3 and [s != IC.EMPTY for s in slots] == [True] * 5 + [False] * 8 + [True] * 3
    # 600 keys with repeats in 1024 entries against the brute-force scan
    pts = []
    for i in range(600):
        pts.append(pts[i - 50] if i % 7 == 3 and i > 50 else _point(rnd, None, 2048, i))
    order = [(7 * i + 3) % 600 for i in range(600)]
    queries = pts + [_point(rnd, None, 2048, 1000 + i) for i in range(100)]
    slots, found = _run(hei, pts, 600, order, queries)
    assert found == [_brute(pts, 600, q) for q in queries]
    assert sum(s != IC.EMPTY for s in slots) == len(set(pts))   # every distinct point owns exactly one slot


def test_program_of_its_own_under_the_sanitizers(tmp_path):
    exe = tmp_path / 'host_escrow_index'
    subprocess.check_call(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-DHOST_ESCROW_INDEX_MAIN'] + FLAGS + [SRC, '-o', str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and 'host_escrow_index: ok' in r.stdout, r.stdout + r.stderr
