"""not-gpu: the capacity rule of the accountable attestations over several rings (zkp-ecdsa_amd/csrc/accountable_plan.h: zkc_capacity_rings and the sums over it)
compiled for the host CPU as a program of its own (tests/host_arith/host_accountable_rings.cpp) under the address and undefined-behaviour sanitizers, against
a plain Python restatement: ids that are not resident contribute 0, a table of 16 rings, sums near 2^64 that must not wrap silently, random id lists.  No
sanitizer runs in anything loaded into Python."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host_arith', 'host_accountable_rings.cpp')
FLAGS = ['-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-I' + os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')]
TOP = (1 << 64) - 1
HDR, TAG = 16, 472

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')


# ------------------------------------------------------------------ the restatement: a table is a list of (id, resident, proof_max)
def max_size(table, ring_id):
    """zk_rings_accountable_proof_max_size: the first resident entry of that id; 0 where there is none or its proof_max is 0"""
    for i, res, pm in table:
        if res and i == ring_id:
            return HDR + pm + TAG if pm else 0
    return 0


def entry(table, ring_id):
    for r, (i, res, pm) in enumerate(table):
        if res and i == ring_id:
            return r if pm else None
    return None


def total(table, ids):
    t, used = 0, 0
    for i in ids:
        t = min(TOP, t + max_size(table, i))
        if entry(table, i) is not None:
            used |= 1 << entry(table, i)
    return t, used


def fits(table, n):
    most = max([max_size(table, i) for i, res, _ in table if res] + [0])
    return 1 if most == 0 or n * most <= TOP else 0


def _vectors():
    rows = []
    rnd = random.Random(20261021)

    def table(t):
        rows.append('T %d %s' % (len(t), ' '.join('%d %d %d' % e for e in t)))

    def sum_row(t, ids):
        tot, used = total(t, ids)
        rows.append('C %d %d %d %d %s' % (tot, used, fits(t, len(ids)), len(ids), ' '.join(map(str, ids))))
        return tot, used

    # two rings, as the GPU tests have them; an id that is not resident, an entry that is not resident, an entry without params
    t = [(1, 1, 3000), (2, 1, 5400), (3, 0, 7000), (4, 1, 0)]
    table(t)
    for i, want in ((1, 3488), (2, 5888), (3, 0), (4, 0), (999, 0), (0, 0), (0xFFFFFFFF, 0)):
        assert max_size(t, i) == want
        rows.append('M %d %d' % (i, want))
    assert sum_row(t, []) == (0, 0)
    assert sum_row(t, [1, 2, 1, 2, 1]) == (3 * 3488 + 2 * 5888, 3)
    assert sum_row(t, [1, 1, 1, 1]) == (4 * 3488, 1)          # one ring named: the set says so (staging follows the largest ring NAMED)
    assert sum_row(t, [999, 3, 4]) == (0, 0)                  # nothing resident: nothing to stage
    assert sum_row(t, [2, 999, 2, 3, 1, 4]) == (2 * 5888 + 3488, 3)
    # 16 rings, every one named; ids that repeat: the first resident entry answers
    t16 = [(100 + r, 1, 1000 + 4 * r) for r in range(16)]
    table(t16)
    assert sum_row(t16, [100 + r for r in range(16)]) == (sum(1488 + 4 * r for r in range(16)), 0xFFFF)
    assert sum_row(t16, [115] * 3 + [100]) == (3 * 1548 + 1488, 0x8001)
    dup = [(7, 0, 10), (7, 1, 20), (7, 1, 40)]
    table(dup)
    assert sum_row(dup, [7, 7]) == (2 * 508, 2)
    # sums near 2^64: the largest proof a u32 holds, so that 2^32 - 1 slots pass 2^64
    big = [(1, 1, 0xFFFFFFFF), (2, 1, 4)]
    table(big)
    slot = HDR + 0xFFFFFFFF + TAG
    assert sum_row(big, [1] * 5 + [2]) == (5 * slot + 492, 3)
    for n in (0, 1, 1 << 31, TOP // slot, TOP // slot + 1, 0xFFFFFFFF, TOP):
        rows.append('F %d %d' % (n, fits(big, n)))
    assert fits(big, TOP // slot) == 1 and fits(big, TOP // slot + 1) == 0 and fits(big, 0xFFFFFFFF) == 0
    table([(1, 0, 0xFFFFFFFF)])
    rows.append('F %d 1' % TOP)   # nothing resident: every sum is 0
    for a, b in ((0, 0), (1, 2), (TOP, 0), (TOP, 1), (TOP - 5, 5), (TOP - 5, 6), (TOP, TOP), (1 << 63, 1 << 63), ((1 << 63) - 1, 1 << 63), (slot * (TOP // slot), slot)):
        rows.append('A %d %d %d' % (a, b, min(TOP, a + b)))
    # random tables and id lists
    for _ in range(40):
        n = rnd.randrange(1, 17)
        t = [(rnd.randrange(0, 24), rnd.randrange(0, 4) != 0, rnd.choice([0, 4 * rnd.randrange(1, 1 << 20), 0xFFFFFFFC])) for _ in range(n)]
        t = [(i, int(res), pm) for i, res, pm in t]
        table(t)
        for _ in range(4):
            sum_row(t, [rnd.randrange(0, 26) for _ in range(rnd.randrange(0, 70))])
    return rows


def test_program_of_its_own_under_the_sanitizers(tmp_path):
    exe, vec = tmp_path / 'host_accountable_rings', tmp_path / 'vectors.txt'
    rows = _vectors()
    assert sum(r[0] == 'C' for r in rows) > 160 and any(r.startswith('F') and r.endswith(' 0') for r in rows)
    vec.write_text('\n'.join(rows) + '\n')
    subprocess.check_call(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + FLAGS + [SRC, '-o', str(exe)])
    r = subprocess.run([str(exe), str(vec)], capture_output=True, text=True)
    assert r.returncode == 0 and 'host_accountable_rings: ok' in r.stdout, r.stdout + r.stderr
