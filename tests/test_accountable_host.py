"""not-gpu: the accountable attestations' plan (zkp-ecdsa_amd/csrc/accountable_plan.h) compiled for the host CPU as a program of its own
(tests/host_arith/host_accountable.cpp) under the address and undefined-behaviour sanitizers, against vectors written out of the Python statement
(tests/accountable_common.py): good bundles alone and between neighbours, every header error, a truncated slot, an inner total_len one word too long or too
short, a slot that ends inside the tag, join's two header checks, the sizes and the header words.  No sanitizer runs in anything loaded into Python."""
import os
import shutil
import subprocess

import pytest

import accountable_common as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host_arith', 'host_accountable.cpp')
FLAGS = ['-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-I' + os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')]

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')


def test_the_python_statement_checks_itself():
    assert AC.self_check(0) and AC.self_check(1)
    assert AC.header(0x01020304) == b'ZKC1' + bytes([1, 2, 3, 4]) + bytes(8)


def _vectors():
    rows = []
    hx = lambda b: b.hex() if b else '-'

    def walk_row(packed, blob, o0, o1):
        w = AC.walk(blob, o0, o1, packed)
        rows.append('W %d %d %d %d %d %d %s' % (packed, 1 if w else 0, o0, o1, w[0] if w else 0, w[1] if w else 0, hx(blob)))
        return w

    for packed in (0, 1):
        n = 3
        m = AC.FIXED[packed] + AC.GK_N[packed] * n + 32
        atts = [AC.fake_proof(m + 8 * i, packed, n) for i in range(3)]
        tags = [AC.fake_tag(0x40 + i) for i in range(3)]
        good = [AC.bundle(a, t) for a, t in zip(atts, tags)]
        blob = b''.join(good)
        # good bundles: alone (the slot ends where the allocation ends) and between neighbours
        for g in good:
            assert walk_row(packed, g, 0, len(g))
        o = len(good[0])
        assert walk_row(packed, blob, o, o + len(good[1])) == (o + 16, o + len(good[1]) - AC.TAG)
        assert walk_row(packed, blob, o + len(good[1]), len(blob))
        # the other layout; offsets that are not aligned or do not ascend; a slot that takes a neighbour's bytes
        assert not walk_row(1 - packed, good[0], 0, len(good[0]))
        for o0, o1 in ((2, len(good[0]) + 2), (o, 0), (0, o + 4), (4, o), (0, 0), (o, o)):
            assert not walk_row(packed, blob, o0, o1)
        # every way the statement lists, each in an allocation of exactly the slot
        for name, v in AC.bad_vectors(good[1], len(atts[1])):
            assert not walk_row(packed, v, 0, len(v)), name
        # the shortest attestation rr_head accepts for n, and one word less; n above 63
        assert walk_row(packed, AC.bundle(AC.fake_proof(m, packed, n), tags[0]), 0, AC.size(m))
        assert not walk_row(packed, AC.bundle(AC.fake_proof(m - 4, packed, n), tags[0]), 0, AC.size(m - 4))
        big = AC.FIXED[packed] + AC.GK_N[packed] * 64 + 32
        assert not walk_row(packed, AC.bundle(AC.fake_proof(big, packed, 64), tags[0]), 0, AC.size(big))
        # join: the proof's header and the tag's 16 header bytes
        bad_tags = [b'ZKT2' + tags[0][4:], AC.put32(tags[0], 4, 468), AC.put32(tags[0], 8, 1), AC.put32(tags[0], 12, 1)]
        cases = [(atts[0], tags[0]), (atts[2], tags[1])] + [(atts[0], t) for t in bad_tags]
        cases += [(atts[1][:-4], tags[0]), (AC.put32(atts[1], 4, len(atts[1]) + 4), tags[0]), (AC.fake_proof(m, 1 - packed, n), tags[0]), (atts[0][:16], tags[0]), (b'', tags[0])]
        for p, t in cases:
            out, _ = AC.join([p], [t], packed)
            rows.append('J %d %d %s %s' % (packed, len(out[0]) if out[0] else 0, hx(p), hx(t)))
        assert [r.split()[2] != '0' for r in rows[-len(cases):]] == [True, True] + [False] * (len(cases) - 2)
    for proof_max, att in ((0, 0), (1000, 996), (75000, 12344)):
        rows.append('S %d %d %d %d %s' % (proof_max, AC.max_size(proof_max), att, AC.size(att), AC.header(AC.size(att)).hex()))
    return rows


def test_program_of_its_own_under_the_sanitizers(tmp_path):
    exe, vec = tmp_path / 'host_accountable', tmp_path / 'vectors.txt'
    vec.write_text('\n'.join(_vectors()) + '\n')
    subprocess.check_call(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + FLAGS + [SRC, '-o', str(exe)])
    r = subprocess.run([str(exe), str(vec)], capture_output=True, text=True)
    assert r.returncode == 0 and 'host_accountable: ok' in r.stdout, r.stdout + r.stderr
