"""not-gpu: the capacity rule of the quorum calls with one ring id per member (zkp-ecdsa_amd/csrc/quorum_plan.h: zkq_capacity_rings, zkq_max_size_rings) as a
program of its own (tests/host_arith/host_quorum_rings.cpp) under the address and undefined-behaviour sanitizers: k = 2 and 16, all ids equal, one id
missing, sums near 2^32 per slot, a full table.  The program is run directly, as a child process of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host_arith', 'host_quorum_rings.cpp')
FLAGS = ['-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-I' + os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')]

pytestmark = pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')


def test_capacity_rule_under_the_sanitizers(tmp_path):
    exe = tmp_path / 'host_quorum_rings'
    subprocess.check_call(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + FLAGS + [SRC, '-o', str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and 'host_quorum_rings: ok' in r.stdout, r.stdout + r.stderr
