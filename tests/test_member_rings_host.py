"""csrc/member_plan.h -- the index arithmetic of the mixed-ring membership calls (sizes per class, the offsets of a batch with ids that are not resident,
the offsets as the device derives them per census workgroup, the window cuts, the out_cap decision, the verifier's slot rule) -- as a stand-alone host
program: tests/host_arith/host_member_rings.cpp, built with plain g++ against a direct restatement, over fixed shapes (empty classes, classes of one proof,
batches at the census workgroup's size and one either side) and a seeded sweep of 200 class mixes.  Once more under the address and undefined-behaviour
sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'host_arith', 'host_member_rings.cpp')


def _run(tmp_path, name, *flags):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / name)
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', *flags, '-I' + CSRC, SRC, '-o', exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(res.stdout[-3000:])
    assert res.returncode == 0 and not res.stderr.strip(), res.stderr[-4000:]
    assert res.stdout.strip().endswith('member rings plan ok')
    return res.stdout


def test_plan_agrees_with_the_restatement(tmp_path):
    out = _run(tmp_path, 'host_member_rings', '-O1')
    assert 'census block edge, B = 257' in out and 'unknown ids only' in out and 'sweep 199' in out


def test_plan_program_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(tmp_path, 'host_member_rings_san', '-O0', '-fsanitize=address,undefined', '-fno-sanitize-recover=all')
