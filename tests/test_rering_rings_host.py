"""csrc/rering_plan.h -- the plan of a mixed-ring re-ring call (every proof's class, status and slot from its header, its destination ring and its index;
the offsets of a batch whose heads differ in length; the offsets as the device derives them per census workgroup; the out_cap, in-place and overlap
decisions; the window cuts) -- as a stand-alone host program: tests/host_arith/host_rering_rings.cpp, built with plain g++ against a direct restatement,
over fixed shapes (empty classes, classes of one proof, unknown ids only, batches at the census workgroup's size and one either side, mixed secLevels) and
a seeded sweep of 200 mixes.  Once more, the same stand-alone binary, under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'host_arith', 'host_rering_rings.cpp')


def _run(tmp_path, name, *flags):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / name)
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', *flags, '-I' + CSRC, SRC, '-o', exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(res.stdout[-3000:])
    assert res.returncode == 0 and not res.stderr.strip(), res.stderr[-4000:]
    assert res.stdout.strip().endswith('rering rings plan ok')
    return res.stdout


def test_plan_agrees_with_the_restatement(tmp_path):
    out = _run(tmp_path, 'host_rering_rings', '-O1')
    for shape in ('census block edge, B = 255', 'census block edge, B = 256', 'census block edge, B = 257', 'unknown ids only', 'no resident ring', 'one class',
                  'mixed secLevels', 'in place, one proof of another n', 'refusals between good neighbours', 'sweep 199'):
        assert shape in out, shape


def test_plan_program_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(tmp_path, 'host_rering_rings_san', '-O0', '-fsanitize=address,undefined', '-fno-sanitize-recover=all')
