"""csrc/gk_plan.h (the ring fold's geometry: tile exponents, tile counts, finish groups and the element counts of gk_bufA, gk_bufB, res and res2) as a
stand-alone host program: tests/host_arith/host_gk_plan.cpp, built with plain g++ -- the header includes nothing of HIP.  For n in {1, 2, 3, 4, 5, 8, 9, 12,
13, 16, 20, 21}, with and without table E where n allows one, and chunks of 1, 15, 16, 17 and 4096 proofs: every plan value equals the expression the
carvers spelled out before the header existed, and a walk of the prover's and the verifier's launch loops keeps every pass inside the planned buffers -- the
verifier's also where a ring in the table's range has no table (sized as an upper bound).  Once more under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'host_arith', 'host_gk_plan.cpp')


def _run(tmp_path, name, *flags):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / name)
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', *flags, '-I' + CSRC, SRC, '-o', exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0 and not res.stderr.strip(), res.stderr[-4000:]
    assert res.stdout.strip().endswith('gk plan ok')
    return res.stdout


def test_plans_equal_the_old_expressions_and_every_pass_fits_its_buffer(tmp_path):
    out = _run(tmp_path, 'host_gk_plan', '-O1')
    assert '85 shapes' in out   # 12 values of n x 5 chunk sizes, the 5 values of n in the table's range twice


def test_gk_plan_program_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(tmp_path, 'host_gk_plan_san', '-O0', '-fsanitize=address,undefined', '-fno-sanitize-recover=all')
