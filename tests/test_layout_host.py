"""csrc/layout.h (Carver::take and the two-pass helper lay_out, under every layout of the host layer's device buffers) as a stand-alone host program:
tests/host_arith/host_layout.cpp, built with plain g++ -- the header includes nothing of HIP.  Layouts of the host layer's shapes, zero-length regions and
sizes off the 256-byte grid: the size pass gives the real pass's total, every region starts on a multiple of 256 from the base, regions do not overlap, the
last one ends inside what was reserved; a failed reservation comes back as the caller's error.  Once more under the address and undefined-behaviour
sanitizers, with every region written end to end in a heap block of exactly the reserved size."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'host_arith', 'host_layout.cpp')


def _run(tmp_path, name, *flags):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / name)
    subprocess.check_call(['g++', '-std=c++17', '-Wall', '-Werror', *flags, '-I' + CSRC, SRC, '-o', exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(res.stdout)
    assert res.returncode == 0 and not res.stderr.strip(), res.stderr[-4000:]
    assert res.stdout.strip().endswith('layout ok')
    return res.stdout


def test_layout_passes_agree_and_regions_are_aligned_disjoint_and_inside(tmp_path):
    out = _run(tmp_path, 'host_layout', '-O1')
    assert 'zero-length regions' in out and 'census of 1000' in out


def test_layout_program_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _run(tmp_path, 'host_layout_san', '-O0', '-fsanitize=address,undefined', '-fno-sanitize-recover=all')
