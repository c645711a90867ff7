"""-m gpu: the exhaustive verify mode behind the N-API facade (bindings/napi/verify_reps_check.js): setVerifyReps('all') rejects a proof with one
broken repetition that the default 'sample' lets through when it does not draw it.  Skipped as tests/test_napi_binding.py skips."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAPI = os.path.join(ROOT, 'bindings', 'napi')


@pytest.mark.gpu
def test_set_verify_reps_from_javascript(tmp_path):
    if not (shutil.which('node') and shutil.which('gcc') and os.path.exists('/usr/include/node/node_api.h')):
        pytest.skip('node / gcc / node_api.h not available')
    out = str(tmp_path / 'zkattest.node')
    subprocess.check_call(['make', '-s', '-C', NAPI, 'OUT=' + out])
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'verify_reps_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert 'sample: a broken repetition passes' in res.stdout and 'all: rejected' in res.stdout, res.stdout
