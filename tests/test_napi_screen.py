"""-m gpu: the witness screen behind the N-API facade (bindings/napi/screen_check.js): screenSignatureLists finds the signer's index over several rings, flags a
wrong message, a foreign signature, an absent key and a wrong index, and exactly the statements it passes yield proofs that verifySignatureLists accepts."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAPI = os.path.join(ROOT, 'bindings', 'napi')


def _build(tmp_path):
    if not (shutil.which('node') and shutil.which('gcc') and os.path.exists('/usr/include/node/node_api.h')):
        pytest.skip('node / gcc / node_api.h not available')
    out = str(tmp_path / 'zkattest.node')
    subprocess.check_call(['make', '-s', '-C', NAPI, 'OUT=' + out])
    return out


@pytest.mark.gpu
def test_screen_signature_lists_from_javascript(tmp_path):
    out = _build(tmp_path)
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'screen_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'screen ok' in res.stdout, res.stdout + res.stderr
