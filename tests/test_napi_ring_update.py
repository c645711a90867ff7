"""-m gpu: Engine.updateRing and the facade's ringDelta option from JavaScript (bindings/napi/ring_update_check.js): with ringDelta 16 two
verifySignatureList calls whose key lists differ in 2 entries leave one resident ring with its generation up by one; with ringDelta 0 they leave two."""
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
def test_update_ring_and_ring_delta_from_javascript(tmp_path):
    out = _build(tmp_path)
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'ring_update_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'ring update ok' in res.stdout, res.stdout + res.stderr
