"""-m gpu: after zk_ctx_update_ring every TABLE of the ring equals the one a full build makes (tests/ring_update_checksum_check.py, run in a child process on
the test-hooks build: zk_test_ring_checksum exists only there)."""
import os

import pytest

pytestmark = pytest.mark.gpu


def test_every_table_of_an_updated_ring_equals_the_full_build():
    import subprocess
    import sys
    import zkp_ecdsa_amd as Z
    th = os.path.join(os.path.dirname(Z.LIB_PATH), 'libzkattest_hip_testhooks.so')
    if not os.path.exists(th):
        pytest.skip('the test-hooks build is not there (make -C zkp-ecdsa_amd/csrc testhooks)')
    assert not hasattr(Z.lib(), 'zk_test_ring_checksum')   # the product library does not export the hook
    env = dict(os.environ)
    env['ZKATTEST_LIB'] = th
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, 'tests', 'ring_update_checksum_check.py')], env=env, capture_output=True, text=True, timeout=600)
    print(res.stdout[-6000:])
    assert res.returncode == 0 and 'ring_update_checksum_check ok' in res.stdout, res.stdout[-3000:] + res.stderr[-3000:]
