"""Quorum proofs behind the N-API facade.  not-gpu: the facade exports proveQuorum / verifyQuorum and the QuorumProof class, the typings declare them, the addon
registers its two entry points and compiles.  -m gpu: bindings/napi/quorum_check.js -- a proveQuorum -> verifyQuorum round trip, a repeated signer throws, a
tampered bundle gives false."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAPI = os.path.join(ROOT, 'bindings', 'napi')


def _read(name):
    return open(os.path.join(NAPI, name)).read()


def _build(tmp_path):
    if not (shutil.which('node') and shutil.which('gcc') and os.path.exists('/usr/include/node/node_api.h')):
        pytest.skip('node / gcc / node_api.h not available')
    out = str(tmp_path / 'zkattest.node')
    subprocess.check_call(['make', '-s', '-C', NAPI, 'OUT=' + out])
    return out


def test_facade_exports_and_signatures():
    js = _read('zkattest.js')
    exports = js[js.rindex('module.exports'):]
    for name in ('proveQuorum', 'verifyQuorum', 'QuorumProof'):
        assert re.search(r'\b%s\b' % name, exports), name
    assert re.search(r'async function proveQuorum\(params, msgHashes, sigs, publicKeys, whichs, keys\)', js)
    assert re.search(r'async function verifyQuorum\(params, msgHashes, keys, proof\)', js)
    assert re.search(r'class QuorumProof\b', js)
    for m in ('quorumProveBatch', 'quorumVerifyBatch'):
        assert re.search(r'^    %s\(' % m, js, re.M), m   # the Engine's methods
    assert os.path.exists(os.path.join(NAPI, 'quorum_check.js'))


def test_typings_declare_the_calls():
    dts = _read('zkattest.d.ts')
    for pat in (r'export function proveQuorum\(params: [^,]+, msgHashes: [^,]+, sigs: [^,]+, publicKeys: [^,]+, whichs: [^,]+, keys: [^)]+\): Promise<QuorumProof>',
                r'export function verifyQuorum\(params: [^,]+, msgHashes: [^,]+, keys: [^,]+, proof: [^)]+\): Promise<boolean>',
                r'export class QuorumProof \{', r'    quorumProveBatch\(', r'    quorumVerifyBatch\('):
        assert re.search(pat, dts), pat


def test_addon_registers_the_entry_points():
    c = _read('zkattest_napi.c')
    for name, fn in (('quorumProveBatch', 'zk_quorum_prove_batch'), ('quorumVerifyBatch', 'zk_quorum_verify_batch')):
        assert re.search(r'\{"%s", \w+\}' % name, c), name
        assert re.search(r'\b%s\(' % fn, c), fn


def test_addon_compiles(tmp_path):
    out = _build(tmp_path)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_quorum_proofs_from_javascript(tmp_path):
    out = _build(tmp_path)
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'quorum_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'quorum ok' in res.stdout, res.stdout + res.stderr
