"""Quorum proofs over several rings behind the N-API facade.  not-gpu: the Engine has ringsQuorumProveBatch / ringsQuorumVerifyBatch, the typings declare them and
the key-lists form of `keys`, the addon registers its two entry points and compiles.  -m gpu: bindings/napi/quorum_rings_check.js -- proveQuorum ->
verifyQuorum with one key list per member over two registries, the same key through both registries throws, the wrong registry gives false."""
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


def test_facade_and_engine_methods():
    js = _read('zkattest.js')
    assert re.search(r'^    ringsQuorumProveBatch\(k, msg, sig, pk, whichs, ringIds, seeds, pairSeeds\)', js, re.M)
    assert re.search(r'^    ringsQuorumVerifyBatch\(k, msg, bundles, ringIds\)', js, re.M)
    for fn in ('proveQuorum', 'verifyQuorum'):
        body = js[js.index('async function %s(' % fn):]
        body = body[:body.index('\n}\n')]
        assert 'isKeyLists(keys)' in body and 'withRings(' in body and 'ringsQuorum%sBatch(' % ('Prove' if fn == 'proveQuorum' else 'Verify') in body, fn
    assert os.path.exists(os.path.join(NAPI, 'quorum_rings_check.js'))


def test_typings_declare_the_calls():
    dts = _read('zkattest.d.ts')
    for pat in (r'    ringsQuorumProveBatch\(k: number, msg: Buffer, sig: Buffer, pk: Buffer, whichs: number\[\], ringIds: number\[\], seeds\?: Buffer, pairSeeds\?: Buffer\)',
                r'    ringsQuorumVerifyBatch\(k: number, msg: Buffer, bundles: Buffer\[\], ringIds: number\[\]\)',
                r'export type QuorumKeys = bigint\[\] \| Buffer \| Array<bigint\[\] \| Buffer>',
                r'export function proveQuorum\([^)]*keys: QuorumKeys\)', r'export function verifyQuorum\([^)]*keys: QuorumKeys, proof:'):
        assert re.search(pat, dts), pat


def test_addon_registers_the_entry_points():
    c = _read('zkattest_napi.c')
    for name, fn in (('ringsQuorumProveBatch', 'zk_rings_quorum_prove_batch'), ('ringsQuorumVerifyBatch', 'zk_rings_quorum_verify_batch')):
        assert re.search(r'\{"%s", \w+\}' % name, c), name
        assert re.search(r'\b%s\(' % fn, c), fn


def test_addon_compiles(tmp_path):
    out = _build(tmp_path)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_quorum_proofs_over_two_registries_from_javascript(tmp_path):
    out = _build(tmp_path)
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'quorum_rings_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'quorum rings ok' in res.stdout, res.stdout + res.stderr
