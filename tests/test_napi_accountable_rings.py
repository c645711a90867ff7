"""Accountable attestations over several rings behind the N-API facade.  not-gpu: the Engine has accountableProveBatchRings / accountableVerifyBatchRings /
accountableOpenBatchRings, the typings declare them and the key-lists form of `keys`, the addon registers its three entry points and compiles.  -m gpu:
bindings/napi/accountable_rings_check.js -- proveAccountables -> verifyAccountables -> openAccountables with one key list per proof over two registries."""
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
    assert re.search(r'^    accountableProveBatchRings\(msg, sig, pk, whichs, ringIds, seeds, tagSeeds\)', js, re.M)
    assert re.search(r'^    accountableVerifyBatchRings\(msg, bundles, ringIds\)', js, re.M)
    assert re.search(r'^    accountableOpenBatchRings\(secret32, bundles, ringIds\)', js, re.M)
    for fn, call in (('proveAccountables', 'accountableProveBatchRings('), ('verifyAccountables', 'accountableVerifyBatchRings('),
                     ('openAccountables', 'accountableOpenBatchRings(')):
        body = js[js.index('async function %s(' % fn):]
        body = body[:body.index('\n}\n')]
        assert 'isKeyLists(' in body and 'accountableGroups(' in body and call in body, fn
    assert 'openAccountables' in js[js.index('module.exports'):]
    assert os.path.exists(os.path.join(NAPI, 'accountable_rings_check.js'))


def test_typings_declare_the_calls():
    dts = _read('zkattest.d.ts')
    for pat in (r'    accountableProveBatchRings\(msg: Buffer, sig: Buffer, pk: Buffer, whichs: number\[\], ringIds: number\[\], seeds\?: Buffer, tagSeeds\?: Buffer\)',
                r'    accountableVerifyBatchRings\(msg: Buffer, bundles: Buffer\[\], ringIds: number\[\]\)',
                r'    accountableOpenBatchRings\(secret32: Uint8Array, bundles: Buffer\[\], ringIds: number\[\]\)',
                r'export type AccountableKeys = bigint\[\] \| Buffer \| Array<bigint\[\] \| Buffer>',
                r'export function proveAccountable\([^)]*keys: AccountableKeys\)', r'export function proveAccountables\([^)]*keys: AccountableKeys\)',
                r'export function verifyAccountable\([^)]*keys: AccountableKeys, proof:', r'export function verifyAccountables\([^)]*keys: AccountableKeys, proofs:',
                r'export function openAccountables\([^)]*keyLists: Array<bigint\[\] \| Buffer>, proofs:'):
        assert re.search(pat, dts), pat


def test_addon_registers_the_entry_points():
    c = _read('zkattest_napi.c')
    for name, fn in (('accountableProveBatchRings', 'zk_rings_accountable_prove_batch'), ('accountableVerifyBatchRings', 'zk_rings_accountable_verify_batch'),
                     ('accountableOpenBatchRings', 'zk_rings_accountable_open_batch')):
        assert re.search(r'\{"%s", \w+\}' % name, c), name
        assert re.search(r'\b%s\(' % fn, c), fn


def test_addon_compiles(tmp_path):
    out = _build(tmp_path)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_accountable_attestations_over_two_registries_from_javascript(tmp_path):
    out = _build(tmp_path)
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'accountable_rings_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'accountable rings ok' in res.stdout, res.stdout + res.stderr
