"""Accountable attestations behind the N-API facade.  not-gpu: the facade exports proveAccountable(s) / verifyAccountable(s) / splitAccountable / joinAccountable and
the AccountableProof class, the typings declare them, the addon registers its four entry points and compiles.  -m gpu: bindings/napi/accountable_check.js -- a
prove -> verify round trip in both wire layouts, the parts pass the existing verifiers, swapped tags and a tampered tag give false, split and join are inverse,
the split tags open to the signers."""
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
    for name in ('proveAccountable', 'proveAccountables', 'verifyAccountable', 'verifyAccountables', 'splitAccountable', 'joinAccountable', 'AccountableProof'):
        assert re.search(r'\b%s\b' % name, exports), name
    assert re.search(r'async function proveAccountables\(params, auditor, msgHashes, sigs, publicKeys, whichs, keys\)', js)
    assert re.search(r'async function proveAccountable\(params, auditor, msgHash, sig, publicKey, which, keys\)', js)
    assert re.search(r'async function verifyAccountables\(params, auditor, msgHashes, keys, proofs\)', js)
    assert re.search(r'async function verifyAccountable\(params, auditor, msgHash, keys, proof\)', js)
    assert re.search(r'async function splitAccountable\(params, proofs\)', js)
    assert re.search(r'async function joinAccountable\(params, attestations, tags\)', js)
    assert re.search(r'class AccountableProof\b', js)
    for m in ('accountableProveBatch', 'accountableVerifyBatch', 'accountableSplitBatch', 'accountableJoinBatch'):
        assert re.search(r'^    %s\(' % m, js, re.M), m   # the Engine's methods
    assert os.path.exists(os.path.join(NAPI, 'accountable_check.js'))


def test_typings_declare_the_calls():
    dts = _read('zkattest.d.ts')
    for pat in (r'export function proveAccountable\(params: [^,]+, auditor: [^,]+, msgHash: [^,]+, sig: [^,]+, publicKey: [^,]+, which: [^,]+, keys: [^)]+\): Promise<AccountableProof>',
                r'export function proveAccountables\(params: [^,]+, auditor: [^,]+, msgHashes: [^,]+, sigs: [^,]+, publicKeys: [^,]+, whichs: [^,]+, keys: [^)]+\): Promise<AccountableProof\[\]>',
                r'export function verifyAccountable\(params: [^,]+, auditor: [^,]+, msgHash: [^,]+, keys: [^,]+, proof: [^)]+\): Promise<boolean>',
                r'export function verifyAccountables\(params: [^,]+, auditor: [^,]+, msgHashes: [^,]+, keys: [^,]+, proofs: .+\): Promise<boolean\[\]>',
                r'export function splitAccountable\(', r'export function joinAccountable\(', r'export class AccountableProof \{',
                r'    accountableProveBatch\(', r'    accountableVerifyBatch\(', r'    accountableSplitBatch\(', r'    accountableJoinBatch\('):
        assert re.search(pat, dts), pat


def test_addon_registers_the_entry_points():
    c = _read('zkattest_napi.c')
    for name, fn in (('accountableProveBatch', 'zk_accountable_prove_batch'), ('accountableVerifyBatch', 'zk_accountable_verify_batch'),
                     ('accountableSplitBatch', 'zk_accountable_split_batch'), ('accountableJoinBatch', 'zk_accountable_join_batch')):
        assert re.search(r'\{"%s", \w+\}' % name, c), name
        assert re.search(r'\b%s\(' % fn, c), fn


def test_addon_compiles(tmp_path):
    out = _build(tmp_path)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_accountable_attestations_from_javascript(tmp_path):
    out = _build(tmp_path)
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'accountable_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'accountable ok' in res.stdout, res.stdout + res.stderr
