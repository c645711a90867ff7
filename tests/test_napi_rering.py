"""Re-ring behind the N-API facade.  not-gpu: reringSignatureLists and keyBlinders are exported with the issue's parameter lists, reach the addon's two entry
points, which call the C ABI's host forms; the typings declare them; the addon compiles.  -m gpu: bindings/napi/rering_check.js -- proofs moved to a larger
key list and to a rotated one verify there and nowhere else, heads unchanged, both wire layouts, the refusals."""
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


def test_facade_exports_the_calls():
    js = _read('zkattest.js')
    assert re.search(r'async function reringSignatureLists\(params, msgHashes, proofs, whichNew, keyBlinders, keys\)', js)
    assert re.search(r'async function keyBlinders\(seeds, params = lastParams\)', js)
    exports = js[js.index('module.exports'):]
    assert 'reringSignatureLists' in exports and 'keyBlinders' in exports
    assert re.search(r'native\.reringBatch\(', js) and re.search(r'native\.keyBlinders\(', js)
    assert 'crypto.randomBytes(32 * B))' in js[js.index('reringBatch(msg, proofs, whichNew'):][:900]   # fresh seeds by default
    assert os.path.exists(os.path.join(NAPI, 'rering_check.js'))


def test_typings_declare_the_calls():
    dts = _read('zkattest.d.ts')
    assert re.search(r'export function reringSignatureLists\(params: SystemParametersList, msgHashes: Uint8Array\[\], proofs: [^\n]*, whichNew: number\[\], keyBlinders: Uint8Array\[\], keys: bigint\[\] \| Buffer\): Promise<SignatureProofList\[\]>', dts)
    assert re.search(r'export function keyBlinders\(seeds: [^\n]*\): Promise<Buffer\[\]>', dts)
    assert 'intersection' in dts


def test_addon_registers_the_entry_points():
    c = _read('zkattest_napi.c')
    for name, fn in (('keyBlinders', 'zk_prove_key_blinders'), ('reringBatch', 'zk_proof_rering_batch')):
        assert re.search(r'\{"%s", +\w+\}' % name, c), name
        assert re.search(r'\b%s\(' % fn, c), fn


def test_addon_compiles(tmp_path):
    out = _build(tmp_path)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_rering_from_javascript(tmp_path):
    out = _build(tmp_path)
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'rering_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'rering ok' in res.stdout, res.stdout + res.stderr
