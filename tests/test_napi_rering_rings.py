"""Re-ring with one key list per proof behind the N-API facade.  not-gpu: reringSignatureLists keeps its parameter list and takes an array of key lists in the
place of `keys`, reaches Engine.reringBatchRings and the addon's reringBatchRings, which calls the C ABI's host form; the typings declare both; the addon
compiles.  -m gpu: bindings/napi/rering_rings_check.js -- three proofs moved to three lists in one call verify under their own lists only, heads unchanged,
both wire layouts, the refusals."""
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


def test_facade_takes_one_key_list_per_proof():
    js = _read('zkattest.js')
    assert re.search(r'async function reringSignatureLists\(params, msgHashes, proofs, whichNew, keyBlinders, keys\)', js)   # the same six parameters
    body = js[js.index('async function reringSignatureLists('):][:2500]
    assert 'if (isKeyLists(keys)) return reringToLists(' in body
    lists = js[js.index('async function reringToLists('):][:2500]
    assert 'ringOf(keys)' in lists and 'withRings(' in lists and 'engine.reringBatchRings(' in lists   # rings named and made resident as proveSignatureLists does
    eng = js[js.index('    reringBatchRings(msg, proofs, whichNew, ringIds, blinders, seeds) {'):][:900]
    assert 'native.reringBatchRings(' in eng and 'crypto.randomBytes(32 * B))' in eng                   # fresh seeds by default
    assert os.path.exists(os.path.join(NAPI, 'rering_rings_check.js'))


def test_typings_declare_the_calls():
    dts = _read('zkattest.d.ts')
    assert re.search(r'export function reringSignatureLists\(params: SystemParametersList, msgHashes: Uint8Array\[\], proofs: [^\n]*, whichNew: number\[\], keyBlinders: Uint8Array\[\], keyLists: \(bigint\[\] \| Buffer\)\[\]\): Promise<SignatureProofList\[\]>', dts)
    assert re.search(r'reringBatchRings\(msg: Buffer, proofs: Buffer\[\], whichNew: [^\n]*, ringIds: [^\n]*, blinders: Buffer, seeds\?: Buffer\)', dts)


def test_addon_registers_the_entry_point():
    c = _read('zkattest_napi.c')
    assert re.search(r'\{"reringBatchRings", +ReringBatchRings\}', c)
    assert re.search(r'\bzk_proof_rering_batch_rings\(c, B, msg, blob, off, which, ids, bl, &rng, out, cap, out_off, status\)', c)


def test_addon_compiles(tmp_path):
    out = _build(tmp_path)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_rering_rings_from_javascript(tmp_path):
    out = _build(tmp_path)
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'rering_rings_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'rering rings ok' in res.stdout, res.stdout + res.stderr
