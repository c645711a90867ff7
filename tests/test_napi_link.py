"""Link proofs behind the N-API facade.  not-gpu: the facade exports proveSameKey / verifySameKey, their batched forms, keyCommitment and the LinkProof class, the
typings declare them, the addon registers its three entry points and compiles.  -m gpu: bindings/napi/link_check.js -- link proofs verify, forgeries and
other keys do not, the prover refuses an opening that does not hold, two attestations and a membership proof are tied together in both wire layouts."""
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
    for name in ('proveSameKey', 'verifySameKey', 'proveSameKeys', 'verifySameKeys', 'keyCommitment', 'keyCommitments', 'LinkProof'):
        assert re.search(r'\b%s\b' % name, exports), name
    assert re.search(r'async function proveSameKey\(params, key, comA, blinderA, comB, blinderB\)', js)
    assert re.search(r'async function verifySameKey\(params, comA, comB, link\)', js)
    assert re.search(r'async function keyCommitment\(proof\b', js) and re.search(r'class LinkProof\b', js)
    for m in ('linkProveBatch', 'linkVerifyBatch', 'keyCommitments'):
        assert re.search(r'^    %s\(' % m, js, re.M), m   # the Engine's methods
    assert os.path.exists(os.path.join(NAPI, 'link_check.js'))


def test_typings_declare_the_calls():
    dts = _read('zkattest.d.ts')
    for pat in (r'export function proveSameKey\(params: [^,]+, key: [^,]+, comA: [^,]+, blinderA: [^,]+, comB: [^,]+, blinderB: [^)]+\): Promise<LinkProof>',
                r'export function verifySameKey\(params: [^,]+, comA: [^,]+, comB: [^,]+, link: [^)]+\): Promise<boolean>',
                r'export function proveSameKeys\(', r'export function verifySameKeys\(', r'export function keyCommitment\(proof: [^)]+\): Promise<Point>',
                r'export function keyCommitments\(', r'export class LinkProof \{', r'    linkProveBatch\(', r'    linkVerifyBatch\(', r'    keyCommitments\('):
        assert re.search(pat, dts), pat


def test_addon_registers_the_entry_points():
    c = _read('zkattest_napi.c')
    for name, fn in (('linkProveBatch', 'zk_link_prove_batch'), ('linkVerifyBatch', 'zk_link_verify_batch'), ('keyCommitments', 'zk_proof_key_commitments')):
        assert re.search(r'\{"%s", \w+\}' % name, c), name
        assert re.search(r'\b%s\(' % fn, c), fn


def test_addon_compiles(tmp_path):
    out = _build(tmp_path)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_link_proofs_from_javascript(tmp_path):
    out = _build(tmp_path)
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'link_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'link ok' in res.stdout, res.stdout + res.stderr
