"""Ring membership on its own behind the N-API facade.  not-gpu: the facade exports proveMembership / verifyMembership with the reference's signatures, their batched
forms and the GKProof / Commitment classes, the typings declare them, the addon registers its three entry points and compiles.  -m gpu:
bindings/napi/member_check.js -- proofs verify, forgeries do not, the prover refuses a commitment that does not open to keys[index]."""
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
    for name in ('proveMembership', 'verifyMembership', 'proveMemberships', 'verifyMemberships', 'GKProof', 'Commitment', 'commit'):
        assert re.search(r'\b%s\b' % name, exports), name
    # the reference's argument lists (src/proofGK/gk.ts:94, 197)
    assert re.search(r'async function proveMembership\(pedersenParams, com, index, keys\)', js)
    assert re.search(r'async function verifyMembership\(pedersenParams, comPoint, keys, proof\)', js)
    assert re.search(r'class GKProof\b', js) and re.search(r'class Commitment\b', js)
    assert 'does not commit to keys[index]' in js   # the facade checks the engine's commitment against com.p
    assert os.path.exists(os.path.join(NAPI, 'member_check.js'))


def test_typings_declare_the_calls():
    dts = _read('zkattest.d.ts')
    for pat in (r'export function proveMembership\(params: [^,]+, com: Commitment, index: number, keys: [^)]+\): Promise<GKProof>',
                r'export function verifyMembership\(params: [^,]+, com: Point, keys: [^)]+, proof: GKProof\): Promise<boolean>',
                r'export function proveMemberships\(', r'export function verifyMemberships\(', r'export class GKProof \{', r'export class Commitment \{',
                r'export function commit\('):
        assert re.search(pat, dts), pat


def test_addon_registers_the_entry_points():
    c = _read('zkattest_napi.c')
    for name, fn in (('memberProofSize', 'zk_member_proof_size'), ('memberProveBatch', 'zk_member_prove_batch'), ('memberVerifyBatch', 'zk_member_verify_batch')):
        assert re.search(r'\{"%s", \w+\}' % name, c), name
        assert re.search(r'\b%s\(' % fn, c), fn


def test_addon_compiles(tmp_path):
    out = _build(tmp_path)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_membership_from_javascript(tmp_path):
    out = _build(tmp_path)
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'member_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'member ok' in res.stdout, res.stdout + res.stderr
