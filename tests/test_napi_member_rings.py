"""Membership proofs with one key list per entry behind the N-API facade.  not-gpu: the facade exports proveMembershipLists / verifyMembershipLists, the typings
declare them, the addon registers its three entry points and compiles.  -m gpu: bindings/napi/member_rings_check.js -- proofs over interleaved key lists verify
under their own list and under no other, the one-list calls agree, the prover refuses a commitment that does not open to its list's keys[index]."""
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
    for name in ('proveMembershipLists', 'verifyMembershipLists'):
        assert re.search(r'\b%s\b' % name, exports), name
    assert re.search(r'async function proveMembershipLists\(pedersenParams, coms, indices, keysList\)', js)
    assert re.search(r'async function verifyMembershipLists\(pedersenParams, comPoints, keysList, proofs\)', js)
    assert os.path.exists(os.path.join(NAPI, 'member_rings_check.js'))


def test_typings_declare_the_calls():
    dts = _read('zkattest.d.ts')
    for pat in (r'export function proveMembershipLists\(params: [^,]+, coms: Commitment\[\], indices: number\[\], keysList: [^:]+\): Promise<GKProof\[\]>',
                r'export function verifyMembershipLists\(params: [^,]+, coms: Point\[\], keysList: [^:]+, proofs: GKProof\[\]\): Promise<boolean\[\]>'):
        assert re.search(pat, dts), pat


def test_addon_registers_the_entry_points():
    c = _read('zkattest_napi.c')
    for name, fn in (('memberProofSizeRing', 'zk_member_proof_size_ring'), ('memberProveBatchRings', 'zk_member_prove_batch_rings'),
                     ('memberVerifyBatchRings', 'zk_member_verify_batch_rings')):
        assert re.search(r'\{"%s", \w+\}' % name, c), name
        assert re.search(r'\b%s\(' % fn, c), fn


def test_addon_compiles(tmp_path):
    out = _build(tmp_path)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_membership_lists_from_javascript(tmp_path):
    out = _build(tmp_path)
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'member_rings_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'member rings ok' in res.stdout, res.stdout + res.stderr
