"""Escrow tags behind the N-API facade.  not-gpu: the facade exports proveEscrowTag / verifyEscrowTag, their batched forms, openEscrowTags, escrowAuditorKey and
the EscrowTag class, the typings declare them, the addon registers its five entry points and compiles.  -m gpu: bindings/napi/escrow_check.js -- tags verify,
forgeries, other commitments and another auditor's key do not, the prover refuses an opening that does not hold, the opening finds the ring member, and
attestations carry their tags in both wire layouts."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAPI = os.path.join(ROOT, 'bindings', 'napi')
ADDON = (('setAuditor', 'zk_ctx_set_auditor'), ('escrowKeygen', 'zk_escrow_keygen'), ('escrowProveBatch', 'zk_escrow_prove_batch'),
         ('escrowVerifyBatch', 'zk_escrow_verify_batch'), ('escrowOpenBatch', 'zk_escrow_open_batch'))


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
    for name in ('proveEscrowTag', 'verifyEscrowTag', 'proveEscrowTags', 'verifyEscrowTags', 'openEscrowTags', 'escrowAuditorKey', 'EscrowTag'):
        assert re.search(r'\b%s\b' % name, exports), name
    assert re.search(r'async function proveEscrowTag\(params, auditor, key, com, blinder\)', js)
    assert re.search(r'async function verifyEscrowTag\(params, auditor, com, tag\)', js)
    assert re.search(r'async function openEscrowTags\(params, secret, keys, tags\)', js) and re.search(r'class EscrowTag\b', js)
    for m, _ in ADDON:
        assert re.search(r'^    %s\(' % m, js, re.M), m   # the Engine's methods
    assert os.path.exists(os.path.join(NAPI, 'escrow_check.js'))


def test_typings_declare_the_calls():
    dts = _read('zkattest.d.ts')
    for pat in (r'export function proveEscrowTag\(params: [^,]+, auditor: [^,]+, key: [^,]+, com: [^,]+, blinder: [^)]+\): Promise<EscrowTag>',
                r'export function verifyEscrowTag\(params: [^,]+, auditor: [^,]+, com: [^,]+, tag: [^)]+\): Promise<boolean>',
                r'export function proveEscrowTags\(', r'export function verifyEscrowTags\(',
                r'export function openEscrowTags\(params: [^,]+, secret: [^,]+, keys: [^,]+, tags: [^:]+\): Promise<\(number \| null\)\[\]>',
                r'export function escrowAuditorKey\(', r'export class EscrowTag \{', r'    setAuditor\(', r'    escrowKeygen\(', r'    escrowProveBatch\(',
                r'    escrowVerifyBatch\(', r'    escrowOpenBatch\('):
        assert re.search(pat, dts), pat
    engine = dts[dts.index('export class Engine {'):]
    assert set(re.findall(r'^    (escrow[A-Za-z]+|setAuditor)\(', engine, re.M)) == {m for m, _ in ADDON}


def test_addon_registers_the_entry_points():
    c = _read('zkattest_napi.c')
    for name, fn in ADDON:
        assert re.search(r'\{"%s", \w+\}' % name, c), name
        assert re.search(r'\b%s\(' % fn, c), fn


def test_addon_compiles(tmp_path):
    out = _build(tmp_path)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_escrow_tags_from_javascript(tmp_path):
    out = _build(tmp_path)
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'escrow_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'escrow ok' in res.stdout, res.stdout + res.stderr
