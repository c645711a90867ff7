"""The threshold opening behind the N-API facade.  not-gpu: the Engine has auditorsSplitKey, auditorsSetKeys, auditorsShareBatch, auditorsShareVerifyBatch and
auditorsCombineBatch, the facade splitAuditorKey, shareEscrowTags, verifyEscrowShares, combineEscrowShares and the class EscrowShare, the typings declare them,
none of the new names matches what the single-auditor tests pin, and the addon registers the entry points and compiles.  -m gpu:
bindings/napi/escrow_threshold_check.js -- a 3-of-5 split, every auditor's shares verify, three subsets combine to openEscrowTags' answer."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAPI = os.path.join(ROOT, 'bindings', 'napi')
ENGINE = ['auditorsSplitKey', 'auditorsSetKeys', 'auditorsShareBatch', 'auditorsShareVerifyBatch', 'auditorsCombineBatch']
FACADE = ['splitAuditorKey', 'shareEscrowTags', 'verifyEscrowShares', 'combineEscrowShares']
CALLS = {'auditorsSplitKey': 'zk_auditors_split_key', 'auditorsSetKeys': 'zk_ctx_set_auditors', 'auditorsShareBatch': 'zk_auditors_share_batch',
         'auditorsShareVerifyBatch': 'zk_auditors_share_verify_batch', 'auditorsCombineBatch': 'zk_auditors_combine_batch'}


def _read(name):
    return open(os.path.join(NAPI, name)).read()


def _build(tmp_path):
    if not (shutil.which('node') and shutil.which('gcc') and os.path.exists('/usr/include/node/node_api.h')):
        pytest.skip('node / gcc / node_api.h not available')
    out = str(tmp_path / 'zkattest.node')
    subprocess.check_call(['make', '-s', '-C', NAPI, 'OUT=' + out])
    return out


def test_facade_engine_and_typings():
    js, dts = _read('zkattest.js'), _read('zkattest.d.ts')
    engine = dts[dts.index('export class Engine {'):]
    for m in ENGINE:
        assert re.search(r'^    %s\(' % m, js, re.M) and re.search(r'^    %s\(' % m, engine, re.M) and 'native.%s(this.h, ' % m in js, m
        assert not m.startswith('escrow') and m != 'setAuditor'
    exports = js[js.index('module.exports = {'):]
    for f in FACADE + ['EscrowShare']:
        assert re.search(r'\b%s\b' % f, exports), f
    for f in FACADE:
        assert re.search(r'^async function %s\(' % f, js, re.M) and re.search(r'^export function %s\(' % f, dts, re.M), f
    assert re.search(r'^class EscrowShare \{', js, re.M) and re.search(r'^export class EscrowShare \{', dts, re.M)
    assert len(re.findall(r'^export function combineEscrowShares\(', dts, re.M)) == 2   # one key list, and one key list per tag
    assert len(re.findall(r'^export function openEscrowTags\(', dts, re.M)) == 2        # ... and the single auditor's overloads are as they were
    assert os.path.exists(os.path.join(NAPI, 'escrow_threshold_check.js'))


def test_addon_registers_the_entry_points():
    c = _read('zkattest_napi.c')
    for m, call in CALLS.items():
        assert re.search(r'\{"%s", \w+\}' % m, c) and re.search(r'\b%s\(c, ' % call, c), m


def test_addon_compiles(tmp_path):
    out = _build(tmp_path)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_threshold_opening_from_javascript(tmp_path):
    out = _build(tmp_path)
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'escrow_threshold_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'escrow threshold ok' in res.stdout, res.stdout + res.stderr
