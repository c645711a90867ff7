"""Bound membership proofs ("ZKMB") behind the N-API facade.  not-gpu: proveMembership / verifyMembership, their batched forms and the Lists forms read an
`options` argument behind the reference's parameter lists and hand options.context to the engine; the engine wrappers call the addon's four bound entry
points, which call the eight-call C ABI's host forms; the typings declare the option; GKProof takes both magics; the addon compiles.  -m gpu:
bindings/napi/member_bound_check.js -- bound proofs verify with their context, commitment and ring and with nothing else; each verifier takes its own magic."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAPI = os.path.join(ROOT, 'bindings', 'napi')
CALLS = ('proveMembership', 'verifyMembership', 'proveMemberships', 'verifyMemberships', 'proveMembershipLists', 'verifyMembershipLists')


def _read(name):
    return open(os.path.join(NAPI, name)).read()


def _build(tmp_path):
    if not (shutil.which('node') and shutil.which('gcc') and os.path.exists('/usr/include/node/node_api.h')):
        pytest.skip('node / gcc / node_api.h not available')
    out = str(tmp_path / 'zkattest.node')
    subprocess.check_call(['make', '-s', '-C', NAPI, 'OUT=' + out])
    return out


def _body(js, name):
    start = js.index('async function %s(' % name)
    return js[start:js.index('\n}\n', start)]


def test_facade_calls_read_the_context_option():
    js = _read('zkattest.js')
    assert re.search(r'function memberContexts\(args, at, B, name\)', js)
    for name in CALLS:
        body = _body(js, name)
        assert re.search(r"memberContexts\(arguments, 4, [^,]+, '%s'\)" % name, body), name
    # the contexts reach the engine wrappers, per selected entry in the Lists forms
    assert 'ctx && Buffer.concat(ctx)' in _body(js, 'proveMemberships') and 'ctx && Buffer.concat(ctx)' in _body(js, 'verifyMemberships')
    assert 'ctx && Buffer.concat(sel.map((i) => ctx[i]))' in _body(js, 'proveMembershipLists')
    assert 'ctx && Buffer.concat(sel.map((i) => ctx[i]))' in _body(js, 'verifyMembershipLists')
    assert "a context is a Uint8Array(32)" in js and 'one Uint8Array(32) per entry' in js
    for native in ('memberProveBatchBound', 'memberVerifyBatchBound', 'memberProveBatchRingsBound', 'memberVerifyBatchRingsBound'):
        assert re.search(r'context \? native\.%s\(' % native, js), native
    assert re.search(r"\['ZKM1', 'ZKMB'\]\.includes\(", js) and re.search(r'get bound\(\)', js)
    assert os.path.exists(os.path.join(NAPI, 'member_bound_check.js'))


def test_typings_declare_the_option():
    dts = _read('zkattest.d.ts')
    assert re.search(r'export interface MemberOptions \{ context\?: Uint8Array \}', dts)
    assert re.search(r'export interface MemberBatchOptions \{ context\?: Uint8Array\[\] \}', dts)
    for name in CALLS:
        opt = 'MemberOptions' if name in ('proveMembership', 'verifyMembership') else 'MemberBatchOptions'
        assert re.search(r'export function %s\([^\n]*, options: %s\): Promise<' % (name, opt), dts), name
        assert len(re.findall(r'export function %s\(' % name, dts)) == 2, name   # the reference's list stays declared beside it
    assert re.search(r'readonly bound: boolean', dts)


def test_addon_registers_the_bound_entry_points():
    c = _read('zkattest_napi.c')
    for name, fn in (('memberProveBatchBound', 'zk_member_prove_batch_bound'), ('memberVerifyBatchBound', 'zk_member_verify_batch_bound'),
                     ('memberProveBatchRingsBound', 'zk_member_prove_batch_rings_bound'), ('memberVerifyBatchRingsBound', 'zk_member_verify_batch_rings_bound')):
        assert re.search(r'\{"%s", \w+\}' % name, c), name
        assert re.search(r'\b%s\(' % fn, c), fn
    assert '32 context bytes per proof' in c


def test_addon_compiles(tmp_path):
    out = _build(tmp_path)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_bound_membership_from_javascript(tmp_path):
    out = _build(tmp_path)
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'member_bound_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'member bound ok' in res.stdout, res.stdout + res.stderr
