"""Escrow tags opened against several key rings behind the N-API facade.  not-gpu: openEscrowTags takes one key list per tag (the typings declare the overload
and its { ring, index } result), the Engine has ringsEscrowOpenBatch, the addon registers it on zk_rings_escrow_open_batch and compiles.  -m gpu:
bindings/napi/escrow_rings_check.js -- tags interleaved over three rings open in their own lists, and ring by ring the one-ring form agrees."""
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


def test_facade_engine_and_typings():
    js, dts = _read('zkattest.js'), _read('zkattest.d.ts')
    assert re.search(r'^    ringsEscrowOpenBatch\(secret32, tags, ringIds\) \{', js, re.M)
    body = js[js.index('async function openEscrowTags(params, secret, keys, tags)'):]
    body = body[:body.index('\n}\n')]
    assert 'isKeyLists(keys)' in body and 'ringsEscrowOpenBatch(' in body and 'escrowOpenBatch(a, raw)' in body   # both forms behind one name
    engine = dts[dts.index('export class Engine {'):]
    assert re.search(r'^    ringsEscrowOpenBatch\(secret32: Uint8Array, tags: Buffer\[\], ringIds: number\[\]\): \{ ring: number\[\]; index: number\[\]; status: Int32Array \}', engine, re.M)
    assert re.search(r'export function openEscrowTags\(params: [^,]+, secret: [^,]+, keys: \(bigint\[\] \| Buffer\)\[\], tags: [^:]+\): '
                     r'Promise<\(\{ ring: number; index: number \} \| null\)\[\]>', dts)
    assert os.path.exists(os.path.join(NAPI, 'escrow_rings_check.js'))


def test_addon_registers_the_entry_point():
    c = _read('zkattest_napi.c')
    assert re.search(r'\{"ringsEscrowOpenBatch", \w+\}', c) and re.search(r'\bzk_rings_escrow_open_batch\(c, B, ', c)


def test_addon_compiles(tmp_path):
    out = _build(tmp_path)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_escrow_rings_from_javascript(tmp_path):
    out = _build(tmp_path)
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'escrow_rings_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'escrow rings ok' in res.stdout, res.stdout + res.stderr
