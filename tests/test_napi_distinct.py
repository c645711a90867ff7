"""Distinct-key proofs behind the N-API facade.  not-gpu: the facade exports proveDifferentKeys / verifyDifferentKeys, their batched forms, distinctPairs and the
DistinctProof class, the typings declare them, the addon registers its two entry points and compiles.  -m gpu: bindings/napi/distinct_check.js -- proofs
verify, forgeries, swapped and other commitments do not, equal keys and a wrong opening are refused, three signers are counted pair by pair -- and the proof it
makes from pinned seeds is byte for byte the Python binding's."""
import json
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
    for name in ('proveDifferentKeys', 'verifyDifferentKeys', 'proveDifferentKeysBatch', 'verifyDifferentKeysBatch', 'distinctPairs', 'DistinctProof'):
        assert re.search(r'\b%s\b' % name, exports), name
    assert re.search(r'async function proveDifferentKeys\(params, keyA, comA, blinderA, keyB, comB, blinderB\)', js)
    assert re.search(r'async function verifyDifferentKeys\(params, comA, comB, proof\)', js)
    assert re.search(r'function distinctPairs\(k\)', js) and re.search(r'class DistinctProof\b', js)
    for m in ('distinctProveBatch', 'distinctVerifyBatch'):
        assert re.search(r'^    %s\(' % m, js, re.M), m   # the Engine's methods
    assert os.path.exists(os.path.join(NAPI, 'distinct_check.js'))


def test_typings_declare_the_calls():
    dts = _read('zkattest.d.ts')
    for pat in (r'export function proveDifferentKeys\(params: [^,]+, keyA: [^,]+, comA: [^,]+, blinderA: [^,]+, keyB: [^,]+, comB: [^,]+, blinderB: [^)]+\): Promise<DistinctProof>',
                r'export function verifyDifferentKeys\(params: [^,]+, comA: [^,]+, comB: [^,]+, proof: [^)]+\): Promise<boolean>',
                r'export function proveDifferentKeysBatch\(', r'export function verifyDifferentKeysBatch\(', r'export function distinctPairs\(k: number\): \[number, number\]\[\]',
                r'export class DistinctProof \{', r'    distinctProveBatch\(', r'    distinctVerifyBatch\('):
        assert re.search(pat, dts), pat


def test_addon_registers_the_entry_points():
    c = _read('zkattest_napi.c')
    for name, fn in (('distinctProveBatch', 'zk_distinct_prove_batch'), ('distinctVerifyBatch', 'zk_distinct_verify_batch')):
        assert re.search(r'\{"%s", \w+\}' % name, c), name
        assert re.search(r'\b%s\(' % fn, c), fn


def test_pairs_helpers_agree():
    """the Python helper's order is the one distinct_check.js asserts for the facade's: (i, j), i < j, lexicographic"""
    import zkp_ecdsa_amd as Z
    assert Z.Engine.distinct_pairs(3) == [(0, 1), (0, 2), (1, 2)]
    assert Z.Engine.distinct_pairs(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)] and Z.Engine.distinct_pairs(1) == []
    js = _read('distinct_check.js')
    assert 'distinctPairs(3), [[0, 1], [0, 2], [1, 2]]' in js and 'distinctPairs(4), [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]' in js


def test_addon_compiles(tmp_path):
    out = _build(tmp_path)
    assert os.path.getsize(out) > 0


@pytest.mark.gpu
def test_distinct_proofs_from_javascript(tmp_path):
    out = _build(tmp_path)
    env = dict(os.environ, ZKATTEST_NODE=out)
    res = subprocess.run(['node', 'distinct_check.js'], cwd=NAPI, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and 'distinct ok' in res.stdout, res.stdout + res.stderr
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    # the same proof through the Python binding: the same parameters, openings and seed
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    try:
        eng.set_params(bytes.fromhex(rec['nistH']), bytes.fromhex(rec['tomG']), bytes.fromhex(rec['tomH']), rec['sec'])
        be = lambda v: int(v).to_bytes(32, 'big')
        c1, c2 = bytes.fromhex(rec['com1']), bytes.fromhex(rec['com2'])
        proofs, st = eng.distinct_prove_batch(be(rec['key1']), [c1], be(rec['r1']), be(rec['key2']), [c2], be(rec['r2']), seeds=bytes.fromhex(rec['seed']))
        assert st == [0] and proofs[0].hex() == rec['proof']
        assert eng.distinct_verify_batch([c1], [c2], [bytes.fromhex(rec['proof'])]) == ([1], [0])
    finally:
        eng.close()
