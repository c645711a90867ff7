"""not-gpu: the witness screen's point arithmetic on cooperating waves (csrc/coop_sums.h: co_front_walk over the parked multiples of the key, the range sums
through G's comb and a key's table) compiled for the host CPU against coop.h's SIMT emulation -- tests/host_arith/host_screen_co.cpp, a stand-alone program --
and compared with the oracle's affine u2 * pk and u1 * G for the chosen scalars of tests/test_gpu_screen_small.py; and the register / scratch figures of the
two new kernels in the built library (tools/kernel_meta.py)."""
import importlib.util
import os
import shutil
import subprocess

import pytest

import zkattest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host_arith', 'host_screen_co.cpp')
LIB = os.path.join(ROOT, 'zkp-ecdsa_amd', 'lib', 'libzkattest_hip.so')
FLAGS = ['-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-DPFIX_WIN_BITS=8', '-I' + os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')]

g, n = R.p256, R.p256.order
# the chosen scalars (test_gpu_screen_small.py imports them): u2 at the walk's digit extremes (+8 / -8 in every window, -1 with a carry to the top window, the
# top bit), u1 with empty windows and a zero low comb digit
U2 = [1, 8, n - 1, n - 8, int('88' * 32, 16), int('77' * 32, 16), 2 ** 255 + 1]
U1 = [0, 1, n - 1, (0x5eed1234abcdef << 24) % n]
SK = 0x1F3C5A7E9B2D4F60718293A4B5C6D7E8F9010B2C3D4E5F6A7B8C9DAEBFC0D1E3 % n


def _xy(pt):
    c = pt.toAffine()
    return bytes(64) if not c else c[0].to_bytes(32, 'big') + c[1].to_bytes(32, 'big')


def _mul(k):
    return g.generator().mul(g.newScalar(k % n))


def _run(exe, cases):
    text = 'G %s\nK %s\n' % (_xy(g.generator()).hex(), _xy(_mul(SK)).hex()) + ''.join('C %064x %064x\n' % c for c in cases)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split('\n')
    assert lines[6 * len(cases)] == 'done %d' % len(cases), lines[-3:]
    return [dict(l.split() for l in lines[6 * i:6 * i + 6]) for i in range(len(cases))]


@pytest.mark.skipif(shutil.which('g++') is None, reason='no g++')
def test_walk_and_range_sums_on_the_host_equal_the_oracle(tmp_path):
    """the stand-alone program under the host sanitizers: every chosen (u1, u2), scalars at and above n (the walks take any 256-bit value) and a seeded random few"""
    import random
    exe = tmp_path / 'host_screen_co'
    subprocess.check_call(['g++', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + FLAGS + [SRC, '-o', str(exe)])
    rnd = random.Random(20261019)
    cases = [(u1, u2) for u1 in U1 for u2 in U2] + [(0, 0), (n, n), (2 ** 256 - 1, 2 ** 256 - 1), (1 << 248, 0x80 << 248)]
    cases += [(rnd.randrange(n), rnd.randrange(n)) for _ in range(6)]
    out = _run(exe, cases)
    for (u1, u2), o in zip(cases, out):
        pk, gg = _xy(_mul(u2 * SK)).hex(), _xy(_mul(u1)).hex()
        assert o['walk'] == pk and o['kt+'] == pk, ('u2 * pk', hex(u2), o)
        assert o['kt-'] == _xy(_mul(-u2 * SK)).hex(), ('u2 * (-pk)', hex(u2), o)
        assert o['g4'] == gg and o['g3'] == gg, ('u1 * G', hex(u1), o)
        assert o['R'] == _xy(_mul(u1 + u2 * SK)).hex(), ('u1 * G + u2 * pk', hex(u1), hex(u2), o)
    assert out[len(U1) * len(U2)]['R'] == bytes(64).hex()   # (0, 0): the identity comes out as the identity


def test_cooperative_screen_kernels_in_the_library_fit_the_register_budget():
    if not os.path.exists(LIB):
        pytest.skip('library not built')
    spec = importlib.util.spec_from_file_location('kernel_meta', os.path.join(ROOT, 'tools', 'kernel_meta.py'))
    kernel_meta = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kernel_meta)
    ks = kernel_meta.kernels(LIB)
    for want in ('k_screen_table_co', 'k_screen_walk_co'):
        hits = [(name, k) for name, k in ks.items() if want in name]
        assert len(hits) == 1, (want, [name for name, _ in hits])
        name, k = hits[0]
        print(name, k)
        assert k['vgpr'] <= 256 and k['agpr'] == 0 and k['scratch'] == 0 and k['vgpr_spill'] == 0 and k['sgpr_spill'] == 0, (name, k)
        assert k['max_wg'] == 256 and k['lds'] <= 4096, (name, k)
