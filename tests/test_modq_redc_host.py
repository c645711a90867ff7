"""The Montgomery reduction modulo the P-256 field prime q through q + 1 (csrc/field.h) on the host: the same limb vectors as the generic
reduction, for every one-lane product routine and the wide reduction, on the operand table of tests/modq_redc_common.py; and the trait of the generated constants
that selects it.  No tolerance anywhere."""
import os
import re
import shutil
import subprocess
import sys

import pytest

import modq_redc_common as C
import test_raw_limbs as RL

ROOT = C.ROOT


@pytest.fixture(scope='module')
def case(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    d = tmp_path_factory.mktemp('modq_redc')
    n = C.write_table(d / 'table.bin')
    exe = C.host_exe(d / 'modq_redc_host')
    res = subprocess.run([exe, str(d / 'table.bin'), str(d / 'host.out')], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    return dict(dir=d, n=n, host=open(d / 'host.out', 'rb').read())


def test_the_table_holds_the_cases(case):
    recs = C.table()
    tags = {}
    for r in recs:
        tags[r[4]] = tags.get(r[4], 0) + 1
    print(len(recs), 'records:', sorted(tags.items()))
    assert tags['small'] == 9 and tags['random'] == 3000 and tags['ones'] >= 34 and all(tags.get('worst P%d' % c, 0) >= 100 for c in range(7))
    full = [r for r in recs if r[0][:8] == (C.MASK,) * 8 and r[1][:8] == (C.MASK,) * 8]
    assert {r[4] for r in full} >= {'worst P%d' % c for c in range(7)}          # both operands with limbs 0..7 all ones, in every class
    assert any(C.val(r[0]) == 512 * C.Q - 1 and C.val(r[1]) == 32 * C.Q - 1 for r in recs)     # the corner of the static_assert, both at their bound


def test_reduction_by_q_plus_1_gives_the_limbs_of_the_generic_reduction_on_the_host(case):
    C.check_output(case['host'])


def test_host_program_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(case):
    d = case['dir']
    exe = C.host_exe(d / 'modq_redc_san', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', opt='-O0')
    res = subprocess.run([exe, str(d / 'table.bin'), str(d / 'san.out')], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and not res.stderr.strip(), res.stderr[-4000:]
    assert open(d / 'san.out', 'rb').read() == case['host']


def _generated(tmp_path):
    """the structs of a freshly generated consts_gen.h"""
    out = tmp_path / 'consts_gen.h'
    subprocess.check_call([sys.executable, os.path.join(ROOT, 'tools', 'gen_consts.py'), str(out)])
    txt = out.read_text()
    assert txt == open(os.path.join(C.CSRC, 'consts_gen.h')).read(), 'the committed consts_gen.h is not what tools/gen_consts.py writes'
    res = {}
    for name, body in re.findall(r'struct Mod(\w) \{(.*?)\n\};', txt, re.S):
        arr = lambda key: [int(v.strip().rstrip('u'), 16) for v in re.search(r'uint32_t %s\[9\] = \{([^}]*)\}' % key, body).group(1).split(',')]
        res[name] = dict(mod=arr('mod'), modp1=arr('modp1'), low_ones=re.search(r'bool low_ones = (true|false);', body).group(1) == 'true',
                         n0=int(re.search(r'n0 = (0x[0-9a-f]+)u', body).group(1), 16))
    return res


def test_generated_trait_low_ones_and_modp1(tmp_path):
    g = _generated(tmp_path)
    for name, M in (('Q', RL.MODS[0]), ('N', RL.MODS[1]), ('T', RL.MODS[2])):
        d = g[name]
        assert C.val(d['mod']) == M and C.val(d['modp1']) == M + 1 and max(d['modp1']) <= C.MASK
        ones = 0
        while (M >> ones) & 1:
            ones += 1
        # the rule, from the modulus alone: n0 = 1 and the low limbs are those of 2^s - 1, at least one whole limb, nothing of M + 1 below bit s
        assert d['low_ones'] == (d['n0'] == 1 and ones >= C.W and all(x == 0 for x in d['modp1'][:ones // C.W]) and d['modp1'][ones // C.W] % (1 << (ones % C.W)) == 0)
    assert g['Q']['low_ones'] and not g['T']['low_ones'] and not g['N']['low_ones']
    assert g['Q']['modp1'] == [0, 0, 0, 64, 0, 0, 1 << 12, (1 << 30) - (1 << 14), (1 << 16) - 1] and g['Q']['mod'][:4] == [C.MASK] * 3 + [63]
    assert sum(1 for x in g['Q']['modp1'] if x) == 4 and sum(1 for x in g['Q']['mod'] if x) == 7         # 4 x 9 = 36 multiply-adds per reduction, not 7 x 9 = 63
