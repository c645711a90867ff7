"""csrc/field.h and csrc/coop.h at the WORST CASE their types admit, on the host and on the device.

Every other arithmetic test hands the field code canonical values through a Montgomery conversion, which scrambles the limbs: the operands that reach the templates
are pseudo-random and a limb of all ones has probability 2^-30.  tests/raw_limbs/raw_limbs.hip builds Fe<M, K> / CoFe<M, K> straight from limbs; this module writes
the vectors (per modulus and magnitude class K: K*M - 1, the largest value below K*M with limbs 0..7 full, k*M and k*M +- 1, 0, 1, M - 1, R mod M, one full limb at
each position, alternating limbs; for the cooperative layout also limbs of 2^30 - 1 + CO_NEAR and rows that put them beside a zero row and beside an unrelated value;
64 seeded random limb vectors), every structured a against every structured b, and checks the raw result limbs with Python integers: the residue, the promise of the
result's type (limb range, value < K_out * M, lanes 9..15 zero), that a row does not depend on the other rows of its wave, and that host and device write the same bytes.
No tolerance anywhere.  The moduli and R come from the oracle's curve parameters, not from consts_gen.h: a wrong generated constant shows as a wrong residue."""
import os
import random
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

import zkattest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'raw_limbs', 'raw_limbs.hip')
W, NL, MASK, KCAP = 30, 9, (1 << 30) - 1, 512
RR = 1 << (W * NL)
MODS = [R.p256.p, R.p256.order, R.tomEdwards256.p]           # ModQ, ModN, ModT
KMAX = [RR // m for m in MODS]
NEAR = int(re.search(r'#define CO_NEAR (\d+)u', open(os.path.join(CSRC, 'coop.h')).read()).group(1))
PRODUCT = [(1, 1), (2, 2), (4, 2), (16, 16), (64, 64), (128, 128), None]     # None: the corner (KCAP, kmax / KCAP)
SUB_KB = [1, 3, 4, 7, 127, 255]
SUB2 = [(1, 1), (2, 1), (3, 4), (127, 128)]
UNARY = [1, 2, 4, 16, 64, 128, 256, 512]
ONE_OUT, CO_OUT = 36, 16


def subc(kb):
    return next(c for c in (4, 8, 16, 32, 64, 128, 256) if kb < c)


def limbs(v):
    return tuple((v >> (W * i)) & MASK for i in range(NL - 1)) + (v >> (W * (NL - 1)),)


def val(l):
    return sum(x << (W * i) for i, x in enumerate(l))


def product_class(mod, cls):
    """(Ka, Kb) of a product class for this modulus, None where the static_assert refuses it"""
    if PRODUCT[cls] is None:
        return KCAP, KMAX[mod] // KCAP
    ka, kb = PRODUCT[cls]
    return (ka, kb) if ka * kb <= KMAX[mod] else None


def sum_classes(mod):
    return [(c, PRODUCT[c]) for c in range(6)] + [(7, (256, 256))]


ZERO = ((0,) * NL, 0)
_cache = {}


def vectors(mod, K, near=0):
    """(structured, random) operands of magnitude class K: (limbs, value) pairs, every one within the invariant of Fe<M, K> (near = 0) / CoFe<M, K>"""
    key = (mod, K, near)
    if key in _cache:
        return _cache[key]
    M = MODS[mod]
    KM = K * M
    cap = (KM - 1) >> (W * (NL - 1))
    out = []

    def add(l):
        l = tuple(l)
        v = val(l)
        assert 0 <= v < KM and all(x <= MASK + near for x in l[:NL - 1]) and len(l) == NL
        if (l, v) not in out:
            out.append((l, v))

    def below(low):
        """limbs 0..7 as given, the largest top limb that keeps the value below K*M"""
        return tuple(low) + ((KM - 1 - val(low)) >> (W * (NL - 1)),)
    add(limbs(KM - 1))
    add(below([MASK] * 8))
    for k in (range(K + 1) if K <= 4 else (0, 1, K - 1, K)):
        for d in (-1, 0, 1):
            if 0 <= k * M + d < KM:
                add(limbs(k * M + d))
    for v in (0, 1, M - 1, RR % M):
        add(limbs(v))
    for i in range(NL - 1):
        add(limbs(MASK << (W * i)))
    add(limbs(cap << (W * (NL - 1))))
    add(below([MASK, 0] * 4)[:8] + (min(cap, below([MASK, 0] * 4)[8]),))
    add(tuple([0, MASK] * 4) + (0,))
    if near:
        full = MASK + near
        add(below([full] * 8))
        add(below([full, 0] * 4))
        add(below([MASK, full] * 4))
        add((full,) + (0,) * 8)
        add((0,) * 7 + (full, 0))
    rnd = random.Random('raw limbs %d %d %d' % key)
    rand = []
    for _ in range(64):
        low = [MASK + near if rnd.random() < 0.25 else rnd.randint(0, MASK + near) for _ in range(NL - 1)]
        top = min(rnd.randint(0, cap), below(low)[8])
        rand.append((tuple(low) + (top,), val(low) + (top << (W * (NL - 1)))))
        assert rand[-1][1] < KM
    _cache[key] = (out, rand)
    return _cache[key]


def carry_vectors():
    """co_carry's own contract: any limbs below 2^32 (the top limb leaves room for the 3 it may receive)"""
    full = (1 << 32) - 1
    out = [(full,) * 8 + (full - 3,), (MASK,) * 9, (MASK + 1,) * 8 + (1 << 31,), (0,) * 8 + (full - 3,), (full,) + (0,) * 8, (0,) * 7 + (full, MASK), (MASK, full) * 4 + (1 << 30,),
           (3 << 30,) * 8 + ((1 << 30) + 5,), ((3 << 30) | MASK, MASK) * 4 + (MASK,)]
    rnd = random.Random('raw limbs carry')
    for _ in range(64):
        out.append(tuple(rnd.choice((full, MASK, rnd.randint(0, full))) for _ in range(8)) + (rnd.randint(0, full - 3),))
    return [(l, val(l)) for l in out]


class Group:
    def __init__(self, coop, mod, op, cls, ks, a, b, c=None, iso=None):
        self.coop, self.mod, self.op, self.cls, self.ks, self.a, self.b, self.c, self.iso = coop, mod, op, cls, ks, a, b, c, iso or []
        self.start = None


def pairs(va, vb):
    (sa, ra), (sb, rb) = va, vb
    return [(x, y) for x in sa for y in sb] + list(zip(ra, rb))


def one_lane_groups():
    gs = []
    for mod in range(3):
        def binary(op, cls, ka, kb, kc=None):
            ab = pairs(vectors(mod, ka), vectors(mod, kb))
            c = None
            if kc is not None:
                sc, rc = vectors(mod, kc)
                cs = sc + rc
                c = [cs[(7 * i + i // len(cs)) % len(cs)] for i in range(len(ab))]
            gs.append(Group(False, mod, op, cls, (ka, kb, kc), [p[0] for p in ab], [p[1] for p in ab], c))

        def unary(op, cls, k, in_b=False):
            s, r = vectors(mod, k)
            x, z = s + r, [ZERO] * len(s + r)
            gs.append(Group(False, mod, op, cls, (k,), z if in_b else x, x if in_b else z))
        for cls in range(7):
            pc = product_class(mod, cls)
            if pc is None:
                continue
            ka, kb = pc
            binary(0, cls, ka, kb), binary(9, cls, ka, kb)
            for op in range(2, 8):
                binary(op, cls, ka, kb, kb)
            unary(1, cls, ka, False) if ka * ka <= KMAX[mod] else unary(1, cls, kb, True)
        binary(8, 1, 2, 2)
        for cls, (ka, kb) in sum_classes(mod):
            binary(10, cls, ka, kb)
        for cls, kb in enumerate(SUB_KB):
            ka = KCAP - subc(kb)
            binary(11, cls, ka, kb), binary(18, cls, ka, kb)
            unary(13, cls, kb, True)
        for cls, (kb, kc) in enumerate(SUB2):
            binary(12, cls, KCAP - subc(kb + kc), kb, kc)
        for cls, k in enumerate(UNARY):
            if k <= 256:
                unary(14, cls, k)
            unary(15, cls, k), unary(17, cls, k)
            if k <= 4:
                unary(16, cls, k)
        for op in (19, 20, 21):
            unary(op, 1, 2)
    return gs


def coop_groups():
    gs = []
    for mod in range(3):
        M = MODS[mod]
        rnd = random.Random('raw limbs rows %d' % mod)

        def rows(op, cls, ka, kb, unary=False, va=None):
            """records in wave order: two waves that put the fullest vector beside a zero row and beside an unrelated modulus-sized value, then the pairs; every
            fourth wave (and those two) is repeated four times with only one of its rows kept: the kept row must not change"""
            va = va or vectors(mod, ka, NEAR)
            vb = ([ZERO], []) if unary else vectors(mod, kb, NEAR)
            nfa, nfb = va[0][-5 if len(va[0]) > 5 else 0], (vb[0][-5] if not unary else ZERO)
            m1, m2 = (lambda v: (limbs(v), v))(rnd.randrange(M)), (lambda v: (limbs(v), v))(rnd.randrange(M))
            if unary:
                m2 = ZERO
            ab = [(nfa, nfb), (ZERO, nfb), (m1, ZERO), (nfa, m2), (ZERO, m2), (nfa, ZERO), (nfa, nfb), (m1, nfb)]
            ab += [(x, ZERO) for x in va[0] + va[1]] if unary else pairs(va, vb)
            ab += [(ZERO, ZERO)] * (-len(ab) % 4)
            iso = []
            for w in range(len(ab) // 4):
                if w < 2 or w % 4 == 0:
                    for r in range(4):
                        iso.append((len(ab) + r, 4 * w + r))
                        ab += [ab[4 * w + i] if i == r else (ZERO, ZERO) for i in range(4)]
            gs.append(Group(True, mod, op, cls, (ka, kb), [p[0] for p in ab], [p[1] for p in ab], None, iso))
        for cls in range(7):
            pc = product_class(mod, cls)
            if pc is not None:
                rows(0, cls, *pc)
        rows(9, 2, 4, 2)
        for cls, (ka, kb) in sum_classes(mod):
            rows(1, cls, ka, kb)
        for cls, kb in enumerate(SUB_KB):
            for op in (2, 3, 4):
                rows(op, cls, KCAP - subc(kb), kb)
        rows(5, 0, 1, 1, True, (carry_vectors(), []))
        for cls, k in enumerate(UNARY):
            rows(6, cls, k, 1, True)
            if k <= 256:
                rows(7, cls, k, 1, True)
        for cls, k in ((0, 1), (1, 2), (5, 170)):
            rows(8, cls, k, 1, True)
        # co_rows moves rows: no isolation, whole waves are checked
        x = [p for p in vectors(mod, 2, NEAR)[0] + vectors(mod, 2, NEAR)[1]]
        x += [ZERO] * (-len(x) % 4)
        gs.append(Group(True, mod, 10, 1, (2, 1), x, [ZERO] * len(x)))
    return gs


def write_vectors(path):
    one, co = one_lane_groups(), coop_groups()
    blocks, n = [], 0
    for g in one:
        a = np.zeros((len(g.a), 31), np.uint32)
        a[:, 0], a[:, 2], a[:, 3] = g.mod, g.op, g.cls
        a[:, 4:13] = [x[0] for x in g.a]
        a[:, 13:22] = [x[0] for x in g.b]
        if g.c is not None:
            a[:, 22:31] = [x[0] for x in g.c]
        g.start, n = n, n + len(g.a)
        blocks.append(a)
    n_one, n = n, 0
    for g in co:
        a = np.zeros((len(g.a), 36), np.uint32)
        a[:, 0], a[:, 1], a[:, 2], a[:, 3] = g.mod, 1, g.op, g.cls
        a[:, 4:13] = [x[0] for x in g.a]
        a[:, 20:29] = [x[0] for x in g.b]
        g.start, n = n, n + len(g.a)
        blocks.append(a)
    with open(path, 'wb') as f:
        f.write(np.array([0x4c574152, n_one, n, 0], np.uint32).tobytes())
        for b in blocks:
            f.write(b.tobytes())
    return one, co, n_one, n


def check_output(raw, one, co, n_one, n_co):
    """every record of an output file against Python integers"""
    words = np.frombuffer(raw, np.uint32)
    assert len(words) == n_one * ONE_OUT + n_co * CO_OUT
    o1 = words[:n_one * ONE_OUT].reshape(n_one, ONE_OUT)
    o2 = words[n_one * ONE_OUT:].reshape(n_co, CO_OUT)
    for g in one:
        M, out = MODS[g.mod], o1[g.start:g.start + len(g.a)].tolist()
        rinv = pow(RR, -1, M)
        tag = ('one lane', g.mod, g.op, g.cls)

        def fe(o, slot, kout, want, i):
            l = o[9 * slot:9 * slot + 9]
            v = val(l)
            assert max(l) <= MASK and v < kout * M and v % M == want % M, (tag, i, 'slot', slot, [hex(x) for x in l])
        for i, o in enumerate(out):
            a, b, c = g.a[i][1], g.b[i][1], g.c[i][1] if g.c else 0
            op, used = g.op, 9
            if op in (0, 8, 9):
                fe(o, 0, 2, a * b * rinv, i)
            elif op == 1:
                fe(o, 0, 2, (a + b) ** 2 * rinv, i)       # the unused operand is zero
            elif 2 <= op <= 7:
                want = [a * b, a * c, c * b, b * a][:2 + (op - 2) // 2]
                for s, w in enumerate(want):
                    fe(o, s, 2, w * rinv, i)
                used = 9 * len(want)
            elif op == 10:
                fe(o, 0, g.ks[0] + g.ks[1], a + b, i)
            elif op == 11:
                fe(o, 0, g.ks[0] + subc(g.ks[1]), a - b, i)
            elif op == 12:
                fe(o, 0, g.ks[0] + subc(g.ks[1] + g.ks[2]), a - b - c, i)
            elif op == 13:
                fe(o, 0, subc(g.ks[0]) + 1, -b, i)        # -0 is C*M itself: fe_neg's bound is C + 1
            elif op == 14:
                fe(o, 0, 2 * g.ks[0], 2 * a, i)
            elif op == 15:
                fe(o, 0, 2, a, i)
            elif op == 16:
                assert tuple(o[:9]) == limbs(a % M), (tag, i)
            elif op in (17, 18):
                assert o[0] == (1 if (a - b) % M == 0 else 0), (tag, i, hex(a), hex(b))
                used = 1
            else:
                l = o[:9]
                v = val(l)
                assert max(l) <= MASK and v < 2 * M and (v * a - (RR * RR if a % M else v)) % M == 0, (tag, i, hex(a))   # inv(0) = 0
            assert not any(o[used:]), (tag, i)
    for g in co:
        M, out = MODS[g.mod], o2[g.start:g.start + len(g.a)].tolist()
        rinv = pow(RR, -1, M)
        tag = ('cooperative', g.mod, g.op, g.cls)
        ka, kb = g.ks
        for i, o in enumerate(out):
            (al, a), (bl, b) = g.a[i], g.b[i]
            row, op = i & 3, g.op
            assert not any(o[9:]), (tag, i, 'lanes 9..15')
            l, v = tuple(o[:9]), val(o[:9])
            if op == 5:
                assert v == a and max(l[:8]) <= MASK + 3, (tag, i, [hex(x) for x in l])
                continue
            if op == 6:
                assert l == limbs(a), (tag, i)
                continue
            if op == 9:
                assert l == (al if row in (0, 2) else bl), (tag, i)
                continue
            if op == 10:
                src = (2, 4, 0, 1)[row]
                assert l == (g.a[i - row + src][0] if src < 4 else (0,) * 9), (tag, i)
                continue
            if op == 0:
                want, kout = a * b * rinv, 2
                assert l[8] <= MASK, (tag, i)
            elif op == 1:
                want, kout = a + b, ka + kb
            elif op in (2, 3, 4):
                neg = op == 2 or (op == 3 and row in (1, 2)) or (op == 4 and row in (0, 3))
                want, kout = (a - b if neg else a + b), ka + subc(kb)
            else:
                want, kout = (op - 5) * a, (op - 5) * ka
            assert max(l) <= MASK + NEAR and v < kout * M and (v - want) % M == 0, (tag, i, [hex(x) for x in l])
        for alone, mixed in g.iso:
            assert out[alone] == out[mixed], (tag, 'row', mixed, 'depends on the other rows of its wave')


def _gxx(out, *flags, opt='-O1'):
    subprocess.check_call(['g++', '-x', 'c++', opt, '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-DZK_HOST_BUILD', *flags, '-I' + CSRC, SRC, '-o', str(out)])
    return str(out)


@pytest.fixture(scope='module')
def case(tmp_path_factory):
    """the vector file, the host executable and its output: made once"""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    d = tmp_path_factory.mktemp('raw_limbs')
    one, co, n_one, n_co = write_vectors(d / 'vectors.bin')
    exe = _gxx(d / 'raw_limbs_host')
    res = subprocess.run([exe, str(d / 'vectors.bin'), str(d / 'host.out')], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return dict(dir=d, groups=(one, co, n_one, n_co), host=open(d / 'host.out', 'rb').read())


def test_vector_file_holds_every_op_and_class(case):
    one, co, n_one, n_co = case['groups']
    per = {}
    for g in one + co:
        per[(g.coop, g.op)] = per.get((g.coop, g.op), 0) + len(g.a)
    print('records: %d one-lane, %d cooperative; per (layout, op): %s' % (n_one, n_co, sorted(per.items())))
    assert {op for coop, op in per if not coop} == set(range(22)) and {op for coop, op in per if coop} == set(range(11))
    # the corners are there for every modulus: KCAP x kmax / KCAP products, the largest minuend of every subtrahend class
    assert {(g.mod, g.ks[:2]) for g in one if g.op == 0 and g.cls == 6} == {(0, (512, 32)), (1, (512, 32)), (2, (512, 8))}
    assert {g.ks[:2] for g in one if g.op == 11} == {(508, 1), (508, 3), (504, 4), (504, 7), (384, 127), (256, 255)}
    assert {g.ks for g in one if g.op == 12} == {(508, 1, 1), (508, 2, 1), (504, 3, 4), (256, 127, 128)}
    # an operand really is at its bound: the largest value of the class, limbs of all ones, the fullest nearly normalised limbs
    for mod, M in enumerate(MODS):
        s, _ = vectors(mod, 512, NEAR)
        assert (limbs(512 * M - 1), 512 * M - 1) in s and any(l[:8] == (MASK,) * 8 for l, _ in s) and any(l[:8] == (MASK + NEAR,) * 8 for l, _ in s)


def test_field_templates_keep_their_promises_at_the_worst_case_limbs_on_the_host(case):
    check_output(case['host'], *case['groups'])


def test_host_build_runs_clean_under_the_address_and_undefined_behaviour_sanitizers(case):
    """the stand-alone host program again with -fsanitize=address,undefined on the whole vector file: no report, the same bytes"""
    d = case['dir']
    exe = _gxx(d / 'raw_limbs_san', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', opt='-O0')   # -O0: a quarter of the compile time
    res = subprocess.run([exe, str(d / 'vectors.bin'), str(d / 'san.out')], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and not res.stderr.strip(), res.stderr[-4000:]
    assert open(d / 'san.out', 'rb').read() == case['host']


@pytest.mark.gpu
def test_field_templates_at_the_worst_case_limbs_on_the_device_equal_the_host(case):
    """raw_limbs.hip compiled with hipcc for gfx950: one thread per one-lane record, one wave per four cooperative records -- the real row_newbcast / row_shl / row_shr
    (bound_ctrl zero fill) and ds_bpermute on full limbs.  The device writes the bytes the host build writes, and they pass the same checks."""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    d = case['dir']
    exe = d / 'raw_limbs_dev'
    t0 = time.time()
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-Wno-unused-value', '-Wno-unused-result', '-I' + CSRC, SRC, '-o', str(exe)], timeout=600)
    t1 = time.time()
    res = subprocess.run([str(exe), str(d / 'vectors.bin'), str(d / 'dev.out')], capture_output=True, text=True, timeout=120)
    print('raw_limbs device build: hipcc %.1f s, run %.1f s' % (t1 - t0, time.time() - t1))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    dev = open(d / 'dev.out', 'rb').read()
    if dev != case['host']:
        check_output(dev, *case['groups'])      # names the first record that breaks a promise
    assert dev == case['host']
