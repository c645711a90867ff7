"""Operand table and checks shared by tests/test_modq_redc_host.py and tests/test_gpu_modq_redc.py: tests/modq_redc/modq_redc.hip runs every one-lane ModQ
product routine of csrc/field.h and the wide reduction through the reduction by q + 1 (ModQ::low_ones) AND through the generic reduction (a copy of ModQ with
low_ones = false).  The table: 0, 1, q - 1 against each other; every product class of tests/test_raw_limbs.py at its worst-case raw limbs (all limbs at the
largest value Fe<ModQ, K> allows, the structured vectors that module builds, every one against every other); operands whose quotient digits m_k are ALL 2^30 - 1
(a b = q mod R: 1 x q, q x 1, and random a below q with b = q / a mod R accepted when b < 512 q); 3 000 seeded random pairs over the classes.  The wide
reduction gets the 18 limbs of a b itself (its result must be the product's limbs) -- and, on the records where that is not already so, q + j R and q R - 1."""
import os
import random
import subprocess

import numpy as np

import test_raw_limbs as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'zkp-ecdsa_amd', 'csrc')
SRC = os.path.join(ROOT, 'tests', 'modq_redc', 'modq_redc.hip')
W, NL, MASK = 30, 9, (1 << 30) - 1
RR = 1 << (W * NL)
Q = RL.MODS[0]
KMAX = RR // Q
IN, HALF = 40, 54
SLOTS = ('limbs_mont_mul', 'limbs_mont_mul_n[0]', 'limbs_mont_mul_n[1]', 'limbs_mont_sqr', 'limbs_mont_mul_rows', 'redc_wide')


def limbs(v, n=NL):
    return tuple((v >> (W * i)) & MASK for i in range(n - 1)) + (v >> (W * (n - 1)),)


def val(l):
    return sum(int(x) << (W * i) for i, x in enumerate(l))


def digits(T):
    """the quotient digits m_0..m_8 of the Montgomery reduction of T modulo q"""
    m = T * (-pow(Q, -1, RR)) % RR
    assert (T + m * Q) % RR == 0
    return limbs(m)


_table = None


def table():
    """[(a limbs, b limbs, T, sq, tag)]; computed once"""
    global _table
    if _table is not None:
        return _table
    recs = []

    def add(a, b, ka, kb, tag, T=None):
        a, b = tuple(a), tuple(b)
        assert val(a) < ka * Q and val(b) < kb * Q and ka * kb <= KMAX and max(a[:8] + b[:8]) <= MASK
        sq = 0 if ka * ka <= KMAX else 1
        assert (kb if sq else ka) ** 2 <= KMAX
        T = val(a) * val(b) if T is None else T
        assert 0 <= T < Q * RR
        recs.append((a, b, T, sq, tag))
    small = [0, 1, Q - 1]
    for x in small:
        for y in small:
            add(limbs(x), limbs(y), 1, 1, 'small')
    for cls in range(7):
        ka, kb = RL.product_class(0, cls)
        (sa, ra), (sb, rb) = RL.vectors(0, ka), RL.vectors(0, kb)
        for x, _ in sa:
            for y, _ in sb:
                add(x, y, ka, kb, 'worst P%d' % cls)
    # every m_k = 2^30 - 1  <=>  m = R - 1  <=>  T = -m q = q (mod R)
    add(limbs(1), limbs(Q), 1, 2, 'ones')
    add(limbs(Q), limbs(1), 2, 1, 'ones')
    rnd = random.Random('modq redc all-ones digits')
    found = 0
    while found < 32:
        a = rnd.randrange(1, Q, 2)
        b = Q * pow(a, -1, RR) % RR
        if b < 512 * Q:
            add(limbs(a), limbs(b), 1, 512, 'ones')
            found += 1
    for j in (0, 1, Q - 1, rnd.randrange(Q), rnd.randrange(Q)):
        add(limbs(1), limbs(1), 1, 1, 'ones wide', Q + j * RR)
    add(limbs(1), limbs(1), 1, 1, 'wide max', Q * RR - 1)
    add(limbs(1), limbs(1), 1, 1, 'wide full limbs', val([MASK] * 17 + [limbs(Q * RR - 1, 18)[17] - 1]))
    rnd = random.Random('modq redc random pairs')
    for i in range(3000):
        cls = rnd.randrange(7)
        ka, kb = RL.product_class(0, cls)
        if i % 3 == 0:
            a, b = rnd.randrange(ka * Q), rnd.randrange(kb * Q)
        else:   # limbs drawn one by one, a quarter of them full
            a, b = (val([MASK if rnd.random() < 0.25 else rnd.randint(0, MASK) for _ in range(8)]) + (rnd.randrange(((k * Q - 1) >> 240)) << 240) for k in (ka, kb))
        add(limbs(a), limbs(b), ka, kb, 'random')
    for a, b, T, sq, tag in recs:
        if tag.startswith('ones'):
            assert digits(T) == (MASK,) * NL
    _table = recs
    return recs


def write_table(path):
    recs = table()
    a = np.zeros((len(recs), IN), np.uint32)
    a[:, 0:9] = [r[0] for r in recs]
    a[:, 9:18] = [r[1] for r in recs]
    a[:, 18:36] = [limbs(r[2], 18) for r in recs]
    a[:, 36] = [r[3] for r in recs]
    with open(path, 'wb') as f:
        f.write(np.array([0x4452514d, len(recs), 0, 0], np.uint32).tobytes())
        f.write(a.tobytes())
    return len(recs)


def host_exe(out, *flags, opt='-O1'):
    subprocess.check_call(['g++', '-x', 'c++', opt, '-std=c++17', '-Wall', '-Werror', '-Wno-unknown-pragmas', '-DZK_HOST_BUILD', *flags, '-I' + CSRC, SRC, '-o', str(out)])
    return str(out)


def check_output(raw):
    """new == generic limb for limb; every result is the Montgomery product Python computes, below 2q, limbs below 2^30"""
    recs = table()
    o = np.frombuffer(raw, np.uint32).reshape(len(recs), 2, 6, NL)
    diff = np.argwhere((o[:, 0] != o[:, 1]).any(axis=2))
    assert len(diff) == 0, ['record %d (%s) %s: new %s, generic %s' % (i, recs[i][4], SLOTS[s], [hex(x) for x in o[i, 0, s]], [hex(x) for x in o[i, 1, s]]) for i, s in diff[:4]]
    rinv = pow(RR, -1, Q)
    new = o[:, 0].tolist()
    for i, (a, b, T, sq, tag) in enumerate(recs):
        av, bv = val(a), val(b)
        x = bv if sq else av
        want = [av * bv, av * bv, av * bv, x * x, av * bv, T]
        for s in range(6):
            l = new[i][s]
            v = val(l)
            assert max(l) <= MASK and v < 2 * Q and (v - want[s] * rinv) % Q == 0, (i, tag, SLOTS[s], [hex(x) for x in l])
            # more than the residue: the result is (T + m q) / R with the digits of T, an integer
            assert v == (want[s] + val(digits(want[s])) * Q) // RR, (i, tag, SLOTS[s])
        if T == av * bv:
            assert new[i][5] == new[i][0], (i, tag, 'redc_wide of the product differs from the product')
