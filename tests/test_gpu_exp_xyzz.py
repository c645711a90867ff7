"""The Exp commit phase's key-table kernel (k_p256.hip: k_exp_commit_kt) sums its gathered table entries in XYZZ coordinates and recomputes a lane with the
complete law where a sum met an exceptional pair.  zk_test_exp_sum runs the kernel's own device function (exp_kt_sums) on given scalars next to the
complete-law walks; the oracle's P-256 arithmetic is the third opinion.  The ring's keys are sk_i * G and h_NIST is HS * G with every logarithm known here,
so the collisions a prover could craft are crafted."""
import os
import random
import re

import pytest

import zkattest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
g, n = R.p256, R.p256.order
NKEYS, KEY, SEED = 16, 5, 7171
HS = 0x2468ACE013579BDF0FEDCBA9876543211234567890ABCDEFFEDCBA0987654321 % n
SKS = [(0x1F3C5A7E9B2D4F60718293A4B5C6D7E8F9010B2C3D4E5F6A7B8C9DAEBFC0D1E3 * (i + 1) + i) % n for i in range(NKEYS)]


def _mul(k):
    return g.generator().mul(g.newScalar(k % n))


def _xy(pt):
    c = pt.toAffine()
    return bytes(64) if not c else c[0].to_bytes(32, 'big') + c[1].to_bytes(32, 'big')


@pytest.fixture(scope='module')
def setup():
    """An engine whose h_NIST and 16-key ring have known logarithms; sk: the logarithm of the BASE POINT of key KEY's table (the ring holds x only: +- SKS[KEY])."""
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    _, tg, th = eng.synth_params(SEED)
    eng.set_params(_xy(_mul(HS)), tg, th, 80)
    eng.set_ring(b''.join(_xy(_mul(s))[:32] for s in SKS), NKEYS)
    base = eng.test_exp_sum(KEY, False, [(0, 1, 0)])[0][0]
    sk = SKS[KEY] if base == _xy(_mul(SKS[KEY])) else n - SKS[KEY]
    assert base == _xy(_mul(sk))
    yield eng, sk
    eng.close()


def _check(eng, sk, cases, neg, want_fell):
    T, A, Tc, Ac, fell = eng.test_exp_sum(KEY, neg, cases)
    s = n - sk if neg else sk
    for i, (gs, ks, bs) in enumerate(cases):
        t = gs + ks * s
        print(i, 'fell', fell[i], 'T', T[i][:8].hex(), 'A', A[i][:8].hex())
        assert (T[i], A[i]) == (Tc[i], Ac[i]), (i, 'XYZZ sums differ from the complete law')
        assert T[i] == _xy(_mul(t)) and A[i] == _xy(_mul(t + bs * HS)), (i, 'differs from the oracle')
    assert fell == want_fell, fell


@pytest.mark.gpu
def test_random_sums_equal_the_complete_law_and_the_oracle_without_fallback(setup):
    eng, sk = setup
    rnd = random.Random(61)
    cases = [(rnd.randrange(n), rnd.randrange(n), rnd.randrange(n)) for _ in range(70)]    # more than one 64-lane block, the last one partly filled
    for neg in (False, True):
        _check(eng, sk, cases, neg, [0] * len(cases))


@pytest.mark.gpu
def test_crafted_collisions_take_the_complete_law_and_give_its_bytes(setup):
    """g = +-d sk with d the first key digit: the G-sum is the first key entry (a doubling) or its negative (the identity) -> T and with it A fall back (3).
    g = +-e HS - k sk with e the first digit of h's comb: T is h's first entry or its negative -> A alone falls back (2).  Honest lanes between them stay at 0."""
    eng, sk = setup
    rnd = random.Random(67)
    cases, want = [], []
    for _ in range(3):
        k = (rnd.randrange(n) & ~0xff) | rnd.randrange(1, 128)
        d, b = k & 0xff, rnd.randrange(n)
        cases += [(d * sk % n, k, b), (rnd.randrange(n), k, b), (-d * sk % n, k, b)]
        want += [3, 0, 3]
        b = (rnd.randrange(n) & ~0xfffff) | rnd.randrange(1, 1 << 20)      # h's comb has 20-bit windows
        e, k = b & 0xfffff, rnd.randrange(n)
        cases += [((e * HS - k * sk) % n, k, b), ((-e * HS - k * sk) % n, k, b)]
        want += [2, 2]
    cases += [(9 * sk % n, 9, 0), (-9 * sk % n, 9, 0)]      # nothing from h: A = T; the second is the identity twice
    want += [3, 3]
    _check(eng, sk, cases, False, want)


@pytest.mark.gpu
def test_empty_parts_and_digit_extremes(setup):
    eng, sk = setup
    rnd = random.Random(71)
    r = lambda: rnd.randrange(n)
    cases = [(0, 0, 0), (r(), 0, 0), (0, r(), 0), (0, 0, r()), (r(), r(), 0), (r(), 0, r()), (0, r(), r())]   # (0, 0, *): T is the identity, 64 zero bytes on both paths
    cases += [(5 << 40, 0, 0), (0, 77 << 80, 0), (0, 0, 3 << 240), (0, 128, 0), (0, 129 << 8, 0)]             # a single non-zero digit
    cases += [(r(), int('80' * 32, 16) % n, r()), (r(), int('81' * 32, 16) % n, r()), (n - 1, int('7f80' * 16, 16), n - 1)]
    T = eng.test_exp_sum(KEY, False, cases)[0]
    assert T[0] == bytes(64) and T[3] == bytes(64)
    for neg in (False, True):
        _check(eng, sk, cases, neg, [0] * len(cases))


@pytest.mark.gpu
def test_eight_proofs_end_to_end_against_the_oracle_with_one_foreign_slot():
    """8 proofs, ring 16, secLevel 80 through zk_prove_batch, byte for byte: seven on the key-table path (k_exp_commit_kt), one whose `which` names another
    signer's slot and takes the per-proof table of R (k_exp_commit) in the same chunk."""
    import coracle as CO
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    nh, tg, th = eng.synth_params(SEED)
    eng.set_params(nh, tg, th, 80)
    ring, msg, sig, pk, which, seeds = eng.synth_workload(SEED, NKEYS, 8)
    which = list(which)
    which[6] = (which[6] + 3) % NKEYS
    eng.set_ring(ring, NKEYS)
    got, st = eng.prove_batch(msg, sig, pk, which, seeds=seeds)
    assert st == [0] * 8 and eng.test_counter(1) == 7
    octx = CO.OracleCtx(nh, tg, th, 80)
    octx.set_ring(ring, NKEYS)
    exp, est = octx.prove_batch(msg, sig, pk, which, seeds=seeds, nthreads=8)
    assert est == [0] * 8 and got == exp
    eng.close()


def test_the_kernel_keeps_three_waves_per_simd_without_scratch_or_agprs():
    """tools/kernel_meta.py on the built library: k_exp_commit_kt (not its _wide / _co siblings, which stay on the complete law)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('kernel_meta', os.path.join(ROOT, 'tools', 'kernel_meta.py'))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    ks = {k: v for k, v in km.kernels(os.path.join(ROOT, 'zkp-ecdsa_amd', 'lib', 'libzkattest_hip.so')).items() if re.search(r'\d+k_exp_commit_kt\d', k)}
    assert ks
    for name, k in ks.items():
        print(name, k)
        assert k['scratch'] == 0 and k['agpr'] == 0 and k['vgpr_spill'] == 0 and k['vgpr'] <= 168 and k['waves_per_simd'] >= 3, (name, k)
