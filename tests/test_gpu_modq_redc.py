"""-m gpu: the reduction modulo q through q + 1 (csrc/field.h) on the device.  The operand table of tests/modq_redc_common.py through a tiny kernel, one record per
lane, against the host build's limbs; 64 proofs over a ring of 2^9 keys at secLevel 80 proved and verified, byte for byte against the oracle (the ring fold's wide
reductions, the XYZZ table sums, the PointAdd scalars and responses all multiply modulo q); a proof whose P-256 relation is forged keeps its verdict and status."""
import hashlib
import shutil
import subprocess
import time

import pytest

import modq_redc_common as C
from zka1_mutants import Layout, _flip

pytestmark = pytest.mark.gpu
S, NKEYS, B = 4242, 512, 64


def test_operand_table_on_the_device_gives_the_host_limbs(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    n = C.write_table(tmp_path / 'table.bin')
    assert n > 64 * 4                                        # a few hundred lanes at least, the last block partly filled or not
    host = C.host_exe(tmp_path / 'modq_redc_host')
    subprocess.check_call([host, str(tmp_path / 'table.bin'), str(tmp_path / 'host.out')], timeout=120)
    t0 = time.time()
    subprocess.check_call([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-Wno-unused-value', '-Wno-unused-result', '-I' + C.CSRC, C.SRC, '-o', str(tmp_path / 'modq_redc_dev')],
                          timeout=600)
    t1 = time.time()
    res = subprocess.run([str(tmp_path / 'modq_redc_dev'), str(tmp_path / 'table.bin'), str(tmp_path / 'dev.out')], capture_output=True, text=True, timeout=120)
    print('modq_redc device build: hipcc %.1f s, run %.1f s, %d records' % (t1 - t0, time.time() - t1, n))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    dev, want = open(tmp_path / 'dev.out', 'rb').read(), open(tmp_path / 'host.out', 'rb').read()
    if dev != want:
        C.check_output(dev)        # names the first record that is wrong
    assert dev == want
    C.check_output(dev)


@pytest.fixture(scope='module')
def proved():
    import coracle as CO
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    nh, tg, th = eng.synth_params(S)
    eng.set_params(nh, tg, th, 80)
    ring, msg, sig, pk, which, seeds = eng.synth_workload(S, NKEYS, B)
    eng.set_ring(ring, NKEYS)
    octx = CO.OracleCtx(nh, tg, th, 80)
    octx.set_ring(ring, NKEYS)
    got, st = eng.prove_batch(msg, sig, pk, which, seeds=seeds)
    exp, est = octx.prove_batch(msg, sig, pk, which, seeds=seeds, nthreads=16)
    yield eng, octx, msg, got, st, exp, est
    eng.close()


def test_64_proofs_over_a_ring_of_512_keys_equal_the_oracle_byte_for_byte_and_verify(proved):
    eng, octx, msg, got, st, exp, est = proved
    assert st == est == [0] * B
    assert got == exp, [i for i in range(B) if got[i] != exp[i]]
    vs = b''.join(hashlib.sha256(b'modq redc' + i.to_bytes(4, 'big')).digest() for i in range(B))
    assert eng.verify_batch(msg, got, vseeds=vs) == octx.verify_batch(msg, got, nthreads=16, vseeds=vs) == ([1] * B, [0] * B)


def test_a_forged_p256_relation_is_rejected_with_the_oracles_status(proved):
    """One bit of a PointAdd response scalar -- the relation between the committed coordinates of T1 = z R + Q, modulo q -- flipped in EVERY repetition that carries
    the sub-proof, so that whichever repetitions the verifier samples, it meets one; and one bit of the commitment to a coordinate, likewise."""
    eng, octx, msg, got, st, exp, est = proved
    lay = Layout(got[0], 9)
    scalar, point = got[0], got[0]
    for i in lay.zero_reps:
        scalar = _flip(scalar, lay.padd_scalars(i)[3] + 17, 4)
        point = _flip(point, lay.padd_points(i)[0] + 50, 1)
    forged = [got[1], scalar, point, got[0]]
    msgs = msg[32:64] + msg[:32] * 3
    vs = b''.join(hashlib.sha256(b'modq forged' + i.to_bytes(4, 'big')).digest() for i in range(4))
    g, o = eng.verify_batch(msgs, forged, vseeds=vs), octx.verify_batch(msgs, forged, nthreads=4, vseeds=vs)
    print('engine', g, 'oracle', o)
    assert g == o
    assert g[0] == [1, 0, 0, 1] and g[1][0] == 0 and g[1][3] == 0
