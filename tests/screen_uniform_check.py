"""Helper of tests/test_gpu_screen.py::test_uniform_build_gives_the_same_flags: run in a subprocess with ZKATTEST_LIB pointing at the library under test;
screens a fixed small workload -- valid witnesses and a few mutants, find and check mode, with and without per-key tables -- and prints every answer."""
import json
import os
import sys

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zkp_ecdsa_amd as Z


def flip(b, bit):
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


answers = []
for kt in (1, 0):
    eng = Z.Engine(0)
    eng.set_key_tables(kt)
    eng.set_params(*eng.synth_params(41), 20)
    ring, msg, sig, pk, which, _ = eng.synth_workload(41, 100, 24)
    eng.set_ring(ring, 100)
    msg = flip(msg, 32 * 8 * 3 + 9)                                              # witness 3: another message
    sig = flip(sig, 64 * 8 * 5 + 300)                                            # witness 5: another s
    p7 = int.from_bytes(pk[64 * 7 + 32:64 * 8], 'big')
    P = 2 ** 256 - 2 ** 224 + 2 ** 192 + 2 ** 96 - 1
    pk = pk[:64 * 7 + 32] + ((P - p7) % P).to_bytes(32, 'big') + pk[64 * 8:]     # witness 7: -pk (the key table's negated root)
    pk = pk[:64 * 9] + pk[64 * 10:64 * 11] + pk[64 * 10:]                        # witness 9: witness 10's key
    answers.append(eng.screen_batch(msg, sig, pk))
    answers.append(eng.screen_batch(msg, sig, pk, which=which))
    eng.close()
print(json.dumps({'lib': Z.LIB_PATH, 'answers': answers}))
