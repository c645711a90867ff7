"""Helper of tests/test_gpu_recover.py::test_uniform_build_gives_the_same_answers: run in a subprocess with ZKATTEST_LIB pointing at the library under
test; recovers the keys of a fixed small workload -- valid witnesses and a few mutants -- and prints every answer."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import zkp_ecdsa_amd as Z


def flip(b, bit):
    a = bytearray(b)
    a[bit // 8] ^= 1 << (bit % 8)
    return bytes(a)


eng = Z.Engine(0)
eng.set_params(*eng.synth_params(41), 20)
ring, msg, sig, pk, which, _ = eng.synth_workload(41, 100, 24)
eng.set_ring(ring, 100)
msg = flip(msg, 32 * 8 * 3 + 9)                                              # witness 3: another message
sig = flip(sig, 64 * 8 * 5 + 300)                                            # witness 5: another s
sig = sig[:64 * 8] + bytes(32) + sig[64 * 8 + 32:]                           # witness 8: r = 0
pks, wo, fl = eng.recover_batch(msg, sig)
eng.close()
print(json.dumps({'lib': Z.LIB_PATH, 'pk': [p.hex() if p is not None else None for p in pks], 'which': wo, 'flags': fl,
                  'own': [pk[64 * b:64 * b + 64].hex() for b in range(24)], 'own_which': list(which)}))
