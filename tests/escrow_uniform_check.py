"""Helper of tests/test_gpu_escrow.py::test_uniform_library_gives_the_same_bytes: run in a subprocess with ZKATTEST_LIB pointing at the library under test (one
process holds one build); makes the 67 escrow tags of the test's workload, opens them, and prints the SHA-256 of their bytes and the indices."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import escrow_common as EC
import zkp_ecdsa_amd as Z

B = 67
eng = Z.Engine(0)
eng.set_comb_bits(16)
nh, tg, th = eng.synth_params(EC.PARAM_SEED)
eng.set_params(nh, tg, th, 20)
eng.set_chunk(64)
a32 = EC.tag(b'auditor', 0)
eng.set_auditor(eng.escrow_keygen(a32))
ring = EC.MC.RING300
planted = [0, 299, 7, 7, 150] + [(37 * b + 11) % 300 for b in range(5, B)]
x = [ring[i] for i in planted]
_, r, seeds = EC.workload(b'w67', B)
c = eng.test_tom_commit(x, r)
tags, st = eng.escrow_prove_batch(EC.be32(x), c, EC.be32(r), seeds=seeds)
assert not any(st)
eng.set_ring(EC.MC.ring_bytes(ring), 300)
index, st = eng.escrow_open_batch(a32, tags)
assert not any(st)
print(json.dumps({'lib': Z.LIB_PATH, 'sha256': hashlib.sha256(b''.join(tags)).hexdigest(), 'index': index}))
eng.close()
