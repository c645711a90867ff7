"""Helper of tests/test_gpu_distinct.py::test_bytes_do_not_depend_on_the_plan_or_the_build: run in a subprocess with ZKATTEST_LIB pointing at the library under
test (one process holds one build); proves the 257 distinct-key proofs of the test's workload and prints the SHA-256 of their bytes."""
import hashlib
import json
import os
import sys

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distinct_common as DC
import zkp_ecdsa_amd as Z

B = 257
eng = Z.Engine(0)
eng.set_comb_bits(16)
nh, tg, th = eng.synth_params(DC.PARAM_SEED)
eng.set_params(nh, tg, th, 20)
x1, r1, x2, r2, seeds = DC.workload(b'w257', B)
c1, c2 = eng.test_tom_commit(x1, r1), eng.test_tom_commit(x2, r2)
proofs, st = eng.distinct_prove_batch(DC.be32(x1), c1, DC.be32(r1), DC.be32(x2), c2, DC.be32(r2), seeds=seeds)
assert not any(st)
print(json.dumps({'lib': Z.LIB_PATH, 'sha256': hashlib.sha256(b''.join(proofs)).hexdigest()}))
eng.close()
