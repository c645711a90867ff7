"""Helper of tests/test_gpu_member.py::test_ring300_bytes_do_not_depend_on_the_plan_or_the_build: run in a subprocess with ZKATTEST_LIB pointing at the library
under test (one process holds one build); proves the 300 membership proofs of the test's workload and prints the SHA-256 of their bytes and commitments."""
import hashlib
import json
import os
import sys

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import member_common as M
import zkp_ecdsa_amd as Z

eng = Z.Engine(0)
nh, tg, th = eng.synth_params(M.PARAM_SEED)
eng.set_params(nh, tg, th, 80)
eng.set_ring(M.ring_bytes(M.RING300), 300)
eng.set_chunk(128)
proofs, coms, _, st = eng.member_prove_batch(list(range(300)), seeds=M.seeds_for(b'r300', 300))
assert not any(st)
print(json.dumps({'lib': Z.LIB_PATH, 'sha256': hashlib.sha256(b''.join(proofs) + b''.join(coms)).hexdigest()}))
eng.close()
