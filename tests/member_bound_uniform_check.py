"""Helper of tests/test_gpu_member_bound.py::test_uniform_build_gives_the_same_bytes: run in a subprocess with ZKATTEST_LIB pointing at the library under test
(one process holds one build); proves the 8-key ring's three bound proofs in both blinder modes and prints the SHA-256 of proofs, commitments and blinders,
and the bound verifier's verdicts on the last of them."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import member_bound_common as MB
import zkp_ecdsa_amd as Z

M = MB.M
eng = Z.Engine(0)
nh, tg, th = eng.synth_params(M.PARAM_SEED)
eng.set_params(nh, tg, th, 80)
eng.set_ring(M.ring_bytes(M.ring_values(b'k8', 8)), 8)
which, ctx, seeds, bl = MB.inputs('k8')
h = hashlib.sha256()
for mode in MB.MODES:
    blb = b''.join(b.to_bytes(32, 'big') for b in bl) if mode == 'caller' else None
    proofs, coms, blinders, st = eng.member_prove_batch(which, blinders=blb, seeds=seeds, context=ctx)
    assert not any(st)
    h.update(b''.join(proofs) + b''.join(coms) + b''.join(blinders))
ok, vst = eng.member_verify_batch(coms, proofs, context=ctx)
print(json.dumps({'lib': Z.LIB_PATH, 'sha256': h.hexdigest(), 'verdicts': [ok, vst]}))
eng.close()
