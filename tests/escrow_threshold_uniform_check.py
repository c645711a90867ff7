"""Helper of tests/test_gpu_escrow_threshold.py::test_bytes_do_not_depend_on_comb_width_mode_or_build: run in a subprocess with ZKATTEST_LIB pointing at the
library under test (one process holds one build); splits the test's secret 3-of-5, makes every auditor's shares of the test's tags (read from the file named
on the command line), and prints the SHA-256 of the split's and the shares' bytes."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import escrow_common as EC
import zkp_ecdsa_amd as Z

tags_raw = open(sys.argv[1], 'rb').read()
tags = [tags_raw[o:o + EC.SIZE] for o in range(0, len(tags_raw), EC.SIZE)]
eng = Z.Engine(0)
eng.set_comb_bits(16)
nh, tg, th = eng.synth_params(EC.PARAM_SEED)
eng.set_params(nh, tg, th, 20)
eng.set_chunk(64)
a32 = EC.tag(b'auditor-thr', 0)
eng.set_auditor(eng.escrow_keygen(a32))
shares, keys = eng.auditors_split_key(a32, 3, 5, seed=EC.tag(b'split-seed', 35))
eng.set_auditors(3, keys)
h = hashlib.sha256(b''.join(shares) + b''.join(keys))
for j in range(1, 6):
    sh, st = eng.auditors_share_batch(j, shares[j - 1], tags, seeds=EC.seeds_for(b'sh%d' % j, len(tags)))
    assert not any(st)
    h.update(b''.join(sh))
print(json.dumps({'lib': Z.LIB_PATH, 'sha256': h.hexdigest()}))
eng.close()
