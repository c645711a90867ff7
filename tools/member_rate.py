"""Membership proofs on their own (include/zkattest.h: zk_member_prove_batch / zk_member_verify_batch), measured: --batch proofs (65 536) over a ring of --ring
values (2^16), every buffer device-resident.

Recorded: membership proofs/s and verifies/s (wall time of the device-pointer calls, median of --reps calls after two warm-up calls), the GPU time of each
call's families (zk_last_timing), and the latency of a one-proof prove and verify call.  Beside them the yardstick: in the same process on the same device
zk_prove_batch_device proves full ZKAttest proofs over the same `which` (secLevel 80) and the time of its families gk_fold, tom_commit, hash and
respond_write is recorded.  Those families also hold the full prover's other commitments, hashes and responses, so their sum is an UPPER bound of its
membership part; the expectation is a membership call near that part, and a call above about 1.3 x the sum needs an explanation in DESIGN.md section 5c.
  python tools/member_rate.py [--batch 65536] [--ring 65536] [--reps 10] [--out profiles/member_rate.json]
Prints one JSON line (also written to --out PATH when given)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FAMILIES = ('gk_fold', 'tom_commit', 'hash', 'respond_write')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--ring', type=int, default=65536)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import zkp_ecdsa_amd as Z
    S, B, dev = 20261018, args.batch, 'cuda:0'
    res = {'tool': 'member_rate', 'batch': B, 'ring': args.ring, 'reps': args.reps}

    def up(b, dtype=torch.uint8):
        return torch.frombuffer(bytearray(b), dtype=dtype).to(dev)

    e = Z.Engine(0)
    e.set_timing(1)
    e.set_params(*e.synth_params(S), 80)
    ring, msg, sig, pk, which, seeds = e.synth_workload(S, args.ring, B)
    e.set_ring(ring, args.ring)
    size = e.member_proof_size()
    res['proof_bytes'] = size
    d_which, d_seeds = torch.tensor(which, dtype=torch.int32).to(dev), up(seeds)
    d_com, d_out = torch.empty(72 * B, dtype=torch.uint8, device=dev), torch.empty(size * B, dtype=torch.uint8, device=dev)
    d_st, d_ok = torch.ones(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)

    def timed(call, reps):
        walls, fams = [], []
        for rep in range(reps + 2):
            t0 = time.perf_counter()
            call()
            walls.append((time.perf_counter() - t0) * 1e3)
            fams.append(e.last_timing()[1])
        keys = sorted(set().union(*fams[2:]))
        return statistics.median(walls[2:]), {k: round(statistics.median(f.get(k, 0.0) for f in fams[2:]), 3) for k in keys}

    def prove(n):
        e.member_prove_batch_device(n, d_which.data_ptr(), None, d_seeds.data_ptr(), d_com.data_ptr(), None, d_out.data_ptr(), size * n, d_st.data_ptr())

    def verify(n):
        e.member_verify_batch_device(n, d_com.data_ptr(), d_out.data_ptr(), None, d_ok.data_ptr(), d_st.data_ptr())

    ms, fam = timed(lambda: prove(B), args.reps)
    torch.cuda.synchronize()
    assert int(d_st.abs().sum()) == 0
    res['prove'] = {'ms': round(ms, 3), 'per_s': round(B / ms * 1e3), 'families_ms': fam}
    ms, fam = timed(lambda: verify(B), args.reps)
    torch.cuda.synchronize()
    assert int(d_ok.sum()) == B and int(d_st.abs().sum()) == 0, 'the verifier rejected an honest proof'
    res['verify'] = {'ms': round(ms, 3), 'per_s': round(B / ms * 1e3), 'families_ms': fam}
    res['one_proof_ms'] = {'prove': round(timed(lambda: prove(1), args.reps)[0], 4), 'verify': round(timed(lambda: verify(1), args.reps)[0], 4)}
    # the yardstick: full proofs over the same `which`, in this process, on this device
    cap = e.proof_max_size() * B
    f_out, f_off = torch.empty(cap, dtype=torch.uint8, device=dev), torch.zeros(B + 1, dtype=torch.int64, device=dev)
    d_msg, d_sig, d_pk = up(msg), up(sig), up(pk)
    ms, fam = timed(lambda: e.prove_batch_device(B, d_msg.data_ptr(), d_sig.data_ptr(), d_pk.data_ptr(), d_which.data_ptr(), d_seeds.data_ptr(), f_out.data_ptr(), cap,
                                                 f_off.data_ptr(), d_st.data_ptr()), 3)
    torch.cuda.synchronize()
    assert int(d_st.abs().sum()) == 0
    part = {k: fam.get(k, 0.0) for k in FAMILIES}
    res['full_prover'] = {'ms': round(ms, 3), 'families_ms': part, 'families_sum_ms': round(sum(part.values()), 3)}
    res['prove_over_families_sum'] = round(res['prove']['ms'] / max(sum(part.values()), 1e-9), 4)
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
