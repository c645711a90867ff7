"""Link proofs (include/zkattest.h: zk_link_prove_batch / zk_link_verify_batch), measured: --batch proofs (65 536), every buffer device-resident, --comb-bits
combs (24), alternating prove / verify rounds in one process.

Recorded: link proofs/s and verifies/s (wall time of the device-pointer calls: median and spread over --reps rounds after two warm-up rounds), the GPU time
of each call's families (zk_last_timing; the prover is four comb commitments in two pair launches, whose cost stands beside "tom_commit"'s own share), and
the latency of a one-proof prove and verify call -- the verifier's is a one-lane chain of about 160 Tom-256 point operations, recorded
so that a later change has a parent to beat.
  python tools/link_rate.py [--batch 65536] [--comb-bits 24] [--reps 10] [--out profiles/link_rate.json]
Prints one JSON line (also written to --out PATH when given)."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
Q = 0xffffffff00000001000000000000000000000000ffffffffffffffffffffffff


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--comb-bits', type=int, default=24)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import zkp_ecdsa_amd as Z
    S, B, dev = 20261020, args.batch, 'cuda:0'
    res = {'tool': 'link_rate', 'batch': B, 'comb_bits': args.comb_bits, 'reps': args.reps, 'proof_bytes': 256}

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def sc(t, i):
        return int.from_bytes(hashlib.sha256(b'link-rate' + t + i.to_bytes(4, 'big')).digest(), 'big') % Q

    e = Z.Engine(0)
    e.set_timing(1)
    e.set_comb_bits(args.comb_bits)
    e.set_params(*e.synth_params(S), 80)
    x, r1, r2 = [sc(b'x', i) for i in range(B)], [sc(b'r1', i) for i in range(B)], [sc(b'r2', i) for i in range(B)]
    c1, c2 = e.test_tom_commit(x, r1), e.test_tom_commit(x, r2)
    be = lambda v: b''.join(i.to_bytes(32, 'big') for i in v)
    d_x, d_r1, d_r2, d_c1, d_c2 = up(be(x)), up(be(r1)), up(be(r2)), up(b''.join(c1)), up(b''.join(c2))
    d_seeds = up(b''.join(hashlib.sha256(b'link-rate-seed' + i.to_bytes(4, 'big')).digest() for i in range(B)))
    d_out = torch.empty(256 * B, dtype=torch.uint8, device=dev)
    d_st, d_ok = torch.ones(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)

    def prove(n):
        e.link_prove_batch_device(n, d_x.data_ptr(), d_c1.data_ptr(), d_r1.data_ptr(), d_c2.data_ptr(), d_r2.data_ptr(), d_seeds.data_ptr(), d_out.data_ptr(), 256 * n,
                                  d_st.data_ptr())

    def verify(n):
        e.link_verify_batch_device(n, d_c1.data_ptr(), d_c2.data_ptr(), d_out.data_ptr(), d_ok.data_ptr(), d_st.data_ptr())

    def rounds(n, reps):
        """alternating prove / verify rounds -> per call: wall times and families of the rounds behind the two warm-up ones"""
        rec = {'prove': ([], []), 'verify': ([], [])}
        for rep in range(reps + 2):
            for name, call in (('prove', prove), ('verify', verify)):
                t0 = time.perf_counter()
                call(n)
                wall = (time.perf_counter() - t0) * 1e3
                if rep >= 2:
                    rec[name][0].append(wall), rec[name][1].append(e.last_timing()[1])
        return rec

    def summary(walls, fams, n):
        keys = sorted(set().union(*fams))
        med = statistics.median(walls)
        return {'ms': round(med, 4), 'min_ms': round(min(walls), 4), 'max_ms': round(max(walls), 4), 'per_s': round(n / med * 1e3),
                'families_ms': {k: round(statistics.median(f.get(k, 0.0) for f in fams), 4) for k in keys}}

    rec = rounds(B, args.reps)
    torch.cuda.synchronize()
    assert int(d_ok.sum()) == B and int(d_st.abs().sum()) == 0, 'the verifier rejected an honest proof'
    res['prove'], res['verify'] = summary(*rec['prove'], B), summary(*rec['verify'], B)
    fam = res['prove']['families_ms']
    res['prove']['tom_commit_share'] = round(fam.get('tom_commit', 0.0) / max(sum(fam.values()), 1e-9), 4)
    one = rounds(1, args.reps)
    torch.cuda.synchronize()
    assert int(d_ok[0]) == 1
    res['one_proof'] = {'prove': summary(*one['prove'], 1), 'verify': summary(*one['verify'], 1)}
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
