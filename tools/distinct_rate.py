"""Distinct-key proofs (include/zkattest.h: zk_distinct_prove_batch / zk_distinct_verify_batch), measured beside the link calls: --batch proofs (65 536), every
buffer device-resident, --comb-bits combs (24), rounds of link prove / distinct prove / link verify / distinct verify alternating in one process.

Recorded: proofs/s and verifies/s of both kinds (wall time of the device-pointer calls: median and spread over --reps rounds after two warm-up rounds), the
GPU time of each call's families (zk_last_timing), the ratios distinct / link of the medians with their run-to-run spread (each round's own ratio: median,
min, max), and the same for one-proof calls.  From operation counts the prover is about 17 comb walks against link's 6 plus one inversion, the verifier about
750 point operations against 250: both near 3x are expected; that is an expectation, not a threshold.
  python tools/distinct_rate.py [--batch 65536] [--comb-bits 24] [--reps 10] [--out profiles/distinct_rate.json]
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
    res = {'tool': 'distinct_rate', 'batch': B, 'comb_bits': args.comb_bits, 'reps': args.reps, 'proof_bytes': {'distinct': 744, 'link': 256}}

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def sc(t, i):
        return int.from_bytes(hashlib.sha256(b'distinct-rate' + t + i.to_bytes(4, 'big')).digest(), 'big') % Q

    e = Z.Engine(0)
    e.set_timing(1)
    e.set_comb_bits(args.comb_bits)
    e.set_params(*e.synth_params(S), 80)
    x1, x2, r1, r2, r3 = ([sc(t, i) for i in range(B)] for t in (b'x1', b'x2', b'r1', b'r2', b'r3'))
    c1, c2, c3 = e.test_tom_commit(x1, r1), e.test_tom_commit(x2, r2), e.test_tom_commit(x1, r3)   # (c1, c2): different keys; (c1, c3): one key
    be = lambda v: b''.join(i.to_bytes(32, 'big') for i in v)
    d_x1, d_x2, d_r1, d_r2, d_r3 = up(be(x1)), up(be(x2)), up(be(r1)), up(be(r2)), up(be(r3))
    d_c1, d_c2, d_c3 = up(b''.join(c1)), up(b''.join(c2)), up(b''.join(c3))
    d_seeds = up(b''.join(hashlib.sha256(b'distinct-rate-seed' + i.to_bytes(4, 'big')).digest() for i in range(B)))
    d_dist, d_link = torch.empty(744 * B, dtype=torch.uint8, device=dev), torch.empty(256 * B, dtype=torch.uint8, device=dev)
    d_st = torch.ones(B, dtype=torch.int32, device=dev)
    d_okd, d_okl = torch.zeros(B, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()
    calls = (('link_prove', lambda n: e.link_prove_batch_device(n, p(d_x1), p(d_c1), p(d_r1), p(d_c3), p(d_r3), p(d_seeds), p(d_link), 256 * n, p(d_st))),
             ('distinct_prove', lambda n: e.distinct_prove_batch_device(n, p(d_x1), p(d_c1), p(d_r1), p(d_x2), p(d_c2), p(d_r2), p(d_seeds), p(d_dist), 744 * n, p(d_st))),
             ('link_verify', lambda n: e.link_verify_batch_device(n, p(d_c1), p(d_c3), p(d_link), p(d_okl), p(d_st))),
             ('distinct_verify', lambda n: e.distinct_verify_batch_device(n, p(d_c1), p(d_c2), p(d_dist), p(d_okd), p(d_st))))

    def rounds(n, reps):
        """alternating rounds of the four calls -> per call: wall times and families of the rounds behind the two warm-up ones"""
        rec = {name: ([], []) for name, _ in calls}
        for rep in range(reps + 2):
            for name, call in calls:
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

    def ratio(rec, side):
        per_round = [d / l for d, l in zip(rec['distinct_' + side][0], rec['link_' + side][0])]
        return {'of_medians': round(statistics.median(rec['distinct_' + side][0]) / statistics.median(rec['link_' + side][0]), 3),
                'per_round_median': round(statistics.median(per_round), 3), 'per_round_min': round(min(per_round), 3), 'per_round_max': round(max(per_round), 3)}

    def block(rec, n):
        out = {name: summary(*rec[name], n) for name, _ in calls}
        out['ratio_distinct_over_link'] = {'prove': ratio(rec, 'prove'), 'verify': ratio(rec, 'verify')}
        return out

    rec = rounds(B, args.reps)
    torch.cuda.synchronize()
    assert int(d_okd.sum()) == B and int(d_okl.sum()) == B and int(d_st.abs().sum()) == 0, 'a verifier rejected an honest proof'
    res['batch_calls'] = block(rec, B)
    one = rounds(1, args.reps)
    torch.cuda.synchronize()
    assert int(d_okd[0]) == 1 and int(d_okl[0]) == 1
    res['one_proof'] = block(one, 1)
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
