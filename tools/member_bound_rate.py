"""Bound membership proofs ("ZKMB", include/zkattest.h: zk_member_*_bound) against the unbound calls, measured on the same inputs: --batch proofs (65 536)
over a ring of --ring values (2^16), every buffer device-resident -- tools/member_rate.py's shape.

The statement adds 152 bytes (two or three SHA-256 compressions) to a challenge hash of 268 n bytes, so the expectation is a ratio near 1; no threshold is set.
After two warm-up rounds the tool ALTERNATES unbound and bound calls for --reps rounds on one device in one process (prove unbound, prove bound, verify unbound,
verify bound, and again), so drift of the box falls on both alike.  Recorded per call: the median wall time of the device-pointer call, its proofs per second,
its spread ((max - min) / median over the rounds: the run-to-run spread the ratio is read against), the GPU time of its families (zk_last_timing), and the
ratios bound / unbound of the medians for prove and verify; the same for a one-proof call.
  python tools/member_bound_rate.py [--batch 65536] [--ring 65536] [--reps 10] [--out profiles/member_bound_rate.json]
Prints one JSON line (also written to --out PATH when given)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    res = {'tool': 'member_bound_rate', 'batch': B, 'ring': args.ring, 'reps': args.reps}
    e = Z.Engine(0)
    e.set_timing(1)
    e.set_params(*e.synth_params(S), 80)
    ring, _, _, _, which, seeds = e.synth_workload(S, args.ring, B)
    e.set_ring(ring, args.ring)
    size = e.member_proof_size()
    res['proof_bytes'] = size
    d_which = torch.tensor(which, dtype=torch.int32).to(dev)
    d_seeds = torch.frombuffer(bytearray(seeds), dtype=torch.uint8).to(dev)
    g = torch.Generator().manual_seed(S)
    d_ctx = torch.randint(0, 256, (32 * B,), dtype=torch.uint8, generator=g).to(dev)
    # one set of outputs per kind: each verifier reads the proofs its own prover wrote
    buf = {k: {'com': torch.empty(72 * B, dtype=torch.uint8, device=dev), 'out': torch.empty(size * B, dtype=torch.uint8, device=dev),
               'st': torch.ones(B, dtype=torch.int32, device=dev), 'ok': torch.zeros(B, dtype=torch.uint8, device=dev)} for k in ('unbound', 'bound')}

    def prove(kind, n):
        b = buf[kind]
        e.member_prove_batch_device(n, d_which.data_ptr(), None, d_seeds.data_ptr(), b['com'].data_ptr(), None, b['out'].data_ptr(), size * n, b['st'].data_ptr(),
                                    d_context=d_ctx.data_ptr() if kind == 'bound' else None)

    def verify(kind, n):
        b = buf[kind]
        e.member_verify_batch_device(n, b['com'].data_ptr(), b['out'].data_ptr(), None, b['ok'].data_ptr(), b['st'].data_ptr(),
                                     d_context=d_ctx.data_ptr() if kind == 'bound' else None)

    def alternate(n, reps):
        walls = {(op, k): [] for op in ('prove', 'verify') for k in ('unbound', 'bound')}
        fams = {key: [] for key in walls}
        for rep in range(reps + 2):
            for op, call in (('prove', prove), ('verify', verify)):
                for kind in ('unbound', 'bound'):
                    t0 = time.perf_counter()
                    call(kind, n)
                    dt = (time.perf_counter() - t0) * 1e3
                    if rep >= 2:
                        walls[(op, kind)].append(dt), fams[(op, kind)].append(e.last_timing()[1])
        out = {}
        for op in ('prove', 'verify'):
            out[op] = {}
            for kind in ('unbound', 'bound'):
                w, f = walls[(op, kind)], fams[(op, kind)]
                med = statistics.median(w)
                keys = sorted(set().union(*f))
                out[op][kind] = {'ms': round(med, 4), 'per_s': round(n / med * 1e3), 'min_ms': round(min(w), 4), 'max_ms': round(max(w), 4),
                                 'spread': round((max(w) - min(w)) / med, 4), 'families_ms': {k: round(statistics.median(x.get(k, 0.0) for x in f), 3) for k in keys}}
            out[op]['bound_over_unbound'] = round(out[op]['bound']['ms'] / out[op]['unbound']['ms'], 4)
        return out

    res['batch_calls'] = alternate(B, args.reps)
    torch.cuda.synchronize()
    for kind in ('unbound', 'bound'):
        assert int(buf[kind]['st'].abs().sum()) == 0 and int(buf[kind]['ok'].sum()) == B, 'the %s verifier rejected an honest proof' % kind
    magic = {k: bytes(buf[k]['out'][:4].cpu().numpy()).decode() for k in buf}
    assert magic == {'unbound': 'ZKM1', 'bound': 'ZKMB'}, magic
    assert bytes(buf['bound']['com'].cpu().numpy()) == bytes(buf['unbound']['com'].cpu().numpy())   # the same draws: the same commitments
    one = alternate(1, args.reps)
    res['one_proof_calls'] = {op: {'unbound_ms': one[op]['unbound']['ms'], 'bound_ms': one[op]['bound']['ms'], 'unbound_spread': one[op]['unbound']['spread'],
                                   'bound_over_unbound': one[op]['bound_over_unbound']} for op in one}
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
