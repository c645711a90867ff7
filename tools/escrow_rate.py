"""Escrow tags (include/zkattest.h: zk_escrow_prove_batch / zk_escrow_verify_batch / zk_escrow_open_batch), measured beside the link calls on the same
commitments: --batch tags (65 536), every buffer device-resident, --comb-bits context combs (24), a ring of --ring keys (65 536) for the opening, the five
calls alternating in one process.

Recorded: per call the wall time of the device-pointer form (median, minimum and maximum over --reps rounds behind one warm-up round) and the GPU time of its
families (zk_last_timing); the ratios escrow / link for prove and verify (six commitments against four, three relations against two: about 1.5 is the
estimate); the opening's three families on their own, with the ladder's time per tag; and the latency of one-tag calls.
  python tools/escrow_rate.py [--batch 65536] [--ring 65536] [--comb-bits 24] [--reps 3] [--out profiles/escrow_rate.json]
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
    ap.add_argument('--ring', type=int, default=65536)
    ap.add_argument('--comb-bits', type=int, default=24)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import zkp_ecdsa_amd as Z
    S, B, N, dev = 20261021, args.batch, args.ring, 'cuda:0'
    res = {'tool': 'escrow_rate', 'batch': B, 'ring_keys': N, 'comb_bits': args.comb_bits, 'reps': args.reps, 'tag_bytes': 472}

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def sc(t, i):
        return int.from_bytes(hashlib.sha256(b'escrow-rate' + t + i.to_bytes(4, 'big')).digest(), 'big') % Q

    e = Z.Engine(0)
    e.set_timing(1)
    e.set_comb_bits(args.comb_bits)
    e.set_params(*e.synth_params(S), 80)
    a32 = hashlib.sha256(b'escrow-rate-auditor').digest()
    e.set_auditor(e.escrow_keygen(a32))
    ring = [sc(b'key', i) for i in range(N)]
    be = lambda v: b''.join(i.to_bytes(32, 'big') for i in v)
    e.set_ring(be(ring), N)
    which = [(2654435761 * i) % N for i in range(B)]
    x, r1, r2 = [ring[w] for w in which], [sc(b'r1', i) for i in range(B)], [sc(b'r2', i) for i in range(B)]
    c1, c2 = e.test_tom_commit(x, r1), e.test_tom_commit(x, r2)
    d_x, d_r1, d_r2, d_c1, d_c2, d_a = up(be(x)), up(be(r1)), up(be(r2)), up(b''.join(c1)), up(b''.join(c2)), up(a32)
    d_seeds = up(b''.join(hashlib.sha256(b'escrow-rate-seed' + i.to_bytes(4, 'big')).digest() for i in range(B)))
    d_tags, d_links = torch.empty(472 * B, dtype=torch.uint8, device=dev), torch.empty(256 * B, dtype=torch.uint8, device=dev)
    d_st, d_ok = torch.ones(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
    d_idx = torch.zeros(B, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()
    calls = [('link_prove', lambda n: e.link_prove_batch_device(n, p(d_x), p(d_c1), p(d_r1), p(d_c2), p(d_r2), p(d_seeds), p(d_links), 256 * n, p(d_st))),
             ('link_verify', lambda n: e.link_verify_batch_device(n, p(d_c1), p(d_c2), p(d_links), p(d_ok), p(d_st))),
             ('prove', lambda n: e.escrow_prove_batch_device(n, p(d_x), p(d_c1), p(d_r1), p(d_seeds), p(d_tags), 472 * n, p(d_st))),
             ('verify', lambda n: e.escrow_verify_batch_device(n, p(d_c1), p(d_tags), p(d_ok), p(d_st))),
             ('open', lambda n: e.escrow_open_batch_device(n, p(d_a), p(d_tags), p(d_idx), p(d_st)))]

    def rounds(n, reps):
        """alternating rounds of the five calls -> per call: wall times and families of the rounds behind the warm-up one"""
        rec = {name: ([], []) for name, _ in calls}
        for rep in range(reps + 1):
            for name, call in calls:
                t0 = time.perf_counter()
                call(n)
                wall = (time.perf_counter() - t0) * 1e3
                if rep >= 1:
                    rec[name][0].append(wall), rec[name][1].append(e.last_timing()[1])
        return rec

    def summary(walls, fams, n):
        keys = sorted(set().union(*fams))
        med = statistics.median(walls)
        return {'ms': round(med, 4), 'min_ms': round(min(walls), 4), 'max_ms': round(max(walls), 4), 'per_s': round(n / med * 1e3),
                'families_ms': {k: round(statistics.median(f.get(k, 0.0) for f in fams), 4) for k in keys}}

    rec = rounds(B, args.reps)
    torch.cuda.synchronize()
    assert int(d_ok.sum()) == B and int(d_st.abs().sum()) == 0, 'the verifier rejected an honest tag'
    assert d_idx.cpu().tolist() == [w if w < 1 << 31 else w - (1 << 32) for w in which], 'a tag opened to another index than the planted one'
    for name, _ in calls:
        res[name] = summary(*rec[name], B)
    res['prove_over_link'] = round(res['prove']['ms'] / res['link_prove']['ms'], 3)
    res['verify_over_link'] = round(res['verify']['ms'] / res['link_verify']['ms'], 3)
    fam = res['open']['families_ms']
    res['open']['ladder_us_per_tag'] = round(fam.get('escrow_ladder', 0.0) / B * 1e3, 4)
    res['open']['ring_points_ns_per_key'] = round(fam.get('escrow_ring_points', 0.0) / N * 1e6, 2)
    one = rounds(1, args.reps)
    torch.cuda.synchronize()
    assert int(d_ok[0]) == 1 and int(d_idx[0]) == which[0]
    res['one_tag'] = {name: summary(*one[name], 1) for name, _ in calls}
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
