"""The witness screen (include/zkattest.h: zk_screen_batch), measured against the prover: --batch witnesses (65 536), a ring of --ring keys (2^16), every
buffer device-resident.

For per-key tables on and off, and for find mode and check mode: the GPU time of the screen's two phases (zk_last_timing: screen_lookup, screen_ecdsa),
median of --reps timed calls after two warm-up calls.  In the same process on the same device zk_prove_batch_device proves the same batch (secLevel 80, key
tables on) and screen_ms / prove_ms is recorded.  Last, the lookup phase alone on a ring of --big-ring keys (2^20).
  python tools/screen_rate.py [--batch 65536] [--ring 65536] [--big-ring 1048576] [--reps 10] [--out profiles/screen_rate.json]
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
    ap.add_argument('--big-ring', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import zkp_ecdsa_amd as Z
    S, B, dev = 20261017, args.batch, 'cuda:0'
    res = {'tool': 'screen_rate', 'batch': B, 'ring': args.ring, 'big_ring': args.big_ring, 'reps': args.reps, 'screen_ms': {}}

    def up(b, dtype=torch.uint8):
        return torch.frombuffer(bytearray(b), dtype=dtype).to(dev)

    def screen_phases(e, d, find, reps, ids=None):
        """median GPU ms of (lookup, ecdsa) over `reps` calls after two warm-up calls; every witness must come back with flags 0 at its index"""
        runs = []
        for rep in range(reps + 2):
            e.screen_batch_device(B, d['msg'].data_ptr(), d['sig'].data_ptr(), d['pk'].data_ptr(), None if find else d['which'].data_ptr(), d['wo'].data_ptr(), d['fl'].data_ptr(),
                                  d_ring_ids=ids)
            _, fam = e.last_timing()
            runs.append((fam.get('screen_lookup', 0.0), fam.get('screen_ecdsa', 0.0)))
        torch.cuda.synchronize()
        assert int(d['fl'].abs().sum()) == 0 and bool((d['wo'] == d['which']).all()), 'the screen rejected a valid witness'
        lo, ec = statistics.median(r[0] for r in runs[2:]), statistics.median(r[1] for r in runs[2:])
        return {'lookup_ms': round(lo, 3), 'ecdsa_ms': round(ec, 3), 'total_ms': round(lo + ec, 3)}

    prove_ms = None
    for kt in (1, 0):
        e = Z.Engine(0)
        e.set_key_tables(kt)
        e.set_timing(1)
        e.set_params(*e.synth_params(S), 80)
        ring, msg, sig, pk, which, seeds = e.synth_workload(S, args.ring, B)
        e.set_ring(ring, args.ring)
        d = {'msg': up(msg), 'sig': up(sig), 'pk': up(pk), 'which': torch.tensor(which, dtype=torch.int32).to(dev),
             'wo': torch.zeros(B, dtype=torch.int32, device=dev), 'fl': torch.ones(B, dtype=torch.int32, device=dev)}
        for find in (True, False):
            res['screen_ms']['%s/%s' % ('key_tables' if kt else 'no_key_tables', 'find' if find else 'check')] = screen_phases(e, d, find, args.reps)
        if kt:   # the yardstick: the same batch proved, in this process, on this device
            cap = e.proof_max_size() * B
            d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
            d_off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
            d_st = torch.zeros(B, dtype=torch.int32, device=dev)
            d_seeds = up(seeds)
            walls = []
            for rep in range(4):
                t0 = time.perf_counter()
                e.prove_batch_device(B, d['msg'].data_ptr(), d['sig'].data_ptr(), d['pk'].data_ptr(), d['wo'].data_ptr(), d_seeds.data_ptr(), d_out.data_ptr(), cap, d_off.data_ptr(),
                                     d_st.data_ptr())
                walls.append((time.perf_counter() - t0) * 1e3)
            assert int(d_st.abs().sum()) == 0
            prove_ms = statistics.median(walls[1:])
            res['prove_ms'] = round(prove_ms, 2)
            del d_out
        e.close()
    res['screen_over_prove'] = {k: round(v['total_ms'] / prove_ms, 5) for k, v in res['screen_ms'].items()}
    # the lookup alone against a ring of 2^20 keys (no per-key tables at that size)
    e = Z.Engine(0)
    e.set_timing(1)
    e.set_params(*e.synth_params(S), 80)
    ring, msg, sig, pk, which, _ = e.synth_workload(S + 1, args.big_ring, B)
    e.set_ring(ring, args.big_ring)
    d = {'msg': up(msg), 'sig': up(sig), 'pk': up(pk), 'which': torch.tensor(which, dtype=torch.int32).to(dev),
         'wo': torch.zeros(B, dtype=torch.int32, device=dev), 'fl': torch.ones(B, dtype=torch.int32, device=dev)}
    res['big_ring_find'] = screen_phases(e, d, True, args.reps)
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
