#!/usr/bin/env python3
"""Throughput of the key recovery (zk_recover_batch_device) against the screen's walk path (zk_screen_batch_device on a context without per-key tables:
the same 65-window walk and comb sum per witness), same process, same batch, alternating.

    python tools/recover_rate.py [--out profiles/recover_rate.json] [--batch 65536] [--keys 65536] [--repeats 7]

One context with per-key tables off, a ring of --keys keys, --batch valid witnesses in device memory.  Two calls of warm-up each, then --repeats rounds of
(screen, recover) timed by the wall clock around the blocking call; the medians, witnesses/s and the ratio recover / screen go into the file, and one more
call each under zk_ctx_set_timing(1) gives the families of zk_last_timing (recover_lift / recover_points / recover_lookup; screen_lookup / screen_ecdsa)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261019


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'recover_rate.json'))
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--keys', type=int, default=65536)
    ap.add_argument('--repeats', type=int, default=7)
    a = ap.parse_args()
    import torch   # first: one HIP runtime in the process (tests/conftest.py)
    sys.path.insert(0, ROOT)
    import zkp_ecdsa_amd as Z
    B = a.batch
    assert B <= a.keys, 'a synthetic workload is all valid only while the batch does not exceed the ring'
    e = Z.Engine(0)
    e.set_key_tables(0)
    e.set_params(*e.synth_params(SEED), 20)
    ring, msg, sig, pk, which, _ = e.synth_workload(SEED, a.keys, B)
    e.set_ring(ring, a.keys)
    dev = 'cuda:0'
    dm, ds, dp = (torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev) for x in (msg, sig, pk))
    dwo, dfl = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    dpk = torch.zeros(64 * B, dtype=torch.uint8, device=dev)
    calls = {'screen_walk': lambda: e.screen_batch_device(B, dm.data_ptr(), ds.data_ptr(), dp.data_ptr(), None, dwo.data_ptr(), dfl.data_ptr()),
             'recover': lambda: e.recover_batch_device(B, dm.data_ptr(), ds.data_ptr(), dpk.data_ptr(), dwo.data_ptr(), dfl.data_ptr())}
    e.set_timing(0)
    for name, call in calls.items():
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        assert dfl.cpu().tolist() == [0] * B and dwo.cpu().tolist() == list(which), name
        if name == 'recover':
            assert bytes(dpk.cpu().numpy().tobytes()) == bytes(pk), 'the recovered keys are not the workload\'s'
    ms = {k: [] for k in calls}
    for _ in range(a.repeats):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    e.set_timing(1)
    fam = {}
    for name, call in calls.items():
        call()
        fam[name] = {k: round(v, 3) for k, v in e.last_timing()[1].items()}
    med = {k: statistics.median(v) for k, v in ms.items()}
    doc = {'tool': 'tools/recover_rate.py', 'device': torch.cuda.get_device_name(0), 'batch': B, 'ring_keys': a.keys, 'sec_level': 20, 'repeats': a.repeats,
           'note': 'wall time of one blocking _device call in ms, alternating screen (per-key tables off: the walk path) and recover on one context; families: zk_last_timing, ms',
           'ms': {k: [round(x, 3) for x in v] for k, v in ms.items()}, 'median_ms': {k: round(v, 3) for k, v in med.items()},
           'witnesses_per_s': {k: round(B / v * 1e3) for k, v in med.items()}, 'recover_over_screen_walk': round(med['recover'] / med['screen_walk'], 3),
           'spread_ms': {k: round(max(v) - min(v), 3) for k, v in ms.items()}, 'families_ms': fam}
    e.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(json.dumps({k: doc[k] for k in ('median_ms', 'witnesses_per_s', 'recover_over_screen_walk', 'families_ms')}))
    print('wrote', a.out)


if __name__ == '__main__':
    main()
