#!/usr/bin/env python3
"""Latency of the key recovery, one witness per call (zk_recover_batch / zk_recover_batch_device), cooperating waves against one lane, beside the screen's
walk path (per-key tables off) in the same process.

    python tools/recover_latency.py [--out profiles/recover_latency.json] [--calls 50] [--repeats 3]

A child process per variant -- the library as built, and with ZKATTEST_ONE_LANE_CHAINS set --, alternating, --repeats times each: ring of 256 keys, one
valid witness, host and _device forms of recover and of the screen; 10 calls of warm-up, the median wall time of --calls calls, then 20 calls under
zk_ctx_set_timing(1) for the families of zk_last_timing."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NKEYS, SEED = 256, 20261019


def child(calls):
    import torch   # first: one HIP runtime in the process (tests/conftest.py)
    sys.path.insert(0, ROOT)
    import zkp_ecdsa_amd as Z
    e = Z.Engine(0)
    e.set_key_tables(0)
    e.set_params(*e.synth_params(SEED), 20)
    ring, msg, sig, pk, which, _ = e.synth_workload(SEED, NKEYS, 8)
    e.set_ring(ring, NKEYS)
    m, s, p = msg[32 * 3:32 * 4], sig[64 * 3:64 * 4], pk[64 * 3:64 * 4]
    dev = 'cuda:0'
    dm, ds, dp = (torch.frombuffer(bytearray(x), dtype=torch.uint8).to(dev) for x in (m, s, p))
    dwo, dfl, dpk = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(64, dtype=torch.uint8, device=dev)
    forms = {('recover', 'host'): lambda: e.recover_batch(m, s), ('recover', 'device'): lambda: e.recover_batch_device(1, dm.data_ptr(), ds.data_ptr(), dpk.data_ptr(), dwo.data_ptr(), dfl.data_ptr()),
             ('screen_walk', 'host'): lambda: e.screen_batch(m, s, p), ('screen_walk', 'device'): lambda: e.screen_batch_device(1, dm.data_ptr(), ds.data_ptr(), dp.data_ptr(), None, dwo.data_ptr(), dfl.data_ptr())}
    assert e.recover_batch(m, s) == ([p], [which[3]], [0]) and e.screen_batch(m, s, p) == ([which[3]], [0])
    c0 = e.test_counter(4)
    rows = []
    for (what, form), call in forms.items():
        e.set_timing(0)
        for _ in range(10):
            call()
        t = []
        for _ in range(calls):
            t0 = time.perf_counter()
            call()
            t.append((time.perf_counter() - t0) * 1e6)
        e.set_timing(1)
        fams = {}
        for _ in range(20):
            call()
            for k, v in e.last_timing()[1].items():
                fams.setdefault(k, []).append(v * 1e3)
        rows.append({'what': what, 'form': form, 'median_us': round(statistics.median(t), 2), 'min_us': round(min(t), 2),
                     'families_us': {k: round(statistics.median(v), 2) for k, v in fams.items()}})
    coop = e.test_counter(4) - c0
    name = torch.cuda.get_device_name(0)
    e.close()
    print(json.dumps({'lib': Z.LIB_PATH, 'device': name, 'coop_chains': coop, 'rows': rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'recover_latency.json'))
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--child', action='store_true')
    a = ap.parse_args()
    if a.child:
        return child(a.calls)
    runs, device = [], None
    for rep in range(a.repeats):
        for variant, extra in (('as_built', {}), ('one_lane', {'ZKATTEST_ONE_LANE_CHAINS': '1'})):
            env = {k: v for k, v in os.environ.items() if k != 'ZKATTEST_ONE_LANE_CHAINS'}
            env.update(extra)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--calls', str(a.calls)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
            if out.returncode != 0:
                raise SystemExit('child %s failed (%d): %s' % (variant, out.returncode, out.stderr.decode()[-2000:]))
            r = json.loads(out.stdout.decode().strip().splitlines()[-1])
            device = r['device']
            assert (r['coop_chains'] > 0) == (variant == 'as_built'), (variant, r['coop_chains'])
            runs.append({'variant': variant, 'repeat': rep, 'rows': r['rows']})
            print('%-8s run %d: %s' % (variant, rep, ' '.join('%s/%s %.0f' % (x['what'], x['form'][0], x['median_us']) for x in r['rows'])), flush=True)
    summary = []
    for variant in ('as_built', 'one_lane'):
        for form in ('host', 'device'):
            def med(what):
                return [x['median_us'] for r in runs if r['variant'] == variant for x in r['rows'] if x['what'] == what and x['form'] == form]
            rec, scr = med('recover'), med('screen_walk')
            summary.append({'variant': variant, 'form': form, 'recover_us': rec, 'screen_walk_us': scr, 'recover_mean_us': round(statistics.mean(rec), 2),
                            'screen_walk_mean_us': round(statistics.mean(scr), 2), 'recover_over_screen_walk': round(statistics.mean(rec) / statistics.mean(scr), 3),
                            'recover_spread_us': round(max(rec) - min(rec), 2)})
    doc = {'tool': 'tools/recover_latency.py', 'device': device, 'ring_keys': NKEYS, 'sec_level': 20, 'calls_per_median': a.calls, 'repeats': a.repeats,
           'note': 'wall time of one blocking call of ONE witness in microseconds, median of calls_per_median calls after 10 of warm-up, one value per repeated child process; '
                   'screen_walk: zk_screen_batch on the same context (per-key tables off)', 'summary': summary, 'runs': runs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(json.dumps(summary))
    print('wrote', a.out)


if __name__ == '__main__':
    main()
