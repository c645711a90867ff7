#!/usr/bin/env python3
"""Latency of the witness screen (zk_screen_batch / zk_screen_batch_device) over the batch size, cooperative against one-lane point arithmetic.

    python tools/screen_latency.py [--out profiles/screen_latency.json] [--parent-lib PATH] [--calls 50] [--repeats 3]

Three kinds of witness: 'table' (a ring member, per-key tables on: the key-table path), 'walk' (the same member on a context without per-key tables: the
65-window walk) and 'non_member' (a valid signature by a key that is not in the ring, per-key tables on: the walk behind a lookup that finds nothing).
For every kind a child process sweeps B in {1, 2, 4, 16, 64, 256, 1024, 4096, 4097}, host form and _device form: 10 calls of warm-up, the median wall time
of --calls calls, then 20 calls under zk_ctx_set_timing(1) for the screen_lookup / screen_ecdsa split of zk_last_timing.  The children alternate between the
library as built and the same library with ZKATTEST_ONE_LANE_CHAINS set, --repeats times each, so that the spread between repeated runs of one variant is
known; with --parent-lib (the parent commit's libzkattest_hip.so, taken through ZKATTEST_LIB) the parent is measured at B = 1 and B = 4097 the same way.
The summary compares the variants per (kind, form, B): cooperation wins where the one-lane mean exceeds the cooperative mean by more than the spread of the
repeated one-lane runs.  Reads nothing but the built library."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP = [1, 2, 4, 16, 64, 256, 1024, 4096, 4097]
KINDS = {'table': (1, True), 'walk': (0, True), 'non_member': (1, False)}   # kind -> (per-key tables, ring member)
NKEYS, SEED = 256, 20261019


def child(kind, sizes, calls):
    os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
    import torch   # first: one HIP runtime in the process (tests/conftest.py)
    sys.path.insert(0, ROOT)
    import zkp_ecdsa_amd as Z
    kt, member = KINDS[kind]
    e = Z.Engine(0)
    e.set_key_tables(kt)
    e.set_params(*e.synth_params(SEED), 20)
    ring, msg, sig, pk, _, _ = e.synth_workload(SEED, NKEYS, 8)
    if not member:
        _, msg, sig, pk, _, _ = e.synth_workload(SEED + 1, NKEYS, 8)
    e.set_ring(ring, NKEYS)
    c0 = e.test_counter(4)
    rows = []
    for B in sizes:
        m, s, p = (b''.join(x[w * (i % 8):w * (i % 8) + w] for i in range(B)) for x, w in ((msg, 32), (sig, 64), (pk, 64)))
        dm, ds, dp = (torch.frombuffer(bytearray(x), dtype=torch.uint8).to('cuda:0') for x in (m, s, p))
        dwo, dfl = torch.zeros(B, dtype=torch.int32, device='cuda:0'), torch.zeros(B, dtype=torch.int32, device='cuda:0')
        forms = {'host': lambda: e.screen_batch(m, s, p),
                 'device': lambda: e.screen_batch_device(B, dm.data_ptr(), ds.data_ptr(), dp.data_ptr(), None, dwo.data_ptr(), dfl.data_ptr())}
        want = 0 if member else Z.SCREEN_NOT_IN_RING
        for form, call in forms.items():
            e.set_timing(0)
            for _ in range(10):
                res = call()
            flags = res[1] if form == 'host' else dfl.cpu().tolist()
            assert list(flags) == [want] * B, (kind, form, B, flags[:8])
            t = []
            for _ in range(calls):
                t0 = time.perf_counter()
                call()
                t.append((time.perf_counter() - t0) * 1e6)
            e.set_timing(1)
            lk, ec = [], []
            for _ in range(20):
                call()
                fam = e.last_timing()[1]
                lk.append(fam.get('screen_lookup', 0.0) * 1e3), ec.append(fam.get('screen_ecdsa', 0.0) * 1e3)
            rows.append({'B': B, 'form': form, 'median_us': round(statistics.median(t), 2), 'min_us': round(min(t), 2),
                         'screen_lookup_us': round(statistics.median(lk), 2), 'screen_ecdsa_us': round(statistics.median(ec), 2)})
    coop = e.test_counter(4) - c0
    name = torch.cuda.get_device_name(0)
    e.close()
    print(json.dumps({'kind': kind, 'lib': Z.LIB_PATH, 'device': name, 'coop_chains': coop, 'rows': rows}))


def run_child(kind, sizes, calls, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ('ZKATTEST_ONE_LANE_CHAINS', 'ZKATTEST_LIB')}
    env.update(env_extra)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', kind, '--sizes', ','.join(map(str, sizes)), '--calls', str(calls)], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if out.returncode != 0:
        raise SystemExit('child %s %s failed (%d): %s' % (kind, env_extra, out.returncode, out.stderr.decode()[-2000:]))
    return json.loads(out.stdout.decode().strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'screen_latency.json'))
    ap.add_argument('--parent-lib')
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--child')
    ap.add_argument('--sizes')
    a = ap.parse_args()
    if a.child:
        return child(a.child, [int(x) for x in a.sizes.split(',')], a.calls)
    assert a.calls >= 50 and a.repeats >= 2
    variants = [('as_built', {}, SWEEP), ('one_lane', {'ZKATTEST_ONE_LANE_CHAINS': '1'}, SWEEP)]
    if a.parent_lib:
        variants.append(('parent', {'ZKATTEST_LIB': os.path.abspath(a.parent_lib)}, [1, 4097]))
    runs, device = [], None
    for kind in KINDS:
        for rep in range(a.repeats):
            for variant, env, sizes in variants:   # alternating: as built, one lane, (parent), as built, ...
                r = run_child(kind, sizes, a.calls, env)
                device = r['device']
                assert (r['coop_chains'] > 0) == (variant == 'as_built'), (variant, r['coop_chains'])
                runs.append({'kind': kind, 'variant': variant, 'repeat': rep, 'rows': r['rows']})
                print('%-10s %-8s run %d: %s' % (kind, variant, rep, ' '.join('%s/%d %.0f' % (x['form'][0], x['B'], x['median_us']) for x in r['rows'])), flush=True)
    # per (kind, form, B): the medians of the repeated runs of every variant
    summary = []
    for kind in KINDS:
        for form in ('host', 'device'):
            for B in SWEEP:
                def med(variant, key='median_us'):
                    return [x[key] for r in runs if r['kind'] == kind and r['variant'] == variant for x in r['rows'] if x['form'] == form and x['B'] == B]
                co, one, par = med('as_built'), med('one_lane'), med('parent')
                spread = max(one) - min(one)
                row = {'kind': kind, 'form': form, 'B': B, 'as_built_us': co, 'one_lane_us': one, 'one_lane_spread_us': round(spread, 2),
                       'as_built_mean_us': round(statistics.mean(co), 2), 'one_lane_mean_us': round(statistics.mean(one), 2),
                       'as_built_ecdsa_us': round(statistics.mean(med('as_built', 'screen_ecdsa_us')), 2), 'one_lane_ecdsa_us': round(statistics.mean(med('one_lane', 'screen_ecdsa_us')), 2),
                       'as_built_lookup_us': round(statistics.mean(med('as_built', 'screen_lookup_us')), 2), 'one_lane_lookup_us': round(statistics.mean(med('one_lane', 'screen_lookup_us')), 2),
                       'as_built_faster_by_more_than_spread': statistics.mean(one) - statistics.mean(co) > spread}
                if par:
                    row['parent_us'], row['parent_mean_us'] = par, round(statistics.mean(par), 2)
                    row['parent_ecdsa_us'] = round(statistics.mean(med('parent', 'screen_ecdsa_us')), 2)
                summary.append(row)
    doc = {'tool': 'tools/screen_latency.py', 'device': device, 'ring_keys': NKEYS, 'sec_level': 20, 'calls_per_median': a.calls, 'repeats': a.repeats,
           'note': 'wall time of one blocking call in microseconds, median of calls_per_median calls after 10 of warm-up, one value per repeated child process; '
                   '*_ecdsa_us / *_lookup_us: zk_last_timing families under zk_ctx_set_timing(1), mean of the runs\' medians',
           'summary': summary, 'runs': runs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', a.out)


if __name__ == '__main__':
    main()
