"""In-place ring updates (include/zkattest.h: zk_ctx_update_ring), measured: one context, one ring of --ring keys (2^16), key tables on.

Median host wall time of the C call over --reps repetitions of
  set_ring        zk_ctx_set_ring of the full list: the rebuild every change cost before (its code is what it was)
  update_K        zk_ctx_update_ring of K = 1, 16, 256, 4096 keys at seeded random positions
  key0_full       key 0 of the full ring (no padding entries)
  key0_padded     key 0 of a ring of --padded keys (40 000: 25 536 padding entries follow key 0, their key tables by copy)
  append_16       the last 16 keys appended to a ring of --ring - 16
and the work counters of each (zk_test_counter 5: per-key tables computed, 6: blocks of table E built).  After the timed calls the digest of the updated ring
is compared with the digest of a ring rebuilt from the same list.
  python tools/ring_update_rate.py [--ring 65536] [--padded 40000] [--reps 5] [--out profiles/ring_update_rate.json]
Prints one JSON line (also written to --out PATH when given)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ring', type=int, default=65536)
    ap.add_argument('--padded', type=int, default=40000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import zkp_ecdsa_amd as Z
    S, n = 20261016, args.ring
    rnd = random.Random(S)
    e = Z.Engine(0)
    e.set_params(*e.synth_params(S), 80)
    keys = [bytes(e.synth_workload(S, n, 4)[0])[32 * i:32 * i + 32] for i in range(n)]
    fresh_key = lambda: hashlib.sha256(b'ring_update_rate %d' % rnd.getrandbits(64)).digest()
    L = Z.lib()

    def timed_set(klist):
        blob = b''.join(klist)
        t0 = time.perf_counter()
        rc = L.zk_ctx_set_ring(e.h, blob, len(klist))
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        return dt

    def timed_update(klist, changes, new_n):
        """applies `changes` to the resident ring (id 0) and to klist; -> (seconds of the C call, counter 5 delta, counter 6 delta)"""
        idx = (C.c_uint64 * max(len(changes), 1))(*[i for i, _ in changes])
        blob = b''.join(k for _, k in changes)
        c5, c6 = e.test_counter(5), e.test_counter(6)
        t0 = time.perf_counter()
        rc = L.zk_ctx_update_ring(e.h, 0, len(changes), idx, blob, new_n)
        dt = time.perf_counter() - t0
        assert rc == 0, (rc, L.zk_last_error(e.h))
        del klist[new_n:]
        klist.extend([None] * (new_n - len(klist)))
        for i, k in changes:
            klist[i] = k
        return dt, e.test_counter(5) - c5, e.test_counter(6) - c6

    runs, work = {}, {}

    def record(name, r):
        runs.setdefault(name, []).append(r[0])
        work[name] = {'key_tables_computed': r[1], 'etab_blocks': r[2]}

    cur = list(keys)
    timed_set(cur)   # warm-up: the first build also creates the allocator's pools
    info = e.ring_info(0)
    assert info['flags'] & Z.RING_KEY_TABLES and info['flags'] & Z.RING_TABLE_E_DIGITS, info
    timed_update(cur, [(1, fresh_key())], n)   # ... and the update's kernels are loaded
    for rep in range(args.reps):
        runs.setdefault('set_ring', []).append(timed_set(cur))
        for K in (1, 16, 256, 4096):
            record('update_%d' % K, timed_update(cur, [(i, fresh_key()) for i in rnd.sample(range(n), K)], n))
        record('key0_full', timed_update(cur, [(0, fresh_key())], n))
    digest = e.ring_digest()
    timed_set(cur)
    assert e.ring_digest() == digest, 'the updated ring and the rebuilt ring differ'
    # 16-key append: the ring shrinks by 16 (not timed), then grows back
    for rep in range(args.reps):
        tail = cur[n - 16:]
        timed_update(cur, [], n - 16)
        record('append_16', timed_update(cur, [(n - 16 + i, k) for i, k in enumerate(tail)], n))
    assert e.ring_digest() == digest
    # key 0 of a ring with padding
    cur = list(keys[:args.padded])
    timed_set(cur)
    pad = (1 << e.ring_info(0)['log_n']) - args.padded
    for rep in range(args.reps):
        record('key0_padded', timed_update(cur, [(0, fresh_key())], args.padded))
    digest = e.ring_digest()
    timed_set(cur)
    assert e.ring_digest() == digest, 'the updated padded ring and the rebuilt ring differ'
    med = {k: statistics.median(v) * 1e3 for k, v in runs.items()}
    res = {
        'tool': 'ring_update_rate', 'ring': n, 'padded_ring': args.padded, 'padding_entries': pad, 'reps': args.reps,
        'ms_median': {k: round(v, 3) for k, v in med.items()},
        'ms_all': {k: [round(x * 1e3, 3) for x in v] for k, v in runs.items()},
        'work': work,
        'update_16_over_set_ring': round(med['update_16'] / med['set_ring'], 4),
        'expectation': {'update_16_over_set_ring': '< 0.125 (at most 16 of 256 blocks and 16 of 65 536 key tables: 1/16 of the work, x2 for launch latency and the one-lane root hash)'},
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    e.close()


if __name__ == '__main__':
    main()
