"""Opening escrow tags against any resident ring (include/zkattest.h: zk_rings_escrow_open_batch) beside the one-ring call zk_escrow_open_batch on the same
tags: --batch tags (65 536), every buffer device-resident, --comb-bits context combs (24), one process, the sides alternating round by round, the rings'
point indexes warm.

  (a) one id throughout, a ring of 2^16 keys, against zk_escrow_open_batch with that ring active;
  (b) tags interleaved over rings of 2^16 and 2^12 keys, against zk_ctx_use_ring + zk_escrow_open_batch per ring on the same tags grouped by ring;
  (c) recorded, not gated: (a) at a ring of 2^--big-log keys (20).
Yardstick for (a) and (b): the new call's median is at most the old side's median plus the old side's own min-to-max spread in this file.
Also recorded: the GPU time of "escrow_lookup" and of "escrow_index_build" (the first call per ring size), and zk_ctx_update_ring of 1, 16 and 256 keys of the
2^16 ring with a point index present against the same context before its first open call.
  python tools/escrow_rings_rate.py [--batch 65536] [--comb-bits 24] [--reps 3] [--big-log 20] [--out profiles/escrow_rings_rate.json]
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
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--big-log', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    import zkp_ecdsa_amd as Z
    S, B, dev = 20261021, args.batch, 'cuda:0'
    res = {'tool': 'escrow_rings_rate', 'batch': B, 'comb_bits': args.comb_bits, 'reps': args.reps, 'tag_bytes': 472}

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def sc(t, i):
        return int.from_bytes(hashlib.sha256(b'escrow-rings-rate' + t + i.to_bytes(4, 'big')).digest(), 'big') % Q

    be = lambda v: b''.join(i.to_bytes(32, 'big') for i in v)
    p = lambda t: t.data_ptr()
    e = Z.Engine(0)
    e.set_timing(1)
    e.set_key_tables(0)   # the auditor's context proves nothing: no per-key tables beside rings of this size
    e.set_comb_bits(args.comb_bits)
    e.set_params(*e.synth_params(S), 80)
    a32 = hashlib.sha256(b'escrow-rings-rate-auditor').digest()
    e.set_auditor(e.escrow_keygen(a32))
    d_a = up(a32)
    sizes = {'2^16': 1 << 16, '2^12': 1 << 12, 'big': 1 << args.big_log}
    rings = {k: [sc(k.encode(), i) for i in range(n)] for k, n in sizes.items()}
    d_st, d_idx, d_ring = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))

    def tags_for(keys):
        n = len(keys)
        r = [sc(b'r', i) for i in range(n)]
        c = e.test_tom_commit(keys, r)
        d_t = torch.empty(472 * n, dtype=torch.uint8, device=dev)
        seeds = up(b''.join(hashlib.sha256(b'escrow-rings-rate-seed' + i.to_bytes(4, 'big')).digest() for i in range(n)))
        d_k, d_c, d_r = up(be(keys)), up(b''.join(c)), up(be(r))
        e.escrow_prove_batch_device(n, p(d_k), p(d_c), p(d_r), p(seeds), p(d_t), 472 * n, p(d_st))
        torch.cuda.synchronize()
        assert int(d_st[:n].abs().sum()) == 0
        return d_t

    def summary(walls, fams):
        med = statistics.median(walls)
        keys = sorted(set().union(*fams))
        return {'ms': round(med, 4), 'min_ms': round(min(walls), 4), 'max_ms': round(max(walls), 4), 'per_s': round(B / med * 1e3),
                'families_ms': {k: round(statistics.median(f.get(k, 0.0) for f in fams), 4) for k in keys}}

    def compare(new, old):
        """alternating rounds behind one warm-up round -> {'new', 'old', yardstick}"""
        rec = {'new': ([], []), 'old': ([], [])}
        for rep in range(args.reps + 1):
            for name, call in (('new', new), ('old', old)):
                t0 = time.perf_counter()
                fam = call()
                wall = (time.perf_counter() - t0) * 1e3
                if rep >= 1:
                    rec[name][0].append(wall), rec[name][1].append(fam)
        out = {k: summary(*v) for k, v in rec.items()}
        out['bound_ms'] = round(out['old']['ms'] + out['old']['max_ms'] - out['old']['min_ms'], 4)
        out['yardstick_met'] = out['new']['ms'] <= out['bound_ms']
        return out

    # ---- zk_ctx_update_ring before the ring's first open call (no index), then the first calls (the builds), then the same updates with an index present
    ids = {}
    ids['2^16'] = e.add_ring(be(rings['2^16']), sizes['2^16'])

    def update_times():
        out = {}
        for k in (1, 16, 256):
            walls = []
            for rep in range(args.reps + 1):
                ch = {(7919 * j + rep) % sizes['2^16']: sc(b'upd%d' % rep, j).to_bytes(32, 'big') for j in range(k)}
                t0 = time.perf_counter()
                e.update_ring(ids['2^16'], ch)
                walls.append((time.perf_counter() - t0) * 1e3)
                e.update_ring(ids['2^16'], {i: rings['2^16'][i].to_bytes(32, 'big') for i in ch})   # (back to the measured list)
            out[str(k)] = {'ms': round(statistics.median(walls[1:]), 4), 'min_ms': round(min(walls[1:]), 4), 'max_ms': round(max(walls[1:]), 4)}
        return out

    res['update_ring_ms'] = {'no_index': update_times()}
    which = {k: [(2654435761 * i) % n for i in range(B)] for k, n in sizes.items()}
    d_tags = {k: tags_for([rings[k][w] for w in which[k]]) for k in ('2^16', 'big')}
    res['index_build_ms'] = {}
    for k in ('2^16', '2^12', 'big'):
        if k not in ids:
            ids[k] = e.add_ring(be(rings[k]), sizes[k])
        d_ids = up(np.full(1, ids[k], dtype=np.uint32).tobytes())
        t0 = time.perf_counter()
        e.escrow_open_batch_rings_device(1, p(d_a), p(d_tags['2^16']), p(d_ids), p(d_ring), p(d_idx), p(d_st))
        res['index_build_ms'][k] = {'keys': sizes[k], 'gpu_ms': round(e.last_timing()[1].get('escrow_index_build', 0.0), 4), 'first_call_wall_ms': round((time.perf_counter() - t0) * 1e3, 4)}
    res['update_ring_ms']['index_present'] = update_times()

    def new_call(d_t, d_ids, want_ring, want_idx):
        def run():
            e.escrow_open_batch_rings_device(B, p(d_a), p(d_t), p(d_ids), p(d_ring), p(d_idx), p(d_st))
            return e.last_timing()[1]
        run()
        torch.cuda.synchronize()
        assert int(d_st.abs().sum()) == 0 and d_idx.cpu().tolist() == want_idx and d_ring.cpu().tolist() == want_ring, 'a tag opened to another member than the planted one'
        return run

    def old_call(parts):
        """parts: (ring id, tags, count, offset into the outputs); the outputs are int32 tensors"""
        def run():
            fam = {}
            for rid, d_t, n, off in parts:
                e.use_ring(rid)
                e.escrow_open_batch_device(n, p(d_a), p(d_t), p(d_idx) + 4 * off, p(d_st) + 4 * off)
                for k, v in e.last_timing()[1].items():
                    fam[k] = fam.get(k, 0.0) + v
            return fam
        return run

    # (a), (c): one id throughout
    for name, k in (('a_one_ring_2^16', '2^16'), ('c_one_ring_big', 'big')):
        d_ids = up(np.full(B, ids[k], dtype=np.uint32).tobytes())
        old = old_call([(ids[k], d_tags[k], B, 0)])
        res[name] = compare(new_call(d_tags[k], d_ids, [ids[k]] * B, which[k]), old)
        res[name]['ring_keys'] = sizes[k]
        torch.cuda.synchronize()
        assert d_idx.cpu().tolist() == which[k]
    # (b): tags interleaved over the 2^16 and the 2^12 ring; the old side takes them grouped by ring
    h = B // 2
    mixed_keys, mixed_ids, mixed_idx = [], [], []
    for i in range(B):
        k = '2^16' if i % 2 == 0 else '2^12'
        w = which[k][i]
        mixed_keys.append(rings[k][w]), mixed_ids.append(ids[k]), mixed_idx.append(w)
    d_mixed = tags_for(mixed_keys)
    d_grp = {k: tags_for([mixed_keys[i] for i in range(s, B, 2)]) for s, k in ((0, '2^16'), (1, '2^12'))}
    new = new_call(d_mixed, up(np.array(mixed_ids, dtype=np.uint32).tobytes()), mixed_ids, mixed_idx)
    res['b_two_rings'] = compare(new, old_call([(ids['2^16'], d_grp['2^16'], h, 0), (ids['2^12'], d_grp['2^12'], B - h, h)]))
    torch.cuda.synchronize()
    assert d_idx.cpu().tolist() == mixed_idx[0::2] + mixed_idx[1::2]
    res['lookup_gpu_ms'] = {k: res[k]['new']['families_ms'].get('escrow_lookup', 0.0) for k in ('a_one_ring_2^16', 'b_two_rings', 'c_one_ring_big')}
    res['yardsticks_met'] = bool(res['a_one_ring_2^16']['yardstick_met'] and res['b_two_rings']['yardstick_met'])
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
