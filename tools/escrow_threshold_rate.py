"""Threshold opening of escrow tags (include/zkattest.h: zk_auditors_share_batch / _share_verify_batch / _combine_batch) beside the single-auditor call
zk_rings_escrow_open_batch on the same tags: --batch tags (65 536), every buffer device-resident, --comb-bits context combs (24), a ring of 2^16 keys whose
point index is warm, (t, n) = (3, 5), one process, the four calls alternating round by round; medians of --reps rounds (3) behind one warm-up round, with
minimum and maximum.

Recorded: the share, share-verify and combine times, each as a ratio to the single-auditor call's median in this run, beside what the operation counts say
(a share: two masked ladders against one, 2.0; the combine: 256 doublings + about 128 t additions against 512 point operations, (256 + 128 t) / 512); the
one-tag latencies; the GPU time by family.  The one condition: zk_rings_escrow_open_batch itself is not slower than its median in --parent
(profiles/escrow_rings_rate.json, case a: the same setup on the commit before) by more than that side's own min-to-max spread there.
  python tools/escrow_threshold_rate.py [--batch 65536] [--comb-bits 24] [--reps 3] [--parent profiles/escrow_rings_rate.json] [--out profiles/escrow_threshold_rate.json]
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
T, N, SUBSET = 3, 5, [5, 2, 3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--comb-bits', type=int, default=24)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--parent', default=os.path.join(ROOT, 'profiles', 'escrow_rings_rate.json'))
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    import zkp_ecdsa_amd as Z
    S, B, dev = 20261021, args.batch, 'cuda:0'
    res = {'tool': 'escrow_threshold_rate', 'batch': B, 'comb_bits': args.comb_bits, 'reps': args.reps, 't': T, 'n': N, 'auditors': SUBSET, 'ring_keys': 1 << 16,
           'tag_bytes': 472, 'share_bytes': 264}

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def sc(t, i):
        return int.from_bytes(hashlib.sha256(b'escrow-threshold-rate' + t + i.to_bytes(4, 'big')).digest(), 'big') % Q

    be = lambda v: b''.join(i.to_bytes(32, 'big') for i in v)
    p = lambda t: t.data_ptr()
    e = Z.Engine(0)
    e.set_timing(1)
    e.set_key_tables(0)   # the auditors' context proves nothing: no per-key tables beside a ring of this size
    e.set_comb_bits(args.comb_bits)
    e.set_params(*e.synth_params(S), 80)
    a32 = hashlib.sha256(b'escrow-threshold-rate-auditor').digest()
    e.set_auditor(e.escrow_keygen(a32))
    shares, keys = e.auditors_split_key(a32, T, N, seed=hashlib.sha256(b'escrow-threshold-rate-split').digest())
    e.set_auditors(T, keys)
    ring = [sc(b'ring', i) for i in range(1 << 16)]
    rid = e.add_ring(be(ring), len(ring))
    which = [(2654435761 * i) % len(ring) for i in range(B)]
    d_st, d_idx, d_ring = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
    d_ok = torch.zeros(B, dtype=torch.uint8, device=dev)
    # the tags, from the engine's own prover
    r = [sc(b'r', i) for i in range(B)]
    tag_keys = [ring[w] for w in which]
    d_tags = torch.empty(472 * B, dtype=torch.uint8, device=dev)
    d_k, d_c, d_r = up(be(tag_keys)), up(b''.join(e.test_tom_commit(tag_keys, r))), up(be(r))
    e.escrow_prove_batch_device(B, p(d_k), p(d_c), p(d_r), p(up(b''.join(hashlib.sha256(b'tag-seed' + i.to_bytes(4, 'big')).digest() for i in range(B)))), p(d_tags), 472 * B, p(d_st))
    torch.cuda.synchronize()
    assert int(d_st.abs().sum()) == 0
    d_a, d_ids, d_aud = up(a32), up(np.full(B, rid, dtype=np.uint32).tobytes()), up(np.array(SUBSET, dtype=np.uint32).tobytes())
    d_sec = {j: up(shares[j - 1]) for j in SUBSET}
    d_seeds = {j: up(b''.join(hashlib.sha256(b'share-seed%d' % j + i.to_bytes(4, 'big')).digest() for i in range(B))) for j in SUBSET}
    d_shares = torch.empty(264 * B * T, dtype=torch.uint8, device=dev)   # slot-major: slot s belongs to SUBSET[s]

    def share(slot, n=B):
        j = SUBSET[slot]
        e.auditors_share_batch_device(n, j, p(d_sec[j]), p(d_tags), p(d_seeds[j]), p(d_shares) + 264 * B * slot, 264 * n, p(d_st))
        return e.last_timing()[1]

    def verify(slot, n=B):
        e.auditors_share_verify_batch_device(n, p(d_tags), p(d_shares) + 264 * B * slot, p(d_ok), p(d_st))
        return e.last_timing()[1]

    def combine():
        e.auditors_combine_batch_device(B, T, p(d_aud), p(d_tags), p(d_shares), p(d_ids), p(d_ring), p(d_idx), p(d_st))
        return e.last_timing()[1]

    def single(n=B):
        e.escrow_open_batch_rings_device(n, p(d_a), p(d_tags), p(d_ids), p(d_ring), p(d_idx), p(d_st))
        return e.last_timing()[1]

    # every slot's shares once (they stay for the combine), each call's answers checked, the ring's index built
    for slot in range(T):
        share(slot)
        torch.cuda.synchronize()
        assert int(d_st.abs().sum()) == 0
        verify(slot)
        torch.cuda.synchronize()
        assert int(d_st.abs().sum()) == 0 and int(d_ok.sum()) == B
    for call in (single, combine):
        d_idx.fill_(-1)
        call()
        torch.cuda.synchronize()
        assert int(d_st.abs().sum()) == 0 and d_idx.cpu().tolist() == which and d_ring.cpu().tolist() == [rid] * B, 'a tag opened to another member than the planted one'

    def summary(walls, fams, n):
        med = statistics.median(walls)
        names = sorted(set().union(*fams))
        return {'ms': round(med, 4), 'min_ms': round(min(walls), 4), 'max_ms': round(max(walls), 4), 'per_s': round(n / med * 1e3),
                'families_ms': {k: round(statistics.median(f.get(k, 0.0) for f in fams), 4) for k in names}}

    calls = (('single_auditor_open', single), ('share', lambda: share(0)), ('share_verify', lambda: verify(0)), ('combine', combine))
    rec = {name: ([], []) for name, _ in calls}
    for rep in range(args.reps + 1):   # alternating rounds behind one warm-up round
        for name, call in calls:
            t0 = time.perf_counter()
            fam = call()
            wall = (time.perf_counter() - t0) * 1e3
            if rep >= 1:
                rec[name][0].append(wall), rec[name][1].append(fam)
    for name, v in rec.items():
        res[name] = summary(*v, B)
    # one-tag latencies (the combine's shares of tag 0 lie B shares apart: its one-tag form takes a compact copy)
    d_one = torch.cat([d_shares[264 * B * s:264 * B * s + 264] for s in range(T)]).contiguous()
    def combine_one():
        e.auditors_combine_batch_device(1, T, p(d_aud), p(d_tags), p(d_one), p(d_ids), p(d_ring), p(d_idx), p(d_st))
        return e.last_timing()[1]
    res['one_tag_ms'] = {}
    for name, call in (('single_auditor_open', lambda: single(1)), ('share', lambda: share(0, 1)), ('share_verify', lambda: verify(0, 1)), ('combine', combine_one)):
        walls = []
        for rep in range(args.reps + 3):
            t0 = time.perf_counter()
            call()
            walls.append((time.perf_counter() - t0) * 1e3)
        res['one_tag_ms'][name] = {'ms': round(statistics.median(walls[1:]), 4), 'min_ms': round(min(walls[1:]), 4), 'max_ms': round(max(walls[1:]), 4)}
    base = res['single_auditor_open']['ms']
    counts = {'share': 2.0, 'share_verify': None, 'combine': (256 + 128 * T) / 512}
    res['ratio_to_single_auditor'] = {k: {'measured': round(res[k]['ms'] / base, 3), 'by_operation_counts': v,
                                          'beyond_1.5x_of_the_counts': bool(v and res[k]['ms'] / base > 1.5 * v)} for k, v in counts.items()}
    lad = res['single_auditor_open']['families_ms'].get('escrow_ladder', 0.0)
    res['gpu_ratio_to_escrow_ladder'] = {'share_ladder': round(res['share']['families_ms'].get('share_ladder', 0.0) / lad, 3) if lad else None,
                                         'combine_ladder': round(res['combine']['families_ms'].get('combine_ladder', 0.0) / lad, 3) if lad else None}
    # the one condition, against the same call and setup on the commit before
    parent = json.load(open(args.parent))['a_one_ring_2^16']['new']
    bound = parent['ms'] + parent['max_ms'] - parent['min_ms']
    res['single_auditor_condition'] = {'parent_file': os.path.relpath(args.parent, ROOT), 'parent_ms': parent['ms'], 'parent_min_ms': parent['min_ms'], 'parent_max_ms': parent['max_ms'],
                                       'bound_ms': round(bound, 4), 'ms': base, 'met': bool(base <= bound)}
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
