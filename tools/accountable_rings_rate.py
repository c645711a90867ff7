"""Accountable attestations over several rings (include/zkattest_rings_accountable.h: zk_rings_accountable_prove_batch / _verify_batch / _open_batch), measured
beside what a user of a sharded registry does without them: --proofs device-resident bundles (65 536) interleaved over two resident rings of --ring-a and
--ring-b keys (2^16 and 2^12), secLevel 80, --comb-bits combs (24).  The yardstick for prove and verify is the same rows GROUPED by ring (the groups are laid
out before the clock starts) through use_ring + zk_accountable_prove_batch_device / zk_accountable_verify_batch_device per ring; for the open it is
zk_accountable_split_batch_device + zk_rings_escrow_open_batch_device on the same mixed bundles.  Rounds of rings prove / grouped prove / rings verify /
grouped verify / rings open / split + open alternate in one process.

Recorded per side: wall times (median, min, max over --reps rounds behind one warm-up round), the ratio rings / yardstick (of the medians, and each round's own:
median, min, max), the yardstick's own round-to-round spread, and the GPU time of the rings forms' families (zk_last_timing), the kernels of their own among
them under "accountable_*".  No ratio is fixed in advance.  Then the latency of ONE bundle: the three rings calls with B = 1, host-pointer forms, median of
--latency-reps calls, beside the one-ring forms with that ring active.
  python tools/accountable_rings_rate.py [--proofs 65536] [--ring-a 65536] [--ring-b 4096] [--comb-bits 24] [--reps 3] [--out profiles/accountable_rings_rate.json]
Prints one JSON line (also written to --out PATH when given).  Run it under a time limit (timeout 900 python tools/accountable_rings_rate.py ...)."""
import argparse
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAG = 472


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--proofs', type=int, default=65536)
    ap.add_argument('--ring-a', type=int, default=65536)
    ap.add_argument('--ring-b', type=int, default=4096)
    ap.add_argument('--comb-bits', type=int, default=24)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--latency-reps', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    import zkp_ecdsa_amd as Z
    S, dev, B = 20261021, 'cuda:0', args.proofs
    assert B % 2 == 0, 'the bundles alternate between the two rings'
    h = B // 2
    res = {'tool': 'accountable_rings_rate', 'proofs': B, 'ring_a': args.ring_a, 'ring_b': args.ring_b, 'sec': 80, 'comb_bits': args.comb_bits, 'reps': args.reps}
    e = Z.Engine(0)
    e.set_timing(1)
    e.set_comb_bits(args.comb_bits)
    e.set_params(*e.synth_params(S), 80)
    def workload(seed, nkeys):   # (ring, msg, sig, pk, which, seeds) for h bundles: one witness per ring member, the same witnesses again under fresh seeds beyond that
        n = min(h, nkeys)
        assert h % n == 0, 'half the bundles are a multiple of the smaller ring'
        ring, msg, sig, pk, which, seeds = e.synth_workload(seed, nkeys, n)
        k = h // n
        return ring, msg * k, sig * k, pk * k, which * k, seeds + os.urandom(32 * (h - n))
    wl = [workload(S, args.ring_a), workload(S + 1, args.ring_b)]
    ids = [e.add_ring(wl[0][0], args.ring_a), e.add_ring(wl[1][0], args.ring_b)]
    secret = bytes(31) + b'\x07'
    e.set_auditor(e.escrow_keygen(secret))
    rows = lambda i, w: [np.frombuffer(wl[r][i], dtype=np.uint8).reshape(h, w) for r in (0, 1)]
    mixed = lambda i, w: np.stack(rows(i, w), axis=1).reshape(-1)          # bundle 2 j: ring A's witness j; bundle 2 j + 1: ring B's
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    p = lambda t: t.data_ptr()
    tseeds = np.frombuffer(os.urandom(32 * B), dtype=np.uint8).reshape(h, 2, 32)
    which_m = np.stack([np.array(wl[r][4], dtype=np.uint32) for r in (0, 1)], axis=1).reshape(-1)
    ids_m = np.tile(np.array(ids, dtype=np.uint32), h)
    M = {'msg': up(mixed(1, 32)), 'sig': up(mixed(2, 64)), 'pk': up(mixed(3, 64)), 'seeds': up(mixed(5, 32)), 'tseeds': up(tseeds.reshape(-1)),
         'which': up(which_m.view(np.uint8)), 'ids': up(ids_m.view(np.uint8)), 'any': up(np.full(B, 0xFFFFFFFF, dtype=np.uint32).view(np.uint8))}
    G = [{'msg': up(rows(1, 32)[r]), 'sig': up(rows(2, 64)[r]), 'pk': up(rows(3, 64)[r]), 'seeds': up(rows(5, 32)[r]), 'tseeds': up(tseeds[:, r, :]),
          'which': up(np.array(wl[r][4], dtype=np.uint32).view(np.uint8))} for r in (0, 1)]
    size = [e.ring_accountable_proof_max_size(i) for i in ids]
    cap_m, cap_g = h * (size[0] + size[1]), [h * size[0], h * size[1]]
    new = lambda n, dt=torch.uint8: torch.zeros(n, dtype=dt, device=dev)
    d_bundles, d_boff, d_st, d_pst = torch.empty(cap_m, dtype=torch.uint8, device=dev), new(B + 1, torch.int64), new(B, torch.int32), new(2 * B, torch.int32)
    d_ok, d_bad = new(B), new(B, torch.int32)
    d_ring, d_idx, d_ost = new(B, torch.int32), new(B, torch.int32), new(B, torch.int32)
    g_out = [torch.empty(cap_g[r], dtype=torch.uint8, device=dev) for r in (0, 1)]
    g_off, g_st, g_ok, g_bad = [new(h + 1, torch.int64) for _ in (0, 1)], [new(h, torch.int32) for _ in (0, 1)], [new(h) for _ in (0, 1)], [new(h, torch.int32) for _ in (0, 1)]
    s_att, s_aoff, s_tags, s_st = torch.empty(cap_m, dtype=torch.uint8, device=dev), new(B + 1, torch.int64), new(TAG * B), new(B, torch.int32)
    s_ring, s_idx, s_ost = new(B, torch.int32), new(B, torch.int32), new(B, torch.int32)
    d_secret = up(np.frombuffer(secret, dtype=np.uint8))

    def families():
        import ctypes as C
        total, names, ms = C.c_float(), (C.c_char_p * 64)(), (C.c_float * 64)()
        n = e.L.zk_last_timing(e.h, C.byref(total), names, ms, 64)
        return {names[i].decode(): ms[i] for i in range(min(n, 64))}

    def rings_prove():
        e.accountable_prove_batch_rings_device(B, p(M['msg']), p(M['sig']), p(M['pk']), p(M['which']), p(M['ids']), p(M['seeds']), p(M['tseeds']), p(d_bundles), cap_m, p(d_boff),
                                               p(d_st), p(d_pst))

    def grouped_prove():
        for r in (0, 1):
            e.use_ring(ids[r])
            e.accountable_prove_batch_device(h, p(G[r]['msg']), p(G[r]['sig']), p(G[r]['pk']), p(G[r]['which']), p(G[r]['seeds']), p(G[r]['tseeds']), p(g_out[r]), cap_g[r],
                                             p(g_off[r]), p(g_st[r]), None)

    def rings_verify():
        e.accountable_verify_batch_rings_device(B, p(M['msg']), p(d_bundles), p(d_boff), p(M['ids']), None, p(d_ok), p(d_st), p(d_bad))

    def grouped_verify():
        for r in (0, 1):
            e.use_ring(ids[r])
            e.accountable_verify_batch_device(h, p(G[r]['msg']), p(g_out[r]), p(g_off[r]), None, p(g_ok[r]), p(g_st[r]), p(g_bad[r]))

    def rings_open():
        e.accountable_open_batch_rings_device(B, p(d_secret), p(d_bundles), p(d_boff), p(M['ids']), p(d_ring), p(d_idx), p(d_ost))

    def split_open():
        e.accountable_split_device(B, p(d_bundles), p(d_boff), p(s_att), cap_m, p(s_aoff), p(s_tags), p(s_st))
        e.escrow_open_batch_rings_device(B, p(d_secret), p(s_tags), p(M['ids']), p(s_ring), p(s_idx), p(s_ost))

    calls = (('rings_prove', rings_prove), ('grouped_prove', grouped_prove), ('rings_verify', rings_verify), ('grouped_verify', grouped_verify),
             ('rings_open', rings_open), ('split_open', split_open))
    rec = {name: {'wall': [], 'fam': []} for name, _ in calls}
    for rep in range(args.reps + 1):
        for name, call in calls:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            if rep >= 1:
                rec[name]['wall'].append(wall)
                if name.startswith('rings_'):
                    rec[name]['fam'].append(families())
    def tally(t, step=2):   # status -> count, per ring of the interleaved batch
        a = t.cpu().numpy()
        return [{int(v): int(c) for v, c in zip(*np.unique(a[r::step], return_counts=True))} for r in range(step)]
    state = {'part_status': [tally(d_pst[0::2]), tally(d_pst[1::2])], 'verify_status': tally(d_st), 'ok': tally(d_ok), 'first_bad': tally(d_bad),
             'grouped_status': [tally(g_st[r], 1) for r in (0, 1)]}
    assert int(d_ok.sum()) == B and int(d_st.abs().sum()) == 0 and int(d_pst.abs().sum()) == 0, 'the rings verifier rejected an honest bundle: %s' % json.dumps(state)
    assert all(int(g_ok[r].sum()) == h and int(g_st[r].abs().sum()) == 0 for r in (0, 1)), 'the grouped verifier rejected an honest bundle'
    assert int(d_ost.abs().sum()) == 0 and torch.equal(d_ring, s_ring) and torch.equal(d_idx, s_idx) and torch.equal(d_ost, s_ost), 'the two openings differ'
    assert np.array_equal(d_ring.cpu().numpy().view(np.uint32), ids_m), 'a bundle opened to another ring'
    assert np.array_equal(d_idx.cpu().numpy().view(np.uint32), which_m), 'a bundle opened to another member'
    total = int(d_boff[B])
    assert total == int(g_off[0][h]) + int(g_off[1][h]), 'the mixed bundles are not as long as the grouped ones'

    def summary(r, fams=False):
        w = r['wall']
        s = {'ms': round(statistics.median(w), 3), 'min_ms': round(min(w), 3), 'max_ms': round(max(w), 3), 'spread': round((max(w) - min(w)) / statistics.median(w), 4)}
        if fams:
            keys = sorted(set().union(*r['fam']))
            s['families_ms'] = {f: round(statistics.median(x.get(f, 0.0) for x in r['fam']), 4) for f in keys}
            s['own_kernels_ms'] = round(sum(v for f, v in s['families_ms'].items() if f.startswith('accountable_')), 4)
        return s

    def ratio(a, b):
        per = [x / y for x, y in zip(rec[a]['wall'], rec[b]['wall'])]
        return {'of_medians': round(statistics.median(rec[a]['wall']) / statistics.median(rec[b]['wall']), 4), 'per_round_median': round(statistics.median(per), 4),
                'per_round_min': round(min(per), 4), 'per_round_max': round(max(per), 4)}

    res['bundle_bytes'] = total
    for name, _ in calls:
        res[name] = summary(rec[name], name.startswith('rings_'))
    res['ratio_rings_over_yardstick'] = {'prove': ratio('rings_prove', 'grouped_prove'), 'verify': ratio('rings_verify', 'grouped_verify'),
                                         'open': ratio('rings_open', 'split_open')}
    del d_bundles, s_att, g_out
    torch.cuda.empty_cache()

    # one bundle, host-pointer forms: the rings calls with no ring active beside the one-ring calls with ring A active
    e.set_timing(0)
    w1 = (wl[0][1][:32], wl[0][2][:64], wl[0][3][:64], wl[0][4][:1])
    names = ('rings_prove', 'one_ring_prove', 'rings_verify', 'one_ring_verify', 'rings_open', 'split_open')
    lat = {n: [] for n in names}
    e.use_ring(ids[0])
    for rep in range(args.latency_reps + 2):
        sd, ts = wl[0][5][:32], os.urandom(32)
        t = [time.perf_counter()]
        bundle = e.accountable_prove_batch_rings(*w1, ids[:1], seeds=sd, tag_seeds=ts)[0]
        t.append(time.perf_counter())
        one = e.accountable_prove_batch(*w1, seeds=sd, tag_seeds=ts)[0]
        t.append(time.perf_counter())
        okr = e.accountable_verify_batch_rings(w1[0], bundle, ids[:1])[0]
        t.append(time.perf_counter())
        oko = e.accountable_verify_batch(w1[0], one)[0]
        t.append(time.perf_counter())
        opened = e.accountable_open_batch_rings(secret, bundle, ids[:1])
        t.append(time.perf_counter())
        _, tags, _ = e.accountable_split(bundle)
        opened2 = e.escrow_open_batch_rings(secret, tags, ids[:1])
        t.append(time.perf_counter())
        assert okr == [1] and oko == [1] and bundle == one and opened == opened2 == ([ids[0]], [w1[3][0]], [0])
        if rep >= 2:
            for i, n in enumerate(names):
                lat[n].append((t[i + 1] - t[i]) * 1e3)
    res['latency_one'] = {n: {'ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3)} for n, v in lat.items()}
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
