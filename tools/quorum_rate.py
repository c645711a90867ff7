"""Quorum proofs (include/zkattest.h: zk_quorum_prove_batch / zk_quorum_verify_batch), measured beside the recipe they replace (INTEGRATION.md "Counting
signers"): device-resident buffers, a ring of --ring keys (2^16), secLevel 80, --comb-bits combs (24); per shape (k, Q) rounds of one-call prove / recipe prove
/ one-call verify / recipe verify alternating in one process.  The recipe's calls are zk_prove_batch_device, zk_prove_key_blinders_device,
zk_proof_key_commitments_device and zk_distinct_prove_batch_device (verifier: zk_verify_batch_device, zk_proof_key_commitments_device,
zk_distinct_verify_batch_device and an AND on the host); its pair arrays are built on the HOST between the calls, as a user builds them today, and that part
is timed on its own ("host_pairs_ms": the copies out, the gathers, the copies in).

Recorded per shape and side: both wall times (median, min, max over --reps rounds behind one warm-up round), the ratio one-call / recipe (of the medians, and
each round's own: median, min, max), and the GPU time of the one-call form's families (zk_last_timing), the new kernels among them under "quorum_*".  No
ratio is fixed in advance; from the code alone it should be near 1 on GPU time.
  python tools/quorum_rate.py [--shapes 4x16384,8x8192] [--ring 65536] [--comb-bits 24] [--reps 5] [--out profiles/quorum_rate.json]
Prints one JSON line (also written to --out PATH when given)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAIR = 744


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='4x16384,8x8192', help='k x Q, comma separated')
    ap.add_argument('--ring', type=int, default=65536)
    ap.add_argument('--comb-bits', type=int, default=24)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    import zkp_ecdsa_amd as Z
    S, dev = 20261021, 'cuda:0'
    shapes = [tuple(int(v) for v in s.split('x')) for s in args.shapes.split(',')]
    res = {'tool': 'quorum_rate', 'ring': args.ring, 'sec': 80, 'comb_bits': args.comb_bits, 'reps': args.reps, 'shapes': {}}
    e = Z.Engine(0)
    e.set_timing(1)
    e.set_comb_bits(args.comb_bits)
    e.set_params(*e.synth_params(S), 80)
    n_max = max(k * Q for k, Q in shapes)
    assert n_max <= args.ring, 'one witness per ring member: Q k <= the ring'
    ring, msg, sig, pk, which, seeds = e.synth_workload(S, args.ring, n_max)   # witness b is signed by ring member b: every quorum's members differ
    e.set_ring(ring, args.ring)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    p = lambda t: t.data_ptr()
    d_msg, d_sig, d_pk, d_seeds = up(msg), up(sig), up(pk), up(seeds)
    d_which = torch.tensor(which, dtype=torch.int32, device=dev)
    pmax = e.proof_max_size()
    for k, Q in shapes:
        n, P = k * Q, k * (k - 1) // 2
        NP = Q * P
        d_pseeds = up(os.urandom(32 * NP))
        cap_q, cap_a = e.quorum_proof_max_size(k) * Q, pmax * n
        d_bundles, d_boff = torch.empty(cap_q, dtype=torch.uint8, device=dev), torch.zeros(Q + 1, dtype=torch.int64, device=dev)
        d_qst, d_mst = torch.ones(Q, dtype=torch.int32, device=dev), torch.ones(n, dtype=torch.int32, device=dev)
        d_qok, d_bad = torch.zeros(Q, dtype=torch.uint8, device=dev), torch.zeros(Q, dtype=torch.int32, device=dev)
        d_att, d_aoff, d_ast = torch.empty(cap_a, dtype=torch.uint8, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.ones(n, dtype=torch.int32, device=dev)
        d_bl, d_com, d_kst = torch.empty(32 * n, dtype=torch.uint8, device=dev), torch.empty(72 * n, dtype=torch.uint8, device=dev), torch.ones(n, dtype=torch.int32, device=dev)
        d_pairs, d_pst = torch.empty(PAIR * NP, dtype=torch.uint8, device=dev), torch.ones(NP, dtype=torch.int32, device=dev)
        d_aok, d_pok = torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(NP, dtype=torch.uint8, device=dev)
        pairs = Z.Engine.distinct_pairs(k)
        first = (np.arange(Q)[:, None] * k + np.array([i for i, _ in pairs])[None, :]).reshape(-1)
        second = (np.arange(Q)[:, None] * k + np.array([j for _, j in pairs])[None, :]).reshape(-1)
        host_ms = {}

        def one_prove():
            e.quorum_prove_batch_device(Q, k, p(d_msg), p(d_sig), p(d_pk), p(d_which), p(d_seeds), p(d_pseeds), p(d_bundles), cap_q, p(d_boff), p(d_qst), p(d_mst))

        def one_verify():
            e.quorum_verify_batch_device(Q, k, p(d_msg), p(d_bundles), p(d_boff), None, p(d_qok), p(d_qst), p(d_bad))

        def gather(t, width, idx):   # device rows -> host -> the pairs' rows -> device: what a user of the recipe does between its calls
            return torch.from_numpy(t.cpu().numpy().reshape(-1, width)[idx].reshape(-1)).to(dev)

        def recipe_prove():
            e.prove_batch_device(n, p(d_msg), p(d_sig), p(d_pk), p(d_which), p(d_seeds), p(d_att), cap_a, p(d_aoff), p(d_ast))
            e.prove_key_blinders_device(n, p(d_seeds), p(d_bl))
            e.proof_key_commitments_device(n, p(d_att), p(d_aoff), p(d_com), p(d_kst))
            t0 = time.perf_counter()
            key = d_pk.cpu().numpy().reshape(-1, 64)[:n, :32]
            six = [torch.from_numpy(np.ascontiguousarray(key[first]).reshape(-1)).to(dev), gather(d_com, 72, first), gather(d_bl, 32, first),
                   torch.from_numpy(np.ascontiguousarray(key[second]).reshape(-1)).to(dev), gather(d_com, 72, second), gather(d_bl, 32, second)]
            torch.cuda.synchronize()
            host_ms['prove'] = (time.perf_counter() - t0) * 1e3
            e.distinct_prove_batch_device(NP, *[p(t) for t in six], p(d_pseeds), p(d_pairs), PAIR * NP, p(d_pst))

        def recipe_verify():
            e.verify_batch_device(n, p(d_msg), p(d_att), p(d_aoff), None, p(d_aok), p(d_ast))
            e.proof_key_commitments_device(n, p(d_att), p(d_aoff), p(d_com), p(d_kst))
            t0 = time.perf_counter()
            c1, c2 = gather(d_com, 72, first), gather(d_com, 72, second)
            torch.cuda.synchronize()
            host_ms['verify'] = (time.perf_counter() - t0) * 1e3
            e.distinct_verify_batch_device(NP, p(c1), p(c2), p(d_pairs), p(d_pok), p(d_pst))
            t0 = time.perf_counter()
            ok = d_aok.cpu().numpy().reshape(Q, k).all(axis=1) & d_pok.cpu().numpy().reshape(Q, P).all(axis=1)
            host_ms['verify'] += (time.perf_counter() - t0) * 1e3
            return ok

        calls = (('one_call_prove', one_prove), ('recipe_prove', recipe_prove), ('one_call_verify', one_verify), ('recipe_verify', recipe_verify))
        rec = {name: {'wall': [], 'fam': [], 'host': []} for name, _ in calls}
        for rep in range(args.reps + 1):
            for name, call in calls:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = call()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) * 1e3
                if rep >= 1:
                    rec[name]['wall'].append(wall)
                    if name.startswith('one_call'):
                        rec[name]['fam'].append(e.last_timing()[1])
                    else:
                        rec[name]['host'].append(host_ms[name.split('_')[1]])
        assert int(d_qok.sum()) == Q and int(d_qst.abs().sum()) == 0 and bool(out.all()), 'a verifier rejected an honest quorum'
        total = int(d_boff[Q])
        assert total == 16 * Q + int(d_aoff[n]) + PAIR * NP, 'the bundles are not the recipe\'s bytes long'

        def summary(r, fams=False):
            w = r['wall']
            s = {'ms': round(statistics.median(w), 3), 'min_ms': round(min(w), 3), 'max_ms': round(max(w), 3), 'spread': round((max(w) - min(w)) / statistics.median(w), 4)}
            if fams:
                keys = sorted(set().union(*r['fam']))
                s['families_ms'] = {f: round(statistics.median(x.get(f, 0.0) for x in r['fam']), 4) for f in keys}
                s['new_kernels_ms'] = round(sum(v for f, v in s['families_ms'].items() if f.startswith('quorum_')), 4)
            else:
                s['host_pairs_ms'] = round(statistics.median(r['host']), 3)
                s['ms_without_host_pairs'] = round(statistics.median(a - b for a, b in zip(w, r['host'])), 3)
            return s

        def ratio(side):
            a, b = rec['one_call_' + side], rec['recipe_' + side]
            per = [x / y for x, y in zip(a['wall'], b['wall'])]
            dev_only = [x / (y - h) for x, y, h in zip(a['wall'], b['wall'], b['host'])]
            return {'of_medians': round(statistics.median(a['wall']) / statistics.median(b['wall']), 4), 'per_round_median': round(statistics.median(per), 4),
                    'per_round_min': round(min(per), 4), 'per_round_max': round(max(per), 4), 'against_recipe_without_host_pairs': round(statistics.median(dev_only), 4)}

        res['shapes']['k%d_Q%d' % (k, Q)] = {'attestations': n, 'pairs': NP, 'bundle_bytes': total,
                                             'one_call_prove': summary(rec['one_call_prove'], True), 'recipe_prove': summary(rec['recipe_prove']),
                                             'one_call_verify': summary(rec['one_call_verify'], True), 'recipe_verify': summary(rec['recipe_verify']),
                                             'ratio_one_call_over_recipe': {'prove': ratio('prove'), 'verify': ratio('verify')}}
        del d_bundles, d_att, d_pairs
        torch.cuda.empty_cache()
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
