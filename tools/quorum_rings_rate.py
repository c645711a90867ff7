"""Quorum proofs over several rings (include/zkattest.h: zk_rings_quorum_prove_batch / zk_rings_quorum_verify_batch), measured beside what they replace:
device-resident buffers, secLevel 80, --comb-bits combs (24), --members attestations (65 536) in quorums of --k (4) whose members are interleaved over two
resident rings of --ring-a (2^16) and --ring-b (2^12) keys.  Rounds of six calls alternate in one process:
  rings_prove / rings_verify     the new calls
  recipe_prove / recipe_verify   (a) the "Counting signers" recipe from the `_rings` calls (zk_prove_batch_rings_device, zk_prove_key_blinders_device,
                                 zk_proof_key_commitments_device, zk_distinct_prove_batch_device; zk_verify_batch_rings_device, ..., an AND on the host), its pair
                                 arrays built on the host between the calls ("host_pairs_ms", timed on its own)
  grouped_prove / grouped_verify (b) the one-ring quorum calls on the same members grouped by ring: zk_ctx_use_ring + zk_quorum_prove_batch_device per ring
Recorded per call: wall time (median, min, max, spread = (max - min) / median over --reps rounds behind one warm-up round) and, for the new calls, the GPU time
of the families zk_last_timing reports ("quorum_caps" among them).  The yardstick is (a): ratios rings / recipe per round.  No ratio is fixed in advance.
  python tools/quorum_rings_rate.py [--members 65536] [--k 4] [--ring-a 65536] [--ring-b 4096] [--comb-bits 24] [--reps 5] [--out profiles/quorum_rings_rate.json]
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
    ap.add_argument('--members', type=int, default=65536)
    ap.add_argument('--k', type=int, default=4)
    ap.add_argument('--ring-a', type=int, default=65536)
    ap.add_argument('--ring-b', type=int, default=4096)
    ap.add_argument('--comb-bits', type=int, default=24)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    import zkp_ecdsa_amd as Z
    S, dev = 20261021, 'cuda:0'
    k, n = args.k, args.members
    assert k % 2 == 0 and n % (2 * k) == 0 and k // 2 <= args.ring_b and n // 2 <= args.ring_a, 'half of every quorum in each ring, different keys inside a quorum'
    Q, P, h = n // k, k * (k - 1) // 2, n // 2
    NP = Q * P
    e = Z.Engine(0)
    e.set_timing(1)
    e.set_comb_bits(args.comb_bits)
    e.set_params(*e.synth_params(S), 80)
    # witness b of a workload is signed by its ring's member b; ring b has fewer members than the call has attestations over it, so its witnesses are used again
    # (another attestation by the same key under fresh seeds) -- consecutive witnesses, and so the members of one quorum, have different keys
    wa, wb = e.synth_workload(S, args.ring_a, h), e.synth_workload(S + 1, args.ring_b, min(h, args.ring_b))
    ida, idb = e.add_ring(wa[0], args.ring_a), e.add_ring(wb[0], args.ring_b)
    again = np.arange(h) % len(wb[4])
    rows = lambda i, w: np.frombuffer(w[i], dtype=np.uint8).reshape(len(w[4]), -1)[np.arange(h) if w is wa else again]
    mix = lambda a, b: np.ascontiguousarray(np.stack([a, b], axis=1).reshape(n, -1))   # member m: ring a for even m, ring b for odd m
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy()).to(dev)
    p = lambda t: t.data_ptr()
    seeds = np.frombuffer(os.urandom(32 * n), dtype=np.uint8).reshape(n, 32)
    which = mix(np.array(wa[4], dtype=np.uint32)[:, None], np.array(wb[4], dtype=np.uint32)[again][:, None]).reshape(-1)
    ids = np.tile(np.array([ida, idb], dtype=np.uint32), h)
    h_msg, h_sig, h_pk = mix(rows(1, wa), rows(1, wb)), mix(rows(2, wa), rows(2, wb)), mix(rows(3, wa), rows(3, wb))
    d_msg, d_sig, d_pk, d_seeds, d_which, d_ids = up(h_msg), up(h_sig), up(h_pk), up(seeds), up(which.view(np.uint8)), up(ids.view(np.uint8))
    d_pseeds = up(np.frombuffer(os.urandom(32 * NP), dtype=np.uint8))
    # (b): the same members grouped by ring -- even members first, then odd ones; Q / 2 quorums per ring
    grp = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])
    g_msg, g_sig, g_pk, g_seeds, g_which = up(h_msg[grp]), up(h_sig[grp]), up(h_pk[grp]), up(seeds[grp]), up(which[grp].view(np.uint8))
    sa, sb = e.ring_proof_max_size(ida), e.ring_proof_max_size(idb)
    cap_q, cap_a = Q * (16 + PAIR * P) + h * (sa + sb), h * (sa + sb)
    assert cap_q == Q * e.quorum_proof_max_size_rings(k, [ida, idb] * (k // 2))
    z = lambda cnt, dt: torch.zeros(cnt, dtype=dt, device=dev)
    d_bundles, d_boff, d_qst, d_mst, d_qok, d_bad = torch.empty(cap_q, dtype=torch.uint8, device=dev), z(Q + 1, torch.int64), z(Q, torch.int32), z(n, torch.int32), z(Q, torch.uint8), z(Q, torch.int32)
    d_gb, d_goff = torch.empty(cap_q, dtype=torch.uint8, device=dev), z(Q + 2, torch.int64)
    d_att, d_aoff, d_ast = torch.empty(cap_a, dtype=torch.uint8, device=dev), z(n + 1, torch.int64), z(n, torch.int32)
    d_bl, d_com, d_kst = torch.empty(32 * n, dtype=torch.uint8, device=dev), torch.empty(72 * n, dtype=torch.uint8, device=dev), z(n, torch.int32)
    d_pairs, d_pst, d_aok, d_pok = torch.empty(PAIR * NP, dtype=torch.uint8, device=dev), z(NP, torch.int32), z(n, torch.uint8), z(NP, torch.uint8)
    pairs = Z.Engine.distinct_pairs(k)
    first = (np.arange(Q)[:, None] * k + np.array([i for i, _ in pairs])[None, :]).reshape(-1)
    second = (np.arange(Q)[:, None] * k + np.array([j for _, j in pairs])[None, :]).reshape(-1)
    host_ms = {}
    gather = lambda t, width, idx: torch.from_numpy(t.cpu().numpy().reshape(-1, width)[idx].reshape(-1)).to(dev)

    def rings_prove():
        e.quorum_prove_batch_rings_device(Q, k, p(d_msg), p(d_sig), p(d_pk), p(d_which), p(d_ids), p(d_seeds), p(d_pseeds), p(d_bundles), cap_q, p(d_boff), p(d_qst), p(d_mst))

    def rings_verify():
        e.quorum_verify_batch_rings_device(Q, k, p(d_msg), p(d_bundles), p(d_boff), p(d_ids), None, p(d_qok), p(d_qst), p(d_bad))

    def recipe_prove():
        e.prove_batch_rings_device(n, p(d_msg), p(d_sig), p(d_pk), p(d_which), p(d_ids), p(d_seeds), p(d_att), cap_a, p(d_aoff), p(d_ast))
        e.prove_key_blinders_device(n, p(d_seeds), p(d_bl))
        e.proof_key_commitments_device(n, p(d_att), p(d_aoff), p(d_com), p(d_kst))
        t0 = time.perf_counter()
        key = h_pk[:, :32]
        six = [up(key[first]), gather(d_com, 72, first), gather(d_bl, 32, first), up(key[second]), gather(d_com, 72, second), gather(d_bl, 32, second)]
        torch.cuda.synchronize()
        host_ms['prove'] = (time.perf_counter() - t0) * 1e3
        e.distinct_prove_batch_device(NP, *[p(t) for t in six], p(d_pseeds), p(d_pairs), PAIR * NP, p(d_pst))

    def recipe_verify():
        e.verify_batch_rings_device(n, p(d_msg), p(d_att), p(d_aoff), p(d_ids), None, p(d_aok), p(d_ast))
        e.proof_key_commitments_device(n, p(d_att), p(d_aoff), p(d_com), p(d_kst))
        t0 = time.perf_counter()
        c1, c2 = gather(d_com, 72, first), gather(d_com, 72, second)
        torch.cuda.synchronize()
        host_ms['verify'] = (time.perf_counter() - t0) * 1e3
        e.distinct_verify_batch_device(NP, p(c1), p(c2), p(d_pairs), p(d_pok), p(d_pst))
        t0 = time.perf_counter()
        ok = d_aok.cpu().numpy().reshape(Q, k).all(axis=1) & d_pok.cpu().numpy().reshape(Q, P).all(axis=1)
        host_ms['verify'] += (time.perf_counter() - t0) * 1e3
        assert ok.all(), 'the recipe rejected an honest quorum'

    half = Q // 2
    g_base = [0, 0]   # where ring b's bundles start in d_gb (the first call's end, 8-byte aligned slots: bundle lengths are multiples of 4)

    def grouped(call):
        for r, rid in enumerate((ida, idb)):
            e.use_ring(rid)
            call(r, r * half * k, r * half * P)

    def grouped_prove():
        def one(r, m0, p0):
            base = 0 if r == 0 else g_base[1]
            e.quorum_prove_batch_device(half, k, p(g_msg) + 32 * m0, p(g_sig) + 64 * m0, p(g_pk) + 64 * m0, p(g_which) + 4 * m0, p(g_seeds) + 32 * m0, p(d_pseeds) + 32 * p0,
                                        p(d_gb) + base, cap_q - base, p(d_goff) + 8 * r * (half + 1), p(d_qst) + 4 * r * half, p(d_mst) + 4 * m0)
            if r == 0:
                g_base[1] = (int(d_goff[half]) + 7) & ~7
        grouped(one)

    def grouped_verify():
        grouped(lambda r, m0, p0: e.quorum_verify_batch_device(half, k, p(g_msg) + 32 * m0, p(d_gb) + (0 if r == 0 else g_base[1]), p(d_goff) + 8 * r * (half + 1), None,
                                                               p(d_qok) + r * half, p(d_qst) + 4 * r * half, p(d_bad) + 4 * r * half))

    calls = (('rings_prove', rings_prove), ('recipe_prove', recipe_prove), ('grouped_prove', grouped_prove), ('rings_verify', rings_verify),
             ('recipe_verify', recipe_verify), ('grouped_verify', grouped_verify))
    rec = {name: {'wall': [], 'fam': [], 'host': []} for name, _ in calls}
    for rep in range(args.reps + 1):
        for name, call in calls:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            if int(d_qst.abs().sum()) != 0 or (name.endswith('verify') and not name.startswith('recipe') and int(d_qok.sum()) != Q):
                st, bad = d_qst.cpu().numpy(), d_bad.cpu().numpy().view(np.uint32)
                raise AssertionError('%s: an honest quorum failed: ok %d of %d, statuses %s, first_bad %s, first failing quorums %s' % (
                    name, int(d_qok.sum()), Q, dict(zip(*np.unique(st, return_counts=True))), dict(zip(*np.unique(bad, return_counts=True))),
                    np.nonzero(d_qok.cpu().numpy() == 0)[0][:8]))
            if rep >= 1:
                rec[name]['wall'].append(wall)
                if name.startswith('rings'):
                    rec[name]['fam'].append(e.last_timing()[1])
                if name.startswith('recipe'):
                    rec[name]['host'].append(host_ms[name.split('_')[1]])
    total = int(d_boff[Q])
    assert total == 16 * Q + int(d_aoff[n]) + PAIR * NP, 'the bundles are not the recipe\'s bytes long'

    def summary(r):
        w = r['wall']
        s = {'ms': round(statistics.median(w), 3), 'min_ms': round(min(w), 3), 'max_ms': round(max(w), 3), 'spread': round((max(w) - min(w)) / statistics.median(w), 4)}
        if r['fam']:
            s['families_ms'] = {f: round(statistics.median(x.get(f, 0.0) for x in r['fam']), 4) for f in sorted(set().union(*r['fam']))}
        if r['host']:
            s['host_pairs_ms'] = round(statistics.median(r['host']), 3)
            s['ms_without_host_pairs'] = round(statistics.median(a - b for a, b in zip(w, r['host'])), 3)
        return s

    def ratio(a, b):
        per = [x / y for x, y in zip(rec[a]['wall'], rec[b]['wall'])]
        return {'of_medians': round(statistics.median(rec[a]['wall']) / statistics.median(rec[b]['wall']), 4), 'per_round_median': round(statistics.median(per), 4),
                'per_round_min': round(min(per), 4), 'per_round_max': round(max(per), 4)}

    res = {'tool': 'quorum_rings_rate', 'sec': 80, 'comb_bits': args.comb_bits, 'reps': args.reps, 'k': k, 'Q': Q, 'attestations': n, 'pairs': NP, 'rings': [args.ring_a, args.ring_b],
           'bundle_bytes': total, 'calls': {name: summary(rec[name]) for name, _ in calls},
           'ratio_rings_over_recipe': {'prove': ratio('rings_prove', 'recipe_prove'), 'verify': ratio('rings_verify', 'recipe_verify')},
           'ratio_rings_over_grouped': {'prove': ratio('rings_prove', 'grouped_prove'), 'verify': ratio('rings_verify', 'grouped_verify')}}
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
