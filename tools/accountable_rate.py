"""Accountable attestations (include/zkattest.h: zk_accountable_prove_batch / zk_accountable_verify_batch), measured beside the recipe they replace
(INTEGRATION.md "Accountable attestations"): --proofs device-resident proofs (65 536), a ring of --ring keys (2^16), secLevel 80, --comb-bits combs (24);
rounds of one-call prove / recipe prove / one-call verify / recipe verify alternating in one process.  The recipe's calls are zk_prove_batch_device,
zk_prove_key_blinders_device, zk_proof_key_commitments_device and zk_escrow_prove_batch_device (verifier: zk_verify_batch_device,
zk_proof_key_commitments_device, zk_escrow_verify_batch_device and an AND on the host); its dense key array (pk_xy[0:32] of every row) is built on the HOST
between the calls, as a user builds it today, and that part is timed on its own ("host_keys_ms": the copy out, the gather, the copy in).

Recorded per side: both wall times (median, min, max over --reps rounds behind one warm-up round), the ratio one-call / recipe (of the medians, and each
round's own: median, min, max), the recipe's own round-to-round spread, and the GPU time of the one-call form's families (zk_last_timing), the new kernels
among them under "accountable_*".  No ratio is fixed in advance.  Then the latency of ONE bundle beside one proof: zk_accountable_prove_batch /
zk_accountable_verify_batch with B = 1 against zk_prove_batch / zk_verify_batch with B = 1, host-pointer forms, median of --latency-reps calls.
  python tools/accountable_rate.py [--proofs 65536] [--ring 65536] [--comb-bits 24] [--reps 3] [--out profiles/accountable_rate.json]
Prints one JSON line (also written to --out PATH when given).  Run it under a time limit (timeout 900 python tools/accountable_rate.py ...)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAG = 472


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--proofs', type=int, default=65536)
    ap.add_argument('--ring', type=int, default=65536)
    ap.add_argument('--comb-bits', type=int, default=24)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--latency-reps', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import numpy as np
    import torch
    import zkp_ecdsa_amd as Z
    S, dev, B = 20261021, 'cuda:0', args.proofs
    assert B <= args.ring, 'one witness per ring member'
    res = {'tool': 'accountable_rate', 'proofs': B, 'ring': args.ring, 'sec': 80, 'comb_bits': args.comb_bits, 'reps': args.reps}
    e = Z.Engine(0)
    e.set_timing(1)
    e.set_comb_bits(args.comb_bits)
    e.set_params(*e.synth_params(S), 80)
    ring, msg, sig, pk, which, seeds = e.synth_workload(S, args.ring, B)   # witness b is signed by ring member b
    e.set_ring(ring, args.ring)
    e.set_auditor(e.escrow_keygen(bytes(31) + b'\x07'))
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    p = lambda t: t.data_ptr()
    d_msg, d_sig, d_pk, d_seeds, d_tseeds = up(msg), up(sig), up(pk), up(seeds), up(os.urandom(32 * B))
    d_which = torch.tensor(which, dtype=torch.int32, device=dev)
    cap_c, cap_a = e.accountable_proof_max_size() * B, e.proof_max_size() * B
    d_bundles, d_boff = torch.empty(cap_c, dtype=torch.uint8, device=dev), torch.zeros(B + 1, dtype=torch.int64, device=dev)
    d_cst, d_pst = torch.ones(B, dtype=torch.int32, device=dev), torch.ones(2 * B, dtype=torch.int32, device=dev)
    d_cok, d_bad = torch.zeros(B, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    d_att, d_aoff, d_ast = torch.empty(cap_a, dtype=torch.uint8, device=dev), torch.zeros(B + 1, dtype=torch.int64, device=dev), torch.ones(B, dtype=torch.int32, device=dev)
    d_bl, d_com, d_kst = torch.empty(32 * B, dtype=torch.uint8, device=dev), torch.empty(72 * B, dtype=torch.uint8, device=dev), torch.ones(B, dtype=torch.int32, device=dev)
    d_tags, d_tst = torch.empty(TAG * B, dtype=torch.uint8, device=dev), torch.ones(B, dtype=torch.int32, device=dev)
    d_aok, d_tok = torch.zeros(B, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
    host_ms = {}

    def families():   # (room for more names than Engine.last_timing asks for: the one-call forms add up several pipelines' families)
        import ctypes as C
        total, names, ms = C.c_float(), (C.c_char_p * 64)(), (C.c_float * 64)()
        n = e.L.zk_last_timing(e.h, C.byref(total), names, ms, 64)
        return {names[i].decode(): ms[i] for i in range(min(n, 64))}

    def one_prove():
        e.accountable_prove_batch_device(B, p(d_msg), p(d_sig), p(d_pk), p(d_which), p(d_seeds), p(d_tseeds), p(d_bundles), cap_c, p(d_boff), p(d_cst), p(d_pst))

    def one_verify():
        e.accountable_verify_batch_device(B, p(d_msg), p(d_bundles), p(d_boff), None, p(d_cok), p(d_cst), p(d_bad))

    def recipe_prove():
        e.prove_batch_device(B, p(d_msg), p(d_sig), p(d_pk), p(d_which), p(d_seeds), p(d_att), cap_a, p(d_aoff), p(d_ast))
        e.prove_key_blinders_device(B, p(d_seeds), p(d_bl))
        e.proof_key_commitments_device(B, p(d_att), p(d_aoff), p(d_com), p(d_kst))
        t0 = time.perf_counter()   # device rows -> host -> the dense keys -> device: what a user of the recipe does between its calls
        keys = torch.from_numpy(np.ascontiguousarray(d_pk.cpu().numpy().reshape(-1, 64)[:B, :32]).reshape(-1)).to(dev)
        torch.cuda.synchronize()
        host_ms['prove'] = (time.perf_counter() - t0) * 1e3
        e.escrow_prove_batch_device(B, p(keys), p(d_com), p(d_bl), p(d_tseeds), p(d_tags), TAG * B, p(d_tst))

    def recipe_verify():
        e.verify_batch_device(B, p(d_msg), p(d_att), p(d_aoff), None, p(d_aok), p(d_ast))
        e.proof_key_commitments_device(B, p(d_att), p(d_aoff), p(d_com), p(d_kst))
        e.escrow_verify_batch_device(B, p(d_com), p(d_tags), p(d_tok), p(d_tst))
        t0 = time.perf_counter()
        ok = d_aok.cpu().numpy().astype(bool) & d_tok.cpu().numpy().astype(bool)
        host_ms['verify'] = (time.perf_counter() - t0) * 1e3
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
                    rec[name]['fam'].append(families())
                else:
                    rec[name]['host'].append(host_ms[name.split('_')[1]])
    assert int(d_cok.sum()) == B and int(d_cst.abs().sum()) == 0 and bool(out.all()), 'a verifier rejected an honest bundle'
    total = int(d_boff[B])
    assert total == 16 * B + int(d_aoff[B]) + TAG * B, 'the bundles are not the recipe\'s bytes long'

    def summary(r, fams=False):
        w = r['wall']
        s = {'ms': round(statistics.median(w), 3), 'min_ms': round(min(w), 3), 'max_ms': round(max(w), 3), 'spread': round((max(w) - min(w)) / statistics.median(w), 4)}
        if fams:
            keys = sorted(set().union(*r['fam']))
            s['families_ms'] = {f: round(statistics.median(x.get(f, 0.0) for x in r['fam']), 4) for f in keys}
            s['new_kernels_ms'] = round(sum(v for f, v in s['families_ms'].items() if f.startswith('accountable_')), 4)
        else:
            s['host_keys_ms'] = round(statistics.median(r['host']), 3)
            s['ms_without_host_part'] = round(statistics.median(a - b for a, b in zip(w, r['host'])), 3)
        return s

    def ratio(side):
        a, b = rec['one_call_' + side], rec['recipe_' + side]
        per = [x / y for x, y in zip(a['wall'], b['wall'])]
        dev_only = [x / (y - h) for x, y, h in zip(a['wall'], b['wall'], b['host'])]
        return {'of_medians': round(statistics.median(a['wall']) / statistics.median(b['wall']), 4), 'per_round_median': round(statistics.median(per), 4),
                'per_round_min': round(min(per), 4), 'per_round_max': round(max(per), 4), 'against_recipe_without_host_part': round(statistics.median(dev_only), 4)}

    res.update({'bundle_bytes': total, 'one_call_prove': summary(rec['one_call_prove'], True), 'recipe_prove': summary(rec['recipe_prove']),
                'one_call_verify': summary(rec['one_call_verify'], True), 'recipe_verify': summary(rec['recipe_verify']),
                'ratio_one_call_over_recipe': {'prove': ratio('prove'), 'verify': ratio('verify')}})
    del d_bundles, d_att, d_tags
    torch.cuda.empty_cache()

    # one bundle beside one proof, host-pointer forms
    e.set_timing(0)
    w1 = (msg[:32], sig[:64], pk[:64], which[:1])
    lat = {'bundle_prove': [], 'proof_prove': [], 'bundle_verify': [], 'proof_verify': []}
    for rep in range(args.latency_reps + 2):
        t = [time.perf_counter()]
        bundle = e.accountable_prove_batch(*w1, seeds=seeds[:32], tag_seeds=os.urandom(32))[0]
        t.append(time.perf_counter())
        proof = e.prove_batch(*w1, seeds=seeds[:32])[0]
        t.append(time.perf_counter())
        okb = e.accountable_verify_batch(w1[0], bundle)[0]
        t.append(time.perf_counter())
        okp = e.verify_batch(w1[0], proof)[0]
        t.append(time.perf_counter())
        assert okb == [1] and okp == [1] and bundle[0][16:-TAG] == proof[0]
        if rep >= 2:
            for i, name in enumerate(('bundle_prove', 'proof_prove', 'bundle_verify', 'proof_verify')):
                lat[name].append((t[i + 1] - t[i]) * 1e3)
    res['latency_one'] = {name: {'ms': round(statistics.median(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3)} for name, v in lat.items()}
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
