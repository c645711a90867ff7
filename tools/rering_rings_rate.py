"""Re-ring with one destination ring id per proof (include/zkattest.h: zk_proof_rering_batch_rings) against the one-ring call it replaces, on the same inputs:
--batch device-resident proofs (65 536) at secLevel 80, made on the small ring (one witness per key of it, cycled); half of them bound for a ring of --ring-a keys (2^16), half for one of
--ring-b keys (2^12), interleaved a, b, a, b.  Ring a holds ring b's keys at the same indices, so every proof's key lies in both.

After two warm-up rounds the tool ALTERNATES four sides for --reps rounds on one device in one process, so drift of the box falls on all alike:
  (i)   mixed            zk_proof_rering_batch_rings_device into a second buffer, no ring made active
  (i')  grouped          the yardstick: the same inputs grouped by destination, zk_ctx_use_ring + zk_proof_rering_batch_device per ring (two of each)
  (ii)  mixed_in_place   ... out == proofs, on proofs made for rings of those two sizes (the output of (i))
  (ii') grouped_in_place the yardstick: the grouped outputs of (i'), in place, ring by ring
Recorded per side: the median wall time, proofs per second, the run-to-run spread ((max - min) / median), the GPU time of its families (zk_last_timing; for a
grouped side the sum over its two calls), and the ratios mixed / grouped.  The mixed output is checked: every status 0, every proof accepted by
zk_verify_batch_rings_device under the same ids, its offsets the running sum of head + gk(n of its ring).  No threshold is set here: DESIGN.md section 5d'
reads the numbers (the project's convention asks for an explanation by family above 1.3 x the yardstick).
  python tools/rering_rings_rate.py [--batch 65536] [--ring-a 65536] [--ring-b 4096] [--reps 10] [--out profiles/rering_rings_rate.json]
Prints one JSON line (also written to --out PATH when given)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FAMILIES = ('rr_census', 'rr_offsets', 'rr_move', 'm_gather')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--ring-a', type=int, default=65536)
    ap.add_argument('--ring-b', type=int, default=4096)
    ap.add_argument('--sec', type=int, default=80)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import zkp_ecdsa_amd as Z
    S, B, dev = 20261020, args.batch, 'cuda:0'
    assert B % 2 == 0 and args.ring_a >= args.ring_b
    H = B // 2
    res = {'tool': 'rering_rings_rate', 'batch': B, 'ring_a': args.ring_a, 'ring_b': args.ring_b, 'sec': args.sec, 'reps': args.reps}
    e = Z.Engine(0)
    e.set_timing(1)
    e.set_params(*e.synth_params(S), args.sec)
    Wn = min(B, args.ring_b)   # the synthetic workload gives every proof a key of its own at ring[b % nkeys]: one witness per key of the small ring, cycled over the batch
    ring_b, msg, sig, pk, which, seeds = e.synth_workload(S, args.ring_b, Wn)
    ring_a = e.synth_workload(S + 1, args.ring_a, 1)[0]
    ring_a = ring_b + ring_a[len(ring_b):]           # ring b's keys at the same indices, other keys behind them
    e.set_ring(ring_b, args.ring_b)                  # id 0: the ring the proofs are made on, and destination b
    id_b, id_a = 0, e.add_ring(ring_a, args.ring_a)
    n_a, n_b = e.ring_info(id_a)['log_n'], e.ring_info(id_b)['log_n']
    res['n_a'], res['n_b'] = n_a, n_b

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)

    def half(t, k):   # rows k, k + 2, ... of a per-proof array, contiguous
        return t.view(B, -1)[k::2].contiguous().view(-1)
    cyc = (torch.arange(B) % Wn).to(dev)

    def tile(b):   # witness j % Wn for proof j (the re-ring seeds below are fresh per proof)
        return up(b).view(Wn, -1)[cyc].contiguous().view(-1)
    d_msg, d_sig, d_pk, d_seeds = tile(msg), tile(sig), tile(pk), tile(seeds)
    d_which = torch.tensor(which, dtype=torch.int32).to(dev)[cyc].contiguous()
    g = torch.Generator().manual_seed(S)
    d_fresh = torch.randint(0, 256, (32 * B,), dtype=torch.uint8, generator=g).to(dev)   # never the seeds the proofs were made with
    d_bl = torch.empty(32 * B, dtype=torch.uint8, device=dev)
    e.prove_key_blinders_device(B, d_seeds.data_ptr(), d_bl.data_ptr())
    d_ids = torch.tensor([id_a, id_b] * H, dtype=torch.int32).to(dev)
    size_b = e.proof_max_size()
    grow = e.member_proof_size(id_a) - e.member_proof_size(id_b)
    cap, hcap = (size_b + grow) * B, (size_b + grow) * H
    d_st = torch.ones(B, dtype=torch.int32, device=dev)

    def buf(n):
        return torch.empty(n, dtype=torch.uint8, device=dev)

    def offs(n):
        return torch.zeros(n + 1, dtype=torch.int64, device=dev)
    # the inputs: all B proofs in order, and the same proofs grouped by destination (even indices -> a, odd -> b), every one made on ring b from its own seed
    d_in, d_in_off = buf(size_b * B), offs(B)
    e.prove_batch_device(B, d_msg.data_ptr(), d_sig.data_ptr(), d_pk.data_ptr(), d_which.data_ptr(), d_seeds.data_ptr(), d_in.data_ptr(), size_b * B, d_in_off.data_ptr(),
                         d_st.data_ptr())
    torch.cuda.synchronize()
    assert int(d_st.abs().sum()) == 0
    grp = []
    for k, rid in ((0, id_a), (1, id_b)):
        G = {'id': rid, 'msg': half(d_msg, k), 'which': d_which[k::2].contiguous(), 'bl': half(d_bl, k), 'fresh': half(d_fresh, k), 'in': buf(size_b * H), 'in_off': offs(H),
             'out': buf(hcap), 'out_off': offs(H), 'st': torch.ones(H, dtype=torch.int32, device=dev)}
        h_sig, h_pk, h_seeds = half(d_sig, k), half(d_pk, k), half(d_seeds, k)   # (named: a temporary's memory is reused by the next one)
        e.prove_batch_device(H, G['msg'].data_ptr(), h_sig.data_ptr(), h_pk.data_ptr(), G['which'].data_ptr(), h_seeds.data_ptr(), G['in'].data_ptr(), size_b * H,
                             G['in_off'].data_ptr(), G['st'].data_ptr())
        torch.cuda.synchronize()
        assert int(G['st'].abs().sum()) == 0
        grp.append(G)
    d_out, d_out_off = buf(cap), offs(B)

    def fam_add(acc, f):
        for k, v in f.items():
            acc[k] = acc.get(k, 0.0) + v
        return acc

    def mixed(in_place):
        src, src_off = (d_out, d_out_off) if in_place else (d_in, d_in_off)
        e.rering_batch_rings_device(B, d_msg.data_ptr(), src.data_ptr(), src_off.data_ptr(), d_which.data_ptr(), d_ids.data_ptr(), d_bl.data_ptr(), d_fresh.data_ptr(),
                                    d_out.data_ptr(), cap, d_out_off.data_ptr(), d_st.data_ptr())
        return dict(e.last_timing()[1])

    def grouped(in_place):
        fams = {}
        for G in grp:
            src, src_off = (G['out'], G['out_off']) if in_place else (G['in'], G['in_off'])
            e.use_ring(G['id'])
            e.rering_batch_device(H, G['msg'].data_ptr(), src.data_ptr(), src_off.data_ptr(), G['which'].data_ptr(), G['bl'].data_ptr(), G['fresh'].data_ptr(),
                                  G['out'].data_ptr(), hcap, G['out_off'].data_ptr(), G['st'].data_ptr())
            fam_add(fams, e.last_timing()[1])
        return fams

    sides = (('grouped', lambda: grouped(False)), ('mixed', lambda: mixed(False)), ('grouped_in_place', lambda: grouped(True)), ('mixed_in_place', lambda: mixed(True)))
    walls, fams = {k: [] for k, _ in sides}, {k: [] for k, _ in sides}
    for rep in range(args.reps + 2):
        for name, call in sides:   # (each in-place side works on what the out-of-place side before it wrote)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f = call()
            dt = (time.perf_counter() - t0) * 1e3   # the calls are synchronous: they return with their work done
            torch.cuda.synchronize()
            for st in ([d_st] if name.startswith('mixed') else [G['st'] for G in grp]):
                if int(st.abs().sum()):
                    codes, counts = torch.unique(st.cpu(), return_counts=True)
                    bad = st.nonzero().view(-1).tolist()
                    raise SystemExit('%s, round %d: statuses %s, failing proofs %s ... %s' % (name, rep, dict(zip(codes.tolist(), counts.tolist())), bad[:12], bad[-6:]))
            if rep >= 2:
                walls[name].append(dt), fams[name].append(f)
    e.use_ring(id_b)
    out = res['sides'] = {}
    for name, _ in sides:
        w, f = walls[name], fams[name]
        med = statistics.median(w)
        keys = sorted(set().union(*f))
        out[name] = {'ms': round(med, 4), 'per_s': round(B / med * 1e3), 'min_ms': round(min(w), 4), 'max_ms': round(max(w), 4), 'spread': round((max(w) - min(w)) / med, 4),
                     'families_ms': {k: round(statistics.median(x.get(k, 0.0) for x in f), 3) for k in keys}}
    res['ratio'] = {'second_buffer': round(out['mixed']['ms'] / out['grouped']['ms'], 4), 'in_place': round(out['mixed_in_place']['ms'] / out['grouped_in_place']['ms'], 4)}
    res['front_families_ms'] = {side: {k: out[side]['families_ms'].get(k, 0.0) for k in FAMILIES} for side in ('mixed', 'mixed_in_place')}
    # the mixed output: the layout the contract states, and every proof verifies under its ring
    torch.cuda.synchronize()
    in_len = (d_in_off[1:] - d_in_off[:-1]).cpu()
    want = in_len.clone()
    want[0::2] += grow
    got = (d_out_off[1:] - d_out_off[:-1]).cpu()
    assert int(d_out_off[0]) == 0 and bool((got == want).all()), 'out_off is not the running sum of head + gk(n of the ring)'
    res['out_bytes'], res['in_bytes'] = int(d_out_off[B]), int(d_in_off[B])
    d_ok = torch.zeros(B, dtype=torch.uint8, device=dev)
    e.verify_batch_rings_device(B, d_msg.data_ptr(), d_out.data_ptr(), d_out_off.data_ptr(), d_ids.data_ptr(), None, d_ok.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    assert int(d_ok.sum()) == B and int(d_st.abs().sum()) == 0, 'the verifier rejected a re-ringed proof'
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
