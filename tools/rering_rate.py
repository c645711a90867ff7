"""Re-ring proofs (include/zkattest.h: zk_proof_rering_batch) against what they replace, measured on the same inputs: --batch proofs (65 536) at secLevel 80
over a ring of --ring keys (2^16), every buffer device-resident.

After two warm-up rounds the tool ALTERNATES four calls for --reps rounds on one device in one process, on the same indices and blinders, so drift of the box
falls on all alike:
  (a) rering_in_place   zk_proof_rering_batch_device with out == proofs
  (b) rering            ... into a second buffer (the heads, ~96 % of the bytes, are copied)
  (c) member_prove      zk_member_prove_batch_device with the caller's blinders: the work a re-ring cannot avoid
  (d) prove             zk_prove_batch_device: what re-proving costs
Recorded per call: the median wall time, its proofs per second, its run-to-run spread ((max - min) / median), the GPU time of its families (zk_last_timing);
the device's copy rate over the proofs' bytes (read + write, a device-to-device copy of the same buffer); the yardsticks -- (c) for (a), (c) plus the heads at
the copy rate for (b) -- and the calls' ratios to them; the same four calls on one proof.  No threshold is set here (DESIGN.md section 5d reads the numbers).
  python tools/rering_rate.py [--batch 65536] [--ring 65536] [--reps 10] [--out profiles/rering_rate.json]
Prints one JSON line (also written to --out PATH when given)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--ring', type=int, default=65536)
    ap.add_argument('--sec', type=int, default=80)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import zkp_ecdsa_amd as Z
    S, B, dev = 20261020, args.batch, 'cuda:0'
    res = {'tool': 'rering_rate', 'batch': B, 'ring': args.ring, 'sec': args.sec, 'reps': args.reps}
    e = Z.Engine(0)
    e.set_timing(1)
    e.set_params(*e.synth_params(S), args.sec)
    ring, msg, sig, pk, which, seeds = e.synth_workload(S, args.ring, B)
    e.set_ring(ring, args.ring)

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d_msg, d_sig, d_pk, d_seeds = up(msg), up(sig), up(pk), up(seeds)
    d_which = torch.tensor(which, dtype=torch.int32).to(dev)
    g = torch.Generator().manual_seed(S)
    d_fresh = torch.randint(0, 256, (32 * B,), dtype=torch.uint8, generator=g).to(dev)   # never the seeds the proofs were made with
    cap = e.proof_max_size() * B
    d_proofs, d_out = torch.empty(cap, dtype=torch.uint8, device=dev), torch.empty(cap, dtype=torch.uint8, device=dev)
    d_off, d_ooff = torch.zeros(B + 1, dtype=torch.int64, device=dev), torch.zeros(B + 1, dtype=torch.int64, device=dev)
    d_st, d_bl = torch.ones(B, dtype=torch.int32, device=dev), torch.empty(32 * B, dtype=torch.uint8, device=dev)
    msize = e.member_proof_size()
    d_mcom, d_mout = torch.empty(72 * B, dtype=torch.uint8, device=dev), torch.empty(msize * B, dtype=torch.uint8, device=dev)
    e.prove_key_blinders_device(B, d_seeds.data_ptr(), d_bl.data_ptr())

    def prove(n):
        e.prove_batch_device(n, d_msg.data_ptr(), d_sig.data_ptr(), d_pk.data_ptr(), d_which.data_ptr(), d_seeds.data_ptr(), d_proofs.data_ptr(), cap, d_off.data_ptr(),
                             d_st.data_ptr())

    def member(n):
        e.member_prove_batch_device(n, d_which.data_ptr(), d_bl.data_ptr(), d_fresh.data_ptr(), d_mcom.data_ptr(), None, d_mout.data_ptr(), msize * n, d_st.data_ptr())

    def rering(n, in_place):
        o = d_proofs if in_place else d_out
        e.rering_batch_device(n, d_msg.data_ptr(), d_proofs.data_ptr(), d_off.data_ptr(), d_which.data_ptr(), d_bl.data_ptr(), d_fresh.data_ptr(), o.data_ptr(), cap,
                              d_ooff.data_ptr(), d_st.data_ptr())

    calls = (('prove', prove), ('member_prove', member), ('rering_in_place', lambda n: rering(n, True)), ('rering', lambda n: rering(n, False)))

    def alternate(n, reps):
        walls, fams = {k: [] for k, _ in calls}, {k: [] for k, _ in calls}
        for rep in range(reps + 2):
            for name, call in calls:   # (prove first: the re-ring calls of a round read the proofs it wrote)
                t0 = time.perf_counter()
                call(n)
                dt = (time.perf_counter() - t0) * 1e3
                torch.cuda.synchronize()
                assert int(d_st[:n].abs().sum()) == 0, name
                if rep >= 2:
                    walls[name].append(dt), fams[name].append(e.last_timing()[1])
        out = {}
        for name, _ in calls:
            w, f = walls[name], fams[name]
            med = statistics.median(w)
            keys = sorted(set().union(*f))
            out[name] = {'ms': round(med, 4), 'per_s': round(n / med * 1e3), 'min_ms': round(min(w), 4), 'max_ms': round(max(w), 4),
                         'spread': round((max(w) - min(w)) / med, 4), 'families_ms': {k: round(statistics.median(x.get(k, 0.0) for x in f), 3) for k in keys}}
        return out

    big = res['batch_calls'] = alternate(B, args.reps)
    torch.cuda.synchronize()
    total = int(d_ooff[B])
    res['proof_bytes_total'], res['gk_bytes_per_proof'] = total, msize - 16
    head = total - B * (msize - 16)
    # the same n: the same offsets; and the out-of-place result verifies
    assert int((d_ooff != d_off).sum()) == 0
    d_ok = torch.zeros(B, dtype=torch.uint8, device=dev)
    e.verify_batch_device(B, d_msg.data_ptr(), d_out.data_ptr(), d_ooff.data_ptr(), None, d_ok.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    assert int(d_ok.sum()) == B and int(d_st.abs().sum()) == 0, 'the verifier rejected a re-ringed proof'
    # the device's copy rate over the same bytes
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    rates = []
    for _ in range(5):
        ev[0].record()
        d_out[:total].copy_(d_proofs[:total])
        ev[1].record()
        torch.cuda.synchronize()
        rates.append(total / (ev[0].elapsed_time(ev[1]) * 1e-3) / 1e9)
    copy_gbps = statistics.median(rates[1:])
    res['copy_gb_per_s'] = round(copy_gbps, 1)   # bytes copied per second (each is read once and written once)
    head_ms = head / (copy_gbps * 1e9) * 1e3
    c = big['member_prove']['ms']
    res['yardsticks'] = {'in_place_ms': c, 'out_of_place_ms': round(c + head_ms, 4), 'head_copy_ms': round(head_ms, 4),
                         'in_place_over_yardstick': round(big['rering_in_place']['ms'] / c, 4), 'out_of_place_over_yardstick': round(big['rering']['ms'] / (c + head_ms), 4),
                         'prove_over_in_place': round(big['prove']['ms'] / big['rering_in_place']['ms'], 2), 'prove_over_out_of_place': round(big['prove']['ms'] / big['rering']['ms'], 2)}
    one = alternate(1, args.reps)
    res['one_proof_calls'] = {k: {'ms': v['ms'], 'spread': v['spread']} for k, v in one.items()}
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
