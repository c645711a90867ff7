"""The exhaustive verify mode (include/zkattest.h: zk_ctx_set_verify_reps), measured: device-resident proofs, one process, one GPU.

  sample   ZK_VERIFY_REPS_SAMPLE, the 20 repetitions generateIndices draws (the yardstick, in the same run)
  all      ZK_VERIFY_REPS_ALL, every repetition: P = ceil(secLevel / 20) passes over the same pipeline

65 536 resident proofs over a ring of 2^16 keys at secLevel 80 (P = 4).  The two modes are alternated call by call, so that a drifting clock affects both
alike; every call's verdicts are checked (all accept).  Rates are medians of --steps calls after --warmup; the timing families of one timed call per mode say
where a ratio above P goes.  Also the latency of one proof per call in both modes.
  python tools/verify_all_rate.py [--ring 65536] [--batch 65536] [--steps 10] [--warmup 2] [--comb-bits 16] [--chunk 8192] [--lanes 3]
Prints one JSON line and writes it to --out (default profiles/verify_all_rate.json)."""
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
    ap.add_argument('--ring', type=int, default=65536)
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--sec', type=int, default=80)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--comb-bits', type=int, default=16)
    ap.add_argument('--chunk', type=int, default=8192)
    ap.add_argument('--lanes', type=int, default=3)
    ap.add_argument('--latency-calls', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'verify_all_rate.json'))
    args = ap.parse_args()
    import torch
    import zkp_ecdsa_amd as Z
    dev = 'cuda:0'
    S, B, nkeys = 20261020, args.batch, args.ring
    e = Z.Engine(0)
    e.set_comb_bits(args.comb_bits)
    nh, tg, th = e.synth_params(S)
    ring, msg, sig, pk, which, seeds = e.synth_workload(S, nkeys, B)
    e.set_params(nh, tg, th, args.sec)
    e.set_ring(ring, nkeys)
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d_msg, d_sig, d_pk, d_seeds = t(msg), t(sig), t(pk), t(seeds)
    d_which = torch.tensor(which, dtype=torch.int32).to(dev)
    d_vseeds = t(os.urandom(32 * B))
    e.set_chunk(min(4096, B))
    cap = int(B * e.proof_max_size() * 0.8)
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    d_st = torch.empty(B, dtype=torch.int32, device=dev)
    e.prove_batch_device(B, d_msg.data_ptr(), d_sig.data_ptr(), d_pk.data_ptr(), d_which.data_ptr(), d_seeds.data_ptr(), d_out.data_ptr(), cap, d_off.data_ptr(),
                         d_st.data_ptr())
    torch.cuda.synchronize()
    assert int((d_st != 0).sum()) == 0
    e.set_chunk(min(args.chunk, B)), e.set_lanes(args.lanes)
    d_ok = torch.empty(B, dtype=torch.uint8, device=dev)
    d_vst = torch.empty(B, dtype=torch.int32, device=dev)

    def call(reps_all, n=B):
        e.set_verify_reps(reps_all)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.verify_batch_device(n, d_msg.data_ptr(), d_out.data_ptr(), d_off.data_ptr(), d_vseeds.data_ptr(), d_ok.data_ptr(), d_vst.data_ptr())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert int(d_ok[:n].sum()) == n and int((d_vst[:n] != 0).sum()) == 0, 'a verdict differs'
        return dt

    runs = {False: [], True: []}
    for step in range(args.warmup + args.steps):
        for mode in (False, True):
            dt = call(mode)
            if step >= args.warmup:
                runs[mode].append(dt)
    fam = {}
    e.set_timing(1)
    for mode in (False, True):
        c12 = e.test_counter(12)
        call(mode)
        fam['all' if mode else 'sample'] = {'passes': e.test_counter(12) - c12, 'ms': {k: round(v, 2) for k, v in sorted(e.last_timing()[1].items())}}
    e.set_timing(2)   # the default again
    lat = {False: [], True: []}
    for i in range(args.latency_calls):
        for mode in (False, True):
            lat[mode].append(call(mode, n=1))
    med = {k: statistics.median(v) for k, v in runs.items()}
    passes = (args.sec + 19) // 20
    res = {
        'tool': 'verify_all_rate', 'batch': B, 'ring': nkeys, 'sec': args.sec, 'passes': passes, 'comb_bits': args.comb_bits, 'chunk': min(args.chunk, B), 'lanes': args.lanes,
        'steps': args.steps, 'warmup': args.warmup,
        'ms_median': {'sample': round(med[False] * 1e3, 2), 'all': round(med[True] * 1e3, 2)},
        'ms_min_max': {'sample': [round(min(runs[False]) * 1e3, 2), round(max(runs[False]) * 1e3, 2)], 'all': [round(min(runs[True]) * 1e3, 2), round(max(runs[True]) * 1e3, 2)]},
        'verifies_k_per_s': {'sample': round(B / med[False] / 1e3, 1), 'all': round(B / med[True] / 1e3, 1)},
        'all_over_sample_time': round(med[True] / med[False], 3),
        'latency_b1_ms': {'sample': round(statistics.median(lat[False]) * 1e3, 3), 'all': round(statistics.median(lat[True]) * 1e3, 3)},
        'families_one_call': fam,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    e.close()


if __name__ == '__main__':
    main()
