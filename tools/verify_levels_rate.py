"""Per-proof verify levels (include/zkattest.h: zk_ctx_set_verify_level), measured: device-resident proofs, one process, one GPU.

  (a) default mode, every proof at the context's level 80
  (b) per-proof mode, the same proofs
  (c) per-proof mode on a context at 80, every proof at 128 -- against a context set to 128 in the default mode (1 024 distinct proofs at 128, tiled)
  (d) per-proof mode, proofs alternating 80 / 128 (the census, the partition and one window per level)
  (e) one proof per call through device pointers: per-proof mode (census + one read-back) against the default

Two contexts (at 80 and at 128) with 3 lanes of 8 192-proof chunks each: at 128 a lane's workspaces take ~1.5 MB per proof.
The modes are alternated step by step, so that a drifting clock affects both sides alike.  Every call's verdicts are checked (all accept).
  python tools/verify_levels_rate.py [--ring 65536] [--batch 65536] [--steps 3] [--warmup 1] [--comb-bits 16] [--chunk 8192] [--lanes 3]
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
    ap.add_argument('--ring', type=int, default=65536)
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--comb-bits', type=int, default=16)
    ap.add_argument('--chunk', type=int, default=8192)
    ap.add_argument('--lanes', type=int, default=3)
    ap.add_argument('--latency-calls', type=int, default=200)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import zkp_ecdsa_amd as Z
    dev = 'cuda:0'
    S, B, nkeys = 20261016, args.batch, args.ring

    def engine(sec):
        e = Z.Engine(0)
        e.set_comb_bits(args.comb_bits)
        e.set_key_tables(False)   # prover-only tables (17.7 GB per context at 2^16 keys): two contexts and their workspaces at 128 must fit
        e.set_params(nh, tg, th, sec)
        e.set_ring(ring, nkeys)
        e.set_chunk(min(args.chunk, B)), e.set_lanes(args.lanes)
        return e

    e0 = Z.Engine(0)
    nh, tg, th = e0.synth_params(S)
    ring, msg, sig, pk, which, seeds = e0.synth_workload(S, nkeys, B)
    e0.close()
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d_msg, d_sig, d_pk, d_seeds = t(msg), t(sig), t(pk), t(seeds)
    d_which = torch.tensor(which, dtype=torch.int32).to(dev)
    d_vseeds = t(os.urandom(32 * B))
    eng = {80: engine(80), 128: engine(128)}
    made = {}
    # honest proofs at each level, left in HBM.  At 80 all B of them, in the library's default chunks.  At 128 K distinct ones in chunks of 4 proofs, tiled
    # to B: the prover's list of zero-bit repetitions is sized for challenge bits that are uniform over secLevel, and above bit 80 they are all zero
    # (the challenge is 80 bits wide), so a prover chunk of more than a few proofs at 128 overflows it (ZK_E_BUFFER) -- a prover limit outside this tool.
    K = min(B, 1024)
    for sec, n in ((80, B), (128, K)):
        e = eng[sec]
        e.set_chunk(4096 if sec == 80 else 4)
        cap = int(n * e.proof_max_size() * 0.8)
        d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        d_st = torch.empty(n, dtype=torch.int32, device=dev)
        e.prove_batch_device(n, d_msg.data_ptr(), d_sig.data_ptr(), d_pk.data_ptr(), d_which.data_ptr(), d_seeds.data_ptr(), d_out.data_ptr(), cap,
                             d_off.data_ptr(), d_st.data_ptr())
        torch.cuda.synchronize()
        assert int((d_st != 0).sum()) == 0
        e.set_chunk(min(args.chunk, B))
        made[sec] = (d_out, d_off.cpu().tolist())

    def assemble(pick):   # pick(b) -> (level, index of the made proof, index of its message): one back-to-back batch of B proofs in HBM
        parts, msgs, offs, at = [], [], [0], 0
        for b in range(B):
            sec, k, m = pick(b)
            buf, o = made[sec]
            parts.append(buf[o[k]:o[k + 1]])
            msgs.append(m)
            at += o[k + 1] - o[k]
            offs.append(at)
        mi = torch.tensor(msgs, dtype=torch.int64, device=dev)
        return torch.cat(parts), torch.tensor(offs, dtype=torch.int64, device=dev), d_msg.view(-1, 32)[mi].contiguous().view(-1)

    set80 = (made[80][0], torch.tensor(made[80][1], dtype=torch.int64, device=dev), d_msg)
    set128 = assemble(lambda b: (128, b % K, b % K))
    mix = assemble(lambda b: (80, b, b) if b % 2 == 0 else (128, b % K, b % K))   # (d): alternating 80 / 128
    d_ok = torch.empty(B, dtype=torch.uint8, device=dev)
    d_vst = torch.empty(B, dtype=torch.int32, device=dev)

    def call(e, per_proof, proofs, off, msgs, n=B):
        e.set_verify_level(per_proof)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.verify_batch_device(n, msgs.data_ptr(), proofs.data_ptr(), off.data_ptr(), d_vseeds.data_ptr(), d_ok.data_ptr(), d_vst.data_ptr())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert int(d_ok[:n].sum()) == n and int((d_vst[:n] != 0).sum()) == 0, 'a verdict differs'
        return dt

    runs = {k: [] for k in ('a', 'b', 'c', 'c_ref', 'd')}
    for step in range(args.warmup + args.steps):
        r = {'a': call(eng[80], False, *set80), 'b': call(eng[80], True, *set80),
             'c': call(eng[80], True, *set128), 'c_ref': call(eng[128], False, *set128),
             'd': call(eng[80], True, *mix)}
        if step >= args.warmup:
            for k, v in r.items():
                runs[k].append(v)
    rate = {k: B / statistics.median(v) for k, v in runs.items()}
    hm = 2.0 / (1.0 / rate['b'] + 1.0 / rate['c'])
    lat = {False: [], True: []}
    for i in range(args.latency_calls):
        for pp in (False, True):
            lat[pp].append(call(eng[80], pp, *set80, n=1))
    l0, l1 = statistics.median(lat[False]) * 1e3, statistics.median(lat[True]) * 1e3
    res = {
        'tool': 'verify_levels_rate', 'batch': B, 'ring': nkeys, 'comb_bits': args.comb_bits, 'chunk': min(args.chunk, B), 'lanes': args.lanes, 'steps': args.steps,
        'ms_median': {k: round(statistics.median(v) * 1e3, 2) for k, v in runs.items()},
        'rate_k_per_s': {k: round(v / 1e3, 1) for k, v in rate.items()},
        'b_over_a': round(rate['b'] / rate['a'], 4), 'c_over_c_ref': round(rate['c'] / rate['c_ref'], 4),
        'd_over_harmonic_mean_b_c': round(rate['d'] / hm, 4),
        'latency_b1_ms': {'default': round(l0, 3), 'per_proof': round(l1, 3), 'added_us': round((l1 - l0) * 1e3, 1)},
        'targets': {'b_over_a': '>= 0.99', 'c_over_c_ref': '>= 0.99', 'd_over_harmonic_mean_b_c': '>= 0.85', 'latency_added_us': '<= ~30'},
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    for e in eng.values():
        e.close()


if __name__ == '__main__':
    main()
