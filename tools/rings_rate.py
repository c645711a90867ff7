"""Resident rings (include/zkattest.h: zk_ctx_add_ring, zk_verify_batch_rings), measured: one context, two rings of --ring keys, device-resident proofs.

  (s) switching: zk_ctx_set_ring (a rebuild of the active ring) against zk_ctx_use_ring between the two resident rings
  (a) zk_verify_batch_device, ring A active, --batch proofs over A
  (b) zk_verify_batch_rings_device, the same proofs, every id = A (census + one read-back, then the usual pipeline)
  (c) zk_verify_batch_rings_device, proofs over A and B interleaved (census, partition, one window per ring at a time)
  (e) one proof per call through device pointers: (b)'s path against (a)'s
  hbm_used_gb with both rings resident, and whether their key tables survived the workspaces (shed = given up for them)

The variants are alternated step by step, so that a drifting clock affects them alike.  Every call's verdicts are checked (all accept).
  python tools/rings_rate.py [--ring 65536] [--batch 65536] [--steps 3] [--warmup 1] [--comb-bits 16] [--chunk 8192] [--lanes 3]
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
    ap.add_argument('--switches', type=int, default=5)
    ap.add_argument('--latency-calls', type=int, default=200)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import zkp_ecdsa_amd as Z
    dev = 'cuda:0'
    S, B, nkeys = 20261016, args.batch, args.ring
    e = Z.Engine(0)
    e.set_comb_bits(args.comb_bits)
    nh, tg, th = e.synth_params(S)
    e.set_params(nh, tg, th, 80)
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    rings, made, ids = {}, {}, {}
    for k, seed in (('A', S), ('B', S + 1)):
        ring, msg, sig, pk, which, seeds = e.synth_workload(seed, nkeys, B)
        rings[k] = ring
        ids[k] = e.add_ring(ring, nkeys)
        e.use_ring(ids[k])
        e.set_chunk(4096)
        d_msg, d_sig, d_pk, d_seeds = t(msg), t(sig), t(pk), t(seeds)   # (held: a temporary's memory would be handed to the next one)
        cap = int(B * e.proof_max_size() * 0.8)
        d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        d_st = torch.empty(B, dtype=torch.int32, device=dev)
        d_which = torch.tensor(which, dtype=torch.int32).to(dev)
        e.prove_batch_device(B, d_msg.data_ptr(), d_sig.data_ptr(), d_pk.data_ptr(), d_which.data_ptr(), d_seeds.data_ptr(), d_out.data_ptr(), cap, d_off.data_ptr(),
                             d_st.data_ptr())
        torch.cuda.synchronize()
        assert int((d_st != 0).sum()) == 0, sorted(set(d_st.cpu().tolist()))
        made[k] = (d_out, d_off, d_msg)
        del d_sig, d_pk, d_seeds
    e.set_chunk(min(args.chunk, B)), e.set_lanes(args.lanes)
    e.use_ring(ids['A'])
    # (c): proof b over A for even b, over B for odd b
    offA, offB = made['A'][1].cpu().tolist(), made['B'][1].cpu().tolist()
    parts, msgs, offs, at = [], [], [0], 0
    for b in range(B):
        k, o = ('A', offA) if b % 2 == 0 else ('B', offB)
        parts.append(made[k][0][o[b]:o[b + 1]])
        msgs.append(made[k][2].view(-1, 32)[b])
        at += o[b + 1] - o[b]
        offs.append(at)
    mix = (torch.cat(parts), torch.tensor(offs, dtype=torch.int64, device=dev), torch.stack(msgs).contiguous().view(-1))
    del parts, msgs
    setA = (made['A'][0], made['A'][1], made['A'][2])
    idsA = torch.full((B,), ids['A'], dtype=torch.int32, device=dev)
    idsMix = torch.tensor([ids['A'] if b % 2 == 0 else ids['B'] for b in range(B)], dtype=torch.int32, device=dev)
    d_vseeds = t(os.urandom(32 * B))
    d_ok = torch.empty(B, dtype=torch.uint8, device=dev)
    d_vst = torch.empty(B, dtype=torch.int32, device=dev)

    def call(proofs, off, msgs, rids=None, n=B):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if rids is None:
            e.verify_batch_device(n, msgs.data_ptr(), proofs.data_ptr(), off.data_ptr(), d_vseeds.data_ptr(), d_ok.data_ptr(), d_vst.data_ptr())
        else:
            e.verify_batch_rings_device(n, msgs.data_ptr(), proofs.data_ptr(), off.data_ptr(), rids.data_ptr(), d_vseeds.data_ptr(), d_ok.data_ptr(), d_vst.data_ptr())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert int(d_ok[:n].sum()) == n and int((d_vst[:n] != 0).sum()) == 0, 'a verdict differs'
        return dt

    runs = {k: [] for k in ('a', 'b', 'c')}
    for step in range(args.warmup + args.steps):
        r = {'a': call(*setA), 'b': call(*setA, rids=idsA), 'c': call(*mix, rids=idsMix)}
        if step >= args.warmup:
            for k, v in r.items():
                runs[k].append(v)
    rate = {k: B / statistics.median(v) for k, v in runs.items()}
    lat = {'a': [], 'b': []}
    for i in range(args.latency_calls):
        lat['a'].append(call(*setA, n=1))
        lat['b'].append(call(*setA, rids=idsA, n=1))
    l0, l1 = statistics.median(lat['a']) * 1e3, statistics.median(lat['b']) * 1e3
    free, total = torch.cuda.mem_get_info()
    info = {k: e.ring_info(ids[k]) for k in ids}
    sw = {'set_ring': [], 'use_ring': []}
    for i in range(args.switches):   # ring A is active: rebuilt in place, then the switch to B and back
        t0 = time.perf_counter()
        e.set_ring(rings['A'], nkeys)
        sw['set_ring'].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        e.use_ring(ids['B'])
        e.use_ring(ids['A'])
        sw['use_ring'].append((time.perf_counter() - t0) / 2)
    res = {
        'tool': 'rings_rate', 'batch': B, 'ring': nkeys, 'comb_bits': args.comb_bits, 'chunk': min(args.chunk, B), 'lanes': args.lanes, 'steps': args.steps,
        'switch_ms': {k: round(statistics.median(v) * 1e3, 4) for k, v in sw.items()},
        'ms_median': {k: round(statistics.median(v) * 1e3, 2) for k, v in runs.items()},
        'rate_k_per_s': {k: round(v / 1e3, 1) for k, v in rate.items()},
        'b_over_a': round(rate['b'] / rate['a'], 4), 'c_over_a': round(rate['c'] / rate['a'], 4),
        'latency_b1_ms': {'verify_batch_device': round(l0, 3), 'verify_batch_rings_device': round(l1, 3), 'added_us': round((l1 - l0) * 1e3, 1)},
        'hbm_used_gb': round((total - free) / 1e9, 1),
        'key_tables': {k: bool(v['flags'] & Z.RING_KEY_TABLES) for k, v in info.items()},
        'targets': {'b_over_a': '>= 0.99', 'c_over_a': '>= 0.85', 'latency_added_us': '<= 20'},
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    e.close()


if __name__ == '__main__':
    main()
