"""Mixed-ring proving (include/zkattest.h: zk_prove_batch_rings), measured: one context, two rings of --ring keys, --batch device-resident proofs.

  (p) zk_prove_batch_device, ring A active (and ring B active)                              -- the one-ring rates
  (a) zk_prove_batch_rings_device, every id = A: census + one read-back, then the usual pipeline
  (b) zk_prove_batch_rings_device, proofs over A and B interleaved: partition, windows, staging, scan, byte mover
  (c) one proof per call through device pointers: (a)'s path against (p)'s

The variants are alternated step by step, so that a drifting clock affects them alike; medians of --steps.  Every call's statuses are checked.
With --parent-root PATH (a built checkout of the parent commit) the tool first runs three child processes one after the other on the same box -- parent, this
build's (a) alone, parent again: one process holds one build, and all three repeat one kind of call -- and reports (a) over the parent's zk_prove_batch_device next to the spread of the two parent runs; it exits non-zero when (a) over the parents' mean lies
outside [1 / spread, spread].
  python tools/prove_rings_rate.py [--ring 65536] [--batch 65536] [--steps 5] [--warmup 1] [--comb-bits 16] [--chunk 8192] [--lanes 3] [--parent-root PATH]
Prints one JSON line (also written to --out PATH when given)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(args):
    sys.path.insert(0, args.root or ROOT)   # the package (and its library) of this tree, or of the parent's checkout
    import torch
    import zkp_ecdsa_amd as Z
    dev = 'cuda:0'
    S, B, nkeys = 20261017, args.batch, args.ring
    have = hasattr(Z.lib(), 'zk_prove_batch_rings_device')   # (a parent build has the one-ring call only)
    e = Z.Engine(0)
    e.set_comb_bits(args.comb_bits)
    e.set_params(*e.synth_params(S), 80)
    e.set_chunk(min(args.chunk, B)), e.set_lanes(args.lanes)
    t = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    ids, inp = {}, {}
    for k, seed in (('A', S), ('B', S + 1)):
        ring, msg, sig, pk, which, seeds = e.synth_workload(seed, nkeys, B)
        ids[k] = e.add_ring(ring, nkeys)
        inp[k] = (t(msg), t(sig), t(pk), torch.tensor(which, dtype=torch.int32).to(dev), t(seeds))
    e.use_ring(ids['A'])
    free0, total = torch.cuda.mem_get_info()
    cap = B * e.proof_max_size()
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    d_st = torch.empty(B, dtype=torch.int32, device=dev)
    # (b): input b of A for even b, of B for odd b
    even = (torch.arange(B, device=dev) % 2 == 0)
    mixed = tuple(torch.where(even.view(-1, 1), a.view(B, -1), b.view(B, -1)).contiguous().view(-1) for a, b in zip(inp['A'], inp['B']))
    idsA = torch.full((B,), ids['A'], dtype=torch.int32, device=dev)
    idsMix = torch.where(even, torch.tensor(ids['A'], dtype=torch.int32, device=dev), torch.tensor(ids['B'], dtype=torch.int32, device=dev)).contiguous()

    def call(cols, rids=None, n=B):
        m, s, p, w, sd = cols
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if rids is None:
            e.prove_batch_device(n, m.data_ptr(), s.data_ptr(), p.data_ptr(), w.data_ptr(), sd.data_ptr(), d_out.data_ptr(), cap, d_off.data_ptr(), d_st.data_ptr())
        else:
            e.prove_batch_rings_device(n, m.data_ptr(), s.data_ptr(), p.data_ptr(), w.data_ptr(), rids.data_ptr(), sd.data_ptr(), d_out.data_ptr(), cap, d_off.data_ptr(),
                                       d_st.data_ptr())
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert int((d_st[:n] != 0).sum()) == 0, 'a proof failed'
        return dt

    runs = {k: [] for k in (('a',) if args.only_a else ('pA', 'pB', 'a', 'b') if have else ('pA',))}
    stage_gb = seg_per_call = win_per_call = None
    for step in range(args.warmup + args.steps):
        if args.only_a:   # the parent child's call pattern -- one kind of call, back to back -- with the new entry point
            dt = call(inp['A'], rids=idsA)
            if step >= args.warmup:
                runs['a'].append(dt)
            continue
        r = {'pA': call(inp['A'])}
        if have:
            r['a'] = call(inp['A'], rids=idsA)
            e.use_ring(ids['B'])
            r['pB'] = call(inp['B'])
            e.use_ring(ids['A'])
            before, c7, c8 = torch.cuda.mem_get_info()[0], e.test_counter(7), e.test_counter(8)
            r['b'] = call(mixed, rids=idsMix)
            seg_per_call, win_per_call = e.test_counter(7) - c7, e.test_counter(8) - c8
            if step == 0:   # what the first mixed call allocated: the staging buffer, the window and the partition's arrays
                stage_gb = round((before - torch.cuda.mem_get_info()[0]) / 1e9, 2)
        if step >= args.warmup:
            for k, v in r.items():
                runs[k].append(v)
    lat = {'p': [], 'a': []}
    for i in range(args.latency_calls):
        lat['p'].append(call(inp['A'], n=1))
        if have:
            lat['a'].append(call(inp['A'], rids=idsA, n=1))
    res = {'ms_all': {k: [round(x * 1e3, 2) for x in v] for k, v in runs.items()},
           'rate_k_per_s': {k: round(B / statistics.median(v) / 1e3, 1) for k, v in runs.items()},
           'latency_b1_ms': {k: round(statistics.median(v) * 1e3, 4) for k, v in lat.items() if v}}
    if have and not args.only_a:
        res['staging'] = {'proof_max_size': e.ring_proof_max_size(ids['A']), 'staging_buffer_gb': round(e.test_counter(9) / 1e9, 3),
                          'hbm_taken_by_first_mixed_call_gb': stage_gb, 'segments_per_mixed_call': seg_per_call, 'windows_per_mixed_call': win_per_call}
        res['key_tables_after'] = {k: bool(e.ring_info(ids[k])['flags'] & Z.RING_KEY_TABLES) for k in ids}
        res['hbm_used_gb'] = round((total - torch.cuda.mem_get_info()[0]) / 1e9, 1)
    print('CHILD ' + json.dumps(res), flush=True)
    e.close()


def run_child(args, root, only_a=False):
    env = dict(os.environ)
    env.pop('ZKATTEST_LIB', None)
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--root', root or ROOT, '--ring', str(args.ring), '--batch', str(args.batch), '--steps', str(args.steps), '--warmup', str(args.warmup),
           '--comb-bits', str(args.comb_bits), '--chunk', str(args.chunk), '--lanes', str(args.lanes), '--latency-calls', str(args.latency_calls)] + (['--only-a'] if only_a else [])
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    lines = [l for l in out.stdout.splitlines() if l.startswith('CHILD ')]
    if out.returncode or not lines:
        raise RuntimeError('child failed (%s): %s' % (root or 'this build', (out.stdout + out.stderr)[-2000:]))
    return json.loads(lines[-1][6:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ring', type=int, default=65536)
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--comb-bits', type=int, default=16)
    ap.add_argument('--chunk', type=int, default=8192)
    ap.add_argument('--lanes', type=int, default=3)
    ap.add_argument('--latency-calls', type=int, default=200)
    ap.add_argument('--parent-root', default=None, help='a built checkout of the parent commit: its zk_prove_batch_device is run before and after this build')
    ap.add_argument('--root', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--child-timeout', type=int, default=420)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--only-a', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = {'tool': 'prove_rings_rate', 'batch': args.batch, 'ring': args.ring, 'comb_bits': args.comb_bits, 'chunk': min(args.chunk, args.batch), 'lanes': args.lanes,
           'steps': args.steps}
    parents, alone = [], None
    if args.parent_root:   # three processes with ONE call pattern -- a single kind of call, back to back: parent, this build's (a), parent
        parents.append(run_child(args, args.parent_root))
        alone = run_child(args, None, only_a=True)
        parents.append(run_child(args, args.parent_root))
    new = run_child(args, None)   # ... and the four variants alternated in one process
    res['this_build'] = new
    r = new['rate_k_per_s']
    hm = 2.0 / (1.0 / r['pA'] + 1.0 / r['pB'])
    res['a_over_plain_same_process'] = round(r['a'] / r['pA'], 4)
    res['b_over_harmonic_mean_of_one_ring_rates'] = round(r['b'] / hm, 4)
    res['one_proof_added_us'] = round((new['latency_b1_ms']['a'] - new['latency_b1_ms']['p']) * 1e3, 1)
    if parents:
        p0, p1 = (p['rate_k_per_s']['pA'] for p in parents)
        ra = alone['rate_k_per_s']['a']
        res['parent_runs'], res['this_build_a_alone'] = parents, alone
        res['a_over_parent'] = [round(ra / p0, 4), round(ra / p1, 4)]
        res['parent_spread'] = round(max(p0, p1) / min(p0, p1), 4)   # two runs of the same code, before and after: what a ratio of 1 looks like on this box
        res['a_over_parent_mean'] = round(ra / ((p0 + p1) / 2), 4)
        res['a_inside_parent_spread'] = 1 / res['parent_spread'] <= res['a_over_parent_mean'] <= res['parent_spread']
        lp = statistics.mean(p['latency_b1_ms']['p'] for p in parents)
        res['one_proof_added_us_over_parent'] = round((alone['latency_b1_ms']['a'] - lp) * 1e3, 1)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    if parents and not res['a_inside_parent_spread']:
        sys.exit('(a) all ids equal is outside the spread of the two parent runs: %s against %s' % (res['a_over_parent_mean'], res['parent_spread']))


if __name__ == '__main__':
    main()
