"""Mixed-ring membership calls (include/zkattest.h: zk_member_prove_batch_rings_device / zk_member_verify_batch_rings_device), measured: --batch proofs
(65 536) split evenly and interleaved over two resident rings of --ring-a (2^16) and --ring-b (2^12) keys, every buffer device-resident, one process, one GPU.

Recorded: the wall time of the mixed prove call and of the mixed verify call (median of --reps calls after one warm-up call) and the GPU time of their
families (zk_last_timing: the one-ring families summed over the windows, plus "m_class" and "m_gather").  Beside them the yardstick of the same build in the
same run: the same inputs grouped by ring, proved and verified by the two one-ring device calls (zk_ctx_use_ring between them), whose wall times are summed.
mixed_over_grouped is the ratio; overhead_ms is what the mixed call costs above the grouped calls, to be held against m_class + m_gather -- the time of
classing the ids and moving the inputs once.
  python tools/member_rings_rate.py [--batch 65536] [--ring-a 65536] [--ring-b 4096] [--reps 5] [--out profiles/member_rings_rate.json]
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
    ap.add_argument('--ring-a', type=int, default=65536)
    ap.add_argument('--ring-b', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    args = ap.parse_args()
    import torch
    import zkp_ecdsa_amd as Z
    S, B, dev = 20261020, args.batch, 'cuda:0'
    half = B // 2
    assert B == 2 * half, 'an even batch: half of it per ring'
    res = {'tool': 'member_rings_rate', 'batch': B, 'rings': [args.ring_a, args.ring_b], 'reps': args.reps}

    def up(b, dtype=torch.uint8):
        return torch.frombuffer(bytearray(b), dtype=dtype).to(dev)

    e = Z.Engine(0)
    e.set_timing(1)
    e.set_params(*e.synth_params(S), 80)
    work = [e.synth_workload(S + k, n, half) for k, n in enumerate((args.ring_a, args.ring_b))]
    rid = [e.add_ring(w[0], n) for w, n in zip(work, (args.ring_a, args.ring_b))]
    size = [e.member_proof_size(r) for r in rid]
    res['proof_bytes'] = size
    # grouped by ring: ring a's half, then ring b's; interleaved: a, b, a, b, ...
    g_which = [torch.tensor(w[4], dtype=torch.int32).to(dev) for w in work]
    g_seeds = [up(w[5]) for w in work]
    m_which = torch.stack(g_which, dim=1).reshape(-1).contiguous()
    m_seeds = torch.stack([s.reshape(half, 32) for s in g_seeds], dim=1).reshape(-1).contiguous()
    m_ids = torch.tensor(rid, dtype=torch.int32).repeat(half).to(dev)
    total = half * (size[0] + size[1])
    m_com, m_out = torch.empty(72 * B, dtype=torch.uint8, device=dev), torch.empty(total, dtype=torch.uint8, device=dev)
    m_off, m_st, m_ok = torch.zeros(B + 1, dtype=torch.int64, device=dev), torch.ones(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
    g_com = [torch.empty(72 * half, dtype=torch.uint8, device=dev) for _ in rid]
    g_out = [torch.empty(size[k] * half, dtype=torch.uint8, device=dev) for k in range(2)]
    g_st, g_ok = torch.ones(half, dtype=torch.int32, device=dev), torch.zeros(half, dtype=torch.uint8, device=dev)

    def timed(call):
        walls, fams = [], []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fam = call()
            walls.append((time.perf_counter() - t0) * 1e3)
            fams.append(fam)
        keys = sorted(set().union(*fams[1:]))
        return statistics.median(walls[1:]), {k: round(statistics.median(f.get(k, 0.0) for f in fams[1:]), 3) for k in keys}

    def mixed_prove():
        e.member_prove_batch_rings_device(B, m_which.data_ptr(), m_ids.data_ptr(), None, m_seeds.data_ptr(), m_com.data_ptr(), None, m_out.data_ptr(), total, m_off.data_ptr(),
                                          m_st.data_ptr())
        return e.last_timing()[1]

    def mixed_verify():
        e.member_verify_batch_rings_device(B, m_com.data_ptr(), m_out.data_ptr(), m_off.data_ptr(), m_ids.data_ptr(), None, m_ok.data_ptr(), m_st.data_ptr())
        return e.last_timing()[1]

    def grouped(one):
        fam = {}
        for k in range(2):
            e.use_ring(rid[k])
            one(k)
            for name, ms in e.last_timing()[1].items():
                fam[name] = fam.get(name, 0.0) + ms
        return fam

    def grouped_prove():
        return grouped(lambda k: e.member_prove_batch_device(half, g_which[k].data_ptr(), None, g_seeds[k].data_ptr(), g_com[k].data_ptr(), None, g_out[k].data_ptr(),
                                                             size[k] * half, g_st.data_ptr()))

    def grouped_verify():
        return grouped(lambda k: e.member_verify_batch_device(half, g_com[k].data_ptr(), g_out[k].data_ptr(), None, g_ok.data_ptr(), g_st.data_ptr()))

    w0 = e.test_counter(13)
    for name, mixed, plain in (('prove', mixed_prove, grouped_prove), ('verify', mixed_verify, grouped_verify)):
        ms, fam = timed(mixed)
        torch.cuda.synchronize()
        assert int(m_st.abs().sum()) == 0 and (name == 'prove' or int(m_ok.sum()) == B), 'the mixed %s call failed a proof' % name
        gms, gfam = timed(plain)
        torch.cuda.synchronize()
        assert int(g_st.abs().sum()) == 0
        moved = fam.get('m_class', 0.0) + fam.get('m_gather', 0.0)
        res[name] = {'mixed_ms': round(ms, 3), 'mixed_per_s': round(B / ms * 1e3), 'mixed_families_ms': fam, 'grouped_ms': round(gms, 3), 'grouped_per_s': round(B / gms * 1e3),
                     'grouped_families_ms': gfam, 'mixed_over_grouped': round(ms / gms, 4), 'overhead_ms': round(ms - gms, 3), 'm_class_plus_m_gather_ms': round(moved, 3)}
    res['windows_per_mixed_call'] = (e.test_counter(13) - w0) // (2 * (args.reps + 1))
    # the mixed call's bytes are the grouped calls': proof k of ring a is mixed proof 2 k
    mixed = m_out.cpu().numpy().tobytes()
    step = size[0] + size[1]
    ga, gb = g_out[0].cpu().numpy().tobytes(), g_out[1].cpu().numpy().tobytes()
    for k in (0, 1, half // 2, half - 1):
        assert mixed[step * k:step * k + size[0]] == ga[size[0] * k:size[0] * (k + 1)] and mixed[step * k + size[0]:step * (k + 1)] == gb[size[1] * k:size[1] * (k + 1)], k
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
