"""Run by tests/test_gpu_prove_rings.py::test_segments_and_windows_are_cut in its own process with ZKATTEST_LIB = lib/libzkattest_hip_testhooks.so (the
only build with zk_test_set_prove_segment; one process holds one build).  chunk 256 and one lane -- windows of at most 512 proofs --, two rings of 600
and 2100 keys x 520 proofs interleaved:
  default segment: one segment, every ring's 520 proofs cut into two windows;
  forced segment of 256 proofs: five segments (the last of 16 proofs), one window per ring in each;
  forced segment of 768: two segments.
Bytes, statuses and offsets equal the per-ring zk_prove_batch calls every time, through the host (pageable and page-locked `out`) and the device
entry point."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
S = 6363


def main():
    import torch   # (first: one HIP runtime in the process, see tests/conftest.py)
    import zkp_ecdsa_amd as Z
    assert hasattr(Z.lib(), 'zk_test_set_prove_segment'), 'not the test-hooks build'
    eng = Z.Engine(0)
    eng.set_params(*eng.synth_params(S), 80)
    eng.set_chunk(256)
    eng.set_lanes(1)
    B = 520
    W, ids, made = {}, {}, {}
    for k, n in (('A', 600), ('B', 2100)):
        W[k] = eng.synth_workload(S + n, n, B)
        ids[k] = eng.add_ring(W[k][0], n)
        eng.use_ring(ids[k])
        made[k], st = eng.prove_batch(*W[k][1:5], seeds=W[k][5])
        assert st == [0] * B
    col = lambda j, w: b''.join(W[k][j][w * i:w * i + w] for i in range(B) for k in ('A', 'B'))
    msg, sig, pk, seeds = col(1, 32), col(2, 64), col(3, 64), col(5, 32)
    which = [W[k][4][i] for i in range(B) for k in ('A', 'B')]
    rids = [ids[k] for i in range(B) for k in ('A', 'B')]
    want = [made[k][i] for i in range(B) for k in ('A', 'B')]
    total = sum(len(p) for p in want)
    pinned = Z.PinnedBuffer(total)
    dev = 'cuda:0'
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    d = [up(msg), up(sig), up(pk), torch.tensor(which, dtype=torch.int32).to(dev), torch.tensor(rids, dtype=torch.int32).to(dev), up(seeds)]
    for force, segs, wins in ((0, 1, 4), (256, 5, 10), (768, 2, 4)):
        eng.test_set_prove_segment(force)
        for how in ('pageable', 'page-locked', 'device'):
            s0, w0 = eng.test_counter(7), eng.test_counter(8)
            if how == 'device':
                d_out = torch.zeros(total, dtype=torch.uint8, device=dev)
                d_off = torch.full((2 * B + 1,), -1, dtype=torch.int64, device=dev)
                d_st = torch.full((2 * B,), -1, dtype=torch.int32, device=dev)
                eng.prove_batch_rings_device(2 * B, *[t.data_ptr() for t in d], d_out.data_ptr(), total, d_off.data_ptr(), d_st.data_ptr())
                torch.cuda.synchronize()
                off, st = d_off.cpu().tolist(), d_st.cpu().tolist()
                raw = d_out.cpu().numpy().tobytes()
                got = [raw[off[b]:off[b + 1]] for b in range(2 * B)]
                assert off[0] == 0 and off[-1] == total
            else:
                got, st = eng.prove_batch_rings(msg, sig, pk, which, rids, seeds=seeds, out=pinned if how == 'page-locked' else None)
            ds, dw = eng.test_counter(7) - s0, eng.test_counter(8) - w0
            print('segment %4d %-11s: %d segments, %d windows' % (force, how, ds, dw), flush=True)
            assert st == [0] * (2 * B), (force, how)
            assert got == want, (force, how)
            assert (ds, dw) == (segs, wins), (force, how, ds, dw)
            assert ds > 1 or force == 0
            assert dw > 2   # more than one window per ring
    pinned.free()
    eng.close()


if __name__ == '__main__':
    main()
    print('prove_rings_cut_check ok')
