"""-m gpu: zk_ctx_update_ring (include/zkattest.h).  A resident ring built from the key list L and updated in place must be, in everything a caller can
observe, the ring zk_ctx_set_ring builds from the new list L': zk_ring_info, the digest, the bytes of every proof (also against the oracle over L'), the
verdicts of the three verify entry points -- proofs made over L no longer verify, as the oracle with ring L' says --, in hardened mode and on a pool.
Work counters (zk_test_counter 5 and 6) show that only the touched keys and blocks were rebuilt.  The scenarios are those of tests/ring_update_cases.py;
the table-by-table comparison is tests/test_gpu_ring_update_tables.py."""
import ctypes as C
import hashlib

import pytest

import ring_update_cases as RU

pytestmark = pytest.mark.gpu

S = 6160
ZK_E_ARG = 14
NAMES = ['interior', 'key0', 'append_inside', 'append_past', 'truncate_inside', 'truncate_past', 'duplicate']


def _vseeds(n, tag):
    return b''.join(hashlib.sha256(tag + i.to_bytes(4, 'big')).digest() for i in range(n))


def _off(plist):
    off = (C.c_uint64 * (len(plist) + 1))()
    o = 0
    for b, p in enumerate(plist):
        off[b] = o
        o += len(p)
    off[len(plist)] = o
    return off


def _device(eng, msgs, plist, vs):
    import torch
    B = len(plist)
    dev = 'cuda:0'
    d_msg = torch.frombuffer(bytearray(msgs), dtype=torch.uint8).to(dev)
    d_pr = torch.frombuffer(bytearray(b''.join(plist)), dtype=torch.uint8).to(dev)
    d_off = torch.tensor(list(_off(plist)), dtype=torch.int64).to(dev)
    d_vs = torch.frombuffer(bytearray(vs), dtype=torch.uint8).to(dev)
    d_ok = torch.zeros(B, dtype=torch.uint8, device=dev)
    d_st = torch.full((B,), -1, dtype=torch.int32, device=dev)
    eng.verify_batch_device(B, d_msg.data_ptr(), d_pr.data_ptr(), d_off.data_ptr(), d_vs.data_ptr(), d_ok.data_ptr(), d_st.data_ptr())
    torch.cuda.synchronize()
    return d_ok.cpu().tolist(), d_st.cpu().tolist()


def _batch(work, m, N):
    """The batch proved over a list of m keys padded to N: which = b for b < min(256, m), the changed position 300, and key 0's signer at a PADDING position."""
    B = len(work[4])
    idx = RU.batch_indices(m, (300,), B)
    which = [work[4][i] for i in idx]
    if m < N:
        idx, which = idx + [0], which + [m]
    return RU.cut(work, idx, which)


class _Fx:
    def __init__(self):
        import zkp_ecdsa_amd as Z
        self.Z = Z
        self.Y = Z.Engine(0)
        self.params = self.Y.synth_params(S)
        self.Y.set_params(*self.params, 80)
        self.work, self.W, self.X, self.other, self.ycache = {}, {}, {}, {}, {}

    def engine(self, mode=0):
        e = self.Z.Engine(0)
        e.set_params(*self.params, 80)
        return e

    def size(self, n):
        """the workload of ring size n, and the context X of that size with an untouched ring of 8 keys resident beside the rings under test"""
        if n not in self.X:
            self.work[n] = self.Y.synth_workload(S + n, n, RU.SIZES[n])
            self.W[n] = RU.split(self.work[n][0])
            X = self.engine()
            ow = X.synth_workload(S + 99, 8, 4)
            oid = X.add_ring(ow[0], 8)
            X.use_ring(oid)
            op, st = X.prove_batch(ow[1], ow[2], ow[3], ow[4], seeds=ow[5])
            assert st == [0] * 4
            self.X[n], self.other[n] = X, (oid, ow[1], op)
        return self.X[n], self.work[n], self.W[n], self.other[n]

    def fresh(self, n, Lp):
        """what a context handed L' by zk_ctx_set_ring reports and proves"""
        key = (n, len(Lp))
        if key not in self.ycache:
            Y, m = self.Y, len(Lp)
            Y.set_ring(b''.join(Lp), m)
            info = Y.ring_info(0)   # (zk_ctx_set_ring rebuilds the context's one ring in place, under its id)
            assert info['flags'] & 16
            msg, sig, pk, which, seeds = _batch(self.work[n], m, 1 << info['log_n'])
            proofs, st = Y.prove_batch(msg, sig, pk, which, seeds=seeds)
            assert st == [0] * len(which), st
            self.ycache[key] = {'info': info, 'digest': Y.ring_digest(), 'proofs': proofs, 'kt': Y.test_counter(1)}
        return self.ycache[key]

    def close(self):
        for e in list(self.X.values()) + [self.Y]:
            e.close()


@pytest.fixture(scope='module')
def fx():
    f = _Fx()
    yield f
    f.close()


def _oracle_digest(Lp):
    import zkattest_ref as R
    padded = [v.k for v in R.pad([int.from_bytes(k, 'big') for k in Lp], R.tomEdwards256)]
    return R.ring_digest(padded)


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('n', [8, 1000, 5000])
def test_updated_ring_equals_a_fresh_one(fx, n, name):
    import coracle as CO
    Z = fx.Z
    X, work, W, (oid, omsg, oproofs) = fx.size(n)
    _, L, changes, new_n, Lp, fast = [s for s in RU.scenarios(W) if s[0] == name][0]
    changed = {i for i, _ in changes}
    rid = X.add_ring(b''.join(L), len(L))
    X.use_ring(rid)
    before = X.ring_info(rid)
    # proofs over L by signers whose keys the update leaves alone
    keep = [i for i in range(min(len(L), new_n, len(work[4]))) if i not in changed][:4]
    omsgs, osig, opk, owhich, oseeds = RU.cut(work, keep)
    old, st = X.prove_batch(omsgs, osig, opk, owhich, seeds=oseeds)
    assert st == [0] * len(keep)
    assert X.verify_batch(omsgs, old, vseeds=_vseeds(len(old), b'pre')) == ([1] * len(old), [0] * len(old))

    X.update_ring(rid, changes, new_n)

    Y = fx.fresh(n, Lp)
    after = X.ring_info(rid)
    assert (after['n_keys'], after['log_n']) == (new_n, Y['info']['log_n'])
    assert after['generation'] == before['generation'] + 1
    assert after['flags'] == (before['flags'] if fast else Y['info']['flags'])
    assert after['flags'] & Z.RING_ACTIVE
    assert X.ring_digest() == Y['digest'] == _oracle_digest(Lp)

    # the prover: byte for byte what the fresh context and (on a sample) the oracle over L' emit
    N = 1 << after['log_n']
    msg, sig, pk, which, seeds = _batch(work, new_n, N)
    B = len(which)
    proofs, st = X.prove_batch(msg, sig, pk, which, seeds=seeds)
    assert st == [0] * B
    assert proofs == Y['proofs']
    if after['flags'] & Z.RING_KEY_TABLES:
        kt = X.test_counter(1)
        print('%s/%d: %d of %d proofs took the key-table path (fresh context: %d)' % (name, n, kt, B, Y['kt']))
        assert kt == Y['kt'] and kt > 0
    sample = [0] + [b for b in range(1, B) if which[b] in changed][:3] + [B - 1]   # index 0, changed positions, the padding position where there is one
    for b in range(1, B, max(1, B // 7)):
        if len(set(sample)) < min(8, B):
            sample.append(b)
    sample = sorted(set(sample))
    assert len(sample) >= min(8, B) and 0 in sample
    orc = CO.OracleCtx(*fx.params, 80)
    orc.set_ring(b''.join(Lp), new_n)
    pick = lambda a, w: b''.join(a[w * i:w * i + w] for i in sample)
    exp, est = orc.prove_batch(pick(msg, 32), pick(sig, 64), pick(pk, 64), [which[i] for i in sample], seeds=pick(seeds, 32), nthreads=16)
    assert est == [0] * len(sample) and exp == [proofs[i] for i in sample]

    # the verifier: proofs over L' pass; proofs over L get what the oracle over L' gives them: ok 0, and status 0 (a failed membership check) wherever the
    # padded size, hence the proof's layout, stayed
    vm = msg + omsgs
    vp = proofs + old
    vs = _vseeds(len(vp), b'upd')
    ook, ost = orc.verify_batch(pick(msg, 32) + omsgs, [proofs[i] for i in sample] + old, nthreads=16, vseeds=vs[:32 * (len(sample) + len(old))])
    orc.close()
    assert (ook[:len(sample)], ost[:len(sample)]) == ([1] * len(sample), [0] * len(sample))
    assert ook[len(sample):] == [0] * len(old)
    if fast:
        assert ost[len(sample):] == [0] * len(old)
    want = ([1] * B + [0] * len(old), [0] * B + ost[len(sample):])
    assert X.verify_batch(vm, vp, vseeds=vs) == want
    assert _device(X, vm, vp, vs) == want
    if n == 5000:   # the fold above ran on the matrix pipe (gk_kdig); the vector-ALU fold over table E must agree
        assert after['flags'] & Z.RING_DIGIT_PLANES
        X.set_ring_fold(False)
        assert X.verify_batch(vm, vp, vseeds=vs) == want
        X.set_ring_fold(True)
    # mixed-ring call with the untouched ring interleaved; the active ring does not matter
    X.use_ring(oid)
    pos = list(range(0, B, max(1, B // 12)))[:12] + list(range(B, B + len(old)))
    mm, mp, ids, mw = [], [], [], []
    for j, i in enumerate(pos):
        mm.append(vm[32 * i:32 * i + 32]), mp.append(vp[i]), ids.append(rid), mw.append(want[0][i])
        mm.append(omsg[32 * (j % 4):32 * (j % 4) + 32]), mp.append(oproofs[j % 4]), ids.append(oid), mw.append(1)
    assert X.verify_batch_rings(b''.join(mm), mp, ids, vseeds=_vseeds(len(mp), b'mix')) == (mw, [0] * len(mp))
    X.drop_ring(rid)


def test_hardened_mode_hashes_the_new_digest(fx):
    Z = fx.Z
    _, work, W, _ = fx.size(1000)
    _, L, changes, new_n, Lp, _ = RU.scenarios(W)[0]
    nh, th = Z.hardened_h(b'ring-update')
    made = {}
    engs = {}
    for side in ('X', 'Y'):
        e = Z.Engine(0)
        e.set_params(nh, fx.params[1], th, 80)
        e.set_mode(Z.MODE_HARDENED)
        if side == 'X':
            rid = e.add_ring(b''.join(L), len(L))
            e.use_ring(rid)
            e.update_ring(rid, changes, new_n)
        else:
            e.set_ring(b''.join(Lp), new_n)
        msg, sig, pk, which, seeds = RU.cut(work, [0, 7, 130, 300, 5])
        made[side], st = e.prove_batch(msg, sig, pk, which, seeds=seeds)
        assert st == [0] * 5
        engs[side] = e
    assert made['X'] == made['Y']
    vs = _vseeds(5, b'hard')
    assert engs['Y'].verify_batch(msg, made['X'], vseeds=vs) == ([1] * 5, [0] * 5)
    assert engs['X'].verify_batch(msg, made['Y'], vseeds=vs) == ([1] * 5, [0] * 5)
    stale = Z.Engine(0)   # a context still on L: another digest in the challenge, nothing verifies
    stale.set_params(nh, fx.params[1], th, 80)
    stale.set_mode(Z.MODE_HARDENED)
    stale.set_ring(b''.join(L), len(L))
    assert stale.verify_batch(msg, made['X'], vseeds=vs)[0] == [0] * 5
    for e in list(engs.values()) + [stale]:
        e.close()


def test_work_counters_and_refusals(fx):
    Z = fx.Z
    X, work, W, (oid, _, _) = fx.size(5000)
    sc = {s[0]: s for s in RU.scenarios(W)}
    _, L, changes, new_n, Lp, _ = sc['interior']
    rid = X.add_ring(b''.join(L), len(L))
    assert X.ring_info(rid)['flags'] & Z.RING_KEY_TABLES and X.ring_info(rid)['flags'] & Z.RING_TABLE_E
    c5, c6, gen = X.test_counter(5), X.test_counter(6), X.ring_info(rid)['generation']
    X.update_ring(rid, [], 5000)   # the no-op
    assert (X.test_counter(5), X.test_counter(6), X.ring_info(rid)['generation']) == (c5, c6, gen)
    X.update_ring(rid, changes, new_n)
    print('interior update of 3 keys: counter 5 +%d, counter 6 +%d' % (X.test_counter(5) - c5, X.test_counter(6) - c6))
    assert X.test_counter(5) == c5 + 3
    assert X.test_counter(6) == c6 + 2
    c5, c6 = X.test_counter(5), X.test_counter(6)
    X.update_ring(rid, [(0, RU.junk(0))], 5000)   # key 0: the 3192 padding entries follow it, their tables by copy
    print('key 0 replaced: counter 5 +%d, counter 6 +%d' % (X.test_counter(5) - c5, X.test_counter(6) - c6))
    assert 1 <= X.test_counter(5) - c5 <= 1 + (8192 - 5000)
    assert X.test_counter(6) - c6 == 1 + (8192 // 256 - 5000 // 256)   # block 0 and the blocks that hold padding (19 .. 31)
    X.update_ring(rid, [(0, W[0])], 5000)
    assert X.ring_info(rid)['generation'] == gen + 3

    X.use_ring(rid)
    digest, gen = X.ring_digest(), X.ring_info(rid)['generation']

    def refused(call):
        with pytest.raises(Z.ZkError) as e:
            call()
        assert e.value.status == ZK_E_ARG and str(e.value)

    refused(lambda: X.update_ring(rid, [(5000, RU.junk(1))], 5000))                  # an index out of range
    refused(lambda: X.update_ring(rid, [(5000, RU.junk(1)), (5002, RU.junk(2))], 5003))   # position 5001 is missing
    refused(lambda: X.update_ring(rid, [(0, RU.junk(1))], 1))                        # a ring of one key
    refused(lambda: X.update_ring(4242, [(0, RU.junk(1))], 5000))                    # an unknown id
    # through the C ABI: NULL index / keys with count > 0, and a key count whose padded size does not fit 64 bits
    L_, idx1 = Z.lib(), (C.c_uint64 * 1)(3)
    assert L_.zk_ctx_update_ring(X.h, rid, 1, None, RU.junk(3), 5000) == ZK_E_ARG
    assert L_.zk_ctx_update_ring(X.h, rid, 1, idx1, None, 5000) == ZK_E_ARG
    assert L_.zk_last_error(X.h)
    for huge in ((1 << 63) + 1, (1 << 64) - 1, (1 << 40)):
        assert L_.zk_ctx_update_ring(X.h, rid, 1, idx1, RU.junk(3), huge) == ZK_E_ARG
    assert (X.ring_digest(), X.ring_info(rid)['generation']) == (digest, gen)
    msg, sig, pk, which, seeds = RU.cut(work, [1, 2])
    pin = Z.PinnedBuffer(X.proof_max_size() * 2 + 4096)
    t = X.prove_submit(msg, sig, pk, which, seeds, pin)
    refused(lambda: X.update_ring(rid, [(3, RU.junk(3))], 5000))                     # a streamed job is queued
    off, st = X.prove_wait(t)
    assert list(st) == [0, 0]
    assert (X.ring_digest(), X.ring_info(rid)['generation']) == (digest, gen)
    assert X.verify_batch(msg, [bytes(pin.view[off[i]:off[i + 1]]) for i in range(2)]) == ([1, 1], [0, 0])
    pin.free()
    X.use_ring(oid)
    X.drop_ring(rid)


def test_pool_of_two_contexts_on_device_0(fx):
    Z = fx.Z
    X, work, W, _ = fx.size(1000)
    _, L, changes, new_n, Lp, _ = RU.scenarios(W)[0]
    pool = Z.Pool([0, 0])
    pool.set_params(*fx.params, 80)
    other = pool.engine(0).synth_workload(S + 99, 8, 4)
    oid = pool.add_ring(other[0], 8)
    rid = pool.add_ring(b''.join(L), len(L))
    single = fx.engine()
    assert (single.add_ring(other[0], 8), single.add_ring(b''.join(L), len(L))) == (oid, rid)
    omsg, osig, opk, owhich, oseeds = RU.cut(work, [0, 9, 11, 1, 2, 5])   # signers whose keys the update leaves alone
    msg, sig, pk, which, seeds = RU.cut(work, [0, 7, 130, 300, 9, 11])
    pool.use_ring(rid)
    old, st = pool.prove_batch(omsg, osig, opk, owhich, seeds=oseeds)   # over L
    assert st == [0] * 6
    pool.update_ring(rid, changes, new_n)
    single.update_ring(rid, changes, new_n)
    gens = [pool.engine(i).ring_info(rid)['generation'] for i in range(2)]
    assert gens[0] == gens[1] == single.ring_info(rid)['generation']
    assert [pool.engine(i).ring_info(rid)['n_keys'] for i in range(2)] == [new_n] * 2
    new, st = pool.prove_batch(msg, sig, pk, which, seeds=seeds)
    assert st == [0] * 6
    pool.use_ring(oid)
    op, st = pool.prove_batch(other[1], other[2], other[3], other[4], seeds=other[5])
    assert st == [0] * 4
    mm = msg + omsg + other[1]
    mp = new + old + op
    ids = [rid] * 12 + [oid] * 4
    vs = _vseeds(16, b'pool')
    got = pool.verify_batch_rings(mm, mp, ids, vseeds=vs)
    assert got == ([1] * 6 + [0] * 6 + [1] * 4, [0] * 16)
    assert got == single.verify_batch_rings(mm, mp, ids, vseeds=vs)
    with pytest.raises(Z.ZkError):
        pool.update_ring(rid, [(1000, RU.junk(5))], 1000)
    assert [pool.engine(i).ring_info(rid)['generation'] for i in range(2)] == gens
    single.close()
    pool.close()
