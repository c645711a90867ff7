"""-m gpu: zk_rings_escrow_open_batch -- escrow tags opened against any resident ring through the rings' resident point indexes.  The tags come from the
engine's own prover over known keys; the expected answer is the lowest i with y_i = x (mod q) in the ring the tag names (or in the first resident ring, by
ascending id, that holds x), and for a handful of tags the Python statement's opening (tests/escrow_common.py).  secLevel 20, 12-bit context combs, chunks of
64 tags on 2 lanes; rings of 2, 5, 257 and 600 keys."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

SEC = 20
E_BAD, E_ARG, E_OPENING = 10, 14, 16
NONE = ANY = 0xffffffff


class Ctx:
    pass


def _engine(Z, par, A72=None, chunk=64):
    eng = Z.Engine(0)
    eng.set_comb_bits(12)
    eng.set_params(*par, SEC)
    eng.set_chunk(chunk)
    eng.set_lanes(2)
    if A72:
        eng.set_auditor(A72)
    return eng


def _tags(x, eng, name, keys):
    """tags of the engine's own prover for `keys` (fresh blinders and seeds by name)"""
    EC = x.EC
    _, r, seeds = EC.workload(name, len(keys))
    c = eng.test_tom_commit(keys, r)
    tags, st = eng.escrow_prove_batch(EC.be32(keys), c, EC.be32(r), seeds=seeds)
    assert st == [0] * len(keys)
    return tags


def _lowest(ring, key, Q):
    for i, y in enumerate(ring):
        if (y - key) % Q == 0:
            return i
    return NONE


def _expect(x, rings, keys, ids):
    """rings: {id: key list}; -> (ring_out, index, status) for tags of `keys` asked of `ids`"""
    out = []
    for key, want in zip(keys, ids):
        hit = (NONE, NONE)
        for rid in sorted(rings) if want == ANY else [want]:
            i = _lowest(rings[rid], key, x.EC.Q)
            if i != NONE:
                hit = (rid, i)
                break
        out.append(hit)
    return [h[0] for h in out], [h[1] for h in out], [0] * len(keys)


@pytest.fixture(scope='module')
def X():
    import escrow_common as EC
    import escrow_index_common as IC
    import zkp_ecdsa_amd as Z
    x = Ctx()
    x.Z, x.EC, x.IC, x.R = Z, EC, IC, EC.R
    boot = Z.Engine(0)
    x.par = boot.synth_params(EC.PARAM_SEED)
    boot.close()
    x.pp = EC.MC.oracle_params(x.par[1], x.par[2])
    x.a = int.from_bytes(EC.tag(b'auditor-rings', 0), 'big') % EC.Q
    x.a32 = x.a.to_bytes(32, 'big')
    x.A72 = x.R._tp(EC.keygen(x.pp, x.a))
    eng = x.eng = _engine(Z, x.par, x.A72)
    A, B = EC.scalars(b'ringA', 600), EC.scalars(b'ringB', 257)
    A[400] = A[37]              # one key at two indices of a ring
    A[599] = A[3] + 0           # ... and the last real key a copy too
    B[100] = A[5]               # one key enrolled in two rings
    B[256] = A[37]
    Cc, D = EC.scalars(b'ringC', 5), EC.scalars(b'ringD', 2)
    x.lists = [A, B, Cc, D]
    x.ids = [eng.add_ring(EC.be32(r), len(r)) for r in x.lists]
    assert x.ids == sorted(x.ids)
    x.rings = dict(zip(x.ids, x.lists))
    # 200 tags interleaved over the four rings, every block of 256 keys of A and B, first and last keys, the copies, and keys of no ring
    x.outside = EC.scalars(b'outside', 4)
    plan = []
    for b in range(188):
        r = b % 4
        n = len(x.lists[r])
        plan.append((r, [0, n - 1, (53 * b + 7) % n, (211 * b + 300) % n][(b // 4) % 4]))
    plan += [(0, 400), (0, 37), (0, 599), (1, 100), (0, 5), (1, 256), (0, 256), (0, 511)]
    x.plan = plan
    x.keys = [x.lists[r][i] for r, i in plan] + x.outside
    x.want_ids = [x.ids[r] for r, _ in plan] + [x.ids[0], x.ids[1], x.ids[2], x.ids[3]]
    assert len(x.keys) == 200
    x.tags = _tags(x, eng, b't200', x.keys)
    yield x
    eng.close()


def _open(x, eng, tags, ids):
    return eng.escrow_open_batch_rings(x.a32, tags, ids)


# ------------------------------------------------------------------ 2, 13: tags interleaved over the rings, four chunks on two lanes; no ring is active
def test_tags_interleaved_over_the_rings_without_an_active_ring(X):
    eng = X.eng
    assert not any(eng.ring_info(i)['flags'] & X.Z.RING_ACTIVE for i in X.ids)
    got = _open(X, eng, X.tags, X.want_ids)
    assert got == _expect(X, X.rings, X.keys, X.want_ids)
    ring, idx, st = got
    assert idx[:4] == [0, 0, 0, 0] and idx[188:196] == [37, 37, 3, 100, 5, 256, 256, 511] and idx[196:] == [NONE] * 4 and ring[196:] == [NONE] * 4
    assert not any(eng.ring_info(i)['flags'] & X.Z.RING_ACTIVE for i in X.ids)
    assert _open(X, eng, [], []) == ([], [], [])


# ------------------------------------------------------------------ 1: one id throughout equals zk_escrow_open_batch with that ring active
@pytest.mark.parametrize('r', [0, 1, 2, 3])
def test_one_id_throughout_equals_the_one_ring_call(X, r):
    eng = X.eng
    rid = X.ids[r]
    other = X.ids[(r + 1) % 4]
    eng.use_ring(other)
    ring, idx, st = _open(X, eng, X.tags, [rid] * 200)
    assert eng.ring_info(other)['flags'] & X.Z.RING_ACTIVE and not eng.ring_info(rid)['flags'] & X.Z.RING_ACTIVE   # the active ring: not read, not changed
    eng.use_ring(rid)
    assert eng.escrow_open_batch(X.a32, X.tags) == (idx, st)
    assert (ring, idx, st) == _expect(X, X.rings, X.keys, [rid] * 200)
    assert [w for w, i in zip(ring, idx) if i != NONE] == [rid] * sum(i != NONE for i in idx) and sum(i != NONE for i in idx) >= 47


# ------------------------------------------------------------------ 3, 4: any ring; a key in two rings; a key twice in a ring; the Python statement
def test_any_ring_two_rings_two_indices_and_the_python_opening(X):
    eng, EC = X.eng, X.EC
    ring, idx, st = _open(X, eng, X.tags, [ANY] * 200)
    assert (ring, idx, st) == _expect(X, X.rings, X.keys, [ANY] * 200)
    # B[100] = A[5] and B[256] = A[37] open to ring A under "any", to B when B is named; A[400] = A[37] to index 37; a key of no ring to nothing
    assert (ring[191], idx[191]) == (X.ids[0], 5) and (ring[193], idx[193]) == (X.ids[0], 37) and (ring[188], idx[188]) == (X.ids[0], 37)
    named = _open(X, eng, [X.tags[191], X.tags[193], X.tags[188]], [X.ids[1], X.ids[1], X.ids[0]])
    assert named == ([X.ids[1], X.ids[1], X.ids[0]], [100, 256, 37], [0, 0, 0])
    assert ring[196:] == [NONE] * 4 and idx[196:] == [NONE] * 4 and st[196:] == [0] * 4
    # the Python statement's opening for the tags of the two small rings and one outsider
    for r in (2, 3):
        table = EC.ring_points(X.pp, X.lists[r])
        for b in [b for b in range(16) if X.plan[b][0] == r] + [196]:
            assert EC.open_tag(X.a, X.tags[b], table) == (_lowest(X.lists[r], X.keys[b], EC.Q), 0), (r, b)
            assert _open(X, eng, [X.tags[b]], [X.ids[r]])[1:] == ([_lowest(X.lists[r], X.keys[b], EC.Q)], [0])


# ------------------------------------------------------------------ 5: three points at the last slot of a 16-slot table: the wrap, on the device
def test_crafted_ring_whose_points_share_the_last_slot(X):
    eng, EC, IC = X.eng, X.EC, X.IC
    g4 = EC.times4(X.pp.g)
    y0 = EC.scalars(b'craft', 1)[0]
    P, last, rest = EC.times4(X.pp.g.mul(EC.sc(y0))), [], []
    for k in range(400):   # 4 (y0 + k) g by one addition per candidate; the home slot by the restated function, for 16 slots
        (last if IC.home_of_point(X.R._tp(P), 16) == 15 else rest).append((y0 + k) % EC.Q)
        if len(last) >= 4 and len(rest) >= 2:
            break
        P = P.add(g4)
    assert len(last) >= 4 and len(rest) >= 2
    ring = [last[0], rest[0], last[1], last[2], rest[1]]
    assert IC.slots(len(ring)) == 16
    rid = eng.add_ring(EC.be32(ring), 5)
    try:
        keys = ring + [last[3], X.outside[0]]   # ... and an absent point that starts at slot 15 and walks the wrapped cluster to its end
        tags = _tags(X, eng, b'craft', keys)
        assert _open(X, eng, tags, [rid] * 7) == ([rid] * 5 + [NONE] * 2, [0, 1, 2, 3, 4, NONE, NONE], [0] * 7)
        table = EC.ring_points(X.pp, ring)
        assert [IC.home_of_point(t, 16) for t in table].count(15) == 3
        assert [EC.open_tag(X.a, t, table) for t in tags] == [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (NONE, 0), (NONE, 0)]
        eng.update_ring(rid, {1: EC.be32([last[3]])})   # a fourth point into the cluster, in place
        assert _open(X, eng, tags, [rid] * 7)[1] == [0, NONE, 2, 3, 4, 1, NONE]
    finally:
        eng.drop_ring(rid)


# ------------------------------------------------------------------ 6, 7, 8: ids that are not resident, damaged tags, components of small order
def test_unknown_ids_damaged_tags_and_small_order_components(X):
    eng, EC, R = X.eng, X.EC, X.R
    P2, P4 = EC.small_order_points()
    def pt_plus(t, k, S):
        o = EC.PT[k]
        return t[:o] + R._tp(EC.point(t[o:o + 72]).add(S)) + t[o + 72:]
    def flip(t, at):
        return t[:at] + bytes([t[at] ^ 0x40]) + t[at + 1:]
    t0, t1 = X.tags[0], X.tags[1]   # A[0] and B[0]
    batch = [(t0, 77),                              # an id that is not resident
             (b'ZKT2' + t0[4:], 77),                # ... decided before the bad header
             (b'ZKT2' + t0[4:], X.ids[0]),          # magic
             (t0[:4] + (471).to_bytes(4, 'big') + t0[8:], ANY),   # total_len
             (t0[:12] + b'\x00\x00\x00\x01' + t0[16:], X.ids[0]),   # reserved
             (flip(t0, EC.PT[0] + 20), X.ids[0]),   # E1 off the curve
             (flip(t0, EC.PT[1] + 50), ANY),        # E2 off the curve
             (flip(t0, EC.PT[3] + 20), X.ids[0]),   # T2 damaged: the verifier's business
             (pt_plus(t0, 1, P4), X.ids[0]),        # E2 + a point of order 4
             (pt_plus(t1, 1, P2), X.ids[1]),        # E2 + a point of order 2
             (pt_plus(t0, 0, P4.add(P2)), ANY),     # E1 + a point of order 4
             (t1, X.ids[1])]
    got = _open(X, eng, [t for t, _ in batch], [i for _, i in batch])
    assert got == ([NONE] * 7 + [X.ids[0], X.ids[0], X.ids[1], X.ids[0], X.ids[1]], [NONE] * 7 + [0] * 5, [E_ARG, E_ARG] + [E_BAD] * 5 + [0] * 5)


# ------------------------------------------------------------------ 9, 14: the device forms; a wrong secret writes nothing
def _dev_open(x, eng, secret32, tags, ids, fill=0x5a):
    import numpy as np
    import torch
    B = len(tags)
    def up(b):
        return torch.frombuffer(bytearray(bytes(b)), dtype=torch.uint8).to(torch.device('cuda:0'))
    d_a, d_t, d_i = up(secret32), up(b''.join(tags)), up(np.array(ids, dtype=np.uint32).tobytes())   # (the batch at the very end of its allocations)
    outs = [torch.full((4 * B + 16,), fill, dtype=torch.uint8, device='cuda:0') for _ in range(3)]
    torch.cuda.synchronize()
    rc = 0
    try:
        eng.escrow_open_batch_rings_device(B, d_a.data_ptr(), d_t.data_ptr(), d_i.data_ptr(), *[o.data_ptr() for o in outs])
    except x.Z.ZkError as e:
        rc = e.status
    torch.cuda.synchronize()
    return (rc,) + tuple(bytes(o.cpu().numpy()) for o in outs)


def test_device_form_equals_the_host_form_and_a_wrong_secret_writes_nothing(X):
    import numpy as np
    eng = X.eng
    B = 200
    tags = list(X.tags)
    tags[66] = b'ZKT2' + tags[66][4:]
    ids = list(X.want_ids)
    ids[5], ids[9] = 1234, ANY
    rc, ring, idx, st = _dev_open(X, eng, X.a32, tags, ids)
    assert rc == 0
    host = _open(X, eng, tags, ids)
    assert (list(np.frombuffer(ring[:4 * B], dtype=np.uint32)), list(np.frombuffer(idx[:4 * B], dtype=np.uint32)), list(np.frombuffer(st[:4 * B], dtype=np.int32))) == host
    assert host[2][5] == E_ARG and host[2][66] == E_BAD and host[2].count(0) == B - 2
    assert ring[4 * B:] == idx[4 * B:] == st[4 * B:] == b'\x5a' * 16   # what lies behind B is untouched
    wrong = ((X.a + 1) % (1 << 256)).to_bytes(32, 'big')
    rc, ring, idx, st = _dev_open(X, eng, wrong, tags[:70], ids[:70])
    assert rc == E_OPENING and ring == idx == st == b'\x5a' * (4 * 70 + 16)
    assert eng.test_counter(11) == 0   # ... and leaves neither a nor a E1 behind
    with pytest.raises(X.Z.ZkError) as e:
        eng.escrow_open_batch_rings(wrong, tags[:5], ids[:5])
    assert e.value.status == E_OPENING
    with pytest.raises(X.Z.ZkError) as e:   # misaligned device pointers
        eng.escrow_open_batch_rings_device(1, 4098, 4096, 4096, 4096, 4096, 4096)
    assert e.value.status == E_ARG


# ------------------------------------------------------------------ 15, timing: the index is built once, survives zk_ctx_wipe, and is public
def test_timing_families_wipe_and_the_index_is_built_once(X):
    eng, EC = _engine(X.Z, X.par, X.A72), X.EC
    try:
        ids = [eng.add_ring(EC.be32(r), len(r)) for r in X.lists[1:3]]
        info = [eng.ring_info(i) for i in ids]
        eng.set_timing(1)
        want = _expect(X, dict(zip(ids, X.lists[1:3])), X.keys[:64], [ANY] * 64)
        assert _open(X, eng, X.tags[:64], [ANY] * 64) == want
        assert set(eng.last_timing()[1]) == {'escrow_index_build', 'escrow_open', 'escrow_ladder', 'tom_normalize', 'escrow_lookup'}
        assert [eng.ring_info(i) for i in ids] == info   # zk_ring_info as before: generation and flags do not see the index
        assert eng.test_counter(11) > 0
        eng.wipe()
        assert eng.test_counter(11) == 0   # the et buffer (a, a E1, the tags' points) is zero ...
        assert _open(X, eng, X.tags[:64], [ANY] * 64) == want   # ... and the index still answers, without a build
        assert set(eng.last_timing()[1]) == {'escrow_open', 'escrow_ladder', 'tom_normalize', 'escrow_lookup'}
        with pytest.raises(X.Z.ZkError):   # a wrong secret: the key check is all that ran
            eng.escrow_open_batch_rings(bytes(31) + b'\x05', X.tags[:8], [ANY] * 8)
        assert set(eng.last_timing()[1]) == {'escrow_open'} and eng.test_counter(11) == 0
        # 11: a dropped ring's id is ZK_E_ARG per tag; the other ring still answers
        eng.drop_ring(ids[0])
        ring, idx, st = _open(X, eng, X.tags[:8], [ids[0], ids[1]] * 4)
        assert st == [E_ARG, 0] * 4 and ring[0::2] == [NONE] * 4 and idx[0::2] == [NONE] * 4
        assert (ring[1::2], idx[1::2]) == tuple(_expect(X, {ids[1]: X.lists[2]}, X.keys[1:8:2], [ids[1]] * 4)[:2])
    finally:
        eng.close()


# ------------------------------------------------------------------ 10: zk_ctx_update_ring keeps the index in step; 12: zk_ctx_set_params drops it
def test_update_ring_patches_the_index_and_set_params_drops_it(X):
    Z, EC = X.Z, X.EC
    eng, fresh = _engine(Z, X.par, X.A72), _engine(Z, X.par, X.A72)
    try:
        ring = EC.scalars(b'ringU', 257)
        new = EC.scalars(b'newU', 600)
        other = EC.scalars(b'ringV', 5)
        oid = eng.add_ring(EC.be32(other), 5)
        rid = eng.add_ring(EC.be32(ring), 257)
        keys = [ring[i] for i in (0, 10, 100, 199, 200, 255, 256)] + new[:2] + [new[257], new[299], new[300], new[399]] + [other[4], X.outside[0]]
        tags = _tags(X, eng, b'update', keys)
        def check(cur, what):
            fid = fresh.add_ring(EC.be32(cur), len(cur))
            for ids in ([rid] * len(keys), [ANY] * len(keys)):
                got = _open(X, eng, tags, ids)
                assert got == _expect(X, {oid: other, rid: cur}, keys, ids), what
                ref = _open(X, fresh, tags, [fid] * len(keys))
                if ids[0] == rid:
                    assert (got[1], got[2]) == (ref[1], ref[2]), what   # ... equals a context that builds the new list from nothing
            fresh.drop_ring(fid)
            return got
        assert check(ring, 'as built')[1][:7] == [0, 10, 100, 199, 200, 255, 256]
        gen = eng.ring_info(rid)['generation']
        # replace (entry 0 among them: every padding entry follows it): the old keys open to nothing, the new keys to their indices
        cur = list(ring)
        cur[0], cur[10] = new[0], new[1]
        eng.update_ring(rid, {0: EC.be32([new[0]]), 10: EC.be32([new[1]])})
        got = check(cur, 'replace')
        assert got[1][:2] == [NONE, NONE] and got[1][7:9] == [0, 10] and eng.ring_info(rid)['generation'] == gen + 1
        # append within the padded size (512): 257 -> 300 keys
        cur = cur + new[257:300]
        eng.update_ring(rid, {i: EC.be32([new[i]]) for i in range(257, 300)}, nkeys=300)
        got = check(cur, 'append')
        assert got[1][9:11] == [257, 299] and eng.ring_info(rid)['n_keys'] == 300
        # truncate within the padded size: 300 -> 280 keys; what lay behind opens to nothing
        cur = cur[:280]
        eng.update_ring(rid, {}, nkeys=280)
        got = check(cur, 'truncate')
        assert got[1][3:7] == [199, 200, 255, 256] and got[1][9:11] == [257, NONE] and eng.ring_info(rid)['log_n'] == 9
        # a size change: 280 -> 600 keys (1024 entries): a rebuild, which drops the index; the next call builds it again
        cur = cur + new[280:600]
        eng.update_ring(rid, {i: EC.be32([new[i]]) for i in range(280, 600)}, nkeys=600)
        eng.set_timing(1)
        _open(X, eng, tags[:1], [rid])
        assert 'escrow_index_build' in eng.last_timing()[1]
        got = check(cur, 'size change')
        assert got[1][9:13] == [257, 299, 300, 399] and eng.ring_info(rid)['log_n'] == 10 and 'escrow_index_build' not in eng.last_timing()[1]
        # zk_ctx_set_params with other bases: the rings stay, their indexes go with the g they were built for
        par2 = (X.par[0], eng.test_tom_commit([0x1234567], [0])[0], X.par[2])   # another g: a multiple of the old one
        assert par2[1] != X.par[1]
        eng.set_params(*par2, SEC)
        A2 = eng.escrow_keygen(X.a32)
        eng.set_auditor(A2)
        tags2 = _tags(X, eng, b'update', keys)
        assert tags2 != tags
        nid = eng.add_ring(EC.be32(cur), len(cur))   # ... and a ring added again answers as the one that stayed
        want = _expect(X, {rid: cur}, keys, [rid] * len(keys))
        assert _open(X, eng, tags2, [rid] * len(keys)) == want
        assert 'escrow_index_build' in eng.last_timing()[1]
        assert _open(X, eng, tags2, [nid] * len(keys))[1:] == want[1:]
        assert _open(X, eng, tags, [rid] * len(keys))[1] == [NONE] * len(keys)   # tags of the old bases open to nobody
    finally:
        eng.close()
        fresh.close()


# ------------------------------------------------------------------ kernel resources
def test_new_kernels_report_no_scratch_and_no_spills(X):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('kernel_meta', os.path.join(root, 'tools', 'kernel_meta.py'))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    ks = {n: k for n, k in km.kernels(X.Z.LIB_PATH).items() if 'k_escrow_index' in n}
    for want in ('k_escrow_index_insert', 'k_escrow_index_lookup', 'k_escrow_index_gather', 'k_escrow_index_scatter'):
        assert any(want in n for n in ks), want
    for n, k in ks.items():
        assert k['scratch'] == 0 and k['agpr'] == 0 and k['vgpr_spill'] == 0 and k['vgpr'] <= 256 and k['waves_per_simd'] >= 2, (n, k)
