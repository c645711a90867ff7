"""-m gpu: the stratified mutants of tests/zka1_mutants.py DILUTED among honest proofs, through both cross-proof bucket passes of the verifier (k_msm.hip: the
Tom-256 relations of a group of proofs in one sum; k_pmsm.hip: the P-256 relations) and through the range views of the per-proof fallback, against the oracle.

tests/test_gpu_mutants.py puts hundreds of mutants into one call: every group of the Tom-256 pass then holds dozens of bad proofs and falls back, and the P-256 pass
(chunks of 8 192 proofs by default) never sees one.  Here every mutant sits in a group of honest fillers, so its group's fate depends on it alone: a pass that
accepts a group it must not accept (a term not emitted for a malformed point, a proof with a status whose terms still cancel, a live-term rule that drops the only
failing term) accepts the mutant with it, and a range view that reads the wrong proof's verdict -- the bad proof first or last in its group, in the last ragged
group, in the last short chunk -- moves the mutant's verdict onto a filler.  Every proof of every call is compared with the oracle: exact (ok, status).

Layout of one chunk (restated from the code, never asked of the engine): gsz = ceil(cnt / G) proofs per group (k_msm.hip run_msm_t, k_pmsm.hip pmsm_sums),
group g = proofs [g gsz, min(cnt, (g + 1) gsz)) while g gsz < cnt (api_verify.hip VerifyJob::stage2b).  Chunk number c of the sweep keeps the groups with
g % 4 == 1 + c % 2 clean (fillers only); every other group is dirty: one mutant, fillers elsewhere.  The mutant is the group's first, last or middle proof in
turn, except that the first group of a call holds it first (proof 0 of the call) and the last group of a call holds it last -- in a call that ends in a short
chunk that is the last, short group of a ragged chunk.  A call is cut into chunks of set_chunk proofs, the last one short (ctx.h make_chunk_plan); chunk k runs on
lane k % lanes.

The P-256 pass runs on a chunk when jobs.h VerifyJob::p256_batched() holds: ZKATTEST_P256_BATCH=1 (read in zk_ctx_create) lowers its threshold to one proof, but a call
of ONE chunk of at most 8 192 proofs takes the side-stream path instead (side_streams(cnt)), so the single-chunk shapes claim the Tom-256 pass only and the calls of
three chunks claim both -- proved per call by the 'v_msm_p256' timing family and zk_test_counter(3), as tests/test_gpu_verify.py does for its chunks of 12 and 7."""
import hashlib

import pytest

pytestmark = pytest.mark.gpu

from zka1_mutants import DILUTED_RINGS, DILUTED_TAGS, SUBSET_MORE, SUBSET_PER_STRATUM, diluted_signers, mutants, subset

HONEST = 16                    # proofs 0 and 1 are mutated, 2 .. 15 are the fillers
SIDE_MAXP = 8192               # engine.h V_SIDE_MAXP
OUTCOMES = {(1, 0), (0, 0), (0, 3), (0, 4), (0, 8), (0, 10)}
POSITIONS = ('first', 'last', 'middle')

# name: (groups, set_chunk, proofs per call, lanes).  8 groups: chunks of 64 = groups of 8; the short chunk of 60 has seven groups of 8 and one of 4.
# 64 groups: chunks of 256 = groups of 4; the short chunk of 254 has 63 groups of 4 and one of 2.
SHAPES = {
    'g8-one-chunk': (8, 64, 64, 1),
    'g8-three-chunks-1-lane': (8, 64, 188, 1),
    'g8-three-chunks-2-lanes': (8, 64, 188, 2),
    'g64-one-chunk': (64, 256, 256, 1),
    'g64-three-chunks-1-lane': (64, 256, 766, 1),
    'g64-three-chunks-2-lanes': (64, 256, 766, 2),
}
CASES = [(8, 9001, s) for s in SHAPES] + [(1024, 9002, 'g8-one-chunk'), (1024, 9002, 'g64-one-chunk')]
assert {(k, S) for k, S, _ in CASES} == set(DILUTED_RINGS)


def _vseeds(n, tag):
    return b''.join(hashlib.sha256(tag + i.to_bytes(4, 'big')).digest() for i in range(n))


def chunk_groups(cnt, G):
    """[(first, end)] of the groups of a chunk of cnt proofs: the engine's rule, restated"""
    gsz = (cnt + G - 1) // G
    return [(g * gsz, min(cnt, (g + 1) * gsz)) for g in range(G) if g * gsz < cnt]


def call_chunks(B, chunk):
    C = min(chunk, B)
    return [(f, min(B, f + C)) for f in range(0, B, C)]


def p256_pass_runs(B, chunk):
    """jobs.h p256_batched() with both thresholds at 1: every chunk of the call, unless the call is one chunk of at most V_SIDE_MAXP proofs"""
    return not (len(call_chunks(B, chunk)) == 1 and B <= SIDE_MAXP)


def layout(nmut, G, chunk, B):
    """The calls that dilute mutants 0 .. nmut-1: a list of calls, each a list of B slots (k, chunk in call, group, position, group size) for mutant k
    or None for a filler, and per call the list of its groups (first, end, dirty).  A call that runs out of mutants keeps fillers in the remaining groups."""
    order = list(range(2, nmut)) + [0, 1]      # ('honest/p0' and 'honest/p1' go last: no call opens with a 'mutant' that is none)
    calls, j, c = [], 0, 0
    while j < nmut:
        slots, groups = [None] * B, []
        for ci, (f, e) in enumerate(call_chunks(B, chunk)):
            for g, (p0, p1) in enumerate(chunk_groups(e - f, G)):
                dirty = g % 4 != 1 + c % 2 and j < nmut
                groups.append((f + p0, f + p1, dirty))
                if dirty:
                    pos = 'first' if f + p0 == 0 else 'last' if f + p1 == B else POSITIONS[j % 3]
                    at = {'first': p0, 'last': p1 - 1, 'middle': p0 + (p1 - p0) // 2}[pos]
                    slots[f + at] = (order[j], ci, g, pos, p1 - p0)
                    j += 1
            c += 1
        calls.append((slots, groups))
    return calls


@pytest.mark.parametrize('shape', sorted(SHAPES))
def test_layout_covers_the_edges_of_the_range_views(shape):
    """The layout alone (no GPU work): three groups of four dirty with exactly one mutant each, every mutant placed once, and over the sweep a mutant that is
    proof 0 of a call, one that is the last proof of a call, one in the last, short group of a ragged chunk, and all three positions inside a group."""
    G, chunk, B, lanes = SHAPES[shape]
    nmut = 147
    calls = layout(nmut, G, chunk, B)
    placed = [s[0] for slots, _ in calls for s in slots if s]
    assert sorted(placed) == list(range(nmut))
    first = last = ragged = False
    seen_pos = set()
    for n, (slots, groups) in enumerate(calls):
        assert [g[0] for g in groups] == [0] + [g[1] for g in groups[:-1]] and groups[-1][1] == B == len(slots)      # the groups tile the call
        for f, e in call_chunks(B, chunk):
            mine = [g for g in groups if f <= g[0] < e]
            assert len(mine) == G and mine[-1][1] == e and min(b - a for a, b, _ in mine[:-1]) >= (8 if G == 8 else 4)
            if n + 1 < len(calls):                                   # (the sweep's last call runs out of mutants)
                assert sum(d for _, _, d in mine) == 3 * G // 4
        for a, b, d in groups:
            assert sum(1 for s in slots[a:b] if s) == (1 if d else 0)
        first |= slots[0] is not None
        last |= slots[-1] is not None
        a, b, d = groups[-1]
        gsz = groups[-2][1] - groups[-2][0]
        ragged |= b - a < gsz and any(slots[a:b])
        seen_pos |= {s[3] for s in slots if s}
    assert first and last and seen_pos == set(POSITIONS)
    assert ragged == (len(call_chunks(B, chunk)) > 1)     # the short chunks are the ragged ones
    assert p256_pass_runs(B, chunk) == (len(call_chunks(B, chunk)) > 1)


@pytest.fixture(scope='module')
def worlds():
    cache = {}
    yield cache
    for w in cache.values():
        w['eng'].close()


def _world(worlds, monkeypatch, nkeys, S):
    """Engine, oracle, 16 honest proofs, the subset and the oracle's verdicts on it under both tags: made once per ring, shared by the shapes, never changed."""
    if nkeys in worlds:
        return worlds[nkeys]
    import coracle as CO
    import zkp_ecdsa_amd as Z
    monkeypatch.setenv('ZKATTEST_P256_BATCH', '1')      # read in zk_ctx_create
    eng = Z.Engine(0)
    monkeypatch.delenv('ZKATTEST_P256_BATCH')
    eng.set_timing(1)
    eng.set_batch_verify(1)
    nh, tg, th = eng.synth_params(S)
    eng.set_params(nh, tg, th, 80)
    W = diluted_signers(nkeys)
    ring, msg, sig, pk, which, seeds = eng.synth_workload(S, nkeys, W)
    eng.set_ring(ring, nkeys)
    octx = CO.OracleCtx(nh, tg, th, 80)
    octx.set_ring(ring, nkeys)
    # honest proof i: signer i % W; the first W under the workload's prover seeds (proofs 0 and 1 are the CPU tier's), the others under seeds of their own
    rep = HONEST // W
    seeds += b''.join(hashlib.sha256(b'second prover seed' + seeds[32 * i:32 * i + 32]).digest() for i in range(HONEST - W))
    proofs, st = eng.prove_batch(msg * rep, sig * rep, pk * rep, which * rep, seeds=seeds)
    assert st == [0] * HONEST and len(set(proofs)) == HONEST
    hmsg = [msg[32 * (i % W):32 * (i % W) + 32] for i in range(HONEST)]
    assert octx.verify_batch(b''.join(hmsg), proofs, nthreads=16, vseeds=_vseeds(HONEST, b'h')) == ([1] * HONEST, [0] * HONEST)
    sub = subset(mutants(proofs[:2], (nkeys - 1).bit_length(), S, S), SUBSET_PER_STRATUM, SUBSET_MORE)
    assert all(len(m[2]) % 4 == 0 for m in sub)          # ZKA1 proofs are packed 4-byte aligned: a length-changing mutant may sit anywhere, as in test_gpu_mutants.py
    mmsg = [hmsg[m[1]] for m in sub]
    want = {}
    for tag in DILUTED_TAGS:
        ok, vst = octx.verify_batch(b''.join(mmsg), [m[2] for m in sub], nthreads=16, vseeds=_vseeds(len(sub), tag))
        want[tag] = list(zip(ok, vst))
        assert set(want[tag]) == OUTCOMES, (tag, sorted(set(want[tag])))     # the CPU tier's condition, on the engine's bytes
    worlds[nkeys] = dict(eng=eng, octx=octx, proofs=proofs, hmsg=hmsg, sub=sub, mmsg=mmsg, want=want)
    return worlds[nkeys]


def _fill(w, slots, tag, clean=False):
    """(messages, proofs, verifier seeds, expected (ok, status)) of one call: slot i holds its mutant under the mutant's own seed of this tag, or filler
    2 + i % 14 under a seed of the slot; clean: fillers stand in for the mutants"""
    msgs, plist, vs, exp = [], [], [], []
    mseeds = _vseeds(len(w['sub']), tag)
    for i, s in enumerate(slots):
        if s and not clean:
            k = s[0]
            msgs.append(w['mmsg'][k]), plist.append(w['sub'][k][2]), vs.append(mseeds[32 * k:32 * k + 32]), exp.append(w['want'][tag][k])
        else:
            f = 2 + i % (HONEST - 2)
            msgs.append(w['hmsg'][f]), plist.append(w['proofs'][f]), vs.append(hashlib.sha256(tag + b'filler' + i.to_bytes(4, 'big')).digest()), exp.append((1, 0))
    return b''.join(msgs), plist, b''.join(vs), exp


def _run(eng, call):
    """one verify_batch: (verdicts, rise of counter 0, rise of counter 3, timing families)"""
    msgs, plist, vs, _ = call
    c0, c3 = eng.test_counter(0), eng.test_counter(3)
    ok, st = eng.verify_batch(msgs, plist, vseeds=vs)
    return list(zip(ok, st)), eng.test_counter(0) - c0, eng.test_counter(3) - c3, eng.last_timing()[1]


def test_an_identity_at_a_sampled_repetition_keeps_its_status_in_a_call_of_a_few_proofs(worlds, monkeypatch):
    """Regression, found by the diluted sweep (its smallest form is a call of ONE proof, no pass involved): calls of at most 204 proofs compute T = alpha R and
    T1 = z R + Q on cooperating waves (k_coop.hip k_v_exp_points_co), whose test for the identity took Z for one product (0 or q) where the addition law leaves
    the sum of two (0 .. 3 q): alpha = 0 gave Z = 2 q, 'T is at infinity' (status 3) was missed and the proof came back as (0, 0).  Every mutant of the subset
    that the oracle answers with status 3 or 4, alone in a call and as proof 3 of 8, under both tags."""
    nkeys, S = DILUTED_RINGS[0]
    w = _world(worlds, monkeypatch, nkeys, S)
    eng = w['eng']
    eng.set_verify_groups(8), eng.set_chunk(64), eng.set_lanes(1), eng.set_batch_verify(256)
    ran = set()
    for tag in DILUTED_TAGS:
        mseeds = _vseeds(len(w['sub']), tag)
        for k, exp in enumerate(w['want'][tag]):
            if exp[1] not in (3, 4):
                continue
            one = (w['mmsg'][k], [w['sub'][k][2]], mseeds[32 * k:32 * k + 32])
            assert eng.verify_batch(one[0], one[1], vseeds=one[2]) == ([exp[0]], [exp[1]]), (w['sub'][k][0], tag)
            slots = [None] * 3 + [(k,)] + [None] * 4
            msgs, plist, vs, want = _fill(w, slots, tag)
            ok, st = eng.verify_batch(msgs, plist, vseeds=vs)
            assert list(zip(ok, st)) == want, (w['sub'][k][0], tag, list(zip(ok, st)))
            ran.add(exp)
    assert ran == {(0, 3), (0, 4)}
    eng.set_batch_verify(1)


@pytest.mark.parametrize('nkeys,S,shape', CASES)
def test_diluted_mutants_through_both_passes_equal_the_oracle(worlds, monkeypatch, nkeys, S, shape):
    G, chunk, B, lanes = SHAPES[shape]
    w = _world(worlds, monkeypatch, nkeys, S)
    eng, sub = w['eng'], w['sub']
    eng.set_verify_groups(G), eng.set_chunk(chunk), eng.set_lanes(lanes), eng.set_batch_verify(1)
    pm = p256_pass_runs(B, chunk)
    calls = layout(len(sub), G, chunk, B)

    def check(call, slots, groups, tag, what):
        got, d0, d3, fam = _run(eng, call)
        exp = call[3]
        where = {i: s for i, s in enumerate(slots) if s}
        bad = [(i, sub[where[i][0]][0] + ': chunk %d group %d %s of %d' % where[i][1:] if i in where and what != 'clean' else 'filler', got[i], exp[i])
               for i in range(B) if got[i] != exp[i]]
        assert not bad, (shape, nkeys, tag, what, len(bad), bad[:12])                  # 1 and 2: every slot, mutant or filler, as the oracle says
        ndirty = sum(d for _, _, d in groups) if what != 'clean' else 0
        dirty = sum(b - a for a, b, d in groups if d) if what != 'clean' else 0
        # (-s shows these figures)
        print('%s ring %d %s %s: %d proofs, %d dirty + %d clean groups, %d proofs in dirty groups; counter 0 +%d, counter 3 +%d'
              % (shape, nkeys, tag.decode(), what, B, ndirty, len(groups) - ndirty, dirty, d0, d3))
        assert d0 <= dirty, (shape, tag, what, d0, dirty)                              # 3: no silent fallback of a clean group
        assert 'v_msm_tom' in fam and ('v_msm_p256' in fam) == pm, (shape, tag, what, sorted(fam))
        if pm:
            assert d3 >= B - dirty, (shape, tag, what, d3, B - dirty)                  # 4: the P-256 pass settled the clean groups
            assert d3 > 0
        return got

    seen = set()
    edge = {'first of a call': 0, 'last of a call': 0, 'last short group': 0}
    for tag in DILUTED_TAGS:
        for n, (slots, groups) in enumerate(calls):
            call = _fill(w, slots, tag)
            got = check(call, slots, groups, tag, 'call %d' % n)
            seen |= set(got)
            # a BAD proof at each edge (the oracle's verdict): an honest 'mutant' there would show nothing
            edge['first of a call'] += slots[0] is not None and call[3][0] != (1, 0)
            edge['last of a call'] += slots[-1] is not None and call[3][-1] != (1, 0)
            a, b, d = groups[-1]
            edge['last short group'] += b - a < groups[-2][1] - groups[-2][0] and any(s and call[3][a + j] != (1, 0) for j, s in enumerate(slots[a:b]))
            if n == 0 and tag == DILUTED_TAGS[0]:
                # 5: the same call without the passes (every proof through the per-proof sums): identical verdicts
                eng.set_batch_verify(0)
                again, d0, d3, fam = _run(eng, call)
                eng.set_batch_verify(1)
                assert again == got and 'v_msm_tom' not in fam and 'v_msm_p256' not in fam and d3 == 0, (shape, sorted(fam), d3)
                # 3, all clean: the fillers stand in for the mutants; nothing is re-checked, the passes settle every proof
                clean = _fill(w, slots, tag, clean=True)
                got_clean = check(clean, slots, groups, tag, 'clean')
                assert got_clean == [(1, 0)] * B
    assert seen == OUTCOMES, (shape, sorted(seen))
    multi = len(call_chunks(B, chunk)) > 1
    assert edge['first of a call'] and edge['last of a call'] and bool(edge['last short group']) == multi, edge
