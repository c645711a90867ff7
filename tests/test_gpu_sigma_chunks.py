"""-m gpu: the chunk RNG binding the four sigma provers share (zkp-ecdsa_amd/csrc/sigma.h: sigma_chunk_rng).  A chunk that starts at proof `first` of a call
reads the caller's stream from proof `first` on; in seed mode it reads its own fills from 0 on.  Five proofs in chunks of two on two lanes -- three chunks, a
short last one, lane 0 used twice -- must give what one chunk on one lane gives, byte for byte and status for status, in both RNG modes.  The bytes
themselves are pinned against the statements by each type's own file."""
import hashlib

import pytest

pytestmark = pytest.mark.gpu

SEC = 20
B = 5
# stream mode: the type's draws per proof plus the margin its own stream test gives them
# (test_gpu_link: 3 + 1; test_gpu_distinct: 8 + 1; test_gpu_escrow: 4 + 1; test_gpu_escrow_threshold: 1 + 0)
BLOCKS = {'link': 4, 'distinct': 9, 'escrow': 5, 'share': 1}


class Ctx:
    pass


@pytest.fixture(scope='module')
def X():
    import escrow_common as EC
    import zkp_ecdsa_amd as Z
    x = Ctx()
    x.EC = EC
    eng = x.eng = Z.Engine(0)
    eng.set_comb_bits(16)
    eng.set_params(*eng.synth_params(EC.PARAM_SEED), SEC)
    x.x, x.x2, x.r1, x.r2 = (EC.scalars(n, B) for n in (b'sgx', b'sgx2', b'sgr1', b'sgr2'))
    x.c1, x.c2, x.d2 = eng.test_tom_commit(x.x, x.r1), eng.test_tom_commit(x.x, x.r2), eng.test_tom_commit(x.x2, x.r2)
    a32 = EC.tag(b'sg-auditor', 0)
    eng.set_auditor(eng.escrow_keygen(a32))
    x.tags, st = eng.escrow_prove_batch(EC.be32(x.x), x.c1, EC.be32(x.r1), seeds=EC.seeds_for(b'sg-tags', B))
    assert st == [0] * B
    x.shares, keys = eng.auditors_split_key(a32, 2, 3, seed=EC.tag(b'sg-split', 0))
    eng.set_auditors(2, keys)
    yield x
    eng.close()


def _prove(x, kind, **rng):
    eng, be = x.eng, x.EC.be32
    if kind == 'link':
        return eng.link_prove_batch(be(x.x), x.c1, be(x.r1), x.c2, be(x.r2), **rng)
    if kind == 'distinct':
        return eng.distinct_prove_batch(be(x.x), x.c1, be(x.r1), be(x.x2), x.d2, be(x.r2), **rng)
    if kind == 'escrow':
        return eng.escrow_prove_batch(be(x.x), x.c1, be(x.r1), **rng)
    return eng.auditors_share_batch(1, x.shares[0], x.tags, **rng)


@pytest.mark.parametrize('mode', ['stream', 'seed'])
@pytest.mark.parametrize('kind', ['link', 'distinct', 'escrow', 'share'])
def test_chunks_on_two_lanes_read_the_rng_of_their_own_proofs(X, kind, mode):
    eng, n = X.eng, BLOCKS[kind]
    if mode == 'stream':   # every proof's blocks are its own: a chunk bound to another proof's row gives other bytes
        rows = b''.join(hashlib.sha256(b'sigma-stream' + kind.encode() + bytes([b, k])).digest() for b in range(B) for k in range(n))
        rng = dict(streams=rows, stream_blocks=n)
    else:
        rng = dict(seeds=X.EC.seeds_for(b'sg-' + kind.encode(), B))
    try:
        eng.set_chunk(4096), eng.set_lanes(1)
        want = _prove(X, kind, **rng)
        eng.set_chunk(2), eng.set_lanes(2)
        got = _prove(X, kind, **rng)
    finally:
        eng.set_chunk(4096), eng.set_lanes(2)
    assert want[1] == [0] * B and len(set(want[0])) == B
    assert got == want
