"""Shared by the accountable-attestation tests (test_accountable_host.py, test_gpu_accountable.py): the Python statement of a "ZKC1" bundle's layout --
header, sizes, the slot walk, split and join -- and the hand-made vectors the walk is tested on.  It states layout only: the attestation's bytes are
zk_prove_batch's and the tag's zk_escrow_prove_batch's (tests/escrow_common.py).

    header 16 B : "ZKC1" | total_len u32 big-endian | 0 u32 | 0 u32
    attestation : one ZKA1 / ZK1P proof (its own total_len at bytes 4..8, n at bytes 12..16)
    tag 472 B   : one ZKT1 tag ("ZKT1" | 472 | 0 | 0 | ...)
"""
import struct

HDR, TAG, INNER_HDR = 16, 472, 32
E_BAD = 10
NONE = 0xFFFFFFFF
MAGIC = {0: b'ZKA1', 1: b'ZK1P'}
# wire.h: header, R, comS1, keyXcom, keyYcom (`fixed`) and the GKProof's bytes per index bit (`gk_n`), per wire layout (0: ZKA1, 1: ZK1P)
FIXED = {0: 304, 1: 292}
GK_N = {0: 384, 1: 360}


def header(total):
    return b'ZKC1' + struct.pack('>III', total, 0, 0)


def size(att_bytes):
    return HDR + att_bytes + TAG


def max_size(proof_max):
    return HDR + proof_max + TAG if proof_max else 0


def tag_header():
    return b'ZKT1' + struct.pack('>III', TAG, 0, 0)


def inner_ok(blob, o0, o1, packed):
    """rr_head's rules (rering_plan.h) for the proof in slot [o0, o1): reads 16 bytes of it"""
    if o1 < o0 or o0 & 3 or (o1 - o0) & 3 or o1 - o0 < INNER_HDR or o1 - o0 > 0xffffffff:
        return False
    magic, total, _, n = blob[o0:o0 + 4], *struct.unpack('>III', blob[o0 + 4:o0 + 16])
    return magic == MAGIC[packed] and total == o1 - o0 and n <= 63 and total >= FIXED[packed] + GK_N[packed] * n + 32


def walk(blob, o0, o1, packed):
    """-> (attestation start, tag start) or None where the slot is ZK_E_BAD_ENCODING; no byte outside [o0, o1) is read"""
    if o1 < o0 or o0 & 3 or (o1 - o0) & 3 or o1 - o0 < HDR + INNER_HDR + TAG or o1 - o0 > 0xffffffff:
        return None
    if blob[o0:o0 + 4] != b'ZKC1' or struct.unpack('>III', blob[o0 + 4:o0 + 16]) != (o1 - o0, 0, 0):
        return None
    if not inner_ok(blob, o0 + HDR, o1 - TAG, packed):
        return None
    return o0 + HDR, o1 - TAG


def split(bundles, packed):
    """-> (attestations, tags, statuses): a refused bundle gives b'', 472 zero bytes and 10"""
    att, tags, st = [], [], []
    for b in bundles:
        w = walk(b, 0, len(b), packed)
        att.append(b[w[0]:w[1]] if w else b''), tags.append(b[w[1]:] if w else bytes(TAG)), st.append(0 if w else E_BAD)
    return att, tags, st


def join(proofs, tags, packed):
    """-> (bundles, statuses): None and 10 where the proof's header or the tag's 16 header bytes are refused"""
    out, st = [], []
    for p, t in zip(proofs, tags):
        ok = inner_ok(p, 0, len(p), packed) and len(t) == TAG and t[:16] == tag_header() and size(len(p)) <= 0xffffffff
        out.append(header(size(len(p))) + p + t if ok else None), st.append(0 if ok else E_BAD)
    return out, st


def fake_proof(length, packed, n=3, magic=None):
    """headers only: the walk reads nothing else"""
    return (magic or MAGIC[packed]) + struct.pack('>III', length, 20, n) + bytes(length - 16)


def fake_tag(fill=0x77):
    return tag_header() + bytes([fill]) * (TAG - 16)


def bundle(att, tag):
    return header(size(len(att))) + att + tag


def put32(b, at, v):
    return b[:at] + struct.pack('>I', v) + b[at + 4:]


def bad_vectors(good, att_len):
    """(name, bytes) of every way the walk refuses a bundle made from the good one `good`, whose attestation takes att_len bytes: every header error, a
    truncated slot, an inner total_len one word too long or too short, a slot that ends inside the tag.  Every vector is as long as the slot it is given."""
    inner = HDR + 4
    return [('magic', b'ZKC2' + good[4:]),
            ('the quorum magic', b'ZKQ1' + good[4:]),
            ('total_len + 4', put32(good, 4, len(good) + 4)),
            ('total_len - 4', put32(good, 4, len(good) - 4)),
            ('reserved word 1', put32(good, 8, 1)),
            ('reserved word 2', put32(good, 12, 1 << 24)),
            ('truncated slot, header not adjusted', good[:-4]),
            ('truncated slot, header adjusted', put32(good[:-4], 4, len(good) - 4)),
            ('inner total_len one word too long', put32(good, inner, att_len + 4)),
            ('inner total_len one word too short', put32(good, inner, att_len - 4)),
            ('slot ends inside the tag', put32(good[:-100], 4, len(good) - 100)),
            ('slot of the header alone', header(16)),
            ('no attestation', header(16 + TAG) + good[-TAG:]),
            ('the other layout\'s inner magic', good[:HDR] + (b'ZK1P' if good[HDR:HDR + 4] == b'ZKA1' else b'ZKA1') + good[HDR + 4:]),
            ('length no multiple of 4', put32(good[:-2], 4, len(good) - 2))]


def self_check(packed=0):
    """the statement against itself on hand-made bundles: sizes, the walk's verdicts, both round trips"""
    n = 3
    m = FIXED[packed] + GK_N[packed] * n + 32
    atts = [fake_proof(m + 4 * i, packed, n) for i in range(3)]
    tags = [fake_tag(0x70 + i) for i in range(3)]
    good = [bundle(a, t) for a, t in zip(atts, tags)]
    assert [len(g) for g in good] == [size(len(a)) for a in atts] and max_size(1000) == 1488 and max_size(0) == 0
    blob = b''.join(good)
    o = len(good[0])
    assert walk(blob, o, o + len(good[1]), packed) == (o + 16, o + len(good[1]) - TAG)
    assert walk(blob, o + 2, o + 2 + len(good[1]), packed) is None and walk(blob, o, 0, packed) is None
    assert split(good, packed) == (atts, tags, [0] * 3)
    assert join(atts, tags, packed) == (good, [0] * 3)
    for name, v in bad_vectors(good[1], len(atts[1])):
        assert walk(v, 0, len(v), packed) is None, name
    assert walk(good[1], 0, len(good[1]), 1 - packed) is None
    bad_tag = b'ZKT2' + tags[0][4:]
    assert join([atts[0], atts[1][:-4], atts[2]], [bad_tag, tags[1], tags[2]], packed) == ([None, None, good[2]], [E_BAD, E_BAD, 0])
    assert split([good[0], good[1][:-4]], packed) == ([atts[0], b''], [tags[0], bytes(TAG)], [0, E_BAD])
    return True


if __name__ == '__main__':
    assert self_check(0) and self_check(1)
    print('accountable_common: ok')
