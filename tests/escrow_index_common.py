"""Shared by the tests of the resident point index (test_escrow_index_host.py, test_gpu_escrow_rings.py): the Python restatement of the layout and the slot
function that zkp-ecdsa_amd/csrc/escrow_index.h defines and include/zkattest.h states.

    entries = the least power of two >= nkeys;  slots = 2 * entries;  empty = 0xffffffff;  linear probing with wrap-around
    w0, w1 = bits 0..31 and 32..63 of the point's canonical affine x
    h = w0 * 0x9e3779b1 + w1 * 0x85ebca6b;  h ^= h >> 16;  h *= 0xc2b2ae35;  h ^= h >> 13   (mod 2^32);   home slot = h & (slots - 1)
"""
EMPTY = 0xffffffff
M32 = 0xffffffff


def entries(nkeys):
    c = 1
    while c < nkeys:
        c <<= 1
    return c


def slots(nkeys):
    return 2 * entries(nkeys)


def hash32(w0, w1):
    h = (w0 * 0x9e3779b1 + w1 * 0x85ebca6b) & M32
    h ^= h >> 16
    h = (h * 0xc2b2ae35) & M32
    h ^= h >> 13
    return h


def home(x, nslots):
    """home slot of a point with canonical affine x (an integer) in a table of nslots slots"""
    return hash32(x & M32, (x >> 32) & M32) & (nslots - 1)


def home_of_point(b72, nslots):
    """... of a point given as 72 bytes (two 36-byte big-endian coordinates)"""
    return home(int.from_bytes(b72[:36], 'big'), nslots)


def limbs30(v):
    return [(v >> (30 * i)) & 0x3fffffff for i in range(9)]
