"""Helper of tests/test_gpu_screen_small.py: the contexts and the hand-made witnesses of the small-call screen tests -- the path mix and the chosen scalars --
built in one place; run as a script (in a child process: ZKATTEST_LIB and ZKATTEST_ONE_LANE_CHAINS are read when the library loads) it screens them on both
contexts and prints every answer and what the calls added to zk_test_counter 4."""
import json
import os
import sys

os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle')):
    if p not in sys.path:
        sys.path.insert(0, p)

import zkattest_ref as R
from test_gpu_screen import N_ORD, S, be, curve_y, ints, named_mutants, ring_bytes, screen, wits_of

G, sc = R.p256.generator(), R.p256.newScalar
# (tests/test_screen_co_host.py runs the same scalars through the host build of the walk and the range sums)
U2 = [1, 8, N_ORD - 1, N_ORD - 8, int('88' * 32, 16), int('77' * 32, 16), 2 ** 255 + 1]
U1 = [0, 1, N_ORD - 1, (0x5eed1234abcdef << 24) % N_ORD]   # the last: a zero low digit of the 20-bit comb
ID_IN, ID_OFF = 5, 11                                       # the identity witnesses' keys: 5 G sits in ring M, 11 G in no ring


def xy(pt):
    x, y = pt.toAffine()
    return be(x) + be(y)


def contexts():
    """Two contexts at secLevel 20, per-key tables on ('kt') and off ('nokt').  Resident in both: ring A (the 8 keys of workload A), ring M (A with the wrap
    witness's key at index 3 and 5 G at index 6) and ring B (the 16 keys of workload B, none of them in A)."""
    import zkp_ecdsa_amd as Z
    engs = {}
    for name, kt in (('kt', 1), ('nokt', 0)):
        e = Z.Engine(0)
        e.set_key_tables(kt)
        e.set_params(*e.synth_params(S), 20)
        engs[name] = e
    e = engs['kt']
    WA, WB = e.synth_workload(S, 8, 8), e.synth_workload(S + 1, 16, 16)
    rings = {'A': ints(WA[0]), 'B': ints(WB[0])}
    # the wrap case of tests/test_gpu_screen.py: P0 with x = n + 3, r = 3, pk = r^-1 (s P0 - z G)
    P0 = R.WeierstrassPoint(R.p256, N_ORD + 3, curve_y(N_ORD + 3))
    msgw, sw = WA[1][:32], 0x1234567890abcdef1234567890abcdef
    z = R.truncateToN(int.from_bytes(msgw, 'big'), N_ORD)
    pkw = xy(P0.mul(sc(sw)).add(G.mul(sc((N_ORD - z) % N_ORD))).mul(sc(pow(3, -1, N_ORD))))
    M = list(rings['A'])
    M[3], M[6] = int.from_bytes(pkw[:32], 'big'), G.mul(sc(ID_IN)).toAffine()[0]
    rings['M'] = M
    ids = {name: {k: e.add_ring(ring_bytes(rings[k])) for k in ('A', 'M', 'B')} for name, e in engs.items()}
    return {'engs': engs, 'ids': ids, 'rings': rings, 'wa': wits_of(WA), 'wb': wits_of(WB), 'wrap': (msgw, be(3) + be(sw), pkw)}


def identity_witness(msg, d):
    """pk = d G, r = -z / d, any s: u1 G + u2 pk = (z / s) G - (z / (d s)) d G = O"""
    z = int.from_bytes(msg, 'big') % N_ORD
    r = -z * pow(d, -1, N_ORD) % N_ORD
    assert r
    return (msg, be(r) + be(0x600dcafe << 64), xy(G.mul(sc(d))))


def path_mix(ctx):
    """name -> witness, for ring M: every path of the screen's ECDSA part and both skips"""
    wa, wb = ctx['wa'], ctx['wb']
    muts = named_mutants(wa[2], wa[5])
    return {'member': wa[2], '-pk': muts['-pk'], 'not in ring': wb[1], 'off curve': muts['off curve'], 'r = 0': muts['r = 0'], 'wrap': ctx['wrap'],
            'identity, key in ring': identity_witness(wa[0][0], ID_IN), 'identity, key not in ring': identity_witness(wa[1][0], ID_OFF), 'member 2': wa[5]}


MIX5 = ['member', 'identity, key in ring', 'not in ring', 'off curve', 'identity, key not in ring']


def chosen_scalars(ctx):
    """[(u1, u2, key in ring M, witness)]: a valid signature with prescribed u1 = z / s, u2 = r / s under ring M's key 4 and under a key of no ring"""
    out = []
    for inring, pk in ((True, ctx['wa'][4][2]), (False, ctx['wb'][2][2])):
        PK = R.p256.deserializePoint(b'\x04' + pk)
        for u2 in U2:
            for u1 in U1:
                c = G.mul(sc(u1)).add(PK.mul(sc(u2))).toAffine()
                r = c[0] % N_ORD if c else 0
                if not r:
                    continue   # R is the identity, or r = 0: no such signature
                s = r * pow(u2, -1, N_ORD) % N_ORD
                out.append((u1, u2, inring, (be(u1 * s % N_ORD), be(r) + be(s), pk)))
    return out


def main():
    import zkp_ecdsa_amd as Z
    ctx = contexts()
    mix, chosen = path_mix(ctx), [c[3] for c in chosen_scalars(ctx)]
    answers = []
    c0 = ctx['engs']['kt'].test_counter(4)
    for name, e in ctx['engs'].items():
        e.use_ring(ctx['ids'][name]['M'])
        answers.append(screen(e, list(mix.values())))
        answers.append(screen(e, [mix[k] for k in MIX5]))
        answers.append(screen(e, chosen))
    coop = ctx['engs']['kt'].test_counter(4) - c0
    for e in ctx['engs'].values():
        e.close()
    print(json.dumps({'lib': Z.LIB_PATH, 'answers': answers, 'coop': coop, 'witnesses': 2 * (len(mix) + len(MIX5) + len(chosen))}))


if __name__ == '__main__':
    main()
