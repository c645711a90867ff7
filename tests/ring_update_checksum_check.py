"""Run by tests/test_gpu_ring_update_tables.py in its own process with ZKATTEST_LIB = lib/libzkattest_hip_testhooks.so (the only build with
zk_test_ring_checksum; one process holds one build).  Every scenario of tests/ring_update_cases.py on the rings of 1000 and 5000 keys: a ring built from L and
updated in place has, table by table, the checksum of the ring zk_ctx_set_ring builds from L' -- limbs, table E, both digit tables, the per-key tables and
their flags, the leaves and the digest -- also with the key tables switched off, where the tables a ring does not have read 0 on both sides."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TABLES = ('limbs', 'table E', 'gk_kdig', 'gk_edig', 'ktab', 'ktab_ok', 'leaves', 'digest')


def checksum(Z, eng, rid):
    L = Z.lib()
    L.zk_test_ring_checksum.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
    sums = (C.c_uint64 * 8)()
    rc = L.zk_test_ring_checksum(eng.h, rid, sums)
    assert rc == 0, rc
    return list(sums)


def main():
    import ring_update_cases as RU
    import zkp_ecdsa_amd as Z
    assert hasattr(Z.lib(), 'zk_test_ring_checksum'), 'not the test-hooks build'
    S = 6161
    for key_tables in (True, False):
        X, Y = Z.Engine(0), Z.Engine(0)
        params = X.synth_params(S)
        for e in (X, Y):
            e.set_params(*params, 80)
            e.set_key_tables(key_tables)
        for n in (1000, 5000):
            W = RU.split(X.synth_workload(S + n, n, 4)[0])
            fresh = {}
            for name, L, changes, new_n, Lp, fast in RU.scenarios(W):
                rid = X.add_ring(b''.join(L), len(L))
                had = checksum(Z, X, rid)
                X.update_ring(rid, changes, new_n)
                got = checksum(Z, X, rid)
                if len(Lp) not in fresh:
                    Y.set_ring(b''.join(Lp), len(Lp))
                    fresh[len(Lp)] = checksum(Z, Y, 0)
                want = fresh[len(Lp)]
                print('%-16s n=%d key tables %s: %s' % (name, n, 'on' if key_tables else 'off', ' '.join('%016x' % s for s in got)), flush=True)
                bad = [TABLES[i] for i in range(8) if got[i] != want[i]]
                assert not bad, (name, n, key_tables, bad)
                assert got != had, (name, n)   # (the update wrote something: L differs from L')
                present = [s != 0 for s in want]
                assert present[0] and present[1] and present[6] and present[7], want   # limbs, table E, leaves, digest: both sizes have them
                assert present[2] == present[3] == (len(Lp) > 2048), want             # digit planes from 2^12 keys
                assert present[4] == present[5] == key_tables, want
                X.drop_ring(rid)
        X.close(), Y.close()


if __name__ == '__main__':
    main()
    print('ring_update_checksum_check ok')
