"""Helper of tests/test_gpu_recover.py::test_cooperative_and_one_lane_paths_give_the_same_bytes: run in a child process (ZKATTEST_ONE_LANE_CHAINS is read when
the library loads); recovers the 65 valid witnesses and the two edge lists of that file, checks them against the model, and prints every answer, what the
calls added to zk_test_counter 4, and the verdict on one call of 4 096 + 3 valid witnesses against the workload's keys."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import recover_common as RC
from test_gpu_recover import S, contexts, edge_list_large, edge_list_small, keys_of, recover, wits_of


def main():
    import zkp_ecdsa_amd as Z
    ctx = contexts()
    eng, ids = ctx['engs']['nokt'], ctx['ids']['nokt']
    calls = [('C', wits_of(ctx['W']['C'], 65)), ('E', edge_list_large(ctx)), ('W', edge_list_small(ctx))]
    answers = []
    c0 = eng.test_counter(4)
    for ring, wits in calls:
        eng.use_ring(ids[ring])
        res = recover(eng, wits)
        assert res == RC.expect(wits, ctx['rings'][ring]), ring
        answers.append([[p.hex() if p is not None else None for p in res[0]], res[1], res[2]])
    coop = eng.test_counter(4) - c0
    Wb = eng.synth_workload(S + 9, 5000, 4099)
    rid = eng.add_ring(Wb[0])
    c1 = eng.test_counter(4)
    big = recover(eng, wits_of(Wb), ring_ids=[rid] * 4099) == (keys_of(Wb), Wb[4], [0] * 4099)
    big_coop = eng.test_counter(4) - c1
    for e in ctx['engs'].values():
        e.close()
    print(json.dumps({'lib': Z.LIB_PATH, 'answers': answers, 'coop': coop, 'witnesses': sum(len(w) for _, w in calls), 'big': 'ok' if big else 'differs', 'big_coop': big_coop}))


if __name__ == '__main__':
    main()
