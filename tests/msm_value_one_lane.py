"""Child process of tests/test_gpu_msm_value.py: the Tom-256 bucket pass by value with every dependent chain in one lane (ZKATTEST_ONE_LANE_CHAINS is read
once per process, so the parent cannot switch it).  Prints one JSON line: the cases that matched the reference."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import msm_value_common as MV   # noqa: E402


def main():
    import zkp_ecdsa_amd as Z
    eng = Z.Engine(0)
    raw = eng.synth_params(MV.PARAM_SEED)
    eng.set_params(*raw, 80)
    orc = MV.Oracle(*raw)
    ok = []
    for name in ('random_ragged', 'digit_extremes', 'collisions', 'flags'):
        for groups in (8, 64):
            MV.run_tom(eng, orc, MV.case('tom', name, groups))
            ok.append([name, groups])
    eng.close()
    print(json.dumps({'one_lane': os.environ.get('ZKATTEST_ONE_LANE_CHAINS') is not None, 'ok': ok}))


if __name__ == '__main__':
    main()
