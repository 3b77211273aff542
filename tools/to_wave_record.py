"""Record what the numpy iLQR helper (tests/ilqr_ref.py) does on the stride-straddling inputs of
tests/test_gpu_to_wave.py (tests/to_wave_cases.py: single and double integrator, seed 5, Te = 1, 2,
63, 64, 65, 100) into tests/golden/to_wave_helper.json: per system the lengths, the status and the
backward passes of every episode. CPU only, a minute or two (the 100-step episodes take seconds
each). The car is not recorded: its long episodes stop at max_iter on the helper, and the test
compares a 3-pass solve with the helper at test time instead.

    python tools/to_wave_record.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ilqr_ref as R  # noqa: E402
import to_wave_cases as W  # noqa: E402

SYSTEMS = ("single_integrator", "double_integrator")


def record(system):
    P = R.Problem(system)
    S0, Te = W.stride_inputs(system)
    status, iters = [], []
    for e in range(len(Te)):
        T = int(Te[e])
        r = P.solve(S0[e], np.zeros((T, P.m)), T)
        status.append(int(r["status"]))
        iters.append(int(r["iters"]))
    return dict(seed=W.STRIDE_SEED, Te=[int(t) for t in Te], status=status, iters=iters)


if __name__ == "__main__":
    out = {s: record(s) for s in SYSTEMS}
    for s, r in out.items():
        print(s, "status", r["status"], "iters", r["iters"])
    with open(os.path.join(ROOT, "tests", "golden", "to_wave_helper.json"), "w") as f:
        json.dump(out, f, indent=1)
