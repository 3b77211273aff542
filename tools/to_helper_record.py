"""Record what the numpy iLQR helper (tests/ilqr_ref.py) does on the full-solve inputs of
tests/test_gpu_to_solve.py into tests/golden/to_ilqr_helper.json: per system the status and the
backward passes of every episode (-1: skipped), and "ratio", the largest |adjoint gradient|_inf /
max|Q_u| over its converged solutions (the measurement behind the GPU test's MARGIN). CPU only,
about a minute; UR5 is left out (the oracle's complex-step dynamics are too slow to iterate on).

    python tools/to_helper_record.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ilqr_ref as R  # noqa: E402


def record(system):
    P = R.Problem(system)
    S0, Te = R.solve_inputs(system)
    status, iters, ratio = [], [], 0.0
    for e in range(len(Te)):
        T = int(Te[e])
        if T < 0:
            status.append(-1)
            iters.append(-1)
            continue
        r = P.solve(S0[e], np.zeros((max(T, 1), P.m)), T)
        status.append(int(r["status"]))
        iters.append(int(r["iters"]))
        if T > 0 and r["status"] == R.CONVERGED and r["qu"] > 0:
            ratio = max(ratio, float(np.abs(P.gradient(r["S"], r["U"], T)).max() / r["qu"]))
    return dict(status=status, iters=iters, ratio=ratio)


if __name__ == "__main__":
    out = {s: record(s) for s in R.SOLVE_SHAPES if s != "ur5"}
    for s, r in out.items():
        print(s, "converged", sum(v == R.CONVERGED for v in r["status"]), "of", sum(v >= 0 for v in r["status"]),
              "max iters", max(r["iters"]), "ratio %.3g" % r["ratio"])
    with open(os.path.join(ROOT, "tests", "golden", "to_ilqr_helper.json"), "w") as f:
        json.dump(out, f, indent=1)
