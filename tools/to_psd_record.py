"""Record what the numpy iLQR helper with the projected node Hessian (tests/ilqr_psd.py) does on the
full-solve inputs of tests/test_gpu_to_solve.py into tests/golden/to_psd_helper.json: per system
the status and the backward passes of every episode (-1: skipped), as tools/to_helper_record.py
does for the exact Hessian, whose figures it prints beside them. CPU only, a few minutes; UR5 is
left out (the oracle's complex-step dynamics are too slow to iterate on).

    python tools/to_psd_record.py            # the record
    python tools/to_psd_record.py --seeds    # the random_episodes seeds of the gains test (printed)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ilqr_psd as Q  # noqa: E402
import ilqr_ref as R  # noqa: E402


def record(system):
    P = Q.PsdProblem(system)
    S0, Te = R.solve_inputs(system)
    status, iters = [], []
    for e in range(len(Te)):
        T = int(Te[e])
        if T < 0:
            status.append(-1)
            iters.append(-1)
            continue
        r = P.solve(S0[e], np.zeros((max(T, 1), P.m)), T)
        status.append(int(r["status"]))
        iters.append(int(r["iters"]))
    return dict(status=status, iters=iters)


def seeds():
    out = {}
    for system in R.SOLVE_SHAPES:
        P = Q.PsdProblem(system)
        for seed in range(21, 200):
            S, U, T = R.random_episodes(system, seed=seed)
            change = max(P.projection_change(S[e], int(T[e])) for e in range(len(T)))
            decisive = min(abs(P.backward(S[e], U[e], int(T[e]), mu)["decisive"]) for e in range(len(T)) for mu in (0.0, 1.0))
            if change > 1e-6 and decisive >= 1e-3:
                out[system] = seed
                print(system, "seed", seed, "change %.3g" % change, "decisive %.3g" % decisive)
                break
    print(out)


if __name__ == "__main__":
    if "--seeds" in sys.argv:
        seeds()
        sys.exit(0)
    with open(os.path.join(ROOT, "tests", "golden", "to_ilqr_helper.json")) as f:
        exact = json.load(f)
    out = {s: record(s) for s in R.SOLVE_SHAPES if s != "ur5"}
    for s, r in out.items():
        live = [v for v in r["status"] if v >= 0]
        print(s, "converged", sum(v == R.CONVERGED for v in live), "of", len(live), "passes",
              sum(v for v in r["iters"] if v > 0), "exact Hessian", sum(v for v in exact[s]["iters"] if v > 0))
    with open(os.path.join(ROOT, "tests", "golden", "to_psd_helper.json"), "w") as f:
        json.dump(out, f, indent=1)
