"""Record what the numpy iLQR helper under hard control limits (tests/ilqr_box.py) does on the
full-solve inputs of tests/test_gpu_to_solve.py into tests/golden/to_box_helper.json: per system the
status and the backward passes of every episode (-1: skipped), as tools/to_psd_record.py does for the
projected Hessian, and beside them
  bound_scale  the bounds as a fraction of the conf's u_min / u_max (ilqr_box.BOUND_SCALE: 1 where the
               conf's own bind on these inputs, tightened on the manipulator);
  at_bound     the share of the batch's returned controls that sit on a bound;
  excluded     the episodes along whose solve a PD verdict or a comparison of the line search came
               within ilqr_box.FLIP (relative) of flipping: another rounding may take another path
               there, so a pass count may legitimately differ;
  kkt_ratio    the largest ratio, over the converged episodes, of the first-order (KKT) violation of
               the returned controls measured with the adjoint gradient to the episode's own final
               dJ[2]: what the margin of tests/test_gpu_to_box.py is derived from.
It refuses to write unless, per system, the helper converges on at least 9 in 10 live episodes, at
least 1 in 10 controls are at a bound, at least 1 in 10 are free, and at most 1 in 10 episodes are
excluded. CPU only, several minutes; UR5 is left out (the oracle's complex-step dynamics are too
slow to iterate on).

    python tools/to_box_record.py            # the record
    python tools/to_box_record.py --seeds [system ...]   # the random_episodes seeds of the gains test (printed)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ilqr_box as X  # noqa: E402
import ilqr_ref as R  # noqa: E402


def record(system):
    P = X.BoxProblem(system, "test")
    S0, Te = R.solve_inputs(system)
    status, iters, excluded = [], [], []
    at_bound = total = 0
    ratio = 0.0
    for e in range(len(Te)):
        T = int(Te[e])
        if T < 0:
            status.append(-1)
            iters.append(-1)
            continue
        r = P.solve(S0[e], np.zeros((max(T, 1), P.m)), T)
        status.append(int(r["status"]))
        iters.append(int(r["iters"]))
        if r["flip"] < X.FLIP:
            excluded.append(e)
        U = r["U"][:T]
        assert ((U >= P.lo) & (U <= P.hi)).all()
        at_bound += int(((U == P.lo) | (U == P.hi)).sum())
        total += U.size
        if T > 0 and r["status"] == R.CONVERGED and r["qu"] > 0:     # qu == 0: every control is held, nothing to violate
            ratio = max(ratio, P.kkt_violation(r["S"], r["U"], T) / r["qu"])
    live = sum(s >= 0 for s in status)
    out = dict(status=status, iters=iters, bound_scale=X.BOUND_SCALE[system], at_bound=at_bound / total,
               excluded=excluded, kkt_ratio=ratio)
    print(system, "converged", sum(s == R.CONVERGED for s in status), "of", live, "passes", sum(v for v in iters if v > 0),
          "controls at a bound %d / %d" % (at_bound, total), "excluded", excluded, "kkt ratio %.3g" % ratio, flush=True)
    assert sum(s == R.CONVERGED for s in status) >= 0.9 * live, system
    assert 0.1 <= out["at_bound"] <= 0.9, system
    assert len(excluded) <= 0.1 * live, system
    return out


def seeds(systems):
    out = {}
    for system in systems or R.SOLVE_SHAPES:
        P = X.BoxProblem(system, "conf")       # the gains test's bounds: the conf's own on every system
        for seed in range(21, 200):
            S, U, T = R.random_episodes(system, seed=seed)
            U = P.clamp(U)
            b = {mu: [P.backward(S[e], U[e], int(T[e]), mu) for e in range(len(T))] for mu in (0.0, 1.0)}
            decisive = min(abs(r["decisive"]) for rs in b.values() for r in rs)
            margin = min(r["qp_margin"] for rs in b.values() for r in rs)
            # per mu, over the episodes whose pass went through: controls the QP clamps, controls it leaves free
            clamped = [sum(int((~r["free"]).sum()) for r in rs if r["pd"] < 0) for rs in b.values()]
            free = [sum(int(r["free"].sum()) for r in rs if r["pd"] < 0) for rs in b.values()]
            print(system, "seed", seed, "decisive %.3g" % decisive, "qp margin %.3g" % margin, "clamped", clamped, "free", free,
                  flush=True)
            if decisive >= 1e-3 and margin >= 1e-6 and min(clamped) > 0 and min(free) > 0:
                out[system] = seed
                break
    print(out)


if __name__ == "__main__":
    if "--seeds" in sys.argv:
        seeds([a for a in sys.argv[1:] if a in R.SOLVE_SHAPES])
        sys.exit(0)
    out = {s: record(s) for s in R.SOLVE_SHAPES if s != "ur5"}
    with open(os.path.join(ROOT, "tests", "golden", "to_box_helper.json"), "w") as f:
        json.dump(out, f, indent=1)
