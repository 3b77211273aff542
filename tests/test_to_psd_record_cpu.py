"""CPU check that tests/golden/to_psd_helper.json is what tests/ilqr_psd.py gives today: the helper
with the projected Hessian re-run on the two smallest full-solve batches (car_park and the
manipulator, 9 episodes each) must reproduce the recorded statuses and pass counts, so a change to
tests/ilqr_ref.py, to solve_inputs or to the projection cannot leave the record stale unnoticed
(tools/to_psd_record.py rewrites it). It also pins the record's shape for every system."""
import json
import os

import numpy as np
import pytest

import ilqr_psd as Q
import ilqr_ref as R
from conftest import GOLDEN


def _record():
    with open(os.path.join(GOLDEN, "to_psd_helper.json")) as f:
        return json.load(f)


def test_record_covers_the_full_solve_inputs():
    rec = _record()
    assert sorted(rec) == sorted(s for s in R.SOLVE_SHAPES if s != "ur5")
    for system, r in rec.items():
        Te = R.solve_inputs(system)[1]
        assert len(r["status"]) == len(r["iters"]) == len(Te), system
        for e, T in enumerate(Te):
            if T < 0:
                assert r["status"][e] == r["iters"][e] == -1
            else:
                assert r["status"][e] in (R.CONVERGED, R.MAXITER, R.FAILED) and r["iters"][e] >= (1 if T > 0 else 0)


@pytest.mark.parametrize("system", ["car_park", "manipulator"])
def test_record_is_what_the_helper_gives(system):
    rec = _record()[system]
    P = Q.PsdProblem(system)
    S0, Te = R.solve_inputs(system)
    changed = 0.0
    for e in range(len(Te)):
        T = int(Te[e])
        r = P.solve(S0[e], np.zeros((max(T, 1), P.m)), T)
        assert (int(r["status"]), int(r["iters"])) == (rec["status"][e], rec["iters"][e]), (system, e)
        changed = max(changed, P.projection_change(r["S"], T))
    assert changed > 1e-6           # the projection is at work on these inputs
