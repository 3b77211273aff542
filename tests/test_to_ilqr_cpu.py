"""The numpy iLQR helper (tests/ilqr_ref.py) checked on its own, on the CPU: its adjoint gradient
against central differences of the rolled-out cost, monotone cost, and convergence on the inputs
the GPU tests solve (tests/golden/to_ilqr_helper.json holds its full record, written by
tools/to_helper_record.py; here the first episodes of every system are solved again)."""
import json
import os

import numpy as np
import pytest

import ilqr_ref as R
from conftest import GOLDEN

SYSTEMS = ("single_integrator", "double_integrator", "car", "car_park", "manipulator")


@pytest.fixture(scope="module")
def record():
    with open(os.path.join(GOLDEN, "to_ilqr_helper.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("system", SYSTEMS)
def test_adjoint_gradient_matches_central_differences(system):
    P = R.Problem(system)
    S, U, T = R.random_episodes(system, n_ep=2, seed=4)
    for e in range(2):
        Te = min(int(T[e]), 6)
        Ue = 0.5 * U[e, :Te]
        Se, _, c = P.rollout(S[e, 0], Ue, Te)
        g = P.gradient(Se, Ue, Te)
        num = np.zeros_like(g)
        for t in range(Te):
            for j in range(P.m):
                h = 1e-5 * max(1.0, abs(Ue[t, j]))
                Up, Um = Ue.copy(), Ue.copy()
                Up[t, j] += h
                Um[t, j] -= h
                num[t, j] = (P.rollout(S[e, 0], Up, Te)[2].sum() - P.rollout(S[e, 0], Um, Te)[2].sum()) / (2 * h)
        # central differences with relative step 1e-5: truncation ~ h^2 (1e-10 relative, times the
        # third derivative's growth) and cancellation eps |J| / h ~ 2e-11 |J|; two to three decades above both
        tol = 1e-6 * np.abs(g).max() + 1e-8 * abs(c.sum())
        assert np.abs(g - num).max() <= tol, (system, e, np.abs(g - num).max(), tol)


@pytest.mark.parametrize("system", SYSTEMS)
def test_helper_converges_monotonically_on_the_named_inputs(system, record):
    rec = record[system]
    S0, Te = R.solve_inputs(system)
    assert len(rec["status"]) == len(Te)
    assert all(s == (R.CONVERGED if Te[e] >= 0 else -1) for e, s in enumerate(rec["status"]))
    assert rec["ratio"] * 10 <= 33.5            # the measurement behind the GPU test's MARGIN
    P = R.Problem(system)
    for e in range(4):
        T = int(Te[e])
        if T < 0:
            continue
        r = P.solve(S0[e], np.zeros((max(T, 1), P.m)), T)
        assert r["status"] == R.CONVERGED and r["iters"] == rec["iters"][e]
        assert (np.diff(r["hist"]) <= 0).all() and r["J"][1] <= r["J"][0]
        if T > 0:
            assert np.abs(P.gradient(r["S"], r["U"], T)).max() <= R.SOLVE_CFG["gtol"] * 10 * max(rec["ratio"], 1.0)


def test_te_zero_and_failed():
    P = R.Problem("single_integrator")
    S0, Te = R.solve_inputs("single_integrator")
    r = P.solve(S0[3], np.zeros((1, P.m)), 0)
    assert Te[3] == 0 and r["status"] == R.CONVERGED and r["iters"] == 0 and r["J"][0] == r["J"][1] == P.cost(S0[3])
    # an episode whose Q_uu is indefinite along the zero warm start cannot be regularised when mu_max < mu_min
    for e in range(len(Te)):
        T = int(Te[e])
        if T > 0 and P.backward(P.rollout(S0[e], np.zeros((T, P.m)), T)[0], np.zeros((T, P.m)), T, 0.0)["pd"] >= 0:
            r = P.solve(S0[e], np.zeros((T, P.m)), T, dict(mu_max=1e-7))
            assert r["status"] == R.FAILED and r["iters"] == 1 and not r["U"].any()
            break
    else:
        pytest.fail("no episode needs regularisation")
