"""GPU checks of the trajectory optimiser's convexified-Hessian mode (cacto_to_opts.hessian =
CACTO_TO_HESS_PSD, `hessian="psd"`): every node's l_xx replaced by its projection onto the positive
semidefinite cone (cacto_amd/csrc/psd_project.h, a Jacobi iteration) before the Riccati recursion.
The reference is tests/ilqr_psd.py: tests/ilqr_ref.py's numpy iLQR with l_xx clipped through
numpy.linalg.eigh, whose statuses and pass counts on the full-solve inputs are recorded in
tests/golden/to_psd_helper.json (tools/to_psd_record.py). Tolerances are those of
test_gpu_to_solve.py; comparisons between the solvers of a system are np.array_equal."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import ilqr_psd as Q
import ilqr_ref as R
import to_wave_cases as W
from conftest import GOLDEN
from test_gpu_to_solve import GTOL, MARGIN, RTOL, SYSTEMS, _check_masking, _check_steps, _dev, _prefilled, _setup, _solve
from test_gpu_to_split_wave import OUTPUTS, _assert_bitwise, _stride_inputs, _stride_lengths
from test_gpu_to_wave import _solve_given

pytestmark = pytest.mark.gpu

CLOSED = ("single_integrator", "double_integrator", "car")
PSD = dict(R.SOLVE_CFG, poll_every=8, hessian="psd")


@functools.lru_cache(maxsize=None)
def _problem(system):
    return Q.PsdProblem(system)


# ---------------------------------------------------------------------- 1. backward gains
@functools.lru_cache(maxsize=None)
def _helper_backward(system, mu):
    P = _problem(system)
    S, U, T = R.random_episodes(system, seed=Q.GAINS_SEEDS[system])
    return [(P.backward(S[e], U[e], int(T[e]), mu), P.backward(S[e], U[e], int(T[e]), mu, inverse="inv"))
            for e in range(len(T))]


@pytest.mark.parametrize("mu", [0.0, 1.0])
@pytest.mark.parametrize("system", SYSTEMS)
def test_backward_gains_match_the_projected_helper(system, mu):
    P, to = _problem(system), _setup(system)[1]
    S, U, T = R.random_episodes(system, seed=Q.GAINS_SEEDS[system])
    # the batch exercises the projection: it changes l_xx on some node (the seed was picked for it)
    change = max(P.projection_change(S[e], int(T[e])) for e in range(len(T)))
    print(system, "largest relative change of l_xx under the projection %.3g" % change)
    assert change > 1e-6, system
    out = to.backward_gains_batch(_dev(S), _dev(U), _dev(T), mu=mu, hessian="psd")
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for e, (ref, alt) in enumerate(_helper_backward(system, mu)):
        Te = int(T[e])
        assert abs(ref["decisive"]) >= 1e-3, (system, e, ref["decisive"])      # the verdict does not hang on rounding
        print(system, mu, e, "pd", ref["pd"], got["pd"][e], "decisive %.3g" % ref["decisive"])
        assert got["pd"][e] == ref["pd"], (system, e)
        if ref["pd"] >= 0:
            continue
        for name in ("k", "K", "dJ"):
            r, a = ref[name], alt[name]
            g = got[name][e][:Te] if name != "dJ" else got[name][e]
            tol = RTOL * (np.abs(r).max() + 1e-12) + 100.0 * np.abs(a - r).max()
            err = np.abs(g - r).max() if r.size else 0.0
            print("   ", name, "err %.3g tol %.3g" % (err, tol))
            assert err <= tol, (system, e, name, err, tol)


# ---------------------------------------------------------------------- 2. full solve
@pytest.mark.parametrize("system", SYSTEMS[:5])
def test_full_solve_matches_the_projected_helper(system):
    with open(os.path.join(GOLDEN, "to_psd_helper.json")) as f:
        rec = json.load(f)[system]
    Pq = _problem(system)
    P, S0, Te, out = _solve(system, cfg=PSD)
    live = Te >= 0
    want_status, want_iters = np.asarray(rec["status"]), np.asarray(rec["iters"])
    print(system, "iters", out["iters"][live].tolist(), "helper", want_iters[live].tolist())
    assert (out["status"][live] == want_status[live]).all(), np.nonzero(live & (out["status"] != want_status))
    assert (out["iters"][live] == want_iters[live]).all(), np.nonzero(live & (out["iters"] != want_iters))
    assert (out["J"][live, 1] <= out["J"][live, 0]).all()
    _check_masking(P, S0, Te, out)
    worst = 0.0
    for e in np.nonzero(live)[0]:
        T = int(Te[e])
        _check_steps(system, P, out["S"][e], out["U"][e], out["step_cost"][e], T)
        np.testing.assert_allclose(out["J"][e, 1], out["step_cost"][e, :T + 1].sum(), rtol=1e-12)
        if T > 0 and want_status[e] == R.CONVERGED:
            # the gradient does not see l_xx: the projected problem's stationary points are the exact one's
            worst = max(worst, np.abs(Pq.gradient(out["S"][e], out["U"][e], T)).max())
    print(system, "adjoint gradient inf-norm %.3g (bound %.3g)" % (worst, GTOL * MARGIN))
    assert (want_status[live] == R.CONVERGED).all()         # the helper converged on every episode of these inputs
    assert worst <= GTOL * MARGIN


def test_full_solve_ur5_runs():
    P, S0, Te, out = _solve("ur5", cfg=dict(PSD, max_iter=30))
    print("ur5 psd status", out["status"], "iters", out["iters"], "J", out["J"])
    assert set(out["status"].tolist()) <= {R.CONVERGED, R.MAXITER, R.FAILED}
    assert (out["J"][:, 1] <= out["J"][:, 0]).all()
    assert (out["iters"] >= 1).all() and (out["iters"] <= 30).all()
    for e in range(len(Te)):
        _check_steps("ur5", P, out["S"][e], out["U"][e], out["step_cost"][e], int(Te[e]))


# ---------------------------------------------------------------------- 3. one loop, every solver
@pytest.mark.parametrize("system", CLOSED + ("car_park",))
def test_the_two_solvers_of_a_system_agree_bit_for_bit(system):
    """Thread and wave solver (closed forms), host-issued loop and persistent kernel (car_park) call
    the one psd_project: the full-solve batch and three passes on the lengths around the strides
    give the same outputs under path 0 and path 1."""
    a, b = _solve(system, cfg=dict(PSD, path=0))[3], _solve(system, cfg=dict(PSD, path="wave"))[3]
    _assert_bitwise(a, b)
    if system == "car_park":
        lengths = _stride_lengths(_setup(system)[1].solve_plan(dict(path="wave", hessian="psd"))["block_threads"])
        assert {1, 2, 63, 64, 65, 254, 255, 256} <= set(lengths)
        S0, Te = _stride_inputs(system, lengths)
    else:
        S0, Te = W.stride_inputs(system)
        assert {1, 2, 63, 64, 65} <= set(Te.tolist())
    cfg = dict(PSD, max_iter=3)
    P, c = _solve_given(system, S0, Te, dict(cfg, path=0))
    d = _solve_given(system, S0, Te, dict(cfg, path=1))[1]
    print(system, "status", c["status"].tolist(), "iters", c["iters"].tolist())
    _assert_bitwise(c, d)
    _check_masking(P, S0, Te, c)
    assert np.isfinite(c["J"]).all() and (c["iters"] >= 1).all() and (c["iters"] <= 3).all()
    # the mode is on: the exact Hessian gives other numbers on the same inputs
    x = _solve_given(system, S0, Te, dict(cfg, path=0, hessian="exact"))[1]
    assert not np.array_equal(x["U"], c["U"])


def test_chains_run_the_host_issued_loop_under_either_path_and_repeat():
    a = _solve("manipulator", cfg=dict(PSD, path=0))[3]
    _assert_bitwise(a, _solve("manipulator", cfg=dict(PSD, path=1))[3])
    _assert_bitwise(a, _solve("manipulator", cfg=dict(PSD, path=0, poll_every=0))[3])


@pytest.mark.parametrize("system", ["double_integrator", "car_park"])
def test_masked_empty_and_overlong_episodes(system):
    ldU = 3
    Te = np.array([-1, 0, 3, ldU + 1], dtype=np.int32)
    S0 = R.solve_inputs(system)[0][:len(Te)]
    P, to = _setup(system)
    outs = []
    for path in (0, 1, 1):
        o = to.solve_batch(_dev(S0), _dev(np.zeros((len(Te), ldU, P.m))), _dev(Te), cfg=dict(PSD, path=path),
                           out=_prefilled(len(Te), ldU, P.n + 1, P.m))
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in o.items()})
    ref, out, again = outs
    _assert_bitwise(out, ref)
    _assert_bitwise(out, again)                         # two runs agree
    _check_masking(P, S0[:3], Te[:3], {k: v[:3] for k, v in out.items()})
    assert out["iters"][2] >= 1 and np.isfinite(out["J"][2]).all()
    _check_steps(system, P, out["S"][2], out["U"][2], out["step_cost"][2], 3)
    assert out["status"][3] == R.FAILED and out["iters"][3] == 0       # Te > ldU: nothing of it is written
    prefill = _prefilled(1, ldU, P.n + 1, P.m)
    for name in ("S", "U", "step_cost", "J"):
        assert np.array_equal(out[name][3], prefill[name][0].cpu().numpy()), name


# ---------------------------------------------------------------------- 4. exact mode is unchanged
@pytest.mark.parametrize("system", SYSTEMS)
def test_exact_mode_is_the_call_without_the_key(system):
    base = dict(max_iter=30) if system == "ur5" else {}
    for path in (0, 1):
        a = _solve(system, cfg=dict(base, path=path))[3]
        _assert_bitwise(a, _solve(system, cfg=dict(base, path=path, hessian="exact"))[3])
    S, U, T = R.random_episodes(system)
    to = _setup(system)[1]
    g, h = to.backward_gains_batch(_dev(S), _dev(U), _dev(T), mu=1.0), to.backward_gains_batch(_dev(S), _dev(U), _dev(T),
                                                                                                  mu=1.0, hessian="exact")
    for name in g:
        assert torch.equal(g[name], h[name]), name


# ---------------------------------------------------------------------- 5. plan and capture
def test_plan_reports_the_projection_launch():
    for system in CLOSED:
        to = _setup(system)[1]
        for path in (0, 1):
            assert to.solve_plan(dict(path=path, hessian="psd")) == to.solve_plan(dict(path=path))
            assert to.solve_plan(dict(path=path, hessian="psd"))["on_device"] == 1
    to = _setup("car_park")[1]
    assert to.solve_plan(dict(path="wave", hessian="psd")) == to.solve_plan(dict(path="wave"))
    assert to.solve_plan(dict(path="wave", hessian="psd"))["on_device"] == 1
    exact, psd = to.solve_plan(dict(path=0)), to.solve_plan(dict(path=0, hessian="psd"))
    assert psd == dict(exact, launches_per_iter=4) and exact["launches_per_iter"] == 3
    for system in ("manipulator", "ur5"):
        to = _setup(system)[1]
        for path in (0, 1):
            exact, psd = to.solve_plan(dict(path=path)), to.solve_plan(dict(path=path, hessian="psd"))
            print(system, path, psd)
            assert exact["launches_per_iter"] == 5 and psd == dict(exact, launches_per_iter=6) and psd["on_device"] == 0


def test_psd_wave_solve_captures_into_a_graph():
    system = "double_integrator"
    P, to = _setup(system)
    cfg = dict(PSD, path="wave", poll_every=0)
    assert to.solve_plan(cfg)["on_device"] == 1
    S0, Te = R.solve_inputs(system)
    E, ldU = len(Te), int(Te.max())
    S0_d, U0_d, Te_d = _dev(S0), _dev(np.zeros((E, ldU, P.m))), _dev(Te)
    eager = to.solve_batch(S0_d, U0_d, Te_d, cfg=cfg, out=_prefilled(E, ldU, P.n + 1, P.m))   # also sizes the workspace
    out = _prefilled(E, ldU, P.n + 1, P.m)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            to.solve_batch(S0_d, U0_d, Te_d, cfg=cfg, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    for name in OUTPUTS:
        assert torch.equal(eager[name], out[name]), name


# ---------------------------------------------------------------------- 6. the training loop
def test_training_loop_with_the_projected_hessian_keeps_exact_labels(monkeypatch):
    from cacto_amd import main as M
    from cacto_amd.confs import load_conf
    from cacto_amd.rl import RL_AC
    from cacto_amd.to import TO
    conf = load_conf("single_integrator", fresh=True)
    conf.EP_UPDATE = 16
    conf.UPDATE_LOOPS = np.array([3])
    conf.NNs_path = None
    seen = []
    real = RL_AC.compute_samples

    def spy(self, ep, ICS_list, TrOp, buffer, cfg=None, accept_maxiter=False):
        res = real(self, ep, ICS_list, TrOp, buffer, cfg=cfg, accept_maxiter=accept_maxiter)
        seen.append((cfg, res))
        return res
    monkeypatch.setattr(RL_AC, "compute_samples", spy)
    to_cfg = dict(path="wave", hessian="psd")
    out = M.train(conf, n_loops=1, w_S=1e-2, to_cfg=to_cfg, log=lambda *_: None)
    assert len(seen) == 1 and seen[0][0] == to_cfg           # passed through unchanged
    res = seen[0][1]
    assert out["counts_per_loop"][0]["n_kept"] == res["n_kept"] > 0
    assert out["update_step_counter"] == 3
    assert np.isfinite(res["ep_return"]).all() and len(res["ep_return"]) == res["n_kept"]
    assert np.isfinite(out["ep_reward_arr"][:res["n_kept"]]).all()
    # the Sobolev labels are TO.backward_pass along the kept trajectory: the exact Hessian. Checked on
    # a kept episode along whose solution the projection changes l_xx, where a recursion with the
    # projected Hessian (the gains pass of this mode, whose V_x the labels would then be) differs
    Pq = _problem("single_integrator")
    S_all, U_all = res["dev"]["S"].cpu().numpy(), res["dev"]["U"].cpu().numpy()
    changed = [int(e) for e in np.nonzero(res["kept"] > 0)[0]
               if Pq.projection_change(S_all[e], int(res["kept"][e])) > 1e-6]
    print("kept", res["n_kept"], "episodes where the projection changes l_xx", changed)
    assert changed
    e = changed[0]
    T = int(res["kept"][e])
    S, U = S_all[e, :T + 1], U_all[e, :T]
    labels = res["dev"]["dVdx"][e, :T + 1].cpu().numpy()
    to = TO(out["RLAC"].env, conf, w_S=1e-2)
    np.testing.assert_array_equal(labels, to.backward_pass(T + 1, S[:, :-1], U))
    assert np.abs(labels).max() > 0
    # ... and the two Hessians do give different recursions on that trajectory
    g = [to.backward_gains_batch(_dev(S[None]), _dev(U[None]), _dev(np.array([T], dtype=np.int32)), mu=1.0, hessian=h)
         for h in ("exact", "psd")]
    assert not torch.equal(g[0]["K"], g[1]["K"])
