"""GPU checks of the one-wave-per-episode path of the trajectory optimiser (cacto_to_cfg.path =
CACTO_TO_PATH_WAVE, k_to_solve_wave: single integrator, double integrator, car). It is the solver
of the default path, so it is held to what that one is held to: the numpy helper's statuses and
backward-pass counts (tests/golden/to_ilqr_helper.json, tests/golden/to_wave_helper.json) and the
checks of test_gpu_to_solve.test_full_solve_converges, with its tolerances."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import ilqr_ref as R
import to_wave_cases as W
from conftest import GOLDEN
from test_gpu_to_solve import GTOL, MARGIN, RTOL, _check_masking, _check_steps, _dev, _prefilled, _setup, _solve

pytestmark = pytest.mark.gpu

CLOSED = ("single_integrator", "double_integrator", "car")
CFG = dict(R.SOLVE_CFG, path=1)


def _solve_given(system, S0, Te, cfg):
    P, to = _setup(system)
    E, ldU = len(Te), int(max(Te.max(), 1))
    out = to.solve_batch(_dev(S0), _dev(np.zeros((E, ldU, P.m))), _dev(Te), cfg=cfg,
                         out=_prefilled(E, ldU, P.n + 1, P.m))
    torch.cuda.synchronize()
    return P, {k: v.cpu().numpy() for k, v in out.items()}


def _check_like_full_solve(system, P, S0, Te, out, rec):
    """The assertions of test_full_solve_converges, and status / iters against the helper's record."""
    live = Te >= 0
    want_status, want_iters = np.asarray(rec["status"]), np.asarray(rec["iters"])
    assert all(s in (R.CONVERGED, -1) for s in rec["status"])
    print(system, "iters", out["iters"][live].tolist(), "helper", want_iters[live].tolist())
    assert (out["status"][live] == want_status[live]).all(), np.nonzero(live & (out["status"] != want_status))
    # no episode is excluded from the count comparison
    assert (out["iters"][live] == want_iters[live]).all(), np.nonzero(live & (out["iters"] != want_iters))
    assert (out["J"][live, 1] <= out["J"][live, 0]).all()
    _check_masking(P, S0, Te, out)
    worst = 0.0
    for e in np.nonzero(live)[0]:
        T = int(Te[e])
        _check_steps(system, P, out["S"][e], out["U"][e], out["step_cost"][e], T)
        np.testing.assert_allclose(out["J"][e, 1], out["step_cost"][e, :T + 1].sum(), rtol=1e-12)
        if T > 0:
            worst = max(worst, np.abs(P.gradient(out["S"][e], out["U"][e], T)).max())
    print(system, "adjoint gradient inf-norm %.3g (bound %.3g)" % (worst, GTOL * MARGIN))
    assert worst <= GTOL * MARGIN


# ---------------------------------------------------------------------- the same solver as the helper
@pytest.mark.parametrize("system", CLOSED)
def test_wave_solve_matches_the_helper(system):
    with open(os.path.join(GOLDEN, "to_ilqr_helper.json")) as f:
        rec = json.load(f)[system]
    P, S0, Te, out = _solve(system, cfg=CFG)
    _check_like_full_solve(system, P, S0, Te, out, rec)


# ---------------------------------------------------------------------- lengths around the lanes' stride
@pytest.mark.parametrize("system", CLOSED[:2])
def test_lengths_that_straddle_the_stride(system):
    with open(os.path.join(GOLDEN, "to_wave_helper.json")) as f:
        rec = json.load(f)[system]
    S0, Te = W.stride_inputs(system)
    assert rec["Te"] == Te.tolist() == list(W.STRIDE_TE) and rec["seed"] == W.STRIDE_SEED
    P, out = _solve_given(system, S0, Te, CFG)
    _check_like_full_solve(system, P, S0, Te, out, rec)


@functools.lru_cache(maxsize=None)
def _car_three_passes():
    P, _ = _setup("car")
    S0, Te = W.stride_inputs("car")
    return S0, Te, [P.solve(S0[e], np.zeros((int(Te[e]), P.m)), int(Te[e]), cfg=dict(max_iter=3)) for e in range(len(Te))]


def test_car_lengths_that_straddle_the_stride_three_passes():
    """The car's 64- and 100-step episodes stop at max_iter on the helper, so the comparison is a
    3-pass solve against the helper run here: status and passes equal, the iterate within the
    recursion's rule of test_gpu_ddp.py (RTOL of the largest magnitude: the controls are gains
    applied along a roll-out), every step against the oracle with the step tolerances."""
    S0, Te, ref = _car_three_passes()
    P, out = _solve_given("car", S0, Te, dict(CFG, max_iter=3))
    _check_masking(P, S0, Te, out)
    for e, r in enumerate(ref):
        T = int(Te[e])
        print("car Te", T, "status", out["status"][e], r["status"], "iters", out["iters"][e], r["iters"])
        assert out["status"][e] == r["status"] and out["iters"][e] == r["iters"]
        for name, got in (("U", out["U"][e, :T]), ("S", out["S"][e, :T + 1]), ("step_cost", out["step_cost"][e, :T + 1])):
            err, tol = np.abs(got - r[name]).max(), RTOL * (np.abs(r[name]).max() + 1e-12)
            print("   ", name, "err %.3g tol %.3g" % (err, tol))
            assert err <= tol, (e, name, err, tol)
        np.testing.assert_allclose(out["J"][e], r["J"], rtol=RTOL)
        _check_steps("car", P, out["S"][e], out["U"][e], out["step_cost"][e], T)


@pytest.mark.parametrize("system", CLOSED)
def test_thread_and_wave_solvers_are_one_loop(system):
    """k_to_solve_thread and k_to_solve_wave run the same transitions (to_verdict, to_decide) over
    the same device functions, and the library is built without contraction: three passes on the
    lengths around the stride give the same outputs bit for bit under path 0 and path 1. What each
    kernel still does its own way (sequential backtracking against every step size at once, nodes
    evaluated in the recursion against records) must not change a number."""
    S0, Te = W.stride_inputs(system)
    _, a = _solve_given(system, S0, Te, dict(R.SOLVE_CFG, path=0, max_iter=3))
    _, b = _solve_given(system, S0, Te, dict(CFG, max_iter=3))
    assert sorted(a) == ["J", "S", "U", "iters", "status", "step_cost"]
    print(system, "status", a["status"].tolist(), "iters", a["iters"].tolist())
    # the batch reaches both ends of the loop: the stopping rule (Te = 1) and the pass limit
    assert (a["status"] == R.CONVERGED).any() and (a["status"] == R.MAXITER).any()
    for name in a:
        assert np.array_equal(a[name], b[name]), name


# ---------------------------------------------------------------------- path 0 is untouched
def test_default_path_is_untouched():
    system = "single_integrator"
    a = _solve(system)[3]                       # no path key
    b = _solve(system, cfg=dict(path=0))[3]
    w = _solve(system, cfg=CFG)[3]
    for name in a:
        assert np.array_equal(a[name], b[name]), name
        assert w[name].shape == a[name].shape and w[name].dtype == a[name].dtype, name
    # the split family already runs one wave per episode: path 1 is path 0
    c = _solve("car_park", cfg=dict(path=0))[3]
    d = _solve("car_park", cfg=dict(path="wave"))[3]
    for name in c:
        assert np.array_equal(c[name], d[name]), name


# ---------------------------------------------------------------------- determinism and capture
def test_wave_path_is_deterministic_and_captures_into_a_graph():
    system = "single_integrator"
    a = _solve(system, cfg=CFG)[3]
    b = _solve(system, cfg=CFG)[3]
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    P, to = _setup(system)
    S0, Te = R.solve_inputs(system)
    E, ldU = len(Te), int(Te.max())
    cfg = dict(CFG, poll_every=0)
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
    for name in eager:
        assert torch.equal(eager[name], out[name]), name
        assert np.array_equal(eager[name].cpu().numpy(), a[name]), name


def test_a_system_collected_inside_a_capture_does_not_invalidate_it():
    """The garbage collector may free a System (cacto_sys_destroy: hipFree, a stream synchronised
    and destroyed) at any allocation, also between capture begin and end, where those calls
    invalidate the capture. Its handle then has to wait until the capture is over."""
    import gc
    from cacto_amd import system as Y
    from cacto_amd.confs import load_conf
    P, to = _setup("single_integrator")
    S0, Te = R.solve_inputs("single_integrator")
    E, ldU = len(Te), int(Te.max())
    cfg = dict(CFG, poll_every=0)
    S0_d, U0_d, Te_d = _dev(S0), _dev(np.zeros((E, ldU, P.m))), _dev(Te)
    eager = to.solve_batch(S0_d, U0_d, Te_d, cfg=cfg, out=_prefilled(E, ldU, P.n + 1, P.m))
    out = _prefilled(E, ldU, P.n + 1, P.m)
    gc.collect()                            # whatever earlier tests left goes now, outside the capture
    assert not Y._DYING
    cycle = [Y.System(load_conf("double_integrator", fresh=True))]
    cycle.append(cycle)                     # only the collector frees it
    del cycle
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            gc.collect()
            assert len(Y._DYING) == 1
            to.solve_batch(S0_d, U0_d, Te_d, cfg=cfg, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    for name in eager:
        assert torch.equal(eager[name], out[name]), name
    Y.System(load_conf("double_integrator", fresh=True))        # the next System buries the dead one
    assert not Y._DYING


# ---------------------------------------------------------------------- FAILED, and the workspace
def test_wave_failed_is_reachable_and_keeps_the_warm_start():
    """test_failed_is_reachable_and_keeps_the_warm_start on the wave path."""
    system = "single_integrator"
    P, S0, Te, out = _solve(system, cfg=dict(CFG, mu_max=1e-7))
    need = [e for e in range(len(Te)) if Te[e] > 0
            and P.backward(P.rollout(S0[e], np.zeros((Te[e], P.m)), int(Te[e]))[0], np.zeros((Te[e], P.m)), int(Te[e]),
                           0.0)["pd"] >= 0]
    assert need, "no episode of this batch needs regularisation"
    for e in need:
        T = int(Te[e])
        assert out["status"][e] == R.FAILED and out["iters"][e] == 1
        assert (out["U"][e, :T] == 0).all() and out["J"][e, 0] == out["J"][e, 1]
        _check_steps(system, P, out["S"][e], out["U"][e], out["step_cost"][e], T)
    _check_masking(P, S0, Te, out)


def test_wave_path_refuses_the_default_paths_workspace():
    from cacto_amd import _lib as L
    from cacto_amd.system import dptr, stream
    from cacto_amd.to import make_cfg
    P, to = _setup("single_integrator")
    E, ldU, ns, na = 2, 3, P.n + 1, P.m
    o = _prefilled(E, ldU, ns, na)
    S0 = torch.zeros(E, ns, dtype=torch.float64, device="cuda")
    U0 = torch.zeros(E, ldU, na, dtype=torch.float64, device="cuda")
    n = torch.full((E,), 3, dtype=torch.int32, device="cuda")
    cfg = make_cfg(dict(path="wave"))
    small = int(L.lib().raw("cacto_to_workspace_bytes")(to.sys.handle, E, ldU + 1))
    full = int(L.lib().raw("cacto_to_workspace_bytes_cfg")(to.sys.handle, E, ldU + 1, C.byref(cfg)))
    assert 0 < small < full
    assert int(L.lib().raw("cacto_to_workspace_bytes_cfg")(to.sys.handle, E, ldU + 1, C.byref(make_cfg()))) == small
    assert L.lib().raw("cacto_to_workspace_bytes_cfg")(to.sys.handle, E, ldU + 1, C.byref(make_cfg(dict(path=7)))) == 0
    ws = torch.empty(full, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="workspace"):
        L.lib().call("cacto_to_solve", to.sys.handle, dptr(S0), dptr(U0), ldU, dptr(n), E, ldU + 1, C.byref(cfg),
                     dptr(o["S"]), dptr(o["U"]), dptr(o["step_cost"]), dptr(o["status"]), dptr(o["iters"]), dptr(o["J"]),
                     dptr(ws), small, stream())
    torch.cuda.synchronize()
    assert (o["status"] == -7).all()       # the call did not get as far as a kernel
