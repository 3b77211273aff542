"""GPU checks of the persistent one-workgroup-per-episode solver of car_park (cacto_to_cfg.path =
CACTO_TO_PATH_WAVE, k_to_solve_split) and of cacto_to_solve_plan. The kernel runs the device
functions of the host-issued loop (path 0) and the library is built with contraction off, so it is
held to that loop bit for bit: every comparison of the two paths here is np.array_equal. A
difference is a bug in the kernel, not rounding. The manipulator and UR5 have no persistent kernel
(DESIGN.md §3): their plan says so under either path, and path 1 runs the host-issued loop."""
import ctypes as C
import functools
import json
import os
import random

import numpy as np
import pytest
import torch

import ilqr_ref as R
import to_wave_cases as W
from conftest import GOLDEN
from test_gpu_to_solve import _check_masking, _check_steps, _dev, _prefilled, _setup, _solve
from test_gpu_to_wave import _check_like_full_solve, _solve_given

pytestmark = pytest.mark.gpu

SYSTEM = "car_park"
CHAINS = ("manipulator", "ur5")
CLOSED = ("single_integrator", "double_integrator", "car")
OUTPUTS = ("S", "U", "step_cost", "status", "iters", "J")


def _assert_bitwise(a, b):
    assert sorted(a) == sorted(OUTPUTS) == sorted(b)
    for name in OUTPUTS:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), name


# ---------------------------------------------------------------------- the plan
def test_plan_tells_what_a_config_runs():
    to = _setup(SYSTEM)[1]
    wave, default = to.solve_plan(dict(path="wave")), to.solve_plan(dict(path=0))
    print(SYSTEM, "wave", wave, "default", default)
    assert wave["on_device"] == 1 and wave["launches_per_iter"] == 0
    assert wave["block_threads"] in (64, 128, 256) and wave["lds_bytes"] > 0
    assert default["on_device"] == 0 and default["launches_per_iter"] == 3
    assert to.solve_plan() == default           # the default config is path 0
    for system in CHAINS:                       # the host-issued loop under either path
        to = _setup(system)[1]
        for path in (0, 1):
            plan = to.solve_plan(dict(path=path))
            print(system, path, plan)
            assert plan["on_device"] == 0 and plan["launches_per_iter"] == 5 and plan["block_threads"] == 64
    for system in CLOSED:
        to = _setup(system)[1]
        for path in (0, 1):
            plan = to.solve_plan(dict(path=path))
            assert plan["on_device"] == 1 and plan["launches_per_iter"] == 0 and plan["block_threads"] == 64


# ---------------------------------------------------------------------- the same solver, bit for bit
@functools.lru_cache(maxsize=None)
def _full(system, path):
    """The full-solve batch of test_gpu_to_solve.py."""
    return _solve(system, cfg=dict(R.SOLVE_CFG, path=path))


def test_wave_path_is_the_default_path_bit_for_bit():
    P, S0, Te, ref = _full(SYSTEM, 0)
    out = _full(SYSTEM, 1)[3]
    print(SYSTEM, "status", out["status"].tolist(), "iters", out["iters"].tolist())
    _assert_bitwise(out, ref)
    with open(os.path.join(GOLDEN, "to_ilqr_helper.json")) as f:
        rec = json.load(f)[SYSTEM]
    _check_like_full_solve(SYSTEM, P, S0, Te, out, rec)


def test_chains_run_the_host_issued_loop_under_either_path():
    _assert_bitwise(_full("manipulator", 1)[3], _full("manipulator", 0)[3])


# ---------------------------------------------------------------------- lengths around the strides
def _stride_lengths(B):
    """W.STRIDE_TE, and the lengths whose node count Te + 1 is one short of, at and past one stride
    of a B-thread workgroup."""
    return list(W.STRIDE_TE) + sorted({B - 2, B - 1, B} - set(W.STRIDE_TE))


def _stride_inputs(system, lengths):
    """W.stride_inputs's recipe (oracle.env.reset states drawn with seed W.STRIDE_SEED, time entry
    (NSTEPS - Te) dt) continued to `lengths`, whose head is W.STRIDE_TE."""
    from cacto_amd.confs import load_conf
    from oracle import env as oenv
    conf = load_conf(system)
    oe = oenv.make_env(conf)
    rng = random.Random(W.STRIDE_SEED)
    Te = np.array(lengths, dtype=np.int32)
    S0 = np.array([oe.reset(rng) for _ in Te], dtype=np.float64)
    S0[:, -1] = (conf.NSTEPS - Te) * conf.dt
    head_S0, head_Te = W.stride_inputs(system)
    n = len(head_Te)
    assert np.array_equal(S0[:n], head_S0) and np.array_equal(Te[:n], head_Te)
    return S0, Te


def test_lengths_that_straddle_the_strides():
    system = SYSTEM
    B = _setup(system)[1].solve_plan(dict(path="wave"))["block_threads"]
    lengths = _stride_lengths(B)
    S0, Te = _stride_inputs(system, lengths)
    print(system, "block_threads", B, "Te", lengths)
    cfg = dict(R.SOLVE_CFG, max_iter=3, poll_every=8)
    P, ref = _solve_given(system, S0, Te, dict(cfg, path=0))
    out = _solve_given(system, S0, Te, dict(cfg, path=1))[1]
    print(system, "status", out["status"].tolist(), "iters", out["iters"].tolist())
    _assert_bitwise(out, ref)
    _check_masking(P, S0, Te, out)
    assert np.isfinite(out["J"]).all()
    assert (out["iters"] >= 1).all() and (out["iters"] <= 3).all()
    for e in range(len(Te)):
        _check_steps(system, P, out["S"][e], out["U"][e], out["step_cost"][e], int(Te[e]))


# ---------------------------------------------------------------------- masking
def test_masked_empty_and_overlong_episodes():
    system = "car_park"
    ldU = 3
    Te = np.array([-1, 0, 3, ldU + 1], dtype=np.int32)
    S0 = R.solve_inputs(system)[0][:len(Te)]
    P, to = _setup(system)
    outs = []
    for path in (0, 1):
        o = to.solve_batch(_dev(S0), _dev(np.zeros((len(Te), ldU, P.m))), _dev(Te),
                           cfg=dict(R.SOLVE_CFG, poll_every=8, path=path), out=_prefilled(len(Te), ldU, P.n + 1, P.m))
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in o.items()})
    ref, out = outs
    _assert_bitwise(out, ref)
    # the skipped, the empty and the 3-step episode; the over-long one has no row 0 to compare
    _check_masking(P, S0[:3], Te[:3], {k: v[:3] for k, v in out.items()})
    assert out["iters"][2] >= 1 and np.isfinite(out["J"][2]).all()
    _check_steps(system, P, out["S"][2], out["U"][2], out["step_cost"][2], 3)
    # Te > ldU: FAILED before anything of the episode is written
    assert out["status"][3] == R.FAILED and out["iters"][3] == 0
    prefill = _prefilled(1, ldU, P.n + 1, P.m)
    for name in ("S", "U", "step_cost", "J"):
        assert np.array_equal(out[name][3], prefill[name][0].cpu().numpy()), name


# ---------------------------------------------------------------------- FAILED keeps the warm start
def test_failed_is_reachable_and_keeps_the_warm_start():
    """test_wave_failed_is_reachable_and_keeps_the_warm_start on car_park: with mu_max below mu_min
    an episode whose Q_uu is not positive definite along the zero warm start (episodes 2 and 7 of
    this batch on the helper: pd = 1 and 4 at mu = 0) ends FAILED after one pass."""
    system = "car_park"
    P, S0, Te, out = _solve(system, cfg=dict(R.SOLVE_CFG, path=1, mu_max=1e-7))
    need = [e for e in range(len(Te)) if Te[e] > 0
            and P.backward(P.rollout(S0[e], np.zeros((Te[e], P.m)), int(Te[e]))[0], np.zeros((Te[e], P.m)), int(Te[e]),
                           0.0)["pd"] >= 0]
    print("car_park episodes that need regularisation at the warm start", need)
    assert need, "no episode of this batch needs regularisation"
    for e in need:
        T = int(Te[e])
        assert out["status"][e] == R.FAILED and out["iters"][e] == 1
        assert (out["U"][e, :T] == 0).all() and out["J"][e, 0] == out["J"][e, 1]
        _check_steps(system, P, out["S"][e], out["U"][e], out["step_cost"][e], T)
    _check_masking(P, S0, Te, out)
    _assert_bitwise(out, _solve(system, cfg=dict(R.SOLVE_CFG, path=0, mu_max=1e-7))[3])


# ---------------------------------------------------------------------- determinism and capture
def test_wave_path_is_deterministic_and_captures_into_a_graph():
    system = SYSTEM
    a = _full(system, 1)[3]
    b = _solve(system, cfg=dict(R.SOLVE_CFG, path=1))[3]
    _assert_bitwise(a, b)
    P, to = _setup(system)
    cfg = dict(R.SOLVE_CFG, path=1, poll_every=8)       # the default polling interval: not used on this path
    # only a config whose plan says so is captured: a host-issued loop synchronises the stream
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
    for name in eager:
        assert torch.equal(eager[name], out[name]), name
        assert np.array_equal(eager[name].cpu().numpy(), a[name]), name


# ---------------------------------------------------------------------- the workspace
def test_wave_path_sizes_and_checks_its_workspace():
    system = SYSTEM
    from cacto_amd import _lib as L
    from cacto_amd.system import dptr, stream
    from cacto_amd.to import make_cfg
    P, to = _setup(system)
    E, ldU, ns, na = 2, 3, P.n + 1, P.m
    o = _prefilled(E, ldU, ns, na)
    S0 = torch.zeros(E, ns, dtype=torch.float64, device="cuda")
    U0 = torch.zeros(E, ldU, na, dtype=torch.float64, device="cuda")
    n = torch.full((E,), 3, dtype=torch.int32, device="cuda")
    cfg = make_cfg(dict(path="wave"))
    full = int(L.lib().raw("cacto_to_workspace_bytes_cfg")(to.sys.handle, E, ldU + 1, C.byref(cfg)))
    assert full > 256 and full % 256 == 0
    ws = torch.empty(full, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="workspace"):
        L.lib().call("cacto_to_solve", to.sys.handle, dptr(S0), dptr(U0), ldU, dptr(n), E, ldU + 1, C.byref(cfg),
                     dptr(o["S"]), dptr(o["U"]), dptr(o["step_cost"]), dptr(o["status"]), dptr(o["iters"]), dptr(o["J"]),
                     dptr(ws), full - 256, stream())
    torch.cuda.synchronize()
    fresh = _prefilled(E, ldU, ns, na)                 # the call did not get as far as a kernel
    for name in o:
        assert torch.equal(o[name], fresh[name]), name
