"""GPU checks of the batched iLQR trajectory optimiser (cacto_to_backward_gains, cacto_to_forward,
cacto_to_solve; TO.TO_System_Solve / TO_Solve, TO.py:37-117) against tests/ilqr_ref.py, the same
algorithm in numpy over the oracle.

UR5 full solve: statuses, monotone cost and the step checks only. Whether the solver converges on
UR5 within a given budget has not been measured anywhere (the oracle's complex-step dynamics make
the helper too slow to say), so nothing is asserted about it.
"""
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

import ilqr_ref as R
from conftest import GOLDEN
from cacto_amd.confs import load_conf
from oracle import buffer as obuf

pytestmark = pytest.mark.gpu

SYSTEMS = ("single_integrator", "double_integrator", "car", "car_park", "manipulator", "ur5")
CHAINS = ("manipulator", "ur5")        # the float64 env_step parity classes of test_gpu_parity.py
TRIG = ("car", "car_park")
RTOL = 1e-9                            # the recursion's rule of test_gpu_ddp.py
GTOL = R.SOLVE_CFG["gtol"]
# Stationarity of a solution is checked with the adjoint gradient, which is not the solver's own
# criterion max|Q_u|: the two differ by feedback terms of the order |K| |Q_u|. On the helper's
# converged solutions of solve_inputs() the largest ratio |adjoint gradient|_inf / max|Q_u| was
# 3.3 (tests/golden/to_ilqr_helper.json, "ratio"; single integrator); ten times that.
MARGIN = 33.0
PREFILL = 7.25


@functools.lru_cache(maxsize=None)
def _setup(system):
    from cacto_amd.environment import make_env
    from cacto_amd.to import TO
    P = R.Problem(system)
    return P, TO(make_env(P.conf), P.conf, w_S=1e-2)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _check_steps(system, P, S, U, cost, T):
    """Every step of one returned episode against the oracle: simulate, the TO cost, the time column."""
    n = P.n
    for t in range(T):
        ref = P.oe.simulate(S[t], U[t])
        if system in CHAINS or system in TRIG:
            np.testing.assert_allclose(S[t + 1, :n], ref[:n], rtol=1e-12, atol=1e-12)
        else:
            np.testing.assert_array_equal(S[t + 1, :n], ref[:n])
        np.testing.assert_allclose(cost[t], P.cost(S[t], U[t]), rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(cost[T], P.cost(S[T]), rtol=1e-11, atol=1e-14)
    np.testing.assert_array_equal(S[:T + 1, n], S[0, n] + P.dt * np.arange(T + 1))


# ---------------------------------------------------------------------- backward gains
@functools.lru_cache(maxsize=None)
def _helper_backward(system, mu):
    P, _ = _setup(system)
    S, U, T = R.random_episodes(system)
    return [(P.backward(S[e], U[e], int(T[e]), mu), P.backward(S[e], U[e], int(T[e]), mu, inverse="inv"))
            for e in range(len(T))]


@pytest.mark.parametrize("mu", [0.0, 1.0])
@pytest.mark.parametrize("system", SYSTEMS)
def test_backward_gains_match_helper(system, mu):
    P, to = _setup(system)
    S, U, T = R.random_episodes(system)
    out = to.backward_gains_batch(_dev(S), _dev(U), _dev(T), mu=mu)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for e, (ref, alt) in enumerate(_helper_backward(system, mu)):
        Te = int(T[e])
        # the verdict must not hang on rounding: the helper's decisive eigenvalue ratio is far from 0
        assert abs(ref["decisive"]) >= 1e-3, (system, e, ref["decisive"])
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


# ---------------------------------------------------------------------- forward pass
@pytest.mark.parametrize("system", SYSTEMS)
def test_forward_pass(system):
    P, to = _setup(system)
    S, U, T = R.random_episodes(system)
    # mu = 10 keeps most steps positive definite; gains below a failing step stay zero, which is
    # as good a feedback law as any for this check
    g = to.backward_gains_batch(_dev(S), _dev(U), _dev(T), mu=10.0)
    alpha = 0.25
    S_new, U_new, cost = (t.cpu().numpy() for t in to.forward_batch(_dev(S), _dev(U), g["k"], g["K"], _dev(T), alpha))
    k, K = g["k"].cpu().numpy(), g["K"].cpu().numpy()
    n = P.n
    for e in range(len(T)):
        Te = int(T[e])
        assert np.isfinite(S_new[e, :Te + 1]).all()
        np.testing.assert_array_equal(S_new[e, 0], S[e, 0])
        ref_u = U[e, :Te] + alpha * k[e, :Te] + np.einsum("tij,tj->ti", K[e, :Te], S_new[e, :Te, :n] - S[e, :Te, :n])
        scale = max(np.abs(ref_u).max(), 1.0)
        assert np.abs(U_new[e, :Te] - ref_u).max() <= 1e-12 * scale
        _check_steps(system, P, S_new[e], U_new[e], cost[e], Te)
        assert (S_new[e, Te + 1:] == 0).all() and (U_new[e, Te:] == 0).all() and (cost[e, Te + 1:] == 0).all()


# ---------------------------------------------------------------------- full solve
def _prefilled(E, ldU, ns, na):
    f64 = dict(dtype=torch.float64, device="cuda")
    return dict(S=torch.full((E, ldU + 1, ns), PREFILL, **f64), U=torch.full((E, ldU, na), PREFILL, **f64),
                step_cost=torch.full((E, ldU + 1), PREFILL, **f64),
                status=torch.full((E,), -7, dtype=torch.int32, device="cuda"),
                iters=torch.full((E,), -7, dtype=torch.int32, device="cuda"), J=torch.full((E, 2), PREFILL, **f64))


def _solve(system, cfg=None, U_init=None):
    P, to = _setup(system)
    S0, Te = R.solve_inputs(system)
    E, ldU = len(Te), int(max(Te.max(), 1))
    U0 = np.zeros((E, ldU, P.m)) if U_init is None else U_init
    c = dict(R.SOLVE_CFG, poll_every=8)
    c.update(cfg or {})
    out = to.solve_batch(_dev(S0), _dev(U0), _dev(Te), cfg=c, out=_prefilled(E, ldU, P.n + 1, P.m))
    torch.cuda.synchronize()
    return P, S0, Te, {k: v.cpu().numpy() for k, v in out.items()}


def _check_masking(P, S0, Te, out):
    for e in range(len(Te)):
        T = int(Te[e])
        if T < 0:       # skipped: nothing of it is written
            for name in ("S", "U", "step_cost", "J"):
                assert (out[name][e] == PREFILL).all(), (e, name)
            assert out["status"][e] == -7 and out["iters"][e] == -7
            continue
        assert (out["S"][e, T + 1:] == PREFILL).all() and (out["U"][e, T:] == PREFILL).all()
        assert (out["step_cost"][e, T + 1:] == PREFILL).all()
        np.testing.assert_array_equal(out["S"][e, 0], S0[e])
        if T == 0:
            assert out["status"][e] == R.CONVERGED and out["iters"][e] == 0
            np.testing.assert_allclose(out["step_cost"][e, 0], P.cost(S0[e]), rtol=1e-11, atol=1e-14)
            assert out["J"][e, 0] == out["J"][e, 1] == out["step_cost"][e, 0]


@pytest.mark.parametrize("system", SYSTEMS[:5])
def test_full_solve_converges(system):
    with open(os.path.join(GOLDEN, "to_ilqr_helper.json")) as f:
        rec = json.load(f)[system]
    assert all(s in (R.CONVERGED, -1) for s in rec["status"])      # the helper converged first, on these inputs
    P, S0, Te, out = _solve(system)
    live = Te >= 0
    print(system, "iters max", out["iters"][live].max(), "mean %.1f" % out["iters"][live].mean(),
          "helper max", max(rec["iters"]), "status", np.bincount(out["status"][live], minlength=3))
    assert (out["status"][live] == R.CONVERGED).all(), np.nonzero(live & (out["status"] != R.CONVERGED))
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


def test_full_solve_ur5_runs():
    P, S0, Te, out = _solve("ur5", cfg=dict(max_iter=30))
    print("ur5 status", out["status"], "iters", out["iters"], "J", out["J"])
    assert set(out["status"].tolist()) <= {R.CONVERGED, R.MAXITER, R.FAILED}
    assert (out["J"][:, 1] <= out["J"][:, 0]).all()
    assert (out["iters"] >= 1).all() and (out["iters"] <= 30).all()
    for e in range(len(Te)):
        _check_steps("ur5", P, out["S"][e], out["U"][e], out["step_cost"][e], int(Te[e]))


# ---------------------------------------------------------------------- edges
def test_failed_is_reachable_and_keeps_the_warm_start():
    """mu_max below mu_min: the first episode whose Q_uu is not positive definite along the warm
    start cannot be regularised and ends FAILED after one pass, with the warm start in place."""
    system = "single_integrator"
    P, S0, Te, out = _solve(system, cfg=dict(mu_max=1e-7))
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


@pytest.mark.parametrize("system", ["single_integrator", "manipulator"])
def test_deterministic_and_polling_invariant(system):
    a = _solve(system)[3]
    b = _solve(system)[3]
    c = _solve(system, cfg=dict(poll_every=0))[3]
    d = _solve(system, cfg=dict(poll_every=4))[3]
    for other in (b, c, d):
        for name in a:
            assert np.array_equal(a[name], other[name]), name


def test_solve_without_polling_captures_into_a_graph():
    """poll_every = 0 enqueues no host synchronisation: the closed-form family's solve (k_to_order +
    the persistent kernel) captured into a HIP graph and replayed equals the eager call."""
    system = "single_integrator"
    P, to = _setup(system)
    S0, Te = R.solve_inputs(system)
    E, ldU = len(Te), int(Te.max())
    cfg = dict(R.SOLVE_CFG, poll_every=0)
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


def test_building_blocks_skip_masked_episodes():
    """nsteps = -1 in cacto_to_backward_gains / cacto_to_forward: nothing of the episode is written."""
    for system in ("car", "manipulator"):           # one of each kernel family
        P, to = _setup(system)
        S, U, T = R.random_episodes(system)
        T = T.copy()
        T[1] = -1
        g = to.backward_gains_batch(_dev(S), _dev(U), _dev(T), mu=1.0)
        assert not g["k"][1].any() and not g["K"][1].any() and not g["dJ"][1].any() and g["pd"][1] == -1
        assert g["k"][0].any() and g["dJ"][0].any()
        S_new, U_new, cost = to.forward_batch(_dev(S), _dev(U), g["k"], g["K"], _dev(T), 0.5)
        assert not S_new[1].any() and not U_new[1].any() and not cost[1].any()
        assert S_new[0].any() and cost[0].any()


def test_bad_arguments_fail_loudly():
    import ctypes as C
    from cacto_amd import _lib as L
    from cacto_amd.system import System, dptr, stream
    from cacto_amd.to import make_cfg
    P, to = _setup("double_integrator")
    E, ldU, ns, na = 2, 3, P.n + 1, P.m
    o = _prefilled(E, ldU, ns, na)
    S0 = torch.zeros(E, ns, dtype=torch.float64, device="cuda")
    U0 = torch.zeros(E, ldU, na, dtype=torch.float64, device="cuda")
    n = torch.full((E,), 3, dtype=torch.int32, device="cuda")
    nbytes = int(L.lib().raw("cacto_to_workspace_bytes")(to.sys.handle, E, ldU + 1))
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    cfg = make_cfg()

    def call(handle=to.sys.handle, ldS=ldU + 1, c=C.byref(cfg), ws_bytes=nbytes):
        L.lib().call("cacto_to_solve", handle, dptr(S0), dptr(U0), ldU, dptr(n), E, ldS, c, dptr(o["S"]), dptr(o["U"]),
                     dptr(o["step_cost"]), dptr(o["status"]), dptr(o["iters"]), dptr(o["J"]), dptr(ws), ws_bytes,
                     stream())
    with pytest.raises(RuntimeError, match="ldS < 1"):
        call(ldS=0)
    with pytest.raises(RuntimeError, match="null config"):
        call(c=None)
    with pytest.raises(RuntimeError, match="workspace"):
        call(ws_bytes=nbytes - 1)
    bad = types.SimpleNamespace(**{k: getattr(P.conf, k) for k in dir(P.conf) if not k.startswith("__")})
    bad.cost_weights_terminal = np.array(P.conf.cost_weights_terminal, dtype=np.float64)
    bad.cost_weights_terminal[6] = 0.5
    with pytest.raises(RuntimeError, match=r"w_terminal\[6\]"):
        call(handle=System(bad).handle)
    torch.cuda.synchronize()
    assert (o["status"] == -7).all()       # no call got as far as a kernel
    assert L.lib().raw("cacto_to_workspace_bytes")(to.sys.handle, E, 0) == 0


# ---------------------------------------------------------------------- reference signatures
def test_to_solve_reference_signature():
    P, to = _setup("double_integrator")
    S0, Te = R.solve_inputs("double_integrator")
    e = int(np.argmax(Te))
    T = int(Te[e])
    warm = np.zeros((T + 1, P.n + 1))               # accepted and ignored (single shooting)
    U, X, flag, ee, step_cost, dVdx = to.TO_Solve(S0[e], warm, np.zeros((T, P.m), dtype=np.float32), T)
    assert flag == 1
    assert U.shape == (T, P.m) and X.shape == (T + 1, P.n + 1) and ee.shape == (T + 1, 3)
    assert step_cost.shape == (T + 1,) and dVdx.shape == (T + 1, P.n + 1)
    np.testing.assert_array_equal(X[:, -1], S0[e, -1] + P.dt * np.arange(T + 1))
    np.testing.assert_array_equal(dVdx, to.backward_pass(T + 1, X, U))
    np.testing.assert_allclose(ee[:, :2], X[:, :2], rtol=0, atol=1e-12)        # DI: the EE is (x, y)
    flag, U2, X2, ee2, total, sc2 = to.TO_System_Solve(S0[e], warm, np.zeros((T, P.m)), T)
    assert flag == 1 and X2.shape == (T + 1, P.n) and total == pytest.approx(sc2.sum(), rel=1e-12)
    np.testing.assert_array_equal(U2, U)
    # the reference's failure branch: no budget, no success
    flag, U3, X3, ee3, total3, sc3 = to.TO_System_Solve(S0[e], warm, np.zeros((T, P.m)), T, cfg=dict(max_iter=1))
    assert flag == 0 and ee3 is None and total3 is None and sc3 is None and U3.shape == (T, P.m)
    assert to.TO_System_Solve(S0[e], warm, np.zeros((T, P.m)), T, cfg=dict(max_iter=1), accept_maxiter=True)[0] == 1
    assert to.TO_Solve(S0[e], warm, np.zeros((T, P.m)), T, cfg=dict(max_iter=1))[2] == 0


# ---------------------------------------------------------------------- one closed iteration
def test_one_closed_iteration_single_integrator():
    """create_TO_init_batch -> solve_batch -> backward_pass_batch -> add_episodes (rewards =
    -step_cost: env_RL = 0, RL.py:168) -> 4 updates, all through the shims."""
    from cacto_amd.environment import make_env
    from cacto_amd.neural_network import NN
    from cacto_amd.replay_buffer import ReplayBuffer
    from cacto_amd.rl import RL_AC
    from cacto_amd.to import TO
    conf = load_conf("single_integrator", fresh=True)
    env = make_env(conf)
    rl = RL_AC(env, NN(env, conf, 1e-2), conf, 0)
    rl.setup_model()
    to = TO(env, conf, w_S=1e-2)
    buffer = ReplayBuffer(conf)
    S0, Te = R.solve_inputs("single_integrator")
    keep = np.nonzero(Te > 0)[0][:8]
    ICS = S0[keep]
    init = rl.create_TO_init_batch(0, [s for s in ICS])
    assert all(r[4] == 1 for r in init)
    nsteps = np.array([r[3] for r in init], dtype=np.int32)
    np.testing.assert_array_equal(nsteps, Te[keep])
    ldU, ns, na = int(nsteps.max()), conf.nb_state, conf.nb_action
    U0 = np.zeros((len(init), ldU, na))
    for k, r in enumerate(init):
        U0[k, :r[3]] = np.asarray(r[2], dtype=np.float64)          # roll-out actions are float32
    sol = to.solve_batch(_dev(ICS), _dev(U0), _dev(nsteps), cfg=dict(R.SOLVE_CFG, poll_every=8))
    assert (sol["status"] == R.CONVERGED).all()
    dVdx = to.backward_pass_batch(sol["S"], sol["U"], _dev(nsteps))
    buffer.add_episodes(sol["S"], -sol["step_cost"], nsteps, dVdx=dVdx)
    store = buffer.storage.cpu().numpy()
    S, cost, dV = sol["S"].cpu().numpy(), sol["step_cost"].cpu().numpy(), dVdx.cpu().numpy()
    pos = 0
    for e, T in enumerate(nsteps):
        p, _, sn, d, term = obuf.rl_solve(S[e, :T + 1], cost[e, :T + 1], conf.nsteps_TD_N, MC=bool(conf.MC))
        rows = np.concatenate([S[e, :T + 1], p[:, None], sn, dV[e, :T + 1], d[:, None], term[:, None]], axis=1)
        np.testing.assert_array_equal(store[pos:pos + T + 1], rows)
        pos += T + 1
    assert buffer.next_idx == pos
    idx = torch.as_tensor(np.random.default_rng(3).integers(0, pos, size=(4, conf.BATCH_SIZE)).astype(np.int32),
                          device="cuda")
    rl.update_rows_n(buffer.storage, idx)
    torch.cuda.synchronize()
    for m in (rl.actor_model, rl.critic_model, rl.target_critic):
        assert torch.isfinite(m.buf).all()
    assert rl.steps.cpu().tolist() == [4, 4]
