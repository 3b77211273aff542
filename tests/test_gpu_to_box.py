"""GPU checks of the trajectory optimiser's hard control limits (cacto_to_box, `bounds=`):
control-limited DDP — a box QP per node of the backward pass (cacto_amd/csrc/box_qp.h, projected
Newton), feedback on the unclamped controls only, every roll-out and the warm start clamped. The
reference is tests/ilqr_box.py: tests/ilqr_ref.py's numpy iLQR with the QP solved by enumerating the
active sets, whose statuses and pass counts on the full-solve inputs are recorded in
tests/golden/to_box_helper.json (tools/to_box_record.py). Tolerances are those of
test_gpu_to_solve.py; comparisons between the solvers of a system, and with the unbounded default,
are np.array_equal."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import ilqr_box as X
import ilqr_ref as R
import to_wave_cases as W
from conftest import GOLDEN
from test_gpu_to_solve import GTOL, RTOL, SYSTEMS, _check_masking, _check_steps, _dev, _prefilled, _setup, _solve
from test_gpu_to_split_wave import OUTPUTS, _assert_bitwise, _stride_inputs, _stride_lengths
from test_gpu_to_wave import _solve_given

pytestmark = pytest.mark.gpu

CLOSED = ("single_integrator", "double_integrator", "car")
# First-order conditions of a bounded solution are checked with the adjoint gradient, which is not the
# solver's own criterion (the projected max|Q_u|): the two differ by feedback terms of the order
# |K| |Q_u|. On the helper's converged solutions of solve_inputs() under these bounds the largest ratio
# of the violation to the episode's own final dJ[2] was 15.2 (tests/golden/to_box_helper.json,
# "kkt_ratio": 3.55 single integrator, 3.74 double integrator, 15.2 car, 5.2 car_park, 1.03
# manipulator); about twice that.
KKT_MARGIN = 30.0


@functools.lru_cache(maxsize=None)
def _problem(system, kind="test"):
    return X.BoxProblem(system, kind)


def _bounds(system):
    """The full-solve tests' bounds as the cfg key: "conf" where they are the conf's own."""
    if X.BOUND_SCALE[system] == 1.0:
        return "conf"
    P = _problem(system)
    return (P.lo.copy(), P.hi.copy())


def _box_cfg(system, **kw):
    return dict(R.SOLVE_CFG, poll_every=8, bounds=_bounds(system), **kw)


def _inside(P, U, T):
    U = U[:T]
    return bool(((U >= P.lo) & (U <= P.hi)).all())


# ---------------------------------------------------------------------- 1. backward gains
@functools.lru_cache(maxsize=None)
def _gains_inputs(system):
    P = _problem(system, "conf")
    S, U, T = R.random_episodes(system, seed=X.GAINS_SEEDS[system])
    return S, P.clamp(U), T          # drawn up to 1.2 u_max: the nominal controls must be feasible


@functools.lru_cache(maxsize=None)
def _helper_backward(system, mu):
    P = _problem(system, "conf")
    S, U, T = _gains_inputs(system)
    return [(P.backward(S[e], U[e], int(T[e]), mu), P.backward(S[e], U[e], int(T[e]), mu, inverse="inv"))
            for e in range(len(T))]


@pytest.mark.parametrize("mu", [0.0, 1.0])
@pytest.mark.parametrize("system", SYSTEMS)
def test_backward_gains_match_the_bounded_helper(system, mu):
    to = _setup(system)[1]
    S, U, T = _gains_inputs(system)
    out = to.backward_gains_batch(_dev(S), _dev(U), _dev(T), mu=mu, bounds="conf")
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    clamped = free = 0
    for e, (ref, alt) in enumerate(_helper_backward(system, mu)):
        Te = int(T[e])
        assert abs(ref["decisive"]) >= 1e-3, (system, e, ref["decisive"])      # the verdict does not hang on rounding
        assert ref["qp_margin"] >= 1e-6, (system, e, ref["qp_margin"])        # nor does any QP's active set
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
        # no feedback on a clamped control: its row of K is 0, not small
        assert (got["K"][e][:Te][~ref["free"]] == 0.0).all(), (system, e)
        clamped += int((~ref["free"]).sum())
        free += int(ref["free"].sum())
    print(system, mu, "clamped", clamped, "free", free)
    assert clamped > 0 and free > 0             # the seed was picked for it


# ---------------------------------------------------------------------- 2. forward pass
@pytest.mark.parametrize("system", SYSTEMS)
def test_forward_pass_clamps_then_simulates(system):
    P, to = _problem(system, "conf"), _setup(system)[1]
    S, U, T = _gains_inputs(system)
    g = to.backward_gains_batch(_dev(S), _dev(U), _dev(T), mu=10.0, bounds="conf")
    alpha = 1.0
    S_new, U_new, cost = (t.cpu().numpy() for t in to.forward_batch(_dev(S), _dev(U), g["k"], g["K"], _dev(T), alpha,
                                                                    bounds="conf"))
    k, K = g["k"].cpu().numpy(), g["K"].cpu().numpy()
    n = P.n
    hit = 0
    for e in range(len(T)):
        Te = int(T[e])
        assert np.isfinite(S_new[e, :Te + 1]).all()
        np.testing.assert_array_equal(S_new[e, 0], S[e, 0])
        raw = U[e, :Te] + alpha * k[e, :Te] + np.einsum("tij,tj->ti", K[e, :Te], S_new[e, :Te, :n] - S[e, :Te, :n])
        ref_u = P.clamp(raw)
        hit += int((ref_u != raw).sum())
        scale = max(np.abs(ref_u).max(), 1.0)
        assert np.abs(U_new[e, :Te] - ref_u).max() <= 1e-12 * scale
        assert _inside(P, U_new[e], Te)                 # exactly: no tolerance on the bounds
        _check_steps(system, P, S_new[e], U_new[e], cost[e], Te)
        assert (S_new[e, Te + 1:] == 0).all() and (U_new[e, Te:] == 0).all() and (cost[e, Te + 1:] == 0).all()
    # the open-loop roll-out clamps too: controls drawn up to 1.2 u_max come back as their projection
    Uraw = R.random_episodes(system, seed=X.GAINS_SEEDS[system])[1]
    S2, U2, cost2 = (t.cpu().numpy() for t in to.forward_batch(_dev(S), _dev(Uraw), None, None, _dev(T), bounds="conf"))
    for e in range(len(T)):
        Te = int(T[e])
        np.testing.assert_array_equal(U2[e, :Te], P.clamp(Uraw[e, :Te]))
        _check_steps(system, P, S2[e], U2[e], cost2[e], Te)
    assert (P.clamp(Uraw) != Uraw).any()
    print(system, "closed-loop controls the clamp changed:", hit)


# ---------------------------------------------------------------------- 3. full solve
@pytest.mark.parametrize("system", SYSTEMS[:5])
def test_full_solve_matches_the_bounded_helper(system):
    """Status and pass count of every live, non-excluded episode equal the helper's record; every
    control inside the bounds exactly; monotone cost; steps, masking; first-order conditions.

    The pass counts depend on a clamped control landing on its bound exactly (the stopping rule and the
    QP compare with the bound by ==): the node's box is lo - ubar, hi - ubar with the offsets moved
    outward by a unit in the last place where ubar + offset would stop short of the bound
    (box_offset_lo / box_offset_hi; BoxProblem.box in the helper). With merely rounded offsets four of
    the car's episodes differed from the helper by one pass, and the helper's own count changed when
    one of its sums was reordered."""
    with open(os.path.join(GOLDEN, "to_box_helper.json")) as f:
        rec = json.load(f)[system]
    Pb = _problem(system)
    P, S0, Te, out = _solve(system, cfg=_box_cfg(system))
    live = Te >= 0
    compare = live.copy()
    compare[rec["excluded"]] = False
    want_status, want_iters = np.asarray(rec["status"]), np.asarray(rec["iters"])
    print(system, "iters", out["iters"][live].tolist(), "helper", want_iters[live].tolist(), "excluded", rec["excluded"])
    assert (out["status"][compare] == want_status[compare]).all(), np.nonzero(compare & (out["status"] != want_status))
    assert (out["J"][live, 1] <= out["J"][live, 0]).all()
    _check_masking(P, S0, Te, out)
    worst, at_bound, total = 0.0, 0, 0
    for e in np.nonzero(live)[0]:
        T = int(Te[e])
        assert _inside(Pb, out["U"][e], T), (system, e)         # every episode, whatever its status; no tolerance
        _check_steps(system, P, out["S"][e], out["U"][e], out["step_cost"][e], T)
        np.testing.assert_allclose(out["J"][e, 1], out["step_cost"][e, :T + 1].sum(), rtol=1e-12)
        at_bound += int(((out["U"][e, :T] == Pb.lo) | (out["U"][e, :T] == Pb.hi)).sum())
        total += T * P.m
        if T > 0 and out["status"][e] == R.CONVERGED:
            worst = max(worst, Pb.kkt_violation(out["S"][e], out["U"][e], T))
    print(system, "KKT violation %.3g (bound %.3g)" % (worst, GTOL * KKT_MARGIN), "controls at a bound", at_bound, "/", total)
    assert worst <= GTOL * KKT_MARGIN
    # the bounds bind, and not everywhere, as on the helper
    assert abs(at_bound / total - rec["at_bound"]) <= 0.05 and 0.1 <= at_bound / total <= 0.9
    assert (out["iters"][compare] == want_iters[compare]).all(), np.nonzero(compare & (out["iters"] != want_iters))


def test_full_solve_ur5_runs_inside_its_bounds():
    Pb = _problem("ur5")
    P, S0, Te, out = _solve("ur5", cfg=_box_cfg("ur5", max_iter=30))
    print("ur5 box status", out["status"], "iters", out["iters"], "J", out["J"])
    assert set(out["status"].tolist()) <= {R.CONVERGED, R.MAXITER, R.FAILED}
    assert (out["J"][:, 1] <= out["J"][:, 0]).all()
    assert (out["iters"] >= 1).all() and (out["iters"] <= 30).all()
    for e in range(len(Te)):
        assert _inside(Pb, out["U"][e], int(Te[e])), e
        _check_steps("ur5", P, out["S"][e], out["U"][e], out["step_cost"][e], int(Te[e]))


# ---------------------------------------------------------------------- 4. one loop, every solver
@pytest.mark.parametrize("hessian", ["exact", "psd"])
@pytest.mark.parametrize("system", CLOSED + ("car_park",))
def test_the_two_solvers_of_a_system_agree_bit_for_bit(system, hessian):
    """Thread and wave solver (closed forms), host-issued loop and persistent kernel (car_park) call
    the one to_box_qp: three passes on the lengths around the strides give the same outputs under
    path 0 and path 1, with either Hessian."""
    if system == "car_park":
        lengths = _stride_lengths(_setup(system)[1].solve_plan(dict(path="wave", bounds="conf"))["block_threads"])
        assert {1, 2, 63, 64, 65, 254, 255, 256} <= set(lengths)
        S0, Te = _stride_inputs(system, lengths)
    else:
        S0, Te = W.stride_inputs(system)
        assert {1, 2, 63, 64, 65} <= set(Te.tolist())
    cfg = _box_cfg(system, max_iter=3, hessian=hessian)
    P, c = _solve_given(system, S0, Te, dict(cfg, path=0))
    d = _solve_given(system, S0, Te, dict(cfg, path=1))[1]
    print(system, hessian, "status", c["status"].tolist(), "iters", c["iters"].tolist())
    _assert_bitwise(c, d)
    _check_masking(P, S0, Te, c)
    assert np.isfinite(c["J"]).all() and (c["iters"] >= 1).all() and (c["iters"] <= 3).all()
    Pb = _problem(system)
    assert all(_inside(Pb, c["U"][e], int(Te[e])) for e in range(len(Te)))
    # the mode is on: the unbounded solve gives other numbers on the same inputs
    x = _solve_given(system, S0, Te, dict(cfg, path=0, bounds="none"))[1]
    assert not np.array_equal(x["U"], c["U"])
    assert not all(_inside(Pb, x["U"][e], int(Te[e])) for e in range(len(Te)))


@pytest.mark.parametrize("system", ["double_integrator", "car_park", "manipulator"])
def test_full_batch_is_the_same_under_either_path_and_repeats(system):
    a = _solve(system, cfg=_box_cfg(system, path=0))[3]
    _assert_bitwise(a, _solve(system, cfg=_box_cfg(system, path=1))[3])
    if system == "manipulator":         # the host-issued loop: polling does not change a number
        _assert_bitwise(a, _solve(system, cfg=dict(_box_cfg(system, path=0), poll_every=0))[3])


@pytest.mark.parametrize("system", ["double_integrator", "car_park"])
def test_masked_empty_and_overlong_episodes(system):
    ldU = 3
    Te = np.array([-1, 0, 3, ldU + 1], dtype=np.int32)
    S0 = R.solve_inputs(system)[0][:len(Te)]
    P, to = _setup(system)
    outs = []
    for path in (0, 1, 1):
        o = to.solve_batch(_dev(S0), _dev(np.zeros((len(Te), ldU, P.m))), _dev(Te), cfg=_box_cfg(system, path=path),
                           out=_prefilled(len(Te), ldU, P.n + 1, P.m))
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in o.items()})
    ref, out, again = outs
    _assert_bitwise(out, ref)
    _assert_bitwise(out, again)                         # two runs agree
    _check_masking(P, S0[:3], Te[:3], {k: v[:3] for k, v in out.items()})
    assert out["iters"][2] >= 1 and np.isfinite(out["J"][2]).all()
    _check_steps(system, P, out["S"][2], out["U"][2], out["step_cost"][2], 3)
    assert _inside(_problem(system), out["U"][2], 3)
    assert out["status"][3] == R.FAILED and out["iters"][3] == 0       # Te > ldU: nothing of it is written
    prefill = _prefilled(1, ldU, P.n + 1, P.m)
    for name in ("S", "U", "step_cost", "J"):
        assert np.array_equal(out[name][3], prefill[name][0].cpu().numpy()), name


def test_an_infeasible_warm_start_is_clamped_before_its_roll_out():
    system = "double_integrator"
    P, Pb = _setup(system)[0], _problem(system)
    S0, Te = R.solve_inputs(system)
    ldU = int(Te.max())
    U0 = np.random.default_rng(0).uniform(-3, 3, (len(Te), ldU, P.m)) * Pb.hi
    for path in (0, 1):
        out = _solve(system, cfg=_box_cfg(system, path=path, max_iter=0), U_init=U0)[3]
        for e in np.nonzero(Te > 0)[0][:8]:
            T = int(Te[e])
            np.testing.assert_array_equal(out["U"][e, :T], Pb.clamp(U0[e, :T]))
            ref = Pb.rollout(S0[e], U0[e], T)[2]
            np.testing.assert_allclose(out["J"][e, 0], ref.sum(), rtol=1e-11)       # J[0]: the clamped warm start's cost
            assert out["J"][e, 1] == out["J"][e, 0] and out["iters"][e] == 0
            _check_steps(system, P, out["S"][e], out["U"][e], out["step_cost"][e], T)


# ---------------------------------------------------------------------- 5. the default is untouched
def _none_box():
    from cacto_amd import _lib as L
    b = L.ToBox()
    b.mode = L.CACTO_TO_BOUNDS_NONE
    b.lo[0] = b.hi[0] = float("nan")        # not looked at
    return b


@pytest.mark.parametrize("system", SYSTEMS)
def test_no_bounds_is_the_call_without_the_key(system):
    base = dict(max_iter=30) if system == "ur5" else {}
    P = _setup(system)[0]
    inf = np.full(P.m, np.inf)
    for path in (0, 1):
        a = _solve(system, cfg=dict(base, path=path))[3]                            # no key
        _assert_bitwise(a, _solve(system, cfg=dict(base, path=path, bounds="none"))[3])
        _assert_bitwise(a, _solve(system, cfg=dict(base, path=path, bounds=None))[3])
        # a cacto_to_box with mode NONE through the `_box` entry: the same kernels
        _assert_bitwise(a, _solve(system, cfg=dict(base, path=path, bounds=_none_box()))[3])
        if path == 0:
            # an open box constrains nothing: the bounded kernels reach the unbounded solution
            b = _solve(system, cfg=dict(base, path=path, bounds=(-inf, inf)))[3]
            assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["iters"], b["iters"])
            for name in ("S", "U", "step_cost", "J"):
                tol = RTOL * np.abs(a[name]).max()
                assert np.abs(a[name] - b[name]).max() <= tol, (system, name)
    S, U, T = R.random_episodes(system)
    to = _setup(system)[1]
    g = to.backward_gains_batch(_dev(S), _dev(U), _dev(T), mu=1.0)
    for none in ("none", None, _none_box()):
        h = to.backward_gains_batch(_dev(S), _dev(U), _dev(T), mu=1.0, bounds=none)
        for name in g:
            assert torch.equal(g[name], h[name]), name
    f = to.forward_batch(_dev(S), _dev(U), g["k"], g["K"], _dev(T), 0.5)
    for none in ("none", _none_box()):
        for a, b in zip(f, to.forward_batch(_dev(S), _dev(U), g["k"], g["K"], _dev(T), 0.5, bounds=none)):
            assert torch.equal(a, b)


def test_bad_bounds_of_a_real_system_are_refused():
    from cacto_amd import _lib as L
    P, to = _setup("double_integrator")
    S, U, T = R.random_episodes("double_integrator")
    for lo1, hi1 in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0)):
        b = L.ToBox()
        b.mode = L.CACTO_TO_BOUNDS_BOX
        b.lo[0], b.hi[0], b.lo[1], b.hi[1] = -1.0, 1.0, lo1, hi1        # entry 0 is fine: entry 1 < nb_action is not
        with pytest.raises(RuntimeError, match="bad bounds"):
            to.backward_gains_batch(_dev(S), _dev(U), _dev(T), bounds=b)
        with pytest.raises(RuntimeError, match="bad bounds"):
            to.forward_batch(_dev(S), _dev(U), None, None, _dev(T), bounds=b)
        with pytest.raises(RuntimeError, match="bad bounds"):
            to.solve_plan(dict(bounds=b))
        with pytest.raises(RuntimeError, match="bad bounds"):
            _solve("double_integrator", cfg=dict(bounds=b))
    b = L.ToBox()
    b.mode = L.CACTO_TO_BOUNDS_BOX
    b.lo[0], b.hi[0], b.lo[1], b.hi[1], b.lo[2], b.hi[2] = -1.0, 1.0, -1.0, 1.0, 5.0, -5.0   # past nb_action: not read
    assert to.solve_plan(dict(bounds=b))["on_device"] == 1
    with pytest.raises(ValueError, match="bounds"):
        to.solve_plan(dict(bounds=([-1.0], [1.0])))         # one value for two controls


# ---------------------------------------------------------------------- 6. plan and capture
def test_plan_is_unchanged_by_bounds():
    for system in SYSTEMS:
        to = _setup(system)[1]
        for path in (0, 1):
            for hessian in ("exact", "psd"):
                plain = to.solve_plan(dict(path=path, hessian=hessian))
                assert to.solve_plan(dict(path=path, hessian=hessian, bounds=_bounds(system))) == plain
        assert to.solve_plan(dict(path=1, bounds="conf"))["on_device"] == (0 if system in ("manipulator", "ur5") else 1)


def test_bounded_wave_solve_captures_into_a_graph():
    system = "double_integrator"
    P, to = _setup(system)
    cfg = _box_cfg(system, path="wave")
    cfg["poll_every"] = 0
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
    U = out["U"].cpu().numpy()
    assert all(_inside(_problem(system), U[e], int(Te[e])) for e in range(E) if Te[e] > 0)


# ---------------------------------------------------------------------- 7. the training loop
def test_training_loop_under_bounds_replays_feasible_controls_with_the_reference_labels(monkeypatch):
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
    to_cfg = dict(path="wave", bounds="conf")
    out = M.train(conf, n_loops=1, w_S=1e-2, to_cfg=to_cfg, log=lambda *_: None)
    assert len(seen) == 1 and seen[0][0] == to_cfg           # passed through unchanged
    res = seen[0][1]
    assert out["counts_per_loop"][0]["n_kept"] == res["n_kept"] > 0
    assert out["update_step_counter"] == 3
    assert np.isfinite(res["ep_return"]).all() and len(res["ep_return"]) == res["n_kept"]
    S_all, U_all = res["dev"]["S"].cpu().numpy(), res["dev"]["U"].cpu().numpy()
    kept = [int(e) for e in np.nonzero(res["kept"] > 0)[0]]
    lo, hi = conf.u_min, conf.u_max
    at_bound = 0
    for e in kept:
        T = int(res["kept"][e])
        U = U_all[e, :T]
        assert ((U >= lo) & (U <= hi)).all(), e             # what is replayed is feasible, exactly
        at_bound += int(((U == lo) | (U == hi)).sum())
    print("kept", res["n_kept"], "controls at a bound", at_bound)
    assert at_bound > 0                                     # and the bounds did bind on this batch
    # the Sobolev labels are TO.backward_pass along the kept trajectory: the reference's unconstrained
    # recursion, which knows no bounds. Checked on a kept episode with a control on a bound, where the
    # bounded gains pass (whose V_x the labels would otherwise be) has a zero row in K
    e = next(e for e in kept if ((U_all[e, :int(res["kept"][e])] == lo) | (U_all[e, :int(res["kept"][e])] == hi)).any())
    T = int(res["kept"][e])
    S, U = S_all[e, :T + 1], U_all[e, :T]
    labels = res["dev"]["dVdx"][e, :T + 1].cpu().numpy()
    to = TO(out["RLAC"].env, conf, w_S=1e-2)
    np.testing.assert_array_equal(labels, to.backward_pass(T + 1, S[:, :-1], U))
    assert np.abs(labels).max() > 0
    g = [to.backward_gains_batch(_dev(S[None]), _dev(U[None]), _dev(np.array([T], dtype=np.int32)), mu=1.0, bounds=b)
         for b in ("none", "conf")]
    assert not torch.equal(g[0]["K"], g[1]["K"])


def test_train_ensemble_under_bounds_equals_train_seed_by_seed(tmp_path):
    from cacto_amd import main as M
    from test_gpu_ensemble_train import SEEDS, W_S, _conf, _same_run
    to_cfg = dict(max_iter=30, bounds="conf")
    quiet = lambda *_: None  # noqa: E731
    solo = [M.train(_conf(tmp_path / ("solo%d" % r)), seed=s, N_try=r, w_S=W_S, to_cfg=to_cfg, accept_maxiter=True, log=quiet)
            for r, s in enumerate(SEEDS)]
    for o in solo:
        assert len(o["counts_per_loop"]) == 2 and all(c["n_kept"] >= 1 for c in o["counts_per_loop"])
    outs = M.train_ensemble(_conf(tmp_path / "ens"), SEEDS, N_try=0, w_S=W_S, to_cfg=to_cfg, accept_maxiter=True, log=quiet)
    torch.cuda.synchronize()
    for r, (got, ref) in enumerate(zip(outs, solo)):
        _same_run(got, ref, SEEDS[r])
    # the bounds took part: the unbounded run of the first seed fills its buffer differently
    plain = M.train(_conf(tmp_path / "plain"), seed=SEEDS[0], N_try=0, w_S=W_S, to_cfg=dict(max_iter=30),
                    accept_maxiter=True, log=quiet)
    assert not torch.equal(plain["buffer"].storage, solo[0]["buffer"].storage)
