"""GPU checks of main.py's evaluation stage: PLOT.value_grid and PLOT.traj_from_ICS against the
oracle and against the per-episode shim sequence they batch (create_TO_init -> TO_System_Solve ->
get_end_effector_position), the host random numbers the stage draws (numpy for the car, `random`
for the manipulator), and cacto_amd.main.train(evaluate=True): its records, its figures, and that it
leaves the training untouched where it draws no random number.

Tolerances: the critic against the float64 oracle within F32_TOL * abs_bound (the bound and the
helper of test_gpu_parity.py::test_forward_and_input_grad); EE positions within 1e-12 of the oracle
(test_gpu_main_loop.py); TO solutions of the batch against the one-episode solves within RTOL = 1e-9
of the largest magnitude (test_gpu_to_wave.py); everything else exact.
"""
import math
import os
import random

import numpy as np
import pytest
import torch

from conftest import load_weights
from oracle import env as oenv
from oracle import nn as onn
from test_gpu_collect import _learner
from test_gpu_parity import F32_TOL, abs_bound
from test_gpu_to_solve import RTOL
from cacto_amd.confs import load_conf

pytestmark = pytest.mark.gpu

PNG = b"\x89PNG\r\n\x1a\n"


def _plot(system, weights=None, **over):
    from cacto_amd.plot_utils import PLOT
    conf, env, rl, to = _learner(system, 1e-2, weights=weights, **over)
    return conf, env, rl, to, PLOT(0, env, rl.NN, conf, learner=rl)


def _critic_check(conf, rl, states, V):
    cw = rl.critic_model.get_weights()
    norm = conf.state_norm_arr.astype(np.float64)
    S = states.astype(np.float32).astype(np.float64)           # NN.eval's input is float32
    ref = onn.critic_forward(cw, S, norm).reshape(-1)
    bound = (F32_TOL * abs_bound("critic", cw, S, norm)).reshape(-1)
    err = np.abs(V.reshape(-1) - ref)
    print("critic: max |err| / bound = %.3g over %d states" % ((err / bound).max(), len(ref)))
    assert np.all(err <= bound), (err / bound).max()


# ---------------------------------------------------------------------- 1-3. the value grid
def test_value_grid_double_integrator():
    conf, env, rl, to, plot = _plot("double_integrator", load_weights("di_seed0_0"))
    g = plot.value_grid(rl.critic_model)
    assert g["V"].shape == (31, 31) and g["V"].dtype == np.float64 and g["ICS"].shape == (961, 5)
    np.testing.assert_array_equal(g["x"], np.linspace(-15, 15, 31))
    np.testing.assert_array_equal(g["y"], g["x"])
    s37, flag = plot.compute_ICS([g["x"][3], g["y"][7], 0], "double_integrator")
    assert flag == 0
    np.testing.assert_array_equal(g["ICS"][7 * 31 + 3], s37)   # k_y outer, k_x inner
    one = rl.NN.eval(rl.critic_model, s37[None]).cpu().numpy().astype(np.float64)
    _critic_check(conf, rl, s37[None], g["V"][3, 7])           # V[k_x, k_y]
    _critic_check(conf, rl, s37[None], one)
    _critic_check(conf, rl, g["ICS"], g["V"].T)
    assert np.array_equal(g["V"], g["V"].astype(np.float32))   # f32 outputs, stored as float64
    assert not np.isnan(g["V"]).any()
    assert plot.value_grid(rl.critic_model, "double_integrator")["V"].tolist() == g["V"].tolist()
    with pytest.raises(ValueError, match="entries"):
        plot.value_grid(rl.critic_model, "single_integrator")


def test_value_grid_car_draws_the_reference_numpy_numbers():
    conf, env, rl, to, plot = _plot("car")
    np.random.seed(3)
    g = plot.value_grid(rl.critic_model)
    got = np.random.get_state()
    np.random.seed(3)
    for _ in range(961):
        np.random.uniform(-math.pi, math.pi)
    ref = np.random.get_state()
    np.testing.assert_array_equal(got[1], ref[1])
    assert got[2:] == ref[2:]
    assert g["ICS"].shape == (961, 6) and (g["ICS"][:, 2] == 0).all()
    _critic_check(conf, rl, g["ICS"], g["V"].T)


def test_value_grid_manipulator_draws_the_reference_resets():
    conf, env, rl, to, plot = _plot("manipulator")
    random.seed(5)
    g = plot.value_grid(rl.critic_model)
    got = random.getstate()
    random.seed(5)
    ref = np.empty((61 * 61, conf.nb_state))
    for k_x in range(61):
        for k_y in range(61):
            s = env.reset()
            s[-1] = 0
            ref[k_x * 61 + k_y] = s
    assert random.getstate() == got
    np.testing.assert_array_equal(g["ICS"], ref)
    assert g["ee"].shape == (3721, 3) and g["V"].shape == (3721,)
    oe = oenv.make_env(conf)
    ee_ref = np.array([oe.get_end_effector_position(s) for s in ref])
    print("manipulator EE: max |err| = %.3g" % np.abs(g["ee"] - ee_ref).max())
    np.testing.assert_allclose(g["ee"], ee_ref, rtol=0, atol=1e-12)
    _critic_check(conf, rl, ref, g["V"])


def test_value_grid_ur5_raises():
    conf, env, rl, to, plot = _plot("ur5")
    with pytest.raises(ValueError, match="ur5"):
        plot.value_grid(rl.critic_model)


# ---------------------------------------------------------------------- 4. the TO trajectories
def _time_for(conf, rl, nsh):
    """A time built as Env.reset builds it, dt * round(time / dt), that gives NSTEPS_SH == nsh."""
    for k in (conf.NSTEPS - nsh, conf.NSTEPS - nsh + 1):
        t = conf.dt * round(k * conf.dt / conf.dt)
        if rl.nsteps_sh([t]) == nsh:
            return t
    raise AssertionError(nsh)


@pytest.mark.parametrize("init", [0, 1])
@pytest.mark.parametrize("path", ["default", "wave"])
def test_traj_from_ICS_equals_the_per_episode_sequence(path, init, monkeypatch):
    conf, env, rl, to, plot = _plot("double_integrator", load_weights("di_seed0_0"))
    cfg = dict(max_iter=30) if path == "default" else dict(max_iter=30, path="wave")
    steps, T = 21, 20
    want_nsh = [24, 30, 24, 0]
    pos = [(5.0, 5.0, 1.0, -1.0), (10.0, -8.0, 0.0, 0.0), (-12.0, 9.0, -2.0, 1.0), (3.0, 3.0, 0.0, 0.0)]
    S0 = np.array([list(p) + [_time_for(conf, rl, n)] for p, n in zip(pos, want_nsh)])
    assert [rl.nsteps_sh(s) for s in S0] == want_nsh
    lines = []
    res = plot.traj_from_ICS(S0, to, rl, init, steps, cfg=cfg, log=lines.append)
    assert len(lines) == 1 and "init = %d" % init in lines[0]
    assert res["ok"].tolist() == [True, True, True, False] and res["status"][3] == -1 and res["iters"][3] == 0
    for name, shape in (("S_RL", (4, 21, 5)), ("U_RL", (4, 20, 2)), ("S_TO", (4, 21, 5)), ("U_TO", (4, 20, 2)),
                        ("ee_RL", (4, 21, 3)), ("ee_TO", (4, 21, 3)), ("J", (4, 2))):
        assert res[name].shape == shape and res[name].dtype == np.float64, name
        assert np.isnan(res[name][3]).all() and not np.isnan(res[name][:3]).any(), name

    solved = []
    real = to.solve_batch
    monkeypatch.setattr(to, "solve_batch", lambda *a, **k: solved.append(real(*a, **k)) or solved[-1])
    worst = 0.0
    for e in range(3):
        _, X, U, nsh, ok = rl.create_TO_init(init, S0[e])
        assert ok == 1 and nsh == want_nsh[e]
        flag, U_TO, X_TO, _, _, _ = to.TO_System_Solve(S0[e], X, U, T, cfg=cfg)
        out = solved[-1]
        assert np.array_equal(res["S_RL"][e], X[:steps]) and np.array_equal(res["U_RL"][e], U[:T])
        ee_RL = np.array([env.get_end_effector_position(x) for x in X[:steps]])
        assert np.array_equal(res["ee_RL"][e], ee_RL)
        assert res["status"][e] == int(out["status"][0].item()) and res["iters"][e] == int(out["iters"][0].item())
        assert flag == int(res["status"][e] == 0)
        S_full = out["S"][0].cpu().numpy()
        ee_TO = np.array([env.get_end_effector_position(x) for x in S_full])
        for name, got, ref in (("S_TO", res["S_TO"][e][:, :4], X_TO), ("U_TO", res["U_TO"][e], U_TO),
                               ("ee_TO", res["ee_TO"][e], ee_TO), ("J", res["J"][e], out["J"][0].cpu().numpy())):
            err, tol = np.abs(got - ref).max(), RTOL * (np.abs(ref).max() + 1e-12)
            worst = max(worst, err)
            assert err <= tol, (e, name, err, tol)
    print("traj_from_ICS path %s init %d: status %s passes %s J %s, largest deviation from the one-episode solves %.3g"
          % (path, init, res["status"].tolist(), res["iters"].tolist(), res["J"][:3].tolist(), worst))
    assert (res["J"][:3, 1] <= res["J"][:3, 0]).all()
    with pytest.raises(ValueError, match="24 < steps - 1 = 25"):
        plot.traj_from_ICS(S0, to, rl, init, 26, cfg=cfg)
    # only skipped episodes: nothing is launched, everything is NaN
    none = plot.traj_from_ICS(S0[3:], to, rl, init, steps, cfg=cfg)
    assert not none["ok"].any() and np.isnan(none["ee_TO"]).all() and none["ee_TO"].shape == (1, 21, 3)
    assert len(solved) == 3


def test_traj_from_ICS_library_calls_do_not_depend_on_the_batch(monkeypatch):
    from test_gpu_collect import _Spy
    conf, env, rl, to, plot = _plot("double_integrator", load_weights("di_seed0_0"))
    S0 = np.array(conf.init_states_sim)
    seqs = []
    for n in (2, 9):
        spy = _Spy(monkeypatch)
        res = plot.traj_from_ICS(S0[:n], to, rl, 1, 11, cfg=dict(max_iter=5))
        assert res["ok"].all()
        seqs.append(spy.names)
        monkeypatch.undo()
    assert seqs[0] == seqs[1]
    assert sorted(seqs[0]) == ["cacto_env_ee", "cacto_env_ee", "cacto_rollout_sched", "cacto_to_solve"]
    spy = _Spy(monkeypatch)
    plot.value_grid(rl.critic_model)
    assert spy.names == ["cacto_critic_forward"]


# ---------------------------------------------------------------------- 5. train(evaluate=True)
def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype and \
            np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
    return type(a) is type(b) and a == b


def _train(tmp_path, tag, **kw):
    from cacto_amd import main as M
    conf = load_conf("double_integrator", fresh=True)
    over = dict(EP_UPDATE=6, UPDATE_LOOPS=np.array([3, 4]), save_interval=5, NNs_path=str(tmp_path / tag / "NNs"),
                Fig_path=str(tmp_path / tag / "Figures"), init_states_sim=conf.init_states_sim[:2])
    for k, v in over.items():
        setattr(conf, k, v)
    lines = []
    out = M.train(conf, seed=0, N_try=0, w_S=1e-2, to_cfg=dict(max_iter=30), accept_maxiter=True,
                  weights=load_weights("di_seed0_0"), log=lines.append, **kw)
    torch.cuda.synchronize()
    return conf, out, lines


def test_train_with_the_evaluation_stage(tmp_path):
    conf, out, lines = _train(tmp_path, "draw", evaluate=True)
    assert out["update_step_counter"] == 7
    folder = os.path.join(conf.Fig_path, "N_try_0")
    names = ["ee_traj_0_0", "V_3", "ee_traj_1_3", "V_7", "ee_traj_1_7", "EpReturn_0", "PolicyEvaluationSingleInit_0_7"]
    assert sorted(os.listdir(folder)) == sorted(n + ".png" for n in names)
    for n in names:
        with open(os.path.join(folder, n + ".png"), "rb") as f:
            assert f.read(8) == PNG, n
    ev = out["evaluation"]
    assert [(r["kind"], r["update_step_counter"], r["ep"]) for r in ev] == [
        ("traj", 0, None), ("value", 3, 0), ("traj", 3, 0), ("value", 7, 1), ("traj", 7, 1), ("return", 7, None),
        ("rollout", 7, None)]
    assert ev[0]["data"]["ok"].all() and ev[0]["data"]["ee_TO"].shape == (2, conf.NSTEPS, 3)
    assert not ev[0]["data"]["U_RL"].any() and ev[2]["data"]["U_RL"].any()       # zero / actor warm start
    assert ev[1]["data"]["V"].shape == (31, 31)
    np.testing.assert_array_equal(ev[5]["data"], out["ep_reward_arr"])
    assert isinstance(out["returns"], dict) and len(out["returns"]) == 2
    assert ev[6]["data"]["returns"] == out["returns"] and ev[6]["data"]["p_ee"].shape == (2, conf.NSTEPS + 1, 3)
    assert list(out["returns"]) == [(2.0, 0.0), (10.0, 0.0)]
    assert sum(l.startswith("System: double_integrator - N_try = 0") for l in lines) == 2
    assert sum(l.startswith("TO from init_states_sim") for l in lines) == 3
    assert out["evaluation_seconds"]["draw"] > 0

    # the stage draws no random number and writes no training state on this system
    _, plain, plain_lines = _train(tmp_path, "plain", evaluate=False)
    assert plain["evaluation"] == [] and plain["returns"] is None
    assert not os.path.exists(tmp_path / "plain" / "Figures")
    a, b = out["RLAC"], plain["RLAC"]
    for name in ("actor_model", "critic_model", "target_critic"):
        assert torch.equal(getattr(a, name).buf, getattr(b, name).buf), name
    for name in ("actor_m", "actor_v", "critic_m", "critic_v", "steps"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert (out["buffer"].next_idx, out["buffer"].full) == (plain["buffer"].next_idx, plain["buffer"].full)
    assert torch.equal(out["buffer"].storage, plain["buffer"].storage)
    np.testing.assert_array_equal(out["ep_reward_arr"], plain["ep_reward_arr"])
    assert [l for l in lines if l.startswith("Episode")] == plain_lines

    # draw=False: the same records, no file
    _, data, _ = _train(tmp_path, "data", evaluate=True, draw=False)
    assert not os.path.exists(tmp_path / "data" / "Figures")
    assert len(data["evaluation"]) == 7 and all(_same(x, y) for x, y in zip(data["evaluation"], ev))
    assert data["evaluation_seconds"]["draw"] == 0


# ---------------------------------------------------------------------- 6. the manipulator's resets
def test_train_evaluation_consumes_the_reference_resets(monkeypatch):
    from cacto_amd import main as M
    from cacto_amd.environment import make_env
    from cacto_amd.rl import RL_AC
    seen = []
    real = RL_AC.compute_samples

    def spy(self, ep, ICS_list, *a, **k):
        seen.append(np.array(ICS_list))
        return real(self, ep, ICS_list, *a, **k)
    monkeypatch.setattr(RL_AC, "compute_samples", spy)

    def run(**kw):
        conf = load_conf("manipulator", fresh=True)
        for k, v in dict(EP_UPDATE=4, UPDATE_LOOPS=np.array([2, 2]), init_states_sim=conf.init_states_sim[:1]).items():
            setattr(conf, k, v)
        del seen[:]
        out = M.train(conf, seed=0, to_cfg=dict(max_iter=3), accept_maxiter=True, n_loops=2, log=lambda s: None, **kw)
        return conf, out, [s.copy() for s in seen]
    conf, out, with_stage = run(evaluate=True, draw=False)
    assert [r["kind"] for r in out["evaluation"]] == ["traj", "value", "traj", "value", "traj", "return", "rollout"]
    assert out["evaluation"][1]["data"]["ICS"].shape == (3721, 7)
    _, _, without = run()
    assert len(with_stage) == len(without) == 2
    np.testing.assert_array_equal(with_stage[0], without[0])
    assert not np.array_equal(with_stage[1], without[1])
    env = make_env(conf)
    random.seed(0)
    loop0 = np.array([env.reset() for _ in range(4)])
    grid = np.array([env.reset() for _ in range(3721)])
    loop1 = np.array([env.reset() for _ in range(4)])
    np.testing.assert_array_equal(with_stage[0], loop0)
    np.testing.assert_array_equal(with_stage[1], loop1)
    grid[:, -1] = 0
    np.testing.assert_array_equal(out["evaluation"][1]["data"]["ICS"], grid)
