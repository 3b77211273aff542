"""GPU checks of the sample-collection stage: cacto_collect_plan, cacto_env_rl_episodes and
cacto_episode_returns against numpy / the per-step calls they replace, RL_AC.compute_samples against
the per-episode shim sequence of main.py:174-195 + :240 (create_TO_init -> TO_Solve -> RL_Solve ->
buffer.add) and against the batched pieces, and cacto_amd.main.train against a hand-written loop
through the shims. Every comparison is exact: the stage only batches and filters what the pieces
compute, so a difference would mean that a piece depends on the batch it runs in.

The full-solve inputs of ilqr_ref.solve_inputs put the time (NSTEPS - Te) dt into the state; for a
few episodes RL_AC.nsteps_sh's int(t / dt) of that product is Te + 1. _ics() moves such a time up
by single ulps until nsteps_sh gives Te, so the recorded pass counts of
tests/golden/to_ilqr_helper.json (taken at Te) describe the episodes the stage solves. Neither the
cost nor the dynamics read the time.
"""
import functools
import json
import os
import random

import numpy as np
import pytest
import torch

import ilqr_ref as R
from conftest import GOLDEN, load_weights
from cacto_amd import _lib as L
from cacto_amd.confs import load_conf
from cacto_amd.system import dptr, stream

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
COUNTERS = ("rows", "n_kept", "zero_length", "nan_rollouts", "converged", "maxiter", "failed")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


# ---------------------------------------------------------------------- 1. the plan
def _plan_ref(n, rs, ts, accept):
    E = len(n)
    kept = np.full(E, -1, dtype=np.int32)
    c = np.zeros(8, dtype=np.int64)
    for e in range(E):
        if n[e] <= 0:
            c[2] += 1
            continue
        if rs is not None and rs[e] != 0:
            c[3] += 1
            continue
        ok = True
        if ts is not None:
            c[4 + ts[e]] += 1
            ok = ts[e] == R.CONVERGED or (accept and ts[e] == R.MAXITER)
        if ok:
            kept[e] = n[e]
            c[1] += 1
    off = np.zeros(E + 1, dtype=np.int64)
    np.cumsum(np.where(kept >= 0, kept.astype(np.int64) + 1, 0), out=off[1:])
    c[0] = off[-1]
    return kept, off, c


def _plan(n, rs, ts, accept):
    E = len(n)
    kept = torch.full((E,), -99, dtype=torch.int32, device="cuda")
    off = torch.full((E + 1,), -99, dtype=torch.int64, device="cuda")
    counts = torch.full((8,), -99, dtype=torch.int64, device="cuda")
    d = lambda a: None if a is None else _dev(np.asarray(a, dtype=np.int32))
    n_d, rs_d, ts_d = d(n), d(rs), d(ts)
    L.lib().call("cacto_collect_plan", dptr(n_d), dptr(rs_d), dptr(ts_d), int(accept), E, dptr(kept), dptr(off),
                 dptr(counts), stream())
    return kept.cpu().numpy(), off.cpu().numpy(), counts.cpu().numpy()


def _check_plan(n, rs, ts, accept):
    got, ref = _plan(n, rs, ts, accept), _plan_ref(n, rs, ts, accept)
    for g, r, name in zip(got, ref, ("kept", "row_off", "counts")):
        np.testing.assert_array_equal(g, r, err_msg=name)
    return ref


# the kernel scans chunks of 256 episodes (one workgroup), 64 lanes per wave
@pytest.mark.parametrize("accept", [0, 1])
@pytest.mark.parametrize("n_ep", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_plan_matches_numpy(n_ep, accept):
    rng = np.random.default_rng(100 + n_ep)
    n = rng.integers(-1, 101, size=n_ep)
    rs = (rng.uniform(size=n_ep) < 0.2).astype(np.int32)
    ts = rng.integers(0, 3, size=n_ep)
    kept, off, c = _check_plan(n, rs, ts, accept)
    if n_ep >= 255:                                # every branch of the filter is taken
        assert c[1] > 0 and c[2] > 0 and c[3] > 0 and c[5] > 0 and c[6] > 0
    _check_plan(n, None, None, accept)             # no statuses: every episode of positive length is kept
    _check_plan(n, rs, None, accept)
    _check_plan(n, None, ts, accept)


def test_plan_with_every_episode_dropped():
    n = np.array([5, 0, -1, 7, 9] * 60)
    rs = np.array([1, 0, 0, 0, 0] * 60)
    ts = np.array([0, 0, 0, 2, 1] * 60)
    kept, off, c = _check_plan(n, rs, ts, 0)
    assert (kept == -1).all() and (off == 0).all() and c[0] == 0 and c[1] == 0


# ---------------------------------------------------------------------- 2. env_RL episodes
@functools.lru_cache(maxsize=None)
def _system(system):
    from cacto_amd.environment import make_env
    conf = load_conf(system, fresh=True)
    return conf, make_env(conf)


@pytest.mark.parametrize("system", ["double_integrator", "manipulator", "car_park", "ur5"])
def test_env_rl_episodes_equal_the_per_step_calls(system):
    from oracle import env as oenv
    conf, env = _system(system)
    ns, na = conf.nb_state, conf.nb_action
    T = 6 if system == "ur5" else 12
    nsteps = np.array([T, 3, 0, -1, 1], dtype=np.int32)
    E, ldS, ldU = len(nsteps), T + 3, T + 1
    rng = random.Random(9)
    oe = oenv.make_env(conf)
    S0 = _dev(np.array([oe.reset(rng) for _ in range(E)], dtype=np.float64))
    nrng = np.random.default_rng(4)
    U = _dev(nrng.normal(size=(E, ldU, na)) * 0.5 * np.asarray(conf.u_max, dtype=np.float64)[:na])
    f64 = dict(dtype=torch.float64, device="cuda")
    new = lambda *shape: torch.full(shape, SENTINEL, **f64)
    S, Rw, EE = new(E, ldS, ns), new(E, ldS), new(E, ldS, 3)
    n_d = _dev(nsteps)
    L.lib().call("cacto_env_rl_episodes", env.sys.handle, dptr(S0), dptr(U), ldU, dptr(n_d), E, ldS, dptr(S),
                 dptr(Rw), dptr(EE), stream())
    # the loop RL_AC._env_rl_episode ran before cacto_env_rl_episodes: one cacto_env_step per step
    S_r, R_r, EE_r = new(E, ldS, ns), new(E, ldS), new(E, ldS, 3)
    W = _dev(np.asarray(conf.cost_weights_running, dtype=np.float64))
    Wt = _dev(np.asarray(conf.cost_weights_terminal, dtype=np.float64))
    zero = torch.zeros(1, na, **f64)
    h = env.sys.handle
    for e, Te in enumerate(nsteps):
        if Te < 0:
            continue
        S_r[e, 0] = S0[e]
        for i in range(Te):
            L.lib().call("cacto_env_step", h, dptr(S_r[e, i:i + 1]), dptr(U[e, i:i + 1]), dptr(W),
                         dptr(S_r[e, i + 1:i + 2]), dptr(R_r[e, i:i + 1]), dptr(EE_r[e, i + 1:i + 2]), 1, stream())
        L.lib().call("cacto_env_step", h, dptr(S_r[e, Te:Te + 1]), dptr(zero), dptr(Wt), None, dptr(R_r[e, Te:Te + 1]),
                     None, 1, stream())
        L.lib().call("cacto_env_ee", h, dptr(S_r[e, 0:1]), dptr(EE_r[e, 0:1]), 1, stream())
    for got, ref, name in ((S, S_r, "S"), (Rw, R_r, "R"), (EE, EE_r, "EE")):
        got, ref = got.cpu().numpy(), ref.cpu().numpy()
        assert np.array_equal(got, ref), (system, name, np.argwhere(got != ref)[:1])
        for e, Te in enumerate(nsteps):            # the skipped episode and the rows past Te: untouched
            assert (got[e, max(Te + 1, 0):] == SENTINEL).all(), (system, name, e)
        assert np.isfinite(got).all()
    # any output may be NULL
    S2 = new(E, ldS, ns)
    L.lib().call("cacto_env_rl_episodes", h, dptr(S0), dptr(U), ldU, dptr(n_d), E, ldS, dptr(S2), None, None, stream())
    assert torch.equal(S2, S)


# ---------------------------------------------------------------------- 3. returns
@pytest.mark.parametrize("negate", [0, 1])
def test_episode_returns_equal_python_sum(negate):
    rng = np.random.default_rng(17)
    E, ldR = 150, 50
    Rw = rng.normal(size=(E, ldR)) * 10.0 ** rng.integers(-6, 4, size=(E, ldR))
    Rw[0, 0] = -0.0
    kept = rng.integers(-1, ldR, size=E).astype(np.int32)
    kept[:4] = [0, ldR - 1, -1, 1]
    ret = torch.full((E,), SENTINEL, dtype=torch.float64, device="cuda")
    R_d, kept_d = _dev(Rw), _dev(kept)
    L.lib().call("cacto_episode_returns", dptr(R_d), ldR, dptr(kept_d), E, negate, dptr(ret), stream())
    ref = np.array([sum(-Rw[e, :k + 1] if negate else Rw[e, :k + 1]) if k >= 0 else 0.0
                    for e, k in enumerate(kept)], dtype=np.float64)
    np.testing.assert_array_equal(ret.cpu().numpy(), ref)


# ---------------------------------------------------------------------- the shim path
def _ics(system, count):
    """The first `count` full-solve inputs, the time moved up by ulps where nsteps_sh would not give Te."""
    conf = load_conf(system)
    S0, Te = R.solve_inputs(system)
    S0, Te = S0[:count].copy(), Te[:count]
    for e in range(count):
        for _ in range(4):
            if conf.NSTEPS - int(S0[e, -1] / conf.dt) == Te[e]:
                break
            S0[e, -1] = np.nextafter(S0[e, -1], np.inf)
        assert conf.NSTEPS - int(S0[e, -1] / conf.dt) == Te[e]
    return S0, Te


def _learner(system, w_S, weights=None, **over):
    from cacto_amd.environment import make_env
    from cacto_amd.neural_network import NN
    from cacto_amd.rl import RL_AC
    from cacto_amd.to import TO
    conf = load_conf(system, fresh=True)
    for k, v in over.items():
        setattr(conf, k, v)
    env = make_env(conf)
    rl = RL_AC(env, NN(env, conf, w_S, seed=5), conf, 0)
    rl.setup_model(weights=weights)
    return conf, env, rl, TO(env, conf, w_S)


def _new_buffer(conf):
    from cacto_amd.replay_buffer import PrioritizedReplayBuffer, ReplayBuffer
    return ReplayBuffer(conf) if conf.prioritized_replay_alpha == 0 else PrioritizedReplayBuffer(conf)


def _shim_iteration(rl, to, buffer, ep, ICS_list, cfg, accept_maxiter):
    """main.py:174-195 per episode and :236-240 through the reference-signature shims. Returns the
    kept episodes' (index, NSTEPS_SH, ep_return)."""
    tmp = []
    for k, ICS in enumerate(ICS_list):
        init, states, controls, T, ok = rl.create_TO_init(ep, ICS)
        if ok == 0:
            continue
        U, X, flag, ee, step_cost, dVdx = to.TO_Solve(init, states, controls, T, cfg=cfg, accept_maxiter=accept_maxiter)
        if flag == 0:
            continue
        state_arr, partial, total, s_next, done, rwrd, term, ep_return, ee_rl = rl.RL_Solve(U, X, step_cost)
        tmp.append((k, T, dVdx, state_arr.tolist(), partial, s_next, done, term, ep_return))
    if tmp:
        k, T, dVdx, state_arr, partial, s_next, done, term, ep_return = zip(*tmp)
        buffer.add(state_arr, partial, s_next, dVdx, done, term)
        return list(zip(k, T, ep_return))
    return []


def _same_buffer(a, b):
    assert (a.next_idx, a.full) == (b.next_idx, b.full)
    got, ref = a.storage.cpu().numpy(), b.storage.cpu().numpy()
    assert np.array_equal(got, ref), ("storage", np.argwhere(got != ref)[:1])
    if a.prioritized:
        for name in ("sum_tree", "min_tree"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name


class _Spy:
    """Records the entry names of lib().call."""

    def __init__(self, monkeypatch):
        self.names = []
        lib = L.lib()
        real = lib.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)
        monkeypatch.setattr(lib, "call", call)


# ---------------------------------------------------------------------- 4. stage == call sequence
PASSES = [8, 15, 6, 0, 36, 6, 10, 20, 9, 5, 14]
MAX_ITER = 12


@pytest.mark.parametrize("accept,path", [(False, "default"), (True, "default"), (False, "wave")])
def test_stage_equals_the_reference_call_sequence(accept, path):
    with open(os.path.join(GOLDEN, "to_ilqr_helper.json")) as f:
        rec = json.load(f)["single_integrator"]
    assert rec["iters"][:11] == PASSES and all(s == R.CONVERGED for s in rec["status"][:11])
    assert all(abs(p - MAX_ITER) > 1 for p in PASSES)          # the split does not hang on an edge
    ICS, Te = _ics("single_integrator", 11)
    assert Te[3] == 0 and (np.delete(Te, 3) > 0).all()
    conf, env, rl, to = _learner("single_integrator", 1e-2)
    cfg = dict(R.SOLVE_CFG, max_iter=MAX_ITER, path=path)
    buf, ref_buf = _new_buffer(conf), _new_buffer(conf)
    res = rl.compute_samples(0, [s for s in ICS], to, buf, cfg=cfg, accept_maxiter=accept)
    conv = [e for e in range(11) if e != 3 and PASSES[e] <= MAX_ITER]
    late = [e for e in range(11) if e != 3 and PASSES[e] > MAX_ITER]
    assert conv == [0, 2, 5, 6, 8, 9] and late == [1, 4, 7, 10]
    want_kept = sorted(conv + late) if accept else conv
    assert np.nonzero(res["kept"] >= 0)[0].tolist() == want_kept
    np.testing.assert_array_equal(res["kept"][want_kept], Te[want_kept])
    rows = int((Te[want_kept] + 1).sum())
    assert [res[k] for k in COUNTERS] == [rows, len(want_kept), 1, 0, 6, 4, 0]
    assert len(want_kept) == (10 if accept else 6)
    st = res["dev"]["status"].cpu().numpy()
    assert (st[conv] == R.CONVERGED).all() and (st[late] == R.MAXITER).all() and st[3] == -1
    kept = _shim_iteration(rl, to, ref_buf, 0, [s for s in ICS], cfg, accept)
    assert [k for k, _, _ in kept] == want_kept
    _same_buffer(buf, ref_buf)
    assert buf.next_idx == rows
    assert res["ep_return"].tolist() == [r for _, _, r in kept]
    assert res["dev"]["dVdx"] is not None and res["dev"]["dVdx"].any()
    assert res["dev"]["EE_TO"].shape == (11, int(Te.max()) + 1, 3)


def test_stage_without_sobolev_labels_runs_no_label_pass(monkeypatch):
    ICS, Te = _ics("single_integrator", 11)
    conf, env, rl, to = _learner("single_integrator", 0.0)
    cfg = dict(R.SOLVE_CFG, max_iter=MAX_ITER)
    buf, ref_buf = _new_buffer(conf), _new_buffer(conf)
    spy = _Spy(monkeypatch)
    res = rl.compute_samples(0, [s for s in ICS], to, buf, cfg=cfg)
    assert "cacto_ddp_backward" not in spy.names and "cacto_rl_solve_add" in spy.names
    assert res["dev"]["dVdx"] is None
    ns = conf.nb_state
    assert res["rows"] == buf.next_idx > 0
    assert not buf.storage[:, 2 * ns + 1:3 * ns + 1].any()
    _shim_iteration(rl, to, ref_buf, 0, [s for s in ICS], cfg, False)
    _same_buffer(buf, ref_buf)


def test_stage_with_nothing_to_do():
    ICS, Te = _ics("single_integrator", 11)
    conf, env, rl, to = _learner("single_integrator", 0.0)
    buf = _new_buffer(conf)
    res = rl.compute_samples(0, [ICS[3]], to, buf)              # NSTEPS_SH == 0 only: nothing is launched
    assert res["rows"] == 0 and res["n_kept"] == 0 and res["zero_length"] == 1 and buf.next_idx == 0
    assert res["kept"].tolist() == [-1] and len(res["ep_return"]) == 0
    res = rl.compute_samples(0, [s for s in ICS[:3]], to, buf, cfg=dict(R.SOLVE_CFG, max_iter=1))
    assert res["rows"] == 0 and res["maxiter"] == 3 and buf.next_idx == 0 and not buf.storage.any()
    small = _learner("single_integrator", 0.0, REPLAY_SIZE=16)
    with pytest.raises(ValueError, match="REPLAY_SIZE"):
        small[2].compute_samples(0, [s for s in ICS[:3]], small[3], _new_buffer(small[0]), cfg=dict(R.SOLVE_CFG))


# ---------------------------------------------------------------------- 5. NaN roll-outs
def test_stage_drops_nan_rollouts():
    from oracle import env as oenv
    from test_gpu_nan_abort import gated_actor, oracle_outcomes
    w = load_weights("di_seed0_final")
    conf, env, rl, to = _learner("double_integrator", 1e-2, weights=w)
    rl.actor_model.set_weights(gated_actor(w["actor"]))
    oe = oenv.make_env(conf)
    rng = random.Random(21)                                   # the start states of test_gpu_nan_abort.py
    S0 = np.array([oe.reset(rng) for _ in range(48)])[:18]
    fail, stable = oracle_outcomes(oe, w["actor"], S0)
    pinned = [k for k in range(len(S0)) if stable[k] and rl.nsteps_sh(S0[k]) > 0]
    dropped = [k for k in pinned if fail[k] is not None][:3]
    clean = [k for k in pinned if fail[k] is None][:9]
    sel = sorted(dropped + clean)
    assert len(sel) == 12 and len(dropped) >= 2 and len(clean) >= 6
    ICS = S0[sel]
    cfg = dict(R.SOLVE_CFG, max_iter=20)
    buf, ref_buf = _new_buffer(conf), _new_buffer(conf)
    res = rl.compute_samples(1, [s for s in ICS], to, buf, cfg=cfg, accept_maxiter=True)
    assert res["nan_rollouts"] == len(dropped) and res["zero_length"] == 0
    assert res["converged"] + res["maxiter"] + res["failed"] == len(clean)
    want = [j for j, k in enumerate(sel) if k in clean]
    # the pieces on the oracle-kept episodes alone
    ns_ = [rl.nsteps_sh(s) for s in S0[clean]]
    T = max(ns_)
    roll = rl.rollout_batch(S0[clean], ns_, T, ep=1, want=("S", "A"))
    assert (roll["status"] == 0).all()
    n_d = _dev(np.asarray(ns_, dtype=np.int32))
    sol = to.solve_batch(_dev(S0[clean]), roll["A"].double(), n_d, cfg=cfg)
    bad = (sol["status"] == R.FAILED).to(torch.int32)
    dVdx = to.backward_pass_batch(sol["S"], sol["U"], n_d, status=bad)
    ref_buf.add_episodes(sol["S"], -sol["step_cost"], ns_, dVdx=dVdx, status=bad)
    ok = (bad == 0).cpu().numpy()
    assert np.nonzero(res["kept"] >= 0)[0].tolist() == [j for j, good in zip(want, ok) if good]
    assert res["n_kept"] == int(ok.sum()) >= 6
    _same_buffer(buf, ref_buf)
    assert not torch.isnan(buf.storage).any()


# ---------------------------------------------------------------------- 6. env_RL, PER and wrap
def test_stage_env_rl_per_and_ring_wrap():
    ICS, _ = R.solve_inputs("car_park")
    over = dict(prioritized_replay_alpha=0.6, env_RL=1, REPLAY_SIZE=256)
    conf, env, rl, to = _learner("car_park", 1e-2, **over)
    cfg = dict(R.SOLVE_CFG, path="wave")
    buf, ref_buf = _new_buffer(conf), _new_buffer(conf)
    assert buf.prioritized
    # nine episodes give about a hundred rows: the third add passes the end of the 256-row ring
    for call, ep in enumerate((0, 1, 1)):
        res = rl.compute_samples(ep, [s for s in ICS], to, buf, cfg=cfg, accept_maxiter=True)
        kept = _shim_iteration(rl, to, ref_buf, ep, [s for s in ICS], cfg, True)
        assert res["n_kept"] == len(kept) >= 1
        assert res["ep_return"].tolist() == [r for _, _, r in kept]
        _same_buffer(buf, ref_buf)
        for name in ("S_RL", "R_RL", "EE_RL"):
            assert torch.isfinite(res["dev"][name]).all()
    assert buf.full == 1


# ---------------------------------------------------------------------- 7. call count
def test_library_calls_do_not_depend_on_the_batch(monkeypatch):
    ICS, Te = _ics("single_integrator", 11)
    live = [s for s, t in zip(ICS, Te) if t > 0]
    conf, env, rl, to = _learner("single_integrator", 1e-2)
    cfg = dict(R.SOLVE_CFG)
    seqs = []
    for E in (4, 12):
        spy = _Spy(monkeypatch)
        res = rl.compute_samples(0, (live + live)[:E], to, _new_buffer(conf), cfg=cfg)
        assert res["n_kept"] == E
        seqs.append(spy.names)
        monkeypatch.undo()
    assert seqs[0] == seqs[1] and "cacto_collect_plan" in seqs[0] and len(seqs[0]) <= 8


# ---------------------------------------------------------------------- 8. the loop
def test_train_equals_a_loop_through_the_shims(tmp_path):
    from cacto_amd import main as M
    over = dict(EP_UPDATE=6, UPDATE_LOOPS=np.array([3, 4]), save_interval=5)
    cfg = dict(max_iter=30)
    w = load_weights("di_seed0_0")
    conf = load_conf("double_integrator", fresh=True)
    for k, v in dict(over, NNs_path=str(tmp_path / "a")).items():
        setattr(conf, k, v)
    lines = []
    out = M.train(conf, seed=0, N_try=0, w_S=1e-2, to_cfg=cfg, accept_maxiter=True, weights=w, log=lines.append)
    got = out["RLAC"]
    for name in ("0", "5", "final"):
        for net in ("actor", "critic", "target_critic"):
            assert os.path.exists(os.path.join(conf.NNs_path, "N_try_0", "%s_%s.h5" % (net, name))), (net, name)
    assert out["update_step_counter"] == 7 and len(out["counts_per_loop"]) == 2

    # main.py:145-165, :216-262 by hand through the per-episode shims, same seeds
    random.seed(0)
    np.random.seed(0)
    conf2, env, rl, to = _learner("double_integrator", 1e-2, weights=w, NNs_path=str(tmp_path / "b"), **over)
    os.makedirs(os.path.join(conf2.NNs_path, "N_try_0"))
    buffer = _new_buffer(conf2)
    counter = 0
    rl.RL_save_weights(counter)
    ep_reward_arr = np.zeros(conf2.EP_UPDATE * len(conf2.UPDATE_LOOPS)) * np.nan
    idx = 0
    ref_lines = []
    for ep in range(len(conf2.UPDATE_LOOPS)):
        init_rand_state = [env.reset() for _ in range(conf2.EP_UPDATE)]
        kept = _shim_iteration(rl, to, buffer, ep, init_rand_state, cfg, True)
        assert kept
        counter = rl.learn_and_update(counter, buffer, ep)
        ep_return = [r for _, _, r in kept]
        ep_reward_arr[idx:idx + len(kept)] = ep_return
        idx += len(kept)
        for i in range(len(kept)):
            ref_lines.append("Episode  {}  --->   Return = {}".format(ep * len(kept) + i, ep_return[i]))
        assert out["counts_per_loop"][ep]["n_kept"] == len(kept)
    torch.cuda.synchronize()
    assert counter == out["update_step_counter"]
    _same_buffer(out["buffer"], buffer)
    for name in ("actor_model", "critic_model", "target_critic"):
        assert torch.equal(getattr(got, name).buf, getattr(rl, name).buf), name
    for name in ("actor_m", "actor_v", "critic_m", "critic_v", "steps"):
        assert torch.equal(getattr(got, name), getattr(rl, name)), name
    np.testing.assert_array_equal(out["ep_reward_arr"], ep_reward_arr)
    assert idx >= 6 and not np.isnan(ep_reward_arr[:idx]).any()
    assert lines == ref_lines
