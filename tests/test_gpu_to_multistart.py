"""GPU checks of the multi-start TO (cacto_to_starts, cacto_to_select, TO.solve_multistart and its
callers) against tests/multistart_ref.py. Every comparison is exact: the generator is integer
arithmetic, the perturbation two separately rounded float64 operations, the selection a copy, and
the solver treats every episode on its own, so candidate block c of the one N E solve equals a
plain solve_batch of that block."""
import functools
import random

import numpy as np
import pytest
import torch

import ilqr_ref as R
import multistart_ref as M
from test_gpu_to_solve import PREFILL, _dev, _prefilled, _setup
from test_to_multistart_boundary import select_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _np(d):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


def _same(got, want, names=None):
    for k in names or want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k], equal_nan=True), k


# ---------------------------------------------------------------------- cacto_to_starts
@pytest.mark.parametrize("zero_start", [0, 1])
def test_starts_equal_the_reference_bit_for_bit(zero_start):
    P, to = _setup("double_integrator")
    E, ldU, N, hold, sigma = 5, 7, 4, 3, 0.5           # ldU is no multiple of hold
    rng = np.random.default_rng(3)
    S0, U = rng.normal(size=(E, P.n + 1)), rng.normal(size=(E, ldU, P.m))
    n = np.array([7, 3, -1, 0, 5], dtype=np.int32)
    cfg = dict(starts=N, start_sigma=sigma, start_hold=hold)
    half = np.asarray(P.conf.u_max, dtype=np.float64)[:P.m]
    assert np.array_equal(to._half_range(cfg), half)
    seed = (11 << 32) | 2
    got = [a.cpu().numpy() for a in to.multistart_expand(_dev(S0), _dev(U), _dev(n), cfg, seed=seed,
                                                         zero_start=zero_start)]
    want = M.starts(S0, U, n, N, sigma, hold, half, zero_start, seed)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert np.array_equal(got[1][:E], U) and np.array_equal(got[0], np.tile(S0, (N, 1)))
    assert np.array_equal(got[2], np.tile(n, N))
    assert (np.abs(got[1][2 * E:] - np.tile(U, (N - 2, 1, 1))) > 0).all()        # really perturbed
    other = to.multistart_expand(_dev(S0), _dev(U), _dev(n), cfg, seed=seed + 1, zero_start=zero_start)[1].cpu().numpy()
    first = 2 if zero_start else 1                      # another seed moves the perturbed candidates only
    assert np.array_equal(other[:first * E], got[1][:first * E]) and not (other[first * E:] == got[1][first * E:]).any()
    # the cfg's own stream when no seed is given, and bounds set the unit of sigma
    a = to.multistart_expand(_dev(S0), _dev(U), _dev(n), dict(cfg, start_seed=seed), zero_start=zero_start)[1]
    assert np.array_equal(a.cpu().numpy(), got[1])
    box = dict(cfg, bounds=([-1.0, -4.0], [2.0, 4.0]))
    b = to.multistart_expand(_dev(S0), _dev(U), _dev(n), box, seed=seed, zero_start=zero_start)[1].cpu().numpy()
    assert np.array_equal(b, M.starts(S0, U, n, N, sigma, hold, [1.5, 4.0], zero_start, seed)[1])


# ---------------------------------------------------------------------- cacto_to_select
@pytest.mark.parametrize("accept_maxiter", [0, 1])
def test_select_equals_the_reference_on_the_hand_made_cases(accept_maxiter):
    """The cases of test_to_multistart_boundary.select_cases (no acceptable candidate, an exact tie,
    MAXITER with and without accept_maxiter, a NaN cost under CONVERGED, a skipped episode, rows past
    Te); what the reference itself gives on them is asserted there."""
    from cacto_amd.confs import load_conf
    from cacto_amd.environment import make_env
    from cacto_amd.to import TO
    sol, nsteps, out = select_cases()                  # ns = 3, na = 2: the single integrator's shapes
    conf = load_conf("single_integrator")
    assert (conf.nb_state, conf.nb_action) == (3, 2)
    to = TO(make_env(conf), conf)
    E, N = 6, 3
    want = M.select(sol, nsteps, N, accept_maxiter, out)
    got = _np(to.multistart_select({k: _dev(v) for k, v in sol.items()}, _dev(nsteps), N, accept_maxiter,
                                   out={k: _dev(v) for k, v in out.items()}))
    assert sorted(got) == sorted(want)
    _same(got, want)
    assert got["start"][4] == -1 and (got["S"][4] == -777.0).all() and got["status"][4] == -7
    assert np.array_equal(got["J"][got["start"] >= 0, 0], sol["J"][:E, 0][got["start"] >= 0])
    # without `out`: solve_batch's own prefill (zeros, status -1)
    bare = _np(to.multistart_select({k: _dev(v) for k, v in sol.items()}, _dev(nsteps), N, accept_maxiter))
    zero = {k: np.zeros_like(v) for k, v in out.items()}
    zero["status"][:] = -1
    _same(bare, M.select(sol, nsteps, N, accept_maxiter, zero))


# ---------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _inputs(system):
    """Six episodes, Te <= 12: one skipped, one of length 0, and a warm start that is not zero."""
    from oracle import env as oenv
    P, _ = _setup(system)
    rng = random.Random(17)
    oe = oenv.make_env(P.conf)
    S0 = np.array([oe.reset(rng) for _ in range(6)], dtype=np.float64)
    Te = np.array([12, 7, 1, -1, 5, 0], dtype=np.int32)
    S0[:, -1] = (P.conf.NSTEPS - np.maximum(Te, 0)) * P.conf.dt
    g = np.random.default_rng(5)
    U0 = 0.3 * np.asarray(P.conf.u_max, dtype=np.float64)[:P.m] * g.uniform(-1, 1, size=(6, 12, P.m))
    return S0, Te, U0


@pytest.mark.parametrize("path", [0, "wave"])
@pytest.mark.parametrize("system", ["single_integrator", "double_integrator"])
def test_solve_multistart_equals_the_pick_among_separate_solves(system, path):
    P, to = _setup(system)
    S0, Te, U0 = _inputs(system)
    E, ldU, N = 6, 12, 3
    # four passes: some candidates converge, others stop at the limit, so both acceptance rules bite
    cfg = dict(R.SOLVE_CFG, poll_every=0, path=path, max_iter=4, starts=N, start_sigma=0.5, start_hold=4)
    seed = 77
    half = np.asarray(P.conf.u_max, dtype=np.float64)[:P.m]
    S0a, Ua, na = M.starts(S0, U0, Te, N, 0.5, 4, half, 1, seed)
    blocks = [_np(to.solve_batch(_dev(S0a[c * E:(c + 1) * E]), _dev(Ua[c * E:(c + 1) * E]), _dev(na[c * E:(c + 1) * E]),
                                 cfg=cfg)) for c in range(N)]
    sol_all = {k: np.concatenate([b[k] for b in blocks]) for k in blocks[0]}
    print(system, path, "status per candidate", sol_all["status"].reshape(N, E).tolist())
    pre = _np(_prefilled(E, ldU, P.n + 1, P.m))
    S0_d, U0_d, Te_d = _dev(S0), _dev(U0), _dev(Te)
    for accept in (False, True):
        want = M.select(sol_all, Te, N, accept, pre)
        got = _np(to.solve_multistart(S0_d, U0_d, Te_d, cfg=cfg, out=_prefilled(E, ldU, P.n + 1, P.m), seed=seed,
                                      zero_start=True, accept_maxiter=accept))
        assert sorted(got) == sorted(want)
        _same(got, want)
        live = Te >= 0
        assert (got["start"][live] >= 0).all() and got["start"][~live].tolist() == [-1]
        assert (got["S"][3] == PREFILL).all() and got["status"][3] == -7          # the skipped episode
        st0, J0 = want["status_starts"][:, 0], want["J_starts"][:, 0]
        ok0 = live & ((st0 == R.CONVERGED) | (accept & (st0 == R.MAXITER))) & np.isfinite(J0)
        assert (got["J"][ok0, 1] <= J0[ok0]).all()
        if accept:
            assert ok0[live].all() and (got["n_ok"][live] >= 1).all()
    # two identical calls
    again = _np(to.solve_multistart(S0_d, U0_d, Te_d, cfg=cfg, out=_prefilled(E, ldU, P.n + 1, P.m), seed=seed,
                                    zero_start=True, accept_maxiter=True))
    _same(again, got)
    # one start is solve_batch: the same dict, nothing added
    one = dict(cfg, starts=1)
    a = to.solve_multistart(S0_d, U0_d, Te_d, cfg=one, out=_prefilled(E, ldU, P.n + 1, P.m), seed=seed)
    b = to.solve_batch(S0_d, U0_d, Te_d, cfg=one, out=_prefilled(E, ldU, P.n + 1, P.m))
    assert sorted(a) == sorted(b) == ["J", "S", "U", "iters", "status", "step_cost"]
    a, b = _np(a), _np(b)
    _same(a, b)
    for k in ("status", "iters", "J"):                  # and it is candidate 0's solve (the skipped episode aside)
        assert np.array_equal(a[k][live], blocks[0][k][live]), k
    # captured into a graph and replayed
    assert to.solve_plan(cfg)["on_device"] == 1
    out = _prefilled(E, ldU, P.n + 1, P.m)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            cap = to.solve_multistart(S0_d, U0_d, Te_d, cfg=cfg, out=out, seed=seed, zero_start=True,
                                      accept_maxiter=True)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    _same(_np(cap), got)


# ---------------------------------------------------------------------- compute_samples
def _di_conf():
    from test_gpu_ensemble_train import _conf
    return _conf()


def test_compute_samples_with_three_starts():
    from cacto_amd.environment import make_env
    from cacto_amd.neural_network import NN
    from cacto_amd.replay_buffer import ReplayBuffer
    from cacto_amd.rl import RL_AC, multistart_stats
    from cacto_amd.to import TO, stream_key
    conf = _di_conf()
    env = make_env(conf)
    TrOp = TO(env, conf, 1e-2)
    rl = RL_AC(env, NN(env, conf, 1e-2, seed=3), conf)
    rl.setup_model()
    rl.start_seed = 4
    random.seed(5)
    ics = [env.reset() for _ in range(6)]
    N = 3
    cfg = dict(max_iter=30, starts=N)
    half = np.asarray(conf.u_max, dtype=np.float64)[:conf.nb_action]
    COUNTERS = ("rows", "n_kept", "zero_length", "nan_rollouts", "converged", "maxiter", "failed")
    for ep in (0, 1):                    # zero warm start (no zero candidate), then the actor's roll-out
        buf = ReplayBuffer(conf)
        got = rl.compute_samples(ep, ics, TrOp, buf, cfg=cfg, accept_maxiter=True)
        # by hand: the reference's candidates, one plain solve per block, the reference's pick
        res, pre = rl.samples_rollout(ep, ics)
        E, T = pre["E"], pre["T"]
        warm, live = pre["warm"].cpu().numpy(), pre["live"].cpu().numpy()
        assert (warm == 0).all() == (ep == 0)
        S0a, Ua, na = M.starts(pre["S0"].cpu().numpy(), warm, live, N, 0.5, 8, half, ep != 0, stream_key(4, ep))
        blocks = [_np(TrOp.solve_batch(_dev(S0a[c * E:(c + 1) * E]), _dev(Ua[c * E:(c + 1) * E]),
                                       _dev(na[c * E:(c + 1) * E]), cfg=cfg)) for c in range(N)]
        sol_all = {k: np.concatenate([b[k] for b in blocks]) for k in blocks[0]}
        zero = {k: np.zeros_like(v[:E]) for k, v in sol_all.items()}
        zero["status"][:] = -1
        pick = M.select(sol_all, live, N, True, zero)
        print("loop", ep, "start", pick["start"].tolist(), "n_ok", pick["n_ok"].tolist(), got["multistart"])
        hand_buf = ReplayBuffer(conf)
        hand = rl.samples_collect(res, pre, {k: _dev(v) for k, v in pick.items()}, TrOp, hand_buf, True, cfg=cfg)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got["kept"], hand["kept"])
        assert [got[k] for k in COUNTERS] == [hand[k] for k in COUNTERS]
        np.testing.assert_array_equal(got["ep_return"], hand["ep_return"])
        assert torch.equal(buf.storage, hand_buf.storage) and buf.next_idx == hand_buf.next_idx
        for name in ("status", "iters", "S", "U", "step_cost", "dVdx", "EE_TO"):
            assert torch.equal(got["dev"][name], hand["dev"][name]), (ep, name)
        assert got["multistart"] == multistart_stats(pick, hand["kept"], True)
        assert got["multistart"]["starts"] == N and sum(got["multistart"]["won_by"]) == got["n_kept"]
        # one start on the same initial states: candidate 0 is that very solve, so nothing kept is lost
        one = rl.compute_samples(ep, ics, TrOp, ReplayBuffer(conf), cfg=dict(max_iter=30), accept_maxiter=True)
        assert "multistart" not in one
        assert got["n_kept"] >= one["n_kept"] >= 1
        _same(_np(dict(status=one["dev"]["status"], iters=one["dev"]["iters"])),
              dict(status=blocks[0]["status"], iters=blocks[0]["iters"]))


# ---------------------------------------------------------------------- train_ensemble against train
def test_train_ensemble_equals_train_with_two_starts(tmp_path):
    from cacto_amd import main as Mn
    from test_gpu_ensemble_train import SEEDS, W_S, _conf, _same_run
    quiet = lambda *_: None
    kw = dict(w_S=W_S, to_cfg=dict(max_iter=30, starts=2), accept_maxiter=True, n_loops=1, log=quiet)
    solo = [Mn.train(_conf(tmp_path / ("solo%d" % r)), seed=s, N_try=r, **kw) for r, s in enumerate(SEEDS)]
    for o in solo:
        assert len(o["multistart"]) == 1 and o["multistart"][0]["starts"] == 2 and o["multistart"][0]["ep"] == 0
        assert sum(o["multistart"][0]["won_by"]) == o["counts_per_loop"][0]["n_kept"] >= 1
    random.seed(99)
    np.random.seed(99)
    keep = random.getstate(), np.random.get_state()
    lines = []
    outs = Mn.train_ensemble(_conf(tmp_path / "ens"), SEEDS, N_try=0, **dict(kw, log=lambda *a: lines.append(a[0])))
    assert random.getstate() == keep[0]
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), keep[1]))
    torch.cuda.synchronize()
    for r, (got, ref) in enumerate(zip(outs, solo)):
        _same_run(got, ref, SEEDS[r], counter=3)
        assert repr(got["multistart"]) == repr(ref["multistart"])             # repr: a NaN median compares equal
    assert sum("Multi-start loop 0: starts=2" in str(x) for x in lines) == len(SEEDS)
    # one start: the list is there and empty
    one = Mn.train(_conf(tmp_path / "one"), seed=SEEDS[0], **dict(kw, to_cfg=dict(max_iter=30)))
    assert one["multistart"] == []


# ---------------------------------------------------------------------- refusals
def test_refusals_enqueue_nothing():
    from cacto_amd import _lib as L
    from cacto_amd.system import dptr, stream
    P, to = _setup("double_integrator")
    E, ldU, N = 3, 4, 2
    S0, U, n = _dev(np.zeros((E, P.n + 1))), _dev(np.ones((E, ldU, P.m))), _dev(np.full(E, 4, dtype=np.int32))
    S0a = torch.full((N * E, P.n + 1), PREFILL, dtype=torch.float64, device="cuda")
    Ua = torch.full((N * E, ldU, P.m), PREFILL, dtype=torch.float64, device="cuda")
    na = torch.full((N * E,), -7, dtype=torch.int32, device="cuda")
    half = np.ones(P.m)

    def starts(N=N, sigma=0.5, hold=2, U=U):
        L.lib().call("cacto_to_starts", to.sys.handle, dptr(S0), dptr(U) if U is not None else None, ldU, dptr(n), E, N,
                     sigma, hold, half.ctypes.data, 1, 0, dptr(S0a), dptr(Ua), dptr(na), stream())
    for bad, msg in ((dict(N=0), "n_starts"), (dict(N=17), "n_starts"), (dict(hold=0), "hold < 1"),
                     (dict(sigma=-0.5), "sigma"), (dict(sigma=float("nan")), "sigma"),
                     (dict(sigma=float("inf")), "sigma"), (dict(U=None), "null")):
        with pytest.raises(RuntimeError, match="cacto_to_starts: .*" + msg):
            starts(**bad)
    torch.cuda.synchronize()
    assert (S0a == PREFILL).all() and (Ua == PREFILL).all() and (na == -7).all()
    starts()                                            # and the same call with good arguments writes
    torch.cuda.synchronize()
    assert torch.equal(Ua[:E], U) and (na == 4).all()
    sol = _prefilled(N * E, ldU, P.n + 1, P.m)
    with pytest.raises(ValueError, match="multistart_select"):
        to.multistart_select(sol, n, 17)
    with pytest.raises(ValueError, match="multistart_select"):
        to.multistart_select(sol, n, 3)                 # 6 rows are not 3 candidates of 3 episodes
    for bad in (dict(starts=0), dict(starts=17), dict(start_sigma=-1.0), dict(start_hold=0)):
        with pytest.raises(ValueError, match="TO start"):
            to.solve_multistart(S0, U, n, cfg=bad)
        with pytest.raises(ValueError, match="TO start"):
            to.solve_batch(S0, U, n, cfg=bad)
