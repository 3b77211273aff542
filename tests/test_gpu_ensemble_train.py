"""cacto_amd.main.train_ensemble against cacto_amd.main.train, seed by seed, and
Ensemble.compute_samples (one TO solve over every replica's episodes) against each replica's
RL_AC.compute_samples. Everything is compared bit for bit.

The conf is the double integrator shrunk as tests/test_gpu_collect.py shrinks it for its train test:
six episodes per loop, two loops of a few updates, a checkpoint interval inside the second loop, and
that test's TO settings (max_iter = 30 with accept_maxiter, so episodes are kept)."""
import os
import random

import numpy as np
import pytest
import torch

from cacto_amd.confs import load_conf

pytestmark = pytest.mark.gpu
SEEDS = (3, 11)
OVER = dict(EP_UPDATE=6, UPDATE_LOOPS=np.array([3, 4]), save_interval=5, BATCH_SIZE=20)
TO_CFG = dict(max_iter=30)
W_S = 1e-2


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _conf(path=None):
    conf = load_conf("double_integrator", fresh=True)
    for k, v in OVER.items():
        setattr(conf, k, v)
    if path is not None:
        conf.NNs_path = str(path)
    return conf


def _same_run(got, ref, tag, counter=7):
    a, b = got["RLAC"], ref["RLAC"]
    for name in ("actor_model", "critic_model", "target_critic"):
        assert torch.equal(getattr(a, name).buf, getattr(b, name).buf), (tag, name)
    for name in ("actor_m", "actor_v", "critic_m", "critic_v", "steps"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (tag, name)
    assert torch.equal(got["buffer"].storage, ref["buffer"].storage), (tag, "storage")
    assert (got["buffer"].next_idx, got["buffer"].full) == (ref["buffer"].next_idx, ref["buffer"].full), tag
    assert got["counts_per_loop"] == ref["counts_per_loop"], tag
    np.testing.assert_array_equal(got["ep_reward_arr"], ref["ep_reward_arr"])
    assert got["update_step_counter"] == ref["update_step_counter"] == counter


def test_train_ensemble_equals_train_seed_by_seed(tmp_path):
    from cacto_amd import main as M
    quiet = lambda *_: None
    solo = [M.train(_conf(tmp_path / ("solo%d" % r)), seed=s, N_try=r, w_S=W_S, to_cfg=TO_CFG, accept_maxiter=True,
                    log=quiet) for r, s in enumerate(SEEDS)]
    # the test's own conditions: every loop of every solo run keeps an episode, and the two seeds
    # keep different row counts in some loop (their buffers and index draws really differ)
    print("rows per loop:", [[c["rows"] for c in o["counts_per_loop"]] for o in solo])
    for o in solo:
        assert len(o["counts_per_loop"]) == 2 and all(c["n_kept"] >= 1 for c in o["counts_per_loop"])
    assert any(a["rows"] != b["rows"] for a, b in zip(solo[0]["counts_per_loop"], solo[1]["counts_per_loop"]))
    assert not torch.equal(solo[0]["RLAC"].critic_model.buf, solo[1]["RLAC"].critic_model.buf)

    conf = _conf(tmp_path / "ens")
    random.seed(99)                      # the process-global generators are left as they were found
    np.random.seed(99)
    keep = random.getstate(), np.random.get_state()
    outs = M.train_ensemble(conf, SEEDS, N_try=0, w_S=W_S, to_cfg=TO_CFG, accept_maxiter=True, log=quiet)
    assert random.getstate() == keep[0]
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state(), keep[1]))
    torch.cuda.synchronize()
    assert [o["seed"] for o in outs] == list(SEEDS) and [o["N_try"] for o in outs] == [0, 1]
    for r, (got, ref) in enumerate(zip(outs, solo)):
        _same_run(got, ref, SEEDS[r])
        # every replica wrote the reference's checkpoints under its own N_try, equal to the solo run's
        from cacto_amd import h5
        for step in ("0", "5", "final"):
            for net in ("actor", "critic", "target_critic"):
                mine = os.path.join(conf.NNs_path, "N_try_%d" % r, "%s_%s.h5" % (net, step))
                theirs = os.path.join(str(tmp_path / ("solo%d" % r)), "N_try_%d" % r, "%s_%s.h5" % (net, step))
                assert os.path.exists(mine), mine
                for a, b in zip(h5.read_keras_weights(mine), h5.read_keras_weights(theirs)):
                    np.testing.assert_array_equal(a, b)

    # recover_training = (path, N_try, step): replica r starts from the checkpoints under
    # N_try + r, as its solo run started from (path, N_try + r, step) does
    kw = dict(w_S=W_S, to_cfg=TO_CFG, accept_maxiter=True, n_loops=1, log=quiet)
    rec = M.train_ensemble(_conf(tmp_path / "rec_ens"), SEEDS, N_try=0, recover_training=(conf.NNs_path, 0, 5), **kw)
    for r, s in enumerate(SEEDS):
        ref = M.train(_conf(tmp_path / ("rec_solo%d" % r)), seed=s, N_try=r,
                      recover_training=(conf.NNs_path, r, 5), **kw)
        _same_run(rec[r], ref, ("recover", s), counter=8)
        assert not torch.equal(rec[r]["RLAC"].critic_model.buf, outs[r]["RLAC"].critic_model.buf)
    assert not torch.equal(rec[0]["RLAC"].critic_model.buf, rec[1]["RLAC"].critic_model.buf)
    with pytest.raises(ValueError, match="integer N_try"):
        M.train_ensemble(_conf(), SEEDS, recover_training=(conf.NNs_path, "a", 5), **kw)


def test_a_replica_that_keeps_no_episode_names_its_seed(tmp_path):
    from cacto_amd import main as M
    conf = _conf()
    # one iLQR pass converges for hardly any episode: whichever replica is the first to keep none is
    # named with its seed and its N_try (seed 11 keeps none; seed 3 may keep one)
    with pytest.raises(RuntimeError, match=r"(seed 3 \(N_try 0\)|seed 11 \(N_try 1\)), loop 0: no episode of 6"):
        M.train_ensemble(conf, SEEDS, w_S=W_S, to_cfg=dict(max_iter=1), accept_maxiter=False, log=lambda *_: None)
    pconf = _conf()
    pconf.prioritized_replay_alpha = 0.6
    with pytest.raises(ValueError, match="PER replay buffers"):
        M.train_ensemble(pconf, SEEDS, w_S=W_S)


def test_joint_solve_equals_each_replicas_own_solve():
    from cacto_amd.environment import make_env
    from cacto_amd.neural_network import NN
    from cacto_amd.replay_buffer import ReplayBuffer
    from cacto_amd.rl import RL_AC, Ensemble
    from cacto_amd.to import TO
    conf = _conf()
    env = make_env(conf)
    TrOp = TO(env, conf, W_S)
    random.seed(5)
    ics = [[env.reset() for _ in range(5)], [env.reset() for _ in range(7)]]   # different counts and horizons

    def learners():
        out = []
        for s in SEEDS:
            rl = RL_AC(env, NN(env, conf, W_S, seed=s), conf)
            rl.setup_model()
            out.append(rl)
        return out
    COUNTERS = ("rows", "n_kept", "zero_length", "nan_rollouts", "converged", "maxiter", "failed")
    for ep in (0, 1):                    # zero warm start, then the replica's own actor's roll-out
        solo_rl, solo_buf = learners(), [ReplayBuffer(conf) for _ in SEEDS]
        solo = [rl.compute_samples(ep, ics[r], TrOp, solo_buf[r], cfg=TO_CFG, accept_maxiter=True)
                for r, rl in enumerate(solo_rl)]
        assert all(s["n_kept"] >= 1 for s in solo)
        ens, bufs = Ensemble(learners()), [ReplayBuffer(conf) for _ in SEEDS]
        got = ens.compute_samples(ep, ics, TrOp, bufs, cfg=TO_CFG, accept_maxiter=True)
        torch.cuda.synchronize()
        for r in range(2):
            g, s = got[r], solo[r]
            np.testing.assert_array_equal(g["kept"], s["kept"])
            assert [g[k] for k in COUNTERS] == [s[k] for k in COUNTERS]
            np.testing.assert_array_equal(g["ep_return"], s["ep_return"])
            assert torch.equal(bufs[r].storage, solo_buf[r].storage) and bufs[r].next_idx == solo_buf[r].next_idx
            for name in ("status", "iters", "S", "U", "step_cost", "dVdx", "EE_TO"):
                assert torch.equal(g["dev"][name], s["dev"][name]), (ep, r, name)
