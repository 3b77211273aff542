"""critic_type 'elu' (NeuralNetwork.py:65-78: Dense 16, 32, 256, 256 with elu, then Dense 1) on the
default library: forward, NN.eval and dV/ds, the Sobolev critic gradient, the actor gradient against
the elu critic, every update loop (pipelined == sequential bit for bit), a three-update trajectory
against the oracle's Adam + soft update, the handle rules and the .h5 checkpoints.

The oracle is oracle/nn.py with acts = ('elu',) * 4 (pinned at these widths by finite differences in
test_elu_critic_cpu.py). Every gradient case first asserts, on the CPU, the input condition of
elu_cases.check_preacts (both signs in every hidden layer, nothing within 1e-5 of the elu kink).

Tolerances: the project's (tests/test_gpu_sine_elu.py): V within 1e-5 of max(1, |V|max), dV/ds rel-L2
< 2e-5, gradient tensors rel-L2 < 2e-4; the trajectory |dw| < 5e-6 per Adam step
(tests/test_gpu_update_parity.py)."""
import gc

import numpy as np
import pytest
import torch

from elu_cases import ELU, check_preacts, make_rows, make_weights, rel_l2, split_rows
from oracle import env as oenv
from oracle import nn as onn
from cacto_amd.confs import load_conf

pytestmark = pytest.mark.gpu

V_TOL, DVDS_TOL, GRAD_TOL, STEP_TOL = 1e-5, 2e-5, 2e-4, 5e-6
# the weights' seed per system, and the rows' seed per case: the first from 100 on at which the oracle
# satisfies the input condition (elu_cases.check_preacts asserts it) with these weights
WSEED = {"single_integrator": 1, "double_integrator": 2, "manipulator": 3, "ur5": 4, "car_park": 5}
ROW_SEEDS = {("fwd", "single_integrator", 1): 100, ("fwd", "single_integrator", 16): 100,
             ("fwd", "single_integrator", 37): 101, ("fwd", "ur5", 1): 100, ("fwd", "ur5", 16): 101,
             ("fwd", "ur5", 37): 104, ("crit", "double_integrator", 5): 100, ("crit", "double_integrator", 16): 100,
             ("crit", "double_integrator", 40): 108, ("crit", "ur5", 5): 100, ("crit", "ur5", 16): 101,
             ("crit", "ur5", 40): 104, ("actor", "double_integrator", 40): 101, ("actor", "manipulator", 40): 101,
             ("actor", "ur5", 40): 103, ("actor", "car_park", 40): 100, ("traj", "double_integrator", 40): 551}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_LEARNERS = {}


def _learner(system, fresh=False, w_S=1e-2, critic_type="elu", weights="seeded"):
    """(conf, oracle env, RL_AC) with the elu critic and the seeded weights; one per system unless `fresh`."""
    from cacto_amd.environment import make_env
    from cacto_amd.neural_network import NN
    from cacto_amd.rl import RL_AC
    if not fresh and system in _LEARNERS:
        return _LEARNERS[system]
    conf = load_conf(system, fresh=True)
    conf.critic_type = critic_type
    env = make_env(conf)
    rl = RL_AC(env, NN(env, conf, w_S=w_S, seed=0), conf)
    rl.setup_model(weights=make_weights(conf, WSEED[system]) if weights == "seeded" else weights)
    out = (conf, oenv.make_env(conf), rl)
    if not fresh:
        _LEARNERS[system] = out
    return out


def _norm(conf):
    return conf.state_norm_arr.astype(np.float64)


def _v_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    return np.abs(np.asarray(got, dtype=np.float64).reshape(-1) - ref).max() / max(1.0, np.abs(ref).max())


# ------------------------------------------------------------------ forward, NN.eval, dV/ds
@pytest.mark.parametrize("B", [1, 16, 37])
@pytest.mark.parametrize("system", ["single_integrator", "ur5"])
def test_forward_and_input_grad(system, B):
    conf = load_conf(system, fresh=True)
    cw = make_weights(conf, WSEED[system])["critic"]
    ns = conf.nb_state
    S = make_rows(conf, B, np.random.default_rng(ROW_SEEDS["fwd", system, B]))[:, :ns].astype(np.float32)
    check_preacts(cw, S, _norm(conf))
    conf, _, rl = _learner(system)
    assert rl.sys.critic_type == "elu" and rl.critic_model.P == 16 * ns + 75057
    ref_V = onn.critic_forward(cw, S.astype(np.float64), _norm(conf), acts=ELU)
    ref_g, _ = onn.critic_input_grad(cw, S.astype(np.float64), _norm(conf), acts=ELU)
    V, g = rl.NN.critic_input_grad(rl.critic_model, S)
    Ve = rl.NN.eval(rl.critic_model, S)
    assert V.shape == (B, 1) and Ve.shape == (B, 1) and g.shape == (B, ns)
    print("V_err %.3g eval_err %.3g dVds_rel %.3g" % (_v_err(V.cpu().numpy(), ref_V), _v_err(Ve.cpu().numpy(), ref_V),
                                                     rel_l2(g.cpu().numpy(), ref_g)))
    assert _v_err(V.cpu().numpy(), ref_V) <= V_TOL and _v_err(Ve.cpu().numpy(), ref_V) <= V_TOL
    assert rel_l2(g.cpu().numpy(), ref_g) < DVDS_TOL


# ------------------------------------------------------------------ critic gradient
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("MC", [0, 1])
@pytest.mark.parametrize("w_S", [0.0, 1e-2])
@pytest.mark.parametrize("B", [5, 16, 40])
@pytest.mark.parametrize("system", ["double_integrator", "ur5"])
def test_critic_grad(system, B, w_S, MC, weighted):
    """B = 5: a partial tile; 16: exactly one; 40: several with a ragged tail."""
    conf, _, rl = _learner(system)
    cw, tw = rl.critic_model.get_weights(), rl.target_critic.get_weights()
    rng = np.random.default_rng(ROW_SEEDS["crit", system, B])
    rows = make_rows(conf, B, rng)
    w = rng.uniform(0.2, 1.0, size=B).astype(np.float32) if weighted else np.ones(B, dtype=np.float32)
    s, R, sn, dv, d, _ = split_rows(conf, rows)
    check_preacts(cw, s, _norm(conf))
    ref = onn.compute_critic_grad(cw, tw, s, sn, R, dv, d, w.astype(np.float64).reshape(B, 1), w_S, _norm(conf),
                                  MC=bool(MC), acts=ELU)
    old = (rl.cfg.w_S, rl.cfg.MC)
    rl.cfg.w_S, rl.cfg.MC = w_S, MC
    try:
        g, y, V, Vt = rl.critic_grad_rows(torch.as_tensor(rows, device="cuda"),
                                          torch.arange(B, dtype=torch.int32, device="cuda"),
                                          torch.as_tensor(w, device="cuda") if weighted else None, want_vt=True)
    finally:
        rl.cfg.w_S, rl.cfg.MC = old
    errs = [rel_l2(a.cpu().numpy(), b) for a, b in zip(g, ref[0])]
    print("critic grad rel-L2 per tensor:", " ".join("%.3g" % e for e in errs))
    print("y %.3g V %.3g Vt %.3g" % (_v_err(y.cpu().numpy(), ref[1]), _v_err(V.cpu().numpy(), ref[2]),
                                     _v_err(Vt.cpu().numpy(), ref[3])))
    for i, e in enumerate(errs):
        assert e < GRAD_TOL, (i, e)
    assert _v_err(y.cpu().numpy(), ref[1]) <= V_TOL
    assert _v_err(V.cpu().numpy(), ref[2]) <= V_TOL
    assert _v_err(Vt.cpu().numpy(), ref[3]) <= V_TOL


# ------------------------------------------------------------------ actor gradient against the elu critic
@pytest.mark.parametrize("system", ["double_integrator", "manipulator", "ur5", "car_park"])
def test_actor_grad(system):
    """One system per dynamics path of the actor chain (prismatic chain, planar 3R closed form, spread
    revolute chain, car_park)."""
    B = 40
    conf, oe, rl = _learner(system)
    cw, aw = rl.critic_model.get_weights(), rl.actor_model.get_weights()
    ns = conf.nb_state
    rows = make_rows(conf, B, np.random.default_rng(ROW_SEEDS["actor", system, B]))
    S32, term = rows[:, :ns].astype(np.float32), rows[:, 3 * ns + 2:3 * ns + 3]
    s_next = onn.actor_dq_da(oe, aw, cw, S32, term, _norm(conf), acts=ELU)[2]
    check_preacts(cw, s_next, _norm(conf))  # the critic pass of the actor chain is at s'
    ref = onn.compute_actor_grad(oe, aw, cw, S32, term, _norm(conf), acts=ELU)
    g = rl.actor_grad_rows(torch.as_tensor(rows, device="cuda"), torch.arange(B, dtype=torch.int32, device="cuda"))
    errs = [rel_l2(a.cpu().numpy(), b) for a, b in zip(g, ref)]
    print("actor grad rel-L2 per tensor:", " ".join("%.3g" % e for e in errs))
    for i, e in enumerate(errs):
        assert e < GRAD_TOL, (i, e)


# ------------------------------------------------------------------ loops, bit for bit
def _state(rl):
    return [t.cpu().numpy() for t in (rl.actor_model.buf, rl.critic_model.buf, rl.target_critic.buf, rl.actor_m,
                                      rl.actor_v, rl.critic_m, rl.critic_v, rl.steps)]


def _storage(conf, N, seed):
    rng = np.random.default_rng(seed)
    return rng, torch.as_tensor(make_rows(conf, N, rng), device="cuda")


@pytest.mark.parametrize("B", [64, 528])
def test_update_rows_n_equals_sequential(B):
    """B = 64: the fused small-batch pipeline (paired chain grid, fused GEMM + Adam); B = 528: the
    two-stream pipeline (2 Bp > 1024 rows: split-K slabs and k_adam)."""
    K = 4
    conf, _, seq = _learner("double_integrator", fresh=True)
    rng, storage = _storage(conf, 3000, 31)
    idx = torch.as_tensor(rng.integers(0, 3000, size=(K, B)).astype(np.int32), device="cuda")
    for k in range(K):
        seq.update_rows(storage, idx[k])
    _, _, pipe = _learner("double_integrator", fresh=True)
    pipe.update_rows_n(storage, idx)
    torch.cuda.synchronize()
    assert seq.steps.cpu().tolist() == [K, K]
    for a, b in zip(_state(seq), _state(pipe)):
        assert np.array_equal(a, b)
    assert not np.array_equal(_state(seq)[1], _state(_learner("double_integrator", fresh=True)[2])[1])


def test_update_rows_n_per_equals_sequential():
    from cacto_amd.replay_buffer import PrioritizedReplayBuffer
    K, B, N = 4, 64, 3000
    rows = make_rows(load_conf("double_integrator"), N, np.random.default_rng(32))
    U = torch.as_tensor(np.random.default_rng(33).uniform(size=(K, B)), device="cuda")

    def setup():
        conf = load_conf("double_integrator", fresh=True)
        conf.critic_type = "elu"
        conf.prioritized_replay_alpha = 0.6
        from cacto_amd.environment import make_env
        from cacto_amd.neural_network import NN
        from cacto_amd.rl import RL_AC
        env = make_env(conf)
        rl = RL_AC(env, NN(env, conf, w_S=1e-2, seed=0), conf)
        rl.setup_model(weights=make_weights(conf, WSEED["double_integrator"]))
        buf = PrioritizedReplayBuffer(conf, env.sys)
        buf.add_rows(rows)
        return rl, buf

    seq, sbuf = setup()
    y = torch.empty(B, dtype=torch.float32, device="cuda")
    V = torch.empty_like(y)
    for k in range(K):
        idx, w = sbuf.sample_device(U[k])
        seq.update_rows(sbuf.storage, idx, w, y, V)
        sbuf.update_priorities_device(idx, y, V)
    pipe, pbuf = setup()
    pipe.update_rows_n_per(pbuf, U)
    torch.cuda.synchronize()
    for a, b in zip(_state(seq), _state(pipe)):
        assert np.array_equal(a, b)
    for name in ("sum_tree", "min_tree", "exp_counter", "max_priority"):
        assert torch.equal(getattr(sbuf, name), getattr(pbuf, name)), name


def test_graph_replay_equals_eager():
    K, B = 4, 64
    conf, _, eager = _learner("double_integrator", fresh=True)
    rng, storage = _storage(conf, 3000, 34)
    idx = torch.as_tensor(rng.integers(0, 3000, size=(K, B)).astype(np.int32), device="cuda")
    for k in range(K):
        eager.update_rows(storage, idx[k])
    _, _, graphed = _learner("double_integrator", fresh=True)
    g = graphed.capture_updates(storage, idx)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(_state(eager), _state(graphed)):
        assert np.array_equal(a, b)


def test_one_rank_data_parallel_equals_update_rows_n(tmp_path, monkeypatch):
    """The exchange path at one rank over RCCL: the library's loop (cacto_update_n_dp) and the host
    loop on the staged pair calls (cacto_update_pair_grads_stage / _apply)."""
    import torch.distributed as dist
    K, B = 4, 64
    conf, _, single = _learner("double_integrator", fresh=True)
    rng, storage = _storage(conf, 3000, 35)
    idx = torch.as_tensor(rng.integers(0, 3000, size=(K, B)).astype(np.int32), device="cuda")
    single.update_rows_n(storage, idx)
    torch.cuda.synchronize()
    dist.init_process_group("nccl", init_method="file://" + str(tmp_path / "pg"), rank=0, world_size=1)
    try:
        _, _, native = _learner("double_integrator", fresh=True)
        native.set_data_parallel(1, dist.group.WORLD)
        assert native._dp_native
        native.update_rows_n(storage, idx)
        _, _, host = _learner("double_integrator", fresh=True)
        monkeypatch.setenv("CACTO_DP_NATIVE", "0")
        host.set_data_parallel(1, dist.group.WORLD)
        monkeypatch.delenv("CACTO_DP_NATIVE")
        assert not host._dp_native
        host.update_rows_n(storage, idx)
        torch.cuda.synchronize()
        for a, b, c in zip(_state(single), _state(native), _state(host)):
            assert np.array_equal(a, b) and np.array_equal(a, c)
    finally:
        dist.destroy_process_group()


def test_update_rows_returns_y_V_and_target_V():
    """The ReLO priority rule (cacto_per_update_relo) takes y, V and V_tgt(s) from the fused update
    (RL_AC._learn_and_update_relo): cacto_update's outputs with the elu critic against the oracle."""
    B = 40
    conf, _, rl = _learner("double_integrator", fresh=True)
    cw, tw = rl.critic_model.get_weights(), rl.target_critic.get_weights()
    rng = np.random.default_rng(ROW_SEEDS["crit", "double_integrator", B])
    rows = make_rows(conf, B, rng)
    w = rng.uniform(0.2, 1.0, size=B).astype(np.float32)
    s, R, sn, dv, d, _ = split_rows(conf, rows)
    ref = onn.compute_critic_grad(cw, tw, s, sn, R, dv, d, w.astype(np.float64).reshape(B, 1), 1e-2, _norm(conf),
                                  MC=bool(conf.MC), acts=ELU)
    y = torch.empty(B, dtype=torch.float32, device="cuda")
    V, Vt = torch.empty_like(y), torch.empty_like(y)
    rl.update_rows(torch.as_tensor(rows, device="cuda"), torch.arange(B, dtype=torch.int32, device="cuda"),
                   torch.as_tensor(w, device="cuda"), y, V, Vt)
    torch.cuda.synchronize()
    assert rl.steps.cpu().tolist() == [1, 1]
    for got, want in ((y, ref[1]), (V, ref[2]), (Vt, ref[3])):
        assert _v_err(got.cpu().numpy(), want) <= V_TOL


# ------------------------------------------------------------------ trajectory against the oracle
def test_three_updates_match_oracle():
    K, B, w_S = 3, 40, 1e-2
    conf, oe, rl = _learner("double_integrator", fresh=True)
    rng = np.random.default_rng(ROW_SEEDS["traj", "double_integrator", B])
    rows = make_rows(conf, 400, rng)
    idx = rng.integers(0, 400, size=(K, B))
    norm = _norm(conf)
    nets = (rl.critic_model.get_weights(), rl.target_critic.get_weights(), rl.actor_model.get_weights())
    opt = (onn.KerasAdam(conf.CRITIC_LEARNING_RATE), onn.KerasAdam(conf.ACTOR_LEARNING_RATE))
    for k in range(K):  # RL_AC.update + update_target (RL.py:101-118) in float64
        crit, tgt, act = nets
        s, R, sn, dv, d, term = split_rows(conf, rows[idx[k]])
        check_preacts(crit, s, norm)
        gc_ = onn.compute_critic_grad(crit, tgt, s, sn, R, dv, d, np.ones((B, 1)), w_S, norm, MC=bool(conf.MC),
                                      acts=ELU)[0]
        crit = opt[0].apply(crit, gc_)
        s_next = onn.actor_dq_da(oe, act, crit, s.astype(np.float32), term, norm, acts=ELU)[2]
        check_preacts(crit, s_next, norm)
        act = opt[1].apply(act, onn.compute_actor_grad(oe, act, crit, s.astype(np.float32), term, norm, acts=ELU))
        if not conf.MC:
            tgt = onn.soft_update(tgt, crit, conf.UPDATE_RATE)
        nets = (crit, tgt, act)
    storage = torch.as_tensor(rows, device="cuda")
    for k in range(K):
        rl.update_rows(storage, torch.as_tensor(idx[k].astype(np.int32), device="cuda"))
    torch.cuda.synchronize()
    got = (rl.critic_model.get_weights(), rl.target_critic.get_weights(), rl.actor_model.get_weights())
    worst = 0.0
    for name, g, ref in zip(("critic", "target", "actor"), got, nets):
        for i, (a, b) in enumerate(zip(g, ref)):
            err = np.abs(a - b).max()
            worst = max(worst, err)
            assert err < STEP_TOL * K, (name, i, err)
    print("trajectory max |dw| %.3g" % worst)


# ------------------------------------------------------------------ handle rules
def test_sine_critic_refused_while_elu_nets_live():
    conf, _, rl = _learner("double_integrator")
    with pytest.raises(ValueError):
        rl.NN.create_critic_sine()
    assert rl.sys.critic_type == "elu"


def test_relu_still_not_built():
    from cacto_amd.environment import make_env
    from cacto_amd.neural_network import NN
    from cacto_amd.rl import RL_AC
    conf = load_conf("double_integrator", fresh=True)
    conf.critic_type = "relu"
    env = make_env(conf)
    with pytest.raises(NotImplementedError):
        RL_AC(env, NN(env, conf, w_S=1e-2, seed=0), conf).setup_model()
    with pytest.raises(NotImplementedError):
        NN(env, conf).create_critic_relu()


def test_handle_switched_back_to_sine_equals_fresh_sine_handle():
    from conftest import load_weights
    from cacto_amd.environment import make_env
    from cacto_amd.neural_network import NN
    from cacto_amd.rl import RL_AC
    B = 16
    rows = torch.as_tensor(make_rows(load_conf("double_integrator"), B, np.random.default_rng(36)), device="cuda")
    idx = torch.arange(B, dtype=torch.int32, device="cuda")

    def sine_grad(conf, env):
        conf.critic_type = "sine"
        rl = RL_AC(env, NN(env, conf, w_S=1e-2, seed=0), conf)
        rl.setup_model(weights=load_weights("di_seed0_0"))
        assert rl.sys.critic_type == "sine" and rl.critic_model.P == 5 * 64 + 64 + 64 * 65 + 64 * 128 + 128 + 128 * 129 + 129
        g, y, V, Vt = rl.critic_grad_rows(rows, idx)
        return [t.cpu().numpy() for t in list(g) + [y, V, Vt]]

    conf = load_conf("double_integrator", fresh=True)
    conf.critic_type = "elu"
    env = make_env(conf)
    rl = RL_AC(env, NN(env, conf, w_S=1e-2, seed=0), conf)
    rl.setup_model(weights=make_weights(conf, WSEED["double_integrator"]))
    g_elu = rl.critic_grad_rows(rows, idx)[0]
    assert g_elu[0].shape == (conf.nb_state, 16)
    torch.cuda.synchronize()
    del rl, g_elu
    gc.collect()
    assert len(env.sys.critic_nets) == 0
    switched = sine_grad(conf, env)                       # the same handle, now sine
    conf2 = load_conf("double_integrator", fresh=True)
    fresh = sine_grad(conf2, make_env(conf2))
    assert env.sys is not None and len(switched) == len(fresh)
    for a, b in zip(switched, fresh):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ .h5
def test_h5_checkpoints_of_live_elu_nets(tmp_path):
    from cacto_amd import h5
    conf, _, rl = _learner("double_integrator")
    want = {"critic": ["dense_%d" % k for k in range(3, 8)], "target": ["dense_%d" % k for k in range(8, 13)]}
    for role, net in (("critic", rl.critic_model), ("target", rl.target_critic)):
        path = str(tmp_path / (role + ".h5"))
        net.save_weights(path)
        with open(path, "rb") as f:
            hf = h5.H5File(f.read())
        assert h5._strings(hf.attributes(hf.object(hf.root))["layer_names"]) == want[role]
        assert all(np.array_equal(a, b) for a, b in zip(h5.read_keras_weights(path), net.get_weights()))
        from cacto_amd.neural_network import CRITIC, Net
        back = Net(rl.sys, CRITIC, role=role)
        back.load_weights(path)
        assert torch.equal(back.buf, net.buf)
