"""Ensemble.update_rows_n (cacto_ensemble_update): the paired update loop of R independent learners
as one chain launch and one GEMM + Adam launch per step. The reference of every comparison is
RL_AC.update_rows_n on a solo learner with the same initial weights, storage and indices; every
comparison is torch.equal, nothing looser: actor, critic, target, both moment pairs, both step
counters, y and V of each replica.

Shapes: B = 4 is one 4-sample tile; B = 20 pads to Bp = 32 (8 tiles, 12 padded rows); K = 1 has no
paired step (the lone critic step and the lone actor step only), K = 3 has two; R = 1, 2, 3 with
pair_xcds = 1 or 2 puts the replicas on different XCD groups. The double integrator (NJ = 2) and the
manipulator (NJ = 3) take different actor chain instances; w_S = 0 drops the Sobolev half."""
import ctypes as C

import numpy as np
import pytest
import torch

from cacto_amd import _lib as L
from cacto_amd.confs import load_conf
from elu_cases import make_rows

pytestmark = pytest.mark.gpu
N_ROWS = 96


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _conf(system, **over):
    conf = load_conf(system, fresh=True)
    for k, v in over.items():
        setattr(conf, k, v)
    return conf


def _learner(env, conf, w_S, seed):
    from cacto_amd.neural_network import NN
    from cacto_amd.rl import RL_AC
    rl = RL_AC(env, NN(env, conf, w_S, seed=seed), conf)
    rl.setup_model()                         # fresh initialisers: different weights per seed
    return rl


def _inputs(conf, seed, K, B):
    """A replica's storage and indices: its own rows and its own draws."""
    rng = np.random.default_rng(1000 + seed)
    storage = torch.as_tensor(make_rows(conf, N_ROWS, rng), device="cuda")
    idx = torch.as_tensor(rng.integers(0, N_ROWS, size=(K, B)).astype(np.int32), device="cuda")
    return storage, idx


def _yv(rl, B):
    """y and V of a solo learner's last critic step (inside its workspace)."""
    off = L.lib().raw("cacto_workspace_yv_offset")(rl.sys.handle, B) // 4
    assert off > 0
    Bp = (B + 15) // 16 * 16
    ws = rl.workspace(B)
    return ws[off:off + B].clone(), ws[off + Bp:off + Bp + B].clone()


NAMES = ("actor", "critic", "target", "actor_m", "actor_v", "critic_m", "critic_v", "steps")


def _state(rl):
    return [t.clone() for t in (rl.actor_model.buf, rl.critic_model.buf, rl.target_critic.buf, rl.actor_m,
                                rl.actor_v, rl.critic_m, rl.critic_v, rl.steps)]


def _assert_same(got, ref, tag):
    for name, a, b in zip(NAMES, got, ref):
        assert torch.equal(a, b), (tag, name)


def _solo(env, conf, w_S, seed, K, B, steps0=0):
    rl = _learner(env, conf, w_S, seed)
    if steps0:
        rl.steps.fill_(steps0)
    storage, idx = _inputs(conf, seed, K, B)
    rl.update_rows_n(storage, idx)
    torch.cuda.synchronize()
    return _state(rl) + list(_yv(rl, B))


def _ensemble(env, conf, w_S, seeds, K, B, steps0=None):
    from cacto_amd.rl import Ensemble
    learners = [_learner(env, conf, w_S, s) for s in seeds]
    for rl, s0 in zip(learners, steps0 or []):
        if s0:
            rl.steps.fill_(s0)
    ins = [_inputs(conf, s, K, B) for s in seeds]
    ens = Ensemble(learners)
    return ens, [s for s, _ in ins], torch.stack([i for _, i in ins]).contiguous()


def _ens_states(ens, B):
    torch.cuda.synchronize()
    return [_state(rl) + list(ens.outputs(r, B)) for r, rl in enumerate(ens.learners)]


# ---------------------------------------------------------------------- 1. small shapes
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("B", [4, 20])
@pytest.mark.parametrize("w_S", [0.0, 1e-2])
@pytest.mark.parametrize("system", ["double_integrator", "manipulator"])
def test_every_replica_equals_its_solo_run(system, w_S, B, K):
    from cacto_amd.environment import make_env
    conf = _conf(system, BATCH_SIZE=B)
    env = make_env(conf)
    solo = {s: _solo(env, conf, w_S, s, K, B) for s in (0, 1, 2)}
    assert not torch.equal(solo[0][1], solo[1][1]) and not torch.equal(solo[1][1], solo[2][1])
    assert int(solo[0][7][0]) == K and int(solo[0][7][1]) == K
    for R in (1, 2, 3):
        ens, storages, idx = _ensemble(env, conf, w_S, range(R), K, B)
        plan = ens.plan(B)
        assert plan["supported"] == 1 and plan["R"] == R and plan["launches_per_update"] == 2
        one = ens.learners[0].update_plan(B)         # the one-learner route of this handle
        assert one["paired"] == 1 and one["chain_tile"] == 4
        assert (plan["Bp"], plan["pair_xcds"], plan["cus"]) == (one["Bp"], one["pair_xcds"], one["cus"])
        ens.update_rows_n(storages, idx)
        got = _ens_states(ens, B)
        for r in range(R):
            _assert_same(got[r], solo[r], (system, w_S, B, K, R, r))
            assert torch.equal(got[r][8], solo[r][8]), ("y", R, r)
            assert torch.equal(got[r][9], solo[r][9]), ("V", R, r)
        ens.close()


@pytest.mark.parametrize("B,R", [(20, 5), (64, 3), (128, 2)])
def test_replicas_stacked_in_layers_equal_their_solo_runs(B, R):
    """More replicas than XCD groups: the deal stacks them in layers (B = 20: 4 groups of 2 XCDs,
    B = 64: 2 groups of 4, B = 128: 1 group of 8 — the reference's batches)."""
    from cacto_amd.environment import make_env
    conf = _conf("double_integrator", BATCH_SIZE=B)
    env = make_env(conf)
    K, w_S = 2, 1e-2
    ens, storages, idx = _ensemble(env, conf, w_S, range(R), K, B)
    plan = ens.plan(B)
    assert plan["layers"] >= 2 and plan["xcd_groups"] < R
    ens.update_rows_n(storages, idx)
    got = _ens_states(ens, B)
    for r in range(R):
        solo = _solo(env, conf, w_S, r, K, B)
        _assert_same(got[r], solo, (B, R, r))
        assert torch.equal(got[r][8], solo[8]) and torch.equal(got[r][9], solo[9])


# ---------------------------------------------------------------------- 2. replica order
def test_results_follow_the_replica_not_the_slot():
    from cacto_amd.environment import make_env
    conf = _conf("double_integrator", BATCH_SIZE=20)
    env = make_env(conf)
    K, B, w_S = 3, 20, 1e-2
    ens, storages, idx = _ensemble(env, conf, w_S, (0, 1, 2), K, B)
    ens.update_rows_n(storages, idx)
    a = _ens_states(ens, B)
    perm = (2, 0, 1)
    ens2, storages2, idx2 = _ensemble(env, conf, w_S, perm, K, B)
    ens2.update_rows_n(storages2, idx2)
    b = _ens_states(ens2, B)
    for slot, seed in enumerate(perm):
        _assert_same(b[slot], a[seed], (slot, seed))
        assert torch.equal(b[slot][8], a[seed][8]) and torch.equal(b[slot][9], a[seed][9])
    # the replicas' final critics differ from one another, so a mix-up cannot hide
    for i in range(3):
        for j in range(i + 1, 3):
            assert not torch.equal(a[i][1], a[j][1]), (i, j)
            assert not torch.equal(a[i][0], a[j][0]), (i, j)


# ---------------------------------------------------------------------- 3. LR schedule
def test_each_replica_reads_its_own_iteration_counters_for_the_lr_schedule():
    from cacto_amd.environment import make_env
    bounds = [10, 20, 30, 40]
    conf = _conf("double_integrator", BATCH_SIZE=20, LR_SCHEDULE=1, boundaries_schedule_LR_C=bounds,
                 boundaries_schedule_LR_A=bounds)
    assert conf.values_schedule_LR_C[0] != conf.values_schedule_LR_C[1]
    env = make_env(conf)
    K, B, w_S = 4, 20, 1e-2
    steps0 = [0, 8, 0]                       # replica 1 crosses the boundary at 10 inside the call
    solo = [_solo(env, conf, w_S, s, K, B, steps0=s0) for s, s0 in zip(range(3), steps0)]
    # the boundary matters: the same replica started at 0 ends elsewhere
    assert not torch.equal(solo[1][1], _solo(env, conf, w_S, 1, K, B)[1])
    ens, storages, idx = _ensemble(env, conf, w_S, range(3), K, B, steps0=steps0)
    ens.update_rows_n(storages, idx)
    got = _ens_states(ens, B)
    for r in range(3):
        _assert_same(got[r], solo[r], r)
    assert [int(g[7][0]) for g in got] == [4, 12, 4]


# ---------------------------------------------------------------------- 4. call pattern
def test_two_calls_equal_one_and_a_replayed_graph_equals_eager_calls():
    from cacto_amd.environment import make_env
    conf = _conf("manipulator", BATCH_SIZE=20)
    env = make_env(conf)
    K, B, w_S, seeds = 3, 20, 1e-2, (0, 1)
    one, st1, idx = _ensemble(env, conf, w_S, seeds, 2 * K, B)
    one.update_rows_n(st1, idx)
    ref = _ens_states(one, B)
    two, st2, _ = _ensemble(env, conf, w_S, seeds, 2 * K, B)
    two.update_rows_n(st2, idx[:, :K].contiguous())
    two.update_rows_n(st2, idx[:, K:].contiguous())
    got = _ens_states(two, B)
    for r in range(2):
        _assert_same(got[r], ref[r], ("two calls", r))
        assert torch.equal(got[r][8], ref[r][8]) and torch.equal(got[r][9], ref[r][9])

    # a captured call replayed twice == the same call issued twice
    first = idx[:, :K].contiguous()
    eager, st3, _ = _ensemble(env, conf, w_S, seeds, 2 * K, B)
    eager.update_rows_n(st3, first)
    eager.update_rows_n(st3, first)
    want = _ens_states(eager, B)
    graphed, st4, _ = _ensemble(env, conf, w_S, seeds, 2 * K, B)
    graphed.update_rows_n(st4, first[:, :0].contiguous())        # K = 0: creates the handle, runs nothing
    before = _ens_states(graphed, B)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.update_rows_n(st4, first)
    torch.cuda.synchronize()
    for r in range(2):                                           # the capture ran nothing
        _assert_same(_ens_states(graphed, B)[r], before[r], ("capture", r))
    g.replay()
    g.replay()
    got = _ens_states(graphed, B)
    for r in range(2):
        _assert_same(got[r], want[r], ("graph", r))
        assert torch.equal(got[r][8], want[r][8]) and torch.equal(got[r][9], want[r][9])
    assert not torch.equal(want[0][1], ref[0][1])


# ---------------------------------------------------------------------- 5. refusals
def _dp_handle_worker(port, q):
    """In a process of its own: a one-rank RCCL group attached to the system handle
    (set_data_parallel over backend 'nccl' runs cacto_dp_attach), then cacto_ensemble_create on that
    handle, called directly. Reports (return code, message, the handle it was given)."""
    import torch.distributed as dist
    from cacto_amd.environment import make_env
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1)
    try:
        R, B = 2, 20
        conf = _conf("double_integrator", BATCH_SIZE=B)
        env = make_env(conf)
        learners = [_learner(env, conf, 1e-2, s) for s in range(R)]
        storages = [_inputs(conf, s, 1, B)[0] for s in range(R)]
        nets = (L.Nets * R)(*[rl.nets for rl in learners])
        st = (C.c_void_p * R)(*[s.data_ptr() for s in storages])
        ws = [rl.workspace(B) for rl in learners]
        wp = (C.c_void_p * R)(*[w.data_ptr() for w in ws])
        cfg = learners[0]._cfg_for(B)
        args = (env.sys.handle, R, nets, st, wp, env.sys.workspace_bytes(B), C.byref(cfg), B)
        create = L.lib().raw("cacto_ensemble_create")
        # the same call is accepted before the communicators are attached ...
        h0 = C.c_void_p()
        rc0 = create(*args, C.byref(h0))
        ok0 = bool(h0.value)
        L.lib().raw("cacto_ensemble_destroy")(h0)
        # ... and refused after (the handle is shared by every learner of the Env)
        learners[0].set_data_parallel(1, dist.group.WORLD)
        native = learners[0]._dp_native
        h = C.c_void_p()
        rc = create(*args, C.byref(h))
        msg = L.lib().dll.cacto_last_error().decode()
        q.put((rc0, ok0, native, rc, msg, h.value))
    finally:
        dist.destroy_process_group()


def test_a_data_parallel_handle_is_refused_by_the_library():
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_dp_handle_worker, args=(port, q))
    p.start()
    try:
        rc0, ok0, native, rc, msg, handle = q.get(timeout=240)
    finally:
        p.join(timeout=60)
        if p.is_alive():
            p.kill()
    assert p.exitcode == 0
    assert rc0 == 0 and ok0
    assert native                                   # cacto_dp_attach ran on the handle
    assert rc == L.CACTO_EINVAL == -1 and not handle
    assert "the handle is data parallel (cacto_dp_attach)" in msg


def test_refusals():
    from cacto_amd.environment import make_env
    from cacto_amd.replay_buffer import PrioritizedReplayBuffer
    from cacto_amd.rl import Ensemble
    conf = _conf("double_integrator", BATCH_SIZE=20)
    env = make_env(conf)
    ens, storages, idx = _ensemble(env, conf, 1e-2, (0, 1), 1, 20)
    # a batch with 2 Bp > 1024
    big = torch.zeros(2, 1, 520, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="not paired"):
        ens.update_rows_n(storages, big)
    with pytest.raises(ValueError, match="not paired"):
        ens.plan(520)
    with pytest.raises(ValueError, match="R = 2"):
        ens.update_rows_n(storages, idx[:1])
    # a workspace that is too small, at the C boundary
    R, B = 2, 20
    nets = (L.Nets * R)(*[rl.nets for rl in ens.learners])
    st = (C.c_void_p * R)(*[s.data_ptr() for s in storages])
    ws = [rl.workspace(B) for rl in ens.learners]
    wp = (C.c_void_p * R)(*[w.data_ptr() for w in ws])
    cfg = ens.learners[0]._cfg_for(B)
    need = env.sys.workspace_bytes(B)
    h = C.c_void_p()
    with pytest.raises(RuntimeError, match=r"\(-1\).*workspace too small"):
        L.lib().call("cacto_ensemble_create", env.sys.handle, R, nets, st, wp, need - 4, C.byref(cfg), B, C.byref(h))
    with pytest.raises(RuntimeError, match=r"\(-4\).*not paired"):
        L.lib().call("cacto_ensemble_create", env.sys.handle, R, nets, st, wp, need, C.byref(cfg), 520, C.byref(h))
    with pytest.raises(RuntimeError, match=r"\(-1\).*CACTO_ENSEMBLE_MAX"):
        L.lib().call("cacto_ensemble_create", env.sys.handle, 0, nets, st, wp, need, C.byref(cfg), B, C.byref(h))
    assert not h.value
    # data parallel, PER, ReLO: the Python layer
    ens.learners[1].set_data_parallel(2)
    with pytest.raises(ValueError, match="data-parallel"):
        ens.update_rows_n(storages, idx)
    ens.learners[1].set_data_parallel(1)
    pconf = _conf("double_integrator", BATCH_SIZE=20, prioritized_replay_alpha=0.6, UPDATE_LOOPS=np.array([2]))
    for rb_type, word in (("PER", "PER"), ("ReLO", "ReLO")):
        pconf.RB_type = rb_type
        bufs = [PrioritizedReplayBuffer(pconf, env.sys) for _ in range(2)]
        with pytest.raises(ValueError, match=word + " replay buffers"):
            ens.learn_and_update(0, bufs, 0)
    # the elu critic
    econf = _conf("double_integrator", BATCH_SIZE=20, critic_type="elu")
    eenv = make_env(econf)
    elu = Ensemble([_learner(eenv, econf, 1e-2, s) for s in (0, 1)])
    with pytest.raises(ValueError, match="elu critic"):
        elu.update_rows_n(storages, idx)
