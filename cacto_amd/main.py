"""The CACTO training loop (main.py:145-165, :216-262, :276) on the device, with the reference's
evaluation stage (main.py:168, :249-252, :273, :279) as an option.

    python -m cacto_amd.main --system-id double_integrator --w-S 1e-2 [--plots]
    python -m cacto_amd.main --system-id double_integrator --w-S 1e-2 --seeds 0,1,2   # train_ensemble
    python -m cacto_amd.main --system-id double_integrator --w-S 1e-2 --validate [--validate-csv FILE]

Per loop: EP_UPDATE initial states from Env.reset (the host's `random`, as the reference), one
RL_AC.compute_samples (roll-outs -> batched TO -> filter -> labels -> RL_Solve + ring write, all on
the device), one RL_AC.learn_and_update. No CasADi, no per-episode host work.

With --plots (train(evaluate=True)) the loop also runs what the reference's main.py draws, through
cacto_amd.plot_utils.PLOT: the TO trajectories from conf.init_states_sim with a zero warm start
before the first loop, after every learn_and_update the critic over a planar grid and the same TO
trajectories warm-started by the actor, at the end the return history and the final policy's
roll-outs. The stage consumes the host random numbers the reference's consumes (manipulator: 3,721
Env.reset per loop; car: 961 np.random.uniform per loop), so only a run with it sees the reference's
initial states on those systems. It is off by default: its TO solves over the full NSTEPS cost
about a second per loop and each figure 0.07-0.08 s ("The evaluation stage");
--eval-every K runs it in every K-th loop only.

With --validate (train(validate=True)) every loop also compares the critic and the actor with the
loop's TO trajectories before they are trained on (RL_AC.validate_samples: their initial states were
drawn for this loop, so it is a held-out test) and logs one line; --validate-csv FILE writes the
numbers, one row per loop (per seed and loop with --seeds). The stage draws no host random number and
changes nothing that is trained; it is off by default ("The validation stage").
"""
import argparse
import csv
import os
import random

import numpy as np

from .confs import SYSTEM_MAP, load_conf


def parse_args(argv=None):
    """The reference's options (main.py:18-46) that have a meaning here, plus --nb-loops (stop after
    that many loops), --to-path (which kernels solve the TO batch, cacto_amd.to.PATHS) and
    --accept-maxiter (keep episodes whose solve stopped at max_iter). --to-hessian (the node Hessian
    of the TO's backward pass, cacto_amd.to.HESSIANS; exact when absent), --to-bounds (hard control
    limits of the TO, the conf's u_min / u_max; none when absent), --to-labels (the Sobolev labels
    after a solve, cacto_amd.to.LABELS; bounded needs --to-bounds conf; reference when absent), --to-starts,
    --to-start-sigma and --to-start-hold (several warm starts per TO episode, the cfg keys `starts`,
    `start_sigma`, `start_hold`; one start when absent), --plots, --fig-path and
    --eval-every (the evaluation stage) and --seeds (several seeds at once, train_ensemble; not with
    --seed or --plots), --validate and --validate-csv (the validation stage; allowed with --seeds) are
    in the dict only when they are given. Returns a dict."""
    p = argparse.ArgumentParser(prog="python -m cacto_amd.main", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--test-n", type=int, default=0, help="Test number")
    seed_given = []

    class _Seed(argparse.Action):
        def __call__(self, parser, namespace, values, option_string=None):
            setattr(namespace, self.dest, values)
            seed_given.append(option_string)

    def _seed_list(text):
        try:
            out = [int(s) for s in text.split(",")]
        except ValueError:
            raise argparse.ArgumentTypeError("a comma-separated list of integers, e.g. 0,1,2")
        if len(set(out)) != len(out):
            raise argparse.ArgumentTypeError("the seeds must differ")
        return out
    p.add_argument("--seed", type=int, default=0, action=_Seed, help="random and numpy.random seed")
    p.add_argument("--seeds", type=_seed_list, default=argparse.SUPPRESS,
                   help="Train these seeds at once on one GPU (train_ensemble), e.g. 0,1,2: seed k runs as N_try "
                        "test-n + k's position; not with --seed or --plots")
    p.add_argument("--system-id", type=str, default="single_integrator", choices=sorted(SYSTEM_MAP),
                   help="System-id")
    p.add_argument("--recover-training-flag", action="store_true", help="Flag to recover training")
    p.add_argument("--w-S", type=float, default=0, help="Sobolev training - weight of the value related error")
    p.add_argument("--nb-loops", type=int, default=None, help="Stop after this many loops (default: conf.NLOOPS)")
    p.add_argument("--to-path", type=str, default="default", choices=["default", "wave"],
                   help="Kernels of the batched trajectory optimiser")
    p.add_argument("--accept-maxiter", action="store_true",
                   help="Keep episodes whose TO solve stopped at max_iter without converging")
    p.add_argument("--to-hessian", type=str, default=argparse.SUPPRESS, choices=["exact", "psd"],
                   help="Node Hessian of the trajectory optimiser's backward pass: the cost's own, or its "
                        "projection onto the positive semidefinite cone (default: exact)")
    p.add_argument("--to-bounds", type=str, default=argparse.SUPPRESS, choices=["none", "conf"],
                   help="Hard control limits of the trajectory optimiser: none (the reference's penalty alone), or "
                        "the conf's u_min / u_max enforced by control-limited DDP (default: none)")
    p.add_argument("--to-labels", type=str, default=argparse.SUPPRESS, choices=["reference", "bounded"],
                   help="Sobolev labels after a TO solve: the reference's unconstrained dV/dx, or with --to-bounds conf "
                        "the recursion that leaves the controls a limit holds out (default: reference)")
    p.add_argument("--to-starts", type=int, default=argparse.SUPPRESS,
                   help="Solve every TO episode from this many warm starts (1..16) in one solve and keep the best: "
                        "the actor's roll-out, zero controls, and perturbed roll-outs (default: 1, one solve)")
    p.add_argument("--to-start-sigma", type=float, default=argparse.SUPPRESS,
                   help="With --to-starts: size of the perturbations, as a fraction of half the control range "
                        "(default: cacto_amd.to.DEFAULT_CFG, an unmeasured working value)")
    p.add_argument("--to-start-hold", type=int, default=argparse.SUPPRESS,
                   help="With --to-starts: steps over which a perturbation stays constant (default: "
                        "cacto_amd.to.DEFAULT_CFG, an unmeasured working value)")
    p.add_argument("--plots", action="store_true", default=argparse.SUPPRESS,
                   help="Run the evaluation stage: value grid, TO trajectories, return and roll-out figures")
    p.add_argument("--fig-path", type=str, default=argparse.SUPPRESS,
                   help="Where --plots writes (default: 'Results <system-id>/Figures')")
    p.add_argument("--eval-every", type=int, default=argparse.SUPPRESS,
                   help="With --plots: evaluate in every K-th loop only (default: 1)")
    p.add_argument("--validate", action="store_true", default=argparse.SUPPRESS,
                   help="Run the validation stage: critic and actor against each loop's fresh TO trajectories")
    p.add_argument("--validate-csv", type=str, default=argparse.SUPPRESS,
                   help="With --validate: write the validation numbers to this CSV file, one row per loop")
    args = vars(p.parse_args(argv))
    if "validate_csv" in args and not args.get("validate"):
        p.error("--validate-csv needs --validate")
    if args.get("to_labels") == "bounded" and args.get("to_bounds", "none") != "conf":
        p.error("--to-labels bounded needs --to-bounds conf: the labels take the bounds of the solve")
    from .to import make_starts
    try:
        make_starts({k: args[a] for k, a in (("starts", "to_starts"), ("start_sigma", "to_start_sigma"),
                                             ("start_hold", "to_start_hold")) if a in args})
    except ValueError as err:
        p.error(str(err))
    if "seeds" in args:
        if seed_given:
            p.error("--seed and --seeds exclude each other")
        if args.get("plots"):
            p.error("--plots is not available with --seeds: the evaluation stage draws host random numbers")
    return args


def train_kwargs(args):
    """parse_args' dict -> (system_id, keyword arguments of train)."""
    kw = dict(seed=args["seed"], N_try=args["test_n"], w_S=args["w_S"], to_cfg=dict(path=args["to_path"]),
              accept_maxiter=args["accept_maxiter"], n_loops=args["nb_loops"], recover=args["recover_training_flag"])
    if "to_hessian" in args:
        kw["to_cfg"]["hessian"] = args["to_hessian"]
    if "to_bounds" in args:
        kw["to_cfg"]["bounds"] = args["to_bounds"]
    if "to_labels" in args:
        kw["to_cfg"]["labels"] = args["to_labels"]
    for key, arg in (("starts", "to_starts"), ("start_sigma", "to_start_sigma"), ("start_hold", "to_start_hold")):
        if arg in args:
            kw["to_cfg"][key] = args[arg]
    if args.get("plots"):
        kw.update(evaluate=True, eval_every=args.get("eval_every", 1))
    if args.get("validate"):
        kw["validate"] = True
    return args["system_id"], kw


def validation_line(v, prefix=""):
    """One log line for a validation record (train's `validation` entries)."""
    fmt = lambda x: "-" if x is None else ("%.4g" % x if isinstance(x, float) else str(x))
    keys = ("rows", "value_rmse", "value_r2", "grad_rel", "sobolev_loss", "actor_rmse_u", "warm", "gap_mean",
            "gap_rel_median")
    return "{}Validation loop {} (updates {}): {}".format(prefix, v["ep"], v["update_step_counter"],
                                                         "  ".join("%s=%s" % (k, fmt(v[k])) for k in keys))


def multistart_line(m, prefix=""):
    """One log line for a loop's multi-start record (train's `multistart` entries)."""
    return "{}Multi-start loop {}: starts={}  rescued={}  improved={}  won_by={}  gain_rel_median={:.4g}".format(
        prefix, m["ep"], m["starts"], m["rescued"], m["improved"], m["won_by"], m["gain_rel_median"])


def write_validation_csv(path, outs, with_seed=False):
    """train's (or each of train_ensemble's) `validation` lists as one CSV: a row per loop, in the
    order of `outs`; with_seed: `seed` and `N_try` columns first. A None (no labels) is an empty cell."""
    from .rl import VALIDATION_KEYS
    cols = (["seed", "N_try"] if with_seed else []) + ["ep", "update_step_counter"] + list(VALIDATION_KEYS)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(cols)
        for o in outs:
            for v in o["validation"]:
                row = dict(v, seed=o.get("seed"), N_try=o.get("N_try"))
                w.writerow(["" if row[c] is None else row[c] for c in cols])


# main.py:249: these evaluate after every learn_and_update, UR5 only when the update counter hits
# conf.plot_rollout_interval_diff_loc
EVALUATED_EVERY_LOOP = ("single_integrator", "double_integrator", "car_park", "car", "manipulator")


def train(conf, seed=0, N_try=0, w_S=0.0, to_cfg=None, accept_maxiter=False, n_loops=None, weights=None,
          recover_training=None, log=print, evaluate=False, draw=True, eval_every=1, validate=False):
    """main.py:145-165, :216-262, :276. `to_cfg`: a dict over cacto_amd.to.DEFAULT_CFG; `weights`:
    setup_model's dict of initial weights; `recover_training`: (path, N_try, step) of checkpoints to
    start from (the update counter starts at step). A loop in which no episode is kept raises
    RuntimeError (the reference fails there too, on zip(*tmp)).

    `evaluate`: run the reference's evaluation stage (cacto_amd.plot_utils.PLOT) in the reference's
    order — traj_from_ICS(init=0) after the initial save (main.py:168); after each learn_and_update,
    in loops with ep % eval_every == 0 and under main.py:249's condition, the value grid (not for
    UR5) and traj_from_ICS(init=1); the return history after the loop (main.py:273); PLOT.rollout
    after the final save (main.py:279). Its TO solves use `to_cfg`. The figures are written below
    conf.Fig_path unless `draw` is false or Fig_path is unset; the data is computed either way.
    Without `evaluate` nothing of it runs and no random number is drawn for it.

    `validate`: run the validation stage in every loop (RL_AC.validate_samples, inside
    compute_samples, before the loop's rows are trained on) and log one line per loop. It reads the
    networks and writes nothing they or the replay buffer depend on, so the trained result is the
    same bits with and without it.

    `to_cfg["starts"]` > 1: every TO episode of a loop is solved from that many warm starts and the
    best is kept (RL_AC.compute_samples); the candidates' generator is keyed by `seed` and the loop
    index and draws no host random number. One log line per loop; `multistart` in the result is one
    rl.multistart_stats dict per loop with `ep` added, an empty list with one start.

    Returns dict(update_step_counter, ep_reward_arr, counts_per_loop, RLAC, buffer, evaluation,
    returns, evaluation_seconds, validation, multistart): validation is one validate_samples dict per loop with
    `ep` and `update_step_counter` (the counter before that loop's updates) added, an empty list
    without `validate`; evaluation is the stage's records in call order, each dict(kind
    ('traj' | 'value' | 'return' | 'rollout'), update_step_counter, ep (None outside the loop),
    data (the numbers behind the figure; for 'rollout' dict(returns, p_ee, states))); returns is
    PLOT.rollout's dict (None without evaluate); evaluation_seconds PLOT.seconds."""
    from .environment import make_env
    from .neural_network import NN
    from .plot_utils import PLOT
    from .replay_buffer import PrioritizedReplayBuffer, ReplayBuffer
    from .rl import RL_AC
    from .to import TO
    random.seed(seed)
    np.random.seed(seed)
    env = make_env(conf)
    NN_inst = NN(env, conf, w_S, seed=seed)
    TrOp = TO(env, conf, w_S)
    RLAC = RL_AC(env, NN_inst, conf, N_try)
    RLAC.start_seed = seed          # the multi-start candidates' stream (to_cfg["starts"] > 1) follows the run's seed
    buffer = ReplayBuffer(conf) if conf.prioritized_replay_alpha == 0 else PrioritizedReplayBuffer(conf)
    if getattr(conf, "NNs_path", None):
        os.makedirs(os.path.join(conf.NNs_path, "N_try_%s" % N_try), exist_ok=True)
    update_step_counter = 0
    if recover_training is not None:
        update_step_counter = int(recover_training[2])
    RLAC.setup_model(recover_training=recover_training, weights=weights)
    if getattr(conf, "NNs_path", None):
        RLAC.RL_save_weights(update_step_counter)
    evaluation = []
    if evaluate:
        plot_fun = PLOT(N_try, env, NN_inst, conf, learner=RLAC)
        plot_fun.draw = bool(draw)
        init_states_sim = np.array(conf.init_states_sim)

        def record(kind, ep, data):
            evaluation.append(dict(kind=kind, update_step_counter=update_step_counter, ep=ep, data=data))
        record("traj", None, plot_fun.plot_traj_from_ICS(init_states_sim, TrOp, RLAC, steps=conf.NSTEPS, init=0,
                                                         update_step_counter=update_step_counter, cfg=to_cfg, log=log))

    # NLOOPS and NEPISODES (conf_*.py) from the schedule itself, so a conf whose UPDATE_LOOPS or
    # EP_UPDATE was changed after import is read consistently
    n_sched = len(conf.UPDATE_LOOPS)
    loops = n_sched if n_loops is None else min(int(n_loops), n_sched)
    ep_arr_idx = 0
    ep_reward_arr = np.zeros(int(conf.EP_UPDATE) * n_sched) * np.nan
    counts_per_loop = []
    validation = []
    multistart = []
    val_kw = dict(validate=True) if validate else {}     # off: compute_samples is called as it always was
    for ep in range(loops):
        init_rand_state = [env.reset() for _ in range(conf.EP_UPDATE)]
        res = RLAC.compute_samples(ep, init_rand_state, TrOp, buffer, cfg=to_cfg, accept_maxiter=accept_maxiter,
                                   **val_kw)
        counts_per_loop.append({k: res[k] for k in ("rows", "n_kept", "zero_length", "nan_rollouts", "converged",
                                                    "maxiter", "failed")})
        n = res["n_kept"]
        if n == 0:
            raise RuntimeError("loop %d: no episode of %d was kept (%s)" % (ep, conf.EP_UPDATE, counts_per_loop[-1]))
        if "multistart" in res:
            multistart.append(dict(res["multistart"], ep=ep))
            log(multistart_line(multistart[-1]))
        if validate:
            validation.append(dict(res["validation"], ep=ep, update_step_counter=update_step_counter))
            log(validation_line(validation[-1]))
        update_step_counter = RLAC.learn_and_update(update_step_counter, buffer, ep)
        if evaluate and ep % eval_every == 0 and (update_step_counter % conf.plot_rollout_interval_diff_loc == 0
                                                  or conf.system_id in EVALUATED_EVERY_LOOP):
            log("System: {} - N_try = {}".format(conf.system_id, N_try))
            if conf.system_id != "ur5":     # the reference's value grid cannot run for UR5 (PLOT.compute_ICS)
                record("value", ep, plot_fun.plot_Critic_Value_function(RLAC.critic_model, update_step_counter,
                                                                        conf.system_id))
            record("traj", ep, plot_fun.plot_traj_from_ICS(init_states_sim, TrOp, RLAC, steps=conf.NSTEPS, init=1,
                                                           update_step_counter=update_step_counter, ep=ep, cfg=to_cfg,
                                                           log=log))
        ep_return = res["ep_return"]
        ep_reward_arr[ep_arr_idx:ep_arr_idx + n] = ep_return
        ep_arr_idx += n
        for i in range(n):
            log("Episode  {}  --->   Return = {}".format(ep * n + i, ep_return[i]))
        if hasattr(conf, "NUPDATES") and update_step_counter > conf.NUPDATES:
            break
    if evaluate:
        plot_fun.plot_Return(ep_reward_arr)
        record("return", None, ep_reward_arr.copy())
    if getattr(conf, "NNs_path", None):
        RLAC.RL_save_weights()
    returns = None
    if evaluate:
        returns = plot_fun.rollout(update_step_counter, RLAC.actor_model, conf.init_states_sim)
        record("rollout", None, dict(returns=returns, p_ee=np.array(plot_fun.p_ee_all_sim),
                                     states=np.array(plot_fun.states_all_sim)))
    return dict(update_step_counter=update_step_counter, ep_reward_arr=ep_reward_arr, counts_per_loop=counts_per_loop,
                RLAC=RLAC, buffer=buffer, evaluation=evaluation, returns=returns,
                evaluation_seconds=dict(plot_fun.seconds) if evaluate else None, validation=validation,
                multistart=multistart)


class HostRng:
    """One replica's copy of the two process-global generators train draws from — `random`
    (Env.reset) and `numpy.random` (ReplayBuffer.sample_indices) — seeded as train seeds them. Used
    as a context manager around that replica's host draws: the replica's states are swapped into the
    globals on entry and saved back on exit (the globals get their own state back), so the replica
    sees exactly the draws of its solo run whatever the other replicas draw in between."""

    def __init__(self, seed):
        keep = random.getstate(), np.random.get_state()
        random.seed(seed)
        np.random.seed(seed)
        self.state = random.getstate(), np.random.get_state()
        random.setstate(keep[0])
        np.random.set_state(keep[1])

    def __enter__(self):
        self._keep = random.getstate(), np.random.get_state()
        random.setstate(self.state[0])
        np.random.set_state(self.state[1])
        return self

    def __exit__(self, *exc):
        self.state = random.getstate(), np.random.get_state()
        random.setstate(self._keep[0])
        np.random.set_state(self._keep[1])
        return False


def train_ensemble(conf, seeds, N_try=0, w_S=0.0, to_cfg=None, accept_maxiter=False, n_loops=None, weights=None,
                   recover_training=None, log=print, validate=False):
    """train for every seed of `seeds` at once (the reference's ten-seed sets,
    generate_tests_set_script.py) in one process on one GPU: one Env, one TO, per seed an NN, an
    RL_AC (replica r runs as N_try + r) and a replay buffer; per loop one Ensemble.compute_samples
    (every replica's roll-outs, ONE TO solve over all their episodes) and one
    Ensemble.learn_and_update (one chain launch and one GEMM + Adam launch per step for all
    replicas). Each seed's networks, Adam state, replay buffer, counts and returns equal those of
    train(conf, seed=seed, N_try=N_try + r, ...), bit for bit: every replica has its own copy of the
    host generators (HostRng), swapped in around its draws in train's order.

    train's arguments without the evaluation stage (which draws host random numbers of its own);
    `validate` as train's, per replica with that replica's networks (it draws none).
    `weights`: one setup_model dict for all replicas, or a list of one per seed. `recover_training`:
    (path, N_try, step) as train's, read as the checkpoints of an earlier ensemble run: replica r
    starts from <path>/N_try_<N_try + r>/*_<step>.h5 — what train(seed, N_try=N_try + r,
    recover_training=(path, N_try + r, step)) loads — so N_try must be an integer; the update counter
    starts at step. Uniform replay, the
    paired small-batch route, one rank (Ensemble's ValueErrors otherwise). A loop in which some
    replica keeps no episode raises RuntimeError naming the seed. Returns one train-shaped dict per
    seed (evaluation fields empty), in the order of `seeds`."""
    from .environment import make_env
    from .neural_network import NN
    from .replay_buffer import ReplayBuffer
    from .rl import RL_AC, Ensemble
    from .to import TO
    seeds = [int(s) for s in seeds]
    if not seeds:
        raise ValueError("train_ensemble: no seeds")
    if conf.prioritized_replay_alpha != 0:
        raise ValueError("train_ensemble: PER replay buffers are not supported (uniform replay only); train those "
                         "seeds with train")
    R = len(seeds)
    rngs = [HostRng(s) for s in seeds]
    env = make_env(conf)
    TrOp = TO(env, conf, w_S)
    learners, buffers = [], []
    update_step_counter = int(recover_training[2]) if recover_training is not None else 0
    if recover_training is not None:
        try:
            n_try_rec = int(recover_training[1])
        except (TypeError, ValueError):
            raise ValueError("train_ensemble: recover_training = (path, N_try, step) needs an integer N_try: replica r "
                             "recovers from N_try + r, got %r" % (recover_training[1],))
    for r, seed in enumerate(seeds):
        with rngs[r]:
            rl = RL_AC(env, NN(env, conf, w_S, seed=seed), conf, N_try + r)
            rl.start_seed = seed    # as train sets it: the replica's multi-start stream is its solo run's
            buffers.append(ReplayBuffer(conf))
            if getattr(conf, "NNs_path", None):
                os.makedirs(os.path.join(conf.NNs_path, "N_try_%s" % (N_try + r)), exist_ok=True)
            rec = None if recover_training is None else (recover_training[0], n_try_rec + r, recover_training[2])
            rl.setup_model(recover_training=rec, weights=weights[r] if isinstance(weights, (list, tuple)) else weights)
            if getattr(conf, "NNs_path", None):
                rl.RL_save_weights(update_step_counter)
            learners.append(rl)
    ens = Ensemble(learners, host_rng=lambda r: rngs[r])
    ens.plan(conf.BATCH_SIZE)       # refuse an unsupported batch / critic before any work
    n_sched = len(conf.UPDATE_LOOPS)
    loops = n_sched if n_loops is None else min(int(n_loops), n_sched)
    ep_arr_idx = [0] * R
    ep_reward_arr = [np.zeros(int(conf.EP_UPDATE) * n_sched) * np.nan for _ in range(R)]
    counts_per_loop = [[] for _ in range(R)]
    validation = [[] for _ in range(R)]
    multistart = [[] for _ in range(R)]
    val_kw = dict(validate=True) if validate else {}
    for ep in range(loops):
        ics = []
        for r in range(R):
            with rngs[r]:
                ics.append([env.reset() for _ in range(conf.EP_UPDATE)])
        res = ens.compute_samples(ep, ics, TrOp, buffers, cfg=to_cfg, accept_maxiter=accept_maxiter,
                                  **val_kw)
        for r in range(R):
            counts_per_loop[r].append({k: res[r][k] for k in ("rows", "n_kept", "zero_length", "nan_rollouts",
                                                              "converged", "maxiter", "failed")})
        for r in range(R):
            if res[r]["n_kept"] == 0:
                raise RuntimeError("seed %d (N_try %d), loop %d: no episode of %d was kept (%s)"
                                   % (seeds[r], N_try + r, ep, conf.EP_UPDATE, counts_per_loop[r][-1]))
        for r in range(R):
            if "multistart" in res[r]:
                multistart[r].append(dict(res[r]["multistart"], ep=ep))
                log(multistart_line(multistart[r][-1], prefix="N_try {} ".format(N_try + r)))
        if validate:
            for r in range(R):
                validation[r].append(dict(res[r]["validation"], ep=ep, update_step_counter=update_step_counter))
                log(validation_line(validation[r][-1], prefix="N_try {} ".format(N_try + r)))
        update_step_counter = ens.learn_and_update(update_step_counter, buffers, ep)
        for r in range(R):
            n, ep_return = res[r]["n_kept"], res[r]["ep_return"]
            ep_reward_arr[r][ep_arr_idx[r]:ep_arr_idx[r] + n] = ep_return
            ep_arr_idx[r] += n
            for i in range(n):
                log("N_try {} Episode  {}  --->   Return = {}".format(N_try + r, ep * n + i, ep_return[i]))
        if hasattr(conf, "NUPDATES") and update_step_counter > conf.NUPDATES:
            break
    if getattr(conf, "NNs_path", None):
        for rl in learners:
            rl.RL_save_weights()
    ens.close()
    return [dict(update_step_counter=update_step_counter, ep_reward_arr=ep_reward_arr[r],
                 counts_per_loop=counts_per_loop[r], RLAC=learners[r], buffer=buffers[r], evaluation=[], returns=None,
                 evaluation_seconds=None, seed=seeds[r], N_try=N_try + r, validation=validation[r],
                 multistart=multistart[r])
            for r in range(R)]


def main(argv=None):
    args = parse_args(argv)
    system_id, kw = train_kwargs(args)
    conf = load_conf(system_id)
    if not getattr(conf, "NNs_path", None):
        conf.NNs_path = os.path.join(os.getcwd(), "Results " + system_id, "NNs")
    if args.get("seeds") is not None:
        kw.pop("seed")
        recover = None
        if kw.pop("recover"):
            recover = (conf.NNs_path_rec, conf.N_try_rec, conf.update_step_counter_rec)
        print("System: {} - N_try = {} .. {} (seeds {})".format(conf.system_id, kw["N_try"],
                                                                 kw["N_try"] + len(args["seeds"]) - 1, args["seeds"]))
        outs = train_ensemble(conf, args["seeds"], recover_training=recover, log=print, **kw)
        for o in outs:
            print("seed {} (N_try {}): updates {}  kept per loop: {}".format(
                o["seed"], o["N_try"], o["update_step_counter"], [c["n_kept"] for c in o["counts_per_loop"]]))
        if "validate_csv" in args:
            write_validation_csv(args["validate_csv"], outs, with_seed=True)
        return outs
    if kw.get("evaluate") and (args.get("fig_path") or not getattr(conf, "Fig_path", None)):
        conf.Fig_path = args.get("fig_path") or os.path.join(os.getcwd(), "Results " + system_id, "Figures")
    recover = None
    if kw.pop("recover"):
        recover = (conf.NNs_path_rec, conf.N_try_rec, conf.update_step_counter_rec)
    log = print
    log("System: {} - N_try = {}".format(conf.system_id, kw["N_try"]))
    out = train(conf, recover_training=recover, log=log, **kw)
    log("Updates: {}  kept per loop: {}".format(out["update_step_counter"],
                                                [c["n_kept"] for c in out["counts_per_loop"]]))
    if out["evaluation_seconds"] is not None:
        log("Evaluation: {} records, seconds {}{}".format(
            len(out["evaluation"]), {k: round(v, 3) for k, v in out["evaluation_seconds"].items()},
            "  figures in " + os.path.join(conf.Fig_path, "N_try_%s" % kw["N_try"]) if conf.Fig_path else ""))
    if "validate_csv" in args:
        write_validation_csv(args["validate_csv"], [out])
    return out


if __name__ == "__main__":
    main()
