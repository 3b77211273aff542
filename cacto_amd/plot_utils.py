"""PLOT — the evaluation stage of the reference's main.py (plot_utils.py:47-70, :111-158, :209-279,
:332-405, :545-611) in two halves.

The data half runs on the device, batched, and returns numpy; it needs no matplotlib:

  compute_ICS    plot_utils.py:111-158 on host scalars: the state behind a point of the plane
  value_grid     the numbers of plot_Critic_Value_function: the grid's states (for the manipulator
                 3,721 Env.reset states and their EE positions, one `cacto_env_ee`) and the critic
                 on all of them in ONE NN.eval (one `cacto_critic_forward`)
  traj_from_ICS  the numbers of plot_traj_from_ICS for every initial state at once: one
                 RL_AC.rollout_batch, one TO.solve_batch, two `cacto_env_ee`
  rollout        PLOT.rollout: the actor rolled out from every state of `init_states_sim` for the
                 full NSTEPS (no NSTEPS_SH shortening) with the running weights in one `cacto_rollout`
                 launch; returns the reference's `returns` dict {(x0, y0): episodic reward}. The
                 episodic reward is Python's left-to-right float sum of the per-step rewards, as
                 `rollout_episodic_reward += rwrd_sim` accumulates it. The EE trajectories keep the
                 reference's quirk `rollout_p_ee[i+1, -1] = rollout_states[i+1, 2]`
                 (plot_utils.py:265) and stay in `self.p_ee_all_sim`.

The number of library calls of each method does not depend on the number of grid points or initial
states. The stage draws the reference's host random numbers: per value grid 3,721 Env.reset calls
(CPython `random`) for the manipulator and 961 `np.random.uniform` for the car; nothing for the
other systems.

The drawing half is the module-level functions draw_value_grid, draw_traj, draw_return and
draw_policy_eval: pure functions of that data and the conf, which write the reference's figures as
PNG files under the reference's names below '<Fig_path>/N_try_<N_try>/'. They use matplotlib's
object API (a Figure with an Agg canvas, no pyplot, no rcParams, nothing global), import it when
called, and raise RuntimeError where it is missing. The reference-named methods of PLOT
(plot_Critic_Value_function, plot_traj_from_ICS, plot_Return, plot_policy_eval, plot_obstaces) are a
data call followed by a drawing call; they draw when `conf.Fig_path` is set and `self.draw` is true
and return the data either way.
"""
import math
import os
import time

import numpy as np

PLANAR_GRID = 30 + 1          # plot_utils.py:376-382: 31 x 31 points over [-15, 15]^2
MANIPULATOR_GRID = 60 + 1     # plot_utils.py:348-349: 61 x 61 Env.reset states


class PLOT:
    def __init__(self, N_try, env, NN, conf, learner=None):
        self.N_try = N_try
        self.env = env
        self.NN = NN
        self.conf = conf
        self.learner = learner            # the RL_AC that owns the device rollout (cacto_amd.rl)
        self.draw = True                  # False: the reference-named methods compute and do not draw
        self.p_ee_all_sim = []
        self.states_all_sim = []
        # wall-clock seconds spent per part of the stage (the data methods end with a copy to the
        # host, so the device work is inside)
        self.seconds = dict(value_grid=0.0, traj=0.0, rollout=0.0, draw=0.0)

    def _fig_path(self):
        return getattr(self.conf, "Fig_path", None) if self.draw else None

    def _timed(self, key, fn, *args, **kw):
        t0 = time.perf_counter()
        out = fn(*args, **kw)
        self.seconds[key] += time.perf_counter() - t0
        return out

    # ------------------------------------------------------------------ data
    def compute_ICS(self, p_ee, sys_id, theta=None, continue_flag=0):
        """plot_utils.py:111-158: (the state with zero velocities and time 0 the reference puts
        behind the point p_ee of the plane, continue_flag). For the manipulator the closed-form
        planar IK with conf.x_base, y_base and l, restated operation by operation (its c1 has a
        minus where a two-link IK has a plus, so the EE of the state is not at p_ee; kept, the
        values are compared bit for bit); (None, 1) outside radius 30 and where the third joint
        falls on the origin. For the car the heading
        is 0 * np.random.uniform(-pi, pi): the draw advances numpy's global generator, and the
        product may be -0.0. A system without a planar EE (ur5) raises ValueError (the reference
        leaves ICS unbound there)."""
        c = self.conf
        if sys_id == 'manipulator':
            dx, dy = p_ee[0] - c.x_base, p_ee[1] - c.y_base
            if math.sqrt(dx ** 2 + (p_ee[1]) ** 2) > 30:
                return None, 1
            phi = math.atan2(dy, dx)                      # the sum of the three angles
            x3 = dx - c.l * math.cos(phi)                 # the third joint
            y3 = dy - c.l * math.sin(phi)
            if abs(x3) <= 1e-6 and abs(y3) <= 1e-6:
                return None, 1
            c2 = (x3 ** 2 + y3 ** 2 - 2 * c.l ** 2) / (2 * c.l ** 2)
            s2 = math.sqrt(1 - c2 ** 2) if p_ee[1] >= 0 else -math.sqrt(1 - c2 ** 2)
            s1 = ((c.l + c.l * c2) * y3 - c.l * s2 * x3) / (x3 ** 2 + y3 ** 2)
            c1 = ((c.l + c.l * c2) * x3 - c.l * s2 * y3) / (x3 ** 2 + y3 ** 2)
            q0 = math.atan2(s1, c1)
            q1 = math.atan2(s2, c2)
            return np.array([q0, q1, phi - q0 - q1, 0.0, 0.0, 0.0, 0.0]), continue_flag
        if sys_id == 'car':
            if theta is None:
                theta = 0 * np.random.uniform(-math.pi, math.pi)
            return np.array([p_ee[0], p_ee[1], theta, 0.0, 0.0, 0.0]), continue_flag
        if sys_id == 'car_park':
            if theta is None:
                theta = np.pi / 2
            return np.array([p_ee[0], p_ee[1], theta, 0.0, 0.0, 0.0]), continue_flag
        if sys_id == 'double_integrator':
            return np.array([p_ee[0], p_ee[1], 0.0, 0.0, 0.0]), continue_flag
        if sys_id == 'single_integrator':
            return np.array([p_ee[0], p_ee[1], 0.0]), continue_flag
        raise ValueError("compute_ICS: system %r has no planar initial state" % (sys_id,))

    def _critic(self, critic_model, states):
        """The f32 critic outputs of one NN.eval over all rows, stored as float64."""
        return self.NN.eval(critic_model, states).reshape(-1).cpu().numpy().astype(np.float64)

    def _ee(self, states):
        """EE positions of the rows of `states` ([..., ns], host or device) in one cacto_env_ee."""
        import torch
        from . import _lib as L
        from .system import DEVICE, dptr, stream
        S = torch.as_tensor(states, dtype=torch.float64, device=DEVICE).contiguous()
        rows = S.numel() // S.shape[-1]
        EE = torch.empty(*S.shape[:-1], 3, dtype=torch.float64, device=DEVICE)
        L.lib().call("cacto_env_ee", self.env.sys.handle, dptr(S), dptr(EE), rows, stream())
        return EE.cpu().numpy()

    def value_grid(self, critic_model, sys_id=None):
        """The numbers of plot_Critic_Value_function (plot_utils.py:345-405).

        Manipulator: dict(ICS [3721, 7], ee [3721, 3], V [3721]) — 61 x 61 Env.reset states with the
        time set to 0, k_x outer and k_y inner, as the reference draws them from `random`.
        The other planar systems: dict(x [31], y [31], ICS [961, ns], V [31, 31]) — the states of
        compute_ICS([x[k_x], y[k_y], 0]) in the reference's order (k_y outer, k_x inner: row
        k_y * 31 + k_x), V[k_x, k_y] as the reference indexes it (it draws V.T), NaN where
        continue_flag was set. UR5 raises ValueError."""
        sys_id = self.conf.system_id if sys_id is None else sys_id
        if sys_id == 'ur5':
            raise ValueError("value_grid: system 'ur5' has no planar value function")
        if sys_id == 'manipulator':
            n = MANIPULATOR_GRID * MANIPULATOR_GRID
            ICS = np.empty((n, self.conf.nb_state))
            for k in range(n):
                ICS[k] = self.env.reset()
            ICS[:, -1] = 0
            return dict(ICS=ICS, ee=self._ee(ICS), V=self._critic(critic_model, ICS))
        x = np.linspace(-15, 15, PLANAR_GRID)
        y = np.linspace(-15, 15, PLANAR_GRID)
        ICS = np.full((PLANAR_GRID * PLANAR_GRID, self.conf.nb_state), np.nan)
        for k_y in range(PLANAR_GRID):
            for k_x in range(PLANAR_GRID):
                s, skip = self.compute_ICS(np.array([x[k_x], y[k_y], 0]), sys_id, continue_flag=0)
                if skip:
                    continue
                if len(s) != self.conf.nb_state:
                    raise ValueError("value_grid: a %r state has %d entries, the conf's system %d"
                                     % (sys_id, len(s), self.conf.nb_state))
                ICS[k_y * PLANAR_GRID + k_x] = s
        ok = ~np.isnan(ICS).any(axis=1)
        V = np.full(len(ICS), np.nan)
        if ok.any():
            V[ok] = self._critic(critic_model, ICS[ok])
        return dict(x=x, y=y, ICS=ICS, V=V.reshape(PLANAR_GRID, PLANAR_GRID).T.copy())

    def traj_from_ICS(self, init_state, TrOp, RLAC, init, steps, cfg=None, log=None):
        """The numbers of plot_traj_from_ICS (plot_utils.py:545-611) for all initial states at once.

        create_TO_init(init, s) for every state (one RLAC.rollout_batch over each episode's NSTEPS_SH:
        init = 0 zero controls, init = 1 the actor), TO_System_Solve over T = steps - 1 from the first T
        roll-out controls (one TrOp.solve_batch, `cfg` over cacto_amd.to.DEFAULT_CFG), the EE positions
        of the first `steps` warm-start states and of the TO states (one cacto_env_ee each).
        An episode with NSTEPS_SH == 0 or a NaN roll-out is skipped (success_init_flag == 0); a live
        episode with NSTEPS_SH < steps - 1 raises ValueError (the reference indexes past its arrays);
        a solve that does not succeed contributes its last iterate.

        Returns host arrays: dict(ok [n] bool, status [n] (-1 skipped), iters [n], J [n, 2] (warm
        start's cost, final cost), S_RL [n, steps, ns], U_RL [n, steps - 1, na], S_TO [n, steps, ns],
        U_TO [n, steps - 1, na], ee_RL [n, steps, 3], ee_TO [n, steps, 3]); the rows of a skipped
        episode are NaN. One line with the statuses, pass counts and costs goes to `log`."""
        import torch
        from .system import DEVICE
        S0 = np.asarray([np.asarray(s, dtype=np.float64) for s in init_state]).reshape(len(init_state), -1)
        n, T = len(S0), int(steps) - 1
        ns, na = self.conf.nb_state, self.conf.nb_action
        if T < 1:
            raise ValueError("traj_from_ICS: steps = %d leaves nothing to solve" % steps)
        nsh = np.array([RLAC.nsteps_sh(s) for s in S0], dtype=np.int32)
        nan = lambda *shape: np.full(shape, np.nan)
        res = dict(ok=np.zeros(n, dtype=bool), status=np.full(n, -1, dtype=np.int32), iters=np.zeros(n, dtype=np.int32),
                   J=nan(n, 2), S_RL=nan(n, T + 1, ns), U_RL=nan(n, T, na), S_TO=nan(n, T + 1, ns), U_TO=nan(n, T, na),
                   ee_RL=nan(n, T + 1, 3), ee_TO=nan(n, T + 1, 3))
        Tmax = int(nsh.max()) if n else 0
        if Tmax > 0:
            inputs = RLAC.rollout_inputs(S0, nsh)
            roll = RLAC.rollout_batch(S0, nsh, Tmax, ep=init, want=("S", "A"), inputs=inputs)
            live = (nsh > 0) & (roll["status"].cpu().numpy() == 0)
            short = live & (nsh < T)
            if short.any():
                k = int(np.nonzero(short)[0][0])
                raise ValueError("traj_from_ICS: episode %d has NSTEPS_SH = %d < steps - 1 = %d" % (k, nsh[k], T))
            if live.any():
                if init != 0:
                    warm = roll["A"][:, :T].double().contiguous()
                else:
                    warm = torch.zeros(n, T, na, dtype=torch.float64, device=DEVICE)
                S_RL = roll["S"][:, :T + 1].contiguous()
                Te = torch.as_tensor(np.where(live, T, -1).astype(np.int32), device=DEVICE)
                sol = TrOp.solve_batch(inputs[0], warm, Te, cfg=cfg)
                host = dict(S_RL=S_RL, U_RL=warm, S_TO=sol["S"], U_TO=sol["U"], J=sol["J"])
                host = {k: v.cpu().numpy() for k, v in host.items()}
                host["ee_RL"], host["ee_TO"] = self._ee(S_RL), self._ee(sol["S"])
                for k, v in host.items():
                    res[k][live] = v[live]
                res["ok"] = live
                res["status"] = np.where(live, sol["status"].cpu().numpy(), -1).astype(np.int32)
                res["iters"] = np.where(live, sol["iters"].cpu().numpy(), 0).astype(np.int32)
        if log is not None:
            log("TO from init_states_sim, init = {} ({} warm start): status {}  passes {}  J warm start {}  J {}".format(
                init, "actor" if init else "zero", res["status"].tolist(), res["iters"].tolist(),
                res["J"][:, 0].tolist(), res["J"][:, 1].tolist()))
        return res

    def rollout(self, update_step_cntr, actor_model, init_states_sim, diff_loc=0):
        """plot_utils.py:245-279."""
        if self.learner is None:
            raise RuntimeError("PLOT.rollout needs the RL_AC learner that runs cacto_rollout")
        t0 = time.perf_counter()
        S0 = np.asarray([np.asarray(s, dtype=np.float64) for s in init_states_sim])
        n = len(S0)
        T = int(self.conf.NSTEPS)
        out = self.learner.rollout_batch(S0, [T] * n, T, ep=1, weights=self.conf.cost_weights_running,
                                         want=("S", "R", "EE"), actor=actor_model)
        S = out["S"].cpu().numpy()
        R = out["R"].cpu().numpy()
        EE = out["EE"].cpu().numpy()
        returns = {}
        self.p_ee_all_sim, self.states_all_sim = [], []
        for k in range(n):
            p_ee = EE[k].copy()
            p_ee[1:, -1] = S[k, 1:, 2]                    # plot_utils.py:265
            ret = 0
            for r in R[k]:                                # plot_utils.py:267, Python float accumulation
                ret += float(r)
            if k == 0:
                print("N try = {}: Simulation Return @ N updates = {} ==> {}".format(self.N_try, update_step_cntr,
                                                                                    ret))
            self.p_ee_all_sim.append(p_ee)
            self.states_all_sim.append(S[k])
            returns[init_states_sim[k][0], init_states_sim[k][1]] = ret
        self.seconds["rollout"] += time.perf_counter() - t0
        if self._fig_path():                              # plot_utils.py:277
            self.plot_policy_eval(self.p_ee_all_sim, update_step_cntr, diff_loc=diff_loc)
        return returns

    # ------------------------------------------------------------------ the reference's figures
    def plot_obstaces(self, a=1):
        """plot_utils.py:47-70: the three obstacles as matplotlib patches."""
        return obstacle_patches(self.conf, a)

    def plot_Critic_Value_function(self, critic_model, n_update, sys_id, name='V'):
        data = self._timed("value_grid", self.value_grid, critic_model, sys_id)
        if self._fig_path():
            self._timed("draw", draw_value_grid, data, self.conf, self.N_try, n_update, self._fig_path(), name=name)
        return data

    def plot_traj_from_ICS(self, init_state, TrOp, RLAC, update_step_counter=0, ep=0, steps=200, init=0, cfg=None,
                           log=None):
        data = self._timed("traj", self.traj_from_ICS, init_state, TrOp, RLAC, init, steps, cfg=cfg, log=log)
        if self._fig_path():
            self._timed("draw", draw_traj, data, self.conf, self.N_try, init, update_step_counter, self._fig_path())
        return data

    def plot_Return(self, ep_reward_list):
        if self._fig_path():
            self._timed("draw", draw_return, ep_reward_list, self.conf, self.N_try, self._fig_path())

    def plot_policy_eval(self, p_list, n_updates, diff_loc=0, theta=0):
        if self._fig_path():
            self._timed("draw", draw_policy_eval, p_list, self.conf, self.N_try, n_updates, self._fig_path(),
                        diff_loc=diff_loc)


# ---------------------------------------------------------------------- drawing (numpy + conf only)
OBSTACLE_COLOUR = [30 / 255, 130 / 255, 76 / 255, 1]
TICK_SIZE, FONT_SIZE = 22, 20     # the reference's global rcParams, here set per figure


def _mpl():
    """matplotlib's object API, imported on first use; RuntimeError where it is missing."""
    try:
        import matplotlib.patches as patches
        import matplotlib.transforms as transforms
        from matplotlib import cm
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure
    except ImportError as e:
        raise RuntimeError("drawing the evaluation figures needs matplotlib, which cannot be imported (%s); "
                           "the data methods of PLOT run without it" % e) from e
    return Figure, FigureCanvasAgg, cm, patches, transforms


def _figure(figsize):
    Figure, FigureCanvasAgg = _mpl()[:2]
    fig = Figure(figsize=figsize)
    FigureCanvasAgg(fig)
    return fig


def _fonts(fig):
    for ax in fig.axes:
        ax.tick_params(labelsize=TICK_SIZE)
        for text in (ax.title, ax.xaxis.label, ax.yaxis.label):
            text.set_fontsize(FONT_SIZE)


def _save(fig, path, N_try, name):
    """'<path>/N_try_<N_try>/<name>.png' (the reference's savefig without a suffix writes PNG)."""
    folder = os.path.join(path, "N_try_{}".format(N_try))
    os.makedirs(folder, exist_ok=True)
    _fonts(fig)
    fname = os.path.join(folder, name + ".png")
    fig.savefig(fname, format="png")
    return fname


def _plane(ax, conf):
    ax.set_xlim(conf.fig_ax_lim[0].tolist())
    ax.set_ylim(conf.fig_ax_lim[1].tolist())
    ax.set_aspect('equal', 'box')


def obstacle_patches(conf, a=1):
    """Rectangles for car_park, ellipses otherwise, from XC1 .. B3 (plot_utils.py:47-70)."""
    patches = _mpl()[3]
    out = []
    for k in ("1", "2", "3"):
        xc, yc, w, h = (getattr(conf, n + k) for n in ("XC", "YC", "A", "B"))
        if conf.system_id == 'car_park':
            p = patches.Rectangle((xc - w / 2, yc - h / 2), w, h, angle=0.0, alpha=a)
        else:
            p = patches.Ellipse((xc, yc), w, h, angle=0.0, alpha=a)
        p.set_facecolor(OBSTACLE_COLOUR)
        out.append(p)
    return out


def draw_value_grid(data, conf, N_try, n_update, path, name='V'):
    """value_grid's dict -> 'V_<int(n_update)>' (plot_utils.py:361-373, :392-405): contourf of V.T over
    the grid, or for the manipulator's dict a scatter over its EE positions. Returns the file name."""
    cm = _mpl()[2]
    fig = _figure((8, 8))
    ax = fig.add_subplot()
    if "ee" in data:
        drawn = ax.scatter(data["ee"][:, 0], data["ee"][:, 1], c=data["V"], cmap=cm.coolwarm, antialiased=False)
    else:
        drawn = ax.contourf(data["x"], data["y"], np.ma.masked_invalid(data["V"].T), cmap=cm.coolwarm,
                            antialiased=False)
    for p in obstacle_patches(conf, 0.5):
        ax.add_patch(p)
    bar = fig.colorbar(drawn, ax=ax)
    bar.ax.tick_params(labelsize=TICK_SIZE)
    ax.set_title('N_try {} - n_update {}'.format(N_try, n_update))
    _plane(ax, conf)
    return _save(fig, path, N_try, '{}_{}'.format(name, int(n_update)))


def draw_traj(data, conf, N_try, init, update_step_counter, path):
    """traj_from_ICS's dict -> 'ee_traj_<init>_<update_step_counter>' (plot_utils.py:547-611): the
    warm-start trajectories (dashed) beside the TO trajectories, one colour per initial state, the
    start as a dot, the target as a star; skipped episodes are not drawn."""
    cm = _mpl()[2]
    n = len(data["ok"])
    colours = cm.coolwarm(np.linspace(0.1, 1, n))
    fig = _figure((12, 8))
    panels = ((fig.add_subplot(1, 2, 1), data["ee_RL"], '--', 'Warmstart traj.'),
              (fig.add_subplot(1, 2, 2), data["ee_TO"], '-', 'TO traj.'))
    for ax, ee, style, title in panels:
        for j in np.nonzero(data["ok"])[0]:
            ax.plot([conf.TARGET_STATE[0]], [conf.TARGET_STATE[1]], 'b*', markersize=5)
            ax.scatter(ee[j, 0, 0], ee[j, 0, 1], color=colours[j])
            ax.plot(ee[j, 1:, 0], ee[j, 1:, 1], style, color=colours[j])
        for p in obstacle_patches(conf, 0.5):
            ax.add_patch(p)
        _plane(ax, conf)
        ax.set_xlabel('X [m]')
        ax.set_title(title)
        ax.grid(True)
    panels[0][0].set_ylabel('Y [m]')
    return _save(fig, path, N_try, 'ee_traj_{}_{}'.format(init, update_step_counter))


def draw_return(ep_reward_list, conf, N_try, path):
    """The return history -> 'EpReturn_<N_try>' (plot_utils.py:332-343): ep_reward_list ** 2 on a log axis."""
    fig = _figure((15, 8))
    ax = fig.add_subplot(1, 1, 1)
    ax.set_yscale('log')
    ax.plot(np.asarray(ep_reward_list, dtype=np.float64) ** 2)
    ax.set_xlabel("Episode")
    ax.set_ylabel("Return")
    ax.set_title("N_try = {}".format(N_try))
    ax.grid(True)
    return _save(fig, path, N_try, 'EpReturn_{}'.format(N_try))


def draw_policy_eval(p_list, conf, N_try, n_updates, path, diff_loc=0):
    """PLOT.rollout's EE paths ([steps, 3] each, the last column the heading) ->
    'PolicyEvaluationSingleInit_<N_try>_<n_updates>' (MultiInit with diff_loc) (plot_utils.py:209-243):
    the paths with their start dots, for car_park the body box at the last pose."""
    patches, transforms = _mpl()[3:]
    fig = _figure((12, 8))
    fig.suptitle('POLICY: Discrete model, N try = {} N updates = {}'.format(N_try, n_updates), y=1, fontsize=FONT_SIZE)
    ax = fig.add_subplot(1, 1, 1)
    for p in p_list:
        ax.plot(p[:, 0], p[:, 1], marker='o', linewidth=0.3, markersize=1)
        ax.plot(p[0, 0], p[0, 1], 'ko', markersize=5)
        if conf.system_id == 'car_park' and np.isfinite(p[-1]).all():
            box = patches.FancyBboxPatch((-conf.L / 2, -conf.W / 2), conf.L, conf.W, edgecolor='none', alpha=0.5,
                                         boxstyle='round,pad=0')
            box.set_transform(transforms.Affine2D().rotate_deg(np.rad2deg(p[-1, 2])).translate(p[-1, 0], p[-1, 1])
                              + ax.transData)
            ax.add_patch(box)
    for p in obstacle_patches(conf):
        ax.add_artist(p)
    ax.plot(conf.TARGET_STATE[0], conf.TARGET_STATE[1], 'b*', markersize=10)
    _plane(ax, conf)
    ax.set_xlabel('X [m]')
    ax.set_ylabel('Y [m]')
    ax.grid(True)
    _fonts(fig)
    fig.tight_layout()
    kind ='PolicyEvaluationSingleInit' if diff_loc == 0 else 'PolicyEvaluationMultiInit'
    return _save(fig, path, N_try, '{}_{}_{}'.format(kind, N_try, n_updates))
