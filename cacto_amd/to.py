"""TO — the reference's trajectory optimisation (TO.py:9-202) on the GPU.

`TO_System_Solve` (TO.py:37-100) states one NLP per episode with CasADi and solves it with IPOPT.
The problem is unconstrained apart from the dynamics and the fixed initial state (the control
bounds are the penalty w_b (u/u_max)^10 inside the cost, environment_TO.py:201-206; `bounds="conf"`
enforces them as hard limits besides, by control-limited DDP), so here it is
solved by a batched iLQR (`cacto_to_solve`): single shooting, Gauss-Newton DDP with first-order
dynamics and exact cost Hessians (or, `hessian="psd"`, their projections onto the positive
semidefinite cone), a backtracking line search and Levenberg-Marquardt regularisation, all episodes of a main.py iteration in one call, float64 throughout. The cost is
the TO cost (-Env.reward; for UR5 plus the bound penalty that environment_TO.py has and
UR5.reward leaves out), the dynamics Env.simulate. It is a local method like IPOPT: both stop at a
stationary point of the same problem, not necessarily the same one.

  solve_batch            the solver on device tensors
  solve_multistart       solve_batch from cfg["starts"] warm starts per episode, the best one kept
                         (multistart_expand, one solve_batch, multistart_select)
  solve_plan             what solve_batch runs for a config (one kernel or a host-issued loop)
  backward_gains_batch   one regularised backward pass (gains k, K, expected decrease, PD verdict)
  forward_batch          one closed-loop roll-out with step size alpha
  TO_System_Solve        the reference's per-episode signature and return tuple (TO.py:100)
  TO_Solve               TO.py:102-117: + the time column and the Sobolev label dV/dx
  backward_pass[_batch]  TO.backward_pass (TO.py:119-202, `cacto_ddp_backward`) along any recorded
                         trajectory — a TO solution or the policy roll-outs of RL_AC.rollout_batch;
                         with `bounds` the bound-aware labels (`cacto_ddp_backward_box`)
"""
import ctypes as C
import numbers

import numpy as np
import torch

from . import _lib as L
from .system import DEVICE, dptr, stream

CONVERGED, MAXITER, FAILED = L.CACTO_TO_CONVERGED, L.CACTO_TO_MAXITER, L.CACTO_TO_FAILED

# max_iter backward passes, step sizes 2^0..2^-max_ls, stop at max_t |Q_u|_inf <= gtol, the Armijo
# fraction, mu x10 (from mu_min) on failure and /10 on success, poll the device every 8 iterations
# path: which kernels solve. 0 / "default": one thread per episode for the single integrator, the car
# and the double integrator (large batches), a loop issued by the host (which polls the device every
# poll_every iterations) for car_park, the manipulator and UR5; 1 / "wave": one workgroup per episode
# and the whole loop in one kernel for those three and car_park (per-episode calls and batches of a
# few hundred; no host round trip, poll_every is not used), the host-issued loop for the manipulator
# and UR5. TO.solve_plan tells what a config runs.
# hessian: the node Hessian l_xx of the backward pass. "exact" / 0: the cost's own; "psd" / 1: its
# projection onto the positive semidefinite cone at every node (cacto_to_opts), which keeps Q_uu
# positive definite without mu where the cost is concave. The Sobolev labels (backward_pass) are
# exact under either.
# bounds: hard limits lo <= u <= hi on the controls (cacto_to_box; control-limited DDP: a box QP per
# node of the backward pass, feedback on the unclamped controls only, every roll-out and the warm start
# clamped, gtol on the projected gradient). "none" / None: the reference's problem, where the penalty
# alone holds the controls; "conf": conf.u_min, conf.u_max; a pair (lo, hi) of nb_action values each
# (+-inf: that side open). Every returned control then lies in [lo, hi] exactly.
# labels: which Sobolev labels follow a solve (TO_Solve, RL_AC.compute_samples; the solver itself does
# not read the key). "reference": TO.backward_pass as the reference has it, the unconstrained dV/dx
# along the solution, bounded or not; "bounded": backward_pass with the bounds of the same cfg, which
# leaves the controls a bound holds out of the recursion (cacto_ddp_backward_box). Needs `bounds`.
# starts: candidate warm starts per episode (solve_multistart; solve_batch itself does not read the
# key). 1: the one solve from the caller's warm start, nothing else launched. N in 2..STARTS_MAX: every
# episode is solved from N warm starts in one solve over N E episodes — the caller's own, all-zero
# controls, and the caller's plus a perturbation that is constant over start_hold steps and uniform
# within +- start_sigma times half the control range (cacto_to_starts) — and the acceptable candidate
# with the lowest final cost is kept (cacto_to_select). start_seed: the generator's stream for callers
# of solve_multistart / TO_System_Solve that pass no seed (RL_AC.compute_samples makes its own key
# from RL_AC.start_seed and the loop index).
# start_sigma = 0.5 and start_hold = 8 are working values that NOBODY HAS MEASURED: nothing rests on
# them while starts defaults to 1, and the table of DESIGN.md §6 is where a measured pair belongs.
DEFAULT_CFG = dict(max_iter=400, max_ls=10, gtol=1e-4, armijo=1e-4, mu_min=1e-6, mu_up=10.0, mu_down=10.0,
                   mu_max=1e10, poll_every=8, path=0, hessian="exact", bounds="none", labels="reference",
                   starts=1, start_sigma=0.5, start_hold=8, start_seed=0)
PATHS = {"default": L.CACTO_TO_PATH_DEFAULT, "wave": L.CACTO_TO_PATH_WAVE}
HESSIANS = {"exact": L.CACTO_TO_HESS_EXACT, "psd": L.CACTO_TO_HESS_PSD}
LABELS = ("reference", "bounded")
STARTS_MAX = L.CACTO_TO_STARTS_MAX
# cfg keys that travel beside the ToCfg (make_opts, make_box, label_bounds, make_starts)
NOT_FIELDS = ("hessian", "bounds", "labels", "starts", "start_sigma", "start_hold", "start_seed")


def make_opts(cfg=None):
    """The ToOpts (cacto_to_opts) of a cfg dict: its `hessian` key ("exact" / "psd" / 0 / 1, any
    integer type), or of a bare hessian value. A ToOpts is returned as it is."""
    if isinstance(cfg, L.ToOpts):
        return cfg
    h = DEFAULT_CFG["hessian"] if cfg is None else cfg
    if isinstance(cfg, dict):
        h = cfg.get("hessian", DEFAULT_CFG["hessian"])
    if isinstance(h, str) and h in HESSIANS:
        h = HESSIANS[h]
    if isinstance(h, bool) or not isinstance(h, numbers.Integral) or int(h) not in HESSIANS.values():
        raise ValueError("unknown TO hessian %r (one of %s, or 0 / 1)" % (h, sorted(HESSIANS)))
    o = L.ToOpts()
    o.hessian = int(h)
    return o


def make_box(cfg=None, conf=None):
    """The ToBox (cacto_to_box) of a cfg dict's `bounds` key, or of a bare bounds value: None for
    "none" / None (no bounds: the entries without them are called); "conf": conf.u_min, conf.u_max; a
    pair (lo, hi) of array-likes of conf.nb_action values, lo < hi, no NaN. A ToBox is returned as it
    is. Anything else: ValueError. Without a conf only the form is checked (make_cfg) and the result
    is None."""
    b = cfg.get("bounds", DEFAULT_CFG["bounds"]) if isinstance(cfg, dict) else cfg
    if isinstance(b, L.ToBox):
        return b
    if b is None or (isinstance(b, str) and b == "none"):
        return None
    bad = ValueError("unknown TO bounds %r (\"none\", \"conf\", or a pair (lo, hi) of nb_action values, lo < hi)" % (b,))
    if isinstance(b, str):
        if b != "conf":
            raise bad
        if conf is None:
            return None
        lo, hi = conf.u_min, conf.u_max
    else:
        try:
            lo, hi = b
            lo, hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
        except (TypeError, ValueError):
            raise bad from None
        if lo.ndim != 1 or lo.shape != hi.shape or not 1 <= len(lo) <= L.MAX_ACTION:
            raise bad
        if conf is None:
            return None
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    if lo.shape != (conf.nb_action,) or hi.shape != (conf.nb_action,) or not (lo < hi).all():
        raise bad
    box = L.ToBox()
    box.mode = L.CACTO_TO_BOUNDS_BOX
    for j in range(conf.nb_action):
        box.lo[j], box.hi[j] = float(lo[j]), float(hi[j])
    return box


def label_bounds(cfg=None):
    """The `bounds` that the labels after a solve with `cfg` take (backward_pass's argument): None for
    labels="reference" (and for a ToCfg, which holds no such key), the cfg's own `bounds` for
    labels="bounded". ValueError for an unknown `labels`, and for "bounded" in a cfg without bounds."""
    if not isinstance(cfg, dict):
        return None
    lab = cfg.get("labels", DEFAULT_CFG["labels"])
    if not isinstance(lab, str) or lab not in LABELS:
        raise ValueError("unknown TO labels %r (one of %s)" % (lab, list(LABELS)))
    if lab == "reference":
        return None
    b = cfg.get("bounds", DEFAULT_CFG["bounds"])
    none = isinstance(b, L.ToBox) and b.mode == L.CACTO_TO_BOUNDS_NONE
    if b is None or (isinstance(b, str) and b == "none") or none:
        raise ValueError("TO labels=\"bounded\" needs bounds (\"conf\" or a pair (lo, hi)) in the same cfg, "
                         "not bounds=%r" % (b,))
    return b


def make_starts(cfg=None):
    """(starts, start_sigma, start_hold, start_seed) of a cfg dict, checked: starts an integer in
    [1, STARTS_MAX], start_sigma finite and >= 0, start_hold an integer >= 1, start_seed an integer.
    A ToCfg (which holds none of them) and None give the defaults: one start."""
    d = cfg if isinstance(cfg, dict) else {}
    n, sigma, hold, seed = (d.get(k, DEFAULT_CFG[k]) for k in ("starts", "start_sigma", "start_hold", "start_seed"))
    integer = lambda v: isinstance(v, numbers.Integral) and not isinstance(v, bool)
    if not integer(n) or not 1 <= int(n) <= STARTS_MAX:
        raise ValueError("TO starts must be an integer in [1, %d], not %r" % (STARTS_MAX, n))
    if isinstance(sigma, bool) or not isinstance(sigma, numbers.Real) or not np.isfinite(sigma) or sigma < 0:
        raise ValueError("TO start_sigma must be finite and >= 0, not %r" % (sigma,))
    if not integer(hold) or int(hold) < 1:
        raise ValueError("TO start_hold must be an integer >= 1, not %r" % (hold,))
    if not integer(seed):
        raise ValueError("TO start_seed must be an integer, not %r" % (seed,))
    return int(n), float(sigma), int(hold), int(seed)


def stream_key(seed, ep=0):
    """The 64-bit generator key of cacto_to_starts for a run's seed and a loop index: seed mod 2^32 in
    the high word, ep mod 2^32 in the low one, so no two loops of a run and no two runs share a stream."""
    return ((int(seed) & 0xFFFFFFFF) << 32) | (int(ep) & 0xFFFFFFFF)


def make_cfg(cfg=None):
    """The 64-byte ToCfg (cacto_to_cfg) of a cfg dict over DEFAULT_CFG. The `hessian`, `bounds` and
    `labels` keys are checked here but are no fields of that struct: they travel in the ToOpts that
    make_opts(cfg) and the ToBox that make_box(cfg, conf) give, and a caller who hands solve_batch /
    solve_plan a ToCfg passes those as `opts` and `bounds`; `labels` is read after the solve
    (label_bounds). Neither are the multi-start keys (make_starts), which solve_multistart reads."""
    vals = dict(DEFAULT_CFG)
    vals.update(cfg or {})
    unknown = set(vals) - set(DEFAULT_CFG)
    if unknown:
        raise ValueError("unknown TO settings: %s" % sorted(unknown))
    if isinstance(vals["path"], str):
        if vals["path"] not in PATHS:
            raise ValueError("unknown TO path %r (one of %s, or 0 / 1)" % (vals["path"], sorted(PATHS)))
        vals["path"] = PATHS[vals["path"]]
    make_opts(vals)
    make_box(vals)
    label_bounds(vals)
    make_starts(vals)
    c = L.ToCfg()
    for k, v in vals.items():
        if k not in NOT_FIELDS:
            setattr(c, k, v)
    return c


def _cfg_opts(cfg, opts=None):
    """(ToCfg, ToOpts) of a call's `cfg` and `opts`. cfg: a dict over DEFAULT_CFG (its hessian key
    gives the options) or a ToCfg, which holds no options; opts: a ToOpts or a hessian value, which
    overrides the dict's key; None with a ToCfg means the defaults."""
    if isinstance(cfg, L.ToCfg):
        return cfg, make_opts(opts)
    return make_cfg(cfg), make_opts(cfg if opts is None else opts)


def _cfg_box(cfg, conf, bounds=None):
    """The ToBox (or None) of a call's `cfg` and `bounds`: the dict's key, or `bounds` over it; a ToCfg
    holds none."""
    if bounds is not None:
        return make_box(bounds, conf)
    return make_box(cfg, conf) if isinstance(cfg, dict) else None


def _opts_args(o, box=None):
    """(suffix of the entry's name, trailing arguments): the `_box` entry (options, bounds) when there
    are bounds, the `_opts` entry when only an option differs from the defaults, else the entry both
    extend, which is that call with NULL options and NULL bounds."""
    if box is not None:
        return "_box", (C.byref(o), C.byref(box))
    return ("_opts", (C.byref(o),)) if o.hessian != L.CACTO_TO_HESS_EXACT else ("", ())


class TO:
    def __init__(self, env, conf, w_S=0):
        self.env = env
        self.conf = conf
        self.w_S = w_S
        self.sys = env.sys

    # ------------------------------------------------------------------ the solver
    def solve_batch(self, S0, U_init, nsteps, cfg=None, out=None, opts=None, bounds=None):
        """cacto_to_solve. S0 [E, ns] f64, U_init [E, ldU, na] f64 (the warm start's controls),
        nsteps [E] int32 (Te; < 0 skips the episode), all on the device; cfg: a dict over
        DEFAULT_CFG, or a ToCfg together with opts (a ToOpts or a hessian value; _cfg_opts) and bounds
        (as the cfg key; over the dict's when given). Returns a dict of device tensors S [E, ldS, ns], U [E, ldU, na], step_cost
        [E, ldS], status [E] (CONVERGED / MAXITER / FAILED), iters [E], J [E, 2] (warm start's cost,
        final cost), ldS = ldU + 1. Rows past Te, and every row of a skipped episode, keep what
        `out` (the same dict, optional) held — zeros (status -1) when it is not given."""
        E, ldU = U_init.shape[0], U_init.shape[1]
        ldS = ldU + 1
        ns, na = self.conf.nb_state, self.conf.nb_action
        if out is None:
            f64 = dict(dtype=torch.float64, device=DEVICE)
            out = dict(S=torch.zeros(E, ldS, ns, **f64), U=torch.zeros(E, ldU, na, **f64),
                       step_cost=torch.zeros(E, ldS, **f64),
                       status=torch.full((E,), -1, dtype=torch.int32, device=DEVICE),
                       iters=torch.zeros(E, dtype=torch.int32, device=DEVICE), J=torch.zeros(E, 2, **f64))
        c, o = _cfg_opts(cfg, opts)
        # 0 for a path the library does not know: cacto_to_solve then reports the bad config
        sfx, extra = _opts_args(o, _cfg_box(cfg, self.conf, bounds))
        ws_bytes = L.lib().raw("cacto_to_workspace_bytes" + (sfx or "_cfg"))
        nbytes = int(ws_bytes(self.sys.handle, E, ldS, C.byref(c), *extra))
        ws = getattr(self, "_to_ws", None)
        if ws is None or ws.numel() < nbytes:
            ws = self._to_ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEVICE)
        L.lib().call("cacto_to_solve" + sfx, self.sys.handle, dptr(S0, torch.float64), dptr(U_init, torch.float64), ldU,
                     dptr(nsteps, torch.int32), E, ldS, C.byref(c), dptr(out["S"], torch.float64),
                     dptr(out["U"], torch.float64), dptr(out["step_cost"], torch.float64),
                     dptr(out["status"], torch.int32), dptr(out["iters"], torch.int32), dptr(out["J"], torch.float64),
                     dptr(ws), nbytes, stream(), *extra)
        return out

    # ------------------------------------------------------------------ several warm starts per episode
    def _half_range(self, cfg=None, bounds=None):
        """Half the control range per action, the unit of start_sigma: (hi - lo) / 2 under bounds
        where both sides are finite, else conf.u_max."""
        half = np.array(np.asarray(self.conf.u_max, dtype=np.float64).reshape(-1)[:self.conf.nb_action])
        box = _cfg_box(cfg, self.conf, bounds)
        if box is not None and box.mode == L.CACTO_TO_BOUNDS_BOX:
            for j in range(self.conf.nb_action):
                if np.isfinite(box.lo[j]) and np.isfinite(box.hi[j]):
                    half[j] = (box.hi[j] - box.lo[j]) / 2
        return np.ascontiguousarray(np.abs(half))

    def multistart_expand(self, S0, U_init, nsteps, cfg=None, seed=None, zero_start=True, bounds=None):
        """cacto_to_starts: the candidate batch of a multi-start solve, (S0_all [N E, ns], U_all
        [N E, ldU, na], nsteps_all [N E]) with N = cfg["starts"], candidate-major (candidate c of
        episode e is row c E + e; block 0 is the caller's batch, bit for bit). Candidate 1 is all
        zeros when zero_start (clear it when U_init is zero already); the others are U_init plus
        start_sigma * half range * xi, xi uniform in [-1, 1) and constant over start_hold steps, from
        the counter-based generator the header states, keyed by `seed` (a 64-bit integer; None:
        cfg["start_seed"]). Draws no host random number. One launch, asynchronous."""
        N, sigma, hold, cfg_seed = make_starts(cfg)
        seed = cfg_seed if seed is None else int(seed)
        E, ldU = U_init.shape[0], U_init.shape[1]
        ns, na = self.conf.nb_state, self.conf.nb_action
        S0_all = torch.empty(N * E, ns, dtype=torch.float64, device=DEVICE)
        U_all = torch.empty(N * E, ldU, na, dtype=torch.float64, device=DEVICE)
        n_all = torch.empty(N * E, dtype=torch.int32, device=DEVICE)
        half = self._half_range(cfg, bounds)
        L.lib().call("cacto_to_starts", self.sys.handle, dptr(S0, torch.float64, (E, ns), "S0"),
                     dptr(U_init, torch.float64, (E, ldU, na), "U_init"), ldU,
                     dptr(nsteps, torch.int32, (E,), "nsteps"), E, N, sigma, hold, half.ctypes.data_as(C.c_void_p),
                     int(bool(zero_start)), seed & 0xFFFFFFFFFFFFFFFF, dptr(S0_all), dptr(U_all), dptr(n_all),
                     stream())
        return S0_all, U_all, n_all

    def multistart_select(self, sol_all, nsteps, N, accept_maxiter=False, out=None):
        """cacto_to_select: per episode the acceptable candidate (CONVERGED, or MAXITER with
        accept_maxiter, and a finite final cost) with the lowest final cost of sol_all — solve_batch's
        dict over the N E rows of multistart_expand — lowest index on a tie, candidate 0 when none is
        acceptable. Returns solve_batch's E-shaped dict (`out`, optional, with solve_batch's masking:
        rows past Te and skipped episodes keep what it held; J[:, 0] is candidate 0's warm-start
        cost) plus start [E] int32 (-1: skipped), n_ok [E] int32, J_starts [E, N], status_starts
        [E, N]. One launch, asynchronous."""
        N = int(N)
        E = nsteps.shape[0]
        ldS, ldU = sol_all["S"].shape[1], sol_all["U"].shape[1]
        ns, na = self.conf.nb_state, self.conf.nb_action
        f64 = dict(dtype=torch.float64, device=DEVICE)
        i32 = dict(dtype=torch.int32, device=DEVICE)
        if out is None:
            out = dict(S=torch.zeros(E, ldS, ns, **f64), U=torch.zeros(E, ldU, na, **f64),
                       step_cost=torch.zeros(E, ldS, **f64), status=torch.full((E,), -1, **i32),
                       iters=torch.zeros(E, **i32), J=torch.zeros(E, 2, **f64))
        else:
            out = dict(out)
            for k in ("S", "U", "step_cost", "status", "iters", "J"):
                if tuple(out[k].shape) != (E,) + tuple(sol_all[k].shape[1:]):
                    raise ValueError("multistart_select: out[%r] is %s, not %s" % (k, tuple(out[k].shape),
                                                                                    (E,) + tuple(sol_all[k].shape[1:])))
        if not 1 <= N <= STARTS_MAX or any(sol_all[k].shape[0] != N * E for k in ("S", "U", "step_cost", "status",
                                                                                  "iters", "J")):
            raise ValueError("multistart_select: N = %d candidates of %d episodes need N in [1, %d] and N E rows in "
                             "every array of sol_all (S has %d)" % (N, E, STARTS_MAX, sol_all["S"].shape[0]))
        out.update(start=torch.empty(E, **i32), n_ok=torch.empty(E, **i32),
                   J_starts=torch.empty(E, N, **f64), status_starts=torch.empty(E, N, **i32))
        R = N * E
        L.lib().call("cacto_to_select", self.sys.handle, dptr(sol_all["S"], torch.float64, (R, ldS, ns), "S"),
                     dptr(sol_all["U"], torch.float64, (R, ldU, na), "U"),
                     dptr(sol_all["step_cost"], torch.float64, (R, ldS), "step_cost"),
                     dptr(sol_all["status"], torch.int32, (R,), "status"),
                     dptr(sol_all["iters"], torch.int32, (R,), "iters"),
                     dptr(sol_all["J"], torch.float64, (R, 2), "J"), dptr(nsteps, torch.int32, (E,), "nsteps"),
                     E, N, ldS, ldU,
                     int(bool(accept_maxiter)), dptr(out["S"], torch.float64), dptr(out["U"], torch.float64),
                     dptr(out["step_cost"], torch.float64), dptr(out["status"], torch.int32),
                     dptr(out["iters"], torch.int32), dptr(out["J"], torch.float64), dptr(out["start"]),
                     dptr(out["n_ok"]), dptr(out["J_starts"]), dptr(out["status_starts"]), stream())
        return out

    def solve_multistart(self, S0, U_init, nsteps, cfg=None, out=None, opts=None, bounds=None, seed=None,
                         zero_start=True, accept_maxiter=False):
        """solve_batch from cfg["starts"] warm starts per episode: multistart_expand, ONE solve_batch
        over the N E candidates, multistart_select. Returns solve_batch's dict plus start, n_ok,
        J_starts, status_starts (multistart_select). With starts == 1 (the default, and any ToCfg) it
        is solve_batch: that call and nothing else, its dict without the four extras. The solver
        treats every episode on its own, so candidate 0's solve is the one solve_batch would have
        run, and the winner's cost is never above it where it is acceptable. Two kernels more than
        solve_batch (and the fills of the candidates' outputs), nothing read back: capturable where
        solve_plan says on_device."""
        N = make_starts(cfg)[0]
        if N == 1:
            return self.solve_batch(S0, U_init, nsteps, cfg=cfg, out=out, opts=opts, bounds=bounds)
        S0_all, U_all, n_all = self.multistart_expand(S0, U_init, nsteps, cfg, seed=seed, zero_start=zero_start,
                                                      bounds=bounds)
        sol_all = self.solve_batch(S0_all, U_all, n_all, cfg=cfg, opts=opts, bounds=bounds)
        return self.multistart_select(sol_all, nsteps, N, accept_maxiter=accept_maxiter, out=out)

    def solve_plan(self, cfg=None, opts=None, bounds=None):
        """cacto_to_solve_plan: what solve_batch runs for this system with cfg and opts (as
        solve_batch's), as a dict: on_device (1: the whole loop is one kernel, nothing synchronises, the
        call can be captured into a graph), block_threads and lds_bytes of the solving kernel,
        launches_per_iter (kernel launches the host issues per iteration; 0 when on_device)."""
        c, o = _cfg_opts(cfg, opts)
        plan = L.ToPlan()
        sfx, extra = _opts_args(o, _cfg_box(cfg, self.conf, bounds))
        L.lib().call("cacto_to_solve_plan" + sfx, self.sys.handle, C.byref(c), C.byref(plan), *extra)
        return {name: int(getattr(plan, name)) for name, _ in L.ToPlan._fields_}

    def backward_gains_batch(self, S_traj, U_traj, nsteps, mu=0.0, hessian="exact", bounds=None):
        """cacto_to_backward_gains (hessian: "exact" / "psd" / 0 / 1, bounds: as the cfg keys; under
        bounds k is the box QP's solution around U_traj, K's clamped rows are 0 and dJ[2] is the
        projected gradient) along S_traj
        [E, ldS, ns], U_traj [E, ldU, na]: a dict k [E, ldU, na], K [E, ldU, na, nx], dJ [E, 3] = (sum k^T Q_u, 1/2 sum k^T Q_uu k, max |Q_u|), pd [E]
        (-1: Q_uu + mu I positive definite at every step, else the step where it was not; nothing
        below that step is defined)."""
        E, ldS, ldU = S_traj.shape[0], S_traj.shape[1], U_traj.shape[1]
        ns, na = self.conf.nb_state, self.conf.nb_action
        f64 = dict(dtype=torch.float64, device=DEVICE)
        out = dict(k=torch.zeros(E, ldU, na, **f64), K=torch.zeros(E, ldU, na, ns - 1, **f64),
                   dJ=torch.zeros(E, 3, **f64), pd=torch.full((E,), -1, dtype=torch.int32, device=DEVICE))
        sfx, extra = _opts_args(make_opts(hessian), make_box(bounds, self.conf))
        L.lib().call("cacto_to_backward_gains" + sfx, self.sys.handle, dptr(S_traj, torch.float64), ldS,
                     dptr(U_traj, torch.float64), ldU, dptr(nsteps, torch.int32), E, float(mu), dptr(out["k"]),
                     dptr(out["K"]), dptr(out["dJ"]), dptr(out["pd"]), stream(), *extra)
        return out

    def forward_batch(self, S_traj, U_traj, k, K, nsteps, alpha=1.0, bounds=None):
        """cacto_to_forward: u_t = ubar_t + alpha k_t + K_t (x_t - xbar_t) rolled out from S_traj[:, 0],
        every u_t clamped to `bounds` (as the cfg key) when given.
        Returns (S_new, U_new, cost_new [E, ldS]); k = K = None gives the open-loop roll-out."""
        E, ldS, ldU = S_traj.shape[0], S_traj.shape[1], U_traj.shape[1]
        S_new, U_new = torch.zeros_like(S_traj), torch.zeros_like(U_traj)
        cost = torch.zeros(E, ldS, dtype=torch.float64, device=DEVICE)
        box = make_box(bounds, self.conf)
        sfx, extra = ("_box", (C.byref(box),)) if box is not None else ("", ())
        L.lib().call("cacto_to_forward" + sfx, self.sys.handle, dptr(S_traj, torch.float64), ldS,
                     dptr(U_traj, torch.float64), ldU, dptr(k, torch.float64), dptr(K, torch.float64),
                     dptr(nsteps, torch.int32), E, float(alpha), dptr(S_new), dptr(U_new), dptr(cost), stream(), *extra)
        return S_new, U_new, cost

    # ------------------------------------------------------------------ the reference's signatures
    def TO_System_Solve(self, ICS_state, init_TO_states, init_TO_controls, T, cfg=None, accept_maxiter=False):
        """TO.py:37-100 for one episode: returns (success_flag, TO_controls [T, na], TO_states
        [T+1, nx], TO_ee_pos_arr [T+1, 3], TO_total_cost, TO_step_cost [T+1]) as numpy float64.
        The solver is single shooting: the warm start is its controls rolled out from ICS_state, so
        init_TO_states is accepted and ignored. Controls may be float32 (a roll-out's actions);
        they are converted to float64. success_flag is 1 only when the solver converged (or, with
        accept_maxiter, stopped at max_iter); otherwise the reference's failure branch: the last
        iterate's controls and states, None for the EE positions, the total and the step costs."""
        ns, na = self.conf.nb_state, self.conf.nb_action
        T = int(T)
        S0 = torch.as_tensor(np.asarray(ICS_state, dtype=np.float64).reshape(1, ns), device=DEVICE)
        U = np.zeros((1, max(T, 1), na))
        U[0, :T] = np.asarray(init_TO_controls, dtype=np.float64).reshape(-1, na)[:T]
        # cfg["starts"] > 1: the best of that many warm starts (stream cfg["start_seed"]; the all-zero
        # candidate only where the warm start is not zero itself); 1: solve_batch, as ever
        out = self.solve_multistart(S0, torch.as_tensor(U, device=DEVICE),
                                    torch.tensor([T], dtype=torch.int32, device=DEVICE), cfg=cfg,
                                    zero_start=bool(U.any()), accept_maxiter=accept_maxiter)
        status = int(out["status"][0].item())
        states = out["S"][0, :T + 1]
        TO_states = states[:, :ns - 1].cpu().numpy()
        TO_controls = out["U"][0, :T].cpu().numpy()
        if not (status == CONVERGED or (accept_maxiter and status == MAXITER)):
            return 0, TO_controls, TO_states, None, None, None
        EE = torch.empty(T + 1, 3, dtype=torch.float64, device=DEVICE)
        L.lib().call("cacto_env_ee", self.sys.handle, dptr(states.contiguous()), dptr(EE), T + 1, stream())
        return (1, TO_controls, TO_states, EE.cpu().numpy(), float(out["J"][0, 1].item()),
                out["step_cost"][0, :T + 1].cpu().numpy())

    def TO_Solve(self, ICS_state, init_TO_states, init_TO_controls, T, cfg=None, accept_maxiter=False):
        """TO.py:102-117: (TO_controls, TO_states [T+1, ns] with the time column ICS time + dt * t,
        success_flag, TO_ee_pos_arr, TO_step_cost, dVdx [T+1, ns]); dVdx from backward_pass
        (mu = 1e-9; with labels="bounded" in cfg under the cfg's bounds) when w_S != 0, else zeros.
        On failure (None, None, 0, None, None, None)."""
        flag, U, X, ee, _, step_cost = self.TO_System_Solve(ICS_state, init_TO_states, init_TO_controls, T, cfg=cfg,
                                                            accept_maxiter=accept_maxiter)
        if flag == 0:
            return None, None, flag, None, None, None
        T = int(T)
        if self.w_S != 0:
            dVdx = self.backward_pass(T + 1, X, U, bounds=label_bounds(cfg))
        else:
            dVdx = np.zeros((T + 1, self.conf.nb_state))
        t0 = float(np.asarray(ICS_state, dtype=np.float64).reshape(-1)[-1])
        X = np.concatenate((X, t0 + np.transpose(self.conf.dt * np.array([range(T + 1)]))), axis=1)
        return U, X, flag, ee, step_cost, dVdx

    # ------------------------------------------------------------------ Sobolev labels
    def backward_pass(self, T, TO_states, TO_controls, mu=1e-9, bounds=None):
        """TO.py:119-202 for one episode: T states s_0..s_{T-1} ([T, >= ns-1]; a time column is
        ignored), T-1 controls. Returns V_x [T, ns] (numpy float64, last column 0). bounds: as
        backward_pass_batch's."""
        ns, na = self.conf.nb_state, self.conf.nb_action
        S = np.zeros((1, T, ns))
        S[0, :, :ns - 1] = np.asarray(TO_states, dtype=np.float64)[:T, :ns - 1]
        U = np.zeros((1, max(T - 1, 1), na))
        U[0, :T - 1] = np.asarray(TO_controls, dtype=np.float64)[:T - 1, :na]
        out = self.backward_pass_batch(torch.as_tensor(S, device=DEVICE), torch.as_tensor(U, device=DEVICE),
                                       torch.tensor([T - 1], dtype=torch.int32, device=DEVICE), mu=mu, bounds=bounds)
        return out[0].cpu().numpy()

    def backward_pass_batch(self, S_traj, U_traj, nsteps, mu=1e-9, out=None, status=None, bounds=None):
        """Device batch: S_traj [E, ldS, ns] f64, U_traj [E, ldU, na] f64, nsteps [E] int32 (Te per
        episode: Te + 1 states). Returns dVdx [E, ldS, ns] f64 (rows past Te untouched).
        status [E] int32 (device, a rollout's): episodes with status != 0 were dropped for a NaN
        state (RL.py:229-231, main.py:236) and get no labels (their rows stay untouched).
        bounds (as the cfg key; None / "none": the reference's recursion, cacto_ddp_backward): the
        bound-aware labels of cacto_ddp_backward_box. A control that sits on a limit with the reward's
        gradient Q_u pointing out of the box is held: it takes no part in that node's
        V_x = Q_x - Q_xu Qbar^-1 Q_u, V_xx = Q_xx - Q_xu Qbar^-1 Q_xu^T. On a trajectory where no
        control is held the result is the unbounded call's bit for bit."""
        E, ldS = S_traj.shape[0], S_traj.shape[1]
        if out is None:
            out = torch.zeros_like(S_traj)
        if status is not None:
            nsteps = torch.where(status.to(device=DEVICE) == 0, nsteps.to(device=DEVICE, dtype=torch.int32),
                                 torch.full_like(nsteps, -1, dtype=torch.int32, device=DEVICE)).contiguous()
        box = make_box(bounds, self.conf)
        sfx, extra = ("_box", (C.byref(box),)) if box is not None else ("", ())
        L.lib().call("cacto_ddp_backward" + sfx, self.sys.handle, dptr(S_traj, torch.float64), ldS,
                     dptr(U_traj, torch.float64), U_traj.shape[1], dptr(nsteps, torch.int32), E, float(mu),
                     dptr(out, torch.float64), stream(), *extra)
        return out
