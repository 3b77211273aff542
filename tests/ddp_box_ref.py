"""Test infrastructure: the bound-aware Sobolev labels (cacto_ddp_backward_box, TO.backward_pass with
`bounds`) in numpy float64, in the reward convention of oracle.ddp.backward_pass and on its building
blocks (oracle.ddp.cost_functions, augmented_derivative).

Per node, control j is held when it sits on or outside a limit and the reward's gradient points out of
the box (u_j <= lo_j with Q_u[j] < 0, or u_j >= hi_j with Q_u[j] > 0); with f the controls not held,
    V_x = Q_x - Q_xu[:, f] Qbar_uu[f, f]^-1 Q_u[f],   V_xx = Q_xx - Q_xu[:, f] Qbar_uu[f, f]^-1 Q_xu[:, f]^T,
and V_x = Q_x, V_xx = Q_xx when f is empty. The free block is cut out with index sets and inverted on
its own: nothing here masks a matrix, which is how the kernels do it (ddp_label_mask, ddp_device.h).
"""
import numpy as np

from oracle import ddp as oddp


def held_set(u, Q_u, lo, hi):
    """(held [m] bool, on [m] bool): the controls a bound holds, and those on or outside a limit."""
    at_lo, at_hi = u <= lo, u >= hi
    return (at_lo & (Q_u < 0)) | (at_hi & (Q_u > 0)), at_lo | at_hi


def backward_pass_box(conf, states, controls, lo, hi, mu=1e-9, inverse="pinv", symmetrize=False):
    """oracle.ddp.backward_pass under the bounds lo <= u <= hi ([m] each; +-inf: that side open).
    states [T, >= n], controls [T-1, m]. Returns (V_x [T, n+1] with the time column 0, held [T-1, m]
    bool, margin): margin is the smallest |Q_u[j]| / max|Q_u| of the node over the controls on a
    limit — how far the nearest held decision is from flipping (0: a control on a limit whose Q_u[j]
    is 0; inf: no control on a limit). symmetrize: as in oracle.ddp.backward_pass."""
    n, m = oddp._n_m(conf)
    T = states.shape[0]
    X_bar = np.asarray(states, dtype=np.float64)[:, :n]
    U_bar = np.asarray(controls, dtype=np.float64)[:T - 1, :m]
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    f = oddp.cost_functions(conf)
    w_run = [float(v) for v in conf.cost_weights_running[:7]]
    w_term = [float(v) for v in conf.cost_weights_terminal[:7]]
    inv = np.linalg.pinv if inverse == "pinv" else np.linalg.inv
    V_x = np.zeros((T, n + 1))
    V_xx = np.zeros((T, n, n))
    held = np.zeros((max(T - 1, 0), m), dtype=bool)
    margin = np.inf
    V_x[T - 1, :-1] = np.reshape(f["lx"](X_bar[-1], w_term), n)
    V_xx[T - 1] = f["lxx"](X_bar[-1], w_term)
    for i in range(T - 2, -1, -1):
        A, B = oddp.augmented_derivative(conf, X_bar[i], U_bar[i])
        l_x = np.reshape(f["lx"](X_bar[i], w_run), n)
        l_xx = np.asarray(f["lxx"](X_bar[i], w_run), dtype=np.float64)
        l_u = np.reshape(f["lu"](U_bar[i], w_run), m)
        l_uu = np.asarray(f["luu"](U_bar[i], w_run), dtype=np.float64)
        l_xu = np.asarray(f["lxu"](X_bar[i], U_bar[i], w_run), dtype=np.float64).reshape(n, m)
        Q_x = l_x + A.T @ V_x[i + 1, :-1]
        Q_u = l_u + B.T @ V_x[i + 1, :-1]
        Q_xx = l_xx + A.T @ V_xx[i + 1] @ A
        Q_uu = l_uu + B.T @ V_xx[i + 1] @ B
        Q_xu = l_xu + A.T @ V_xx[i + 1] @ B
        Qbar_uu = Q_uu + mu * np.identity(m)
        held[i], on = held_set(U_bar[i], Q_u, lo, hi)
        if on.any():
            margin = min(margin, float((np.abs(Q_u[on]) / max(np.abs(Q_u).max(), 1e-300)).min()))
        free = np.flatnonzero(~held[i])
        if len(free) == m:                                  # nothing held: the oracle's own expressions
            Qi = inv(Qbar_uu)
            V_x[i, :-1] = Q_x - Q_xu @ Qi @ Q_u
            V_xx[i] = Q_xx - Q_xu @ Qi @ Q_xu.T
        elif len(free) == 0:
            V_x[i, :-1] = Q_x
            V_xx[i] = Q_xx
        else:
            Qi = inv(Qbar_uu[np.ix_(free, free)])
            Q_xf = Q_xu[:, free]
            V_x[i, :-1] = Q_x - Q_xf @ Qi @ Q_u[free]
            V_xx[i] = Q_xx - Q_xf @ Qi @ Q_xf.T
        if symmetrize:
            V_xx[i] = 0.5 * (V_xx[i] + V_xx[i].T)
    return V_x, held, margin


def label_inputs(system, kind="conf", n_ep=6, seed=None, zero=4, skip=5):
    """The GPU parity inputs: ilqr_ref.random_episodes(system, n_ep, seed) (seed: LABEL_CASES) with the
    controls clamped to the bounds `kind` names (ilqr_box.BoxProblem: "conf" or "test") and the states
    re-simulated; episode `zero` has Te = 0 and episode `skip` nsteps = -1. Returns (problem, S, U, T)."""
    import ilqr_box as X
    import ilqr_ref as R
    P = X.BoxProblem(system, kind)
    S, U, T = R.random_episodes(system, n_ep, LABEL_CASES[system, kind] if seed is None else seed)
    T = T.copy()
    T[zero], T[skip] = 0, -1
    S, U = clamped_episodes(P, S, U, T)
    return P, S, U, T


def label_reference(P, S, U, T):
    """The helper over a batch. Returns (ref, alt, stats): per episode V_x with pinv and with inv (None
    for a skipped episode), and dict(held, on_free, inside, margin) counted over the batch's controls."""
    ref, alt = [], []
    st = dict(held=0, on_free=0, inside=0, margin=np.inf)
    for e in range(len(T)):
        Te = int(T[e])
        if Te < 0:
            ref.append(None)
            alt.append(None)
            continue
        V, held, margin = backward_pass_box(P.conf, S[e, :Te + 1], U[e, :Te], P.lo, P.hi)
        ref.append(V)
        alt.append(backward_pass_box(P.conf, S[e, :Te + 1], U[e, :Te], P.lo, P.hi, inverse="inv")[0])
        on = (U[e, :Te] <= P.lo) | (U[e, :Te] >= P.hi)
        st["held"] += int(held.sum())
        st["on_free"] += int((on & ~held).sum())
        st["inside"] += int((~on).sum())
        st["margin"] = min(st["margin"], margin)
    return ref, alt, st


def label_inputs_ok(st):
    """The rule the seeds of LABEL_CASES were picked by: no held decision closer than 1e-6 (relative) to
    flipping, and at least three controls of the batch held, three on a limit without being held, three
    inside."""
    return st["margin"] >= 1e-6 and st["held"] >= 3 and st["on_free"] >= 3 and st["inside"] >= 3


# (system, bounds) -> random_episodes seed of the GPU parity test, picked on the CPU: the first seed >= 21
# that label_inputs_ok accepts (21 everywhere; margins 3e-3 .. 2e-2, 8 .. 41 held controls). The conf's
# own bounds on every system but the manipulator, where seeds 21 .. 26 hold no control under them (14 .. 40
# sit on a limit with the gradient pointing inwards): ilqr_box's tightened "test" bounds there. UR5 under
# the conf's holds 3 controls, the rule's minimum, so it runs under the "test" bounds (34 held) besides.
LABEL_CASES = {("single_integrator", "conf"): 21, ("double_integrator", "conf"): 21, ("car", "conf"): 21,
               ("car_park", "conf"): 21, ("manipulator", "test"): 21, ("ur5", "conf"): 21, ("ur5", "test"): 21}


def clamped_episodes(problem, S, U, T):
    """Random-control episodes (ilqr_ref.random_episodes) with every control clamped to the box of
    `problem` (an ilqr_box.BoxProblem) and the states re-simulated from S[e, 0]. T[e] <= 0: the
    episode keeps its first state only. Returns new (S, U)."""
    S2, U2 = np.zeros_like(S), np.zeros_like(U)
    for e in range(len(T)):
        Te = max(int(T[e]), 0)
        s, u, _ = problem.rollout(S[e, 0], U[e], Te)
        S2[e, :Te + 1], U2[e, :Te] = s, u
    return S2, U2
