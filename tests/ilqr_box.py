"""Test infrastructure: tests/ilqr_ref.py's iLQR under hard control limits, the trajectory optimiser's
`bounds` mode (control-limited DDP; Tassa, Mansard, Todorov, ICRA 2014), in numpy float64.

The choices are those of cacto_amd/csrc/to_kernels.hip: Qbar_uu = Q_uu + mu I takes the positive
definite verdict whole, as without bounds; k is the minimiser of 1/2 x^T Qbar_uu x + Q_u^T x over
lo - ubar <= x <= hi - ubar (the offsets moved outward by rounding errors until ubar + offset reaches
the bound, BoxProblem.box); K = -Qbar_ff^-1 Q_ux,f on the free rows and 0 on the clamped ones; V_x,
V_xx, dJ[0], dJ[1] by the parent's formulas; dJ[2] the projected gradient; every roll-out clamps its
controls. The QP is solved by enumerating the 3^M assignments (free / at lo / at hi per component)
and keeping the one that satisfies the KKT conditions: nothing here shares code or method with the
projected-Newton iteration of cacto_amd/csrc/box_qp.h. solve is the parent's loop, re-stated so that
it can report how close each of its comparisons came to flipping.
"""
import itertools

import numpy as np

import ilqr_ref as R

# bounds of the full-solve and gains tests as a fraction of the conf's u_min / u_max: the conf's own
# where they bind on the test inputs, tightened on the two arms, whose short test episodes never
# reach theirs (tools/to_box_record.py prints the share of controls at a bound)
BOUND_SCALE = {"single_integrator": 1.0, "double_integrator": 1.0, "car": 1.0, "car_park": 1.0, "manipulator": 0.03,
               "ur5": 0.15}
# random_episodes seeds of the gains test (controls clamped to the conf's bounds, which are that test's
# on every system), picked on the CPU (tools/to_box_record.py --seeds): the first seed >= 21 at which, at
# mu = 0 and at mu = 1, the helper's PD verdicts are decisive (|decisive| >= 1e-3, the rule of
# test_gpu_to_solve.py), some control of the batch is clamped by the QP and some is free, and no QP is
# degenerate (box_qp's margin >= 1e-6)
GAINS_SEEDS = {"single_integrator": 21, "double_integrator": 22, "car": 21, "car_park": 21, "manipulator": 23, "ur5": 21}
# an episode of the record is excluded from the pass-count comparison when a comparison on the helper's
# path came this close (relative) to flipping
FLIP = 1e-9


def box_qp(H, q, lo, hi, inverse="solve"):
    """argmin 1/2 x^T H x + q^T x over lo <= x <= hi by enumeration. Returns (x, free [M] bool, margin):
    free[j] is False where x_j sits on a bound with the gradient pointing out of the box; margin is
    the smallest slack of the KKT inequalities that hold strictly at the solution, relative to the
    problem's scale (0: degenerate — a component on a bound with a vanishing multiplier)."""
    m = len(q)
    H = 0.5 * (H + H.T)

    def sol(A, b):
        return np.linalg.inv(A) @ b if inverse == "inv" else np.linalg.solve(A, b)
    best = None
    for assign in itertools.product((0, -1, 1), repeat=m):
        a = np.asarray(assign)
        if any((s == -1 and not np.isfinite(lo[j])) or (s == 1 and not np.isfinite(hi[j])) for j, s in enumerate(a)):
            continue
        x = np.where(a == -1, lo, np.where(a == 1, hi, 0.0))
        f = a == 0
        if f.any():
            x[f] = sol(H[np.ix_(f, f)], -(q[f] + H[np.ix_(f, ~f)] @ x[~f]))
        g = q + H @ x
        xs, gs = max(np.abs(x).max(), 1e-300), max(np.abs(q).max(), np.abs(g).max(), 1e-300)
        # slacks (>= 0 when the conditions hold): free components inside the box, multipliers outward
        slack = [min((x[j] - lo[j]) / xs, (hi[j] - x[j]) / xs) if f[j] else (g[j] if a[j] == -1 else -g[j]) / gs
                 for j in range(m)]
        viol = -min(min(slack), 0.0)
        val = 0.5 * x @ H @ x + q @ x
        if best is None or viol < best[0] - 1e-12 or (abs(viol - best[0]) <= 1e-12 and val < best[1]):
            best = (viol, val, x, f, min(slack))
        if viol == 0.0 and min(slack) > 1e-9:
            break       # strictly convex: the assignment that satisfies the conditions strictly is the only one
    viol, _, x, f, margin = best
    assert viol <= 1e-9, ("no active set satisfies the KKT conditions", viol)
    x = np.minimum(np.maximum(x, lo), hi)
    return x, f, max(margin, 0.0)


class BoxProblem(R.Problem):
    def __init__(self, system, bounds="conf"):
        R.Problem.__init__(self, system)
        if isinstance(bounds, str) and bounds == "conf":
            lo, hi = self.conf.u_min, self.conf.u_max
        elif isinstance(bounds, str) and bounds == "test":
            lo, hi = BOUND_SCALE[system] * self.conf.u_min, BOUND_SCALE[system] * self.conf.u_max
        else:
            lo, hi = bounds
        self.lo, self.hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)

    def clamp(self, u):
        return np.minimum(np.maximum(np.asarray(u, dtype=np.float64), self.lo), self.hi)

    def rollout(self, s0, U, T, k=None, K=None, Sbar=None, alpha=1.0):
        """The parent's roll-out with u_t = clamp(U_t + alpha k_t + K_t (x_t - xbar_t)); the open-loop
        one (k None) clamps U_t."""
        ns = self.n + 1
        S = np.zeros((T + 1, ns))
        Un = np.zeros((T, self.m))
        c = np.zeros(T + 1)
        S[0] = s0
        t0 = float(s0[-1])
        with np.errstate(all="ignore"):
            for t in range(T):
                u = np.array(U[t], dtype=np.float64)
                if k is not None:
                    u = u + alpha * k[t] + K[t] @ (S[t, :self.n] - Sbar[t, :self.n])
                u = self.clamp(u)
                Un[t] = u
                c[t] = self.cost(S[t], u)
                S[t + 1] = self.oe.simulate(S[t], u)
                S[t + 1, -1] = t0 + self.dt * (t + 1)
            c[T] = self.cost(S[T])
        return S, Un, c

    def box(self, u):
        """The node's box around its nominal control u: (lo - u, hi - u), each offset moved outward by
        single units in the last place until u + offset reaches the bound in float64 (no move where
        the difference is exact). With the offsets merely rounded, u + (hi - u) can stop one rounding
        error short of hi: a control the QP clamps would then not sit on its bound after the full
        step, and the next pass would count it as free."""
        u = np.asarray(u, dtype=np.float64)
        bl, bh = self.lo - u, self.hi - u
        for _ in range(8):
            short = u + bh < self.hi
            if not short.any():
                break
            bh = np.where(short, np.nextafter(bh, np.inf), bh)
        for _ in range(8):
            short = u + bl > self.lo
            if not short.any():
                break
            bl = np.where(short, np.nextafter(bl, -np.inf), bl)
        return bl, bh

    def held(self, u, Qu):
        """Components of a node that sit on a bound with the gradient pointing out of the box."""
        return ((u == self.lo) & (Qu > 0)) | ((u == self.hi) & (Qu < 0))

    def backward(self, S, U, T, mu, inverse="solve"):
        """The parent's pass under bounds. Besides its keys: free [T, m] bool (the QP's free set per
        node), qp_margin (the smallest box_qp margin over the nodes)."""
        n, m = self.n, self.m
        k, K = np.zeros((T, m)), np.zeros((T, m, n))
        free = np.ones((T, m), dtype=bool)
        Vx, Vxx = self.lx(S[T], terminal=True)
        dJ = np.zeros(3)
        decisive, qp_margin = np.inf, np.inf
        for t in range(T - 1, -1, -1):
            A, B = self.jac(S[t, :n], U[t])
            lx, lxx = self.lx(S[t])
            lu, luu = self.lu(U[t])
            Qx, Qu = lx + A.T @ Vx, lu + B.T @ Vx
            Qxx, Qux, Quu = lxx + A.T @ Vxx @ A, B.T @ Vxx @ A, luu + B.T @ Vxx @ B
            Qbar = Quu + mu * np.identity(m)
            ev = np.linalg.eigvalsh(0.5 * (Qbar + Qbar.T))
            ratio = ev[0] / np.abs(ev).max()
            try:
                if not np.isfinite(Qbar).all():
                    raise np.linalg.LinAlgError
                np.linalg.cholesky(Qbar)
            except np.linalg.LinAlgError:
                return dict(k=k, K=K, dJ=dJ, pd=t, decisive=ratio, free=free, qp_margin=qp_margin)
            decisive = min(decisive, ratio)
            bl, bh = self.box(U[t])
            k[t], f, margin = box_qp(Qbar, Qu, bl, bh, inverse=inverse)
            qp_margin = min(qp_margin, margin)
            free[t] = f
            if f.any():
                Qff = Qbar[np.ix_(f, f)]
                K[t][f] = -(np.linalg.inv(Qff) @ Qux[f] if inverse == "inv" else np.linalg.solve(Qff, Qux[f]))
            dJ[0] += k[t] @ Qu
            dJ[1] += 0.5 * k[t] @ Quu @ k[t]
            open_ = ~self.held(np.asarray(U[t], dtype=np.float64), Qu)
            if open_.any():
                dJ[2] = max(dJ[2], np.abs(Qu[open_]).max())
            Vx = Qx + K[t].T @ Quu @ k[t] + K[t].T @ Qu + Qux.T @ k[t]
            Vxx = Qxx + K[t].T @ Quu @ K[t] + K[t].T @ Qux + Qux.T @ K[t]
            Vxx = 0.5 * (Vxx + Vxx.T)
        return dict(k=k, K=K, dJ=dJ, pd=-1, decisive=decisive, free=free, qp_margin=qp_margin)

    def kkt_violation(self, S, U, T):
        """Largest violation of the first-order conditions of the bounded problem at (S, U), with the
        adjoint gradient g: |g| where lo < u < hi, max(-g, 0) at lo, max(g, 0) at hi."""
        g = self.gradient(S, U, T)
        U = np.asarray(U, dtype=np.float64)[:T]
        at_lo, at_hi = U == self.lo, U == self.hi
        v = np.where(at_lo, np.maximum(-g, 0.0), np.where(at_hi, np.maximum(g, 0.0), np.abs(g)))
        return float(v.max()) if v.size else 0.0

    def solve(self, s0, U_init, T, cfg=None):
        """R.Problem.solve, statement for statement, plus `flip`: the smallest relative distance from
        flipping over the PD verdicts and the line search's comparisons on the way."""
        c = dict(R.SOLVE_CFG)
        c.update(cfg or {})
        S, U, cost = self.rollout(s0, U_init, T)
        J = J0 = cost.sum()
        status, iters, mu, qu = R.MAXITER, 0, 0.0, np.nan
        flip = np.inf
        if T == 0:
            status = R.CONVERGED
        elif not np.isfinite(J):
            status = R.FAILED

        def near(a, b):
            return abs(a - b) / max(abs(a), abs(b), 1e-300)
        while status == R.MAXITER and iters < c["max_iter"]:
            iters += 1
            b = self.backward(S, U, T, mu)
            flip = min(flip, abs(b["decisive"]))
            raise_mu = b["pd"] >= 0
            if not raise_mu:
                qu = b["dJ"][2]
                if qu <= c["gtol"]:
                    status = R.CONVERGED
                    break
                raise_mu = True
                for j in range(c["max_ls"] + 1):
                    a = 2.0 ** -j
                    Sn, Un, cn = self.rollout(s0, U, T, b["k"], b["K"], S, a)
                    Jn = cn.sum()
                    want = c["armijo"] * -(a * b["dJ"][0] + a * a * b["dJ"][1])
                    if np.isfinite(Jn):
                        flip = min(flip, near(J - Jn, want), near(Jn, J) if Jn != J else np.inf)
                    if np.isfinite(Jn) and J - Jn >= want and Jn <= J:
                        S, U, cost, J = Sn, Un, cn, Jn
                        mu = mu / c["mu_down"]
                        if mu < c["mu_min"]:
                            mu = 0.0
                        raise_mu = False
                        break
            if raise_mu:
                mu = max(mu * c["mu_up"], c["mu_min"])
                if mu > c["mu_max"]:
                    status = R.FAILED
        return dict(S=S, U=U, step_cost=cost, status=status, iters=iters, J=(J0, J), qu=qu, flip=flip)
