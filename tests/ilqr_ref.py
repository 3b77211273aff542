"""Test infrastructure: the iLQR of cacto_to_solve in numpy float64 over the oracle.

The same algorithm as cacto_amd/csrc/to_kernels.hip, written independently of it: cost derivatives
from oracle.ddp.cost_functions (sympy), dynamics Jacobians from oracle.ddp.augmented_derivative,
dynamics from oracle.env. Cost convention throughout (cost = -reward, l_xu = 0). Besides the solver
it provides the adjoint gradient of the rolled-out cost with respect to the controls,
    lambda_T = l_x(x_T),  lambda_t = l_x + A^T lambda_{t+1},  g_t = l_u + B^T lambda_{t+1},
which checks stationarity of a solution without any part of the Riccati recursion.
"""
import random

import numpy as np

from cacto_amd.confs import load_conf
from oracle import ddp as oddp
from oracle import env as oenv

CONVERGED, MAXITER, FAILED = 0, 1, 2
# the full-solve settings of the GPU tests and tools/to_bench.py
SOLVE_CFG = dict(max_iter=400, max_ls=10, gtol=1e-4, armijo=1e-4, mu_min=1e-6, mu_up=10.0, mu_down=10.0, mu_max=1e10)


class Problem:
    def __init__(self, system):
        self.system = system
        self.conf = conf = load_conf(system)
        self.oe = oenv.make_env(conf)
        self.f = oddp.cost_functions(conf)
        self.n, self.m = conf.nb_state - 1, conf.nb_action
        self.w_run = [float(v) for v in conf.cost_weights_running[:7]]
        self.w_term = [float(v) for v in conf.cost_weights_terminal[:7]]
        self.dt = float(conf.dt)

    # ---- cost and its derivatives (cost = -reward of the TO cost function)
    def cost(self, x, u=None):
        """Running cost at (x, u), or the terminal cost at x when u is None."""
        if u is None:
            return -float(self.f["r"](x[:self.n], np.zeros(self.m), self.w_term))
        return -float(self.f["r"](x[:self.n], u, self.w_run))

    def lx(self, x, terminal=False):
        w = self.w_term if terminal else self.w_run
        return (-np.reshape(self.f["lx"](x[:self.n], w), self.n),
                -np.asarray(self.f["lxx"](x[:self.n], w), dtype=np.float64).reshape(self.n, self.n))

    def lu(self, u):
        return (-np.reshape(self.f["lu"](u, self.w_run), self.m),
                -np.asarray(self.f["luu"](u, self.w_run), dtype=np.float64).reshape(self.m, self.m))

    def jac(self, x, u):
        return oddp.augmented_derivative(self.conf, x, u)

    # ---- roll-outs
    def rollout(self, s0, U, T, k=None, K=None, Sbar=None, alpha=1.0):
        """u_t = U_t + alpha k_t + K_t (x_t - xbar_t) from s0 (with time). Returns S [T+1, ns],
        U_new [T, m], step_cost [T+1]; the time column is t0 + dt * t."""
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
                Un[t] = u
                c[t] = self.cost(S[t], u)
                S[t + 1] = self.oe.simulate(S[t], u)
                S[t + 1, -1] = t0 + self.dt * (t + 1)
            c[T] = self.cost(S[T])
        return S, Un, c

    # ---- backward pass
    def backward(self, S, U, T, mu, inverse="solve"):
        """One regularised backward pass. Returns dict(k [T, m], K [T, m, n], dJ [3], pd, decisive):
        pd = -1 or the step whose Qbar_uu has no Cholesky factor; decisive = lambda_min / max|lambda|
        of Qbar_uu at that step, or its minimum over the steps when every one is positive definite.
        inverse="inv" forms Qbar_uu^-1 explicitly (the rounding yardstick of the GPU comparison)."""
        n, m = self.n, self.m
        k, K = np.zeros((T, m)), np.zeros((T, m, n))
        Vx, Vxx = self.lx(S[T], terminal=True)
        dJ = np.zeros(3)
        decisive = np.inf
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
                return dict(k=k, K=K, dJ=dJ, pd=t, decisive=ratio)
            decisive = min(decisive, ratio)
            if inverse == "inv":
                Qi = np.linalg.inv(Qbar)
                k[t], K[t] = -Qi @ Qu, -Qi @ Qux
            else:
                k[t], K[t] = -np.linalg.solve(Qbar, Qu), -np.linalg.solve(Qbar, Qux)
            dJ[0] += k[t] @ Qu
            dJ[1] += 0.5 * k[t] @ Quu @ k[t]
            dJ[2] = max(dJ[2], np.abs(Qu).max())
            Vx = Qx + K[t].T @ Quu @ k[t] + K[t].T @ Qu + Qux.T @ k[t]
            Vxx = Qxx + K[t].T @ Quu @ K[t] + K[t].T @ Qux + Qux.T @ K[t]
            Vxx = 0.5 * (Vxx + Vxx.T)
        return dict(k=k, K=K, dJ=dJ, pd=-1, decisive=decisive)

    # ---- adjoint gradient
    def gradient(self, S, U, T):
        """dJ/dU [T, m] of the rolled-out cost at the trajectory (S, U) by the adjoint recursion."""
        g = np.zeros((T, self.m))
        lam = self.lx(S[T], terminal=True)[0]
        for t in range(T - 1, -1, -1):
            A, B = self.jac(S[t, :self.n], U[t])
            g[t] = self.lu(U[t])[0] + B.T @ lam
            lam = self.lx(S[t])[0] + A.T @ lam
        return g

    # ---- the solver
    def solve(self, s0, U_init, T, cfg=None):
        c = dict(SOLVE_CFG)
        c.update(cfg or {})
        S, U, cost = self.rollout(s0, U_init, T)
        J = J0 = cost.sum()
        hist = [J]
        status, iters, mu, qu = MAXITER, 0, 0.0, np.nan
        if T == 0:
            status = CONVERGED
        elif not np.isfinite(J):
            status = FAILED
        while status == MAXITER and iters < c["max_iter"]:
            iters += 1
            b = self.backward(S, U, T, mu)
            raise_mu = b["pd"] >= 0
            if not raise_mu:
                qu = b["dJ"][2]
                if qu <= c["gtol"]:
                    status = CONVERGED
                    break
                raise_mu = True
                for j in range(c["max_ls"] + 1):
                    a = 2.0 ** -j
                    Sn, Un, cn = self.rollout(s0, U, T, b["k"], b["K"], S, a)
                    Jn = cn.sum()
                    if np.isfinite(Jn) and J - Jn >= c["armijo"] * -(a * b["dJ"][0] + a * a * b["dJ"][1]) and Jn <= J:
                        S, U, cost, J = Sn, Un, cn, Jn
                        hist.append(J)
                        mu = mu / c["mu_down"]
                        if mu < c["mu_min"]:
                            mu = 0.0
                        raise_mu = False
                        break
            if raise_mu:
                mu = max(mu * c["mu_up"], c["mu_min"])
                if mu > c["mu_max"]:
                    status = FAILED
        return dict(S=S, U=U, step_cost=cost, status=status, iters=iters, J=(J0, J), hist=hist, qu=qu)


# ---------------------------------------------------------------------- named inputs of the tests
# full-solve batches: (episodes, largest Te, seed)
SOLVE_SHAPES = {"single_integrator": (70, 24, 5), "double_integrator": (70, 24, 5), "car": (70, 24, 101),
                "car_park": (9, 24, 5), "manipulator": (9, 12, 5), "ur5": (3, 6, 5)}


def solve_inputs(system):
    """Initial states and lengths of the full-solve tests: oracle.env.reset states whose time entry
    is overwritten with (NSTEPS - Te) dt, Te drawn from 1..Tmax; in the 70-episode batches episode 3
    has Te = 0 and episode 11 is skipped (nsteps = -1). Returns (S0 [E, ns], nsteps [E] int32)."""
    conf = load_conf(system)
    oe = oenv.make_env(conf)
    E, Tmax, seed = SOLVE_SHAPES[system]
    rng = random.Random(seed)
    S0 = np.array([oe.reset(rng) for _ in range(E)], dtype=np.float64)
    Te = np.array([rng.randint(1, Tmax) for _ in range(E)], dtype=np.int32)
    if E >= 64:
        Te[3] = 0
    S0[:, -1] = (conf.NSTEPS - Te) * conf.dt
    if E >= 64:
        Te[11] = -1
    return S0, Te


def random_episodes(system, n_ep=6, seed=21):
    """Random-control episodes as tests/test_gpu_ddp.py makes them, T capped at 24 / 12 (manipulator) /
    8 (UR5). Returns (S [E, L, ns], U [E, L, na], T [E] int32)."""
    conf = load_conf(system)
    oe = oenv.make_env(conf)
    cap = {"manipulator": 12, "ur5": 8}.get(system, 24)
    rng = random.Random(seed)
    ns, na = conf.nb_state, conf.nb_action
    S0 = [oe.reset(rng) for _ in range(n_ep)]
    T = [min(conf.NSTEPS - int(s[-1] / conf.dt), cap) for s in S0]
    L = max(T) + 1
    S, U = np.zeros((n_ep, L, ns)), np.zeros((n_ep, L, na))
    for e in range(n_ep):
        S[e, 0] = S0[e]
        for t in range(T[e]):
            U[e, t] = [rng.uniform(-1.2, 1.2) * conf.u_max[i] for i in range(na)]
            S[e, t + 1] = oe.simulate(S[e, t], U[e, t])
    return S, U, np.asarray(T, dtype=np.int32)
