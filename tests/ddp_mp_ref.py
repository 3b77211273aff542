"""Test infrastructure: the Sobolev-label recursion (oracle.ddp.backward_pass, ddp_box_ref.backward_pass_box)
in mpmath at 80 digits, as the truth for episodes of full length.

The float64 recursion of the reference's formula never symmetrises V_xx. The antisymmetric rounding residue
of A^T V_xx A then grows geometrically (about 2.5x per step on a solved double-integrator episode), and
some 60 steps from the end of an episode the float64 labels no longer have a correct digit. Comparing two
float64 variants (pinv against inv, the rule of test_gpu_ddp.py) says nothing there: both are wrong. Here
the per-node float64 records (A, B, l_x, l_xx, l_u, l_uu of oracle.ddp) are taken as exact inputs and the
recursion itself is carried at 80 digits, where neither masking nor symmetrisation matters: the free
block is cut out by index, as ddp_box_ref does.
"""
import functools
import os

import mpmath
import numpy as np

from oracle import ddp as oddp


def episode_records(conf, states, controls):
    """The float64 inputs of the recursion along one episode, from oracle.ddp's building blocks, exactly as
    backward_pass evaluates them. states [T, >= n], controls [T-1, m]. Returns (records, lxT [n], lxxT [n, n],
    U [T-1, m]); records is a dict of A [T-1, n, n], B [T-1, n, m], l_x [T-1, n], l_xx [T-1, n, n],
    l_u [T-1, m], l_uu [T-1, m, m]. l_xu is 0 on every system (the cost separates in x and u); asserted."""
    n, m = oddp._n_m(conf)
    T = states.shape[0]
    X = np.asarray(states, dtype=np.float64)[:, :n]
    U = np.asarray(controls, dtype=np.float64)[:T - 1, :m]
    f = oddp.cost_functions(conf)
    w_run = [float(v) for v in conf.cost_weights_running[:7]]
    w_term = [float(v) for v in conf.cost_weights_terminal[:7]]
    rec = dict(A=np.zeros((T - 1, n, n)), B=np.zeros((T - 1, n, m)), l_x=np.zeros((T - 1, n)),
               l_xx=np.zeros((T - 1, n, n)), l_u=np.zeros((T - 1, m)), l_uu=np.zeros((T - 1, m, m)))
    for i in range(T - 1):
        rec["A"][i], rec["B"][i] = oddp.augmented_derivative(conf, X[i], U[i])
        rec["l_x"][i] = np.reshape(f["lx"](X[i], w_run), n)
        rec["l_xx"][i] = np.asarray(f["lxx"](X[i], w_run), dtype=np.float64)
        rec["l_u"][i] = np.reshape(f["lu"](U[i], w_run), m)
        rec["l_uu"][i] = np.asarray(f["luu"](U[i], w_run), dtype=np.float64)
        assert not np.asarray(f["lxu"](X[i], U[i], w_run), dtype=np.float64).any()
    lxT = np.reshape(f["lx"](X[-1], w_term), n).astype(np.float64)
    lxxT = np.asarray(f["lxx"](X[-1], w_term), dtype=np.float64).reshape(n, n)
    return rec, lxT, lxxT, U


def _mat(a):
    return [[mpmath.mpf(float(v)) for v in row] for row in np.asarray(a, dtype=np.float64)]


def _vec(a):
    return [mpmath.mpf(float(v)) for v in np.asarray(a, dtype=np.float64)]


def _tr(a):
    return [list(c) for c in zip(*a)]


def _mm(a, b):
    bt = _tr(b)
    return [[mpmath.fdot(r, c) for c in bt] for r in a]


def _mv(a, v):
    return [mpmath.fdot(r, v) for r in a]


def riccati_mp(records, lxT, lxxT, U, lo, hi, mu=1e-9, dps=80):
    """The label recursion of ddp_box_ref.backward_pass_box at `dps` digits over float64 records taken as
    exact (episode_records). lo = -inf, hi = +inf: the unbounded pass of oracle.ddp.backward_pass. Returns
    (V_x [T, n + 1] rounded to float64, time column 0; held [T-1, m] bool; margin: the smallest
    |Q_u[j]| / max|Q_u| over the controls on a limit, inf when there is none; max|V_xx| as a float)."""
    Tm1, n = records["l_x"].shape
    m = records["l_u"].shape[1]
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), (m,))
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64), (m,))
    V_x = np.zeros((Tm1 + 1, n + 1))
    held = np.zeros((Tm1, m), dtype=bool)
    margin, vxx_max = np.inf, 0.0
    with mpmath.workdps(dps):
        Vx, Vxx = _vec(lxT), _mat(lxxT)
        V_x[Tm1, :n] = [float(v) for v in Vx]
        mu_mp = mpmath.mpf(float(mu))
        for i in range(Tm1 - 1, -1, -1):
            A, B = _mat(records["A"][i]), _mat(records["B"][i])
            At, Bt = _tr(A), _tr(B)
            VA, VB = _mm(Vxx, A), _mm(Vxx, B)
            Qx = [a + b for a, b in zip(_vec(records["l_x"][i]), _mv(At, Vx))]
            Qu = [a + b for a, b in zip(_vec(records["l_u"][i]), _mv(Bt, Vx))]
            Qxx = [[a + b for a, b in zip(r1, r2)] for r1, r2 in zip(_mat(records["l_xx"][i]), _mm(At, VA))]
            Quu = [[a + b for a, b in zip(r1, r2)] for r1, r2 in zip(_mat(records["l_uu"][i]), _mm(Bt, VB))]
            Qxu = _mm(At, VB)                                   # + l_xu = 0
            for j in range(m):
                Quu[j][j] += mu_mp
            u = U[i]
            on = [bool(u[j] <= lo[j] or u[j] >= hi[j]) for j in range(m)]
            held[i] = [(u[j] <= lo[j] and Qu[j] < 0) or (u[j] >= hi[j] and Qu[j] > 0) for j in range(m)]
            if any(on):
                big = max(max(abs(q) for q in Qu), mpmath.mpf("1e-300"))
                margin = min(margin, float(min(abs(Qu[j]) / big for j in range(m) if on[j])))
            free = [j for j in range(m) if not held[i, j]]
            if free:
                Qi = mpmath.inverse(mpmath.matrix([[Quu[a][b] for b in free] for a in free]))
                Qi = [[Qi[a, b] for b in range(len(free))] for a in range(len(free))]
                Qxf = [[row[j] for j in free] for row in Qxu]
                QK = _mm(Qxf, Qi)                               # Q_xu[:, f] Qbar_ff^-1
                Vx = [a - b for a, b in zip(Qx, _mv(QK, [Qu[j] for j in free]))]
                Vxx = [[a - b for a, b in zip(r1, r2)] for r1, r2 in zip(Qxx, _mm(QK, _tr(Qxf)))]
            else:
                Vx, Vxx = Qx, Qxx
            V_x[i, :n] = [float(v) for v in Vx]
            vxx_max = max(vxx_max, float(max(abs(v) for row in Vxx for v in row)))
    return V_x, held, margin, vxx_max


def row_error(V, V_mp):
    """Per row, max |V - V_mp| over the state columns, relative to the episode's max |V_mp| (non-finite
    entries of V count as inf)."""
    n = V_mp.shape[1] - 1
    scale = np.abs(V_mp[:, :n]).max() + 1e-300
    with np.errstate(all="ignore"):
        err = np.abs(np.asarray(V)[:, :n] - V_mp[:, :n])
    err = np.where(np.isfinite(err), err, np.inf)
    return err.max(axis=1) / scale


def amplification(conf, states, controls, V_mp, lo=None, hi=None, symmetrize=False, inverse="inv"):
    """Per row, the float64 helper's error against the mp result V_mp, relative to the episode's max|V_x|:
    ddp_box_ref.backward_pass_box under the bounds (lo, hi), oracle.ddp.backward_pass when lo is None."""
    with np.errstate(all="ignore"):
        if lo is None:
            V = oddp.backward_pass(conf, states, controls, inverse=inverse, symmetrize=symmetrize)
        else:
            import ddp_box_ref as D
            V = D.backward_pass_box(conf, states, controls, lo, hi, inverse=inverse, symmetrize=symmetrize)[0]
    return row_error(V, V_mp)


@functools.lru_cache(maxsize=None)
def long_cases():
    """tests/golden/label_long.npz (tests/golden/make_label_long.py) as {case: dict(system, conf, S, U, T, lo,
    hi, Vb, Vu)}: one episode per case with the 80-digit labels of the bounded (Vb) and unbounded (Vu) pass."""
    from cacto_amd.confs import load_conf
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label_long.npz"))
    out = {}
    for c in (str(c) for c in z["cases"]):
        d = {k: z[k + "_" + c] for k in ("S", "U", "lo", "hi", "Vb", "Vu")}
        d.update(system=str(z["system_" + c]), T=int(z["T_" + c]))
        d["conf"] = load_conf(d["system"])
        out[c] = d
    return out


LONG_CASES = ("di_solved", "di_maxiter", "rand_single_integrator", "rand_double_integrator", "rand_car", "rand_car_park",
              "rand_manipulator", "rand_ur5")


@functools.lru_cache(maxsize=None)
def sym_error(case, bounded):
    """Per row of a fixture case, the symmetrised float64 helper's own error against the 80-digit labels,
    relative to the episode's max|V_x| (inverse="inv": an explicit inverse, as in the kernels)."""
    c = long_cases()[case]
    e = amplification(c["conf"], c["S"], c["U"], c["Vb"] if bounded else c["Vu"], c["lo"] if bounded else None, c["hi"],
                      symmetrize=True)
    e.setflags(write=False)
    return e


def first_failing_horizon(err, thresh=1e-6):
    """The smallest horizon (steps from the end of the episode) at which a row's relative error exceeds
    thresh; None when no row does."""
    bad = np.flatnonzero(np.asarray(err) > thresh)
    return None if len(bad) == 0 else int(len(err) - 1 - bad.max())
