"""Record the long-horizon Sobolev-label fixtures of tests/test_ddp_long_cpu.py and tests/test_gpu_ddp_long.py:

    python -B tests/golden/make_label_long.py            # writes tests/golden/label_long.npz, prints the table
    python -B tests/golden/make_label_long.py --check    # regenerates and compares with the file bit for bit
    python -B tests/golden/make_label_long.py --seeds    # how the random cases' seeds were picked

Runs on the CPU from the project's own helpers only (tests/ilqr_box.py, tests/ddp_box_ref.py, oracle/) and
needs mpmath; nothing comes from a reference checkout. The two solved cases take about a minute each (the
numpy iLQR), the rest seconds.

Per case <c> the file holds system_<c>, S_<c> [T + 1, ns], U_<c> [T, na], T_<c>, lo_<c>, hi_<c> (the bounds of
the bounded pass) and Vb_<c>, Vu_<c> [T + 1, ns]: the labels of the bounded and the unbounded pass from
ddp_mp_ref.riccati_mp (80 digits over the float64 records of oracle.ddp, rounded to float64). `cases` lists
the names. The table printed per case (plain against symmetrised float64 helper, and the smallest horizon at
which the plain one is off by more than 1e-6 of the scale) is the one of DESIGN.md §3.

Cases:
* di_solved — BoxProblem("double_integrator", "conf"), the fifth oe.reset of random.Random(2), zero warm
  start, SOLVE_CFG: CONVERGED after 281 iterations, Te = 192.
* di_maxiter — the eighth reset of the same generator: MAXITER after 400 iterations, Te = 163 (the longest
  of that family's first twelve that the numpy solver finishes in about a minute). Unconverged trajectories
  are what accept_maxiter keeps; there Q_u != 0 carries the V_xx error into the labels.
* rand_<system> — one random-control episode per system (controls uniform in +-1.2 u_max) clamped to the
  bounds by ddp_box_ref.clamped_episodes, of the conf's full length NSTEPS (the car: 200 of its 500, the
  length limit of the GPU test), seed: RANDOM_CASES, the first seed >= 21 that ddp_box_ref.label_inputs_ok
  accepts with the held sets and margin of the 80-digit pass.
"""
import os
import random
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import ddp_box_ref as D  # noqa: E402
import ddp_mp_ref as MP  # noqa: E402
import ilqr_box as X  # noqa: E402
import ilqr_ref as R  # noqa: E402

OUT = os.path.join(HERE, "label_long.npz")
MAX_T = 200                                     # the GPU test's limit on an episode's length
# (system, bounds kind) -> seed of the random clamped episode
RANDOM_CASES = {("single_integrator", "conf"): 21, ("double_integrator", "conf"): 21, ("car", "conf"): 21,
                ("car_park", "conf"): 21, ("manipulator", "conf"): 21, ("ur5", "conf"): 21}
# name -> (index of the reset of random.Random(2), expected status, iterations, Te)
SOLVED_CASES = {"di_solved": (4, R.CONVERGED, 281, 192), "di_maxiter": (7, R.MAXITER, 400, 163)}


def solved_episode(name):
    k, status, iters, Te = SOLVED_CASES[name]
    P = X.BoxProblem("double_integrator", "conf")
    rng = random.Random(2)
    s0 = np.asarray([P.oe.reset(rng) for _ in range(k + 1)][k], dtype=np.float64)
    T = P.conf.NSTEPS - int(s0[-1] / P.conf.dt)
    r = P.solve(s0, np.zeros((T, P.m)), T)
    assert (r["status"], r["iters"], T) == (status, iters, Te), (name, r["status"], r["iters"], T)
    return P, r["S"], r["U"]


def random_episode(system, kind, seed):
    P = X.BoxProblem(system, kind)
    conf = P.conf
    T = min(int(conf.NSTEPS), MAX_T)
    rng = random.Random(seed)
    S = np.zeros((1, T + 1, conf.nb_state))
    U = np.zeros((1, T + 1, conf.nb_action))
    S[0, 0] = P.oe.reset(rng)
    S[0, 0, -1] = (conf.NSTEPS - T) * conf.dt
    for t in range(T):
        U[0, t] = [rng.uniform(-1.2, 1.2) * conf.u_max[i] for i in range(conf.nb_action)]
    S, U = D.clamped_episodes(P, S, U, np.array([T]))
    return P, S[0], U[0, :T]


def reference(P, S, U):
    """The 80-digit labels of both passes and the rule's counts from the bounded one."""
    rec, lxT, lxxT, Uc = MP.episode_records(P.conf, S, U)
    Vb, held, margin, vxx_b = MP.riccati_mp(rec, lxT, lxxT, Uc, P.lo, P.hi)
    Vu, _, _, vxx_u = MP.riccati_mp(rec, lxT, lxxT, Uc, -np.inf, np.inf)
    on = (Uc <= P.lo) | (Uc >= P.hi)
    st = dict(held=int(held.sum()), on_free=int((on & ~held).sum()), inside=int((~on).sum()), margin=margin)
    return Vb, Vu, st, (vxx_b, vxx_u)


def helper_vxx_max(P, S, U, bounded, symmetrize):
    """max|V_xx| of the float64 recursion: the helpers return V_x only, so the recursion over the records."""
    rec, lxT, lxxT, Uc = MP.episode_records(P.conf, S, U)
    n, m = P.n, P.m
    lo, hi = (P.lo, P.hi) if bounded else (np.full(m, -np.inf), np.full(m, np.inf))
    Vx, Vxx, big = lxT, lxxT, 0.0
    with np.errstate(all="ignore"):
        for i in range(len(Uc) - 1, -1, -1):
            A, B = rec["A"][i], rec["B"][i]
            Qx, Qu = rec["l_x"][i] + A.T @ Vx, rec["l_u"][i] + B.T @ Vx
            Qxx, Quu, Qxu = rec["l_xx"][i] + A.T @ Vxx @ A, rec["l_uu"][i] + B.T @ Vxx @ B, A.T @ Vxx @ B
            Qbar = Quu + 1e-9 * np.identity(m)
            free = np.flatnonzero(~D.held_set(Uc[i], Qu, lo, hi)[0])
            if len(free):
                try:
                    Qi = np.linalg.inv(Qbar[np.ix_(free, free)])
                except np.linalg.LinAlgError:
                    return np.inf
                Vx = Qx - Qxu[:, free] @ Qi @ Qu[free]
                Vxx = Qxx - Qxu[:, free] @ Qi @ Qxu[:, free].T
            else:
                Vx, Vxx = Qx, Qxx
            if symmetrize:
                Vxx = 0.5 * (Vxx + Vxx.T)
            big = max(big, float(np.abs(Vxx).max()) if np.isfinite(Vxx).all() else np.inf)
    return big


def table_rows(name, P, S, U, Vb, Vu, vxx_mp):
    """The amplification table of DESIGN.md: per pass, plain against symmetrised float64 helper."""
    rows = []
    for tag, V, bounded, vmp in (("bounded", Vb, True, vxx_mp[0]), ("unbounded", Vu, False, vxx_mp[1])):
        for sym in (False, True):
            try:
                e = MP.amplification(P.conf, S, U, V, P.lo if bounded else None, P.hi, symmetrize=sym)
            except np.linalg.LinAlgError:
                e = np.full(len(V), np.inf)
            h = MP.first_failing_horizon(e)
            rows.append("%-22s T=%3d %-9s %-5s >1e-9 %5.1f%%  >1e-6 %5.1f%%  worst %8.1e  max|V_xx| %8.1e (mp %8.1e)  "
                        "first horizon >1e-6: %s" % (name, len(U), tag, "sym" if sym else "plain", 100 * (e > 1e-9).mean(),
                                                     100 * (e > 1e-6).mean(), e.max(), helper_vxx_max(P, S, U, bounded, sym),
                                                     vmp, "none up to %d" % len(U) if h is None else h))
    return rows


def build():
    out, names = {}, []
    episodes = [(name,) + solved_episode(name) for name in SOLVED_CASES]
    episodes += [("rand_" + system,) + random_episode(system, kind, seed) for (system, kind), seed in RANDOM_CASES.items()]
    for name, P, S, U in episodes:
        Vb, Vu, st, vxx_mp = reference(P, S, U)
        print(name, st, flush=True)
        if name.startswith("rand_"):
            assert D.label_inputs_ok(st), (name, st)
        else:
            assert st["margin"] >= 1e-6 and st["held"] >= 3, (name, st)
        for row in table_rows(name, P, S, U, Vb, Vu, vxx_mp):
            print("  " + row, flush=True)
        names.append(name)
        out.update({"system_" + name: np.array(P.system), "S_" + name: S, "U_" + name: U, "T_" + name: np.int32(len(U)),
                    "lo_" + name: P.lo, "hi_" + name: P.hi, "Vb_" + name: Vb, "Vu_" + name: Vu})
    out["cases"] = np.array(names)
    return out


def pick_seeds():
    for (system, kind) in RANDOM_CASES:
        for seed in range(21, 41):
            P, S, U = random_episode(system, kind, seed)
            st = reference(P, S, U)[2]
            print(system, kind, seed, st, D.label_inputs_ok(st), flush=True)
            if D.label_inputs_ok(st):
                break


def main():
    if "--seeds" in sys.argv:
        return pick_seeds()
    out = build()
    if "--check" in sys.argv:
        z = np.load(OUT)
        assert sorted(z.files) == sorted(out), (sorted(z.files), sorted(out))
        for k, v in out.items():
            assert np.asarray(v).tobytes() == z[k].tobytes() and np.asarray(v).shape == z[k].shape, k
        print("label_long.npz reproduced bit for bit")
    else:
        np.savez_compressed(OUT, **out)
        print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
