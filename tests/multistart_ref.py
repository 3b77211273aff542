"""numpy restatements of the two multi-start entries (include/cacto_hip.h): the counter-based
generator and the candidate batch of cacto_to_starts, in 64-bit integer arithmetic, and the
selection rule of cacto_to_select. The library is built without contraction and the float steps are
stated one rounding at a time, so the device results are expected to equal these bit for bit."""
import numpy as np

CONVERGED, MAXITER, FAILED = 0, 1, 2
U64 = np.uint64


def mix(z):
    """splitmix64's output function of the state z (any uint64 array), modulo 2^64."""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=U64) + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def xi(seed, e, c, block, k):
    """xi in [-1, 1) of (seed, e, c, block, k); the last four broadcast."""
    e, c, block, k = (np.asarray(v, dtype=U64) for v in (e, c, block, k))
    packed = (e << U64(31)) | (block << U64(7)) | (c << U64(3)) | k
    h = mix(mix(np.array(int(seed) & 0xFFFFFFFFFFFFFFFF, dtype=U64)) ^ packed)
    return (h >> U64(11)).astype(np.float64) * 2.0 ** -52 - 1.0


def starts(S0, U_init, nsteps, N, sigma, hold, half_range, zero_start, seed):
    """cacto_to_starts: (S0_all [N E, ns], U_all [N E, ldU, na], nsteps_all [N E]), candidate-major."""
    E, ldU, na = U_init.shape
    U_all = np.empty((N, E, ldU, na))
    e = np.arange(E)[:, None, None]
    block = (np.arange(ldU) // hold)[None, :, None]
    k = np.arange(na)[None, None, :]
    scale = np.array([np.float64(sigma) * np.float64(h) for h in half_range])[None, None, :]
    for c in range(N):
        if c == 0:
            U_all[c] = U_init
        elif c == 1 and zero_start:
            U_all[c] = 0.0
        else:
            U_all[c] = U_init + scale * xi(seed, e, c, block, k)
    return (np.tile(S0, (N, 1)), U_all.reshape(N * E, ldU, na), np.tile(np.asarray(nsteps, dtype=np.int32), N))


def select(sol_all, nsteps, N, accept_maxiter, out):
    """cacto_to_select on numpy arrays: sol_all a dict S, U, step_cost, status, iters, J over N E rows,
    `out` the same dict over E rows holding the prefill. Returns a new dict: the six outputs and start,
    n_ok, J_starts, status_starts."""
    E = len(nsteps)
    res = {k: np.array(v) for k, v in out.items()}
    J_starts = sol_all["J"][:, 1].reshape(N, E).T.copy()
    status_starts = sol_all["status"].reshape(N, E).T.copy()
    ok = ((status_starts == CONVERGED) | (bool(accept_maxiter) & (status_starts == MAXITER))) & np.isfinite(J_starts)
    start = np.full(E, -1, dtype=np.int32)
    n_ok = np.zeros(E, dtype=np.int32)
    for e in range(E):
        Te = int(nsteps[e])
        if Te < 0:
            continue
        win = 0
        for c in range(N):                          # strict <: the lowest index wins a tie
            if ok[e, c] and (not ok[e, win] or J_starts[e, c] < J_starts[e, win]):
                win = c
        w = win * E + e
        start[e], n_ok[e] = win, ok[e].sum()
        res["S"][e, :Te + 1] = sol_all["S"][w, :Te + 1]
        res["U"][e, :Te] = sol_all["U"][w, :Te]
        res["step_cost"][e, :Te + 1] = sol_all["step_cost"][w, :Te + 1]
        res["status"][e], res["iters"][e] = sol_all["status"][w], sol_all["iters"][w]
        res["J"][e, 0], res["J"][e, 1] = sol_all["J"][e, 0], sol_all["J"][w, 1]
    res.update(start=start, n_ok=n_ok, J_starts=J_starts, status_starts=status_starts.astype(np.int32))
    return res
