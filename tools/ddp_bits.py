"""Diagnostic: every entry of the DDP layer (the label pass, the jacobians, the optimiser's backward
gains and its solvers) on one small batch per system, saved to an .npz, for bit-for-bit comparison
of two library builds (CACTO_HIP_LIB) or of two settings of CACTO_DDP_SPLIT. Not part of the
product path.

    CACTO_HIP_LIB=cacto_amd/libA.so python tools/ddp_bits.py a.npz [system,system,...]
    CACTO_HIP_LIB=cacto_amd/libB.so python tools/ddp_bits.py b.npz [system,system,...]
    python tools/ddp_bits.py --compare a.npz b.npz    # prints the number of arrays compared

Per system: 70 episodes (past a wave of the one-thread kernels) of 0, 1 and up to 12 steps and one
dropped one (nsteps = -1), trajectories of the oracle's Env.simulate under random controls up to
1.2 u_max. Entries: cacto_ddp_backward; cacto_ddp_backward_box under the conf's bounds, along the
controls clamped to them (the share of controls on a limit and of episodes whose labels the bounds
change are printed); cacto_env_jacobians on the 70 first nodes; cacto_to_backward_gains for
{exact, psd} x {no bounds, conf bounds} x mu in {0, 1e-3}; cacto_to_solve on both paths for
{exact, psd} x {no bounds, conf bounds} with max_iter = 5. --compare counts the arrays that differ
by bit pattern over the rows each episode owns, over the arrays both files hold.

Against a build from before the label recursion symmetrised V_xx per node (ddp_kernels.hip's header) the
dVdx arrays of cacto_ddp_backward and cacto_ddp_backward_box, and those of cacto_to_solve, which end with
the same label pass, differ by design from the second step of an episode on (by rounding at these
lengths); the jacobians, the gains and the solvers' trajectories must not."""
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SYSTEMS = ("single_integrator", "double_integrator", "car", "car_park", "manipulator", "ur5")
N_EP, MAX_STEPS = 70, 12
# rows an episode of n steps owns, by the array's name: n + ROWS[name]; the others are per episode
ROWS = {"dVdx": 1, "k": 0, "K": 0, "S": 1, "U": 0, "step_cost": 1}


def compare(pa, pb):
    """Number of arrays both files hold and of those that differ, over the rows each episode owns."""
    za, zb = np.load(pa), np.load(pb)
    keys = sorted(set(za.files) & set(zb.files))
    arrays = bad = 0
    for key in keys:
        a, b = za[key], zb[key]
        system, name = key.split("/")[0], key.split("/")[-1]
        if name == "n":
            assert np.array_equal(a, b), key
            continue
        arrays += 1
        same = a.shape == b.shape and a.dtype == b.dtype
        if same and name in ROWS:
            n = za[system + "/n"].astype(np.int64)
            own = np.arange(a.shape[1])[None, :] < (n + ROWS[name])[:, None]      # [episode, row]
            a, b = a[own], b[own]
        if same:
            bits = {8: np.uint64, 4: np.uint32}[a.dtype.itemsize]                 # NaN payloads too
            same = np.array_equal(np.ascontiguousarray(a).view(bits), np.ascontiguousarray(b).view(bits))
        if not same:
            print("differs:", key)
        bad += not same
    only = len(set(za.files) ^ set(zb.files))
    return arrays, bad, only


def episodes(conf, oe, rng):
    """S [E, 13, ns], U [E, 12, na], n [E]: as tests/test_gpu_ddp.py::_episodes, with lengths 0, 1, ..
    12 and one dropped episode."""
    ns, na = conf.nb_state, conf.nb_action
    n = np.array([rng.choice((0, 1, 2, 3, 5, 8, 11, MAX_STEPS)) for _ in range(N_EP)], dtype=np.int32)
    n[:4] = (MAX_STEPS, 0, 1, MAX_STEPS - 1)
    S = np.zeros((N_EP, MAX_STEPS + 1, ns))
    U = np.zeros((N_EP, MAX_STEPS, na))
    for e in range(N_EP):
        S[e, 0] = oe.reset(rng)
        for t in range(int(n[e])):
            U[e, t] = [rng.uniform(-1.2, 1.2) * conf.u_max[i] for i in range(na)]
            S[e, t + 1] = oe.simulate(S[e, t], U[e, t])
    n[9] = -1                                     # a dropped episode: every entry skips it
    return S, U, n


def run_system(system, res):
    import torch
    from cacto_amd.confs import load_conf
    from cacto_amd.environment import make_env
    from cacto_amd.to import TO
    from oracle import env as oenv
    conf = load_conf(system)
    env = make_env(conf)
    to = TO(env, conf, w_S=1e-2)
    S, U, n = episodes(conf, oenv.make_env(conf), random.Random(5))
    lo, hi = np.asarray(conf.u_min, dtype=np.float64), np.asarray(conf.u_max, dtype=np.float64)
    Uc = np.minimum(np.maximum(U, lo), hi)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731
    S_d, U_d, Uc_d, n_d = dev(S), dev(U), dev(Uc), dev(n)

    def put(name, v):
        res["%s/%s" % (system, name)] = v.cpu().numpy() if hasattr(v, "cpu") else v

    put("n", n)
    plain = to.backward_pass_batch(S_d, U_d, n_d)
    put("labels/dVdx", plain)
    box = to.backward_pass_batch(S_d, Uc_d, n_d, bounds="conf")
    put("labels_box/dVdx", box)
    live = np.arange(MAX_STEPS)[None, :, None] < n[:, None, None]
    on = float((((Uc <= lo) | (Uc >= hi)) & live).sum()) / max(float(live.sum()) * conf.nb_action, 1.0)
    changed = int((box != to.backward_pass_batch(S_d, Uc_d, n_d)).any(dim=2).any(dim=1).sum().item())
    print("%s: %.1f%% of the clamped controls on a limit; the bounds hold some in %d of %d episodes (their labels "
          "differ from the unbounded pass's)" % (system, 100.0 * on, changed, N_EP))
    Fx, Fu = env.augmented_derivative_batch(S_d[:, 0].contiguous(), U_d[:, 0].contiguous())
    put("jac/Fx", Fx)
    put("jac/Fu", Fu)
    for hess in ("exact", "psd"):
        for bounds in ("none", "conf"):
            for mu in (0.0, 1e-3):
                g = to.backward_gains_batch(S_d, Uc_d if bounds == "conf" else U_d, n_d, mu=mu, hessian=hess,
                                            bounds=bounds)
                for k, v in g.items():
                    put("gains_%s_%s_mu%g/%s" % (hess, bounds, mu, k), v)
            for path in ("default", "wave"):
                out = to.solve_batch(S_d[:, 0].contiguous(), 0.5 * U_d, n_d,
                                     cfg=dict(max_iter=5, path=path, hessian=hess, bounds=bounds))
                for k, v in out.items():
                    put("solve_%s_%s_%s/%s" % (path, hess, bounds, k), v)
    torch.cuda.synchronize()


def main():
    if sys.argv[1] == "--compare":
        arrays, bad, only = compare(sys.argv[2], sys.argv[3])
        print("arrays compared: %d, differing: %d (in one file only: %d)" % (arrays, bad, only))
        sys.exit(1 if bad else 0)
    res = {}
    for system in (sys.argv[2].split(",") if len(sys.argv) > 2 else SYSTEMS):
        run_system(system, res)
    np.savez(sys.argv[1], **res)
    print("saved %s (%d arrays)" % (sys.argv[1], sum(not k.endswith("/n") for k in res)))


if __name__ == "__main__":
    main()
