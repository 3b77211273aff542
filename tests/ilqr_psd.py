"""Test infrastructure: tests/ilqr_ref.py's iLQR with the convexified node Hessian of the
trajectory optimiser's `hessian="psd"` mode. Every node's l_xx (cost convention) is replaced by its
projection onto the positive semidefinite cone, P(H) = V max(L, 0) V^T, through numpy.linalg.eigh
(LAPACK): nothing here shares code or method with the Jacobi iteration of
cacto_amd/csrc/psd_project.h. backward / solve / gradient are the parent class's.
"""
import numpy as np

import ilqr_ref as R

# random_episodes seeds of the gains test, picked on the CPU (tools/to_psd_record.py --seeds) as the
# first seed >= 21 at which the projection changes l_xx on some node of the batch and the helper's PD
# verdicts at mu = 0 and mu = 1 are decisive (|decisive| >= 1e-3, the rule of test_gpu_to_solve.py)
GAINS_SEEDS = {"single_integrator": 35, "double_integrator": 21, "car": 21, "car_park": 21, "manipulator": 21,
               "ur5": 21}


def psd(H):
    H = 0.5 * (H + H.T)
    w, V = np.linalg.eigh(H)
    P = (V * np.maximum(w, 0.0)) @ V.T
    return 0.5 * (P + P.T)


class PsdProblem(R.Problem):
    def lx(self, x, terminal=False):
        g, H = R.Problem.lx(self, x, terminal)
        return g, psd(H)

    def projection_change(self, S, T):
        """max over the nodes of one episode of |P(l_xx) - l_xx|_max / |l_xx|_max."""
        worst = 0.0
        for t in range(T + 1):
            H = R.Problem.lx(self, S[t], terminal=t == T)[1]
            worst = max(worst, np.abs(psd(H) - H).max() / max(np.abs(H).max(), 1e-300))
        return worst
