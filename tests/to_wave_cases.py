"""Test infrastructure: the inputs of the wave-path tests whose lengths straddle the 64-lane
stride of k_to_solve_wave (tests/test_gpu_to_wave.py, tools/to_wave_record.py)."""
import random

import numpy as np

from cacto_amd.confs import load_conf
from oracle import env as oenv

# one node short of / at / past one stride of the lanes (Te + 1 nodes: 64 -> 65), and a second stride
STRIDE_TE = (1, 2, 63, 64, 65, 100)
STRIDE_SEED = 5


def stride_inputs(system):
    """oracle.env.reset states (seed 5) with the time entry (NSTEPS - Te) dt, as ilqr_ref.solve_inputs
    sets it. Returns (S0 [6, ns], nsteps [6] int32)."""
    conf = load_conf(system)
    oe = oenv.make_env(conf)
    rng = random.Random(STRIDE_SEED)
    Te = np.array(STRIDE_TE, dtype=np.int32)
    S0 = np.array([oe.reset(rng) for _ in Te], dtype=np.float64)
    S0[:, -1] = (conf.NSTEPS - Te) * conf.dt
    return S0, Te
