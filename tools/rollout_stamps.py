"""Diagnostic: cycles per step and phase of a rollout kernel, from the phase clock of the
CACTO_STAMPS build (RoClock in csrc/rollout_kernels.hip, where the phases are described). Not part
of the product path.

    python -c "from cacto_amd.build import build_variant; build_variant('libcacto_hip_stamps', ['CACTO_STAMPS'])"
    CACTO_HIP_LIB=cacto_amd/libcacto_hip_stamps.so python tools/rollout_stamps.py [system [R [groups,workgroups]]]

The table is [1024 workgroups][8 hardware waves][9 phases + the wave's step count], written by lane
0 of every wave of the last rollout launch. k_rollout has waves 0-3; k_rollout_tt's team is wave >> 2
and its dynamics wave is wave 0 (team 0) or 7 (team 1); every wave of k_rollout_ks runs a slot.
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cacto_amd import _lib as L  # noqa: E402
import bench  # noqa: E402

PHASES = ["L1", "L2", "L3", "DYN", "STEP", "STORE", "REFILL", "X0", "BAR"]
WGS, WAVES, COLS = 1024, 8, len(PHASES) + 1


def clock_table(entry="cacto_debug_rollout_stamps"):
    acc = (ctypes.c_ulonglong * (WGS * WAVES * COLS))()
    getattr(L.lib().dll, entry)(acc)
    return np.array(acc[:], dtype=np.float64).reshape(WGS, WAVES, COLS)


def report(system, R, sched, entry="cacto_debug_rollout_stamps"):
    conf, env, rl = bench.make_learner(system)
    S0, n = bench.initial_states(env, conf, R, seed=0)
    T = int(n.max())
    inputs = rl.rollout_inputs(S0, n)
    plan = rl.rollout_plan(R, sched)
    for _ in range(3):
        rl.rollout_batch(None, None, T, inputs=inputs, want=("S", "A"), sched=sched)
    torch.cuda.synchronize()
    a = clock_table(entry)[:plan["workgroups"], :plan["block_threads"] // 64]
    print(system, R, "sched", sched, "plan", plan)
    print("   wave  steps  cycles/step  " + "  ".join("%6s" % p for p in PHASES))
    for w in range(a.shape[1]):
        steps = a[:, w, -1].sum()
        per = a[:, w, :-1].sum(axis=0) / max(steps, 1)
        print("   %4d %6d  %11.0f  " % (w, steps, per.sum()) + "  ".join("%6.0f" % x for x in per))


if __name__ == "__main__":
    system = sys.argv[1] if len(sys.argv) > 1 else "double_integrator"
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
    sched = tuple(int(x) for x in sys.argv[3].split(",")) if len(sys.argv) > 3 else (0, 0)
    report(system, R, sched)
