"""Diagnostic: cycles per step and phase of k_rollout_tt (groups -1) or, with 'ks', of k_rollout_ks
(groups -3) at 4096 episodes (CACTO_STAMPS build): tools/rollout_stamps.py under those schedules.
Not part of the product path.
    CACTO_HIP_LIB=cacto_amd/libcacto_hip_stamps.so python tools/tt_stamps.py [system] [ks]"""
import sys

from rollout_stamps import report

if __name__ == "__main__":
    system = sys.argv[1] if len(sys.argv) > 1 else "double_integrator"
    if len(sys.argv) > 2 and sys.argv[2] == "ks":
        report(system, 4096, (-3, 0), "cacto_debug_rollout_ws_acc")
    else:
        report(system, 4096, (-1, 0), "cacto_debug_rollout_tt_acc")
