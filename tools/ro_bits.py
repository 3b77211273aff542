"""Diagnostic: one rollout batch of a system (bench.py's initial states and weights) under a
schedule, with S, A, R, EE and status saved to an .npz, for bit-for-bit comparison of two library
builds (CACTO_HIP_LIB; CACTO_LIB_PARTIAL=1 for a library of an older revision). Not part of the
product path.

    CACTO_HIP_LIB=cacto_amd/libA.so python tools/ro_bits.py ur5 2048 a.npz [groups,workgroups [ep]]
    CACTO_HIP_LIB=cacto_amd/libB.so python tools/ro_bits.py ur5 2048 b.npz [groups,workgroups [ep]]
    python tools/ro_bits.py --compare a.npz b.npz     # prints the number of arrays compared
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS = {"S": 1, "A": 0, "R": 0, "EE": 1}     # rows an episode of n steps owns: n + ROWS[key]


def compare(pa, pb):
    """Number of arrays compared and of arrays that differ, over the rows each episode owns."""
    za, zb = np.load(pa), np.load(pb)
    a, b = {k: za[k] for k in za.files}, {k: zb[k] for k in zb.files}
    n = a["n"].astype(np.int64)
    assert np.array_equal(n, b["n"])
    arrays = bad = 0
    for key in ("S", "A", "R", "EE", "status"):
        if key not in a and key not in b:
            continue
        arrays += 1
        if key == "status":
            same = np.array_equal(a[key], b[key])
        else:
            own = np.arange(a[key].shape[1])[None, :] < (n + ROWS[key])[:, None]      # [episode, row]
            bits = np.uint64 if a[key].dtype == np.float64 else np.uint32        # NaN payloads too
            same = (a[key].shape == b[key].shape and a[key].dtype == b[key].dtype and
                    np.array_equal(a[key][own].view(bits), b[key][own].view(bits)))
        bad += not same
    return arrays, bad


def main():
    if sys.argv[1] == "--compare":
        arrays, bad = compare(sys.argv[2], sys.argv[3])
        print("arrays compared: %d, differing: %d" % (arrays, bad))
        sys.exit(1 if bad else 0)
    import torch
    import bench
    system, R, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    sched = tuple(int(x) for x in sys.argv[4].split(",")) if len(sys.argv) > 4 else (0, 0)
    ep = int(sys.argv[5]) if len(sys.argv) > 5 else 1
    conf, env, rl = bench.make_learner(system)
    S0, n = bench.initial_states(env, conf, R, seed=0)
    T = int(n.max())
    res = rl.rollout_batch(S0, n, T, ep=ep, sched=sched)
    torch.cuda.synchronize()
    np.savez(out, n=np.asarray(n), **{k: v.cpu().numpy() for k, v in res.items()})
    print("saved", out)


if __name__ == "__main__":
    main()
