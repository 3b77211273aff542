"""Diagnostic: K = 5 learner updates on seeded rows at every route of the update calls, with the
state they leave (net buffers = weights + packed copies, Adam moments, target, step counters; the PER
trees for the PER cases), and the PER entries alone at every route of cacto_per_plan (by shape),
saved to an .npz, for bit-for-bit comparison of two library builds (CACTO_HIP_LIB;
CACTO_LIB_PARTIAL=1 for a library of an older revision, where an entry the library lacks is skipped
and named in the output). Not part of the product path.

    CACTO_HIP_LIB=cacto_amd/libA.so python tools/upd_bits.py a.npz
    CACTO_HIP_LIB=cacto_amd/libB.so python tools/upd_bits.py b.npz
    python tools/upd_bits.py --compare a.npz b.npz     # prints the number of arrays compared
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = 5
# (name, system, critic_type, B, w_S, PER): DI across the routes (paired q4; k_wgrad + k_adam<16>;
# both networks on k_wgrad_big; xcd_tiles; the looped k_adam<0>), a w_S = 0 system, the elu critic
# (k_wgrad only), and the overlapped PER form (k_wgrad_big_per, k_adam_sample)
CASES = [("di%d" % B, "double_integrator", "sine", B, 1e-2, False) for B in (128, 513, 1025, 4096, 8193)] + [
    ("manip64", "manipulator", "sine", 64, 0.0, False),
    ("di_elu528", "double_integrator", "elu", 528, 1e-2, False),
    ("carpark_per4096", "car_park", "sine", 4096, 0.0, True),
    # the PER loop by shape: one workgroup; the multi-workgroup kernels paired; overlap_shape 0
    ("carpark_per64", "car_park", "sine", 64, 0.0, True),
    ("carpark_per512", "car_park", "sine", 512, 0.0, True),
    ("carpark_per4096_cap17", "car_park", "sine", 4096, 0.0, 2 ** 17)]


def compare(pa, pb):
    """Number of arrays compared and of arrays that differ (by bit pattern: NaN payloads too)."""
    za, zb = np.load(pa), np.load(pb)
    only = sorted(set(za.files) ^ set(zb.files))
    if only:    # an entry one of the libraries lacks (CACTO_LIB_PARTIAL=1): compared where both ran it
        print("in one file only (not compared): %d arrays, e.g. %s" % (len(only), only[0]))
    bad = []
    for key in sorted(set(za.files) & set(zb.files)):
        a, b = za[key], zb[key]
        bits = {8: np.uint64, 4: np.uint32}[a.dtype.itemsize]
        if not (a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(bits), b.view(bits))):
            bad.append(key)
    return len(set(za.files) & set(zb.files)), bad


def run_case(system, critic_type, B, w_S, per):
    import torch
    from cacto_amd.confs import load_conf
    from cacto_amd.environment import make_env
    from cacto_amd.neural_network import NN
    from cacto_amd.rl import RL_AC
    conf = load_conf(system, fresh=True)
    conf.critic_type = critic_type
    if per:
        conf.prioritized_replay_alpha = 0.6
        if per is not True:
            conf.REPLAY_SIZE = per
    env = make_env(conf)
    rl = RL_AC(env, NN(env, conf, w_S=w_S, seed=4), conf)
    rl.setup_model()
    ns = conf.nb_state
    rng = np.random.default_rng(23)
    N = 8192
    S = np.column_stack([rng.uniform(-3, 3, (N, ns - 1)), rng.uniform(0, 4.9, N)])
    rows = np.concatenate([S, rng.normal(size=(N, 1)), S + 0.01, rng.normal(size=(N, ns)) * 0.3,
                           (rng.uniform(size=(N, 1)) < 0.1).astype(float), np.zeros((N, 1))], axis=1)
    out = {}
    if per:
        from cacto_amd.replay_buffer import PrioritizedReplayBuffer
        buf = PrioritizedReplayBuffer(conf, env.sys)
        buf.add_rows(rows)
        rl.update_rows_n_per(buf, torch.as_tensor(rng.uniform(size=(K, B)), device="cuda"))
        out = {k: getattr(buf, k) for k in ("sum_tree", "min_tree", "exp_counter", "max_priority")}
    else:
        idx = torch.as_tensor(rng.integers(0, N, size=(K, B)).astype(np.int32), device="cuda")
        rl.update_rows_n(torch.as_tensor(rows, device="cuda"), idx)
    torch.cuda.synchronize()
    rl.check_pipeline()
    out.update(actor=rl.actor_model.buf, critic=rl.critic_model.buf, target=rl.target_critic.buf, actor_m=rl.actor_m,
               actor_v=rl.actor_v, critic_m=rl.critic_m, critic_v=rl.critic_v, steps=rl.steps)
    return {k: v.cpu().numpy() for k, v in out.items()}


def pack(t):
    """A tensor as a numpy array; a large one (the 2^21- and 2^22-leaf trees) as its SHA-256."""
    import hashlib
    a = t.cpu().numpy()
    if a.nbytes <= 1 << 22:
        return a
    return np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint32).copy()


def per_entry_cases():
    """The PER entries alone on seeded trees, every route of cacto_per_plan reached by shape."""
    import torch
    from cacto_amd import _lib as L
    from cacto_amd.system import dptr, stream
    lib, out, skipped = L.lib(), {}, []

    def trees(cap, rows, seed):
        rng = np.random.default_rng(seed)
        leaves = np.zeros(cap)
        leaves[:rows] = rng.uniform(0.01, 2.0, size=rows) ** 0.6
        st, mt = np.zeros(2 * cap), np.full(2 * cap, np.inf)
        st[cap:], mt[cap:] = leaves, np.where(leaves > 0, leaves, np.inf)
        lo = cap // 2
        while lo >= 1:
            k = np.arange(lo, 2 * lo)
            st[k] = st[2 * k] + st[2 * k + 1]
            mt[k] = np.where(mt[2 * k + 1] < mt[2 * k], mt[2 * k + 1], mt[2 * k])
            lo //= 2
        cnt = rng.integers(0, 5, size=cap).astype(np.float64)
        return [torch.as_tensor(x, device="cuda") for x in (st, mt, cnt)], rng

    for cap in (1 << 16, 1 << 20):
        for B in (64, 1000):
            rows = cap - 5
            (sd, md, cnt), rng = trees(cap, rows, cap + B)
            u = torch.as_tensor(rng.uniform(size=B), device="cuda")
            stats = torch.as_tensor(np.array([[3.0, 0.01, 100.0], [0, 0, rows], [7.0, 0.02, 50.0]]), device="cuda")
            lib.call("cacto_per_shard_stats", dptr(sd), dptr(md), rows, dptr(stats[1]), stream())
            for entry in ("cacto_per_sample", "cacto_per_sample_global", "cacto_per_sample_runs"):
                if not hasattr(lib.dll, entry):
                    skipped.append("%s cap=%d B=%d" % (entry, cap, B))
                    continue
                idx = torch.empty(B, dtype=torch.int32, device="cuda")
                w = torch.empty(B, dtype=torch.float32, device="cuda")
                c = cnt.clone()
                head = (dptr(sd), dptr(md), cap, rows, 0.6, dptr(u), B)
                res = {}
                if entry == "cacto_per_sample":
                    lib.call(entry, *head, dptr(idx), dptr(w), dptr(c), stream())
                elif entry == "cacto_per_sample_global":
                    lib.call(entry, *head, dptr(stats), 3, dptr(idx), dptr(w), dptr(c), stream())
                else:
                    nsub = cap // L.PER_RUN_SUB
                    runs = torch.cat([torch.full((nsub,), L.PER_RUN_EMPTY, dtype=torch.int32),
                                      torch.zeros(nsub, dtype=torch.int32)]).cuda()
                    lib.call(entry, *head, dptr(idx), dptr(w), dptr(c), dptr(runs), None, 0, stream())
                    res["runs"] = runs
                res.update(idx=idx, w=w, cnt=c)
                for k, v in res.items():
                    out["%s_c%d_b%d.%s" % (entry[6:], cap, B, k)] = pack(v)
    for cap in (1 << 16, 1 << 21, 1 << 22):
        for n in (64, 1024):
            rows = 50000
            for kind in ("update", "relo", "leaves"):
                (sd, md, cnt), rng = trees(cap, rows, cap + n)
                idx = torch.as_tensor(np.sort(rng.integers(0, rows, size=n)).astype(np.int32), device="cuda")
                if kind == "leaves":    # an unsorted list with duplicates
                    idx = torch.as_tensor(rng.integers(0, 300, size=n).astype(np.int32), device="cuda")
                y, V, Vt = (torch.as_tensor(rng.normal(size=n).astype(np.float32), device="cuda") for _ in range(3))
                mp = torch.ones(1, dtype=torch.float64, device="cuda")
                if kind == "update":
                    lib.call("cacto_per_update", dptr(sd), dptr(md), cap, dptr(idx), dptr(y), dptr(V), dptr(cnt), 0.95,
                             1e-2, 0.6, dptr(mp), n, stream())
                elif kind == "relo":
                    ws = torch.empty(n, dtype=torch.float64, device="cuda")
                    status = torch.zeros(1, dtype=torch.int32, device="cuda")
                    lib.call("cacto_per_update_relo", dptr(sd), dptr(md), cap, dptr(idx), dptr(y), dptr(V), dptr(Vt),
                             dptr(cnt), 0.95, 1e-2, 0.6, dptr(mp), dptr(ws), dptr(status), n, stream())
                else:
                    vals = torch.as_tensor(rng.uniform(0.01, 2.0, size=n), device="cuda")
                    lib.call("cacto_per_set_leaves", dptr(sd), dptr(md), cap, dptr(idx), dptr(vals), n, stream())
                for k, v in (("sum", sd), ("min", md), ("leaves", sd[cap:cap + rows]), ("max_priority", mp)):
                    out["per_%s_c%d_n%d.%s" % (kind, cap, n, k)] = pack(v)
    torch.cuda.synchronize()
    return out, skipped


def main():
    if sys.argv[1] == "--compare":
        arrays, bad = compare(sys.argv[2], sys.argv[3])
        print("arrays compared: %d, differing: %d %s" % (arrays, len(bad), bad if bad else ""))
        sys.exit(1 if bad else 0)
    res = {}
    for name, system, critic_type, B, w_S, per in CASES:
        for k, v in run_case(system, critic_type, B, w_S, per).items():
            res["%s.%s" % (name, k)] = v
        print("ran", name, flush=True)
    per, skipped = per_entry_cases()
    res.update(per)
    print("ran the PER entries; skipped (absent from this library): %s" % (skipped or "none"), flush=True)
    np.savez(sys.argv[1], **res)
    print("saved", sys.argv[1], "arrays:", len(res))


if __name__ == "__main__":
    main()
