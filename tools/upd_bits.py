"""Diagnostic: K = 5 learner updates on seeded rows at every route of the update calls, with the
state they leave (net buffers = weights + packed copies, Adam moments, target, step counters; the PER
trees for the PER case) saved to an .npz, for bit-for-bit comparison of two library builds
(CACTO_HIP_LIB; CACTO_LIB_PARTIAL=1 for a library of an older revision). Not part of the product path.

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
    ("carpark_per4096", "car_park", "sine", 4096, 0.0, True)]


def compare(pa, pb):
    """Number of arrays compared and of arrays that differ (by bit pattern: NaN payloads too)."""
    za, zb = np.load(pa), np.load(pb)
    assert sorted(za.files) == sorted(zb.files), "the two files hold different arrays"
    bad = []
    for key in za.files:
        a, b = za[key], zb[key]
        bits = {8: np.uint64, 4: np.uint32}[a.dtype.itemsize]
        if not (a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(bits), b.view(bits))):
            bad.append(key)
    return len(za.files), bad


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
    np.savez(sys.argv[1], **res)
    print("saved", sys.argv[1], "arrays:", len(res))


if __name__ == "__main__":
    main()
