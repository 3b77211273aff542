"""Shared by the elu-critic tests (test_elu_critic_cpu.py, test_gpu_elu_critic.py): the weights,
replay rows and the input condition, all built on the CPU from fixed seeds.

Input condition (asserted by `check_preacts` before a test touches the GPU): in the float64 oracle's
forward pass every hidden layer of the elu critic has pre-activations of both signs, and none within
1e-5 of zero — elu'' jumps at zero, so a float32 / float64 sign disagreement there is not a kernel
error. The seeds below were picked so that the oracle alone satisfies it at the tests' shapes."""
import numpy as np

from oracle import nn as onn
from cacto_amd.neural_network import ACTOR, CRITIC, init_weights

ELU = ("elu",) * 4
ELU_WIDTHS = (16, 32, 256, 256)
KINK = 1e-5


def elu_shapes(ns):
    dims = [ns] + list(ELU_WIDTHS) + [1]
    out = []
    for i, o in zip(dims[:-1], dims[1:]):
        out += [(i, o), (o,)]
    return out


def make_weights(conf, seed):
    """Actor, critic and target in Keras order: the package's initialisers (Glorot-uniform kernels),
    with small non-zero biases so that no bias path is trivially zero, and a target of its own draw."""
    rng = np.random.default_rng(seed)
    ns, na = conf.nb_state, conf.nb_action
    out = {"actor": init_weights(ACTOR, ns, na, rng),
           "critic": init_weights(CRITIC, ns, na, rng, critic_acts=ELU),
           "target": init_weights(CRITIC, ns, na, rng, critic_acts=ELU)}
    for k in ("critic", "target"):
        for i in range(1, 10, 2):
            out[k][i] = rng.uniform(-0.2, 0.2, size=out[k][i].shape).astype(np.float32)
    return out


def make_rows(conf, B, rng):
    """Replay rows as tests/test_gpu_sine_elu.py builds them: [s, R, s', dVdx, d, term]."""
    ns = conf.nb_state
    lo, hi = np.array(conf.x_init_min, dtype=float), np.array(conf.x_init_max, dtype=float)
    S = rng.uniform(lo, hi, size=(B, ns))
    Sn = rng.uniform(lo, hi, size=(B, ns))
    return np.concatenate([S, rng.normal(size=(B, 1)) * 0.5, Sn, rng.normal(size=(B, ns)) * 0.3,
                           (rng.uniform(size=(B, 1)) < 0.3).astype(float),
                           (rng.uniform(size=(B, 1)) < 0.2).astype(float)], axis=1)


def split_rows(conf, rows):
    """replay_buffer.py:52-61 column split; the reference converts the sample to float32."""
    ns = conf.nb_state
    r = rows.astype(np.float32).astype(np.float64)
    return (r[:, :ns], r[:, ns:ns + 1], r[:, ns + 1:2 * ns + 1], r[:, 2 * ns + 1:3 * ns + 1],
            r[:, 3 * ns + 1:3 * ns + 2], rows[:, 3 * ns + 2:3 * ns + 3])


def preact_margin(critic, S, norm):
    """(min |z| over all hidden units and rows, every layer has both signs) in the oracle's forward."""
    zs = onn.critic_forward(critic, np.asarray(S, dtype=np.float64), norm, keep=True, acts=ELU)[1][1]
    both = all((z > 0).any() and (z < 0).any() for z in zs)
    return min(np.abs(z).min() for z in zs), both


def check_preacts(critic, S, norm):
    assert len(S) <= 48, "the input condition is picked for at most 48 rows x 560 units"
    margin, both = preact_margin(critic, S, norm)
    assert both, "a hidden layer's pre-activations have one sign only"
    assert margin > KINK, "a pre-activation within 1e-5 of the elu kink: %g" % margin


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)
