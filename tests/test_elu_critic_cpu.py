"""critic_type 'elu' (NeuralNetwork.py:65-78: Dense 16, 32, 256, 256 with elu, then Dense 1) without a
GPU: the oracle's gradients at this shape against finite differences (the step, tolerances and
coordinate sampling of tests/test_oracle_math.py, which pins them for the sine widths), the host
layer's shapes and initialisers, and the .h5 layer names of the reference's elu models."""
import numpy as np
import pytest

from elu_cases import ELU, elu_shapes, preact_margin
from oracle import nn as onn
from cacto_amd import h5
from cacto_amd import neural_network as gnn


def _rand_params(rng, shapes, scale=0.3):
    return [rng.normal(scale=scale, size=s) for s in shapes]


@pytest.mark.parametrize("w_S", [0.0, 1e-2])
def test_critic_grad_fd_elu_widths(w_S):
    rng = np.random.default_rng(0)
    ns, B = 5, 6
    norm = np.array([15., 15., 6., 6., 10.])
    crit = _rand_params(rng, elu_shapes(ns))
    tgt = _rand_params(rng, elu_shapes(ns))
    S = rng.uniform(-10, 10, size=(B, ns)); S[:, -1] = rng.uniform(0, 9, size=B)
    Sn = rng.uniform(-10, 10, size=(B, ns))
    R = rng.normal(size=(B, 1)); d = (rng.uniform(size=(B, 1)) < .4) * 1.0
    dVdx = rng.normal(size=(B, ns)); w = rng.uniform(.5, 2, size=(B, 1))
    # a finite difference across the elu kink is no derivative: the step must stay on one side
    assert preact_margin(crit, S, norm)[0] > 100 * 1e-6
    grads = onn.compute_critic_grad(crit, tgt, S, Sn, R, dVdx, d, w, w_S, norm, acts=ELU)[0]
    assert [g.shape for g in grads] == elu_shapes(ns)
    f = lambda P: onn.critic_loss(P, tgt, S, Sn, R, dVdx, d, w, w_S, norm, acts=ELU)
    eps = 1e-6
    for li, (p, g) in enumerate(zip(crit, grads)):
        flat = p.reshape(-1)
        for k in rng.choice(flat.size, size=min(6, flat.size), replace=False):
            old = flat[k]
            flat[k] = old + eps; fp = f(crit)
            flat[k] = old - eps; fm = f(crit)
            flat[k] = old
            fd = (fp - fm) / (2 * eps)
            assert abs(fd - g.reshape(-1)[k]) <= 1e-6 * max(1.0, abs(fd)), (li, k, fd, g.reshape(-1)[k])


def test_critic_input_grad_fd_elu_widths():
    rng = np.random.default_rng(1)
    ns = 7
    norm = np.array([15., 15., 15., 10., 10., 10., 5.])
    crit = _rand_params(rng, elu_shapes(ns))
    S = rng.uniform(-3, 3, size=(4, ns))
    assert preact_margin(crit, S, norm)[0] > 100 * 1e-6
    g, _ = onn.critic_input_grad(crit, S, norm, acts=ELU)
    eps = 1e-6
    for j in range(ns):
        Sp, Sm = S.copy(), S.copy()
        Sp[:, j] += eps; Sm[:, j] -= eps
        fd = (onn.critic_forward(crit, Sp, norm, acts=ELU) - onn.critic_forward(crit, Sm, norm, acts=ELU))[:, 0] / (2 * eps)
        np.testing.assert_allclose(g[:, j], fd, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize("ns,na", [(3, 2), (5, 2), (13, 6)])
def test_layer_shapes_and_param_count(ns, na):
    shapes = gnn.layer_shapes(gnn.CRITIC, ns, na, "elu")
    assert shapes == elu_shapes(ns)
    assert sum(int(np.prod(s)) for s in shapes) == 16 * ns + 75057
    # the other critic types and the actor keep their shapes
    sine = [(ns, 64), (64,), (64, 64), (64,), (64, 128), (128,), (128, 128), (128,), (128, 1), (1,)]
    assert gnn.layer_shapes(gnn.CRITIC, ns, na) == sine == gnn.layer_shapes(gnn.CRITIC, ns, na, "sine-elu")
    assert gnn.layer_shapes(gnn.ACTOR, ns, na, "elu") == [(ns, 256), (256,), (256, 256), (256,), (256, na), (na,)]


def test_init_weights_glorot_uniform_zero_bias():
    ns, na = 5, 2
    ws = gnn.init_weights(gnn.CRITIC, ns, na, np.random.default_rng(7), critic_acts=ELU)
    assert [w.shape for w in ws] == elu_shapes(ns) and all(w.dtype == np.float32 for w in ws)
    for li in range(0, 10, 2):
        fi, fo = ws[li].shape
        lim = np.sqrt(6.0 / (fi + fo))
        assert np.abs(ws[li]).max() <= lim
        if ws[li].size >= 512:  # a uniform draw fills its range: the largest of n draws is within a few lim / n
            assert np.abs(ws[li]).max() > lim * (1 - 20.0 / ws[li].size)
        assert not ws[li + 1].any()
    # the sine critic's initialiser is unchanged by the elu shape
    assert [w.shape for w in gnn.init_weights(gnn.CRITIC, ns, na, np.random.default_rng(7))][0] == (ns, 64)


def test_h5_round_trip_under_elu_layer_names(tmp_path):
    """Keras numbers Dense layers in creation order across actor, critic and target (RL.py:52-76)."""
    assert gnn.LAYER_NAMES_ELU == {"actor": ["dense", "dense_1", "dense_2"],
                                   "critic": ["dense_%d" % k for k in range(3, 8)],
                                   "target": ["dense_%d" % k for k in range(8, 13)]}
    rng = np.random.default_rng(8)
    for role in ("critic", "target"):
        ws = [w.astype(np.float32) for w in _rand_params(rng, elu_shapes(5))]
        names = gnn.LAYER_NAMES_ELU[role]
        p = str(tmp_path / (role + ".h5"))
        h5.write_keras_weights(p, [(n, [(n + "/kernel:0", ws[2 * i]), (n + "/bias:0", ws[2 * i + 1])])
                                   for i, n in enumerate(names)])
        got = h5.read_keras_weights(p)  # in layer_names order, not sorted: dense_10 follows dense_9
        assert len(got) == 10 and all(np.array_equal(a, b) for a, b in zip(got, ws))
        with open(p, "rb") as f:
            hf = h5.H5File(f.read())
        assert h5._strings(hf.attributes(hf.object(hf.root))["layer_names"]) == names
