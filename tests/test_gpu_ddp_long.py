"""GPU checks of the Sobolev labels (cacto_ddp_backward, cacto_ddp_backward_box) at full episode length,
against the label recursion at 80 digits (tests/ddp_mp_ref.py; fixture tests/golden/label_long.npz, one
episode of up to 200 steps per case). The parity tests of test_gpu_ddp.py and test_gpu_ddp_box.py stop at
24 steps and measure against a float64 helper that is itself wrong beyond ~60: without V_xx symmetrised
per node the solved double-integrator case here fails by many orders of magnitude.

Tolerance per row: RTOL * scale + MARGIN * err_sym(row), scale the episode's max|V_x| at 80 digits and
err_sym the symmetrised float64 helper's own error against the 80-digit labels on that row: what float64
can do on this trajectory, never what the kernel gives. err_sym <= RTOL * scale is asserted on every row, so
the tolerance cannot exceed 101 * RTOL * scale."""
import functools

import numpy as np
import pytest
import torch

import ddp_mp_ref as MP

pytestmark = pytest.mark.gpu

RTOL = 1e-9             # test_gpu_ddp.py's
MARGIN = 100.0          # the multiple of the reference's own rounding that test_gpu_ddp.py allows this pass


@functools.lru_cache(maxsize=None)
def _to(system):
    from cacto_amd.confs import load_conf
    from cacto_amd.environment import make_env
    from cacto_amd.to import TO
    conf = load_conf(system)
    return TO(make_env(conf), conf, w_S=1e-2)


def _labels(system, S, U, T, **kw):
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731
    out = _to(system).backward_pass_batch(dev(S), dev(U), dev(np.asarray(T, dtype=np.int32)), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _batch(c, extra=0):
    """[the case's episode, its first state as a Te = 0 episode, its episode again but skipped (nsteps = -1)]
    plus `extra` zero episodes; the arrays one step longer than the episode, as a replay batch would be."""
    T, ns, na = c["T"], c["S"].shape[1], c["U"].shape[1]
    S, U = np.zeros((3 + extra, T + 2, ns)), np.zeros((3 + extra, T + 2, na))
    S[0, :T + 1], U[0, :T] = c["S"], c["U"]
    S[1, 0] = c["S"][0]
    S[2, :T + 1], U[2, :T] = c["S"], c["U"]
    return S, U, np.array([T, 0, -1] + [0] * extra, dtype=np.int32)


def _check(case, bounded, got, e=0):
    """Episode e of `got` against the case's 80-digit labels. Returns the largest err / tol."""
    c = MP.long_cases()[case]
    T, n = c["T"], c["S"].shape[1] - 1
    ref = c["Vb"] if bounded else c["Vu"]
    scale = np.abs(ref[:, :n]).max()
    err_sym = MP.sym_error(case, bounded) * scale
    assert (err_sym <= RTOL * scale).all(), (case, bounded, float(err_sym.max() / scale))
    tol = RTOL * scale + MARGIN * err_sym
    assert np.isfinite(got).all(), (case, bounded)
    err = np.abs(got[e, :T + 1, :n] - ref[:, :n]).max(axis=1)           # every row, no row excluded
    worst = float((err / tol).max())
    print("%s %s: max err / tol = %.3g at row %d, max err / scale = %.3g" % (
        case, "bounded" if bounded else "unbounded", worst, int((err / tol).argmax()), float(err.max() / scale)))
    assert (err <= tol).all(), (case, bounded, worst)
    big = np.abs(got[e]).max()
    assert 0.5 * scale <= big <= 2.0 * scale, (case, bounded, big, scale)
    assert (got[e, :T + 1, n] == 0).all()                               # the time column
    assert (got[e, T + 1:] == 0).all()                                  # rows past Te untouched
    return worst


# ---------------------------------------------------------------------- 1. parity with the 80-digit labels
@pytest.mark.parametrize("case", MP.LONG_CASES)
def test_long_labels_match_the_80_digit_recursion(case):
    c = MP.long_cases()[case]
    S, U, T = _batch(c)
    n = S.shape[2] - 1
    plain = _labels(c["system"], S, U, T)
    boxed = _labels(c["system"], S, U, T, bounds=(c["lo"], c["hi"]))
    _check(case, False, plain)
    _check(case, True, boxed)
    assert not np.array_equal(plain[0], boxed[0])                       # the bounds took part
    for got in (plain, boxed):
        # Te = 0: the terminal gradient alone (the same under bounds); nsteps = -1: nothing written
        assert got[1, 0, :n].any() and (got[1, 1:] == 0).all() and got[1, 0, n] == 0
        assert (got[2] == 0).all()
    assert np.array_equal(plain[1], boxed[1])


# ---------------------------------------------------------------------- 2. the recursion only looks back
@pytest.mark.parametrize("case", ["di_solved", "rand_car", "rand_ur5"])
def test_a_tail_of_the_episode_gives_the_same_rows(case):
    """The last 70 nodes as an episode of their own (beside the whole one, a skipped and an empty one; the
    fused kernel's and the wave kernel's systems): its labels are the whole episode's last rows bit for bit,
    and so already past the horizon (~60) at which the unsymmetrised recursion fails."""
    c = MP.long_cases()[case]
    T, k = c["T"], 70
    S, U, Te = _batch(c, extra=1)
    S[3, :k + 1], U[3, :k], Te[3] = c["S"][T - k:], c["U"][T - k:], k
    order = [2, 0, 1, 3]                                                # skipped first, the tail last
    got = _labels(c["system"], S[order], U[order], Te[order], bounds=(c["lo"], c["hi"]))
    assert (got[0] == 0).all()
    _check(case, True, got, e=1)
    assert np.array_equal(got[3, :k + 1], got[1, T - k:T + 1]) and (got[3, k + 1:] == 0).all()


# ---------------------------------------------------------------------- 3. nothing held: bit for bit
@pytest.mark.parametrize("case", ["di_solved", "rand_car_park", "rand_ur5"])
def test_infinite_bounds_are_the_unbounded_pass_bit_for_bit_at_full_length(case):
    c = MP.long_cases()[case]
    S, U, T = _batch(c)
    inf = np.full(U.shape[2], np.inf)
    plain = _labels(c["system"], S, U, T)
    assert np.isfinite(plain).all() and plain[0].any()
    assert np.array_equal(_labels(c["system"], S, U, T, bounds=(-inf, inf)), plain)
