"""CPU checks of the long-horizon label fixture (tests/golden/label_long.npz) and of what it is there to show:
the float64 label recursion of the reference's formula loses every digit over a full-length episode, the
same recursion with V_xx symmetrised per node does not. The truth is the recursion at 80 digits
(tests/ddp_mp_ref.py). The GPU side is tests/test_gpu_ddp_long.py."""
import numpy as np
import pytest

import ddp_mp_ref as MP


def test_fixture_lists_the_cases():
    cases = MP.long_cases()
    assert tuple(cases) == MP.LONG_CASES
    for name, c in cases.items():
        ns = c["conf"].nb_state
        assert c["S"].shape == (c["T"] + 1, ns) and c["U"].shape == (c["T"], c["conf"].nb_action), name
        assert c["Vb"].shape == c["Vu"].shape == c["S"].shape and c["T"] <= 200, name
        assert np.isfinite(c["Vb"]).all() and np.isfinite(c["Vu"]).all() and not np.array_equal(c["Vb"], c["Vu"]), name
        assert ((c["U"] >= c["lo"]) & (c["U"] <= c["hi"])).all(), name
    # the conf's full length, the car cut to the GPU test's limit; the solved episodes as long as they came
    assert {n: c["T"] for n, c in cases.items()} == dict(
        di_solved=192, di_maxiter=163, rand_single_integrator=100, rand_double_integrator=200, rand_car=200,
        rand_car_park=100, rand_manipulator=100, rand_ur5=100)


@pytest.mark.parametrize("case", MP.LONG_CASES)
def test_the_fixture_reproduces(case):
    """The 80-digit recursion, recomputed from the stored S, U, gives the stored labels bit for bit."""
    c = MP.long_cases()[case]
    rec, lxT, lxxT, U = MP.episode_records(c["conf"], c["S"], c["U"])
    Vb, held, margin, _ = MP.riccati_mp(rec, lxT, lxxT, U, c["lo"], c["hi"])
    Vu, held_u, _, _ = MP.riccati_mp(rec, lxT, lxxT, U, -np.inf, np.inf)
    assert Vb.tobytes() == c["Vb"].tobytes() and Vu.tobytes() == c["Vu"].tobytes()
    # the rule of ddp_box_ref.label_inputs_ok on the held decisions, and bounds that take part
    assert margin >= 1e-6 and held.sum() >= 3 and not held_u.any()


@pytest.mark.parametrize("bounded", [True, False])
def test_the_instability_is_pinned(bounded):
    """On the solved double-integrator episode the reference's formula in float64 has more than half its rows
    further than 1e-6 of the scale from the truth. If this stops holding, the case tests nothing."""
    c = MP.long_cases()["di_solved"]
    e = MP.amplification(c["conf"], c["S"], c["U"], c["Vb"] if bounded else c["Vu"], c["lo"] if bounded else None, c["hi"])
    print("plain helper: share of rows > 1e-6", (e > 1e-6).mean(), "worst", e.max(), "first failing horizon",
          MP.first_failing_horizon(e))
    assert (e > 1e-6).mean() > 0.5
    assert 40 <= MP.first_failing_horizon(e) <= 80          # ~60 steps from the end


@pytest.mark.parametrize("bounded", [True, False])
@pytest.mark.parametrize("case", MP.LONG_CASES)
def test_the_symmetrised_helper_is_accurate(case, bounded):
    e = MP.sym_error(case, bounded)
    print(case, bounded, "symmetrised helper: worst row", e.max())
    assert len(e) == MP.long_cases()[case]["T"] + 1
    assert (e <= 1e-9).all()


def test_symmetrize_defaults_off_and_changes_nothing_short():
    """The default of both helpers stays the reference's formula, and at the length of the existing parity
    tests (24 steps) symmetrising moves the labels by a fraction of those tests' tolerance
    (test_gpu_ddp.py: 1e-9 scale + 100 |helper(inv) - helper(pinv)| per row), so they keep their reference."""
    import ddp_box_ref as D
    from oracle import ddp as oddp
    c = MP.long_cases()["di_solved"]
    conf, S, U = c["conf"], c["S"][-25:], c["U"][-24:]
    passes = (lambda **kw: oddp.backward_pass(conf, S, U, **kw),
              lambda **kw: D.backward_pass_box(conf, S, U, c["lo"], c["hi"], **kw)[0])
    for run in passes:
        a = run()
        assert np.array_equal(a, run(symmetrize=False))
        tol = 1e-9 * np.abs(a).max() + 100.0 * np.abs(run(inverse="inv") - a).max(axis=1, keepdims=True)
        ratio = (np.abs(run(symmetrize=True) - a) / tol).max()
        print("symmetrised against plain at 24 steps: worst share of the tolerance", ratio)
        assert ratio <= 0.5
