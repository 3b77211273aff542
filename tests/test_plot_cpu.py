"""CPU checks of the evaluation stage's host half (cacto_amd.plot_utils): PLOT.compute_ICS against
the reference's recorded values (tests/golden/plot_vectors.npz, written by make_plot_vectors.py) bit
for bit, the draw_* functions on synthetic data (a PNG at the reference's file name), the module's
independence of matplotlib, and the confs' new settings."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from cacto_amd import plot_utils as PU
from cacto_amd.confs import SYSTEM_MAP, load_conf

PNG = b"\x89PNG\r\n\x1a\n"
PLANAR = ["single_integrator", "double_integrator", "car", "car_park", "manipulator"]


@pytest.fixture(scope="module")
def vec():
    return dict(np.load(os.path.join(GOLDEN, "plot_vectors.npz")))


def _plot(system, N_try=0):
    return PU.PLOT(N_try, None, None, load_conf(system, fresh=True))


def _same_bits(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return got.shape == ref.shape and np.array_equal(got.view(np.uint64), ref.view(np.uint64))


def _grid(plot, system, points):
    ics = np.full((len(points), plot.conf.nb_state), np.nan)
    flag = np.zeros(len(points), dtype=np.int64)
    for i, p in enumerate(points):
        s, flag[i] = plot.compute_ICS(p, system, continue_flag=0)
        assert (s is None) == bool(flag[i])
        if s is not None:
            ics[i] = s
    return ics, flag


# ---------------------------------------------------------------------- compute_ICS
@pytest.mark.parametrize("system", PLANAR)
def test_compute_ICS_equals_the_reference_on_the_value_grid(system, vec):
    lin = np.linspace(-15, 15, 31)
    points = [np.array([x, y, 0]) for y in lin for x in lin]         # k_y outer, k_x inner
    if system == "car":
        np.random.seed(3)
    ics, flag = _grid(_plot(system), system, points)
    np.testing.assert_array_equal(flag, vec["flag_" + system])
    assert _same_bits(ics, vec["ics_" + system])
    if system == "car":                                              # 961 uniform draws, in the reference's order
        st = np.random.get_state()
        np.testing.assert_array_equal(st[1], vec["car_rng_keys"])
        assert st[2] == int(vec["car_rng_pos"])
        assert np.signbit(ics[:, 2]).any() and (ics[:, 2] == 0).all()   # the product 0 * draw, kept


def test_compute_ICS_manipulator_inverse_kinematics(vec):
    plot = _plot("manipulator")
    c = plot.conf
    np.testing.assert_array_equal([c.x_base, c.y_base, c.l], vec["manip_base"])
    ics, flag = _grid(plot, "manipulator", vec["manip_p"])
    np.testing.assert_array_equal(flag, vec["manip_flag"])
    assert _same_bits(ics, vec["manip_ics"])
    p, live = vec["manip_p"], flag == 0
    assert live.sum() > 800 and (flag == 1).sum() > 50                # inside and outside the reach
    assert (p[live, 1] > 0).any() and (p[live, 1] < 0).any()          # both elbow signs
    assert flag[961:965].all()                                        # the third joint at the origin
    # what the closed form keeps of an inverse kinematics: the three angles sum to the direction
    # of p from the base (the reference's c1 carries a sign that moves the EE off p; kept as it is)
    q = ics[live, :3]
    phi = np.arctan2(p[live, 1] - c.y_base, p[live, 0] - c.x_base)
    np.testing.assert_allclose(q.sum(axis=1), phi, rtol=0, atol=1e-12)


def test_compute_ICS_options_and_unknown_systems():
    plot = _plot("car")
    state = np.random.get_state()
    s, flag = plot.compute_ICS([1.0, 2.0, 0], "car", theta=0.5, continue_flag=3)
    assert s.tolist() == [1.0, 2.0, 0.5, 0.0, 0.0, 0.0] and flag == 3
    assert plot.compute_ICS([1.0, 2.0, 0], "car_park")[0][2] == np.pi / 2
    assert np.array_equal(np.random.get_state()[1], state[1]) and np.random.get_state()[2] == state[2]
    for system in ("ur5", "pendulum"):
        with pytest.raises(ValueError, match=system):
            plot.compute_ICS([0.0, 0.0, 0], system)
    with pytest.raises(ValueError, match="ur5"):
        _plot("ur5").value_grid(None)


# ---------------------------------------------------------------------- drawing
def _is_png(path):
    with open(path, "rb") as f:
        return f.read(8) == PNG


def _traj_data(n=3, steps=20):
    rng = np.random.default_rng(0)
    ee = np.cumsum(rng.normal(size=(n, steps, 3)), axis=1)
    ok = np.array([True, False, True])
    ee[~ok] = np.nan
    return dict(ok=ok, ee_RL=ee, ee_TO=ee * 0.5)


@pytest.mark.parametrize("system", ["double_integrator", "car_park", "manipulator"])
def test_draw_functions_write_png_at_the_reference_names(system, tmp_path, vec):
    conf = load_conf(system, fresh=True)
    N_try, n_update, init, counter = (int(v) for v in vec["name_args"])
    fig = str(tmp_path / "Figures")
    want = {k: os.path.join(fig, os.path.relpath(str(vec[k]), "FIG")) + ".png"
            for k in ("name_value", "name_traj", "name_return", "name_policy_single", "name_policy_multi")}
    rng = np.random.default_rng(1)
    if system == "manipulator":
        grid = dict(ICS=np.zeros((3721, 7)), ee=rng.uniform(-30, 20, size=(3721, 3)), V=rng.normal(size=3721))
    else:
        V = rng.normal(size=(31, 31))
        V[2, 3] = V[30, 0] = np.nan
        lin = np.linspace(-15, 15, 31)
        grid = dict(x=lin, y=lin, ICS=np.zeros((961, conf.nb_state)), V=V)
    assert PU.draw_value_grid(grid, conf, N_try, float(n_update), fig) == want["name_value"]
    assert os.path.isdir(os.path.join(fig, "N_try_%d" % N_try))       # made by the first call, accepted by the rest
    assert PU.draw_traj(_traj_data(), conf, N_try, init, counter, fig) == want["name_traj"]
    returns = np.full(40, np.nan)
    returns[:25] = -np.exp(rng.normal(size=25))
    assert PU.draw_return(returns, conf, N_try, fig) == want["name_return"]
    paths = [np.cumsum(rng.normal(size=(20, 3)), axis=0) for _ in range(2)] + [np.full((20, 3), np.nan)]
    assert PU.draw_policy_eval(paths, conf, N_try, counter, fig) == want["name_policy_single"]
    assert PU.draw_policy_eval(paths, conf, N_try, counter, fig, diff_loc=1) == want["name_policy_multi"]
    for name in want.values():
        assert _is_png(name), name
    assert sorted(os.listdir(os.path.join(fig, "N_try_%d" % N_try))) == sorted(os.path.basename(n) for n in want.values())
    assert "matplotlib.pyplot" not in sys.modules


def test_obstacles_are_rectangles_for_car_park_and_ellipses_otherwise():
    from matplotlib.patches import Ellipse, Rectangle
    for system, kind in (("car_park", Rectangle), ("double_integrator", Ellipse)):
        plot = _plot(system)
        obs = plot.plot_obstaces(a=0.5)
        assert len(obs) == 3 and all(type(o) is kind and o.get_alpha() == 0.5 for o in obs)
        c = plot.conf
        assert (obs[1].get_width(), obs[1].get_height()) == (c.A2, c.B2)
        centre = obs[1].get_center() if kind is Ellipse else (obs[1].get_x() + c.A2 / 2, obs[1].get_y() + c.B2 / 2)
        assert tuple(centre) == (c.XC2, c.YC2)


def test_methods_draw_only_with_a_fig_path(tmp_path):
    plot = _plot("double_integrator", N_try=2)
    assert plot.conf.Fig_path is None
    plot.plot_Return(np.array([1.0, 2.0]))                            # no Fig_path: nothing to do, no error
    plot.conf.Fig_path = str(tmp_path)
    plot.draw = False
    plot.plot_Return(np.array([1.0, 2.0]))
    assert os.listdir(tmp_path) == []
    plot.draw = True
    plot.plot_Return(np.array([1.0, 2.0]))
    plot.plot_policy_eval([np.zeros((3, 3))], 5)
    assert sorted(os.listdir(tmp_path / "N_try_2")) == ["EpReturn_2.png", "PolicyEvaluationSingleInit_2_5.png"]
    assert plot.seconds["draw"] > 0


def test_drawing_without_matplotlib_raises(monkeypatch, tmp_path):
    monkeypatch.setitem(sys.modules, "matplotlib", None)              # `import matplotlib...` now fails
    for name in [m for m in sys.modules if m.startswith("matplotlib.")]:
        monkeypatch.delitem(sys.modules, name)
    with pytest.raises(RuntimeError, match="matplotlib"):
        PU.draw_return(np.array([1.0]), load_conf("double_integrator", fresh=True), 0, str(tmp_path))
    assert os.listdir(tmp_path) == []


def test_the_module_imports_without_matplotlib():
    code = ("import sys; import cacto_amd.plot_utils, cacto_amd.main; "
            "bad = [m for m in sys.modules if m.split('.')[0] == 'matplotlib']; assert not bad, bad")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)


# ---------------------------------------------------------------------- confs
@pytest.mark.parametrize("system", sorted(SYSTEM_MAP))
def test_confs_carry_the_plot_settings(system, vec):
    conf = load_conf(system, fresh=True)
    flag, every, diff_loc = vec["plot_" + system]
    assert conf.plot_flag == flag
    assert conf.plot_rollout_interval == every and conf.plot_rollout_interval_diff_loc == diff_loc
    assert (every == np.inf) == (flag == 0)
    assert conf.Fig_path is None


def test_main_parser_maps_the_evaluation_options():
    from cacto_amd import main as M
    assert "plots" not in M.parse_args([]) and "evaluate" not in M.train_kwargs(M.parse_args([]))[1]
    a = M.parse_args(["--plots"])
    assert a["plots"] is True and "fig_path" not in a
    assert M.train_kwargs(a)[1]["evaluate"] is True and M.train_kwargs(a)[1]["eval_every"] == 1
    a = M.parse_args(["--plots", "--fig-path", "somewhere", "--eval-every", "4"])
    assert a["fig_path"] == "somewhere" and M.train_kwargs(a)[1]["eval_every"] == 4
