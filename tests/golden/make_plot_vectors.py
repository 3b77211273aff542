"""Record what the reference's plot_utils.py computes on the host, for tests/test_plot_cpu.py:

    python -B tests/golden/make_plot_vectors.py REFERENCE_DIR

Like make_ref_vectors.py it imports the reference's own module (a stub `tensorflow` in sys.modules,
PLOT.__new__ with a small conf object) and runs where a reference checkout is; the tests read only
its output, tests/golden/plot_vectors.npz, which holds numbers and names:

* ics_<sys> [961, ns], flag_<sys> [961] — compute_ICS over the 31 x 31 grid of
  plot_Critic_Value_function (k_y outer, k_x inner) for the five planar systems, NaN rows where
  continue_flag was set;
* manip_p [961 + extra, 3], manip_ics, manip_flag — the manipulator over a 31 x 31 grid on
  [-30, 20] x [-25, 25] (inside its reach: both signs of p_ee[1]) and a few points that put the
  third joint at the origin or the EE on the radius-30 circle;
* car_rng_keys, car_rng_pos — numpy's global generator after the car's 961 calls from
  np.random.seed(3);
* name_* — the file names the reference's figure methods hand to savefig (recorded by running
  them with savefig replaced);
* plot_<sys> = [plot_flag, plot_rollout_interval, plot_rollout_interval_diff_loc] and manip_base =
  [x_base, y_base, l] — the confs' settings, read as text via ast (the `if plot_flag:` rule
  evaluated), nothing executed. The reference's conf_manipulator.py defines no `l`; the value
  recorded is the link length of its urdf/planar_manipulator_3dof.urdf (joint origins 10 apart),
  the only one under which compute_ICS's radius-30 test is the arm's reach.
"""
import ast
import os
import sys
import types

sys.dont_write_bytecode = True  # never write __pycache__ into the reference tree
os.environ["MPLBACKEND"] = "Agg"

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plot_vectors.npz")
PLANAR = {"single_integrator": 3, "double_integrator": 5, "car": 6, "car_park": 6, "manipulator": 7}
SYSTEMS = sorted(PLANAR) + ["ur5"]
LINK = 10.0


def conf_plot_settings(path):
    with open(path) as f:
        body = ast.parse(f.read()).body
    vals = {}

    def take(nodes):
        for node in nodes:
            if isinstance(node, ast.Assign) and isinstance(node.targets[0], ast.Name):
                name = node.targets[0].id
                if name in ("plot_flag", "plot_rollout_interval", "plot_rollout_interval_diff_loc", "x_base", "y_base"):
                    vals[name] = eval(compile(ast.Expression(node.value), path, "eval"), {"np": np})
            elif isinstance(node, ast.If) and isinstance(node.test, ast.Name) and node.test.id == "plot_flag":
                take(node.body if vals["plot_flag"] else node.orelse)
    take(body)
    return vals


def main(ref):
    tf = types.ModuleType("tensorflow")
    sys.modules["tensorflow"] = tf
    sys.path.insert(0, ref)
    import plot_utils as P
    out = {}

    settings = {s: conf_plot_settings(os.path.join(ref, "conf_%s.py" % s)) for s in SYSTEMS}
    for s, v in settings.items():
        out["plot_" + s] = np.array([v["plot_flag"], v["plot_rollout_interval"], v["plot_rollout_interval_diff_loc"]],
                                    dtype=np.float64)
    m = settings["manipulator"]
    out["manip_base"] = np.array([m["x_base"], m["y_base"], LINK])

    plot = P.PLOT.__new__(P.PLOT)
    plot.conf = types.SimpleNamespace(x_base=m["x_base"], y_base=m["y_base"], l=LINK)

    def grid(sys_id, xs, ys, extra=()):
        pts = [np.array([x, y, 0]) for y in ys for x in xs] + [np.array(p, dtype=np.float64) for p in extra]
        ics = np.full((len(pts), PLANAR[sys_id]), np.nan)
        flag = np.zeros(len(pts), dtype=np.int64)
        for i, p in enumerate(pts):
            s, flag[i] = plot.compute_ICS(p, sys_id, continue_flag=0)
            if not flag[i]:
                ics[i] = s
        return np.array(pts), ics, flag

    lin = np.linspace(-15, 15, 31)
    for s in sorted(PLANAR):
        if s == "car":
            np.random.seed(3)
        _, out["ics_" + s], out["flag_" + s] = grid(s, lin, lin)
        if s == "car":
            st = np.random.get_state()
            out["car_rng_keys"], out["car_rng_pos"] = np.asarray(st[1]), np.asarray(st[2])
    extra = [(3, 0, 0), (-17, 0, 0), (-7, 10, 0), (-7, -10, 0), (23, 0, 0), (-37, 0, 0), (-7, 30, 0), (-7, -30, 0),
             (-7, 0, 0), (13, 1e-9, 0), (13, -1e-9, 0)]
    out["manip_p"], out["manip_ics"], out["manip_flag"] = grid("manipulator", np.linspace(-30, 20, 31),
                                                                np.linspace(-25, 25, 31), extra)

    # the file names: run the figure methods on a few numbers with savefig replaced
    names = []
    P.plt.savefig = lambda fname, *a, **k: names.append(str(fname))
    c = types.SimpleNamespace(system_id="double_integrator", Fig_path="FIG", TARGET_STATE=np.array([-7.0, 0.0]),
                              fig_ax_lim=np.array([[-15, 15], [-15, 15]]), XC1=-2.0, YC1=0.0, A1=6, B1=10, XC2=3.0,
                              YC2=4.0, A2=12, B2=4, XC3=3.0, YC3=-4.0, A3=12, B3=4)
    plot = P.PLOT(4, None, types.SimpleNamespace(eval=lambda model, x: float(x[0][0] + x[0][1])), c)
    plot.plot_obstaces = lambda a=1: []            # its positional `angle` predates the installed matplotlib
    plot.plot_Critic_Value_function(None, 3.0, "double_integrator")
    out["name_value"] = np.array(names.pop())
    skip = types.SimpleNamespace(create_TO_init=lambda ep, s: (None, None, None, None, 0))
    plot.plot_traj_from_ICS(np.zeros((2, 5)), None, skip, update_step_counter=7, steps=5, init=1)
    out["name_traj"] = np.array(names.pop())
    plot.plot_Return(np.array([1.0, 2.0, np.nan]))
    out["name_return"] = np.array(names.pop())
    path = [np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 0.0]])]
    plot.plot_policy_eval(path, 7)
    out["name_policy_single"] = np.array(names.pop())
    plot.plot_policy_eval(path, 7, diff_loc=1)
    out["name_policy_multi"] = np.array(names.pop())
    out["name_args"] = np.array([4, 3, 1, 7])      # N_try, n_update, init, update_step_counter of the calls above
    assert not names

    np.savez_compressed(OUT, **out)
    print("wrote", OUT, {k: (v.shape if v.ndim else str(v)) for k, v in out.items()})
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
