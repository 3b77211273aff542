"""Copy the reference's data files the tests read into tests/golden/, given a reference checkout:

    python -B tests/golden/make_ref_files.py REFERENCE_DIR

* urdf/*.urdf — the robot descriptions the reference loads (test_boundary.py parses them);
* h5/*.h5 — the Keras-2.11 checkpoints test_h5.py reads (the .npz weight fixtures beside them were
  extracted from the same files by make_h5_fixtures.py);
* ref_conf_constants.json — the literal module-level constants of the reference's conf_*.py, read as
  text via ast (nothing is executed); `*_path` entries are left out.
"""
import ast
import json
import os
import shutil
import sys

OUT = os.path.dirname(os.path.abspath(__file__))
URDF = ["double_integrator.urdf", "planar_manipulator_3dof.urdf", "ur5_robot.urdf"]
DI = "Results Double Integrator/Results set test/NNs/N_try_6"
SI = "Results Single Integrator/Results set test/NNs"
H5 = {
    "di_seed0_actor_0.h5": DI + "/actor_0.h5",
    "di_seed0_critic_0.h5": DI + "/critic_0.h5",
    "di_seed0_target_critic_0.h5": DI + "/target_critic_0.h5",
    "di_seed0_actor_final.h5": DI + "/actor_final.h5",
    "di_seed0_critic_final.h5": DI + "/critic_final.h5",
    "di_seed0_target_critic_final.h5": DI + "/target_critic_final.h5",
    "si_seed0_actor_0.h5": SI + "/N_try_0/actor_0.h5",
    "si_seed10_critic_0.h5": SI + "/N_try_5/critic_0.h5",
}
SYSTEMS = ["single_integrator", "double_integrator", "manipulator", "car", "car_park", "ur5"]


def conf_constants(path):
    out = {}
    with open(path) as f:
        body = ast.parse(f.read()).body
    for node in body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            name = node.targets[0].id
            if name.endswith("_path"):
                continue
            try:
                value = ast.literal_eval(node.value)
                json.dumps(value)
            except Exception:
                continue
            out[name] = value
    return out


def main(ref):
    for sub in ("urdf", "h5"):
        os.makedirs(os.path.join(OUT, sub), exist_ok=True)
    for name in URDF:
        shutil.copyfile(os.path.join(ref, "urdf", name), os.path.join(OUT, "urdf", name))
    for name, src in H5.items():
        shutil.copyfile(os.path.join(ref, src), os.path.join(OUT, "h5", name))
    consts = {s: conf_constants(os.path.join(ref, "conf_%s.py" % s)) for s in SYSTEMS}
    with open(os.path.join(OUT, "ref_conf_constants.json"), "w") as f:
        json.dump(consts, f, indent=1, sort_keys=True)
        f.write("\n")
    print({s: len(c) for s, c in consts.items()})
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
