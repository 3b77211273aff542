"""CPU-side checks of the trajectory optimiser's hard control limits (cacto_to_box, the five `_box`
entries, `bounds=`):
  - tests/golden/to_box_helper.json is what tests/ilqr_box.py gives today (re-run on car_park and the
    manipulator) and has the shape of every system's inputs;
  - cacto_amd/csrc/box_qp.h, compiled for the host into a stand-alone program, against the
    enumeration of active sets on seeded random problems;
  - the header declares the struct, the enum and the entries, the library exports and binds them, the
    ctypes mirror has the header's layout beside an unchanged cacto_to_cfg and cacto_to_opts, bad bounds
    and a null system are refused without a GPU, and the Python layer and the command lines map and
    check the `bounds` key."""
import ctypes
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ilqr_box as X
import ilqr_ref as R
from conftest import GOLDEN
from cacto_amd import _lib as L
from cacto_amd import to as T
from cacto_amd.build import hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"cacto_to_solve_box": "cacto_to_solve_opts", "cacto_to_backward_gains_box": "cacto_to_backward_gains_opts",
           "cacto_to_forward_box": "cacto_to_forward", "cacto_to_solve_plan_box": "cacto_to_solve_plan_opts",
           "cacto_to_workspace_bytes_box": "cacto_to_workspace_bytes_opts"}
RTOL = 1e-9             # test_gpu_to_solve.py's


# ---------------------------------------------------------------------- 1. the record
def _record():
    with open(os.path.join(GOLDEN, "to_box_helper.json")) as f:
        return json.load(f)


def test_record_covers_the_full_solve_inputs():
    rec = _record()
    assert sorted(rec) == sorted(s for s in R.SOLVE_SHAPES if s != "ur5")
    for system, r in rec.items():
        Te = R.solve_inputs(system)[1]
        assert len(r["status"]) == len(r["iters"]) == len(Te), system
        assert r["bound_scale"] == X.BOUND_SCALE[system]
        live = int((Te >= 0).sum())
        for e, T_ in enumerate(Te):
            if T_ < 0:
                assert r["status"][e] == r["iters"][e] == -1
            else:
                assert r["status"][e] in (R.CONVERGED, R.MAXITER, R.FAILED) and r["iters"][e] >= (1 if T_ > 0 else 0)
        # what tools/to_box_record.py asserted before it wrote the record
        assert sum(s == R.CONVERGED for s in r["status"]) >= 0.9 * live
        assert 0.1 <= r["at_bound"] <= 0.9
        assert all(0 <= e < len(Te) and Te[e] >= 0 for e in r["excluded"]) and len(r["excluded"]) <= 0.1 * live
        assert r["kkt_ratio"] > 0


@pytest.mark.parametrize("system", ["car_park", "manipulator"])
def test_record_is_what_the_helper_gives(system):
    rec = _record()[system]
    P = X.BoxProblem(system, "test")
    S0, Te = R.solve_inputs(system)
    at_bound = total = 0
    for e in range(len(Te)):
        T_ = int(Te[e])
        r = P.solve(S0[e], np.zeros((max(T_, 1), P.m)), T_)
        assert (int(r["status"]), int(r["iters"])) == (rec["status"][e], rec["iters"][e]), (system, e)
        assert (r["flip"] < X.FLIP) == (e in rec["excluded"]), (system, e, r["flip"])
        U = r["U"][:T_]
        assert ((U >= P.lo) & (U <= P.hi)).all()
        at_bound += int(((U == P.lo) | (U == P.hi)).sum())
        total += U.size
    assert at_bound / total == pytest.approx(rec["at_bound"], abs=1e-12)


# ---------------------------------------------------------------------- 2. box_qp.h on the host
def _spd(rng, m):
    Q, _ = np.linalg.qr(rng.normal(size=(m, m)))
    return (Q * 10.0 ** rng.uniform(-2, 2, m)) @ Q.T


def qp_problems(seed=0, per_kind=20):
    """Seeded random strictly convex box QPs for M = 1, 2, 3, 6: the solution inside the box (all
    free), in a corner (all clamped), mixed, a component whose start (the projection of 0) lies exactly
    on a bound, boxes with open (infinite) sides, and a (nearly) diagonal H whose Newton step leaves the
    box in some components (the first projected step is then already the solution, and the next
    gradient on the free set is rounding noise). Returns a list of (kind, H, q, lo, hi)."""
    rng = np.random.default_rng(seed)
    out = []
    for m in (1, 2, 3, 6):
        for _ in range(per_kind):
            H, q = _spd(rng, m), rng.normal(size=m)
            x = np.linalg.solve(H, -q)
            w = np.abs(x).max() + 1.0
            out.append(("free", H, q, x - w * rng.uniform(1, 2, m), x + w * rng.uniform(1, 2, m)))
            # every component pushed into the corner sign(-q): a small box and a diagonally dominant pull
            Hc = H / np.abs(H).max()
            qc = np.sign(q) * (np.abs(q) + 10.0 * m)
            out.append(("clamped", Hc, qc, -rng.uniform(0.01, 1, m), rng.uniform(0.01, 1, m)))
            lo, hi = -rng.uniform(0.0, 1.5, m) * np.abs(x) - 1e-3, rng.uniform(0.0, 1.5, m) * np.abs(x) + 1e-3
            out.append(("mixed", H, q, lo, hi))
            lo2, hi2 = lo.copy(), hi.copy()
            for j in range(m):          # 0 is the projection's start: put it on a bound
                if rng.random() < 0.6:
                    (lo2 if rng.random() < 0.5 else hi2)[j] = 0.0
            j = int(rng.integers(m))
            lo2[j] = 0.0
            out.append(("on_bound", H, q, lo2, hi2))
            lo3, hi3 = lo.copy(), hi.copy()
            lo3[rng.random(m) < 0.5] = -np.inf
            hi3[rng.random(m) < 0.5] = np.inf
            out.append(("inf", H, q, lo3, hi3))
            Hd = np.diag(10.0 ** rng.uniform(-4, 0, m))
            if m > 1:
                Hd[1, 0] = Hd[0, 1] = 1e-18 * rng.normal()
            xd = np.linalg.solve(Hd, -q)
            cut = rng.random(m) < 0.5
            cut[int(rng.integers(m))] = True
            lo4 = np.where(cut & (xd < 0), xd * rng.uniform(0.1, 0.9, m), -np.abs(xd) - 1.0)
            hi4 = np.where(cut & (xd > 0), xd * rng.uniform(0.1, 0.9, m), np.abs(xd) + 1.0)
            out.append(("diagonal", Hd, q, lo4, hi4))
    return out


@pytest.fixture(scope="module")
def qp_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("box_qp")
    exe = str(d / "box_qp_main")
    cmd = [hipcc(), "-x", "hip", "--offload-host-only", "-O2", "-std=c++17", "-ffp-contract=off",
           "-I", os.path.join(ROOT, "cacto_amd", "csrc"), os.path.join(ROOT, "tests", "box_qp_main.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe, d


def _fmt(v):
    return " ".join("inf" if x == np.inf else "-inf" if x == -np.inf else float(x).hex() for x in np.ravel(v))


def run_qp_program(exe, d, problems):
    """to_box_qp<M>'s (ok, free [M] bool, x [M], Lf [M, M]) per problem. The numbers cross as hex floats."""
    fin, fout = str(d / "in.txt"), str(d / "out.txt")
    with open(fin, "w") as f:
        for _, H, q, lo, hi in problems:
            f.write("%d %s %s %s %s\n" % (len(q), _fmt(H), _fmt(q), _fmt(lo), _fmt(hi)))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = []
    with open(fout) as f:
        for (_, _, q, _, _), line in zip(problems, f):
            tok = line.split()
            m = len(q)
            vals = np.array([float.fromhex(t) for t in tok[2:]])
            out.append((tok[0] == "1", np.array([(int(tok[1]) >> j) & 1 == 1 for j in range(m)]), vals[:m],
                        vals[m:].reshape(m, m)))
    assert len(out) == len(problems)
    return out


def test_hex_input_is_read_by_the_program(qp_program):
    # strtod reads C99 hex floats: the program sees the very doubles of the test
    exe, d = qp_program
    H = np.array([[math.pi]])
    ok, free, x, Lf = run_qp_program(exe, d, [("one", H, np.array([-1.0]), np.array([-np.inf]), np.array([np.inf]))])[0]
    assert ok and free.all() and Lf[0, 0] == math.sqrt(math.pi)
    assert abs(x[0] - 1.0 / math.pi) <= 4 * np.finfo(float).eps


def test_box_qp_matches_the_enumeration(qp_program):
    exe, d = qp_program
    problems = qp_problems()
    assert len(problems) == 480
    got = run_qp_program(exe, d, problems)
    kinds = {}
    for (kind, H, q, lo, hi), (ok, free, x, Lf) in zip(problems, got):
        m = len(q)
        ref, ref_free, margin = X.box_qp(H, q, lo, hi)
        alt = X.box_qp(H, q, lo, hi, inverse="inv")[0]
        assert ok, (kind, m)
        assert ((x >= lo) & (x <= hi)).all(), (kind, m)
        tol = RTOL * (np.abs(ref).max() + 1e-12) + 100.0 * np.abs(alt - ref).max()
        err = np.abs(x - ref).max()
        assert err <= tol, (kind, m, err, tol)
        # a clamped component sits on its bound exactly; the free set is the enumeration's where the
        # problem is not degenerate
        assert ((x == lo) | (x == hi))[~free].all(), (kind, m)
        if margin >= 1e-6:
            assert (free == ref_free).all(), (kind, m, free, ref_free)
        # the factor: L L^T is H on the free block, the identity outside it; L is lower triangular
        want = np.where(np.outer(free, free), 0.5 * (H + H.T), np.identity(m))
        assert np.abs(Lf @ Lf.T - want).max() <= 1e-12 * np.abs(want).max(), (kind, m)
        assert (np.triu(Lf, 1) == 0).all()
        k = kinds.setdefault(kind, dict(n=0, free=0, clamped=0, started_on_bound=0, open_sides=0))
        k["n"] += 1
        k["free"] += int(free.sum())
        k["clamped"] += int((~free).sum())
        k["started_on_bound"] += int(((lo == 0) | (hi == 0)).sum())
        k["open_sides"] += int(np.isinf(lo).sum() + np.isinf(hi).sum())
    print(kinds)
    # the cases are what their names say
    assert kinds["free"]["clamped"] == 0 and kinds["clamped"]["free"] == 0
    assert kinds["mixed"]["free"] > 50 and kinds["mixed"]["clamped"] > 50
    assert kinds["on_bound"]["started_on_bound"] >= kinds["on_bound"]["n"] and kinds["on_bound"]["clamped"] > 20
    assert kinds["inf"]["open_sides"] > 100 and kinds["inf"]["clamped"] > 20
    assert kinds["diagonal"]["clamped"] >= kinds["diagonal"]["n"]


@pytest.mark.parametrize("system", ["single_integrator", "double_integrator"])
def test_box_qp_solves_the_nodes_of_a_backward_pass(qp_program, system, monkeypatch):
    """The QPs the helper meets along the gains test's episodes (mu = 0 and 1): to_box_qp solves every
    one, to the enumeration's solution."""
    exe, d = qp_program
    nodes = []
    real = X.box_qp

    def spy(H, q, lo, hi, inverse="solve"):
        r = real(H, q, lo, hi, inverse)
        nodes.append((("node", H.copy(), q.copy(), lo.copy(), hi.copy()), r, real(H, q, lo, hi, "inv")[0]))
        return r
    monkeypatch.setattr(X, "box_qp", spy)
    P = X.BoxProblem(system, "conf")
    S, U, T_ = R.random_episodes(system, seed=X.GAINS_SEEDS[system])
    for mu in (0.0, 1.0):
        for e in range(len(T_)):
            P.backward(S[e], P.clamp(U[e]), int(T_[e]), mu)
    assert len(nodes) > 150
    clamped = 0
    for (prob, (ref, ref_free, margin), alt), (ok, free, x, _) in zip(nodes, run_qp_program(exe, d, [n[0] for n in nodes])):
        assert ok
        assert np.abs(x - ref).max() <= RTOL * (np.abs(ref).max() + 1e-12) + 100.0 * np.abs(alt - ref).max()
        if margin >= 1e-6:
            assert (free == ref_free).all()
        clamped += int((~free).sum())
    assert clamped > 20


def test_box_offsets_reach_the_bound(qp_program):
    """box_offset_lo / box_offset_hi: u + offset reaches the bound in float64 (so the clamped full step of
    a clamped control lands on it), the offset is the rounded difference where that already does, never
    more than a few units in the last place from it, and equal to the helper's BoxProblem.box bit for bit."""
    exe, d = qp_program
    rng = np.random.default_rng(3)
    lo, hi = np.array([-6.0, -1.0, -0.3]), np.array([6.0, 1.0, 0.7])
    P = X.BoxProblem("single_integrator", (lo[:1], hi[:1]))
    cases = []
    for j in range(3):
        us = np.concatenate([rng.uniform(lo[j], hi[j], 400), [lo[j], hi[j], 0.0, np.nextafter(hi[j], -np.inf),
                                                               np.nextafter(lo[j], np.inf)]])
        cases += [(u, lo[j], hi[j]) for u in us]
    cases += [(0.25, -np.inf, np.inf), (0.25, -1.0, np.inf)]
    fin, fout = str(d / "off_in.txt"), str(d / "off_out.txt")
    with open(fin, "w") as f:
        for c in cases:
            f.write("0 %s\n" % _fmt(c))
    assert subprocess.run([exe, fin, fout]).returncode == 0
    moved = 0
    with open(fout) as f:
        for (u, l, h), line in zip(cases, f):
            bl, bh = (float.fromhex(t) for t in line.split()[2:])
            assert u + bh >= h and u + bl <= l
            assert min(max(u + bh, l), h) == h and min(max(u + bl, l), h) == l      # the clamped full step
            assert bh >= h - u and bl <= l - u
            if np.isfinite(h):
                assert bh - (h - u) <= 4 * np.spacing(abs(h - u)) and (bh == h - u or u + np.nextafter(bh, -np.inf) < h)
            if np.isfinite(l):
                assert (l - u) - bl <= 4 * np.spacing(abs(l - u)) and (bl == l - u or u + np.nextafter(bl, np.inf) > l)
            P.lo, P.hi = np.array([l]), np.array([h])
            ref = P.box(np.array([u]))
            assert (ref[0][0], ref[1][0]) == (bl, bh)
            moved += int(bh != h - u) + int(bl != l - u)
    print("offsets moved off the rounded difference:", moved, "of", 2 * len(cases))
    assert moved >= 5           # the case is met (it is rare): the rounded difference falls short for some u


def test_box_qp_reports_a_matrix_that_is_not_positive_definite(qp_program):
    exe, d = qp_program
    H = np.array([[1.0, 2.0], [2.0, 1.0]])
    z, o = np.zeros(2), np.ones(2)
    bad = run_qp_program(exe, d, [("indefinite", H, o, -o, o), ("nan", H * np.nan, o, -o, o),
                                  ("negative", -np.identity(2), z + 0.5, -o, o)])
    assert [b[0] for b in bad] == [False, False, False]


# ---------------------------------------------------------------------- 3. the ABI
def _box(mode=1, reserved=0, lo=(-1.0,), hi=(1.0,)):
    b = L.ToBox()
    b.mode, b.reserved = mode, reserved
    for j, v in enumerate(lo):
        b.lo[j] = v
    for j, v in enumerate(hi):
        b.hi[j] = v
    return b


def test_header_declares_the_entries_and_the_library_exports_and_binds_them():
    names = L.header_exports()
    lib = L.lib()
    for n, base in ENTRIES.items():
        assert n in names and n in L._SIGS and hasattr(lib.dll, n), n
        fn = getattr(lib.dll, n)
        assert fn.argtypes[-1] is ctypes.POINTER(L.ToBox), n
        assert L._SIGS[n][0] is L._SIGS[base][0] and L._SIGS[n][1][:-1] == L._SIGS[base][1], n
    assert lib.dll.cacto_abi_version() == 1


def test_box_layout_and_enum_match_the_header_and_the_other_structs_did_not_move():
    with open(L.HEADER) as f:
        text = f.read()
    body = re.search(r"typedef struct \{([^}]*)\} cacto_to_box;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+)(\[\w+\])?(?:, (\w+)(\[\w+\]))?;", body) == [
        ("int32_t", "mode", "", "", ""), ("int32_t", "reserved", "", "", ""),
        ("double", "lo", "[CACTO_MAX_ACTION]", "hi", "[CACTO_MAX_ACTION]")]
    assert int(re.search(r"#define CACTO_MAX_ACTION (\d+)", text).group(1)) == L.MAX_ACTION == 8
    assert [n for n, _ in L.ToBox._fields_] == ["mode", "reserved", "lo", "hi"]
    assert ctypes.sizeof(L.ToBox) == 136 and L.ToBox.lo.offset == 8 and L.ToBox.hi.offset == 72
    assert ctypes.sizeof(L.ToOpts) == 16 and ctypes.sizeof(L.ToCfg) == 64      # neither grew
    enum = re.search(r"enum cacto_to_bounds \{([^}]*)\}", text).group(1)
    assert dict((k, int(v)) for k, v in re.findall(r"(CACTO_TO_BOUNDS_[A-Z]+) = (\d)", enum)) == {
        "CACTO_TO_BOUNDS_NONE": L.CACTO_TO_BOUNDS_NONE, "CACTO_TO_BOUNDS_BOX": L.CACTO_TO_BOUNDS_BOX}
    assert (L.CACTO_TO_BOUNDS_NONE, L.CACTO_TO_BOUNDS_BOX) == (0, 1)


def _call_all(lib, cfg, plan, o, b, match, forward_match=None):
    with pytest.raises(RuntimeError, match=match):
        lib.call("cacto_to_solve_box", None, None, None, 1, None, 1, 2, ctypes.byref(cfg), None, None, None, None, None,
                 None, None, 0, None, o, b)
    with pytest.raises(RuntimeError, match=match):
        lib.call("cacto_to_solve_plan_box", None, ctypes.byref(cfg), ctypes.byref(plan), o, b)
    with pytest.raises(RuntimeError, match=match):
        lib.call("cacto_to_backward_gains_box", None, None, 1, None, 1, None, 1, 0.0, None, None, None, None, None, o, b)
    with pytest.raises(RuntimeError, match=forward_match or match):
        lib.call("cacto_to_forward_box", None, None, 1, None, 1, None, None, None, 1, 1.0, None, None, None, None, b)
    assert lib.dll.cacto_to_workspace_bytes_box(None, 4, 8, ctypes.byref(cfg), o, b) == 0
    assert (plan.on_device, plan.block_threads, plan.lds_bytes, plan.launches_per_iter) == (-7, -7, -7, -7)


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("bad", [_box(2), _box(-1), _box(1, 1), _box(0, 5), _box(1, 0, (NAN,), (1.0,)),
                                 _box(1, 0, (-1.0,), (NAN,)), _box(1, 0, (1.0,), (1.0,)), _box(1, 0, (2.0,), (1.0,)),
                                 _box(1, 0, (INF,), (INF,)), _box(1, 0, (0.0,), (-INF,))])
def test_bad_bounds_are_refused_without_a_gpu(bad):
    """With a null system nb_action is not known yet: entry 0 is the one checked, before the other
    arguments. (Entries 1.. of a real system: tests/test_gpu_to_box.py.)"""
    lib = L.lib()
    _call_all(lib, T.make_cfg(), L.ToPlan(-7, -7, -7, -7), None, ctypes.byref(bad), "bad bounds")
    # bad options come first, as in the `_opts` entries (cacto_to_forward has none)
    o = L.ToOpts()
    o.hessian = 7
    _call_all(lib, T.make_cfg(), L.ToPlan(-7, -7, -7, -7), ctypes.byref(o), ctypes.byref(bad), "bad options", "bad bounds")


@pytest.mark.parametrize("good", [None, _box(0), _box(0, 0, (NAN,), (NAN,)), _box(1), _box(1, 0, (-INF,), (INF,))])
def test_a_null_system_is_refused_without_a_gpu(good):
    lib = L.lib()
    b = ctypes.byref(good) if good is not None else None
    _call_all(lib, T.make_cfg(), L.ToPlan(-7, -7, -7, -7), None, b, "bad arguments")
    with pytest.raises(RuntimeError, match="null config"):
        lib.call("cacto_to_solve_box", None, None, None, 1, None, 1, 2, None, None, None, None, None, None, None, None, 0,
                 None, None, b)


# ---------------------------------------------------------------------- 4. Python
class _Conf:
    nb_action = 2
    u_min = np.array([-2.0, -3.0])
    u_max = np.array([2.0, 4.0])


def test_python_maps_and_checks_the_bounds_key():
    assert T.DEFAULT_CFG["bounds"] == "none"
    c = T.make_cfg(dict(bounds="conf", max_iter=7))
    assert isinstance(c, L.ToCfg) and ctypes.sizeof(c) == 64 and c.max_iter == 7
    assert "bounds" not in [n for n, _ in L.ToCfg._fields_] and not hasattr(c, "box")
    for none in (None, "none", dict(), dict(bounds="none"), dict(bounds=None), dict(max_iter=3)):
        assert T.make_box(none, _Conf) is None
    b = T.make_box(dict(bounds="conf"), _Conf)
    assert isinstance(b, L.ToBox) and (b.mode, b.reserved) == (1, 0) and T.make_box(b, _Conf) is b
    assert list(b.lo)[:2] == [-2.0, -3.0] and list(b.hi)[:2] == [2.0, 4.0] and list(b.lo)[2:] == [0.0] * 6
    b = T.make_box(([-1, -np.inf], (0.5, np.inf)), _Conf)
    assert list(b.lo)[:2] == [-1.0, -np.inf] and list(b.hi)[:2] == [0.5, np.inf] and b.mode == 1
    assert T.make_box("conf", _Conf).mode == 1
    # which entry a call takes: none -> the old names, bounds -> `_box` with options and bounds
    o = T.make_opts()
    assert T._opts_args(o) == ("", ()) and T._opts_args(o, None) == ("", ())
    assert T._opts_args(T.make_opts("psd"))[0] == "_opts"
    sfx, extra = T._opts_args(o, b)
    assert sfx == "_box" and len(extra) == 2
    assert T._cfg_box(dict(bounds="conf"), _Conf).mode == 1 and T._cfg_box(None, _Conf) is None
    assert T._cfg_box(c, _Conf) is None and T._cfg_box(c, _Conf, bounds="conf").mode == 1
    assert T._cfg_box(dict(bounds="conf"), _Conf, bounds="none") is None
    for bad in ("box", "Conf", 1, 1.0, True, ([-1.0], [1.0]), ([-1, -1, -1], [1, 1, 1]), ([-1, -1], [1, 1], [2, 2]),
                ([-1, 1], [1, 1]), ([-1, 2], [1, 1]), ([np.nan, -1], [1, 1]), ([-1, -1], [1, np.nan]),
                ([[-1, -1]], [[1, 1]]), ("ab", "cd")):
        with pytest.raises(ValueError, match="bounds"):
            T.make_box(dict(bounds=bad), _Conf)
    for bad in ("box", 1, True, ([-1, -1], [1, 1], [2, 2]), ("ab", "cd")):
        with pytest.raises(ValueError, match="bounds"):
            T.make_cfg(dict(bounds=bad))                # the form is checked where there is no conf yet
    assert isinstance(T.make_cfg(dict(bounds=([-1, -1], [1, 1]))), L.ToCfg)


def test_command_lines_take_the_option():
    from cacto_amd import main as M
    assert "to_bounds" not in M.parse_args([]) and M.train_kwargs(M.parse_args([]))[1]["to_cfg"] == dict(path="default")
    a = M.parse_args(["--to-bounds", "conf", "--to-path", "wave", "--to-hessian", "psd"])
    assert a["to_bounds"] == "conf"
    assert M.train_kwargs(a)[1]["to_cfg"] == dict(path="wave", hessian="psd", bounds="conf")
    assert M.train_kwargs(M.parse_args(["--to-bounds", "none"]))[1]["to_cfg"] == dict(path="default", bounds="none")
    a = M.parse_args(["--to-bounds", "conf", "--seeds", "0,1"])
    assert a["seeds"] == [0, 1] and M.train_kwargs(a)[1]["to_cfg"]["bounds"] == "conf"
    with pytest.raises(SystemExit):
        M.parse_args(["--to-bounds", "box"])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "to_bench.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--bounds {none,conf}" in r.stdout
