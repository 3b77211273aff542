"""CPU-side checks of the bound-aware Sobolev labels (cacto_ddp_backward_box, `labels="bounded"`):
  - tests/ddp_box_ref.py without bounds is oracle.ddp.backward_pass, bit for bit;
  - at converged solutions of the bounded problem (tests/ilqr_box.py) its V_x[0] is the central
    difference of the optimal cost J* in the initial state, where the reference's unconstrained
    recursion is off by orders of magnitude more;
  - its V_x[t] is the adjoint costate of the constrained problem at every t, by a recursion that uses
    no part of the Riccati pass;
  - the header declares the entry, the library exports and binds it, and the Python layer and the
    command line map and check the `labels` key."""
import ctypes
import functools
import re

import numpy as np
import pytest

import ddp_box_ref as D
import ilqr_box as X
import ilqr_ref as R
from cacto_amd import _lib as L
from cacto_amd import main as M
from cacto_amd import to as T
from oracle import ddp as oddp

FD_SYSTEMS = ["single_integrator", "double_integrator", "car", "car_park", "manipulator"]
SOLVE = dict(gtol=1e-9, max_iter=2000)
H = 1e-5
# Relative error of the helper's V_x[0] against the central difference of J*, and of its V_x[t] against
# the adjoint costate, both max-abs over components divided by the max-abs of the yardstick. Measured
# with the committed helper on the qualifying episodes (worst per system):
#     system               finite difference     adjoint
#     single_integrator    7.3e-10               3.3e-08
#     double_integrator    2.1e-10               1.1e-10
#     car                  1.3e-08               3.9e-08
#     car_park             7.6e-07               1.2e-07
#     manipulator          9.0e-07               9.8e-08
#     ur5 (adjoint only)                         4.8e-10
# (the reference's unconstrained formula on the same episodes: 1.9e-04 .. 1.04 against the difference).
# TOL is 10 x the worst of them, 9.0e-07: the margin covers the h^2 truncation of the difference and the
# residue Q_u[f] <= gtol of the solves, both of which move with the episode.
TOL = 9.0e-6
PARENT_FACTOR = 100.0       # the reference's formula is at least this many times further from the difference


def _neg_vx(P, S, U, Te):
    V, held, margin = D.backward_pass_box(P.conf, S[:Te + 1], U[:Te], P.lo, P.hi)
    return -V[:, :P.n], held


def _solve(P, s0, U0, Te):
    return P.solve(s0, U0, Te, SOLVE)


@functools.lru_cache(maxsize=None)
def _candidates(system):
    """The first episodes of solve_inputs(system) with Te >= 4, solved from a zero warm start, with the
    2n perturbed solves (warm-started from the solution). Stops after 8 candidates or 6 qualifying
    ones. Returns a list of dicts: qualifies, S, U, Te, vx [Te+1, n] (the helper's, cost sign), held,
    fd [n] (None unless every solve converged)."""
    P = X.BoxProblem(system, "test")
    S0, Tes = R.solve_inputs(system)
    out = []
    for e in range(len(Tes)):
        Te = int(Tes[e])
        if Te < 4:
            continue
        if len(out) == 8 or sum(c["qualifies"] for c in out) == 6:
            break
        r = _solve(P, S0[e], np.zeros((Te, P.m)), Te)
        c = dict(e=e, Te=Te, S=r["S"], U=r["U"], qualifies=False, fd=None)
        out.append(c)
        if r["status"] != R.CONVERGED:
            continue
        c["vx"], c["held"] = _neg_vx(P, r["S"], r["U"], Te)
        same, fd = bool(c["held"].any()), np.zeros(P.n)
        for k in range(P.n):
            J = []
            for sgn in (+1.0, -1.0):
                s0 = S0[e].copy()
                s0[k] += sgn * H
                rp = _solve(P, s0, r["U"], Te)
                if rp["status"] != R.CONVERGED:
                    same = None
                    break
                same = same and np.array_equal(_neg_vx(P, rp["S"], rp["U"], Te)[1], c["held"])
                J.append(rp["J"][1])
            if same is None:
                break
            fd[k] = (J[0] - J[1]) / (2.0 * H)
        if same is None:
            continue
        c["fd"] = fd
        c["qualifies"] = bool(same)
    return P, out


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---------------------------------------------------------------------- 1. no bounds: the oracle
@pytest.mark.parametrize("system", ["double_integrator", "car_park"])
def test_helper_without_bounds_is_the_oracle(system):
    P = R.Problem(system)
    S, U, Tn = R.random_episodes(system)
    inf = np.full(P.m, np.inf)
    for e in range(len(Tn)):
        Te = int(Tn[e])
        for inverse in ("pinv", "inv"):
            V, held, margin = D.backward_pass_box(P.conf, S[e, :Te + 1], U[e, :Te], -inf, inf, inverse=inverse)
            assert np.array_equal(V, oddp.backward_pass(P.conf, S[e, :Te + 1], U[e, :Te], inverse=inverse))
            assert not held.any() and margin == np.inf


# ---------------------------------------------------------------------- 2. finite differences of J*
@pytest.mark.parametrize("system", FD_SYSTEMS)
def test_labels_are_the_gradient_of_the_bounded_optimum(system):
    P, cands = _candidates(system)
    good = [c for c in cands if c["qualifies"]]
    print(system, "candidates", [(c["e"], c["Te"], c["qualifies"]) for c in cands])
    assert len(good) >= 5, (system, len(good), len(cands))
    for c in good:
        parent = -oddp.backward_pass(P.conf, c["S"][:c["Te"] + 1], c["U"][:c["Te"]])[0, :P.n]
        err, err_parent = _rel(c["vx"][0], c["fd"]), _rel(parent, c["fd"])
        print("  episode %d Te %d held share %.2f: helper %.2e parent %.2e" % (c["e"], c["Te"], c["held"].mean(), err,
                                                                              err_parent))
        assert err <= TOL, (system, c["e"], err)
        assert err_parent >= PARENT_FACTOR * err, (system, c["e"], err, err_parent)


# ---------------------------------------------------------------------- 3. the adjoint costate
def _adjoint(P, S, U, Te):
    lam = np.zeros((Te + 1, P.n))
    lam[Te] = P.lx(S[Te], terminal=True)[0]
    for t in range(Te - 1, -1, -1):
        A, _ = P.jac(S[t, :P.n], U[t])
        lam[t] = P.lx(S[t])[0] + A.T @ lam[t + 1]
    return lam


@pytest.mark.parametrize("system", FD_SYSTEMS)
def test_labels_are_the_adjoint_at_every_step(system):
    P, cands = _candidates(system)
    good = [c for c in cands if c["qualifies"]]
    assert len(good) >= 5
    for c in good:
        err = _rel(c["vx"], _adjoint(P, c["S"], c["U"], c["Te"]))
        print("  %s episode %d: adjoint %.2e" % (system, c["e"], err))
        assert err <= TOL, (system, c["e"], err)


def test_labels_are_the_adjoint_ur5():
    """One short UR5 episode (its sympy oracle is too slow for the 2n re-solves of the difference)."""
    P = X.BoxProblem("ur5", "test")
    S0, Tes = R.solve_inputs("ur5")
    e = int(np.argmax(Tes))
    Te = int(Tes[e])
    assert 1 <= Te <= 6
    r = _solve(P, S0[e], np.zeros((Te, P.m)), Te)
    assert r["status"] == R.CONVERGED
    vx, held = _neg_vx(P, r["S"], r["U"], Te)
    assert held.any()
    err = _rel(vx, _adjoint(P, r["S"], r["U"], Te))
    print("  ur5 episode %d Te %d held share %.2f: adjoint %.2e" % (e, Te, held.mean(), err))
    assert err <= TOL


# ---------------------------------------------------------------------- 4. the boundary
def test_entry_is_declared_exported_and_bound():
    name = "cacto_ddp_backward_box"
    assert name in L.header_exports() and name in L._SIGS
    res, args = L._SIGS[name]
    pres, pargs = L._SIGS["cacto_ddp_backward"]
    assert res is pres and args[:-1] == pargs and args[-1] is ctypes.POINTER(L.ToBox)
    lib = L.lib()
    assert hasattr(lib.dll, name) and lib.dll.cacto_abi_version() == 1
    with open(L.HEADER) as f:
        text = f.read()
    assert re.search(r"#define\s+CACTO_ABI_VERSION\s+1\b", text)
    decl = re.search(r"int cacto_ddp_backward_box\(([^;]*)\);", text).group(1)
    parent = re.search(r"int cacto_ddp_backward\(([^;]*)\);", text).group(1)
    squeeze = lambda s: re.sub(r"\s+", " ", s).strip()      # noqa: E731
    assert squeeze(decl) == squeeze(parent) + ", const cacto_to_box* box"


def test_bad_bounds_are_refused_before_anything_else():
    """No device work: a null system and null pointers, yet the bounds are what is reported."""
    bad = L.ToBox()
    bad.mode = L.CACTO_TO_BOUNDS_BOX
    bad.lo[0], bad.hi[0] = 1.0, 1.0
    with pytest.raises(RuntimeError, match="bad bounds"):
        L.lib().call("cacto_ddp_backward_box", None, None, 1, None, 1, None, 1, 1e-9, None, None, ctypes.byref(bad))
    bad.lo[0], bad.mode = 0.0, 7
    with pytest.raises(RuntimeError, match="bad bounds"):
        L.lib().call("cacto_ddp_backward_box", None, None, 1, None, 1, None, 1, 1e-9, None, None, ctypes.byref(bad))
    # good bounds, NULL bounds: the parent's own argument check
    for box in (None, ctypes.byref(L.ToBox())):
        with pytest.raises(RuntimeError, match="cacto_ddp_backward: bad arguments"):
            L.lib().call("cacto_ddp_backward_box", None, None, 1, None, 1, None, 1, 1e-9, None, None, box)


def test_labels_key_of_the_cfg():
    assert T.DEFAULT_CFG["labels"] == "reference" and "labels" in T.NOT_FIELDS
    assert bytes(T.make_cfg(dict(labels="bounded", bounds="conf"))) == bytes(T.make_cfg())
    assert bytes(T.make_cfg(dict(labels="reference"))) == bytes(T.make_cfg())
    assert T.label_bounds(None) is None and T.label_bounds(dict(bounds="conf")) is None
    assert T.label_bounds(dict(labels="bounded", bounds="conf")) == "conf"
    pair = ([-1.0], [1.0])
    assert T.label_bounds(dict(labels="bounded", bounds=pair)) is pair
    for cfg in (dict(labels="bounded"), dict(labels="bounded", bounds="none"), dict(labels="bounded", bounds=None)):
        with pytest.raises(ValueError, match="labels.*bounds"):
            T.make_cfg(cfg)
        with pytest.raises(ValueError, match="labels.*bounds"):
            T.label_bounds(cfg)
    for bad in ("exact", "Bounded", 1, None):
        with pytest.raises(ValueError, match="unknown TO labels"):
            T.make_cfg(dict(labels=bad, bounds="conf"))


def test_command_line():
    base = M.train_kwargs(M.parse_args([]))
    assert "labels" not in base[1]["to_cfg"] and base[1]["to_cfg"] == dict(path="default")
    _, kw = M.train_kwargs(M.parse_args(["--to-labels", "bounded", "--to-bounds", "conf"]))
    assert kw["to_cfg"] == dict(path="default", bounds="conf", labels="bounded")
    args = M.parse_args(["--to-labels", "bounded", "--to-bounds", "conf", "--seeds", "0,1"])
    assert args["seeds"] == [0, 1] and M.train_kwargs(args)[1]["to_cfg"]["labels"] == "bounded"
    _, kw = M.train_kwargs(M.parse_args(["--to-labels", "reference"]))
    assert kw["to_cfg"] == dict(path="default", labels="reference")
    for argv in (["--to-labels", "bounded"], ["--to-labels", "bounded", "--to-bounds", "none"], ["--to-labels", "x"]):
        with pytest.raises(SystemExit) as ex:
            M.parse_args(argv)
        assert ex.value.code == 2
