"""GPU checks of the bound-aware Sobolev labels (cacto_ddp_backward_box, TO.backward_pass with
`bounds`, the TO cfg key `labels`) against tests/ddp_box_ref.py, which cuts the free block out with
index sets where the kernels mask. The tolerance is test_gpu_ddp.py's rule with that helper in the
oracle's place; a trajectory on which no control is held must give the unbounded call's labels bit
for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import ddp_box_ref as D
import ilqr_box as X
import ilqr_ref as R
from cacto_amd import _lib as L

pytestmark = pytest.mark.gpu

RTOL = 1e-9             # test_gpu_ddp.py's


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


@functools.lru_cache(maxsize=None)
def _to(system):
    from cacto_amd.environment import make_env
    from cacto_amd.to import TO
    conf = R.Problem(system).conf
    return TO(make_env(conf), conf, w_S=1e-2)


def _labels(system, S, U, T, **kw):
    out = _to(system).backward_pass_batch(_dev(S), _dev(U), _dev(np.asarray(T, dtype=np.int32)), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_against_helper(system, P, S, U, T, got, ref, alt):
    n = P.n
    for e in range(len(T)):
        Te = int(T[e])
        if Te < 0:
            assert (got[e] == 0).all(), (system, e)         # a skipped episode: nothing written
            continue
        scale = np.abs(ref[e][:, :n]).max() + 1e-12
        tol = RTOL * scale + 100.0 * np.abs(alt[e][:, :n] - ref[e][:, :n]).max(axis=1, keepdims=True)
        err = np.abs(got[e, :Te + 1, :n] - ref[e][:, :n])
        assert (err <= tol).all(), (system, e, float((err / tol).max()))
        assert (got[e, :Te + 1, n] == 0).all()
        assert (got[e, Te + 1:] == 0).all()                 # rows past Te untouched


# ---------------------------------------------------------------------- 1. parity with the helper
@pytest.mark.parametrize("system,kind", list(D.LABEL_CASES))
def test_bounded_labels_match_the_helper(system, kind):
    P, S, U, T = D.label_inputs(system, kind)
    assert T[4] == 0 and T[5] == -1 and S.shape[1] == {"manipulator": 12, "ur5": 8}.get(system, 24) + 1
    ref, alt, st = D.label_reference(P, S, U, T)
    print(system, kind, st)
    assert D.label_inputs_ok(st), st
    got = _labels(system, S, U, T, bounds=(P.lo, P.hi))
    _check_against_helper(system, P, S, U, T, got, ref, alt)
    # and the bounds took part: the unbounded labels differ on an episode with a held control
    assert not np.array_equal(got, _labels(system, S, U, T))


# ---------------------------------------------------------------------- 2. the fused kernel's grid tail
def test_fused_kernel_second_workgroup_partly_filled():
    system = "double_integrator"
    P, S, U, T = D.label_inputs(system, "conf", n_ep=70, zero=3, skip=11)
    assert len(T) == 70 and T[3] == 0 and T[11] == -1
    ref, alt, st = D.label_reference(P, S, U, T)
    assert st["held"] >= 3
    got = _labels(system, S, U, T, bounds="conf")
    _check_against_helper(system, P, S, U, T, got, ref, alt)


# ---------------------------------------------------------------------- 3. nothing held: bit for bit
@pytest.mark.parametrize("system", ["double_integrator", "car_park", "ur5"])
def test_nothing_held_is_the_unbounded_pass_bit_for_bit(system):
    P = X.BoxProblem(system, "conf")
    S, U, T = R.random_episodes(system)
    T = T.copy()
    T[4], T[5] = 0, -1
    plain = _labels(system, S, U, T)
    assert np.abs(plain).max() > 0
    inf = np.full(P.m, np.inf)
    assert np.array_equal(_labels(system, S, U, T, bounds=(-inf, inf)), plain)
    # inside the conf's box everywhere: random controls up to 1.2 u_max, halved, states re-simulated
    S2, U2 = D.clamped_episodes(P, S, 0.5 * U, T)
    assert np.array_equal(U2, 0.5 * U * (np.arange(U.shape[1])[None, :, None] < np.maximum(T, 0)[:, None, None]))
    assert ((U2 > P.lo) & (U2 < P.hi)).all()
    plain2 = _labels(system, S2, U2, T)
    assert np.array_equal(_labels(system, S2, U2, T, bounds="conf"), plain2)
    # a ToBox of mode NONE through the `_box` entry: the call it extends
    none = L.ToBox()
    none.mode = L.CACTO_TO_BOUNDS_NONE
    none.lo[0], none.hi[0] = 1.0, -1.0                      # not read
    assert np.array_equal(_labels(system, S2, U2, T, bounds=none), plain2)


# ---------------------------------------------------------------------- 4. per-episode API, plumbing
def test_per_episode_api_equals_the_batch_call():
    system = "double_integrator"
    P, S, U, T = D.label_inputs(system, "conf")
    to = _to(system)
    batch = _labels(system, S, U, T, bounds="conf")
    for e in (0, 4):
        Te = int(T[e])
        one = to.backward_pass(Te + 1, S[e, :Te + 1, :-1], U[e, :Te], bounds="conf")
        assert np.array_equal(one, batch[e, :Te + 1])
    assert not np.array_equal(to.backward_pass(int(T[0]) + 1, S[0, :T[0] + 1, :-1], U[0, :T[0]]), batch[0, :T[0] + 1])


def _bounded_di_state():
    """A double-integrator full-solve input whose bounded solution holds a control."""
    from test_gpu_collect import _ics
    ICS, Te = _ics("double_integrator", 8)
    return ICS, Te


def test_to_solve_reads_the_labels_key():
    system = "double_integrator"
    to = _to(system)
    P = X.BoxProblem(system, "conf")
    ICS, Te = _bounded_di_state()
    seen_held = False
    for e in range(len(Te)):
        T = int(Te[e])
        if T < 4:
            continue
        init = np.zeros((T, P.m))
        cfg = dict(R.SOLVE_CFG, path="wave", bounds="conf")
        Ub, Xb, flag_b, _, _, dV_b = to.TO_Solve(ICS[e], None, init, T, cfg=dict(cfg, labels="bounded"))
        Ur, Xr, flag_r, _, _, dV_r = to.TO_Solve(ICS[e], None, init, T, cfg=dict(cfg, labels="reference"))
        Ud, Xd, flag_d, _, _, dV_d = to.TO_Solve(ICS[e], None, init, T, cfg=cfg)
        assert flag_b == flag_r == flag_d == 1
        assert np.array_equal(Ub, Ur) and np.array_equal(Xb, Xr)        # the solver ignores the key
        assert np.array_equal(dV_r, dV_d) and np.array_equal(Ur, Ud)    # "reference" is the default
        assert np.array_equal(dV_b, to.backward_pass(T + 1, Xb, Ub, bounds="conf"))
        assert np.array_equal(dV_r, to.backward_pass(T + 1, Xr, Ur))
        if ((Ub == P.lo) | (Ub == P.hi)).any():
            assert not np.array_equal(dV_b, dV_r)
            seen_held = True
            break
    assert seen_held
    with pytest.raises(ValueError, match="labels.*bounds"):
        to.TO_Solve(ICS[0], None, np.zeros((int(Te[0]), P.m)), int(Te[0]), cfg=dict(R.SOLVE_CFG, labels="bounded"))


def test_compute_samples_writes_the_bounded_labels_into_the_replay_rows():
    from test_gpu_collect import _learner, _new_buffer
    ICS, Te = _bounded_di_state()
    conf, env, rl, to = _learner("double_integrator", 1e-2)
    cfg = dict(R.SOLVE_CFG, path="wave", bounds="conf", labels="bounded")
    buf = _new_buffer(conf)
    res = rl.compute_samples(0, [s for s in ICS], to, buf, cfg=cfg)
    assert res["n_kept"] >= 4
    dev = res["dev"]
    kept = _dev(res["kept"].astype(np.int32))
    want = to.backward_pass_batch(dev["S"], dev["U"], kept, bounds="conf")
    assert torch.equal(dev["dVdx"], want)
    assert not torch.equal(want, to.backward_pass_batch(dev["S"], dev["U"], kept))
    ns, row = conf.nb_state, 0
    store = buf.storage.cpu().numpy()
    want = want.cpu().numpy()
    for e in np.nonzero(res["kept"] >= 0)[0]:
        T = int(res["kept"][e])
        assert np.array_equal(store[row:row + T + 1, 2 * ns + 1:3 * ns + 1], want[e, :T + 1]), e
        row += T + 1
    assert row == res["rows"] == buf.next_idx
    # the reference labels of the same solve differ, the solve does not
    buf2 = _new_buffer(conf)
    res2 = rl.compute_samples(0, [s for s in ICS], to, buf2, cfg=dict(cfg, labels="reference"))
    assert torch.equal(res2["dev"]["U"], dev["U"]) and not torch.equal(res2["dev"]["dVdx"], dev["dVdx"])


# ---------------------------------------------------------------------- 5. the error path
def test_bad_bounds_of_a_real_system_leave_the_output_untouched():
    from cacto_amd.system import dptr, stream
    system = "double_integrator"
    to = _to(system)
    P, S, U, T = D.label_inputs(system, "conf")
    Sd, Ud, Td = _dev(S), _dev(U), _dev(T.astype(np.int32))
    out = torch.full_like(Sd, 7.0)
    bad = L.ToBox()
    bad.mode = L.CACTO_TO_BOUNDS_BOX
    for j in range(P.m):
        bad.lo[j], bad.hi[j] = -1.0, 1.0
    bad.lo[0] = bad.hi[0] = 0.5
    with pytest.raises(RuntimeError, match="bad bounds"):
        L.lib().call("cacto_ddp_backward_box", to.sys.handle, dptr(Sd, torch.float64), Sd.shape[1],
                     dptr(Ud, torch.float64), Ud.shape[1], dptr(Td, torch.int32), len(T), 1e-9,
                     dptr(out, torch.float64), stream(), ctypes.byref(bad))
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    with pytest.raises(ValueError, match="unknown TO bounds"):
        to.backward_pass_batch(Sd, Ud, Td, bounds=([0.5, -1.0], [0.5, 1.0]))
