"""GPU checks of the validation stage (cacto_validate, RL_AC.validate_samples, train(validate=True),
train_ensemble(validate=True), --validate / --validate-csv).

The sums are checked against numpy float64 on the outputs of the public network entries
(cacto_critic_input_grad, cacto_actor_forward) for the same float32 rows: the stage's network
passes are those entries' launchers, the terms are formed in float64 from the same numbers, so only
the order of the additions (and the device's log, by a few ulps) may differ. Rows past an episode's
length, and every row of a dropped episode, hold NaN: one read of them poisons a sum.

The loop tests shrink the double integrator as tests/test_gpu_ensemble_train.py does (six episodes
per loop, two loops, BATCH_SIZE 20), with the wave TO path and accept_maxiter."""
import csv
import math

import numpy as np
import pytest
import torch

from cacto_amd import _lib as L
from cacto_amd.confs import load_conf
from cacto_amd.system import dptr, stream

pytestmark = pytest.mark.gpu

KEPT = np.array([-1, 0, 1, 2, 63, 64, 65], dtype=np.int32)   # dropped, no actor row, around a wave's 64 lanes
LD = 70
U52 = 2.0 ** -52
SENTINEL = 7.25
C = L.CACTO_VAL_COLS


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def _offsets(kept):
    off = np.zeros(len(kept) + 1, dtype=np.int64)
    np.cumsum(np.where(kept >= 0, kept.astype(np.int64) + 1, 0), out=off[1:])
    return off


def _clog(x):
    return np.where(x > 0, np.log(np.maximum(x, 1e-7) + 1), -np.log(np.maximum(-x, 1e-7) + 1))


class Case:
    """One system with random networks and the random trajectories of KEPT, NaN where nothing lives."""

    def __init__(self, system, seed):
        from cacto_amd.environment import make_env
        from cacto_amd.neural_network import NN
        self.conf = load_conf(system, fresh=True)
        self.env = make_env(self.conf)
        self.sys = self.env.sys
        self.nn = NN(self.env, self.conf, 1e-2, seed=seed)
        self.actor = self.nn.create_actor()
        self.critic = self.nn.create_critic_sine()
        self.ns, self.na = self.conf.nb_state, self.conf.nb_action
        rng = np.random.default_rng(seed)
        E = len(KEPT)
        self.S = rng.normal(size=(E, LD, self.ns)) * 2.0
        self.U = rng.normal(size=(E, LD, self.na)) * np.asarray(self.conf.u_max, dtype=np.float64) * 0.5
        self.R = rng.normal(size=(E, LD))
        self.dVdx = rng.normal(size=(E, LD, self.ns)) * np.exp(rng.normal(size=(E, LD, self.ns)) * 2.0)
        for e, Te in enumerate(KEPT):
            for a in (self.S, self.U, self.R, self.dVdx):
                a[e, max(Te + 1, 0):] = np.nan
            if Te >= 0:
                self.U[e, Te:] = np.nan             # no control at the terminal state
        self.negate = 1
        self.off = _offsets(KEPT)
        self.rows = int(self.off[-1])
        # the live rows as NN.eval casts them, and the public entries on them
        live = np.concatenate([self.S[e, :Te + 1] for e, Te in enumerate(KEPT) if Te >= 0]).astype(np.float32)
        V, g = self.nn.critic_input_grad(self.critic, live)
        self.V = V.reshape(-1).cpu().numpy().astype(np.float64)
        self.g = g.cpu().numpy().astype(np.float64)
        self.a = self.nn.eval(self.actor, live).cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module", params=["single_integrator", "double_integrator", "ur5"])
def case(request):
    return Case(request.param, seed=17)


def run(case, S=None, U=None, R=None, dVdx="own", kept=KEPT, off=None, rows=None, critic=True, actor=True,
        n_ep=None, ws_short=0, null_kept=False, ld=LD):
    """cacto_validate on the case's arrays (or the given ones); outputs pre-filled with SENTINEL.
    Returns (rc, per_ep, totals)."""
    S = case.S if S is None else S
    U = case.U if U is None else U
    R = case.R if R is None else R
    dVdx = case.dVdx if isinstance(dVdx, str) else dVdx
    off = _offsets(kept) if off is None else off
    rows = int(off[-1]) if rows is None else rows
    E = len(kept) if n_ep is None else n_ep
    per_ep = torch.full((len(kept), C), SENTINEL, dtype=torch.float64, device="cuda")
    totals = torch.full((C,), SENTINEL, dtype=torch.float64, device="cuda")
    need = L.lib().raw("cacto_validate_workspace_bytes")(case.sys.handle, rows)
    ws = torch.empty(need // 4 + 1, dtype=torch.float32, device="cuda")
    S_d, U_d, R_d, kept_d, off_d = _dev(S), _dev(U), _dev(R), _dev(kept), _dev(off)
    l_d = None if dVdx is None else _dev(dVdx)
    rc = L.lib().raw("cacto_validate")(
        case.sys.handle, dptr(case.critic.buf) if critic else None, dptr(case.actor.buf) if actor else None,
        dptr(S_d), ld, dptr(U_d), ld, dptr(R_d), ld, case.negate, dptr(l_d), None if null_kept else dptr(kept_d),
        dptr(off_d), E, rows, dptr(per_ep), dptr(totals), dptr(ws), need - ws_short, stream())
    torch.cuda.synchronize()
    return rc, per_ep.cpu().numpy(), totals.cpu().numpy()


def reference(case, R=None, U=None, dVdx="own"):
    """Every column of every episode in numpy float64 (exact sums of the float64 terms), and the
    bound of the issue per entry: 4 * rows * 2^-52 * sum |terms|, plus for sse_clog the room for a
    device log a few ulps off numpy's."""
    R = case.R if R is None else R
    U = case.U if U is None else U
    dVdx = case.dVdx if isinstance(dVdx, str) else dVdx
    ns, na = case.ns, case.na
    E = len(KEPT)
    ref, mag, extra = np.zeros((E, C)), np.zeros((E, C)), np.zeros((E, C))
    for e, Te in enumerate(KEPT):
        if Te < 0:
            continue
        o = int(case.off[e])
        r = -R[e, :Te + 1] if case.negate else R[e, :Te + 1]
        G = np.empty(Te + 1)
        G[Te] = r[Te]
        for t in range(Te - 1, -1, -1):
            G[t] = r[t] + G[t + 1]
        V, g, a = case.V[o:o + Te + 1], case.g[o:o + Te + 1, :ns - 1], case.a[o:o + Te]
        terms = {L.CACTO_VAL_SUM_G: G, L.CACTO_VAL_SUM_G2: G * G, L.CACTO_VAL_SUM_V: V,
                 L.CACTO_VAL_SSE_V: (V - G) ** 2}
        if dVdx is not None:
            l = dVdx[e, :Te + 1, :ns - 1]
            cg, cl = _clog(g), _clog(l)
            d = cg - cl
            terms.update({L.CACTO_VAL_SSE_G: (g - l) ** 2, L.CACTO_VAL_SUM_L2: l * l, L.CACTO_VAL_SSE_CLOG: d * d})
            delta = 4 * U52 * np.maximum(np.abs(cg), np.abs(cl))
            extra[e, L.CACTO_VAL_SSE_CLOG] = (2 * np.abs(d) * delta + delta ** 2).sum()
        for j in range(na):
            terms[L.CACTO_VAL_SSE_U + j] = (a[:, j] - U[e, :Te, j]) ** 2
        ref[e, L.CACTO_VAL_ROWS] = Te + 1
        for c, x in terms.items():
            ref[e, c] = math.fsum(x.ravel())
            mag[e, c] = math.fsum(np.abs(x).ravel())
    n = np.where(KEPT >= 0, KEPT + 1, 0).astype(np.float64)[:, None]
    tol = 4 * n * U52 * mag + extra
    tol_tot = 4 * n.sum() * U52 * mag.sum(axis=0) + extra.sum(axis=0)
    return ref, tol, tol_tot


def _sequential(per_ep):
    tot = np.zeros(per_ep.shape[1])
    for row in per_ep:
        tot = tot + row
    return tot


# ---------------------------------------------------------------------- 1. the sums
def test_sums_against_the_public_entries(case):
    rc, per_ep, totals = run(case)
    assert rc == 0
    ref, tol, tol_tot = reference(case)
    print("max |err| / tol:", (np.abs(per_ep - ref)[tol > 0] / tol[tol > 0]).max())
    np.testing.assert_array_equal(per_ep[:, L.CACTO_VAL_ROWS], np.where(KEPT >= 0, KEPT + 1, 0))
    np.testing.assert_array_equal(per_ep[0], np.zeros(C))                 # the dropped episode
    np.testing.assert_array_equal(per_ep[:, L.CACTO_VAL_SSE_U + case.na:], 0.0)
    np.testing.assert_array_equal(per_ep[1, L.CACTO_VAL_SSE_U:], 0.0)     # Te = 0: no actor row
    assert np.isfinite(per_ep).all() and np.isfinite(totals).all()
    assert (np.abs(per_ep - ref) <= tol).all(), np.argwhere(np.abs(per_ep - ref) > tol)
    # every column is really compared: the networks, the labels and the controls all differ
    live = ref[KEPT >= 1]
    for c in list(range(1, L.CACTO_VAL_SSE_U)) + [L.CACTO_VAL_SSE_U + j for j in range(case.na)]:
        assert (np.abs(live[:, c]) > 0).all(), c
    # the totals: the documented order exactly, and the reference within the bound
    np.testing.assert_array_equal(totals, _sequential(per_ep))
    assert (np.abs(totals - _sequential(ref)) <= tol_tot).all()


# ---------------------------------------------------------------------- 2. exact zeros
def test_exact_zeros_when_the_data_is_the_networks_own(case):
    ns = case.ns
    dVdx, U, R = case.dVdx.copy(), case.U.copy(), case.R.copy()
    Gmax = 0.0
    for e, Te in enumerate(KEPT):
        if Te < 0:
            continue
        o = int(case.off[e])
        dVdx[e, :Te + 1] = case.g[o:o + Te + 1]
        U[e, :Te] = case.a[o:o + Te]
        V = case.V[o:o + Te + 1]
        r = V.copy()
        r[:Te] = V[:Te] - V[1:]                # G_t = r_t + G_{t+1} = V_t
        R[e, :Te + 1] = -r                      # negate = 1
        Gmax = max(Gmax, np.abs(V).max())
    rc, per_ep, totals = run(case, U=U, R=R, dVdx=dVdx)
    assert rc == 0
    for c in [L.CACTO_VAL_SSE_G, L.CACTO_VAL_SSE_CLOG] + [L.CACTO_VAL_SSE_U + j for j in range(case.na)]:
        np.testing.assert_array_equal(per_ep[:, c], 0.0)
        assert totals[c] == 0.0
    assert (per_ep[2:, L.CACTO_VAL_SUM_L2] > 0).all()
    # sse_V: V is float32, so r_t = V_t - V_{t+1} is exact in float64 unless the two exponents are more
    # than 29 binades apart, and then G_t = r_t + V_{t+1} is V_t itself and the sum is 0. Where a
    # difference does round, G_t is off by an ulp or two of the largest |G|; 4 ulps per row, squared:
    n = np.where(KEPT >= 0, KEPT + 1, 0)
    assert (per_ep[:, L.CACTO_VAL_SSE_V] <= n * (U52 * Gmax) ** 2 * 16).all()
    assert totals[L.CACTO_VAL_SSE_V] <= n.sum() * (U52 * Gmax) ** 2 * 16
    np.testing.assert_allclose(per_ep[:, L.CACTO_VAL_SUM_G], per_ep[:, L.CACTO_VAL_SUM_V], rtol=1e-12, atol=0)


# ---------------------------------------------------------------------- 3. determinism, embedding
def test_two_calls_and_a_larger_batch_give_the_same_bits(case):
    rc, per_ep, totals = run(case)
    rc2, per_ep2, totals2 = run(case)
    assert rc == 0 and rc2 == 0
    assert np.array_equal(per_ep, per_ep2) and np.array_equal(totals, totals2)
    E, at = 12, 3
    kept = np.full(E, -1, dtype=np.int32)
    kept[at:at + len(KEPT)] = KEPT

    def embed(a):
        out = np.full((E,) + a.shape[1:], np.nan)
        out[at:at + len(KEPT)] = a
        return out
    rc3, big, totals3 = run(case, S=embed(case.S), U=embed(case.U), R=embed(case.R), dVdx=embed(case.dVdx), kept=kept)
    assert rc3 == 0
    assert np.array_equal(big[at:at + len(KEPT)], per_ep) and np.array_equal(totals3, totals)
    np.testing.assert_array_equal(big[:at], 0.0)
    np.testing.assert_array_equal(big[at + len(KEPT):], 0.0)


# ---------------------------------------------------------------------- 4. null parts, refusals
def test_null_parts_and_refusals(case):
    rc, full, full_tot = run(case)
    assert rc == 0
    cols = lambda *c: sorted(set(c))
    su = [L.CACTO_VAL_SSE_U + j for j in range(L.MAX_ACTION)]
    labels = cols(L.CACTO_VAL_SSE_G, L.CACTO_VAL_SUM_L2, L.CACTO_VAL_SSE_CLOG)
    critic = cols(L.CACTO_VAL_SUM_V, L.CACTO_VAL_SSE_V, L.CACTO_VAL_SSE_G, L.CACTO_VAL_SSE_CLOG)
    for kw, zero in ((dict(dVdx=None), labels), (dict(critic=False), critic), (dict(actor=False), su)):
        rc, per_ep, totals = run(case, **kw)
        assert rc == 0, kw
        same = [c for c in range(C) if c not in zero]
        np.testing.assert_array_equal(per_ep[:, zero], 0.0, err_msg=str(kw))
        np.testing.assert_array_equal(totals[zero], 0.0, err_msg=str(kw))
        assert np.array_equal(per_ep[:, same], full[:, same]) and np.array_equal(totals[same], full_tot[same]), kw
    # nothing kept: the outputs are zeroed, nothing else runs
    none = np.full(len(KEPT), -1, dtype=np.int32)
    rc, per_ep, totals = run(case, kept=none)
    assert rc == 0 and not per_ep.any() and not totals.any()
    # refused before anything is enqueued: the outputs keep what they held
    for kw in (dict(ws_short=1), dict(n_ep=0), dict(null_kept=True), dict(rows=-1), dict(ld=0)):
        rc, per_ep, totals = run(case, **kw)
        assert rc == L.CACTO_EINVAL, kw
        assert (per_ep == SENTINEL).all() and (totals == SENTINEL).all(), kw
    assert b"cacto_validate" in L.lib().dll.cacto_last_error()


# ---------------------------------------------------------------------- 5. the stage in the loop
OVER = dict(EP_UPDATE=6, UPDATE_LOOPS=np.array([8, 8]), BATCH_SIZE=20)
TO_CFG = dict(path="wave")
W_S = 1e-2
SEEDS = (3, 11)
quiet = lambda *_: None


def _conf(path=None):
    conf = load_conf("double_integrator", fresh=True)
    for k, v in OVER.items():
        setattr(conf, k, v)
    if path is not None:
        conf.NNs_path = str(path)
    return conf


def _train(seed=0, N_try=0, w_S=W_S, **kw):
    from cacto_amd import main as M
    return M.train(_conf(), seed=seed, N_try=N_try, w_S=w_S, to_cfg=TO_CFG, accept_maxiter=True, log=quiet, **kw)


@pytest.fixture(scope="module")
def solo():
    """train(validate=True) per seed of SEEDS (N_try = its position), shared by the loop tests."""
    return [_train(seed=s, N_try=r, validate=True) for r, s in enumerate(SEEDS)]


def test_the_stage_changes_nothing_that_is_trained(solo):
    on = solo[0]
    off = _train(seed=SEEDS[0], N_try=0)
    assert off["validation"] == []
    a, b = on["RLAC"], off["RLAC"]
    for name in ("actor_model", "critic_model", "target_critic"):
        assert torch.equal(getattr(a, name).buf, getattr(b, name).buf), name
    for name in ("actor_m", "actor_v", "critic_m", "critic_v", "steps"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(on["buffer"].storage, off["buffer"].storage)
    np.testing.assert_array_equal(on["ep_reward_arr"], off["ep_reward_arr"])
    assert on["counts_per_loop"] == off["counts_per_loop"] and on["update_step_counter"] == 16

    val = on["validation"]
    assert len(val) == 2 and [v["warm"] for v in val] == ["zero", "actor"]
    assert [v["ep"] for v in val] == [0, 1] and [v["update_step_counter"] for v in val] == [0, 8]
    for v, c in zip(val, on["counts_per_loop"]):
        assert v["rows"] == c["rows"] and v["episodes"] == c["n_kept"]
        for k in ("value_rmse", "value_r2", "grad_rmse", "grad_rel", "sobolev_loss", "actor_rmse_u", "gap_mean",
                  "gap_rel_median", "warm_cost_mean", "to_cost_mean"):
            assert isinstance(v[k], float) and math.isfinite(v[k]), (k, v[k])


def test_the_first_loops_numbers_from_the_public_entries(monkeypatch):
    """What validate_samples stored in loop 0, recomputed at that moment (the networks as they were)
    from res["dev"] with cacto_critic_input_grad and cacto_actor_forward, in numpy."""
    from cacto_amd.rl import RL_AC
    real = RL_AC.validate_samples
    seen = []

    def spy(self, res, pre, sol, kept_d, off_d, S_rows, R_sum, negate):
        out = real(self, res, pre, sol, kept_d, off_d, S_rows, R_sum, negate)
        if not seen:
            kept = kept_d.cpu().numpy()
            dev = res["dev"]
            S, U, Rw, l = (x.cpu().numpy() for x in (S_rows, dev["U"], R_sum, dev["dVdx"]))
            live = np.concatenate([S[e, :Te + 1] for e, Te in enumerate(kept) if Te >= 0]).astype(np.float32)
            V, g = self.NN.critic_input_grad(self.critic_model, live)
            a = self.NN.eval(self.actor_model, live)
            seen.append(dict(kept=kept, S=S, U=U, R=Rw, l=l, negate=negate, V=V.reshape(-1).cpu().numpy().astype(float),
                             g=g.cpu().numpy().astype(float), a=a.cpu().numpy().astype(float),
                             J=sol["J"].cpu().numpy(), per_ep=dev["validation"].cpu().numpy(), got=dict(out),
                             rows=res["rows"]))
        return out
    monkeypatch.setattr(RL_AC, "validate_samples", spy)
    out = _train(seed=0, n_loops=1, validate=True)
    d = seen[0]
    conf = out["RLAC"].conf
    ns, na, u_max = conf.nb_state, conf.nb_action, np.asarray(conf.u_max, dtype=float)
    kept, off = d["kept"], _offsets(d["kept"])
    assert d["per_ep"].shape == (conf.EP_UPDATE, C) and off[-1] == d["rows"] == d["got"]["rows"]
    sse_V = sum_G = sum_G2 = sse_g = sum_l2 = sse_c = su = 0.0
    for e, Te in enumerate(kept):
        if Te < 0:
            continue
        o = int(off[e])
        r = -d["R"][e, :Te + 1] if d["negate"] else d["R"][e, :Te + 1]
        G = np.cumsum(r[::-1])[::-1]
        V, g, a = d["V"][o:o + Te + 1], d["g"][o:o + Te + 1, :ns - 1], d["a"][o:o + Te]
        l = d["l"][e, :Te + 1, :ns - 1]
        sse_V += ((V - G) ** 2).sum()
        sum_G += G.sum()
        sum_G2 += (G * G).sum()
        sse_g += ((g - l) ** 2).sum()
        sum_l2 += (l * l).sum()
        sse_c += ((_clog(g) - _clog(l)) ** 2).sum()
        su += (((a - d["U"][e, :Te]) / u_max) ** 2).sum()
    rows, n = float(off[-1]), int((kept >= 0).sum())
    J = d["J"][kept >= 0]
    want = dict(value_rmse=math.sqrt(sse_V / rows), value_r2=1 - sse_V / (sum_G2 - sum_G ** 2 / rows),
                grad_rmse=math.sqrt(sse_g / (rows * (ns - 1))), grad_rel=math.sqrt(sse_g / sum_l2),
                sobolev_loss=sse_c / (rows * (ns - 1)), actor_rmse_u=math.sqrt(su / ((rows - n) * na)))
    got = out["validation"][0]
    assert got["warm"] == "zero" and got["episodes"] == n and got["ep"] == 0
    for k, v in want.items():
        # sums of a few hundred float64 terms in another order: far inside 1e-10 relative (value_r2
        # divides by a variance formed as a difference of sums, the loosest of them)
        assert abs(got[k] - v) <= 1e-10 * max(abs(v), 1.0), (k, got[k], v)
    assert got["warm_cost_mean"] == float(J[:, 0].mean()) and got["to_cost_mean"] == float(J[:, 1].mean())
    assert got["gap_mean"] == float((J[:, 0] - J[:, 1]).mean())
    nz = J[:, 1] != 0
    assert got["gap_rel_median"] == float(np.median((J[:, 0] - J[:, 1])[nz] / np.abs(J[:, 1][nz])))
    assert got["gap_rel_left_out"] == int((~nz).sum())


def test_no_labels_no_gradient_numbers():
    out = _train(seed=0, w_S=0.0, n_loops=1, validate=True)
    v = out["validation"][0]
    assert v["grad_rmse"] is None and v["grad_rel"] is None and v["sobolev_loss"] is None
    assert math.isfinite(v["value_rmse"]) and math.isfinite(v["actor_rmse_u"]) and v["rows"] > 0


# ---------------------------------------------------------------------- 6. the ensemble
def test_ensemble_validation_equals_each_seeds_own_and_the_csv(solo, tmp_path, monkeypatch):
    from cacto_amd import main as M
    conf = _conf(tmp_path / "nns")
    monkeypatch.setattr(M, "load_conf", lambda system_id: conf)
    path = tmp_path / "val.csv"
    outs = M.main(["--system-id", "double_integrator", "--w-S", str(W_S), "--to-path", "wave", "--accept-maxiter",
                   "--seeds", ",".join(str(s) for s in SEEDS), "--validate", "--validate-csv", str(path)])
    assert [o["seed"] for o in outs] == list(SEEDS)
    for got, ref in zip(outs, solo):
        assert len(got["validation"]) == len(ref["validation"]) == 2
        for a, b in zip(got["validation"], ref["validation"]):
            assert list(a) == list(b)
            for k in a:
                assert a[k] == b[k], (got["seed"], k, a[k], b[k])
        assert torch.equal(got["RLAC"].critic_model.buf, ref["RLAC"].critic_model.buf)
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 2 * 2
    assert [(int(r["seed"]), int(r["N_try"]), int(r["ep"])) for r in rows] == [(3, 0, 0), (3, 0, 1), (11, 1, 0),
                                                                             (11, 1, 1)]
    for r, v in zip(rows, [v for o in outs for v in o["validation"]]):
        assert float(r["value_rmse"]) == v["value_rmse"] and r["warm"] == v["warm"]
        assert int(r["rows"]) == v["rows"] and int(r["update_step_counter"]) == v["update_step_counter"]
