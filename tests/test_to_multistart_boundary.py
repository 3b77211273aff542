"""CPU-side checks of the multi-start TO: the cfg keys and their validation, the struct that must not
grow, the flags of cacto_amd.main, the two entries in the header, the ctypes table and the library,
their argument refusals (reported before anything touches a device), and the numpy restatement
tests/multistart_ref.py itself — the generator's range, its hold blocks, what it depends on — with
hand-made selection cases."""
import ctypes
import re

import numpy as np
import pytest

import multistart_ref as M
from cacto_amd import _lib as L
from cacto_amd import to as T

ENTRIES = ("cacto_to_starts", "cacto_to_select")


# ---------------------------------------------------------------------- cfg keys
def test_defaults_and_struct_size():
    assert T.DEFAULT_CFG["starts"] == 1
    for k in ("starts", "start_sigma", "start_hold", "start_seed"):
        assert k in T.DEFAULT_CFG and k in T.NOT_FIELDS
    assert ctypes.sizeof(L.ToCfg) == 64
    assert T.STARTS_MAX == L.CACTO_TO_STARTS_MAX == 16
    assert T.make_starts() == T.make_starts({}) == T.make_starts(T.make_cfg()) == (1, 0.5, 8, 0)


def test_cfg_keys_are_accepted_and_validated():
    c = T.make_cfg(dict(starts=4, start_sigma=0.25, start_hold=3, start_seed=7, max_iter=30))
    assert isinstance(c, L.ToCfg) and c.max_iter == 30
    assert T.make_starts(dict(starts=16, start_sigma=0.0, start_hold=1, start_seed=-3)) == (16, 0.0, 1, -3)
    assert T.make_starts(dict(starts=np.int32(2)))[0] == 2
    for bad in (dict(starts=0), dict(starts=17), dict(starts=-1), dict(starts=2.0), dict(starts="2"),
                dict(starts=True), dict(start_sigma=-0.1), dict(start_sigma=float("nan")),
                dict(start_sigma=float("inf")), dict(start_sigma="x"), dict(start_hold=0), dict(start_hold=-2),
                dict(start_hold=1.5), dict(start_seed=0.5)):
        with pytest.raises(ValueError, match="TO start"):
            T.make_cfg(bad)
        with pytest.raises(ValueError, match="TO start"):
            T.make_starts(bad)
    with pytest.raises(ValueError, match="unknown TO settings"):
        T.make_cfg(dict(starts=2, start=3))
    with pytest.raises(ValueError, match="unknown TO settings"):
        T.make_cfg(dict(start_sigm=0.1))


def test_stream_key_packs_seed_and_loop():
    assert T.stream_key(0, 0) == 0 and T.stream_key(3, 5) == (3 << 32) | 5
    assert T.stream_key(-1, 1) == (0xFFFFFFFF << 32) | 1
    keys = {T.stream_key(s, ep) for s in range(4) for ep in range(4)}
    assert len(keys) == 16 and all(0 <= k < 2 ** 64 for k in keys)


# ---------------------------------------------------------------------- flags
def test_main_parser_has_the_three_options():
    from cacto_amd import main as Mn
    base = Mn.parse_args([])
    for k in ("to_starts", "to_start_sigma", "to_start_hold"):
        assert k not in base
    assert not {"starts", "start_sigma", "start_hold"} & set(Mn.train_kwargs(base)[1]["to_cfg"])
    a = Mn.parse_args(["--to-starts", "4", "--to-start-sigma", "0.25", "--to-start-hold", "3"])
    assert (a["to_starts"], a["to_start_sigma"], a["to_start_hold"]) == (4, 0.25, 3)
    kw = Mn.train_kwargs(a)[1]
    assert kw["to_cfg"] == dict(Mn.train_kwargs(base)[1]["to_cfg"], starts=4, start_sigma=0.25, start_hold=3)
    T.make_cfg(kw["to_cfg"])
    a = Mn.parse_args(["--seeds", "3,11", "--to-starts", "2"])
    assert a["seeds"] == [3, 11] and Mn.train_kwargs(a)[1]["to_cfg"]["starts"] == 2
    for bad in (["--to-starts", "0"], ["--to-starts", "17"], ["--to-start-sigma", "-1"], ["--to-start-hold", "0"]):
        with pytest.raises(SystemExit):
            Mn.parse_args(bad)


# ---------------------------------------------------------------------- the two entries
def test_header_declares_the_entries_and_the_library_exports_them():
    names = L.header_exports()
    lib = L.lib()
    for n in ENTRIES:
        assert n in names and n in L._SIGS and hasattr(lib.dll, n)
    with open(L.HEADER) as f:
        text = f.read()
    assert int(re.search(r"#define CACTO_TO_STARTS_MAX (\d+)", text).group(1)) == L.CACTO_TO_STARTS_MAX


def test_argument_refusals_without_a_gpu():
    lib = L.lib()
    one = 8              # a non-null address that is never dereferenced: every call below is refused first
    half = (ctypes.c_double * 8)(*([1.0] * 8))

    def starts(sys=one, S0=one, U=one, n=one, E=3, N=2, sigma=0.5, hold=2, hr=half, out=(one, one, one), ldU=4):
        return lib.call("cacto_to_starts", sys, S0, U, ldU, n, E, N, sigma, hold, hr, 1, 5, *out, None)
    for bad, msg in ((dict(sys=None), "null"), (dict(S0=None), "null"), (dict(U=None), "null"), (dict(n=None), "null"),
                     (dict(hr=None), "null"), (dict(out=(None, one, one)), "null"), (dict(out=(one, None, one)), "null"),
                     (dict(out=(one, one, None)), "null"), (dict(N=0), "n_starts"), (dict(N=17), "n_starts"),
                     (dict(N=-1), "n_starts"), (dict(hold=0), "hold"), (dict(hold=-4), "hold"),
                     (dict(sigma=-1e-9), "sigma"), (dict(sigma=float("nan")), "sigma"),
                     (dict(sigma=float("inf")), "sigma"), (dict(E=0), "bad arguments"), (dict(ldU=0), "bad arguments")):
        with pytest.raises(RuntimeError, match=r"cacto_to_starts failed \(-1\): cacto_to_starts: .*" + msg):
            starts(**bad)

    def select(N=2, E=3, ldS=5, ldU=4, null=None):
        p = [one] * 18
        if null is not None:
            p[null] = None
        return lib.call("cacto_to_select", *p[:8], E, N, ldS, ldU, 1, *p[8:], None)
    for i in range(18):
        with pytest.raises(RuntimeError, match=r"cacto_to_select failed \(-1\): cacto_to_select: null"):
            select(null=i)
    for bad, msg in ((dict(N=0), "n_starts"), (dict(N=17), "n_starts"), (dict(E=0), "bad arguments"),
                     (dict(ldS=0), "bad arguments"), (dict(ldU=0), "bad arguments")):
        with pytest.raises(RuntimeError, match="cacto_to_select: .*" + msg):
            select(**bad)


# ---------------------------------------------------------------------- the generator of the reference
def test_mix_is_splitmix64():
    # the first outputs of splitmix64 seeded with 0 and with 1234567 (Vigna's reference implementation:
    # state += golden, output = finaliser(state)), i.e. mix of the state before the increment
    assert int(M.mix(np.uint64(0))) == 0xE220A8397B1DCDAF
    g = 0x9E3779B97F4A7C15
    assert int(M.mix(np.uint64(g))) == 0x6E789E6AA1B965F4
    assert [int(M.mix(np.uint64((1234567 + i * g) % 2 ** 64))) for i in range(2)] == [6457827717110365317,
                                                                                      3203168211198807973]


def test_generator_range_blocks_and_dependence():
    e = np.arange(50)[:, None, None, None]
    c = np.arange(16)[None, :, None, None]
    b = np.arange(40)[None, None, :, None]
    k = np.arange(8)[None, None, None, :]
    x = M.xi(12345, e, c, b, k)
    assert x.shape == (50, 16, 40, 8) and x.dtype == np.float64
    assert x.min() >= -1.0 and x.max() < 1.0
    assert abs(x.mean()) < 0.01 and abs(x.var() - 1.0 / 3.0) < 0.01          # uniform on [-1, 1): 256000 draws
    assert len(np.unique(x)) == x.size                                       # differs across e, c, block and k
    # every value is a multiple of 2^-52: the formula is exact
    assert np.array_equal(x * 2.0 ** 52, np.round(x * 2.0 ** 52))
    for axis in range(4):                                                    # and along each of them alone
        a, bb = np.take(x, 0, axis=axis), np.take(x, 1, axis=axis)
        assert not (a == bb).any()
    y = M.xi(12346, e, c, b, k)
    assert not (x == y).any()                                                # and across the seed
    assert np.array_equal(x, M.xi(12345, e, c, b, k))
    assert np.array_equal(M.xi(-1, 3, 2, 1, 0), M.xi(2 ** 64 - 1, 3, 2, 1, 0))   # the seed is taken modulo 2^64
    # the largest fields the header allows stay apart
    assert M.xi(1, 2 ** 31 - 1, 15, 2 ** 24 - 1, 7) != M.xi(1, 2 ** 31 - 1, 15, 2 ** 24 - 2, 7)


def test_reference_batch_layout_and_hold_blocks():
    rng = np.random.default_rng(0)
    E, ldU, na, ns, N, hold = 5, 7, 2, 5, 4, 3
    S0, U, n = rng.normal(size=(E, ns)), rng.normal(size=(E, ldU, na)), np.array([7, 3, -1, 0, 5], dtype=np.int32)
    half = np.array([2.0, 0.5])
    for zero in (0, 1):
        S0a, Ua, na_ = M.starts(S0, U, n, N, 0.5, hold, half, zero, seed=9)
        assert S0a.shape == (N * E, ns) and Ua.shape == (N * E, ldU, na) and na_.shape == (N * E,)
        assert np.array_equal(Ua[:E], U) and np.array_equal(S0a, np.tile(S0, (N, 1)))
        assert np.array_equal(na_.reshape(N, E), np.tile(n, (N, 1)))
        d = (Ua.reshape(N, E, ldU, na) - U) / (0.5 * half)
        assert np.array_equal(Ua[E:2 * E] == 0.0, np.full((E, ldU, na), bool(zero)))
        for c in range(2 if zero else 1, N):
            assert (np.abs(d[c]) <= 1.0 + 1e-12).all() and (d[c] != 0).all()
            # constant inside a hold block (up to the rounding of U + s xi), different across blocks
            for t0 in range(0, ldU, hold):
                blk = d[c][:, t0:t0 + hold]
                assert np.allclose(blk, blk[:, :1], rtol=0, atol=1e-13)
            assert (np.abs(d[c][:, 0] - d[c][:, hold]) > 1e-9).all()
    a = M.starts(S0, U, n, N, 0.5, hold, half, 1, seed=9)[1]
    b = M.starts(S0, U, n, N, 0.5, hold, half, 1, seed=10)[1]
    assert np.array_equal(a[:2 * E], b[:2 * E]) and not (a[2 * E:] == b[2 * E:]).any()
    # sigma = 0: every perturbed candidate is the warm start
    z = M.starts(S0, U, n, N, 0.0, hold, half, 0, seed=9)[1]
    assert np.array_equal(z, np.tile(U, (N, 1, 1)))


# ---------------------------------------------------------------------- hand-made selection cases
def select_cases():
    """E = 6, N = 3, ldU = 4: (sol_all, nsteps, prefilled out). Costs and statuses per episode
    (candidate 0, 1, 2):
      0  FAILED, FAILED, MAXITER 5   -> none acceptable without accept_maxiter; candidate 2 with it
      1  CONVERGED 3, CONVERGED 3, CONVERGED 4 -> an exact tie: candidate 0
      2  MAXITER 1, CONVERGED 2, CONVERGED 2   -> 1 without accept_maxiter (a tie of 1 and 2), 0 with it
      3  CONVERGED NaN, CONVERGED 7, FAILED 0  -> the NaN is never picked: 1
      4  skipped (Te = -1)
      5  CONVERGED 9, CONVERGED 8, CONVERGED -inf -> -inf is not finite: 1; Te = 2 < ldU (rows past Te)"""
    C_, Mx, F = M.CONVERGED, M.MAXITER, M.FAILED
    E, N, ldU, ns, na = 6, 3, 4, 3, 2
    status = np.array([[F, F, Mx], [C_, C_, C_], [Mx, C_, C_], [C_, C_, F], [C_, C_, C_], [C_, C_, C_]], dtype=np.int32)
    J1 = np.array([[6.0, 6.0, 5.0], [3.0, 3.0, 4.0], [1.0, 2.0, 2.0], [np.nan, 7.0, 0.0], [1.0, 1.0, 1.0],
                   [9.0, 8.0, -np.inf]])
    nsteps = np.array([4, 3, 4, 1, -1, 2], dtype=np.int32)
    rng = np.random.default_rng(1)
    rows = N * E
    sol = dict(S=rng.normal(size=(rows, ldU + 1, ns)), U=rng.normal(size=(rows, ldU, na)),
               step_cost=rng.normal(size=(rows, ldU + 1)), status=status.T.reshape(-1).copy(),
               iters=np.arange(rows, dtype=np.int32) + 10,
               J=np.stack([100.0 + np.arange(rows), J1.T.reshape(-1)], axis=1))
    out = dict(S=np.full((E, ldU + 1, ns), -777.0), U=np.full((E, ldU, na), -777.0),
               step_cost=np.full((E, ldU + 1), -777.0), status=np.full(E, -7, dtype=np.int32),
               iters=np.full(E, -7, dtype=np.int32), J=np.full((E, 2), -777.0))
    return sol, nsteps, out


@pytest.mark.parametrize("accept_maxiter,want_start,want_ok", [(0, [0, 0, 1, 1, -1, 1], [0, 3, 2, 1, 0, 2]),
                                                               (1, [2, 0, 0, 1, -1, 1], [1, 3, 3, 1, 0, 2])])
def test_selection_rule_on_hand_made_cases(accept_maxiter, want_start, want_ok):
    sol, nsteps, out = select_cases()
    E, N = 6, 3
    got = M.select(sol, nsteps, N, accept_maxiter, out)
    assert got["start"].tolist() == want_start and got["n_ok"].tolist() == want_ok
    for e, w in enumerate(want_start):
        Te = int(nsteps[e])
        if w < 0:                                   # skipped: the prefill, everywhere
            for k in ("S", "U", "step_cost", "J"):
                assert (got[k][e] == -777.0).all()
            assert got["status"][e] == -7 and got["iters"][e] == -7
            continue
        row = w * E + e
        assert np.array_equal(got["S"][e, :Te + 1], sol["S"][row, :Te + 1]) and (got["S"][e, Te + 1:] == -777.0).all()
        assert np.array_equal(got["U"][e, :Te], sol["U"][row, :Te]) and (got["U"][e, Te:] == -777.0).all()
        assert np.array_equal(got["step_cost"][e, :Te + 1], sol["step_cost"][row, :Te + 1])
        assert (got["step_cost"][e, Te + 1:] == -777.0).all()
        assert got["status"][e] == sol["status"][row] and got["iters"][e] == sol["iters"][row]
        assert got["J"][e, 0] == sol["J"][e, 0] == 100.0 + e          # candidate 0's warm-start cost
        assert np.array_equal(got["J"][e, 1], sol["J"][row, 1], equal_nan=True)
    assert np.array_equal(got["J_starts"], sol["J"][:, 1].reshape(N, E).T, equal_nan=True)
    assert np.array_equal(got["status_starts"], sol["status"].reshape(N, E).T)
    # the inputs are left as they were
    again = select_cases()
    for k in sol:
        assert np.array_equal(sol[k], again[0][k], equal_nan=True)


def test_multistart_stats_on_the_host():
    from cacto_amd.rl import multistart_stats
    sol, nsteps, out = select_cases()
    got = M.select(sol, nsteps, 3, 1, out)             # starts 2 0 0 1 -1 1
    kept = np.array([4, 3, 4, 1, -1, -1])              # episode 5 dropped by something else
    m = multistart_stats(got, kept, accept_maxiter=True)
    # episode 0: candidate 0 FAILED, won by 2 -> rescued; episode 3: candidate 0's cost is NaN, won by 1 -> rescued
    assert m == dict(starts=3, rescued=2, improved=0, won_by=[2, 1, 1], gain_rel_median=m["gain_rel_median"])
    assert np.isnan(m["gain_rel_median"])
    got = M.select(sol, nsteps, 3, 0, out)             # starts 0 0 1 1 -1 1
    m = multistart_stats(got, np.array([-1, 3, 4, 1, -1, 2]), accept_maxiter=False)
    # episode 2: candidate 0 MAXITER (not acceptable) -> rescued; 5: 9 -> 8, improved by 1/9
    assert m == dict(starts=3, rescued=2, improved=1, won_by=[1, 3, 0], gain_rel_median=(9.0 - 8.0) / 9.0)
