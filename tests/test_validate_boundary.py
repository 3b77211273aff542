"""CPU-side checks of the validation stage's boundary: the header declares cacto_validate and its
workspace query, the ctypes table binds them and the library exports them; the CACTO_VAL_* column
indices of the ctypes layer are the header's; argument errors are reported without a GPU; the two
options of cacto_amd.main parse, are absent when not given, and go together with --seeds."""
import re

import pytest

from cacto_amd import _lib as L

ENTRIES = ("cacto_validate", "cacto_validate_workspace_bytes")


def test_header_declares_the_entries_and_the_library_exports_them():
    names = L.header_exports()
    lib = L.lib()
    for n in ENTRIES:
        assert n in names and n in L._SIGS and hasattr(lib.dll, n)
    assert lib.dll.cacto_abi_version() == 1


def test_column_indices_match_the_header():
    with open(L.HEADER) as f:
        text = f.read()
    defs = {k: int(v) for k, v in re.findall(r"#define (CACTO_VAL_[A-Z0-9_]+) (\d+)", text)}
    assert set(defs) == {"CACTO_VAL_ROWS", "CACTO_VAL_SUM_G", "CACTO_VAL_SUM_G2", "CACTO_VAL_SUM_V", "CACTO_VAL_SSE_V",
                         "CACTO_VAL_SSE_G", "CACTO_VAL_SUM_L2", "CACTO_VAL_SSE_CLOG", "CACTO_VAL_SSE_U",
                         "CACTO_VAL_COLS"}
    for name, value in defs.items():
        assert getattr(L, name) == value, name
    assert sorted(v for k, v in defs.items() if k != "CACTO_VAL_COLS") == list(range(9))
    max_action = int(re.search(r"#define CACTO_MAX_ACTION (\d+)", text).group(1))
    assert defs["CACTO_VAL_COLS"] == defs["CACTO_VAL_SSE_U"] + max_action == L.CACTO_VAL_SSE_U + L.MAX_ACTION


def test_argument_errors_without_a_gpu():
    lib = L.lib()
    one = 8          # a non-null address that is never dereferenced: every call below is refused first

    def call(sys=one, S=one, U=one, R=one, kept=one, off=one, n_ep=1, rows=0, per_ep=one, totals=one, ld=2):
        return lib.call("cacto_validate", sys, None, None, S, ld, U, ld, R, ld, 1, None, kept, off, n_ep, rows,
                        per_ep, totals, None, 0, None)
    for bad in (dict(sys=None), dict(S=None), dict(U=None), dict(R=None), dict(kept=None), dict(off=None),
                dict(per_ep=None), dict(totals=None), dict(n_ep=0), dict(n_ep=-2), dict(rows=-1), dict(ld=0)):
        with pytest.raises(RuntimeError, match="cacto_validate: bad arguments"):
            call(**bad)
    assert lib.raw("cacto_validate_workspace_bytes")(None, 10) == 0
    assert lib.raw("cacto_validate_workspace_bytes")(one, -1) == 0


def test_main_parser_has_the_two_options():
    from cacto_amd import main as M
    base = M.parse_args([])
    assert "validate" not in base and "validate_csv" not in base
    assert "validate" not in M.train_kwargs(base)[1]
    a = M.parse_args(["--validate"])
    assert a["validate"] is True and "validate_csv" not in a
    assert M.train_kwargs(a)[1] == dict(M.train_kwargs(base)[1], validate=True)
    a = M.parse_args(["--validate", "--validate-csv", "out.csv"])
    assert a["validate"] is True and a["validate_csv"] == "out.csv"
    a = M.parse_args(["--seeds", "3,11", "--validate", "--validate-csv", "out.csv"])
    assert a["seeds"] == [3, 11] and a["validate"] is True and a["validate_csv"] == "out.csv"
    assert M.train_kwargs(a)[1]["validate"] is True
    with pytest.raises(SystemExit):
        M.parse_args(["--validate-csv", "out.csv"])


def test_metrics_from_totals_on_the_host():
    """validation_metrics is host arithmetic: the issue's formulas on a hand-made totals row."""
    import math

    import numpy as np

    from cacto_amd.rl import VALIDATION_KEYS, validation_metrics
    t = np.zeros(L.CACTO_VAL_COLS)
    t[L.CACTO_VAL_ROWS], t[L.CACTO_VAL_SUM_G], t[L.CACTO_VAL_SUM_G2] = 10, 20.0, 90.0
    t[L.CACTO_VAL_SSE_V], t[L.CACTO_VAL_SSE_G], t[L.CACTO_VAL_SUM_L2], t[L.CACTO_VAL_SSE_CLOG] = 5.0, 8.0, 32.0, 2.0
    t[L.CACTO_VAL_SSE_U], t[L.CACTO_VAL_SSE_U + 1] = 16.0, 36.0
    J = np.array([[3.0, 1.0], [5.0, 0.0], [2.0, 4.0]])
    m = validation_metrics(t, J, ns=5, na=2, u_max=np.array([2.0, 3.0]), labels=True, warm="actor")
    assert tuple(m) == VALIDATION_KEYS
    assert m["rows"] == 10 and m["episodes"] == 3 and m["warm"] == "actor"
    assert m["value_rmse"] == math.sqrt(0.5) and m["value_r2"] == 1 - 5.0 / 50.0
    assert m["grad_rmse"] == math.sqrt(8.0 / 40) and m["grad_rel"] == 0.5 and m["sobolev_loss"] == 2.0 / 40
    assert m["actor_rmse_u"] == math.sqrt((4.0 + 4.0) / (7 * 2))
    assert m["warm_cost_mean"] == 10.0 / 3 and m["to_cost_mean"] == 5.0 / 3 and m["gap_mean"] == 5.0 / 3
    assert m["gap_rel_median"] == np.median([2.0, -0.5]) and m["gap_rel_left_out"] == 1
    # nothing kept, no variance, no labels: NaN and None, never an exception
    z = validation_metrics(np.zeros(L.CACTO_VAL_COLS), np.zeros((0, 2)), 5, 2, np.ones(2), False, "zero")
    assert z["rows"] == 0 and z["grad_rmse"] is None and z["grad_rel"] is None and z["sobolev_loss"] is None
    for k in ("value_rmse", "value_r2", "actor_rmse_u", "warm_cost_mean", "to_cost_mean", "gap_mean",
              "gap_rel_median"):
        assert math.isnan(z[k]), k
