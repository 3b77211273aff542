"""CPU-side checks of the trajectory optimiser's boundary: the header declares its entries and
status enum, the ctypes mirror of cacto_to_cfg has the header's layout, and argument errors are
reported through cacto_last_error without a GPU."""
import ctypes
import os
import re

import pytest

from cacto_amd import _lib as L

ENTRIES = ("cacto_to_backward_gains", "cacto_to_forward", "cacto_to_workspace_bytes", "cacto_to_solve")


def test_header_declares_the_entries_and_the_library_exports_them():
    names = L.header_exports()
    lib = L.lib()
    for n in ENTRIES:
        assert n in names and n in L._SIGS and hasattr(lib.dll, n)


def test_cfg_layout_and_status_enum_match_the_header():
    with open(L.HEADER) as f:
        text = f.read()
    body = re.search(r"typedef struct \{([^}]*)\} cacto_to_cfg;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n.strip()) for t, names in re.findall(r"(int32_t|double)\s+([^;]+);", body) for n in names.split(",")]
    assert [n for _, n in fields] == [n for n, _ in L.ToCfg._fields_]
    assert [t for t, _ in fields] == ["int32_t" if c is ctypes.c_int32 else "double" for _, c in L.ToCfg._fields_]
    assert ctypes.sizeof(L.ToCfg) == 2 * 4 + 6 * 8 + 2 * 4
    enum = dict(re.findall(r"(CACTO_TO_[A-Z]+) = (\d)", text))
    assert {k: int(v) for k, v in enum.items()} == {"CACTO_TO_CONVERGED": L.CACTO_TO_CONVERGED,
                                                    "CACTO_TO_MAXITER": L.CACTO_TO_MAXITER,
                                                    "CACTO_TO_FAILED": L.CACTO_TO_FAILED}
    assert os.path.basename(L.HEADER) == "cacto_hip.h"


def test_argument_errors_without_a_gpu():
    from cacto_amd.to import make_cfg
    lib = L.lib()
    assert lib.dll.cacto_to_workspace_bytes(None, 4, 8) == 0
    with pytest.raises(RuntimeError, match="null config"):
        lib.call("cacto_to_solve", None, None, None, 1, None, 1, 2, None, None, None, None, None, None, None, None, 0,
                 None)
    cfg = make_cfg(dict(max_iter=7))
    assert cfg.max_iter == 7 and cfg.max_ls == 10 and cfg.mu_up == 10.0
    with pytest.raises(RuntimeError, match="bad arguments"):
        lib.call("cacto_to_solve", None, None, None, 1, None, 1, 2, ctypes.byref(cfg), None, None, None, None, None,
                 None, None, 0, None)
    with pytest.raises(RuntimeError, match="cacto_to_forward"):
        lib.call("cacto_to_forward", None, None, 1, None, 1, None, None, None, 1, 1.0, None, None, None, None)
    with pytest.raises(ValueError):
        make_cfg(dict(tolerance=1.0))
