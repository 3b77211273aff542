"""CPU-side checks of cacto_update_plan (which kernels the update calls run for a batch): the header
declares it, the library exports and binds it, the plan struct has the header's int32 fields, and
null arguments are refused without a GPU."""
import ctypes
import re

import pytest

from cacto_amd import _lib as L

NAME = "cacto_update_plan"


def test_header_declares_the_plan_entry_and_the_library_exports_it():
    lib = L.lib()
    assert NAME in L.header_exports() and NAME in L._SIGS and hasattr(lib.dll, NAME)
    assert getattr(lib.dll, NAME).argtypes[3] is ctypes.POINTER(L.UpdPlan)
    assert lib.dll.cacto_abi_version() == 1


def test_plan_struct_matches_the_header():
    assert ctypes.sizeof(L.UpdPlan) == 21 * 4
    with open(L.HEADER) as f:
        text = f.read()
    body = re.search(r"typedef struct \{([^}]*)\} cacto_upd_plan;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [("int32_t", name) for name, _ in L.UpdPlan._fields_]


def test_null_arguments_are_refused_without_a_gpu():
    lib = L.lib()
    plan = L.UpdPlan(*([-7] * 21))
    with pytest.raises(RuntimeError, match="bad arguments"):
        lib.call(NAME, None, 1, 128, ctypes.byref(plan))
    with pytest.raises(RuntimeError, match="bad arguments"):
        lib.call(NAME, None, 1, 128, None)
    assert plan.Bp == -7 and plan.cus == -7
