"""CPU-side checks of cacto_to_solve_plan (what cacto_to_solve runs for a system and a config): the
header declares it, the library exports and binds it, the plan struct has the header's four int32
fields, and a null system or an unknown path is refused without a GPU."""
import ctypes
import re

import pytest

from cacto_amd import _lib as L
from cacto_amd.to import make_cfg

NAME = "cacto_to_solve_plan"


def test_header_declares_the_plan_entry_and_the_library_exports_it():
    lib = L.lib()
    assert NAME in L.header_exports() and NAME in L._SIGS and hasattr(lib.dll, NAME)
    fn = getattr(lib.dll, NAME)
    assert fn.argtypes[1] is ctypes.POINTER(L.ToCfg) and fn.argtypes[2] is ctypes.POINTER(L.ToPlan)
    assert lib.dll.cacto_abi_version() == 1


def test_plan_struct_matches_the_header():
    assert ctypes.sizeof(L.ToPlan) == 16
    with open(L.HEADER) as f:
        text = f.read()
    body = re.search(r"typedef struct \{([^}]*)\} cacto_to_plan;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s+(\w+);", body)
    assert fields == [("int32_t", name) for name, _ in L.ToPlan._fields_]
    assert all(t is ctypes.c_int32 for _, t in L.ToPlan._fields_)
    # neither the config nor the path enum changed
    assert ctypes.sizeof(L.ToCfg) == 64 and (L.CACTO_TO_PATH_DEFAULT, L.CACTO_TO_PATH_WAVE) == (0, 1)


def test_null_arguments_are_refused_without_a_gpu():
    lib = L.lib()
    plan = L.ToPlan(-7, -7, -7, -7)
    with pytest.raises(RuntimeError, match="bad arguments"):
        lib.call(NAME, None, ctypes.byref(make_cfg(dict(path="wave"))), ctypes.byref(plan))
    with pytest.raises(RuntimeError, match="null config"):
        lib.call(NAME, None, None, ctypes.byref(plan))
    assert (plan.on_device, plan.block_threads, plan.lds_bytes, plan.launches_per_iter) == (-7, -7, -7, -7)


def test_unknown_path_is_a_bad_config_without_a_gpu():
    lib = L.lib()
    plan = L.ToPlan()
    with pytest.raises(RuntimeError, match="bad config"):
        lib.call(NAME, None, ctypes.byref(make_cfg(dict(path=7))), ctypes.byref(plan))
