"""CPU-side checks of cacto_per_plan (which PER kernels a batch takes on a tree): the header declares
it and cacto_per_sample_runs, the library exports and binds them, the plan struct has the header's
int32 fields, bad arguments are refused without a GPU, and the route is the rule table of the header's
comment, written out here, at every bound."""
import ctypes
import re

import pytest

from cacto_amd import _lib as L

NAME = "cacto_per_plan"
FIELDS = ("sampler", "sampler_top", "sampler_wgs", "count_deferred", "update", "update_sub", "update_roots",
          "overlap_shape")


def test_header_declares_the_entries_and_the_library_exports_them():
    lib = L.lib()
    for name in (NAME, "cacto_per_sample_runs"):
        assert name in L.header_exports() and name in L._SIGS and hasattr(lib.dll, name)
    assert getattr(lib.dll, NAME).argtypes[2] is ctypes.POINTER(L.PerPlan)
    assert lib.dll.cacto_abi_version() == 1


def test_plan_struct_matches_the_header():
    assert ctypes.sizeof(L.PerPlan) == 8 * 4
    assert tuple(name for name, _ in L.PerPlan._fields_) == FIELDS
    with open(L.HEADER) as f:
        text = f.read()
    body = re.search(r"struct cacto_per_plan \{([^}]*)\};", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [("int32_t", name) for name in FIELDS]


@pytest.mark.parametrize("capacity,B", [(0, 64), (3, 64), (1000, 64), (-1024, 64), (1024, 0), (1024, -1),
                                        (1024, 8193)])
def test_bad_arguments_are_refused_without_a_gpu(capacity, B):
    lib = L.lib()
    plan = L.PerPlan(*([-7] * 8))
    with pytest.raises(RuntimeError, match="cacto_per_plan"):
        lib.call(NAME, capacity, B, ctypes.byref(plan))
    assert all(getattr(plan, f) == -7 for f in FIELDS)


def test_null_out_is_refused():
    with pytest.raises(RuntimeError, match="cacto_per_plan"):
        L.lib().call(NAME, 1024, 64, None)


def expected(capacity, B):
    """The rule table: sub = min(1024, capacity), roots = capacity / sub."""
    sub = min(1024, capacity)
    roots = capacity // sub
    big = B >= 512
    if big and roots <= 1024:
        update = 1          # k_per_update_sub
    elif not big or roots > 2048:
        update = 0          # k_per_set
    else:
        update = 2          # the chain
    return dict(sampler=int(big), sampler_top=8192 if big else 1024, sampler_wgs=-(-B // 256) if big else 1,
                count_deferred=int(big), update=update, update_sub=sub, update_roots=roots,
                overlap_shape=int(big and 512 <= capacity <= 65536))


@pytest.mark.parametrize("capacity", [2, 256, 512, 2 ** 16, 2 ** 17, 2 ** 20, 2 ** 21, 2 ** 22])
@pytest.mark.parametrize("B", [1, 511, 512, 8192])
def test_route_is_the_rule_table(capacity, B):
    plan = L.PerPlan()
    L.lib().call(NAME, capacity, B, ctypes.byref(plan))
    assert {f: getattr(plan, f) for f in FIELDS} == expected(capacity, B)


def test_the_table_names_each_route_where_the_issue_puts_it():
    """The literal corners: the chain serves 2^21 alone; k_per_set takes small batches and 2^22."""
    def upd(capacity, B):
        plan = L.PerPlan()
        L.lib().call(NAME, capacity, B, ctypes.byref(plan))
        return plan.update, plan.overlap_shape
    assert upd(2 ** 20, 512) == (1, 0) and upd(2 ** 21, 512) == (2, 0) and upd(2 ** 22, 512) == (0, 0)
    assert upd(2 ** 20, 511) == (0, 0) and upd(2 ** 21, 511) == (0, 0)
    assert upd(2 ** 16, 512) == (1, 1) and upd(2 ** 17, 512) == (1, 0) and upd(512, 512) == (1, 1)
    assert upd(256, 512) == (1, 0) and upd(2 ** 16, 511) == (0, 0)
