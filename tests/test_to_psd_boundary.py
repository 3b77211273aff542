"""CPU-side checks of the trajectory optimiser's Hessian option (cacto_to_opts, the four `_opts`
entries): the header declares them and the enum, the library exports and binds them, the ctypes
mirror has the header's layout beside an unchanged cacto_to_cfg, bad options and a null system are
refused without a GPU, and the Python layer maps and checks the `hessian` key."""
import ctypes
import re

import numpy as np
import pytest

from cacto_amd import _lib as L
from cacto_amd import to as T

ENTRIES = ("cacto_to_solve_opts", "cacto_to_workspace_bytes_opts", "cacto_to_solve_plan_opts",
           "cacto_to_backward_gains_opts")


def _opts(hessian=0, reserved=(0, 0, 0)):
    o = L.ToOpts()
    o.hessian = hessian
    for k, v in enumerate(reserved):
        o.reserved[k] = v
    return o


def test_header_declares_the_entries_and_the_library_exports_and_binds_them():
    names = L.header_exports()
    lib = L.lib()
    for n in ENTRIES:
        assert n in names and n in L._SIGS and hasattr(lib.dll, n), n
        fn = getattr(lib.dll, n)
        assert fn.argtypes[-1] is ctypes.POINTER(L.ToOpts), n
        # the arguments of the entry it is named after, plus the options
        base = L._SIGS[n[:-len("_opts")]][1] if n != "cacto_to_workspace_bytes_opts" else L._SIGS["cacto_to_workspace_bytes_cfg"][1]
        assert L._SIGS[n][1][:-1] == base, n
    assert lib.dll.cacto_abi_version() == 1


def test_opts_layout_and_enum_match_the_header():
    with open(L.HEADER) as f:
        text = f.read()
    body = re.search(r"typedef struct \{([^}]*)\} cacto_to_opts;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+)(\[\d+\])?;", body) == [("int32_t", "hessian", ""), ("int32_t", "reserved", "[3]")]
    assert [n for n, _ in L.ToOpts._fields_] == ["hessian", "reserved"]
    assert ctypes.sizeof(L.ToOpts) == 16
    assert ctypes.sizeof(L.ToCfg) == 64                     # the config did not grow
    enum = re.search(r"enum cacto_to_hessian \{([^}]*)\}", text).group(1)
    assert dict((k, int(v)) for k, v in re.findall(r"(CACTO_TO_HESS_[A-Z]+) = (\d)", enum)) == {
        "CACTO_TO_HESS_EXACT": L.CACTO_TO_HESS_EXACT, "CACTO_TO_HESS_PSD": L.CACTO_TO_HESS_PSD}
    assert (L.CACTO_TO_HESS_EXACT, L.CACTO_TO_HESS_PSD) == (0, 1)


@pytest.mark.parametrize("bad", [_opts(2), _opts(-1), _opts(0, (0, 0, 1)), _opts(1, (5, 0, 0))])
def test_bad_options_are_refused_without_a_gpu(bad):
    lib = L.lib()
    cfg = T.make_cfg()
    plan = L.ToPlan(-7, -7, -7, -7)
    o = ctypes.byref(bad)
    with pytest.raises(RuntimeError, match="bad options"):
        lib.call("cacto_to_solve_opts", None, None, None, 1, None, 1, 2, ctypes.byref(cfg), None, None, None, None, None,
                 None, None, 0, None, o)
    with pytest.raises(RuntimeError, match="bad options"):
        lib.call("cacto_to_solve_plan_opts", None, ctypes.byref(cfg), ctypes.byref(plan), o)
    with pytest.raises(RuntimeError, match="bad options"):
        lib.call("cacto_to_backward_gains_opts", None, None, 1, None, 1, None, 1, 0.0, None, None, None, None, None, o)
    assert lib.dll.cacto_to_workspace_bytes_opts(None, 4, 8, ctypes.byref(cfg), o) == 0
    assert (plan.on_device, plan.block_threads, plan.lds_bytes, plan.launches_per_iter) == (-7, -7, -7, -7)


@pytest.mark.parametrize("good", [None, _opts(0), _opts(1)])
def test_a_null_system_is_refused_without_a_gpu(good):
    lib = L.lib()
    cfg = T.make_cfg()
    plan = L.ToPlan(-7, -7, -7, -7)
    o = ctypes.byref(good) if good is not None else None
    with pytest.raises(RuntimeError, match="bad arguments"):
        lib.call("cacto_to_solve_opts", None, None, None, 1, None, 1, 2, ctypes.byref(cfg), None, None, None, None, None,
                 None, None, 0, None, o)
    with pytest.raises(RuntimeError, match="null config"):
        lib.call("cacto_to_solve_opts", None, None, None, 1, None, 1, 2, None, None, None, None, None, None, None, None, 0,
                 None, o)
    with pytest.raises(RuntimeError, match="bad arguments"):
        lib.call("cacto_to_solve_plan_opts", None, ctypes.byref(cfg), ctypes.byref(plan), o)
    with pytest.raises(RuntimeError, match="bad arguments"):
        lib.call("cacto_to_backward_gains_opts", None, None, 1, None, 1, None, 1, 0.0, None, None, None, None, None, o)
    assert lib.dll.cacto_to_workspace_bytes_opts(None, 4, 8, ctypes.byref(cfg), o) == 0
    assert lib.dll.cacto_to_workspace_bytes_opts(None, 4, 8, None, o) == 0


def test_python_maps_and_checks_the_hessian_key():
    assert T.DEFAULT_CFG["hessian"] == "exact" and T.HESSIANS == {"exact": 0, "psd": 1}
    c = T.make_cfg(dict(hessian="psd", max_iter=7))
    assert isinstance(c, L.ToCfg) and ctypes.sizeof(c) == 64 and c.max_iter == 7 and c.path == 0
    assert "hessian" not in [n for n, _ in L.ToCfg._fields_]
    assert not hasattr(c, "opts")                           # the struct carries no hidden option
    o = T.make_opts(dict(hessian="psd", max_iter=7))
    assert isinstance(o, L.ToOpts) and o.hessian == 1 and list(o.reserved) == [0, 0, 0] and T.make_opts(o) is o
    assert T.make_opts().hessian == 0 and T.make_opts(dict(max_iter=3)).hessian == 0 and T.make_opts("exact").hessian == 0
    assert T.make_opts("psd").hessian == 1 and T.make_opts(1).hessian == 1 and T.make_opts(0).hessian == 0
    assert T.make_opts(np.int64(1)).hessian == 1 and T.make_opts(dict(hessian=np.int32(0))).hessian == 0
    # what a call makes of its cfg and opts: a dict's key, an explicit opts over it, a ToCfg with opts
    assert T._cfg_opts(dict(hessian="psd", path="wave"))[0].path == 1
    assert T._cfg_opts(dict(hessian="psd"))[1].hessian == 1 and T._cfg_opts(None)[1].hessian == 0
    assert T._cfg_opts(dict(hessian="psd"), opts="exact")[1].hessian == 0
    assert T._cfg_opts(c)[0] is c and T._cfg_opts(c)[1].hessian == 0 and T._cfg_opts(c, opts=o)[1] is o
    assert T._cfg_opts(L.ToCfg.from_buffer_copy(c), opts="psd")[1].hessian == 1
    for bad in ("spd", 2, -1, 1.0, True, None, np.int64(2)):
        with pytest.raises(ValueError, match="hessian"):
            T.make_cfg(dict(hessian=bad))
    with pytest.raises(ValueError, match="hessian"):
        T._cfg_opts(c, opts="spd")
    with pytest.raises(ValueError, match="hessian"):
        T.make_opts("spd")


def test_command_lines_take_the_option():
    from cacto_amd import main as M
    assert "to_hessian" not in M.parse_args([]) and M.train_kwargs(M.parse_args([]))[1]["to_cfg"] == dict(path="default")
    a = M.parse_args(["--to-hessian", "psd", "--to-path", "wave"])
    assert a["to_hessian"] == "psd"
    assert M.train_kwargs(a)[1]["to_cfg"] == dict(path="wave", hessian="psd")
    assert M.train_kwargs(M.parse_args(["--to-hessian", "exact"]))[1]["to_cfg"] == dict(path="default", hessian="exact")
    with pytest.raises(SystemExit):
        M.parse_args(["--to-hessian", "spd"])
