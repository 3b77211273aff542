"""CPU-side checks of the trajectory optimiser's path setting (cacto_to_cfg.path, the one-wave-per-
episode kernel of the closed-form family): the header declares cacto_to_workspace_bytes_cfg and the
path enum, the library exports and binds the entry, make_cfg maps the path names, and an unknown
path is refused by cacto_to_solve without a GPU."""
import ctypes
import re

import pytest

from cacto_amd import _lib as L
from cacto_amd.to import DEFAULT_CFG, make_cfg


def test_header_declares_the_sized_workspace_entry_and_the_library_exports_it():
    name = "cacto_to_workspace_bytes_cfg"
    lib = L.lib()
    assert name in L.header_exports() and name in L._SIGS and hasattr(lib.dll, name)
    assert lib.dll.cacto_to_workspace_bytes_cfg.argtypes[3] is ctypes.POINTER(L.ToCfg)
    # no system, no config: 0, like cacto_to_workspace_bytes
    assert lib.dll.cacto_to_workspace_bytes_cfg(None, 4, 8, None) == 0
    assert lib.dll.cacto_to_workspace_bytes_cfg(None, 4, 8, ctypes.byref(make_cfg(dict(path=1)))) == 0
    assert lib.dll.cacto_abi_version() == 1


def test_path_enum_matches_the_header():
    with open(L.HEADER) as f:
        text = f.read()
    enum = dict(re.findall(r"(CACTO_TO_PATH_[A-Z]+) = (\d)", text))
    assert {k: int(v) for k, v in enum.items()} == {"CACTO_TO_PATH_DEFAULT": L.CACTO_TO_PATH_DEFAULT,
                                                    "CACTO_TO_PATH_WAVE": L.CACTO_TO_PATH_WAVE}
    assert (L.CACTO_TO_PATH_DEFAULT, L.CACTO_TO_PATH_WAVE) == (0, 1)
    assert L.ToCfg._fields_[-1] == ("path", ctypes.c_int32) and ctypes.sizeof(L.ToCfg) == 64


def test_make_cfg_maps_the_path_names():
    assert DEFAULT_CFG["path"] == 0 and make_cfg().path == 0
    assert make_cfg(dict(path="wave")).path == 1 and make_cfg(dict(path=1)).path == 1
    assert make_cfg(dict(path="default")).path == 0 and make_cfg(dict(path=0)).path == 0
    with pytest.raises(ValueError, match="path"):
        make_cfg(dict(path="warp"))


def test_unknown_path_is_a_bad_config_without_a_gpu():
    lib = L.lib()
    cfg = make_cfg(dict(path=7))
    assert cfg.path == 7
    with pytest.raises(RuntimeError, match="bad config"):
        lib.call("cacto_to_solve", None, None, None, 1, None, 1, 2, ctypes.byref(cfg), None, None, None, None, None,
                 None, None, 0, None)
    # a known path gets as far as the argument check
    with pytest.raises(RuntimeError, match="bad arguments"):
        lib.call("cacto_to_solve", None, None, None, 1, None, 1, 2, ctypes.byref(make_cfg(dict(path="wave"))), None,
                 None, None, None, None, None, None, 0, None)
