"""CPU-side checks of the ensemble entries (R independent learners of one system in one update
call): the header declares them, the library exports and binds them with explicit argtypes, the plan
answers without a GPU and reports the one-learner route's workgroup counts at R = 1, every refusal
that needs no handle returns its code and message, and the plan struct matches _lib.py. The two
refusals that need a live system handle are checked at the C boundary on the GPU, in
tests/test_gpu_ensemble_update.py: a workspace that is too small (test_refusals) and a handle with
RCCL communicators attached (test_a_data_parallel_handle_is_refused_by_the_library)."""
import ctypes
import re

import pytest

from cacto_amd import _lib as L

NAMES = ("cacto_ensemble_plan", "cacto_ensemble_create", "cacto_ensemble_destroy", "cacto_ensemble_update",
         "cacto_ensemble_outputs", "cacto_workspace_yv_offset")
NFIELDS = 19


def _plan(ns, na, ctype, sob, B, R, cus=256):
    p = L.EnsPlan(*([-7] * NFIELDS))
    rc = L.lib().raw("cacto_ensemble_plan")(ns, na, ctype, sob, B, R, cus, ctypes.byref(p))
    return rc, p, L.lib().dll.cacto_last_error().decode()


def test_header_declares_the_entries_and_the_library_exports_and_binds_them():
    lib = L.lib()
    for name in NAMES:
        assert name in L.header_exports() and name in L._SIGS and hasattr(lib.dll, name), name
        assert getattr(lib.dll, name).argtypes is not None, name
        assert list(getattr(lib.dll, name).argtypes) == L._SIGS[name][1], name
    assert lib.raw("cacto_ensemble_plan").argtypes[7] is ctypes.POINTER(L.EnsPlan)
    assert lib.dll.cacto_abi_version() == 1


def test_plan_struct_and_constants_match_the_header():
    assert ctypes.sizeof(L.EnsPlan) == NFIELDS * 4
    with open(L.HEADER) as f:
        text = f.read()
    body = re.search(r"typedef struct \{([^}]*)\} cacto_ens_plan;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [("int32_t", name) for name, _ in L.EnsPlan._fields_]
    defs = dict(re.findall(r"#define (CACTO_E\w+) (-?\d+)", text))
    assert int(defs["CACTO_ENSEMBLE_MAX"]) == L.ENSEMBLE_MAX >= 16
    for k, v in dict(CACTO_ENS_OK=L.ENS_OK, CACTO_ENS_BAD_R=L.ENS_BAD_R, CACTO_ENS_NOT_PAIRED=L.ENS_NOT_PAIRED,
                     CACTO_ENS_ELU=L.ENS_ELU, CACTO_ENS_BAD_B=L.ENS_BAD_B, CACTO_EINVAL=L.CACTO_EINVAL,
                     CACTO_EUNSUPPORTED=L.CACTO_EUNSUPPORTED).items():
        assert int(defs[k]) == v, k


def _pair_xcds(Bp):
    """The documented rule of cacto_upd_plan.pair_xcds: about 8 tiles of 2 Bp / 4 per XCD."""
    nx = 1
    while nx < 8 and 2 * (Bp // 4) > 8 * nx:
        nx *= 2
    return nx


def _wa_stride(ns, na, mode):
    """k_wgrad_adam's work-list stride, restated from its description ("The learner's
    optimiser half"; the comment above cacto_build_wgrad_adam_items): per layer the IT x OT weight
    tiles are cut into bi x bo = 8 blocks as square as the tile grid allows, block k to XCD bin k, a
    layer's bias tiles to the bin of their out-tile block; the bins are padded to a common multiple
    of 4. mode 0: the sine critic (ns, 64, 64, 128, 128, 1), 1: the actor (ns, 256, 256, na), 2: both."""
    nets = {0: [[ns, 64, 64, 128, 128, 1]], 1: [[ns, 256, 256, na]]}
    nets[2] = nets[0] + nets[1]
    bins = [0] * 8
    for dims in nets[mode]:
        for d_in, d_out in zip(dims[:-1], dims[1:]):
            IT, OT = -(-d_in // 16), -(-d_out // 16)
            bi, best = None, None
            for c in (1, 2, 4, 8):
                if c > IT or 8 // c > OT:
                    continue
                d = abs(IT / c - OT / (8 // c))
                if best is None or d < best:
                    best, bi = d, c
            if bi is None:
                bi = max(1, min(IT, 8))
            bo = max(1, 8 // bi)
            for it in range(IT):
                for ot in range(OT):
                    bins[(((it * bi) // IT) * bo + min(bo - 1, (ot * bo) // OT)) % 8] += 1
            for ot in range(OT):
                bins[min(bo - 1, (ot * bo) // OT) % 8] += 1
    return max(4, -(-max(bins) // 4) * 4)


# (ns, na): double integrator (5, 2), manipulator (7, 3)
@pytest.mark.parametrize("ns,na", [(5, 2), (7, 3)])
@pytest.mark.parametrize("B", [4, 20, 64, 128, 512])
def test_one_replica_reports_the_one_learner_routes_workgroups(ns, na, B):
    rc, p, _ = _plan(ns, na, 0, 1, B, 1)
    assert rc == 0 and p.supported == 1 and p.reason == L.ENS_OK and p.R == 1
    Bp = (B + 15) // 16 * 16
    nx = _pair_xcds(Bp)
    nct = Bp // 4
    assert (p.Bp, p.pair_xcds, p.xcd_groups, p.layers, p.xcds) == (Bp, nx, 8 // nx, 1, nx)
    # k_chain_pair_q4's grid: 8 * ceil(2 nct / nx) workgroups of 512 threads
    assert p.chain_wgs == 8 * -(-2 * nct // nx) and p.chain_wgs_lone == 8 * -(-nct // nx)
    assert (p.chain_threads, p.wgrad_threads, p.launches_per_update, p.cus) == (512, 256, 2, 256)
    # k_wgrad_adam's grid: 8 bins of a common stride, a multiple of 4 that holds the fullest bin
    assert (p.wgrad_wgs_critic, p.wgrad_wgs_actor, p.wgrad_wgs) == tuple(8 * _wa_stride(ns, na, m) for m in range(3))
    # every item has a slot: tiles + bias tiles of the 64-64-128-128-1 critic and the 256-256 actor
    critic_items = (1 * 4 + 4) + (4 * 4 + 4) + (4 * 8 + 8) + (8 * 8 + 8) + (8 * 1 + 1)
    actor_items = (1 * 16 + 16) + (16 * 16 + 16) + (16 * 1 + 1)
    assert p.wgrad_wgs_critic >= critic_items and p.wgrad_wgs_actor >= actor_items
    assert p.wgrad_wgs >= critic_items + actor_items
    assert 0 < p.chain_lds_bytes <= 65536 and p.wgrad_lds_bytes == 17408


@pytest.mark.parametrize("B,R", [(128, 10), (64, 10), (64, 3), (4, 16), (20, 2)])
def test_replicas_spread_over_the_xcd_groups(B, R):
    _, one, _ = _plan(5, 2, 0, 1, B, 1)
    rc, p, _ = _plan(5, 2, 0, 1, B, R)
    assert rc == 0 and p.supported == 1
    groups = 8 // one.pair_xcds
    layers = -(-R // groups)
    assert (p.xcd_groups, p.layers) == (groups, layers)
    assert p.xcds == one.pair_xcds * min(R, groups)
    assert p.chain_wgs == one.chain_wgs * layers and p.chain_wgs_lone == one.chain_wgs_lone * layers
    assert p.wgrad_wgs == one.wgrad_wgs * R and p.wgrad_wgs_critic == one.wgrad_wgs_critic * R
    assert p.launches_per_update == 2           # whatever R is


def test_the_plan_does_not_depend_on_the_sobolev_half_for_its_chain_grid():
    a, b = _plan(5, 2, 0, 0, 128, 4)[1], _plan(5, 2, 0, 1, 128, 4)[1]
    assert (a.chain_wgs, a.wgrad_wgs) == (b.chain_wgs, b.wgrad_wgs)


@pytest.mark.parametrize("args,code,reason,msg", [
    ((5, 2, 0, 1, 1024, 2), L.CACTO_EUNSUPPORTED, L.ENS_NOT_PAIRED, "not paired"),
    ((5, 2, 0, 1, 513, 2), L.CACTO_EUNSUPPORTED, L.ENS_NOT_PAIRED, "not paired"),
    ((5, 2, 2, 1, 64, 2), L.CACTO_EUNSUPPORTED, L.ENS_ELU, "elu critic"),
    ((5, 2, 0, 1, 64, 0), L.CACTO_EINVAL, L.ENS_BAD_R, "CACTO_ENSEMBLE_MAX"),
    ((5, 2, 0, 1, 64, L.ENSEMBLE_MAX + 1), L.CACTO_EINVAL, L.ENS_BAD_R, "CACTO_ENSEMBLE_MAX"),
    ((5, 2, 0, 1, 0, 2), L.CACTO_EINVAL, L.ENS_BAD_B, "B must be positive"),
])
def test_refusals_return_their_code_reason_and_message(args, code, reason, msg):
    rc, p, err = _plan(*args)
    assert rc == code and p.supported == 0 and p.reason == reason and msg in err
    assert p.chain_wgs == 0 and p.wgrad_wgs == 0


def test_the_cap_itself_is_accepted():
    rc, p, _ = _plan(5, 2, 0, 1, 64, L.ENSEMBLE_MAX)
    assert rc == 0 and p.supported == 1 and p.R == L.ENSEMBLE_MAX


def test_null_arguments_are_refused_without_a_gpu():
    lib = L.lib()
    with pytest.raises(RuntimeError, match="cacto_ensemble_plan: bad arguments"):
        lib.call("cacto_ensemble_plan", 5, 2, 0, 1, 64, 2, 256, None)
    with pytest.raises(RuntimeError, match="cacto_ensemble_plan: bad arguments"):
        lib.call("cacto_ensemble_plan", 99, 2, 0, 1, 64, 2, 256, ctypes.byref(L.EnsPlan()))
    h = ctypes.c_void_p()
    with pytest.raises(RuntimeError, match="cacto_ensemble_create: bad arguments"):
        lib.call("cacto_ensemble_create", None, 2, None, None, None, 0, None, 64, ctypes.byref(h))
    with pytest.raises(RuntimeError, match="cacto_ensemble_update: bad arguments"):
        lib.call("cacto_ensemble_update", None, None, 1, None)
    with pytest.raises(RuntimeError, match="cacto_ensemble_outputs: bad arguments"):
        lib.call("cacto_ensemble_outputs", None, 0, None, None)
    assert lib.call("cacto_ensemble_destroy", None) == 0
    assert lib.raw("cacto_workspace_yv_offset")(None, 64) == 0


def test_main_parser_takes_seeds_and_refuses_the_combinations():
    from cacto_amd import main as M
    a = M.parse_args(["--system-id", "double_integrator", "--seeds", "0,1,2", "--test-n", "4"])
    assert a["seeds"] == [0, 1, 2] and a["seed"] == 0 and a["test_n"] == 4
    assert "seeds" not in M.parse_args(["--seed", "3"])
    for bad in (["--seeds", "0,1", "--seed", "3"], ["--seed", "3", "--seeds", "0,1"], ["--seeds", "0,1", "--plots"],
                ["--seeds", "0,x"], ["--seeds", "1,1"]):
        with pytest.raises(SystemExit):
            M.parse_args(bad)
