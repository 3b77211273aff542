"""ctypes binding of libcacto_hip.so (include/cacto_hip.h).

This is the thin boundary layer: structs mirror the C header, every call checks the return code
and raises with `cacto_last_error()`. There is no fallback: if the library is missing or fails to
load, importing anything that needs it raises (the product path is the HIP path only).
"""
import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CACTO_HIP_LIB", os.path.join(HERE, "libcacto_hip.so"))
HEADER = os.path.join(HERE, "..", "include", "cacto_hip.h")

CACTO_DYN_SINGLE_INTEGRATOR, CACTO_DYN_CHAIN, CACTO_DYN_CAR, CACTO_DYN_CAR_PARK = 0, 1, 2, 3
CACTO_REW_PLANAR, CACTO_REW_MANIPULATOR, CACTO_REW_UR5, CACTO_REW_CAR_PARK = 0, 1, 2, 3
CACTO_NET_ACTOR, CACTO_NET_CRITIC = 0, 1
MAX_STATE, MAX_ACTION, MAX_JOINTS, JOINT_COLS = 16, 8, 6, 27


class SysParams(C.Structure):
    _fields_ = [
        ("dyn_kind", C.c_int32), ("reward_kind", C.c_int32), ("nb_state", C.c_int32),
        ("nb_action", C.c_int32), ("nq", C.c_int32), ("nv", C.c_int32), ("normalize", C.c_int32),
        ("n_joints", C.c_int32), ("ee_parent", C.c_int32), ("n_check", C.c_int32),
        ("n_weights", C.c_int32), ("const_dyn", C.c_int32),
        ("dt", C.c_double), ("state_norm", C.c_double * MAX_STATE), ("u_max", C.c_double * MAX_ACTION),
        ("w_b", C.c_double), ("scale", C.c_double), ("offset", C.c_double), ("alpha", C.c_double),
        ("alpha2", C.c_double), ("obs", C.c_double * 18), ("target", C.c_double * 3),
        ("w_running", C.c_double * 8), ("w_terminal", C.c_double * 8), ("L_delta", C.c_double),
        ("tau_delta", C.c_double), ("k_db", C.c_double), ("check_points", C.c_double * 20),
        ("ee_R", C.c_double * 9), ("ee_p", C.c_double * 3), ("gravity", C.c_double * 3),
    ]


class Nets(C.Structure):
    _fields_ = [
        ("actor_d", C.c_void_p), ("actor_m_d", C.c_void_p), ("actor_v_d", C.c_void_p),
        ("critic_d", C.c_void_p), ("critic_m_d", C.c_void_p), ("critic_v_d", C.c_void_p),
        ("target_d", C.c_void_p), ("step_d", C.c_void_p),
    ]


class UpdateCfg(C.Structure):
    _fields_ = [
        ("w_S", C.c_double), ("tau", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double),
        ("epsilon", C.c_double), ("critic_lr", C.c_double * 5), ("actor_lr", C.c_double * 5),
        ("lr_bounds", C.c_double * 4), ("MC", C.c_int32), ("B_global", C.c_int32),
        ("want_target_V", C.c_int32), ("pad", C.c_int32),
    ]


class ToCfg(C.Structure):
    """cacto_to_cfg: the iLQR solver's settings (cacto_to_solve)."""
    _fields_ = [
        ("max_iter", C.c_int32), ("max_ls", C.c_int32), ("gtol", C.c_double), ("armijo", C.c_double),
        ("mu_min", C.c_double), ("mu_up", C.c_double), ("mu_down", C.c_double), ("mu_max", C.c_double),
        ("poll_every", C.c_int32), ("path", C.c_int32),
    ]


class ToOpts(C.Structure):
    """cacto_to_opts: per-call options of the trajectory optimiser (the `_opts` entries)."""
    _fields_ = [("hessian", C.c_int32), ("reserved", C.c_int32 * 3)]


class ToBox(C.Structure):
    """cacto_to_box: hard control limits of the trajectory optimiser (the `_box` entries)."""
    _fields_ = [("mode", C.c_int32), ("reserved", C.c_int32), ("lo", C.c_double * MAX_ACTION),
                ("hi", C.c_double * MAX_ACTION)]


class ToPlan(C.Structure):
    """cacto_to_plan: what cacto_to_solve runs for a system and a config (cacto_to_solve_plan)."""
    _fields_ = [("on_device", C.c_int32), ("block_threads", C.c_int32), ("lds_bytes", C.c_int32),
                ("launches_per_iter", C.c_int32)]


class RoPlan(C.Structure):
    """cacto_ro_plan: what cacto_rollout_sched runs for a batch and a schedule (cacto_rollout_plan)."""
    _fields_ = [("kind", C.c_int32), ("groups", C.c_int32), ("workgroups", C.c_int32),
                ("block_threads", C.c_int32), ("lds_bytes", C.c_int32), ("cus", C.c_int32)]


class UpdPlan(C.Structure):
    """cacto_upd_plan: which kernels the update calls run for a batch (cacto_update_plan)."""
    _fields_ = [(n, C.c_int32) for n in (
        "Bp", "chain_tile", "elu", "paired",
        "critic_rows", "critic_chunk", "critic_nch", "critic_gemm", "critic_xcd", "critic_adam_nch",
        "actor_rows", "actor_chunk", "actor_nch", "actor_gemm", "actor_xcd", "actor_adam_nch",
        "xcd_tiles", "pair_xcds", "per_overlap", "devwait_actor", "cus")]


class EnsPlan(C.Structure):
    """cacto_ens_plan: what cacto_ensemble_update launches for R replicas (cacto_ensemble_plan)."""
    _fields_ = [(n, C.c_int32) for n in (
        "supported", "reason", "R", "Bp", "pair_xcds", "xcd_groups", "layers", "xcds",
        "chain_wgs", "chain_wgs_lone", "chain_threads", "chain_lds_bytes",
        "wgrad_wgs", "wgrad_wgs_critic", "wgrad_wgs_actor", "wgrad_threads", "wgrad_lds_bytes",
        "launches_per_update", "cus")]


ENSEMBLE_MAX = 64
ENS_OK, ENS_BAD_R, ENS_NOT_PAIRED, ENS_ELU, ENS_BAD_B = 0, 1, 2, 3, 4
CACTO_EINVAL, CACTO_EUNSUPPORTED = -1, -4


class PerPlan(C.Structure):
    """struct cacto_per_plan: which PER kernels a batch takes on a tree (cacto_per_plan)."""
    _fields_ = [(n, C.c_int32) for n in (
        "sampler", "sampler_top", "sampler_wgs", "count_deferred", "update", "update_sub", "update_roots",
        "overlap_shape")]


RO_KIND_TEAM, RO_KIND_TWO_TEAMS, RO_KIND_WAVE_SLOT = 0, 1, 2
WG_FUSED, WG_SPLIT, WG_BIG = 0, 1, 2
CACTO_TO_CONVERGED, CACTO_TO_MAXITER, CACTO_TO_FAILED = 0, 1, 2
CACTO_TO_PATH_DEFAULT, CACTO_TO_PATH_WAVE = 0, 1
CACTO_TO_HESS_EXACT, CACTO_TO_HESS_PSD = 0, 1
CACTO_TO_BOUNDS_NONE, CACTO_TO_BOUNDS_BOX = 0, 1
CACTO_TO_STARTS_MAX = 16     # candidates per episode of a multi-start solve (cacto_to_starts / cacto_to_select)
PER_UPDATE_SET, PER_UPDATE_SUB, PER_UPDATE_CHAIN = 0, 1, 2
# columns of cacto_validate's per_ep / totals (CACTO_VAL_* in the header)
(CACTO_VAL_ROWS, CACTO_VAL_SUM_G, CACTO_VAL_SUM_G2, CACTO_VAL_SUM_V, CACTO_VAL_SSE_V, CACTO_VAL_SSE_G,
 CACTO_VAL_SUM_L2, CACTO_VAL_SSE_CLOG, CACTO_VAL_SSE_U) = range(9)
CACTO_VAL_COLS = CACTO_VAL_SSE_U + MAX_ACTION
PER_RUN_SUB, PER_RUN_EMPTY = 256, 0x7f7f7f7f

vp, i32, i64, dbl, flt, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_float, C.c_size_t
_SIGS = {
    "cacto_last_error": (C.c_char_p, []),
    "cacto_abi_version": (C.c_int, []),
    "cacto_sys_create": (C.c_int, [C.POINTER(SysParams), vp, C.POINTER(vp)]),
    "cacto_sys_destroy": (C.c_int, [vp]),
    "cacto_sys_set_critic_type": (C.c_int, [vp, C.c_int]),
    "cacto_env_step_batch": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]),
    "cacto_env_ee": (C.c_int, [vp, vp, vp, C.c_int, vp]),
    "cacto_env_step": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]),
    "cacto_env_jacobians": (C.c_int, [vp, vp, vp, C.c_int, vp, vp, vp]),
    "cacto_env_bound_control_cost": (C.c_int, [vp, vp, vp, C.c_int, vp]),
    "cacto_mlp_param_count": (i64, [vp, C.c_int]),
    "cacto_mlp_netbuf_floats": (i64, [vp, C.c_int]),
    "cacto_mlp_pack": (C.c_int, [vp, C.c_int, vp, vp]),
    "cacto_actor_forward": (C.c_int, [vp, vp, vp, vp, C.c_int, vp]),
    "cacto_critic_forward": (C.c_int, [vp, vp, vp, vp, C.c_int, vp]),
    "cacto_critic_input_grad": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, vp]),
    "cacto_workspace_bytes": (sz, [vp, C.c_int]),
    "cacto_update_plan": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(UpdPlan)]),
    "cacto_critic_grad": (C.c_int, [vp, C.POINTER(Nets), C.POINTER(UpdateCfg), vp, vp, vp, C.c_int, vp, vp,
                                    vp, vp, vp, sz, vp]),
    "cacto_actor_grad": (C.c_int, [vp, C.POINTER(Nets), C.POINTER(UpdateCfg), vp, vp, C.c_int, vp, vp, sz, vp]),
    "cacto_adam_step": (C.c_int, [vp, C.POINTER(Nets), C.POINTER(UpdateCfg), C.c_int, vp, C.c_int, vp]),
    "cacto_soft_update": (C.c_int, [vp, C.POINTER(Nets), flt, vp]),
    "cacto_update": (C.c_int, [vp, C.POINTER(Nets), C.POINTER(UpdateCfg), vp, vp, vp, C.c_int, vp, vp, vp,
                               vp, sz, vp]),
    "cacto_pipeline_status": (C.c_int, [vp, vp]),
    "cacto_pipeline_check": (C.c_int, [vp, vp]),
    "cacto_update_n": (C.c_int, [vp, C.POINTER(Nets), C.POINTER(UpdateCfg), vp, vp, C.c_int, C.c_int, vp, sz, vp]),
    "cacto_update_n_per": (C.c_int, [vp, C.POINTER(Nets), C.POINTER(UpdateCfg), vp, vp, vp, i64, i64, C.c_double, vp,
                                     vp, C.c_double, C.c_double, C.c_double, vp, C.c_int, C.c_int, vp, sz, vp]),
    "cacto_ensemble_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.POINTER(EnsPlan)]),
    "cacto_ensemble_create": (C.c_int, [vp, C.c_int, C.POINTER(Nets), C.POINTER(vp), C.POINTER(vp), sz,
                                        C.POINTER(UpdateCfg), C.c_int, C.POINTER(vp)]),
    "cacto_ensemble_destroy": (C.c_int, [vp]),
    "cacto_ensemble_update": (C.c_int, [vp, vp, C.c_int, vp]),
    "cacto_ensemble_outputs": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(vp)]),
    "cacto_workspace_yv_offset": (sz, [vp, C.c_int]),
    "cacto_dp_unique_ids": (C.c_int, [vp, C.c_int]),
    "cacto_dp_attach": (C.c_int, [vp, vp, C.c_int, C.c_int]),
    "cacto_dp_detach": (C.c_int, [vp]),
    "cacto_update_n_dp": (C.c_int, [vp, C.POINTER(Nets), C.POINTER(UpdateCfg), vp, vp, C.c_int, C.c_int, vp, sz,
                                    vp]),
    "cacto_update_n_per_dp": (C.c_int, [vp, C.POINTER(Nets), C.POINTER(UpdateCfg), vp, vp, vp, i64, i64, C.c_double,
                                        vp, vp, C.c_double, C.c_double, C.c_double, vp, C.c_int, C.c_int, vp, sz,
                                        vp]),
    "cacto_update_pair_grads": (C.c_int, [vp, C.POINTER(Nets), C.POINTER(UpdateCfg), vp, vp, vp, vp, C.c_int, vp, vp,
                                          vp, vp, sz, vp]),
    "cacto_update_pair_grads_stage": (C.c_int, [vp, C.POINTER(Nets), C.POINTER(UpdateCfg), vp, vp, vp, vp, C.c_int,
                                                vp, vp, vp, vp, sz, C.c_int, vp]),
    "cacto_update_pair_apply": (C.c_int, [vp, C.POINTER(Nets), C.POINTER(UpdateCfg), vp, C.c_int, C.c_int, C.c_int,
                                          vp]),
    "cacto_rollout": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]),
    "cacto_rollout_sched": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int,
                                      C.c_int, C.c_int, vp]),
    "cacto_rollout_plan": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(RoPlan)]),
    "cacto_rollout_rewards": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp]),
    "cacto_ddp_backward": (C.c_int, [vp, vp, i64, vp, i64, vp, C.c_int, C.c_double, vp, vp]),
    "cacto_ddp_backward_box": (C.c_int, [vp, vp, i64, vp, i64, vp, C.c_int, C.c_double, vp, vp, C.POINTER(ToBox)]),
    "cacto_to_backward_gains": (C.c_int, [vp, vp, i64, vp, i64, vp, C.c_int, C.c_double, vp, vp, vp, vp, vp]),
    "cacto_to_forward": (C.c_int, [vp, vp, i64, vp, i64, vp, vp, vp, C.c_int, C.c_double, vp, vp, vp, vp]),
    "cacto_to_workspace_bytes": (sz, [vp, C.c_int, i64]),
    "cacto_to_workspace_bytes_cfg": (sz, [vp, C.c_int, i64, C.POINTER(ToCfg)]),
    "cacto_to_solve": (C.c_int, [vp, vp, vp, i64, vp, C.c_int, i64, C.POINTER(ToCfg), vp, vp, vp, vp, vp, vp, vp, sz,
                                 vp]),
    "cacto_to_solve_plan": (C.c_int, [vp, C.POINTER(ToCfg), C.POINTER(ToPlan)]),
    "cacto_to_backward_gains_opts": (C.c_int, [vp, vp, i64, vp, i64, vp, C.c_int, C.c_double, vp, vp, vp, vp, vp,
                                               C.POINTER(ToOpts)]),
    "cacto_to_workspace_bytes_opts": (sz, [vp, C.c_int, i64, C.POINTER(ToCfg), C.POINTER(ToOpts)]),
    "cacto_to_solve_opts": (C.c_int, [vp, vp, vp, i64, vp, C.c_int, i64, C.POINTER(ToCfg), vp, vp, vp, vp, vp, vp, vp,
                                      sz, vp, C.POINTER(ToOpts)]),
    "cacto_to_solve_plan_opts": (C.c_int, [vp, C.POINTER(ToCfg), C.POINTER(ToPlan), C.POINTER(ToOpts)]),
    "cacto_to_backward_gains_box": (C.c_int, [vp, vp, i64, vp, i64, vp, C.c_int, C.c_double, vp, vp, vp, vp, vp,
                                              C.POINTER(ToOpts), C.POINTER(ToBox)]),
    "cacto_to_forward_box": (C.c_int, [vp, vp, i64, vp, i64, vp, vp, vp, C.c_int, C.c_double, vp, vp, vp, vp,
                                       C.POINTER(ToBox)]),
    "cacto_to_workspace_bytes_box": (sz, [vp, C.c_int, i64, C.POINTER(ToCfg), C.POINTER(ToOpts), C.POINTER(ToBox)]),
    "cacto_to_solve_box": (C.c_int, [vp, vp, vp, i64, vp, C.c_int, i64, C.POINTER(ToCfg), vp, vp, vp, vp, vp, vp, vp,
                                     sz, vp, C.POINTER(ToOpts), C.POINTER(ToBox)]),
    "cacto_to_solve_plan_box": (C.c_int, [vp, C.POINTER(ToCfg), C.POINTER(ToPlan), C.POINTER(ToOpts),
                                          C.POINTER(ToBox)]),
    "cacto_to_starts": (C.c_int, [vp, vp, vp, i64, vp, C.c_int, C.c_int, dbl, C.c_int, vp, C.c_int, C.c_uint64, vp, vp,
                                  vp, vp]),
    "cacto_to_select": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, i64, i64, C.c_int, vp, vp, vp, vp,
                                  vp, vp, vp, vp, vp, vp, vp]),
    "cacto_buffer_add": (C.c_int, [vp, vp, i64, i64, vp, i64, vp]),
    "cacto_rl_solve_add": (C.c_int, [vp, vp, i64, vp, i64, vp, vp, vp, C.c_int, C.c_int, i64, C.c_int, C.c_int, vp,
                                     i64, i64, vp, vp]),
    "cacto_env_rl_episodes": (C.c_int, [vp, vp, vp, i64, vp, C.c_int, i64, vp, vp, vp, vp]),
    "cacto_collect_plan": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
    "cacto_episode_returns": (C.c_int, [vp, i64, vp, C.c_int, C.c_int, vp, vp]),
    "cacto_validate_workspace_bytes": (sz, [vp, i64]),
    "cacto_validate": (C.c_int, [vp, vp, vp, vp, i64, vp, i64, vp, i64, C.c_int, vp, vp, vp, C.c_int, i64, vp, vp,
                                 vp, sz, vp]),
    "cacto_buffer_gather": (C.c_int, [vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]),
    "cacto_per_init": (C.c_int, [vp, vp, i64, vp]),
    "cacto_per_set_range": (C.c_int, [vp, vp, i64, i64, i64, i64, dbl, vp]),
    "cacto_per_set_range_max": (C.c_int, [vp, vp, i64, i64, i64, i64, vp, dbl, vp]),
    "cacto_per_sample": (C.c_int, [vp, vp, i64, i64, dbl, vp, C.c_int, vp, vp, vp, vp]),
    "cacto_per_plan": (C.c_int, [i64, C.c_int, C.POINTER(PerPlan)]),
    "cacto_per_sample_runs": (C.c_int, [vp, vp, i64, i64, dbl, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp]),
    "cacto_per_shard_stats": (C.c_int, [vp, vp, i64, vp, vp]),
    "cacto_per_sample_global": (C.c_int, [vp, vp, i64, i64, dbl, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]),
    "cacto_per_update": (C.c_int, [vp, vp, i64, vp, vp, vp, vp, dbl, dbl, dbl, vp, C.c_int, vp]),
    "cacto_per_set_leaves": (C.c_int, [vp, vp, i64, vp, vp, C.c_int, vp]),
    "cacto_per_update_relo": (C.c_int, [vp, vp, i64, vp, vp, vp, vp, vp, dbl, dbl, dbl, vp, vp, vp, C.c_int, vp]),
}


def header_exports():
    """Names of every function declared in include/cacto_hip.h."""
    with open(HEADER) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(cacto_[a-z0-9_]+)\s*\(", text)))


class _Lib:
    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise RuntimeError("libcacto_hip.so not found at %s — build it with `python -m cacto_amd.build` "
                               "(there is no CPU fallback)" % path)
        self.path = path
        self.dll = C.CDLL(path)
        # CACTO_LIB_PARTIAL=1 (diagnostics only: A/B runs against libraries of older revisions)
        # binds the symbols the library has and skips the rest
        partial = os.environ.get("CACTO_LIB_PARTIAL") == "1"
        for name, (res, args) in _SIGS.items():
            if partial and not hasattr(self.dll, name):
                continue
            fn = getattr(self.dll, name)
            fn.restype = res
            fn.argtypes = args
        if self.dll.cacto_abi_version() != 1:
            raise RuntimeError("libcacto_hip.so ABI mismatch")

    def call(self, name, *args):
        rc = getattr(self.dll, name)(*args)
        if rc != 0:
            msg = self.dll.cacto_last_error().decode(errors="replace")
            raise RuntimeError("%s failed (%d): %s" % (name, rc, msg))
        return rc

    def raw(self, name):
        return getattr(self.dll, name)


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _Lib()
    return _LIB
