"""MI355X-native batched whole-body-control hot path (host-side Python binding).

Thin ctypes layer over lib/libwbc_hip.so (the C-ABI in include/wbc_hip.h).  PyTorch is used only
for device memory and streams.  There is NO CPU fallback: if the HIP library is missing or no
gfx950 device is present, construction fails loudly.

Mirrors the reference controller's shape (/root/reference/README.md:60: the controller is
started with the URDF path; README.md:11: observer + GRF optimisation per tick):
    model  = Model.from_urdf(path)
    solver = Solver(model, params, dtype="f64", device=0, max_batch=N)
    out    = solver.step(q=..., v=..., w_des=..., ...)      # one control tick for N states
Batch tensors are component-major: shape [ncomp, N] (see include/wbc_hip.h).
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WBC_LIB") or os.path.join(_HERE, "lib", "libwbc_hip.so")
SYNTHETIC_URDF = os.path.join(_HERE, "assets", "synthetic_quadruped.urdf")
WBC_MAXV = 32
F64, F32 = 0, 1
ABI_VERSION = 10   # include/wbc_hip.h: wbc_abi_version()

_lib = None


class WbcError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        detail = lib().wbc_last_error().decode() if _lib is not None else ""
        super().__init__("%s failed: status %d (%s) %s" % (where, code, lib().wbc_strerror(code).decode(), detail))


def build_library(force=False):
    """Compile the HIP library in-tree (hipcc --offload-arch=gfx950)."""
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-s"] + (["-B"] if force else [])
    subprocess.check_call(cmd)
    return LIB_PATH


class Params(C.Structure):
    _fields_ = [("S", C.c_double * 6), ("alpha", C.c_double), ("fn_min", C.c_double), ("fn_max", C.c_double),
                ("mu_scale", C.c_double), ("dt", C.c_double), ("observer_order", C.c_int), ("max_iter", C.c_int),
                ("qp_tol", C.c_double), ("K1", C.c_double * WBC_MAXV), ("K2", C.c_double * WBC_MAXV)]

    @staticmethod
    def default(dtype="f64"):
        p = Params()
        lib().wbc_params_default(C.byref(p), F64 if dtype == "f64" else F32)
        return p

    @staticmethod
    def from_dict(d, dtype="f64"):
        p = Params.default(dtype)
        for i in range(6):
            p.S[i] = float(d["S"][i])
        for k in ("alpha", "fn_min", "fn_max", "mu_scale", "dt", "qp_tol"):
            setattr(p, k, float(d[k]))
        p.observer_order, p.max_iter = int(d["observer_order"]), int(d["max_iter"])
        for i in range(min(len(d["K1"]), WBC_MAXV)):
            p.K1[i] = float(d["K1"][i])
            p.K2[i] = float(d["K2"][i])
        return p


class RefParams(C.Structure):
    """wbc_ref_params: gains of the CoM reference generator (include/wbc_hip.h)."""
    _fields_ = [("kp_com", C.c_double * 3), ("kd_com", C.c_double * 3), ("kp_rot", C.c_double * 3), ("kd_rot", C.c_double * 3),
                ("kp_joint", C.c_double), ("kd_joint", C.c_double), ("inertia_nom", C.c_double * 3),
                ("q_nom", C.c_double * WBC_MAXV)]

    @staticmethod
    def default():
        g = RefParams()
        lib().wbc_ref_params_default(C.byref(g))
        return g

    @staticmethod
    def from_dict(d):
        g = RefParams.default()
        for k in ("kp_com", "kd_com", "kp_rot", "kd_rot", "inertia_nom"):
            for i in range(3):
                getattr(g, k)[i] = float(d[k][i])
        g.kp_joint, g.kd_joint = float(d["kp_joint"]), float(d["kd_joint"])
        for i, x in enumerate(d["q_nom"]):
            g.q_nom[i] = float(x)
        return g


PLAN_WORDS = 12


class SolverOptions(C.Structure):
    """wbc_solver_options (include/wbc_hip.h): the kernel-selection switches of a solver.  The library itself never reads
    the environment; Solver(options=None) builds them from the defaults overridden by the WBC_* variables below -- a
    convenience of THIS binding for the A/B scripts under tools/ and bench.py."""
    _fields_ = [("struct_size", C.c_size_t), ("fused_max", C.c_longlong), ("rollout_persistent", C.c_int),
                ("rollout_spw", C.c_int), ("obs_split_min", C.c_longlong), ("one_zerocopy", C.c_int), ("timing_mode", C.c_int), ("qp_tile", C.c_int), ("obs_split_serial", C.c_int), ("qp_lane", C.c_int), ("f32_pack2", C.c_int), ("keep_structural", C.c_int), ("rollout_warm", C.c_int),
                ("multi_threads", C.c_int), ("multi_spin_us", C.c_int), ("obs_colaunch", C.c_int), ("tile_tick", C.c_int), ("fused_pair", C.c_int)]
    ENV = {"WBC_FUSED_MAX": ("fused_max", int), "WBC_ROLLOUT_PERSISTENT": ("rollout_persistent", int),
           "WBC_ROLLOUT_SPW": ("rollout_spw", int), "WBC_OBS_SPLIT_MIN": ("obs_split_min", int),
           "WBC_ONE_ZEROCOPY": ("one_zerocopy", int), "WBC_QP_TILE": ("qp_tile", int), "WBC_OBS_SPLIT_SERIAL": ("obs_split_serial", int), "WBC_QP_LANE": ("qp_lane", int), "WBC_F32_PACK2": ("f32_pack2", int), "WBC_KEEP_STRUCTURAL": ("keep_structural", int), "WBC_ROLLOUT_WARM": ("rollout_warm", int),
           "WBC_MULTI_THREADS": ("multi_threads", int), "WBC_MULTI_SPIN_US": ("multi_spin_us", int), "WBC_OBS_COLAUNCH": ("obs_colaunch", int), "WBC_TILE_TICK": ("tile_tick", int), "WBC_FUSED_PAIR": ("fused_pair", int),
           "WBC_TIMING": ("timing_mode", lambda v: 1 if v == "pair" else 0)}

    @staticmethod
    def default():
        o = SolverOptions()
        lib().wbc_solver_options_default(C.byref(o))
        return o

    @staticmethod
    def make(options=None):
        """options: None (defaults + WBC_* environment), a dict of field overrides, or a SolverOptions."""
        if isinstance(options, SolverOptions):
            return options
        o = SolverOptions.default()
        if options is None:
            for var, (field, conv) in SolverOptions.ENV.items():
                if var in os.environ:
                    setattr(o, field, conv(os.environ[var]))
        else:
            for k, v in options.items():
                if k not in dict(SolverOptions._fields_) or k == "struct_size":
                    raise KeyError("unknown solver option %r" % k)
                setattr(o, k, int(v))
        return o


class _BatchIn(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("q", "v", "w_des", "vdot_des", "normals", "mu", "mask", "tau_prev", "f_prev")]


class _BatchOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("tau", "f", "status", "iters", "M", "h", "Jc", "pf")]


class TickPlan(C.Structure):
    """wbc_tick_plan (include/wbc_hip.h): which kernels a tick of N states runs."""
    _fields_ = [("struct_size", C.c_size_t), ("fused", C.c_int), ("front", C.c_int), ("qp", C.c_int), ("qp_tile", C.c_int),
                ("qp_body", C.c_int), ("sweep_pack2", C.c_int), ("sweep_block", C.c_int), ("qp_warm", C.c_int)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "struct_size"}


def plan_tick(N, dtype="f64", observer_order=0, options=None, want_mats=True, want_pf=True, warm=False):
    """wbc_plan_tick: the kernels a tick of N states runs with these options (dict of wbc_tick_plan's fields); needs no device."""
    pl = TickPlan()
    pl.struct_size = C.sizeof(TickPlan)
    o = SolverOptions.make({} if options is None else options)
    _check(lib().wbc_plan_tick(F64 if dtype == "f64" else F32, int(observer_order), C.byref(o), int(N), int(want_mats), int(want_pf), int(warm), C.byref(pl)),
           "wbc_plan_tick")
    return pl.as_dict()


def dispatch_thresholds(dtype="f64", observer_order=0, options=None, want_mats=True, warm=False):
    """wbc_dispatch_thresholds: the batch sizes at which the tick's kernels change (warm: those of a warm-started tick), ascending; needs no device."""
    out = (C.c_size_t * 16)()
    n = C.c_int(0)
    o = SolverOptions.make({} if options is None else options)
    _check(lib().wbc_dispatch_thresholds(F64 if dtype == "f64" else F32, int(observer_order), C.byref(o), (1 if want_mats else 0) | (2 if warm else 0), out, 16, C.byref(n)),
           "wbc_dispatch_thresholds")
    return [int(out[i]) for i in range(n.value)]


class _ObsState(C.Structure):
    _fields_ = [("integ", C.c_void_p), ("r", C.c_void_p)]


def lib():
    """Load libwbc_hip.so; fail loudly when it has not been built."""
    global _lib
    if _lib is None:
        # torch first: its bundled libamdhip64.so.7 must be THE HIP runtime of the process, so that device
        # pointers and streams handed over from torch are valid inside the library (same SONAME => shared).
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("HIP library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback for the WBC hot path)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.wbc_strerror.restype = C.c_char_p
        L.wbc_last_error.restype = C.c_char_p
        L.wbc_model_joint_name.restype = C.c_char_p
        L.wbc_model_foot_link.restype = C.c_char_p
        L.wbc_model_total_mass.restype = C.c_double
        L.wbc_model_total_mass.argtypes = [C.c_void_p]
        L.wbc_model_joint_name.argtypes = [C.c_void_p, C.c_int]
        L.wbc_model_foot_link.argtypes = [C.c_void_p, C.c_int]
        L.wbc_model_free.argtypes = [C.c_void_p]
        L.wbc_solver_destroy.argtypes = [C.c_void_p]
        L.wbc_solver_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p]
        L.wbc_solver_create_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]
        L.wbc_solver_options_default.argtypes = [C.c_void_p]
        L.wbc_solver_options_default.restype = None
        L.wbc_observer_init.argtypes = [C.c_void_p] * 5
        L.wbc_one_map.argtypes = [C.c_void_p, C.c_void_p]
        L.wbc_one_tick.argtypes = [C.c_void_p]
        L.wbc_shard_range.argtypes = [C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.wbc_multi_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
        L.wbc_multi_destroy.argtypes = [C.c_void_p]
        L.wbc_multi_destroy.restype = None
        L.wbc_multi_size.argtypes = [C.c_void_p]
        L.wbc_multi_device.argtypes = [C.c_void_p, C.c_int]
        L.wbc_multi_solver.argtypes = [C.c_void_p, C.c_int]
        L.wbc_multi_solver.restype = C.c_void_p
        L.wbc_multi_stream.argtypes = [C.c_void_p, C.c_int]
        L.wbc_multi_stream.restype = C.c_void_p
        L.wbc_multi_rccl_ranks.argtypes = [C.c_void_p]
        L.wbc_multi_set_params.argtypes = [C.c_void_p, C.c_void_p]
        L.wbc_multi_step_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.wbc_multi_step_batch_warm.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.wbc_multi_rollout_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.wbc_multi_allgather_tau.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.wbc_multi_synchronize.argtypes = [C.c_void_p]
        L.wbc_multi_allgather_tau_async.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int]
        L.wbc_multi_gather_wait.argtypes = [C.c_void_p, C.c_int]
        L.wbc_multi_step_host.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.wbc_dynamics_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 9
        L.wbc_step_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 4
        L.wbc_integrate_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 9
        L.wbc_rollout_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_int] + [C.c_void_p] * 6
        L.wbc_ref_params_default.argtypes = [C.c_void_p]
        L.wbc_ref_params_default.restype = None
        L.wbc_solver_set_ref_params.argtypes = [C.c_void_p, C.c_void_p]
        L.wbc_reference_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 3 + [C.c_double] + [C.c_void_p] * 4
        L.wbc_compute_reference.argtypes = [C.c_void_p] * 4 + [C.c_double] + [C.c_void_p] * 3
        L.wbc_rollout_tracking_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_int] + [C.c_void_p] * 8
        L.wbc_integrate_plant_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 9
        L.wbc_rollout_plant_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_int] + [C.c_void_p] * 6
        L.wbc_rollout_tracking_plant_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_int] + [C.c_void_p] * 8
        # scored rollouts: additive to ABI 10, detected by the symbols (a library without them is an older build of the same ABI)
        if not hasattr(L, "wbc_rollout_scored_batch"):
            raise RuntimeError("%s lacks the scored-rollout entry points: rebuild the library (python -c 'import __graft_entry__ as g; g.build()')" % LIB_PATH)
        L.wbc_score_params_default.argtypes = [C.c_void_p]
        L.wbc_score_params_default.restype = None
        L.wbc_solver_set_score_params.argtypes = [C.c_void_p, C.c_void_p]
        L.wbc_rollout_scored_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_int] + [C.c_void_p] * 9
        L.wbc_score_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
        L.wbc_rollout_select.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        # joint torque limits: additive to ABI 10 too, detected by the symbols.  An older build of the same ABI still loads (every other call works
        # on it); the limit calls themselves refuse it (_limit_lib)
        if hasattr(L, "wbc_step_limited_batch"):
            L.wbc_model_effort_limits.argtypes = [C.c_void_p, C.c_void_p]
            L.wbc_solver_set_torque_limits.argtypes = [C.c_void_p, C.c_void_p]
            L.wbc_limit_torques_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 5
            L.wbc_step_limited_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 5
            L.wbc_solver_limited_count.argtypes = [C.c_void_p, C.c_void_p]
        # swing-foot references: additive to ABI 10, detected by the symbols in the same way (_swing_lib)
        if hasattr(L, "wbc_swing_reference_batch"):
            L.wbc_swing_params_default.argtypes = [C.c_void_p]
            L.wbc_swing_params_default.restype = None
            L.wbc_solver_set_swing_params.argtypes = [C.c_void_p, C.c_void_p]
            L.wbc_swing_reference_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 4 + [C.c_double] + [C.c_void_p] * 3
            L.wbc_reference_swing_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 5 + [C.c_double] + [C.c_void_p] * 5
            L.wbc_compute_swing_reference.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
        # gait scheduler: additive to ABI 10, detected by the symbols in the same way (_gait_lib)
        if hasattr(L, "wbc_gait_batch"):
            L.wbc_gait_params_default.argtypes = [C.c_void_p, C.c_void_p]
            L.wbc_gait_params_default.restype = None
            L.wbc_solver_set_gait_params.argtypes = [C.c_void_p, C.c_void_p]
            L.wbc_gait_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 9
            L.wbc_compute_gait.argtypes = [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 4
        # ground-contact plant: additive to ABI 10, detected by the symbols in the same way (_ground_lib)
        if hasattr(L, "wbc_integrate_ground_batch"):
            L.wbc_ground_params_default.argtypes = [C.c_void_p]
            L.wbc_ground_params_default.restype = None
            L.wbc_solver_set_ground_params.argtypes = [C.c_void_p, C.c_void_p]
            L.wbc_ground_force_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 10
            L.wbc_integrate_ground_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 14
        # stiction on the ground plant: additive to ABI 10, detected by the symbols in the same way (_stick_lib)
        if hasattr(L, "wbc_integrate_ground_stick_batch"):
            L.wbc_stiction_params_default.argtypes = [C.c_void_p]
            L.wbc_stiction_params_default.restype = None
            L.wbc_solver_set_stiction_params.argtypes = [C.c_void_p, C.c_void_p]
            L.wbc_ground_stick_force_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 12
            L.wbc_integrate_ground_stick_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 16
        # contact sensing from the observer's residual: additive to ABI 10, detected by the symbols in the same way (_contact_lib)
        if hasattr(L, "wbc_gait_estimated_batch"):
            L.wbc_contact_params_default.argtypes = [C.c_void_p]
            L.wbc_contact_params_default.restype = None
            L.wbc_solver_set_contact_params.argtypes = [C.c_void_p, C.c_void_p]
            L.wbc_contact_estimate_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 9
            L.wbc_gait_estimated_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 14
            L.wbc_compute_contact_estimate.argtypes = [C.c_void_p] * 9
        # terrain heightfield: additive to ABI 10, detected by the symbols in the same way (_terrain_lib)
        if hasattr(L, "wbc_gait_terrain_batch"):
            L.wbc_terrain_sample_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 5
            L.wbc_terrain_feet_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 7
            L.wbc_gait_terrain_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 13
            L.wbc_gait_estimated_terrain_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 17
        # foothold selection: additive to ABI 10, detected by the symbols in the same way (_foothold_lib)
        if hasattr(L, "wbc_gait_terrain_select_batch"):
            L.wbc_foothold_params_default.argtypes = [C.c_void_p]
            L.wbc_foothold_params_default.restype = None
            L.wbc_solver_set_foothold_params.argtypes = [C.c_void_p, C.c_void_p]
            L.wbc_terrain_cost_batch.argtypes = [C.c_void_p] * 4
            L.wbc_foothold_select_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 5
            L.wbc_gait_terrain_select_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 16
            L.wbc_gait_estimated_terrain_select_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 20
        # base state from leg odometry: additive to ABI 10, detected by the symbols in the same way (_odom_lib)
        if hasattr(L, "wbc_gait_estimated_odom_batch"):
            L.wbc_odom_params_default.argtypes = [C.c_void_p]
            L.wbc_odom_params_default.restype = None
            L.wbc_solver_set_odom_params.argtypes = [C.c_void_p, C.c_void_p]
            L.wbc_base_estimate_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 12
            L.wbc_gait_estimated_odom_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 20
            L.wbc_compute_base_estimate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
        # trunk reference from the velocity command: additive to ABI 10, detected by the symbols in the same way (_trunk_lib)
        if hasattr(L, "wbc_reference_cmd_swing_batch"):
            L.wbc_trunk_params_default.argtypes = [C.c_void_p]
            L.wbc_trunk_params_default.restype = None
            L.wbc_solver_set_trunk_params.argtypes = [C.c_void_p, C.c_void_p]
            L.wbc_reference_cmd_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 12
            L.wbc_reference_cmd_swing_batch.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 15
            L.wbc_compute_reference_cmd.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 5
        L.wbc_plan_tick.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.wbc_solver_plan_tick.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.wbc_step_batch_warm.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 6
        L.wbc_dispatch_thresholds.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.wbc_solver_invalidate_structural.argtypes = [C.c_void_p]
        L.wbc_qp_dense_batch.argtypes = [C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_double] + [C.c_void_p] * 5
        # this binding's struct layouts and array sizes are those of ONE header version: refuse any other library
        if L.wbc_abi_version() != ABI_VERSION:
            raise RuntimeError("%s is ABI %d, this binding is written against ABI %d: rebuild the library (python -c 'import __graft_entry__ as g; g.build()')"
                               % (LIB_PATH, L.wbc_abi_version(), ABI_VERSION))
        L.wbc_solver_collect_timing_n.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.wbc_multi_tick_gather.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.wbc_multi_issue_threads.argtypes = [C.c_void_p]
        L.wbc_multi_set_peer_copies.argtypes = [C.c_void_p, C.c_int]
        L.wbc_multi_gather_pushes.argtypes = [C.c_void_p]
        L.wbc_multi_host_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.wbc_multi_probe_issue.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _lib = L
    return _lib


def _limit_lib():
    """lib(), for the torque-limit calls: a library without their symbols is an older build of the same ABI"""
    L = lib()
    if not hasattr(L, "wbc_step_limited_batch"):
        raise RuntimeError("%s lacks the torque-limit entry points: rebuild the library (python -c 'import __graft_entry__ as g; g.build()')" % LIB_PATH)
    return L


def _swing_lib():
    """lib(), for the swing-foot reference calls: a library without their symbols is an older build of the same ABI"""
    L = lib()
    if not hasattr(L, "wbc_swing_reference_batch"):
        raise RuntimeError("%s lacks the swing-reference entry points: rebuild the library (python -c 'import __graft_entry__ as g; g.build()')" % LIB_PATH)
    return L


def _gait_lib():
    """lib(), for the gait scheduler's calls: a library without their symbols is an older build of the same ABI"""
    L = lib()
    if not hasattr(L, "wbc_gait_batch"):
        raise RuntimeError("%s lacks the gait-scheduler entry points: rebuild the library (python -c 'import __graft_entry__ as g; g.build()')" % LIB_PATH)
    return L


def _ground_lib():
    """lib(), for the ground plant's calls: a library without their symbols is an older build of the same ABI"""
    L = lib()
    if not hasattr(L, "wbc_integrate_ground_batch"):
        raise RuntimeError("%s lacks the ground-plant entry points: rebuild the library (python -c 'import __graft_entry__ as g; g.build()')" % LIB_PATH)
    return L


def _stick_lib():
    """lib(), for the stiction calls of the ground plant: a library without their symbols is an older build of the same ABI"""
    L = lib()
    if not hasattr(L, "wbc_integrate_ground_stick_batch"):
        raise RuntimeError("%s lacks the stiction entry points: rebuild the library (python -c 'import __graft_entry__ as g; g.build()')" % LIB_PATH)
    return L


def _contact_lib():
    """lib(), for the contact-estimate calls: a library without their symbols is an older build of the same ABI"""
    L = lib()
    if not hasattr(L, "wbc_gait_estimated_batch"):
        raise RuntimeError("%s lacks the contact-estimate entry points: rebuild the library (python -c 'import __graft_entry__ as g; g.build()')" % LIB_PATH)
    return L


def _terrain_lib():
    """lib(), for the terrain calls: a library without their symbols is an older build of the same ABI"""
    L = lib()
    if not hasattr(L, "wbc_gait_terrain_batch"):
        raise RuntimeError("%s lacks the terrain entry points: rebuild the library (python -c 'import __graft_entry__ as g; g.build()')" % LIB_PATH)
    return L


def _foothold_lib():
    """lib(), for the foothold-selection calls: a library without their symbols is an older build of the same ABI"""
    L = lib()
    if not hasattr(L, "wbc_gait_terrain_select_batch"):
        raise RuntimeError("%s lacks the foothold-selection entry points: rebuild the library (python -c 'import __graft_entry__ as g; g.build()')" % LIB_PATH)
    return L


def _odom_lib():
    """lib(), for the base-estimate calls: a library without their symbols is an older build of the same ABI"""
    L = lib()
    if not hasattr(L, "wbc_gait_estimated_odom_batch"):
        raise RuntimeError("%s lacks the base-estimate entry points: rebuild the library (python -c 'import __graft_entry__ as g; g.build()')" % LIB_PATH)
    return L


def _check(code, where):
    if code != 0:
        raise WbcError(code, where)


PAYLOAD_WORDS = 10   # include/wbc_hip.h: WBC_PAYLOAD_WORDS


class Plant(C.Structure):
    """wbc_plant (ABI 10): what the plant of wbc_*_plant_batch has that the controller's model lacks"""
    _fields_ = [("struct_size", C.c_size_t), ("tau_ext", C.c_void_p), ("payload", C.c_void_p)]


GOAL_WORDS = 10   # include/wbc_hip.h: WBC_GOAL_WORDS -- goal [GOAL_WORDS, N]: g_p (3), g_quat (x, y, z, w), g_v (3)


class ScoreParams(C.Structure):
    """wbc_score_params: the weights of the running cost of the scored rollouts (include/wbc_hip.h)"""
    _fields_ = [("struct_size", C.c_size_t), ("w_tau", C.c_double), ("w_f", C.c_double), ("w_fail", C.c_double),
                ("w_pos", C.c_double * 3), ("w_rot", C.c_double * 3), ("w_vel", C.c_double * 3), ("w_omega", C.c_double * 3),
                ("w_q", C.c_double), ("w_qd", C.c_double), ("terminal", C.c_double), ("q_nom", C.c_double * WBC_MAXV)]

    @staticmethod
    def default():
        p = ScoreParams()
        lib().wbc_score_params_default(C.byref(p))
        return p

    @staticmethod
    def from_dict(d):
        """keys = field names; scalars for the 3-vectors broadcast; missing keys keep the defaults (all 0, w_fail = 1e6, terminal = 1)"""
        p = ScoreParams.default()
        for k, val in d.items():
            if k in ("w_pos", "w_rot", "w_vel", "w_omega"):
                a = np.broadcast_to(np.asarray(val, dtype=np.float64), (3,))
                for i in range(3):
                    getattr(p, k)[i] = float(a[i])
            elif k == "q_nom":
                for i, x in enumerate(np.asarray(val, dtype=np.float64).ravel()):
                    p.q_nom[i] = float(x)
            elif k in ("w_tau", "w_f", "w_fail", "w_q", "w_qd", "terminal"):
                setattr(p, k, float(val))
            else:
                raise KeyError("ScoreParams has no field %r" % k)
        return p


SWING_WORDS = 36   # include/wbc_hip.h: WBC_SWING_WORDS -- swing [SWING_WORDS, N]: per foot k rows 9 k ...: p0 (3), p1 (3), hgt, T, t0
FOOT_WORDS = 24    # include/wbc_hip.h: WBC_FOOT_WORDS -- foot [FOOT_WORDS, N]: per foot k rows 6 k ...: p_f (3), J_k v (3)


class SwingParams(C.Structure):
    """wbc_swing_params: the gains of the swing-foot references (include/wbc_hip.h)"""
    _fields_ = [("struct_size", C.c_size_t), ("kp", C.c_double * 3), ("kd", C.c_double * 3), ("damping", C.c_double)]

    @staticmethod
    def default():
        p = SwingParams()
        _swing_lib().wbc_swing_params_default(C.byref(p))
        return p

    @staticmethod
    def from_dict(d):
        """keys kp, kd (scalars broadcast over the world axes), damping; missing keys keep the defaults (400, 40, 1e-4)"""
        p = SwingParams.default()
        for k, val in d.items():
            if k in ("kp", "kd"):
                a = np.broadcast_to(np.asarray(val, dtype=np.float64), (3,))
                for i in range(3):
                    getattr(p, k)[i] = float(a[i])
            elif k == "damping":
                p.damping = float(val)
            else:
                raise KeyError("SwingParams has no field %r" % k)
        return p


class GroundParams(C.Structure):
    """wbc_ground_params: the contact law of the ground plant (include/wbc_hip.h, "Ground-contact plant")"""
    _fields_ = [("struct_size", C.c_size_t), ("k_n", C.c_double), ("c_n", C.c_double), ("c_t", C.c_double), ("f_touch", C.c_double)]

    @staticmethod
    def default():
        p = GroundParams()
        _ground_lib().wbc_ground_params_default(C.byref(p))
        return p

    @staticmethod
    def from_dict(d):
        """keys k_n, c_n, c_t, f_touch; missing keys keep the defaults"""
        p = GroundParams.default()
        for k, val in d.items():
            if k not in ("k_n", "c_n", "c_t", "f_touch"):
                raise KeyError("GroundParams has no field %r" % k)
            setattr(p, k, float(val))
        return p

    def as_dict(self):
        return dict(k_n=self.k_n, c_n=self.c_n, c_t=self.c_t, f_touch=self.f_touch)


class StictionParams(C.Structure):
    """wbc_stiction_params: the anchor spring of the ground plant's stiction calls (include/wbc_hip.h, "Stiction on the ground plant")"""
    _fields_ = [("struct_size", C.c_size_t), ("k_t", C.c_double)]

    @staticmethod
    def default():
        p = StictionParams()
        _stick_lib().wbc_stiction_params_default(C.byref(p))
        return p

    @staticmethod
    def from_dict(d):
        """key k_t; a missing key keeps the default"""
        p = StictionParams.default()
        for k, val in d.items():
            if k != "k_t":
                raise KeyError("StictionParams has no field %r" % k)
            setattr(p, k, float(val))
        return p

    def as_dict(self):
        return dict(k_t=self.k_t)


class ContactParams(C.Structure):
    """wbc_contact_params: the thresholds of the contact estimate (include/wbc_hip.h, "Contact sensing from the disturbance observer")"""
    _fields_ = [("struct_size", C.c_size_t), ("f_on", C.c_double), ("f_off", C.c_double), ("det_min", C.c_double)]

    @staticmethod
    def default():
        p = ContactParams()
        _contact_lib().wbc_contact_params_default(C.byref(p))
        return p

    @staticmethod
    def from_dict(d):
        """keys f_on, f_off, det_min; missing keys keep the defaults"""
        p = ContactParams.default()
        for k, val in d.items():
            if k not in ("f_on", "f_off", "det_min"):
                raise KeyError("ContactParams has no field %r" % k)
            setattr(p, k, float(val))
        return p

    def as_dict(self):
        return dict(f_on=self.f_on, f_off=self.f_off, det_min=self.det_min)


def _trunk_lib():
    """lib(), for the trunk-reference calls: a library without their symbols is an older build of the same ABI"""
    L = lib()
    if not hasattr(L, "wbc_reference_cmd_swing_batch"):
        raise RuntimeError("%s lacks the trunk-reference entry points: rebuild the library (python -c 'import __graft_entry__ as g; g.build()')" % LIB_PATH)
    return L


TRUNK_WORDS = 6       # include/wbc_hip.h: WBC_TRUNK_WORDS -- trunk [TRUNK_WORDS, N]: x, y, psi, z_s, s_x, s_y
TRUNKREF_WORDS = 10   # include/wbc_hip.h: WBC_TRUNKREF_WORDS -- ref [TRUNKREF_WORDS, N]: c_ref (3), cd_ref (3), quat_des (x, y, z, w)


class TrunkParams(C.Structure):
    """wbc_trunk_params: the trunk reference from the velocity command (include/wbc_hip.h, "Trunk reference from the velocity command")"""
    _fields_ = [("struct_size", C.c_size_t), ("height", C.c_double), ("leash", C.c_double), ("yaw_leash", C.c_double), ("a_s", C.c_double),
                ("tilt", C.c_double), ("nz_min", C.c_double), ("det_min", C.c_double)]
    FIELDS = ("height", "leash", "yaw_leash", "a_s", "tilt", "nz_min", "det_min")

    @staticmethod
    def default():
        p = TrunkParams()
        _trunk_lib().wbc_trunk_params_default(C.byref(p))
        return p

    @staticmethod
    def from_dict(d):
        """keys height, leash, yaw_leash, a_s, tilt, nz_min, det_min; missing keys keep the defaults"""
        p = TrunkParams.default()
        for k, val in d.items():
            if k not in TrunkParams.FIELDS:
                raise KeyError("TrunkParams has no field %r" % k)
            setattr(p, k, float(val))
        return p

    def as_dict(self):
        return {k: getattr(self, k) for k in TrunkParams.FIELDS}


class OdomParams(C.Structure):
    """wbc_odom_params: the blend gains of the base estimate (include/wbc_hip.h, "Base state from leg odometry")"""
    _fields_ = [("struct_size", C.c_size_t), ("a_v", C.c_double), ("a_p", C.c_double)]

    @staticmethod
    def default():
        p = OdomParams()
        _odom_lib().wbc_odom_params_default(C.byref(p))
        return p

    @staticmethod
    def from_dict(d):
        """keys a_v, a_p; missing keys keep the defaults"""
        p = OdomParams.default()
        for k, val in d.items():
            if k not in ("a_v", "a_p"):
                raise KeyError("OdomParams has no field %r" % k)
            setattr(p, k, float(val))
        return p

    def as_dict(self):
        return dict(a_v=self.a_v, a_p=self.a_p)


class FootholdParams(C.Structure):
    """wbc_foothold_params: the weights of the terrain cost map and of the foothold search (include/wbc_hip.h, "Foothold selection")"""
    _fields_ = [("struct_size", C.c_size_t), ("radius", C.c_int), ("margin", C.c_int), ("w_step", C.c_double), ("w_slope", C.c_double),
                ("w_dist", C.c_double), ("cost_ok", C.c_double), ("u_max", C.c_double)]
    _INTS, _REALS = ("radius", "margin"), ("w_step", "w_slope", "w_dist", "cost_ok", "u_max")

    @staticmethod
    def default():
        p = FootholdParams()
        _foothold_lib().wbc_foothold_params_default(C.byref(p))
        return p

    @staticmethod
    def from_dict(d):
        """keys radius, margin (ints), w_step, w_slope, w_dist, cost_ok, u_max; missing keys keep the defaults"""
        p = FootholdParams.default()
        for k, val in d.items():
            if k in FootholdParams._INTS:
                if int(val) != val:
                    raise ValueError("FootholdParams.%s is an integer" % k)
                setattr(p, k, int(val))
            elif k in FootholdParams._REALS:
                setattr(p, k, float(val))
            else:
                raise KeyError("FootholdParams has no field %r" % k)
        return p

    def as_dict(self):
        return {k: getattr(self, k) for k in FootholdParams._INTS + FootholdParams._REALS}


class TerrainStruct(C.Structure):
    """wbc_terrain (include/wbc_hip.h, "Terrain heightfield")"""
    _fields_ = [("struct_size", C.c_size_t), ("nx", C.c_int), ("ny", C.c_int), ("n_tiles", C.c_int), ("x0", C.c_double), ("y0", C.c_double),
                ("cell", C.c_double), ("z", C.c_void_p), ("tile", C.c_void_p)]


class Terrain:
    """A heightfield for the terrain calls: z [n_tiles, ny, nx] (or [ny, nx] = one tile), a contiguous CUDA tensor of the solver's scalar type, node
    (ix, iy) of a tile at (x0 + ix cell, y0 + iy cell); tile: int32 CUDA tensor, one entry per state (or per sample point), or None = tile 0.  Holds the
    C struct and keeps both tensors alive; the library checks the values at every call (WbcError)."""

    def __init__(self, z, x0, y0, cell, tile=None):
        if z.dim() == 2:
            z = z.unsqueeze(0)
        assert z.dim() == 3 and z.is_cuda and z.is_contiguous(), "z: a contiguous CUDA tensor [n_tiles, ny, nx]"
        if tile is not None:
            assert tile.is_cuda and tile.is_contiguous() and str(tile.dtype) == "torch.int32", "tile: a contiguous int32 CUDA tensor"
        self.z, self.tile = z, tile
        self.c = TerrainStruct(C.sizeof(TerrainStruct), z.shape[2], z.shape[1], z.shape[0], float(x0), float(y0), float(cell), z.data_ptr(),
                               tile.data_ptr() if tile is not None else None)

    def with_tile(self, tile):
        """the same grid with another per-state tile tensor"""
        return Terrain(self.z, self.c.x0, self.c.y0, self.c.cell, tile)


GAIT_CMD_WORDS = 4   # include/wbc_hip.h: WBC_GAIT_CMD_WORDS -- cmd [GAIT_CMD_WORDS, N]: vx, vy (heading frame), wz, z_g


class GaitParams(C.Structure):
    """wbc_gait_params: the schedule and foothold rule of the gait scheduler (include/wbc_hip.h)"""
    _fields_ = [("struct_size", C.c_size_t), ("period", C.c_double), ("duty", C.c_double * 4), ("offset", C.c_double * 4), ("clearance", C.c_double),
                ("k_v", C.c_double), ("late", C.c_double), ("retarget", C.c_int), ("base_xy", (C.c_double * 2) * 4)]

    @staticmethod
    def default(model=None):
        """wbc_gait_params_default: base_xy from the model's hip origins (zeros without a model)"""
        p = GaitParams()
        _gait_lib().wbc_gait_params_default(model._h if model is not None else None, C.byref(p))
        return p

    @staticmethod
    def from_dict(d, model=None):
        """keys period, duty, offset (scalars broadcast over the feet), clearance, k_v, late, retarget, base_xy [4, 2]; missing keys keep the defaults"""
        p = GaitParams.default(model)
        for k, val in d.items():
            if k in ("duty", "offset"):
                a = np.broadcast_to(np.asarray(val, dtype=np.float64), (4,))
                for i in range(4):
                    getattr(p, k)[i] = float(a[i])
            elif k == "base_xy":
                a = np.broadcast_to(np.asarray(val, dtype=np.float64), (4, 2))
                for i in range(4):
                    p.base_xy[i][0], p.base_xy[i][1] = float(a[i, 0]), float(a[i, 1])
            elif k == "retarget":
                p.retarget = int(val)
            elif k in ("period", "clearance", "k_v", "late"):
                setattr(p, k, float(val))
            else:
                raise KeyError("GaitParams has no field %r" % k)
        return p

    def as_dict(self):
        return dict(period=self.period, duty=tuple(self.duty), offset=tuple(self.offset), clearance=self.clearance, k_v=self.k_v, late=self.late,
                    retarget=self.retarget, base_xy=tuple((r[0], r[1]) for r in self.base_xy))


class TorqueLimits(C.Structure):
    """wbc_torque_limits: tau_max > 0 per joint in the caller's joint order, inf = no limit."""
    _fields_ = [("struct_size", C.c_size_t), ("tau_max", C.c_double * WBC_MAXV)]


class RolloutScore(C.Structure):
    """wbc_rollout_score: the buffers of one scored call"""
    _fields_ = [("struct_size", C.c_size_t), ("goal", C.c_void_p), ("cost", C.c_void_p), ("fail_ticks", C.c_void_p), ("accumulate", C.c_int)]


def select_rollouts(cost, group, lam=0.0, want_weights=False, stream=None):
    """Per group of `group` consecutive candidates of cost [N] (a contiguous CUDA tensor, float64 or float32; N = n_groups * group):
    dict(best [n_groups] int32 = index within the group of the smallest cost (-1: none finite), best_cost [n_groups][, weights [N] = the MPPI
    weights exp(-(c - c_min) / lam), normalised per group; lam <= 0: one-hot on best]).  wbc_rollout_select: one launch on the current stream."""
    import torch
    assert cost.is_cuda and cost.is_contiguous() and cost.dtype in (torch.float64, torch.float32)
    N = cost.numel()
    group = int(group)
    if group < 1 or N % group:
        raise ValueError("cost holds %d candidates: not a multiple of group = %d" % (N, group))
    ng = N // group
    out = dict(best=torch.empty(ng, dtype=torch.int32, device=cost.device), best_cost=torch.empty(ng, dtype=cost.dtype, device=cost.device))
    if want_weights:
        out["weights"] = torch.empty(N, dtype=cost.dtype, device=cost.device)
    st = stream if stream is not None else torch.cuda.current_stream(cost.device).cuda_stream
    with torch.cuda.device(cost.device):
        _check(lib().wbc_rollout_select(F64 if cost.dtype == torch.float64 else F32, ng, group, C.c_void_p(cost.data_ptr()), C.c_double(lam),
                                        C.c_void_p(out["best"].data_ptr()), C.c_void_p(out["best_cost"].data_ptr()),
                                        C.c_void_p(out["weights"].data_ptr()) if want_weights else None, C.c_void_p(st)), "wbc_rollout_select")
    return out


def payload_rows(m, c, I):
    """The [PAYLOAD_WORDS, N] payload array of the *_plant_batch calls (numpy float64) from per-state values: m [N] (kg), c [N, 3]
    (payload CoM in the BASE frame, m), I [N, 3, 3] (inertia about c, base axes, kg m^2) or [N, 6] as xx yy zz xy xz yz.
    Scalars and single rows broadcast over N.  A state with m = 0 and I = 0 carries no payload."""
    m = np.atleast_1d(np.asarray(m, dtype=np.float64))
    c = np.atleast_2d(np.asarray(c, dtype=np.float64))
    I = np.asarray(I, dtype=np.float64)
    if I.shape[-2:] == (3, 3):
        I = np.stack([I[..., 0, 0], I[..., 1, 1], I[..., 2, 2], I[..., 0, 1], I[..., 0, 2], I[..., 1, 2]], axis=-1)
    I = np.atleast_2d(I)
    N = max(len(m), len(c), len(I))
    out = np.empty((PAYLOAD_WORDS, N))
    out[0] = np.broadcast_to(m, (N,))
    out[1:4] = np.broadcast_to(c, (N, 3)).T
    out[4:10] = np.broadcast_to(I, (N, 6)).T
    return out


class Model:
    def __init__(self, handle):
        self._h = C.c_void_p(handle)
        nb, nq, nv, nj, nf = (C.c_int() for _ in range(5))
        _check(lib().wbc_model_dims(self._h, C.byref(nb), C.byref(nq), C.byref(nv), C.byref(nj), C.byref(nf)), "wbc_model_dims")
        self.nb, self.nq, self.nv, self.nj, self.nf = nb.value, nq.value, nv.value, nj.value, nf.value

    @staticmethod
    def from_urdf(path, foot_links=None):
        h = C.c_void_p()
        if foot_links:
            arr = (C.c_char_p * len(foot_links))(*[s.encode() for s in foot_links])
            rc = lib().wbc_model_load_urdf(path.encode(), arr, len(foot_links), C.byref(h))
        else:
            rc = lib().wbc_model_load_urdf(path.encode(), None, 0, C.byref(h))
        _check(rc, "wbc_model_load_urdf")
        return Model(h.value)

    @staticmethod
    def from_flat(flat):
        h = C.c_void_p()
        c = lambda k, t: np.ascontiguousarray(flat[k], dtype=t)
        a = [c("parent", np.int32), c("Rt", np.float64), c("rt", np.float64), c("axis", np.float64),
             c("mass", np.float64), c("com", np.float64), c("Ic", np.float64), c("foot_body", np.int32),
             c("foot_off", np.float64), c("gravity", np.float64)]
        p = [x.ctypes.data_as(C.c_void_p) for x in a]
        rc = lib().wbc_model_from_flat(int(flat["nb"]), p[0], p[1], p[2], p[3], p[4], p[5], p[6], len(a[7]), p[7], p[8],
                                       p[9], C.byref(h))
        _check(rc, "wbc_model_from_flat")
        return Model(h.value)

    def flat(self):
        nb, nf = self.nb, self.nf
        o = dict(nb=nb, parent=np.zeros(nb, np.int32), Rt=np.zeros((nb, 9)), rt=np.zeros((nb, 3)), axis=np.zeros((nb, 3)),
                 mass=np.zeros(nb), com=np.zeros((nb, 3)), Ic=np.zeros((nb, 6)), foot_body=np.zeros(nf, np.int32),
                 foot_off=np.zeros((nf, 3)), gravity=np.zeros(3))
        p = lambda k: o[k].ctypes.data_as(C.c_void_p)
        _check(lib().wbc_model_get_flat(self._h, p("parent"), p("Rt"), p("rt"), p("axis"), p("mass"), p("com"), p("Ic"),
                                        p("foot_body"), p("foot_off"), p("gravity")), "wbc_model_get_flat")
        o["joint_names"] = [(lib().wbc_model_joint_name(self._h, j) or b"").decode() for j in range(self.nj)]
        o["foot_links"] = [(lib().wbc_model_foot_link(self._h, k) or b"").decode() for k in range(self.nf)]
        return o

    @property
    def total_mass(self):
        return lib().wbc_model_total_mass(self._h)

    def effort_limits(self):
        """<limit effort> of each actuated joint (float64 [nj], caller's joint order); inf where the URDF gives none and for from_flat models."""
        lim = np.zeros(self.nj)
        _check(_limit_lib().wbc_model_effort_limits(self._h, lim.ctypes.data_as(C.c_void_p)), "wbc_model_effort_limits")
        return lim

    def gait_params_default(self):
        """GaitParams.default(self): the default schedule with this model's hip origins as nominal footholds"""
        return GaitParams.default(self)

    def __del__(self):
        try:
            lib().wbc_model_free(self._h)
        except Exception:
            pass


class Solver:
    """Device-side context: one per GPU (and per stream)."""

    def __init__(self, model, params=None, dtype="f64", device=0, max_batch=4096, options=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible to torch: the WBC hot path has no CPU fallback")
        self.torch = torch
        self.model = model
        self.dtype = dtype
        self.tdtype = torch.float64 if dtype == "f64" else torch.float32
        self.device = torch.device("cuda", device)
        self.max_batch = int(max_batch)
        self.params = params if params is not None else Params.default(dtype)
        h = C.c_void_p()
        self.options = SolverOptions.make(options)
        _check(lib().wbc_solver_create_ex(model._h, C.byref(self.params), F64 if dtype == "f64" else F32, device,
                                          self.max_batch, C.byref(self.options), C.byref(h)), "wbc_solver_create_ex")
        self._h = h

    def set_params(self, params):
        _check(lib().wbc_solver_set_params(self._h, C.byref(params)), "wbc_solver_set_params")
        self.params = params

    def __del__(self):
        try:
            lib().wbc_solver_destroy(self._h)
        except Exception:
            pass

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    def _ptr(self, t, rows, N, dtype=None):
        if t is None:
            return None
        assert t.is_cuda and t.is_contiguous(), "batch tensors must be contiguous CUDA tensors"
        assert t.dtype == (dtype or self.tdtype), (t.dtype, dtype or self.tdtype)
        assert t.numel() == rows * N, (tuple(t.shape), rows, N)
        return C.c_void_p(t.data_ptr())

    def _batch(self, N, q, v, w_des, vdot_des, normals, mu, mask, out, obs_integ, obs_r, tau_prev=None, f_prev=None):
        """The C argument structs of a tick or a rollout: (_BatchIn, _BatchOut, _ObsState)."""
        torch = self.torch
        m = self.model
        rows = dict(tau=m.nj, f=3 * m.nf, M=m.nv * (m.nv + 1) // 2, h=m.nv, Jc=3 * m.nf * m.nv, pf=3 * m.nf)
        bi = _BatchIn(self._ptr(q, m.nq, N), self._ptr(v, m.nv, N), self._ptr(w_des, 6, N), self._ptr(vdot_des, m.nv, N),
                      self._ptr(normals, 3 * m.nf, N), self._ptr(mu, m.nf, N), self._ptr(mask, 1, N, torch.int32),
                      self._ptr(tau_prev, m.nj, N), self._ptr(f_prev, 3 * m.nf, N))
        g = lambda k: self._ptr(out.get(k), rows[k], N)
        bo = _BatchOut(g("tau"), g("f"), self._ptr(out["status"], 1, N, torch.int32),
                       self._ptr(out.get("iters"), 1, N, torch.int32), g("M"), g("h"), g("Jc"), g("pf"))
        return bi, bo, _ObsState(self._ptr(obs_integ, m.nv, N), self._ptr(obs_r, m.nv, N))

    @staticmethod
    def _traj(t, words):
        """A rollout's trajectory buffer (tau_traj, com_traj: horizon * rows * N words, or None) as the C call takes it."""
        if t is None:
            return None
        assert t.is_cuda and t.is_contiguous() and t.numel() == words
        return C.c_void_p(t.data_ptr())

    def empty(self, rows, N, dtype=None):
        return self.torch.empty((rows, N), dtype=dtype or self.tdtype, device=self.device)

    def dynamics(self, q, v, want=("M", "h", "Jc", "pf"), out=None):
        """Dynamics sweep: returns dict of [ncomp, N] tensors for the names in `want`."""
        m = self.model
        N = q.shape[1]
        rows = dict(M=m.nv * (m.nv + 1) // 2, h=m.nv, Jc=3 * m.nf * m.nv, pf=3 * m.nf, p=m.nv, beta=m.nv)
        out = dict(out or {})
        for k in want:
            if k not in out:
                out[k] = self.empty(rows[k], N)
        g = lambda k: self._ptr(out.get(k), rows[k], N)
        _check(lib().wbc_dynamics_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N), g("M"), g("h"), g("Jc"),
                                        g("pf"), g("p"), g("beta"), self._stream()), "wbc_dynamics_batch")
        return out

    def step(self, q, v, w_des, vdot_des, normals, mu, mask, tau_prev=None, f_prev=None, obs_integ=None, obs_r=None,
             out=None, want_mats=False, _prepared=False, active_in=None, warm=False):
        """One control tick.  Observer state tensors are updated in place.  Returns dict(tau, f, status, iters[, M, h, Jc, pf]).
        warm=True (or active_in given): wbc_step_batch_warm -- the QPs start from the int32 [N] tensor active_in (None: cold) and the
        final active sets are returned as out["active"] (pass out={"active": active_in} to update a set in place)."""
        torch = self.torch
        m = self.model
        N = q.shape[1]
        out = dict(out or {})
        rows = dict(tau=m.nj, f=3 * m.nf, M=m.nv * (m.nv + 1) // 2, h=m.nv, Jc=3 * m.nf * m.nv, pf=3 * m.nf)
        for k in ("tau", "f"):
            if k not in out:
                out[k] = self.empty(rows[k], N)
        for k in ("status", "iters"):
            if k not in out:
                out[k] = torch.empty(N, dtype=torch.int32, device=self.device)
        if want_mats:
            if "M" not in out or "Jc" not in out:
                # keep_structural identifies "the same buffers" by address, and the caching allocator hands a just-freed address out
                # again: buffers allocated HERE are always written in full (only a caller that passes out= keeps the constants)
                lib().wbc_solver_invalidate_structural(self._h)
            for k in ("M", "h", "Jc", "pf"):
                if k not in out:
                    out[k] = self.empty(rows[k], N)
        bi, bo, ob = self._batch(N, q, v, w_des, vdot_des, normals, mu, mask, out, obs_integ, obs_r, tau_prev, f_prev)
        warm = warm or active_in is not None
        if warm and "active" not in out:
            out["active"] = torch.zeros(N, dtype=torch.int32, device=self.device)
        if _prepared:   # prepare_step(): hand back the validated argument structs instead of launching
            return out, (N, bi, bo, ob, (q, v, w_des, vdot_des, normals, mu, mask, tau_prev, f_prev, obs_integ, obs_r, active_in), warm)
        if warm:
            _check(lib().wbc_step_batch_warm(self._h, N, C.byref(bi), C.byref(bo), C.byref(ob), self._ptr(active_in, 1, N, torch.int32),
                                             self._ptr(out["active"], 1, N, torch.int32), self._stream()), "wbc_step_batch_warm")
        else:
            _check(lib().wbc_step_batch(self._h, N, C.byref(bi), C.byref(bo), C.byref(ob), self._stream()), "wbc_step_batch")
        return out

    def set_torque_limits(self, tau_max=None):
        """The limits the torque-limit post-pass enforces: a scalar or [nj] array (> 0, inf = none); None = the model's effort limits.
        Not inside a stream capture (a captured graph keeps the limits it was captured with)."""
        if tau_max is None:
            _check(_limit_lib().wbc_solver_set_torque_limits(self._h, None), "wbc_solver_set_torque_limits")
            return
        t = TorqueLimits()
        t.struct_size = C.sizeof(TorqueLimits)
        lim = np.broadcast_to(np.asarray(tau_max, dtype=np.float64), (self.model.nj,))
        for j in range(WBC_MAXV):
            t.tau_max[j] = float(lim[j]) if j < self.model.nj else float("inf")
        _check(_limit_lib().wbc_solver_set_torque_limits(self._h, C.byref(t)), "wbc_solver_set_torque_limits")

    def limit_torques(self, w_des, normals, mu, mask, out, obs_r=None, limited=None):
        """wbc_limit_torques_batch: the post-pass alone, behind any tick of the same batch on the current stream.  out = that tick's dict (tau, f,
        status[, iters] are rewritten in place; M, h, Jc required), obs_r = the observer state the tick left (observer on).  Returns out with
        out["limited"] (int32 [N]: 0 within limits, 1 re-solved, 2 clamped)."""
        torch = self.torch
        m = self.model
        N = out["tau"].shape[1]
        if limited is None:
            limited = out.get("limited")
        if limited is None:
            limited = torch.empty(N, dtype=torch.int32, device=self.device)
        out["limited"] = limited
        bi, bo, ob = self._batch(N, None, None, w_des, None, normals, mu, mask, out, None, obs_r)
        _check(_limit_lib().wbc_limit_torques_batch(self._h, N, C.byref(bi), C.byref(bo), C.byref(ob), self._ptr(limited, 1, N, torch.int32),
                                             self._stream()), "wbc_limit_torques_batch")
        return out

    def step_limited(self, q, v, w_des, vdot_des, normals, mu, mask, tau_prev=None, f_prev=None, obs_integ=None, obs_r=None, out=None):
        """wbc_step_limited_batch: step(want_mats=True) followed by the torque-limit post-pass.  Returns step()'s dict plus out["limited"]."""
        torch = self.torch
        out, (N, bi, bo, ob, keep, _) = self.step(q, v, w_des, vdot_des, normals, mu, mask, tau_prev, f_prev, obs_integ, obs_r, out=out,
                                                  want_mats=True, _prepared=True)
        if "limited" not in out:
            out["limited"] = torch.empty(N, dtype=torch.int32, device=self.device)
        _check(_limit_lib().wbc_step_limited_batch(self._h, N, C.byref(bi), C.byref(bo), C.byref(ob), self._ptr(out["limited"], 1, N, torch.int32),
                                            self._stream()), "wbc_step_limited_batch")
        return out

    def limited_count(self):
        """How many states the last post-pass re-solved (synchronises the device)."""
        n = C.c_int(0)
        _check(_limit_lib().wbc_solver_limited_count(self._h, C.byref(n)), "wbc_solver_limited_count")
        return n.value

    def prepare_step(self, *args, **kw):
        """Same arguments as step(); validates them and builds the C argument structs ONCE.  Returns (tick, out):
        tick() launches one control tick on the current stream with nothing but the C call in it (a control loop or a
        benchmark that reuses its buffers: ~3 us of host time per tick instead of ~15), out is step()'s dict."""
        out, (N, bi, bo, ob, keep, warm) = self.step(*args, _prepared=True, **kw)
        h, rbi, rbo, rob, stream_of = self._h, C.byref(bi), C.byref(bo), C.byref(ob), self._stream
        if warm:   # (a prepared warm tick carries its sets from call to call in out["active"]; the first call starts from active_in, or cold)
            import torch
            fnw = lib().wbc_step_batch_warm
            a_in = keep[-1]
            p_out = self._ptr(out["active"], 1, N, torch.int32)
            state = {"first": self._ptr(a_in, 1, N, torch.int32) if a_in is not None else None, "n": 0}

            def tick(_keep=(keep, bi, bo, ob, out)):
                rc = fnw(h, N, rbi, rbo, rob, state["first"] if state["n"] == 0 else p_out, p_out, stream_of())
                state["n"] += 1
                if rc:
                    _check(rc, "wbc_step_batch_warm")
            return tick, out
        fn = lib().wbc_step_batch

        def tick(_keep=(keep, bi, bo, ob, out)):   # the tensors and structs stay alive as long as the closure does
            rc = fn(h, N, rbi, rbo, rob, stream_of())
            if rc:
                _check(rc, "wbc_step_batch")
        return tick, out

    def plan_tick(self, N, want_mats=True, want_pf=True, warm=False):
        """wbc_solver_plan_tick: which kernels a tick of N states runs on THIS solver (dict of wbc_tick_plan's fields)."""
        pl = TickPlan()
        pl.struct_size = C.sizeof(TickPlan)
        _check(lib().wbc_solver_plan_tick(self._h, int(N), int(want_mats), int(want_pf), int(warm), C.byref(pl)), "wbc_solver_plan_tick")
        return pl.as_dict()

    def invalidate_structural(self):
        """keep_structural: the next tick writes M / Jc in full again (their buffers were freed, reallocated or overwritten)."""
        _check(lib().wbc_solver_invalidate_structural(self._h), "wbc_solver_invalidate_structural")

    def _plant(self, tau_ext, payload, N):
        """wbc_plant for the *_plant_batch calls (payload [PAYLOAD_WORDS, N]: a device tensor of the solver's dtype, or the numpy array of
        payload_rows, copied to the device here)"""
        if isinstance(payload, np.ndarray):
            payload = self.torch.from_numpy(np.ascontiguousarray(payload)).to(device=self.device, dtype=self.tdtype)
        pl = Plant()
        pl.struct_size = C.sizeof(Plant)
        pl.tau_ext = self._ptr(tau_ext, self.model.nv, N)
        pl.payload = self._ptr(payload, PAYLOAD_WORDS, N)
        pl._keep = payload   # (the caching allocator reuses its memory only behind this call's work on the stream)
        return pl

    def integrate(self, q, v, M, h, Jc, tau, f, tau_ext=None, payload=None):
        """Forward dynamics with the planned GRFs + semi-implicit Euler; q, v advance IN PLACE (one dt).
        payload [PAYLOAD_WORDS, N] (optional, see payload_rows): the PLANT carries it on its trunk (wbc_integrate_plant_batch); M, h, Jc
        stay the nominal model's."""
        m = self.model
        N = q.shape[1]
        if payload is not None:
            pl = self._plant(tau_ext, payload, N)
            _check(lib().wbc_integrate_plant_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N),
                                                   self._ptr(M, m.nv * (m.nv + 1) // 2, N), self._ptr(h, m.nv, N),
                                                   self._ptr(Jc, 3 * m.nf * m.nv, N), self._ptr(tau, m.nj, N), self._ptr(f, 3 * m.nf, N),
                                                   C.byref(pl), self._stream()), "wbc_integrate_plant_batch")
            return
        _check(lib().wbc_integrate_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N),
                                         self._ptr(M, m.nv * (m.nv + 1) // 2, N), self._ptr(h, m.nv, N),
                                         self._ptr(Jc, 3 * m.nf * m.nv, N), self._ptr(tau, m.nj, N), self._ptr(f, 3 * m.nf, N), self._ptr(tau_ext, m.nv, N),
                                         self._stream()), "wbc_integrate_batch")

    def rollout(self, horizon, q, v, w_des, vdot_des, normals, mu, mask, out, obs_integ=None, obs_r=None, tau_ext=None,
                tau_traj=None, payload=None):
        """`horizon` dependent ticks; q, v advance IN PLACE; `out` must hold tau, f (previous outputs or zeros), status,
        iters, M, h, Jc (e.g. the dict a previous step(..., want_mats=True) returned).
        payload [PAYLOAD_WORDS, N] (optional, see payload_rows): the PLANT carries it on its trunk, the controller keeps the nominal model
        (wbc_rollout_plant_batch)."""
        m = self.model
        N = q.shape[1]
        bi, bo, ob = self._batch(N, q, v, w_des, vdot_des, normals, mu, mask, out, obs_integ, obs_r)
        tt = self._traj(tau_traj, horizon * m.nj * N)
        if payload is not None:
            pl = self._plant(tau_ext, payload, N)
            _check(lib().wbc_rollout_plant_batch(self._h, N, int(horizon), C.byref(bi), C.byref(bo), C.byref(ob), C.byref(pl), tt,
                                                 self._stream()), "wbc_rollout_plant_batch")
            return out
        _check(lib().wbc_rollout_batch(self._h, N, int(horizon), C.byref(bi), C.byref(bo), C.byref(ob),
                                       self._ptr(tau_ext, m.nv, N), tt, self._stream()), "wbc_rollout_batch")
        return out

    def set_score_params(self, p):
        """p: ScoreParams or dict (see ScoreParams.from_dict): the weights of every later scored call of this solver."""
        if isinstance(p, dict):
            p = ScoreParams.from_dict(p)
        _check(lib().wbc_solver_set_score_params(self._h, C.byref(p)), "wbc_solver_set_score_params")

    def _score(self, goal, cost, fail_ticks, accumulate, N):
        sc = RolloutScore()
        sc.struct_size = C.sizeof(RolloutScore)
        sc.goal = self._ptr(goal, GOAL_WORDS, N)
        sc.cost = self._ptr(cost, 1, N)
        sc.fail_ticks = self._ptr(fail_ticks, 1, N, self.torch.int32)
        sc.accumulate = 1 if accumulate else 0
        return sc

    def rollout_scored(self, horizon, q, v, normals, mu, mask, out, w_des, vdot_des, goal, cost=None, fail_ticks=None, accumulate=False,
                       plan=None, payload=None, obs_integ=None, obs_r=None, tau_ext=None, tau_traj=None, com_traj=None):
        """rollout() (plan None: w_des / vdot_des are the constant references) or rollout_tracking() (plan given: they are scratch), with or without a
        payload on the plant, AND the running cost of the state path against goal [GOAL_WORDS, N] under the solver's ScoreParams, accumulated on
        chip (wbc_rollout_scored_batch).  cost [N] (allocated when None) and fail_ticks [N] int32 (optional) start at zero, or -- accumulate --
        at what they hold.  Returns cost."""
        torch = self.torch
        m = self.model
        N = q.shape[1]
        if cost is None:
            assert not accumulate, "accumulate needs the cost of the earlier call"
            cost = torch.empty(N, dtype=self.tdtype, device=q.device)
        bi, bo, ob = self._batch(N, q, v, w_des, vdot_des, normals, mu, mask, out, obs_integ, obs_r)
        tt, ct = self._traj(tau_traj, horizon * m.nj * N), self._traj(com_traj, horizon * 6 * N)
        pl = self._plant(tau_ext, payload, N) if (payload is not None or tau_ext is not None) else None
        sc = self._score(goal, cost, fail_ticks, accumulate, N)
        _check(lib().wbc_rollout_scored_batch(self._h, N, int(horizon), C.byref(bi), C.byref(bo), C.byref(ob), C.byref(pl) if pl is not None else None,
                                              self._ptr(plan, PLAN_WORDS, N), tt, ct, C.byref(sc), self._stream()), "wbc_rollout_scored_batch")
        return cost

    def score(self, q, v, tau, f, status, goal, cost, fail_ticks=None, accumulate=True, is_last=False):
        """One tick's cost l_k of the state (q, v) the tick ended in and the tau, f, status it produced, for callers that drive their own loop
        (wbc_score_batch): added to cost [N] (accumulate, the default) or written to it (the first tick of a sum).  Returns cost."""
        m = self.model
        N = q.shape[1]
        sc = self._score(goal, cost, fail_ticks, accumulate, N)
        _check(lib().wbc_score_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N), self._ptr(tau, m.nj, N), self._ptr(f, 3 * m.nf, N),
                                     self._ptr(status, 1, N, self.torch.int32), C.byref(sc), 1 if is_last else 0, self._stream()), "wbc_score_batch")
        return cost

    def set_ref_params(self, g):
        """g: RefParams or dict (see RefParams.from_dict)."""
        if isinstance(g, dict):
            g = RefParams.from_dict(g)
        _check(lib().wbc_solver_set_ref_params(self._h, C.byref(g)), "wbc_solver_set_ref_params")

    def reference(self, q, v, plan, t=0.0, out=None, want_com=False):
        """CoM reference generator: plan [12, N] -> dict(w_des [6, N], vdot_des [nv, N][, com [6, N]])."""
        torch = self.torch
        m = self.model
        N = q.shape[1]
        out = {} if out is None else out
        for k, rows in (("w_des", 6), ("vdot_des", m.nv)) + ((("com", 6),) if want_com else ()):
            if k not in out:
                out[k] = torch.empty((rows, N), dtype=self.tdtype, device=q.device)
        _check(lib().wbc_reference_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N),
                                         self._ptr(plan, PLAN_WORDS, N), C.c_double(t), self._ptr(out["w_des"], 6, N),
                                         self._ptr(out["vdot_des"], m.nv, N),
                                         self._ptr(out["com"], 6, N) if want_com else None, self._stream()),
               "wbc_reference_batch")
        return out

    def set_swing_params(self, p):
        """p: SwingParams or dict (see SwingParams.from_dict): the gains of every later swing-reference call of this solver."""
        if isinstance(p, dict):
            p = SwingParams.from_dict(p)
        _check(_swing_lib().wbc_solver_set_swing_params(self._h, C.byref(p)), "wbc_solver_set_swing_params")

    def swing_reference(self, q, v, mask, swing, t=0.0, vdot_des=None, want_foot=False):
        """Swing-foot references (wbc_swing_reference_batch): for every foot whose mask bit is clear, the leg's joint rows of vdot_des [nv, N] are
        REPLACED IN PLACE by the joint accelerations that track the foot trajectory of swing [SWING_WORDS, N] at time t; the base rows are read as
        they stand, everything else is left alone.  Returns dict(vdot_des[, foot [FOOT_WORDS, N]])."""
        m = self.model
        N = q.shape[1]
        assert vdot_des is not None, "vdot_des is in/out: pass the tensor reference() filled"
        out = dict(vdot_des=vdot_des)
        if want_foot:
            out["foot"] = self.torch.empty((FOOT_WORDS, N), dtype=self.tdtype, device=q.device)
        _check(_swing_lib().wbc_swing_reference_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N), self._ptr(mask, 1, N, self.torch.int32),
                                                      self._ptr(swing, SWING_WORDS, N), C.c_double(t), self._ptr(vdot_des, m.nv, N),
                                                      self._ptr(out.get("foot"), FOOT_WORDS, N), self._stream()), "wbc_swing_reference_batch")
        return out

    def reference_swing(self, q, v, plan, mask, swing, t=0.0, out=None, want_com=False, want_foot=False):
        """reference() followed by swing_reference(), as one launch (wbc_reference_swing_batch):
        dict(w_des [6, N], vdot_des [nv, N][, com [6, N]][, foot [FOOT_WORDS, N]])."""
        torch = self.torch
        m = self.model
        N = q.shape[1]
        out = {} if out is None else out
        for k, rows in (("w_des", 6), ("vdot_des", m.nv)) + ((("com", 6),) if want_com else ()) + ((("foot", FOOT_WORDS),) if want_foot else ()):
            if k not in out:
                out[k] = torch.empty((rows, N), dtype=self.tdtype, device=q.device)
        _check(_swing_lib().wbc_reference_swing_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N), self._ptr(plan, PLAN_WORDS, N),
                                                      self._ptr(mask, 1, N, torch.int32), self._ptr(swing, SWING_WORDS, N), C.c_double(t),
                                                      self._ptr(out["w_des"], 6, N), self._ptr(out["vdot_des"], m.nv, N),
                                                      self._ptr(out["com"], 6, N) if want_com else None,
                                                      self._ptr(out["foot"], FOOT_WORDS, N) if want_foot else None, self._stream()),
               "wbc_reference_swing_batch")
        return out

    def set_trunk_params(self, p):
        """p: TrunkParams or dict (see TrunkParams.from_dict): the parameters of every later reference_cmd call of this solver."""
        if isinstance(p, dict):
            p = TrunkParams.from_dict(p)
        _check(_trunk_lib().wbc_solver_set_trunk_params(self._h, C.byref(p)), "wbc_solver_set_trunk_params")

    def _cmd_out(self, N, out, want_com, want_ref, want_foot):
        m = self.model
        out = {} if out is None else out
        for k, rows in ((("w_des", 6), ("vdot_des", m.nv)) + ((("com", 6),) if want_com else ()) + ((("ref", TRUNKREF_WORDS),) if want_ref else ())
                        + ((("foot", FOOT_WORDS),) if want_foot else ())):
            if k not in out:
                out[k] = self.empty(rows, N)
        return out

    def reference_cmd(self, q, v, cmd, normals, height, trunk, reset=None, out=None, want_com=False, want_ref=False):
        """Trunk reference from the velocity command (wbc_reference_cmd_batch): cmd [4, N] (rows 0-2 are read), normals [12, N] and height [4, N] the
        plane under every foot, trunk [TRUNK_WORDS, N] advanced IN PLACE, reset (int32 [N] or None): non-zero starts a robot's trunk words from its
        state.  Returns dict(w_des [6, N], vdot_des [nv, N], trunk[, com [6, N]][, ref [TRUNKREF_WORDS, N]])."""
        m = self.model
        N = q.shape[1]
        out = self._cmd_out(N, out, want_com, want_ref, False)
        _check(_trunk_lib().wbc_reference_cmd_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N), self._ptr(cmd, GAIT_CMD_WORDS, N),
                                                    self._ptr(normals, 3 * m.nf, N), self._ptr(height, m.nf, N),
                                                    self._ptr(reset, 1, N, self.torch.int32), self._ptr(trunk, TRUNK_WORDS, N),
                                                    self._ptr(out["w_des"], 6, N), self._ptr(out["vdot_des"], m.nv, N),
                                                    self._ptr(out["com"], 6, N) if want_com else None,
                                                    self._ptr(out["ref"], TRUNKREF_WORDS, N) if want_ref else None, self._stream()),
               "wbc_reference_cmd_batch")
        out["trunk"] = trunk
        return out

    def reference_cmd_swing(self, q, v, cmd, normals, height, trunk, mask, swing, reset=None, out=None, want_com=False, want_ref=False,
                            want_foot=False):
        """reference_cmd() followed by swing_reference() at t = 0, as one launch (wbc_reference_cmd_swing_batch):
        dict(w_des, vdot_des, trunk[, com][, ref][, foot [FOOT_WORDS, N]])."""
        m = self.model
        N = q.shape[1]
        i32 = self.torch.int32
        out = self._cmd_out(N, out, want_com, want_ref, want_foot)
        _check(_trunk_lib().wbc_reference_cmd_swing_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N), self._ptr(cmd, GAIT_CMD_WORDS, N),
                                                          self._ptr(normals, 3 * m.nf, N), self._ptr(height, m.nf, N), self._ptr(reset, 1, N, i32),
                                                          self._ptr(trunk, TRUNK_WORDS, N), self._ptr(mask, 1, N, i32),
                                                          self._ptr(swing, SWING_WORDS, N), self._ptr(out["w_des"], 6, N),
                                                          self._ptr(out["vdot_des"], m.nv, N), self._ptr(out["com"], 6, N) if want_com else None,
                                                          self._ptr(out["ref"], TRUNKREF_WORDS, N) if want_ref else None,
                                                          self._ptr(out["foot"], FOOT_WORDS, N) if want_foot else None, self._stream()),
               "wbc_reference_cmd_swing_batch")
        out["trunk"] = trunk
        return out

    def compute_reference_cmd(self, q, v, cmd, normals, height, trunk, reset=0):
        """Single-robot host-array form of reference_cmd (numpy float64, fp64 solvers): returns (trunk[6], w_des[6], vdot_des[18], com[6], ref[10]);
        the inputs are not modified."""
        arr = lambda a, n: np.ascontiguousarray(np.asarray(a, np.float64).reshape(n))
        q, v, cmd, normals, height, trunk = arr(q, 19), arr(v, 18), arr(cmd, 4), arr(normals, 12), arr(height, 4), arr(trunk, 6).copy()
        w, vd, com, ref = np.empty(6), np.empty(18), np.empty(6), np.empty(TRUNKREF_WORDS)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _check(_trunk_lib().wbc_compute_reference_cmd(self._h, p(q), p(v), p(cmd), p(normals), p(height), int(reset), p(trunk), p(w), p(vd), p(com),
                                                      p(ref)), "wbc_compute_reference_cmd")
        return trunk, w, vd, com, ref

    def compute_swing_reference(self, q, v, mask, swing, vdot_des, t=0.0):
        """Single-robot host-array form of swing_reference (numpy float64, fp64 solvers): returns (vdot_des[nv] with the swing legs' rows replaced,
        foot[FOOT_WORDS]); the argument vdot_des is not modified."""
        d = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        q, v, swing = d(q), d(v), d(swing)
        vd, foot = np.array(vdot_des, dtype=np.float64), np.zeros(FOOT_WORDS)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _check(_swing_lib().wbc_compute_swing_reference(self._h, p(q), p(v), int(mask), p(swing), C.c_double(t), p(vd), p(foot)),
               "wbc_compute_swing_reference")
        return vd, foot

    def set_gait_params(self, p):
        """p: GaitParams or dict (see GaitParams.from_dict; base_xy defaults to this solver's model): the schedule of every later gait call."""
        if isinstance(p, dict):
            p = GaitParams.from_dict(p, self.model)
        _check(_gait_lib().wbc_solver_set_gait_params(self._h, C.byref(p)), "wbc_solver_set_gait_params")

    def gait(self, q, v, cmd, phase, mask, swing, contact=None, events=None):
        """Gait scheduler (wbc_gait_batch): phase [N], mask [N] (int32) and swing [SWING_WORDS, N] advance IN PLACE by one control period from the state
        q, v and the command cmd [GAIT_CMD_WORDS, N]; contact / events: optional int32 [N].  The swing call behind it takes t = 0."""
        m = self.model
        N = q.shape[1]
        i32 = self.torch.int32
        _check(_gait_lib().wbc_gait_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N), self._ptr(cmd, GAIT_CMD_WORDS, N),
                                          self._ptr(contact, 1, N, i32), self._ptr(phase, 1, N), self._ptr(mask, 1, N, i32),
                                          self._ptr(swing, SWING_WORDS, N), self._ptr(events, 1, N, i32), self._stream()), "wbc_gait_batch")
        return dict(phase=phase, mask=mask, swing=swing, events=events)

    def compute_gait(self, q, v, cmd, phase, mask, swing, contact=0):
        """Single-robot host-array form of gait (numpy float64, fp64 solvers): returns (phase, mask, swing[SWING_WORDS], events); the arguments are
        not modified."""
        d = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        q, v, cmd = d(q), d(v), d(cmd)
        sw, ph = np.array(swing, dtype=np.float64), C.c_double(float(phase))
        mk, ev = C.c_int(int(mask)), C.c_int(0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _check(_gait_lib().wbc_compute_gait(self._h, p(q), p(v), p(cmd), int(contact), C.byref(ph), C.byref(mk), p(sw), C.byref(ev)), "wbc_compute_gait")
        return ph.value, mk.value, sw, ev.value

    def set_ground_params(self, p):
        """p: GroundParams or dict (see GroundParams.from_dict): the contact law of every later ground call of this solver."""
        if isinstance(p, dict):
            p = GroundParams.from_dict(p)
        _check(_ground_lib().wbc_solver_set_ground_params(self._h, C.byref(p)), "wbc_solver_set_ground_params")

    def _ground_out(self, N, f_gr, contact, gap, want_contact, want_gap, device):
        torch = self.torch
        f_gr = self.empty(3 * self.model.nf, N) if f_gr is None else f_gr
        if contact is None and want_contact:
            contact = torch.empty(N, dtype=torch.int32, device=device)
        if gap is None and want_gap:
            gap = self.empty(self.model.nf, N)
        return f_gr, contact, gap

    def _terrain_ptrs(self, N, normals, height, mu):
        m = self.model
        return self._ptr(normals, 3 * m.nf, N), self._ptr(height, m.nf, N), self._ptr(mu, m.nf, N)

    def _ground_out_ptrs(self, N, f_gr, contact, gap):
        m = self.model
        return self._ptr(f_gr, 3 * m.nf, N), self._ptr(contact, 1, N, self.torch.int32), self._ptr(gap, m.nf, N)

    def ground_force(self, q, v, Jc, normals, height, mu, f_gr=None, contact=None, gap=None, want_contact=True, want_gap=False):
        """The contact law alone (wbc_ground_force_batch): the terrain n_k . x = height[k] under every foot pushes back with f_gr [12, N]; contact [N]
        int32 has bit k set where foot k presses harder than f_touch; gap [4, N] is the signed distance (negative = penetration).  Tensors not
        passed are allocated.  Returns dict(f_gr, contact, gap)."""
        m = self.model
        N = q.shape[1]
        f_gr, contact, gap = self._ground_out(N, f_gr, contact, gap, want_contact, want_gap, q.device)
        _check(_ground_lib().wbc_ground_force_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N), self._ptr(Jc, 3 * m.nf * m.nv, N),
                                                    *self._terrain_ptrs(N, normals, height, mu), *self._ground_out_ptrs(N, f_gr, contact, gap),
                                                    self._stream()), "wbc_ground_force_batch")
        return dict(f_gr=f_gr, contact=contact, gap=gap)

    def integrate_ground(self, q, v, M, h, Jc, tau, normals, height, mu, tau_ext=None, f_gr=None, contact=None, gap=None, want_contact=True,
                         want_gap=False):
        """ground_force() followed by integrate(f = f_gr), as one launch (wbc_integrate_ground_batch): q, v advance IN PLACE (one dt) under the
        terrain's reaction forces instead of the planned ones.  Returns dict(f_gr, contact, gap); pass contact to the next tick's gait()."""
        m = self.model
        N = q.shape[1]
        f_gr, contact, gap = self._ground_out(N, f_gr, contact, gap, want_contact, want_gap, q.device)
        _check(_ground_lib().wbc_integrate_ground_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N),
                                                        self._ptr(M, m.nv * (m.nv + 1) // 2, N), self._ptr(h, m.nv, N),
                                                        self._ptr(Jc, 3 * m.nf * m.nv, N), self._ptr(tau, m.nj, N),
                                                        *self._terrain_ptrs(N, normals, height, mu), self._ptr(tau_ext, m.nv, N),
                                                        *self._ground_out_ptrs(N, f_gr, contact, gap), self._stream()),
               "wbc_integrate_ground_batch")
        return dict(f_gr=f_gr, contact=contact, gap=gap)

    def set_stiction_params(self, p):
        """p: StictionParams or dict (see StictionParams.from_dict): the anchor spring of every later stiction call of this solver."""
        if isinstance(p, dict):
            p = StictionParams.from_dict(p)
        _check(_stick_lib().wbc_solver_set_stiction_params(self._h, C.byref(p)), "wbc_solver_set_stiction_params")

    def ground_stick_force(self, q, v, Jc, normals, height, mu, anchor, stick, f_gr=None, contact=None, gap=None, want_contact=True, want_gap=False):
        """ground_force() with the per-foot anchor spring (wbc_ground_stick_force_batch).  anchor [12, N] and stick [N] int32 are the caller's and
        advance IN PLACE: stick in = bit k set where foot k has an anchor (store 0 before the first tick), out = bit k loaded, bit 4+k slid this tick.
        Returns dict(f_gr, contact, gap)."""
        m = self.model
        N = q.shape[1]
        if anchor is None or stick is None:
            raise ValueError("anchor and stick are required in/out tensors")
        f_gr, contact, gap = self._ground_out(N, f_gr, contact, gap, want_contact, want_gap, q.device)
        _check(_stick_lib().wbc_ground_stick_force_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N), self._ptr(Jc, 3 * m.nf * m.nv, N),
                                                         *self._terrain_ptrs(N, normals, height, mu),
                                                         self._ptr(anchor, 3 * m.nf, N), self._ptr(stick, 1, N, self.torch.int32),
                                                         *self._ground_out_ptrs(N, f_gr, contact, gap), self._stream()), "wbc_ground_stick_force_batch")
        return dict(f_gr=f_gr, contact=contact, gap=gap)

    def integrate_ground_stick(self, q, v, M, h, Jc, tau, normals, height, mu, anchor, stick, tau_ext=None, f_gr=None, contact=None, gap=None,
                               want_contact=True, want_gap=False):
        """ground_stick_force() followed by integrate(f = f_gr), as one launch (wbc_integrate_ground_stick_batch): q, v, anchor and stick advance
        IN PLACE.  Returns dict(f_gr, contact, gap); pass contact to the next tick's gait()."""
        m = self.model
        N = q.shape[1]
        if anchor is None or stick is None:
            raise ValueError("anchor and stick are required in/out tensors")
        f_gr, contact, gap = self._ground_out(N, f_gr, contact, gap, want_contact, want_gap, q.device)
        _check(_stick_lib().wbc_integrate_ground_stick_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N),
                                                             self._ptr(M, m.nv * (m.nv + 1) // 2, N), self._ptr(h, m.nv, N),
                                                             self._ptr(Jc, 3 * m.nf * m.nv, N), self._ptr(tau, m.nj, N),
                                                             *self._terrain_ptrs(N, normals, height, mu), self._ptr(tau_ext, m.nv, N),
                                                             self._ptr(anchor, 3 * m.nf, N), self._ptr(stick, 1, N, self.torch.int32),
                                                             *self._ground_out_ptrs(N, f_gr, contact, gap), self._stream()),
               "wbc_integrate_ground_stick_batch")
        return dict(f_gr=f_gr, contact=contact, gap=gap)

    def set_contact_params(self, p):
        """p: ContactParams or dict (see ContactParams.from_dict): the thresholds of every later contact-estimate call of this solver."""
        if isinstance(p, dict):
            p = ContactParams.from_dict(p)
        _check(_contact_lib().wbc_solver_set_contact_params(self._h, C.byref(p)), "wbc_solver_set_contact_params")

    def _contact_in_ptrs(self, N, Jc, r, f_prev, normals, contact):
        m = self.model
        if contact is None:
            raise ValueError("contact is a required in/out tensor (int32 [N]; store 0 before the first call)")
        return (self._ptr(Jc, 3 * m.nf * m.nv, N), self._ptr(r, m.nv, N), self._ptr(f_prev, 3 * m.nf, N), self._ptr(normals, 3 * m.nf, N),
                self._ptr(contact, 1, N, self.torch.int32))

    def contact_estimate(self, Jc, r, f_prev, normals, contact, f_est=None, fn_est=None, singular=None, want_f=False, want_fn=False,
                         want_singular=False):
        """Foot forces and contact bits from the observer's residual (wbc_contact_estimate_batch): Jc = the last step's out["Jc"], r = the observer
        residual after that step, f_prev = the buffer that step was given as f_prev.  contact [N] int32 advances IN PLACE (bits 0-3: in = the
        previous estimate, out = the new one).  f_est [12, N], fn_est [4, N], singular [N] int32 are optional; want_* allocates them.  Returns
        dict(contact, f_est, fn_est, singular)."""
        m = self.model
        N = Jc.shape[1]
        if f_est is None and want_f:
            f_est = self.empty(3 * m.nf, N)
        if fn_est is None and want_fn:
            fn_est = self.empty(m.nf, N)
        if singular is None and want_singular:
            singular = self.torch.empty(N, dtype=self.torch.int32, device=Jc.device)
        _check(_contact_lib().wbc_contact_estimate_batch(self._h, N, *self._contact_in_ptrs(N, Jc, r, f_prev, normals, contact),
                                                         self._ptr(f_est, 3 * m.nf, N), self._ptr(fn_est, m.nf, N),
                                                         self._ptr(singular, 1, N, self.torch.int32), self._stream()), "wbc_contact_estimate_batch")
        return dict(contact=contact, f_est=f_est, fn_est=fn_est, singular=singular)

    def gait_estimated(self, q, v, cmd, Jc, r, f_prev, normals, contact, phase, mask, swing, events=None, f_est=None, want_f=False):
        """contact_estimate() followed by gait(contact = the word just formed), as one launch (wbc_gait_estimated_batch): contact, phase, mask and
        swing advance IN PLACE.  Returns dict(contact, phase, mask, swing, events, f_est)."""
        m = self.model
        N = q.shape[1]
        i32 = self.torch.int32
        if f_est is None and want_f:
            f_est = self.empty(3 * m.nf, N)
        _check(_contact_lib().wbc_gait_estimated_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N), self._ptr(cmd, GAIT_CMD_WORDS, N),
                                                       *self._contact_in_ptrs(N, Jc, r, f_prev, normals, contact), self._ptr(phase, 1, N),
                                                       self._ptr(mask, 1, N, i32), self._ptr(swing, SWING_WORDS, N), self._ptr(events, 1, N, i32),
                                                       self._ptr(f_est, 3 * m.nf, N), self._stream()), "wbc_gait_estimated_batch")
        return dict(contact=contact, phase=phase, mask=mask, swing=swing, events=events, f_est=f_est)

    def _terrain_arg(self, terrain, n):
        assert terrain.z.dtype == self.tdtype, (terrain.z.dtype, self.tdtype)
        assert terrain.tile is None or terrain.tile.numel() == n, (tuple(terrain.tile.shape), n)
        return C.byref(terrain.c)

    def _terrain_out(self, N, normals, height, surf, want_surf):
        m = self.model
        normals = self.empty(3 * m.nf, N) if normals is None else normals
        height = self.empty(m.nf, N) if height is None else height
        if surf is None and want_surf:
            surf = self.empty(m.nf, N)
        return normals, height, surf

    def terrain_sample(self, terrain, xy, z=None, n=None, d=None, want_z=True, want_n=True, want_d=True):
        """The sampling law at the points xy [2, M] (wbc_terrain_sample_batch): the surface height z [M], the unit normal n [3, M] of the cell's
        bilinear patch and the offset d [M] of the tangent plane n . x = d.  terrain.tile, if any, has M entries.  want_* allocates an output that was
        not passed; an output neither passed nor wanted is not computed.  Returns dict(z, n, d)."""
        M = xy.shape[1]
        if z is None and want_z:
            z = self.empty(1, M).view(M)
        if n is None and want_n:
            n = self.empty(3, M)
        if d is None and want_d:
            d = self.empty(1, M).view(M)
        _check(_terrain_lib().wbc_terrain_sample_batch(self._h, self._terrain_arg(terrain, M), M, self._ptr(xy, 2, M), self._ptr(z, 1, M),
                                                       self._ptr(n, 3, M), self._ptr(d, 1, M), self._stream()), "wbc_terrain_sample_batch")
        return dict(z=z, n=n, d=d)

    def terrain_feet(self, terrain, q, mask=None, swing=None, normals=None, height=None, surf=None, want_surf=False):
        """The terrain's planes under the four feet of every state (wbc_terrain_feet_batch): normals [12, N] and height [4, N] as the step, the contact
        estimate and the ground calls read them, surf [4, N] = the surface height under each foot.  mask (int32 [N]) and swing [SWING_WORDS, N] are
        given both or neither: p1_z of every foot whose bit is clear becomes the surface height at its plan's own p1_x, p1_y, IN PLACE.  Returns
        dict(normals, height, surf, swing)."""
        m = self.model
        N = q.shape[1]
        normals, height, surf = self._terrain_out(N, normals, height, surf, want_surf)
        _check(_terrain_lib().wbc_terrain_feet_batch(self._h, self._terrain_arg(terrain, N), N, self._ptr(q, m.nq, N),
                                                     self._ptr(mask, 1, N, self.torch.int32), self._ptr(swing, SWING_WORDS, N),
                                                     self._ptr(normals, 3 * m.nf, N), self._ptr(height, m.nf, N), self._ptr(surf, m.nf, N),
                                                     self._stream()), "wbc_terrain_feet_batch")
        return dict(normals=normals, height=height, surf=surf, swing=swing)

    def gait_terrain(self, terrain, q, v, cmd, phase, mask, swing, contact=None, events=None, normals=None, height=None, surf=None, want_surf=False):
        """gait() followed by terrain_feet(mask, swing = what it left), as one launch (wbc_gait_terrain_batch).  Returns dict(phase, mask, swing,
        events, normals, height, surf)."""
        m = self.model
        N = q.shape[1]
        i32 = self.torch.int32
        normals, height, surf = self._terrain_out(N, normals, height, surf, want_surf)
        _check(_terrain_lib().wbc_gait_terrain_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N), self._ptr(cmd, GAIT_CMD_WORDS, N),
                                                     self._ptr(contact, 1, N, i32), self._ptr(phase, 1, N), self._ptr(mask, 1, N, i32),
                                                     self._ptr(swing, SWING_WORDS, N), self._ptr(events, 1, N, i32), self._terrain_arg(terrain, N),
                                                     self._ptr(normals, 3 * m.nf, N), self._ptr(height, m.nf, N), self._ptr(surf, m.nf, N),
                                                     self._stream()), "wbc_gait_terrain_batch")
        return dict(phase=phase, mask=mask, swing=swing, events=events, normals=normals, height=height, surf=surf)

    def gait_estimated_terrain(self, terrain, q, v, cmd, Jc, r, f_prev, normals, contact, phase, mask, swing, events=None, f_est=None, want_f=False,
                               height=None, surf=None, want_surf=False):
        """gait_estimated() followed by terrain_feet(mask, swing = what it left), as one launch (wbc_gait_estimated_terrain_batch).  normals [12, N]
        is IN/OUT: the contact law reads the previous tick's planes, then this tick's are written over them.  Returns dict(contact, phase, mask,
        swing, events, f_est, normals, height, surf)."""
        m = self.model
        N = q.shape[1]
        i32 = self.torch.int32
        if normals is None:
            raise ValueError("normals is a required in/out tensor ([12, N]; store unit normals before the first call)")
        if f_est is None and want_f:
            f_est = self.empty(3 * m.nf, N)
        _, height, surf = self._terrain_out(N, normals, height, surf, want_surf)
        _check(_terrain_lib().wbc_gait_estimated_terrain_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N),
                                                               self._ptr(cmd, GAIT_CMD_WORDS, N),
                                                               *self._contact_in_ptrs(N, Jc, r, f_prev, normals, contact), self._ptr(phase, 1, N),
                                                               self._ptr(mask, 1, N, i32), self._ptr(swing, SWING_WORDS, N),
                                                               self._ptr(events, 1, N, i32), self._ptr(f_est, 3 * m.nf, N),
                                                               self._terrain_arg(terrain, N), self._ptr(height, m.nf, N), self._ptr(surf, m.nf, N),
                                                               self._stream()), "wbc_gait_estimated_terrain_batch")
        return dict(contact=contact, phase=phase, mask=mask, swing=swing, events=events, f_est=f_est, normals=normals, height=height, surf=surf)

    def set_foothold_params(self, p):
        """p: FootholdParams or dict (see FootholdParams.from_dict): the weights of every later terrain_cost and selection call of this solver."""
        if isinstance(p, dict):
            p = FootholdParams.from_dict(p)
        _check(_foothold_lib().wbc_solver_set_foothold_params(self._h, C.byref(p)), "wbc_solver_set_foothold_params")

    def _foothold_ptrs(self, terrain, N, cost, hold, latch):
        if cost is None or hold is None or latch is None:
            raise ValueError("cost (terrain_cost()), hold ([8, N]) and latch (int32 [N]; store 0 before the first tick) are required tensors")
        assert cost.dtype == self.tdtype and cost.is_contiguous() and cost.numel() == terrain.z.numel(), (cost.dtype, tuple(cost.shape))
        return cost.data_ptr(), self._ptr(hold, 8, N), self._ptr(latch, 1, N, self.torch.int32)

    def terrain_cost(self, terrain, cost=None):
        """The cost of every node of a terrain (wbc_terrain_cost_batch), with the solver's foothold parameters: cost [n_tiles, ny, nx], laid out like
        terrain.z.  One launch; make it once per map.  Returns cost."""
        if cost is None:
            cost = self.torch.empty_like(terrain.z)
        assert cost.dtype == self.tdtype and cost.is_contiguous() and cost.shape == terrain.z.shape, (cost.dtype, tuple(cost.shape))
        assert terrain.z.dtype == self.tdtype, (terrain.z.dtype, self.tdtype)
        _check(_foothold_lib().wbc_terrain_cost_batch(self._h, C.byref(terrain.c), cost.data_ptr(), self._stream()), "wbc_terrain_cost_batch")
        return cost

    def foothold_select(self, terrain, cost, mask, swing, hold, latch):
        """The selection law alone (wbc_foothold_select_batch) on mask and swing as a gait call left them: swing's p1_x, p1_y, hold [8, N] and latch
        (int32 [N]) advance IN PLACE.  Returns dict(swing, hold, latch)."""
        N = swing.shape[1]
        cost_p, hold_p, latch_p = self._foothold_ptrs(terrain, N, cost, hold, latch)
        _check(_foothold_lib().wbc_foothold_select_batch(self._h, self._terrain_arg(terrain, N), cost_p, N, self._ptr(mask, 1, N, self.torch.int32),
                                                         self._ptr(swing, SWING_WORDS, N), hold_p, latch_p, self._stream()),
               "wbc_foothold_select_batch")
        return dict(swing=swing, hold=hold, latch=latch)

    def gait_terrain_select(self, terrain, cost, hold, latch, q, v, cmd, phase, mask, swing, contact=None, events=None, normals=None, height=None,
                            surf=None, want_surf=False):
        """gait(), then foothold_select(), then terrain_feet(mask, swing), as one launch (wbc_gait_terrain_select_batch).  Returns dict(phase, mask,
        swing, events, normals, height, surf, hold, latch)."""
        m = self.model
        N = q.shape[1]
        i32 = self.torch.int32
        normals, height, surf = self._terrain_out(N, normals, height, surf, want_surf)
        _check(_foothold_lib().wbc_gait_terrain_select_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N),
                                                             self._ptr(cmd, GAIT_CMD_WORDS, N), self._ptr(contact, 1, N, i32), self._ptr(phase, 1, N),
                                                             self._ptr(mask, 1, N, i32), self._ptr(swing, SWING_WORDS, N),
                                                             self._ptr(events, 1, N, i32), self._terrain_arg(terrain, N),
                                                             self._ptr(normals, 3 * m.nf, N), self._ptr(height, m.nf, N), self._ptr(surf, m.nf, N),
                                                             *self._foothold_ptrs(terrain, N, cost, hold, latch), self._stream()),
               "wbc_gait_terrain_select_batch")
        return dict(phase=phase, mask=mask, swing=swing, events=events, normals=normals, height=height, surf=surf, hold=hold, latch=latch)

    def gait_estimated_terrain_select(self, terrain, cost, hold, latch, q, v, cmd, Jc, r, f_prev, normals, contact, phase, mask, swing, events=None,
                                      f_est=None, want_f=False, height=None, surf=None, want_surf=False):
        """gait_estimated(), then foothold_select(), then terrain_feet(mask, swing), as one launch (wbc_gait_estimated_terrain_select_batch).
        normals [12, N] is IN/OUT as in gait_estimated_terrain().  Returns dict(contact, phase, mask, swing, events, f_est, normals, height, surf,
        hold, latch)."""
        m = self.model
        N = q.shape[1]
        i32 = self.torch.int32
        if normals is None:
            raise ValueError("normals is a required in/out tensor ([12, N]; store unit normals before the first call)")
        if f_est is None and want_f:
            f_est = self.empty(3 * m.nf, N)
        _, height, surf = self._terrain_out(N, normals, height, surf, want_surf)
        _check(_foothold_lib().wbc_gait_estimated_terrain_select_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N),
                                                                       self._ptr(cmd, GAIT_CMD_WORDS, N),
                                                                       *self._contact_in_ptrs(N, Jc, r, f_prev, normals, contact),
                                                                       self._ptr(phase, 1, N), self._ptr(mask, 1, N, i32),
                                                                       self._ptr(swing, SWING_WORDS, N), self._ptr(events, 1, N, i32),
                                                                       self._ptr(f_est, 3 * m.nf, N), self._terrain_arg(terrain, N),
                                                                       self._ptr(height, m.nf, N), self._ptr(surf, m.nf, N),
                                                                       *self._foothold_ptrs(terrain, N, cost, hold, latch), self._stream()),
               "wbc_gait_estimated_terrain_select_batch")
        return dict(contact=contact, phase=phase, mask=mask, swing=swing, events=events, f_est=f_est, normals=normals, height=height, surf=surf,
                    hold=hold, latch=latch)

    def set_odom_params(self, p):
        """p: OdomParams or dict (see OdomParams.from_dict): the blend gains of every later base-estimate call of this solver."""
        if isinstance(p, dict):
            p = OdomParams.from_dict(p)
        _check(_odom_lib().wbc_solver_set_odom_params(self._h, C.byref(p)), "wbc_solver_set_odom_params")

    def _odom_ptrs(self, N, q, v, normals, height, base, anchor, odo, q_est, v_est):
        """-> (height, base, anchor, odo, q_est, v_est pointers, q_est, v_est); q_est / v_est None: fresh tensors (pass q, v themselves to write
        rows 0-2 in place)"""
        m = self.model
        if base is None or anchor is None or odo is None:
            raise ValueError("base ([6, N]; store the start state), anchor ([12, N]) and odo (int32 [N]; store 0 before the first tick) are required tensors")
        q_est = self.empty(m.nq, N) if q_est is None else q_est
        v_est = self.empty(m.nv, N) if v_est is None else v_est
        return (self._ptr(height, m.nf, N), self._ptr(base, 6, N), self._ptr(anchor, 3 * m.nf, N), self._ptr(odo, 1, N, self.torch.int32),
                self._ptr(q_est, m.nq, N), self._ptr(v_est, m.nv, N), q_est, v_est)

    def base_estimate(self, q, v, contact, mask, base, anchor, odo, normals=None, height=None, q_est=None, v_est=None):
        """Base position and linear velocity from leg odometry (wbc_base_estimate_batch).  Rows 0-2 of q and v are never read.  contact, mask
        (int32 [N]): a foot is trusted where both have its bit.  normals [12, N] and height [4, N]: given together or not at all.  base [6, N],
        anchor [12, N] and odo (int32 [N]) advance IN PLACE.  q_est, v_est: rows 0-2 the estimate, the other rows copies; they may be q and v
        themselves.  Returns dict(base, anchor, odo, q_est, v_est)."""
        m = self.model
        N = q.shape[1]
        i32 = self.torch.int32
        hp, bp, ap, op, qp, vp, q_est, v_est = self._odom_ptrs(N, q, v, normals, height, base, anchor, odo, q_est, v_est)
        _check(_odom_lib().wbc_base_estimate_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N), self._ptr(contact, 1, N, i32),
                                                   self._ptr(mask, 1, N, i32), self._ptr(normals, 3 * m.nf, N), hp, bp, ap, op, qp, vp,
                                                   self._stream()), "wbc_base_estimate_batch")
        return dict(base=base, anchor=anchor, odo=odo, q_est=q_est, v_est=v_est)

    def gait_estimated_odom(self, q, v, cmd, Jc, r, f_prev, normals, contact, phase, mask, swing, base, anchor, odo, height=None, q_est=None,
                            v_est=None, events=None, f_est=None, want_f=False):
        """base_estimate() on contact and mask as they arrive (the previous tick's), then gait_estimated(q_est, v_est), as one launch
        (wbc_gait_estimated_odom_batch).  contact, phase, mask, swing, base, anchor and odo advance IN PLACE.  height None: new anchors are not
        dropped onto the planes.  Returns dict(contact, phase, mask, swing, events, f_est, base, anchor, odo, q_est, v_est)."""
        m = self.model
        N = q.shape[1]
        i32 = self.torch.int32
        if f_est is None and want_f:
            f_est = self.empty(3 * m.nf, N)
        hp, bp, ap, op, qp, vp, q_est, v_est = self._odom_ptrs(N, q, v, normals, height, base, anchor, odo, q_est, v_est)
        _check(_odom_lib().wbc_gait_estimated_odom_batch(self._h, N, self._ptr(q, m.nq, N), self._ptr(v, m.nv, N), self._ptr(cmd, GAIT_CMD_WORDS, N),
                                                         *self._contact_in_ptrs(N, Jc, r, f_prev, normals, contact), self._ptr(phase, 1, N),
                                                         self._ptr(mask, 1, N, i32), self._ptr(swing, SWING_WORDS, N), self._ptr(events, 1, N, i32),
                                                         self._ptr(f_est, 3 * m.nf, N), hp, bp, ap, op, qp, vp, self._stream()),
               "wbc_gait_estimated_odom_batch")
        return dict(contact=contact, phase=phase, mask=mask, swing=swing, events=events, f_est=f_est, base=base, anchor=anchor, odo=odo,
                    q_est=q_est, v_est=v_est)

    def compute_base_estimate(self, q, v, contact, mask, base, anchor, odo=0, normals=None, height=None):
        """Single-robot host-array form of base_estimate (numpy float64, fp64 solvers): returns (base[6], anchor[12], odo, q_est[19], v_est[18]);
        the inputs are not modified."""
        import numpy as np
        arr = lambda a, n: None if a is None else np.ascontiguousarray(np.asarray(a, np.float64).reshape(n))
        q, v, normals, height = arr(q, 19), arr(v, 18), arr(normals, 12), arr(height, 4)
        base, anchor = arr(base, 6).copy(), arr(anchor, 12).copy()
        qe, ve, ow = np.empty(19), np.empty(18), C.c_int(int(odo))
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _check(_odom_lib().wbc_compute_base_estimate(self._h, p(q), p(v), int(contact), int(mask), p(normals), p(height), p(base), p(anchor),
                                                     C.byref(ow), p(qe), p(ve)), "wbc_compute_base_estimate")
        return base, anchor, ow.value, qe, ve

    def compute_contact_estimate(self, Jc, r, f_prev, normals, contact=0):
        """Single-robot host-array form of contact_estimate (numpy float64, fp64 solvers; Jc [216] row-major 12 x 18): returns (contact, f_est[12],
        fn_est[4], singular)."""
        d = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        Jc, r, f_prev, normals = d(Jc), d(r), d(f_prev), d(normals)
        assert Jc.size == 216 and r.size == 18 and f_prev.size == 12 and normals.size == 12
        fe, fn = np.zeros(12), np.zeros(4)
        cw, sg = C.c_int(int(contact)), C.c_int(0)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _check(_contact_lib().wbc_compute_contact_estimate(self._h, p(Jc), p(r), p(f_prev), p(normals), C.byref(cw), p(fe), p(fn), C.byref(sg)),
               "wbc_compute_contact_estimate")
        return cw.value, fe, fn, sg.value

    def rollout_tracking(self, horizon, q, v, plan, normals, mu, mask, out, w_des, vdot_des, obs_integ=None, obs_r=None,
                         tau_ext=None, tau_traj=None, com_traj=None, payload=None):
        """rollout() with the planner in the loop: w_des / vdot_des are scratch buffers regenerated every tick.
        payload: as in rollout() (wbc_rollout_tracking_plant_batch)."""
        m = self.model
        N = q.shape[1]
        bi, bo, ob = self._batch(N, q, v, w_des, vdot_des, normals, mu, mask, out, obs_integ, obs_r)
        tt, ct = self._traj(tau_traj, horizon * m.nj * N), self._traj(com_traj, horizon * 6 * N)
        if payload is not None:
            pl = self._plant(tau_ext, payload, N)
            _check(lib().wbc_rollout_tracking_plant_batch(self._h, N, int(horizon), C.byref(bi), C.byref(bo), C.byref(ob), C.byref(pl),
                                                          self._ptr(plan, PLAN_WORDS, N), tt, ct, self._stream()),
                   "wbc_rollout_tracking_plant_batch")
            return out
        _check(lib().wbc_rollout_tracking_batch(self._h, N, int(horizon), C.byref(bi), C.byref(bo), C.byref(ob),
                                                self._ptr(tau_ext, m.nv, N), self._ptr(plan, PLAN_WORDS, N), tt, ct,
                                                self._stream()), "wbc_rollout_tracking_batch")
        return out

    def compute_torques(self, q, v, w_des, vdot_des, normals, mu, mask, tau_prev=None, f_prev=None, obs_integ=None,
                        obs_r=None):
        """Single-robot host-array call (numpy float64 in/out): the reference's one-robot tick shape."""
        d = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
        q, v, w_des, vdot_des, normals, mu, tau_prev, f_prev = map(d, (q, v, w_des, vdot_des, normals, mu, tau_prev, f_prev))
        if obs_integ is not None:
            assert obs_integ.dtype == np.float64 and obs_integ.flags.c_contiguous
            assert obs_r.dtype == np.float64 and obs_r.flags.c_contiguous
        tau = np.zeros(self.model.nj)
        f = np.zeros(3 * self.model.nf)
        st = C.c_int(0)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        _check(lib().wbc_compute_torques(self._h, p(q), p(v), p(w_des), p(vdot_des), p(normals), p(mu), int(mask),
                                         p(tau_prev), p(f_prev), p(obs_integ), p(obs_r), p(tau), p(f), C.byref(st)),
               "wbc_compute_torques")
        return tau, f, st.value

    def one_image(self):
        """wbc_one_map: numpy views of the solver's pinned single-robot image (fp64 solvers).  Write q, v, w_des, vdot_des, normals,
        mu, mask[0] (and tau_prev, f_prev, obs_integ, obs_r with the observer on) in place, call one_tick(), read tau, f, status[0]."""
        class _Img(C.Structure):
            _fields_ = [(k, C.POINTER(C.c_double)) for k in ("q", "v", "w_des", "vdot_des", "normals", "mu", "tau_prev", "f_prev", "obs_integ", "obs_r", "tau", "f")] + \
                       [(k, C.POINTER(C.c_int)) for k in ("mask", "status", "iters")]
        img = _Img()
        _check(lib().wbc_one_map(self._h, C.byref(img)), "wbc_one_map")
        m = self.model
        sizes = dict(q=m.nq, v=m.nv, w_des=6, vdot_des=m.nv, normals=3 * m.nf, mu=m.nf, tau_prev=m.nj, f_prev=3 * m.nf, obs_integ=m.nv,
                     obs_r=m.nv, tau=m.nj, f=3 * m.nf, mask=1, status=1, iters=1)
        return {k: np.ctypeslib.as_array(getattr(img, k), shape=(n,)) for k, n in sizes.items()}

    def one_tick(self):
        rc = lib().wbc_one_tick(self._h)
        if rc:
            _check(rc, "wbc_one_tick")

    def observer_init(self, q, v):
        """Observer start-up of the single-robot loop: returns (integ = M(q) v, r = 0) as numpy float64 arrays."""
        d = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        q, v = d(q), d(v)
        integ, r = np.zeros(self.model.nv), np.ones(self.model.nv)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _check(lib().wbc_observer_init(self._h, p(q), p(v), p(integ), p(r)), "wbc_observer_init")
        return integ, r

    def compute_reference(self, q, v, plan, t=0.0):
        """Single-robot host-array planner call (numpy float64): returns (w_des[6], vdot_des[nv], com[6])."""
        d = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        q, v, plan = d(q), d(v), d(plan)
        w, vd, com = np.zeros(6), np.zeros(self.model.nv), np.zeros(6)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _check(lib().wbc_compute_reference(self._h, p(q), p(v), p(plan), C.c_double(t), p(w), p(vd), p(com)),
               "wbc_compute_reference")
        return w, vd, com

    def qp_handover(self):
        """states of the last two-kernel tick that the per-lane QP kernel handed to the dense active-set kernel (synchronises)"""
        c = C.c_int(0)
        _check(lib().wbc_solver_qp_handover(self._h, C.byref(c)), "wbc_solver_qp_handover")
        return c.value

    def enable_timing(self, on=1):
        """0 = off, 1 = HIP events around every kernel, k > 1 = around the kernels of every k-th tick."""
        _check(lib().wbc_solver_enable_timing(self._h, int(on)), "wbc_solver_enable_timing")

    def collect_timing(self):
        ms = (C.c_double * 6)()
        cnt = (C.c_int * 6)()
        _check(lib().wbc_solver_collect_timing_n(self._h, ms, cnt, 6), "wbc_solver_collect_timing_n")
        names = ("dyn", "qp", "rnea", "fused", "qp_lane", "rollout")  # fused = one-kernel tick of small batches; dyn = fused sweep (mass_jac kernel with WBC_SWEEP=split); rnea = rnea_step front half
        out = {}
        for i, n in enumerate(names):
            out[n + "_ms"] = ms[i]
            out[n + "_launches"] = cnt[i]
        return out


def shard_range(n_total, n_shards, shard):
    """wbc_shard_range: (start, count) of a shard's contiguous slice."""
    st, cnt = C.c_size_t(), C.c_size_t()
    _check(lib().wbc_shard_range(n_total, n_shards, shard, C.byref(st), C.byref(cnt)), "wbc_shard_range")
    return st.value, cnt.value


def qp_dense_batch(H, g, Cm=None, d=None, meq=0, max_iter=200, tol=None, want_lambda=True, stream=None):
    """wbc_qp_dense_batch: N dense QPs of one run-time size, one per wavefront (csrc/qp_general.hip.hpp).
        min 1/2 x'Hx + g'x   s.t.   Cm[:, :meq] x = d[:, :meq],   Cm[:, meq:] x >= d[:, meq:]
    H [N, n, n], g [N, n], Cm [N, m, n], d [N, m]: contiguous CUDA tensors of one dtype (float64 / float32), n <= 36, m <= 64.
    Returns dict(x [N, n], lam [N, m] | None, status [N] int32 (0 ok, 1 iteration limit, 2 infeasible, 3 H not PD), iters [N]).
    Enqueued on `stream` (default: torch's current stream); does not synchronise."""
    import torch
    if H.dtype not in (torch.float64, torch.float32):
        raise TypeError("H must be float64 or float32")
    N, n = int(H.shape[0]), int(H.shape[1])
    m = 0 if Cm is None else int(Cm.shape[1])
    ts = [H, g] + ([Cm, d] if m else [])
    for t in ts:
        if not (t.is_cuda and t.is_contiguous() and t.dtype == H.dtype and int(t.shape[0]) == N):
            raise ValueError("qp_dense_batch: contiguous CUDA tensors of one dtype and one batch size")
    if tuple(H.shape) != (N, n, n) or tuple(g.shape) != (N, n) or (m and (tuple(Cm.shape) != (N, m, n) or tuple(d.shape) != (N, m))):
        raise ValueError("qp_dense_batch: shapes H [N,n,n], g [N,n], Cm [N,m,n], d [N,m]")
    if tol is None:
        tol = 1e-9 if H.dtype == torch.float64 else 1e-4
    x = torch.empty((N, n), dtype=H.dtype, device=H.device)
    lam = torch.empty((N, m), dtype=H.dtype, device=H.device) if (want_lambda and m) else None
    status = torch.empty(N, dtype=torch.int32, device=H.device)
    iters = torch.empty(N, dtype=torch.int32, device=H.device)
    st = (stream if stream is not None else torch.cuda.current_stream(H.device)).cuda_stream
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    with torch.cuda.device(H.device):
        _check(lib().wbc_qp_dense_batch(0 if H.dtype == torch.float64 else 1, N, n, m, int(meq), p(H), p(g), p(Cm) if m else None, p(d) if m else None,
                                        int(max_iter), float(tol), p(x), p(lam), p(status), p(iters), C.c_void_p(st)), "wbc_qp_dense_batch")
    return {"x": x, "lam": lam, "status": status, "iters": iters}


GATHER_NONE, GATHER_RCCL, GATHER_PEER_COPY = 0, 1, 2


class MultiSolver:
    """wbc_multi_*: ONE process, one solver per device of the node (the C-ABI path a C++ host uses; the torchrun path of
    bench.py / sharding.py is one process per GPU instead).  devices may repeat a device for NONE / PEER_COPY gathers."""

    def __init__(self, model, params=None, dtype="f64", devices=(0,), max_batch_total=4096, gather="none", options=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible to torch: the WBC hot path has no CPU fallback")
        self.torch, self.model, self.dtype = torch, model, dtype
        self.tdtype = torch.float64 if dtype == "f64" else torch.float32
        self.devices = [int(d) for d in devices]
        self.params = params if params is not None else Params.default(dtype)
        self.options = SolverOptions.make(options)
        self.max_batch_total = int(max_batch_total)
        backend = dict(none=GATHER_NONE, rccl=GATHER_RCCL, peer=GATHER_PEER_COPY)[gather]
        arr = (C.c_int * len(self.devices))(*self.devices)
        h = C.c_void_p()
        _check(lib().wbc_multi_create(model._h, C.byref(self.params), F64 if dtype == "f64" else F32, arr, len(self.devices),
                                      self.max_batch_total, backend, C.byref(self.options), C.byref(h)), "wbc_multi_create")
        self._h = h
        self.n = lib().wbc_multi_size(self._h)

    def __del__(self):
        try:
            lib().wbc_multi_destroy(self._h)
        except Exception:
            pass

    @property
    def rccl_ranks(self):
        return lib().wbc_multi_rccl_ranks(self._h)

    def stream(self, k):
        return lib().wbc_multi_stream(self._h, k)

    def synchronize(self):
        _check(lib().wbc_multi_synchronize(self._h), "wbc_multi_synchronize")

    def sync_torch_streams(self):
        """Wait for torch's current stream on every shard device: the shard streams (wbc_multi_stream) do not synchronise
        with torch's streams or the null stream, so buffers produced there must be complete before the first tick."""
        for dev in sorted(set(self.devices)):
            self.torch.cuda.current_stream(self.torch.device("cuda", dev)).synchronize()

    def scatter(self, full, rows, n_total, dtype=None):
        """host/any-device [rows, n_total] tensor -> list of per-shard contiguous [rows, count_k] tensors on devices[k]"""
        outs = []
        for k, dev in enumerate(self.devices):
            st, cnt = shard_range(n_total, self.n, k)
            x = full[..., st:st + cnt].contiguous().to(self.torch.device("cuda", dev))
            outs.append(x.to(dtype) if dtype is not None else x)
        return outs

    def prepare_step(self, n_total, ins, obs=None, want_mats=False, warm=False):
        """ins: dict name -> list of per-shard tensors (q, v, w_des, vdot_des, normals, mu, mask[, tau_prev, f_prev]);
        obs: (list integ, list r) or None.  Returns (tick, outs): tick() enqueues one control tick on every shard
        (wbc_multi_step_batch), outs is a list of per-shard output dicts.  warm: wbc_multi_step_batch_warm -- every shard carries
        its active sets in outs[k]["active"] (int32 [count_k], zero = cold) from tick to tick."""
        torch, m = self.torch, self.model
        BI, BO, OS = (_BatchIn * self.n)(), (_BatchOut * self.n)(), (_ObsState * self.n)()
        outs, keep = [], []
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        for k, dev in enumerate(self.devices):
            _, cnt = shard_range(n_total, self.n, k)
            d = torch.device("cuda", dev)
            o = dict(tau=torch.zeros((m.nj, cnt), dtype=self.tdtype, device=d), f=torch.zeros((3 * m.nf, cnt), dtype=self.tdtype, device=d),
                     status=torch.zeros(cnt, dtype=torch.int32, device=d), iters=torch.zeros(cnt, dtype=torch.int32, device=d))
            if want_mats:
                o.update(M=torch.empty((m.nv * (m.nv + 1) // 2, cnt), dtype=self.tdtype, device=d), h=torch.empty((m.nv, cnt), dtype=self.tdtype, device=d),
                         Jc=torch.empty((3 * m.nf * m.nv, cnt), dtype=self.tdtype, device=d), pf=torch.empty((3 * m.nf, cnt), dtype=self.tdtype, device=d))
            g = lambda name: ins[name][k] if name in ins and ins[name] is not None else None
            for name in ("q", "v", "w_des", "vdot_des", "normals", "mu", "mask", "tau_prev", "f_prev"):
                t = g(name)
                assert t is None or (t.is_cuda and t.is_contiguous() and t.device == d and t.shape[-1] == cnt), (name, k)
            BI[k] = _BatchIn(p(g("q")), p(g("v")), p(g("w_des")), p(g("vdot_des")), p(g("normals")), p(g("mu")), p(g("mask")),
                             p(g("tau_prev")), p(g("f_prev")))
            BO[k] = _BatchOut(p(o["tau"]), p(o["f"]), p(o["status"]), p(o["iters"]), p(o.get("M")), p(o.get("h")), p(o.get("Jc")), p(o.get("pf")))
            if obs is not None:
                OS[k] = _ObsState(p(obs[0][k]), p(obs[1][k]))
            if warm:
                o["active"] = torch.zeros(max(cnt, 1), dtype=torch.int32, device=d)[:cnt]
            outs.append(o)
        ACT = (C.c_void_p * self.n)(*[o["active"].data_ptr() if warm else None for o in outs])
        keep = (ins, obs, outs, BI, BO, OS, ACT)
        fn, h, has_obs = lib().wbc_multi_step_batch, self._h, obs is not None
        fn_warm = lib().wbc_multi_step_batch_warm
        # The shard streams are library-created non-blocking streams: nothing orders them behind the torch streams that
        # produced these buffers (scatter()'s copies, the zero-fills above, a caller's observer state).  One-off cost.
        self.sync_torch_streams()

        def tick(_keep=keep):
            rc = fn_warm(h, n_total, BI, BO, OS if has_obs else None, ACT) if warm else fn(h, n_total, BI, BO, OS if has_obs else None)
            if rc:
                _check(rc, "wbc_multi_step_batch_warm" if warm else "wbc_multi_step_batch")
        tick.capi = (BI, BO, OS, ACT, has_obs)   # (for prepare_tick_gather)
        return tick, outs

    def allgather_tau(self, n_total, outs, tau_all=None):
        """every device receives all torques: returns list (per device) of [n_shards, nj * count_0] tensors"""
        torch, m = self.torch, self.model
        _, c0 = shard_range(n_total, self.n, 0)
        if tau_all is None:
            tau_all = [torch.zeros((self.n, m.nj * c0), dtype=self.tdtype, device=torch.device("cuda", d)) for d in self.devices]
            self.sync_torch_streams()   # the zero-fills run on torch's streams, the gather on the shard streams
        loc = (C.c_void_p * self.n)(*[o["tau"].data_ptr() for o in outs])
        allp = (C.c_void_p * self.n)(*[t.data_ptr() for t in tau_all])
        _check(lib().wbc_multi_allgather_tau(self._h, n_total, loc, allp), "wbc_multi_allgather_tau")
        return tau_all

    def allgather_tau_async(self, n_total, outs, tau_all, slot):
        """wbc_multi_allgather_tau_async: the gather of `outs` (slot 0 / 1 of a double-buffered tau) on the gather streams, beside the next tick"""
        loc = (C.c_void_p * self.n)(*[o["tau"].data_ptr() for o in outs])
        allp = (C.c_void_p * self.n)(*[t.data_ptr() for t in tau_all])
        _check(lib().wbc_multi_allgather_tau_async(self._h, n_total, loc, allp, int(slot)), "wbc_multi_allgather_tau_async")
        return tau_all

    def prepare_tick_gather(self, n_total, ticks, tau_alls, warm=False):
        """wbc_multi_tick_gather as a closure: ticks = [(BI, BO, OS, ACT) per slot] as kept by prepare_step (its _keep tuple), tau_alls = per slot the
        per-device gather buffers.  Returns run(slot): gather_wait(slot) + tick into the slot's tau + overlapped gather of the slot, ONE call."""
        fn, h = lib().wbc_multi_tick_gather, self._h
        slots = []
        for (BI, BO, OS, ACT, has_obs), tau_all in zip(ticks, tau_alls):
            allp = (C.c_void_p * self.n)(*[t.data_ptr() for t in tau_all])
            slots.append((BI, BO, OS if has_obs else None, ACT if warm else None, allp))

        def run(slot, _keep=(ticks, tau_alls, slots)):
            BI, BO, OS, ACT, allp = slots[slot]
            rc = fn(h, n_total, BI, BO, OS, ACT, allp, slot)
            if rc:
                _check(rc, "wbc_multi_tick_gather")
        return run

    @property
    def issue_threads(self):
        return lib().wbc_multi_issue_threads(self._h)

    def set_peer_copies(self, on):
        """wbc_multi_set_peer_copies: 1 = the peer gather never stores through peer mappings (for gather buffers from virtual-memory pools)"""
        _check(lib().wbc_multi_set_peer_copies(self._h, 1 if on else 0), "wbc_multi_set_peer_copies")

    @property
    def gather_pushes(self):
        """1 when the next peer gather would use the push kernel"""
        return lib().wbc_multi_gather_pushes(self._h)

    def host_stats(self, reset=True):
        """(calls, seconds) the caller has spent inside the tick / rollout / gather entry points since the last reset"""
        calls, sec = C.c_ulonglong(), C.c_double()
        _check(lib().wbc_multi_host_stats(self._h, C.byref(calls), C.byref(sec), 1 if reset else 0), "wbc_multi_host_stats")
        return calls.value, sec.value

    def probe_issue(self, iters=2000):
        """microseconds per EMPTY ticket through the issue threads (serial issue: per empty loop over the shards)"""
        sec = C.c_double()
        _check(lib().wbc_multi_probe_issue(self._h, int(iters), C.byref(sec)), "wbc_multi_probe_issue")
        return sec.value / iters * 1e6

    def gather_wait(self, slot):
        """the shard streams wait (on the device) for the last gather of `slot`: before the tick that overwrites that slot's tau"""
        _check(lib().wbc_multi_gather_wait(self._h, int(slot)), "wbc_multi_gather_wait")

    def step_host(self, q, v, w_des, vdot_des, normals, mu, mask, tau_prev=None, f_prev=None, obs_integ=None, obs_r=None):
        """Host-resident batch (numpy, component-major [ncomp, n_total] in the solver's dtype): scatter, tick, gather.
        Observer state arrays are updated in place.  Returns dict(tau, f, status, iters)."""
        nd = np.float64 if self.dtype == "f64" else np.float32
        n_total = q.shape[1]
        c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=nd)
        q, v, w_des, vdot_des, normals, mu, tau_prev, f_prev = map(c, (q, v, w_des, vdot_des, normals, mu, tau_prev, f_prev))
        mask = np.ascontiguousarray(mask, dtype=np.int32)
        for a in (obs_integ, obs_r):
            assert a is None or (a.dtype == nd and a.flags.c_contiguous)
        m = self.model
        out = dict(tau=np.zeros((m.nj, n_total), nd), f=np.zeros((3 * m.nf, n_total), nd), status=np.zeros(n_total, np.int32),
                   iters=np.zeros(n_total, np.int32))
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        bi = _BatchIn(p(q), p(v), p(w_des), p(vdot_des), p(normals), p(mu), p(mask), p(tau_prev), p(f_prev))
        bo = _BatchOut(p(out["tau"]), p(out["f"]), p(out["status"]), p(out["iters"]), None, None, None, None)
        ob = _ObsState(p(obs_integ), p(obs_r))
        _check(lib().wbc_multi_step_host(self._h, n_total, C.byref(bi), C.byref(bo), C.byref(ob)), "wbc_multi_step_host")
        return out
