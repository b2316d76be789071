"""ctypes binding of libmgcfd_hip.so (include/mgcfd.h).

The Python layer is plumbing for tests, bench.py and torch.distributed — the product is
the HIP library.  There is no CPU fallback: if the shared object is missing or no GPU is
present, construction of a :class:`Solver` raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import List, Optional, Sequence

import numpy as np

from .meshgen import EDGE_DTYPE, LevelMesh, MultigridMesh, to_edge_arrays

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC_DIR = os.path.normpath(os.path.join(PKG_DIR, "..", "csrc"))
# MGCFD_LIB overrides the library path (profiling builds; tools/exp_variants.py)
LIB_PATH = os.environ.get("MGCFD_LIB") or os.path.join(CSRC_DIR, "libmgcfd_hip.so")

NVAR = 5
RK = 3
LOOPS = ("flux", "update", "compute_step", "time_step", "restrict", "prolong", "indirect_rw")
ARR = {"variables": 0, "old_variables": 1, "fluxes": 2, "residuals": 3, "step_factors": 4, "volumes": 5, "stage": 6,
       "time_n": 7, "time_n1": 8, "jst_laplacian": 9, "jst_sensor": 10, "jst_radius": 11,
       "fas_forcing": 12, "fas_start": 13, "viscous_stress": 14, "eddy_viscosity": 15, "wall_distance": 16,
       "sa_nu_tilde": 17, "sa_gradient": 18, "viscous_gradient": 19, "sa_time_n": 20, "sa_time_n1": 21, "sa_length": 22,
       "statistics_mean": 23, "statistics_moments": 24, "upwind_gradient": 25, "upwind_limiter": 26}
NCOLS = {"step_factors": 1, "volumes": 1, "jst_sensor": 1, "jst_radius": 1, "viscous_stress": 12, "eddy_viscosity": 1, "wall_distance": 1,
         "sa_nu_tilde": 1, "sa_gradient": 5, "viscous_gradient": 12, "sa_time_n": 1, "sa_time_n1": 1, "sa_length": 1,
         "statistics_mean": 6, "statistics_moments": 7, "upwind_gradient": 15, "upwind_limiter": 5}    # (every other array: NVAR)
OPT = {"exact": 0, "timing": 1, "indirect_rw": 2, "check_invalid": 3, "flux_variant": 4, "fuse_update": 5, "graph": 6, "rank_split": 7, "stage_wg4": 8}
LIMITERS = {"none": 0, "barth-jespersen": 1, "venkatakrishnan": 2}
UPWIND_VENKAT_K, UPWIND_ENTROPY_FIX = 5.0, 0.1          # MGCFD_UPWIND_VENKAT_K, MGCFD_UPWIND_ENTROPY_FIX
ERR_NAMES = {0: "OK", 1: "ERR_ARG", 2: "ERR_IO", 3: "ERR_HIP", 4: "ERR_NAN", 5: "ERR_NEG_DENSITY",
             6: "ERR_NEG_ENERGY", 7: "ERR_VALIDATION"}

_vp = C.c_void_p
_i64 = C.c_int64


class LevelDesc(C.Structure):
    _fields_ = [("nel", _i64), ("n_edges", _i64), ("n_internal", _i64), ("n_boundary", _i64),
                ("n_wall", _i64), ("internal_start", _i64), ("boundary_start", _i64), ("wall_start", _i64),
                ("volumes", _vp), ("coords", _vp), ("edges", _vp), ("mg_map", _vp), ("mgc", _i64)]


class MgcfdError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {message}")
        self.code = code


# Every symbol include/mgcfd.h declares: (name, restype, argtypes)
# time-step modes (mgcfd_set_time_step): MGCFD_DT_*
DT_MODE = {"reference": 0, "global": 1, "local": 2, "local_legacy": 3}


def _dt_mode(mode) -> int:
    if isinstance(mode, str):
        key = mode.replace("-", "_")
        if key not in DT_MODE:
            raise ValueError(f"time step: unknown mode {mode!r} (one of {', '.join(DT_MODE)})")
        return DT_MODE[key]
    return int(mode)


_SIGNATURES = [
    ("mgcfd_last_error", C.c_char_p, []),
    ("mgcfd_abi_version", C.c_int, []),
    ("mgcfd_mesh_load", C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.POINTER(_vp)]),
    ("mgcfd_mesh_load_ex", C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(_vp)]),
    ("mgcfd_mesh_free", None, [_vp]),
    ("mgcfd_mesh_num_levels", C.c_int, [_vp]),
    ("mgcfd_mesh_variant", C.c_int, [_vp]),
    ("mgcfd_mesh_size", C.c_int, [_vp]),
    ("mgcfd_mesh_level", C.c_int, [_vp, C.c_int, C.POINTER(LevelDesc)]),
    ("mgcfd_write_array", C.c_int, [C.c_char_p, _vp, _i64, C.c_int]),
    ("mgcfd_identify_differences", C.c_int, [_vp, _vp, _i64, C.c_int, C.POINTER(_i64)]),
    ("mgcfd_create", C.c_int, [C.POINTER(LevelDesc), C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    ("mgcfd_plan_audit", C.c_int, [C.POINTER(LevelDesc), C.c_int, C.c_int, C.POINTER(_i64), C.POINTER(C.POINTER(_i64)), C.c_char_p, _i64]),
    ("mgcfd_create_partitioned_mg", C.c_int, [C.POINTER(LevelDesc), C.c_int, C.c_int, C.c_int, C.POINTER(_i64),
                                                 C.POINTER(C.POINTER(_i64)), C.POINTER(_vp)]),
    ("mgcfd_create_from_mesh", C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    ("mgcfd_create_partitioned", C.c_int, [C.POINTER(LevelDesc), C.c_int, C.c_int, C.c_int, C.POINTER(_i64), C.POINTER(_vp)]),
    ("mgcfd_halo_plan", C.c_int, [_vp, C.c_int, _i64, _vp, C.POINTER(C.c_int)]),
    ("mgcfd_halo_pack", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp]),
    ("mgcfd_halo_unpack", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp]),
    ("mgcfd_destroy", None, [_vp]),
    ("mgcfd_live_device_resources", C.c_int, [C.POINTER(_i64)]),
    ("mgcfd_set_option", C.c_int, [_vp, C.c_int, C.c_int]),
    ("mgcfd_level_has_half_rows", C.c_int, [_vp, C.c_int, C.POINTER(C.c_int)]),
    ("mgcfd_pending_invalid_state", C.c_int, [_vp, C.POINTER(C.c_int64)]),
    ("mgcfd_level_has_order_free", C.c_int, [_vp, C.c_int, C.POINTER(C.c_int)]),
    ("mgcfd_level_stage_wg4", C.c_int, [_vp, C.c_int, C.POINTER(C.c_int)]),
    ("mgcfd_level_tiling", C.c_int, [_vp, C.c_int, C.POINTER(C.c_int64)]),
    ("mgcfd_invalid_state_location", C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    ("mgcfd_get_option", C.c_int, [_vp, C.c_int, C.POINTER(C.c_int)]),
    ("mgcfd_set_stream", C.c_int, [_vp, _vp]),
    ("mgcfd_synchronize", C.c_int, [_vp]),
    ("mgcfd_num_levels", C.c_int, [_vp]),
    ("mgcfd_level_nel", _i64, [_vp, C.c_int]),
    ("mgcfd_level_num_internal_edges", _i64, [_vp, C.c_int]),
    ("mgcfd_get_far_field", C.c_int, [_vp, _vp]),
    ("mgcfd_copy_old_variables", C.c_int, [_vp, C.c_int]),
    ("mgcfd_compute_step_factor", C.c_int, [_vp, C.c_int]),
    ("mgcfd_compute_flux_edge", C.c_int, [_vp, C.c_int]),
    ("mgcfd_compute_boundary_flux_edge", C.c_int, [_vp, C.c_int]),
    ("mgcfd_compute_wall_flux_edge", C.c_int, [_vp, C.c_int]),
    ("mgcfd_compute_fluxes", C.c_int, [_vp, C.c_int]),
    ("mgcfd_time_step", C.c_int, [_vp, C.c_int, C.c_int]),
    ("mgcfd_zero_fluxes", C.c_int, [_vp, C.c_int]),
    ("mgcfd_indirect_rw", C.c_int, [_vp, C.c_int]),
    ("mgcfd_residual", C.c_int, [_vp, C.c_int]),
    ("mgcfd_calc_rms", C.c_int, [_vp, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_check_for_invalid_variables", C.c_int, [_vp, C.c_int, C.POINTER(_i64)]),
    ("mgcfd_restrict", C.c_int, [_vp, C.c_int]),
    ("mgcfd_prolong", C.c_int, [_vp, C.c_int]),
    ("mgcfd_smooth", C.c_int, [_vp, C.c_int, C.c_int]),
    ("mgcfd_run_cycles", C.c_int, [_vp, C.c_int, _vp]),
    ("mgcfd_get_array", C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    ("mgcfd_set_array", C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    ("mgcfd_array_devptr", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(C.c_int64)]),
    ("mgcfd_array_written", C.c_int, [_vp, C.c_int, C.c_int]),
    ("mgcfd_get_edges", C.c_int, [_vp, C.c_int, _vp]),
    ("mgcfd_accept_restricted", C.c_int, [_vp, C.c_int, _vp]),
    ("mgcfd_get_loop_iters", C.c_int, [_vp, C.c_int, _vp]),
    ("mgcfd_get_loop_times", C.c_int, [_vp, C.c_int, _vp]),
    ("mgcfd_reset_monitoring", C.c_int, [_vp]),
    ("mgcfd_get_flux_kernel_time", C.c_int, [_vp, C.c_int, C.POINTER(C.c_double), C.POINTER(_i64)]),
    ("mgcfd_bench_flux", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_bench_indirect_rw", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_bench_stream_ceiling", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_diag_fast_math", C.c_int, [_vp, C.c_int, _i64, _vp, _vp]),
    ("mgcfd_device_warm_up", C.c_int, [C.c_int]),
    ("mgcfd_step_factor_local", C.c_int, [_vp, C.c_int]),
    ("mgcfd_step_factor_min_devptr", C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    ("mgcfd_step_factor_partials_devptr", C.c_int, [_vp, C.c_int, C.POINTER(_vp), C.POINTER(C.c_int)]),
    ("mgcfd_sweep_stage", C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
    ("mgcfd_sweep_begin_partials", C.c_int, [_vp, C.c_int]),
    ("mgcfd_sweep_end_partials", C.c_int, [_vp, C.c_int]),
    ("mgcfd_step_factor_apply", C.c_int, [_vp, C.c_int]),
    ("mgcfd_sweep_begin", C.c_int, [_vp, C.c_int]),
    ("mgcfd_sweep_flux0", C.c_int, [_vp, C.c_int]),
    ("mgcfd_sweep_end", C.c_int, [_vp, C.c_int]),
    ("mgcfd_residual_sumsq", C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    ("mgcfd_rccl_unique_id", C.c_int, [_vp]),
    ("mgcfd_rank_attach_rccl", C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    ("mgcfd_rank_detach", C.c_int, [_vp]),
    ("mgcfd_rank_set_halo", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(_i64), C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_vp)]),
    ("mgcfd_rank_halo_info", C.c_int, [_vp, C.c_int, C.POINTER(_i64)]),
    ("mgcfd_rank_exchange", C.c_int, [_vp, C.c_int]),
    ("mgcfd_rank_sweeps", C.c_int, [_vp, C.c_int, C.c_int]),
    ("mgcfd_rank_residual_sumsq", C.c_int, [_vp, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_group_create", C.c_int, [C.c_int, C.POINTER(_vp), C.POINTER(_vp)]),
    ("mgcfd_group_destroy", None, [_vp]),
    ("mgcfd_group_exchange", C.c_int, [_vp, C.c_int]),
    ("mgcfd_rank_attach_plain", C.c_int, [_vp, C.c_int, C.c_int]),
    ("mgcfd_rank_ipc_export_size", C.c_int, [_vp, C.c_int, C.POINTER(C.c_int64)]),
    ("mgcfd_rank_ipc_export", C.c_int, [_vp, C.c_int, _vp]),
    ("mgcfd_rank_ipc_attach", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(_vp)]),
    ("mgcfd_rank_ipc_status", C.c_int, [_vp, C.c_int, C.POINTER(C.c_int)]),
    ("mgcfd_rank_info", C.c_int, [_vp, C.POINTER(C.c_int)]),
    ("mgcfd_rank_graph_status", C.c_int, [_vp, C.c_int, C.POINTER(_i64)]),
    ("mgcfd_group_cycles", C.c_int, [_vp, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_rank_cycles", C.c_int, [_vp, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_rank_ipc_detach", C.c_int, [_vp, C.c_int]),
    ("mgcfd_group_sweeps", C.c_int, [_vp, C.c_int, C.c_int]),
    ("mgcfd_group_sweeps_rms", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_group_rms", C.c_int, [_vp, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_group_synchronize", C.c_int, [_vp]),
    ("mgcfd_surface_loads", C.c_int, [_vp, C.c_int, _vp, _vp]),
    ("mgcfd_run_cycles_loads", C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    ("mgcfd_load_coefficients", C.c_int, [_vp, _vp, C.c_double, C.c_double, _vp]),
    ("mgcfd_rank_set_wall_slots", C.c_int, [_vp, C.c_int, _i64, _i64, _vp]),
    ("mgcfd_group_surface_loads", C.c_int, [_vp, C.c_int, _vp, _vp]),
    ("mgcfd_group_cycles_loads", C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    ("mgcfd_rank_surface_loads", C.c_int, [_vp, C.c_int, _vp, _vp]),
    ("mgcfd_rank_cycles_loads", C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    ("mgcfd_free_stream_constants", C.c_int, [C.c_double, C.c_double, _vp]),
    ("mgcfd_set_free_stream", C.c_int, [_vp, C.c_double, C.c_double, C.c_int]),
    ("mgcfd_get_free_stream", C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("mgcfd_group_set_free_stream", C.c_int, [_vp, C.c_double, C.c_double, C.c_int]),
    ("mgcfd_set_time_step", C.c_int, [_vp, C.c_int, C.c_double]),
    ("mgcfd_get_time_step", C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    ("mgcfd_group_set_time_step", C.c_int, [_vp, C.c_int, C.c_double]),
    ("mgcfd_set_residual_smoothing", C.c_int, [_vp, C.c_double, C.c_int]),
    ("mgcfd_get_residual_smoothing", C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("mgcfd_bench_residual_smoothing", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_set_dual_time", C.c_int, [_vp, C.c_double, C.c_double]),
    ("mgcfd_get_dual_time", C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int)]),
    ("mgcfd_dual_time_set_order", C.c_int, [_vp, C.c_int]),
    ("mgcfd_dual_time_reset", C.c_int, [_vp]),
    ("mgcfd_dual_time_begin_step", C.c_int, [_vp]),
    ("mgcfd_advance", C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    ("mgcfd_set_jst", C.c_int, [_vp, C.c_double, C.c_double, C.c_int]),
    ("mgcfd_get_jst", C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    ("mgcfd_bench_jst", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_set_fas", C.c_int, [_vp, C.c_int]),
    ("mgcfd_get_fas", C.c_int, [_vp, C.POINTER(C.c_int)]),
    ("mgcfd_fas_restrict", C.c_int, [_vp, C.c_int]),
    ("mgcfd_fas_prolong", C.c_int, [_vp, C.c_int]),
    ("mgcfd_bench_fas", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_set_viscous", C.c_int, [_vp, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int]),
    ("mgcfd_get_viscous", C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                    C.POINTER(C.c_int)]),
    ("mgcfd_viscosity_from_reynolds", C.c_int, [_vp, C.c_double, C.c_double, C.POINTER(C.c_double)]),
    ("mgcfd_set_viscosity_model", C.c_int, [_vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double]),
    ("mgcfd_get_viscosity_model", C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int),
                                             C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("mgcfd_bench_viscous", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_surface_loads_viscous", C.c_int, [_vp, C.c_int, _vp, _vp]),
    ("mgcfd_run_cycles_loads_viscous", C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    ("mgcfd_advance_loads_viscous", C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    ("mgcfd_wall_node_count", C.c_int, [_vp, C.c_int, C.POINTER(_i64)]),
    ("mgcfd_wall_distribution", C.c_int, [_vp, C.c_int, _vp, _vp]),
    ("mgcfd_wall_stress", C.c_int, [_vp, C.c_int, _vp, _vp]),
    ("mgcfd_bench_friction_loads", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_compute_wall_distance", C.c_int, [_vp, C.c_int]),
    ("mgcfd_get_wall_distance", C.c_int, [_vp, C.POINTER(C.c_int)]),
    ("mgcfd_release_wall_distance", C.c_int, [_vp]),
    ("mgcfd_wall_nearest", C.c_int, [_vp, C.c_int, _vp]),
    ("mgcfd_wall_spacing", C.c_int, [_vp, C.c_int, _vp, _vp]),
    ("mgcfd_set_wall_damping", C.c_int, [_vp, C.c_int, C.c_double]),
    ("mgcfd_get_wall_damping", C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    ("mgcfd_bench_wall_distance", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_set_sa_free_stream", C.c_int, [_vp, C.c_double, C.c_int]),
    ("mgcfd_get_sa_free_stream", C.c_int, [_vp, C.POINTER(C.c_double)]),
    ("mgcfd_bench_sa", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_set_sa_unsteady", C.c_int, [_vp, C.c_int, C.c_int, C.c_double]),
    ("mgcfd_get_sa_unsteady", C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    ("mgcfd_set_statistics", C.c_int, [_vp, C.c_int]),
    ("mgcfd_get_statistics", C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(_i64), C.POINTER(C.c_double)]),
    ("mgcfd_statistics_reset", C.c_int, [_vp]),
    ("mgcfd_statistics_sample", C.c_int, [_vp, C.c_double]),
    ("mgcfd_statistics_restore", C.c_int, [_vp, _i64, C.c_double]),
    ("mgcfd_wall_statistics", C.c_int, [_vp, _vp, _vp]),
    ("mgcfd_set_wall_statistics", C.c_int, [_vp, _vp]),
    ("mgcfd_statistics_derive", C.c_int, [C.c_double, _vp, _i64, _vp]),
    ("mgcfd_bench_statistics", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_set_wall_temperature", C.c_int, [_vp, C.c_int, C.c_double]),
    ("mgcfd_get_wall_temperature", C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    ("mgcfd_free_stream_temperature", C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("mgcfd_surface_loads_heat", C.c_int, [_vp, C.c_int, _vp, _vp]),
    ("mgcfd_run_cycles_loads_heat", C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    ("mgcfd_advance_loads_heat", C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    ("mgcfd_wall_heat", C.c_int, [_vp, C.c_int, _vp, _vp]),
    ("mgcfd_bench_wall_heat", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_set_face_gradient", C.c_int, [_vp, C.c_int]),
    ("mgcfd_get_face_gradient", C.c_int, [_vp, C.POINTER(C.c_int)]),
    ("mgcfd_bench_face_gradient", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_set_upwind", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double]),
    ("mgcfd_get_upwind", C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("mgcfd_bench_upwind", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    ("mgcfd_set_cycle", C.c_int, [_vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("mgcfd_get_cycle", C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("mgcfd_run_cycles_from", C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    ("mgcfd_prolong_state", C.c_int, [_vp, C.c_int]),
    ("mgcfd_full_multigrid", C.c_int, [_vp, C.POINTER(C.c_int), _vp]),
]

CYCLE_SHAPES = {"V": 0, "W": 1, "F": 2}
MAX_CYCLE_SWEEPS = 8
EXPORTED_SYMBOLS = tuple(name for name, _, _ in _SIGNATURES)

_lib: Optional[C.CDLL] = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load libmgcfd_hip.so and type every entry point.  Raises if the library is absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise FileNotFoundError(f"{p} not found: build it with `make -C {CSRC_DIR}` "
                                f"(or __graft_entry__.build()); there is no CPU fallback")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64, and a second runtime
    # brought up after the system one finds "no ROCm-capable device".  With torch loaded first this library binds to
    # the same (already loaded) runtime, so do that here when torch is installed — a process that never imports
    # torch (the C++ driver, a plain ctypes user) runs on the system runtime alone.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(p)
    for name, res, args in _SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _check(lib, rc: int):
    if rc != 0:
        raise MgcfdError(rc, (lib.mgcfd_last_error() or b"").decode(errors="replace"))


def _ptr(a: np.ndarray):
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(_vp)


class Mesh:
    """Multigrid input parsed by the library's own readers (the reference's file formats)."""

    def __init__(self, input_dat: str, directory: str = "", duplicate: int = 1, legacy_ordering: bool = False):
        self.lib = load_library()
        h = _vp()
        _check(self.lib, self.lib.mgcfd_mesh_load_ex(input_dat.encode(), directory.encode(), duplicate,
                                                      1 if legacy_ordering else 0, C.byref(h)))
        self.handle = h

    @property
    def num_levels(self) -> int:
        return self.lib.mgcfd_mesh_num_levels(self.handle)

    @property
    def variant(self) -> int:
        return self.lib.mgcfd_mesh_variant(self.handle)

    @property
    def size(self) -> int:
        return self.lib.mgcfd_mesh_size(self.handle)

    def level(self, l: int) -> dict:
        d = LevelDesc()
        _check(self.lib, self.lib.mgcfd_mesh_level(self.handle, l, C.byref(d)))

        def view(addr, n, dt):
            if not addr or n == 0:
                return np.zeros(0, dtype=dt)
            buf = (C.c_char * (n * np.dtype(dt).itemsize)).from_address(addr)
            return np.frombuffer(buf, dtype=dt, count=n).copy()

        return {"nel": d.nel, "n_edges": d.n_edges, "n_internal": d.n_internal, "n_boundary": d.n_boundary,
                "n_wall": d.n_wall, "internal_start": d.internal_start, "boundary_start": d.boundary_start,
                "wall_start": d.wall_start, "volumes": view(d.volumes, d.nel, np.float64),
                "coords": view(d.coords, d.nel * 3, np.float64).reshape(-1, 3),
                "edges": view(d.edges, d.n_edges, EDGE_DTYPE), "mg_map": view(d.mg_map, d.mgc, np.int64)}

    def close(self):
        if getattr(self, "handle", None):
            self.lib.mgcfd_mesh_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _level_descs(levels: Sequence[dict]):
    """LevelDesc array over in-memory level dicts + the arrays that must stay alive while it is used."""
    descs = (LevelDesc * len(levels))()
    keep = []
    for l, L in enumerate(levels):
        vol = np.ascontiguousarray(L["volumes"], dtype=np.float64)
        edges = np.ascontiguousarray(L["edges"], dtype=EDGE_DTYPE)
        # (an empty array is "no coordinates", as Mesh.level hands them out for a level loaded without its .coords file)
        crd = None if L.get("coords") is None or np.size(L["coords"]) == 0 else np.ascontiguousarray(L["coords"], dtype=np.float64)
        mp = None if L.get("mg_map") is None else np.ascontiguousarray(L["mg_map"], dtype=np.int64)
        keep += [vol, edges, crd, mp]
        d = descs[l]
        d.nel = int(L["nel"])
        d.n_edges = len(edges)
        d.n_internal, d.n_boundary, d.n_wall = int(L["n_internal"]), int(L["n_boundary"]), int(L["n_wall"])
        d.internal_start = int(L.get("internal_start", 0))
        d.boundary_start = int(L.get("boundary_start", d.n_internal))
        d.wall_start = int(L.get("wall_start", d.n_internal + d.n_boundary))
        d.volumes = _ptr(vol)
        d.coords = _ptr(crd) if crd is not None else None
        d.edges = _ptr(edges)
        d.mg_map = _ptr(mp) if mp is not None else None
        d.mgc = len(mp) if mp is not None else 0
    return descs, keep


def plan_audit(levels: Sequence[dict], mesh_variant: int, n_owned=None, order_keys=None) -> str:
    """Host only (no GPU): build the gather plans mgcfd_create would build for `levels` and check every index the kernels
    form from them against the size of what it indexes (mgcfd_plan_audit).  Returns "" when all is in range, else the report."""
    lib = load_library()
    descs, keep = _level_descs(levels)
    owned = None if n_owned is None else (_i64 * len(levels))(*[int(v) for v in n_owned])
    kp = None
    if order_keys is not None:
        keys = [None if k is None else np.ascontiguousarray(k, dtype=np.int64) for k in order_keys]
        keep += keys
        kp = (C.POINTER(_i64) * len(levels))(*[C.cast(_ptr(k), C.POINTER(_i64)) if k is not None else C.POINTER(_i64)() for k in keys])
    buf = C.create_string_buffer(1 << 16)
    rc = lib.mgcfd_plan_audit(descs, len(levels), mesh_variant, owned, kp, buf, len(buf))
    if rc not in (0, 1):
        _check(lib, rc)
    return buf.value.decode()


def load_coefficients(ff17, loads, ref_area: float = 1.0, ref_length: float = 1.0) -> np.ndarray:
    """Host only (mgcfd_load_coefficients): CD CL CS CMx CMy CMz of a loads vector ``[6]`` or history ``[n, 6]`` against the
    far field ``ff17`` (Solver.far_field())."""
    lib = load_library()
    ff = np.ascontiguousarray(ff17, dtype=np.float64).reshape(17)
    rows = np.ascontiguousarray(loads, dtype=np.float64)
    flat = rows.reshape(-1, 6)
    out = np.zeros_like(flat)
    for k in range(len(flat)):
        row = np.ascontiguousarray(flat[k])
        res = np.zeros(6)
        _check(lib, lib.mgcfd_load_coefficients(_ptr(ff), _ptr(row), float(ref_area), float(ref_length), _ptr(res)))
        out[k] = res
    return out.reshape(rows.shape)


WALL_COLUMNS = 7      # MGCFD_WALL_COLUMNS: ax ay az | dp | tx ty tz


def surface_coefficients(ff17, table):
    """Host only: ``(Cp [n], Cf [n, 3])`` of a surface distribution ``table [n, 7]`` (Solver.wall_distribution) against the far
    field ``ff17``: ``Cp = dp / q_inf`` and the tangential friction coefficient ``Cf = (t - (t.n) n) / (|a| q_inf)`` with
    ``n = a / |a|`` and ``q_inf = 0.5 rho |V|^2``."""
    ff = np.asarray(ff17, dtype=np.float64).reshape(17)
    v = ff[1:4] / ff[0]
    q = 0.5 * ff[0] * float(v @ v)
    if not (q > 0.0 and np.isfinite(q)):
        raise ValueError("surface_coefficients: the far field has no positive dynamic pressure")
    tab = np.asarray(table, dtype=np.float64).reshape(-1, WALL_COLUMNS)
    a, dp, t = tab[:, 0:3], tab[:, 3], tab[:, 4:7]
    area = np.sqrt((a * a).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        n = a / area[:, None]
        cf = (t - (t * n).sum(axis=1)[:, None] * n) / (area * q)[:, None]
    return dp / q, cf


WALL_KAPPA = 0.41     # MGCFD_WALL_KAPPA


def wall_yplus(table, h, rho_w, mu_w):
    """Host only: ``y+ [n]`` of the first node off the wall from a surface distribution ``table [n, 7]``
    (Solver.wall_distribution), the wall spacing ``h [n]`` (Solver.wall_spacing) and the wall's density and viscosity (scalars or
    ``[n]``): ``tau = |t - (t.n) n| / |a|`` with ``n = a / |a|`` and ``y+ = h * sqrt(rho_w * tau) / mu_w``."""
    tab = np.asarray(table, dtype=np.float64).reshape(-1, WALL_COLUMNS)
    a, t = tab[:, 0:3], tab[:, 4:7]
    area = np.sqrt((a * a).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        n = a / area[:, None]
        tt = t - (t * n).sum(axis=1)[:, None] * n
        tau = np.sqrt((tt * tt).sum(axis=1)) / area
        return np.asarray(h, dtype=np.float64) * np.sqrt(np.asarray(rho_w, dtype=np.float64) * tau) / np.asarray(mu_w, dtype=np.float64)


def free_stream_constants(mach: float, alpha_deg: float) -> np.ndarray:
    """Host only (mgcfd_free_stream_constants): the 17 far-field doubles (Solver.far_field()) of a free stream at Mach number
    ``mach`` and angle of attack ``alpha_deg`` degrees.  (1.2, 0.0) is the reference's compile-time free stream."""
    lib = load_library()
    out = np.zeros(17)
    _check(lib, lib.mgcfd_free_stream_constants(float(mach), float(alpha_deg), _ptr(out)))
    return out


VISCOUS_PRANDTL, VISCOUS_CFL = 0.72, 0.25         # MGCFD_VISCOUS_PRANDTL, MGCFD_VISCOUS_CFL
VISCOUS_CFL_CORRECTED = 0.2                       # MGCFD_VISCOUS_CFL_CORRECTED
_FACE_GRADIENTS = {"averaged": 0, "corrected": 1}  # MGCFD_FACE_GRADIENT_*
SUTHERLAND_S, SMAGORINSKY_CS, PRANDTL_TURBULENT = 0.3831, 0.17, 0.9     # MGCFD_SUTHERLAND_S, MGCFD_SMAGORINSKY_CS, MGCFD_PRANDTL_TURBULENT
_VISCOSITY_LAWS = {"constant": 0, "sutherland": 1}      # MGCFD_VISCOSITY_*
_EDDY_MODES = {"none": 0, "field": 1, "smagorinsky": 2}   # MGCFD_EDDY_*
_TRANSPORTED_EDDY_MODES = {"spalart-allmaras": 4}         # MGCFD_EDDY_SPALART_ALLMARAS: a model with a transported quantity of its own
_ALL_EDDY_MODES = {**_EDDY_MODES, **_TRANSPORTED_EDDY_MODES}
SA_RATIO = 3.0                                      # MGCFD_SA_RATIO
SA_CDES = 0.65                                      # MGCFD_SA_CDES
_SA_LENGTHS = {"wall": 0, "des": 1, "ddes": 2}      # MGCFD_SA_LENGTH_*
_STATISTICS_MODES = {"off": 0, "volume": 1, "wall": 2}   # MGCFD_STATISTICS_*
WALL_STATISTICS_COLUMNS = 8                         # MGCFD_WALL_STATISTICS_COLUMNS: mean dp tx ty tz | M2 dp tx ty tz


WALL_HEAT_COLUMNS = 3     # MGCFD_WALL_HEAT_COLUMNS: h | T | area
_WALL_MODES = {"adiabatic": 0, "isothermal": 1, "heat-flux": 2}      # MGCFD_WALL_*
_GAMMA = 1.4


def free_stream_temperature(ff17):
    """Host only (mgcfd_free_stream_temperature): ``(t_static, t_total)`` of the far field ``ff17`` in the solver's units,
    ``T = p / rho`` and ``t_total = t_static * (1 + 0.2 M^2)``."""
    lib = load_library()
    ff = np.ascontiguousarray(ff17, dtype=np.float64).reshape(17)
    ts, tt = C.c_double(), C.c_double()
    _check(lib, lib.mgcfd_free_stream_temperature(_ptr(ff), C.byref(ts), C.byref(tt)))
    return ts.value, tt.value


def heat_coefficients(ff17, table, t_wall=None):
    """Host only: ``(qw [n], St [n])`` of a heat table ``table [n, 3]`` (Solver.wall_heat) against the far field ``ff17``: the
    wall heat flux ``qw = h / area`` (positive heats the fluid) and the Stanton number
    ``St = qw / (rho_inf |V_inf| cp (T_total - Tw))`` with ``cp = GAMMA / (GAMMA - 1)`` and ``Tw = t_wall``, or the node's own
    ``T`` where ``t_wall`` is None."""
    ff = np.asarray(ff17, dtype=np.float64).reshape(17)
    v = ff[1:4] / ff[0]
    speed = float(np.sqrt(v @ v))
    _, t_total = free_stream_temperature(ff)
    tab = np.asarray(table, dtype=np.float64).reshape(-1, WALL_HEAT_COLUMNS)
    tw = tab[:, 1] if t_wall is None else np.float64(t_wall)
    with np.errstate(invalid="ignore", divide="ignore"):
        qw = tab[:, 0] / tab[:, 2]
        st = qw / (ff[0] * speed * (_GAMMA / (_GAMMA - 1.0)) * (t_total - tw))
    return qw, st


def viscosity_from_reynolds(ff17, reynolds: float, ref_length: float = 1.0) -> float:
    """Host only (mgcfd_viscosity_from_reynolds): ``mu = rho_inf * |V_inf| * ref_length / reynolds`` for the far field ``ff17``
    (Solver.far_field(), free_stream_constants)."""
    lib = load_library()
    ff = np.ascontiguousarray(ff17, dtype=np.float64).reshape(17)
    mu = C.c_double()
    _check(lib, lib.mgcfd_viscosity_from_reynolds(_ptr(ff), float(reynolds), float(ref_length), C.byref(mu)))
    return mu.value


class Solver:
    """Device-resident solver.  Construct from a :class:`Mesh`, from a generated
    :class:`~mgcfd.meshgen.MultigridMesh`, or from raw per-level arrays."""

    def __init__(self, handle, lib):
        self.handle = handle
        self.lib = lib
        self._keep = None

    # ---- constructors ----
    @classmethod
    def from_mesh(cls, mesh: Mesh, device: int = 0) -> "Solver":
        lib = load_library()
        h = _vp()
        _check(lib, lib.mgcfd_create_from_mesh(mesh.handle, device, C.byref(h)))
        return cls(h, lib)

    @classmethod
    def from_arrays(cls, levels: Sequence[dict], mesh_variant: int, device: int = 0, n_owned=None, order_keys=None) -> "Solver":
        """levels[l] = dict(nel, volumes, coords|None, edges[EDGE_DTYPE], n_internal, n_boundary, n_wall,
        mg_map|None) — the reference's read_grid()/read_mg_connectivity() outputs.  n_owned / order_keys: a partitioned
        level or hierarchy (mgcfd_create_partitioned / _mg)."""
        lib = load_library()
        descs, keep = _level_descs(levels)
        h = _vp()
        if n_owned is None:
            _check(lib, lib.mgcfd_create(descs, len(levels), mesh_variant, device, C.byref(h)))
        elif order_keys is None:
            owned = (_i64 * len(levels))(*[int(v) for v in n_owned])
            _check(lib, lib.mgcfd_create_partitioned(descs, len(levels), mesh_variant, device, owned, C.byref(h)))
        else:
            owned = (_i64 * len(levels))(*[int(v) for v in n_owned])
            keys = [None if k is None else np.ascontiguousarray(k, dtype=np.int64) for k in order_keys]
            keep += keys
            kp = (C.POINTER(_i64) * len(levels))(*[C.cast(_ptr(k), C.POINTER(_i64)) if k is not None else C.POINTER(_i64)() for k in keys])
            _check(lib, lib.mgcfd_create_partitioned_mg(descs, len(levels), mesh_variant, device, owned, kp, C.byref(h)))
        return cls(h, lib)

    @classmethod
    def from_generated(cls, mg: MultigridMesh, device: int = 0) -> "Solver":
        return cls.from_arrays(generated_to_levels(mg), mg.mesh_variant, device)

    # ---- plumbing ----
    def _c(self, rc):
        _check(self.lib, rc)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.mgcfd_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name: str, value: int):
        self._c(self.lib.mgcfd_set_option(self.handle, OPT[name], int(value)))

    def array_devptr(self, l: int, name: str):
        """(device address, element count) of a node array as the library holds it ([ncols][stride] fp64,
        library numbering); see mgcfd_array_devptr."""
        p, n = _vp(), C.c_int64()
        self._c(self.lib.mgcfd_array_devptr(self.handle, l, ARR[name], C.byref(p), C.byref(n)))
        return p.value, n.value

    def accept_restricted(self, fine: int, dev_ptr: int):
        """Take the next-coarser level's restricted variables computed by another solver (one level per rank)."""
        self._c(self.lib.mgcfd_accept_restricted(self.handle, fine, C.c_void_p(dev_ptr)))

    def array_written(self, l: int, name: str):
        self._c(self.lib.mgcfd_array_written(self.handle, l, ARR[name]))

    def invalid_state_location(self):
        """(original cell id, 0-based cycle or -1) of the last invalid state a run reported."""
        cell, cycle = C.c_int64(-1), C.c_int(-1)
        self._c(self.lib.mgcfd_invalid_state_location(self.handle, C.byref(cell), C.byref(cycle)))
        return cell.value, cycle.value

    def tiling(self, l: int) -> dict:
        """How level ``l`` was cut into LDS tiles (mgcfd_level_tiling)."""
        out = (C.c_int64 * 10)()
        self._c(self.lib.mgcfd_level_tiling(self.handle, l, out))
        keys = ("tiles", "halo_nodes", "halo_max", "halo_capacity", "overflow_refs", "row_entries", "padding_entries", "coordinate_boxes",
                "list_entries", "loop_rows")
        return dict(zip(keys, (int(v) for v in out)))

    def has_half_rows(self, l: int) -> bool:
        yes = C.c_int(0)
        self._c(self.lib.mgcfd_level_has_half_rows(self.handle, l, C.byref(yes)))
        return bool(yes.value)

    def has_order_free(self, l: int) -> bool:
        yes = C.c_int(0)
        self._c(self.lib.mgcfd_level_has_order_free(self.handle, l, C.byref(yes)))
        return bool(yes.value)

    def stage_wg4(self, l: int) -> bool:
        """The fused stages of level l run the four-workgroups-per-CU instantiation (MGCFD_OPT_STAGE_WG4)."""
        yes = C.c_int(0)
        self._c(self.lib.mgcfd_level_stage_wg4(self.handle, l, C.byref(yes)))
        return bool(yes.value)

    def get_option(self, name: str) -> int:
        v = C.c_int()
        self._c(self.lib.mgcfd_get_option(self.handle, OPT[name], C.byref(v)))
        return v.value

    def set_stream(self, stream_handle: Optional[int]):
        """Run this solver's work on an existing HIP stream (e.g. torch.cuda.Stream().cuda_stream);
        None restores the solver's own non-blocking stream.  Handle 0 is the legacy default stream,
        which the library cannot share (its own stream does not synchronise with it): refused, so that
        work torch enqueues (collectives, copies) is never silently unordered with the kernels."""
        if stream_handle is not None and int(stream_handle) == 0:
            raise ValueError("stream handle 0 is the legacy default stream; make a torch.cuda.Stream() current "
                             "(torch.cuda.set_stream) and pass its .cuda_stream, or pass None for the solver's own stream")
        self._c(self.lib.mgcfd_set_stream(self.handle, _vp(stream_handle) if stream_handle is not None else None))
        self._stream_handle = int(stream_handle) if stream_handle is not None else None

    def synchronize(self):
        self._c(self.lib.mgcfd_synchronize(self.handle))

    @property
    def num_levels(self) -> int:
        return self.lib.mgcfd_num_levels(self.handle)

    def nel(self, l: int) -> int:
        return self.lib.mgcfd_level_nel(self.handle, l)

    def num_internal_edges(self, l: int) -> int:
        return self.lib.mgcfd_level_num_internal_edges(self.handle, l)

    def far_field(self) -> np.ndarray:
        out = np.zeros(17)
        self._c(self.lib.mgcfd_get_far_field(self.handle, _ptr(out)))
        return out

    # ---- the reference's kernel set ----
    def copy_old_variables(self, l): self._c(self.lib.mgcfd_copy_old_variables(self.handle, l))
    def compute_step_factor(self, l): self._c(self.lib.mgcfd_compute_step_factor(self.handle, l))
    def compute_flux_edge(self, l): self._c(self.lib.mgcfd_compute_flux_edge(self.handle, l))
    def compute_boundary_flux_edge(self, l): self._c(self.lib.mgcfd_compute_boundary_flux_edge(self.handle, l))
    def compute_wall_flux_edge(self, l): self._c(self.lib.mgcfd_compute_wall_flux_edge(self.handle, l))
    def compute_fluxes(self, l): self._c(self.lib.mgcfd_compute_fluxes(self.handle, l))
    def time_step(self, l, j): self._c(self.lib.mgcfd_time_step(self.handle, l, j))
    def zero_fluxes(self, l): self._c(self.lib.mgcfd_zero_fluxes(self.handle, l))
    def indirect_rw(self, l): self._c(self.lib.mgcfd_indirect_rw(self.handle, l))
    def residual(self, l): self._c(self.lib.mgcfd_residual(self.handle, l))
    def restrict(self, fine): self._c(self.lib.mgcfd_restrict(self.handle, fine))
    def prolong(self, fine): self._c(self.lib.mgcfd_prolong(self.handle, fine))

    def calc_rms(self, l) -> float:
        v = C.c_double()
        self._c(self.lib.mgcfd_calc_rms(self.handle, l, C.byref(v)))
        return v.value

    def check_for_invalid_variables(self, l):
        bad = _i64(-1)
        rc = self.lib.mgcfd_check_for_invalid_variables(self.handle, l, C.byref(bad))
        return rc, bad.value

    def pending_invalid_state(self):
        """(code, cell) of what the checks inside the launches issued so far found; does not look at the current state."""
        bad = _i64(-1)
        rc = self.lib.mgcfd_pending_invalid_state(self.handle, C.byref(bad))
        return rc, bad.value

    def smooth(self, l: int, sweeps: int = 1):
        self._c(self.lib.mgcfd_smooth(self.handle, l, sweeps))

    def run_cycles(self, cycles: int, loads: bool = False, ref_point=(0.0, 0.0, 0.0), friction: bool = False, heat: bool = False):
        """The RMS of every cycle; with ``loads=True`` also the level-0 surface loads at the end of every cycle:
        ``(rms, loads[cycles, 6])`` (Fx Fy Fz Mx My Mz about ``ref_point``; mgcfd_run_cycles_loads).  With ``friction=True`` as
        well the rows are twelve wide, the pressure six then the friction six (mgcfd_run_cycles_loads_viscous); with ``heat=True``
        fourteen wide, the heat rate ``Q`` and the wall area ``A`` behind the twelve (mgcfd_run_cycles_loads_heat)."""
        rms = np.zeros(max(cycles, 1))
        if not loads:
            self._c(self.lib.mgcfd_run_cycles(self.handle, cycles, _ptr(rms)))
            return rms[:cycles]
        hist = np.zeros((max(cycles, 1), 14 if heat else 12 if friction else 6))
        ref = np.ascontiguousarray(ref_point, dtype=np.float64).reshape(3)
        call = (self.lib.mgcfd_run_cycles_loads_heat if heat else
                self.lib.mgcfd_run_cycles_loads_viscous if friction else self.lib.mgcfd_run_cycles_loads)
        self._c(call(self.handle, cycles, _ptr(ref), _ptr(rms), _ptr(hist)))
        return rms[:cycles], hist[:cycles]

    def surface_loads(self, level: int, ref_point=(0.0, 0.0, 0.0), friction: bool = False, heat: bool = False) -> np.ndarray:
        """Fx Fy Fz Mx My Mz: the pressure loads on level ``level``'s solid walls in its current state (mgcfd_surface_loads).
        ``friction=True``: twelve numbers, those six and then the friction force and moment (mgcfd_surface_loads_viscous).
        ``heat=True``: fourteen, the twelve and then the heat rate ``Q`` the fluid receives from the wall and the wall's area ``A``
        (mgcfd_surface_loads_heat)."""
        out = np.zeros(14 if heat else 12 if friction else 6)
        ref = np.ascontiguousarray(ref_point, dtype=np.float64).reshape(3)
        call = self.lib.mgcfd_surface_loads_heat if heat else self.lib.mgcfd_surface_loads_viscous if friction else self.lib.mgcfd_surface_loads
        self._c(call(self.handle, level, _ptr(ref), _ptr(out)))
        return out

    def wall_node_count(self, level: int) -> int:
        n = _i64(0)
        self._c(self.lib.mgcfd_wall_node_count(self.handle, level, C.byref(n)))
        return n.value

    def wall_distribution(self, level: int):
        """``(ids [n], table [n, 7])`` of level ``level``'s wall nodes in its current state (mgcfd_wall_distribution): the original
        ids, ascending, and per node ``ax ay az | dp | tx ty tz``.  ``surface_coefficients`` turns the table into Cp and Cf."""
        n = self.wall_node_count(level)
        ids, out = np.zeros(max(n, 1), dtype=np.int64), np.zeros((max(n, 1), WALL_COLUMNS))
        self._c(self.lib.mgcfd_wall_distribution(self.handle, level, _ptr(ids), _ptr(out)))
        return ids[:n], out[:n]

    def wall_heat(self, level: int):
        """``(ids [n], table [n, 3])`` of level ``level``'s wall nodes in its current state (mgcfd_wall_heat): the original ids,
        ascending, and per node ``h | T | area`` — the heat rate the fluid receives through the node's wall faces, ``T = p / rho``
        and the area of those faces.  ``heat_coefficients`` turns the table into the wall heat flux and the Stanton number."""
        n = self.wall_node_count(level)
        ids, out = np.zeros(max(n, 1), dtype=np.int64), np.zeros((max(n, 1), WALL_HEAT_COLUMNS))
        self._c(self.lib.mgcfd_wall_heat(self.handle, level, _ptr(ids), _ptr(out)))
        return ids[:n], out[:n]

    def set_wall_temperature(self, mode="adiabatic", value: float = 0.0):
        """The thermal condition of the no-slip wall (mgcfd_set_wall_temperature): ``"adiabatic"`` (the default), ``"isothermal"``
        with ``value`` the wall temperature in the solver's units (``T = p / rho``) or ``"heat-flux"`` with ``value`` the heat flux
        into the fluid.  Kept like the viscosity model; in effect on the levels ``set_viscous`` covers while its ``wall`` is 1."""
        self._c(self.lib.mgcfd_set_wall_temperature(self.handle, int(_WALL_MODES.get(mode, mode)), float(value)))

    def wall_temperature(self):
        """``(mode, value)`` (mgcfd_get_wall_temperature); the mode by name."""
        m, v = C.c_int(), C.c_double()
        self._c(self.lib.mgcfd_get_wall_temperature(self.handle, C.byref(m), C.byref(v)))
        return {i: k for k, i in _WALL_MODES.items()}[m.value], v.value

    def set_face_gradient(self, mode="corrected"):
        """The face gradient of the viscous and Spalart-Allmaras diffusion (mgcfd_set_face_gradient): ``"averaged"`` (the default:
        the plain average of the two node gradients) or ``"corrected"`` (its along-edge component replaced by the two-point
        difference, which damps the odd-even mode the averaged one cannot see).  Kept like the viscosity model; in effect on the
        levels ``set_viscous`` covers, which must have come with coordinates.  The corrected operator is stiffer: a later
        ``set_viscous`` that names no ``cfl_v`` takes ``VISCOUS_CFL_CORRECTED``.  Captured graphs are dropped.  Not on
        partitioned solvers, group members or ranks."""
        self._c(self.lib.mgcfd_set_face_gradient(self.handle, int(_FACE_GRADIENTS.get(mode, mode))))

    def face_gradient(self) -> str:
        """The mode in use by name (mgcfd_get_face_gradient)."""
        m = C.c_int()
        self._c(self.lib.mgcfd_get_face_gradient(self.handle, C.byref(m)))
        return {v: k for k, v in _FACE_GRADIENTS.items()}[m.value]

    def bench_face_gradient(self, l: int, kind, launches: int) -> float:
        """Mean GPU seconds of one launch of the corrected face gradient's ``"nodes"`` (0) or ``"correction"`` (1) kernel on
        level ``l``, where the mode must be in effect (mgcfd_bench_face_gradient)."""
        t = C.c_double()
        self._c(self.lib.mgcfd_bench_face_gradient(self.handle, l, {"nodes": 0, "correction": 1}.get(kind, kind), launches, C.byref(t)))
        return t.value

    def bench_wall_heat(self, l: int, kind: int, launches: int) -> float:
        """Mean GPU seconds of one launch of ``kind`` (0 the isothermal wall launch, 1 the adiabatic one, 2 the heat-flux launch, 3
        the fourteen-column loads kernel, 4 the heat table's kernel) over ``launches`` back-to-back launches
        (mgcfd_bench_wall_heat); level ``l`` must be viscous with no-slip walls."""
        t = C.c_double()
        self._c(self.lib.mgcfd_bench_wall_heat(self.handle, l, kind, launches, C.byref(t)))
        return t.value

    def wall_stress(self, level: int):
        """Diagnostic: ``(ids [n], Sw [n, 12])``, the wall nodes' stresses of a viscous level's current state (mgcfd_wall_stress)."""
        n = self.wall_node_count(level)
        ids, out = np.zeros(max(n, 1), dtype=np.int64), np.zeros((max(n, 1), 12))
        self._c(self.lib.mgcfd_wall_stress(self.handle, level, _ptr(ids), _ptr(out)))
        return ids[:n], out[:n]

    # ---- wall distance ----
    def compute_wall_distance(self, levels: Optional[int] = None):
        """Levels ``0 .. levels-1`` (None: all) hold the wall distance afterwards (mgcfd_compute_wall_distance): per node the exact
        distance to the nearest wall node of its level, readable as the ``"wall_distance"`` array.  Levels that hold it are not
        computed again.  Needs the levels' coordinates; not on partitioned solvers, group members or ranks."""
        self._c(self.lib.mgcfd_compute_wall_distance(self.handle, self.num_levels if levels is None else int(levels)))

    def wall_distance_levels(self) -> int:
        """How many leading levels hold the wall distance (mgcfd_get_wall_distance)."""
        n = C.c_int()
        self._c(self.lib.mgcfd_get_wall_distance(self.handle, C.byref(n)))
        return n.value

    def release_wall_distance(self):
        """Frees the wall distance on every level (mgcfd_release_wall_distance); refused while the wall damping is in effect."""
        self._c(self.lib.mgcfd_release_wall_distance(self.handle))

    def wall_nearest(self, l: int) -> np.ndarray:
        """``[nel]`` original ids of every node's nearest wall node, the lowest id on a tie, -1 without a wall (mgcfd_wall_nearest)."""
        out = np.zeros(max(self.nel(l), 1), dtype=np.int64)
        self._c(self.lib.mgcfd_wall_nearest(self.handle, l, _ptr(out)))
        return out[:self.nel(l)]

    def wall_spacing(self, l: int):
        """``(ids [n], h [n])``: per wall node, in ``wall_stress``'s order, the smallest positive wall distance among its edge
        neighbours, +0.0 where there is none (mgcfd_wall_spacing).  ``wall_yplus`` turns it into y+."""
        n = self.wall_node_count(l)
        ids, h = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1))
        self._c(self.lib.mgcfd_wall_spacing(self.handle, l, _ptr(ids), _ptr(h)))
        return ids[:n], h[:n]

    def set_wall_damping(self, on: bool = True, kappa: float = WALL_KAPPA):
        """Wall damping of the Smagorinsky model (mgcfd_set_wall_damping): the length scale becomes ``min(cs * delta, kappa * d)``
        with ``d`` the wall distance, so ``mut`` is +0.0 on the wall.  Kept like the viscosity model; in effect on the levels
        ``set_viscous`` covers while ``eddy="smagorinsky"``; the setter that makes it effective computes a missing distance."""
        self._c(self.lib.mgcfd_set_wall_damping(self.handle, int(bool(on)), float(kappa)))

    def wall_damping(self):
        """``(on, kappa)`` (mgcfd_get_wall_damping)."""
        on, k = C.c_int(), C.c_double()
        self._c(self.lib.mgcfd_get_wall_damping(self.handle, C.byref(on), C.byref(k)))
        return bool(on.value), k.value

    def set_sa_free_stream(self, ratio: float = SA_RATIO, reinitialise: bool = False):
        """The free-stream value of the Spalart-Allmaras model (mgcfd_set_sa_free_stream): ``nu_tilde = ratio * mu / rho_inf``, which
        the enabling call and ``set_free_stream(reinitialise=True)`` write on every covered level (+0.0 on the wall);
        ``reinitialise`` writes it now.  Kept while the model is off."""
        self._c(self.lib.mgcfd_set_sa_free_stream(self.handle, float(ratio), int(bool(reinitialise))))

    def sa_free_stream(self) -> float:
        """``ratio`` in use (mgcfd_get_sa_free_stream)."""
        r = C.c_double()
        self._c(self.lib.mgcfd_get_sa_free_stream(self.handle, C.byref(r)))
        return r.value

    def set_sa_unsteady(self, time_accurate: bool = False, length="wall", c_des: float = SA_CDES):
        """The unsteady Spalart-Allmaras model (mgcfd_set_sa_unsteady).  ``time_accurate`` lets the model and ``set_dual_time`` be on
        together: ``nu_tilde`` then takes the BDF source of the physical step, with its time levels in ``"sa_time_n"`` and
        ``"sa_time_n1"`` (``advance`` and ``begin_step`` shift them beside the state's).  ``length``: ``"wall"`` (the wall distance),
        ``"des"`` (DES97: ``min(d, c_des * delta)``) or ``"ddes"`` (delayed DES, shielded by ``fd``); the model length is the
        read-only ``"sa_length"`` on level 0.  Kept while the model or the viscous terms are off."""
        self._c(self.lib.mgcfd_set_sa_unsteady(self.handle, int(bool(time_accurate)), int(_SA_LENGTHS.get(length, length)), float(c_des)))

    def sa_unsteady(self) -> dict:
        """``{"time_accurate", "length", "c_des"}`` in use (mgcfd_get_sa_unsteady)."""
        t, m, c = C.c_int(), C.c_int(), C.c_double()
        self._c(self.lib.mgcfd_get_sa_unsteady(self.handle, C.byref(t), C.byref(m), C.byref(c)))
        return {"time_accurate": bool(t.value), "length": {v: k for k, v in _SA_LENGTHS.items()}[m.value], "c_des": c.value}

    def bench_sa(self, l: int, kind, launches: int) -> float:
        """Mean GPU seconds of one launch of the Spalart-Allmaras model's ``"gradient"`` or ``"transport"`` kernel (level 0) or of
        its ``"restrict"`` kernel into level ``l >= 1`` (mgcfd_bench_sa)."""
        t = C.c_double()
        self._c(self.lib.mgcfd_bench_sa(self.handle, l, {"gradient": 0, "transport": 1, "restrict": 2}.get(kind, kind), launches, C.byref(t)))
        return t.value

    # ---- flow statistics ----
    def set_statistics(self, mode="volume"):
        """The flow statistics of level 0 (mgcfd_set_statistics): ``"off"``, ``"volume"`` (time means of ``rho u v w p mut`` in
        ``"statistics_mean"`` and the co-moments ``uu vv ww uv uw vw pp`` in ``"statistics_moments"``) or ``"wall"`` (those and the
        mean and second moment of ``dp | tx ty tz`` per wall node, ``wall_statistics``).  While a mode is on ``advance`` takes one
        sample with weight ``dt`` after every completed physical step; ``statistics_sample`` takes one by hand."""
        self._c(self.lib.mgcfd_set_statistics(self.handle, int(_STATISTICS_MODES.get(mode, mode))))

    def statistics(self) -> dict:
        """``{"mode", "samples", "wsum"}`` (mgcfd_get_statistics); the mode by name."""
        m, n, w = C.c_int(), _i64(), C.c_double()
        self._c(self.lib.mgcfd_get_statistics(self.handle, C.byref(m), C.byref(n), C.byref(w)))
        return {"mode": {v: k for k, v in _STATISTICS_MODES.items()}[m.value], "samples": n.value, "wsum": w.value}

    def statistics_reset(self):
        """Accumulators, samples and wsum back to zero (mgcfd_statistics_reset)."""
        self._c(self.lib.mgcfd_statistics_reset(self.handle))

    def statistics_sample(self, weight: float):
        """One sample of level 0's current state with ``weight > 0`` (mgcfd_statistics_sample)."""
        self._c(self.lib.mgcfd_statistics_sample(self.handle, float(weight)))

    def statistics_restore(self, samples: int, wsum: float):
        """A restart (mgcfd_statistics_restore): after ``set`` of the two arrays."""
        self._c(self.lib.mgcfd_statistics_restore(self.handle, int(samples), float(wsum)))

    def wall_statistics(self):
        """``(ids [n], table [n, 8])`` of level 0's wall nodes (mgcfd_wall_statistics): the original ids, ascending, and per node
        ``mean dp tx ty tz | M2 dp tx ty tz``; the variances are ``M2 / wsum``."""
        n = self.wall_node_count(0)
        ids, out = np.zeros(max(n, 1), dtype=np.int64), np.zeros((max(n, 1), WALL_STATISTICS_COLUMNS))
        self._c(self.lib.mgcfd_wall_statistics(self.handle, _ptr(ids), _ptr(out)))
        return ids[:n], out[:n]

    def set_wall_statistics(self, table):
        """A restart (mgcfd_set_wall_statistics): ``table [n, 8]`` in ``wall_statistics``' order."""
        n = self.wall_node_count(0)
        t = np.ascontiguousarray(table, dtype=np.float64).reshape(-1, WALL_STATISTICS_COLUMNS)
        if len(t) != n:
            raise ValueError(f"set_wall_statistics: {len(t)} rows for {n} wall nodes")
        if n == 0:
            t = np.zeros((1, WALL_STATISTICS_COLUMNS))
        self._c(self.lib.mgcfd_set_wall_statistics(self.handle, _ptr(t)))

    def flow_statistics(self) -> dict:
        """``{"mean" [nel, 6], "reynolds" [nel, 6], "p_rms" [nel], "k" [nel], "samples", "wsum"}`` of level 0: the means of
        ``rho u v w p mut``, the resolved Reynolds stresses ``uu vv ww uv uw vw``, the rms of the pressure fluctuation and the
        resolved turbulent kinetic energy (mgcfd_statistics_derive on ``"statistics_moments"``)."""
        st = self.statistics()
        mean, mom = self.get(0, "statistics_mean"), np.ascontiguousarray(self.get(0, "statistics_moments"))
        out = np.zeros((len(mom), 8))
        self._c(self.lib.mgcfd_statistics_derive(st["wsum"], _ptr(mom), len(mom), _ptr(out)))
        return {"mean": mean, "reynolds": out[:, :6].copy(), "p_rms": out[:, 6].copy(), "k": out[:, 7].copy(),
                "samples": st["samples"], "wsum": st["wsum"]}

    def bench_statistics(self, kind, launches: int) -> float:
        """Mean GPU seconds of one launch of the ``"volume"`` sample or the ``"wall"`` accumulation (mgcfd_bench_statistics)."""
        t = C.c_double()
        self._c(self.lib.mgcfd_bench_statistics(self.handle, {"volume": 0, "wall": 1}.get(kind, kind), launches, C.byref(t)))
        return t.value

    def bench_wall_distance(self, l: int, launches: int) -> float:
        """Mean GPU seconds of one wall-distance launch on level ``l``, which must hold the distance (mgcfd_bench_wall_distance)."""
        t = C.c_double()
        self._c(self.lib.mgcfd_bench_wall_distance(self.handle, l, launches, C.byref(t)))
        return t.value

    def load_coefficients(self, loads, ref_area: float = 1.0, ref_length: float = 1.0) -> np.ndarray:
        """CD CL CS CMx CMy CMz of one loads vector, or of every row of a ``[n, 6]`` history, against this solver's far field."""
        return load_coefficients(self.far_field(), loads, ref_area, ref_length)

    # ---- free stream ----
    def set_free_stream(self, mach: float, alpha_deg: float, reinitialise: bool = True):
        """Replace the far field (mgcfd_set_free_stream).  ``reinitialise=True``: every level starts again from the new far
        field; ``False``: the state stays (warm start).  Captured graphs are dropped and captured again by the next run."""
        self._c(self.lib.mgcfd_set_free_stream(self.handle, float(mach), float(alpha_deg), 1 if reinitialise else 0))

    def free_stream(self):
        """``(mach, alpha_deg)`` of the far field in use."""
        m, a = C.c_double(), C.c_double()
        self._c(self.lib.mgcfd_get_free_stream(self.handle, C.byref(m), C.byref(a)))
        return m.value, a.value

    # ---- time step ----
    def set_time_step(self, mode="reference", cfl: float = 0.5):
        """Which step-factor formula the sweeps run and its CFL number (mgcfd_set_time_step): ``"reference"`` (what the mesh
        name selects), ``"global"``, ``"local"`` or ``"local_legacy"``.  The state stays; captured graphs are dropped."""
        self._c(self.lib.mgcfd_set_time_step(self.handle, _dt_mode(mode), float(cfl)))

    def time_step_control(self):
        """``(mode, cfl)`` in use, the mode by name."""
        m, c = C.c_int(), C.c_double()
        self._c(self.lib.mgcfd_get_time_step(self.handle, C.byref(m), C.byref(c)))
        return {v: k for k, v in DT_MODE.items()}[m.value], c.value

    # ---- implicit residual smoothing ----
    def set_residual_smoothing(self, eps: float, iterations: int = 2):
        """Every stage's update goes through ``iterations`` Jacobi iterations of implicit residual smoothing with coefficient
        ``eps`` (mgcfd_set_residual_smoothing), which lets the sweeps run at a CFL number two or more times as large;
        ``iterations=0`` switches it off.  The state stays; captured graphs are dropped.  Not on partitioned solvers or ranks."""
        self._c(self.lib.mgcfd_set_residual_smoothing(self.handle, float(eps), int(iterations)))

    def residual_smoothing(self):
        """``(eps, iterations)`` in use; ``(0.0, 0)`` when off."""
        e, m = C.c_double(), C.c_int()
        self._c(self.lib.mgcfd_get_residual_smoothing(self.handle, C.byref(e), C.byref(m)))
        return e.value, m.value

    # ---- dual time stepping ----
    # ---- JST dissipation ----
    def set_jst(self, kappa2: float = 2.5, kappa4: float = 0.15625, levels: int = 1):
        """JST dissipation on levels ``0 .. levels-1`` (mgcfd_set_jst): the first-difference dissipation stays only where the
        pressure sensor sees a shock, a fourth difference scaled by ``kappa4`` takes over elsewhere; both coefficients are in
        units of the reference's dissipation (the defaults are the textbook 1/2 and 1/32).  ``levels=0`` switches it off.  The
        state stays; captured graphs are dropped.  Not on partitioned solvers or ranks."""
        self._c(self.lib.mgcfd_set_jst(self.handle, float(kappa2), float(kappa4), int(levels)))

    def set_upwind(self, levels: int = 1, muscl_levels: Optional[int] = None, limiter="venkatakrishnan", k: float = UPWIND_VENKAT_K,
                   entropy_fix: float = UPWIND_ENTROPY_FIX):
        """Roe's upwind flux on the internal edges of levels ``0 .. levels-1`` (mgcfd_set_upwind), reconstructed with the
        limited Green-Gauss gradient on levels ``0 .. muscl_levels-1`` (None: every upwind level); ``limiter`` is ``"none"``,
        ``"barth-jespersen"`` or ``"venkatakrishnan"`` (with its constant ``k``), ``entropy_fix`` Harten's fraction (0: none).
        ``levels=0`` switches it off.  Excludes the JST dissipation."""
        levels = int(levels)
        muscl = levels if muscl_levels is None else int(muscl_levels)
        self._c(self.lib.mgcfd_set_upwind(self.handle, levels, muscl, int(LIMITERS.get(limiter, limiter)), float(k), float(entropy_fix)))

    def upwind(self):
        """(levels, muscl_levels, limiter by name, k, entropy_fix) in use (mgcfd_get_upwind); (0, 0, "none", 0.0, 0.0) while off."""
        n, m, lim = C.c_int(0), C.c_int(0), C.c_int(0)
        k, fix = C.c_double(0.0), C.c_double(0.0)
        self._c(self.lib.mgcfd_get_upwind(self.handle, C.byref(n), C.byref(m), C.byref(lim), C.byref(k), C.byref(fix)))
        return n.value, m.value, {v: name for name, v in LIMITERS.items()}[lim.value], k.value, fix.value

    def bench_upwind(self, l: int, kind, launches: int) -> float:
        """Mean GPU seconds of ``launches`` back-to-back launches of pass 1 (``kind`` 0 / "gradient", a MUSCL level) or pass 2
        (1 / "flux") on level ``l``, where the upwind flux must be on (mgcfd_bench_upwind)."""
        t = C.c_double(0.0)
        self._c(self.lib.mgcfd_bench_upwind(self.handle, l, {"gradient": 0, "flux": 1}.get(kind, kind), launches, C.byref(t)))
        return t.value

    def jst(self):
        """``(kappa2, kappa4, levels)`` in use, ``levels`` capped at the solver's; ``(0.0, 0.0, 0)`` when off."""
        k2, k4, n = C.c_double(), C.c_double(), C.c_int()
        self._c(self.lib.mgcfd_get_jst(self.handle, C.byref(k2), C.byref(k4), C.byref(n)))
        return k2.value, k4.value, n.value

    # ---- FAS multigrid ----
    def set_fas(self, on: bool = True):
        """FAS multigrid (mgcfd_set_fas): the V-cycle restricts the fine level's residual beside its state, the coarse sweeps
        carry the forcing ``P`` and what is prolonged is the coarse level's correction, so the cycle converges to the fine
        grid's steady state.  Off by default.  The state stays; captured graphs are dropped.  Needs two levels or more; not on
        partitioned solvers or ranks."""
        self._c(self.lib.mgcfd_set_fas(self.handle, 1 if on else 0))

    def fas(self) -> bool:
        on = C.c_int()
        self._c(self.lib.mgcfd_get_fas(self.handle, C.byref(on)))
        return bool(on.value)

    def fas_restrict(self, fine):
        """The down leg from level ``fine``: its total residual, the restricted state, ``fas_start`` and ``fas_forcing`` of
        level ``fine + 1`` (mgcfd_fas_restrict)."""
        self._c(self.lib.mgcfd_fas_restrict(self.handle, fine))

    def fas_prolong(self, fine):
        """The up leg onto level ``fine``: the coarse level's correction, interpolated as ``prolong`` does (mgcfd_fas_prolong)."""
        self._c(self.lib.mgcfd_fas_prolong(self.handle, fine))

    # ---- the multigrid cycle: shape, sweeps per level, cycles from a coarser level, full multigrid ----
    def set_cycle(self, shape="V", pre=None, post=None):
        """The multigrid cycle (mgcfd_set_cycle): ``shape`` "V", "W" or "F" (or its number), ``pre`` / ``post`` the sweeps per
        level before the down leg and after the up leg, one entry per level; None = the defaults (1 everywhere, no post-sweep on
        level 0; the coarsest level's post entry is ignored).  A non-default cycle runs its launches directly."""
        n = self.num_levels
        number = CYCLE_SHAPES.get(shape.upper(), -1) if isinstance(shape, str) else int(shape)

        def counts(v):
            if v is None:
                return None
            v = [int(x) for x in v]
            if len(v) != n:
                raise ValueError(f"set_cycle: {n} entries per list, one per level (got {len(v)})")
            return (C.c_int * n)(*v)
        self._c(self.lib.mgcfd_set_cycle(self.handle, number, counts(pre), counts(post)))

    def get_cycle(self):
        """(shape, pre, post) as mgcfd_get_cycle reports them: the shape's letter and two lists, one entry per level."""
        n = self.num_levels
        shape, pre, post = C.c_int(0), (C.c_int * n)(), (C.c_int * n)()
        self._c(self.lib.mgcfd_get_cycle(self.handle, C.byref(shape), pre, post))
        return "VWF"[shape.value], list(pre), list(post)

    def run_cycles_from(self, top: int, cycles: int) -> np.ndarray:
        """``cycles`` cycles with level ``top`` in level 0's part (mgcfd_run_cycles_from); the levels below it are untouched.
        Returns that level's RMS per cycle."""
        rms = np.zeros(max(cycles, 1))
        self._c(self.lib.mgcfd_run_cycles_from(self.handle, top, cycles, _ptr(rms)))
        return rms[:cycles]

    def prolong_state(self, fine: int):
        """variables[fine] = the interpolated variables[fine + 1] (mgcfd_prolong_state); the fine state is only written."""
        self._c(self.lib.mgcfd_prolong_state(self.handle, fine))

    def full_multigrid(self, cycles) -> np.ndarray:
        """A full-multigrid start (mgcfd_full_multigrid): the state restricted to every level, then from the coarsest level up
        ``cycles[top]`` cycles from level top and its state interpolated onto top - 1.  ``cycles``: one entry per level, the
        first ignored, or one number for all.  Returns the concatenated RMS histories; level-0 cycles are the next call."""
        n = self.num_levels
        c = [int(cycles)] * n if np.isscalar(cycles) else [int(x) for x in cycles]
        if len(c) != n:
            raise ValueError(f"full_multigrid: {n} entries, one per level (got {len(c)})")
        rms = np.zeros(max(sum(max(x, 0) for x in c[1:]), 1))
        self._c(self.lib.mgcfd_full_multigrid(self.handle, (C.c_int * n)(*c), _ptr(rms)))
        return rms[:sum(c[1:])]

    # ---- laminar viscous terms ----
    def set_viscous(self, mu: float, prandtl: float = VISCOUS_PRANDTL, wall: bool = False, cfl_v: Optional[float] = None, levels: int = 1):
        """Laminar viscous terms on levels ``0 .. levels-1`` (mgcfd_set_viscous): the Navier-Stokes stresses and the heat flux at
        constant dynamic viscosity ``mu`` and Prandtl number ``prandtl`` added to every stage's fluxes, the step factors limited
        by ``cfl_v`` times the viscous step, and with ``wall=True`` a no-slip adiabatic condition on the solid walls (momentum
        zero at their nodes).  ``levels=0`` switches them off.  Captured graphs are dropped.  Not on partitioned solvers or ranks.
        ``cfl_v=None`` is ``VISCOUS_CFL``, or ``VISCOUS_CFL_CORRECTED`` while ``face_gradient()`` is ``"corrected"``."""
        if cfl_v is None:
            cfl_v = VISCOUS_CFL_CORRECTED if self.face_gradient() == "corrected" else VISCOUS_CFL
        self._c(self.lib.mgcfd_set_viscous(self.handle, float(mu), float(prandtl), 1 if wall else 0, float(cfl_v), int(levels)))

    def viscous(self):
        """``(mu, prandtl, wall, cfl_v, levels)`` in use, ``levels`` capped at the solver's; ``(0.0, 0.0, False, 0.0, 0)`` when off."""
        mu, pr, cv, w, n = C.c_double(), C.c_double(), C.c_double(), C.c_int(), C.c_int()
        self._c(self.lib.mgcfd_get_viscous(self.handle, C.byref(mu), C.byref(pr), C.byref(w), C.byref(cv), C.byref(n)))
        return mu.value, pr.value, bool(w.value), cv.value, n.value

    def set_viscosity_model(self, law="constant", t_ref: Optional[float] = None, s: float = SUTHERLAND_S, eddy="none",
                            cs: float = SMAGORINSKY_CS, prandtl_t: float = PRANDTL_TURBULENT):
        """The viscosity model of the levels ``set_viscous`` covers (mgcfd_set_viscosity_model).  ``law``: ``"constant"`` or
        ``"sutherland"`` (``mu(T) = mu * (T / t_ref)^1.5 * (1 + s) / (T / t_ref + s)`` with ``T = p / rho``; ``t_ref=None`` takes
        the far field's ``p / rho`` in use now, ``s`` is Sutherland's constant over the reference temperature).  ``eddy``:
        ``"none"``, ``"field"`` (the caller writes the level's ``"eddy_viscosity"`` array) or ``"smagorinsky"`` (constant ``cs``,
        filter width ``cbrt(vol)``, no wall damping; ``"eddy_viscosity"`` is then read-only).  ``prandtl_t`` is the turbulent
        Prandtl number.  ``"spalart-allmaras"`` transports ``nu_tilde`` (the ``"sa_nu_tilde"`` array) on level 0, restricts it to the
        other covered levels and writes ``"eddy_viscosity"``, which is then read-only; ``cs`` is ignored; the wall distance is
        computed where it is missing; refused under dual time stepping.  The defaults switch the model off.  No effect while the viscous terms are off; kept across
        ``set_viscous``.  Captured graphs are dropped.  Not on partitioned solvers, group members or ranks."""
        self._c(self.lib.mgcfd_set_viscosity_model(self.handle, _VISCOSITY_LAWS.get(law, law), 0.0 if t_ref is None else float(t_ref),
                                                   float(s), _ALL_EDDY_MODES.get(eddy, eddy), float(cs), float(prandtl_t)))

    def viscosity_model(self) -> dict:
        """``law``, ``t_ref`` (the value taken), ``s``, ``eddy``, ``cs`` and ``prandtl_t`` in use (mgcfd_get_viscosity_model)."""
        law, eddy = C.c_int(), C.c_int()
        t, s, cs, pt = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        self._c(self.lib.mgcfd_get_viscosity_model(self.handle, C.byref(law), C.byref(t), C.byref(s), C.byref(eddy), C.byref(cs), C.byref(pt)))
        return {"law": {v: k for k, v in _VISCOSITY_LAWS.items()}[law.value], "t_ref": t.value, "s": s.value,
                "eddy": {v: k for k, v in _ALL_EDDY_MODES.items()}[eddy.value], "cs": cs.value, "prandtl_t": pt.value}

    def set_dual_time(self, dt: float, clamp: float = 2.0 / 3.0):
        """Time-accurate runs (mgcfd_set_dual_time): every stage's update carries the BDF source of the physical step ``dt`` and
        the pseudo step is clamped to ``clamp * dt / vol``; ``dt=0`` switches it off and releases the time levels.  The state
        stays; captured graphs are dropped.  Not on partitioned solvers or ranks."""
        self._c(self.lib.mgcfd_set_dual_time(self.handle, float(dt), float(clamp)))

    def dual_time(self) -> dict:
        """``dt`` (0.0 when off), ``clamp``, ``order`` (1 or 2), ``levels`` (time levels held: 0, 1 or 2) and ``invalid_step``
        (the physical step of the last ``advance`` that found an invalid state, or -1)."""
        dt, cl, o, n, bad = C.c_double(), C.c_double(), C.c_int(), C.c_int(), C.c_int()
        self._c(self.lib.mgcfd_get_dual_time(self.handle, C.byref(dt), C.byref(cl), C.byref(o), C.byref(n), C.byref(bad)))
        return {"dt": dt.value, "clamp": cl.value, "order": o.value, "levels": n.value, "invalid_step": bad.value}

    def dual_time_order(self, n: int):
        """1 keeps BDF1 throughout; 2 (the default) runs BDF2 from the second physical step on."""
        self._c(self.lib.mgcfd_dual_time_set_order(self.handle, int(n)))

    def dual_time_reset(self):
        """The next ``begin_step`` starts again: both time levels become the state and BDF1 runs."""
        self._c(self.lib.mgcfd_dual_time_reset(self.handle))

    def begin_step(self):
        """A physical step begins: Wn1 <- Wn, Wn <- variables on every level (mgcfd_dual_time_begin_step)."""
        self._c(self.lib.mgcfd_dual_time_begin_step(self.handle))

    def advance(self, steps: int, cycles_per_step: int, loads: bool = False, ref_point=(0.0, 0.0, 0.0), friction: bool = False,
                heat: bool = False):
        """``steps`` physical steps of ``begin_step`` + ``cycles_per_step`` V-cycles (mgcfd_advance): the RMS of every cycle
        ``[steps, cycles_per_step]``; with ``loads=True`` also the level-0 surface loads at the end of every physical step:
        ``(rms, loads[steps, 6])``.  An invalid state raises MgcfdError with ``.rms``, ``.loads`` (NaN from the failing cycle on)
        and ``.step`` (the physical step it was found in).  ``loads=True, friction=True``: rows of twelve, the pressure six then
        the friction six (mgcfd_advance_loads_viscous); ``loads=True, heat=True``: rows of fourteen, ``Q`` and ``A`` behind them
        (mgcfd_advance_loads_heat)."""
        heat = bool(loads and heat)
        friction = bool(loads and friction)
        rms = np.zeros(max(steps * cycles_per_step, 1))
        out = np.zeros((max(steps, 1), 14 if heat else 12 if friction else 6))
        ref = np.ascontiguousarray(ref_point, dtype=np.float64).reshape(3)
        call = self.lib.mgcfd_advance_loads_heat if heat else self.lib.mgcfd_advance_loads_viscous if friction else self.lib.mgcfd_advance
        rc = call(self.handle, int(steps), int(cycles_per_step), _ptr(rms), _ptr(out) if loads else None, _ptr(ref))
        if rc in (4, 5, 6):
            # an invalid state: the error carries what the call filled (NaN from the failing cycle on) and the physical step
            try:
                self._c(rc)
            except MgcfdError as e:
                e.rms = rms[:steps * cycles_per_step].reshape(steps, cycles_per_step)
                e.loads = out[:steps] if loads else None
                e.step = self.dual_time()["invalid_step"]
                raise
        self._c(rc)
        rms = rms[:steps * cycles_per_step].reshape(steps, cycles_per_step) if cycles_per_step > 0 else rms[:0]
        return (rms, out[:steps]) if loads else rms

    def polar(self, alphas, cycles: int, mach: Optional[float] = None, warm_start: bool = True, ref_point=(0.0, 0.0, 0.0),
              ref_area: float = 1.0, ref_length: float = 1.0, time_step=None, cfl: Optional[float] = None,
              residual_smoothing=None, jst=None, fas: Optional[bool] = None, viscous=None, viscosity_model=None, wall_damping=None,
              wall_temperature=None, face_gradient=None, upwind=None) -> List[dict]:
        """An alpha polar: for every angle of ``alphas`` (degrees) ``set_free_stream`` then ``run_cycles(cycles, loads=True)``.
        The first angle starts from its own far field; a later one continues from the flow of the angle before it
        (``warm_start=True``) or starts again from its far field.  ``mach=None`` keeps the solver's Mach number.  Per angle a
        dict: ``alpha``, ``mach``, ``rms`` [cycles], ``loads`` [cycles, 6] and ``coefficients`` (CD CL CS CMx CMy CMz of the
        last cycle against that angle's far field).  ``time_step`` / ``cfl`` (None: as the solver has them) are set once,
        before the first angle, and stay (``set_time_step``); likewise ``residual_smoothing=(eps, iterations)``
        (``set_residual_smoothing``), ``jst=(kappa2, kappa4, levels)`` (``set_jst``), ``fas=True / False`` (``set_fas``) and
        ``viscous=(mu, prandtl, wall, cfl_v, levels)`` or a dict of ``set_viscous``'s keywords (``set_viscous``) and
        ``viscosity_model=(law, t_ref, s, eddy, cs, prandtl_t)`` or a dict of ``set_viscosity_model``'s keywords; a ``t_ref`` of
        None is then the far field's of the solver as the call finds it; ``wall_damping=(on, kappa)`` or a dict of
        ``set_wall_damping``'s keywords likewise (``set_wall_damping``), and ``wall_temperature=(mode, value)`` or a dict of
        ``set_wall_temperature``'s keywords (``set_wall_temperature``); ``face_gradient="averaged" / "corrected"``
        (``set_face_gradient``) is set before the viscous terms, so that a ``viscous`` without ``cfl_v`` takes the mode's default;
        ``upwind=(levels, muscl_levels, limiter, k, entropy_fix)`` or a dict of ``set_upwind``'s keywords (``set_upwind``)."""
        if face_gradient is not None:
            self.set_face_gradient(face_gradient)
        if wall_temperature is not None:
            self.set_wall_temperature(**wall_temperature) if isinstance(wall_temperature, dict) else self.set_wall_temperature(*wall_temperature)
        if wall_damping is not None:
            self.set_wall_damping(**wall_damping) if isinstance(wall_damping, dict) else self.set_wall_damping(*wall_damping)
        if viscosity_model is not None:
            self.set_viscosity_model(**viscosity_model) if isinstance(viscosity_model, dict) else self.set_viscosity_model(*viscosity_model)
        if viscous is not None:
            self.set_viscous(**viscous) if isinstance(viscous, dict) else self.set_viscous(*viscous)
        if fas is not None:
            self.set_fas(fas)
        if jst is not None:
            self.set_jst(*jst)
        if upwind is not None:
            self.set_upwind(**upwind) if isinstance(upwind, dict) else self.set_upwind(*upwind)
        if residual_smoothing is not None:
            self.set_residual_smoothing(*residual_smoothing)
        if time_step is not None or cfl is not None:
            mode0, cfl0 = self.time_step_control()
            self.set_time_step(mode0 if time_step is None else time_step, cfl0 if cfl is None else cfl)
        m = self.free_stream()[0] if mach is None else float(mach)
        out = []
        for k, a in enumerate(alphas):
            self.set_free_stream(m, float(a), reinitialise=(k == 0 or not warm_start))
            rms, loads = self.run_cycles(cycles, loads=True, ref_point=ref_point)
            coef = self.load_coefficients(loads[-1], ref_area, ref_length) if cycles > 0 else np.full(6, np.nan)
            out.append({"alpha": float(a), "mach": m, "rms": rms, "loads": loads, "coefficients": coef})
        return out

    # ---- state ----
    def get(self, l: int, name: str) -> np.ndarray:
        ncols = NCOLS.get(name, NVAR)
        out = np.zeros(self.nel(l) * ncols)
        self._c(self.lib.mgcfd_get_array(self.handle, l, ARR[name], _ptr(out)))
        return out.reshape(-1, ncols) if ncols > 1 else out

    def set(self, l: int, name: str, values: np.ndarray):
        a = np.ascontiguousarray(values, dtype=np.float64).ravel()
        ncols = NCOLS.get(name, NVAR)
        assert a.size == self.nel(l) * ncols
        self._c(self.lib.mgcfd_set_array(self.handle, l, ARR[name], _ptr(a)))

    def get_edges(self, l: int, n_edges: int) -> np.ndarray:
        out = np.zeros(n_edges, dtype=EDGE_DTYPE)
        self._c(self.lib.mgcfd_get_edges(self.handle, l, _ptr(out)))
        return out

    # ---- monitoring ----
    def loop_iters(self, l: int) -> dict:
        out = np.zeros(len(LOOPS), dtype=np.int64)
        self._c(self.lib.mgcfd_get_loop_iters(self.handle, l, _ptr(out)))
        return dict(zip(LOOPS, out.tolist()))

    def loop_times(self, l: int) -> dict:
        out = np.zeros(len(LOOPS))
        self._c(self.lib.mgcfd_get_loop_times(self.handle, l, _ptr(out)))
        return dict(zip(LOOPS, out.tolist()))

    def reset_monitoring(self):
        self._c(self.lib.mgcfd_reset_monitoring(self.handle))

    def flux_kernel_time(self, l: int):
        t = C.c_double()
        n = _i64()
        self._c(self.lib.mgcfd_get_flux_kernel_time(self.handle, l, C.byref(t), C.byref(n)))
        return t.value, n.value

    def bench_flux(self, l: int, launches: int) -> float:
        t = C.c_double()
        self._c(self.lib.mgcfd_bench_flux(self.handle, l, launches, C.byref(t)))
        return t.value

    def bench_residual_smoothing(self, l: int, kind: int, launches: int) -> float:
        """Mean GPU seconds of one residual-smoothing launch of ``kind`` (0 first, 1 middle, 2 last iteration) over ``launches``
        back-to-back launches under one event pair (mgcfd_bench_residual_smoothing); the smoothing must be on."""
        t = C.c_double()
        self._c(self.lib.mgcfd_bench_residual_smoothing(self.handle, l, kind, launches, C.byref(t)))
        return t.value

    def bench_jst(self, l: int, kind: int, launches: int) -> float:
        """Mean GPU seconds of one JST launch of ``kind`` (0 sensor, 1 dissipation) over ``launches`` back-to-back launches under
        one event pair (mgcfd_bench_jst); the JST dissipation must be on for level ``l``."""
        t = C.c_double()
        self._c(self.lib.mgcfd_bench_jst(self.handle, l, kind, launches, C.byref(t)))
        return t.value

    FAS_LAUNCHES = {"restrict_fas": 0, "forcing": 1, "time_step_fas": 2, "prolong_fas": 3, "restrict": 4, "time_step": 5, "prolong": 6}

    def bench_viscous(self, l: int, kind: int, launches: int) -> float:
        """Mean GPU seconds of one viscous launch of ``kind`` (0 stress, 1 viscous flux, 2 the step limit) over ``launches`` back-to-back launches
        under one event pair (mgcfd_bench_viscous); the viscous terms must be on for level ``l``."""
        t = C.c_double()
        self._c(self.lib.mgcfd_bench_viscous(self.handle, l, kind, launches, C.byref(t)))
        return t.value

    def bench_friction_loads(self, l: int, kind: int, launches: int) -> float:
        """Mean GPU seconds of one launch of ``kind`` (0 the wall-stress kernel, 1 the twelve-column loads kernel, 2 the pressure
        loads kernel) over ``launches`` back-to-back launches (mgcfd_bench_friction_loads); level ``l`` must be viscous."""
        t = C.c_double()
        self._c(self.lib.mgcfd_bench_friction_loads(self.handle, l, kind, launches, C.byref(t)))
        return t.value

    def bench_fas(self, fine: int, kind: str, launches: int) -> float:
        """Mean GPU seconds of one launch of ``kind`` (a key of ``FAS_LAUNCHES``) between levels ``fine`` and ``fine + 1`` over
        ``launches`` back-to-back launches under one event pair (mgcfd_bench_fas); FAS multigrid must be on."""
        t = C.c_double()
        self._c(self.lib.mgcfd_bench_fas(self.handle, fine, self.FAS_LAUNCHES[kind], launches, C.byref(t)))
        return t.value

    def bench_stream_ceiling(self, l: int, launches: int) -> float:
        """Mean seconds per launch of a tile-shaped stream of exactly the flux launch's algorithmic bytes (mgcfd_bench_stream_ceiling)."""
        t = C.c_double(0.0)
        self._c(self.lib.mgcfd_bench_stream_ceiling(self.handle, l, launches, C.byref(t)))
        return t.value

    FAST_MATH = {"rcp": 0, "sqrt": 1, "sqrt_pos": 2}

    def diag_fast_math(self, kind: str, x) -> np.ndarray:
        """The fast mode's own ``1/x`` (``"rcp"``), ``sqrt(x)`` (``"sqrt"``) or ``sqrt(x)`` for ``x > 0`` (``"sqrt_pos"``) of
        every element of ``x``, computed on the device by the code the order-free flux kernel uses (mgcfd_diag_fast_math)."""
        a = np.ascontiguousarray(x, dtype=np.float64).ravel()
        out = np.zeros_like(a)
        self._c(self.lib.mgcfd_diag_fast_math(self.handle, self.FAST_MATH[kind], a.size, _ptr(a), _ptr(out)))
        return out.reshape(np.shape(x))

    def bench_indirect_rw(self, l: int, launches: int) -> float:
        t = C.c_double()
        self._c(self.lib.mgcfd_bench_indirect_rw(self.handle, l, launches, C.byref(t)))
        return t.value

    # ---- halo exchange of a partitioned level ----
    def halo_plan(self, l: int, node_ids) -> int:
        ids = np.ascontiguousarray(node_ids, dtype=np.int64)
        plan = C.c_int(-1)
        self._c(self.lib.mgcfd_halo_plan(self.handle, l, len(ids), _ptr(ids) if len(ids) else None, C.byref(plan)))
        return plan.value

    def halo_pack(self, l: int, plan: int, name: str, dev_ptr: int):
        self._c(self.lib.mgcfd_halo_pack(self.handle, l, plan, ARR[name], _vp(dev_ptr)))

    def halo_unpack(self, l: int, plan: int, name: str, dev_ptr: int):
        self._c(self.lib.mgcfd_halo_unpack(self.handle, l, plan, ARR[name], _vp(dev_ptr)))

    # ---- multi-GPU hooks ----
    def step_factor_local(self, l): self._c(self.lib.mgcfd_step_factor_local(self.handle, l))
    def step_factor_apply(self, l): self._c(self.lib.mgcfd_step_factor_apply(self.handle, l))

    def sweep_begin(self, l): self._c(self.lib.mgcfd_sweep_begin(self.handle, l))
    def sweep_flux0(self, l): self._c(self.lib.mgcfd_sweep_flux0(self.handle, l))
    def sweep_end(self, l): self._c(self.lib.mgcfd_sweep_end(self.handle, l))

    def step_factor_min_devptr(self, l) -> int:
        p = _vp()
        self._c(self.lib.mgcfd_step_factor_min_devptr(self.handle, l, C.byref(p)))
        return p.value

    def step_factor_partials_devptr(self, l):
        p, n = _vp(), C.c_int()
        self._c(self.lib.mgcfd_step_factor_partials_devptr(self.handle, l, C.byref(p), C.byref(n)))
        return p.value, n.value

    def sweep_stage(self, l, j, partials=True): self._c(self.lib.mgcfd_sweep_stage(self.handle, l, j, 1 if partials else 0))
    def sweep_begin_partials(self, l): self._c(self.lib.mgcfd_sweep_begin_partials(self.handle, l))
    def sweep_end_partials(self, l): self._c(self.lib.mgcfd_sweep_end_partials(self.handle, l))

    # ---- a rank of a partitioned level, the sweep loop inside the library (include/mgcfd.h "Multi-GPU in the C++ host") ----
    def rank_set_halo(self, l: int, part):
        """part: mgcfd.partition.LevelPart — its send / recv lists (local ids per peer, ascending global id)."""
        peers = sorted(set(part.send) | set(part.recv))
        n = len(peers)
        keep = [np.ascontiguousarray(part.send.get(p, np.zeros(0, np.int64)), dtype=np.int64) for p in peers] + \
               [np.ascontiguousarray(part.recv.get(p, np.zeros(0, np.int64)), dtype=np.int64) for p in peers]
        pa = (C.c_int * max(n, 1))(*peers)
        sc = (_i64 * max(n, 1))(*[len(a) for a in keep[:n]])
        rc = (_i64 * max(n, 1))(*[len(a) for a in keep[n:]])
        sp = (_vp * max(n, 1))(*[a.ctypes.data for a in keep[:n]])
        rp = (_vp * max(n, 1))(*[a.ctypes.data for a in keep[n:]])
        self._c(self.lib.mgcfd_rank_set_halo(self.handle, l, n, pa, sc, sp, rc, rp))

    def rank_set_wall_slots(self, l: int, part):
        """part: mgcfd.partition.LevelPart — where its solid-wall edges lie in the whole level's solid-wall slice
        (``wall_slots``, ``wall_total``); what the loads over all ranks need (mgcfd_rank_set_wall_slots)."""
        slots = np.ascontiguousarray(part.wall_slots, dtype=np.int64)
        self._c(self.lib.mgcfd_rank_set_wall_slots(self.handle, l, int(part.wall_total), len(slots), _ptr(slots)))

    def rank_halo_info(self, l: int) -> dict:
        out = (_i64 * 4)()
        self._c(self.lib.mgcfd_rank_halo_info(self.handle, l, out))
        return dict(zip(("boundary_tiles", "interior_tiles", "nodes_sent", "nodes_received"), [int(v) for v in out]))

    def rank_graph_status(self, l: int) -> dict:
        """MGCFD_OPT_GRAPH on an RCCL rank: graphs instantiated, whether a capture was refused, sweeps replayed (mgcfd_rank_graph_status)."""
        out = (_i64 * 3)()
        self._c(self.lib.mgcfd_rank_graph_status(self.handle, l, out))
        return {"graphs": int(out[0]), "capture_refused": bool(out[1]), "sweeps_replayed": int(out[2])}

    def rank_info(self) -> dict:
        """What this solver is a rank of, as the library sees it (mgcfd_rank_info)."""
        out = (C.c_int * 4)()
        self._c(self.lib.mgcfd_rank_info(self.handle, out))
        return {"rank": out[0], "ranks": out[1], "transport": ("none", "rccl", "in-process group", "plain (HIP IPC messages)")[out[2]], "rccl_comm_count": out[3]}

    def rank_attach_rccl(self, rank: int, world: int, unique_id: bytes):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._c(self.lib.mgcfd_rank_attach_rccl(self.handle, rank, world, buf))

    def rank_detach(self): self._c(self.lib.mgcfd_rank_detach(self.handle))
    def rank_attach_plain(self, rank: int, world: int): self._c(self.lib.mgcfd_rank_attach_plain(self.handle, rank, world))

    def rank_ipc_export(self, l: int) -> bytes:
        """HIP IPC handles of this rank's state buffers and flag words + its ghost list: for the neighbouring ranks' rank_ipc_attach."""
        n = _i64(0)
        self._c(self.lib.mgcfd_rank_ipc_export_size(self.handle, l, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        self._c(self.lib.mgcfd_rank_ipc_export(self.handle, l, buf))
        return buf.raw

    def rank_ipc_attach(self, l: int, exports):
        """exports: what other ranks exported (any order; the own one is skipped): at least every neighbour's — with every
        rank's the time-step all-reduce goes through the flags as well."""
        keep = [C.create_string_buffer(e, len(e)) for e in exports]
        arr = (_vp * max(len(keep), 1))(*[C.cast(b, _vp) for b in keep])
        self._c(self.lib.mgcfd_rank_ipc_attach(self.handle, l, len(keep), arr))

    def rank_ipc_detach(self, l: int): self._c(self.lib.mgcfd_rank_ipc_detach(self.handle, l))

    def rank_ipc_status(self, l: int) -> int:
        n = C.c_int(0)
        self._c(self.lib.mgcfd_rank_ipc_status(self.handle, l, C.byref(n)))
        return n.value
    def rank_exchange(self, l: int): self._c(self.lib.mgcfd_rank_exchange(self.handle, l))
    def rank_sweeps(self, l: int, sweeps: int = 1): self._c(self.lib.mgcfd_rank_sweeps(self.handle, l, sweeps))

    def rank_cycles(self, cycles: int, rms: bool = True, loads: bool = False, ref_point=(0.0, 0.0, 0.0)):
        """V-cycles of this rank's share of a partitioned hierarchy over RCCL (mgcfd_rank_cycles); the level-0 RMS of each cycle.
        With ``loads=True`` (rank_set_wall_slots on level 0 first) also the whole level's surface loads at the end of every
        cycle: ``(rms, loads[cycles, 6])``, the same rows on every rank (mgcfd_rank_cycles_loads)."""
        out = np.zeros(max(cycles, 1), dtype=np.float64)
        rms_ptr = out.ctypes.data_as(C.POINTER(C.c_double)) if rms else None
        if not loads:
            self._c(self.lib.mgcfd_rank_cycles(self.handle, cycles, rms_ptr))
            return out[:cycles]
        hist = np.zeros((max(cycles, 1), 6))
        ref = np.ascontiguousarray(ref_point, dtype=np.float64).reshape(3)
        self._c(self.lib.mgcfd_rank_cycles_loads(self.handle, cycles, _ptr(ref), _ptr(out) if rms else None, _ptr(hist)))
        return out[:cycles], hist[:cycles]

    def rank_surface_loads(self, level: int, ref_point=(0.0, 0.0, 0.0)) -> np.ndarray:
        """Fx Fy Fz Mx My Mz of the WHOLE level ``level`` from an RCCL rank (collective; mgcfd_rank_surface_loads)."""
        out = np.zeros(6)
        ref = np.ascontiguousarray(ref_point, dtype=np.float64).reshape(3)
        self._c(self.lib.mgcfd_rank_surface_loads(self.handle, level, _ptr(ref), _ptr(out)))
        return out

    def rank_residual_sumsq(self, l: int) -> float:
        v = C.c_double()
        self._c(self.lib.mgcfd_rank_residual_sumsq(self.handle, l, C.byref(v)))
        return v.value

    def residual_sumsq_devptr(self, l) -> int:
        p = _vp()
        self._c(self.lib.mgcfd_residual_sumsq(self.handle, l, C.byref(p)))
        return p.value


def generated_to_levels(mg: MultigridMesh) -> List[dict]:
    """Turn a generated mesh into read_grid()-shaped per-level dicts without touching disk."""
    out = []
    for lvl in mg.levels:
        edges, ni, nb, nw = to_edge_arrays(lvl, mg.mesh_variant)
        out.append({"nel": lvl.nel, "volumes": lvl.volumes, "coords": lvl.coords, "edges": edges,
                    "n_internal": ni, "n_boundary": nb, "n_wall": nw, "mg_map": lvl.mg_map})
    return out


def live_device_resources() -> dict:
    """What the library holds on the devices in this process: allocations, their bytes, handles (streams, events, graph
    executables, opened IPC mappings), as the library counts them itself (mgcfd_live_device_resources)."""
    lib = load_library()
    out = (_i64 * 3)()
    _check(lib, lib.mgcfd_live_device_resources(out))
    return {"allocations": int(out[0]), "bytes": int(out[1]), "handles": int(out[2])}


def rccl_unique_id() -> bytes:
    """ncclGetUniqueId through the library (rank 0 calls it; the launcher hands the 128 bytes to every rank)."""
    lib = load_library()
    buf = C.create_string_buffer(128)
    _check(lib, lib.mgcfd_rccl_unique_id(buf))
    return buf.raw


class Group:
    """The solvers of THIS process as the ranks of one partitioned level (mgcfd_group_*): solvers[r] = rank r."""

    def __init__(self, solvers):
        self.lib = load_library()
        self.solvers = list(solvers)
        arr = (_vp * len(self.solvers))(*[s.handle for s in self.solvers])
        h = _vp()
        _check(self.lib, self.lib.mgcfd_group_create(len(self.solvers), arr, C.byref(h)))
        self.handle = h

    def exchange(self, l: int = 0): _check(self.lib, self.lib.mgcfd_group_exchange(self.handle, l))
    def sweeps(self, l: int = 0, n: int = 1): _check(self.lib, self.lib.mgcfd_group_sweeps(self.handle, l, n))

    def sweeps_rms(self, l: int = 0, n: int = 1) -> np.ndarray:
        """n sweeps, the RMS after each (read back once at the end)."""
        out = np.zeros(max(n, 1), dtype=np.float64)
        _check(self.lib, self.lib.mgcfd_group_sweeps_rms(self.handle, l, n, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out[:n]
    def synchronize(self): _check(self.lib, self.lib.mgcfd_group_synchronize(self.handle))

    def set_free_stream(self, mach: float, alpha_deg: float, reinitialise: bool = True):
        """Solver.set_free_stream on every rank (mgcfd_group_set_free_stream).  The group's sweeps, cycles and loads raise
        MgcfdError (MGCFD_ERR_ARG) while the ranks' far fields differ."""
        _check(self.lib, self.lib.mgcfd_group_set_free_stream(self.handle, float(mach), float(alpha_deg), 1 if reinitialise else 0))

    def set_time_step(self, mode="reference", cfl: float = 0.5):
        """Solver.set_time_step on every rank (mgcfd_group_set_time_step).  The group's sweeps, cycles and loads raise
        MgcfdError (MGCFD_ERR_ARG) while the ranks' mode or CFL number differ."""
        _check(self.lib, self.lib.mgcfd_group_set_time_step(self.handle, _dt_mode(mode), float(cfl)))

    def cycles(self, n: int = 1, rms: bool = True, loads: bool = False, ref_point=(0.0, 0.0, 0.0)):
        """n V-cycles of a partitioned hierarchy (mgcfd_group_cycles); the level-0 RMS of each cycle.  With ``loads=True``
        (Solver.rank_set_wall_slots on level 0 of every rank first) also the whole level's surface loads at the end of every
        cycle: ``(rms, loads[n, 6])`` (mgcfd_group_cycles_loads)."""
        out = np.zeros(max(n, 1), dtype=np.float64)
        rms_ptr = out.ctypes.data_as(C.POINTER(C.c_double)) if rms else None
        if not loads:
            _check(self.lib, self.lib.mgcfd_group_cycles(self.handle, n, rms_ptr))
            return out[:n]
        hist = np.zeros((max(n, 1), 6))
        ref = np.ascontiguousarray(ref_point, dtype=np.float64).reshape(3)
        _check(self.lib, self.lib.mgcfd_group_cycles_loads(self.handle, n, _ptr(ref), _ptr(out) if rms else None, _ptr(hist)))
        return out[:n], hist[:n]

    def surface_loads(self, level: int, ref_point=(0.0, 0.0, 0.0)) -> np.ndarray:
        """Fx Fy Fz Mx My Mz of the WHOLE level ``level`` in the ranks' current state (mgcfd_group_surface_loads)."""
        out = np.zeros(6)
        ref = np.ascontiguousarray(ref_point, dtype=np.float64).reshape(3)
        _check(self.lib, self.lib.mgcfd_group_surface_loads(self.handle, level, _ptr(ref), _ptr(out)))
        return out

    def rms(self, l: int = 0) -> float:
        v = C.c_double()
        _check(self.lib, self.lib.mgcfd_group_rms(self.handle, l, C.byref(v)))
        return v.value

    def close(self):
        if self.handle:
            self.lib.mgcfd_group_destroy(self.handle)
            self.handle = None
