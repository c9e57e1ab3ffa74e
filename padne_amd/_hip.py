"""ctypes binding of ``libpadne_hip.so`` (the C ABI declared in ``include/padne_hip.h``).

The product path has NO CPU fallback: if the shared library is missing, or no
GPU is visible, the first call raises ``HipUnavailableError``.
"""
from __future__ import annotations

import ctypes as C
import weakref
import os
import sys
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpadne_hip.so")

OK = 0
E_INVALID, E_HIP, E_NOMEM, E_NONMANIFOLD, E_NOTCONVERGED, E_COMM, E_BREAKDOWN, E_TOOLARGE, E_NOCOARSEN = \
    -1, -2, -3, -4, -5, -6, -7, -8, -9


class HipUnavailableError(RuntimeError):
    """libpadne_hip.so cannot be loaded or no MI355X is visible."""


class HipError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libpadne_hip error {code}: {message}")
        self.code = code


class NotConvergedError(HipError):
    pass


class SolveOpts(C.Structure):
    _fields_ = [("rtol", C.c_double), ("atol", C.c_double), ("max_iter", C.c_int32),
                ("precond", C.c_int32), ("check_every", C.c_int32), ("flags", C.c_int32)]


class SolveInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("restarts", C.c_int32), ("rel_residual", C.c_double),
                ("abs_residual", C.c_double), ("solve_seconds", C.c_double), ("spmv_seconds", C.c_double),
                ("status", C.c_int32), ("n_rhs", C.c_int32), ("precond_setup_seconds", C.c_double),
                ("operator_complexity", C.c_double), ("levels", C.c_int32), ("precond_fallbacks", C.c_int32)]


_P = C.c_void_p
_I64 = C.c_int64
_PI32 = C.POINTER(C.c_int32)
_PI64 = C.POINTER(C.c_int64)
_PF64 = C.POINTER(C.c_double)

# name -> (restype, argtypes): every symbol include/padne_hip.h declares
SIGNATURES = {
    "padne_abi_version": (C.c_int, []),
    "padne_last_error": (C.c_char_p, []),
    "padne_device_count": (C.c_int, []),
    "padne_ctx_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "padne_ctx_destroy": (C.c_int, [_P]),
    "padne_ctx_synchronize": (C.c_int, [_P]),
    "padne_ctx_stream": (_P, [_P]),
    "padne_comm_unique_id": (C.c_int, [_P]),
    "padne_ctx_comm_init": (C.c_int, [_P, _P, C.c_int, C.c_int]),
    "padne_ctx_comm_rank": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "padne_comm_call_counts": (C.c_int, [C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
    "padne_launch_count": (C.c_int, [C.POINTER(C.c_longlong)]),
    "padne_ctx_comm_init_host": (C.c_int, [_P, C.c_int, C.c_int, _P, _P]),
    "padne_ctx_p2p_export": (C.c_int, [_P, C.c_int32, _P]),
    "padne_ctx_p2p_import": (C.c_int, [_P, _P, C.c_int32]),
    "padne_ctx_p2p_selftest": (C.c_int, [_P, _PI32]),
    "padne_ctx_p2p_close": (C.c_int, [_P]),
    "padne_ctx_set_halo": (C.c_int, [_P, _I64, C.c_int32, C.c_int32, _PI32]),
    "padne_dev_alloc": (C.c_int, [_P, _I64, C.POINTER(_P)]),
    "padne_dev_free": (C.c_int, [_P, _P]),
    "padne_dev_upload": (C.c_int, [_P, _P, _P, _I64]),
    "padne_dev_download": (C.c_int, [_P, _P, _P, _I64]),
    "padne_dev_memset": (C.c_int, [_P, _P, C.c_int, _I64]),
    "padne_csr_from_host": (C.c_int, [_P, _I64, _I64, _PI32, _PI32, _PF64, C.POINTER(_P)]),
    "padne_csr_destroy": (C.c_int, [_P]),
    "padne_csr_shape": (C.c_int, [_P, _PI64, _PI64, _PI64]),
    "padne_csr_to_host": (C.c_int, [_P, _P, _PI32, _PI32, _PF64]),
    "padne_assemble_system": (C.c_int, [_P, _I64, _I64, _PF64, _I64, _PI32, _I64, _PI64, _PI64, _PF64,
                                        _I64, _PI64, _PI64, _PF64, C.POINTER(_P)]),
    "padne_assemble_system_ex": (C.c_int, [_P, _I64, _I64, _PF64, _I64, _PI32, _I64, _PI64, _PI64, _PF64,
                                           _I64, _PI64, _PI64, _PF64, C.c_int32, C.POINTER(_P)]),
    "padne_generate_grid_mesh": (C.c_int, [_P, _I64, _I64, C.c_double, C.c_double, C.c_double, C.c_double,
                                           C.POINTER(C.c_uint64), _P, _P]),
    "padne_csr_reduce": (C.c_int, [_P, _P, _PI32, _I64, C.c_double, C.POINTER(_P)]),
    "padne_csr_relabel": (C.c_int, [_P, _P, _PI32, _I64, _PI32, _I64, C.c_double, C.POINTER(_P)]),
    "padne_csr_vstack": (C.c_int, [_P, _P, _P, C.POINTER(_P)]),
    "padne_spmv": (C.c_int, [_P, _P, _PF64, _PF64]),
    "padne_spmv_dev": (C.c_int, [_P, _P, _P, _P, C.c_int]),
    "padne_spmm8_dev": (C.c_int, [_P, _P, _P, _P, C.c_int]),
    "padne_spmm8_algorithmic_bytes": (_I64, [_P]),
    "padne_spmm8_time": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _PF64]),
    "padne_residual_norm": (C.c_int, [_P, _P, _PF64, _PF64, _PF64]),
    "padne_solve_spd": (C.c_int, [_P, _P, _PF64, _PF64, C.c_int32, C.POINTER(SolveOpts), C.POINTER(SolveInfo)]),
    "padne_solve_spd_dev": (C.c_int, [_P, _P, _P, _P, C.c_int32, C.POINTER(SolveOpts), C.POINTER(SolveInfo)]),
    "padne_kkt_create": (C.c_int, [_P, _P, _I64, _I64, _PI64, _I64, _PI64, _PI64, _PI32, _I64, C.c_int32, C.POINTER(_P)]),
    "padne_kkt_destroy": (C.c_int, [_P]),
    "padne_kkt_matrix": (C.c_int, [_P, C.POINTER(_P)]),
    "padne_kkt_solve": (C.c_int, [_P, _P, _PF64, _I64, _PI64, _PF64, C.c_int32, _PI64, _PI64, _PF64, _I64, _PI64, _PF64,
                                  C.POINTER(SolveOpts), C.c_double, C.POINTER(SolveInfo)]),
    "padne_kkt_finish": (C.c_int, [_P, _P, C.c_int32, _PF64, _I64, _PI64, _PF64, _PF64, _PF64]),
    "padne_kkt_solve_block": (C.c_int, [_P, _P, C.c_int32, _PF64, _I64, _PI64, _PF64, C.c_int32, _PI64, _PI64, _PF64, _I64,
                                        _PI64, _PF64, C.POINTER(SolveOpts), C.c_double, C.POINTER(SolveInfo)]),
    "padne_kkt_finish_block": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _PF64, _I64, _PI64, _PF64, _PF64, _PF64]),
    "padne_kkt_solve_block_coo": (C.c_int, [_P, _P, C.c_int32, _I64, _PI64, _PI32, _PF64, _I64, _PI64, _PF64, C.c_int32, _PI64,
                                            _PI64, _PF64, _I64, _PI64, _PF64, C.POINTER(SolveOpts), C.c_double,
                                            C.POINTER(SolveInfo)]),
    "padne_kkt_solve_block_dev": (C.c_int, [_P, _P, C.c_int32, _P, _I64, _PI64, _PF64, C.c_int32, _PI64, _PI64, _PF64, _I64,
                                            _PI64, _PF64, C.POINTER(SolveOpts), C.c_double, C.POINTER(SolveInfo)]),
    "padne_kkt_power_density_block": (C.c_int, [_P, _P, C.c_int32, _PF64]),
    "padne_kkt_combine_block": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _PI64, _PI32, _PF64, _PF64]),
    "padne_kkt_sensitivity_block": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _PF64, _PF64, _PF64, _PF64]),
    "padne_kkt_current_report": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, _PI32, C.c_int32, _PI32, _PF64, _PF64, _PF64,
                                           _PF64, _PI64, _PF64]),
    "padne_kkt_current_cases": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int32, _PI32, C.c_int32, _PI32, _PF64, _PF64, _PF64,
                                          _PF64, _PI32, _PF64, _PI64, _PF64, _PF64]),
    "padne_kkt_error_estimate": (C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int64, C.c_int32, _PF64, _PF64, _PF64, _PF64, _PF64,
                                           _PI64]),
    "padne_kkt_goal_error": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _PF64, C.c_int64, C.c_int64, C.c_int32, _PF64, _PF64, _PF64, _PF64,
                                       _PF64, _PF64, _PI64, _PF64, _PF64, _PF64, _PF64, _PF64, _PF64, _PI64]),
    "padne_amg_apply": (C.c_int, [_P, _P, _PF64, _PF64]),
    "padne_amg_apply_batch": (C.c_int, [_P, _P, C.c_int32, _PF64, _PF64, _PF64]),
    "padne_csr_set_preconditioner_block": (C.c_int, [_P, _P]),
    "padne_amg_level": (C.c_int, [_P, _P, C.c_int, C.c_int, C.POINTER(_P)]),
    "padne_nearest_vertex": (C.c_int, [_P, _I64, _PF64, _I64, _PF64, _PI64]),
    "padne_nearest_vertex_ties": (C.c_int, [_P, _I64, _PF64, _I64, _PF64, _PI64, _PI32]),
    "padne_power_density": (C.c_int, [_P, _I64, _PF64, _I64, _PI32, _I64, _PI64, _PI64, _PF64, _PF64, _PF64]),
    "padne_csr_power_density": (C.c_int, [_P, _P, _PF64, _PF64]),
    "padne_face_gradient": (C.c_int, [_P, _I64, _PF64, _I64, _PI32, _I64, _PI64, _PI64, _PF64, _PF64, _PF64]),
    "padne_error_estimate": (C.c_int, [_P, _I64, _PF64, _I64, _PI32, _I64, _PI64, _PI64, _PF64, _PF64, _PF64, _PF64, _PF64, _PF64,
                                       _PF64, _PI64]),
    "padne_goal_error": (C.c_int, [_P, _I64, _PF64, _I64, _PI32, _I64, _PI64, _PI64, _PF64, C.c_int32, _PF64, _PF64, _PF64, _PF64, _PF64,
                                   _PF64, _PF64, _PI64, _PF64, _PF64, _PF64, _PF64, _PF64, _PF64, _PI64]),
    "padne_refine_create": (C.c_int, [_P, _I64, _PF64, _I64, _PI32, _I64, _PI64, _PI64, C.POINTER(C.c_uint8), _PI64, _PI64, _PI64,
                                      C.POINTER(_P)]),
    "padne_refine_fetch": (C.c_int, [_P, _P, _PF64, _PI32, _PI32, _PI32]),
    "padne_refine_destroy": (C.c_int, [_P]),
    "padne_polymesh_create": (C.c_int, [_P, _I64, _PI64, _PI64, _PF64, C.c_double, C.c_double, _PI64, _PI64, C.POINTER(_P)]),
    "padne_polymesh_create_graded": (C.c_int, [_P, _I64, _PI64, _PI64, _PF64, C.c_double, C.c_double, _I64, _PI32, _I64, _PF64, _PI64,
                                               _PI64, _PI64, C.POINTER(_P)]),
    "padne_polymesh_fetch": (C.c_int, [_P, _P, _PF64, _PI32, _PI32]),
    "padne_polymesh_arrays": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P)]),
    "padne_polymesh_destroy": (C.c_int, [_P]),
    "padne_polygons_locate": (C.c_int, [_P, _I64, _PI64, _PI64, _PF64, _PI32, _I64, _PF64, _PI32, _PI64, C.POINTER(_P)]),
    "padne_polygons_locate_fetch": (C.c_int, [_P, _P, _PI32, _PI32, _PI32]),
    "padne_polygons_locate_destroy": (C.c_int, [_P]),
    "padne_sampler_create": (C.c_int, [_P, _I64, _PF64, _I64, _PI32, C.c_int32, _PI64, _PI64, _PI32, _PF64, C.c_int32, _PF64, _I64,
                                       C.POINTER(_P)]),
    "padne_sampler_destroy": (C.c_int, [_P]),
    "padne_sampler_points": (C.c_int, [_P, _P, C.c_int32, _I64, _PF64, _PI32, _PF64, _PF64, _PF64]),
    "padne_sampler_raster": (C.c_int, [_P, _P, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, _I64, _I64, _PI32,
                                       _PF64, _PF64, _PF64]),
    "padne_sampler_stats": (C.c_int, [_P, C.c_int32, _PI64, _PF64]),
    "padne_sampler_set_fields": (C.c_int, [_P, _P, C.c_int32, _PF64, _PF64]),
    "padne_sampler_field_points": (C.c_int, [_P, _P, C.c_int32, _I64, _PF64, _PI32, _PF64, _PF64, _PF64, _PI32]),
    "padne_sampler_field_raster": (C.c_int, [_P, _P, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, _I64, _I64, _PI32,
                                             _PF64, _PF64, _PF64, _PI32, _PF64, _PI64]),
    "padne_thermal_create": (C.c_int, [_P, _P, _I64, C.c_int32, _PF64, _PF64, _I64, _PI64, _PI64, _PF64, C.POINTER(_P)]),
    "padne_thermal_destroy": (C.c_int, [_P]),
    "padne_thermal_matrix": (C.c_int, [_P, C.POINTER(_P)]),
    "padne_thermal_lumped": (C.c_int, [_P, _P, _PF64]),
    "padne_thermal_solve": (C.c_int, [_P, _P, C.c_int32, _PF64, _I64, _PI64, _PI32, _PF64, C.POINTER(SolveOpts), _PF64,
                                      C.POINTER(SolveInfo)]),
    "padne_thermal_load": (C.c_int, [_P, _P, C.c_int32, _PF64, _I64, _PI64, _PI32, _PF64, _PF64]),
    "padne_thermal_solve_kkt": (C.c_int, [_P, _P, _P, C.c_int32, _I64, _PI64, _PI32, _PF64, C.POINTER(SolveOpts), _PF64,
                                          C.POINTER(SolveInfo)]),
    "padne_thermal_face_power": (C.c_int, [_P, _P, C.c_int32, _PF64]),
    "padne_thermal_report": (C.c_int, [_P, _P, C.c_int32, _I64, _I64, C.c_int32, _PF64, _PF64, _PI64, _PF64, _PF64, _PF64, _PI32]),
    "padne_thermal_create_stacked": (C.c_int, [_P, _P, _I64, C.c_int32, _PF64, _PF64, _I64, _PI64, _PI64, _PF64, C.c_int32, _PI32,
                                               C.c_int32, _PI32, _PI32, _PF64, C.POINTER(_P)]),
    "padne_thermal_stack_flows": (C.c_int, [_P, _P, C.c_int32, _PF64, _PF64]),
    "padne_thermal_stack_sizes": (C.c_int, [_P, _PI64]),
    "padne_thermal_stack_links": (C.c_int, [_P, _P, _I64, _PI64, _PI32, _PI32, _PF64, _PF64]),
    "padne_thermal_stack_matrix": (C.c_int, [_P, _P, _I64, _PI32, _PI32, _PF64, _PF64]),
    "padne_thermal_set_sources": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _PI32, C.c_int32, _PI32, _PI64, _PF64, _PI64, _PI32,
                                            _PF64]),
    "padne_thermal_source_power": (C.c_int, [_P, _P, C.c_int32, _PF64]),
    "padne_thermal_source_lists": (C.c_int, [_P, _P, C.c_int32, _I64, _PI64, _PI32]),
    "padne_thermal_source_report": (C.c_int, [_P, _P, C.c_int32, _PF64]),
    "padne_thermal_set_film_curves": (C.c_int, [_P, _P, C.c_int32, _PI32, _PF64, _PF64]),
    "padne_thermal_film_terms": (C.c_int, [_P, _P, _PF64, _PF64, _PF64, _PF64, _PI64]),
    "padne_thermal_film_linearise": (C.c_int, [_P, _P, C.c_int32]),
    "padne_thermal_solve_kkt_column": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _I64, _PI64, _PI32, _PF64, C.POINTER(SolveOpts),
                                                 _PF64, C.POINTER(SolveInfo)]),
    "padne_thermal_resolve": (C.c_int, [_P, _P, C.POINTER(SolveOpts), _PF64, C.POINTER(SolveInfo)]),
    "padne_thermal_film_increment": (C.c_int, [_P, _P, _PF64, _PI64, _PI64]),
    "padne_tsens_create": (C.c_int, [_P, _P, _P, C.c_int32, C.c_int32, _PF64, C.POINTER(_P)]),
    "padne_tsens_destroy": (C.c_int, [_P]),
    "padne_tsens_thermal_adjoints": (C.c_int, [_P, _P, C.c_int32, _PI32, _PI32, _PI32, _PF64, _PI64, _PF64, C.c_int32, _PI32, _I64,
                                               _PI64, _PF64, C.POINTER(SolveOpts), C.POINTER(SolveInfo)]),
    "padne_tsens_electrical_rhs": (C.c_int, [_P, _P, C.c_int32, _I64, _PI64, _PI64, _PF64, C.POINTER(_P)]),
    "padne_tsens_faces": (C.c_int, [_P, _P, C.c_int32, _I64, C.c_int32, _PF64, _PF64, _PF64, _PF64, _PF64]),
    "padne_tsens_vertices": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _PF64]),
    "padne_tsens_pairs": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _PF64]),
    "padne_tsens_sources": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _PF64]),
    "padne_transient_create": (C.c_int, [_P, _P, C.c_int32, _PF64, C.POINTER(_P)]),
    "padne_transient_destroy": (C.c_int, [_P]),
    "padne_transient_capacity": (C.c_int, [_P, _P, _PF64]),
    "padne_transient_loads": (C.c_int, [_P, _P, C.c_int32, _PF64, _I64, _PI64, _PI32, _PF64]),
    "padne_transient_loads_kkt": (C.c_int, [_P, _P, _P, C.c_int32, _I64, _PI64, _PI32, _PF64]),
    "padne_transient_load_vectors": (C.c_int, [_P, _P, C.c_int32, _PF64]),
    "padne_transient_start": (C.c_int, [_P, _P, C.c_int32, _PI32, C.POINTER(SolveOpts), C.POINTER(SolveInfo)]),
    "padne_transient_matrix": (C.c_int, [_P, C.c_double, C.POINTER(_P)]),
    "padne_transient_rhs": (C.c_int, [_P, _P, C.c_double, _PI32, _PF64]),
    "padne_transient_run": (C.c_int, [_P, _P, C.c_double, C.c_int32, _PI32, C.c_int32, _PI64, C.POINTER(SolveOpts), _PF64, _PI64,
                                      _PF64, _PF64, _PF64, _PI32, _PF64, _PF64, _PF64, C.POINTER(SolveInfo)]),
    "padne_transient_report": (C.c_int, [_P, _P, _PF64, _PI64, _PF64, _PF64]),
    "padne_transient_state": (C.c_int, [_P, _P, _PF64]),
    "padne_transient_envelope": (C.c_int, [_P, _P, _PF64, _PI32]),
    "padne_transient_clock": (C.c_int, [_P, C.POINTER(_I64), C.POINTER(C.c_double), C.POINTER(_I64)]),
    "padne_transient_try_step": (C.c_int, [_P, _P, C.c_double, _PI32, C.c_int32, C.POINTER(SolveOpts), _PF64, _PI64, _PI32, _PF64,
                                           C.POINTER(SolveInfo)]),
    "padne_transient_accept": (C.c_int, [_P, _P, C.c_int32, _PI64, _PF64, _PI64, _PF64, _PF64, _PF64, _PF64]),
    "padne_transient_trial": (C.c_int, [_P, _P, C.c_int32, _PF64]),
    "padne_periodic_create": (C.c_int, [_P, _P, C.c_int32, C.POINTER(_P)]),
    "padne_periodic_destroy": (C.c_int, [_P]),
    "padne_periodic_mark": (C.c_int, [_P, _P]),
    "padne_periodic_residual": (C.c_int, [_P, _P, _PF64, _PF64, _PI64]),
    "padne_periodic_load": (C.c_int, [_P, _P, C.c_int32]),
    "padne_periodic_push": (C.c_int, [_P, _P, C.c_int32, _PF64]),
    "padne_periodic_predict": (C.c_int, [_P, _P, C.c_int32, _PF64, _PF64, _PI64]),
    "padne_periodic_combine": (C.c_int, [_P, _P, C.c_int32, _PF64]),
    "padne_periodic_vector": (C.c_int, [_P, _P, C.c_int32, _PF64]),
    "padne_periodic_put": (C.c_int, [_P, _P, C.c_int32, _PF64]),
    "padne_coupled_create": (C.c_int, [_P, _P, _P, C.c_int32, _PF64, C.c_double, C.c_double, C.POINTER(_P)]),
    "padne_coupled_destroy": (C.c_int, [_P]),
    "padne_coupled_reset": (C.c_int, [_P, _P]),
    "padne_coupled_set_scale": (C.c_int, [_P, _P, _I64, _PF64]),
    "padne_coupled_get_scale": (C.c_int, [_P, _P, C.c_int32, _I64, _PF64, _PF64]),
    "padne_coupled_revalue": (C.c_int, [_P, _P]),
    "padne_coupled_update": (C.c_int, [_P, _P, _I64, _PF64, _PF64]),
    "padne_coupled_solve_kkt": (C.c_int, [_P, _P, _P, _I64, _PI64, _PI32, _PF64, C.POINTER(SolveOpts), _PF64, C.POINTER(SolveInfo)]),
    "padne_coupled_power_density": (C.c_int, [_P, _P, _P, _PF64]),
    "padne_coupled_set_resistors": (C.c_int, [_P, _P, _I64, _PI64, _PI64, _PF64, _PF64, _PF64]),
    "padne_coupled_get_resistors": (C.c_int, [_P, _P, C.c_int32, _I64, _PF64, _PF64]),
    "padne_transient_reserve_loads": (C.c_int, [_P, _P, C.c_int32]),
    "padne_coupled_transient_load": (C.c_int, [_P, _P, _P, _P, C.c_int32, _I64, _PI64, _PI32, _PF64, C.c_int32, _PF64]),
    "padne_coupled_update_transient": (C.c_int, [_P, _P, _P, C.c_int32, _PF64]),
    "padne_coupled_scale_range": (C.c_int, [_P, _P, _PF64, _PF64]),
    "padne_spmv_algorithmic_bytes": (_I64, [_P]),
    "padne_spmv_time": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _PF64]),
}

# test-only entry points (include/padne_hip_test.h): the in-process team that rehearses several ranks on one GPU
TEST_SIGNATURES = {
    "padne_team_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "padne_team_destroy": (C.c_int, [_P]),
    "padne_team_abort": (C.c_int, [_P]),
    "padne_ctx_join_team": (C.c_int, [_P, _P, C.c_int]),
    "padne_csr_split_tiles": (C.c_int, [_P, C.c_int, _PI64, _PI64]),
    "padne_ctx_lockstep_groups": (C.c_int, [_P, _PI64]),
    "padne_asm_second_path_count": (C.c_int, [_PI64]),
    "padne_ctx_halo_exchange_time": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double)]),
    "padne_ctx_reload_options": (C.c_int, [_P]),
}

# the test probes (include/padne_hip_probe.h): one product launcher of the solver, run once on a test's inputs; one device
# array of a padne_kkt plan, copied out; what a multigrid level decided in its setup, copied out; the gathered operator, one
# halo exchange and one cycle of a row-partitioned hierarchy; the counters of the allocator's guarded mode; one exclusive scan
# and one transpose or sparse product of the multigrid setup on a test's inputs
PROBE_SIGNATURES = {
    "padne_test_product": (C.c_int, [_P, _P, C.c_int32, _I64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P, _P, _P,
                                     _P, _P, _P, _P, C.c_double, _P, _PF64, _I64, _PI32]),
    "padne_test_kkt_state": (C.c_int, [_P, C.c_int32, _P, _I64]),
    "padne_test_amg_state": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, _I64]),
    "padne_test_amg_tail": (C.c_int, [_P, C.POINTER(_P)]),
    "padne_test_halo_exchange": (C.c_int, [_P, C.c_int32, _PF64, _PF64]),
    "padne_test_amg_apply_dist": (C.c_int, [_P, _P, _PF64, _PF64]),
    "padne_test_pool_guard": (C.c_int, [_P, C.c_int32, _P]),
    "padne_test_scan": (C.c_int, [_P, C.c_int32, _I64, _PI32, C.c_int32, C.c_int32, _PI32, _PI64]),
    "padne_test_csr_op": (C.c_int, [_P, C.c_int32, _P, _P, _P, C.POINTER(_P)]),
}

_lib = None


def load_library(path: str | None = None) -> C.CDLL:
    """dlopen the in-tree library and attach prototypes.  Does not touch the GPU."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise HipUnavailableError(
            f"{p} not found: build it with `python -m padne_amd.build` (hipcc --offload-arch=gfx950). "
            "padne_amd has no CPU fallback.")
    # When the process also uses torch (bench.py, torch.distributed ranks) let torch load its
    # HIP runtime first so that both share one libamdhip64.so.7 / librccl.so.1.
    if "torch" in sys.modules:
        pass
    try:
        lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
    except OSError as exc:
        raise HipUnavailableError(f"cannot load {p}: {exc}") from exc
    for name, (res, args) in list(SIGNATURES.items()) + list(TEST_SIGNATURES.items()) + list(PROBE_SIGNATURES.items()):
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.padne_abi_version() != 1:
        raise HipUnavailableError("libpadne_hip.so ABI version mismatch; rebuild it")
    if path is None:
        _lib = lib
    return lib


def _check(rc: int) -> None:
    if rc == OK:
        return
    msg = (load_library().padne_last_error() or b"").decode("utf-8", "replace")
    if rc == E_NONMANIFOLD:
        raise ValueError(msg or "Non-manifold mesh")   # mesh.py:342-343
    if rc == E_INVALID:
        raise ValueError(msg)
    if rc == E_NOMEM:
        raise MemoryError(msg)
    if rc == E_TOOLARGE:
        raise OverflowError(msg)
    if rc == E_NOTCONVERGED:
        raise NotConvergedError(rc, msg)
    raise HipError(rc, msg)


def _f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int32)


def _i64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.int64)


def _ptr(a: np.ndarray, typ):
    return a.ctypes.data_as(typ)


def device_count() -> int:
    n = load_library().padne_device_count()
    return max(n, 0)


def launch_count() -> int:
    """Kernels and asynchronous fills this process has queued through the library so far (all contexts)."""
    n = C.c_longlong(0)
    _check(load_library().padne_launch_count(C.byref(n)))
    return int(n.value)


def asm_second_path_count() -> int:
    """Assemblies of this process that took the two-pass second path of the row kernel (test introspection)."""
    n = C.c_int64(0)
    _check(load_library().padne_asm_second_path_count(C.byref(n)))
    return int(n.value)


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, _P, _P, _P, C.c_int64)      # padne_allgather_fn


_live_contexts = weakref.WeakSet()


def reload_options_everywhere() -> None:
    """Every live context reads the PADNE_* environment switches again (test scaffolding: the library reads them once,
    when a context is created)."""
    for c in list(_live_contexts):
        if getattr(c, "_h", None):
            c.reload_options()


class Context:
    """Device context: GPU, stream, workspaces, optional RCCL communicator."""

    def __init__(self, device: int = 0):
        lib = load_library()
        self._lib = lib
        h = _P()
        rc = lib.padne_ctx_create(int(device), C.byref(h))
        if rc != OK:
            msg = (lib.padne_last_error() or b"").decode()
            raise HipUnavailableError(f"cannot create a context on GPU {device}: {msg}")
        self._h = h
        self.device = int(device)
        self.halo_n_owned = None      # length of b / x when a halo plan is active
        _live_contexts.add(self)

    # -- lifetime ------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.padne_ctx_destroy(self._h)
            self._h = None

    def pool_guard(self, op: int = 0) -> dict:
        """TEST-ONLY (``padne_test_pool_guard``): counters of the allocator's guarded mode, PADNE_POOL_GUARD (op 0), after a
        reset (op 1) or after the mode's self-test (op 2); of this context and its second stream's together."""
        out = np.zeros(8, dtype=np.int64)
        _check(self._lib.padne_test_pool_guard(self._h, int(op), out.ctypes.data_as(_P)))
        side = {0: None, 1: "front", 2: "back"}
        return {"allocations": int(out[0]), "violations": int(out[1]),
                "first": (int(out[2]), side[int(out[3])], int(out[4])), "last": (side[int(out[5])], int(out[6])),
                "fill": int(out[7])}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def synchronize(self):
        _check(self._lib.padne_ctx_synchronize(self._h))

    @property
    def stream(self) -> int:
        return int(self._lib.padne_ctx_stream(self._h) or 0)

    # -- communicator ---------------------------------------------------------
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        _check(self._lib.padne_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world_size: int):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        _check(self._lib.padne_ctx_comm_init(self._h, buf, int(rank), int(world_size)))

    def comm_init_host(self, rank: int, world_size: int, allgather):
        """Collectives through a transport of the caller (gloo, MPI): ``allgather(send: np.ndarray[uint8]) -> bytes-like`` of
        ``world_size * len(send)`` bytes in rank order.  An exception in it fails the collective with PADNE_E_COMM."""
        world_size = int(world_size)

        def cb(_user, send, recv, nbytes):
            try:
                src = np.ctypeslib.as_array(C.cast(send, C.POINTER(C.c_ubyte)), shape=(int(nbytes),)).copy()
                out = np.frombuffer(allgather(src), dtype=np.uint8)
                if out.size != world_size * int(nbytes):
                    return 2
                C.memmove(recv, out.ctypes.data, out.size)
                return 0
            except BaseException:      # noqa: BLE001 -- whatever the transport raises: the collective failed
                return 1
        self._host_allgather = ALLGATHER_FN(cb)             # (kept alive with the context)
        _check(self._lib.padne_ctx_comm_init_host(self._h, int(rank), world_size, C.cast(self._host_allgather, _P), None))

    def p2p_export(self, slots_per_rank: int) -> bytes:
        """This rank's mailbox of the peer-to-peer halo exchange between processes: allocate, return the 64-byte hipIpc handle."""
        buf = C.create_string_buffer(64)
        _check(self._lib.padne_ctx_p2p_export(self._h, int(slots_per_rank), buf))
        return buf.raw

    def p2p_import(self, handles: bytes, world_size: int) -> None:
        buf = C.create_string_buffer(bytes(handles), 64 * int(world_size))
        _check(self._lib.padne_ctx_p2p_import(self._h, buf, int(world_size)))

    def p2p_selftest(self) -> bool:
        """One real exchange of known values through the shared mailboxes (collective): did every rank's stores arrive here?"""
        ok = C.c_int32(0)
        _check(self._lib.padne_ctx_p2p_selftest(self._h, C.byref(ok)))
        return bool(ok.value)

    def p2p_close(self) -> None:
        _check(self._lib.padne_ctx_p2p_close(self._h))

    def comm_call_counts(self):
        """(calls, bytes) of the communication issued so far: all-reduce, all-gather f64, all-gather f32 (the collectives)
        and peer-to-peer halo exchanges."""
        calls = (C.c_longlong * 4)()
        nbytes = (C.c_longlong * 4)()
        _check(self._lib.padne_comm_call_counts(calls, nbytes))
        return list(calls), list(nbytes)

    def reload_options(self) -> None:
        """Read the PADNE_* environment switches again (they are read once, at creation; test scaffolding)."""
        _check(self._lib.padne_ctx_reload_options(self._h))

    def halo_exchange_time(self, repeats: int = 200) -> float:
        """Average device seconds of one halo exchange of this context's plan (collective; test introspection)."""
        t = C.c_double(0.0)
        _check(self._lib.padne_ctx_halo_exchange_time(self._h, int(repeats), C.byref(t)))
        return float(t.value)

    def halo_exchange_probe(self, x, m: int, world: int, as_float: bool = False) -> np.ndarray:
        """TEST-ONLY (``padne_test_halo_exchange``): one exchange of x[n_owned] through this context's halo plan; returns the
        whole vector [n_owned + world * m] as the device holds it afterwards (collective)."""
        x = _f64(x)
        if x.shape != (self.halo_n_owned,):
            raise ValueError("x must hold the owned values")
        out = np.empty(x.shape[0] + int(world) * int(m))
        _check(self._lib.padne_test_halo_exchange(self._h, 1 if as_float else 0, _ptr(x, _PF64), _ptr(out, _PF64)))
        return out

    def lockstep_groups(self) -> int:
        """Groups of right-hand sides this context has advanced in lockstep so far (test introspection)."""
        g = C.c_int64(0)
        _check(self._lib.padne_ctx_lockstep_groups(self._h, C.byref(g)))
        return int(g.value)

    def set_halo(self, n_owned: int, m: int, export_idx) -> None:
        e = _i32(export_idx)
        _check(self._lib.padne_ctx_set_halo(self._h, int(n_owned), int(m), int(e.shape[0]), _ptr(e, _PI32)))
        self.halo_n_owned = int(n_owned)

    def clear_halo(self) -> None:
        _check(self._lib.padne_ctx_set_halo(self._h, -1, 0, 0, None))
        self.halo_n_owned = None

    # -- raw device memory ------------------------------------------------------
    def alloc(self, nbytes: int) -> int:
        p = _P()
        _check(self._lib.padne_dev_alloc(self._h, int(nbytes), C.byref(p)))
        return int(p.value)

    def free(self, dev: int):
        _check(self._lib.padne_dev_free(self._h, _P(dev)))

    def upload(self, dev: int, host: np.ndarray):
        host = np.ascontiguousarray(host)
        _check(self._lib.padne_dev_upload(self._h, _P(dev), host.ctypes.data_as(_P), host.nbytes))

    def download(self, dev: int, shape, dtype=np.float64) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        _check(self._lib.padne_dev_download(self._h, out.ctypes.data_as(_P), _P(dev), out.nbytes))
        return out

    def to_device(self, host: np.ndarray) -> "DeviceArray":
        host = np.ascontiguousarray(host)
        d = DeviceArray(self, host.shape, host.dtype)
        self.upload(d.ptr, host)
        return d

    def empty(self, shape, dtype=np.float64) -> "DeviceArray":
        return DeviceArray(self, shape, dtype)

    # -- matrices -------------------------------------------------------------------
    def csr_from_scipy(self, A) -> "CsrMatrix":
        import scipy.sparse as sp
        A = sp.csr_matrix(A)
        A.sum_duplicates()
        A.sort_indices()
        if A.nnz >= 2**31 - 8192:
            raise ValueError("matrix too large for int32 indices")
        indptr, indices, data = _i32(A.indptr), _i32(A.indices), _f64(A.data)
        h = _P()
        _check(self._lib.padne_csr_from_host(self._h, A.shape[0], A.shape[1], _ptr(indptr, _PI32),
                                             _ptr(indices, _PI32), _ptr(data, _PF64), C.byref(h)))
        return CsrMatrix(self, h)

    def assemble_system(self, n_unknowns, xy, tri, mesh_vertex_offset, mesh_tri_offset, conductance,
                        coo_row, coo_col, coo_val, partial_mesh: bool = False) -> "CsrMatrix":
        """L in the reference layout: cotangent Laplacians of all meshes + lumped stamps.  ``partial_mesh``: the
        triangles are one rank's piece of a partitioned mesh (no manifold test, see padne_assemble_system_ex)."""
        # xy / tri: host arrays, or DeviceArrays (e.g. filled by generate_grid_mesh): then nothing crosses PCIe
        xy_dev = isinstance(xy, DeviceArray)
        tri_dev = isinstance(tri, DeviceArray)
        if xy_dev != tri_dev:
            raise ValueError("xy and tri must both be host arrays or both DeviceArrays")
        if not xy_dev:
            xy = _f64(xy).reshape(-1, 2)
            tri = _i32(tri).reshape(-1, 3)
        elif xy.dtype != np.float64 or tri.dtype != np.int32:
            raise ValueError("device xy must be float64 and device tri int32")
        n_xy = int(np.prod(xy.shape)) // 2
        n_tr = int(np.prod(tri.shape)) // 3
        p_xy = C.cast(_P(xy.ptr), _PF64) if xy_dev else _ptr(xy, _PF64)
        p_tri = C.cast(_P(tri.ptr), _PI32) if tri_dev else _ptr(tri, _PI32)
        mvo, mto, sig = _i64(mesh_vertex_offset), _i64(mesh_tri_offset), _f64(conductance)
        cr, cc, cv = _i64(coo_row), _i64(coo_col), _f64(coo_val)
        n_mesh = sig.shape[0]
        if mvo.shape[0] != n_mesh + 1 or mto.shape[0] != n_mesh + 1:
            raise ValueError("offset tables must have n_mesh+1 entries")
        if not (cr.shape == cc.shape == cv.shape):
            raise ValueError("coo arrays must have equal length")
        h = _P()
        _check(self._lib.padne_assemble_system_ex(
            self._h, int(n_unknowns), n_xy, p_xy, n_tr, p_tri, n_mesh,
            _ptr(mvo, _PI64), _ptr(mto, _PI64), _ptr(sig, _PF64), cr.shape[0], _ptr(cr, _PI64),
            _ptr(cc, _PI64), _ptr(cv, _PF64), 1 if partial_mesh else 0, C.byref(h)))
        return CsrMatrix(self, h)

    def generate_grid_mesh(self, nx: int, ny: int, h: float, seed: int = 0, jitter: float = 0.2, origin=(0.0, 0.0),
                           xy_out: "DeviceArray | None" = None, tri_out: "DeviceArray | None" = None,
                           vertex_offset: int = 0, tri_offset: int = 0):
        """``synthetic.jittered_grid(nx, ny, h, seed, jitter, origin)`` generated on the device, bit for bit (the jitter is
        numpy's ``default_rng(seed)`` stream, evaluated per vertex by jump-ahead).  Returns (xy, tri) DeviceArrays; with
        ``xy_out`` / ``tri_out`` the mesh is written at ``vertex_offset`` / ``tri_offset`` of existing arrays."""
        n_v, n_t = nx * ny, 2 * (nx - 1) * (ny - 1)
        xy = xy_out if xy_out is not None else DeviceArray(self, (n_v, 2), np.float64)
        tri = tri_out if tri_out is not None else DeviceArray(self, (n_t, 3), np.int32)
        st = np.random.default_rng(seed).bit_generator.state["state"]
        g = (C.c_uint64 * 4)(st["state"] >> 64, st["state"] & (2 ** 64 - 1), st["inc"] >> 64, st["inc"] & (2 ** 64 - 1))
        _check(self._lib.padne_generate_grid_mesh(self._h, int(nx), int(ny), float(h), float(jitter), float(origin[0]),
                                                  float(origin[1]), g, _P(xy.ptr + 16 * int(vertex_offset)),
                                                  _P(tri.ptr + 12 * int(tri_offset))))
        return xy, tri

    def nearest_vertex(self, points: np.ndarray, queries: np.ndarray, with_ties: bool = False):
        """Index of the nearest of ``points`` (n, 2) for every row of ``queries`` (m, 2); ties to the smallest index.
        ``with_ties``: also the number of points at exactly the minimum distance, per query."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
        q = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 2)
        out = np.empty(len(q), dtype=np.int64)
        ties = np.ones(len(q), dtype=np.int32)
        if len(q):
            _check(self._lib.padne_nearest_vertex_ties(self._h, len(pts), _ptr(pts, _PF64), len(q), _ptr(q, _PF64),
                                                       _ptr(out, _PI64), _ptr(ties, _PI32)))
        return (out, ties) if with_ties else out

    def power_density(self, xy, tri, mesh_vertex_offset, mesh_tri_offset, conductance, potential) -> np.ndarray:
        # xy / tri: host arrays, or DeviceArrays (e.g. filled by generate_grid_mesh): then nothing crosses PCIe
        xy_dev = isinstance(xy, DeviceArray)
        tri_dev = isinstance(tri, DeviceArray)
        if xy_dev != tri_dev:
            raise ValueError("xy and tri must both be host arrays or both DeviceArrays")
        if not xy_dev:
            xy = _f64(xy).reshape(-1, 2)
            tri = _i32(tri).reshape(-1, 3)
        elif xy.dtype != np.float64 or tri.dtype != np.int32:
            raise ValueError("device xy must be float64 and device tri int32")
        n_xy = int(np.prod(xy.shape)) // 2
        n_tr = int(np.prod(tri.shape)) // 3
        p_xy = C.cast(_P(xy.ptr), _PF64) if xy_dev else _ptr(xy, _PF64)
        p_tri = C.cast(_P(tri.ptr), _PI32) if tri_dev else _ptr(tri, _PI32)
        mvo, mto, sig = _i64(mesh_vertex_offset), _i64(mesh_tri_offset), _f64(conductance)
        pot = _f64(potential)
        if pot.shape[0] < xy.shape[0]:
            raise ValueError("potential vector shorter than the vertex count")
        out = np.zeros(tri.shape[0], dtype=np.float64)
        _check(self._lib.padne_power_density(self._h, xy.shape[0], _ptr(xy, _PF64), tri.shape[0],
                                             _ptr(tri, _PI32), sig.shape[0], _ptr(mvo, _PI64), _ptr(mto, _PI64),
                                             _ptr(sig, _PF64), _ptr(pot, _PF64), _ptr(out, _PF64)))
        return out


    def face_gradient(self, xy, tri, mesh_vertex_offset, mesh_tri_offset, potential):
        xy = _f64(xy).reshape(-1, 2)
        tri = _i32(tri).reshape(-1, 3)
        mvo, mto, pot = _i64(mesh_vertex_offset), _i64(mesh_tri_offset), _f64(potential)
        gx = np.zeros(tri.shape[0], dtype=np.float64)
        gy = np.zeros(tri.shape[0], dtype=np.float64)
        _check(self._lib.padne_face_gradient(self._h, xy.shape[0], _ptr(xy, _PF64), tri.shape[0], _ptr(tri, _PI32),
                                             mvo.shape[0] - 1, _ptr(mvo, _PI64), _ptr(mto, _PI64), _ptr(pot, _PF64),
                                             _ptr(gx, _PF64), _ptr(gy, _PF64)))
        return gx, gy

    def error_estimate(self, xy, tri, mesh_vertex_offset, mesh_tri_offset, conductance, potential):
        """The gradient-recovery error estimate (include/padne_hip.h, ``padne_error_estimate``) of ``potential`` on meshes
        given as ``power_density`` takes them: (G (n_vert, 2), eta (n_tri,), and per mesh sum eta^2, sum sigma A |g|^2, the
        largest eta and its face as a global index, -1 for a mesh without faces)."""
        xy = _f64(xy).reshape(-1, 2)
        tri = _i32(tri).reshape(-1, 3)
        mvo, mto, sig, pot = _i64(mesh_vertex_offset), _i64(mesh_tri_offset), _f64(conductance), _f64(potential)
        n_mesh = sig.shape[0]
        if mvo.shape[0] != n_mesh + 1 or mto.shape[0] != n_mesh + 1:
            raise ValueError("the offset tables must have one entry more than there are meshes")
        if pot.shape[0] < xy.shape[0]:
            raise ValueError("potential vector shorter than the vertex count")
        G = np.empty((xy.shape[0], 2), dtype=np.float64)
        eta = np.empty(tri.shape[0], dtype=np.float64)
        mesh_error, mesh_power, mesh_max = (np.empty(n_mesh, dtype=np.float64) for _ in range(3))
        mesh_face = np.empty(n_mesh, dtype=np.int64)
        _check(self._lib.padne_error_estimate(self._h, xy.shape[0], _ptr(xy, _PF64), tri.shape[0], _ptr(tri, _PI32), n_mesh,
                                              _ptr(mvo, _PI64), _ptr(mto, _PI64), _ptr(sig, _PF64), _ptr(pot, _PF64),
                                              _ptr(G, _PF64), _ptr(eta, _PF64), _ptr(mesh_error, _PF64), _ptr(mesh_power, _PF64),
                                              _ptr(mesh_max, _PF64), _ptr(mesh_face, _PI64)))
        return G, eta, mesh_error, mesh_power, mesh_max, mesh_face

    def goal_error(self, xy, tri, mesh_vertex_offset, mesh_tri_offset, conductance, fields):
        """The goal-oriented error estimate (include/padne_hip.h, ``padne_goal_error``) of ``fields`` (n_fields, n_vert),
        n_fields >= 2, on meshes given as ``error_estimate`` takes them: field 0 is paired with each of the others.  Returns
        (the power density of field 0 (n_tri,), the bits of ``power_density``; ``error_estimate``'s six results for field 0,
        bit for bit; then per other field j: eta (n_obj, n_tri), delta
        (n_obj, n_tri), omega (n_obj, n_tri), and per mesh the sums of omega and of delta (n_obj, n_mesh), the largest omega
        and its face as a global index, -1 for a mesh without faces)."""
        xy = _f64(xy).reshape(-1, 2)
        tri = _i32(tri).reshape(-1, 3)
        mvo, mto, sig = _i64(mesh_vertex_offset), _i64(mesh_tri_offset), _f64(conductance)
        F = _f64(fields)
        n_mesh, n_vert, n_tri = sig.shape[0], xy.shape[0], tri.shape[0]
        if mvo.shape[0] != n_mesh + 1 or mto.shape[0] != n_mesh + 1:
            raise ValueError("the offset tables must have one entry more than there are meshes")
        if F.ndim != 2 or F.shape[0] < 2:
            raise ValueError("fields must have shape (n_fields, n_vert) with n_fields >= 2")
        if F.shape[1] < n_vert:
            raise ValueError("potential vectors shorter than the vertex count")
        pot = np.ascontiguousarray(F[:, :n_vert].T)                      # (n_vert, n_fields): one row per vertex
        n_obj = F.shape[0] - 1
        G = np.empty((n_vert, 2), dtype=np.float64)
        power, eta = np.empty(n_tri, dtype=np.float64), np.empty(n_tri, dtype=np.float64)
        mesh_error, mesh_power, mesh_max = (np.empty(n_mesh, dtype=np.float64) for _ in range(3))
        mesh_face = np.empty(n_mesh, dtype=np.int64)
        dual, delta, omega = (np.empty((n_obj, n_tri), dtype=np.float64) for _ in range(3))
        m_omega, m_delta, m_top = (np.empty((n_obj, n_mesh), dtype=np.float64) for _ in range(3))
        m_face = np.empty((n_obj, n_mesh), dtype=np.int64)
        _check(self._lib.padne_goal_error(self._h, n_vert, _ptr(xy, _PF64), n_tri, _ptr(tri, _PI32), n_mesh, _ptr(mvo, _PI64),
                                          _ptr(mto, _PI64), _ptr(sig, _PF64), F.shape[0], _ptr(pot, _PF64), _ptr(power, _PF64), _ptr(G, _PF64),
                                          _ptr(eta, _PF64), _ptr(mesh_error, _PF64), _ptr(mesh_power, _PF64), _ptr(mesh_max, _PF64),
                                          _ptr(mesh_face, _PI64), _ptr(dual, _PF64), _ptr(delta, _PF64), _ptr(omega, _PF64),
                                          _ptr(m_omega, _PF64), _ptr(m_delta, _PF64), _ptr(m_top, _PF64), _ptr(m_face, _PI64)))
        return power, (G, eta, mesh_error, mesh_power, mesh_max, mesh_face), dual, delta, omega, m_omega, m_delta, m_top, m_face


class LocalTeam:
    """In-process team of contexts acting as ranks on one GPU (rehearsal of the multi-rank path)."""

    def __init__(self, world_size: int):
        lib = load_library()
        self._lib = lib
        h = _P()
        _check(lib.padne_team_create(int(world_size), C.byref(h)))
        self._h = h
        self.world = int(world_size)

    def join(self, ctx: "Context", rank: int) -> None:
        _check(self._lib.padne_ctx_join_team(ctx._h, self._h, int(rank)))
        ctx._team = self       # keep the team alive as long as its members

    def abort(self) -> None:
        """Wake every rank that waits in a collective; all team collectives return E_COMM from now on."""
        if getattr(self, "_h", None):
            self._lib.padne_team_abort(self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.padne_team_destroy(self._h)
            self._h = None


class DeviceArray:
    """A flat device allocation with numpy-like shape/dtype metadata."""

    def __init__(self, ctx: Context, shape, dtype=np.float64):
        self.ctx = ctx
        self.shape = tuple(np.atleast_1d(shape)) if not isinstance(shape, tuple) else shape
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = ctx.alloc(max(self.nbytes, 8))

    def numpy(self) -> np.ndarray:
        return self.ctx.download(self.ptr, self.shape, self.dtype)

    def set(self, host: np.ndarray):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        if host.nbytes != self.nbytes:
            raise ValueError("size mismatch")
        self.ctx.upload(self.ptr, host)

    def free(self):
        if self.ptr:
            self.ctx.free(self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            if self.ptr and self.ctx._h:
                self.free()
        except Exception:
            pass


@dataclass
class SolveResult:
    x: np.ndarray | None
    iterations: int
    restarts: int
    rel_residual: float
    abs_residual: float
    seconds: float
    status: int
    spmv_seconds: float = 0.0
    setup_seconds: float = 0.0
    operator_complexity: float = 0.0
    levels: int = 0
    precond_fallbacks: int = 0      # right-hand sides redone with the Jacobi preconditioner after a multigrid failure


def _prefaulted(shape):
    """A result array of ``shape`` whose pages threads touch while the device works: (array, threads), or (None, None) when
    it is too small to matter.  A fresh 80 MB array at 10 M unknowns is 20 000 page faults in the path of the copy that
    brings it home; one thread per 80 MB, up to 8."""
    if int(np.prod(shape)) < (1 << 18):
        return None, None
    import threading
    arr = np.empty(shape, dtype=np.float64)
    flat = arr.reshape(-1)
    parts = np.array_split(flat, min(8, -(-flat.nbytes // (80 << 20))))
    # (the threads hold the array itself, not just its address: it outlives a plan that is dropped on an error path)
    threads = [threading.Thread(target=lambda a=a: C.memset(a.ctypes.data, 0, a.nbytes), daemon=True) for a in parts]
    for t in threads:
        t.start()
    return arr, threads


class KktPlan:
    """``padne_kkt``: the reduction of one assembled KKT system to its SPD core, resident on the device (index map,
    reduced matrix with its multigrid hierarchy, the N-vectors).  ``solve`` + ``finish`` are the two device stages of
    ``solver.solve_system``; the multiplier recovery between them is O(#constraints) host work."""

    def __init__(self, L: "CsrMatrix", n_potential: int, elim, tied, n_free: int, index_map=None, strip_order: bool = False):
        self.ctx, self.L = L.ctx, L
        elim = _i64(elim)
        tm = _i64([m for m, _ in tied])
        tr = _i64([r for _, r in tied])
        imap = None if index_map is None else _i32(index_map)
        if imap is not None and imap.shape[0] != L.shape[0]:
            raise ValueError("index map length must equal the matrix dimension")
        h = _P()
        _check(self.ctx._lib.padne_kkt_create(self.ctx._h, L._h, int(n_potential), elim.shape[0], _ptr(elim, _PI64), tm.shape[0],
                                              _ptr(tm, _PI64), _ptr(tr, _PI64), None if imap is None else _ptr(imap, _PI32),
                                              int(n_free), 1 if strip_order else 0, C.byref(h)))
        self._h = h
        self.n_free = int(n_free)
        self.N = L.shape[0]

    def close(self):
        if getattr(self, "_h", None) and self.ctx._h:
            self.ctx._lib.padne_kkt_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reduced_matrix(self) -> "CsrMatrix":
        """Borrowed view of A = -P^T L P (valid while the plan lives)."""
        h = _P()
        _check(self.ctx._lib.padne_kkt_matrix(self._h, C.byref(h)))
        m = CsrMatrix(self.ctx, h)
        m._borrowed = True
        return m

    STATE = {"IMAP": (0, np.int32), "SRC_OF": (1, np.int32), "B": (2, np.float64), "Y": (3, np.float64), "C": (4, np.float64),
             "V": (5, np.float64), "Z": (6, np.float64)}

    def state(self, which: str, n: int) -> np.ndarray:
        """TEST-ONLY (``padne_test_kkt_state``): the ``n`` elements of the plan's device array ``which`` as they lie there.
        ValueError when the array has another size or does not exist yet."""
        sel, dtype = self.STATE[which]
        out = np.empty(int(n), dtype=dtype)
        _check(self.ctx._lib.padne_test_kkt_state(self._h, sel, out.ctypes.data_as(_P), out.nbytes))
        return out

    def solve(self, r, known: dict, extras: list, probes, *, rtol=1e-12, max_iter=200000, precond="amg",
              abs_residual_target=0.0, rebuild=False):
        """Stage 1.  ``known`` {unknown: c}; ``extras``: list of {row: value} columns; ``probes``: unknowns whose residual
        rows come back.  Returns (probe values [(1 + len(extras)), len(probes)], SolveResult)."""
        r = _f64(r)
        if r.ndim != 1 or r.shape[0] != self.N:
            raise ValueError("right-hand side has the wrong length")
        kidx = _i64(sorted(known))
        kval = _f64([known[int(i)] for i in kidx])
        return self._stage1(None, r, kidx, kval, extras, probes, rtol, max_iter, precond, abs_residual_target, rebuild)

    def solve_block(self, R, known_idx, known_val, extras: list, probes, *, rtol=1e-12, max_iter=200000, precond="amg",
                    abs_residual_target=0.0, rebuild=False):
        """Stage 1 for a block ``R`` (N, k) of right-hand sides, uploaded in its row-major layout (a Fortran-ordered block
        is copied once).  ``known_idx`` [n_known] with ``known_val`` (k, n_known); the ``extras`` are solved once for the
        block.  Returns (probe values [(k + len(extras)), len(probes)], SolveResult summed over all reduced solves)."""
        R = _f64(R)
        if R.ndim != 2 or R.shape[0] != self.N or R.shape[1] < 1:
            raise ValueError("the block of right-hand sides must have shape (N, k) with k >= 1")
        kidx = _i64(known_idx)
        kval = _f64(known_val).reshape(R.shape[1], kidx.shape[0])
        return self._stage1(R.shape[1], R, kidx, kval, extras, probes, rtol, max_iter, precond, abs_residual_target, rebuild)

    def solve_block_coo(self, n_cols, rows, cols, vals, known_idx, known_val, extras: list, probes, *, rtol=1e-12,
                        max_iter=200000, precond="amg", abs_residual_target=0.0, rebuild=False, power_tri: int = 0,
                        power_rows: int = 0, current_tri: int = 0, current_cols: int = 1):
        """``solve_block`` with the block (N, n_cols) given by its non-zero entries: R[rows[e], cols[e]] = vals[e], each (row,
        column) pair at most once.  Only the triples cross PCIe; the device zeroes its block and scatters them.
        ``power_tri``: the triangles of the mesh the system carries, when ``power_density_block`` will follow -- its result
        array is then made ready while the device solves, like V's (``power_rows`` rows of it instead of n_cols: 1 + the
        objectives of a ``sensitivity_block``).  ``current_tri``: the same for the J and |J| arrays of a ``current_report``, or,
        with ``current_cols`` = the columns whose fields a ``current_cases`` will bring home, for those."""
        rows, cols, vals = _i64(rows).reshape(-1), _i32(cols).reshape(-1), _f64(vals).reshape(-1)
        if not (rows.shape == cols.shape == vals.shape):
            raise ValueError("rows, cols and vals must have equal length")
        n_cols = int(n_cols)
        if n_cols < 1:
            raise ValueError("a block has at least one column")
        kidx = _i64(known_idx)
        kval = _f64(known_val).reshape(n_cols, kidx.shape[0])
        return self._stage1(n_cols, (rows, cols, vals), kidx, kval, extras, probes, rtol, max_iter, precond,
                            abs_residual_target, rebuild, power_tri=int(power_tri), power_rows=int(power_rows),
                            current_tri=int(current_tri), current_cols=int(current_cols))

    def solve_block_dev(self, n_cols, r_dev, known_idx, known_val, extras: list, probes, *, rtol=1e-12, max_iter=200000,
                        precond="amg", abs_residual_target=0.0, rebuild=False):
        """``solve_block`` with the block (N, n_cols), row-major, already on the device: ``r_dev`` is its address (an int, or a
        :class:`DeviceArray`).  One device copy takes the place of the upload; the results have the bits of ``solve_block``
        on the same block."""
        n_cols = int(n_cols)
        if n_cols < 1:
            raise ValueError("a block has at least one column")
        if isinstance(r_dev, DeviceArray):
            if int(np.prod(r_dev.shape)) != self.N * n_cols:
                raise ValueError("the device block must hold N * n_cols doubles")
            r_dev = r_dev.ptr
        if not r_dev:
            raise ValueError("the device block is a null pointer")
        kidx = _i64(known_idx)
        kval = _f64(known_val).reshape(n_cols, kidx.shape[0])
        return self._stage1(n_cols, int(r_dev), kidx, kval, extras, probes, rtol, max_iter, precond, abs_residual_target, rebuild)

    def _stage1(self, n_cols, r, kidx, kval, extras, probes, rtol, max_iter, precond, abs_residual_target, rebuild,
                power_tri=0, power_rows=0, current_tri=0, current_cols=1):
        ptr, rows, vals = [0], [], []
        for col in extras:
            for row, val in col.items():
                rows.append(int(row))
                vals.append(float(val))
            ptr.append(len(rows))
        ptr, rows, vals = _i64(ptr), _i64(rows), _f64(vals)
        pidx = _i64(list(probes))
        out = np.zeros(((n_cols or 1) + len(extras), max(len(pidx), 1)), dtype=np.float64)
        opts = CsrMatrix._opts(rtol, 0.0, max_iter, 0, False, precond=precond, rebuild=rebuild)
        info = SolveInfo()
        # the array stage 2 will hand back (and that of the power densities of a block that asks for them): their pages are
        # touched while the device solves, so that a block's result is ready when the device is
        coo, dev = isinstance(r, tuple), isinstance(r, int)
        v_shape = (self.N, n_cols) if coo or dev else r.shape
        self._prefault = {"v": _prefaulted(v_shape)}
        if coo and power_tri > 0:
            self._prefault["pd"] = _prefaulted((power_rows or n_cols, power_tri))
        if coo and current_tri > 0:
            self._prefault["cur"] = _prefaulted((3 * current_cols * current_tri,))
        lib, common = self.ctx._lib, (kidx.shape[0], _ptr(kidx, _PI64), _ptr(kval, _PF64), len(extras),
                                      _ptr(ptr, _PI64), _ptr(rows, _PI64), _ptr(vals, _PF64), pidx.shape[0], _ptr(pidx, _PI64),
                                      _ptr(out, _PF64), C.byref(opts), float(abs_residual_target), C.byref(info))
        if coo:
            r_rows, r_cols, r_vals = r
            rc = lib.padne_kkt_solve_block_coo(self.ctx._h, self._h, int(n_cols), r_rows.shape[0], _ptr(r_rows, _PI64),
                                               _ptr(r_cols, _PI32), _ptr(r_vals, _PF64), *common)
        elif dev:
            rc = lib.padne_kkt_solve_block_dev(self.ctx._h, self._h, int(n_cols), _P(r), *common)
        elif n_cols is None:
            rc = lib.padne_kkt_solve(self.ctx._h, self._h, _ptr(r, _PF64), *common)
        else:
            rc = lib.padne_kkt_solve_block(self.ctx._h, self._h, int(n_cols), _ptr(r, _PF64), *common)
        if rc != OK and rc != E_NOTCONVERGED:
            _check(rc)
        res = SolveResult(None, info.iterations, info.restarts, info.rel_residual, info.abs_residual, info.solve_seconds,
                          info.status, info.spmv_seconds, info.precond_setup_seconds, info.operator_complexity, info.levels,
                          info.precond_fallbacks)
        return out[:, :len(pidx)], res

    def _result_array(self, shape, slot: str = "v"):
        """The array stage 1 made ready for ``slot`` ("v": stage 2's result, "pd": power densities, "cur": J and |J|) once
        its pages are touched, if it has ``shape``; else a fresh one.  The slot is left empty."""
        arr, toucher = getattr(self, "_prefault", {}).pop(slot, (None, None))
        for t in toucher or ():
            t.join()
        if arr is None or arr.shape != shape:
            arr = np.empty(shape, dtype=np.float64)
        return arr

    def power_density_block(self, n_cols: int, n_tri: int) -> np.ndarray:
        """Per-face sigma |grad V|^2 of every column of the block the last ``finish_block`` left on the device, over the mesh
        the system was assembled from (``n_tri`` triangles, as ``CsrMatrix.power_density`` takes it): (n_cols, n_tri), row j
        bit-identical to ``CsrMatrix.power_density`` of V[:, j].  Raises ValueError when no block has been finished since the
        last solve, on another column count, and on a matrix without a mesh."""
        out = self._result_array((int(n_cols), int(n_tri)), "pd")
        _check(self.ctx._lib.padne_kkt_power_density_block(self.ctx._h, self._h, int(n_cols), _ptr(out, _PF64)))
        return out

    def combine_block(self, n_cols: int, w_ptr, w_col, w_val, download: bool = True):
        """Element cases: the block V (N, n_cols) the last ``finish_block`` left on the device becomes V' (N, n_out) with
        V'[:, c] = sum_e w_val[e] V[:, w_col[e]] over the entries e = w_ptr[c] .. w_ptr[c + 1] - 1 of row c of the CSR weights,
        in that order (the first product starts the sum; a row of one entry 1.0 copies the column's bits).  V' takes the
        block's place on the device -- ``power_density_block(n_out, ...)``, ``current_cases`` and the others then work on it --
        and is returned (N, n_out) C-contiguous unless ``download`` is False (then None).  V and V' are on the device
        together: (n_cols + n_out) * N * 8 bytes.  Raises ValueError as ``power_density_block`` does, and unless
        1 <= n_out <= 4096, every row's columns are strictly ascending and in [0, n_cols) and every coefficient is finite."""
        ptr, col, val = _i64(w_ptr).reshape(-1), _i32(w_col).reshape(-1), _f64(w_val).reshape(-1)
        if ptr.shape[0] < 1 or col.shape[0] != val.shape[0] or (ptr.shape[0] > 1 and int(ptr[-1]) != col.shape[0]):
            raise ValueError("w_ptr must have n_out + 1 entries, the last one the number of weights in w_col and w_val")
        n_out = ptr.shape[0] - 1
        out = np.empty((self.N, n_out), dtype=np.float64) if download and 1 <= n_out <= 4096 else None
        _check(self.ctx._lib.padne_kkt_combine_block(self.ctx._h, self._h, int(n_cols), n_out, _ptr(ptr, _PI64), _ptr(col, _PI32),
                                                     _ptr(val, _PF64), _ptr(out, _PF64) if out is not None else None))
        return out

    def sensitivity_block(self, weights, n_tri: int, n_mesh: int):
        """Adjoint sensitivities from the block the last ``finish_block`` left on the device, over the mesh the system was
        assembled from (``n_tri`` triangles in ``n_mesh`` meshes): adjoint j is sum_m weights[j, m] V[:, m] for ``weights``
        (n_obj, n_cols).  Returns (power (n_tri,) of column 0, bit-identical to ``CsrMatrix.power_density`` of V[:, 0];
        s_f / area_f (n_obj, n_tri); per-mesh sums of s_f (n_obj, n_mesh)), s_f = sigma dJ_j / dsigma_f (include/padne_hip.h).
        Raises ValueError as ``power_density_block`` does, and for weights that are not finite."""
        W = _f64(weights)
        if W.ndim != 2 or W.shape[0] < 1:
            raise ValueError("weights must have shape (n_obj, n_cols) with n_obj >= 1")
        n_obj = W.shape[0]
        power = self._result_array((n_obj + 1, int(n_tri)), "pd")
        density = power[1:]
        totals = np.empty((n_obj, int(n_mesh)), dtype=np.float64)
        _check(self.ctx._lib.padne_kkt_sensitivity_block(self.ctx._h, self._h, W.shape[1], n_obj, _ptr(W, _PF64),
                                                         _ptr(power[0], _PF64), _ptr(density, _PF64), _ptr(totals, _PF64)))
        return power[0], density, totals

    @staticmethod
    def _cut_arguments(mesh_layer, cut_layer, cut_xy):
        """The arrays as the currents entries take them; ValueError when the two cut arrays do not list the same cuts."""
        ml, cl, xy = _i32(mesh_layer).reshape(-1), _i32(cut_layer).reshape(-1), _f64(cut_xy).reshape(-1, 4)
        if xy.shape[0] != cl.shape[0]:
            raise ValueError("cut_layer and cut_xy must list the same cuts")
        return ml, cl, xy

    def current_report(self, n_cols: int, n_tri: int, mesh_layer, cut_layer, cut_xy):
        """The currents of column 0 of the block the last ``finish_block`` left on the device, over the mesh the system was
        assembled from (``n_tri`` triangles; ``mesh_layer`` (n_mesh,): the layer of each mesh).  Cut c is the segment
        ``cut_xy[c]`` = (start x, y, end x, y) on layer ``cut_layer[c]``.  Returns (J (n_tri, 2) = -sigma grad V, |J| (n_tri,),
        the largest |J| of each mesh (n_mesh,), its face (n_mesh,) as a global index (-1 for a mesh without faces), the
        current through each cut (n_cut,)): ``current_cases`` of one column, less the envelope and the power.  Raises
        ValueError as ``sensitivity_block`` does, for over 4096 cuts, end points not finite and a cut of no length."""
        ml, cl, xy = self._cut_arguments(mesh_layer, cut_layer, cut_xy)
        n_tri, n_mesh, n_cut = int(n_tri), ml.shape[0], cl.shape[0]
        buf = self._result_array((3 * n_tri,), "cur")
        J, mag = buf[:2 * n_tri].reshape(n_tri, 2), buf[2 * n_tri:]
        mesh_max, mesh_face = np.empty(n_mesh, dtype=np.float64), np.empty(n_mesh, dtype=np.int64)
        cuts = np.empty(n_cut, dtype=np.float64)
        _check(self.ctx._lib.padne_kkt_current_report(self.ctx._h, self._h, int(n_cols), n_tri, n_mesh, _ptr(ml, _PI32), n_cut,
                                                      _ptr(cl, _PI32), _ptr(xy, _PF64), _ptr(J, _PF64), _ptr(mag, _PF64),
                                                      _ptr(mesh_max, _PF64), _ptr(mesh_face, _PI64), _ptr(cuts, _PF64)))
        return J, mag, mesh_max, mesh_face, cuts

    def current_cases(self, n_cols: int, n_tri: int, mesh_layer, cut_layer, cut_xy, fields: bool = True, envelope: bool = True):
        """``current_report`` for every column of the block the last ``finish_block`` left on the device, and the envelope
        over the columns.  Returns (J (n_cols, n_tri, 2), |J| (n_cols, n_tri) -- both None without ``fields``: the device
        then writes and sends home no per-column field --, max_j |J_j| (n_tri,), the lowest column that attains it (n_tri,)
        int32 -- both None without ``envelope``, likewise --, and per column the largest |J| of each mesh (n_cols, n_mesh), its face (n_cols, n_mesh), the power of each
        mesh in the |cot|/2 weights' form (n_cols, n_mesh) and the current through each cut (n_cols, n_cut))
        (include/padne_hip.h).  Row 0 holds ``current_report``'s bits.  Raises ValueError as ``current_report`` does."""
        ml, cl, xy = self._cut_arguments(mesh_layer, cut_layer, cut_xy)
        n_cols, n_tri, n_mesh, n_cut = int(n_cols), int(n_tri), ml.shape[0], cl.shape[0]
        if n_cols < 1:
            raise ValueError("a block has at least one column")
        J = mag = None
        if fields:
            buf = self._result_array((3 * n_cols * n_tri,), "cur")
            J, mag = buf[:2 * n_cols * n_tri].reshape(n_cols, n_tri, 2), buf[2 * n_cols * n_tri:].reshape(n_cols, n_tri)
        env = np.empty(n_tri, dtype=np.float64) if envelope else None
        env_case = np.empty(n_tri, dtype=np.int32) if envelope else None
        mesh_max, mesh_power = (np.empty((n_cols, n_mesh), dtype=np.float64) for _ in range(2))
        mesh_face = np.empty((n_cols, n_mesh), dtype=np.int64)
        cuts = np.empty((n_cols, n_cut), dtype=np.float64)
        _check(self.ctx._lib.padne_kkt_current_cases(
            self.ctx._h, self._h, n_cols, n_tri, n_mesh, _ptr(ml, _PI32), n_cut, _ptr(cl, _PI32), _ptr(xy, _PF64),
            None if J is None else _ptr(J, _PF64), None if mag is None else _ptr(mag, _PF64),
            None if env is None else _ptr(env, _PF64), None if env_case is None else _ptr(env_case, _PI32), _ptr(mesh_max, _PF64), _ptr(mesh_face, _PI64), _ptr(mesh_power, _PF64), _ptr(cuts, _PF64)))
        return J, mag, env, env_case, mesh_max, mesh_face, mesh_power, cuts

    def error_estimate(self, n_cols: int, n_tri: int, n_vert: int, n_mesh: int):
        """The gradient-recovery error estimate of column 0 of the block the last ``finish_block`` left on the device, over
        the mesh the system was assembled from (``n_tri`` triangles and ``n_vert`` vertices in ``n_mesh`` meshes).  Returns
        (G (n_vert, 2) the recovered gradient, eta (n_tri,) the indicators, and per mesh sum eta^2, sum sigma A |g|^2, the
        largest eta and its face as a global index, -1 for a mesh without faces) (include/padne_hip.h).  The vertex lists
        are built by the first call and kept with the plan.  Raises ValueError as ``current_report`` does."""
        n_tri, n_vert, n_mesh = int(n_tri), int(n_vert), int(n_mesh)
        G = np.empty((n_vert, 2), dtype=np.float64)
        eta = np.empty(n_tri, dtype=np.float64)
        mesh_error, mesh_power, mesh_max = (np.empty(n_mesh, dtype=np.float64) for _ in range(3))
        mesh_face = np.empty(n_mesh, dtype=np.int64)
        _check(self.ctx._lib.padne_kkt_error_estimate(self.ctx._h, self._h, int(n_cols), n_tri, n_vert, n_mesh, _ptr(G, _PF64),
                                                      _ptr(eta, _PF64), _ptr(mesh_error, _PF64), _ptr(mesh_power, _PF64),
                                                      _ptr(mesh_max, _PF64), _ptr(mesh_face, _PI64)))
        return G, eta, mesh_error, mesh_power, mesh_max, mesh_face

    def goal_error(self, weights, n_tri: int, n_vert: int, n_mesh: int):
        """The goal-oriented error estimate of the block the last ``finish_block`` left on the device: field 0 is column 0,
        field 1 + j the adjoint sum_m weights[j, m] V[:, m] for ``weights`` (n_obj, n_cols), as ``sensitivity_block`` takes
        them.  Returns (the power density of column 0 (n_tri,), bit-identical to ``CsrMatrix.power_density``; ``error_estimate``'s six
        results, bit for bit; then per objective: eta of the adjoint (n_obj, n_tri),
        delta (n_obj, n_tri), omega (n_obj, n_tri), and per mesh the sums of omega and of delta (n_obj, n_mesh), the largest
        omega and its face as a global index, -1 for a mesh without faces) (include/padne_hip.h).  The vertex lists are
        ``error_estimate``'s.  Raises ValueError as ``sensitivity_block`` and ``error_estimate`` do."""
        W = _f64(weights)
        if W.ndim != 2 or W.shape[0] < 1:
            raise ValueError("weights must have shape (n_obj, n_cols) with n_obj >= 1")
        n_obj, n_tri, n_vert, n_mesh = W.shape[0], int(n_tri), int(n_vert), int(n_mesh)
        G = np.empty((n_vert, 2), dtype=np.float64)
        power, eta = np.empty(n_tri, dtype=np.float64), np.empty(n_tri, dtype=np.float64)
        mesh_error, mesh_power, mesh_max = (np.empty(n_mesh, dtype=np.float64) for _ in range(3))
        mesh_face = np.empty(n_mesh, dtype=np.int64)
        dual, delta, omega = (np.empty((n_obj, n_tri), dtype=np.float64) for _ in range(3))
        m_omega, m_delta, m_top = (np.empty((n_obj, n_mesh), dtype=np.float64) for _ in range(3))
        m_face = np.empty((n_obj, n_mesh), dtype=np.int64)
        _check(self.ctx._lib.padne_kkt_goal_error(self.ctx._h, self._h, W.shape[1], n_obj, _ptr(W, _PF64), n_tri, n_vert, n_mesh,
                                                  _ptr(power, _PF64), _ptr(G, _PF64), _ptr(eta, _PF64), _ptr(mesh_error, _PF64), _ptr(mesh_power, _PF64),
                                                  _ptr(mesh_max, _PF64), _ptr(mesh_face, _PI64), _ptr(dual, _PF64),
                                                  _ptr(delta, _PF64), _ptr(omega, _PF64), _ptr(m_omega, _PF64), _ptr(m_delta, _PF64),
                                                  _ptr(m_top, _PF64), _ptr(m_face, _PI64)))
        return power, (G, eta, mesh_error, mesh_power, mesh_max, mesh_face), dual, delta, omega, m_omega, m_delta, m_top, m_face

    def finish(self, extra_coeff, multipliers: dict):
        """Stage 2: (v, ||L v - r||)."""
        coeff = _f64(extra_coeff)
        midx = _i64(sorted(multipliers))
        mval = _f64([multipliers[int(i)] for i in midx])
        v = self._result_array((self.N,))
        norm = C.c_double()
        _check(self.ctx._lib.padne_kkt_finish(self.ctx._h, self._h, coeff.shape[0], _ptr(coeff, _PF64), midx.shape[0],
                                              _ptr(midx, _PI64), _ptr(mval, _PF64), _ptr(v, _PF64), C.byref(norm)))
        return v, norm.value

    def finish_block(self, extra_coeff, mult_idx, mult_val):
        """Stage 2 of a block: ``extra_coeff`` (k, n_extra) regulator currents per column, ``mult_val`` (k, n_mult)
        multiplier currents per column at the unknowns ``mult_idx``.  Returns (V (N, k) C-contiguous, ||L v_j - r_j|| (k,))."""
        coeff = _f64(extra_coeff)
        if coeff.ndim != 2:
            raise ValueError("extra_coeff must have shape (k, n_extra)")
        k = coeff.shape[0]
        midx = _i64(mult_idx)
        mval = _f64(mult_val).reshape(k, midx.shape[0])
        V = self._result_array((self.N, k))
        norms = np.zeros(k, dtype=np.float64)
        _check(self.ctx._lib.padne_kkt_finish_block(self.ctx._h, self._h, k, coeff.shape[1], _ptr(coeff, _PF64), midx.shape[0],
                                                    _ptr(midx, _PI64), _ptr(mval, _PF64), _ptr(V, _PF64), _ptr(norms, _PF64)))
        return V, norms


class SourceOffCopperError(ValueError):
    """``Thermal.set_sources``: the heat sources ``sources`` (indices) cover no face and no face owns their vertex mean."""

    def __init__(self, message: str, sources: list):
        super().__init__(message)
        self.sources = sources


class Thermal:
    """``padne_thermal``: the thermal sheet problem A theta = b on the meshes an assembled system ``L`` keeps on the device
    (include/padne_hip.h, "thermal").  ``kappa`` and ``film`` per mesh, ``links`` an (n, 2) array of unknowns with
    ``link_g`` (n,) W/K.  Holds A with its hierarchy, the lumped areas and, after a solve, the face powers and theta.

    With ``mesh_layer`` (the layer of every mesh) the handle is made by ``padne_thermal_create_stacked`` (include/padne_hip.h,
    "stack"): ``pairs`` is a sequence of (layer a, layer b, g [W/(K mesh-unit^2)]) and the matrix is A' = A + G, the heat
    conduction between the layers of every pair; ``stack_flows`` and the ``stack_*`` read-outs then work.

    ``set_film_curves`` makes the film of every mesh a table over the temperature rise (include/padne_hip.h, "film curves"):
    the solves then take one column, and a Newton round is ``film_linearise``, a solve (``solve``, ``solve_kkt_column``,
    ``resolve``, ``Coupled.solve_kkt``) and ``film_increment``."""

    def __init__(self, L: "CsrMatrix", n_potential: int, kappa, film, link_a=(), link_b=(), link_g=(), *, mesh_layer=None,
                 pairs=(), n_layer=None):
        self.ctx, self.L = L.ctx, L
        kap, flm = _f64(kappa).reshape(-1), _f64(film).reshape(-1)
        la, lb, lg = _i64(link_a).reshape(-1), _i64(link_b).reshape(-1), _f64(link_g).reshape(-1)
        if kap.shape != flm.shape:
            raise ValueError("one kappa and one film per mesh")
        if not (la.shape == lb.shape == lg.shape):
            raise ValueError("link_a, link_b and link_g must list the same links")
        h = _P()
        self.stacked, self.n_pair = mesh_layer is not None, 0
        if not self.stacked:
            if len(pairs):
                raise ValueError("pairs of layers need mesh_layer")
            _check(self.ctx._lib.padne_thermal_create(self.ctx._h, L._h, int(n_potential), kap.shape[0], _ptr(kap, _PF64),
                                                      _ptr(flm, _PF64), la.shape[0], _ptr(la, _PI64), _ptr(lb, _PI64),
                                                      _ptr(lg, _PF64), C.byref(h)))
        else:
            ml = _i32(mesh_layer).reshape(-1)
            if ml.shape != kap.shape:
                raise ValueError("one layer per mesh")
            pairs = list(pairs)
            pa, pb = _i32([p[0] for p in pairs]), _i32([p[1] for p in pairs])
            pg = _f64([p[2] for p in pairs])
            if n_layer is None:
                n_layer = max([1] + [int(x) + 1 for x in ml] + [int(x) + 1 for x in pa] + [int(x) + 1 for x in pb])
            _check(self.ctx._lib.padne_thermal_create_stacked(
                self.ctx._h, L._h, int(n_potential), kap.shape[0], _ptr(kap, _PF64), _ptr(flm, _PF64), la.shape[0], _ptr(la, _PI64),
                _ptr(lb, _PI64), _ptr(lg, _PF64), int(n_layer), _ptr(ml, _PI32), len(pairs), _ptr(pa, _PI32), _ptr(pb, _PI32),
                _ptr(pg, _PF64), C.byref(h)))
            self.n_pair = len(pairs)
        self._h = h
        self.n_potential, self.n_mesh = int(n_potential), kap.shape[0]
        self.n_source, self.n_source_entries = 0, 0

    def stack_sizes(self):
        """(pairs, sides, (side, vertex) slots, stored off-diagonals of G) of a stacked handle."""
        out = np.zeros(4, dtype=np.int64)
        _check(self.ctx._lib.padne_thermal_stack_sizes(self._h, _ptr(out, _PI64)))
        return tuple(int(x) for x in out)

    def stack_links(self):
        """The link slots of a stacked handle: (side offsets (sides + 1,), vertex (n,), owner face (n,) or -1, weights (n, 3),
        conductances (n, 3)), side by side (include/padne_hip.h)."""
        _, n_side, n, _ = self.stack_sizes()
        off = np.zeros(n_side + 1, dtype=np.int64)
        vert, owner = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
        w, c = np.empty((n, 3), dtype=np.float64), np.empty((n, 3), dtype=np.float64)
        _check(self.ctx._lib.padne_thermal_stack_links(self.ctx._h, self._h, n, _ptr(off, _PI64), _ptr(vert, _PI32),
                                                       _ptr(owner, _PI32), _ptr(w, _PF64), _ptr(c, _PF64)))
        return off, vert, owner, w, c

    def stack_matrix(self):
        """G of a stacked handle: (indptr, indices, data) of its off-diagonals as CSR and its diagonal (n_potential,)."""
        nnz = self.stack_sizes()[3]
        indptr, indices = np.empty(self.n_potential + 1, dtype=np.int32), np.empty(nnz, dtype=np.int32)
        data, diag = np.empty(nnz, dtype=np.float64), np.empty(self.n_potential, dtype=np.float64)
        _check(self.ctx._lib.padne_thermal_stack_matrix(self.ctx._h, self._h, nnz, _ptr(indptr, _PI32), _ptr(indices, _PI32),
                                                        _ptr(data, _PF64), _ptr(diag, _PF64)))
        return indptr, indices, data, diag

    def stack_flows(self, n_cols: int):
        """On the theta of the last solve: (flow (n_cols, n_pair) [W] from layer a to layer b of every pair, coupled area
        (n_pair,)).  ``n_cols`` 0: the areas alone."""
        n_cols = int(n_cols)
        flow, area = np.zeros((n_cols, self.n_pair), dtype=np.float64), np.zeros(self.n_pair, dtype=np.float64)
        _check(self.ctx._lib.padne_thermal_stack_flows(self.ctx._h, self._h, n_cols, _ptr(flow, _PF64), _ptr(area, _PF64)))
        return flow, area

    def set_sources(self, n_layer: int, mesh_layer, source_layer, polygons):
        """The heat sources of the handle (include/padne_hip.h, "heat sources"): ``mesh_layer`` the layer of every mesh,
        ``source_layer`` (n,) and ``polygons`` a sequence of n arrays (m, 2).  Returns (faces in each source's list (n,) int64,
        fallback flags (n,) int32, A_s (n,)); a second call replaces the sources, none removes them.
        :class:`SourceOffCopperError` for sources that lie on no copper the system keeps."""
        ml, sl = _i32(mesh_layer).reshape(-1), _i32(source_layer).reshape(-1)
        polys = [_f64(p) for p in polygons]
        if len(polys) != sl.shape[0] or any(p.ndim != 2 or p.shape[1] != 2 for p in polys):
            raise ValueError("one polygon of shape (m, 2) per source")
        ptr = _i64(np.concatenate([[0], np.cumsum([len(p) for p in polys])]))
        xy = _f64(np.concatenate(polys)) if polys else np.zeros((0, 2))
        n = sl.shape[0]
        counts, fallback, area = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float64)
        self.n_source, self.n_source_entries = 0, 0
        rc = self.ctx._lib.padne_thermal_set_sources(self.ctx._h, self._h, int(n_layer), ml.shape[0], _ptr(ml, _PI32), n,
                                                     _ptr(sl, _PI32), _ptr(ptr, _PI64), _ptr(xy, _PF64), _ptr(counts, _PI64),
                                                     _ptr(fallback, _PI32), _ptr(area, _PF64))
        if rc == E_INVALID and (fallback == 2).any():
            msg = (load_library().padne_last_error() or b"").decode("utf-8", "replace")
            raise SourceOffCopperError(msg, [int(i) for i in np.flatnonzero(fallback == 2)])
        _check(rc)
        self.n_source, self.n_source_entries = n, int(counts.sum())
        return counts, fallback, area

    def source_power(self, power) -> None:
        """The powers (n_cols, n_source) [W] the next loads of the handle use; a load of another number of columns fails."""
        P = _f64(power)
        if P.ndim != 2 or P.shape[1] != self.n_source:
            raise ValueError("power must have shape (n_cols, n_source)")
        _check(self.ctx._lib.padne_thermal_source_power(self.ctx._h, self._h, P.shape[0], _ptr(P, _PF64)))

    def source_lists(self):
        """(ptr (n_source + 1,), face (entries,)): the faces of every source in ascending global number."""
        ptr, face = np.zeros(self.n_source + 1, dtype=np.int64), np.empty(self.n_source_entries, dtype=np.int32)
        _check(self.ctx._lib.padne_thermal_source_lists(self.ctx._h, self._h, self.n_source, self.n_source_entries, _ptr(ptr, _PI64),
                                                        _ptr(face, _PI32)))
        return ptr, face

    def source_report(self, n_cols: int) -> np.ndarray:
        """On the theta of the last solve: T_s - ambient (n_cols, n_source), the area-weighted mean over every source's list."""
        out = np.empty((int(n_cols), self.n_source), dtype=np.float64)
        _check(self.ctx._lib.padne_thermal_source_report(self.ctx._h, self._h, int(n_cols), _ptr(out, _PF64)))
        return out

    def close(self):
        if getattr(self, "_h", None) and self.ctx._h:
            self.ctx._lib.padne_thermal_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def matrix(self) -> "CsrMatrix":
        """Borrowed view of A (valid while the handle lives)."""
        h = _P()
        _check(self.ctx._lib.padne_thermal_matrix(self._h, C.byref(h)))
        m = CsrMatrix(self.ctx, h)
        m._borrowed = True
        return m

    def lumped(self, n_vert: int) -> np.ndarray:
        """M_v (n_vert,)."""
        out = np.empty(int(n_vert), dtype=np.float64)
        _check(self.ctx._lib.padne_thermal_lumped(self.ctx._h, self._h, _ptr(out, _PF64)))
        return out

    @staticmethod
    def _heat(heat):
        node, col, val = heat if heat is not None else ((), (), ())
        node, col, val = _i64(node).reshape(-1), _i32(col).reshape(-1), _f64(val).reshape(-1)
        if not (node.shape == col.shape == val.shape):
            raise ValueError("the node-heat triples must have equal lengths")
        return node, col, val

    def _solve(self, call, n_cols, heat, rtol, max_iter, precond, download):
        node, col, val = self._heat(heat)
        opts = CsrMatrix._opts(rtol, 0.0, max_iter, 0, False, precond=precond)
        info = SolveInfo()
        theta = np.empty((n_cols, self.n_potential), dtype=np.float64) if download else None
        rc = call(node.shape[0], _ptr(node, _PI64), _ptr(col, _PI32), _ptr(val, _PF64), C.byref(opts),
                  None if theta is None else _ptr(theta, _PF64), C.byref(info))
        if rc != OK and rc != E_NOTCONVERGED:
            _check(rc)
        res = SolveResult(None, info.iterations, info.restarts, info.rel_residual, info.abs_residual, info.solve_seconds,
                          info.status, info.spmv_seconds, info.precond_setup_seconds, info.operator_complexity, info.levels,
                          info.precond_fallbacks)
        return theta, res

    def load(self, face_power, heat=None) -> np.ndarray:
        """The heat load b (n_cols, n_potential) as ``solve`` forms it from the same arguments; nothing is solved."""
        P = _f64(face_power)
        if P.ndim != 2 or P.shape[0] < 1:
            raise ValueError("face_power must have shape (n_cols, n_tri) with n_cols >= 1")
        node, col, val = self._heat(heat)
        out = np.empty((P.shape[0], self.n_potential), dtype=np.float64)
        _check(self.ctx._lib.padne_thermal_load(self.ctx._h, self._h, P.shape[0], _ptr(P, _PF64), node.shape[0], _ptr(node, _PI64),
                                                _ptr(col, _PI32), _ptr(val, _PF64), _ptr(out, _PF64)))
        return out

    def solve(self, face_power, heat=None, *, rtol=1e-12, max_iter=200000, precond="amg", download=True):
        """theta (n_cols, n_potential) for the face powers ``face_power`` (n_cols, n_tri) [W] and the node-heat triples
        ``heat`` = (node, column, watts), and the SolveResult of the block solve.  Without ``download`` theta stays on the
        device for ``report`` and None is returned in its place."""
        P = _f64(face_power)
        if P.ndim != 2 or P.shape[0] < 1:
            raise ValueError("face_power must have shape (n_cols, n_tri) with n_cols >= 1")
        lib = self.ctx._lib
        return self._solve(lambda *a: lib.padne_thermal_solve(self.ctx._h, self._h, P.shape[0], _ptr(P, _PF64), *a), P.shape[0],
                           heat, rtol, max_iter, precond, download)

    def solve_kkt(self, plan: "KktPlan", n_cols: int, heat=None, *, rtol=1e-12, max_iter=200000, precond="amg", download=True):
        """``solve`` with the face powers of every column of the block ``plan``'s last ``finish_block`` left on the device,
        computed there (the |cot|/2 weights' form that ``current_cases`` sums per mesh)."""
        lib, n_cols = self.ctx._lib, int(n_cols)
        if n_cols < 1:
            raise ValueError("a block has at least one column")
        return self._solve(lambda *a: lib.padne_thermal_solve_kkt(self.ctx._h, self._h, plan._h, n_cols, *a), n_cols, heat, rtol,
                           max_iter, precond, download)

    def set_film_curves(self, curves) -> None:
        """The film curves of the handle (include/padne_hip.h, "film curves"): per mesh a pair (rise (n,), film (n,)) of 1 to
        64 knots whose first film is the film the handle was made with; an empty sequence removes the curves.  ValueError
        for what ``padne_thermal_set_film_curves`` refuses."""
        curves = [(_f64(r).reshape(-1), _f64(f).reshape(-1)) for r, f in curves]
        if any(r.shape != f.shape for r, f in curves):
            raise ValueError("one film per rise")
        ptr = _i32(np.concatenate([[0], np.cumsum([len(r) for r, _ in curves])]))
        rise = _f64(np.concatenate([r for r, _ in curves])) if curves else np.zeros(0)
        film = _f64(np.concatenate([f for _, f in curves])) if curves else np.zeros(0)
        _check(self.ctx._lib.padne_thermal_set_film_curves(self.ctx._h, self._h, len(curves), _ptr(ptr, _PI32), _ptr(rise, _PF64),
                                                           _ptr(film, _PF64)))

    def film_terms(self, theta, n_vert: int):
        """(g, c, hM) (n_vert,) each and the number of vertices above their last knot, for any ``theta`` (n_vert,)."""
        th = _f64(theta).reshape(-1)
        if th.shape[0] != int(n_vert):
            raise ValueError("theta has one entry per vertex")
        g, c, hM = (np.empty(int(n_vert), dtype=np.float64) for _ in range(3))
        beyond = np.zeros(1, dtype=np.int64)
        _check(self.ctx._lib.padne_thermal_film_terms(self.ctx._h, self._h, _ptr(th, _PF64), _ptr(g, _PF64), _ptr(c, _PF64),
                                                      _ptr(hM, _PF64), _ptr(beyond, _PI64)))
        return g, c, hM, int(beyond[0])

    def film_linearise(self, from_held: bool) -> None:
        """The film linearised about the held theta of a one-column solve, or about zero."""
        _check(self.ctx._lib.padne_thermal_film_linearise(self.ctx._h, self._h, 1 if from_held else 0))

    def film_increment(self) -> tuple:
        """After a one-column solve: (max_v |theta_v - the iterate of the last linearise|, its vertex, the number of vertices
        above their last knot); hM becomes h(theta_v) M_v for the reports."""
        inc = np.zeros(1, dtype=np.float64)
        vert, beyond = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
        _check(self.ctx._lib.padne_thermal_film_increment(self.ctx._h, self._h, _ptr(inc, _PF64), _ptr(vert, _PI64),
                                                          _ptr(beyond, _PI64)))
        return float(inc[0]), int(vert[0]), int(beyond[0])

    def solve_kkt_column(self, plan: "KktPlan", n_cols: int, col: int, heat=None, *, rtol=1e-12, max_iter=200000, precond="amg",
                         download=True):
        """``solve_kkt`` for column ``col`` alone of the block of ``n_cols`` columns: theta (1, n_potential); the triples of
        ``heat`` name column 0."""
        lib = self.ctx._lib
        return self._solve(lambda *a: lib.padne_thermal_solve_kkt_column(self.ctx._h, self._h, plan._h, int(n_cols), int(col), *a),
                           1, heat, rtol, max_iter, precond, download)

    def resolve(self, *, rtol=1e-12, max_iter=200000, precond="amg", download=True):
        """The one-column solve again on the load the handle holds, with the c of the last ``film_linearise``."""
        opts = CsrMatrix._opts(rtol, 0.0, max_iter, 0, False, precond=precond)
        info = SolveInfo()
        theta = np.empty((1, self.n_potential), dtype=np.float64) if download else None
        rc = self.ctx._lib.padne_thermal_resolve(self.ctx._h, self._h, C.byref(opts), None if theta is None else _ptr(theta, _PF64),
                                                 C.byref(info))
        if rc != OK and rc != E_NOTCONVERGED:
            _check(rc)
        res = SolveResult(None, info.iterations, info.restarts, info.rel_residual, info.abs_residual, info.solve_seconds,
                          info.status, info.spmv_seconds, info.precond_setup_seconds, info.operator_complexity, info.levels,
                          info.precond_fallbacks)
        return theta, res

    def face_power(self, n_cols: int, n_tri: int) -> np.ndarray:
        """The face powers (n_cols, n_tri) of the last solve, as the handle holds them."""
        out = np.empty((int(n_cols), int(n_tri)), dtype=np.float64)
        _check(self.ctx._lib.padne_thermal_face_power(self.ctx._h, self._h, int(n_cols), _ptr(out, _PF64)))
        return out

    def report(self, n_cols: int, n_tri: int, n_vert: int, fields: bool = True, envelope: bool = True):
        """On the theta of the last solve: (face means (n_cols, n_tri) or None without ``fields``; per column and mesh the
        largest theta (n_cols, n_mesh), its vertex as a global index (-1 for a mesh without vertices), the heat put in and the
        film loss; max over the columns per vertex (n_vert,) and the lowest column that attains it (n_vert,) int32, both None
        without ``envelope``) (include/padne_hip.h)."""
        n_cols, n_tri, n_vert, n_mesh = int(n_cols), int(n_tri), int(n_vert), self.n_mesh
        mean = np.empty((n_cols, n_tri), dtype=np.float64) if fields else None
        mesh_max, heat, loss = (np.empty((n_cols, n_mesh), dtype=np.float64) for _ in range(3))
        vert = np.empty((n_cols, n_mesh), dtype=np.int64)
        env = np.empty(n_vert, dtype=np.float64) if envelope else None
        env_case = np.empty(n_vert, dtype=np.int32) if envelope else None
        _check(self.ctx._lib.padne_thermal_report(
            self.ctx._h, self._h, n_cols, n_tri, n_vert, n_mesh, None if mean is None else _ptr(mean, _PF64), _ptr(mesh_max, _PF64),
            _ptr(vert, _PI64), _ptr(heat, _PF64), _ptr(loss, _PF64), None if env is None else _ptr(env, _PF64),
            None if env_case is None else _ptr(env_case, _PI32)))
        return mean, mesh_max, vert, heat, loss, env, env_case


SDIRK_GAMMA = 0.29289321881345247560        # 1 - 1/sqrt(2), the library's kSdirkGamma
SDIRK_Q = 2.41421356237309504880            # sqrt(2) + 1 = (1 - gamma) / gamma, the library's kSdirkQ
SDIRK_GUESS = 2                             # what stage 2 starts from by default (DESIGN.md "Adaptive transient")


class Transient:
    """``padne_transient``: backward-Euler steps of C dtheta/dt + A theta = b(t) on a :class:`Thermal` handle
    (include/padne_hip.h, "transient").  ``capacity`` per mesh [J / (K mesh-unit^2)].  Holds the lumped capacities, the
    step matrix S with the dt it was formed for, the load table, the state of every column and its running envelope.
    Close it before ``thermal``."""

    def __init__(self, thermal: "Thermal", capacity):
        self.ctx, self.thermal = thermal.ctx, thermal
        cap = _f64(capacity).reshape(-1)
        h = _P()
        _check(self.ctx._lib.padne_transient_create(self.ctx._h, thermal._h, cap.shape[0], _ptr(cap, _PF64), C.byref(h)))
        self._h = h
        self.n_potential, self.n_mesh, self.n_case, self.n_cols = thermal.n_potential, thermal.n_mesh, 0, 0

    def close(self):
        if getattr(self, "_h", None) and self.ctx._h:
            self.ctx._lib.padne_transient_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def capacity(self, n_vert: int) -> np.ndarray:
        """Cv (n_vert,) [J/K]."""
        out = np.empty(int(n_vert), dtype=np.float64)
        _check(self.ctx._lib.padne_transient_capacity(self.ctx._h, self._h, _ptr(out, _PF64)))
        return out

    def loads(self, face_power, heat=None) -> None:
        """The load table from the face powers (n_case, n_tri) [W] and the node-heat triples (node, case, watts):
        ``Thermal.load``'s bits."""
        P = _f64(face_power)
        if P.ndim != 2 or P.shape[0] < 1:
            raise ValueError("face_power must have shape (n_case, n_tri) with n_case >= 1")
        node, col, val = Thermal._heat(heat)
        _check(self.ctx._lib.padne_transient_loads(self.ctx._h, self._h, P.shape[0], _ptr(P, _PF64), node.shape[0],
                                                   _ptr(node, _PI64), _ptr(col, _PI32), _ptr(val, _PF64)))
        self.n_case = P.shape[0]

    def loads_kkt(self, plan: "KktPlan", n_case: int, heat=None) -> None:
        """``loads`` with the face powers of every column of the block ``plan``'s last ``finish_block`` left on the device."""
        node, col, val = Thermal._heat(heat)
        _check(self.ctx._lib.padne_transient_loads_kkt(self.ctx._h, self._h, plan._h, int(n_case), node.shape[0],
                                                       _ptr(node, _PI64), _ptr(col, _PI32), _ptr(val, _PF64)))
        self.n_case = int(n_case)

    def reserve_loads(self, n_case: int) -> None:
        """The load table as ``n_case`` slots of zeros, for ``Coupled.transient_load`` to fill; ``start`` follows."""
        _check(self.ctx._lib.padne_transient_reserve_loads(self.ctx._h, self._h, int(n_case)))
        self.n_case = int(n_case)

    def load_vectors(self) -> np.ndarray:
        """The load table (n_case, n_potential)."""
        out = np.empty((self.n_case, self.n_potential), dtype=np.float64)
        _check(self.ctx._lib.padne_transient_load_vectors(self.ctx._h, self._h, self.n_case, _ptr(out, _PF64)))
        return out

    @staticmethod
    def _cases(cases) -> np.ndarray:
        return _i32([-1 if c is None else int(c) for c in cases]).reshape(-1)

    def start(self, initial, *, rtol=1e-12, max_iter=200000, precond="amg") -> SolveResult:
        """The state at time 0, one column per entry of ``initial``: None or -1 = ambient, j = the steady state of case j.
        Returns the SolveResult of the block solve for the steady states (all zeros when no column needs one)."""
        ini = self._cases(initial)
        opts = CsrMatrix._opts(rtol, 0.0, max_iter, 0, False, precond=precond)
        info = SolveInfo()
        rc = self.ctx._lib.padne_transient_start(self.ctx._h, self._h, ini.shape[0], _ptr(ini, _PI32), C.byref(opts), C.byref(info))
        if rc != OK and rc != E_NOTCONVERGED:
            _check(rc)
        self.n_cols = ini.shape[0]
        return SolveResult(None, info.iterations, info.restarts, info.rel_residual, info.abs_residual, info.solve_seconds,
                           info.status, info.spmv_seconds, info.precond_setup_seconds, info.operator_complexity, info.levels,
                           info.precond_fallbacks)

    def matrix(self, dt: float) -> "CsrMatrix":
        """Borrowed view of S revalued for ``dt`` (valid while the handle lives and until the next change of dt)."""
        h = _P()
        _check(self.ctx._lib.padne_transient_matrix(self._h, float(dt), C.byref(h)))
        m = CsrMatrix(self.ctx, h)
        m._borrowed = True
        return m

    def rhs(self, dt: float, case_of_col) -> np.ndarray:
        """The right-hand side (n_cols, n_potential) the next step of length ``dt`` would solve."""
        cases = self._cases(case_of_col)
        if cases.shape[0] != self.n_cols:
            raise ValueError("one case per column of the start")
        out = np.empty((self.n_cols, self.n_potential), dtype=np.float64)
        _check(self.ctx._lib.padne_transient_rhs(self.ctx._h, self._h, float(dt), _ptr(cases, _PI32), _ptr(out, _PF64)))
        return out

    def run(self, dt: float, n_steps: int, case_of_col, probes=(), *, rtol=1e-12, max_iter=200000, precond="amg") -> dict:
        """``n_steps`` steps of length ``dt`` under ``case_of_col`` (None or -1: sources off).  A dict of per-step arrays:
        ``max``, ``vertex``, ``stored``, ``loss`` (n_steps, n_cols, n_mesh), ``probes`` (n_steps, n_cols, n_probe),
        ``iterations``, ``rel_residual``, ``seconds``, ``setup_seconds`` (n_steps,), and ``result`` the SolveResult over the run."""
        cases, probe = self._cases(case_of_col), _i64(probes).reshape(-1)
        if cases.shape[0] != self.n_cols:
            raise ValueError("one case per column of the start")
        n_steps, k, m = int(n_steps), self.n_cols, self.n_mesh
        shape = (max(n_steps, 0), k, m)
        top, stored, loss = (np.empty(shape, dtype=np.float64) for _ in range(3))
        vert = np.empty(shape, dtype=np.int64)
        trace = np.empty((max(n_steps, 0), k, probe.shape[0]), dtype=np.float64)
        its = np.zeros(max(n_steps, 0), dtype=np.int32)
        rel, secs, setup = (np.zeros(max(n_steps, 0), dtype=np.float64) for _ in range(3))
        opts = CsrMatrix._opts(rtol, 0.0, max_iter, 0, True, precond=precond)
        info = SolveInfo()
        rc = self.ctx._lib.padne_transient_run(
            self.ctx._h, self._h, float(dt), n_steps, _ptr(cases, _PI32), probe.shape[0], _ptr(probe, _PI64), C.byref(opts),
            _ptr(top, _PF64), _ptr(vert, _PI64), _ptr(stored, _PF64), _ptr(loss, _PF64), _ptr(trace, _PF64), _ptr(its, _PI32),
            _ptr(rel, _PF64), _ptr(secs, _PF64), _ptr(setup, _PF64), C.byref(info))
        if rc != OK and rc != E_NOTCONVERGED:
            _check(rc)
        res = SolveResult(None, info.iterations, info.restarts, info.rel_residual, info.abs_residual, info.solve_seconds,
                          info.status, info.spmv_seconds, info.precond_setup_seconds, info.operator_complexity, info.levels,
                          info.precond_fallbacks)
        return {"max": top, "vertex": vert, "stored": stored, "loss": loss, "probes": trace, "iterations": its,
                "rel_residual": rel, "seconds": secs, "setup_seconds": setup, "result": res}

    def report(self):
        """Of the current state: (max, vertex, stored, loss), each (n_cols, n_mesh)."""
        shape = (self.n_cols, self.n_mesh)
        top, stored, loss = (np.empty(shape, dtype=np.float64) for _ in range(3))
        vert = np.empty(shape, dtype=np.int64)
        _check(self.ctx._lib.padne_transient_report(self.ctx._h, self._h, _ptr(top, _PF64), _ptr(vert, _PI64), _ptr(stored, _PF64),
                                                    _ptr(loss, _PF64)))
        return top, vert, stored, loss

    def state(self) -> np.ndarray:
        """theta (n_cols, n_potential)."""
        out = np.empty((self.n_cols, self.n_potential), dtype=np.float64)
        _check(self.ctx._lib.padne_transient_state(self.ctx._h, self._h, _ptr(out, _PF64)))
        return out

    def envelope(self, n_vert: int):
        """(the largest theta seen (n_cols, n_vert), the first step that attained it (n_cols, n_vert) int32)."""
        env = np.empty((self.n_cols, int(n_vert)), dtype=np.float64)
        step = np.empty((self.n_cols, int(n_vert)), dtype=np.int32)
        _check(self.ctx._lib.padne_transient_envelope(self.ctx._h, self._h, _ptr(env, _PF64), _ptr(step, _PI32)))
        return env, step

    def clock(self) -> tuple:
        """(steps since the start, their time, hierarchies built for S since creation)."""
        step, hier, t = _I64(), _I64(), C.c_double()
        _check(self.ctx._lib.padne_transient_clock(self._h, C.byref(step), C.byref(t), C.byref(hier)))
        return int(step.value), float(t.value), int(hier.value)

    def try_step(self, dt: float, case_of_col, *, guess=None, rtol=1e-12, max_iter=200000, precond="amg") -> dict:
        """One SDIRK2 trial step of length ``dt`` under ``case_of_col`` (include/padne_hip.h, "adaptive transient"); the state
        does not advance.  ``err`` (n_cols,) [K] with ``vertex`` (n_cols,), ``stage_iterations`` (2,), ``stage_setup_seconds``
        (2,) and ``result`` the SolveResult over both stages.  ``guess``: what stage 2's solve starts from (0 theta_1,
        1 theta*, 2 the line through theta_n and theta_1 at the end of the step; None: ``SDIRK_GUESS``)."""
        guess = SDIRK_GUESS if guess is None else guess
        cases = self._cases(case_of_col)
        if cases.shape[0] != self.n_cols:
            raise ValueError("one case per column of the start")
        err, vert = np.empty(self.n_cols, dtype=np.float64), np.empty(self.n_cols, dtype=np.int64)
        its, setup = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.float64)
        opts = CsrMatrix._opts(rtol, 0.0, max_iter, 0, True, precond=precond)
        info = SolveInfo()
        rc = self.ctx._lib.padne_transient_try_step(self.ctx._h, self._h, float(dt), _ptr(cases, _PI32), int(guess), C.byref(opts),
                                                    _ptr(err, _PF64), _ptr(vert, _PI64), _ptr(its, _PI32), _ptr(setup, _PF64),
                                                    C.byref(info))
        if rc != OK and rc != E_NOTCONVERGED:
            _check(rc)
        res = SolveResult(None, info.iterations, info.restarts, info.rel_residual, info.abs_residual, info.solve_seconds,
                          info.status, info.spmv_seconds, info.precond_setup_seconds, info.operator_complexity, info.levels,
                          info.precond_fallbacks)
        return {"err": err, "vertex": vert, "stage_iterations": its, "stage_setup_seconds": setup, "result": res}

    def accept(self, probes=()) -> dict:
        """The live trial becomes the state.  ``max``, ``vertex``, ``stored``, ``loss`` (n_cols, n_mesh) of the new state as
        ``run`` reports a step, ``stage_loss`` (n_cols, n_mesh) the film loss of theta_1, ``probes`` (n_cols, n_probe)."""
        probe = _i64(probes).reshape(-1)
        shape = (self.n_cols, self.n_mesh)
        top, stored, loss, stage = (np.empty(shape, dtype=np.float64) for _ in range(4))
        vert = np.empty(shape, dtype=np.int64)
        trace = np.empty((self.n_cols, probe.shape[0]), dtype=np.float64)
        _check(self.ctx._lib.padne_transient_accept(self.ctx._h, self._h, probe.shape[0], _ptr(probe, _PI64), _ptr(top, _PF64),
                                                    _ptr(vert, _PI64), _ptr(stored, _PF64), _ptr(loss, _PF64), _ptr(stage, _PF64),
                                                    _ptr(trace, _PF64)))
        return {"max": top, "vertex": vert, "stored": stored, "loss": loss, "stage_loss": stage, "probes": trace}

    def trial(self, which: int) -> np.ndarray:
        """theta_1 (0), theta* (1) or theta_{n+1} (2) of the live trial, (n_cols, n_potential)."""
        out = np.empty((self.n_cols, self.n_potential), dtype=np.float64)
        _check(self.ctx._lib.padne_transient_trial(self.ctx._h, self._h, int(which), _ptr(out, _PF64)))
        return out


class Periodic:
    """``padne_periodic``: the Krylov arithmetic of a duty cycle's period map on a started :class:`Transient`
    (include/padne_hip.h, "periodic steady state").  Holds x0, r0 and up to ``max_vectors`` basis vectors per column on the
    device.  Close it before ``transient``."""

    R0, X0, STATE = -1, -2, -3               # what ``vector`` and ``put`` name besides a basis vector

    def __init__(self, transient: "Transient", max_vectors: int):
        self.ctx, self.transient = transient.ctx, transient
        h = _P()
        _check(self.ctx._lib.padne_periodic_create(self.ctx._h, transient._h, int(max_vectors), C.byref(h)))
        self._h = h
        self.n_potential, self.n_cols, self.max_vectors = transient.n_potential, transient.n_cols, int(max_vectors)

    def close(self):
        if getattr(self, "_h", None) and self.ctx._h:
            self.ctx._lib.padne_periodic_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def mark(self) -> None:
        """x0 = the state."""
        _check(self.ctx._lib.padne_periodic_mark(self.ctx._h, self._h))

    def residual(self):
        """r0 = state - x0 and v_0: (beta (n_cols,), max |r0| over the vertices (n_cols,), its vertex (n_cols,))."""
        beta, top = np.empty(self.n_cols, dtype=np.float64), np.empty(self.n_cols, dtype=np.float64)
        vert = np.empty(self.n_cols, dtype=np.int64)
        _check(self.ctx._lib.padne_periodic_residual(self.ctx._h, self._h, _ptr(beta, _PF64), _ptr(top, _PF64), _ptr(vert, _PI64)))
        return beta, top, vert

    def load(self, j: int) -> None:
        """state = v_j; clock and envelope as after a start."""
        _check(self.ctx._lib.padne_periodic_load(self.ctx._h, self._h, int(j)))

    def push(self, j: int) -> np.ndarray:
        """w = v_j - state orthogonalised into v_{j+1}: the Hessenberg column (n_cols, j + 2)."""
        h = np.empty((self.n_cols, int(j) + 2), dtype=np.float64)
        _check(self.ctx._lib.padne_periodic_push(self.ctx._h, self._h, int(j), _ptr(h, _PF64)))
        return h

    def _coefficients(self, coef) -> np.ndarray:
        coef = _f64(coef)
        if coef.ndim != 2 or coef.shape[0] != self.n_cols:
            raise ValueError("coefficients must have shape (n_cols, n)")
        return np.ascontiguousarray(coef)

    def predict(self, coef):
        """(max_v |r0 - sum_i coef[c][i] v_i| (n_cols,), its vertex (n_cols,))."""
        coef = self._coefficients(coef)
        top, vert = np.empty(self.n_cols, dtype=np.float64), np.empty(self.n_cols, dtype=np.int64)
        _check(self.ctx._lib.padne_periodic_predict(self.ctx._h, self._h, coef.shape[1], _ptr(coef, _PF64), _ptr(top, _PF64),
                                                    _ptr(vert, _PI64)))
        return top, vert

    def combine(self, y) -> None:
        """state = x0 + sum_i y[c][i] v_i; clock and envelope as after a start."""
        y = self._coefficients(y)
        _check(self.ctx._lib.padne_periodic_combine(self.ctx._h, self._h, y.shape[1], _ptr(y, _PF64)))

    def vector(self, j: int) -> np.ndarray:
        """v_j (n_cols, n_potential); ``R0`` and ``X0`` name r0 and x0."""
        out = np.empty((self.n_cols, self.n_potential), dtype=np.float64)
        _check(self.ctx._lib.padne_periodic_vector(self.ctx._h, self._h, int(j), _ptr(out, _PF64)))
        return out

    def put(self, j: int, values) -> None:
        """v_j = ``values`` (n_cols, n_potential); ``R0``, ``X0`` and ``STATE`` name r0, x0 and the transient state."""
        values = np.ascontiguousarray(_f64(values))
        if values.shape != (self.n_cols, self.n_potential):
            raise ValueError("values must have shape (n_cols, n_potential)")
        _check(self.ctx._lib.padne_periodic_put(self.ctx._h, self._h, int(j), _ptr(values, _PF64)))


class Coupled:
    """``padne_coupled``: the electro-thermal coupling of an assembled system ``L`` and the :class:`Thermal` made from it
    (include/padne_hip.h, "electro-thermal coupling").  ``alpha`` per mesh [1/K].  Rewrites L's values in place (``revalue``)
    and puts the assembled ones back on ``close``; close it before ``thermal`` and ``L``."""

    def __init__(self, L: "CsrMatrix", thermal: "Thermal", alpha, ambient: float, conductance_temperature: float):
        self.ctx, self.L, self.thermal = L.ctx, L, thermal
        a = _f64(alpha).reshape(-1)
        h = _P()
        _check(self.ctx._lib.padne_coupled_create(self.ctx._h, L._h, thermal._h, a.shape[0], _ptr(a, _PF64), float(ambient),
                                                  float(conductance_temperature), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and self.ctx._h:
            self.ctx._lib.padne_coupled_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self) -> None:
        """Back to the copper at ambient."""
        _check(self.ctx._lib.padne_coupled_reset(self.ctx._h, self._h))

    def set_scale(self, scale) -> None:
        s = _f64(scale).reshape(-1)
        _check(self.ctx._lib.padne_coupled_set_scale(self.ctx._h, self._h, s.shape[0], _ptr(s, _PF64)))

    def get_scale(self, n_tri: int, used: bool = False, means: bool = False):
        """The next revalue's scale (n_tri,), or with ``used`` the last one's; with ``means`` also the face means of the
        last update."""
        s = np.empty(int(n_tri), dtype=np.float64)
        mean = np.empty(int(n_tri), dtype=np.float64) if means else None
        _check(self.ctx._lib.padne_coupled_get_scale(self.ctx._h, self._h, 1 if used else 0, int(n_tri), _ptr(s, _PF64),
                                                     None if mean is None else _ptr(mean, _PF64)))
        return (s, mean) if means else s

    def set_resistors(self, a, b, resistance, alpha, t0) -> None:
        """The lumped resistors whose resistance follows their temperature: ends ``a``, ``b`` (potential unknowns), the
        assembled ``resistance``, ``alpha`` [1/K] and ``t0`` per resistor; empty arrays remove them."""
        a, b = np.ascontiguousarray(a, dtype=np.int64).reshape(-1), np.ascontiguousarray(b, dtype=np.int64).reshape(-1)
        r, al, t = _f64(resistance).reshape(-1), _f64(alpha).reshape(-1), _f64(t0).reshape(-1)
        if not (a.shape == b.shape == r.shape == al.shape == t.shape):
            raise ValueError("one end a, end b, resistance, alpha and t0 per resistor")
        _check(self.ctx._lib.padne_coupled_set_resistors(self.ctx._h, self._h, a.shape[0], _ptr(a, _PI64), _ptr(b, _PI64),
                                                         _ptr(r, _PF64), _ptr(al, _PF64), _ptr(t, _PF64)))

    def get_resistors(self, n_res: int, used: bool = False, means: bool = False):
        """``get_scale`` for the resistors: the next revalue's scale (n_res,), or with ``used`` the last one's; with ``means``
        also the resistors' mean temperature rises of the last update."""
        s = np.empty(int(n_res), dtype=np.float64)
        mean = np.empty(int(n_res), dtype=np.float64) if means else None
        _check(self.ctx._lib.padne_coupled_get_resistors(self.ctx._h, self._h, 1 if used else 0, int(n_res), _ptr(s, _PF64),
                                                         None if mean is None else _ptr(mean, _PF64)))
        return (s, mean) if means else s

    def revalue(self) -> None:
        """L's values from the assembled ones and the scale; plans made from L before this hold the old values."""
        _check(self.ctx._lib.padne_coupled_revalue(self.ctx._h, self._h))

    def update(self, theta=None) -> float:
        """The next scale from the thermal handle's last solve (or from ``theta`` (n_potential,)): the largest change of a
        face mean [K]."""
        d = C.c_double()
        th = None if theta is None else _f64(theta).reshape(-1)
        _check(self.ctx._lib.padne_coupled_update(self.ctx._h, self._h, 0 if th is None else th.shape[0],
                                                  None if th is None else _ptr(th, _PF64), C.byref(d)))
        return d.value

    def solve_kkt(self, plan: "KktPlan", heat=None, *, rtol=1e-12, max_iter=200000, precond="amg", download=True):
        """``Thermal.solve_kkt`` for the one column of ``plan``'s finished block with the used scale in the face powers."""
        lib = self.ctx._lib
        return self.thermal._solve(lambda *a: lib.padne_coupled_solve_kkt(self.ctx._h, self._h, plan._h, *a), 1, heat, rtol,
                                   max_iter, precond, download)

    def update_transient(self, transient: "Transient", col: int = 0) -> float:
        """``update`` reading column ``col`` of ``transient``'s state on the device (include/padne_hip.h, "transient
        electro-thermal"): the largest change of a face mean [K]."""
        d = C.c_double()
        _check(self.ctx._lib.padne_coupled_update_transient(self.ctx._h, self._h, transient._h, int(col), C.byref(d)))
        return d.value

    def transient_load(self, transient: "Transient", plan: "KktPlan", slot: int, heat=None) -> np.ndarray:
        """Slot ``slot`` of ``transient``'s load table from the one column of ``plan``'s finished block, with the used scale in
        the face powers, the node-heat triples ``heat`` (columns 0) and the thermal handle's heat sources: the load
        ``solve_kkt`` forms.  Returns the copper heat of every mesh (n_mesh,) [W]."""
        node, col, val = Thermal._heat(heat)
        out = np.empty(transient.n_mesh, dtype=np.float64)
        _check(self.ctx._lib.padne_coupled_transient_load(self.ctx._h, self._h, transient._h, plan._h, int(slot), node.shape[0],
                                                          _ptr(node, _PI64), _ptr(col, _PI32), _ptr(val, _PF64), transient.n_mesh,
                                                          _ptr(out, _PF64)))
        return out

    def scale_range(self) -> tuple:
        """(the smallest, the largest) used scale over the faces."""
        lo, hi = C.c_double(), C.c_double()
        _check(self.ctx._lib.padne_coupled_scale_range(self.ctx._h, self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    def power_density(self, plan: "KktPlan", n_tri: int) -> np.ndarray:
        """``KktPlan.power_density_block(1, n_tri)[0]`` times the used scale, on the device."""
        out = np.empty(int(n_tri), dtype=np.float64)
        _check(self.ctx._lib.padne_coupled_power_density(self.ctx._h, self._h, plan._h, _ptr(out, _PF64)))
        return out


class ThermalSensitivities:
    """``padne_tsens``: the adjoints of temperature objectives on a solved :class:`Thermal` handle and the plan whose
    finished block holds the load cases' potentials (include/padne_hip.h, "temperature sensitivities").  ``kappa`` per mesh,
    as the thermal handle was made with.  The calls follow one another: ``thermal_adjoints``, ``electrical_rhs``, the plan's
    ``solve_block_dev`` and ``finish_block``, then ``faces``; ``vertices``, ``pairs`` and ``sources`` need the thermal
    adjoints only."""

    KIND_POINT, KIND_UNKNOWNS, KIND_SOURCE = 0, 1, 2

    def __init__(self, thermal: "Thermal", plan: "KktPlan", n_cases: int, kappa):
        self.ctx, self.thermal, self.plan = thermal.ctx, thermal, plan
        kap = _f64(kappa).reshape(-1)
        h = _P()
        _check(self.ctx._lib.padne_tsens_create(self.ctx._h, thermal._h, plan._h, int(n_cases), kap.shape[0], _ptr(kap, _PF64),
                                                C.byref(h)))
        self._h = h
        self.n_cases, self.n_obj = int(n_cases), 0

    def close(self):
        if getattr(self, "_h", None) and self.ctx._h:
            self.ctx._lib.padne_tsens_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def thermal_adjoints(self, case, kind, arg, xy, unknown, weight, mesh_layer, probes=(), *, rtol=1e-12, max_iter=200000,
                         precond="amg"):
        """lambda of the objectives: ``case``, ``kind`` and ``arg`` (n_obj,), ``xy`` (n_obj, 2), ``unknown`` and ``weight``
        (n_obj, 3) as the header states them.  Returns (unknown (n_obj, 3) int64 and weight (n_obj, 3) with the owners of the
        points filled in, lambda at the unknowns ``probes`` (n_obj, n_probe), SolveResult)."""
        case, kind, arg = _i32(case).reshape(-1), _i32(kind).reshape(-1), _i32(arg).reshape(-1)
        n_obj = case.shape[0]
        xy = _f64(xy).reshape(n_obj, 2)
        unknown, weight = np.array(unknown, dtype=np.int64).reshape(n_obj, 3), np.array(weight, dtype=np.float64).reshape(n_obj, 3)
        if not (kind.shape == arg.shape == case.shape):
            raise ValueError("case, kind and arg must list the same objectives")
        ml, pidx = _i32(mesh_layer).reshape(-1), _i64(list(probes))
        out = np.zeros((n_obj, max(pidx.shape[0], 1)), dtype=np.float64)
        opts = CsrMatrix._opts(rtol, 0.0, max_iter, 0, False, precond=precond)
        info = SolveInfo()
        self.n_obj = 0
        rc = self.ctx._lib.padne_tsens_thermal_adjoints(
            self.ctx._h, self._h, n_obj, _ptr(case, _PI32), _ptr(kind, _PI32), _ptr(arg, _PI32), _ptr(xy, _PF64),
            _ptr(unknown, _PI64), _ptr(weight, _PF64), ml.shape[0], _ptr(ml, _PI32), pidx.shape[0], _ptr(pidx, _PI64),
            _ptr(out, _PF64), C.byref(opts), C.byref(info))
        if rc != OK and rc != E_NOTCONVERGED:
            _check(rc)
        self.n_obj = n_obj
        res = SolveResult(None, info.iterations, info.restarts, info.rel_residual, info.abs_residual, info.solve_seconds,
                          info.status, info.spmv_seconds, info.precond_setup_seconds, info.operator_complexity, info.levels,
                          info.precond_fallbacks)
        return unknown, weight, out[:, :pidx.shape[0]], res

    def electrical_rhs(self, res_a=(), res_b=(), res_R=()) -> int:
        """The right-hand sides of the electrical adjoints, formed on the device; the resistors (terminals as unknowns,
        resistance) with element heat, none without.  Returns the address of the block (N, n_obj) for ``solve_block_dev``."""
        a, b, R = _i64(res_a).reshape(-1), _i64(res_b).reshape(-1), _f64(res_R).reshape(-1)
        if not (a.shape == b.shape == R.shape):
            raise ValueError("res_a, res_b and res_R must list the same resistors")
        out = _P()
        _check(self.ctx._lib.padne_tsens_electrical_rhs(self.ctx._h, self._h, self.n_obj, a.shape[0], _ptr(a, _PI64),
                                                        _ptr(b, _PI64), _ptr(R, _PF64), C.byref(out)))
        return int(out.value)

    def faces(self, n_tri: int, n_mesh: int):
        """(e_f / area, k_f / area, (e_f + k_f) / area, each (n_obj, n_tri); the per-mesh sums of e_f and of k_f, each (n_obj,
        n_mesh)), after the plan's ``finish_block`` of the electrical adjoints."""
        n_tri, n_mesh, n_obj = int(n_tri), int(n_mesh), self.n_obj
        e, k, c = (np.empty((n_obj, n_tri), dtype=np.float64) for _ in range(3))
        me, mk = (np.empty((n_obj, n_mesh), dtype=np.float64) for _ in range(2))
        _check(self.ctx._lib.padne_tsens_faces(self.ctx._h, self._h, n_obj, n_tri, n_mesh, _ptr(e, _PF64), _ptr(k, _PF64),
                                               _ptr(c, _PF64), _ptr(me, _PF64), _ptr(mk, _PF64)))
        return e, k, c, me, mk

    def vertices(self, n_mesh: int) -> np.ndarray:
        """film dT/dfilm of every mesh, (n_obj, n_mesh)."""
        out = np.empty((self.n_obj, int(n_mesh)), dtype=np.float64)
        _check(self.ctx._lib.padne_tsens_vertices(self.ctx._h, self._h, self.n_obj, int(n_mesh), _ptr(out, _PF64)))
        return out

    def pairs(self) -> np.ndarray:
        """g dT/dg of every pair of the stacked thermal handle, (n_obj, n_pair)."""
        out = np.zeros((self.n_obj, self.thermal.n_pair), dtype=np.float64)
        _check(self.ctx._lib.padne_tsens_pairs(self.ctx._h, self._h, self.n_obj, self.thermal.n_pair, _ptr(out, _PF64)))
        return out

    def sources(self) -> np.ndarray:
        """dT/dP of every heat source of the thermal handle, (n_obj, n_source)."""
        out = np.zeros((self.n_obj, self.thermal.n_source), dtype=np.float64)
        _check(self.ctx._lib.padne_tsens_sources(self.ctx._h, self._h, self.n_obj, self.thermal.n_source, _ptr(out, _PF64)))
        return out


class Sampler:
    """``padne_sampler``: meshes, potentials and a point-location index per layer, resident on the device until ``close``
    (include/padne_hip.h, "field sampler").  Queries return (face (n,) int32 global face or -1, V (n,), J (n, 2), p (n,))."""

    def __init__(self, ctx: "Context", xy, tri, mesh_vertex_offset, mesh_tri_offset, mesh_layer, conductance, n_layer: int,
                 potential, bins_hint: int = 0):
        xy, tri = _f64(xy).reshape(-1, 2), _i32(tri).reshape(-1, 3)
        mvo, mto, ml, sig = _i64(mesh_vertex_offset), _i64(mesh_tri_offset), _i32(mesh_layer).reshape(-1), _f64(conductance)
        pot = _f64(potential).reshape(-1)
        n_mesh = ml.shape[0]
        if mvo.shape[0] != n_mesh + 1 or mto.shape[0] != n_mesh + 1 or sig.shape[0] != n_mesh:
            raise ValueError("offset tables must have n_mesh+1 entries and every mesh a conductance")
        if pot.shape[0] != xy.shape[0]:
            raise ValueError("one potential per vertex")
        self.ctx, self.n_layer = ctx, int(n_layer)
        self.n_vert, self.n_mesh, self.n_field = int(xy.shape[0]), int(n_mesh), 0
        h = _P()
        _check(ctx._lib.padne_sampler_create(ctx._h, xy.shape[0], _ptr(xy, _PF64), tri.shape[0], _ptr(tri, _PI32), n_mesh,
                                             _ptr(mvo, _PI64), _ptr(mto, _PI64), _ptr(ml, _PI32), _ptr(sig, _PF64), int(n_layer),
                                             _ptr(pot, _PF64), int(bins_hint), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and self.ctx._h:
            self.ctx._lib.padne_sampler_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _outputs(n: int):
        return (np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float64), np.empty((n, 2), dtype=np.float64),
                np.empty(n, dtype=np.float64))

    def points(self, layer: int, xy):
        q = _f64(xy).reshape(-1, 2)
        face, v, j, p = self._outputs(q.shape[0])
        _check(self.ctx._lib.padne_sampler_points(self.ctx._h, self._h, int(layer), q.shape[0], _ptr(q, _PF64),
                                                  _ptr(face, _PI32), _ptr(v, _PF64), _ptr(j, _PF64), _ptr(p, _PF64)))
        return face, v, j, p

    def raster(self, layer: int, x0: float, y0: float, dx: float, dy: float, width: int, height: int):
        """Row j, column i of the raster at index j * width + i of the flat results."""
        n = max(int(width), 0) * max(int(height), 0)
        face, v, j, p = self._outputs(n)
        _check(self.ctx._lib.padne_sampler_raster(self.ctx._h, self._h, int(layer), float(x0), float(y0), float(dx), float(dy),
                                                  int(width), int(height), _ptr(face, _PI32), _ptr(v, _PF64), _ptr(j, _PF64),
                                                  _ptr(p, _PF64)))
        return face, v, j, p

    def stats(self, layer: int) -> dict:
        """Of ``layer``: bins along x and y, list entries, faces; of the last query call: candidate faces tested, queries,
        device seconds of its kernel; of the creation: host seconds of the upload and of the index build."""
        counts = np.zeros(6, dtype=np.int64)
        secs = np.zeros(3, dtype=np.float64)
        _check(self.ctx._lib.padne_sampler_stats(self._h, int(layer), _ptr(counts, _PI64), _ptr(secs, _PF64)))
        return {"bins_x": int(counts[0]), "bins_y": int(counts[1]), "entries": int(counts[2]), "faces": int(counts[3]),
                "last_candidates": int(counts[4]), "last_queries": int(counts[5]), "upload_seconds": float(secs[0]),
                "build_seconds": float(secs[1]), "last_kernel_seconds": float(secs[2])}

    # ---- thermal images: a block of fields on the same handle (include/padne_hip.h, "thermal images")

    def set_fields(self, fields, kappa=None) -> None:
        """``fields`` (n_field, n_vert) replaces the handle's block, (0, n_vert) or None removes it; ``kappa`` (n_mesh,) the
        sheet conductances of the heat flux, None for none."""
        block = _f64(np.zeros((0, 0)) if fields is None else fields)
        if block.ndim != 2:
            raise ValueError("fields must have shape (n_field, n_vert)")
        if block.shape[0] and block.shape[1] != self.n_vert:
            raise ValueError("every field has one value per vertex")
        kap = None if kappa is None else _f64(kappa).reshape(-1)
        if kap is not None and kap.shape[0] != self.n_mesh:
            raise ValueError("every mesh has a sheet conductance")
        _check(self.ctx._lib.padne_sampler_set_fields(self.ctx._h, self._h, block.shape[0], _ptr(block, _PF64),
                                                      None if kap is None else _ptr(kap, _PF64)))
        self.n_field = int(block.shape[0])

    def _field_outputs(self, n: int, per_field: bool, flux: bool):
        f = self.n_field
        return (np.empty(n, dtype=np.int32), np.empty((f, n), dtype=np.float64) if per_field else None,
                np.empty((f, n, 2), dtype=np.float64) if flux else None, np.empty(n, dtype=np.float64),
                np.empty(n, dtype=np.int32))

    def field_points(self, layer: int, xy, per_field: bool = True, flux: bool = False):
        """(face (n,), T (n_field, n) or None, q (n_field, n, 2) or None, hottest (n,), hottest field (n,) int32)."""
        q = _f64(xy).reshape(-1, 2)
        face, t, flx, hot, hot_field = self._field_outputs(q.shape[0], per_field, flux)
        _check(self.ctx._lib.padne_sampler_field_points(
            self.ctx._h, self._h, int(layer), q.shape[0], _ptr(q, _PF64), _ptr(face, _PI32),
            None if t is None else _ptr(t, _PF64), None if flx is None else _ptr(flx, _PF64), _ptr(hot, _PF64),
            _ptr(hot_field, _PI32)))
        return face, t, flx, hot, hot_field

    def field_raster(self, layer: int, x0: float, y0: float, dx: float, dy: float, width: int, height: int,
                     per_field: bool = True, flux: bool = False):
        """The five of ``field_points`` with row j, column i at j * width + i, then the tops of the n_field + 1 slots: the
        values (n_field + 1,) and their flat pixels (n_field + 1,) int64, -inf and -1 for a slot without a pixel on copper."""
        n = max(int(width), 0) * max(int(height), 0)
        face, t, flx, hot, hot_field = self._field_outputs(n, per_field, flux)
        slots = self.n_field + 1
        top, top_pixel = np.empty(slots, dtype=np.float64), np.empty(slots, dtype=np.int64)
        _check(self.ctx._lib.padne_sampler_field_raster(
            self.ctx._h, self._h, int(layer), float(x0), float(y0), float(dx), float(dy), int(width), int(height),
            _ptr(face, _PI32), None if t is None else _ptr(t, _PF64), None if flx is None else _ptr(flx, _PF64),
            _ptr(hot, _PF64), _ptr(hot_field, _PI32), _ptr(top, _PF64), _ptr(top_pixel, _PI64)))
        return face, t, flx, hot, hot_field, top, top_pixel


def refine(ctx: "Context", xy, tri, mesh_vertex_offset, mesh_tri_offset, flags):
    """One refinement round (include/padne_hip.h, ``padne_refine_create`` / ``_fetch`` / ``_destroy``) of meshes given as
    ``power_density`` takes them, ``flags`` one uint8 per face.  Returns (xy (n, 2), tri (k, 3) and parent (k,) with
    mesh-local indices, ends (n_new, 2) mesh-local, vertex counts and face counts per mesh, and the counts dict: edges,
    edges marked by the flags, edges marked after the closure, closure sweeps queued)."""
    xy, tri = _f64(xy).reshape(-1, 2), _i32(tri).reshape(-1, 3)
    mvo, mto = _i64(mesh_vertex_offset), _i64(mesh_tri_offset)
    flag = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
    n_mesh = mvo.shape[0] - 1
    if n_mesh < 1 or mto.shape[0] != n_mesh + 1:
        raise ValueError("the offset tables must have one entry more than there are meshes, and there is at least one mesh")
    if flag.shape[0] != tri.shape[0]:
        raise ValueError("one flag per face")
    n_vert_out, n_tri_out = np.zeros(n_mesh, dtype=np.int64), np.zeros(n_mesh, dtype=np.int64)
    counts = np.zeros(4, dtype=np.int64)
    h = _P()
    _check(ctx._lib.padne_refine_create(ctx._h, xy.shape[0], _ptr(xy, _PF64), tri.shape[0], _ptr(tri, _PI32), n_mesh,
                                        _ptr(mvo, _PI64), _ptr(mto, _PI64), _ptr(flag, C.POINTER(C.c_uint8)),
                                        _ptr(n_vert_out, _PI64), _ptr(n_tri_out, _PI64), _ptr(counts, _PI64), C.byref(h)))
    try:
        nv, nt = int(n_vert_out.sum()), int(n_tri_out.sum())
        xy_out = np.empty((nv, 2), dtype=np.float64)
        tri_out, parent = np.empty((nt, 3), dtype=np.int32), np.empty(nt, dtype=np.int32)
        ends = np.empty((nv - xy.shape[0], 2), dtype=np.int32)
        _check(ctx._lib.padne_refine_fetch(ctx._h, h, _ptr(xy_out, _PF64), _ptr(tri_out, _PI32), _ptr(parent, _PI32),
                                           _ptr(ends, _PI32)))
    finally:
        ctx._lib.padne_refine_destroy(h)
    return xy_out, tri_out, parent, ends, n_vert_out, n_tri_out, {
        "edges": int(counts[0]), "marked_by_flags": int(counts[1]), "marked": int(counts[2]), "sweeps": int(counts[3])}


def polymesh(ctx: "Context", polygons, h: float, snap: float = 0.25):
    """One batch of the grid mesher (include/padne_hip.h, ``padne_polymesh_create`` / ``_fetch`` / ``_destroy``).
    ``polygons``: a sequence of polygons, each a sequence of rings (the exterior first), each ring an (n, 2) array without a
    closing duplicate.  Returns a list of (xy (n, 2) float64, tri (k, 3) int32, kind (n,) int32), one per polygon."""
    rings = [_f64(r).reshape(-1, 2) for poly in polygons for r in poly]
    poly_ring_ptr = _i64(np.concatenate([[0], np.cumsum([len(poly) for poly in polygons])]))
    ring_ptr = _i64(np.concatenate([[0], np.cumsum([len(r) for r in rings])]))
    ring_xy = _f64(np.concatenate(rings)) if rings else np.zeros((0, 2))
    n_poly = len(polygons)
    n_vert, n_tri = np.zeros(max(n_poly, 1), dtype=np.int64), np.zeros(max(n_poly, 1), dtype=np.int64)
    h_ = _P()
    _check(ctx._lib.padne_polymesh_create(ctx._h, n_poly, _ptr(poly_ring_ptr, _PI64), _ptr(ring_ptr, _PI64), _ptr(ring_xy, _PF64),
                                          float(h), float(snap), _ptr(n_vert, _PI64), _ptr(n_tri, _PI64), C.byref(h_)))
    try:
        nv, nt = int(n_vert.sum()), int(n_tri.sum())
        xy, tri, kind = np.empty((nv, 2), dtype=np.float64), np.empty((nt, 3), dtype=np.int32), np.empty(nv, dtype=np.int32)
        _check(ctx._lib.padne_polymesh_fetch(ctx._h, h_, _ptr(xy, _PF64), _ptr(tri, _PI32), _ptr(kind, _PI32)))
    finally:
        ctx._lib.padne_polymesh_destroy(h_)
    vo, to = np.concatenate([[0], np.cumsum(n_vert)]), np.concatenate([[0], np.cumsum(n_tri)])
    return [(xy[vo[p]:vo[p + 1]], tri[to[p]:to[p + 1]], kind[vo[p]:vo[p + 1]]) for p in range(n_poly)]


def polymesh_graded(ctx: "Context", polygons, h: float, snap: float = 0.25, thresholds=(0,), seeds=()):
    """One batch of the graded grid mesher (include/padne_hip.h, ``padne_polymesh_create_graded``).  ``polygons`` as
    :func:`polymesh`; ``thresholds``: ``t[0] = 0 < t[1] < ...`` in cells, at most 6, ``t[l] >= t[l - 1] + 2^(l - 1)``;
    ``seeds``: (n, 2) fine spots, applied to every polygon.  Returns a list of (xy, tri, kind, cells_per_level) per polygon,
    the first three as :func:`polymesh`, the last the lattice's cells by level (int64, one entry per threshold)."""
    rings = [_f64(r).reshape(-1, 2) for poly in polygons for r in poly]
    poly_ring_ptr = _i64(np.concatenate([[0], np.cumsum([len(poly) for poly in polygons])]))
    ring_ptr = _i64(np.concatenate([[0], np.cumsum([len(r) for r in rings])]))
    ring_xy = _f64(np.concatenate(rings)) if rings else np.zeros((0, 2))
    t = np.asarray(thresholds).reshape(-1)
    if len(t) and not (np.issubdtype(t.dtype, np.integer) and t.min() >= -2 ** 31 and t.max() < 2 ** 31):
        raise ValueError("the thresholds are 32-bit integers")
    t = _i32(t) if len(t) else np.zeros(1, dtype=np.int32)
    n_level = len(np.asarray(thresholds).reshape(-1))
    seed_xy = _f64(seeds).reshape(-1, 2)
    n_poly = len(polygons)
    n_vert, n_tri = np.zeros(max(n_poly, 1), dtype=np.int64), np.zeros(max(n_poly, 1), dtype=np.int64)
    cells = np.zeros((max(n_poly, 1), max(n_level, 1)), dtype=np.int64)
    h_ = _P()
    _check(ctx._lib.padne_polymesh_create_graded(ctx._h, n_poly, _ptr(poly_ring_ptr, _PI64), _ptr(ring_ptr, _PI64), _ptr(ring_xy, _PF64),
                                                 float(h), float(snap), n_level, _ptr(t, _PI32), len(seed_xy),
                                                 _ptr(seed_xy, _PF64) if len(seed_xy) else None, _ptr(n_vert, _PI64),
                                                 _ptr(n_tri, _PI64), _ptr(cells, _PI64), C.byref(h_)))
    try:
        nv, nt = int(n_vert.sum()), int(n_tri.sum())
        xy, tri, kind = np.empty((nv, 2), dtype=np.float64), np.empty((nt, 3), dtype=np.int32), np.empty(nv, dtype=np.int32)
        _check(ctx._lib.padne_polymesh_fetch(ctx._h, h_, _ptr(xy, _PF64), _ptr(tri, _PI32), _ptr(kind, _PI32)))
    finally:
        ctx._lib.padne_polymesh_destroy(h_)
    vo, to = np.concatenate([[0], np.cumsum(n_vert)]), np.concatenate([[0], np.cumsum(n_tri)])
    return [(xy[vo[p]:vo[p + 1]], tri[to[p]:to[p + 1]], kind[vo[p]:vo[p + 1]], cells[p]) for p in range(n_poly)]


def _groups(groups, n: int, what: str) -> np.ndarray:
    g = np.asarray(groups).reshape(-1)
    if len(g) != n:
        raise ValueError(f"one group per {what}: {len(g)} groups for {n}")
    if len(g) and not (np.issubdtype(g.dtype, np.integer) and g.min() >= -2 ** 31 and g.max() < 2 ** 31):
        raise ValueError("the groups are 32-bit integers")
    return _i32(g)


def locate_polygons(ctx: "Context", polygons, groups, points, point_groups):
    """The connectivity pre-pass's kernel (include/padne_hip.h, ``padne_polygons_locate`` / ``_fetch`` / ``_destroy``): which
    polygons does every point touch.  ``polygons`` as :func:`polymesh`; ``groups``: the group (layer) of every polygon,
    ascending; ``points``: (n, 2); ``point_groups``: the group of every point, which meets the polygons of its group only.
    Returns (hit_ptr (n + 1,) int64, hit_poly int32, hit_kind int32): the hits of point q are
    ``hit_ptr[q] .. hit_ptr[q + 1]``, in ascending polygon number; kind 1 inside, 2 on the boundary."""
    rings = [_f64(r).reshape(-1, 2) for poly in polygons for r in poly]
    poly_ring_ptr = _i64(np.concatenate([[0], np.cumsum([len(poly) for poly in polygons])]))
    ring_ptr = _i64(np.concatenate([[0], np.cumsum([len(r) for r in rings])]))
    ring_xy = _f64(np.concatenate(rings)) if rings else np.zeros((0, 2))
    n_poly = len(polygons)
    xy = _f64(points).reshape(-1, 2)
    n_query = len(xy)
    pg, qg = _groups(groups, n_poly, "polygon"), _groups(point_groups, n_query, "point")
    n_hit = C.c_int64(0)
    h_ = _P()
    _check(ctx._lib.padne_polygons_locate(ctx._h, n_poly, _ptr(poly_ring_ptr, _PI64), _ptr(ring_ptr, _PI64), _ptr(ring_xy, _PF64),
                                          _ptr(pg, _PI32), n_query, _ptr(xy, _PF64), _ptr(qg, _PI32), C.byref(n_hit), C.byref(h_)))
    try:
        hit_ptr = np.empty(n_query + 1, dtype=np.int32)
        hit_poly, hit_kind = np.empty(n_hit.value, dtype=np.int32), np.empty(n_hit.value, dtype=np.int32)
        _check(ctx._lib.padne_polygons_locate_fetch(ctx._h, h_, _ptr(hit_ptr, _PI32), _ptr(hit_poly, _PI32), _ptr(hit_kind, _PI32)))
    finally:
        ctx._lib.padne_polygons_locate_destroy(h_)
    return hit_ptr.astype(np.int64), hit_poly, hit_kind


class CsrMatrix:
    """Device-resident CSR matrix (opaque handle of the C ABI)."""

    def __init__(self, ctx: Context, handle):
        self.ctx = ctx
        self._h = handle
        nr, nc, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        _check(ctx._lib.padne_csr_shape(handle, C.byref(nr), C.byref(nc), C.byref(nnz)))
        self.shape = (nr.value, nc.value)
        self.nnz = nnz.value

    def close(self):
        if getattr(self, "_h", None) and self.ctx._h and not getattr(self, "_borrowed", False):
            self.ctx._lib.padne_csr_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def spmv_bytes(self) -> int:
        return int(self.ctx._lib.padne_spmv_algorithmic_bytes(self._h))

    def to_scipy(self):
        import scipy.sparse as sp
        indptr = np.empty(self.shape[0] + 1, dtype=np.int32)
        indices = np.empty(self.nnz, dtype=np.int32)
        data = np.empty(self.nnz, dtype=np.float64)
        _check(self.ctx._lib.padne_csr_to_host(self.ctx._h, self._h, _ptr(indptr, _PI32), _ptr(indices, _PI32),
                                               _ptr(data, _PF64)))
        return sp.csr_matrix((data, indices, indptr), shape=self.shape)

    def reduce(self, index_map, n_out: int, scale: float = 1.0) -> "CsrMatrix":
        """``scale * P^T M P``.  ``index_map``: a host array, or a ``DeviceArray`` of int32 already on this GPU (the
        library reads a device-resident map where it lies: no upload per call)."""
        if isinstance(index_map, DeviceArray):
            if index_map.dtype != np.int32 or int(np.prod(index_map.shape)) != self.shape[0]:
                raise ValueError("index map must be int32 of the matrix dimension")
            mp = C.cast(_P(index_map.ptr), _PI32)
        else:
            m = _i32(index_map)
            if m.shape[0] != self.shape[0]:
                raise ValueError("index map length must equal the matrix dimension")
            mp = _ptr(m, _PI32)
        h = _P()
        _check(self.ctx._lib.padne_csr_reduce(self.ctx._h, self._h, mp, int(n_out), float(scale), C.byref(h)))
        return CsrMatrix(self.ctx, h)

    def relabel(self, row_map: np.ndarray, n_rows_out: int, col_map: np.ndarray, n_cols_out: int,
                scale: float = 1.0) -> "CsrMatrix":
        """``scale * R^T M C`` with separate row / column index maps (-1 drops the row / column)."""
        rm = np.ascontiguousarray(row_map, dtype=np.int32)
        cm = np.ascontiguousarray(col_map, dtype=np.int32)
        if rm.shape[0] != self.shape[0] or cm.shape[0] != self.shape[1]:
            raise ValueError("index map lengths must equal the matrix dimensions")
        h = _P()
        _check(self.ctx._lib.padne_csr_relabel(self.ctx._h, self._h, _ptr(rm, _PI32), int(n_rows_out), _ptr(cm, _PI32),
                                               int(n_cols_out), float(scale), C.byref(h)))
        return CsrMatrix(self.ctx, h)

    def power_density(self, potential: np.ndarray, n_tri: int) -> np.ndarray:
        """Per-triangle power density on the mesh this system was assembled from (kept on the device with it)."""
        pot = _f64(potential)
        out = np.empty(int(n_tri), dtype=np.float64)
        _check(self.ctx._lib.padne_csr_power_density(self.ctx._h, self._h, _ptr(pot, _PF64), _ptr(out, _PF64)))
        return out

    def vstack(self, bottom: "CsrMatrix") -> "CsrMatrix":
        h = _P()
        _check(self.ctx._lib.padne_csr_vstack(self.ctx._h, self._h, bottom._h, C.byref(h)))
        return CsrMatrix(self.ctx, h)

    def matvec(self, x) -> np.ndarray:
        x = _f64(x)
        if x.shape[0] != self.shape[1]:
            raise ValueError("dimension mismatch")
        y = np.empty(self.shape[0], dtype=np.float64)
        _check(self.ctx._lib.padne_spmv(self.ctx._h, self._h, _ptr(x, _PF64), _ptr(y, _PF64)))
        return y

    def matvec_dev(self, x: DeviceArray, y: DeviceArray, repeat: int = 1):
        _check(self.ctx._lib.padne_spmv_dev(self.ctx._h, self._h, _P(x.ptr), _P(y.ptr), int(repeat)))

    def spmv_time(self, x: DeviceArray, y: DeviceArray, warmup: int = 5, repeat: int = 50) -> float:
        t = C.c_double()
        _check(self.ctx._lib.padne_spmv_time(self.ctx._h, self._h, _P(x.ptr), _P(y.ptr), warmup, repeat,
                                             C.byref(t)))
        return t.value

    def matmat8_dev(self, x: DeviceArray, y: DeviceArray, repeat: int = 1):
        """Y = M X for 8 interleaved vectors: x holds shape[1]*8 doubles laid out [i][j], y shape[0]*8."""
        if x.nbytes != self.shape[1] * 64 or y.nbytes != self.shape[0] * 64:
            raise ValueError("dimension mismatch")
        _check(self.ctx._lib.padne_spmm8_dev(self.ctx._h, self._h, _P(x.ptr), _P(y.ptr), int(repeat)))

    def matmat8(self, X) -> np.ndarray:
        """Host convenience: X (n_cols, 8) -> M @ X (n_rows, 8)."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.shape != (self.shape[1], 8):
            raise ValueError("X must have shape (n_cols, 8)")
        xd = self.ctx.to_device(X.reshape(-1))
        yd = self.ctx.empty(self.shape[0] * 8)
        self.matmat8_dev(xd, yd)
        return yd.numpy().reshape(self.shape[0], 8)

    def spmm8_time(self, x: DeviceArray, y: DeviceArray, warmup: int = 5, repeat: int = 50) -> float:
        t = C.c_double()
        _check(self.ctx._lib.padne_spmm8_time(self.ctx._h, self._h, _P(x.ptr), _P(y.ptr), warmup, repeat,
                                              C.byref(t)))
        return t.value

    @property
    def spmm8_bytes(self) -> int:
        return int(self.ctx._lib.padne_spmm8_algorithmic_bytes(self._h))

    def residual_norm(self, x, b) -> float:
        x, b = _f64(x), _f64(b)
        out = C.c_double()
        _check(self.ctx._lib.padne_residual_norm(self.ctx._h, self._h, _ptr(x, _PF64), _ptr(b, _PF64),
                                                 C.byref(out)))
        return out.value

    def set_preconditioner_block(self, block: "CsrMatrix | None") -> None:
        """Row-partitioned runs: multigrid is built on this owned x owned diagonal block."""
        _check(self.ctx._lib.padne_csr_set_preconditioner_block(self._h, block._h if block is not None else None))
        self._prec_block = block        # keep it alive

    def amg_level(self, level: int, which: str = "A"):
        """scipy copy of a hierarchy operator: which in 'A', 'P', 'R'."""
        import scipy.sparse as sp
        h = _P()
        _check(self.ctx._lib.padne_amg_level(self.ctx._h, self._h, int(level), {"A": 0, "P": 1, "R": 2}[which], C.byref(h)))
        nr, nc, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        _check(self.ctx._lib.padne_csr_shape(h, C.byref(nr), C.byref(nc), C.byref(nnz)))
        indptr = np.empty(nr.value + 1, dtype=np.int32)
        indices = np.empty(nnz.value, dtype=np.int32)
        data = np.empty(nnz.value, dtype=np.float64)
        _check(self.ctx._lib.padne_csr_to_host(self.ctx._h, h, _ptr(indptr, _PI32), _ptr(indices, _PI32), _ptr(data, _PF64)))
        return sp.csr_matrix((data, indices, indptr), shape=(nr.value, nc.value))

    def amg_shapes(self):
        """(rows, cols, nnz) of every operator of the cached hierarchy, level by level: [{"A": .., "P": .., "R": ..}, ...]
        (the last level has only "A").  Shapes only, nothing is downloaded."""
        out = []
        for level in range(32):
            entry = {}
            for which, code in (("A", 0), ("P", 1), ("R", 2)):
                h = _P()
                if self.ctx._lib.padne_amg_level(self.ctx._h, self._h, level, code, C.byref(h)) != OK:
                    continue
                nr, nc, nnz = C.c_int64(), C.c_int64(), C.c_int64()
                _check(self.ctx._lib.padne_csr_shape(h, C.byref(nr), C.byref(nc), C.byref(nnz)))
                entry[which] = (nr.value, nc.value, nnz.value)
            if "A" not in entry:
                break
            out.append(entry)
        return out

    def split_tiles(self, level: int = -1):
        """(interior, boundary) 64-row tiles of the split plan of this row-partitioned operator (level >= 0: of the
        level operator of its hierarchy); (0, 0) without one.  Test-only introspection."""
        a, b = C.c_int64(), C.c_int64()
        _check(self.ctx._lib.padne_csr_split_tiles(self._h, int(level), C.byref(a), C.byref(b)))
        return a.value, b.value

    AMG_STATE = {"AGG": (0, np.int32), "ROOT": (1, np.int8), "SCALARS": (2, np.float64), "EXPORT": (3, np.int32),
                 "HALO": (4, np.int64)}

    def amg_state(self, level: int, which: str) -> np.ndarray:
        """TEST-ONLY (``padne_test_amg_state``): what level ``level`` of the cached hierarchy decided in its setup -- "AGG",
        "ROOT" (both kept only under PADNE_AMG_KEEP=1), "SCALARS" = (lambda, jac, has W, single precision) or, on a level of
        a row-partitioned hierarchy, "EXPORT" (the exported owned vertices) and "HALO" = (m, n_export, tail_n, tail_off)."""
        sel, dtype = self.AMG_STATE[which]
        if which in ("SCALARS", "HALO"):
            n = 4
        elif which == "EXPORT":
            n = int(self.amg_state(level, "HALO")[1])
        else:
            n = self.amg_shapes()[int(level)]["A"][0]
        out = np.empty(n, dtype=dtype)
        _check(self.ctx._lib.padne_test_amg_state(self.ctx._h, self._h, int(level), sel, out.ctypes.data_as(_P), out.nbytes))
        return out

    def amg_tail(self) -> "CsrMatrix":
        """TEST-ONLY (``padne_test_amg_tail``): the gathered operator of this matrix's row-partitioned hierarchy, as a
        borrowed handle -- it belongs to the hierarchy and is not destroyed with the wrapper."""
        h = _P()
        _check(self.ctx._lib.padne_test_amg_tail(self._h, C.byref(h)))
        t = CsrMatrix(self.ctx, h)
        t._borrowed = True
        t._lender = self             # the hierarchy lives as long as its matrix
        return t

    def amg_apply_dist(self, r) -> np.ndarray:
        """TEST-ONLY (``padne_test_amg_apply_dist``): z = M^-1 r on this rank's rows, one cycle of the row-partitioned
        hierarchy (collective)."""
        r = _f64(r)
        if r.shape != (self.shape[0],):
            raise ValueError("dimension mismatch")
        z = np.empty_like(r)
        _check(self.ctx._lib.padne_test_amg_apply_dist(self.ctx._h, self._h, _ptr(r, _PF64), _ptr(z, _PF64)))
        return z

    def amg_apply(self, r) -> np.ndarray:
        """z = M^-1 r: one multigrid V-cycle (the preconditioner of solve_spd)."""
        r = _f64(r)
        if r.shape[0] != self.shape[0]:
            raise ValueError("dimension mismatch")
        z = np.empty_like(r)
        _check(self.ctx._lib.padne_amg_apply(self.ctx._h, self._h, _ptr(r, _PF64), _ptr(z, _PF64)))
        return z

    def amg_apply_batch(self, R, unit2=None) -> np.ndarray:
        """Z[k, n] = the batched cycle of the lockstep loops on R[k, n] (k = 2, 4 or 8), column j in units of
        sqrt(unit2[j]) (0 / None: as it is)."""
        R = _f64(R)
        if R.ndim != 2 or R.shape[1] != self.shape[0] or R.shape[0] not in (2, 4, 8):
            raise ValueError("R must be [2 | 4 | 8, n]")
        u2 = np.zeros(R.shape[0]) if unit2 is None else _f64(unit2)
        if u2.shape != (R.shape[0],):
            raise ValueError("one unit per column")
        Z = np.empty_like(R)
        _check(self.ctx._lib.padne_amg_apply_batch(self.ctx._h, self._h, R.shape[0], _ptr(R, _PF64), _ptr(u2, _PF64),
                                                   _ptr(Z, _PF64)))
        return Z

    @staticmethod
    def _opts(rtol, atol, max_iter, check_every, guess, time_spmv=False, precond="jacobi", rebuild=False) -> SolveOpts:
        pc = {"jacobi": 0, "amg": 1, 0: 0, 1: 1}[precond]
        return SolveOpts(float(rtol), float(atol), int(max_iter), pc, int(check_every),
                         (1 if guess else 0) | (2 if time_spmv else 0) | (4 if rebuild else 0))

    def solve_spd(self, b, *, rtol=1e-12, atol=0.0, max_iter=200000, check_every=0, x0=None,
                  raise_on_fail=True, precond="amg", rebuild=False) -> SolveResult:
        """Jacobi-PCG on the device; b is host f64[n] or f64[k, n]."""
        b = _f64(b)
        n = self.shape[0] if self.ctx.halo_n_owned is None else self.ctx.halo_n_owned
        k = 1 if b.ndim == 1 else b.shape[0]
        if b.shape[-1] != n:
            raise ValueError("right-hand side has the wrong length")
        x = np.empty_like(b) if x0 is None else _f64(x0).copy()      # (no guess: the device starts from zero and writes all of x)
        opts = self._opts(rtol, atol, max_iter, check_every, x0 is not None, precond=precond, rebuild=rebuild)
        info = SolveInfo()
        rc = self.ctx._lib.padne_solve_spd(self.ctx._h, self._h, _ptr(b, _PF64), _ptr(x, _PF64), k,
                                           C.byref(opts), C.byref(info))
        if rc != OK and (raise_on_fail or rc != E_NOTCONVERGED):
            _check(rc)
        return SolveResult(x, info.iterations, info.restarts, info.rel_residual, info.abs_residual,
                           info.solve_seconds, info.status, info.spmv_seconds, info.precond_setup_seconds,
                           info.operator_complexity, info.levels, info.precond_fallbacks)

    def solve_spd_dev(self, b: DeviceArray, x: DeviceArray, *, n_rhs=1, rtol=1e-12, atol=0.0, max_iter=200000,
                      check_every=0, guess=False, raise_on_fail=True, time_spmv=False, precond="amg",
                      rebuild=False) -> SolveResult:
        opts = self._opts(rtol, atol, max_iter, check_every, guess, time_spmv, precond, rebuild)
        info = SolveInfo()
        rc = self.ctx._lib.padne_solve_spd_dev(self.ctx._h, self._h, _P(b.ptr), _P(x.ptr), int(n_rhs),
                                               C.byref(opts), C.byref(info))
        if rc != OK and (raise_on_fail or rc != E_NOTCONVERGED):
            _check(rc)
        return SolveResult(None, info.iterations, info.restarts, info.rel_residual, info.abs_residual,
                           info.solve_seconds, info.status, info.spmv_seconds, info.precond_setup_seconds,
                           info.operator_complexity, info.levels, info.precond_fallbacks)
