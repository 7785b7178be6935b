"""ctypes binding of libmghip.so (include/mghip.h).  There is no CPU fallback: a missing library,
a missing symbol or a missing device raises."""
import ctypes as C
import os

import numpy as np

from . import _build

MG_OK = 0
MG_ERR_INVALID_VALUE, MG_ERR_NO_DEVICE, MG_ERR_HIP, MG_ERR_STATE, MG_ERR_ALLOC, MG_ERR_TIMEOUT = -1, -2, -3, -4, -5, -6
MG_PLAN_PHASES = 7
PLAN_PHASE_NAMES = ("legs", "halo_copy", "halo_exchange", "coarse_allgather", "replicated_engine", "allreduce", "other")


class PlanTimeout(RuntimeError):
    """mg_plan_wait gave up (MG_ERR_TIMEOUT): the queued device work is still queued, so the process must not
    synchronise on it again -- report and leave (distributed.bench_main does, with os._exit)."""
MG_F32, MG_F64 = 0, 1
MG_JACOBI, MG_RBGS, MG_LEXGS = 0, 1, 2
MG_ZEBRA_X, MG_ZEBRA_Y, MG_ZEBRA_ALT = 3, 4, 5      # zebra line relaxation (include/mghip_line.h)
MG_CYCLE_V, MG_CYCLE_W, MG_CYCLE_F = 0, 1, 2
MG_PREC_DOUBLE, MG_PREC_SINGLE, MG_PREC_MIXED_LEVELS, MG_PREC_ADAPTIVE, MG_PREC_SINGLE_MANAGED, MG_PREC_DEFECT = 0, 1, 2, 3, 4, 5

CYCLES = {"V": MG_CYCLE_V, "W": MG_CYCLE_W, "F": MG_CYCLE_F}


class MgConfig(C.Structure):
    _fields_ = [
        ("nx", C.c_int32), ("ny", C.c_int32),
        ("x0", C.c_double), ("x1", C.c_double), ("y0", C.c_double), ("y1", C.c_double),
        ("coeff", C.c_double),
        ("max_levels", C.c_int32), ("cycle", C.c_int32), ("pre", C.c_int32), ("post", C.c_int32),
        ("smoother", C.c_int32),
        ("omega", C.c_double),
        ("coarse_tol", C.c_double), ("coarse_maxit", C.c_int32),
        ("precision", C.c_int32),
        ("switch_threshold", C.c_double), ("memory_threshold_gb", C.c_double),
        ("adaptive_reference_rule", C.c_int32),
        ("device", C.c_int32), ("profile", C.c_int32), ("colour_offset", C.c_int32), ("fused", C.c_int32),
        ("tail", C.c_int32), ("fmg_cycles", C.c_int32), ("speculate", C.c_int32), ("coarse_direct", C.c_int32),
        ("mixed_split", C.c_int32),
    ]


class MgStats(C.Structure):
    _fields_ = [
        ("solve_seconds", C.c_double), ("h2d_seconds", C.c_double), ("d2h_seconds", C.c_double),
        ("initial_residual", C.c_double),
        ("precision_switches", C.c_int32), ("last_coarse_sweeps", C.c_int32),
        ("switch_reason", C.c_int32), ("fp32_floor", C.c_double),
    ]


class MgPcgStats(C.Structure):
    """mg_pcg_stats (include/mghip.h, "Krylov outer loop")"""
    _fields_ = [("solve_seconds", C.c_double), ("precond_seconds", C.c_double), ("initial_residual", C.c_double),
                ("true_residual", C.c_double), ("iterations", C.c_int32), ("status", C.c_int32)]


class MgEigStats(C.Structure):
    """mg_eig_stats (include/mghip_eig.h)"""
    _fields_ = [("solve_seconds", C.c_double), ("precond_seconds", C.c_double), ("iterations", C.c_int32),
                ("restarts", C.c_int32), ("status", C.c_int32)]


class MgHeatStepInfo(C.Structure):
    """mg_heat_step_info (include/mghip.h, "Time stepping")"""
    _fields_ = [("lambda", C.c_double), ("rhs_norm", C.c_double), ("initial_residual", C.c_double),
                ("final_residual", C.c_double), ("solve_seconds", C.c_double), ("cycles", C.c_int32), ("converged", C.c_int32)]


MG_HEAT_EXPLICIT_EULER, MG_HEAT_IMPLICIT_EULER, MG_HEAT_CRANK_NICOLSON, MG_HEAT_BDF2 = 0, 1, 2, 3
MG_HEAT_INNER_CYCLE, MG_HEAT_INNER_PCG = 0, 1
PCG_STATUS = {0: "converged", 1: "max_iterations", 2: "breakdown"}
SWITCH_REASONS = {0: None, 1: "threshold", 2: "stagnation", 3: "fp32_floor", 4: "fp32_skipped"}


class MgPlanOp(C.Structure):
    """mg_plan_op (include/mghip.h, "Cycle plans")"""
    _fields_ = [("op", C.c_int32), ("stream", C.c_int32), ("i", C.c_int32 * 24), ("d", C.c_double * 4), ("p", C.c_void_p * 8)]


(MG_PLAN_DOWN_LEG, MG_PLAN_UP_LEG, MG_PLAN_COPY2D, MG_PLAN_ADD_F64, MG_PLAN_GROUP_BEGIN, MG_PLAN_SEND, MG_PLAN_RECV,
 MG_PLAN_GROUP_END, MG_PLAN_ALLGATHER, MG_PLAN_ALLREDUCE_F64, MG_PLAN_COARSE_BEGIN, MG_PLAN_COARSE_CYCLE, MG_PLAN_COARSE_END,
 MG_PLAN_EVENT_RECORD, MG_PLAN_STREAM_WAIT, MG_PLAN_RESULT, MG_PLAN_SPAN_LEG) = range(1, 18)

_vp, _i, _d = C.c_void_p, C.c_int, C.c_double
_pi, _pd = C.POINTER(C.c_int), C.POINTER(C.c_double)

# name -> (restype, argtypes); every symbol include/mghip.h declares
SIGNATURES = {
    "mg_version": (C.c_char_p, []),
    "mg_device_count": (_i, [_pi]),
    "mg_last_error": (C.c_char_p, [_vp]),
    "mg_create": (_i, [C.POINTER(MgConfig), C.POINTER(_vp)]),
    "mg_destroy": (_i, [_vp]),
    "mg_num_levels": (_i, [_vp, _pi]),
    "mg_level_shape": (_i, [_vp, _i, _pi, _pi]),
    "mg_level_timings": (_i, [_vp, _i, _pd]),
    "mg_solve": (_i, [_vp, _vp, _vp, _vp, _i, _d, _i, _pd, _i, _pi, _pi, C.POINTER(C.c_int32), C.POINTER(MgStats)]),
    "mg_iterate": (_i, [_vp, _d, _i, _pd, _i, _pi, _pi, C.POINTER(C.c_int32), C.POINTER(MgStats)]),
    "mg_set_coefficient": (_i, [_vp, _vp, _i]),
    "mg_set_shift": (_i, [_vp, _d]),
    "mg_set_rhs": (_i, [_vp, _vp, _i]),
    "mg_set_solution": (_i, [_vp, _vp, _i]),
    "mg_get_solution": (_i, [_vp, _vp, _i]),
    "mg_cycle": (_i, [_vp, _i]),
    "mg_fmg": (_i, [_vp, _i]),
    "mg_residual_norm": (_i, [_vp, _pd]),
    "mg_set_working_precision": (_i, [_vp, _i]),
    "mg_synchronize": (_i, [_vp]),
    "mg_get_stream": (_i, [_vp, C.POINTER(_vp)]),
    "mg_time_op": (_i, [_vp, _i, _i, _i, _i, _pd]),
    "mg_op_residual": (_i, [_i, _i, _i, _d, _d, _d, _vp, _vp, _vp]),
    "mg_op_residual_mixed": (_i, [_i, _i, _d, _d, _d, _vp, _vp, _vp]),
    "mg_dev_residual_f32in_f64out": (_i, [_i, _i, _i, _i, _d, _d, _d, _vp, _vp, _vp, _vp]),
    "mg_op_apply": (_i, [_i, _i, _i, _d, _d, _d, _vp, _vp]),
    "mg_op_norm": (_i, [_i, _i, _i, _d, _d, _vp, _pd]),
    "mg_op_jacobi": (_i, [_i, _i, _i, _d, _d, _d, _i, _vp, _vp, _vp]),
    "mg_op_rbgs": (_i, [_i, _i, _i, _d, _d, _d, _i, _vp, _vp, _vp]),
    "mg_op_helmholtz": (_i, [_i, _i, _i, _i, _d, _d, _d, _d, _d, _i, _vp, _vp, _vp]),
    "mg_op_residual_var": (_i, [_i, _i, _i, _d, _d, _d, _vp, _vp, _vp, _vp]),
    "mg_op_jacobi_var": (_i, [_i, _i, _i, _d, _d, _d, _i, _vp, _vp, _vp, _vp]),
    "mg_op_rbgs_var": (_i, [_i, _i, _i, _d, _d, _d, _i, _vp, _vp, _vp, _vp]),
    "mg_op_restrict_fw": (_i, [_i, _i, _i, _i, _vp, _vp]),
    "mg_op_prolong_bilinear": (_i, [_i, _i, _i, _i, _vp, _vp]),
    "mg_op_coarse_solve": (_i, [_i, _i, _i, _d, _d, _d, _d, _i, _vp, _vp, _vp, _pi]),
    "mg_dev_jacobi": (_i, [_i, _i, _i, _i, _d, _d, _d, _vp, _vp, _vp, _vp]),
    "mg_dev_rbgs_colour": (_i, [_i, _i, _i, _i, _d, _d, _d, _i, _i, _vp, _vp, _vp]),
    "mg_dev_residual": (_i, [_i, _i, _i, _i, _d, _d, _d, _vp, _vp, _vp, _vp]),
    "mg_dev_sumsq": (_i, [_i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "mg_dev_restrict_fw": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "mg_dev_prolong_add": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "mg_set_stream": (_i, [_vp, _vp, _i]),
    "mg_set_rhs_device": (_i, [_vp, _vp, _i, _i]),
    "mg_update_rhs_device": (_i, [_vp, _vp, _i, _i]),
    "mg_zero_solution_device": (_i, [_vp]),
    "mg_get_solution_device": (_i, [_vp, _vp, _i, _i]),
    "mg_dev_convert": (_i, [_i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "mg_dev_down_leg": (_i, [_i] * 11 + [_d] * 4 + [_i] * 3 + [_vp] * 5 + [_i, C.POINTER(C.c_int)]),
    "mg_dev_up_leg": (_i, [_i] * 13 + [_d] * 4 + [_i] * 2 + [_vp] * 4 + [_i] * 5 + [_vp] * 3),
    "mg_dev_down_leg_var": (_i, [_i] * 11 + [_d] * 4 + [_i] * 3 + [_vp] * 5 + [_i, C.POINTER(C.c_int), _vp, _vp]),
    "mg_dev_up_leg_var": (_i, [_i] * 13 + [_d] * 4 + [_i] * 2 + [_vp] * 4 + [_i] * 5 + [_vp] * 5),
    "mg_dev_span_leg_ok": (_i, [_i] * 6),
    "mg_dev_span_leg": (_i, [_i] * 13 + [_d] * 4 + [_i] * 3 + [_vp] * 6 + [_i] * 4 + [_vp] * 3),
    "mg_dev_var_rdiag": (_i, [_i] * 4 + [_d] * 3 + [_vp] * 3),
    "mg_dev_inject_ring": (_i, [_i] * 11 + [_vp] * 3),
    "mg_dev_scratch_bytes": (_i, [_i, _i, C.POINTER(C.c_int64)]),
    "mg_pitch_elems": (_i, [_i, _i, _pi]),
    "mg_plan_create": (_i, [C.POINTER(MgPlanOp), _i, _vp, _i, C.POINTER(_vp)]),
    "mg_plan_run": (_i, [_vp, _vp, _vp, _pd]),
    "mg_plan_run_async": (_i, [_vp, _vp, _vp]),
    "mg_plan_wait": (_i, [_vp, _pd]),
    "mg_plan_num_ops": (_i, [_vp, _pi]),
    "mg_plan_copy_launches": (_i, [_vp, _pi, _pi]),
    "mg_plan_profile": (_i, [_vp, _i]),
    "mg_plan_phase_times": (_i, [_vp, _pd]),
    "mg_comm_ranks": (_i, [_vp, _pi, _pi]),
    "mg_plan_error": (C.c_char_p, [_vp]),
    "mg_plan_destroy": (_i, [_vp]),
    "mg_comm_unique_id": (_i, [C.c_char_p, _vp]),
    "mg_comm_init": (_i, [C.c_char_p, _vp, _i, _i, _i, C.POINTER(_vp)]),
    "mg_comm_destroy": (_i, [_vp]),
    "mg_pcg_create": (_i, [C.POINTER(MgConfig), _i, _i, C.POINTER(_vp)]),
    "mg_pcg_destroy": (_i, [_vp]),
    "mg_pcg_set_coefficient": (_i, [_vp, _vp, _i]),
    "mg_pcg_set_shift": (_i, [_vp, _d]),
    "mg_pcg_solve": (_i, [_vp, _vp, _vp, _vp, _i, _d, _i, _pd, _i, _pi, _pi, C.POINTER(MgPcgStats)]),
    "mg_pcg_solve_device": (_i, [_vp, _vp, _i, _vp, _i, _i, _d, _i, _pd, _i, _pi, _pi, C.POINTER(MgPcgStats)]),
    "mg_pcg_set_lookahead": (_i, [_vp, _i]),
    "mg_pcg_last_error": (C.c_char_p, [_vp]),
    "mg_dev_pcg_direction": (_i, [_i] * 3 + [_d] * 4 + [_vp] * 9),
    "mg_dev_pcg_update": (_i, [_i] * 3 + [_vp] * 8),
    "mg_dev_pcg_dots": (_i, [_i] * 3 + [_vp] * 7),
    "mg_dev_pcg_scalars": (_i, [_i, _vp, _i, _vp, _i, _vp, _vp]),
    "mg_heat_create": (_i, [C.POINTER(MgConfig), _d, C.POINTER(_vp)]),
    "mg_heat_destroy": (_i, [_vp]),
    "mg_heat_last_error": (C.c_char_p, [_vp]),
    "mg_heat_set_slot": (_i, [_vp, _i, _vp, _i]),
    "mg_heat_get_slot": (_i, [_vp, _i, _vp, _i]),
    "mg_heat_set_slot_device": (_i, [_vp, _i, _vp, _i, _i]),
    "mg_heat_get_slot_device": (_i, [_vp, _i, _vp, _i, _i]),
    "mg_heat_set_source": (_i, [_vp, _vp, _i]),
    "mg_heat_step": (_i, [_vp, _i, _d, _i, _i, _i, _d, _d, _pd, _i, _d, _i, C.POINTER(MgHeatStepInfo)]),
    "mg_heat_diff_norm": (_i, [_vp, _i, _i, _pd]),
    "mg_dev_heat_rhs": (_i, [_i] * 4 + [_d] * 4 + [_vp] * 3 + [_d] * 2 + [_vp] * 4),
    "mg_dev_heat_ring": (_i, [_i] * 3 + [_pd, _vp, _vp]),
    "mg_dev_heat_diff_sumsq": (_i, [_i] * 3 + [_vp] * 5),
}

# name -> (restype, argtypes); every symbol include/mghip_heat.h declares (the time stepper's extensions)
HEAT_EXT_SIGNATURES = {
    "mg_heat_create_ex": (_i, [C.POINTER(MgConfig), _d, _i, _i, _i, C.POINTER(_vp)]),
    "mg_heat_set_coefficient": (_i, [_vp, _vp, _i]),
    "mg_dev_heat_rhs_var": (_i, [_i] * 4 + [_d] * 4 + [_vp] * 4 + [_d] * 2 + [_vp] * 4),
}

# name -> (restype, argtypes); every symbol include/mghip_line.h declares (zebra line relaxation, call by call)
LINE_SIGNATURES = {
    "mg_line_plan_create": (_i, [_i] * 5 + [_d] * 3 + [C.POINTER(_vp)]),
    "mg_line_plan_destroy": (_i, [_vp]),
    "mg_dev_line_colour": (_i, [_vp, _i, _d, _vp, _vp, _vp]),
    "mg_op_zebra": (_i, [_i] * 4 + [_d] * 4 + [_i] + [_vp] * 3),
    "mg_line_time_sweep": (_i, [_vp, _i, _pd]),
}

# name -> (restype, argtypes); every symbol include/mghip_eig.h declares (the block eigensolver)
EIG_SIGNATURES = {
    "mg_eig_create": (_i, [C.POINTER(MgConfig), _i, _i, C.POINTER(_vp)]),
    "mg_eig_destroy": (_i, [_vp]),
    "mg_eig_last_error": (C.c_char_p, [_vp]),
    "mg_eig_set_coefficient": (_i, [_vp, _vp, _i]),
    "mg_eig_solve": (_i, [_vp, _i, _vp, _i, _d, _i, _pd, _vp, _pd, _pd, _i, _pi, _pi, C.POINTER(MgEigStats)]),
    "mg_eig_host_ritz": (_i, [_i, _i, _pd, _pd, _pd, _pd]),
    "mg_dev_eig_apply": (_i, [_i] * 4 + [C.c_int64] + [_d] * 3 + [_vp] * 4),
    "mg_dev_eig_gram": (_i, [_i] * 3 + [C.c_int64, _i, _vp, _i] + [_vp] * 4),
    "mg_dev_eig_combine": (_i, [_i] * 3 + [C.c_int64, _i, _vp, _i] + [_vp] * 3),
    "mg_dev_eig_residual": (_i, [_i] * 4 + [C.c_int64] + [_vp] * 7),
    "mg_eig_time_op": (_i, [_vp, _i, _i, _pd]),
}

# name -> (restype, argtypes); every symbol include/mghip_ho.h declares (the fourth-order compact scheme of the Krylov loop)
HO_SIGNATURES = {
    "mg_pcg_set_order": (_i, [_vp, _i]),
    "mg_dev_ho_direction": (_i, [_i] * 3 + [_d] * 4 + [_vp] * 8),
    "mg_dev_ho_residual": (_i, [_i] * 3 + [_d] * 4 + [_vp] * 6),
    "mg_dev_ho_rhs": (_i, [_i] * 3 + [_vp] * 3),
    "mg_op_apply_ho": (_i, [_i] * 2 + [_d] * 4 + [_vp] * 2),
    "mg_op_rhs_ho": (_i, [_i] * 2 + [_vp] * 2),
}


class MgFlowStepInfo(C.Structure):
    """mg_flow_step_info (include/mghip_flow.h)"""
    _fields_ = [("sigma", C.c_double), ("c0", C.c_double), ("c1", C.c_double), ("cfl", C.c_double), ("rhs_norm", C.c_double),
                ("omega_initial_residual", C.c_double), ("omega_final_residual", C.c_double), ("psi_rhs_norm", C.c_double),
                ("psi_initial_residual", C.c_double), ("psi_final_residual", C.c_double), ("omega_change", C.c_double),
                ("seconds", C.c_double), ("omega_cycles", C.c_int32), ("psi_cycles", C.c_int32),
                ("omega_converged", C.c_int32), ("psi_converged", C.c_int32)]


MG_FLOW_FREE_SLIP, MG_FLOW_NO_SLIP = 0, 1
MG_FLOW_OMEGA, MG_FLOW_PSI, MG_FLOW_N = 0, 1, 2

# name -> (restype, argtypes); every symbol include/mghip_flow.h declares (the vorticity / stream-function stepper)
FLOW_SIGNATURES = {
    "mg_flow_create": (_i, [C.POINTER(MgConfig), _d, _i, C.POINTER(_vp)]),
    "mg_flow_destroy": (_i, [_vp]),
    "mg_flow_last_error": (C.c_char_p, [_vp]),
    "mg_flow_set_walls": (_i, [_vp, _pd]),
    "mg_flow_set_forcing": (_i, [_vp, _vp, _i]),
    "mg_flow_set_state": (_i, [_vp, _vp, _i, _d, _i, C.POINTER(MgFlowStepInfo)]),
    "mg_flow_get": (_i, [_vp, _i, _vp, _i]),
    "mg_flow_get_device": (_i, [_vp, _i, _vp, _i, _i]),
    "mg_flow_set_device": (_i, [_vp, _i, _vp, _i, _i]),
    "mg_flow_step": (_i, [_vp, _d, _d, _i, C.POINTER(MgFlowStepInfo)]),
    "mg_flow_diagnostics": (_i, [_vp, _pd]),
    "mg_flow_velocity_max": (_i, [_vp, _pd]),
    "mg_dev_flow_rhs": (_i, [_i] * 3 + [_d] * 6 + [_vp] * 9),
    "mg_dev_flow_wall": (_i, [_i] * 3 + [_d] * 2 + [_i, _pd] + [_vp] * 3),
    "mg_dev_flow_diag": (_i, [_i] * 3 + [_vp] * 5),
    "mg_dev_flow_interior": (_i, [_i] * 3 + [_vp] * 6),
}



class MgNlOptions(C.Structure):
    """mg_nl_options (include/mghip_nl.h)"""
    _fields_ = [("forcing", C.c_int32), ("max_backtracks", C.c_int32), ("max_inner", C.c_int32), ("reserved", C.c_int32),
                ("eta", C.c_double), ("gamma", C.c_double), ("eta_max", C.c_double), ("eta_min", C.c_double)]


class MgNlStats(C.Structure):
    """mg_nl_stats (include/mghip_nl.h)"""
    _fields_ = [("solve_seconds", C.c_double), ("initial_residual", C.c_double), ("final_residual", C.c_double),
                ("newton_iterations", C.c_int32), ("inner_iterations", C.c_int32), ("evaluations", C.c_int32),
                ("status", C.c_int32)]


MG_NL_LINEAR, MG_NL_CUBIC, MG_NL_SINH, MG_NL_EXP = 0, 1, 2, 3
MG_NL_FORCING_EISENSTAT_WALKER, MG_NL_FORCING_FIXED = 0, 1
NL_KINDS = {"linear": MG_NL_LINEAR, "cubic": MG_NL_CUBIC, "sinh": MG_NL_SINH, "exp": MG_NL_EXP}
NL_FORCINGS = {"eisenstat_walker": MG_NL_FORCING_EISENSTAT_WALKER, "fixed": MG_NL_FORCING_FIXED}
NL_STATUS = {0: "converged", 1: "max_newton", 2: "breakdown", 3: "line_search_failed"}

# name -> (restype, argtypes); every symbol include/mghip_nl.h declares (the semilinear Newton method)
NL_SIGNATURES = {
    "mg_dev_nl_eval": (_i, [_i] * 4 + [_d] * 5 + [_vp] * 4 + [_d] + [_vp] * 7),
    "mg_op_nl_eval": (_i, [_i] * 3 + [_d] * 5 + [_vp] * 4 + [_d] + [_vp] * 5),
    "mg_pcg_set_reaction_device": (_i, [_vp, _vp, _i, _d]),
    "mg_dev_pcg_direction_react": (_i, [_i] * 3 + [_d] * 4 + [_vp] * 10),
    "mg_nl_create": (_i, [C.POINTER(MgConfig), _i, _i, C.POINTER(_vp)]),
    "mg_nl_destroy": (_i, [_vp]),
    "mg_nl_last_error": (C.c_char_p, [_vp]),
    "mg_nl_options_default": (_i, [C.POINTER(MgNlOptions)]),
    "mg_nl_set_coefficient": (_i, [_vp, _vp, _i]),
    "mg_nl_set_shift": (_i, [_vp, _d]),
    "mg_nl_set_nonlinearity": (_i, [_vp, _i, _d, _vp, _i]),
    "mg_nl_set_options": (_i, [_vp, C.POINTER(MgNlOptions)]),
    "mg_nl_solve": (_i, [_vp, _vp, _vp, _vp, _i, _d, _i, _pd, _pi, _pd, _pd, _i, _pi, _pi, C.POINTER(MgNlStats)]),
    "mg_nl_solve_device": (_i, [_vp, _vp, _i, _vp, _i, _i, _d, _i, _pd, _pi, _pd, _pd, _i, _pi, _pi, C.POINTER(MgNlStats)]),
}



class MgRdStepInfo(C.Structure):
    """mg_rd_step_info (include/mghip_rd.h)"""
    _fields_ = [("lambda", C.c_double), ("rhs_norm", C.c_double), ("initial_residual", C.c_double),
                ("final_residual", C.c_double), ("solve_seconds", C.c_double), ("newton_iterations", C.c_int32),
                ("inner_iterations", C.c_int32), ("evaluations", C.c_int32), ("status", C.c_int32), ("converged", C.c_int32),
                ("reserved", C.c_int32)]


RD_SCHEMES = {"implicit_euler": MG_HEAT_IMPLICIT_EULER, "crank_nicolson": MG_HEAT_CRANK_NICOLSON, "bdf2": MG_HEAT_BDF2}

# name -> (restype, argtypes); every symbol include/mghip_rd.h declares (the reaction-diffusion stepper)
RD_SIGNATURES = {
    "mg_dev_rd_rhs": (_i, [_i] * 5 + [_d] * 6 + [_vp] * 5 + [_d] * 2 + [_vp] * 4),
    "mg_dev_rd_energy": (_i, [_i] * 4 + [_d] * 2 + [_vp] * 6),
    "mg_rd_create": (_i, [C.POINTER(MgConfig), _d, _i, _i, C.POINTER(_vp)]),
    "mg_rd_destroy": (_i, [_vp]),
    "mg_rd_last_error": (C.c_char_p, [_vp]),
    "mg_rd_set_slot": (_i, [_vp, _i, _vp, _i]),
    "mg_rd_get_slot": (_i, [_vp, _i, _vp, _i]),
    "mg_rd_set_slot_device": (_i, [_vp, _i, _vp, _i, _i]),
    "mg_rd_get_slot_device": (_i, [_vp, _i, _vp, _i, _i]),
    "mg_rd_set_coefficient": (_i, [_vp, _vp, _i]),
    "mg_rd_set_source": (_i, [_vp, _vp, _i]),
    "mg_rd_set_reaction": (_i, [_vp, _i, _d, _vp, _i, _d]),
    "mg_rd_set_newton_options": (_i, [_vp, C.POINTER(MgNlOptions)]),
    "mg_rd_step": (_i, [_vp, _i, _d, _i, _i, _i, _d, _d, _pd, _d, _i, C.POINTER(MgRdStepInfo)]),
    "mg_rd_energy": (_i, [_vp, _i, _pd]),
    "mg_rd_diff_norm": (_i, [_vp, _i, _i, _pd]),
}


class Mg3Config(C.Structure):
    """mg3_config (include/mghip_3d.h)"""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("max_levels", C.c_int32),
                ("x0", C.c_double), ("x1", C.c_double), ("y0", C.c_double), ("y1", C.c_double), ("z0", C.c_double), ("z1", C.c_double),
                ("sigma", C.c_double), ("omega", C.c_double), ("cycle", C.c_int32), ("pre", C.c_int32), ("post", C.c_int32),
                ("smoother", C.c_int32), ("coarse_sweeps", C.c_int32), ("precision", C.c_int32), ("device", C.c_int32),
                ("reserved", C.c_int32)]


class Mg3Stats(C.Structure):
    """mg3_stats (include/mghip_3d.h)"""
    _fields_ = [("initial_residual", C.c_double), ("final_residual", C.c_double), ("solve_seconds", C.c_double),
                ("device_bytes", C.c_int64), ("iterations", C.c_int32), ("converged", C.c_int32), ("levels", C.c_int32),
                ("reserved", C.c_int32)]


MG3_PREC_DOUBLE, MG3_PREC_SINGLE, MG3_PREC_DEFECT = 0, 1, 2
MG3_PRECISIONS = {"double": MG3_PREC_DOUBLE, "single": MG3_PREC_SINGLE, "defect": MG3_PREC_DEFECT}

# name -> (restype, argtypes); every symbol include/mghip_3d.h declares (the 3-D multigrid family)
MG3_SIGNATURES = {
    "mg3_create": (_i, [C.POINTER(Mg3Config), C.POINTER(_vp)]),
    "mg3_destroy": (_i, [_vp]),
    "mg3_last_error": (C.c_char_p, [_vp]),
    "mg3_set_rhs": (_i, [_vp, _vp, _i]),
    "mg3_set_solution": (_i, [_vp, _vp, _i]),
    "mg3_get_solution": (_i, [_vp, _vp, _i]),
    "mg3_set_rhs_device": (_i, [_vp, _vp, _i, _i]),
    "mg3_set_solution_device": (_i, [_vp, _vp, _i, _i]),
    "mg3_get_solution_device": (_i, [_vp, _vp, _i, _i]),
    "mg3_zero_solution": (_i, [_vp]),
    "mg3_cycle": (_i, [_vp, _i]),
    "mg3_residual_norm": (_i, [_vp, _pd]),
    "mg3_solve": (_i, [_vp, _d, _i, _pd, _i, _pi, _pi, C.POINTER(Mg3Stats)]),
    "mg3_synchronize": (_i, [_vp]),
    "mg3_stream": (_i, [_vp, C.POINTER(_vp)]),
    "mg3_num_levels": (_i, [_vp, _pi]),
    "mg3_device_bytes": (_i, [C.POINTER(Mg3Config), C.POINTER(C.c_int64)]),
    "mg3_dev_scratch_bytes": (_i, [_i, _i, _i, C.POINTER(C.c_int64)]),
    "mg3_dev_residual": (_i, [_i] * 7 + [_d] * 4 + [_vp] * 6),
    "mg3_dev_jacobi": (_i, [_i] * 5 + [_d] * 5 + [_vp] * 4),
    "mg3_dev_rbgs_colour": (_i, [_i] * 5 + [_d] * 5 + [_i, _i] + [_vp] * 3),
    "mg3_dev_restrict": (_i, [_i] * 6 + [_vp] * 3),
    "mg3_dev_prolong_add": (_i, [_i] * 6 + [_vp] * 3),
    "mg3_dev_upcast_add": (_i, [_i] * 5 + [_vp] * 3),
    "mg3_dev_norm": (_i, [_i] * 5 + [_vp] * 4),
    "mg3_dev_coarse_solve": (_i, [_i] * 5 + [_d] * 4 + [_i, _vp, _vp, _pi, _vp]),
}

_lib = None


def _share_torch_hip_runtime():
    """PyTorch's ROCm wheel bundles its own libamdhip64.so / libhsa-runtime64.so and loads them by path.
    Two HIP runtimes in one process cannot both own the device (the second reports "no ROCm-capable
    device"), so whichever of {torch, libmghip} comes first must bring in the SAME copy: when torch is
    installed but not imported yet, preload its libamdhip64.so so that libmghip.so binds to it by SONAME
    and a later `import torch` finds its own file already mapped."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def library_path():
    return os.environ.get("MGHIP_LIBRARY", _build.LIBPATH)


def load():
    """Load libmghip.so (building it first when the sources are newer and hipcc is present)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if path == _build.LIBPATH and _build.is_stale():
        try:
            _build.build_library()
        except Exception as exc:                      # no compiler on this machine: use what ships
            if not os.path.exists(path):
                raise ImportError(f"libmghip.so is not built and cannot be built here: {exc}") from exc
    if not os.path.exists(path):
        raise ImportError(f"libmghip.so not found at {path}; run `python -m "
                          "mixed_precision_multigrid_solvers_for_pdes_amd._build`")
    _share_torch_hip_runtime()
    lib = C.CDLL(path)
    for name, (res, args) in list(SIGNATURES.items()) + list(HEAT_EXT_SIGNATURES.items()) + list(LINE_SIGNATURES.items()) + \
            list(EIG_SIGNATURES.items()) + list(HO_SIGNATURES.items()) + list(FLOW_SIGNATURES.items()) + list(NL_SIGNATURES.items()) + \
            list(RD_SIGNATURES.items()) + list(MG3_SIGNATURES.items()):
        fn = getattr(lib, name)                       # AttributeError if the ABI is incomplete
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def dtype_code(dt):
    dt = np.dtype(dt)
    if dt == np.float32:
        return MG_F32
    if dt == np.float64:
        return MG_F64
    raise TypeError(f"unsupported dtype {dt}: the multigrid path computes in float32 or float64")


def np_dtype(code):
    return np.float32 if code == MG_F32 else np.float64


def last_error(handle=None):
    msg = load().mg_last_error(handle)
    return msg.decode() if msg else ""


def check(rc, handle=None):
    """Map a status code to the exception the reference raises for the same condition."""
    if rc == MG_OK:
        return
    msg = last_error(handle) or last_error(None) or f"mghip error {rc}"
    if rc in (MG_ERR_INVALID_VALUE, MG_ERR_STATE):
        raise ValueError(msg)
    if rc == MG_ERR_ALLOC:
        raise MemoryError(msg)
    if rc == MG_ERR_NO_DEVICE:
        raise RuntimeError("mghip: no usable HIP device (the multigrid path has no CPU fallback): " + msg)
    raise RuntimeError("mghip: " + msg)


def check_plan(rc, plan=None):
    """status of a mg_plan_* / mg_comm_* call"""
    if rc == MG_OK:
        return
    msg = load().mg_plan_error(plan)
    msg = (msg.decode() if msg else "") or f"mghip plan error {rc}"
    if rc == MG_ERR_INVALID_VALUE:
        raise ValueError(msg)
    if rc == MG_ERR_TIMEOUT:
        raise PlanTimeout("mghip: " + msg)
    raise RuntimeError("mghip: " + msg)


def device_count():
    n = C.c_int(0)
    rc = load().mg_device_count(C.byref(n))
    return n.value if rc == MG_OK else 0


def on_gpu_box():
    """True where the AMD compute device node exists."""
    return os.path.exists("/dev/kfd")


def as_c(a, dtype=None):
    """C-contiguous view/copy of `a` in a supported dtype (never modifies the caller's array)."""
    a = np.asarray(a)
    if dtype is None:
        dtype = a.dtype if a.dtype in (np.float32, np.float64) else np.float64
    return np.ascontiguousarray(a, dtype=dtype)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)
