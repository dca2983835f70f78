"""ctypes binding of the C ABI in include/fiveeq.h (libfiveeq_hip.so).

There is NO fallback: if the HIP library is missing or does not export the
expected symbols, `load()` raises.  The ensemble engine cannot run without it.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FIVEEQ_LIB_PATH selects another build of the same library (e.g. the host-sanitizer build of tools/sanitize_host.sh)
LIB_PATH = os.environ.get("FIVEEQ_LIB_PATH") or os.path.join(_HERE, "csrc", "libfiveeq_hip.so")

ABI_VERSION = 13
MAX_GAS = 3
MAX_POOLS = 4
N_BOX = 2
DRIVE_STRIDE = 8
LHS_MAX_TOTAL = 1 << 28
MAX_FEXT = 4
WSCAN_TILE = 1024                   # weights per workgroup of fiveeq_wscan (fiveeq_resample.hpp)
MAX_LEVELS = 8                      # FIVEEQ_MAX_LEVELS / FIVEEQ_MAX_WINDOWS of fiveeq_traj_metrics_* (fiveeq_metrics.hpp)
MAX_WINDOWS = 4
METRICS_TILE_F64 = 512              # members per workgroup of traj_metrics_kernel: 256 lanes of 16 bytes of a row
METRICS_TILE_F32 = 1024
METRICS_UNROLL = 8                  # rows whose loads its row loop issues before it uses the first (16-byte loads)
METRICS_UNROLL_NARROW = 2           # the same on the element-load path; load() checks all four against the library
MAX_SMOOTH_WINDOW = 32              # FIVEEQ_MAX_SMOOTH_WINDOW of fiveeq_running_mean_* (fiveeq_smooth.hpp); load() checks it
MAX_JOINT_ROWS = 32                 # fiveeq_max_joint_rows() / fiveeq_max_cond_bins() of the joint statistics (fiveeq_joint.hpp)
MAX_COND_BINS = 32
# fiveeq_joint_tile(0..7): x rows, y rows per workgroup of the co-moment pass; members per chunk; members per lane and load of
# fp64 / fp32 rows; bins, y rows per workgroup of the conditional sums; lanes per workgroup.  load() checks them.
JOINT_TILE = (4, 4, 4096, 2, 4, 16, 4, 256)
MAX_PULSES = 3                      # fiveeq_max_pulses() / fiveeq_max_horizons() of fiveeq_pulse_response_* (fiveeq_pulse.hpp)
MAX_HORIZONS = 8
MAX_SCORE_Q = 4                     # fiveeq_max_score_quantities() of fiveeq_score_rows_* (fiveeq_score.hpp)
SCORE_TILE_F64 = 512                # members per workgroup of score_rows_kernel: 256 lanes of 16 bytes of a row
SCORE_TILE_F32 = 1024
SCORE_UNROLL = 8                    # live rows whose loads its row loop issues before it uses the first (16-byte loads)
SCORE_UNROLL_NARROW = 4             # the same on the element-load path; load() checks all five against the library
JOINT_TILE_X, JOINT_TILE_Y, JOINT_CHUNK, JOINT_LANE_F64, JOINT_LANE_F32, COND_TILE_BINS, COND_TILE_Y, JOINT_BLOCK = JOINT_TILE

OK = 0
E_INVALID = -1
E_UNSUPPORTED = -2
E_HIP = -3
FORM_PER_STEP = 0
FORM_FUSED = 1


class FiveEqError(RuntimeError):
    """A C-ABI call returned a negative code; `.code` holds it."""

    def __init__(self, code, message):
        super().__init__(f"fiveeq error {code}: {message}")
        self.code = code


class Gas(ctypes.Structure):
    """struct fiveeq_gas (include/fiveeq.h)."""
    _fields_ = [
        ("a", ctypes.c_double * MAX_POOLS),
        ("tau", ctypes.c_double * MAX_POOLS),
        ("g0", ctypes.c_double),
        ("g1", ctypes.c_double),
        ("ra", ctypes.c_double),
        ("C0", ctypes.c_double),
        ("emis2conc", ctypes.c_double),
        ("f", ctypes.c_double * 3),
        ("n_pools", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class Model(ctypes.Structure):
    """struct fiveeq_model (include/fiveeq.h)."""
    _fields_ = [
        ("gas", Gas * MAX_GAS),
        ("d", ctypes.c_double * N_BOX),
        ("iirf_max", ctypes.c_double),
        ("dt", ctypes.c_double),
        ("n_gas", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_i32 = ctypes.c_int32
_mp = ctypes.POINTER(Model)

_STEP_ARGS = [_mp, _i64, _i64, _p, _i32, _i32, _p, _p, _p, _p, _p, _p, _i32, _p, _p]


def _run_args(tail, scen=False, cumE=False):
    """argtypes of a stepping entry point: (model, n, ld, [n_scen,] drive, n_steps, t_begin, t_end, r, q, R, S, [cumE,] C_traj,
    T_traj, n_rows, T_stats), then its own tail."""
    return ([_mp, _i64, _i64] + [_i32] * scen + [_p, _i32, _i32, _i32, _p, _p, _p, _p] + [_p] * cumE + [_p, _p, _i32, _p]
            + list(tail))


# the tails: stream; plan_out; (form, k_steps, stream); (obs, misfit); (fscale, fext, n_fext); (lo, hi, n_bins, bin_ring, ring_rows)
_ST, _PLAN, _FORM, _OBS, _FORC = [_p], [ctypes.POINTER(_p)], [_i32, _i32, _p], [_p, _p], [_p, _p, _i32]
_RING = [ctypes.c_double, ctypes.c_double, _i32, _p, _i32]
_UNI = [ctypes.c_uint32, _p]        # (mask, values): the single-valued parameter rows, values on the host
_MFORC = [_p, _i32]                 # (mforc, n_mforc_rows): the member-forcing rows
# the stepping entry points that come as _f64 and _f32: name -> _run_args(...)
_RUNS = {
    "run": _run_args(_ST),
    "run_fused": _run_args(_ST),
    "run_ksteps": _run_args([_i32] + _ST),
    "run_small": _run_args([_i32] + _ST),
    "run_bins": _run_args(_RING + _ST),
    "run_fused_bins": _run_args(_RING + _ST),
    "run_inverse": _run_args(_ST, cumE=True),
    "run_inverse_forc": _run_args(_FORC + _OBS + _ST, cumE=True),
    "run_mixed": _run_args([_i32] + _FORC + _OBS + _ST, cumE=True),       # conc_mask behind T_stats
    "plan_create": _run_args(_PLAN),
    "run_obs": _run_args(_OBS + _FORM),
    "plan_create_obs": _run_args(_OBS + _PLAN),
    "run_scen": _run_args(_FORM, scen=True),
    "plan_create_scen": _run_args(_PLAN, scen=True),
    "run_forc": _run_args(_FORC + _OBS + _FORM),
    "plan_create_forc": _run_args(_FORC + _OBS + _PLAN),
    "run_mforc": _run_args(_FORC + _OBS + _MFORC + _FORM),
    "plan_create_mforc": _run_args(_FORC + _OBS + _MFORC + _PLAN),
    "run_scen_forc": _run_args(_FORC + _FORM, scen=True),
    "plan_create_scen_forc": _run_args(_FORC + _PLAN, scen=True),
    "run_uniform": _run_args(_UNI + _ST),
    "plan_create_uniform": _run_args(_UNI + _PLAN),
}
# fiveeq_forcing_rows_*: (model, n_rows, n_members, ld, C_rows, c_row_stride, c_gas_stride, T_rows, t_row_stride, steps, drive,
# n_steps, q, fscale, n_fext, fext, F, F_gas, N, H, ld_out, H_io, S_io, n_mismatch, stream)
_FORCROWS = [_mp, _i32, _i64, _i64, _p, _i64, _i64, _p, _i64, _p, _p, _i32, _p, _p, _i32, _p, _p, _p, _p, _p, _i64, _p, _p, _p, _p]
# fiveeq_carbon_rows_*: (model, n_rows, n_members, ld, rows, c_row_stride, c_gas_stride, T_rows, t_row_stride, steps, drive, cum_end,
# n_steps, r, conc_mask, gas_mask, airborne, cumE, uptake, fraction, iirf, alpha, sink, ld_out, cum_io, ga_io, stream)
_CARBON = [_mp, _i32, _i64, _i64, _p, _i64, _i64, _p, _i64, _p, _p, _p, _i32, _p, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _i64, _p, _p, _p]
# fiveeq_pulse_response_*: (model, n_scen, n_rows, n_members, ld, C_rows, c_scen_stride, c_row_stride, c_gas_stride, T_rows,
# t_scen_stride, t_row_stride, steps, drive, n_steps, fscale, n_fext, fext, base, n_pulses, pulse_scen, pulse_gas, n_horizons,
# horizons, row0, out, ld_out, io, stream); pulse_scen, pulse_gas and horizons are HOST arrays of int32
_i32p = ctypes.POINTER(_i32)
_PULSE = [_mp, _i32, _i32, _i64, _i64, _p, _i64, _i64, _i64, _p, _i64, _i64, _p, _p, _i32, _p, _i32, _p, _i32, _i32, _i32p, _i32p, _i32,
          _i32p, _i32, _p, _i64, _p, _p]
# name -> (restype, argtypes); every symbol include/fiveeq.h declares
SIGNATURES = {
    "fiveeq_abi_version": (ctypes.c_int, []),
    "fiveeq_last_error": (ctypes.c_char_p, []),
    "fiveeq_source_hash": (ctypes.c_char_p, []),
    "fiveeq_build_flags": (ctypes.c_char_p, []),
    "fiveeq_sizeof_model": (ctypes.c_int64, []),
    "fiveeq_layout_supported": (ctypes.c_int, [_i32, ctypes.POINTER(_i32)]),
    "fiveeq_stats_waves": (ctypes.c_int64, [_i64]),
    "fiveeq_step_f64": (ctypes.c_int, _STEP_ARGS),
    "fiveeq_step_f32": (ctypes.c_int, _STEP_ARGS),
    **{f"fiveeq_{name}_{sfx}": (ctypes.c_int, args) for name, args in _RUNS.items() for sfx in ("f64", "f32")},
    "fiveeq_run_fused_comp_f32": (ctypes.c_int, _run_args([_i32] + _RING + _ST)),
    "fiveeq_run_small_comp_f32": (ctypes.c_int, _run_args(_ST)),
    "fiveeq_hist_bins": (ctypes.c_int, [_i32, _i64, _i64, _p, _i32, _p, _p]),
    "fiveeq_misfit_layout_supported": (ctypes.c_int, [_i32, ctypes.POINTER(_i32)]),
    "fiveeq_max_scenarios": (_i32, []),
    "fiveeq_forcing_layout_supported": (ctypes.c_int, [_i32, ctypes.POINTER(_i32)]),
    "fiveeq_mixed_layout_supported": (ctypes.c_int, [_i32, ctypes.POINTER(_i32), _i32]),
    "fiveeq_max_fext": (_i32, []),
    "fiveeq_small_lanes": (_i32, [_i32, ctypes.POINTER(_i32)]),
    "fiveeq_set_f32_packing": (ctypes.c_int, [ctypes.c_int]),
    "fiveeq_set_row_policy": (ctypes.c_int, [_i32]),
    "fiveeq_rows_streamed": (ctypes.c_int, [_i32, ctypes.POINTER(_i32), _i64, _i64, _i32]),
    "fiveeq_lhs_rows_f64": (ctypes.c_int, [ctypes.c_uint64, _i64, _i64, _i64, _i32, _i32, _i64, _p, _p]),
    "fiveeq_lhs_rows_host_f64": (ctypes.c_int, [ctypes.c_uint64, _i64, _i64, _i64, _i32, _i32, _i64, _p]),
    # (seed, m0, n_members, ld, t_begin, t_end, phi, s, xi_state, rows, stream)
    "fiveeq_noise_rows_f64": (ctypes.c_int, [ctypes.c_uint64, _i64, _i64, _i64, _i32, _i32, _p, _p, _p, _p, _p]),
    "fiveeq_noise_rows_f32": (ctypes.c_int, [ctypes.c_uint64, _i64, _i64, _i64, _i32, _i32, _p, _p, _p, _p, _p]),
    # (n_species, n_members, ld, n_rows, dt, c [host], emis, tau, eff, R, rows, accumulate, stream)
    "fiveeq_minor_rows_f64": (ctypes.c_int, [_i32, _i64, _i64, _i32, ctypes.c_double, _p, _p, _p, _p, _p, _p, _i32, _p]),
    "fiveeq_minor_rows_f32": (ctypes.c_int, [_i32, _i64, _i64, _i32, ctypes.c_double, _p, _p, _p, _p, _p, _p, _i32, _p]),
    # (n_species, aci_mask, n_members, ld, n_rows, base [host], emis, ari, shape, beta, rows, accumulate, stream)
    "fiveeq_aerosol_rows_f64": (ctypes.c_int, [_i32, _i32, _i64, _i64, _i32, _p, _p, _p, _p, _p, _p, _i32, _p]),
    "fiveeq_aerosol_rows_f32": (ctypes.c_int, [_i32, _i32, _i64, _i64, _i32, _p, _p, _p, _p, _p, _p, _i32, _p]),
    # (n_scen, n_comp, rate_mask, n_members, ld, n_rows, dt, T_rows, t_row_stride, t_scen_stride, par, heat, h_row_stride,
    # h_scen_stride, eta, S_io, total, comps, ld_out, stream)
    **{f"fiveeq_sea_level_rows_{sfx}": (ctypes.c_int, [_i32, _i32, _i32, _i64, _i64, _i32, ctypes.c_double, _p, _i64, _i64, _p, _p, _i64,
                                                       _i64, _p, _p, _p, _p, _i64, _p]) for sfx in ("f64", "f32")},
    "fiveeq_plan_launch": (ctypes.c_int, [_p, _p]),
    "fiveeq_plan_destroy": (ctypes.c_int, [_p]),
    "fiveeq_hfc_conc_f64": (ctypes.c_int, [_i64, _i64, _i32, _p, _p, _p, _p]),
    "fiveeq_hist_rows_f64": (ctypes.c_int, [_i32, _i64, _i64, _p, ctypes.c_double, ctypes.c_double, _i32, _p, _p]),
    "fiveeq_hist_rows_f32": (ctypes.c_int, [_i32, _i64, _i64, _p, ctypes.c_double, ctypes.c_double, _i32, _p, _p]),
    "fiveeq_row_moments_chunks": (ctypes.c_int64, [_i32, _i64]),
    "fiveeq_row_moments_f64": (ctypes.c_int, [_i32, _i64, _i64, _p, _p, _p, _p]),
    "fiveeq_row_moments_f32": (ctypes.c_int, [_i32, _i64, _i64, _p, _p, _p, _p]),
    "fiveeq_hist_rows_ranged_f64": (ctypes.c_int, [_i32, _i64, _i64, _p, _p, _i32, _p, _p]),
    "fiveeq_hist_rows_ranged_f32": (ctypes.c_int, [_i32, _i64, _i64, _p, _p, _i32, _p, _p]),
    "fiveeq_select_bins_f64": (ctypes.c_int, [_i32, _i64, _i64, _p, _p, _i32, _p, _p, _i64, _p, _p]),
    "fiveeq_select_bins_f32": (ctypes.c_int, [_i32, _i64, _i64, _p, _p, _i32, _p, _p, _i64, _p, _p]),
    "fiveeq_select_pick_f64": (ctypes.c_int, [_i32, _i32, _i64, _p, _p, _i32, _p, _p, _p]),
    "fiveeq_select_pick_f32": (ctypes.c_int, [_i32, _i32, _i64, _p, _p, _i32, _p, _p, _p]),
    "fiveeq_wrow_moments_chunks": (ctypes.c_int64, [_i32, _i64]),
    **{f"fiveeq_{name}_{sfx}": (ctypes.c_int, args) for sfx in ("f64", "f32") for name, args in (
        ("wrow_moments", [_i32, _i64, _i64, _p, _p, _p, _p, _p]),
        ("whist_rows_ranged", [_i32, _i64, _i64, _p, _p, _p, _i32, _p, _p]),
        ("wselect_bins", [_i32, _i64, _i64, _p, _p, _p, _i32, _p, _p, _p, _i64, _p, _p]),
        ("wselect_pick", [_i32, _i32, _i64, _p, _p, _p, _i32, _p, _p, _p]))},
    "fiveeq_wscan_chunks": (ctypes.c_int64, [_i64]),
    "fiveeq_wscan": (ctypes.c_int, [_i64, _p, _p, _p, _p, _p]),
    "fiveeq_resample_pick": (ctypes.c_int, [_i64, _p, ctypes.c_uint64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _p, _p]),
    "fiveeq_gather_rows_f64": (ctypes.c_int, [_i32, _i64, _i64, _p, _i64, _p, _p, _p]),
    "fiveeq_gather_rows_f32": (ctypes.c_int, [_i32, _i64, _i64, _p, _i64, _p, _p, _p]),
    "fiveeq_max_levels": (_i32, []),
    "fiveeq_max_windows": (_i32, []),
    "fiveeq_metrics_tile": (_i32, [_i32]),
    "fiveeq_metrics_unroll": (_i32, [_i32]),
    "fiveeq_traj_metrics_f64": (ctypes.c_int, [_i32, _i32, _i64, _i64, _p, _i64, _p, _i32, _p, _i32, _p, _p, _p, _i32, _p]),
    "fiveeq_traj_metrics_f32": (ctypes.c_int, [_i32, _i32, _i64, _i64, _p, _i64, _p, _i32, _p, _i32, _p, _p, _p, _i32, _p]),
    "fiveeq_max_smooth_window": (_i32, []),
    "fiveeq_smooth_tile": (_i32, [_i32]),
    "fiveeq_smooth_unroll": (_i32, [_i32]),
    # (n_scen, n_rows, n_members, ld, rows, scen_stride, window, n_tail, tail, tail_scen_stride, out, out_scen_stride, stream)
    "fiveeq_running_mean_f64": (ctypes.c_int, [_i32, _i32, _i64, _i64, _p, _i64, _i32, _i32, _p, _i64, _p, _i64, _p]),
    "fiveeq_running_mean_f32": (ctypes.c_int, [_i32, _i32, _i64, _i64, _p, _i64, _i32, _i32, _p, _i64, _p, _i64, _p]),
    # (n_scen, n_rows, n_members, ld, rows, scen_stride, steps, n_windows, windows, tsum, first_call, stream)
    "fiveeq_window_trends_f64": (ctypes.c_int, [_i32, _i32, _i64, _i64, _p, _i64, _p, _i32, _p, _p, _i32, _p]),
    "fiveeq_window_trends_f32": (ctypes.c_int, [_i32, _i32, _i64, _i64, _p, _i64, _p, _i32, _p, _p, _i32, _p]),
    "fiveeq_max_joint_rows": (_i32, []),
    "fiveeq_max_cond_bins": (_i32, []),
    "fiveeq_joint_tile": (_i32, [_i32]),
    "fiveeq_joint_chunks": (ctypes.c_int64, [_i64]),
    "fiveeq_joint_moments_words": (ctypes.c_int64, [_i32, _i32]),
    "fiveeq_cond_sums_words": (ctypes.c_int64, [_i32, _i32, _i32]),
    **{f"fiveeq_{name}_{sfx}": (ctypes.c_int, args) for sfx in ("f64", "f32") for name, args in (
        ("joint_moments", [_i64, _i32, _i64, _p, _i32, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _p]),
        ("cond_sums", [_i64, _i32, _i64, _p, _i32, _i64, _p, _p, _i32, _p, _p, _p, _p, _p, _p, _p]))},
    "fiveeq_max_score_quantities": (_i32, []),
    "fiveeq_score_tile": (_i32, [_i32]),
    "fiveeq_score_unroll": (_i32, [_i32]),
    "fiveeq_score_rows_f64": (ctypes.c_int, [_i32, _i32, _i64, _p, _i64, _i64, _p, _p, _i32, _p, _i64, _p]),
    "fiveeq_score_rows_f32": (ctypes.c_int, [_i32, _i32, _i64, _p, _i64, _i64, _p, _p, _i32, _p, _i64, _p]),
    "fiveeq_forcing_rows_tile": (_i32, [_i32]),
    "fiveeq_forcing_rows_f64": (ctypes.c_int, _FORCROWS),
    "fiveeq_forcing_rows_f32": (ctypes.c_int, _FORCROWS),
    "fiveeq_carbon_rows_tile": (_i32, [_i32]),
    "fiveeq_carbon_rows_unroll": (_i32, [_i32, _i32]),
    "fiveeq_carbon_rows_yrows": (_i32, []),
    "fiveeq_carbon_rows_f64": (ctypes.c_int, _CARBON),
    "fiveeq_carbon_rows_f32": (ctypes.c_int, _CARBON),
    "fiveeq_max_pulses": (_i32, []),
    "fiveeq_max_horizons": (_i32, []),
    "fiveeq_pulse_response_f64": (ctypes.c_int, _PULSE),
    "fiveeq_pulse_response_f32": (ctypes.c_int, _PULSE),
    "fiveeq_uniform_rows_f64": (ctypes.c_int, [_i64, _i64, _i32, _p, _p, ctypes.POINTER(ctypes.c_uint32), _p, _p]),
    "fiveeq_uniform_rows_f32": (ctypes.c_int, [_i64, _i64, _i32, _p, _p, ctypes.POINTER(ctypes.c_uint32), _p, _p]),
    "fiveeq_stream_copy_f64": (ctypes.c_int, [_i64, _p, _p, _p]),
    "fiveeq_stream_copy_wide_f64": (ctypes.c_int, [_i64, _p, _p, _p]),
    "fiveeq_stream_copy_nt_f64": (ctypes.c_int, [_i64, _p, _p, _p]),
    "fiveeq_busy": (ctypes.c_int, [_i64, _p, _p]),
    "fiveeq_math_probe_f64": (ctypes.c_int, [_i32, _i64, _p, _p, _p]),
    "fiveeq_math_probe_f32": (ctypes.c_int, [_i32, _i64, _p, _p, _p]),
}

_lib = None
# every source of the library, in the order csrc/Makefile (SRCS) hashes them
SOURCES = tuple(os.path.join(_HERE, "csrc", name) for name in (
    "fiveeq_capi.hip", "fiveeq_device.hpp", "fiveeq_math.hpp", "fiveeq_stats.hpp", "fiveeq_member.hpp", "fiveeq_step.hpp",
    "fiveeq_fused.hpp", "fiveeq_small.hpp", "fiveeq_summary.hpp", "fiveeq_wsummary.hpp", "fiveeq_resample.hpp",
    "fiveeq_metrics.hpp", "fiveeq_joint.hpp", "fiveeq_diag.hpp", "fiveeq_score.hpp", "fiveeq_forcrows.hpp", "fiveeq_pulse.hpp", "fiveeq_noise.hpp",
    "fiveeq_smooth.hpp", "fiveeq_carbon.hpp", "fiveeq_minor.hpp", "fiveeq_aerosol.hpp", "fiveeq_sea.hpp")) + (
    os.path.join(os.path.dirname(_HERE), "include", "fiveeq.h"),)


def source_hash():
    """sha256 (hex) of the library's sources as they lie in this tree, concatenated in SOURCES order — what
    csrc/Makefile stamps into the library; None when the tree carries no sources (an installed binary)."""
    import hashlib
    if not all(os.path.exists(p) for p in SOURCES):
        return None
    h = hashlib.sha256()
    for p in SOURCES:
        with open(p, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def load(path=None):
    """Load libfiveeq_hip.so and bind every entry point.  Raises if anything is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    lib_path = path or LIB_PATH
    if not os.path.exists(lib_path):
        raise ImportError(
            f"{lib_path} not found: the HIP extension is not built. "
            "Run `python -c 'import __graft_entry__ as g; g.build()'` (or `make -C fiveeqscm_amd/csrc`). "
            "There is no CPU fallback for the ensemble engine.")
    # torch (if present) must be imported first so that its bundled libamdhip64.so.7 is the
    # HIP runtime this library binds to by soname: one runtime per process, so torch tensor
    # pointers and torch streams are valid in our launches.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(lib_path)
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise ImportError(f"{lib_path} does not export {name}") from exc
        fn.restype = restype
        fn.argtypes = argtypes
    got = lib.fiveeq_abi_version()
    if got != ABI_VERSION:
        raise ImportError(f"{lib_path}: ABI version {got}, expected {ABI_VERSION}")
    if lib.fiveeq_sizeof_model() != ctypes.sizeof(Model):
        raise ImportError(f"{lib_path}: sizeof(fiveeq_model)={lib.fiveeq_sizeof_model()} but the ctypes "
                          f"mirror is {ctypes.sizeof(Model)} bytes")
    shape = (lib.fiveeq_metrics_tile(8), lib.fiveeq_metrics_tile(4), lib.fiveeq_metrics_unroll(1), lib.fiveeq_metrics_unroll(0))
    if shape != (METRICS_TILE_F64, METRICS_TILE_F32, METRICS_UNROLL, METRICS_UNROLL_NARROW):
        raise ImportError(f"{lib_path}: traj_metrics_kernel's tiles / unrolls are {shape}, the binding's constants say otherwise")
    joint = tuple(lib.fiveeq_joint_tile(k) for k in range(len(JOINT_TILE))) + (lib.fiveeq_max_joint_rows(), lib.fiveeq_max_cond_bins())
    if joint != JOINT_TILE + (MAX_JOINT_ROWS, MAX_COND_BINS):
        raise ImportError(f"{lib_path}: the joint passes' tiles / limits are {joint}, the binding's constants say otherwise")
    score = (lib.fiveeq_score_tile(8), lib.fiveeq_score_tile(4), lib.fiveeq_score_unroll(1), lib.fiveeq_score_unroll(0),
             lib.fiveeq_max_score_quantities())
    if score != (SCORE_TILE_F64, SCORE_TILE_F32, SCORE_UNROLL, SCORE_UNROLL_NARROW, MAX_SCORE_Q):
        raise ImportError(f"{lib_path}: score_rows_kernel's tiles / unrolls / limit are {score}, the binding's constants say otherwise")
    pulse = (lib.fiveeq_max_pulses(), lib.fiveeq_max_horizons())
    if pulse != (MAX_PULSES, MAX_HORIZONS):
        raise ImportError(f"{lib_path}: pulse_response_kernel's limits are {pulse}, the binding's constants say otherwise")
    if lib.fiveeq_max_smooth_window() != MAX_SMOOTH_WINDOW:
        raise ImportError(f"{lib_path}: running_mean_kernel's window limit is {lib.fiveeq_max_smooth_window()}, the binding's constant "
                          "says otherwise")
    # The library must have been compiled from the sources lying next to this file: a prebuilt .so that travelled to
    # another box, or survived a source edit, is refused instead of tested.  (FIVEEQ_ALLOW_STALE_LIB=1: experiment
    # variants built from patched sources, tools/ only.)
    want, got_hash = source_hash(), (lib.fiveeq_source_hash() or b"").decode()
    if want is not None and got_hash != want and os.environ.get("FIVEEQ_ALLOW_STALE_LIB") != "1":
        raise ImportError(f"{lib_path} was built from other sources (library {got_hash[:16]}, tree {want[:16]}): "
                          "run `make -C fiveeqscm_amd/csrc`")
    # ... and it must be the PRODUCT build: a variant compiled with experiment knobs (csrc/Makefile EXTRA=-D...) carries the same
    # source hash, and only fiveeq_build_flags() tells it apart
    flags = (lib.fiveeq_build_flags() or b"").decode().strip()
    if flags and os.environ.get("FIVEEQ_ALLOW_STALE_LIB") != "1":
        raise ImportError(f"{lib_path} is an experiment build ({flags}); set FIVEEQ_ALLOW_STALE_LIB=1 to load it (tools/ only)")
    if path is None:
        _lib = lib
    return lib


def build_flags(lib=None):
    """Experiment knobs the loaded library was compiled with ('' for the product build)."""
    return ((lib or load()).fiveeq_build_flags() or b"").decode().strip()


def check(lib, rc):
    if rc != OK:
        msg = lib.fiveeq_last_error()
        raise FiveEqError(rc, msg.decode("utf-8", "replace") if msg else "")
