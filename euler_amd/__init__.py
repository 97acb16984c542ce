"""euler_amd — host-side binding of libeuler_hip.so, the MI355X-native simulation path of
cgmb/euler (reference main.c: sim_init :209, sim_step :843, draw :953).

This module is plumbing over the C ABI declared in include/euler.h (ctypes; no torch types cross
the boundary).  There is NO CPU implementation behind it: if the shared library is missing, or
no gfx950 device is present, construction fails loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libeuler_hip.so")

# --- enums of include/euler.h ------------------------------------------------------------------
DOT_AUTO, DOT_SEQUENTIAL, DOT_TREE = 0, 1, 2
PRECOND_IC0, PRECOND_JACOBI, PRECOND_IC0_TILE, PRECOND_IC0_TILE2, PRECOND_IC0_TILE_MG = 0, 1, 2, 3, 4
(OPT_P_STEPS, OPT_TILE_STORE_AS, OPT_TILE_REVERSE, OPT_RESIDENT_CAP, OPT_GRID4_MIN_CELLS, OPT_SLAB_FUSION, OPT_RCCL_SMALL, OPT_RCCL_NO_EXCHANGE, OPT_MARKERS_ROWMAJOR,
 OPT_SA_RUN, OPT_NO_INTERIOR, OPT_BUILD_GATHER, OPT_RESIDENT_FORCE_TIMEOUT, OPT_MG_SPLIT_LEVEL, OPT_MG_SPLIT_ACTIVE, OPT_MARKERS_TWO_PASS, OPT_BUILD_TWO_PASS,
 OPT_VELOCITY_TWO_PASS, OPT_NO_TILE_MAP, OPT_PROFILE_STRIDE, OPT_TILE_STORE_Z, OPT_ADVECT_RK2, OPT_ADVECT_MACCORMACK) = range(1, 24)      # include/euler.h EULER_OPT_*
SWEEP_AUTO, SWEEP_BAND, SWEEP_SIMPLE = 0, 1, 2
PCG_F64, PCG_F32 = 0, 1
RESIDENT_AUTO, RESIDENT_OFF = 0, 1
IMAGE_COVERAGE, IMAGE_DYE, IMAGE_SPEED = 0, 1, 2      # EULER_IMAGE_*: euler_overview_rgb's modes
EDIT_SOLID, EDIT_CLEAR, EDIT_SINK, EDIT_SOURCE, EDIT_FILL, EDIT_DRAIN = range(6)      # EULER_EDIT_*: euler_edit_box's ops
# euler_overview_px (include/euler.h): one pixel of the whole-domain overview = one box of interior cells
OVERVIEW_DTYPE = np.dtype({"names": ["cells", "solid", "sink", "water", "marks", "max_speed2", "dye"],
                           "formats": [np.uint32, np.uint32, np.uint32, np.uint32, np.uint32, np.float32, (np.uint64, 3)],
                           "offsets": [0, 4, 8, 12, 16, 20, 24], "itemsize": 48})
# euler_diag (include/euler.h): the record of the flow diagnostics, and the doubles euler_diag_derive forms from it
DIAG_CROWDED = 8      # EULER_DIAG_CROWDED
DIAG_DTYPE = np.dtype({"names": ["cells", "fluid", "markers", "crowded", "mass_x", "mass_y", "div_l1", "ke_hi", "ke_lo", "count_max", "nonfinite", "max_div", "max_speed2"],
                       "formats": [np.uint64] * 9 + [np.uint32, np.uint32, np.float32, np.float32],
                       "offsets": [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80, 84], "itemsize": 88})
# euler_flow_px (include/euler.h): one pixel of the flow raster; EULER_FLOW_* flags of euler_flow_raster, EULER_PAINT_* fields of euler_flow_paint
FLOW_PRESSURE = 1
PAINT_VORTICITY, PAINT_PRESSURE, PAINT_SPEED = 0, 1, 2
FLOW_DTYPE = np.dtype({"names": ["cells", "water", "nodes", "nonfinite", "u_pos", "u_neg", "v_pos", "v_neg", "w_pos", "w_neg", "p_sum", "max_speed2", "max_abs_w", "max_p", "reserved"],
                       "formats": [np.uint32] * 4 + [np.uint64] * 7 + [np.float32] * 3 + [np.uint32],
                       "offsets": [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80, 84], "itemsize": 88})
# euler_gauge, euler_gauge_rec (include/euler.h): one instrument of euler_gauges and its record; the doubles euler_gauge_derive forms from a record
GAUGE_LEVEL, GAUGE_PRESSURE, GAUGE_FORCE, GAUGE_FLUX = range(4)      # EULER_GAUGE_*
GAUGES_MAX = 1024
GAUGE_DTYPE = np.dtype({"names": ["kind", "x0", "y0", "x1", "y1", "reserved"], "formats": [np.int32] * 6, "offsets": [0, 4, 8, 12, 16, 20], "itemsize": 24})
GAUGE_REC_DTYPE = np.dtype({"names": ["cells", "fluid", "lo_x", "hi_x", "lo_y", "hi_y", "terms", "nonfinite", "a_pos", "a_neg", "b_pos", "b_neg", "max_a", "max_b"],
                            "formats": [np.uint32] * 8 + [np.uint64] * 4 + [np.float32] * 2,
                            "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 68], "itemsize": 72})
# euler_forcing, euler_force_box (include/euler.h): the forcing record of euler_set_forcing and one force box ("pump")
FORCE_BOXES_MAX = 64
FORCING_DTYPE = np.dtype({"names": ["gx", "gy", "shake_x", "shake_y", "shake_hz", "shake_phase", "nboxes", "reserved", "reserved2"],
                          "formats": [np.float32] * 4 + [np.float64] * 2 + [np.int32] * 2 + [np.float64],
                          "offsets": [0, 4, 8, 12, 16, 24, 32, 36, 40], "itemsize": 48})
FORCE_BOX_DTYPE = np.dtype({"names": ["x0", "y0", "x1", "y1", "fx", "fy"], "formats": [np.int32] * 4 + [np.float32] * 2, "offsets": [0, 4, 8, 12, 16, 20], "itemsize": 24})
# euler_heat, euler_heat_box (include/euler.h): the record of euler_set_heat and one heat box; EULER_HEAT_FIX / _RATE
HEAT_BOXES_MAX = 64
HEAT_FIX, HEAT_RATE = 0, 1
HEAT_DTYPE = np.dtype({"names": ["ambient", "beta", "kappa", "source_t", "nboxes", "reserved", "reserved2"],
                       "formats": [np.float32] * 4 + [np.int32] * 2 + [np.float64], "offsets": [0, 4, 8, 12, 16, 20, 24], "itemsize": 32})
HEAT_PX_DTYPE = np.dtype({"names": ["cells", "water", "t_pos", "t_neg", "max_above", "max_below"], "formats": [np.uint32] * 2 + [np.uint64] * 2 + [np.float32] * 2,
                          "offsets": [0, 4, 8, 16, 24, 28], "itemsize": 32})      # euler_heat_px: one pixel of euler_heat_raster
HEAT_BOX_DTYPE = np.dtype({"names": ["x0", "y0", "x1", "y1", "value", "kind"], "formats": [np.int32] * 4 + [np.float32, np.int32], "offsets": [0, 4, 8, 12, 16, 20], "itemsize": 24})
# euler_body, euler_body_state (include/euler.h): one moving body of euler_set_bodies and its position at a time
BODIES_MAX = 16
BODY_DTYPE = np.dtype({"names": ["x", "y", "hz", "phase", "vx", "vy", "amp_x", "amp_y", "w", "h", "reserved"],
                       "formats": [np.float64] * 4 + [np.float32] * 4 + [np.int32] * 2 + [(np.int32, 2)],
                       "offsets": [0, 8, 16, 24, 32, 36, 40, 44, 48, 52, 56], "itemsize": 64})
BODY_STATE_DTYPE = np.dtype({"names": ["px", "py", "ox", "oy"], "formats": [np.float64] * 2 + [np.int32] * 2, "offsets": [0, 8, 16, 20], "itemsize": 24})
# euler_reseed, euler_reseed_stats (include/euler.h): the marker density control's record and its totals
RESEED_DTYPE = np.dtype({"names": ["thin_above", "fill_holes", "max_cells", "max_fill", "reserved"], "formats": [np.int32] * 4 + [(np.int32, 4)],
                         "offsets": [0, 4, 8, 12, 16], "itemsize": 32})
RESEED_STATS_DTYPE = np.dtype({"names": ["removed", "added", "cells_thinned", "deferred"], "formats": [np.uint64] * 4, "offsets": [0, 8, 16, 24], "itemsize": 32})
# the run-long envelopes (include/euler.h EULER_ENV_*, euler_envelope_px; docs/envelope.md): the channel bits and one pixel of euler_envelope_raster
ENV_ARRIVAL, ENV_WET, ENV_SPEED, ENV_PRESSURE, ENV_ALL = 1, 2, 4, 8, 15
ENV_NAMES = {ENV_ARRIVAL: "arrival", ENV_WET: "wet", ENV_SPEED: "speed", ENV_PRESSURE: "pressure"}
ENVELOPE_PX_DTYPE = np.dtype({"names": ["cells", "touched", "arrival_min", "arrival_max", "wet_max", "speed2_max", "p_max", "reserved"],
                              "formats": [np.uint32] * 8, "offsets": [0, 4, 8, 12, 16, 20, 24, 28], "itemsize": 32})
# euler_tracer (include/euler.h): one passive tracer; EULER_TRACER_* flag bits; EULER_TRACER_RASTER_ALL of euler_tracer_raster
TRACERS_MAX = 1 << 22
TRACER_WET, TRACER_RETIRED, TRACER_IN_SOLID, TRACER_IN_SINK, TRACER_LOST, TRACER_WAS_DRY = 1, 2, 4, 8, 16, 32
TRACER_RASTER_ALL = 1
TRACER_DTYPE = np.dtype({"names": ["x", "y", "path", "age", "wet_time", "substeps", "flags", "reserved"],
                         "formats": [np.float32] * 5 + [np.uint32] * 3, "offsets": [0, 4, 8, 12, 16, 20, 24, 28], "itemsize": 32})
# the SETT chunk of a session file (csrc/euler_host.h eu_session_settings, docs/session.md); EULER_SESSION_* flags of euler_load_session
SESSION_IGNORE_SETTINGS = 1
SESSION_OPTS = 32
SESSION_SETTINGS_DTYPE = np.dtype({"names": ["max_iterations", "dot_mode", "precond", "tile_records", "sweep_mode", "max_substeps", "rainbow", "pcg_precision", "resident",
                                             "pcg_poll_interval", "viscosity_bits", "frame_time_bits", "tol", "nopts", "reserved", "opt"],
                                   "formats": [np.int32] * 10 + [np.uint32] * 2 + [np.float64] + [np.int32] * 2 + [(np.int64, SESSION_OPTS)],
                                   "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 56, 60, 64], "itemsize": 320})
SESSION_STAT_KEYS = ("last_substeps", "last_pcg_iterations", "last_residual", "last_dt", "pad", "marker_dt_events", "marker_multi_events")      # the STAT chunk, 40 bytes
SESSION_STAT_FORMAT = "<iidfIQQ"
SESSION_TAGS = (b"TIME", b"FORC", b"HEAT", b"TRAC", b"BODY", b"RSED", b"SETT", b"STAT", b"END\0")      # the chunks of a session file, in file order
GAUGE_VALUES = ("a", "b", "mean_a", "depth")      # euler_gauge_values, four doubles
DIAG_VALUES = ("mean_abs_div", "kinetic_energy", "com_x", "com_y", "markers_per_cell", "crowded_fraction")      # euler_diag_values, six doubles
(F_U, F_V, F_UTMP, F_VTMP, F_SOLID, F_SOURCE, F_SINK, F_COUNT, F_PREV_COUNT, F_MARKERS, F_PRECON,
 F_PRESSURE, F_PCG_B, F_PCG_R, F_PCG_Z, F_PCG_S, F_PCG_Q, F_CELLMASK,
 F_DYE_R, F_DYE_G, F_DYE_B, F_DYE_RTMP, F_DYE_GTMP, F_DYE_BTMP, F_MARKER_KEYS) = range(25)
(STAGE_ADVECT_MARKERS, STAGE_REFRESH_COUNTS, STAGE_SOURCES, STAGE_EXTRAPOLATE, STAGE_ADVECT_VELOCITY,
 STAGE_PROJECT) = range(6)
(OP_BUILD_SYSTEM, OP_PRECON_FACTOR, OP_FORWARD_SOLVE, OP_BACKWARD_SOLVE, OP_APPLY_A, OP_DOT_ZR, OP_DOT_ZS,
 OP_INF_NORM_R, OP_UPDATE_PR, OP_UPDATE_SEARCH) = range(10)

_FIELD_DTYPE = {
    F_U: np.float32, F_V: np.float32, F_UTMP: np.float32, F_VTMP: np.float32,
    F_SOLID: np.uint8, F_SOURCE: np.uint8, F_SINK: np.uint8, F_COUNT: np.uint8, F_PREV_COUNT: np.uint8,
    F_MARKERS: np.float32, F_PRECON: np.float64, F_PRESSURE: np.float64, F_PCG_B: np.float64,
    F_PCG_R: np.float64, F_PCG_Z: np.float64, F_PCG_S: np.float64, F_PCG_Q: np.float64, F_CELLMASK: np.uint8,
    F_DYE_R: np.float32, F_DYE_G: np.float32, F_DYE_B: np.float32,
    F_DYE_RTMP: np.float32, F_DYE_GTMP: np.float32, F_DYE_BTMP: np.float32, F_MARKER_KEYS: np.uint32,
}


class EulerError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libeuler_hip error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("X", C.c_int32), ("Y", C.c_int32), ("device", C.c_int32),
        ("max_iterations", C.c_int32), ("tol", C.c_double), ("dot_mode", C.c_int32), ("precond", C.c_int32),
        ("sweep_mode", C.c_int32), ("max_substeps", C.c_int32), ("frame_time", C.c_float),
        ("viscosity", C.c_float), ("pcg_poll_interval", C.c_int32), ("rainbow", C.c_int32),
        ("precond_tile_records", C.c_int32), ("slab_rank", C.c_int32), ("slab_nranks", C.c_int32),
        ("slab_band_lo", C.c_int32), ("slab_band_hi", C.c_int32), ("pcg_precision", C.c_int32), ("resident", C.c_int32),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("frames", C.c_uint64), ("total_substeps", C.c_uint64), ("total_pcg_iterations", C.c_uint64),
        ("last_substeps", C.c_int32), ("last_pcg_iterations", C.c_int32), ("last_residual", C.c_double),
        ("last_dt", C.c_float), ("n_markers", C.c_uint64), ("source_exhausted", C.c_int32),
        ("rng_state", C.c_uint64), ("marker_dt_events", C.c_uint64), ("marker_multi_events", C.c_uint64),
        ("fluid_cells", C.c_uint64),
    ]


_lib = None

EXPORTS = [
    "euler_config_default", "euler_create", "euler_destroy", "euler_last_error", "euler_abi_version",
    "euler_load_scenario_mem", "euler_load_scenario_file", "euler_load_half_tank", "euler_load_half_tanks", "euler_parse_scenario",
    "euler_seed_markers", "euler_step", "euler_timestep", "euler_substep", "euler_stage", "euler_pcg_op", "euler_set_precond", "euler_set_solver",
    "euler_get_field", "euler_set_field", "euler_set_markers", "euler_set_rng", "euler_get_stats",
    "euler_field_bytes", "euler_render", "euler_render_grids", "euler_render_grids_rgb", "euler_colorize", "euler_profile_enable",
    "euler_profile_class_count", "euler_profile_class_name", "euler_profile_get", "euler_profile_reset",
    "euler_measure_copy_bandwidth", "euler_measure_exchange", "euler_device_name", "euler_hbm_bytes", "euler_sweep_timeline", "euler_save_state", "euler_load_state", "euler_save_session", "euler_load_session", "euler_set_comm", "euler_set_stream", "euler_slab_info",
    "euler_rccl_unique_id", "euler_rccl_version", "euler_set_comm_rccl", "euler_comm_calls",
    "euler_p2p_export", "euler_p2p_connect", "euler_p2p_disconnect", "euler_p2p_calls", "euler_resident_info",
    "euler_set_option", "euler_get_option",
    "euler_overview", "euler_overview_text", "euler_overview_rgb", "euler_render_fit",
    "euler_diagnostics", "euler_diag_derive",
    "euler_overview_box", "euler_marker_raster", "euler_view_text", "euler_render_view",
    "euler_edit_box",
    "euler_flow_raster", "euler_flow_paint",
    "euler_gauges", "euler_gauge_derive",
    "euler_forcing_default", "euler_set_forcing", "euler_get_forcing", "euler_forcing_at", "euler_get_time", "euler_set_time",
    "euler_heat_default", "euler_set_heat", "euler_get_heat", "euler_heat_get_field", "euler_heat_set_field", "euler_heat_fill", "euler_heat_raster", "euler_heat_paint",
    "euler_body_at", "euler_set_bodies", "euler_get_bodies",
    "euler_set_reseed", "euler_get_reseed",
    "euler_set_envelope", "euler_get_envelope", "euler_envelope_reset", "euler_envelope_get_field", "euler_envelope_set_field", "euler_envelope_raster", "euler_envelope_rgb",
    "euler_tracers_add", "euler_tracers_count", "euler_tracers_get", "euler_tracers_clear", "euler_tracer_raster", "euler_tracer_paint",
]


def load_library():
    """dlopen libeuler_hip.so (built in-tree by `make -C euler_amd/csrc`). Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("EULER_HIP_LIB", LIB_PATH)   # development: an alternative build of the same library
    if not os.path.exists(path):
        raise ImportError(
            "euler_amd: %s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C euler_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    L = C.CDLL(path)
    vp, i32, u64, f32, f64 = C.c_void_p, C.c_int32, C.c_uint64, C.c_float, C.c_double
    sig = {
        "euler_config_default": (C.c_int, [C.POINTER(Config)]),
        "euler_create": (C.c_int, [C.POINTER(Config), C.POINTER(vp)]),
        "euler_destroy": (None, [vp]),
        "euler_last_error": (C.c_char_p, []),
        "euler_abi_version": (C.c_int, []),
        "euler_load_scenario_mem": (C.c_int, [vp, C.c_char_p, i32, i32]),
        "euler_load_scenario_file": (C.c_int, [vp, C.c_char_p, i32]),
        "euler_load_half_tank": (C.c_int, [vp]),
        "euler_load_half_tanks": (C.c_int, [vp, i32]),
        "euler_parse_scenario": (C.c_int, [C.c_char_p, i32, i32, i32, i32, vp, vp, vp, vp]),
        "euler_seed_markers": (C.c_int, [vp, i32, i32, C.POINTER(u64), vp, C.POINTER(u64)]),
        "euler_step": (C.c_int, [vp]),
        "euler_timestep": (C.c_int, [vp, f32, C.POINTER(f32)]),
        "euler_substep": (C.c_int, [vp, f32]),
        "euler_stage": (C.c_int, [vp, i32, f32]),
        "euler_pcg_op": (C.c_int, [vp, i32, f32, f64, C.POINTER(f64)]),
        "euler_set_precond": (C.c_int, [vp, i32, i32]),
        "euler_set_solver": (C.c_int, [vp, i32, f64]),
        "euler_get_field": (C.c_int, [vp, i32, vp, C.c_size_t]),
        "euler_set_field": (C.c_int, [vp, i32, vp, C.c_size_t]),
        "euler_set_markers": (C.c_int, [vp, vp, u64]),
        "euler_set_rng": (C.c_int, [vp, u64, i32]),
        "euler_get_stats": (C.c_int, [vp, C.POINTER(Stats)]),
        "euler_field_bytes": (C.c_size_t, [vp, i32]),
        "euler_render": (C.c_int, [vp, i32, i32, C.c_char_p, i32, C.POINTER(i32)]),
        "euler_render_grids": (C.c_int, [vp, vp, vp, i32, i32, i32, i32, C.c_char_p, i32, C.POINTER(i32)]),
        "euler_render_grids_rgb": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, C.c_char_p, i32, C.POINTER(i32)]),
        "euler_colorize": (C.c_int, [vp]),
        "euler_profile_enable": (C.c_int, [vp, u64]),
        "euler_profile_class_count": (C.c_int, []),
        "euler_profile_class_name": (C.c_char_p, [i32]),
        "euler_profile_get": (C.c_int, [vp, i32, C.POINTER(f64), C.POINTER(u64)]),
        "euler_profile_reset": (C.c_int, [vp]),
        "euler_resident_info": (C.c_int, [vp, C.POINTER(u64)]),
        "euler_measure_copy_bandwidth": (C.c_int, [vp, C.c_size_t, i32, C.POINTER(f64)]),
        "euler_measure_exchange": (C.c_int, [vp, i32, i32, i32, C.POINTER(f64)]),
        "euler_device_name": (C.c_int, [vp, C.c_char_p, i32]),
        "euler_hbm_bytes": (u64, [vp]),
        "euler_sweep_timeline": (C.c_int, [vp, C.POINTER(C.c_uint64), i32]),
        "euler_save_state": (C.c_int, [vp, C.c_char_p]),
        "euler_load_state": (C.c_int, [vp, C.c_char_p]),
        "euler_save_session": (C.c_int, [vp, C.c_char_p]),
        "euler_load_session": (C.c_int, [vp, C.c_char_p, C.c_uint32]),
        "euler_set_comm": (C.c_int, [vp, vp, i32]),                 # euler_amd/slab.py passes a CommOps struct
        "euler_set_stream": (C.c_int, [vp, vp]),
        "euler_slab_info": (C.c_int, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "euler_rccl_unique_id": (C.c_int, [vp, i32]),
        "euler_rccl_version": (C.c_int, []),
        "euler_set_comm_rccl": (C.c_int, [vp, vp, i32, i32, i32, i32]),
        "euler_comm_calls": (C.c_int, [vp, C.POINTER(u64)]),
        "euler_p2p_export": (C.c_int, [vp, vp, i32]),
        "euler_p2p_connect": (C.c_int, [vp, vp, i32]),
        "euler_p2p_disconnect": (C.c_int, [vp]),
        "euler_p2p_calls": (C.c_int, [vp, C.POINTER(u64)]),
        "euler_set_option": (C.c_int, [vp, i32, C.c_int64]),
        "euler_get_option": (C.c_int, [vp, i32, C.POINTER(C.c_int64)]),
        "euler_overview": (C.c_int, [vp, i32, i32, vp, C.c_size_t]),
        "euler_overview_text": (C.c_int, [vp, i32, i32, i32, C.c_char_p, i32, C.POINTER(i32)]),
        "euler_overview_rgb": (C.c_int, [vp, i32, i32, i32, f32, vp, C.c_size_t]),
        "euler_render_fit": (C.c_int, [vp, i32, i32, C.c_char_p, i32, C.POINTER(i32)]),
        "euler_diagnostics": (C.c_int, [vp, i32, i32, i32, i32, vp, C.c_size_t]),
        "euler_diag_derive": (C.c_int, [vp, vp]),
        "euler_overview_box": (C.c_int, [vp, i32, i32, i32, i32, i32, i32, vp, C.c_size_t]),
        "euler_marker_raster": (C.c_int, [vp, i32, i32, i32, i32, i32, vp, C.c_size_t]),
        "euler_view_text": (C.c_int, [vp, vp, i32, i32, i32, i32, C.c_char_p, i32, C.POINTER(i32)]),
        "euler_render_view": (C.c_int, [vp, i32, i32, i32, i32, i32, i32, C.c_char_p, i32, C.POINTER(i32)]),
        "euler_edit_box": (C.c_int, [vp, i32, i32, i32, i32, i32]),
        "euler_flow_raster": (C.c_int, [vp, i32, i32, i32, i32, i32, i32, i32, vp, C.c_size_t]),
        "euler_flow_paint": (C.c_int, [vp, vp, i32, i32, i32, f64]),
        "euler_gauges": (C.c_int, [vp, vp, i32, vp, C.c_size_t]),
        "euler_gauge_derive": (C.c_int, [vp, i32, vp]),
        "euler_forcing_default": (C.c_int, [vp]),
        "euler_set_forcing": (C.c_int, [vp, vp, vp]),
        "euler_get_forcing": (C.c_int, [vp, vp, vp, i32]),
        "euler_forcing_at": (C.c_int, [vp, f64, C.POINTER(f32)]),
        "euler_get_time": (C.c_int, [vp, C.POINTER(f64)]),
        "euler_set_time": (C.c_int, [vp, f64]),
        "euler_heat_default": (C.c_int, [vp]),
        "euler_set_heat": (C.c_int, [vp, vp, vp]),
        "euler_get_heat": (C.c_int, [vp, vp, vp, i32]),
        "euler_heat_get_field": (C.c_int, [vp, vp, C.c_size_t]),
        "euler_heat_set_field": (C.c_int, [vp, vp, C.c_size_t]),
        "euler_heat_fill": (C.c_int, [vp, i32, i32, i32, i32, f32]),
        "euler_heat_raster": (C.c_int, [vp, i32, i32, i32, i32, i32, i32, vp, C.c_size_t]),
        "euler_heat_paint": (C.c_int, [vp, vp, i32, i32, f32, f64]),
        "euler_body_at": (C.c_int, [vp, f64, i32, i32, vp]),
        "euler_set_bodies": (C.c_int, [vp, vp, i32]),
        "euler_get_bodies": (C.c_int, [vp, vp, i32, vp, C.POINTER(i32)]),
        "euler_set_reseed": (C.c_int, [vp, vp]),
        "euler_get_reseed": (C.c_int, [vp, vp, vp]),
        "euler_set_envelope": (C.c_int, [vp, C.c_uint32]),
        "euler_get_envelope": (C.c_int, [vp, C.POINTER(C.c_uint32), C.POINTER(u64)]),
        "euler_envelope_reset": (C.c_int, [vp]),
        "euler_envelope_get_field": (C.c_int, [vp, i32, vp, C.c_size_t]),
        "euler_envelope_set_field": (C.c_int, [vp, i32, vp, C.c_size_t]),
        "euler_envelope_raster": (C.c_int, [vp, i32, i32, i32, i32, i32, i32, vp, C.c_size_t]),
        "euler_envelope_rgb": (C.c_int, [vp, i32, i32, i32, f64, vp, C.c_size_t]),
        "euler_tracers_add": (C.c_int, [vp, vp, C.c_size_t]),
        "euler_tracers_count": (C.c_int, [vp, C.POINTER(C.c_size_t)]),
        "euler_tracers_get": (C.c_int, [vp, C.c_size_t, C.c_size_t, vp, C.c_size_t]),
        "euler_tracers_clear": (C.c_int, [vp]),
        "euler_tracer_raster": (C.c_int, [vp, i32, i32, i32, i32, i32, i32, i32, vp, C.c_size_t]),
        "euler_tracer_paint": (C.c_int, [vp, vp, i32, i32, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)   # AttributeError here = a symbol include/euler.h declares is not exported
        fn.restype = res
        fn.argtypes = args
    L.eu_tracer_lattice.restype = C.c_size_t      # (internal, euler_host.h: the lattice of a box as the command line seeds it)
    L.eu_tracer_lattice.argtypes = [i32, i32, i32, i32, i32, vp]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise EulerError(rc, load_library().euler_last_error().decode(errors="replace"))


def _check_host(rc, who):
    """a host-only formatter that refuses leaves no message behind"""
    if rc != 0:
        raise EulerError(rc, "%s refused its arguments" % who)


# --- host-only helpers (no GPU) ------------------------------------------------------------------
def parse_scenario(text, X, Y, upscale=False):
    """Scenario text -> (solid, source, sink, fluid) uint8 [Y][X] (reference main.c:217-252)."""
    if isinstance(text, str):
        text = text.encode()
    out = [np.zeros((Y, X), np.uint8) for _ in range(4)]
    _check(load_library().euler_parse_scenario(text, len(text), X, Y, int(upscale), *[a.ctypes.data for a in out]))
    return tuple(out)


def seed_markers(fluid, rng_state=0x9bd185c449534b91):
    """Four jittered markers per fluid cell (reference main.c:255-266). Returns (markers[n,2], rng_state)."""
    fluid = np.ascontiguousarray(fluid, np.uint8)
    Y, X = fluid.shape
    m = np.zeros((4 * X * Y, 2), np.float32)
    st, n = C.c_uint64(rng_state), C.c_uint64(0)
    _check(load_library().euler_seed_markers(fluid.ctypes.data, X, Y, C.byref(st), m.ctypes.data, C.byref(n)))
    return m[: n.value].copy(), st.value


def render_grids(solid, sink, count, wx, wy, rgb=None):
    """draw_rows() over host grids (reference main.c:914-951); rgb = (r, g, b) float grids for --rainbow."""
    Y, X = count.shape
    L = load_library()
    n = C.c_int32(0)
    a = [np.ascontiguousarray(g, np.uint8) for g in (solid, sink, count)]
    ptrs = [g.ctypes.data for g in a]
    fn = L.euler_render_grids
    if rgb is not None:
        a += [np.ascontiguousarray(g, np.float32) for g in rgb]
        ptrs = [g.ctypes.data for g in a]
        fn = L.euler_render_grids_rgb
    _check(fn(*ptrs, X, Y, wx, wy, None, 0, C.byref(n)))
    buf = C.create_string_buffer(max(n.value, 1))
    _check(fn(*ptrs, X, Y, wx, wy, buf, n.value, C.byref(n)))
    return buf.raw[: n.value]


def _overview_records(px):
    px = np.ascontiguousarray(px, OVERVIEW_DTYPE)
    if px.ndim != 2 or px.size == 0:
        raise ValueError("overview records: an array of shape (h, w)")
    return px


def overview_text(px, rainbow=False):
    """The fit-to-window frame of overview records (euler_overview_text): one glyph per record through the formatter of draw()."""
    px = _overview_records(px)
    h, w = px.shape
    L = load_library()
    n = C.c_int32(0)
    _check(L.euler_overview_text(px.ctypes.data, w, h, int(rainbow), None, 0, C.byref(n)))
    buf = C.create_string_buffer(max(n.value, 1))
    _check(L.euler_overview_text(px.ctypes.data, w, h, int(rainbow), buf, n.value, C.byref(n)))
    return buf.raw[: n.value]


def overview_rgb(px, mode=IMAGE_COVERAGE, speed_scale=1.0):
    """Overview records -> uint8 (h, w, 3), row 0 = top (euler_overview_rgb)."""
    px = _overview_records(px)
    h, w = px.shape
    rgb = np.empty((h, w, 3), np.uint8)
    _check(load_library().euler_overview_rgb(px.ctypes.data, w, h, int(mode), float(speed_scale), rgb.ctypes.data, rgb.nbytes))
    return rgb


def view_text(cells, raster, scale, rainbow=False):
    """The magnified frame of a box (euler_view_text): cells = its overview at one cell per record, shape (bh, bw); raster = the marker counts of
    euler_marker_raster over the same box, shape (bh * scale, bw * scale); every cell becomes scale x scale glyphs."""
    cells = _overview_records(cells)
    bh, bw = cells.shape
    raster = np.ascontiguousarray(raster, np.uint32)
    if raster.shape != (bh * int(scale), bw * int(scale)):
        raise ValueError("view_text: a raster of shape (%d, %d)" % (bh * int(scale), bw * int(scale)))
    L = load_library()
    n = C.c_int32(0)
    _check(L.euler_view_text(cells.ctypes.data, raster.ctypes.data, bw, bh, int(scale), int(rainbow), None, 0, C.byref(n)))
    buf = C.create_string_buffer(max(n.value, 1))
    _check(L.euler_view_text(cells.ctypes.data, raster.ctypes.data, bw, bh, int(scale), int(rainbow), buf, n.value, C.byref(n)))
    return buf.raw[: n.value]


def flow_paint(flow, px, field, scale):
    """A painted copy of the overview records px: their dye sums show `field` (PAINT_VORTICITY, PAINT_PRESSURE, PAINT_SPEED) of the flow records of the
    same box, raster and state at `scale` (euler_flow_paint), so that overview_text / view_text with rainbow and overview_rgb(IMAGE_DYE) draw it."""
    px = _overview_records(px).copy()
    flow = np.ascontiguousarray(flow, FLOW_DTYPE)
    if flow.shape != px.shape:
        raise ValueError("flow_paint: flow records of shape %r for overview records of shape %r" % (flow.shape, px.shape))
    h, w = px.shape
    _check_host(load_library().euler_flow_paint(flow.ctypes.data, px.ctypes.data, w, h, int(field), float(scale)), "euler_flow_paint")
    return px


def write_ppm(path, rgb):
    """uint8 (h, w, 3) -> a binary PPM (P6, maxval 255)."""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    if rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("write_ppm: an array of shape (h, w, 3)")
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
        f.write(rgb.tobytes())


def diag_derive(rec):
    """An euler_diag record (DIAG_DTYPE) -> the dict of euler_diag_derive's doubles (host only)."""
    rec = np.ascontiguousarray(rec, DIAG_DTYPE).reshape(1)
    out = np.zeros(len(DIAG_VALUES), np.float64)
    _check(load_library().euler_diag_derive(rec.ctypes.data, out.ctypes.data))
    return dict(zip(DIAG_VALUES, (float(x) for x in out)))


def gauge_derive(rec, kind):
    """One euler_gauge_rec record (GAUGE_REC_DTYPE) of a gauge of `kind` -> the dict of euler_gauge_derive's doubles (host only)."""
    rec = np.ascontiguousarray(rec, GAUGE_REC_DTYPE).reshape(1)
    out = np.zeros(len(GAUGE_VALUES), np.float64)
    _check_host(load_library().euler_gauge_derive(rec.ctypes.data, int(kind), out.ctypes.data), "euler_gauge_derive")
    return dict(zip(GAUGE_VALUES, (float(x) for x in out)))


def forcing_default():
    """The default forcing record (euler_forcing_default): gravity (0, -10), no shake, no boxes; FORCING_DTYPE, shape ()."""
    f = np.zeros((), FORCING_DTYPE)
    _check_host(load_library().euler_forcing_default(f.ctypes.data), "euler_forcing_default")
    return f


def forcing_record(gravity=(0.0, -10.0), shake=None, nboxes=0):
    """A forcing record (FORCING_DTYPE, shape ()): gravity = (gx, gy); shake = None or (sx, sy, hz[, phase in radians])."""
    f = forcing_default()
    f["gx"], f["gy"] = gravity
    if shake is not None:
        f["shake_x"], f["shake_y"], f["shake_hz"] = shake[:3]
        f["shake_phase"] = shake[3] if len(shake) > 3 else 0.0
    f["nboxes"] = nboxes
    return f


def forcing_at(f, t):
    """The uniform acceleration (ax, ay) of forcing record f at simulated time t, two np.float32 (euler_forcing_at, host only)."""
    f = np.ascontiguousarray(f, FORCING_DTYPE).reshape(1)
    a = (C.c_float * 2)()
    _check_host(load_library().euler_forcing_at(f.ctypes.data, float(t), a), "euler_forcing_at")
    return np.float32(a[0]), np.float32(a[1])


def body(size, at, velocity=(0.0, 0.0), amplitude=(0.0, 0.0), hz=0.0, phase=0.0):
    """A moving body (BODY_DTYPE, shape ()): size = (w, h) in cells, at = the lower-left corner at t = 0, velocity in cells per second, amplitude, hz and
    phase (radians) of the harmonic part: p(t) = at + velocity t + amplitude sin(2 pi hz t + phase)."""
    b = np.zeros((), BODY_DTYPE)
    b["w"], b["h"] = size
    b["x"], b["y"] = at
    b["vx"], b["vy"] = velocity
    b["amp_x"], b["amp_y"] = amplitude
    b["hz"], b["phase"] = hz, phase
    return b


def bodies_array(bodies):
    """A list of body records, or of the argument tuples of body(), as one contiguous array of BODY_DTYPE."""
    if isinstance(bodies, np.ndarray) and bodies.dtype == BODY_DTYPE:
        return np.ascontiguousarray(bodies).reshape(-1)
    out = np.zeros(len(bodies), BODY_DTYPE)
    for k, b in enumerate(bodies):
        out[k] = b if isinstance(b, np.ndarray) else body(*b)
    return out


def reseed(thin_above=0, fill_holes=False, max_cells=0, max_fill=0):
    """A record of the marker density control (RESEED_DTYPE, shape (); euler_set_reseed, docs/reseed.md): a cell whose count byte exceeds thin_above (0: no
    thinning, else 4 ... 254) is thinned to one marker per quarter-cell square, fill_holes puts a marker into every single-cell hole in the water; max_cells and
    max_fill bound the cells treated per pass (0: 65536)."""
    r = np.zeros((), RESEED_DTYPE)
    r["thin_above"], r["fill_holes"], r["max_cells"], r["max_fill"] = int(thin_above), int(fill_holes), int(max_cells), int(max_fill)
    return r


def body_at(b, t, X, Y):
    """Where body record b stands at simulated time t on an X x Y grid (euler_body_at, host only): BODY_STATE_DTYPE of shape () - the clamped continuous
    position (px, py) and the origin (ox, oy) of its rectangle of cells."""
    b = np.ascontiguousarray(b, BODY_DTYPE).reshape(1)
    st = np.zeros((), BODY_STATE_DTYPE)
    _check_host(load_library().euler_body_at(b.ctypes.data, float(t), int(X), int(Y), st.ctypes.data), "euler_body_at")
    return st


def heat_default():
    """The default heat record (euler_heat_default): ambient, beta, kappa, source_t 0, no boxes; HEAT_DTYPE, shape ()."""
    h = np.zeros((), HEAT_DTYPE)
    _check_host(load_library().euler_heat_default(h.ctypes.data), "euler_heat_default")
    return h


def heat_paint(heat, px, ambient, scale):
    """A painted copy of the overview records px: their dye sums show the mean temperature above (white to red) and below (white to blue) `ambient` of the
    heat records of the same box, raster and state, saturated at `scale` (euler_heat_paint), so that overview_text / view_text with rainbow and
    overview_rgb(IMAGE_DYE) draw it."""
    px = _overview_records(px).copy()
    heat = np.ascontiguousarray(heat, HEAT_PX_DTYPE)
    if heat.shape != px.shape:
        raise ValueError("heat_paint: heat records of shape %r for overview records of shape %r" % (heat.shape, px.shape))
    h, w = px.shape
    _check_host(load_library().euler_heat_paint(heat.ctypes.data, px.ctypes.data, w, h, float(ambient), float(scale)), "euler_heat_paint")
    return px


def envelope_rgb(px, channel, scale):
    """Envelope records (ENVELOPE_PX_DTYPE, shape (h, w)) -> uint8 (h, w, 3), row 0 = top (euler_envelope_rgb, host only): white to red with the channel's value
    over `scale` - the arrival time, the wet time, the peak speed or the peak pressure of the pixel -, black where the water never was."""
    px = np.ascontiguousarray(px, ENVELOPE_PX_DTYPE)
    if px.ndim != 2:
        raise ValueError("envelope_rgb: records of shape %r" % (px.shape,))
    h, w = px.shape
    rgb = np.empty((h, w, 3), np.uint8)
    _check_host(load_library().euler_envelope_rgb(px.ctypes.data, w, h, int(channel), float(scale), rgb.ctypes.data, rgb.nbytes), "euler_envelope_rgb")
    return rgb


def tracer_lattice(box, k):
    """The k x k lattice (k = 1, 2 or 4) of every cell of box = (x0, y0, x1, y1), inclusive: float32 positions of shape (n, 2), cell x outer, cell y inner,
    i outer, j inner, at x + (i + 0.5) / k, y + (j + 0.5) / k - what `euler --tracer-box` adds (docs/tracers.md)."""
    x0, y0, x1, y1 = (int(t) for t in box)
    L = load_library()
    n = L.eu_tracer_lattice(x0, y0, x1, y1, int(k), None)
    if n == 0:
        raise ValueError("tracer_lattice: a box with x0 <= x1, y0 <= y1 and k = 1, 2 or 4")
    xy = np.empty((n, 2), np.float32)
    L.eu_tracer_lattice(x0, y0, x1, y1, int(k), xy.ctypes.data)
    return xy


def tracer_paint(counts, px, fg, bg=None):
    """A painted copy of the overview records px: where the tracer raster `counts` of the same box and raster is > 0 a water pixel's dye shows the linear
    colour fg, elsewhere bg (None: it stays) - euler_tracer_paint, so that overview_text / view_text with rainbow and overview_rgb(IMAGE_DYE) draw the tracers."""
    px = _overview_records(px).copy()
    counts = np.ascontiguousarray(counts, np.uint32)
    if counts.shape != px.shape:
        raise ValueError("tracer_paint: counts of shape %r for overview records of shape %r" % (counts.shape, px.shape))
    h, w = px.shape
    f = np.ascontiguousarray(fg, np.float32).reshape(3)
    b = None if bg is None else np.ascontiguousarray(bg, np.float32).reshape(3)
    _check_host(load_library().euler_tracer_paint(counts.ctypes.data, px.ctypes.data, w, h, f.ctypes.data, None if b is None else b.ctypes.data), "euler_tracer_paint")
    return px


SNAPSHOT_F32 = ("u", "v", "utmp", "vtmp")
SNAPSHOT_U8 = ("solid", "source", "sink", "count", "prev_count")
SNAPSHOT_DYE = ("dye_r", "dye_g", "dye_b", "dye_rtmp", "dye_gtmp", "dye_btmp")   # version 2 (euler_config.rainbow)


def _fnv1a64(data, h=14695981039346656037):
    # vectorised FNV-1a is not possible (sequential dependence); snapshots of test size only
    for b in memoryview(data).cast("B"):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def read_snapshot(path, verify=True):
    """Parse a state snapshot written by euler_save_state (layout: include/euler.h) into a dict of
    numpy arrays + scalars.  verify=True recomputes the FNV-1a-64 checksum (pure Python: slow beyond a
    few MB)."""
    import struct
    raw = open(path, "rb").read()
    magic, version, X, Y, _, n, rng, exhausted, _, frames, substeps, iters = struct.unpack_from("<8sIiiIQQiiQQQ", raw, 0)
    if magic != b"EULERSNP" or version not in (1, 2):
        raise ValueError("%s is not an euler state snapshot (version 1 or 2)" % path)
    out = {"X": X, "Y": Y, "n_markers": n, "rng_state": rng, "source_exhausted": exhausted, "frames": frames,
           "total_substeps": substeps, "total_pcg_iterations": iters}
    off, Cn = 72, X * Y
    for name in SNAPSHOT_F32:
        out[name] = np.frombuffer(raw, np.float32, Cn, off).reshape(Y, X).copy(); off += 4 * Cn
    for name in SNAPSHOT_U8:
        out[name] = np.frombuffer(raw, np.uint8, Cn, off).reshape(Y, X).copy(); off += Cn
    out["precon"] = np.frombuffer(raw, np.float64, Cn, off).reshape(Y, X).copy(); off += 8 * Cn
    if version == 2:
        for name in SNAPSHOT_DYE:
            out[name] = np.frombuffer(raw, np.float32, Cn, off).reshape(Y, X).copy(); off += 4 * Cn
    out["markers"] = np.frombuffer(raw, np.float32, 2 * n, off).reshape(n, 2).copy(); off += 8 * n
    (want,) = struct.unpack_from("<Q", raw, off)
    if len(raw) != off + 8:
        raise ValueError("%s: %d trailing bytes" % (path, len(raw) - off - 8))
    if verify and _fnv1a64(raw[:off]) != want:
        raise ValueError("%s: checksum mismatch" % path)
    return out


def write_snapshot(path, st):
    """Inverse of read_snapshot (e.g. to turn a golden fixture into a resumable state)."""
    import struct
    Y, X = st["u"].shape
    mk = np.ascontiguousarray(st["markers"], np.float32).reshape(-1, 2)
    dye = "dye_r" in st
    body = struct.pack("<8sIiiIQQiiQQQ", b"EULERSNP", 2 if dye else 1, X, Y, 0, len(mk), int(st["rng_state"]), int(st.get("source_exhausted", 0)), 0,
                       int(st.get("frames", 0)), int(st.get("total_substeps", 0)), int(st.get("total_pcg_iterations", 0)))
    body += b"".join(np.ascontiguousarray(st[k], np.float32).tobytes() for k in SNAPSHOT_F32)
    body += b"".join(np.ascontiguousarray(st[k], np.uint8).tobytes() for k in SNAPSHOT_U8)
    body += np.ascontiguousarray(st["precon"], np.float64).tobytes()
    if dye:
        body += b"".join(np.ascontiguousarray(st[k], np.float32).tobytes() for k in SNAPSHOT_DYE)
    body += mk.tobytes()
    with open(path, "wb") as f:
        f.write(body + struct.pack("<Q", _fnv1a64(body)))


def _session_core(raw, path):
    """header, arrays and markers of a version-4 file: the dict of read_snapshot and the offset where the chunks begin"""
    import struct
    magic, version, X, Y, flags, n, rng, exhausted, _, frames, substeps, iters = struct.unpack_from("<8sIiiIQQiiQQQ", raw, 0)
    if magic != b"EULERSNP" or version != 4:
        raise ValueError("%s is not an euler session file (version 4)" % path)
    out = {"X": X, "Y": Y, "n_markers": n, "rng_state": rng, "source_exhausted": exhausted, "frames": frames,
           "total_substeps": substeps, "total_pcg_iterations": iters}
    off, Cn = 72, X * Y
    for name in SNAPSHOT_F32:
        out[name] = np.frombuffer(raw, np.float32, Cn, off).reshape(Y, X).copy(); off += 4 * Cn
    for name in SNAPSHOT_U8:
        out[name] = np.frombuffer(raw, np.uint8, Cn, off).reshape(Y, X).copy(); off += Cn
    out["precon"] = np.frombuffer(raw, np.float64, Cn, off).reshape(Y, X).copy(); off += 8 * Cn
    if flags & 1:
        for name in SNAPSHOT_DYE:
            out[name] = np.frombuffer(raw, np.float32, Cn, off).reshape(Y, X).copy(); off += 4 * Cn
    out["markers"] = np.frombuffer(raw, np.float32, 2 * n, off).reshape(n, 2).copy(); off += 8 * n
    return out, off


def read_session(path, verify=True):
    """Parse a session file written by euler_save_session (layout: include/euler.h "session files") into the dict of read_snapshot plus
      time      float
      forcing   {"record": FORCING_DTYPE scalar array [1], "boxes": FORCE_BOX_DTYPE [nboxes]}
      heat      {"on": bool, "record": HEAT_DTYPE [1], "boxes": HEAT_BOX_DTYPE [nboxes], "field": float32 [Y][X] or None}
      tracers   TRACER_DTYPE [n]
      bodies    {"bodies": BODY_DTYPE [n], "origins": int32 [n][2]}
      reseed    {"record": RESEED_DTYPE [1], "stats": RESEED_STATS_DTYPE [1]}
      settings  SESSION_SETTINGS_DTYPE [1]
      stats     {SESSION_STAT_KEYS: value}
    A file with other chunks than these in their order is refused, as the library refuses it."""
    import struct
    raw = open(path, "rb").read()
    out, off = _session_core(raw, path)
    X, Y = out["X"], out["Y"]
    if verify and _fnv1a64(raw[:-8]) != struct.unpack_from("<Q", raw, len(raw) - 8)[0]:
        raise ValueError("%s: checksum mismatch" % path)
    for tag in SESSION_TAGS:
        got, version, nbytes = struct.unpack_from("<4sIQ", raw, off)
        if got != tag or version != 1:
            raise ValueError("%s: chunk %r version %d where %r belongs" % (path, got, version, tag))
        p, off = off + 16, off + 16 + ((nbytes + 7) & ~7)
        arr = lambda dt, n, at: np.frombuffer(raw, dt, n, at).copy()
        if tag == b"TIME":
            out["time"] = struct.unpack_from("<d", raw, p)[0]
        elif tag == b"FORC":
            rec = arr(FORCING_DTYPE, 1, p)
            out["forcing"] = {"record": rec, "boxes": arr(FORCE_BOX_DTYPE, int(rec["nboxes"][0]), p + 48)}
        elif tag == b"HEAT":
            on = struct.unpack_from("<i", raw, p)[0]
            rec = arr(HEAT_DTYPE, 1, p + 8)
            nb = int(rec["nboxes"][0])
            out["heat"] = {"on": bool(on), "record": rec, "boxes": arr(HEAT_BOX_DTYPE, nb, p + 40),
                           "field": arr(np.float32, X * Y, p + 40 + 24 * nb).reshape(Y, X) if on else None}
        elif tag == b"TRAC":
            out["tracers"] = arr(TRACER_DTYPE, struct.unpack_from("<Q", raw, p)[0], p + 8)
        elif tag == b"BODY":
            n = struct.unpack_from("<i", raw, p)[0]
            out["bodies"] = {"bodies": arr(BODY_DTYPE, n, p + 8), "origins": arr(np.int32, 2 * n, p + 8 + 64 * n).reshape(n, 2)}
        elif tag == b"RSED":
            out["reseed"] = {"record": arr(RESEED_DTYPE, 1, p), "stats": arr(RESEED_STATS_DTYPE, 1, p + 32)}
        elif tag == b"SETT":
            out["settings"] = arr(SESSION_SETTINGS_DTYPE, 1, p)
        elif tag == b"STAT":
            out["stats"] = dict(zip(SESSION_STAT_KEYS, struct.unpack_from(SESSION_STAT_FORMAT, raw, p)))
    if len(raw) != off + 8:
        raise ValueError("%s: %d bytes between the END chunk and the checksum" % (path, len(raw) - off - 8))
    return out


def session_bytes(st, chunks=None):
    """The bytes of a session file without its checksum: the core of write_snapshot's layout (version 4), then the chunks.  chunks: None for the chunks of `st`,
    or a list of (tag, chunk_version, payload bytes) to forge another sequence (tests: an unknown tag, a chunk out of order)."""
    import struct
    Y, X = st["u"].shape
    mk = np.ascontiguousarray(st["markers"], np.float32).reshape(-1, 2)
    dye = "dye_r" in st
    body = struct.pack("<8sIiiIQQiiQQQ", b"EULERSNP", 4, int(st.get("X", X)), int(st.get("Y", Y)), 1 if dye else 0, len(mk), int(st["rng_state"]),
                       int(st.get("source_exhausted", 0)), 0, int(st.get("frames", 0)), int(st.get("total_substeps", 0)), int(st.get("total_pcg_iterations", 0)))
    body += b"".join(np.ascontiguousarray(st[k], np.float32).tobytes() for k in SNAPSHOT_F32)
    body += b"".join(np.ascontiguousarray(st[k], np.uint8).tobytes() for k in SNAPSHOT_U8)
    body += np.ascontiguousarray(st["precon"], np.float64).tobytes()
    if dye:
        body += b"".join(np.ascontiguousarray(st[k], np.float32).tobytes() for k in SNAPSHOT_DYE)
    body += mk.tobytes()
    if chunks is None:
        chunks = [(tag, 1, payload) for tag, payload in zip(SESSION_TAGS, session_payloads(st))]
    for tag, version, payload in chunks:
        body += struct.pack("<4sIQ", tag, version, len(payload)) + payload + b"\0" * (-len(payload) % 8)
    return body


def session_payloads(st):
    """the payloads of the chunks of `st` (read_session's entries), in file order"""
    import struct
    tb = lambda a, dt: np.ascontiguousarray(a, dt).tobytes()
    fo, he, bo, rs = st["forcing"], st["heat"], st["bodies"], st["reseed"]
    heat = struct.pack("<ii", 1 if he["on"] else 0, 0) + tb(he["record"], HEAT_DTYPE) + tb(he["boxes"], HEAT_BOX_DTYPE)
    if he["on"]:
        heat += tb(he["field"], np.float32)
    tr = np.ascontiguousarray(st["tracers"], TRACER_DTYPE)
    return [struct.pack("<d", float(st["time"])), tb(fo["record"], FORCING_DTYPE) + tb(fo["boxes"], FORCE_BOX_DTYPE), heat, struct.pack("<Q", len(tr)) + tr.tobytes(),
            struct.pack("<ii", len(bo["bodies"]), 0) + tb(bo["bodies"], BODY_DTYPE) + tb(bo["origins"], np.int32),
            tb(rs["record"], RESEED_DTYPE) + tb(rs["stats"], RESEED_STATS_DTYPE), tb(st["settings"], SESSION_SETTINGS_DTYPE),
            struct.pack(SESSION_STAT_FORMAT, *(st["stats"][k] for k in SESSION_STAT_KEYS)), b""]


def write_session(path, st, chunks=None):
    """Inverse of read_session.  st["X"] / st["Y"], where present, go into the header as they are (tests forge a wrong size with them); chunks as for session_bytes."""
    import struct
    body = session_bytes(st, chunks)
    with open(path, "wb") as f:
        f.write(body + struct.pack("<Q", _fnv1a64(body)))


def profile_class_names():
    L = load_library()
    return [L.euler_profile_class_name(i).decode() for i in range(L.euler_profile_class_count())]


class Simulation:
    """One simulation on one MI355X.  Mirrors the reference's surface: sim_init / sim_step / draw,
    plus state access for parity tests."""

    def __init__(self, X=100, Y=40, device=0, dot_mode=DOT_AUTO, precond=PRECOND_IC0, sweep_mode=SWEEP_AUTO,
                 max_iterations=100, tol=None, pcg_poll_interval=8, viscosity=0.0, rainbow=False, tile_records=0, slab=None,
                 pcg_precision=0, resident=0):
        self.L = load_library()
        cfg = Config()
        _check(self.L.euler_config_default(C.byref(cfg)))
        cfg.X, cfg.Y, cfg.device = X, Y, device
        cfg.dot_mode, cfg.precond, cfg.sweep_mode = dot_mode, precond, sweep_mode
        cfg.max_iterations = max_iterations
        if tol is not None:
            cfg.tol = tol
        cfg.pcg_poll_interval = pcg_poll_interval
        cfg.viscosity = viscosity            # extension: 0 = the inviscid reference
        cfg.rainbow = int(rainbow)           # args_t.rainbow (main.c:54): carry and advect the dye fields
        cfg.precond_tile_records = tile_records  # PRECOND_IC0_TILE: records per tile, 8 / 16 / 32 (0 = default 16)
        if slab is not None:                 # (rank, nranks[, band_lo, band_hi]): row slabs for every stage, this process holds one slab only
            cfg.slab_rank, cfg.slab_nranks = slab[0], slab[1]
            if len(slab) == 4:               # an explicit (fluid-balanced) partition instead of the even split
                cfg.slab_band_lo, cfg.slab_band_hi = slab[2], slab[3]
        self.slab = slab if slab is not None and slab[1] >= 1 else None
        cfg.pcg_precision = pcg_precision    # PCG_F32: solver vectors in float (BASELINE configs[1]'s "fp32"; resident solver only)
        cfg.resident = resident              # RESIDENT_OFF: never the one-launch resident solver (k_resident.hip)
        self.cfg = cfg
        self.X, self.Y = X, Y
        self.h = C.c_void_p()
        _check(self.L.euler_create(C.byref(cfg), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            self.L.euler_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- reference surface
    def sim_init(self, scenario_file, upscale=False):
        _check(self.L.euler_load_scenario_file(self.h, os.fsencode(scenario_file), int(upscale)))
        return self

    def load_text(self, text, upscale=False):
        if isinstance(text, str):
            text = text.encode()
        _check(self.L.euler_load_scenario_mem(self.h, text, len(text), int(upscale)))
        return self

    def load_half_tank(self, tanks=1):
        _check(self.L.euler_load_half_tanks(self.h, tanks))
        return self

    def sim_step(self):
        _check(self.L.euler_step(self.h))

    step = sim_step

    def draw(self, wx, wy):
        n = C.c_int32(0)
        _check(self.L.euler_render(self.h, wx, wy, None, 0, C.byref(n)))
        buf = C.create_string_buffer(max(n.value, 1))
        _check(self.L.euler_render(self.h, wx, wy, buf, n.value, C.byref(n)))
        return buf.raw[: n.value]

    def overview(self, w, h, box=None):
        """The whole interior, or box = (x0, y0, x1, y1) inclusive (euler_overview_box), reduced on the device to h x w boxes of cells
        (euler_overview): an array of OVERVIEW_DTYPE, shape (h, w), row 0 = top."""
        px = np.zeros((max(int(h), 0), max(int(w), 0)), OVERVIEW_DTYPE)
        dst = px.ctypes.data if px.size else np.zeros(1, OVERVIEW_DTYPE).ctypes.data
        if box is None:
            _check(self.L.euler_overview(self.h, w, h, dst, px.nbytes))
        else:
            _check(self.L.euler_overview_box(self.h, *(int(t) for t in box), w, h, dst, px.nbytes))
        return px

    def flow(self, w, h, box=None, pressure=False):
        """The flow raster of the whole interior, or of box = (x0, y0, x1, y1) inclusive, over the pixels of overview(w, h, box) (euler_flow_raster): signed
        sums of the velocity and of the vorticity with their maxima, with pressure=True also of the pressure: an array of FLOW_DTYPE, shape (h, w), row 0 = top."""
        x0, y0, x1, y1 = (1, 1, self.X - 2, self.Y - 2) if box is None else (int(t) for t in box)
        px = np.zeros((max(int(h), 0), max(int(w), 0)), FLOW_DTYPE)
        dst = px.ctypes.data if px.size else np.zeros(1, FLOW_DTYPE).ctypes.data
        _check(self.L.euler_flow_raster(self.h, x0, y0, x1, y1, w, h, FLOW_PRESSURE if pressure else 0, dst, px.nbytes))
        return px

    def marker_raster(self, box, scale):
        """The markers of box = (x0, y0, x1, y1) counted on the device into scale x scale sub-pixels per cell (euler_marker_raster):
        uint32, shape (bh * scale, bw * scale), row 0 = top."""
        x0, y0, x1, y1 = (int(t) for t in box)
        out = np.zeros((max(y1 - y0 + 1, 0) * max(int(scale), 0), max(x1 - x0 + 1, 0) * max(int(scale), 0)), np.uint32)
        _check(self.L.euler_marker_raster(self.h, x0, y0, x1, y1, int(scale), out.ctypes.data if out.size else np.zeros(1, np.uint32).ctypes.data, out.nbytes))
        return out

    def render_view(self, box, wx, wy):
        """The frame of box = (x0, y0, x1, y1) in a window of wx x wy glyphs (euler_render_view): boxes of cells below one cell per glyph,
        the markers' raster above."""
        b = [int(t) for t in box]
        n = C.c_int32(0)
        _check(self.L.euler_render_view(self.h, *b, wx, wy, None, 0, C.byref(n)))
        buf = C.create_string_buffer(max(n.value, 1))
        _check(self.L.euler_render_view(self.h, *b, wx, wy, buf, n.value, C.byref(n)))
        return buf.raw[: n.value]

    def render_fit(self, wx, wy):
        """draw() of the WHOLE interior fitted into wx x wy glyphs (euler_render_fit)."""
        n = C.c_int32(0)
        _check(self.L.euler_render_fit(self.h, wx, wy, None, 0, C.byref(n)))
        buf = C.create_string_buffer(max(n.value, 1))
        _check(self.L.euler_render_fit(self.h, wx, wy, buf, n.value, C.byref(n)))
        return buf.raw[: n.value]

    def diagnostics_record(self, box=None):
        """euler_diagnostics over box = (x0, y0, x1, y1), inclusive (None: the whole interior): one record of DIAG_DTYPE, shape ()."""
        x0, y0, x1, y1 = (1, 1, self.X - 2, self.Y - 2) if box is None else box
        rec = np.zeros((), DIAG_DTYPE)
        _check(self.L.euler_diagnostics(self.h, int(x0), int(y0), int(x1), int(y1), rec.ctypes.data, rec.nbytes))
        return rec

    def diagnostics(self, box=None):
        """Residual divergence, kinetic energy, mass and marker crowding of a box of cells, reduced on the device (docs/diagnostics.md):
        a dict of the record's fields (include/euler.h euler_diag) plus the derived values of euler_diag_derive."""
        rec = self.diagnostics_record(box)
        out = {n: (float(rec[n]) if n in ("max_div", "max_speed2") else int(rec[n])) for n in DIAG_DTYPE.names}
        out.update(diag_derive(rec))
        return out

    def gauges(self, gauges):
        """A list of instruments evaluated on the device in one launch and one read-back (euler_gauges, docs/gauges.md): `gauges` is a list of
        (kind, (x0, y0, x1, y1)) - kind one of GAUGE_LEVEL, GAUGE_PRESSURE, GAUGE_FORCE, GAUGE_FLUX, the box inclusive - or an array of GAUGE_DTYPE.
        Returns the records, an array of GAUGE_REC_DTYPE with one entry per gauge."""
        if isinstance(gauges, np.ndarray) and gauges.dtype == GAUGE_DTYPE:
            g = np.ascontiguousarray(gauges).reshape(-1)
        else:
            g = np.zeros(len(gauges), GAUGE_DTYPE)
            for k, (kind, box) in enumerate(gauges):
                g[k] = (int(kind),) + tuple(int(t) for t in box) + (0,)
        rec = np.zeros(len(g), GAUGE_REC_DTYPE)
        src = g.ctypes.data if g.size else np.zeros(1, GAUGE_DTYPE).ctypes.data
        dst = rec.ctypes.data if rec.size else np.zeros(1, GAUGE_REC_DTYPE).ctypes.data
        _check(self.L.euler_gauges(self.h, src, len(g), dst, rec.nbytes))
        return rec

    def set_forcing(self, gravity=(0.0, -10.0), shake=None, boxes=()):
        """Drive the tank (euler_set_forcing, docs/forcing.md): gravity = (gx, gy); shake = None or (sx, sy, hz[, phase]) - a harmonic acceleration of the
        tank frame; boxes = a list of ((x0, y0, x1, y1), (fx, fy)) or an array of FORCE_BOX_DTYPE - accelerations added to the live faces of the boxes' cells
        in list order."""
        if isinstance(boxes, np.ndarray) and boxes.dtype == FORCE_BOX_DTYPE:
            b = np.ascontiguousarray(boxes).reshape(-1)
        else:
            b = np.zeros(len(boxes), FORCE_BOX_DTYPE)
            for k, (box, force) in enumerate(boxes):
                b[k] = tuple(int(t) for t in box) + (float(force[0]), float(force[1]))
        f = forcing_record(gravity, shake, len(b))
        _check(self.L.euler_set_forcing(self.h, f.ctypes.data, b.ctypes.data if b.size else None))
        return self

    def forcing(self):
        """(record, boxes) as set (euler_get_forcing): FORCING_DTYPE of shape () and an array of FORCE_BOX_DTYPE."""
        f = np.zeros((), FORCING_DTYPE)
        b = np.zeros(FORCE_BOXES_MAX, FORCE_BOX_DTYPE)
        _check(self.L.euler_get_forcing(self.h, f.ctypes.data, b.ctypes.data, FORCE_BOXES_MAX))
        return f, b[: int(f["nboxes"])].copy()

    @property
    def time(self):
        """The handle's clock of simulated time (euler_get_time): 0 after a load, += dt behind every substep."""
        t = C.c_double(0)
        _check(self.L.euler_get_time(self.h, C.byref(t)))
        return t.value

    @time.setter
    def time(self, t):
        _check(self.L.euler_set_time(self.h, float(t)))

    # --- moving bodies (docs/bodies.md)
    def set_bodies(self, bodies):
        """Replace the handle's moving bodies (euler_set_bodies, docs/bodies.md): a list of records of body() (or of its argument tuples), or an array of
        BODY_DTYPE, at most BODIES_MAX.  The old rectangles are cleared, the new ones made solid at the handle's present clock."""
        b = bodies_array(bodies)
        _check(self.L.euler_set_bodies(self.h, b.ctypes.data if b.size else None, len(b)))
        return self

    def clear_bodies(self):
        _check(self.L.euler_set_bodies(self.h, None, 0))
        return self

    def bodies(self):
        """(bodies, now) as set (euler_get_bodies): an array of BODY_DTYPE and one of BODY_STATE_DTYPE - the position at the handle's clock, with the origin of
        the cells that are solid now."""
        b = np.zeros(BODIES_MAX, BODY_DTYPE)
        st = np.zeros(BODIES_MAX, BODY_STATE_DTYPE)
        n = C.c_int32(0)
        _check(self.L.euler_get_bodies(self.h, b.ctypes.data, BODIES_MAX, st.ctypes.data, C.byref(n)))
        return b[: n.value].copy(), st[: n.value].copy()

    # --- marker density control (docs/reseed.md)
    def set_reseed(self, record=None, **kw):
        """Switch the marker density control on or off (euler_set_reseed, docs/reseed.md): a record of reseed(), or its keyword arguments; an all-zero record
        switches it off.  The totals count from this call."""
        r = np.ascontiguousarray(reseed(**kw) if record is None else record, RESEED_DTYPE).reshape(1)
        _check(self.L.euler_set_reseed(self.h, r.ctypes.data))
        return self

    def clear_reseed(self):
        _check(self.L.euler_set_reseed(self.h, None))
        return self

    def reseed(self):
        """(record, totals) as set (euler_get_reseed): RESEED_DTYPE and RESEED_STATS_DTYPE of shape () - markers removed and added, cells thinned and cells
        deferred since the last set_reseed."""
        r, st = np.zeros((), RESEED_DTYPE), np.zeros((), RESEED_STATS_DTYPE)
        _check(self.L.euler_get_reseed(self.h, r.ctypes.data, st.ctypes.data))
        return r, st

    # --- temperature (docs/heat.md)
    def set_heat(self, ambient=0.0, beta=0.0, kappa=0.0, source_t=0.0, boxes=()):
        """Switch the temperature on, or replace beta, kappa, source_t and the boxes of a handle that has it (euler_set_heat, docs/heat.md): an advected scalar
        that starts at `ambient`, expands with beta (0: passive), diffuses with kappa; boxes = a list of (kind, value, (x0, y0, x1, y1)) - kind HEAT_FIX or
        HEAT_RATE - or an array of HEAT_BOX_DTYPE, applied to the fluid cells in list order."""
        if isinstance(boxes, np.ndarray) and boxes.dtype == HEAT_BOX_DTYPE:
            b = np.ascontiguousarray(boxes).reshape(-1)
        else:
            b = np.zeros(len(boxes), HEAT_BOX_DTYPE)
            for k, (kind, value, box) in enumerate(boxes):
                b[k] = tuple(int(t) for t in box) + (float(value), int(kind))
        h = heat_default()
        h["ambient"], h["beta"], h["kappa"], h["source_t"], h["nboxes"] = ambient, beta, kappa, source_t, len(b)
        _check(self.L.euler_set_heat(self.h, h.ctypes.data, b.ctypes.data if b.size else None))
        return self

    def heat_off(self):
        """Switch the temperature off (euler_set_heat with a null record): the handle launches what it launched before."""
        _check(self.L.euler_set_heat(self.h, None, None))
        return self

    def heat(self):
        """(record, boxes) as set (euler_get_heat): HEAT_DTYPE of shape () and an array of HEAT_BOX_DTYPE."""
        h = np.zeros((), HEAT_DTYPE)
        b = np.zeros(HEAT_BOXES_MAX, HEAT_BOX_DTYPE)
        _check(self.L.euler_get_heat(self.h, h.ctypes.data, b.ctypes.data, HEAT_BOXES_MAX))
        return h, b[: int(h["nboxes"])].copy()

    @property
    def temperature(self):
        """The temperature field, float32 of shape (Y, X) (euler_heat_get_field): cells without markers hold ambient.  A row-slab handle returns and accepts
        its own rows, shape (rows, X); setting it is collective there (the neighbours' ghost rows follow)."""
        lo, hi = self.slab_rows()
        t = np.zeros((hi - lo, self.X), np.float32)
        _check(self.L.euler_heat_get_field(self.h, t.ctypes.data, t.nbytes))
        return t

    @temperature.setter
    def temperature(self, t):
        a = np.ascontiguousarray(t, np.float32)
        _check(self.L.euler_heat_set_field(self.h, a.ctypes.data, a.nbytes))

    def heat_fill(self, box, value):
        """T = value in the cells of box = (x0, y0, x1, y1), inclusive, that hold markers, now (euler_heat_fill)."""
        x0, y0, x1, y1 = (int(t) for t in box)
        _check(self.L.euler_heat_fill(self.h, x0, y0, x1, y1, float(value)))
        return self

    def heat_raster(self, w, h, box=None):
        """The temperature of the whole interior, or of box = (x0, y0, x1, y1) inclusive, over the pixels of overview(w, h, box) (euler_heat_raster): signed
        sums of T - ambient over the water cells with their maxima: an array of HEAT_PX_DTYPE, shape (h, w), row 0 = top."""
        x0, y0, x1, y1 = (1, 1, self.X - 2, self.Y - 2) if box is None else (int(t) for t in box)
        px = np.zeros((max(int(h), 0), max(int(w), 0)), HEAT_PX_DTYPE)
        dst = px.ctypes.data if px.size else np.zeros(1, HEAT_PX_DTYPE).ctypes.data
        _check(self.L.euler_heat_raster(self.h, x0, y0, x1, y1, w, h, dst, px.nbytes))
        return px

    # --- run-long envelopes (docs/envelope.md)
    def set_envelope(self, channels):
        """Switch envelope channels on or off (euler_set_envelope): a set of ENV_* bits; a newly enabled channel starts from its initial words, one that stays
        keeps its plane, 0 frees them all.  From then on every substep ends with the planes' update."""
        _check(self.L.euler_set_envelope(self.h, int(channels)))
        return self

    def envelope(self):
        """(channels, substeps) (euler_get_envelope): the ENV_* bits that are on and the substeps accumulated since they were switched on or last reset."""
        ch, n = C.c_uint32(0), C.c_uint64(0)
        _check(self.L.euler_get_envelope(self.h, C.byref(ch), C.byref(n)))
        return int(ch.value), int(n.value)

    def envelope_reset(self):
        _check(self.L.euler_envelope_reset(self.h))
        return self

    def envelope_field(self, channel):
        """One plane (euler_envelope_get_field): float32 of shape (Y, X); view it as uint32 for the arrival's "never" word 0xffffffff."""
        out = np.empty((self.Y, self.X), np.float32)
        _check(self.L.euler_envelope_get_field(self.h, int(channel), out.ctypes.data, out.nbytes))
        return out

    def set_envelope_field(self, channel, array):
        """Restore a plane the caller kept (euler_envelope_set_field): float32 (or its uint32 view) of shape (Y, X)."""
        a = np.asarray(array)
        a = np.ascontiguousarray(a.view(np.float32) if a.dtype == np.uint32 else a, np.float32)
        _check(self.L.euler_envelope_set_field(self.h, int(channel), a.ctypes.data, a.nbytes))
        return self

    def envelope_raster(self, box, w, h):
        """The planes per pixel of overview(w, h, box) (euler_envelope_raster): an array of ENVELOPE_PX_DTYPE, shape (h, w), row 0 = top.  box = None: the
        whole interior."""
        x0, y0, x1, y1 = (1, 1, self.X - 2, self.Y - 2) if box is None else (int(t) for t in box)
        px = np.zeros((max(int(h), 0), max(int(w), 0)), ENVELOPE_PX_DTYPE)
        dst = px.ctypes.data if px.size else np.zeros(1, ENVELOPE_PX_DTYPE).ctypes.data
        _check(self.L.euler_envelope_raster(self.h, x0, y0, x1, y1, int(w), int(h), dst, px.nbytes))
        return px

    # --- passive tracers (docs/tracers.md)
    def add_tracers(self, xy):
        """Append tracers at the positions xy, shape (n, 2) in the markers' units (euler_tracers_add): they move with the flow by the marker's rule in
        front of every marker advection and accumulate path, age and wet time."""
        a = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        _check(self.L.euler_tracers_add(self.h, a.ctypes.data if len(a) else None, len(a)))
        return self

    @property
    def n_tracers(self):
        n = C.c_size_t(0)
        _check(self.L.euler_tracers_count(self.h, C.byref(n)))
        return int(n.value)

    def tracers(self, first=0, n=None):
        """Records [first, first + n) (n = None: to the end) in the order they were added (euler_tracers_get): an array of TRACER_DTYPE."""
        if n is None:
            n = max(self.n_tracers - int(first), 0)
        out = np.zeros(int(n), TRACER_DTYPE)
        _check(self.L.euler_tracers_get(self.h, int(first), int(n), out.ctypes.data if out.size else None, out.nbytes))
        return out

    def clear_tracers(self):
        _check(self.L.euler_tracers_clear(self.h))
        return self

    def tracer_raster(self, box, w, h, all=False):
        """The live tracers (all=True: the retired ones too) per pixel of overview(w, h, box) (euler_tracer_raster): uint32, shape (h, w), row 0 = top.
        box = None: the whole interior."""
        x0, y0, x1, y1 = (1, 1, self.X - 2, self.Y - 2) if box is None else (int(t) for t in box)
        out = np.zeros((max(int(h), 0), max(int(w), 0)), np.uint32)
        dst = out.ctypes.data if out.size else np.zeros(1, np.uint32).ctypes.data
        _check(self.L.euler_tracer_raster(self.h, x0, y0, x1, y1, int(w), int(h), TRACER_RASTER_ALL if all else 0, dst, out.nbytes))
        return out

    def edit_box(self, op, box):
        """Edit box = (x0, y0, x1, y1), inclusive, and the markers in it on the device (euler_edit_box, docs/editing.md): op is one of EDIT_SOLID,
        EDIT_CLEAR, EDIT_SINK, EDIT_SOURCE, EDIT_FILL, EDIT_DRAIN."""
        _check(self.L.euler_edit_box(self.h, int(op), *(int(t) for t in box)))
        return self

    def colorize(self):
        """The reference's 'r' key (main.c:970-973): colour the current fluid afresh."""
        _check(self.L.euler_colorize(self.h))

    # --- finer control
    def timestep(self, frame_time_left=0.1):
        dt = C.c_float(0)
        _check(self.L.euler_timestep(self.h, frame_time_left, C.byref(dt)))
        return dt.value

    def substep(self, dt):
        _check(self.L.euler_substep(self.h, dt))

    def stage(self, stage, dt=0.0):
        _check(self.L.euler_stage(self.h, stage, dt))

    def set_precond(self, precond, tile_records=0):
        _check(self.L.euler_set_precond(self.h, precond, tile_records))

    def set_solver(self, max_iterations=0, tol=-1.0):
        """iteration budget / tolerance of the following solves (<= 0 / < 0: unchanged)"""
        _check(self.L.euler_set_solver(self.h, max_iterations, tol))

    def pcg_op(self, op, dt=0.0, scalar=0.0):
        out = C.c_double(0)
        _check(self.L.euler_pcg_op(self.h, op, dt, scalar, C.byref(out)))
        return out.value

    # --- state
    def get(self, field):
        nbytes = self.L.euler_field_bytes(self.h, field)
        dt = np.dtype(_FIELD_DTYPE[field])
        a = np.empty(nbytes // dt.itemsize, dt)
        if nbytes:
            _check(self.L.euler_get_field(self.h, field, a.ctypes.data, nbytes))
        elif field not in (F_MARKERS, F_MARKER_KEYS):      # an unknown or unavailable field: let the library say why
            _check(self.L.euler_get_field(self.h, field, np.empty(8, np.uint8).ctypes.data, 0) or -1)
        if field == F_MARKERS:
            return a.reshape(-1, 2)
        if field == F_MARKER_KEYS:
            return a
        return a.reshape(-1, self.X)        # a row-slab handle returns its own rows (euler_slab_info)

    def set(self, field, arr):
        a = np.ascontiguousarray(arr, _FIELD_DTYPE[field])
        _check(self.L.euler_set_field(self.h, field, a.ctypes.data, a.nbytes))

    def slab_rows(self):
        """[row_lo, row_hi) this handle owns (the whole grid without slabs)."""
        lo, hi, nb = C.c_int32(), C.c_int32(), C.c_int32()
        _check(self.L.euler_slab_info(self.h, C.byref(lo), C.byref(hi), C.byref(nb)))
        return (64 * lo.value, min(64 * hi.value, self.Y)) if self.slab else (0, self.Y)

    def set_markers(self, m):
        a = np.ascontiguousarray(m, np.float32).reshape(-1, 2)
        _check(self.L.euler_set_markers(self.h, a.ctypes.data, len(a)))

    def set_rng(self, state, exhausted=0):
        _check(self.L.euler_set_rng(self.h, int(state), int(exhausted)))

    def set_option(self, key, value):
        """include/euler.h EULER_OPT_*: a per-handle option (what used to be an EULER_* environment variable)"""
        _check(self.L.euler_set_option(self.h, int(key), C.c_int64(int(value))))
        return self

    def get_option(self, key):
        v = C.c_int64(0)
        _check(self.L.euler_get_option(self.h, int(key), C.byref(v)))
        return int(v.value)

    def resident_info(self):
        """(eligible, solves run by the resident solver, solves that fell back to the multi-kernel path)"""
        out = (C.c_uint64 * 3)()
        _check(self.L.euler_resident_info(self.h, out))
        return bool(out[0]), int(out[1]), int(out[2])

    def stats(self):
        s = Stats()
        _check(self.L.euler_get_stats(self.h, C.byref(s)))
        return s

    # --- measurement
    def profile_enable(self, classes):
        names = profile_class_names()
        mask = 0
        for c in classes:
            mask |= 1 << (names.index(c) if isinstance(c, str) else c)
        _check(self.L.euler_profile_enable(self.h, mask))

    def profile_reset(self):
        _check(self.L.euler_profile_reset(self.h))

    def profile(self):
        out = {}
        for i, n in enumerate(profile_class_names()):
            ms, k = C.c_double(0), C.c_uint64(0)
            _check(self.L.euler_profile_get(self.h, i, C.byref(ms), C.byref(k)))
            if k.value:
                out[n] = (ms.value, k.value)
        return out

    def copy_bandwidth(self, nbytes=1 << 30, reps=10):
        g = C.c_double(0)
        _check(self.L.euler_measure_copy_bandwidth(self.h, nbytes, reps, C.byref(g)))
        return g.value

    def exchange_latency(self, reps=200, row_doubles=0, nsmall=2):
        """collective: microseconds per exchange point of a distributed PCG iteration over the installed communicator"""
        g = C.c_double(0)
        _check(self.L.euler_measure_exchange(self.h, reps, row_doubles, nsmall, C.byref(g)))
        return g.value

    def save_state(self, path):
        """Checkpoint (include/euler.h "state snapshots"): everything sim_step() depends on."""
        _check(self.L.euler_save_state(self.h, os.fsencode(path)))

    def load_state(self, path):
        _check(self.L.euler_load_state(self.h, os.fsencode(path)))
        return self

    def save_session(self, path):
        """A session file (include/euler.h "session files", docs/session.md): the snapshot plus clock, forcing, heat, tracers, bodies, reseed record and totals."""
        _check(self.L.euler_save_session(self.h, os.fsencode(path)))

    def load_session(self, path, ignore_settings=False):
        """Puts the handle into the saving handle's state; a refused load leaves it as it was.  ignore_settings: do not compare the file's SETT chunk with this handle's settings."""
        _check(self.L.euler_load_session(self.h, os.fsencode(path), SESSION_IGNORE_SETTINGS if ignore_settings else 0))
        return self

    def sweep_timeline(self, raw=False):
        """[(entry_us, first_ready_us, exit_us, blocks, stalled_blocks)] per band of the last sweep launch,
        times relative to the first band's entry.  raw=True: additionally the 4 development words as integers
        (stall counts per helper, or 100 MHz time stamps in an SW_TRACE_HANDOFF build) and the origin tick."""
        nb = (self.Y + 63) // 64
        buf = (C.c_uint64 * (8 * nb))()
        n = self.L.euler_sweep_timeline(self.h, buf, nb)
        if n < 0:
            _check(n)
        rows = [tuple(buf[8 * i + k] for k in range(8)) for i in range(n)]
        t0 = min(r[0] for r in rows) if rows else 0
        out = []
        for r in rows:
            row = ((r[0] - t0) / 100.0, (r[1] - t0) / 100.0, (r[2] - t0) / 100.0, r[3] >> 32, r[3] & 0xffffffff)
            if raw:
                row += tuple(int(x) for x in r[4:8]) + (int(t0),)
            out.append(row)
        return out

    def hbm_bytes(self):
        """device memory this handle allocated (a row-slab handle: its slab only)"""
        return int(self.L.euler_hbm_bytes(self.h))

    def device_name(self):
        buf = C.create_string_buffer(256)
        _check(self.L.euler_device_name(self.h, buf, 256))
        return buf.value.decode()
