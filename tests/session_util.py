"""Shared by the session-file tests (docs/session.md): a small state forged in numpy, the library's parser called on a file's bytes, and the scene with every extra on."""
import ctypes as C

import numpy as np

import euler_amd as ea

F32 = np.float32
EINVAL, EIO, ESTATE = -1, -3, -5


def settings_record(max_iterations=100, dot_mode=ea.DOT_SEQUENTIAL, precond=ea.PRECOND_IC0, tile_records=16, rainbow=0, viscosity=0.0, resident=0, opts=None):
    """the SETT record of a handle created with these arguments and otherwise the defaults of euler_config_default and euler_create"""
    s = np.zeros(1, ea.SESSION_SETTINGS_DTYPE)
    s["max_iterations"], s["dot_mode"], s["precond"], s["tile_records"], s["rainbow"], s["resident"] = max_iterations, dot_mode, precond, tile_records, rainbow, resident
    s["max_substeps"], s["pcg_poll_interval"], s["tol"], s["nopts"] = 8, 8, float(F32(1e-6)), 24
    s["viscosity_bits"], s["frame_time_bits"] = F32(viscosity).view(np.uint32), F32(0.1).view(np.uint32)
    for k, v in (opts or {}).items():
        s["opt"][0][k] = v
    return s


def forged_state(X=12, Y=9, seed=5):
    """a session's worth of state that every host check accepts: a solid ring, a 2 x 2 body standing at (4, 3), water, heat on, three tracers, reseed on"""
    rng = np.random.default_rng(seed)
    st = {"X": X, "Y": Y, "rng_state": 0x9bd185c449534b91, "source_exhausted": 0, "frames": 6, "total_substeps": 31, "total_pcg_iterations": 977}
    for k in ea.SNAPSHOT_F32:
        st[k] = rng.standard_normal((Y, X)).astype(F32)
    solid = np.zeros((Y, X), np.uint8)
    solid[0], solid[-1], solid[:, 0], solid[:, -1] = 1, 1, 1, 1
    solid[3:5, 4:6] = 1
    count = ((rng.random((Y, X)) < 0.6) & (solid == 0)).astype(np.uint8) * 4
    st.update(solid=solid, source=np.zeros((Y, X), np.uint8), sink=np.zeros((Y, X), np.uint8), count=count, prev_count=count.copy(), precon=rng.random((Y, X)))
    ys, xs = np.nonzero(count)
    st["markers"] = np.stack([xs + 0.25, ys + 0.75], 1).astype(F32).repeat(4, 0)
    st["time"] = 0.6000000052154064
    fo = ea.forcing_default()
    fo["gx"], fo["shake_x"], fo["shake_hz"], fo["nboxes"] = 1.5, 2.0, 0.5, 2
    boxes = np.zeros(2, ea.FORCE_BOX_DTYPE)
    boxes[0], boxes[1] = (1, 1, 3, 2, 4.0, 0.0), (7, 2, X - 2, Y - 2, 0.0, -3.0)
    st["forcing"] = {"record": fo.reshape(1), "boxes": boxes}
    he = ea.heat_default()
    he["beta"], he["kappa"], he["source_t"], he["nboxes"] = 0.5, 0.3, 8.0, 1
    hb = np.zeros(1, ea.HEAT_BOX_DTYPE)
    hb[0] = (1, 1, 2, 2, 16.0, ea.HEAT_FIX)
    st["heat"] = {"on": True, "record": he.reshape(1), "boxes": hb, "field": np.where(count > 0, rng.random((Y, X)) * 8, 0).astype(F32)}
    tr = np.zeros(3, ea.TRACER_DTYPE)
    tr[0] = (2.5, 2.5, 1.0, 0.6, 0.6, 31, ea.TRACER_WET, 0)
    tr[1] = (4.5, 3.5, 0.0, 0.0, 0.0, 0, ea.TRACER_RETIRED | ea.TRACER_IN_SOLID, 0)
    tr[2] = (np.nan, 1.5, 0.0, 0.0, 0.0, 0, ea.TRACER_RETIRED | ea.TRACER_LOST, 0)
    st["tracers"] = tr
    st["bodies"] = {"bodies": ea.bodies_array([ea.body((2, 2), (3.0, 3.0), velocity=(1.0, 0.0), amplitude=(1.0, 0.0), hz=0.25)]), "origins": np.array([[4, 3]], np.int32)}
    rs = np.zeros(1, ea.RESEED_STATS_DTYPE)
    rs[0] = (5, 2, 1, 0)
    st["reseed"] = {"record": ea.reseed(thin_above=16, fill_holes=True).reshape(1), "stats": rs}
    st["settings"] = settings_record(opts={ea.OPT_P_STEPS: 8, ea.OPT_TILE_REVERSE: 1, ea.OPT_GRID4_MIN_CELLS: 1 << 22, ea.OPT_SA_RUN: 8, ea.OPT_PROFILE_STRIDE: 1})
    st["stats"] = dict(last_substeps=5, last_pcg_iterations=160, last_residual=3e-7, last_dt=float(F32(0.02)), pad=0, marker_dt_events=4, marker_multi_events=0)
    return st


def parse_with_library(raw, X, Y, dye=0, max_markers=None):
    """eu_session_parse (csrc/euler_host.c) on the bytes of a file: (return code, message)"""
    L = ea.load_library()
    L.eu_session_parse.restype = C.c_int
    L.eu_session_parse.argtypes = [C.c_char_p, C.c_size_t, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p, C.c_char_p, C.c_size_t]
    out = C.create_string_buffer(1 << 16)      # (eu_session is some 6 KB: the layout program of the host test prints its size)
    why = C.create_string_buffer(400)
    rc = L.eu_session_parse(bytes(raw), len(raw), X, Y, dye, 4 * X * Y if max_markers is None else max_markers, out, why, len(why))
    return rc, why.value.decode(errors="replace")


def same_entries(a, b):
    """two dicts of read_session: every entry equal as bytes (NaN positions included)"""
    def eq(x, y):
        if isinstance(x, dict):
            return set(x) == set(y) and all(eq(x[k], y[k]) for k in x)
        if x is None or y is None:
            return x is None and y is None
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
            return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        return x == y
    return set(a) == set(b) and all(eq(a[k], b[k]) for k in a)
