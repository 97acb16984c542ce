"""The test-side restatement of the midpoint (RK2) transport (tests/c/advect_rk2.c, tests/advect_rk2_ref.py), pinned on the CPU
before any GPU test relies on it:
  - with the midpoint bypassed it is the oracle's forward-Euler stages bit for bit, and the composed frame is eo_step;
  - on a rigid rotation the midpoint rule is second order (the back-trace error falls 8x per halved dt, forward Euler 4x) and
    the markers keep their radius (forward Euler spirals them outward).
"""
import ctypes as C

import numpy as np
import pytest

import advect_rk2_ref as ref
from golden_util import SCENARIOS, X, Y, bits_equal, load, scenario_text
from oracle_lib import Oracle, U, V


@pytest.fixture(scope="module")
def ar(tmp_path_factory):
    return ref.build(tmp_path_factory.mktemp("advect_rk2"))


def _state(o):
    return [o.u.copy(), o.v.copy(), o.count.copy(), o.prev_count.copy(), o.markers.copy(), int(o.c.rng_state),
            o.cr.copy(), o.cg.copy(), o.cb.copy()]


def _assert_state(a, b, what):
    names = ("u", "v", "count", "prev_count", "markers", "rng", "dye_r", "dye_g", "dye_b")
    for x, y, n in zip(a, b, names):
        if isinstance(x, int):
            assert x == y, "%s: %s" % (what, n)
        else:
            assert bits_equal(x, y), "%s: %s" % (what, n)


@pytest.mark.parametrize("scn", SCENARIOS)
def test_restated_stages_without_the_midpoint_are_the_oracles(ar, scn):
    """advect_u / _v / _p and advect_markers with rk2 = 0, against eo_advect_*, on states along the scenario's own run (dt chains included: filter)"""
    o = Oracle(X, Y, rainbow=True).load_text(scenario_text(load(scn + "_frames.npz")))
    events = 0
    for f in range(12):
        o.step()
        if f % 3 != 2:
            continue
        dt = o.timestep(0.1)
        for fn, ours, t in ((o.lib.eo_advect_u, ar.ar_advect_u, U), (o.lib.eo_advect_v, ar.ar_advect_v, V)):
            want = np.full((Y, X), 7.0, np.float32)
            got = want.copy()
            fn(o.ptr, o.f32p(o.u), o.f32p(o.v), C.c_float(dt), o.f32p(want))
            ours(C.cast(o.ptr, C.c_void_p), o.f32p(o.u), o.f32p(o.v), C.c_float(dt), o.f32p(got), 0)
            assert bits_equal(got, want), (scn, f, t)
        for q in (o.cr, o.cg, o.cb):
            want = np.full((Y, X), 7.0, np.float32)
            got = want.copy()
            o.lib.eo_advect_p(o.ptr, o.f32p(q), o.f32p(o.u), o.f32p(o.v), C.c_float(dt), o.f32p(want))
            ar.ar_advect_p(C.cast(o.ptr, C.c_void_p), o.f32p(q), o.f32p(o.u), o.f32p(o.v), C.c_float(dt), o.f32p(got), 0)
            assert bits_equal(got, want), (scn, f, "dye")
        m0 = o.markers.copy()
        o.lib.eo_advect_markers(o.ptr, C.c_float(dt))
        want = o.markers.copy()
        o.set_markers(m0)
        events += ref.advect_markers(ar, o, dt, 0)
        assert bits_equal(o.markers, want), (scn, f, "markers")
        o.set_markers(m0)
    # the golden substep state (the teacher-forced GPU tests start from it): the filter's holds a collision that shortens dt for later markers (main.c:501)
    g = load(scn + "_substep.npz")
    o = substep_oracle(g)
    dt = float(g["dt"])
    o.lib.eo_advect_markers(o.ptr, C.c_float(dt))
    want = o.markers.copy()
    o = substep_oracle(g)
    events = ref.advect_markers(ar, o, dt, 0)
    assert bits_equal(o.markers, want) and bits_equal(want, g["s00_markers"]), (scn, "substep markers")
    if scn == "filter":
        assert events >= 1, "the filter substep should shorten dt along the marker array"


def substep_oracle(g, rainbow=False):
    """an oracle holding a golden *_substep.npz state (the reference's arrays in front of a substep)"""
    o = Oracle(X, Y, rainbow=rainbow)
    for n in ("solid", "source", "sink"):
        getattr(o, n)[...] = g[n]
    for n in ("u", "v", "utmp", "vtmp", "count", "prev_count"):
        getattr(o, n)[...] = g["before_" + n]
    o.set_markers(g["before_markers"])
    o.c.rng_state = int(g["rng_before"])
    o.c.source_exhausted = int(g["exhausted_before"])
    return o


@pytest.mark.parametrize("scn", SCENARIOS)
def test_composed_frame_without_the_midpoint_is_eo_step(ar, scn):
    text = scenario_text(load(scn + "_frames.npz"))
    rainbow = scn == "waterfall"
    a = Oracle(X, Y, rainbow=rainbow).load_text(text)
    b = Oracle(X, Y, rainbow=rainbow).load_text(text)
    for f in range(30):
        a.step()
        n, it = ref.step(ar, b, 0)
        assert (n, it) == (a.c.last_substeps, a.c.last_pcg_iterations), (scn, f)
        assert a.c.frame_count == b.c.frame_count and a.c.total_substeps == b.c.total_substeps
        _assert_state(_state(a), _state(b), "%s frame %d" % (scn, f))


def test_the_midpoint_changes_the_frame(ar):
    """RK2 is not RK1 on a moving scene (the composed frames part within a few frames)"""
    text = scenario_text(load("block_frames.npz"))
    a = Oracle(X, Y).load_text(text)
    b = Oracle(X, Y).load_text(text)
    for f in range(20):
        ref.step(ar, a, 0)
        ref.step(ar, b, 1)
    assert not bits_equal(a.u, b.u) and not bits_equal(a.markers, b.markers)
    assert np.isfinite(b.u).all() and np.isfinite(b.v).all()


def _rotation_oracle():
    u, v, count, sink = ref.rotation_fields()
    o = Oracle(ref.ROT_N, ref.ROT_N)
    o.u[...] = u; o.v[...] = v; o.count[...] = count; o.prev_count[...] = count; o.sink[...] = sink
    o.solid[...] = 0; o.source[...] = 0
    return o


def rotation_backtrace_errors(ar):
    """{rk2: (error at the CFL dt, error at dt / 2)} of the advected u on the rotation's test faces, and the CFL dt"""
    o = _rotation_oracle()
    dt = o.timestep(0.1)
    out = {}
    for rk2 in (0, 1):
        errs = []
        for h in (dt, dt / 2):
            o.utmp[...] = 0
            ar.ar_advect_u(C.cast(o.ptr, C.c_void_p), o.f32p(o.u), o.f32p(o.v), C.c_float(h), o.f32p(o.utmp), rk2)
            errs.append(ref.rotation_u_error(o.utmp, np.float32(h)))
        out[rk2] = errs
    return out, dt


def rotation_marker_drift(ar, steps=20):
    o = _rotation_oracle()
    dt = o.timestep(0.1)
    out = {}
    for rk2 in (0, 1):
        o.set_markers(ref.rotation_markers())
        for _ in range(steps):
            ref.advect_markers(ar, o, dt, rk2)
        out[rk2] = ref.radius_drift(o.markers)
    return out, dt


def test_rotation_backtrace_is_second_order_with_the_midpoint(ar):
    e, dt = rotation_backtrace_errors(ar)
    assert 0.07 < dt * ref.ROT_OMEGA < 0.1      # the turn per CFL step
    r1, r2 = e[0][0] / e[0][1], e[1][0] / e[1][1]
    assert 3.0 <= r1 <= 5.0, e
    assert r2 >= 6.0, e
    # the float32 floor: rounding of positions near the centre (~28 cells: ulp 1.9e-6) moves u by about omega * ulp - far below the RK2 error at dt / 2
    floor = ref.ROT_OMEGA * float(np.spacing(np.float32(2 * ref.ROT_C)))
    assert e[1][1] > 10 * floor, (e, floor)
    assert e[1][0] < e[0][0] / 20


def test_rotation_markers_keep_their_radius_with_the_midpoint(ar):
    d, dt = rotation_marker_drift(ar)
    assert d[0] > 0.1, d                     # forward Euler: r (1 + theta^2)^(n/2) - the spiral outward
    assert d[1] <= d[0] / 20, d
    floor = 20 * float(np.spacing(np.float32(ref.ROT_C + 3.0)))      # 20 steps of position rounding at the markers' coordinates (~27 cells)
    assert d[1] > 5 * floor, (d, floor)
