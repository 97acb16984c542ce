"""EULER_OPT_ADVECT_RK2 on the GPU: the midpoint (RK2) transport of u, v, the dye and the markers (docs/advection_rk2.md) against
the test-side restatement (tests/c/advect_rk2.c, tests/advect_rk2_ref.py; pinned on the CPU by test_advect_rk2_host.py), bit for bit
with EULER_DOT_SEQUENTIAL: stage by stage from the golden substep states, free-running, in every marker form, on a 1024^2 grid, through
a snapshot and through the `euler` front end; and the rotation checks of the host test on the device's own arithmetic."""
import os
import subprocess

import numpy as np
import pytest

import advect_rk2_ref as ref
import euler_amd as ea
from euler_amd import scenarios
from golden_util import SCENARIOS, X, Y, load, scenario_text
from oracle_lib import Oracle, U, V
from test_gpu_parity import _random_marker_state, assert_bits, load_substep_state

pytestmark = pytest.mark.gpu

DYE = (ea.F_DYE_R, ea.F_DYE_G, ea.F_DYE_B)
EULER_EINVAL, EULER_ESTATE = -1, -5      # include/euler.h


@pytest.fixture(scope="module")
def ar(tmp_path_factory):
    return ref.build(tmp_path_factory.mktemp("advect_rk2"))


def rk2_sim(*args, **kw):
    s = ea.Simulation(*args, **kw)
    s.set_option(ea.OPT_ADVECT_RK2, 1)
    return s


def compare_state(o, sim, what, dye=False):
    for fld, want, n in ((ea.F_U, o.u, "u"), (ea.F_V, o.v, "v"), (ea.F_COUNT, o.count, "count"), (ea.F_PREV_COUNT, o.prev_count, "prev_count"),
                         (ea.F_MARKERS, o.markers, "markers")):
        assert_bits(sim.get(fld), want, "%s %s" % (what, n))
    st = sim.stats()
    assert int(st.rng_state) == int(o.c.rng_state), what
    if dye:
        for fld, want in zip(DYE, (o.cr, o.cg, o.cb)):
            assert_bits(sim.get(fld), want, "%s dye %d" % (what, fld))


# ----------------------------------------------------------------------------- the option
def test_option_surface():
    sim = ea.Simulation(X, Y)
    assert sim.get_option(ea.OPT_ADVECT_RK2) == 0
    for val in (1, 0, 1):
        sim.set_option(ea.OPT_ADVECT_RK2, val)
        assert sim.get_option(ea.OPT_ADVECT_RK2) == val
    for bad in (2, -1):
        with pytest.raises(ea.EulerError) as e:
            sim.set_option(ea.OPT_ADVECT_RK2, bad)
        assert e.value.code == EULER_EINVAL
        assert sim.get_option(ea.OPT_ADVECT_RK2) == 1
    slab = ea.Simulation(X, Y, slab=(0, 1))
    with pytest.raises(ea.EulerError) as e:
        slab.set_option(ea.OPT_ADVECT_RK2, 1)
    assert e.value.code == EULER_ESTATE and "slab" in str(e.value)
    assert slab.get_option(ea.OPT_ADVECT_RK2) == 0
    slab.set_option(ea.OPT_ADVECT_RK2, 0)
    slab.close(); sim.close()


def test_switched_on_and_off_again_is_the_default():
    text = scenario_text(load("filter_frames.npz"))
    a = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL).load_text(text)
    b = ea.Simulation(X, Y, dot_mode=ea.DOT_SEQUENTIAL).load_text(text)
    b.set_option(ea.OPT_ADVECT_RK2, 1)
    b.set_option(ea.OPT_ADVECT_RK2, 0)
    for f in range(20):
        a.step(); b.step()
        for fld in (ea.F_U, ea.F_V, ea.F_COUNT, ea.F_MARKERS):
            assert_bits(b.get(fld), a.get(fld), "frame %d field %d" % (f, fld))


# ----------------------------------------------------------------------------- teacher-forced stages
@pytest.mark.parametrize("scn", SCENARIOS)
def test_teacher_forced_rk2_stages_vs_restatement(ar, scn):
    g = load(scn + "_substep.npz")
    dt = float(g["dt"])
    sim = rk2_sim(X, Y, dot_mode=ea.DOT_SEQUENTIAL, rainbow=True)
    load_substep_state(sim, g)
    o = Oracle(X, Y, rainbow=True)
    for n in ("solid", "source", "sink"):
        getattr(o, n)[...] = g[n]
    for n in ("u", "v", "utmp", "vtmp", "count", "prev_count"):
        getattr(o, n)[...] = g["before_" + n]
    o.set_markers(g["before_markers"])
    o.c.rng_state = int(g["rng_before"]); o.c.source_exhausted = int(g["exhausted_before"])
    rng = np.random.default_rng(7)
    for fld, q in zip(DYE, (o.cr, o.cg, o.cb)):
        q[...] = rng.random((Y, X), dtype=np.float32)
        sim.set(fld, q)
    ms0 = sim.stats().marker_dt_events
    sim.stage(ea.STAGE_ADVECT_MARKERS, dt)
    ref.advect_markers(ar, o, dt, 1)
    assert_bits(sim.get(ea.F_MARKERS), o.markers, scn + " markers")
    if scn == "filter":
        assert sim.stats().marker_dt_events - ms0 >= 1
    sim.stage(ea.STAGE_REFRESH_COUNTS)
    o.lib.eo_refresh_marker_counts(o.ptr)
    sim.stage(ea.STAGE_SOURCES)
    for q in (o.cr, o.cg, o.cb):
        o.lib.eo_extrapolate(o.ptr, o.f32p(q), 0)
    o.lib.eo_update_fluid_sources(o.ptr)
    sim.stage(ea.STAGE_EXTRAPOLATE)
    for q, t in ((o.u, U), (o.v, V)):
        o.lib.eo_extrapolate(o.ptr, o.f32p(q), t)
    for q, t in ((o.u, U), (o.v, V)):
        o.lib.eo_zero_bounds(o.ptr, o.f32p(q), t)
    assert_bits(sim.get(ea.F_U), o.u, scn + " u in front of advection")
    sim.stage(ea.STAGE_ADVECT_VELOCITY, dt)
    ref.advect_velocity_stage(ar, o, dt, 1)
    assert_bits(sim.get(ea.F_UTMP), o.utmp, scn + " utmp")
    assert_bits(sim.get(ea.F_VTMP), o.vtmp, scn + " vtmp")
    for fld, q in zip(DYE, (o.cr, o.cg, o.cb)):
        assert_bits(sim.get(fld), q, "%s dye %d" % (scn, fld))
    sim.close()


# ----------------------------------------------------------------------------- free-running
@pytest.mark.parametrize("scn", SCENARIOS)
def test_free_running_rk2_bit_exact_vs_restatement(ar, scn):
    text = scenario_text(load(scn + "_frames.npz"))
    dye = scn == "waterfall"
    sim = rk2_sim(X, Y, dot_mode=ea.DOT_SEQUENTIAL, rainbow=dye).load_text(text)
    o = Oracle(X, Y, rainbow=dye).load_text(text)
    for f in range(100):
        sim.step()
        ref.step(ar, o, 1)
        st = sim.stats()
        assert st.last_substeps == o.c.last_substeps and st.last_pcg_iterations == o.c.last_pcg_iterations, (scn, f)
        compare_state(o, sim, "%s frame %d" % (scn, f), dye=dye)
    assert sim.stats().marker_multi_events == 0
    sim.close()


# ----------------------------------------------------------------------------- the marker forms
def test_marker_forms_agree_under_rk2_on_a_moving_4096_dam_break():
    """default (column-major, fused binning), MARKERS_TWO_PASS, MARKERS_ROWMAJOR, NO_TILE_MAP: the same bits with the tile map and the
    column-major copies active (a falling 4096^2 dam break, frames 50-52)"""
    kw = dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=20)
    sims = []
    for key in (None, ea.OPT_MARKERS_TWO_PASS, ea.OPT_MARKERS_ROWMAJOR, ea.OPT_NO_TILE_MAP):
        s = rk2_sim(4096, 4096, **kw).load_text(scenarios.dam_break(), upscale=True)
        if key is not None:
            s.set_option(key, 1)
        sims.append(s)
    for f in range(53):
        for s in sims:
            s.step()
        if f < 50:
            continue
        a = sims[0]
        for fld in (ea.F_MARKERS, ea.F_COUNT, ea.F_U, ea.F_V):
            want = a.get(fld)
            for k, b in enumerate(sims[1:]):
                got = b.get(fld)
                assert got.shape == want.shape and np.array_equal(got.view(np.uint8), want.view(np.uint8)), "frame %d field %d form %d" % (f, fld, k + 1)
                del got
            del want
    assert sims[0].stats().marker_multi_events == 0
    assert np.abs(sims[0].get(ea.F_V)).max() > 1.0      # (moving: the column is falling)
    for s in sims:
        s.close()


@pytest.mark.parametrize("shape,seed,n,solid_frac", [((96, 72), 1, 6000, 0.25), ((200, 130), 2, 60000, 0.15)])
@pytest.mark.parametrize("form", ["one_pass", "two_pass", "rowmajor"])
def test_random_marker_stress_rk2_vs_restatement(ar, shape, seed, n, solid_frac, form):
    X2, Y2 = shape
    solid, sink, m, u, v = _random_marker_state(X2, Y2, seed, n, solid_frac)
    o = Oracle(X2, Y2)
    o.solid[...] = solid; o.sink[...] = sink; o.u[...] = u; o.v[...] = v
    o.set_markers(m)
    o.lib.eo_refresh_marker_counts(o.ptr)
    o.lib.eo_refresh_marker_counts(o.ptr)
    sim = rk2_sim(X2, Y2, dot_mode=ea.DOT_SEQUENTIAL)
    if form == "two_pass":
        sim.set_option(ea.OPT_MARKERS_TWO_PASS, 1)
    if form == "rowmajor":
        sim.set_option(ea.OPT_MARKERS_ROWMAJOR, 1)
    for f, a in ((ea.F_SOLID, solid), (ea.F_SOURCE, np.zeros_like(solid)), (ea.F_SINK, sink), (ea.F_U, u), (ea.F_V, v),
                 (ea.F_COUNT, o.count), (ea.F_PREV_COUNT, o.prev_count)):
        sim.set(f, a)
    sim.set_markers(o.markers)
    for rep in range(3):
        dt = sim.timestep(0.1)
        assert dt == o.timestep(0.1)
        sim.stage(ea.STAGE_ADVECT_MARKERS, dt)
        ref.advect_markers(ar, o, dt, 1)
        assert_bits(sim.get(ea.F_MARKERS), o.markers, "advect rep %d" % rep)
        sim.stage(ea.STAGE_REFRESH_COUNTS)
        o.lib.eo_refresh_marker_counts(o.ptr)
        assert_bits(sim.get(ea.F_MARKERS), o.markers, "compaction rep %d" % rep)
        assert_bits(sim.get(ea.F_COUNT), o.count, "count rep %d" % rep)
    st = sim.stats()
    assert st.marker_dt_events > 5 and st.marker_multi_events == 0
    sim.close()


# ----------------------------------------------------------------------------- larger grids
def test_1024_dam_break_rk2_bit_exact_vs_restatement(ar):
    text = scenarios.dam_break()
    sim = rk2_sim(1024, 1024, dot_mode=ea.DOT_SEQUENTIAL).load_text(text, upscale=True)
    o = Oracle(1024, 1024).load_text(text, upscale=True)
    for f in range(3):
        sim.step()
        ref.step(ar, o, 1)
        st = sim.stats()
        assert st.last_substeps == o.c.last_substeps and st.last_pcg_iterations == o.c.last_pcg_iterations, f
        compare_state(o, sim, "1024 dam break frame %d" % f)
    sim.close()


def _max_div(sim):
    u, v, c = sim.get(ea.F_U), sim.get(ea.F_V), sim.get(ea.F_COUNT)
    s = sim.get(ea.F_SOLID)
    div = np.zeros_like(u)
    div[1:, 1:] = u[1:, 1:] - u[1:, :-1] + v[1:, 1:] - v[:-1, 1:]
    fl = (c != 0) & (s == 0)
    interior = np.zeros_like(fl)
    interior[2:-2, 2:-2] = fl[2:-2, 2:-2] & fl[1:-3, 2:-2] & fl[3:-1, 2:-2] & fl[2:-2, 1:-3] & fl[2:-2, 3:-1]
    return float(np.abs(div[interior]).max())


def test_1024_dam_break_multilevel_converged_rk2_stays_sound():
    """the multilevel mode solved to 1e-6 for 20 frames: finite fields, no marker crossing two boundaries, divergence as small as RK1's"""
    divs = {}
    for rk2 in (0, 1):
        sim = ea.Simulation(1024, 1024, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE_MG, max_iterations=2000).load_text(scenarios.dam_break(), upscale=True)
        sim.set_option(ea.OPT_ADVECT_RK2, rk2)
        for f in range(20):
            sim.step()
            assert sim.stats().last_residual <= 1e-6, (rk2, f)
        u, v = sim.get(ea.F_U), sim.get(ea.F_V)
        assert np.isfinite(u).all() and np.isfinite(v).all()
        assert sim.stats().marker_multi_events == 0
        divs[rk2] = _max_div(sim)
        sim.close()
    assert divs[1] < 1e-4 and divs[1] <= 4 * divs[0] + 1e-6, divs


# ----------------------------------------------------------------------------- the rotation, on the device
def _rotation_sim(rk2):
    u, v, count, sink = ref.rotation_fields()
    z = np.zeros_like(count)
    sim = ea.Simulation(ref.ROT_N, ref.ROT_N, dot_mode=ea.DOT_SEQUENTIAL)
    sim.set_option(ea.OPT_ADVECT_RK2, rk2)
    for f, a in ((ea.F_SOLID, z), (ea.F_SOURCE, z), (ea.F_SINK, sink), (ea.F_U, u), (ea.F_V, v), (ea.F_COUNT, count), (ea.F_PREV_COUNT, count)):
        sim.set(f, a)
    return sim


def test_rotation_checks_on_the_device(ar):
    from test_advect_rk2_host import _rotation_oracle
    o = _rotation_oracle()
    dt = o.timestep(0.1)
    err = {}
    drift = {}
    for rk2 in (0, 1):
        e = []
        for h in (dt, dt / 2):
            sim = _rotation_sim(rk2)
            assert sim.timestep(0.1) == dt
            sim.stage(ea.STAGE_ADVECT_VELOCITY, h)
            o.u[...] = sim.get(ea.F_U); o.v[...] = sim.get(ea.F_V)
            ref.advect_velocity_stage(ar, o, h, rk2)
            ut = sim.get(ea.F_UTMP)
            assert_bits(ut, o.utmp, "rotation utmp rk2=%d" % rk2)
            e.append(ref.rotation_u_error(ut, np.float32(h)))
            sim.close()
        err[rk2] = e
        sim = _rotation_sim(rk2)
        sim.set_markers(ref.rotation_markers())
        for _ in range(20):
            sim.stage(ea.STAGE_ADVECT_MARKERS, dt)
        m = sim.get(ea.F_MARKERS)
        o.set_markers(ref.rotation_markers())
        for _ in range(20):
            ref.advect_markers(ar, o, dt, rk2)
        assert_bits(m, o.markers, "rotation markers rk2=%d" % rk2)
        drift[rk2] = ref.radius_drift(m)
        sim.close()
    assert 3.0 <= err[0][0] / err[0][1] <= 5.0 and err[1][0] / err[1][1] >= 6.0, err
    assert drift[0] > 0.1 and drift[1] <= drift[0] / 20, drift


# ----------------------------------------------------------------------------- snapshot, front end
def test_snapshot_resume_under_rk2(tmp_path):
    text = scenario_text(load("waterfall_frames.npz"))
    a = rk2_sim(X, Y, dot_mode=ea.DOT_SEQUENTIAL).load_text(text)
    for _ in range(15):
        a.step()
    path = str(tmp_path / "mid.snap")
    a.save_state(path)
    b = rk2_sim(X, Y, dot_mode=ea.DOT_SEQUENTIAL).load_state(path)
    for f in range(15):
        a.step(); b.step()
        for fld in (ea.F_U, ea.F_V, ea.F_COUNT, ea.F_MARKERS):
            assert_bits(b.get(fld), a.get(fld), "resumed frame %d field %d" % (f, fld))
    a.close(); b.close()


def test_cli_advection_flag(ar, tmp_path):
    g = load("block_frames.npz")
    scn = tmp_path / "block.txt"
    scn.write_text(scenario_text(g))
    exe = os.path.join(os.path.dirname(ea.LIB_PATH), "..", "bin", "euler")
    base = [exe, "--dump", "--frames", "6", "--window", "98x38"]
    rk2 = subprocess.run(base + ["--advection", "rk2", str(scn)], capture_output=True, timeout=120)
    assert rk2.returncode == 0, rk2.stderr.decode()
    o = Oracle(X, Y).load_text(scenario_text(g))
    frames = rk2.stdout.split(b"--- frame ")[1:]
    assert len(frames) == 7
    for k in range(7):
        if k:
            ref.step(ar, o, 1)
        header, body = frames[k].split(b"\n", 1)
        n = int(header.split(b"(")[1].split()[0])
        assert body[:n] == o.render(98, 38), k
    plain = subprocess.run(base + [str(scn)], capture_output=True, timeout=120)
    rk1 = subprocess.run(base + ["--advection", "rk1", str(scn)], capture_output=True, timeout=120)
    assert plain.returncode == rk1.returncode == 0 and plain.stdout == rk1.stdout
    bad = subprocess.run(base + ["--advection", "rk3", str(scn)], capture_output=True, timeout=60)
    assert bad.returncode == 1 and b"--advection rk1|rk2" in bad.stderr
