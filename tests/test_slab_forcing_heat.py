"""Forcing and temperature on row-slab handles (docs/forcing.md, docs/heat.md "On row slabs"): 2-3 gloo ranks sharing the test box's GPU, each holding one slab,
against a whole-grid handle in the same process (tests/slab_forcing_worker.py; the pattern of tests/test_slab_rows.py).  The whole-grid handle's forcing and heat
are pinned bit for bit against tests/forcing_ref.py and tests/heat_ref.py, so agreement with it is agreement with the restatements.

Neither feature has a reduction of its own: with the velocities of the whole-grid run fed back behind every solve (the solve's dot products are summed per rank,
tests/test_slab_rows.py), T, utmp, vtmp, the count grids and the markers are the whole-grid handle's BIT FOR BIT in every substep.  In a free run they follow
the solve's tolerance.

With the dye on, euler_stage refuses a slab handle (the dye's steps sit between the stages), so the --rainbow case takes whole substeps and compares behind each:
T, the count grids and the markers as the stages left them, and utmp / vtmp, which the projection reads and leaves - so a stale ghost row of T under the buoyancy
would show in the slab's top row there too."""
import json
import os

import numpy as np
import pytest

import euler_amd as ea
import ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "slab_forcing_worker.py")
EULER_EINVAL, EULER_ESTATE = -1, -5


def run(nproc, X, Y, workload, mode, port, extra=()):
    rc, out, err = ranks.launch(nproc, WORKER, [X, Y, workload, mode] + list(extra), port, timeout=600)
    assert rc == 0, (out[-1500:], err[-3000:])
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def all_true(rec):
    return all(bool(v) for v in rec.values())


def check_substeps(log, who):
    for i, s in enumerate(log):
        assert s["dt"][0] == s["dt"][1], (who, i, s)
        assert s["time"][0] == s["time"][1], (who, i, s)
        for point in ("sources", "advect", "substep"):
            if point in s:
                assert all_true(s[point]), (who, i, point, s[point])
        assert ("sources" in s and "advect" in s) or "substep" in s


# ----------------------------------------------------------------------------- 1 and 3: teacher-forced at the velocity, bit for bit; raster and fill behind it
@pytest.mark.gpu
@pytest.mark.parametrize("nproc,X,Y,extra", [
    (3, 200, 192, ()),                              # one band each: boundaries at rows 64 and 128
    (2, 103, 150, ("bands=0-1,1-3",)),              # ragged X, an uneven partition, a last band of 22 rows
    (3, 200, 192, ("rainbow",)),                    # the dye's channels and T travel in one exchange behind the sources
    (2, 200, 192, ("kappa=0",)),                    # no diffusion: no T exchange in front of it
    (2, 200, 192, ("beta=0",)),                     # passive: T's ghost rows travel with vtmp's behind the stage
    (2, 200, 192, ("kappa=0", "beta=0")),           # ... and so they do when nothing inside the stage reads them
])
def test_teacher_forced_slabs_are_the_whole_grid_bit_for_bit(nproc, X, Y, extra, tmp_path):
    d = run(nproc, X, Y, "dam_break", "teacher", 29701, tuple(extra) + ("path=" + str(tmp_path / "state.snap"),))
    # the test is about rows that hold water on both sides of every slab boundary, at the first and the last substep
    assert d["water_first"] and d["water_last"], d["rows"]
    assert d["T0_spread"][0] < 1.0 < d["T0_spread"][1]      # the saved field is not ambient everywhere: FIX -2 and FIX 8 have acted
    for r, p in enumerate(d["per_rank"]):
        assert len(p["substeps"]) == 12
        check_substeps(p["substeps"], ("rank", r))
        # euler_heat_raster: every rank reads the whole-grid handle's bytes
        assert len(p["rasters"]) >= 12 and all(x[3] for x in p["rasters"]), (r, [x for x in p["rasters"] if not x[3]])
        assert any(x[4] > 0 for x in p["rasters"])
        # euler_heat_fill, then a substep that reads the ghost rows it refreshed
        assert p["fill_T"], r
        check_substeps(p["after_fill"], ("after the fill, rank", r))
        # a load with heat on: ambient over the whole window
        assert p["load_leaves_ambient"], r
        check_substeps(p["after_load"], ("after the load, rank", r))
    assert d["fill_changed"]


# ----------------------------------------------------------------------------- 2: the free run
@pytest.mark.gpu
@pytest.mark.parametrize("nproc,X,Y,workload", [(2, 256, 256, "waterfall"), (3, 200, 330, "waterfall")])      # (free fall first: solves that converge; sources set source_t)
def test_free_run_follows_the_solve_and_keeps_the_maximum_principle(nproc, X, Y, workload):
    """10 frames of euler_step with the same records on both sides: the structural invariants and the u / v / p bounds of
    test_row_slabs_reproduce_the_single_gpu_run up to the first capped frame; the clocks are equal; with no RATE box every T lies within the minimum and maximum
    over ambient, source_t and the FIX values (interpolation, FIX, the extension's mean and diffusion with kappa dt <= 1/4 are convex combinations).  T's distance
    from the whole-grid run behind the solves is printed, not asserted: it inherits the solve's rounding through a chaotic flow (docs/heat.md)."""
    d = run(nproc, X, Y, workload, "free", 29711)
    capped, checked = False, 0
    for i, f in enumerate(d["frames"]):
        print("frame %d: dT %.3g du %.3g dv %.3g dp %.3g (pmax %.3g, iterations %s) T in [%g, %g]" % (i, f["dT"], f["du"], f["dv"], f["dp"], f["pmax"], f["iters"], f["T_range"][0], f["T_range"][1]))
        assert f["markers_in_rows"] and f["keys_cover_own_count"], (i, f)
        assert f["T_in_bounds"], (i, f["T_range"], d["T_bound"])
        assert len(set(f["time"])) == 1, (i, f["time"])
        capped = capped or (f["iters"][0] >= 100 * f["substeps"][0] and f["pmax"] > 0)
        if capped:
            continue
        checked += 1
        assert f["substeps"][0] == f["substeps"][1] and f["count_differ"] == 0 and f["markers_at_keys"], (i, f)
        assert f["dp"] <= 1e-8 * f["pmax"] + 2e-6 and f["du"] < 1e-6 and f["dv"] < 1e-6, (i, f)
    assert checked > 0 and d["frames"][-1]["T_moved"]


# ----------------------------------------------------------------------------- 4: properties
@pytest.mark.gpu
def test_untouched_job_memory_and_box_launches():
    X, Y = 200, 192
    d = run(3, X, Y, "dam_break", "props", 29721)
    for r, p in enumerate(d["per_rank"]):
        # the default record set before every frame, heat never on: the bits and the launches of a job that never called either entry point
        assert p["untouched_same_bits"] == [[]] * 4, (r, p["untouched_same_bits"])      # (per frame: the fields that differ)
        for fr in p["untouched_launches"]:
            assert fr and all(a == b for a, b in fr.values()), (r, fr)
        # two halves of the window (own rows + 1 ghost row below + 2 above, clipped to the grid), then the boxes' 1536 bytes and the rank's table entries
        assert p["heat_bytes"][0] == p["heat_bytes"][1] > 0, (r, p["heat_bytes"])
        assert p["box_buffer_bytes"] == 64 * 24 + (16 if r == 0 else 0), (r, p["box_buffer_bytes"])
        # a force box and a heat box inside the lowest band: two more launches there, none on a rank no box touches
        assert p["box_launches"] == [2 if r == 0 else 0], (r, p["box_launches"])
        # three handles with heat, boxes and a raster created, stepped and destroyed: each counts the same bytes before and behind switching on, more behind
        assert len(p["life_cycle"]) == 3 and all(c == p["life_cycle"][0] and c[1] > c[0] for c in p["life_cycle"]), (r, p["life_cycle"])


@pytest.mark.gpu
def test_disagreement_is_an_error_on_every_rank_and_changes_nothing():
    d = run(3, 200, 192, "dam_break", "disagree", 29731)
    for r, p in enumerate(d["per_rank"]):
        c = p["cases"]
        for name in ("beta", "box_order", "heat_box_order", "off_on_one_rank"):
            assert c[name][0] == EULER_ESTATE and "differs between ranks" in c[name][1] and c[name][2], (r, name, c[name])
        for name, word in (("invalid", "gravity"), ("invalid_heat", "kappa")):
            if r == 2:      # the rank with the bad record keeps its own refusal
                assert c[name][0] == EULER_EINVAL and word in c[name][1] and c[name][2], (r, name, c[name])
            else:
                assert c[name][0] == EULER_ESTATE and c[name][2], (r, name, c[name])
        assert p["stepped_on"] and p["off_together"], r


# ----------------------------------------------------------------------------- 5: refusals
@pytest.mark.gpu
def test_sessions_and_the_other_advections_still_refuse_slabs(tmp_path):
    d = run(2, 200, 192, "dam_break", "refuse", 29741, ("path=" + str(tmp_path / "s.session"),))
    for r, p in enumerate(d["per_rank"]):
        for name in ("save_session", "load_session", "rk2", "maccormack"):
            assert p["refused"][name][0] != 0 and "slab" in p["refused"][name][1], (r, name, p["refused"][name])


@pytest.mark.gpu
def test_without_a_communicator_every_call_refuses_first():
    """behind the null check, in front of "nothing loaded" and of any look at the record: EULER_ESTATE with "slab" in the text"""
    L = ea.load_library()
    err = lambda: L.euler_last_error()
    X, Y = 200, 192
    slab = ea.Simulation(X, Y, slab=(0, 2))
    f = ea.forcing_default()
    f["reserved"] = 1      # a record its own check refuses
    h = ea.heat_default()
    h["reserved"] = 1
    buf = np.zeros((Y, X), np.float32)
    px = np.zeros((3, 4), ea.HEAT_PX_DTYPE)
    assert L.euler_set_forcing(None, f.ctypes.data, None) == EULER_EINVAL and L.euler_set_forcing(slab.h, None, None) == EULER_EINVAL      # the null check comes first
    assert L.euler_set_forcing(slab.h, f.ctypes.data, None) == EULER_ESTATE and b"slab" in err()
    assert L.euler_set_heat(slab.h, h.ctypes.data, None) == EULER_ESTATE and b"slab" in err()
    assert L.euler_set_heat(slab.h, None, None) == EULER_ESTATE and b"slab" in err()
    assert L.euler_heat_get_field(slab.h, buf.ctypes.data, buf.nbytes) == EULER_ESTATE and b"slab" in err()
    assert L.euler_heat_set_field(slab.h, buf.ctypes.data, buf.nbytes) == EULER_ESTATE and b"slab" in err()
    assert L.euler_heat_fill(slab.h, 1, 1, 5, 5, 1.0) == EULER_ESTATE and b"slab" in err()
    assert L.euler_heat_raster(slab.h, 1, 1, 50, 30, 4, 3, px.ctypes.data, px.nbytes) == EULER_ESTATE and b"slab" in err()
    with pytest.raises(ea.EulerError) as e:
        slab.set_forcing((0, -5))
    assert e.value.code == EULER_ESTATE and "slab" in str(e.value)
    with pytest.raises(ea.EulerError) as e:
        slab.set_heat(0.0, 0.5)
    assert e.value.code == EULER_ESTATE and "slab" in str(e.value)
    # the clock and the getters need no communicator: they are local
    slab.time = 2.5
    assert slab.time == 2.5 and slab.forcing()[0].tobytes() == ea.forcing_default().tobytes()
    slab.close()
