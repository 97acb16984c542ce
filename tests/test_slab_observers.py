"""The observer passes on row-slab handles (docs/observer_passes.md "On row slabs"): euler_overview, euler_overview_box, euler_render_fit, euler_diagnostics,
euler_flow_raster, euler_gauges, euler_marker_raster and euler_render_view are collective there and return, on every rank, the bytes a whole-grid handle holding
the same state returns.  2 - 3 gloo ranks sharing the test box's one MI355X (tests/slab_observers_worker.py through tests/ranks.py); every launch runs many checks.

Every comparison is for equal bytes - the records are integer sums, integer extremes and maxima of bit patterns - against the numpy restatements
(overview_ref, viewport_ref, diagnostics_ref, flow_ref, gauges_ref) on the state assembled from the ranks' own rows, and between the ranks."""
import json
import os

import pytest

import euler_amd as ea
import ranks
from euler_amd import scenarios

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "slab_observers_worker.py")
EULER_EINVAL, EULER_ESTATE = -1, -5


def run(nproc, X, Y, workload, frames, mode, port, extra=(), timeout=600):
    rc, out, err = ranks.launch(nproc, WORKER, [X, Y, workload, frames, mode] + list(extra), port, timeout=timeout)
    assert rc == 0, (out[-1500:], err[-4000:])
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def clean(d, what):
    print(what, {k: v for k, v in d.items() if k not in ("differ_between_ranks", "differ_from_reference")})
    assert d["differ_between_ranks"] == [] and d["differ_from_reference"] == [] and d["n"] > 20, (what, d)


@pytest.mark.gpu
@pytest.mark.parametrize("nproc,X,Y,workload,frames,extra", [
    (3, 200, 330, "waterfall", 12, ()),                          # sources and sinks; 6 bands, the last of 10 rows
    (3, 203, 192, "half_tank", 10, ()),                          # X % 4 != 0: one cell per lane; water across the boundaries at rows 64 and 128
    (2, 256, 256, "waterfall", 12, ("rainbow",)),                # the dye sums
    (3, 200, 330, "waterfall", 15, ("bands=0-1,1-3,3-6",)),      # an uneven partition: the lowest slab is a single band
])
def test_every_pass_returns_the_whole_grid_bytes_on_every_rank(nproc, X, Y, workload, frames, extra):
    d = run(nproc, X, Y, workload, frames, "all", 29701, extra)
    assert d["world"] == nproc
    clean(d["loaded"], "after the load")
    clean(d["stepped"], "after %d frames" % frames)
    clean(d["substep"], "after a substep")
    assert d["stepped"]["fluid"] > 0 and d["stepped"]["markers"] > 0
    if "rainbow" not in extra:
        assert len(d["stages"]) == 6
        for k, s in enumerate(d["stages"]):
            clean(s, "after stage %d" % k)
    clean(d["sink_edit"], "after one rank's euler_set_field(SINK)")
    assert d["sink_edit"]["row_below_follows"], d["sink_edit"]
    if workload == "half_tank":      # the tank's water stands across rows 63 / 64: the boxes there are not empty, and the sink cells take wet nodes away from the rank below
        assert d["stepped"]["boundary_water"] > 0 and d["stepped"]["boundary_nodes"] > 0 and all(t > 0 for t in d["stepped"]["gauge_terms"][:7]), d["stepped"]
        before, after = d["sink_edit"]["nodes_before_and_after"]
        assert after < before, d["sink_edit"]


@pytest.mark.gpu
def test_a_slab_job_that_loads_a_snapshot_matches_the_whole_grid_handle_that_saved_it(tmp_path):
    """A whole-grid handle steps and saves; two slabs load the file.  Their passes return the bytes of the passes of a whole-grid handle that loaded the same file
    (without the pressure fields: a snapshot carries no p)."""
    X, Y = 200, 330
    path = str(tmp_path / "whole.snap")
    whole = ea.Simulation(X, Y, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE).load_text(scenarios.waterfall(), upscale=True)
    for _ in range(10):
        whole.step()
    whole.save_state(path)
    whole.close()
    d = run(2, X, Y, "waterfall", 0, "snapshot", 29711, ("load=" + path,))["snapshot"]
    assert d["differ_between_ranks"] == [] and d["differ_from_whole_grid_handle"] == [] and d["n"] > 20 and d["fluid"] > 0, d
    assert d["level_after_a_frame"], d


@pytest.mark.gpu
@pytest.mark.parametrize("mode,workload,extra", [("notrace", "waterfall", ("rainbow",)), ("notrace_stages", "waterfall", ())])
def test_the_passes_leave_no_trace_in_a_slab_run(mode, workload, extra):
    """Two slab jobs of one scenario, 20 frames (notrace_stages: 20 substeps taken stage by stage); one calls every pass before every frame (behind every stage of every fourth
    substep).  At the end every rank's own rows of every field, its markers and their keys, the counters and the RNG state are the same bit for bit."""
    d = run(3, 200, 330, workload, 20, mode, 29721, extra)["notrace"]
    assert d["differ"] == [] and d["looked"] > 400 and d["markers"] > 0 and d["max_abs_v"] > 0, d      # (the water has moved: the run was one)
    if mode == "notrace":      # (euler_stage keeps none of the frame counters)
        assert d["substeps"] >= 20 and d["pcg_iterations"] > 0, d


@pytest.mark.gpu
def test_the_passes_over_the_builtin_rccl_communicator():
    """The same checks with every exchange issued to RCCL from the C library (csrc/comm_rccl.hip): as many ranks as the box has GPUs - one on the test box, which
    still runs the whole path (plan, staging, all-gather with one share, fold) through the real transport."""
    import torch
    n = max(1, min(torch.cuda.device_count(), 4))
    d = run(n, 200, 330, "waterfall", 10, "all", 29731, ("rccl",))
    assert d["world"] == n
    for k in ("loaded", "stepped", "substep"):
        clean(d[k], k)
    assert d["calls"]["allgather"] > 100, d["calls"]


@pytest.mark.gpu
def test_refusals_are_the_same_on_every_rank_and_nobody_waits():
    """A slab handle with a communicator and nothing loaded: EULER_ESTATE.  A bad box, raster, flag, list or scale: EULER_EINVAL on every rank before any exchange - the
    launcher's time limit would catch a rank left waiting.  euler_tracer_raster, euler_edit_box and euler_tracers_add still refuse slabs."""
    d = run(2, 200, 192, "half_tank", 1, "refusals", 29741, timeout=120)["refusals"]
    assert len(d) == 2
    for r in d:
        assert all(ok for ok, _, _ in r["nothing_loaded"]), r["nothing_loaded"]
        assert all(ok for ok, _, _ in r["bad_arguments"]), r["bad_arguments"]
        assert all(ok and "slab" in msg for ok, _, msg in r["still_whole_grid_only"]), r["still_whole_grid_only"]
        assert r["works_afterwards"]
