"""Worker for tests/test_slab_observers.py: N rank processes (gloo, all sharing cuda:0; "rccl": the library's own communicator, one rank per GPU), each holding ONE row
slab of the job.  The observer passes are collective there; every rank must get the bytes a whole-grid handle holding the same state would: the numpy restatements on
the state assembled from the ranks' own rows (rank 0 computes them), or a whole-grid handle's own passes (the snapshot mode).  Rank 0 prints one JSON line.

  slab_observers_worker.py X Y workload frames mode [rainbow] [rccl] [bands=0-1,1-3,3-6] [load=FILE]
  mode: all | snapshot | notrace | notrace_stages | refusals"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.distributed as dist

import euler_amd as ea
import diagnostics_ref as dref
import flow_ref as fref
import gauges_ref as gref
import overview_ref as oref
import viewport_ref as vref
from euler_amd import scenarios
from euler_amd.slab import SLAB_LOCAL, RcclComm, TorchComm

EULER_EINVAL, EULER_ESTATE = -1, -5
DYE = (ea.F_DYE_R, ea.F_DYE_G, ea.F_DYE_B)
ARGS = sys.argv[6:]


def opt(name):
    return next((a[len(name) + 1:] for a in ARGS if a.startswith(name + "=")), None)


def load(sim, workload):
    if workload == "half_tank":
        sim.load_half_tank()
    else:
        sim.load_text(getattr(scenarios, workload)(), upscale=True)
    return sim


def make_slab(X, Y, rank, world, rainbow, rccl, local):
    slab = (rank, world)
    if opt("bands"):
        lo, hi = opt("bands").split(",")[rank].split("-")
        slab = (rank, world, int(lo), int(hi))
    sim = ea.Simulation(X, Y, device=local, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, slab=slab, rainbow=rainbow)
    comm = RcclComm(sim, SLAB_LOCAL) if rccl else TorchComm(sim, SLAB_LOCAL)
    return sim, comm


# ----------------------------------------------------------------------------- the calls, in one order on every rank
def boxes_of(X, Y, light=False):
    """light: the whole interior and the two rows across the boundary only (the rounds between the stages)"""
    b = [("interior", (1, 1, X - 2, Y - 2)), ("rows63_64", (1, 63, X - 2, 64)), ("one_rank", (5, 70, min(60, X - 2), 120)), ("column", (X // 2, 1, X // 2, Y - 2))]
    if Y > 130:
        b.append(("rows127_128", (3, 127, X - 3, 128)))
    return b[:2] if light else b


def rasters_of(box, light=False):
    bw, bh = box[2] - box[0] + 1, box[3] - box[1] + 1
    out = [(bw, bh), (1, min(2, bh)), (min(bw, 7), min(bh, 37)), (bw, 1)]      # H = Bh and W = Bw; W = 1, H = 2; a prime H; one pixel row that every rank shares
    return list(dict.fromkeys(out[:2] if light else out))


def gauge_list(X, Y):
    g = [(ea.GAUGE_PRESSURE, (5, 63, 5, 63)), (ea.GAUGE_PRESSURE, (5, 64, 5, 64)), (ea.GAUGE_FORCE, (1, 1, 2, Y - 2)), (ea.GAUGE_FORCE, (1, 1, X - 2, 3)),
         (ea.GAUGE_FLUX, (10, 60, min(60, X - 2), 70)), (ea.GAUGE_FLUX, (3, 64, X - 3, 64)), (ea.GAUGE_FLUX, (3, 63, X - 3, 63)), (ea.GAUGE_LEVEL, (X // 3, 1, X // 3 + 2, Y - 2))]
    if Y > 130:
        g += [(ea.GAUGE_PRESSURE, (7, 127, 7, 128)), (ea.GAUGE_FLUX, (10, 120, min(60, X - 2), 135)), (ea.GAUGE_FORCE, (X - 3, 100, X - 2, 140))]
    return g


def random_gauges(X, Y, n, kinds, seed=11):
    rng = np.random.default_rng(seed)
    g = []
    for _ in range(n // 2):
        xa, xb = sorted(int(t) for t in rng.integers(1, X - 1, 2))
        ya = int(rng.integers(1, Y - 1))
        yb = min(Y - 2, ya + int(rng.integers(0, 90)))      # small boxes, many of them across a slab boundary
        g.append((int(rng.choice(kinds)), (xa, ya, min(xb, xa + 40), yb)))
    return g + [g[int(k)] for k in rng.integers(0, len(g), n - len(g))]      # ... with repeats


def observe(sim, X, Y, pressure=True, heavy=True, light=False):
    """every pass on the slab handle: {name: array or bytes}, the same calls in the same order on every rank.  heavy: with the list of 1024 gauges"""
    out = {}
    for name, box in boxes_of(X, Y, light):
        out["diag/" + name] = sim.diagnostics_record(box)
        for (w, h) in rasters_of(box, light):
            key = "%s/%dx%d" % (name, w, h)
            out["overview/" + key] = sim.overview(w, h, box=box)
            out["flow/" + key] = sim.flow(w, h, box=box)
            if pressure:
                out["flowp/" + key] = sim.flow(w, h, box=box, pressure=True)
    out["overview/whole/9x5"] = sim.overview(9, 5)
    kinds = (ea.GAUGE_LEVEL, ea.GAUGE_PRESSURE, ea.GAUGE_FORCE, ea.GAUGE_FLUX) if pressure else (ea.GAUGE_LEVEL, ea.GAUGE_FLUX)
    out["gauges/list"] = sim.gauges([g for g in gauge_list(X, Y) if g[0] in kinds])
    if heavy:
        out["gauges/1024"] = sim.gauges(random_gauges(X, Y, 1024, kinds))
    mbox = (10, 58, min(40, X - 2), 69)      # across the boundary at row 64
    for s in (1, 2, 16):
        out["raster/%d" % s] = sim.marker_raster(mbox, s)
    if Y > 130:
        out["raster/127"] = sim.marker_raster((3, 120, X - 3, 135), 2)
    out["view/zoom"] = sim.render_view(mbox, 98, 38)
    out["view/wide"] = sim.render_view((1, 40, X - 2, 140 if Y > 142 else Y - 2), 98, 38)
    out["fit/98x38"] = sim.render_fit(98, 38)
    out["fit/all"] = sim.render_fit(1000, 1000)
    return out


def expected(st, X, Y, rainbow, pressure=True, heavy=True, light=False):
    """the same through the numpy restatements on the assembled state st = {field: whole-grid array, "markers": (n, 2)}"""
    solid, sink, count, u, v, p = (st[f] for f in (ea.F_SOLID, ea.F_SINK, ea.F_COUNT, ea.F_U, ea.F_V, ea.F_PRESSURE))
    dye = tuple(st[f] for f in DYE) if rainbow else None
    out = {}
    for name, box in boxes_of(X, Y, light):
        out["diag/" + name] = dref.diag_ref(solid, count, u, v, box)
        for (w, h) in rasters_of(box, light):
            key = "%s/%dx%d" % (name, w, h)
            out["overview/" + key] = vref.overview_box_ref(solid, sink, count, u, v, dye, box, w, h)
            out["flow/" + key] = fref.flow_ref(solid, sink, count, u, v, box, w, h)
            if pressure:
                out["flowp/" + key] = fref.flow_ref(solid, sink, count, u, v, box, w, h, p=p)
    out["overview/whole/9x5"] = oref.overview_ref(solid, sink, count, u, v, dye, 9, 5)
    kinds = (ea.GAUGE_LEVEL, ea.GAUGE_PRESSURE, ea.GAUGE_FORCE, ea.GAUGE_FLUX) if pressure else (ea.GAUGE_LEVEL, ea.GAUGE_FLUX)
    out["gauges/list"] = gref.gauges_ref(solid, count, u, v, p, [g for g in gauge_list(X, Y) if g[0] in kinds])
    if heavy:
        out["gauges/1024"] = gref.gauges_ref(solid, count, u, v, p, random_gauges(X, Y, 1024, kinds))
    mbox = (10, 58, min(40, X - 2), 69)
    for s in (1, 2, 16):
        out["raster/%d" % s] = vref.raster_ref(st["markers"], mbox, s)
    if Y > 130:
        out["raster/127"] = vref.raster_ref(st["markers"], (3, 120, X - 3, 135), 2)
    for name, box in (("view/zoom", mbox), ("view/wide", (1, 40, X - 2, 140 if Y > 142 else Y - 2))):
        bw, bh = box[2] - box[0] + 1, box[3] - box[1] + 1
        s = vref.view_zoom(bw, bh, 98, 38)
        if s:
            out[name] = ea.view_text(vref.overview_box_ref(solid, sink, count, u, v, dye, box, bw, bh).astype(ea.OVERVIEW_DTYPE), vref.raster_ref(st["markers"], box, s), s, rainbow=rainbow)
        else:
            out[name] = ea.overview_text(vref.overview_box_ref(solid, sink, count, u, v, dye, box, min(98, bw), min(38, bh)).astype(ea.OVERVIEW_DTYPE), rainbow=rainbow)
    out["fit/98x38"] = ea.overview_text(oref.overview_ref(solid, sink, count, u, v, dye, min(98, X - 2), min(38, Y - 2)).astype(ea.OVERVIEW_DTYPE), rainbow=rainbow)
    out["fit/all"] = ea.overview_text(oref.overview_ref(solid, sink, count, u, v, dye, X - 2, Y - 2).astype(ea.OVERVIEW_DTYPE), rainbow=rainbow)
    return out


def as_bytes(a):
    return a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()


def digest(results):
    return {k: hashlib.sha1(as_bytes(a)).hexdigest() for k, a in results.items()}


def assemble(sim, rainbow, world):
    """every rank's own rows of the fields and its markers -> the whole-grid state, on every rank"""
    mine = {f: sim.get(f) for f in (ea.F_SOLID, ea.F_SINK, ea.F_COUNT, ea.F_U, ea.F_V, ea.F_PRESSURE) + (DYE if rainbow else ())}
    mine["markers"] = sim.get(ea.F_MARKERS)
    every = [None] * world
    dist.all_gather_object(every, mine)
    return {k: np.concatenate([e[k] for e in every], axis=0) for k in mine}


def compare(got, want):
    """names whose bytes differ (records compare field by field through their bytes: the restatements' dtypes are the structs')"""
    bad = []
    for k, a in got.items():
        w = want[k]
        if isinstance(a, bytes):
            same = a == w
        else:
            w = np.asarray(w)      # (a record of shape () stays one)
            same = a.shape == w.shape and a.dtype.itemsize == w.dtype.itemsize and a.tobytes() == w.tobytes()
        if not same:
            bad.append(k)
    return bad


def agree(results, world):
    """do all ranks hold rank 0's bytes?  -> names that differ somewhere"""
    every = [None] * world
    dist.all_gather_object(every, digest(results))
    return sorted({k for e in every[1:] for k in e if e[k] != every[0][k]})


def check_round(sim, X, Y, rainbow, world, rank, pressure=True, heavy=True, light=False):
    got = observe(sim, X, Y, pressure, heavy, light)
    st = assemble(sim, rainbow, world)
    d = {"differ_between_ranks": agree(got, world), "n": len(got)}
    if rank == 0:
        d["differ_from_reference"] = compare(got, expected(st, X, Y, rainbow, pressure, heavy, light))
        whole = got["diag/interior"]
        d["fluid"], d["markers"] = int(whole["fluid"]), int(whole["markers"])
        d["boundary_water"] = int(got["overview/rows63_64/1x2"]["water"].sum())
        d["boundary_nodes"] = int(got["flow/rows63_64/1x2"]["nodes"].sum())
        d["gauge_terms"] = [int(t) for t in got["gauges/list"]["terms"]]
    return d, got, st


def state_of(sim, rainbow):
    fields = (ea.F_U, ea.F_V, ea.F_UTMP, ea.F_VTMP, ea.F_COUNT, ea.F_PREV_COUNT, ea.F_SINK, ea.F_PRESSURE, ea.F_MARKERS, ea.F_MARKER_KEYS) + (DYE if rainbow else ())
    s = {str(f): sim.get(f).tobytes() for f in fields}
    t = sim.stats()
    s["counters"] = repr((t.total_substeps, t.total_pcg_iterations, t.n_markers, t.rng_state, t.source_exhausted)).encode()
    return s


def expect_code(fn, code):
    try:
        fn()
    except ea.EulerError as e:
        return [e.code == code, e.code, str(e)]
    return [False, 0, "no error"]


def main():
    X, Y, workload, frames, mode = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]), sys.argv[5]
    rccl, rainbow = "rccl" in ARGS, "rainbow" in ARGS
    if rccl:
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        local = 0
        dist.init_process_group("gloo")
        torch.cuda.set_device(0)
    rank, world = dist.get_rank(), dist.get_world_size()
    out = {"world": world, "mode": mode}

    if mode == "all":
        sim, comm = make_slab(X, Y, rank, world, rainbow, rccl, local)
        load(sim, workload)
        out["rows"] = list(sim.slab_rows())
        out["loaded"], _, _ = check_round(sim, X, Y, rainbow, world, rank, heavy=False)      # a state straight out of the load: no pressure yet, ghost rows the load's
        for _ in range(frames):
            sim.step()
        out["stepped"], before, _ = check_round(sim, X, Y, rainbow, world, rank)
        one = sim.timestep(0.1)      # ... and in the middle of a frame: behind a substep, and behind each stage of the next one (euler_stage does not take the dye)
        sim.substep(one)
        out["substep"], _, _ = check_round(sim, X, Y, rainbow, world, rank, heavy=False)
        if not rainbow:
            dt = sim.timestep(0.1)
            out["stages"] = []
            for stg in range(6):
                sim.stage(stg, dt)
                out["stages"].append(check_round(sim, X, Y, rainbow, world, rank, heavy=False, light=True)[0])
        # one rank alone edits its sink grid (euler_set_field(SINK) is local on a slab): sink cells under water in its bottom and in its top own row.  The rank BELOW reads
        # the bottom one through its ghost row above - the wet-node count of its top rows must follow
        if world > 1:
            edge = [None] * world
            dist.all_gather_object(edge, list(sim.slab_rows()))
            y = edge[1][0]      # rank 1's bottom row: the rows under it are rank 0's, their nodes look up into it
            box = (1, y - 2, X - 2, y - 1)
            flow0 = sim.flow(X - 2, 2, box=box)
            if rank == 1:
                sink, count = sim.get(ea.F_SINK).copy(), sim.get(ea.F_COUNT)
                for row in (0, -1):
                    sink[row, 2:X - 2][count[row, 2:X - 2] > 0] = 1
                sim.set(ea.F_SINK, sink)
            flow1 = sim.flow(X - 2, 2, box=box)
            out["sink_edit"], _, st = check_round(sim, X, Y, rainbow, world, rank, heavy=False)
            if rank == 0:
                want = fref.flow_ref(st[ea.F_SOLID], st[ea.F_SINK], st[ea.F_COUNT], st[ea.F_U], st[ea.F_V], box, X - 2, 2)
                out["sink_edit"]["row_below_follows"] = bool(flow1.tobytes() == np.ascontiguousarray(want).tobytes())
                out["sink_edit"]["nodes_before_and_after"] = [int(flow0["nodes"].sum()), int(flow1["nodes"].sum())]
        if rccl:
            out["calls"] = comm.counts
        elif comm.error:
            raise RuntimeError(comm.error)

    elif mode == "snapshot":
        # the slab job loads a whole-grid handle's file; the expected values are that handle's own passes (no pressure: a snapshot carries no p)
        sim, comm = make_slab(X, Y, rank, world, rainbow, rccl, local)
        sim.load_state(opt("load"))
        ref = ea.Simulation(X, Y, device=local, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, rainbow=rainbow).load_state(opt("load"))
        got, want = observe(sim, X, Y, pressure=False), observe(ref, X, Y, pressure=False)
        out["snapshot"] = {"differ_between_ranks": agree(got, world), "differ_from_whole_grid_handle": compare(got, want), "n": len(got),
                           "fluid": int(got["diag/interior"]["fluid"])}
        sim.step(); ref.step()      # ... and once more a frame on: the solve has run, so velocities carry its tolerance; the integer grids do not
        a, b = sim.gauges([(ea.GAUGE_LEVEL, (1, 1, X - 2, Y - 2))]), ref.gauges([(ea.GAUGE_LEVEL, (1, 1, X - 2, Y - 2))])
        out["snapshot"]["level_after_a_frame"] = bool(a.tobytes() == b.tobytes())
        bad = [None] * world
        dist.all_gather_object(bad, out["snapshot"]["differ_from_whole_grid_handle"])
        out["snapshot"]["differ_from_whole_grid_handle"] = sorted({k for b_ in bad for k in b_})

    elif mode in ("notrace", "notrace_stages"):
        # two slab jobs of one scenario side by side in the same processes; b is looked at all the time.  Afterwards every own row, marker, key and counter is the same
        a, ca = make_slab(X, Y, rank, world, rainbow, rccl, local)
        b, cb = make_slab(X, Y, rank, world, rainbow, rccl, local)
        load(a, workload); load(b, workload)
        looked = 0
        for f in range(frames):
            if mode == "notrace":
                looked += len(observe(b, X, Y, heavy=(f == frames // 2), light=(f != frames // 2)))      # every frame; every box, raster and the long gauge list once
                a.step(); b.step()
            else:
                dt = a.timestep(0.1)
                assert b.timestep(0.1) == dt
                for stg in range(6):
                    a.stage(stg, dt); b.stage(stg, dt)
                    if f % 4 == 0:
                        looked += len(observe(b, X, Y, heavy=False, light=True))      # between the stages of every fourth substep, the last stage included
        sa, sb = state_of(a, rainbow), state_of(b, rainbow)
        mine = sorted(k for k in sa if sa[k] != sb[k])
        every = [None] * world
        dist.all_gather_object(every, mine)
        t = a.stats()
        speed = [None] * world
        dist.all_gather_object(speed, float(np.abs(a.get(ea.F_V)).max()))
        out["notrace"] = {"differ": sorted({k for e in every for k in e}), "looked": looked, "substeps": int(t.total_substeps), "pcg_iterations": int(t.total_pcg_iterations),
                          "markers": int(t.n_markers), "max_abs_v": max(speed)}
        for c in (ca, cb):
            if not rccl and c.error:
                raise RuntimeError(c.error)

    elif mode == "refusals":
        empty, _ = make_slab(X, Y, rank, world, rainbow, rccl, local)      # a communicator, nothing loaded
        r = {"nothing_loaded": [expect_code(lambda: empty.overview(4, 4), EULER_ESTATE), expect_code(lambda: empty.diagnostics_record(), EULER_ESTATE),
                                expect_code(lambda: empty.gauges([(ea.GAUGE_LEVEL, (1, 1, 5, 5))]), EULER_ESTATE), expect_code(lambda: empty.render_fit(10, 10), EULER_ESTATE)]}
        sim, comm = make_slab(X, Y, rank, world, rainbow, rccl, local)
        load(sim, workload)
        sim.step()
        box = (1, 1, X - 2, Y - 2)
        # refused on every rank before any exchange: nobody waits for anybody (the launcher's time limit is the guard)
        r["bad_arguments"] = [expect_code(fn, EULER_EINVAL) for fn in (
            lambda: sim.overview(4, 4, box=(0, 1, 5, 5)), lambda: sim.overview(4, 4, box=(1, 1, X - 1, 5)), lambda: sim.overview(0, 4), lambda: sim.overview(4, Y),
            lambda: sim.flow(4, 4, box=(3, 9, 3, 8)), lambda: sim.flow(X, 1), lambda: sim.diagnostics_record((1, 1, 5, Y - 1)),
            lambda: _check_flags(sim, box), lambda: sim.gauges([]), lambda: sim.gauges([(ea.GAUGE_LEVEL, (1, 1, 5, 5)), (7, (1, 1, 5, 5))]),
            lambda: sim.gauges([(ea.GAUGE_FLUX, (1, 1, X, 5))]), lambda: sim.marker_raster((1, 1, 5, 5), 3), lambda: sim.marker_raster((5, 5, 4, 9), 1),
            lambda: sim.render_view((0, 0, 5, 5), 20, 20), lambda: sim.render_view((1, 1, 5, 5), 0, 20))]
        r["still_whole_grid_only"] = [expect_code(lambda: sim.tracer_raster(None, 4, 4), EULER_ESTATE), expect_code(lambda: sim.edit_box(ea.EDIT_FILL, (2, 2, 4, 4)), EULER_ESTATE),
                                      expect_code(lambda: sim.add_tracers(np.array([[5.5, 5.5]], np.float32)), EULER_ESTATE)]
        r["works_afterwards"] = bool(sim.overview(4, 4)["cells"].sum() == (X - 2) * (Y - 2))
        every = [None] * world
        dist.all_gather_object(every, r)
        out["refusals"] = every

    if rank == 0:
        print(json.dumps(out))
    dist.barrier()
    dist.destroy_process_group()


def _check_flags(sim, box):
    px = np.zeros((2, 2), ea.FLOW_DTYPE)
    rc = sim.L.euler_flow_raster(sim.h, *box, 2, 2, 8, px.ctypes.data, px.nbytes)
    if rc:
        raise ea.EulerError(rc, sim.L.euler_last_error().decode())


if __name__ == "__main__":
    main()
