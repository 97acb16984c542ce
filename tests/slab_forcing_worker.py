"""Worker for tests/test_slab_forcing_heat.py: N gloo ranks sharing cuda:0 (tests/ranks.py), every rank one row slab of the job with forcing and temperature on, and
a whole-grid handle of the same scene in the same process as the thing to match - its forcing and heat are pinned bit for bit against tests/forcing_ref.py and
tests/heat_ref.py (test_gpu_forcing.py, test_gpu_heat.py), so agreement with it is agreement with the restatements.  Rank 0 prints one JSON line.

argv: X Y workload mode [bands=..] [kappa=..] [beta=..] [rainbow] [path=..]; mode = teacher | free | props | disagree | refuse."""
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
from euler_amd import scenarios
from euler_amd.slab import SLAB_LOCAL, TorchComm
from slab_observers_worker import boxes_of, rasters_of

U32 = np.uint32
EULER_EINVAL, EULER_ESTATE = -1, -5


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return bool(a.shape == b.shape and np.array_equal(a.view(U32 if a.dtype == np.float32 else a.dtype), b.view(U32 if b.dtype == np.float32 else b.dtype)))


def force_boxes(X, Y):
    """seven boxes: overlapping, repeated, across rows 63|64 and 127|128, one cell, one in cells that stay dry, one touching X - 2"""
    return [((10, 50, 60, 70), (4.0, -1.0)), ((30, 60, 80, 100), (-2.5, 3.0)), ((10, 50, 60, 70), (4.0, -1.0)), ((20, 120, 50, 135), (1.5, 2.0)),
            ((40, 40, 40, 40), (-6.0, 6.0)), ((X - 20, 100, X - 12, 110), (3.0, 3.0)), ((X - 12, 2, X - 2, 20), (-1.0, 0.5))]


def heat_boxes(X, Y):
    """FIX and RATE boxes across the slab boundaries, and one inside the lowest band only"""
    return [(ea.HEAT_FIX, 8.0, (15, 55, 45, 70)), (ea.HEAT_RATE, 3.0, (25, 120, 60, 132)), (ea.HEAT_FIX, -2.0, (5, 5, 30, 20)), (ea.HEAT_RATE, -1.5, (50, 60, 70, 66))]


GRAVITY, SHAKE = (2.0, -9.0), (0.75, 0.5, 1.5, 0.3)
AMBIENT, SOURCE_T = 1.0, 5.0


def drive(sim, X, Y, kappa, beta, boxes=True, rate=True):
    hb = heat_boxes(X, Y) if boxes else ()
    sim.set_forcing(GRAVITY, SHAKE, force_boxes(X, Y) if boxes else ())
    sim.set_heat(AMBIENT, beta, kappa, SOURCE_T, [b for b in hb if rate or b[0] == ea.HEAT_FIX])


def load(sim, workload):
    if workload == "half_tank":
        sim.load_half_tank()
    else:
        sim.load_text(getattr(scenarios, workload)(), upscale=True)
    return sim


def gather(obj, world):
    agg = [None] * world
    dist.all_gather_object(agg, obj)
    return agg


def main():
    X, Y, workload, mode = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    extra = sys.argv[5:]
    opt = dict(a.split("=", 1) for a in extra if "=" in a)
    kappa, beta = float(opt.get("kappa", 0.05)), float(opt.get("beta", 0.02))
    rainbow = "rainbow" in extra
    dist.init_process_group("gloo")
    torch.cuda.set_device(0)
    rank, world = dist.get_rank(), dist.get_world_size()
    slab = (rank, world)
    if "bands" in opt:
        lo, hi = opt["bands"].split(",")[rank].split("-")
        slab = (rank, world, int(lo), int(hi))
    kw = dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, rainbow=rainbow)
    make_ref = lambda: ea.Simulation(X, Y, **kw)
    sim = ea.Simulation(X, Y, slab=slab, **kw)
    comm = TorchComm(sim, SLAB_LOCAL)
    out = {"world": world}
    lo, hi = sim.slab_rows()
    rows = gather([lo, hi], world)
    out["rows"] = rows
    edges = [r[0] for r in rows[1:]]      # the first row of every rank but the lowest: the slab boundaries

    def own(a):
        return a[lo:hi]

    def compare(ref, fields=True):
        """bit for bit over the own rows: T, utmp, vtmp, both count grids, every marker at its key"""
        d = {"T": same_bits(sim.temperature, own(ref.temperature)),
             "count": same_bits(sim.get(ea.F_COUNT), own(ref.get(ea.F_COUNT))), "prev_count": same_bits(sim.get(ea.F_PREV_COUNT), own(ref.get(ea.F_PREV_COUNT)))}
        if fields:
            d["utmp"] = same_bits(sim.get(ea.F_UTMP), own(ref.get(ea.F_UTMP)))
            d["vtmp"] = same_bits(sim.get(ea.F_VTMP), own(ref.get(ea.F_VTMP)))
        m, k, rm = sim.get(ea.F_MARKERS), sim.get(ea.F_MARKER_KEYS), ref.get(ea.F_MARKERS)
        d["markers"] = bool(len(m) == len(k) and (len(k) == 0 or int(k.max()) < len(rm)) and same_bits(m, rm[k]))
        return d

    def water_across(ref):
        c = ref.get(ea.F_COUNT)
        return bool(all((c[e - 1] > 0).any() and (c[e] > 0).any() for e in edges))

    def staged_substep(ref, teacher, log):
        """one substep stage by stage on both sides, compared behind SOURCES and ADVECT_VELOCITY (with the dye: as a whole - euler_stage refuses slabs with the dye -,
        compared behind it: T and the counts are the stages' last words, utmp / vtmp what ADVECT_VELOCITY left)"""
        dt_r, dt_s = ref.timestep(0.1), sim.timestep(0.1)
        rec = {"dt": [dt_r, dt_s]}
        if rainbow:
            ref.substep(dt_r)
            sim.substep(dt_s)
            rec["substep"] = compare(ref)      # (the projection reads utmp / vtmp and leaves them: behind the substep they are what ADVECT_VELOCITY left)
        else:
            for st in range(6):
                ref.stage(st, dt_r)
                sim.stage(st, dt_s)
                if st == ea.STAGE_SOURCES:
                    rec["sources"] = compare(ref)
                if st == ea.STAGE_ADVECT_VELOCITY:
                    rec["advect"] = compare(ref)
            t = ref.time + float(np.float32(dt_r))      # (a stage is not a substep: the caller advances both clocks alike)
            ref.time = t
            sim.time = t
        rec["time"] = [ref.time, sim.time]
        if teacher:      # the solve's rounding differs between one and several ranks: the slabs go on from the whole-grid handle's own rows
            sim.set(ea.F_U, own(ref.get(ea.F_U)))
            sim.set(ea.F_V, own(ref.get(ea.F_V)))
        log.append(rec)

    if mode == "teacher":
        path = opt["path"]
        first = make_ref()
        load(first, workload)
        drive(first, X, Y, kappa, beta)
        for _ in range(3):
            first.step()
        T0, t0 = first.temperature, first.time
        if rank == 0:
            first.save_state(path)
        dist.barrier()
        first.close()
        ref = make_ref().load_state(path)
        sim.load_state(path)
        for s in (ref, sim):
            drive(s, X, Y, kappa, beta)
            s.time = t0
        ref.temperature = T0
        sim.temperature = own(T0)
        out["T0_spread"] = [float(T0.min()), float(T0.max())]
        log = []
        out["water_first"] = water_across(ref)
        for _ in range(12):
            staged_substep(ref, True, log)
        out["water_last"] = water_across(ref)
        out["substeps"] = log
        # ---- euler_heat_raster behind that state: every rank's bytes are the whole-grid handle's
        ras = []
        for name, box in boxes_of(X, Y):
            for (w, h) in rasters_of(box):
                a, b = sim.heat_raster(w, h, box), ref.heat_raster(w, h, box)
                ras.append([name, w, h, bool(a.tobytes() == b.tobytes()), int(b["water"].sum())])
        out["rasters"] = ras
        # ---- euler_heat_fill: a box across the first boundary, one inside the top rank only; then one more substep, so the ghost rows were current
        top = rows[-1]
        for box, val in (((12, edges[0] - 6, 70, edges[0] + 5), 6.5), ((8, top[0] + 2, 60, min(top[1] - 2, Y - 2)), -3.25)):
            ref.heat_fill(box, val)
            sim.heat_fill(box, val)
        out["fill_T"] = same_bits(sim.temperature, own(ref.temperature))
        out["fill_changed"] = bool((ref.temperature == np.float32(6.5)).any())
        log2 = []
        staged_substep(ref, True, log2)
        out["after_fill"] = log2
        # ---- a load with heat on leaves T = ambient over the whole window, ghost rows included: the next substep is still the whole-grid handle's
        ref.load_state(path)
        sim.load_state(path)
        out["load_leaves_ambient"] = bool((sim.temperature == np.float32(AMBIENT)).all() and (ref.temperature == np.float32(AMBIENT)).all())
        for s in (ref, sim):
            s.time = t0
        log3 = []
        staged_substep(ref, True, log3)
        out["after_load"] = log3
    elif mode == "free":
        ref = load(make_ref(), workload)
        load(sim, workload)
        for s in (ref, sim):
            drive(s, X, Y, kappa, beta, rate=False)      # no RATE box: T obeys the maximum principle
        bound = [min(AMBIENT, SOURCE_T, 8.0, -2.0), max(AMBIENT, SOURCE_T, 8.0, -2.0)]
        frames = []
        for _ in range(10):
            ref.step()
            sim.step()
            sr, ss = ref.stats(), sim.stats()
            d = {}
            for name, fld in (("u", ea.F_U), ("v", ea.F_V), ("p", ea.F_PRESSURE)):
                d["d" + name] = float(np.abs(sim.get(fld) - own(ref.get(fld))).max())
            d["pmax"] = float(np.abs(ref.get(ea.F_PRESSURE)).max())
            T, Tr = sim.temperature, own(ref.temperature)
            d["dT"] = float(np.abs(T - Tr).max())
            d["T_range"] = [float(T.min()), float(T.max())]
            d["T_in_bounds"] = bool(T.min() >= bound[0] and T.max() <= bound[1])
            d["T_moved"] = bool((T != np.float32(AMBIENT)).any())
            d["time"] = [ref.time, sim.time]
            m, k, rm = sim.get(ea.F_MARKERS), sim.get(ea.F_MARKER_KEYS), ref.get(ea.F_MARKERS)
            d["markers_in_rows"] = bool(len(m) == 0 or (np.floor(m[:, 1]).min() >= lo and np.floor(m[:, 1]).max() < hi))
            d["markers_at_keys"] = bool(len(m) == len(k) and (len(k) == 0 or int(k.max()) < len(rm)) and same_bits(m, rm[k]))
            d["count_differ"] = int((sim.get(ea.F_COUNT) != own(ref.get(ea.F_COUNT))).sum())
            flat = np.sort(np.concatenate([np.asarray(x, np.int64) for x in gather(k.tolist(), world)]))
            d["keys_cover_own_count"] = bool(len(flat) == int(ss.n_markers) and np.array_equal(flat, np.arange(len(flat))))
            d["iters"] = [sr.last_pcg_iterations, ss.last_pcg_iterations]
            d["substeps"] = [sr.last_substeps, ss.last_substeps]
            agg = gather(d, world)
            w = dict(agg[0])
            for o in agg[1:]:
                for key in ("du", "dv", "dp", "dT", "count_differ"):
                    w[key] = max(w[key], o[key])
                for key in ("T_in_bounds", "markers_in_rows", "markers_at_keys", "keys_cover_own_count"):
                    w[key] = w[key] and o[key]
                w["T_moved"] = w["T_moved"] or o["T_moved"]
                w["T_range"] = [min(w["T_range"][0], o["T_range"][0]), max(w["T_range"][1], o["T_range"][1])]
                w["time"] = w["time"] + o["time"]
            frames.append(w)
        out["frames"] = frames
        out["T_bound"] = bound
    elif mode == "props":
        # ---- a job that sets the default record before every frame against one that never calls either entry point: the same bits, the same launches
        other = ea.Simulation(X, Y, slab=slab, **kw)
        comm2 = TorchComm(other, SLAB_LOCAL)
        load(sim, workload)
        load(other, workload)
        names = [n for n in ea.profile_class_names()]
        sim.profile_enable(names)
        other.profile_enable(names)
        same, launches = [], []
        for _ in range(4):
            sim.set_forcing()
            sim.profile_reset()
            other.profile_reset()
            sim.step()
            other.step()
            # (the local marker order means nothing - migrants are appended as they arrive -: a marker is compared at its key)
            ka, kb = sim.get(ea.F_MARKER_KEYS), other.get(ea.F_MARKER_KEYS)
            ma, mb = sim.get(ea.F_MARKERS)[np.argsort(ka)], other.get(ea.F_MARKERS)[np.argsort(kb)]
            differ = [f for f in (ea.F_U, ea.F_V, ea.F_UTMP, ea.F_VTMP, ea.F_COUNT, ea.F_PREV_COUNT) if not same_bits(sim.get(f), other.get(f))]
            if not np.array_equal(sim.get(ea.F_PRESSURE).view(np.uint64), other.get(ea.F_PRESSURE).view(np.uint64)):
                differ.append("p")
            if not (np.array_equal(np.sort(ka), np.sort(kb)) and same_bits(ma, mb)):
                differ.append("markers")
            same.append(differ)
            pa, pb = sim.profile(), other.profile()
            launches.append({n: [int(pa.get(n, (0, 0))[1]), int(pb.get(n, (0, 0))[1])] for n in set(pa) | set(pb)})
        out["untouched_same_bits"] = same
        out["untouched_launches"] = launches
        other.close()
        # ---- euler_destroy: slab handles with heat, boxes and the raster's buffers on are created, stepped and destroyed; every call returns EULER_OK (the binding
        # raises otherwise) and each handle counts the same bytes - nothing of a destroyed handle is left for the next (the ledger's own count after
        # eu_mem_free_all is the host program's, tests/c/sanitize_slab_forcing.c)
        cycle = []
        for _ in range(3):
            s3 = ea.Simulation(X, Y, slab=slab, **kw)
            c3 = TorchComm(s3, SLAB_LOCAL)
            load(s3, workload)
            b0 = s3.hbm_bytes()
            drive(s3, X, Y, kappa, beta)
            s3.heat_raster(7, 5)
            s3.step()
            cycle.append([b0, s3.hbm_bytes()])
            s3.close()
            if c3.error:
                raise RuntimeError(c3.error)
        out["life_cycle"] = cycle
        # ---- memory: switching heat on grows the handle by the two halves of the window plus the box buffer; every rank frees everything
        before = sim.hbm_bytes()
        sim.set_heat(AMBIENT, beta, kappa, SOURCE_T, ())
        win = (min(hi + 2, Y) - max(lo - 1, 0))
        out["heat_bytes"] = [sim.hbm_bytes() - before, 2 * 4 * X * win]
        before = sim.hbm_bytes()
        # ---- one heat box and one force box inside the lowest band: the other ranks launch no box kernel (the velocity class: advection + boxes + heat passes)
        sim.set_heat(AMBIENT, 0.0, 0.0, SOURCE_T, [(ea.HEAT_RATE, 1.0, (5, 5, 30, 20))])
        out["box_buffer_bytes"] = sim.hbm_bytes() - before
        sim.set_forcing((0.0, -10.0), None, [((5, 5, 30, 20), (1.0, 0.0))])
        sim.profile_reset()
        sim.stage(ea.STAGE_ADVECT_VELOCITY, 0.01)
        with_boxes = int(sim.profile().get("advect_velocity", (0, 0))[1])
        sim.set_heat(AMBIENT, 0.0, 0.0, SOURCE_T, ())
        sim.set_forcing()
        sim.profile_reset()
        sim.stage(ea.STAGE_ADVECT_VELOCITY, 0.01)
        without = int(sim.profile().get("advect_velocity", (0, 0))[1])
        out["box_launches"] = [with_boxes - without]
    elif mode == "disagree":
        load(sim, workload)
        drive(sim, X, Y, kappa, beta)
        sim.step()
        f0, h0, T0 = sim.forcing(), sim.heat(), sim.temperature
        cases = {}

        def attempt(name, fn):
            code, msg = 0, ""
            try:
                fn()
            except ea.EulerError as e:
                code, msg = e.code, str(e)
            f1, h1 = sim.forcing(), sim.heat()
            kept = bool(f1[0].tobytes() == f0[0].tobytes() and f1[1].tobytes() == f0[1].tobytes() and h1[0].tobytes() == h0[0].tobytes() and
                        h1[1].tobytes() == h0[1].tobytes() and same_bits(sim.temperature, T0))
            cases[name] = [code, msg, kept]

        odd = rank == world - 1
        hb = heat_boxes(X, Y)
        fb = force_boxes(X, Y)
        attempt("beta", lambda: sim.set_heat(AMBIENT, 0.5 if odd else 0.25, kappa, SOURCE_T, hb))
        attempt("box_order", lambda: sim.set_forcing(GRAVITY, SHAKE, fb[::-1] if odd else fb))
        attempt("heat_box_order", lambda: sim.set_heat(AMBIENT, beta, kappa, SOURCE_T, hb[::-1] if odd else hb))
        attempt("invalid", lambda: sim.set_forcing((np.nan if odd else 1.0, -9.0), SHAKE, fb))
        attempt("invalid_heat", lambda: sim.set_heat(AMBIENT, beta, -1.0 if odd else kappa, SOURCE_T, hb))
        attempt("off_on_one_rank", lambda: sim.heat_off() if odd else sim.set_heat(AMBIENT, beta, kappa, SOURCE_T, hb))
        sim.step()      # the job steps on
        out["stepped_on"] = bool(np.isfinite(sim.temperature).all())
        sim.heat_off()      # ... and switching off together works
        try:
            sim.heat()
            out["off_together"] = False
        except ea.EulerError:
            out["off_together"] = True
        sim.step()
        out["cases"] = cases
    elif mode == "refuse":
        load(sim, workload)
        drive(sim, X, Y, kappa, beta)
        ref = {}

        def refused(name, fn):
            try:
                fn()
                ref[name] = [0, ""]
            except ea.EulerError as e:
                ref[name] = [e.code, str(e)]

        refused("save_session", lambda: sim.save_session(opt["path"] + ".%d" % rank))
        refused("load_session", lambda: sim.load_session(opt["path"] + ".none"))
        refused("rk2", lambda: sim.set_option(ea.OPT_ADVECT_RK2, 1))
        refused("maccormack", lambda: sim.set_option(ea.OPT_ADVECT_MACCORMACK, 1))
        sim.step()
        out["refused"] = ref
    if comm.error:
        raise RuntimeError(comm.error)
    # every rank's view, for the properties that differ by rank
    per_rank = gather({k: out[k] for k in ("heat_bytes", "box_buffer_bytes", "life_cycle", "box_launches", "cases", "refused", "rasters", "fill_T", "untouched_same_bits", "untouched_launches",
                                           "load_leaves_ambient", "substeps", "after_fill", "after_load", "stepped_on", "off_together") if k in out}, world)
    sim.close()
    if rank == 0:
        out["per_rank"] = per_rank
        print(json.dumps(out))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
