#!/usr/bin/env python3
"""What the marker density control (euler_set_reseed, docs/reseed.md) costs per substep in the kernel classes its launches belong to, on one GPU.

For each scene the time per substep of the `marker_bin`, `marker_compact`, `sources` and `select` profile classes (a HIP event pair around each of their
launches: the refresh with the pass behind it, and the source stage) under
  (a) a build of the parent commit (--parent-root: a checkout of it with its library built; without it the row is left out),
  (b) this build with the pass off - the launches of (a) -,
  (c) the pass on where it finds nothing to do: thin_above = 254 and filling (the totals are printed: they should be all but zero),
  (d) the pass on with crowding: thin_above = 5 (water seeded four to a cell exceeds it within frames), filling, max_cells at its maximum of 1 << 20.
The method is tools/bodies_cost.py's: a library is loaded once per process, so a worker process measures ONE configuration of ONE library on ONE scene; after
the warm-up frames it runs --blocks blocks of one untimed frame and --frames timed ones.  The workers run in turn (--rounds), each under its own time limit; a
worker that fails ends the run.  Reported: the median and the range over all blocks of all rounds; for (c) and (d) the added time over (b) per substep and as
a share of a substep's wall time; for (d) also the cells thinned and the markers removed per substep, the marker bytes the pass streams (the claim and the
ballot pass read the array once each: 16 bytes per marker) and that figure against the added time as a rate - a LOWER bound of the two passes' own rate,
since the added time also holds the cell pass, three selects, the compaction and the hole kernels - next to the copy ceiling the same run measures with
euler_measure_copy_bandwidth.
The condition: (b) is not slower than (a) by more than the spread of (a)'s own blocks; the tool ends with status 2 where it is not met.
The added times are differences of medians of separate worker processes: read them against the ranges the table prints.
Prints a markdown table and one JSON line.

  python tools/reseed_cost.py --parent-root /path/to/parent/checkout
  python tools/reseed_cost.py --scenes 4096:dam_break:20 --rounds 1
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("marker_bin", "marker_compact", "sources", "select")
NAMES = {"a": "(a) parent commit", "b": "(b) pass off", "c": "(c) on, nothing to do", "d": "(d) on, thin_above = 5"}
RECORDS = {"c": dict(thin_above=254, fill_holes=True), "d": dict(thin_above=5, fill_holes=True, max_cells=1 << 20)}


def worker(args):
    sys.path.insert(0, args.worker)
    import euler_amd as ea
    from euler_amd import scenarios
    size, workload, warmup = args.scene.split(":")
    size, warmup = int(size), int(warmup)
    c = args.config
    s = ea.Simulation(size, size, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=args.max_iterations)
    if workload == "half_tank":
        s.load_half_tank()
    else:
        s.load_text(getattr(scenarios, workload)(), upscale=True)
    for _ in range(warmup):
        s.step()
    if c in RECORDS:
        s.set_reseed(**RECORDS[c])
    out = {k: [] for k in CLASSES + ("substep_ms", "thinned_per_substep", "removed_per_substep", "added_per_substep", "markers")}
    for _ in range(args.blocks):
        s.step()      # untimed: the first frame of a block
        before = {k: int(s.reseed()[1][k]) for k in ("removed", "added", "cells_thinned")} if c in RECORDS else None
        s.profile_enable(list(CLASSES))
        s.profile_reset()
        nsub = 0
        t0 = time.perf_counter()
        for _ in range(args.frames):
            s.step()
            nsub += s.stats().last_substeps
        wall = time.perf_counter() - t0
        prof = s.profile()
        s.L.euler_profile_enable(s.h, 0)
        for k in CLASSES:
            out[k].append(prof.get(k, (0.0, 0))[0] / max(nsub, 1))
        out["substep_ms"].append(1e3 * wall / max(nsub, 1))
        out["markers"].append(int(s.stats().n_markers))
        if before is not None:
            now = s.reseed()[1]
            out["thinned_per_substep"].append((int(now["cells_thinned"]) - before["cells_thinned"]) / max(nsub, 1))
            out["removed_per_substep"].append((int(now["removed"]) - before["removed"]) / max(nsub, 1))
            out["added_per_substep"].append((int(now["added"]) - before["added"]) / max(nsub, 1))
    info = {"copy_gbs": s.copy_bandwidth(1 << 30, 10)} if c == "d" else {}
    print(json.dumps({"ms_per_substep": out, "info": info, "device": s.device_name()}))
    s.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="8192:half_tank:3,4096:dam_break:20", help="size:workload:frames stepped before anything is measured")
    ap.add_argument("--parent-root", default="", help="a checkout of the parent commit with its library built: row (a)")
    ap.add_argument("--rounds", type=int, default=2, help="passes over the workers per scene")
    ap.add_argument("--blocks", type=int, default=3, help="blocks per worker")
    ap.add_argument("--frames", type=int, default=4, help="timed frames per block")
    ap.add_argument("--max-iterations", type=int, default=20)
    ap.add_argument("--worker-timeout", type=int, default=240, help="seconds a worker may take")
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--scene", default="", help=argparse.SUPPRESS)
    ap.add_argument("--config", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    res = {"rounds": args.rounds, "blocks": args.blocks, "frames": args.frames, "rows": []}
    failed = False
    print("| scene | configuration | marker_bin | marker_compact | sources | select | the four: median (min - max) ms per substep | added over (b) | share of a substep here | cells thinned / markers removed / added per substep | marker bytes streamed | rate, copy ceiling |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    order = ("a", "b", "c", "d")
    keys = CLASSES + ("substep_ms", "thinned_per_substep", "removed_per_substep", "added_per_substep", "markers")
    for scene in args.scenes.split(","):
        got, info = {c: {k: [] for k in keys} for c in order}, {}
        for _ in range(args.rounds):
            for root, c in ((args.parent_root, "a"), (ROOT, "b"), (ROOT, "c"), (ROOT, "d")):
                if not root:
                    continue
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", root, "--scene", scene, "--config", c, "--blocks", str(args.blocks),
                       "--frames", str(args.frames), "--max-iterations", str(args.max_iterations)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.worker_timeout)
                except subprocess.TimeoutExpired:      # a worker at its time limit ends the run: nothing more is started on the GPU
                    sys.stderr.write("worker %s on %s ran into its time limit of %d s\n" % (c, scene, args.worker_timeout))
                    return 1
                if r.returncode != 0:      # ... and so does one that failed
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    return 1
                w = json.loads(r.stdout.strip().splitlines()[-1])
                res["device"] = w["device"]
                info.update(w["info"])
                for k, x in w["ms_per_substep"].items():
                    got[c][k] += x
        total = {c: [sum(t) for t in zip(*(got[c][k] for k in CLASSES))] for c in order if got[c][CLASSES[0]]}
        med = {c: statistics.median(v) for c, v in total.items()}
        label = scene.rsplit(":", 1)[0].replace(":", "^2 ")
        for c in order:
            if c not in med:
                continue
            v = total[c]
            cells = ["%.4f" % statistics.median(got[c][k]) for k in CLASSES]
            row = {"scene": scene, "config": c, "median_ms": med[c], "min_ms": min(v), "max_ms": max(v), "classes": dict(zip(CLASSES, (statistics.median(got[c][k]) for k in CLASSES)))}
            tail = [""] * 5
            if c in RECORDS and "b" in med:
                added = med[c] - med["b"]
                sub = statistics.median(got[c]["substep_ms"])
                work = [statistics.mean(got[c][k]) for k in ("thinned_per_substep", "removed_per_substep", "added_per_substep")]
                row.update(added_ms=added, substep_ms=sub, thinned_per_substep=work[0], removed_per_substep=work[1], added_per_substep=work[2])
                tail = ["%.4f ms" % added, "%.1f %% of %.2f ms" % (100 * added / sub, sub), "%.0f / %.0f / %.0f" % tuple(work), "", ""]
                if c == "d":
                    nbytes = 16 * statistics.median(got[c]["markers"])
                    gbs = nbytes / max(added, 1e-9) / 1e6
                    row.update(stream_bytes=nbytes, gbs=gbs, copy_gbs=info.get("copy_gbs", 0.0))
                    tail[3:] = ["%.0f MB" % (nbytes / 1e6), ">= %.0f GB/s, %.0f GB/s" % (gbs, info.get("copy_gbs", 0.0))]
            res["rows"].append(row)
            print("| %s | %s | %s | %.4f (%.4f - %.4f) | %s |" % (label, NAMES[c], " | ".join(cells), med[c], min(v), max(v), " | ".join(tail)))
        if "a" in med:
            spread = max(total["a"]) - min(total["a"])
            ok = med["b"] - med["a"] <= spread
            failed = failed or not ok
            res["rows"].append({"scene": scene, "b_minus_a_ms": med["b"] - med["a"], "spread_a_ms": spread, "condition_met": ok})
            print("| %s | (b) - (a) = %.4f ms; spread of (a) = %.4f ms: condition %s | | | | | | | | | | |" % (label, med["b"] - med["a"], spread, "met" if ok else "NOT met"))
    print()
    print(json.dumps(res))
    return 2 if failed else 0      # (a condition that is not met is the tool's failure, after everything has been printed)


if __name__ == "__main__":
    sys.exit(main())
