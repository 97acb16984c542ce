#!/usr/bin/env python3
"""What the moving bodies (euler_set_bodies, docs/bodies.md) cost per substep in the kernel classes their launches belong to, on one GPU.

For each scene the time per substep of the `marker_advect`, `build_system` and `velocity_update` profile classes (a HIP event pair around each of their
launches: the marker stage, and the two passes of the projection around its solve - the bodies' face launches stand with the assembly) under
  (a) a build of the parent commit (--parent-root: a checkout of it with its library built; without it the row is left out),
  (b) this build without bodies - the launches of (a) -,
  (c) this build with one piston, 8 cells thick and a quarter of the grid high, that moves through the water at 10 cells per second: about one unit shift
      per frame, the wall velocity on its faces in every substep.
The method is tools/heat_cost.py's: a library is loaded once per process, so a worker process measures ONE library on ONE scene; after the warm-up frames
it walks its configurations --blocks times, each time one untimed frame and --frames timed ones.  The parent's worker, this build's with (b) and this
build's with (c) run in turn (--rounds), each under its own time limit; a worker that fails ends the run.  Reported: the median and the range over all
blocks of all rounds; for (c) the added time over (b) per substep and per unit shift, the marker bytes one push pass streams (8 bytes per marker, read
once; the few pushed markers are written back), that figure against the added time per shift as a rate - a LOWER bound of the push pass's own rate, since
the added time also holds the strips' and the rectangle's cell passes and the full forms the next stages run behind a mask change - and the rate as a share
of the copy ceiling the same run measures with euler_measure_copy_bandwidth.
The condition: (b) is not slower than (a) by more than the spread of (a)'s own blocks; the tool ends with status 2 where it is not met.
The added time of (c) is a difference of medians of separate worker processes: read it against the ranges of rows (b) and (c), which the table prints.
Prints a markdown table and one JSON line.

  python tools/bodies_cost.py --parent-root /path/to/parent/checkout
  python tools/bodies_cost.py --scenes 4096:dam_break:20 --rounds 1
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("marker_advect", "build_system", "velocity_update")
NAMES = {"a": "(a) parent commit", "b": "(b) no bodies", "c": "(c) a piston at 10 cells / s"}


def worker(args):
    sys.path.insert(0, args.worker)
    import euler_amd as ea
    from euler_amd import scenarios
    size, workload, warmup = args.scene.split(":")
    size, warmup = int(size), int(warmup)
    s = ea.Simulation(size, size, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=args.max_iterations)
    if workload == "half_tank":
        s.load_half_tank()
    else:
        s.load_text(getattr(scenarios, workload)(), upscale=True)
    for _ in range(warmup):
        s.step()
    out = {c: {k: [] for k in CLASSES + ("substep_ms", "shifts_per_substep")} for c in args.configs}
    info = {}
    for blk in range(args.blocks):
        for c in args.configs:
            if c == "c":      # every block starts the piston afresh, a little further on, at the handle's present clock
                s.clear_bodies()
                t = s.time
                x0 = size // 8 + 40 * blk
                s.set_bodies([ea.body((8, size // 4), (x0 - 10.0 * t, size // 4 if workload != "half_tank" else 2), (10.0, 0.0))])
            s.step()      # untimed: the first frame under a configuration
            s.profile_enable(list(CLASSES))
            s.profile_reset()
            nsub = shifts = 0
            t0 = time.perf_counter()
            for _ in range(args.frames):
                before = int(s.bodies()[1]["ox"][0]) if c == "c" else 0
                s.step()
                nsub += s.stats().last_substeps
                shifts += (int(s.bodies()[1]["ox"][0]) - before) if c == "c" else 0
            wall = time.perf_counter() - t0
            prof = s.profile()
            s.L.euler_profile_enable(s.h, 0)
            for k in CLASSES:
                out[c][k].append(prof.get(k, (0.0, 0))[0] / max(nsub, 1))
            out[c]["substep_ms"].append(1e3 * wall / max(nsub, 1))
            out[c]["shifts_per_substep"].append(shifts / max(nsub, 1))
    if "a" not in args.configs:
        info["markers"] = int(s.stats().n_markers)
        info["copy_gbs"] = s.copy_bandwidth(1 << 30, 10)
    print(json.dumps({"ms_per_substep": out, "info": info, "device": s.device_name()}))
    s.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="8192:half_tank:3,4096:dam_break:20", help="size:workload:frames stepped before anything is measured")
    ap.add_argument("--parent-root", default="", help="a checkout of the parent commit with its library built: row (a)")
    ap.add_argument("--rounds", type=int, default=2, help="parent / new worker pairs per scene")
    ap.add_argument("--blocks", type=int, default=3, help="passes over its configurations per worker")
    ap.add_argument("--frames", type=int, default=4, help="timed frames per block")
    ap.add_argument("--max-iterations", type=int, default=20)
    ap.add_argument("--worker-timeout", type=int, default=240, help="seconds a worker may take")
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--scene", default="", help=argparse.SUPPRESS)
    ap.add_argument("--configs", default="", type=lambda t: t.split(","), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    res = {"rounds": args.rounds, "blocks": args.blocks, "frames": args.frames, "rows": []}
    failed = False
    print("| scene | configuration | marker_advect | build_system | velocity_update | the three: median (min - max) ms per substep | added over no bodies | shifts per substep | added per shift | marker bytes of a push | rate against the copy ceiling | share of a substep here |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    order = ("a", "b", "c")
    for scene in args.scenes.split(","):
        got, info = {c: {k: [] for k in CLASSES + ("substep_ms", "shifts_per_substep")} for c in order}, {}
        for _ in range(args.rounds):
            for root, configs in ((args.parent_root, "a"), (ROOT, "b"), (ROOT, "c")):
                if not root:
                    continue
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", root, "--scene", scene, "--configs", configs, "--blocks", str(args.blocks),
                       "--frames", str(args.frames), "--max-iterations", str(args.max_iterations)]
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.worker_timeout)
                except subprocess.TimeoutExpired:      # a worker at its time limit ends the run: nothing more is started on the GPU
                    sys.stderr.write("worker %s on %s ran into its time limit of %d s\n" % (configs, scene, args.worker_timeout))
                    return 1
                if r.returncode != 0:      # ... and so does one that failed
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    return 1
                w = json.loads(r.stdout.strip().splitlines()[-1])
                res["device"] = w["device"]
                info.update(w["info"])
                for c, v in w["ms_per_substep"].items():
                    for k, x in v.items():
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
            tail = [""] * 6
            if c == "c" and "b" in med:
                added = med[c] - med["b"]
                sps = statistics.mean(got[c]["shifts_per_substep"])
                per_shift = added / sps if sps > 0 else float("nan")
                nbytes = 8 * info.get("markers", 0)
                gbs = nbytes / max(per_shift, 1e-9) / 1e6 if sps > 0 else 0.0
                sub = statistics.median(got[c]["substep_ms"])
                row.update(added_ms=added, shifts_per_substep=sps, added_per_shift_ms=per_shift, push_bytes=nbytes, gbs=gbs, copy_gbs=info.get("copy_gbs", 0.0), substep_ms=sub)
                tail = ["%.4f ms" % added, "%.2f" % sps, "%.4f ms" % per_shift, "%.0f MB" % (nbytes / 1e6),
                        ">= %.0f GB/s of %.0f: %.0f %%" % (gbs, info.get("copy_gbs", 0.0), 100 * gbs / max(info.get("copy_gbs", 0.0), 1e-9)), "%.1f %% of %.2f ms" % (100 * added / sub, sub)]
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
