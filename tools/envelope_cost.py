#!/usr/bin/env python3
"""What the run-long envelopes (euler_set_envelope, docs/envelope.md) cost per substep in the kernel classes their launches belong to, on one GPU.

For each scene the time per substep of the `misc`, `velocity_update` and `update_pr` profile classes (a HIP event pair around each of their launches: the
envelope's two passes run as `misc`; what eu_pressure_current owes with the pressure channel on - the clamp and the last p += alpha s - as the other two) under
  (a) a build of the parent commit (--parent-root: a checkout of it with its library built; without it the row is left out),
  (b) this build with the envelope never switched on - the launches of (a) -,
  (c) arrival + wet, (d) speed, (e) pressure, (f) all four channels.
The method is tools/bodies_cost.py's: a library is loaded once per process, so a worker process measures ONE library on ONE scene; after the warm-up frames
it walks its configurations --blocks times, each time one untimed frame and --frames timed ones.  The parent's worker and this build's run in turn
(--rounds), each under its own time limit; a worker that fails ends the run.  Reported: the median and the range over all blocks of all rounds; for (c) - (f)
the added time over (b) per substep, the algorithmic bytes of the passes per substep - bytes per wet cell as docs/envelope.md derives them from the kernels,
times the fluid cells of the scene -, that figure against the added time as a rate, and the rate as a share of the copy ceiling the same run measures with
euler_measure_copy_bandwidth.  The bytes are a LOWER bound of the traffic (the passes also read the masks of the dry cells of a wet tile, and the pressure
pass's bytes leave eu_pressure_current's passes out), so the rate is a lower bound too.
The condition: (b) is not slower than (a) by more than the spread of (a)'s own blocks; the tool ends with status 2 where it is not met.
An added time is a difference of medians of blocks of one worker: read it against the ranges of the rows it is formed from, which the table prints.
Prints a markdown table and one JSON line.

  python tools/envelope_cost.py --parent-root /path/to/parent/checkout
  python tools/envelope_cost.py --scenes 4096:dam_break:20 --rounds 1
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("misc", "velocity_update", "update_pr")
NAMES = {"a": "(a) parent commit", "b": "(b) never switched on", "c": "(c) arrival + wet", "d": "(d) speed", "e": "(e) pressure", "f": "(f) all"}
CHANNELS = {"b": 0, "c": 3, "d": 4, "e": 8, "f": 15}
# bytes per wet cell and substep, from k_envelope.hip (docs/envelope.md "Bytes"): the masks 2; arrival 4 read; wet 4 + 4; speed u, v 8 and the plane 4 read (its
# store only where the peak rises); pressure: the masks 2, p 8, the plane 4 read
BYTES = {"c": 2 + 4 + 8, "d": 2 + 8 + 4, "e": 2 + 8 + 4, "f": 2 + 4 + 8 + 8 + 4 + 2 + 8 + 4}


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
    out = {c: {k: [] for k in CLASSES + ("substep_ms",)} for c in args.configs}
    info = {}
    for blk in range(args.blocks):
        for c in args.configs:
            if c != "a":
                s.set_envelope(CHANNELS[c])      # (the parent has no such call; (b) clears what the configuration before it set)
            s.step()      # untimed: the first frame under a configuration
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
                out[c][k].append(prof.get(k, (0.0, 0))[0] / max(nsub, 1))
            out[c]["substep_ms"].append(1e3 * wall / max(nsub, 1))
    if "a" not in args.configs:
        s.set_envelope(0)
        info["fluid_cells"] = int(s.stats().fluid_cells)
        info["copy_gbs"] = s.copy_bandwidth(1 << 30, 10)
    print(json.dumps({"ms_per_substep": out, "info": info, "device": s.device_name()}))
    s.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="8192:half_tank:3,4096:dam_break:20", help="size:workload:frames stepped before anything is measured")
    ap.add_argument("--parent-root", default="", help="a checkout of the parent commit with its library built: row (a)")
    ap.add_argument("--rounds", type=int, default=2, help="parent / new worker pairs per scene")
    ap.add_argument("--blocks", type=int, default=3, help="passes over its configurations per worker")
    ap.add_argument("--frames", type=int, default=3, help="timed frames per block")
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
    print("| scene | configuration | misc | velocity_update | update_pr | the three: median (min - max) ms per substep | added over never switched on | bytes per wet cell | bytes per substep | rate against the copy ceiling | share of a substep here |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    order = ("a", "b", "c", "d", "e", "f")
    for scene in args.scenes.split(","):
        got, info = {c: {k: [] for k in CLASSES + ("substep_ms",)} for c in order}, {}
        for _ in range(args.rounds):
            for root, configs in ((args.parent_root, "a"), (ROOT, "b,c,d,e,f")):
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
            tail = [""] * 5
            if c in BYTES and "b" in med:
                added = med[c] - med["b"]
                nbytes = BYTES[c] * info.get("fluid_cells", 0)
                gbs = nbytes / max(added, 1e-9) / 1e6
                sub = statistics.median(got[c]["substep_ms"])
                noise = max(max(total["b"]) - min(total["b"]), max(v) - min(v))
                row.update(added_ms=added, bytes_per_cell=BYTES[c], bytes=nbytes, gbs=gbs, copy_gbs=info.get("copy_gbs", 0.0), substep_ms=sub, range_ms=noise)
                tail = ["%.4f ms%s" % (added, " (within the rows' range of %.4f)" % noise if abs(added) <= noise else ""), "%d" % BYTES[c], "%.0f MB" % (nbytes / 1e6),
                        ">= %.0f GB/s of %.0f: %.0f %%" % (gbs, info.get("copy_gbs", 0.0), 100 * gbs / max(info.get("copy_gbs", 0.0), 1e-9)), "%.1f %% of %.2f ms" % (100 * added / sub, sub)]
            res["rows"].append(row)
            print("| %s | %s | %s | %.4f (%.4f - %.4f) | %s |" % (label, NAMES[c], " | ".join(cells), med[c], min(v), max(v), " | ".join(tail)))
        if "a" in med:
            spread = max(total["a"]) - min(total["a"])
            ok = med["b"] - med["a"] <= spread
            failed = failed or not ok
            res["rows"].append({"scene": scene, "b_minus_a_ms": med["b"] - med["a"], "spread_a_ms": spread, "condition_met": ok})
            print("| %s | (b) - (a) = %.4f ms; spread of (a) = %.4f ms: condition %s | | | | | | | | | |" % (label, med["b"] - med["a"], spread, "met" if ok else "NOT met"))
    print()
    print(json.dumps(res))
    return 2 if failed else 0      # (a condition that is not met is the tool's failure, after everything has been printed)


if __name__ == "__main__":
    sys.exit(main())
