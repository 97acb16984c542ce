#!/usr/bin/env python3
"""What the passive tracers (euler_tracers_add, docs/tracers.md) cost in the marker advection's kernel class, per substep, on one GPU.

For each scene ONE process measures the time of the `marker_advect` profile class per substep (a HIP event pair around each of its launches) under
  (none)      no tracers: the launches of a handle that never heard of them,
  (lattice N) N = 2^16, 2^20, 2^22 tracers on a lattice in the water, in the lattice's order (cell x outer: neighbours in the array are neighbours in space),
  (shuffled N) the same positions in a random order (a wave's 64 tracers lie anywhere in the water),
  (row-major) no tracers and EULER_OPT_MARKERS_ROWMAJOR = 1: the fluid's markers through the row-major kernels - the same walk over the same row-major fields
              as a tracer's, so that time per tracer stands next to time per marker.
After the warm-up frames the process walks its configurations --blocks times (alternating blocks: slow drifts of the scene and the clocks hit every
configuration alike), each time one untimed frame and --frames timed ones; the tracers are placed afresh from the water as it stands.  Reported: the median and
the range over the blocks, the time a configuration ADDS to (none) of the same process per substep, and that per tracer; for (row-major) the class time per marker.
Prints a markdown table and one JSON line.

  python tools/tracers_cost.py
  python tools/tracers_cost.py --scenes 4096:dam_break:20 --blocks 2
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLS = "marker_advect"
COUNTS = (1 << 16, 1 << 20, 1 << 22)


def water_points(s, ea, np, n):
    """n positions on a lattice in the water as it stands: the centres of n wet interior cells, evenly spread over them, cell x outer"""
    wet = (s.get(ea.F_COUNT) > 0) & (s.get(ea.F_SOLID) == 0) & (s.get(ea.F_SINK) == 0)
    wet[0, :] = wet[-1, :] = wet[:, 0] = wet[:, -1] = False
    cells = np.argwhere(wet.T)      # (x, y), x outer
    k = 1
    while len(cells) * k * k < n:      # fewer wet cells than tracers: a k x k lattice per cell
        k *= 2
    pick = cells[np.linspace(0, len(cells) - 1, -(-n // (k * k))).astype(np.int64)]
    off = (np.arange(k, dtype=np.float32) + np.float32(0.5)) / np.float32(k)
    x = (pick[:, 0, None, None].astype(np.float32) + off[None, :, None]) + np.zeros((1, 1, k), np.float32)
    y = (pick[:, 1, None, None].astype(np.float32) + off[None, None, :]) + np.zeros((1, k, 1), np.float32)
    return np.stack([x.reshape(-1), y.reshape(-1)], 1)[:n]


def worker(args):
    sys.path.insert(0, ROOT)
    import numpy as np
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
    configs = ["none"] + ["lattice %d" % n for n in COUNTS] + ["shuffled %d" % n for n in COUNTS] + ["row-major"]
    out = {c: [] for c in configs}
    rng = np.random.default_rng(1)
    markers, live = [], {}
    for _ in range(args.blocks):
        for c in configs:
            s.clear_tracers()
            s.set_option(ea.OPT_MARKERS_ROWMAJOR, int(c == "row-major"))
            if c not in ("none", "row-major"):
                xy = water_points(s, ea, np, int(c.split()[1]))
                s.add_tracers(xy[rng.permutation(len(xy))] if c.startswith("shuffled") else xy)
            s.step()      # untimed: the first frame under a configuration
            s.profile_enable([CLS])
            s.profile_reset()
            nsub = 0
            for _ in range(args.frames):
                s.step()
                nsub += s.stats().last_substeps
            ms = s.profile().get(CLS, (0.0, 0))[0]
            s.L.euler_profile_enable(s.h, 0)
            out[c].append(ms / max(nsub, 1))
            if c == "row-major":
                markers.append(int(s.stats().n_markers))
            elif c != "none":
                live[c] = int(((s.tracers()["flags"] & ea.TRACER_RETIRED) == 0).sum())
    s.set_option(ea.OPT_MARKERS_ROWMAJOR, 0)
    print(json.dumps({"ms_per_substep": out, "markers": markers, "live": live, "device": s.device_name()}))
    s.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="4096:dam_break:20,8192:half_tank:3", help="size:workload:frames stepped before anything is measured")
    ap.add_argument("--blocks", type=int, default=3, help="passes over the configurations")
    ap.add_argument("--frames", type=int, default=3, help="timed frames per block")
    ap.add_argument("--max-iterations", type=int, default=20)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--scene", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    res = {"blocks": args.blocks, "frames": args.frames, "rows": []}
    print("| scene | configuration | marker_advect ms per substep: median (min - max) | added to (none) | per tracer / per marker |")
    print("|---|---|---|---|---|")
    for scene in args.scenes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--scene", scene, "--blocks", str(args.blocks), "--frames", str(args.frames),
               "--max-iterations", str(args.max_iterations)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
        if r.returncode != 0:      # a worker that failed ends the run: nothing more is started on the GPU
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            return 1
        w = json.loads(r.stdout.strip().splitlines()[-1])
        res["device"] = w["device"]
        got = w["ms_per_substep"]
        med = {c: statistics.median(v) for c, v in got.items()}
        name = scene.rsplit(":", 1)[0].replace(":", "^2 ")
        for c, v in got.items():
            row = {"scene": scene, "config": c, "median_ms": med[c], "min_ms": min(v), "max_ms": max(v)}
            added, per = "", ""
            if c == "row-major":
                n = statistics.median(w["markers"])
                row.update(markers=n, ns_per_marker=1e6 * med[c] / n)
                per = "%.3f ns per marker (%d markers)" % (row["ns_per_marker"], n)
            elif c != "none":
                n = int(c.split()[1])
                row.update(added_ms=med[c] - med["none"], ns_per_tracer=1e6 * (med[c] - med["none"]) / n, live_at_end=w["live"][c])
                added = "%+.4f ms" % row["added_ms"]
                per = "%.3f ns per tracer (%d of them live at the end)" % (row["ns_per_tracer"], w["live"][c])
            res["rows"].append(row)
            print("| %s | %s | %.4f (%.4f - %.4f) | %s | %s |" % (name, c, med[c], min(v), max(v), added, per))
    print()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
