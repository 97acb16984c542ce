#!/usr/bin/env python3
"""What the temperature (euler_set_heat, docs/heat.md) costs per substep in the kernel classes its launches belong to, on one GPU.

For each scene the time per substep of the `advect_velocity`, `extrapolate` and `sources` profile classes (a HIP event pair around each of their
launches) under
  (a) a build of the parent commit (--parent-root: a checkout of it with its library built; without it the row is left out),
  (b) this build with heat off - the launches of (a) -,
  (c) a passive temperature (beta = 0),
  (d) beta = 0.5, kappa = 0.3 and 16 boxes of 64 x 64 cells in the water, off the tile grid,
  (e) (d) under MacCormack + RK2.
The method is tools/forcing_cost.py's: a library is loaded once per process, so a worker process measures ONE library on ONE scene; after the warm-up
frames it walks its configurations --blocks times, each time one untimed frame and --frames timed ones.  Three kinds of worker run in turn (--rounds):
the parent's with (a), this build's with (b) alone - (a)'s schedule, the same states frame for frame - and this build's with (c), (d), (e).  Reported:
the median and the range over all blocks of all rounds; for (c) - (e) the added time over (b) - (e): over (b) under the same transport, measured in the
same worker as (b2) -, the bytes the heat passes move, computed from the shapes (docs/heat.md), that figure as a share of the copy ceiling the same run
measures with euler_measure_copy_bandwidth, and the added time as a share of a substep of the scene as run here.
The condition: (b) is not slower than (a) by more than the spread of (a)'s own blocks.
Prints a markdown table and one JSON line.

  python tools/heat_cost.py --parent-root /path/to/parent/checkout
  python tools/heat_cost.py --scenes 4096:dam_break:20 --rounds 1
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ("advect_velocity", "extrapolate", "sources")
NAMES = {"a": "(a) parent commit", "b": "(b) heat off", "c": "(c) passive, beta = 0", "d": "(d) beta, kappa, 16 boxes", "b2": "(b2) heat off, MacCormack + RK2",
         "e": "(e) (d) under MacCormack + RK2"}


def boxes_of(size):
    """16 boxes of 64 x 64 cells in the lower left of the grid - water in both scenes -, off the tile grid; every other one a RATE"""
    x, y = size // 8 + 10, size // 4 + 5
    return [(k & 1, 3.0, (x + 90 * (k % 4), y + 90 * (k // 4), x + 90 * (k % 4) + 63, y + 90 * (k // 4) + 63)) for k in range(16)]


def heat_bytes(size, config, fluid):
    """bytes per substep of the heat passes (docs/heat.md "The kernels"): C cells, F of them fluid"""
    C = size * size
    ext = C * (4 + 4 + 3)                                   # T in, T out, prev / cur / source bytes
    adv = C * (1 + 4) + fluid * (4 * 4 + 4 + 8)             # count, T out; per fluid cell four corners of T, their counts, u and v (lines shared with the neighbours)
    if config == "e":
        adv = 2 * adv + fluid * 8                           # forward pass + correction, which reads the forward result and T again
    box = 16 * 64 * 64 * (1 + 8) if config in ("d", "e") else 0
    dif = C * (1 + 4 + 4) if config in ("d", "e") else 0
    buo = C * (2 + 4) + fluid * 2 * 8 if config in ("d", "e") else 0
    return ext + adv + box + dif + buo


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
    for _ in range(args.blocks):
        for c in args.configs:
            if c != "a":
                mc = 1 if c in ("b2", "e") else 0
                s.set_option(ea.OPT_ADVECT_MACCORMACK, mc)
                s.set_option(ea.OPT_ADVECT_RK2, mc)
                if c in ("b", "b2"):
                    s.heat_off()
                else:
                    s.heat_off()      # (every block starts its field afresh: a hot blob in ambient water)
                    s.set_heat(0.0, 0.0 if c == "c" else 0.5, 0.0 if c == "c" else 0.3, 0.0, [] if c == "c" else boxes_of(size))
                    s.heat_fill((size // 8, size // 8, size // 2, size // 3), 5.0)
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
        s.heat_off()
        info["fluid"] = int((s.get(ea.F_COUNT) != 0).sum())
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
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--scene", default="", help=argparse.SUPPRESS)
    ap.add_argument("--configs", default="", type=lambda t: t.split(","), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    res = {"rounds": args.rounds, "blocks": args.blocks, "frames": args.frames, "rows": []}
    print("| scene | configuration | advect_velocity | extrapolate | sources | the three: median (min - max) ms per substep | added over heat off | bytes of the heat passes | share of the copy ceiling | share of a substep here |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    order = ("a", "b", "c", "d", "b2", "e")
    for scene in args.scenes.split(","):
        size = int(scene.split(":")[0])
        got, info = {c: {k: [] for k in CLASSES + ("substep_ms",)} for c in order}, {}
        for _ in range(args.rounds):
            for root, configs in ((args.parent_root, "a"), (ROOT, "b"), (ROOT, "c,d,b2,e")):
                if not root:
                    continue
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", root, "--scene", scene, "--configs", configs, "--blocks", str(args.blocks),
                       "--frames", str(args.frames), "--max-iterations", str(args.max_iterations)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:      # a worker that failed ends the run: nothing more is started on the GPU
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
            tail = ["", "", "", ""]
            base = "b2" if c == "e" else "b"
            if c in ("c", "d", "e") and base in med:
                added = med[c] - med[base]
                nbytes = heat_bytes(size, c, info.get("fluid", 0))
                gbs = nbytes / max(added, 1e-9) / 1e6
                sub = statistics.median(got[c]["substep_ms"])
                row.update(added_ms=added, bytes=nbytes, gbs=gbs, copy_gbs=info.get("copy_gbs", 0.0), substep_ms=sub)
                tail = ["%.4f ms" % added, "%.0f MB" % (nbytes / 1e6), "%.0f GB/s of %.0f: %.0f %%" % (gbs, info.get("copy_gbs", 0.0), 100 * gbs / max(info.get("copy_gbs", 0.0), 1e-9)),
                        "%.1f %% of %.2f ms" % (100 * added / sub, sub)]
            res["rows"].append(row)
            print("| %s | %s | %s | %.4f (%.4f - %.4f) | %s |" % (label, NAMES[c], " | ".join(cells), med[c], min(v), max(v), " | ".join(tail)))
        if "a" in med:
            spread = max(total["a"]) - min(total["a"])
            ok = med["b"] - med["a"] <= spread
            res["rows"].append({"scene": scene, "b_minus_a_ms": med["b"] - med["a"], "spread_a_ms": spread, "condition_met": ok})
            print("| %s | (b) - (a) = %.4f ms; spread of (a) = %.4f ms: condition %s | | | | | | | | |" % (label, med["b"] - med["a"], spread, "met" if ok else "NOT met"))
    print()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
