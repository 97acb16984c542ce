#!/usr/bin/env python3
"""What the forcing (euler_set_forcing, docs/forcing.md) costs in the velocity advection's kernel class, per substep, on one GPU.

For each scene the time of the `advect_velocity` profile class per substep (a HIP event pair around each of its launches) under
  (a) a build of the parent commit (--parent-root: a checkout of it with its library built; without it the row is left out),
  (b) this build with the default forcing - the kernels of (a) -,
  (c) gravity (3, -8) plus a shake - the forced instantiations -,
  (d) (c) plus 16 boxes of 64 x 64 cells in the water, off the tile grid,
  (e) (c) plus one box over the whole interior.
A library is loaded once per process, so a worker process measures ONE library on ONE scene: after the warm-up frames it walks its configurations
--blocks times, each time one untimed frame and --frames timed ones.  Three kinds of worker run in turn (--rounds): the parent's with (a), this build's
with (b) alone - the same schedule as (a)'s, so the two step through the same states frame for frame - and this build's with (c), (d), (e), whose
states follow their own forcing.  Reported: the median and the range over all blocks of all rounds.  The condition: (b) is not slower than (a) by more than
the spread of (a)'s own blocks.
Prints a markdown table and one JSON line.

  python tools/forcing_cost.py --parent-root /path/to/parent/checkout
  python tools/forcing_cost.py --scenes 4096:dam_break:20 --rounds 1
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLS = "advect_velocity"
GRAVITY, SHAKE = (3.0, -8.0), (1.5, 0.5, 0.8, 0.3)


def boxes_of(size, config):
    if config == "d":      # 16 boxes of 64 x 64 cells in the lower left of the grid - water in both scenes -, off the tile grid
        x, y = size // 8 + 10, size // 4 + 5
        return [((x + 90 * (k % 4), y + 90 * (k // 4), x + 90 * (k % 4) + 63, y + 90 * (k // 4) + 63), (2.0, 1.0)) for k in range(16)]
    if config == "e":
        return [((1, 1, size - 2, size - 2), (2.0, 1.0))]
    return []


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
    out = {c: [] for c in args.configs}
    live = {}
    for _ in range(args.blocks):
        for c in args.configs:
            if c == "b":
                s.set_forcing()
            elif c != "a":
                s.set_forcing(GRAVITY, SHAKE, boxes_of(size, c))
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
            if c in ("d", "e") and c not in live:      # live faces the boxes touch, from the fields as they stand
                cn, so = s.get(ea.F_COUNT) > 0, s.get(ea.F_SOLID) != 0
                n = 0
                for (x0, y0, x1, y1), _f in boxes_of(size, c):
                    b, r, u = (slice(y0, y1 + 1), slice(x0, x1 + 1)), (slice(y0, y1 + 1), slice(x0 + 1, x1 + 2)), (slice(y0 + 1, y1 + 2), slice(x0, x1 + 1))
                    n += int(((cn[b] | cn[r]) & ~(so[b] | so[r])).sum()) + int(((cn[b] | cn[u]) & ~(so[b] | so[u])).sum())
                live[c] = n
    print(json.dumps({"ms_per_substep": out, "live_faces": live, "device": s.device_name()}))
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
    print("| scene | configuration | advect_velocity ms per substep: median (min - max) | against (b) | live faces in the boxes | box pass: added time over (c) |")
    print("|---|---|---|---|---|---|")
    names = {"a": "(a) parent commit", "b": "(b) default forcing", "c": "(c) gravity + shake", "d": "(d) (c) + 16 boxes of 64 x 64", "e": "(e) (c) + one box over the interior"}
    for scene in args.scenes.split(","):
        got, live = {c: [] for c in "abcde"}, {}
        for _ in range(args.rounds):
            for root, configs in ((args.parent_root, "a"), (ROOT, "b"), (ROOT, "c,d,e")):
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
                live.update(w["live_faces"])
                for c, v in w["ms_per_substep"].items():
                    got[c] += v
        med = {c: statistics.median(v) for c, v in got.items() if v}
        for c in "abcde":
            if c not in med:
                continue
            v = got[c]
            extra = ""
            if c in live and live[c]:
                extra = "%.1f ns per 1000 faces" % (1e6 * max(med[c] - med["c"], 0.0) / live[c] * 1000)
            res["rows"].append({"scene": scene, "config": c, "median_ms": med[c], "min_ms": min(v), "max_ms": max(v), "live_faces": live.get(c, 0)})
            print("| %s | %s | %.4f (%.4f - %.4f) | %.3f | %s | %s |" % (scene.rsplit(":", 1)[0].replace(":", "^2 "), names[c], med[c], min(v), max(v), med[c] / med["b"], live.get(c, ""), extra))
        if "a" in med:
            spread = max(got["a"]) - min(got["a"])
            ok = med["b"] - med["a"] <= spread
            res["rows"].append({"scene": scene, "b_minus_a_ms": med["b"] - med["a"], "spread_a_ms": spread, "condition_met": ok})
            print("| %s | (b) - (a) = %.4f ms; spread of (a) = %.4f ms: condition %s | | | | |" % (scene.rsplit(":", 1)[0].replace(":", "^2 "), med["b"] - med["a"], spread, "met" if ok else "NOT met"))
    print()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
