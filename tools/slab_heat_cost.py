#!/usr/bin/env python3
"""What forcing and temperature cost a row-slab job per substep (docs/heat.md, docs/forcing.md "On row slabs"), over the library's RCCL communicator.

One rank per GPU: on a box with one GPU that is ONE rank, which still runs every staging copy and every exchange of the slab path through the real transport.
The tile-local solver is capped (--max-iterations, 20), so a substep's time is mostly the stages around the iterations.  Per configuration two figures:
  wall      milliseconds per substep of euler_step by the host's clock, frames not profiled: kernels, exchanges, staging copies and host-side work together;
  outside   the profile classes outside the iterations (every class but the solver's per-iteration ones), summed, per substep - in frames of their own, since
            the event pairs serialise the stream.
under
  (a) a build of the parent commit (--parent-root: a checkout of it with its library built; without it the row is left out),
  (b) this build, neither entry point ever called,
  (c) forcing: gravity (3, -8), a shake and 16 boxes of 64 x 64 cells in the water, off the tile grid,
  (d) (c) plus heat with kappa > 0 and beta != 0, a FIX and a RATE box,
with the number of T exchanges a substep issues beside (c) and (d): the ones of its own, and the rides in groups that travel anyway (docs/heat.md).
A library is loaded once per process, so a worker measures ONE library on ONE scene: after the warm-up frames it walks its configurations --blocks times, each
time one untimed frame, --frames wall frames and --frames profiled ones.  Worker kinds alternate (--rounds): the parent's with (a), this build's with (b) - the same
schedule, so the two step through the same states frame for frame -, this build's with (c), (d).  Reported: median and range over all blocks of all rounds.
The condition: (b)'s wall median is not above (a)'s by more than the spread of (a)'s own blocks.
Prints a markdown table and one JSON line.

  python tools/slab_heat_cost.py --parent-root /path/to/parent/checkout
  python tools/slab_heat_cost.py --scenes 4096:dam_break:20 --rounds 1
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERATION_CLASSES = {"precon_factor", "forward_solve", "backward_solve", "apply_a", "dot", "update_pr", "update_search", "reduce_final", "jacobi", "precond_tile",
                     "coarse_cycle", "resident_pcg"}
GRAVITY, SHAKE = (3.0, -8.0), (1.5, 0.5, 0.8, 0.3)
KAPPA, BETA = 0.05, 0.02


def force_boxes(size):      # 16 boxes of 64 x 64 cells in the lower left of the grid - water in both scenes -, off the tile grid
    x, y = size // 8 + 10, size // 4 + 5
    return [((x + 90 * (k % 4), y + 90 * (k // 4), x + 90 * (k % 4) + 63, y + 90 * (k // 4) + 63), (2.0, 1.0)) for k in range(16)]


def t_exchanges(config):
    """(of its own, riding in a group that travels anyway) per substep"""
    if config != "d":
        return (0, 0)
    own = (1 if KAPPA > 0 else 0) + (1 if BETA != 0 else 0)
    return (own, 1 + (0 if BETA != 0 else 1))      # behind the sources always; with vtmp where the last writer left the rows stale


def worker(args):
    sys.path.insert(0, args.worker)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29871")
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    import torch
    import torch.distributed as dist
    import euler_amd as ea
    from euler_amd import scenarios
    from euler_amd.slab import SLAB_LOCAL, RcclComm
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    size, workload, warmup = args.scene.split(":")
    size, warmup = int(size), int(warmup)
    s = ea.Simulation(size, size, device=local, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=args.max_iterations, slab=(rank, world))
    comm = RcclComm(s, SLAB_LOCAL)
    if workload == "half_tank":
        s.load_half_tank()
    else:
        s.load_text(getattr(scenarios, workload)(), upscale=True)
    for _ in range(warmup):
        s.step()
    names = [n for n in ea.profile_class_names() if n not in ITERATION_CLASSES]
    wall = {c: [] for c in args.configs}
    outside = {c: [] for c in args.configs}
    for _ in range(args.blocks):
        for c in args.configs:
            if c in ("c", "d"):
                s.set_forcing(GRAVITY, SHAKE, force_boxes(size))
                if c == "d":
                    x, y = size // 8 + 10, size // 4 + 5
                    s.set_heat(1.0, BETA, KAPPA, 5.0, [(ea.HEAT_FIX, 8.0, (x, y, x + 200, y + 40)), (ea.HEAT_RATE, 3.0, (x + 50, y + 100, x + 300, y + 160))])
                else:
                    s.heat_off()
            s.step()      # untimed: the first frame under a configuration
            nsub = 0
            t0 = time.perf_counter()
            for _ in range(args.frames):
                s.step()      # (returns behind the frame's last synchronisation)
                nsub += s.stats().last_substeps
            wall[c].append(1e3 * (time.perf_counter() - t0) / max(nsub, 1))
            s.profile_enable(names)
            s.profile_reset()
            nsub = 0
            for _ in range(args.frames):
                s.step()
                nsub += s.stats().last_substeps
            outside[c].append(sum(v[0] for v in s.profile().values()) / max(nsub, 1))
            s.L.euler_profile_enable(s.h, 0)
    if comm.error:
        raise RuntimeError(comm.error)
    if rank == 0:
        print(json.dumps({"wall": wall, "outside": outside, "device": s.device_name(), "world": world}))
    s.close()
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="8192:half_tank:2,4096:dam_break:20", help="size:workload:frames stepped before anything is measured")
    ap.add_argument("--parent-root", default="", help="a checkout of the parent commit with its library built: row (a)")
    ap.add_argument("--rounds", type=int, default=2, help="parent / new worker pairs per scene")
    ap.add_argument("--blocks", type=int, default=3, help="passes over its configurations per worker")
    ap.add_argument("--frames", type=int, default=3, help="timed frames per block and figure")
    ap.add_argument("--max-iterations", type=int, default=20)
    ap.add_argument("--worker", default="", help=argparse.SUPPRESS)
    ap.add_argument("--scene", default="", help=argparse.SUPPRESS)
    ap.add_argument("--configs", default="", type=lambda t: t.split(","), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    res = {"rounds": args.rounds, "blocks": args.blocks, "frames": args.frames, "max_iterations": args.max_iterations, "rows": []}
    print("| scene | configuration | wall ms per substep: median (min - max) | classes outside the iterations, ms per substep: median (min - max) | T exchanges per substep: own + riding |")
    print("|---|---|---|---|---|")
    names = {"a": "(a) parent commit", "b": "(b) this build, untouched", "c": "(c) gravity + shake + 16 boxes", "d": "(d) (c) + heat, kappa > 0, beta != 0"}
    for scene in args.scenes.split(","):
        wall, outside = {c: [] for c in "abcd"}, {c: [] for c in "abcd"}
        for _ in range(args.rounds):
            for root, configs in ((args.parent_root, "a"), (ROOT, "b"), (ROOT, "c,d")):
                if not root:
                    continue
                cmd = [sys.executable, os.path.abspath(__file__), "--worker", root, "--scene", scene, "--configs", configs, "--blocks", str(args.blocks),
                       "--frames", str(args.frames), "--max-iterations", str(args.max_iterations)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:      # a worker that failed ends the run: nothing more is started on the GPU
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    return 1
                w = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
                res["device"], res["world"] = w["device"], w["world"]
                for c in w["wall"]:
                    wall[c] += w["wall"][c]
                    outside[c] += w["outside"][c]
        label = scene.rsplit(":", 1)[0].replace(":", "^2 ")
        for c in "abcd":
            if not wall[c]:
                continue
            mw, mo = statistics.median(wall[c]), statistics.median(outside[c])
            own, ride = t_exchanges(c)
            res["rows"].append({"scene": scene, "config": c, "wall_median_ms": mw, "wall_min_ms": min(wall[c]), "wall_max_ms": max(wall[c]), "outside_median_ms": mo,
                                "outside_min_ms": min(outside[c]), "outside_max_ms": max(outside[c]), "t_exchanges_own": own, "t_exchanges_riding": ride})
            print("| %s | %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %s |" % (label, names[c], mw, min(wall[c]), max(wall[c]), mo, min(outside[c]), max(outside[c]),
                                                                            "%d + %d" % (own, ride) if c in "cd" else ""))
        if wall["a"] and wall["b"]:
            for what, got in (("wall", wall), ("outside", outside)):
                spread = max(got["a"]) - min(got["a"])
                diff = statistics.median(got["b"]) - statistics.median(got["a"])
                ok = diff <= spread
                res["rows"].append({"scene": scene, "figure": what, "b_minus_a_ms": diff, "spread_a_ms": spread, "condition_met": ok})
                print("| %s | %s: (b) - (a) = %.4f ms; spread of (a) = %.4f ms: condition %s | | | |" % (label, what, diff, spread, "met" if ok else "NOT met"))
    print()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
