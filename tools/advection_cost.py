#!/usr/bin/env python3
"""What the midpoint transport (EULER_OPT_ADVECT_RK2, docs/advection_rk2.md) costs against the reference's forward Euler.

Two handles on one GPU are brought to the same state (both step the warm-up frames with RK1), then the second is switched to RK2 and the
two step alternately: first timed by wall clock per frame (no event brackets), then again with euler_profile brackets on the classes the
option touches (advect_velocity: u, v and the dye; marker_advect: the marker passes; marker_events: the dt-chain walk).  Prints a markdown
table and one JSON line.

  python tools/advection_cost.py --size 8192 --workload half_tank              # the headline state (roofline mode)
  python tools/advection_cost.py --size 4096 --workload dam_break --warmup 40  # moving, after the impact
  python tools/advection_cost.py --scheme maccormack                           # EULER_OPT_ADVECT_MACCORMACK instead (docs/advection_maccormack.md)
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import euler_amd as ea  # noqa: E402
from euler_amd import scenarios  # noqa: E402

CLASSES = ("advect_velocity", "marker_advect", "marker_events")
SCHEMES = {"rk2": ("RK2", ((ea.OPT_ADVECT_RK2, 1),)), "maccormack": ("MC", ((ea.OPT_ADVECT_MACCORMACK, 1),)),
           "rk2+maccormack": ("RK2+MC", ((ea.OPT_ADVECT_RK2, 1), (ea.OPT_ADVECT_MACCORMACK, 1)))}


def make(args):
    kw = dict(dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=args.max_iterations)
    s = ea.Simulation(args.size, args.size, **kw)
    if args.workload == "half_tank":
        s.load_half_tank()
    else:
        s.load_text(getattr(scenarios, args.workload)(), upscale=True)
    return s


def timed_frame(s):
    t0 = time.perf_counter()
    s.step()
    st = s.stats()      # (reads the counters: the frame has finished)
    return (time.perf_counter() - t0) * 1e3, st.last_substeps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--workload", default="half_tank", choices=["half_tank", "dam_break", "waterfall"])
    ap.add_argument("--warmup", type=int, default=3, help="frames both handles step with RK1 before the second is switched to RK2")
    ap.add_argument("--frames", type=int, default=6, help="frames per handle and phase")
    ap.add_argument("--max-iterations", type=int, default=100)
    ap.add_argument("--scheme", default="rk2", choices=list(SCHEMES), help="what the second handle switches to (default rk2)")
    args = ap.parse_args()
    label = SCHEMES[args.scheme][0]

    a, b = make(args), make(args)
    for _ in range(args.warmup):
        a.step(); b.step()
    for key, val in SCHEMES[args.scheme][1]:
        b.set_option(key, val)
    a.step(); b.step()      # (one untimed frame each in the new mode)

    wall = {0: [], 1: []}
    subs = {0: [], 1: []}
    for _ in range(args.frames):
        for k, s in ((0, a), (1, b)):
            ms, n = timed_frame(s)
            wall[k].append(ms); subs[k].append(n)

    for s in (a, b):
        s.profile_enable(CLASSES)
        s.profile_reset()
    nsub = {0: 0, 1: 0}
    for _ in range(args.frames):
        for k, s in ((0, a), (1, b)):
            s.step()
            nsub[k] += s.stats().last_substeps
    prof = {k: s.profile() for k, s in ((0, a), (1, b))}
    res = {"size": args.size, "workload": args.workload, "warmup": args.warmup, "frames": args.frames, "device": a.device_name(),
           "frame_ms": {k: statistics.median(wall[k]) for k in (0, 1)},
           "frame_substeps": {k: statistics.median(subs[k]) for k in (0, 1)},
           "class_ms_per_substep": {k: {c: prof[k].get(c, (0.0, 0))[0] / max(nsub[k], 1) for c in CLASSES} for k in (0, 1)},
           "multi_events": b.stats().marker_multi_events}
    if args.scheme != "rk2":
        res["scheme"] = args.scheme
    f1, f2 = res["frame_ms"][0], res["frame_ms"][1]
    per_sub = {k: res["frame_ms"][k] / max(res["frame_substeps"][k], 1) for k in (0, 1)}
    print("| %d^2 %s | RK1 | %s | %s / RK1 |" % (args.size, args.workload, label, label))
    print("|---|---|---|---|")
    for c in CLASSES:
        x, y = res["class_ms_per_substep"][0][c], res["class_ms_per_substep"][1][c]
        print("| %s, ms per substep | %.3f | %.3f | %.2f |" % (c, x, y, y / x if x else float("nan")))
    print("| frame wall time, ms (median) | %.2f | %.2f | %.3f |" % (f1, f2, f2 / f1))
    print("| substeps per frame (median) | %g | %g | |" % (res["frame_substeps"][0], res["frame_substeps"][1]))
    print("| wall time per substep, ms | %.2f | %.2f | %.3f |" % (per_sub[0], per_sub[1], per_sub[1] / per_sub[0]))
    print(json.dumps(res))
    a.close(); b.close()


if __name__ == "__main__":
    main()
