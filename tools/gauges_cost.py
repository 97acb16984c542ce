#!/usr/bin/env python3
"""What the batched gauges (euler_gauges, docs/gauges.md) cost on one GPU, beside what the library offered before them.

The yardstick is the same 16 boxes - four of each kind: one cell, one column of 512 cells, one row of 512 cells, one 64 x 64 box - as 16 calls of
euler_flow_raster(box, 1, 1, EULER_FLOW_PRESSURE), on the same handle, state and run.  In ONE run, for each scene, with the tile map on and off:
  - the kernel time of one euler_gauges call and of the 16 flow calls (a HIP event pair around each launch of the `misc` profile class with nothing
    else running, summed over the call's launches; median of --calls calls after warm-up);
  - the whole-call wall time of both (launches, copies, syncs; the Python wrapper included on both sides), and their ratio.
The goal: one euler_gauges call costs at most the sum of the 16 flow calls in whole-call time.  Prints a markdown table and one JSON line.

  python tools/gauges_cost.py
  python tools/gauges_cost.py --scenes 4096:dam_break:20
"""
import argparse
import json

from cost_common import ea, kernel_ms, make


def boxes_of(size):
    """the four shapes, placed in the water of both scenes (the half tank's lower half, the dam break's block) and off the tile grid"""
    x, y = size // 4 + 10, 3 * size // 8 + 5
    return [(x, y, x, y), (x, y, x, y + 511), (x, y, x + 511, y), (x + 30, y - 20, x + 93, y + 43)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="8192:half_tank:3,4096:dam_break:20", help="size:workload:frames stepped before anything is measured")
    ap.add_argument("--calls", type=int, default=25, help="timed calls per figure (after 3 untimed ones)")
    ap.add_argument("--max-iterations", type=int, default=20)
    args = ap.parse_args()
    res = {"calls": args.calls, "rows": []}
    print("| scene | tile map | gauges: kernel ms (median, min - max) | 16 flow calls: kernel ms | gauges: whole call ms | 16 flow calls: whole ms | whole-call ratio | fluid cells in the 16 boxes |")
    print("|---|---|---|---|---|---|---|---|")
    for scene in args.scenes.split(","):
        size, workload, warmup = scene.split(":")
        size, warmup = int(size), int(warmup)
        s = make(size, workload, args.max_iterations)
        res["device"] = s.device_name()
        for _ in range(warmup):
            s.step()
        boxes = boxes_of(size)
        gauges = [(kind, box) for kind in (ea.GAUGE_LEVEL, ea.GAUGE_PRESSURE, ea.GAUGE_FORCE, ea.GAUGE_FLUX) for box in boxes]
        assert len(gauges) == 16
        for no_map in (0, 1):
            s.set_option(ea.OPT_NO_TILE_MAP, no_map)
            ga = kernel_ms(s, lambda: s.gauges(gauges), args.calls)
            fl = kernel_ms(s, lambda: [s.flow(1, 1, box=box, pressure=True) for (_, box) in gauges], args.calls)
            fluid = int(s.gauges(gauges)["fluid"].sum())
            row = {"size": size, "workload": workload, "no_tile_map": no_map, "gauges_kernel_ms": ga[0], "gauges_kernel_ms_range": ga[1:3], "flow16_kernel_ms": fl[0],
                   "flow16_kernel_ms_range": fl[1:3], "gauges_call_ms": ga[3], "flow16_call_ms": fl[3], "ratio": ga[3] / fl[3], "fluid": fluid}
            res["rows"].append(row)
            print("| %d^2 %s | %s | %.4f (%.4f - %.4f) | %.4f (%.4f - %.4f) | %.3f | %.3f | %.2f | %d |" %
                  (size, workload, "off" if no_map else "on", ga[0], ga[1], ga[2], fl[0], fl[1], fl[2], ga[3], fl[3], row["ratio"], fluid))
        s.set_option(ea.OPT_NO_TILE_MAP, 0)
        s.close()
    print()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
