#!/usr/bin/env python3
"""What the flow raster (euler_flow_raster, docs/flow_raster.md) costs on one GPU, beside the overview of the same box and raster.

In ONE run, on handles without dye, for each scene and raster, with the tile map on and off:
  - the kernel time of the velocity part (a HIP event pair around each launch of the `misc` profile class with nothing else running, median of
    --calls calls after warm-up) against euler_overview_box's, and their ratio (the goal: at most 1.5);
  - the kernel time of the pressure part: the `misc` time of a call with EULER_FLOW_PRESSURE less that of a call without;
  - the whole call with the pressure beside the euler_get_field(EULER_F_PRESSURE) it replaces.
Prints a markdown table and one JSON line.

  python tools/flow_cost.py
  python tools/flow_cost.py --scenes 4096:dam_break:20 --rasters 200x50
"""
import argparse
import json
import statistics
import time

from cost_common import ea, kernel_ms, make


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="8192:half_tank:3,4096:dam_break:20", help="size:workload:frames stepped before anything is measured")
    ap.add_argument("--rasters", default="200x50,1024x1024")
    ap.add_argument("--calls", type=int, default=25, help="timed calls per figure (after 3 untimed ones)")
    ap.add_argument("--max-iterations", type=int, default=20)
    args = ap.parse_args()
    rasters = [tuple(int(t) for t in r.split("x")) for r in args.rasters.split(",")]
    res = {"calls": args.calls, "rows": []}
    print("| scene | raster | tile map | overview ms (median) | flow, velocity ms | ratio | pressure part ms | flow call with pressure ms | get_field(PRESSURE) ms |")
    print("|---|---|---|---|---|---|---|---|---|")
    for scene in args.scenes.split(","):
        size, workload, warmup = scene.split(":")
        size, warmup = int(size), int(warmup)
        s = make(size, workload, args.max_iterations)
        res["device"] = s.device_name()
        for _ in range(warmup):
            s.step()
        get = []
        for _ in range(3):
            t0 = time.perf_counter()
            s.get(ea.F_PRESSURE)
            get.append((time.perf_counter() - t0) * 1e3)
        get_ms = statistics.median(get)
        for (w, h) in rasters:
            for no_map in (0, 1):
                s.set_option(ea.OPT_NO_TILE_MAP, no_map)
                ov = kernel_ms(s, lambda: s.overview(w, h), args.calls)
                fl = kernel_ms(s, lambda: s.flow(w, h), args.calls)
                fp = kernel_ms(s, lambda: s.flow(w, h, pressure=True), args.calls)
                row = {"size": size, "workload": workload, "raster": [w, h], "no_tile_map": no_map, "overview_ms": ov[0], "overview_ms_range": ov[1:3], "flow_ms": fl[0], "flow_ms_range": fl[1:3],
                       "ratio": fl[0] / ov[0], "pressure_part_ms": fp[0] - fl[0], "flow_pressure_call_ms": fp[3], "get_pressure_ms": get_ms}
                res["rows"].append(row)
                print("| %d^2 %s | %d x %d | %s | %.3f (%.3f - %.3f) | %.3f (%.3f - %.3f) | %.2f | %.3f | %.2f | %.1f |" %
                      (size, workload, w, h, "off" if no_map else "on", ov[0], ov[1], ov[2], fl[0], fl[1], fl[2], row["ratio"], row["pressure_part_ms"], fp[3], get_ms))
            s.set_option(ea.OPT_NO_TILE_MAP, 0)
        s.close()
    print()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
