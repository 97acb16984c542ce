#!/usr/bin/env python3
"""What the flow diagnostics (euler_diagnostics, docs/diagnostics.md) cost on one GPU, beside the whole-domain overview as the yardstick.

On ONE handle (no dye), one state, one run: the kernel of euler_diagnostics over the whole interior and the kernel of euler_overview at 200 x 50
(k_overview<4, false> where X % 4 == 0), each as a HIP event pair around the launch (the `misc` profile class with nothing else running), median of
--calls calls after 3 untimed ones, with the tile map and with EULER_OPT_NO_TILE_MAP = 1.  The diagnostics must read 2 B per interior cell (count,
solid) + 8 B (u, v) - 10 B per cell of the tiles it visits; the overview 3 B + 8 B.  Also the whole call (memset, launch, 88-byte copy, sync)
and the box's copy figure from the same run.  Prints a markdown table and one JSON line.

  python tools/diagnostics_cost.py --size 8192 --workload half_tank
  python tools/diagnostics_cost.py --size 4096 --workload dam_break --warmup 40
"""
import argparse
import json
import os

import numpy as np
from cost_common import ea, kernel_ms, make


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--workload", default="half_tank", choices=["half_tank", "dam_break", "waterfall"])
    ap.add_argument("--warmup", type=int, default=3, help="frames before anything is measured")
    ap.add_argument("--calls", type=int, default=25, help="timed calls per row (after 3 untimed ones)")
    ap.add_argument("--max-iterations", type=int, default=100)
    ap.add_argument("--raster", default="200x50", help="the overview raster of the yardstick")
    args = ap.parse_args()
    w, h = (int(t) for t in args.raster.split("x"))
    s = make(args.size, args.workload, args.max_iterations)
    for _ in range(args.warmup):
        s.step()
    res = {"size": args.size, "workload": args.workload, "warmup": args.warmup, "calls": args.calls, "raster": [w, h], "device": s.device_name(),
           "lib": os.environ.get("EULER_HIP_LIB", ""), "rows": []}
    res["copy_gbps"] = s.copy_bandwidth(1 << 30, 10)
    count = s.get(ea.F_COUNT)
    n = args.size
    ty = (n + 63) // 64
    pad = np.zeros((ty * 64, ty * 64), bool)
    pad[:n, :n] = count > 0
    wet = pad.reshape(ty, 64, ty, 64).any(axis=(1, 3))
    inner = np.zeros((ty * 64, ty * 64), bool)
    inner[1:n - 1, 1:n - 1] = True
    cells_wet = int((inner.reshape(ty, 64, ty, 64).sum(axis=(1, 3)) * wet).sum())
    del count, pad, inner
    rec = s.diagnostics()
    res["record"] = {k: rec[k] for k in ("cells", "fluid", "markers", "count_max", "crowded", "max_div", "mean_abs_div", "kinetic_energy", "nonfinite")}
    print("| %d^2 %s, frame %d | tile map | kernel ms (median, min - max) | must read MB | TB/s | whole call ms |" % (n, args.workload, args.warmup))
    print("|---|---|---|---|---|---|")
    for no_map in (0, 1):
        s.set_option(ea.OPT_NO_TILE_MAP, no_map)
        for name, call, per_cell_all, per_cell_wet in (("overview %d x %d" % (w, h), lambda: s.overview(w, h), 3, 8), ("diagnostics", lambda: s.diagnostics_record(), 0, 10)):
            k, lo, hi, wh = kernel_ms(s, call, args.calls)
            need = (per_cell_all + per_cell_wet) * (n - 2) ** 2 if no_map else per_cell_all * (n - 2) ** 2 + per_cell_wet * cells_wet
            row = {"pass": name, "no_tile_map": no_map, "kernel_ms": k, "kernel_ms_min": lo, "kernel_ms_max": hi, "must_read_bytes": need, "tbps": need / (k * 1e-3) / 1e12, "call_ms": wh}
            res["rows"].append(row)
            print("| %s | %s | %.4f (%.4f - %.4f) | %.1f | %.2f | %.3f |" % (name, "off" if no_map else "on", k, lo, hi, need / 1e6, row["tbps"], row["call_ms"]))
    s.set_option(ea.OPT_NO_TILE_MAP, 0)
    s.close()
    r = res["rows"]
    res["ratio_tile_map_on"] = r[1]["kernel_ms"] / r[0]["kernel_ms"]
    res["ratio_tile_map_off"] = r[3]["kernel_ms"] / r[2]["kernel_ms"]
    print()
    print("diagnostics / overview kernel time: %.2f with the tile map, %.2f reading every tile (target: <= 1.25)" % (res["ratio_tile_map_on"], res["ratio_tile_map_off"]))
    print("copy figure of the box (euler_measure_copy_bandwidth, 1 GiB): %.0f GB/s" % res["copy_gbps"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
