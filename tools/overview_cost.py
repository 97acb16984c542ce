#!/usr/bin/env python3
"""What the whole-domain overview (euler_overview, docs/overview.md) costs on one GPU.

For one workload and a list of rasters, with and without the dye:
  - the kernel alone: a HIP event pair around each launch (the `misc` profile class with nothing else running), median of --calls calls
    after warm-up, and the bytes it must read - 3 B per interior cell everywhere + 20 B (8 B without the dye) per interior cell of the
    64 x 64 tiles that hold water - as achieved TB/s beside the box's own copy figure (euler_measure_copy_bandwidth) from the same run;
  - the whole call (launch, copy of the records, sync) beside what a user pays without it: euler_get_field of the same fields plus the
    numpy reduction of tests/overview_ref.py;
  - the wall time of a frame with and without one call per frame.
Prints markdown tables and one JSON line.

  python tools/overview_cost.py --size 8192 --workload half_tank
  python tools/overview_cost.py --size 4096 --workload dam_break --warmup 40
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
from cost_common import ROOT, ea, kernel_ms, make

sys.path.insert(0, os.path.join(ROOT, "tests"))
DYE = (ea.F_DYE_R, ea.F_DYE_G, ea.F_DYE_B)


def must_read(count, dye):
    """bytes the pass has to read: the three mask bytes of every interior cell + u, v (+ the dye) of the interior cells of tiles with water"""
    Y, X = count.shape
    ty, tx = (Y + 63) // 64, (X + 63) // 64
    pad = np.zeros((ty * 64, tx * 64), bool)
    pad[:Y, :X] = count > 0
    wet = pad.reshape(ty, 64, tx, 64).any(axis=(1, 3))
    inner = np.zeros((ty * 64, tx * 64), bool)
    inner[1:Y - 1, 1:X - 1] = True
    cells_wet = int((inner.reshape(ty, 64, tx, 64).sum(axis=(1, 3)) * wet).sum())
    return 3 * (X - 2) * (Y - 2) + (20 if dye else 8) * cells_wet, cells_wet


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--workload", default="half_tank", choices=["half_tank", "dam_break", "waterfall"])
    ap.add_argument("--warmup", type=int, default=3, help="frames before anything is measured")
    ap.add_argument("--calls", type=int, default=25, help="timed calls per raster (after 3 untimed ones)")
    ap.add_argument("--frames", type=int, default=4, help="frames per leg of the frame-time comparison")
    ap.add_argument("--max-iterations", type=int, default=100)
    ap.add_argument("--rasters", default="200x50,1024x1024")
    ap.add_argument("--no-host-leg", action="store_true", help="skip the get + numpy comparison (slow at 8192^2)")
    args = ap.parse_args()
    rasters = [tuple(int(t) for t in r.split("x")) for r in args.rasters.split(",")]
    res = {"size": args.size, "workload": args.workload, "warmup": args.warmup, "calls": args.calls, "rows": []}
    print("| %d^2 %s | dye | tile map | kernel ms (median) | must read MB | TB/s | of the copy figure | whole call ms |" % (args.size, args.workload))
    print("|---|---|---|---|---|---|---|---|")
    for rainbow in (False, True):
        s = make(args.size, args.workload, args.max_iterations, rainbow)
        res["device"] = s.device_name()
        for _ in range(args.warmup):
            s.step()
        copy_gbps = s.copy_bandwidth(1 << 30, 10)
        res.setdefault("copy_gbps", []).append(copy_gbps)
        nbytes, cells_wet = must_read(s.get(ea.F_COUNT), rainbow)
        for (w, h) in rasters:
            for no_map in (0, 1):
                s.set_option(ea.OPT_NO_TILE_MAP, no_map)
                need = nbytes if not no_map else (23 if rainbow else 11) * (args.size - 2) ** 2
                k, lo, hi, wh = kernel_ms(s, lambda: s.overview(w, h), args.calls)
                tbps = need / (k * 1e-3) / 1e12
                row = {"raster": [w, h], "dye": rainbow, "no_tile_map": no_map, "kernel_ms": k, "kernel_ms_min": lo, "kernel_ms_max": hi, "must_read_bytes": need,
                       "tbps": tbps, "copy_gbps": copy_gbps, "call_ms": wh}
                res["rows"].append(row)
                print("| %d x %d | %s | %s | %.3f (%.3f - %.3f) | %.1f | %.2f | %.2f | %.2f |" % (w, h, "yes" if rainbow else "no", "off" if no_map else "on", k, lo, hi, need / 1e6, tbps,
                                                                                            tbps * 1e3 / copy_gbps, wh))
            s.set_option(ea.OPT_NO_TILE_MAP, 0)
        if rainbow:
            # what a user pays today for the same picture: the eight fields over PCIe + the reduction on the host
            if not args.no_host_leg:
                import overview_ref as ref
                t0 = time.perf_counter()
                g = [s.get(f) for f in (ea.F_SOLID, ea.F_SINK, ea.F_COUNT, ea.F_U, ea.F_V)]
                d = tuple(s.get(f) for f in DYE)
                t1 = time.perf_counter()
                ref.overview_ref(*g, d, *rasters[0])
                t2 = time.perf_counter()
                res["host_get_ms"], res["host_reduce_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
                del g, d
            # a frame with and without one call per frame
            wall = {0: [], 1: []}
            for k in (0, 1, 0, 1):
                for _ in range(args.frames):
                    t0 = time.perf_counter()
                    s.step()
                    if k:
                        s.overview(*rasters[-1])
                    s.stats()
                    wall[k].append((time.perf_counter() - t0) * 1e3)
            res["frame_ms"] = {k: statistics.median(wall[k]) for k in (0, 1)}
            res["frame_substeps"] = s.stats().last_substeps
        s.close()
    print()
    print("copy figure of the box (euler_measure_copy_bandwidth, 1 GiB): %s GB/s" % ", ".join("%.0f" % g for g in res["copy_gbps"]))
    if "host_get_ms" in res:
        print("get of the eight fields: %.0f ms; numpy reduction to %d x %d: %.0f ms" % (res["host_get_ms"], rasters[0][0], rasters[0][1], res["host_reduce_ms"]))
    print("frame wall time (median, %d substeps in the last): %.2f ms without, %.2f ms with one %d x %d call per frame" % (res["frame_substeps"], res["frame_ms"][0], res["frame_ms"][1], rasters[-1][0], rasters[-1][1]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
