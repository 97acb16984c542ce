#!/usr/bin/env python3
"""What the pan-and-zoom viewport (euler_overview_box, euler_marker_raster; docs/viewport.md) costs on one GPU.

Kernel times are HIP event pairs around the launch (the `misc` profile class with nothing else running), the median of --calls calls after warm-up.
  - zoomed in: the raster of a 64 x 32-cell box at scale 4 on the --size^2 half tank (almost every marker is rejected), beside n_markers * 8 bytes
    at the box's own copy figure (euler_measure_copy_bandwidth on the same handle: reads plus writes);
  - everything in the box: the raster of the whole interior at scale 1 on the --whole-size^2 half tank (the largest square whose interior fits the
    2^24-pixel limit is 4096^2), beside the `marker_bin` profile class of a frame with EULER_OPT_MARKERS_TWO_PASS = 1 per refresh - the class
    holds k_bin_markers AND the counters' rotate / narrow passes, so it is an upper bound of k_bin_markers; --trace-leg runs the same work for a kernel trace
    (a profiler's per-kernel statistics then show k_bin_markers and k_marker_raster side by side);
  - the box overview of the same 64 x 32 box and of a 2048 x 1024 box at 200 x 50.
Prints markdown tables and one JSON line.

  python tools/viewport_cost.py --size 8192 --whole-size 4096
  python tools/viewport_cost.py --trace-leg --whole-size 4096
"""
import argparse
import json
import statistics

from cost_common import ea, kernel_ms, make


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--whole-size", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3, help="frames before anything is measured")
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--max-iterations", type=int, default=20)
    ap.add_argument("--trace-leg", action="store_true", help="only the work a kernel trace should see: frames with two-pass binning and whole-interior rasters")
    args = ap.parse_args()
    res = {"size": args.size, "whole_size": args.whole_size, "calls": args.calls}

    if not args.trace_leg:
        s = make(args.size, "half_tank", args.max_iterations)
        res["device"] = s.device_name()
        for _ in range(args.warmup):
            s.step()
        n = s.stats().n_markers
        copy_gbps = s.copy_bandwidth(1 << 30, 10)
        mid = args.size // 2
        box = (mid - 32, args.size // 4 - 16, mid + 31, args.size // 4 + 15)      # 64 x 32 cells inside the water
        k, lo, hi, _ = kernel_ms(s, lambda: s.marker_raster(box, 4), args.calls)
        inbox = int(s.marker_raster(box, 4).sum())
        yard = n * 8 / (copy_gbps * 1e9) * 1e3
        res["zoomed"] = {"box": box, "scale": 4, "n_markers": n, "in_box": inbox, "kernel_ms": k, "kernel_ms_min": lo, "kernel_ms_max": hi, "copy_gbps": copy_gbps,
                         "yardstick_ms": yard, "ratio": k / yard}
        print("| %d^2 half tank, raster %s scale 4 | markers | in the box | kernel ms (median, min - max) | copy figure GB/s | n * 8 B at it, ms | ratio |" % (args.size, box))
        print("|---|---|---|---|---|---|---|")
        print("| | %d | %d | %.3f (%.3f - %.3f) | %.0f | %.3f | %.2f |" % (n, inbox, k, lo, hi, copy_gbps, yard, k / yard))
        print()
        print("| box overview | raster | kernel ms (median, min - max) |")
        print("|---|---|---|")
        res["overview_box"] = []
        big = (mid - 1024, 2, mid + 1023, 1025)
        for b, w, h in ((box, 64, 32), (big, 200, 50), ((1, 1, args.size - 2, args.size - 2), 200, 50)):
            k, lo, hi, _ = kernel_ms(s, lambda: s.overview(w, h, box=b), args.calls)
            res["overview_box"].append({"box": b, "raster": [w, h], "kernel_ms": k, "kernel_ms_min": lo, "kernel_ms_max": hi})
            print("| %s | %d x %d | %.3f (%.3f - %.3f) |" % (b, w, h, k, lo, hi))
        s.close()

    s = make(args.whole_size, "half_tank", args.max_iterations)
    s.set_option(ea.OPT_MARKERS_TWO_PASS, 1)
    for _ in range(args.warmup):
        s.step()
    whole = (1, 1, args.whole_size - 2, args.whole_size - 2)
    if args.trace_leg:
        for _ in range(2):
            s.step()
        for _ in range(args.calls):
            s.marker_raster(whole, 1)
        s.close()
        return
    n = s.stats().n_markers
    k, lo, hi, _ = kernel_ms(s, lambda: s.marker_raster(whole, 1), args.calls)
    s.profile_enable(["marker_bin"])
    per = []
    for _ in range(5):
        s.profile_reset()
        s.step()
        per.append(s.profile()["marker_bin"][0] / s.stats().last_substeps)
    s.L.euler_profile_enable(s.h, 0)
    binms = statistics.median(per)
    res["whole"] = {"n_markers": n, "kernel_ms": k, "kernel_ms_min": lo, "kernel_ms_max": hi, "marker_bin_class_ms_per_refresh": binms, "ratio_to_class": k / binms}
    print()
    print("| %d^2 half tank, raster of the whole interior, scale 1 | markers | kernel ms (median, min - max) | marker_bin class per refresh, two-pass, ms | ratio |" % args.whole_size)
    print("|---|---|---|---|---|")
    print("| | %d | %.3f (%.3f - %.3f) | %.3f | %.2f |" % (n, k, lo, hi, binms, k / binms))
    s.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
