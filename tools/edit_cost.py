#!/usr/bin/env python3
"""What a device-side scene edit (euler_edit_box, docs/editing.md) costs on one GPU, beside the only way to make the same edit without it: the
euler_get_field / euler_set_field / euler_set_markers round trip of solid, count and the marker array through the host.

Per --sizes entry, the size^2 half tank after --warmup frames; the box is 256 x 256 cells inside the water.  The ops run in a cycle in which every one of
them has work to do (drain, fill, solid, clear, fill, sink, clear, source, clear), --calls times; per op the median (min - max) of
  - the HIP-event time of the WHOLE call: an event pair on the handle's stream around euler_edit_box - kernels, the two read-backs and the waits;
  - the `misc` profile class of the call (census, marker pass, cell pass, seeding: an event pair around each launch), in a second round of cycles.
The marker pass alone is the misc class of `drain` minus that of `clear` (census and cell pass of the same box); its bytes are n_markers * 8, beside the
box's copy figure (euler_measure_copy_bandwidth: reads plus writes).  The host round trip moves the three arrays out and back in (the numpy work of the edit in
between is NOT timed), the same event pair around it, --host-calls times.

Writes the tables to --out (default profiles/editing.md; whatever follows a "## Reading" line in an existing file is kept) and prints one JSON line.

  python tools/edit_cost.py --sizes 4096 8192
"""
import argparse
import json
import os
import statistics

import torch

from cost_common import ROOT, ea, make

CYCLE = ("drain", "fill", "solid", "clear", "fill", "sink", "clear", "source", "clear")
OPS = {"solid": ea.EDIT_SOLID, "clear": ea.EDIT_CLEAR, "sink": ea.EDIT_SINK, "source": ea.EDIT_SOURCE, "fill": ea.EDIT_FILL, "drain": ea.EDIT_DRAIN}
ORDER = ("solid", "clear", "sink", "source", "fill", "drain")


def event_ms(stream, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def fmt(v):
    return "%.3f (%.3f - %.3f)" % (statistics.median(v), min(v), max(v))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--warmup", type=int, default=2, help="frames before anything is measured")
    ap.add_argument("--calls", type=int, default=7, help="cycles of the ops")
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--max-iterations", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "editing.md"))
    args = ap.parse_args()
    res, lines = {"calls": args.calls, "host_calls": args.host_calls, "runs": []}, []
    stream = torch.cuda.Stream()
    for size in args.sizes:
        s = make(size, "half_tank", args.max_iterations)
        assert s.L.euler_set_stream(s.h, ea.C.c_void_p(stream.cuda_stream)) == 0
        for _ in range(args.warmup):
            s.step()
        n = s.stats().n_markers
        copy_gbps = s.copy_bandwidth(1 << 30, 10)
        mid = size // 2
        box = (mid - 128, size // 4 - 128, mid + 127, size // 4 + 127)
        for name in CYCLE:      # untimed: every kernel has run once
            s.edit_box(OPS[name], box)
        whole = {k: [] for k in OPS}
        for _ in range(args.calls):
            for name in CYCLE:
                whole[name].append(event_ms(stream, lambda: s.edit_box(OPS[name], box)))
        s.profile_enable(["misc"])
        misc = {k: [] for k in OPS}
        for _ in range(args.calls):
            for name in CYCLE:
                s.profile_reset()
                s.edit_box(OPS[name], box)
                misc[name].append(s.profile()["misc"][0])
        s.L.euler_profile_enable(s.h, 0)
        host = []
        for _ in range(args.host_calls):
            def round_trip():
                solid, count, markers = s.get(ea.F_SOLID), s.get(ea.F_COUNT), s.get(ea.F_MARKERS)
                s.set(ea.F_SOLID, solid); s.set(ea.F_COUNT, count); s.set_markers(markers)
            host.append(event_ms(stream, round_trip))
        host_ms = statistics.median(host)
        host_bytes = 2 * (2 * size * size + 8 * n)
        pass_ms = statistics.median(misc["drain"]) - statistics.median(misc["clear"])
        pass_gbps = n * 8 / (pass_ms * 1e-3) / 1e9
        run = {"size": size, "device": s.device_name(), "n_markers": n, "box": box, "copy_gbps": copy_gbps, "host_round_trip_ms": host_ms, "host_round_trip_bytes": host_bytes,
               "marker_pass_ms": pass_ms, "marker_pass_gbps": pass_gbps,
               "ops": {k: {"call_ms": statistics.median(whole[k]), "call_ms_min": min(whole[k]), "call_ms_max": max(whole[k]), "misc_ms": statistics.median(misc[k]),
                           "host_over_device": host_ms / statistics.median(whole[k])} for k in ORDER}}
        res["runs"].append(run)
        lines += ["## %d^2 half tank, frame %d: %d markers, box %s (%s)" % (size, args.warmup, n, box, run["device"]), "",
                  "| op | whole call, HIP events, ms (median, min - max) | `misc` class (census, marker pass, cells, seeding), ms | host round trip / device edit |", "|---|---|---|---|"]
        for k in ORDER:
            lines.append("| %s | %s | %s | %.0f x |" % (k, fmt(whole[k]), fmt(misc[k]), run["ops"][k]["host_over_device"]))
        lines += ["", "Host round trip of solid, count and the markers (get x 3, set x 3; %.2f GB moved, the numpy edit not timed): %s ms." % (host_bytes / 1e9, fmt(host)),
                  "", "Marker pass alone (`misc` of drain - `misc` of clear): %.3f ms for %d markers x 8 B = %.0f GB/s; the box's copy figure (reads plus writes) %.0f GB/s: %.2f of it."
                  % (pass_ms, n, pass_gbps, copy_gbps, pass_gbps / copy_gbps), ""]
        s.close()
    head = ["# Device-side scene editing: cost beside the host round trip (`tools/edit_cost.py`, one MI355X)", "",
            "`python tools/edit_cost.py --sizes %s --warmup %d --calls %d --host-calls %d`: the method is the tool's header.  The ops run in the cycle" % (" ".join(map(str, args.sizes)), args.warmup, args.calls, args.host_calls),
            "%s, so that every call has markers to delete or cells to seed." % ", ".join(CYCLE), ""]
    tail = []
    if os.path.exists(args.out):
        old = open(args.out).read().split("\n")
        at = [i for i, l in enumerate(old) if l.startswith("## Reading")]
        if at:
            tail = old[at[0]:]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(head + lines + tail).rstrip("\n") + "\n")
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
