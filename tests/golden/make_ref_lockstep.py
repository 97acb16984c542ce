#!/usr/bin/env python3
"""Regenerate tests/golden/ref_lockstep.json: the compiled unmodified reference (oracle/_ref/libeuler_ref.so) stepped through the cases of
tests/test_oracle_vs_ref.py, per frame the SHA-1 (tests/trajectories.py digest) of every array that test compares.  Runs only where oracle/_ref/ could be
built (the reference tree present); elsewhere test_oracle_vs_ref.py checks the oracle against this record.  python tests/golden/make_ref_lockstep.py"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from golden_util import load, scenario_text  # noqa: E402
from oracle_lib import Reference  # noqa: E402
from trajectories import digest  # noqa: E402
from test_oracle_vs_ref import CASES, FIELDS  # noqa: E402


def main():
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for scn, frames in CASES:
            path = os.path.join(d, scn + ".txt")
            with open(path, "w") as f:
                f.write(scenario_text(load(scn + "_frames.npz")))
            ref = Reference().init(path)
            rec = []
            for _ in range(frames):
                ref.step()
                rec.append({n: digest(getattr(ref, n)) for n in FIELDS + ("markers",)})
            out[scn] = rec
            print(scn, frames, "frames")
    with open(os.path.join(HERE, "ref_lockstep.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_ref_lockstep.py", "reference": "oracle/_ref/libeuler_ref.so (oracle/Makefile `ref`)", "cases": out}, f,
                  separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
