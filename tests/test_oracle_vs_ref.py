"""Oracle vs the compiled reference itself (oracle/_ref/libeuler_ref.so), longer than the
committed fixtures.  Where the reference build is absent, against the reference's per-frame digests
recorded in golden/ref_lockstep.json (golden/make_ref_lockstep.py); where it is present, live, and the
record is checked against it too."""
import json

import pytest

from golden_util import GOLDEN, bits_equal, load, scenario_text
from oracle_lib import Oracle, Reference, have_ref
from trajectories import digest

CASES = [("basic", 200), ("block", 150), ("filter", 200), ("weird-edges", 150)]
FIELDS = ("u", "v", "count", "prev_count", "precon")


def recorded(scn):
    with open(GOLDEN + "/ref_lockstep.json") as f:
        return json.load(f)["cases"][scn]


@pytest.mark.parametrize("scn,frames", CASES)
def test_lockstep(tmp_path, scn, frames):
    g = load(scn + "_frames.npz")
    path = tmp_path / (scn + ".txt")
    path.write_text(scenario_text(g))
    rec = recorded(scn)
    assert len(rec) >= frames
    ref = Reference().init(str(path)) if have_ref() else None
    o = Oracle(100, 40).load_file(str(path))
    for f in range(frames):
        o.step()
        if ref is not None:
            ref.step()
            for n in FIELDS:
                assert bits_equal(getattr(ref, n), getattr(o, n)), (scn, f, n)
            assert bits_equal(ref.markers, o.markers), (scn, f)
            assert all(digest(getattr(ref, n)) == rec[f][n] for n in FIELDS + ("markers",)), ("the record is not the reference's", scn, f)
        for n in FIELDS:
            assert digest(getattr(o, n)) == rec[f][n], (scn, f, n)
        assert digest(o.markers) == rec[f]["markers"], (scn, f)
