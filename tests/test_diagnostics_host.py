"""The host half of the flow diagnostics (docs/diagnostics.md), no GPU: the numpy restatement (tests/diagnostics_ref.py) against its own plain-loop
twin on random grids and planted values, euler_diag_derive against Python doubles, and the record's layout against the header."""
import os
import subprocess

import numpy as np
import pytest

import diagnostics_ref as ref
import euler_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, Y = 37, 23


def random_state(seed, shape=(Y, X)):
    rng = np.random.default_rng(seed)
    solid = (rng.random(shape) < 0.2).astype(np.uint8)
    count = np.where(rng.random(shape) < 0.6, rng.integers(0, 13, shape), 0).astype(np.uint8)
    u, v = (rng.standard_normal(shape).astype(np.float32) * 3 for _ in range(2))
    return solid, count, u, v


@pytest.mark.parametrize("seed", range(4))
def test_vectorised_restatement_is_the_loop_restatement(seed):
    st = random_state(seed)
    terms = ref.cell_terms(*st)
    for box in ref.boxes(X, Y, seed, 6):
        got, want = ref.reduce_box(terms, box), ref.diag_loop(*st, box)
        assert not ref.mismatches(got, want), (box, ref.mismatches(got, want))
    whole = ref.diag_ref(*st)
    assert whole["cells"] == (X - 2) * (Y - 2) and 0 < whole["fluid"] < whole["cells"] and whole["crowded"] > 0 and whole["nonfinite"] == 0
    assert whole["markers"] > whole["fluid"] and whole["div_l1"] > 0 and whole["ke_hi"] > 0 and whole["max_div"] > 0


def test_planted_values():
    """a NaN is counted once and adds nothing, infinities and 1e30 saturate the sums and show in the maxima, count 255 does not wrap anything"""
    solid, count, u, v = random_state(11)
    solid[:] = 0
    count[:] = 4
    u[:] = 0; v[:] = 0
    base = ref.diag_ref(solid, count, u, v)
    assert base["fluid"] == base["cells"] and base["div_l1"] == 0 and base["ke_lo"] == 0 and base["max_div"] == 0 and base["crowded"] == 0
    u[5, 7] = np.nan                       # cells (7, 5) and (8, 5): d and s2 both NaN, each counted once
    r = ref.diag_ref(solid, count, u, v)
    assert r["nonfinite"] == 2 and r["div_l1"] == 0 and r["ke_hi"] == 0 and r["ke_lo"] == 0 and r["max_div"] == 0 and r["max_speed2"] == 0
    u[9, 20] = np.inf                      # d = +-inf on two cells: 256 each; s2 = inf: 2^24 each
    r = ref.diag_ref(solid, count, u, v)
    assert r["nonfinite"] == 2 and r["div_l1"] == 2 * 256 * 2 ** 24 and r["ke_hi"] == 2 * 2 ** 24 and r["ke_lo"] == 0
    assert np.isinf(r["max_div"]) and np.isinf(r["max_speed2"])
    u[9, 21] = -np.inf                     # cell (21, 9): u[i] - u[i-1] = -inf - inf = -inf, (u[i] + u[i-1]) / 2 = NaN: d counts, s2 does not, the cell is non-finite
    r = ref.diag_ref(solid, count, u, v)
    assert r["nonfinite"] == 3 and r["div_l1"] == 3 * 256 * 2 ** 24 and r["ke_hi"] == 2 * 2 ** 24
    u[9, 20] = u[9, 21] = 0
    v[14, 3] = 1e30                        # |d| = 1e30 saturates at 256; s2 = (5e29)^2 overflows float32 to inf
    r = ref.diag_ref(solid, count, u, v)
    assert r["div_l1"] == 2 * 256 * 2 ** 24 and r["max_div"] == np.float32(1e30) and np.isinf(r["max_speed2"]) and r["nonfinite"] == 2
    v[14, 3] = 3.0                         # finite: d = 3, -3; dy = 1.5: qk(2.25) = 2.25 * 2^32 on two cells
    r = ref.diag_ref(solid, count, u, v)
    assert r["div_l1"] == 2 * 3 * 2 ** 24 and r["ke_hi"] == 4 and r["ke_lo"] == 2 ** 31 and r["max_speed2"] == np.float32(2.25)
    count[2, 2] = 255; count[3, 3] = 8; count[4, 4] = 7
    r = ref.diag_ref(solid, count, u, v)
    assert r["count_max"] == 255 and r["crowded"] == 2 and r["markers"] == base["markers"] + 251 + 4 + 3
    for box in (None, (1, 1, 10, 10), (7, 5, 8, 5), (3, 14, 3, 14)):
        assert not ref.mismatches(ref.diag_ref(solid, count, u, v, box), ref.diag_loop(solid, count, u, v, box)), box
    solid[:] = 1                           # no fluid at all
    r = ref.diag_ref(solid, count, u, v)
    assert r["cells"] == base["cells"] and all(r[n] == 0 for n in ref.DTYPE.names[1:])


def test_derive_against_python_doubles():
    recs = [ref.diag_ref(*random_state(s)) for s in range(3)]
    big = np.zeros((), ref.DTYPE)            # sums near the top of their range
    big["fluid"], big["markers"], big["crowded"] = 2 ** 28 - 5, 255 * (2 ** 28 - 5), 12345
    big["mass_x"], big["mass_y"], big["div_l1"], big["ke_hi"], big["ke_lo"] = 2 ** 60 - 3, 2 ** 59 + 7, 2 ** 60 + 1, 2 ** 52 - 1, 2 ** 60 - 11
    empty = np.zeros((), ref.DTYPE)
    empty["cells"] = 1000
    empty["div_l1"] = 77                     # (cannot come from the device: all the derived values are still 0)
    for r in recs + [big, empty]:
        got, want = ea.diag_derive(r), ref.derive(r)
        assert set(got) == set(ea.DIAG_VALUES) == set(want)
        for k in want:
            assert got[k] == want[k], (k, got[k], want[k])
    assert all(v == 0.0 for v in ea.diag_derive(empty).values())
    assert ref.derive(recs[0])["markers_per_cell"] > 1 and 1 < ref.derive(recs[0])["com_x"] < X - 2
    L = ea.load_library()
    assert L.euler_diag_derive(None, np.zeros(6).ctypes.data) == -1 and L.euler_diag_derive(empty.ctypes.data, None) == -1


def test_dtype_is_the_struct(tmp_path):
    d = ea.DIAG_DTYPE
    assert d.itemsize == 88 and d == ref.DTYPE and ea.DIAG_CROWDED == ref.CROWDED == 8
    src = tmp_path / "layout.c"
    fields = list(d.names)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "euler.h"\nint main(void) {\n  printf("%zu %zu %d", sizeof(euler_diag), sizeof(euler_diag_values), (int)EULER_DIAG_CROWDED);\n'
                   + "".join('  printf(" %%zu", offsetof(euler_diag, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    assert out[:3] == [88, 8 * len(ea.DIAG_VALUES), 8]
    assert out[3:] == [d.fields[f][1] for f in fields] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80, 84]
    assert [d.fields[f][0] for f in fields] == [np.uint64] * 9 + [np.uint32, np.uint32, np.float32, np.float32]
