"""The host half of the whole-domain overview (docs/overview.md), no GPU: euler_overview_text / euler_overview_rgb / write_ppm over records
that the numpy restatement (tests/overview_ref.py) forms from states of the five scenarios stepped by the CPU oracle and from random grids."""
import re

import numpy as np
import pytest

import euler_amd as ea
import overview_ref as ref
from golden_util import SCENARIOS, X, Y, load, scenario_text
from oracle_lib import Oracle

EULER_EINVAL = -1
ESC = re.compile(rb"\x1b\[38;2;(\d+);(\d+);(\d+)m")


def oracle_state(scn, frames=30, rainbow=True):
    o = Oracle(X, Y, rainbow=rainbow).load_text(scenario_text(load(scn + "_frames.npz")))
    for _ in range(frames):
        o.step()
    dye = tuple(np.array(q) for q in (o.cr, o.cg, o.cb)) if rainbow else None
    return tuple(np.array(a) for a in (o.solid, o.sink, o.count, o.u, o.v)) + (dye,)


def random_state(seed, shape=(Y, X)):
    rng = np.random.default_rng(seed)
    solid = (rng.random(shape) < 0.2).astype(np.uint8)
    sink = (rng.random(shape) < 0.15).astype(np.uint8)
    count = np.where(rng.random(shape) < 0.6, rng.integers(0, 9, shape), 0).astype(np.uint8)
    u, v = (rng.standard_normal(shape).astype(np.float32) * 3 for _ in range(2))
    dye = tuple(rng.random(shape, dtype=np.float32) for _ in range(3))
    return solid, sink, count, u, v, dye


def states():
    return [(scn, oracle_state(scn)) for scn in SCENARIOS] + [("random%d" % k, random_state(k)) for k in range(3)]


def test_dtype_is_the_struct():
    d = ea.OVERVIEW_DTYPE
    assert d.itemsize == 48 and d == ref.DTYPE
    assert [d.fields[n][1] for n in ("cells", "solid", "sink", "water", "marks", "max_speed2", "dye")] == [0, 4, 8, 12, 16, 20, 24]
    assert d.fields["max_speed2"][0] == np.float32 and d.fields["dye"][0].shape == (3,) and d.fields["dye"][0].base == np.uint64


@pytest.mark.parametrize("name,st", states(), ids=lambda v: v if isinstance(v, str) else "")
def test_text_at_one_cell_per_pixel_is_the_frame_formatter(name, st):
    solid, sink, count, u, v, dye = st
    px = ref.overview_ref(solid, sink, count, u, v, None, X - 2, Y - 2)
    assert (px["cells"] == 1).all()
    assert ea.overview_text(px) == ea.render_grids(solid, sink, count, X - 2, Y - 2), name
    # with the dye: the same glyphs and line structure, every colour byte within 1 (q truncates to 24 bits)
    pxd = ref.overview_ref(solid, sink, count, u, v, dye, X - 2, Y - 2)
    got, want = ea.overview_text(pxd, rainbow=True), ea.render_grids(solid, sink, count, X - 2, Y - 2, rgb=dye)
    assert ESC.sub(b"", got) == ESC.sub(b"", want), name
    cg, cw = np.array(ESC.findall(got), np.int64), np.array(ESC.findall(want), np.int64)
    assert cg.shape == cw.shape and len(cg) > 0 and np.abs(cg - cw).max() <= 1, name


def _rec(cells, solid=0, sink=0, water=0, marks=0):
    px = np.zeros((1, 1), ea.OVERVIEW_DTYPE)
    px["cells"], px["solid"], px["sink"], px["water"], px["marks"] = cells, solid, sink, water, marks
    return px


def _glyph(px):
    t = ea.overview_text(px)
    return re.sub(rb"\x1b\[[0-9;]*[mK]", b"", t)


def test_class_rule_on_hand_made_records():
    assert _glyph(_rec(64, solid=32, water=32, marks=96)) == b"X"        # a tie goes to solid
    assert _glyph(_rec(64, solid=31, water=33, marks=99)) == b"0"
    assert _glyph(_rec(64, sink=40, water=24, marks=72)) == b"="        # a sink-majority box
    assert _glyph(_rec(64, sink=32, water=32, marks=96)) == b"="        # sink >= open
    assert _glyph(_rec(64, sink=31, water=33, marks=99)) == b"0"
    assert _glyph(_rec(64, water=1, marks=1)) == b"o"                   # one marker in a 64-cell box still shows
    assert _glyph(_rec(64, water=64, marks=192)) == b"0"                # marks = 3 * open
    assert _glyph(_rec(64, water=64, marks=128)) == b"O"
    assert _glyph(_rec(64, water=64, marks=129)) == b"0"                # rounds up
    assert _glyph(_rec(64)) == b" "
    assert _glyph(_rec(10, solid=4, sink=3, water=3, marks=3)) == b"="   # open = 3, sink = 3
    assert _glyph(_rec(10, solid=4, sink=2, water=4, marks=4)) == b"o"
    for st in (random_state(5), random_state(6)):
        px = ref.overview_ref(*st[:5], None, 33, 13)
        want = ref.class_ref(px)
        rows = [_r for _r in re.sub(rb"\x1b\[[0-9;]*[mK]", b"", ea.overview_text(px)).split(b"\r\n")]
        assert len(rows) == 13
        table = {0: b" ", 1: b"o", 2: b"O", 3: b"0", 4: b"X", 5: b"="}
        for py in range(13):
            assert rows[py] == b"".join(table[int(k)] for k in want[py]), py


@pytest.mark.parametrize("shape", [(98, 38), (49, 19), (33, 13), (7, 5), (1, 1)])
def test_rgb_against_the_restatement(shape):
    w, h = shape
    for name, st in states():
        px = ref.overview_ref(*st[:5], st[5], w, h)
        got = ea.overview_rgb(px)
        assert got.shape == (h, w, 3) and got.dtype == np.uint8
        assert np.array_equal(got, ref.rgb_ref(px, ref.COVERAGE)), name                     # integers only: exact
        for mode, scale in ((ea.IMAGE_DYE, 1.0), (ea.IMAGE_SPEED, 4.0), (ea.IMAGE_SPEED, 0.25)):
            got = ea.overview_rgb(px, mode, scale).astype(np.int64)
            want = ref.rgb_ref(px, mode, scale).astype(np.int64)
            assert np.abs(got - want).max() <= 1, (name, mode, scale)                          # host powf / sqrtf against numpy's
    nodye = ref.overview_ref(*oracle_state("basic", 10, rainbow=False)[:5], None, w, h)
    assert np.array_equal(ea.overview_rgb(nodye, ea.IMAGE_DYE), ref.rgb_ref(nodye, ref.DYE))   # black water


def test_rgb_refusals():
    px = ref.overview_ref(*random_state(1)[:5], None, 7, 5)
    L = ea.load_library()
    rgb = np.zeros((5, 7, 3), np.uint8)
    ok = lambda mode, scale, nbytes=rgb.nbytes, w=7, h=5: L.euler_overview_rgb(px.ctypes.data, w, h, mode, scale, rgb.ctypes.data, nbytes)
    assert ok(ea.IMAGE_COVERAGE, 0.0) == 0 and ok(ea.IMAGE_DYE, float("nan")) == 0 and ok(ea.IMAGE_SPEED, 1.0) == 0
    for mode in (3, -1, 99):
        assert ok(mode, 1.0) == EULER_EINVAL
    for scale in (0.0, -1.0, float("nan")):
        assert ok(ea.IMAGE_SPEED, scale) == EULER_EINVAL
    assert ok(ea.IMAGE_COVERAGE, 1.0, rgb.nbytes - 1) == EULER_EINVAL and ok(ea.IMAGE_COVERAGE, 1.0, rgb.nbytes + 3) == EULER_EINVAL
    assert ok(ea.IMAGE_COVERAGE, 1.0, 0, 0, 5) == EULER_EINVAL
    with pytest.raises(ea.EulerError) as e:
        ea.overview_rgb(px, 7)
    assert e.value.code == EULER_EINVAL
    n = ea.C.c_int32(0)
    assert L.euler_overview_text(px.ctypes.data, 0, 5, 0, None, 0, ea.C.byref(n)) == EULER_EINVAL


def test_text_sizing_protocol():
    px = ref.overview_ref(*random_state(2)[:5], None, 20, 10)
    L = ea.load_library()
    n = ea.C.c_int32(0)
    assert L.euler_overview_text(px.ctypes.data, 20, 10, 0, None, 0, ea.C.byref(n)) == 0 and n.value > 0
    full = ea.overview_text(px)
    assert len(full) == n.value
    buf = ea.C.create_string_buffer(b"#" * 64, 64)
    assert L.euler_overview_text(px.ctypes.data, 20, 10, 0, buf, 16, ea.C.byref(n)) == 0 and n.value == len(full)
    assert buf.raw[:16] == full[:16] and buf.raw[16:] == b"#" * 48


def test_write_ppm_round_trip(tmp_path):
    px = ref.overview_ref(*random_state(3), 33, 13)
    rgb = ea.overview_rgb(px, ea.IMAGE_DYE)
    path = tmp_path / "f.ppm"
    ea.write_ppm(str(path), rgb)
    raw = path.read_bytes()
    assert raw.startswith(b"P6\n33 13\n255\n")
    body = raw[len(b"P6\n33 13\n255\n"):]
    assert len(body) == 33 * 13 * 3 and np.array_equal(np.frombuffer(body, np.uint8).reshape(13, 33, 3), rgb)
    with pytest.raises(ValueError):
        ea.write_ppm(str(path), np.zeros((4, 4), np.uint8))
