"""The host half of the flow raster (docs/flow_raster.md), no GPU: euler_flow_paint against its numpy restatement (tests/flow_ref.py) on random records
and its edge cases, its composition with the existing formatters over records of the five scenarios stepped by the CPU oracle, every refusal, and the
record's dtype."""
import re

import numpy as np
import pytest

import euler_amd as ea
import flow_ref as fref
import overview_ref as ref
from golden_util import SCENARIOS, X, Y, load, scenario_text
from oracle_lib import Oracle

EULER_EINVAL = -1
ESC = re.compile(rb"\x1b\[38;2;(\d+);(\d+);(\d+)m")
FIELDS = (ea.PAINT_VORTICITY, ea.PAINT_PRESSURE, ea.PAINT_SPEED)


def oracle_records(scn, w, h, frames=30):
    o = Oracle(X, Y).load_text(scenario_text(load(scn + "_frames.npz")))
    for _ in range(frames):
        o.step()
    g = [np.array(a) for a in (o.solid, o.sink, o.count, o.u, o.v)]
    flow = fref.flow_ref(*g, (1, 1, X - 2, Y - 2), w, h, p=np.array(o.p))
    return g, flow.astype(ea.FLOW_DTYPE), ref.overview_ref(*g, None, w, h).astype(ea.OVERVIEW_DTYPE)


def random_records(seed, shape=(9, 13)):
    rng = np.random.default_rng(seed)
    flow = np.zeros(shape, ea.FLOW_DTYPE)
    flow["cells"] = rng.integers(1, 5000, shape)
    flow["water"] = (rng.random(shape) < 0.8) * rng.integers(1, 5000, shape).clip(None, flow["cells"])
    flow["nodes"] = (rng.random(shape) < 0.8) * (rng.random(shape) * flow["water"]).astype(np.uint32)
    for n in ("u_pos", "u_neg", "v_pos", "v_neg", "w_pos", "w_neg", "p_sum"):
        flow[n] = (rng.random(shape) * rng.choice([1 << 10, 1 << 22, 1 << 34, 1 << 44], shape) * np.maximum(flow["water"], 1)).astype(np.uint64)
    px = np.zeros(shape, ea.OVERVIEW_DTYPE)
    px["cells"], px["water"] = flow["cells"], flow["water"]
    px["solid"] = flow["cells"] - flow["water"]
    px["marks"] = flow["water"] * 2
    px["max_speed2"] = rng.random(shape, dtype=np.float32)
    px["dye"] = rng.integers(0, 1 << 40, shape + (3,))
    return flow, px


def same_but_dye(a, b):
    return all(np.array_equal(a[n], b[n]) for n in ea.OVERVIEW_DTYPE.names if n != "dye")


def test_dtype_is_the_struct():
    d = ea.FLOW_DTYPE
    assert d.itemsize == 88 and d == fref.DTYPE
    names = ["cells", "water", "nodes", "nonfinite", "u_pos", "u_neg", "v_pos", "v_neg", "w_pos", "w_neg", "p_sum", "max_speed2", "max_abs_w", "max_p", "reserved"]
    assert list(d.names) == names
    assert [d.fields[n][1] for n in names] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80, 84]
    assert [d.fields[n][0] for n in names] == [np.uint32] * 4 + [np.uint64] * 7 + [np.float32] * 3 + [np.uint32]
    assert (ea.FLOW_PRESSURE, ea.PAINT_VORTICITY, ea.PAINT_PRESSURE, ea.PAINT_SPEED) == (1, 0, 1, 2)


@pytest.mark.parametrize("seed", range(4))
def test_paint_against_the_restatement_on_random_records(seed):
    flow, px = random_records(seed)
    assert (flow["water"] == 0).any() and ((flow["nodes"] == 0) & (flow["water"] > 0)).any()
    for field in FIELDS:
        for scale in (1.0, 0.37, 1000.0, 1e-6, 3e7):
            got = ea.flow_paint(flow, px, field, scale)
            want = fref.paint_ref(flow, px, field, scale)
            assert same_but_dye(got, px)
            assert np.array_equal(got["dye"], want["dye"]), (field, scale)
    assert (ea.flow_paint(flow, px, ea.PAINT_SPEED, 1.0)["dye"][flow["water"] == 0] == 0).all()


def _one(water=10, nodes=10, **sums):
    flow = np.zeros((1, 1), ea.FLOW_DTYPE)
    flow["cells"], flow["water"], flow["nodes"] = 16, water, nodes
    for n, v in sums.items():
        flow[n] = v
    px = np.zeros((1, 1), ea.OVERVIEW_DTYPE)
    px["cells"], px["water"], px["marks"] = 16, water, 3 * water
    px["dye"] = 12345
    return flow, px


def test_paint_edge_cases():
    one = 1 << 24
    q = lambda flow, px, field, scale: [int(v) for v in ea.flow_paint(flow, px, field, scale)["dye"][0, 0]]
    # nodes == 0: the mean vorticity is 0, white
    flow, px = _one(nodes=0, w_pos=5 << 20)
    assert q(flow, px, ea.PAINT_VORTICITY, 1.0) == [10 * one] * 3
    # water == 0: nothing to colour
    flow, px = _one(water=0, nodes=0)
    for field in FIELDS:
        assert q(flow, px, field, 1.0) == [0, 0, 0]
    # t exactly +1, -1 and 0
    flow, px = _one(w_pos=20 << 20)      # mean 2, scale 2
    assert q(flow, px, ea.PAINT_VORTICITY, 2.0) == [10 * one, 0, 0]
    flow, px = _one(w_neg=20 << 20)
    assert q(flow, px, ea.PAINT_VORTICITY, 2.0) == [0, 0, 10 * one]
    flow, px = _one(w_pos=7 << 20, w_neg=7 << 20)
    assert q(flow, px, ea.PAINT_VORTICITY, 2.0) == [10 * one] * 3
    flow, px = _one(p_sum=10 * 256 * 8)      # mean 8
    assert q(flow, px, ea.PAINT_PRESSURE, 8.0) == [10 * one, 5 * one, 0]
    assert q(flow, px, ea.PAINT_PRESSURE, 4.0) == [10 * one, 5 * one, 0]      # clamped
    flow, px = _one()
    assert q(flow, px, ea.PAINT_PRESSURE, 8.0) == [0, 5 * one, 10 * one] == q(flow, px, ea.PAINT_SPEED, 1.0)
    flow, px = _one(u_pos=30 << 20, v_neg=40 << 20)      # mean (3, -4): speed 5
    assert q(flow, px, ea.PAINT_SPEED, 5.0) == [10 * one, 5 * one, 0]
    assert q(flow, px, ea.PAINT_SPEED, 10.0) == [5 * one, 5 * one, 5 * one]
    # saturated sums: every cell of a full 2^28-cell grid at the clamp of qv (2^32) and of qp (2^32)
    flow, px = _one(water=1 << 28, nodes=1 << 28, w_neg=1 << 60, u_neg=1 << 60, p_sum=1 << 60)
    flow["cells"] = px["cells"] = 1 << 28
    px["marks"] = 3 << 28
    w = 1 << 28
    assert q(flow, px, ea.PAINT_VORTICITY, 4096.0) == [0, 0, w * one]
    assert q(flow, px, ea.PAINT_VORTICITY, 8192.0) == [w * one // 2, w * one // 2, w * one]
    assert q(flow, px, ea.PAINT_SPEED, 4096.0) == [w * one, w * one // 2, 0]
    assert q(flow, px, ea.PAINT_PRESSURE, 16777216.0) == [w * one, w * one // 2, 0]
    for field in FIELDS:
        assert np.array_equal(ea.flow_paint(flow, px, field, 3.0)["dye"], fref.paint_ref(flow, px, field, 3.0)["dye"])


@pytest.mark.parametrize("scn", SCENARIOS)
def test_painted_records_through_the_existing_formatters(scn):
    """at one cell per pixel: the painted frame is the unpainted one but for the colour escapes, and each escape is the sRGB byte triple of the painted colour"""
    g, flow, px = oracle_records(scn, X - 2, Y - 2)
    assert (flow["water"] > 0).any() and np.array_equal(flow["water"], px["water"]) and np.array_equal(flow["cells"], px["cells"])
    plain = ea.overview_text(px, rainbow=True)
    for field, scale in ((ea.PAINT_VORTICITY, 2.0), (ea.PAINT_PRESSURE, 40.0), (ea.PAINT_SPEED, 5.0)):
        painted = ea.flow_paint(flow, px, field, scale)
        assert same_but_dye(painted, px)
        text = ea.overview_text(painted, rainbow=True)
        assert ESC.sub(b"", text) == ESC.sub(b"", plain), (scn, field)
        assert len(ESC.findall(text)) == len(ESC.findall(plain)) > 0
        want = fref.paint_ref(flow, px, field, scale)
        assert np.array_equal(painted["dye"], want["dye"])
        # the formatters' mean dye is exactly q24(L) / 2^24: the escapes are the bytes of that colour, glyph by glyph in reading order
        glyphs = (ref.class_ref(px) >= 1) & (ref.class_ref(px) <= 3)
        lin = ref.mean_dye(want)[glyphs]
        got = np.array(ESC.findall(text), np.int64)
        assert got.shape == lin.shape and np.abs(got - ref.srgb_bytes(lin)).max() <= 1, (scn, field)      # host powf against numpy's
        # without the rainbow flag the painted records draw as the unpainted ones, and the image formatter shows the field in its dye mode
        assert ea.overview_text(painted) == ea.overview_text(px)
        assert np.abs(ea.overview_rgb(painted, ea.IMAGE_DYE).astype(np.int64) - ref.rgb_ref(want, ref.DYE).astype(np.int64)).max() <= 1
        # and the magnified frame of the viewport
        ras = np.minimum(g[2][Y - 2:0:-1, 1:X - 1], 3).astype(np.uint32)
        assert ESC.sub(b"", ea.view_text(painted, ras, 1, rainbow=True)) == ESC.sub(b"", ea.view_text(px, ras, 1, rainbow=True))
        assert ESC.findall(ea.view_text(painted, ras, 1, rainbow=True)) == ESC.findall(text)


def test_a_field_of_zeros_paints_vorticity_white():
    g, flow, px = oracle_records("basic", X - 2, Y - 2, frames=0)      # the scene at rest: u = v = 0
    assert (flow["water"] > 0).any() and not flow["w_pos"].any() and not flow["w_neg"].any()
    text = ea.overview_text(ea.flow_paint(flow, px, ea.PAINT_VORTICITY, 1.0), rainbow=True)
    assert set(ESC.findall(text)) == {(b"255", b"255", b"255")}


def test_every_refusal():
    flow, px = random_records(7)
    h, w = px.shape
    L = ea.load_library()
    before = px.copy()
    call = lambda f=flow, p=px, w=w, h=h, field=0, scale=1.0: L.euler_flow_paint(f.ctypes.data if f is not None else None, p.ctypes.data if p is not None else None, w, h, field, scale)
    assert call() == 0
    px[...] = before
    assert call(f=None) == EULER_EINVAL and call(p=None) == EULER_EINVAL
    for (ww, hh) in ((0, h), (w, 0), (-1, h), (w, -2)):
        assert call(w=ww, h=hh) == EULER_EINVAL
    for field in (-1, 3, 99):
        assert call(field=field) == EULER_EINVAL
    for scale in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(scale=scale) == EULER_EINVAL, scale
    for name in ("cells", "water"):
        for k in (0, flow.size - 1):      # the mismatch in the last pixel: nothing painted in front of it either
            other = flow.copy()
            other[name].reshape(-1)[k] += 1
            assert call(f=other) == EULER_EINVAL, (name, k)
    assert px.tobytes() == before.tobytes()
    with pytest.raises(ea.EulerError) as e:
        ea.flow_paint(flow, px, 5, 1.0)
    assert e.value.code == EULER_EINVAL
    with pytest.raises(ValueError):
        ea.flow_paint(flow[:3], px, 0, 1.0)
