"""The test-side restatement of the MacCormack transport (tests/c/advect_maccormack.c, tests/advect_maccormack_ref.py), pinned on the
CPU before any GPU test relies on it:
  - with the correction bypassed it is advect_rk2_ref's stages bit for bit (RK1 and RK2), and the composed frame is advect_rk2_ref.step;
  - every corrected value lies within its own limiter bounds;
  - a smooth bump carried through an all-fluid box: MacCormack is second order, the semi-Lagrangian step first order.
"""
import math

import numpy as np
import pytest

import advect_maccormack_ref as ref
import advect_rk2_ref as rk2ref
from golden_util import SCENARIOS, X, Y, bits_equal, load, scenario_text
from oracle_lib import Oracle
from test_advect_rk2_host import substep_oracle


@pytest.fixture(scope="module")
def am(tmp_path_factory):
    return ref.build(tmp_path_factory.mktemp("advect_maccormack"))


def _golden_with_dye(scn):
    g = load(scn + "_substep.npz")
    o = substep_oracle(g, rainbow=True)
    o.lib.eo_colorize(o.ptr)
    return o, float(g["dt"])


@pytest.mark.parametrize("rk2", [0, 1])
@pytest.mark.parametrize("scn", SCENARIOS)
def test_without_the_correction_it_is_advect_rk2_ref(am, scn, rk2):
    o, dt = _golden_with_dye(scn)
    for ours, theirs in ((ref.advect_u, am.ar_advect_u), (ref.advect_v, am.ar_advect_v)):
        want = np.full((Y, X), 7.0, np.float32)
        got = want.copy()
        theirs(ref._p(o), o.f32p(o.u), o.f32p(o.v), ref.C.c_float(dt), o.f32p(want), rk2)
        ours(am, o, o.u, o.v, dt, got, rk2, 0)
        assert bits_equal(got, want), (scn, rk2)
    for q in (o.cr, o.cg, o.cb):
        want_t = np.full((Y, X), 7.0, np.float32)
        am.ar_advect_p(ref._p(o), o.f32p(q), o.f32p(o.u), o.f32p(o.v), ref.C.c_float(dt), o.f32p(want_t), rk2)
        got_q, got_t = q.copy(), np.full((Y, X), 7.0, np.float32)
        ref.advect_p(am, o, got_q, o.u, o.v, dt, got_t, rk2, 0)
        assert bits_equal(got_t, want_t) and bits_equal(got_q, want_t), (scn, rk2, "dye")


@pytest.mark.parametrize("scn", ["block", "waterfall"])
def test_composed_frame_without_the_correction_is_rk2_step(am, scn):
    text = scenario_text(load(scn + "_frames.npz"))
    for rk2 in (0, 1):
        a = Oracle(X, Y, rainbow=True).load_text(text)
        b = Oracle(X, Y, rainbow=True).load_text(text)
        for f in range(10):
            na = rk2ref.step(am, a, rk2)
            nb = ref.step(am, b, rk2, 0)
            assert na == nb, (scn, rk2, f)
            for n in ("u", "v", "cr", "cg", "cb", "markers"):
                assert bits_equal(getattr(a, n), getattr(b, n)), (scn, rk2, f, n)


def test_the_correction_changes_the_frame(am):
    text = scenario_text(load("basic_frames.npz"))
    a = Oracle(X, Y, rainbow=True).load_text(text)
    b = Oracle(X, Y, rainbow=True).load_text(text)
    for f in range(10):
        ref.step(am, a, 0, 0)
        ref.step(am, b, 0, 1)
    assert not bits_equal(a.u, b.u) and not bits_equal(a.v, b.v) and not bits_equal(a.cr, b.cr)
    assert np.isfinite(b.u).all() and np.isfinite(b.v).all() and np.isfinite(b.cr).all()


def _check_limits(out, lo, hi, what):
    sel = ~np.isnan(lo)
    assert sel.sum() > 0, what
    ok = np.isinf(lo[sel]) | ((out[sel] >= lo[sel]) & (out[sel] <= hi[sel]))
    assert ok.all(), (what, int((~ok).sum()))


def _limits_on(am, o, dt, rk2, what):
    for fn, q in ((ref.advect_u, o.u), (ref.advect_v, o.v)):
        out = np.zeros((o.c.Y, o.c.X), np.float32)
        lo, hi = np.empty_like(out), np.empty_like(out)
        fn(am, o, o.u, o.v, dt, out, rk2, 1, lo, hi)
        _check_limits(out, lo, hi, what)
    if o.c.rainbow:
        for q in (o.cr, o.cg, o.cb):
            qq, t = q.copy(), np.zeros_like(q)
            lo, hi = np.empty_like(q), np.empty_like(q)
            ref.advect_p(am, o, qq, o.u, o.v, dt, t, rk2, 1, lo, hi)
            _check_limits(qq, lo, hi, what + " dye")


@pytest.mark.parametrize("scn", SCENARIOS)
def test_limiter_keeps_every_value_within_its_stencil(am, scn):
    o, dt = _golden_with_dye(scn)
    for rk2 in (0, 1):
        _limits_on(am, o, dt, rk2, scn)


def test_limiter_on_random_masks(am):
    rng = np.random.default_rng(7)
    n = 40
    for trial in range(4):
        o = Oracle(n, n, rainbow=True)
        count = (rng.random((n, n)) < 0.7).astype(np.uint8)
        count[0, :] = count[-1, :] = count[:, 0] = count[:, -1] = 0
        o.count[...] = count; o.prev_count[...] = count
        o.solid[...] = (rng.random((n, n)) < 0.1).astype(np.uint8) * (1 - count)
        o.u[...] = rng.standard_normal((n, n)).astype(np.float32)
        o.v[...] = rng.standard_normal((n, n)).astype(np.float32)
        for q in (o.cr, o.cg, o.cb):
            q[...] = rng.random((n, n)).astype(np.float32)
        _limits_on(am, o, 0.3, trial & 1, "random %d" % trial)


def _box(n):
    u, v, count, sink = ref.translation_box(n)
    o = Oracle(n, n)
    o.u[...] = u; o.v[...] = v; o.count[...] = count; o.prev_count[...] = count; o.sink[...] = sink
    return o


def _dye_run(am, n, mc):
    o = _box(n)
    q, tmp = ref.bump(n).astype(np.float32), np.zeros((n, n), np.float32)
    steps = 40 * n // 64
    for _ in range(steps):
        ref.advect_p(am, o, q, o.u, o.v, 1.0, tmp, 0, mc)
    return ref.rel_l2(q, ref.bump(n, steps)), float(q.max()), float(q.min())


def _vel_run(am, n, mc):
    o = _box(n)
    v = ref.vbump(n).astype(np.float32)
    out = v.copy()
    steps = 40 * n // 64
    for _ in range(steps):
        ref.advect_v(am, o, o.u, v, 1.0, out, 0, mc)
        v = out.copy()
    sl = (slice(2, n - 3), slice(2, n - 2))
    return ref.rel_l2(v[sl] - ref.TR_VEL[1], ref.vbump(n, steps)[sl] - ref.TR_VEL[1])


def test_translation_accuracy_dye(am):
    """measured on this restatement: semi-Lagrangian 0.264 / 0.153 (order 0.79), MacCormack 0.062 / 0.016 (order 1.96), peak 0.963 / 0.990"""
    sl64, _, _ = _dye_run(am, 64, 0)
    sl128, _, _ = _dye_run(am, 128, 0)
    mc64, pk64, mn64 = _dye_run(am, 64, 1)
    mc128, pk128, mn128 = _dye_run(am, 128, 1)
    assert mc64 <= 0.35 * sl64 and mc128 <= 0.35 * sl128, (mc64, sl64, mc128, sl128)
    assert math.log2(mc64 / mc128) >= 1.6, (mc64, mc128)
    assert math.log2(sl64 / sl128) <= 1.2, (sl64, sl128)
    assert pk64 >= 0.9 and pk128 >= 0.9 and mn64 >= 0.0 and mn128 >= 0.0


def test_translation_accuracy_velocity(am):
    """uniform flow with a bump in v (in x alone): measured 0.187 -> 0.049 at 64², 0.107 -> 0.013 at 128²"""
    for n in (64, 128):
        sl, mc = _vel_run(am, n, 0), _vel_run(am, n, 1)
        assert mc <= 0.5 * sl, (n, mc, sl)
