"""The three observer passes taking turns on ONE handle (docs/observer_passes.md): they share the row loader, the entry checks and the device
buffer type, and every other GPU test runs them one pass at a time.  Each result against its numpy reference with no field left out, a second
round bit for bit the first, and the handle's device memory at the end: the record, the largest overview and the largest raster asked for."""
import numpy as np
import pytest

import diagnostics_ref as dref
import euler_amd as ea
import overview_ref as ref
import viewport_ref as vref
from golden_util import load, scenario_text
from observer_util import read_back

pytestmark = pytest.mark.gpu

WINDOW = (98, 60)      # euler_render_view: the whole interior at or below one cell per glyph, the box across x = 64 at scale 2, one cell at scale 16


@pytest.mark.parametrize("size", [(70, 45), (72, 45)])      # X % 4 != 0: one cell per lane; X % 4 == 0: four
def test_the_passes_take_turns_on_one_handle(size):
    Xg, Yg = size
    sim = ea.Simulation(Xg, Yg, dot_mode=ea.DOT_SEQUENTIAL, rainbow=True).load_text(scenario_text(load("block_frames.npz")), upscale=True)
    for _ in range(5):
        sim.step()
    state = read_back(sim, True)
    terms = dref.cell_terms(state[0], state[2], state[3], state[4])
    markers = sim.get(ea.F_MARKERS)
    assert (state[2] > 0).any() and max(np.abs(state[3]).max(), np.abs(state[4]).max()) > 0 and max(float(d.max()) for d in state[5]) > 0      # water, motion, dye
    # one cell; the whole interior (the buffers grow, and are kept by the smaller box behind it); x0 % 4 = 1, x1 % 4 = 2 across the tile-column edge x = 64
    boxes = [(35, 20, 35, 20), (1, 1, Xg - 2, Yg - 2), (57, 7, 66, 30)]
    before = sim.hbm_bytes()
    records, pixels = [], []      # W * H of every overview and every raster asked for
    rounds = []
    for _ in range(2):
        got_all = []
        for box in boxes:
            bw, bh = box[2] - box[0] + 1, box[3] - box[1] + 1
            shapes = sorted({(max(1, bw // 3), max(1, bh // 2)), (bw, bh)})      # w < Bw, h < Bh (where the box has more than one cell), and one cell per record
            for (w, h) in shapes:      # a rotation per shape: record, overview, raster, frame
                d = sim.diagnostics_record(box)
                assert not dref.mismatches(d, dref.reduce_box(terms, box)), (box, "diagnostics")
                px = sim.overview(w, h, box=box)
                want_px = vref.overview_box_ref(*state, box, w, h)
                assert px.shape == (h, w) and not ref.mismatches(px, want_px), (box, w, h, ref.mismatches(px, want_px))
                ras = sim.marker_raster(box, 2)
                want_ras = vref.raster_ref(markers, box, 2)
                assert ras.shape == want_ras.shape and np.array_equal(ras, want_ras), (box, "raster")
                s = vref.view_zoom(bw, bh, *WINDOW)
                text = sim.render_view(box, *WINDOW)
                vw, vh = (bw, bh) if s else (min(WINDOW[0], bw), min(WINDOW[1], bh))
                cells = vref.overview_box_ref(*state, box, vw, vh).astype(ea.OVERVIEW_DTYPE)
                want_text = ea.view_text(cells, vref.raster_ref(markers, box, s), s, rainbow=True) if s else ea.overview_text(cells, rainbow=True)
                assert text == want_text, (box, "render_view", s)
                records += [w * h, vw * vh]
                pixels += [4 * bw * bh, s * s * bw * bh]
                got_all += [d.tobytes(), px.tobytes(), ras.tobytes(), text]
        rounds.append(got_all)
    assert rounds[0] == rounds[1]
    assert [vref.view_zoom(b[2] - b[0] + 1, b[3] - b[1] + 1, *WINDOW) for b in boxes] == [16, 0, 2]
    assert sim.hbm_bytes() == before + 88 + 48 * max(records) + 4 * max(pixels)
    sim.close()
