"""euler_hbm_bytes is the handle's memory ledger's counted bytes (euler_amd/csrc/eu_mem.h, docs/handle_memory.md).  On the GPU: the figure of every handle kind that
never selects a coarse mode is the parent commit's to the byte; the coarse modes report the same figure however the mode was selected, and it holds the multilevel
arrays; thirty handles with every feature that allocates are created, stepped and destroyed.  (That every block is freed exactly once is the host test's:
tests/test_mem_host.py.)"""
import ctypes as C
import threading

import pytest

import euler_amd as ea

pytestmark = pytest.mark.gpu

X, Y = 100, 40

# euler_hbm_bytes at commit b6b3318 ("Share one transport header, flag dispatch and box-table path"), the parent of the ledger, measured on a build of that commit by
# handle_figures() below: 100 x 40 cells
PARENT_FIGURES = {
    "default": 2272239,
    "default, loaded and stepped": 3255279,      # (+ the search directions' ring)
    "rainbow": 2368239,
    "rainbow, loaded and stepped": 3351279,
    "tile-local, loaded": 2272239,
    "tile-local, first step": 3255279,           # (+ the ring)
    "tile-local with tree dots, loaded": 2272239,
    "tile-local with tree dots, first step": 3269167,      # (+ the ring and the halo buffers)
    "maccormack": 2304239,
    "row slab, 1 rank": 2813540,
}


def handle_figures():
    out = {}
    for name, kw in (("default", {}), ("rainbow", dict(rainbow=True))):
        s = ea.Simulation(X, Y, **kw)
        out[name] = s.hbm_bytes()
        s.load_half_tank()
        s.step()
        out[name + ", loaded and stepped"] = s.hbm_bytes()
        s.close()
    s = ea.Simulation(X, Y, precond=ea.PRECOND_IC0_TILE, tile_records=16).load_half_tank()      # (sequential dots at this size: the multi-kernel solve that stores z, with its ring)
    out["tile-local, loaded"] = s.hbm_bytes()
    s.step()
    out["tile-local, first step"] = s.hbm_bytes()
    s.close()
    # tree dots, never the resident kernel: the multi-kernel solve that forms z twice (k_pcg.hip tile_z_begin)
    s = ea.Simulation(X, Y, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, tile_records=16, resident=ea.RESIDENT_OFF).load_half_tank()
    out["tile-local with tree dots, loaded"] = s.hbm_bytes()
    s.step()
    out["tile-local with tree dots, first step"] = s.hbm_bytes()
    s.close()
    s = ea.Simulation(X, Y)
    s.set_option(ea.OPT_ADVECT_MACCORMACK, 1)
    out["maccormack"] = s.hbm_bytes()
    s.close()
    s = ea.Simulation(X, Y, slab=(0, 1))
    out["row slab, 1 rank"] = s.hbm_bytes()
    s.close()
    return out


def test_handles_without_a_coarse_mode_report_the_parents_bytes():
    got = handle_figures()
    print(got)
    assert got == PARENT_FIGURES
    nbands, T = (Y + 63) // 64, (X + 63 + 95) // 96 * 96      # (euler_create's records per band)
    halo = (nbands * (T // 16) * 128 + nbands * 2 * X) * 8      # zhalo + zrows (k_pcg.hip tile_z_begin)
    assert got["tile-local, first step"] > got["tile-local, loaded"]      # the ring did come with the first solve
    assert got["tile-local with tree dots, first step"] - got["tile-local with tree dots, loaded"] == got["tile-local, first step"] - got["tile-local, loaded"] + halo
    assert got["maccormack"] == got["default"] + 2 * X * Y * 4


def mg_array_bytes(nx_cells, ny_cells):
    """mg_a [9] + mg_rhs [3] + mg_null0 [4] doubles per node of every level (k_mg.hip eu_mg_alloc), from eu_mg_levels' level sizes"""
    L = ea.load_library()
    i32 = C.c_int32
    L.eu_mg_levels.argtypes, L.eu_mg_levels.restype = [i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_size_t)], C.c_int
    nx, ny, off = (i32 * 12)(), (i32 * 12)(), (C.c_size_t * 12)()
    n = L.eu_mg_levels(nx_cells, (ny_cells + 63) // 64, nx, ny, off)
    assert n >= 1
    cells = off[n - 1] + nx[n - 1] * ny[n - 1]
    assert cells == sum(nx[l] * ny[l] for l in range(n))
    return (9 + 3 + 4) * cells * 8


# the smallest grids on which tests/test_gpu_tile_precond.py runs each mode
@pytest.mark.parametrize("mode,gx,gy", [(ea.PRECOND_IC0_TILE2, 260, 300), (ea.PRECOND_IC0_TILE_MG, 100, 40)])
def test_a_coarse_mode_reports_the_same_bytes_however_it_was_selected(mode, gx, gy):
    plain = ea.Simulation(gx, gy, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, tile_records=16)
    base = plain.hbm_bytes()
    created = ea.Simulation(gx, gy, dot_mode=ea.DOT_TREE, precond=mode, tile_records=16)
    want = created.hbm_bytes()
    created.close()
    plain.set_precond(mode, 16)
    print(mode, base, want, plain.hbm_bytes())
    assert plain.hbm_bytes() == want
    plain.set_precond(ea.PRECOND_IC0_TILE, 16)
    plain.set_precond(mode, 16)
    assert plain.hbm_bytes() == want
    plain.close()
    if mode == ea.PRECOND_IC0_TILE_MG:
        assert want - base >= mg_array_bytes(gx, gy)
    else:      # the dense level's factor and its inverse: [n][n] doubles each, n >= MG_TOP_MAX = 64 (k_coarse.hip eu_coarse_alloc)
        assert want - base >= 2 * 64 * 64 * 8


FEATURES = ("force boxes", "heat", "tracers", "gauges", "reseed", "overview", "flow raster", "maccormack")


def _life_cycle(result):
    L = ea.load_library()
    try:
        for k in range(30):
            s = ea.Simulation(X, Y, rainbow=k % 5 == 4).load_half_tank()
            f = FEATURES[k % len(FEATURES)]
            if f == "force boxes":
                s.set_forcing(boxes=[((10, 5, 30, 15), (2.0, 0.0)), ((40, 5, 60, 12), (0.0, 3.0))])
            elif f == "heat":
                s.set_heat(ambient=1.0, beta=0.1, kappa=0.01, boxes=[(ea.HEAT_FIX, 5.0, (10, 2, 20, 6))])
                s.heat_raster(10, 4)
            elif f == "tracers":      # 200, 600, 1400 records: the store's 256 grown to 1024, then to 2048
                for n in (200, 400, 800):
                    s.add_tracers([(5.0 + (j % 80), 3.0 + (j % 15)) for j in range(n)])
                assert s.n_tracers == 1400
                s.tracer_raster(None, 10, 4)
            elif f == "gauges":
                s.gauges([(ea.GAUGE_LEVEL, (1, 1, X - 2, Y - 2)), (ea.GAUGE_PRESSURE, (10, 2, 20, 10)), (ea.GAUGE_FLUX, (50, 1, 50, Y - 2))])
            elif f == "reseed":
                s.set_reseed(thin_above=8, fill_holes=True)
            elif f == "overview":
                s.overview(20, 8)
                s.diagnostics()
            elif f == "flow raster":
                s.flow(20, 8, pressure=True)
                s.marker_raster((10, 5, 29, 14), 2)
            elif f == "maccormack":
                s.set_option(ea.OPT_ADVECT_MACCORMACK, 1)
            s.step()
            assert s.hbm_bytes() > 0
            s.close()
        result["error"] = L.euler_last_error().decode(errors="replace")
    except BaseException as e:      # (reported by the test's own thread)
        result["raised"] = repr(e)


def test_thirty_handles_with_every_feature_are_created_stepped_and_destroyed():
    """Every call returns EULER_OK (the binding raises otherwise) and euler_last_error() is empty at the end.  The error text is per thread and is not cleared by a
    call that succeeds, so the loop runs in a thread of its own: what an earlier test of this process provoked on purpose does not show here."""
    result = {}
    t = threading.Thread(target=_life_cycle, args=(result,))
    t.start()
    t.join()
    assert result == {"error": ""}
