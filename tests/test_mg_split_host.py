"""The host half of the multilevel preconditioner's cycle split by rows (docs/solver_multilevel_row_slabs.md), no GPU: the level dimensions, the entry and the gather
level and the split plan of csrc/euler_host.c - which node rows of which level a rank packs, sends, receives, overwrites and sums - against numpy restatements on
BOOLEAN ROW SETS (no interval formulas) over random partitions, and the same code under the sanitizers in a stand-alone program (tests/c/sanitize_mg_split.c)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import euler_amd as ea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G0, RPB, MAXLEV, TOP_MAX, TAIL_MAX, SMALL_LEVEL0, GATHER_MAX, SETUP_HALO, MAXR = 8, 8, 12, 64, 1024, 16384, 16384, 6, 64      # csrc/euler_host.h
NSEG = 4 * MAXLEV
EULER_EINVAL = -1
i32 = C.c_int32


class Seg(C.Structure):       # eu_mg_seg
    _fields_ = [(n, i32) for n in ("level", "row0", "row1", "off")]


class Plan(C.Structure):      # eu_mg_split_plan
    _fields_ = [("Lg", i32), ("ranks", i32), ("rank", i32), ("I", i32 * 2 * MAXR * MAXLEV), ("O", i32 * 2 * MAXR * MAXLEV), ("NR", i32 * 2 * MAXLEV), ("NX", i32 * 2 * MAXLEV),
                ("zs", i32 * 2 * MAXLEV * 2), ("zr", i32 * 2 * MAXLEV * 2), ("zoff_s", i32 * MAXLEV * 2), ("zoff_r", i32 * MAXLEV * 2), ("zone", i32), ("beyond", i32),
                ("setup_bad", i32), ("aslot", i32), ("win_rows", i32), ("nsmall", i32), ("nseg", i32), ("total", i32), ("overflow", i32), ("seg", Seg * NSEG)]


@pytest.fixture(scope="module")
def L():
    lib = ea.load_library()
    p32 = C.POINTER(i32)
    lib.eu_mg_levels.argtypes, lib.eu_mg_levels.restype = [i32, i32, p32, p32, C.POINTER(C.c_size_t)], C.c_int
    lib.eu_mg_entry_level.argtypes, lib.eu_mg_entry_level.restype = [i32, p32, p32], C.c_int
    lib.eu_mg_gather_level.argtypes, lib.eu_mg_gather_level.restype = [i32, p32, p32, C.c_int64], C.c_int
    lib.eu_mg_split_plan_fill.argtypes, lib.eu_mg_split_plan_fill.restype = [C.POINTER(Plan), i32, p32, p32, i32, i32, i32, p32, p32, i32], C.c_int
    return lib


def levels_of(L, X, nbands):
    nx, ny, off = (i32 * MAXLEV)(), (i32 * MAXLEV)(), (C.c_size_t * MAXLEV)()
    return L.eu_mg_levels(X, nbands, nx, ny, off), nx, ny, off


def plan_of(L, n, nx, ny, Lg, part, rank, seg_cap=NSEG):
    R = len(part)
    P = Plan()
    rc = L.eu_mg_split_plan_fill(C.byref(P), n, nx, ny, Lg, R, rank, (i32 * R)(*[p[0] for p in part]), (i32 * R)(*[p[1] for p in part]), seg_cap)
    return rc, P


def rows(r, n, zone=False):      # a half-open range of the plan as a row set; an empty ZONE is stored as {0, 0}
    lo, hi = r[0], r[1]
    assert 0 <= lo <= hi <= n and (lo < hi or not zone or (lo, hi) == (0, 0)), (lo, hi, n)
    m = np.zeros(n, bool)
    m[lo:hi] = True
    return m


def dilate(m):      # the rows within one row of the set, inside the grid
    d = m.copy()
    d[1:] |= m[:-1]
    d[:-1] |= m[1:]
    return d


def band_rows(lo, hi, ny0, grow):
    m = np.zeros(ny0, bool)
    m[max(RPB * lo - grow, 0):min(RPB * hi + grow, ny0)] = True
    return m


def coarse_around(m, cny):      # mg_coarse_around (k_mg_cycle.hip) on the rows: c.i0 = f.i0 >> 1, c.i1 = ((f.i1 - 1) >> 1) + 2, clipped to the coarse level
    f = np.flatnonzero(m)
    f0, f1 = int(f[0]), int(f[-1]) + 1
    c = np.zeros(cny, bool)
    c[f0 >> 1:min(((f1 - 1) >> 1) + 2, cny)] = True
    return c


def brute(ny, Lg, part):
    """the row sets of every rank: supports I, owned rows O (levels 0 .. Lg), needs NX / NR (levels below Lg)"""
    R = len(part)
    I, O, NX, NR = [[None] * R for _ in range(Lg + 1)], [[None] * R for _ in range(Lg + 1)], [[None] * R for _ in range(Lg)], [[None] * R for _ in range(Lg)]
    for r, (lo, hi) in enumerate(part):
        I[0][r] = band_rows(lo, hi, ny[0], 1)
        O[0][r] = band_rows(lo, hi, ny[0], 0)
        for l in range(Lg):
            near = dilate(I[l][r])      # coarse row i: some fine row f within one row of the set with |f - 2 i| <= 1
            I[l + 1][r] = np.array([near[max(2 * i - 1, 0):2 * i + 2].any() for i in range(ny[l + 1])])
            O[l + 1][r] = np.array([O[l][r][2 * i] for i in range(ny[l + 1])])      # a coarse row belongs to the owner of the fine row under it
        x = band_rows(lo, hi, ny[0], 1)
        for l in range(Lg):
            NX[l][r] = x
            NR[l][r] = dilate(x)
            x = coarse_around(NR[l][r], ny[l + 1])
    return I, O, NX, NR


def check_plan(L, n, nx, ny, Lg, part, stats):
    R = len(part)
    I, O, NX, NR = brute(ny, Lg, part)
    plans = []
    for me in range(R):
        rc, P = plan_of(L, n, nx, ny, Lg, part, me)
        assert rc == 0 and (P.Lg, P.ranks, P.rank) == (Lg, R, me)
        plans.append(P)
        for l in range(Lg + 1):
            for r in range(R):
                assert (rows(P.I[l][r], ny[l]) == I[l][r]).all(), ("I", l, r, me)
                assert (rows(P.O[l][r], ny[l]) == O[l][r]).all(), ("O", l, r, me)
        for l in range(Lg):
            assert (rows(P.NX[l], ny[l]) == NX[l][me]).all() and (rows(P.NR[l], ny[l]) == NR[l][me]).all(), ("need", l, me)
        # setup_bad: a rank owns fewer than MG_SETUP_HALO rows of a level below Lg, or this rank reads a row beyond its owned rows + halo
        thin = any(O[l][r].sum() < SETUP_HALO for l in range(Lg) for r in range(R))
        far = False
        for l in range(Lg):
            read = dilate(I[l][me]) | NR[l][me]      # the way down: the residual one row beyond the support; the way up
            for i in np.flatnonzero(O[l + 1][me]):    # the next level's owned rows are formed from the three fine rows under each
                read[max(2 * i - 1, 0):2 * i + 2] = True
            own = np.flatnonzero(O[l][me])
            far = far or bool((np.flatnonzero(read) < own[0] - SETUP_HALO).any() or (np.flatnonzero(read) > own[-1] + SETUP_HALO).any())
        assert P.setup_bad == int(thin or far), (me, thin, far)
        stats["setup_bad"] += P.setup_bad
        # the verdict: a rank other than the two neighbours contributes to rows this rank needs - the brute force asks every rank
        beyond = any((I[l][q] & NR[l][me]).any() for l in range(Lg) for q in range(R) if abs(q - me) > 1)
        assert P.beyond == int(beyond), (me, beyond)
        stats["beyond"] += P.beyond
        # the zones: my share on the rows a neighbour needs, its share on the rows I need; offsets packed level after level
        for side, nb in ((0, me - 1), (1, me + 1)):
            offs = offr = 0
            for l in range(Lg):
                want_s = I[l][me] & NR[l][nb] if 0 <= nb < R else np.zeros(ny[l], bool)
                want_r = I[l][nb] & NR[l][me] if 0 <= nb < R else np.zeros(ny[l], bool)
                assert (rows(P.zs[side][l], ny[l], True) == want_s).all() and (rows(P.zr[side][l], ny[l], True) == want_r).all(), ("zone", side, l, me)
                assert (P.zoff_s[side][l], P.zoff_r[side][l]) == (offs, offr)
                offs += int(want_s.sum()) * nx[l]
                offr += int(want_r.sum()) * nx[l]
            assert P.zone >= max(offs, offr)
            stats["zones"] += offs > 0
        # the segment table: the rows of NR that are not own rows, or that lie in a received zone; ascending runs that do not touch, packed
        assert not P.overflow and P.nseg <= NSEG
        at, prev = 0, (-1, -1)
        got = [np.zeros(ny[l], bool) for l in range(Lg)]
        for k in range(P.nseg):
            s = P.seg[k]
            assert 0 <= s.level < Lg and 0 <= s.row0 < s.row1 <= ny[s.level] and s.off == at
            assert (s.level, s.row0) > prev, "runs ascend and do not touch"
            prev = (s.level, s.row1)
            assert not got[s.level][s.row0:s.row1].any()
            got[s.level][s.row0:s.row1] = True
            at += (s.row1 - s.row0) * nx[s.level]
        assert P.total == at
        for l in range(Lg):
            assert (got[l] == (NR[l][me] & (~I[l][me] | rows(P.zr[0][l], ny[l]) | rows(P.zr[1][l], ny[l])))).all(), ("segments", l, me)
        assert P.win_rows == max(int(I[Lg][r].sum()) for r in range(R)) and P.nsmall == 2 + P.win_rows * nx[Lg]
        assert P.aslot == 9 * max(int(O[Lg][r].sum()) for r in range(R)) * nx[Lg]
    # cross-rank symmetry of the messages: what rank r packs for r + 1 is what r + 1 expects from r, level by level, and the other way round
    zone = max(P.zone for P in plans)
    for r in range(R - 1):
        a, b = plans[r], plans[r + 1]
        for l in range(Lg):
            assert tuple(a.zs[1][l]) == tuple(b.zr[0][l]) and a.zoff_s[1][l] == b.zoff_r[0][l], (r, l)
            assert tuple(b.zs[0][l]) == tuple(a.zr[1][l]) and b.zoff_s[0][l] == a.zoff_r[1][l], (r, l)
    assert all(0 <= P.zone <= zone for P in plans)
    return any(P.beyond for P in plans)


def random_partition(rng, nb, R, kind):
    if kind == 0:
        return [(nb * r // R, nb * (r + 1) // R) for r in range(R)]      # euler_amd.slab.slab_bands
    if kind == 1:      # slabs of ONE band at either end and between thick ones, which share the other bands
        thin = rng.random(R) < 0.4
        thin[0] = thin[-1] = True
        thin[R // 2] = False
        thick = np.flatnonzero(~thin)
        if nb - R >= 2 * len(thick):
            w = np.ones(R, int)
            w[thick] += 2 + rng.multinomial(nb - R - 2 * len(thick), np.ones(len(thick)) / len(thick))
            cuts = [0] + [int(c) for c in np.cumsum(w)]
            return list(zip(cuts[:-1], cuts[1:]))
    cuts = [0] + sorted(int(c) for c in rng.choice(np.arange(1, nb), R - 1, replace=False)) + [nb]
    return list(zip(cuts[:-1], cuts[1:]))


def test_level_dimensions_entry_and_gather_level(L):
    rng = np.random.default_rng(5)
    for X, nbands in [(64, 1), (8, 1), (1, 1), (4096, 64), (16384, 256), (1000, 18)] + [(int(rng.integers(1, 5000)), int(rng.integers(1, 300))) for _ in range(200)]:
        n, nx, ny, off = levels_of(L, X, nbands)
        w, h, at, want = (X + G0 - 1) // G0, RPB * nbands, 0, []
        while True:
            want.append((w, h, at))
            at += w * h
            if w * h <= TOP_MAX:
                break
            w, h = (w + 1) // 2, (h + 1) // 2
        assert n == len(want) <= MAXLEV and [(nx[l], ny[l], off[l]) for l in range(n)] == want
        nodes = [nx[l] * ny[l] for l in range(n)]
        lC = next(l for l in range(n) if nodes[l] <= TAIL_MAX or l == n - 1)      # the first level of at most MG_TAIL_MAX nodes
        assert L.eu_mg_entry_level(n, nx, ny) == lC
        auto = 0 if nodes[0] <= SMALL_LEVEL0 else next(l for l in range(lC + 1) if nodes[l] <= GATHER_MAX or l == lC)
        assert L.eu_mg_gather_level(n, nx, ny, 0) == auto
        assert L.eu_mg_gather_level(n, nx, ny, -1) == 0
        for forced in range(1, lC + 3):
            assert L.eu_mg_gather_level(n, nx, ny, forced) == min(forced, lC)
    nx, ny, off = (i32 * MAXLEV)(), (i32 * MAXLEV)(), (C.c_size_t * MAXLEV)()
    assert L.eu_mg_levels(1 << 20, 1 << 17, nx, ny, off) == EULER_EINVAL      # more than MG_MAXLEV levels
    assert L.eu_mg_levels(0, 4, nx, ny, off) == EULER_EINVAL and L.eu_mg_levels(64, 0, nx, ny, off) == EULER_EINVAL


def test_the_split_plan_against_row_sets(L):
    rng = np.random.default_rng(20251)
    stats = {"beyond": 0, "setup_bad": 0, "zones": 0, "cases": 0, "thin": 0, "refused": 0, "odd_nx": 0}
    shapes = [(int(rng.integers(2, 9)), None) for _ in range(120)] + [(16, 40), (64, 72)]
    for R, nb in shapes:
        nb = nb or int(rng.integers(max(R, 4), 41))
        X = int(rng.choice([64, 100, 200, 264, 520, 1000, 1024, 2040, 4096, int(rng.integers(64, 4097))]))
        part = random_partition(rng, nb, R, int(rng.integers(0, 3)))
        n, nx, ny, off = levels_of(L, X, nb)
        lC = L.eu_mg_entry_level(n, nx, ny)
        stats["thin"] += any(hi - lo == 1 for lo, hi in part)
        stats["odd_nx"] += X % 16 != 0
        for Lg in range(1, lC + 1):
            stats["refused"] += check_plan(L, n, nx, ny, Lg, part, stats)
            stats["cases"] += 1
    assert stats["cases"] >= 200 and all(stats[k] > 0 for k in stats), stats      # valid and refused plans, zones, thin slabs, the replicated setup: all reached


def test_the_pinned_partitions_of_the_gpu_suite(L):
    """the partitions of test_slab_rows.py::test_multilevel_mode_on_row_slabs with a forced level: valid, valid, refused, valid"""
    for X, Y, bands, forced, active in ((512, 1024, "0-7,7-8,8-16", 1, 1), (512, 1024, "0-7,7-8,8-16", 2, 2), (1024, 2048, "0-15,15-16,16-32", 3, 0),
                                        (1024, 8192, "0-10,10-20,20-29,29-38,38-47,47-56,56-66,66-128", 1, 1)):
        part = [tuple(int(t) for t in b.split("-")) for b in bands.split(",")]
        n, nx, ny, off = levels_of(L, X, Y // 64)
        Lg = L.eu_mg_gather_level(n, nx, ny, forced)
        assert Lg == forced
        refused = check_plan(L, n, nx, ny, Lg, part, {"beyond": 0, "setup_bad": 0, "zones": 0})
        assert (0 if refused else Lg) == active, (X, Y, bands, forced)


def test_overflow_and_refusals(L):
    n, nx, ny, off = levels_of(L, 1024, 32)
    part = [(0, 15), (15, 16), (16, 32)]
    rc, P = plan_of(L, n, nx, ny, 2, part, 1)
    assert rc == 0 and P.nseg >= 2 and not P.overflow
    full = P.nseg
    rc, Q = plan_of(L, n, nx, ny, 2, part, 1, seg_cap=full - 1)      # a table one entry short: reported, the entries that fit are the same, nothing behind them
    assert rc == 0 and Q.overflow == 1 and Q.nseg == full - 1 and Q.seg[full - 1].row1 == 0
    assert all((Q.seg[k].level, Q.seg[k].row0, Q.seg[k].row1, Q.seg[k].off) == (P.seg[k].level, P.seg[k].row0, P.seg[k].row1, P.seg[k].off) for k in range(full - 1))
    ok = dict(n=n, Lg=2, part=part, rank=1)
    for bad in (dict(Lg=0), dict(Lg=n), dict(rank=3), dict(rank=-1), dict(part=[(0, 32)], rank=0), dict(part=[(0, 16), (15, 32)], rank=0), dict(part=[(0, 16), (16, 33)], rank=0),
                dict(part=[(0, 16), (16, 16), (16, 32)]), dict(n=1), dict(n=MAXLEV + 1)):
        a = dict(ok, **bad)
        assert plan_of(L, a["n"], nx, ny, a["Lg"], a["part"], a["rank"])[0] == EULER_EINVAL, bad
    assert plan_of(L, n, nx, ny, 2, part, 1, seg_cap=NSEG + 1)[0] == EULER_EINVAL
    assert plan_of(L, n, nx, ny, 2, [(r, r + 1) for r in range(MAXR + 1)], 0)[0] == EULER_EINVAL


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_host_code_is_clean_under_asan_ubsan(tmp_path):
    """a stand-alone program over the planner: random partitions up to 64 ranks and MG_MAXLEV levels, a forced overflow, the refusals"""
    exe = str(tmp_path / "sanitize_mg_split")
    cmd = ["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "euler_amd", "csrc"),
           os.path.join(ROOT, "tests", "c", "sanitize_mg_split.c"), os.path.join(ROOT, "euler_amd", "csrc", "euler_host.c"), "-lm", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])
