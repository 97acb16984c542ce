"""The host half of the marker density control (docs/reseed.md), no GPU: the numpy restatement (tests/reseed_ref.py) against its plain-loop twin and against the
library's own sequential reference (euler_host.c eu_reseed_pass) on random states; the composition with the pass off against eo_step; the layout of both structs
from a small C program; the host C code under the sanitizers (tests/c/sanitize_reseed.c); and what the rule is for, on the CPU composition at the reference's own
100 x 40: without it the count byte wraps in the waterfall and the block loses a fifth of its fluid cells, with it neither happens."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import euler_amd as ea
import reseed_ref as rref
from golden_util import X as GX, Y as GY, load, scenario_text
from oracle_lib import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
COMPARED = ("u", "v", "utmp", "vtmp", "count", "prev_count", "solid", "source", "sink")


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def golden_text(name):
    return scenario_text(load(name + "_frames.npz"))


def true_bins(markers, X, Y):
    m = np.asarray(markers, F32).reshape(-1, 2)
    return np.bincount(np.floor(m[:, 1]).astype(np.int64) * X + np.floor(m[:, 0]).astype(np.int64), minlength=X * Y).reshape(Y, X)


# ----------------------------------------------------------------------------- the three restatements of one pass
def random_state(seed, X, Y, density=3.0):
    """masks at random inside a sink ring, markers clumped so that some cells hold dozens and one holds more than 256, on sub-cell boundaries and cell edges, with
    duplicates; count = the bins as a byte; prev_count mostly wet, and some wet cells emptied afterwards so that holes exist next to every kind of neighbour"""
    rng = np.random.default_rng(seed)
    shape = (Y, X)
    solid, sink, source = (np.zeros(shape, np.uint8) for _ in range(3))
    r = rng.random((Y - 2, X - 2))
    solid[1:-1, 1:-1], sink[1:-1, 1:-1], source[1:-1, 1:-1] = r < 0.08, (0.08 <= r) & (r < 0.11), (0.11 <= r) & (r < 0.14)
    sink[0], sink[-1], sink[:, 0], sink[:, -1] = 1, 1, 1, 1
    ys, xs = np.nonzero(solid[1:-1, 1:-1] == 0)
    ys, xs = ys + 1, xs + 1
    n = int(density * X * Y)
    pick = rng.integers(0, len(xs), n)
    clump = rng.random(n) < 0.35
    pick[clump] = rng.integers(0, max(1, len(xs) // 40), int(clump.sum()))      # a fortieth of the cells takes a third of the markers
    pick[rng.choice(n, 300, replace=False)] = len(xs) // 2                      # ... and one cell three hundred: its byte wraps
    frac = rng.random((n, 2)).astype(F32) * F32(0.998) + F32(0.001)
    snap = rng.random((n, 2)) < 0.25
    frac[snap] = (rng.integers(0, 4, int(snap.sum())) * 0.25).astype(F32)        # exactly on .0, .25, .5, .75
    m = np.stack([xs[pick].astype(F32) + frac[:, 0], ys[pick].astype(F32) + frac[:, 1]], axis=1).astype(F32)
    m[n // 2:n // 2 + 40] = m[n // 2]                                            # forty markers with identical coordinates
    rng.shuffle(m)
    prev = (rng.random(shape) < 0.9).astype(np.uint8) * 3
    bins = true_bins(m, X, Y)
    empty = (rng.random(shape) < 0.06) & (solid == 0)
    keep = ~empty[np.floor(m[:, 1]).astype(int), np.floor(m[:, 0]).astype(int)]
    m = m[keep]
    count = (true_bins(m, X, Y) % 256).astype(np.uint8)
    assert bins.max() > 256
    return dict(markers=m, count=count, prev_count=prev, solid=solid, sink=sink, source=source, rng_state=int(rng.integers(1, 1 << 63)))


RECORDS = [rref.reseed(16, True), rref.reseed(16, False), rref.reseed(0, True), rref.reseed(4, True, 3, 3), rref.reseed(254, True, 1, 1), rref.reseed(40, True, 0, 2)]


@pytest.mark.parametrize("size", [(37, 23), (64, 40), (101, 45)])
def test_the_restatement_against_its_loop_twin_and_the_c_reference(size):
    X, Y = size
    totals = rref.new_stats()
    for seed, r in enumerate(RECORDS):
        st = random_state(1000 * X + seed, X, Y)
        out = []
        for fn in (rref.pass_arrays, rref.pass_loops, rref.pass_c):
            count, stats = st["count"].copy(), rref.new_stats()
            m, rng = fn(r, st["markers"], count, st["prev_count"], st["solid"], st["sink"], st["source"], st["rng_state"], 4 * X * Y, stats)
            out.append((m, count.copy(), rng, dict(stats)))
            # a second pass takes what the first deferred
            m2, rng2 = fn(r, m, count, st["prev_count"], st["solid"], st["sink"], st["source"], rng, 4 * X * Y, stats)
            out[-1] += (m2, count.copy(), rng2, dict(stats))
        for other in out[1:]:
            for a, b in zip(out[0], other):
                if isinstance(a, np.ndarray) and a.dtype == F32:
                    assert np.array_equal(bits(a), bits(b)), (size, r)
                elif isinstance(a, np.ndarray):
                    assert np.array_equal(a, b), (size, r)
                else:
                    assert a == b, (size, r, a, b)
        for k in totals:
            totals[k] += out[0][7][k]
    assert all(v > 0 for v in totals.values()), totals      # every branch was taken somewhere


def test_every_kept_marker_was_there_and_every_new_one_lies_in_its_hole():
    X, Y = 64, 40
    for seed in range(4):
        st = random_state(77 + seed, X, Y)
        count, stats = st["count"].copy(), rref.new_stats()
        holes = rref.holes_of(count, st["prev_count"], st["solid"], st["sink"], st["source"])
        m, rng = rref.pass_arrays(rref.reseed(16, True), st["markers"], count, st["prev_count"], st["solid"], st["sink"], st["source"], st["rng_state"], 4 * X * Y, stats)
        n_kept = len(st["markers"]) - stats["removed"]
        assert len(m) == n_kept + stats["added"] and stats["removed"] > 0 and stats["added"] > 0
        # the kept markers as a multiset of bit patterns: a sub-multiset of what was there
        key = lambda a: np.sort(np.ascontiguousarray(a, F32).view(np.uint64).reshape(-1))
        before, kept = key(st["markers"]), key(m[:n_kept])
        ub, cb = np.unique(before, return_counts=True)
        uk, ck = np.unique(kept, return_counts=True)
        pos = np.searchsorted(ub, uk)
        assert (pos < len(ub)).all() and np.array_equal(ub[pos], uk) and (ck <= cb[pos]).all()
        # markers outside the listed cells are all kept; a listed cell keeps one marker per occupied sub-cell, its count; nothing exceeds the bound afterwards
        was = st["count"] > 16
        cell_of = lambda a: (np.floor(a[:, 1]).astype(int), np.floor(a[:, 0]).astype(int))
        assert (~was[cell_of(st["markers"])]).sum() == (~was[cell_of(m[:n_kept])]).sum()
        assert np.array_equal(true_bins(m[:n_kept], X, Y)[was], count[was]) and count[was].min() >= 1 and count.max() <= 16
        # the appended markers: one per hole, row-major, inside its cell (a draw of exactly 1 or a sum that rounds up would land on the far edge: not with these seeds)
        ys, xs = np.nonzero(holes)
        new = m[n_kept:]
        assert len(new) == len(xs) and np.array_equal(np.floor(new[:, 0]), xs) and np.array_equal(np.floor(new[:, 1]), ys)
        assert (count[holes] == 1).all() and rng != st["rng_state"]


# ----------------------------------------------------------------------------- off is the oracle
@pytest.mark.parametrize("name", ["block", "waterfall"])
def test_the_composition_with_the_pass_off_is_eo_step(name):
    text = golden_text(name)
    a, b = Oracle(GX, GY).load_text(text), Oracle(GX, GY).load_text(text)
    for k in range(20):
        na = rref.step(None, a, rref.reseed())
        nb = b.step()
        assert tuple(na) == tuple(nb), (k, na, nb)
        for n in COMPARED:
            assert np.array_equal(np.array(getattr(a, n)).view(np.uint8), np.array(getattr(b, n)).view(np.uint8)), (k, n)
        assert np.array_equal(bits(a.markers), bits(b.markers)) and a.c.rng_state == b.c.rng_state and a.c.source_exhausted == b.c.source_exhausted
    a.close(); b.close()


# ----------------------------------------------------------------------------- the structs, the sanitizers
def test_dtypes_are_the_structs(tmp_path):
    r, s = ea.RESEED_DTYPE, ea.RESEED_STATS_DTYPE
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "euler.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(euler_reseed), sizeof(euler_reseed_stats));\n'
                   + "".join('  printf(" %%zu", offsetof(euler_reseed, %s));\n' % n for n in r.names)
                   + "".join('  printf(" %%zu", offsetof(euler_reseed_stats, %s));\n' % n for n in s.names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    assert out[:2] == [32, 32] == [r.itemsize, s.itemsize]
    assert out[2:7] == [r.fields[n][1] for n in r.names] == [0, 4, 8, 12, 16]
    assert out[7:] == [s.fields[n][1] for n in s.names] == [0, 8, 16, 24]
    assert [r.fields[n][0].base for n in r.names] == [np.int32] * 5 and r.fields["reserved"][0].shape == (4,)
    assert [s.fields[n][0] for n in s.names] == [np.uint64] * 4
    assert ea.load_library().euler_abi_version() == 2


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_host_code_is_clean_under_asan_ubsan(tmp_path):
    """a stand-alone program over the refusals, the sub-cell index, eu_reseed_pass on hand-made and random states and the command's spec parser"""
    probe = tmp_path / "probe.c"      # are the sanitizers' runtimes installed at all?  Asked before any work, so that no failure of the real build is taken for it
    probe.write_text("int main(void) { return 0; }\n")
    if subprocess.run(["gcc", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("libasan / libubsan not installed")
    exe = str(tmp_path / "sanitize_reseed")
    cmd = ["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "euler_amd", "csrc"), "-I" + os.path.join(ROOT, "euler_amd", "cli"),
           os.path.join(ROOT, "tests", "c", "sanitize_reseed.c"), os.path.join(ROOT, "euler_amd", "csrc", "euler_host.c"), "-lm", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])


# ----------------------------------------------------------------------------- what the rule is for
def test_the_count_byte_wraps_in_the_waterfall_and_never_exceeds_the_bound_with_thinning():
    """the plain oracle reaches a cell that truly holds 256 markers or more within 400 frames (its byte then reads the count modulo 256); with thin_above = 16 the
    byte never exceeds 16 at a frame's end - the pass leaves at most 16 and the source stage behind it only adds to cells below 4"""
    text = golden_text("waterfall")
    o = Oracle(GX, GY).load_text(text)
    worst, at = 0, -1
    for k in range(400):
        o.step()
        top = int(true_bins(o.markers, GX, GY).max())
        if top > worst:
            worst, at = top, k
        if worst >= 256:
            break
    print("plain waterfall: a cell holds %d markers at frame %d, its byte reads %d" % (worst, at, worst % 256))
    assert worst >= 256
    assert int(np.array(o.count).reshape(-1)[np.argmax(true_bins(o.markers, GX, GY))]) == worst % 256
    o.close()
    o = Oracle(GX, GY).load_text(text)
    stats, r = rref.new_stats(), rref.reseed(16, True)
    top = holes = 0
    for k in range(400):
        rref.step(None, o, r, stats)
        bins = true_bins(o.markers, GX, GY)
        assert np.array_equal(bins, np.array(o.count)), k      # no byte has wrapped: the grid IS the bins
        top = max(top, int(bins.max()))
        assert top <= 16, (k, top)
    print("waterfall with thin_above = 16 and filling, 400 frames: count at most %d; %s" % (top, stats))
    assert stats["removed"] > 0 and stats["added"] > 0 and stats["deferred"] == 0
    o.close()


def test_the_block_keeps_its_volume_with_thinning_and_filling():
    """block.txt, 300 frames: the plain oracle's markers gather in fewer cells (911 of 1122 fluid cells are left); with thin_above = 16 and filling the fluid
    cells stay within 5 % of 1122"""
    text = golden_text("block")
    o = Oracle(GX, GY).load_text(text)
    first, n0 = int(np.count_nonzero(o.count)), o.n_markers
    assert (first, n0) == (1122, 4488)
    for _ in range(300):
        o.step()
    plain = int(np.count_nonzero(o.count))
    print("block, frame 300, plain: %d fluid cells of %d, %d markers" % (plain, first, o.n_markers))
    assert plain < 0.85 * first and o.n_markers == n0
    o.close()
    o = Oracle(GX, GY).load_text(text)
    stats = rref.new_stats()
    for _ in range(300):
        rref.step(None, o, rref.reseed(16, True), stats)
    kept = int(np.count_nonzero(o.count))
    print("block, frame 300, thin_above = 16 and filling: %d fluid cells of %d, %d markers; %s" % (kept, first, o.n_markers, stats))
    assert abs(kept - first) <= 0.05 * first
    assert o.n_markers == n0 - stats["removed"] + stats["added"] and int(np.array(o.count).max()) <= 16
    o.close()
