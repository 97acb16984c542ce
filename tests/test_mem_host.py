"""The ledger of a handle's device memory (euler_amd/csrc/eu_mem.h, docs/handle_memory.md) is plain host code: tests/c/sanitize_mem.c drives it over malloc with the
k-th allocation failing, under the address sanitizer with its leak check.  No GPU, a few seconds.  The source checks below keep the ledger the ONLY place that
allocates, frees or counts a handle's device memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "euler_amd", "csrc")
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + SRC]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_the_header_alone_is_clean_c99(tmp_path):
    src = tmp_path / "only.c"
    src.write_text('#include "eu_mem.h"\n')
    b = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only"] + INC + [str(src)], capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stderr[-3000:]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_the_ledger_is_clean_under_asan_ubsan_with_every_allocation_failing_in_turn(tmp_path):
    """a creation-like sequence failing at every k, free-one, free-a-group, grow-and-replace, the full table, zeroed blocks: no leak, no double free"""
    exe = str(tmp_path / "sanitize_mem")
    cmd = ["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] + INC + \
          [os.path.join(ROOT, "tests", "c", "sanitize_mem.c"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])


def _hits(pattern, skip=()):
    pat = re.compile(pattern)
    out = []
    for f in sorted(os.listdir(SRC)):
        if f.endswith((".hip", ".h", ".c")) and f not in skip:
            for n, line in enumerate(open(os.path.join(SRC, f), errors="replace"), 1):
                if pat.search(line):
                    out.append("%s:%d" % (f, n))
    return out


def test_only_the_ledger_allocates_and_frees_a_handles_device_memory():
    """hipMalloc / hipFree: the ledger's ops (mem.hip), the communicator's own memory (comm_p2p.hip), and function-local scratch - the stage buffer of snapshot.hip and
    the two measurement helpers of driver.hip (euler_measure_copy_bandwidth, euler_measure_exchange)"""
    assert _hits(r"\bhipMalloc\s*\(|\bhipFree\s*\(", skip=("mem.hip", "comm_p2p.hip", "snapshot.hip", "driver.hip")) == []
    drv = open(os.path.join(SRC, "driver.hip"), errors="replace").read()
    helpers = drv.index('extern "C" int euler_measure_copy_bandwidth')
    assert not re.search(r"\bhipMalloc\s*\(|\bhipFree\s*\(", drv[:helpers])
    assert len(re.findall(r"\bhipMalloc\s*\(", open(os.path.join(SRC, "snapshot.hip"), errors="replace").read())) == 1


def test_nothing_keeps_a_second_figure_or_a_second_owner():
    assert _hits(r"hbm_bytes\s*[+-]?=|g_alloc_bytes|eu_slab_bytes|->\s*shifted\b|skew_alloc") == []
    assert _hits(r"\bmem\s*\.\s*(n|e)\b|->\s*mem\s*\.", skip=("eu_mem.h",)) == []      # the table's members are eu_mem.h's own: everybody else passes &S->mem
