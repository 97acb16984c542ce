"""The stage hand-off flags (euler_amd/csrc/eu_valid.h, docs/stage_validity.md) are pure host state: tests/c/stage_validity.c runs the canonical substep order
against the table of lean forms and every sequence of up to five events against a naive log-scanning model of each promise.  No GPU, about two seconds."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "euler_amd", "csrc")]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_the_header_alone_is_clean_c99(tmp_path):
    src = tmp_path / "only.c"
    src.write_text('#include "eu_valid.h"\n')
    b = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only"] + INC + [str(src)], capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stderr[-3000:]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_every_lean_decision_agrees_with_the_log_of_events(tmp_path):
    exe = str(tmp_path / "stage_validity")
    b = subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra"] + INC + [os.path.join(ROOT, "tests", "c", "stage_validity.c"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "stage validity: ok" in r.stdout, r.stdout[-4000:]


def test_no_kernel_file_touches_a_flag_directly():
    """Events and queries only: the embedded struct's members are eu_valid.h's own."""
    import re
    src = os.path.join(ROOT, "euler_amd", "csrc")
    names = "p_pending|maxsq_state|uv_clean|uv_zb|count32_dirty|prebin_valid|tmap_valid|utmp_clean|countT_clean|blocked_dirty|solidT_dirty|lean_ok"
    pat = re.compile(r"\bvd\s*\.|->\s*(%s)\b" % names)
    hits = []
    for f in sorted(os.listdir(src)):
        if f.endswith((".hip", ".h")) and f != "eu_valid.h":
            for n, line in enumerate(open(os.path.join(src, f), errors="replace"), 1):
                if pat.search(line):
                    hits.append("%s:%d" % (f, n))
    assert not hits, hits
