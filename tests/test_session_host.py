"""The host half of the session files (docs/session.md), no GPU: read_session / write_session round-trip a forged file and the library's own parser
(euler_host.c eu_session_parse) accepts it and refuses its corruptions with the documented codes; the SETT record and the chunk constants against sizeof / offsetof
from a small C program; the composer, the parser and the settings comparison under the sanitizers (tests/c/sanitize_session.c, a stand-alone program)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import euler_amd as ea
import session_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reseal(raw):
    return bytes(raw[:-8]) + struct.pack("<Q", ea._fnv1a64(bytes(raw[:-8])))


def test_the_new_entry_points_are_exported():
    L = ea.load_library()
    for name in ("euler_save_session", "euler_load_session"):
        assert name in ea.EXPORTS and getattr(L, name)
    assert L.euler_abi_version() == 2
    assert ea.SESSION_IGNORE_SETTINGS == 1 and ea.SESSION_TAGS[0] == b"TIME" and ea.SESSION_TAGS[-1] == b"END\0"


@pytest.mark.parametrize("dye", [False, True])
def test_write_session_and_read_session_round_trip_and_the_library_accepts_the_file(tmp_path, dye):
    st = su.forged_state()
    if dye:
        rng = np.random.default_rng(8)
        for k in ea.SNAPSHOT_DYE:
            st[k] = rng.random((st["Y"], st["X"])).astype(np.float32)
        st["settings"]["rainbow"] = 1
    path = str(tmp_path / "s.session")
    ea.write_session(path, st)
    back = ea.read_session(path)
    st["n_markers"] = len(st["markers"])
    assert su.same_entries(back, st)
    raw = open(path, "rb").read()
    assert raw[8:12] == struct.pack("<I", 4) and raw[20:24] == struct.pack("<I", 1 if dye else 0)
    rc, why = su.parse_with_library(raw, st["X"], st["Y"], dye=int(dye))
    assert rc == 0, why
    # written again from what was read: the same bytes
    ea.write_session(path + "2", back)
    assert open(path + "2", "rb").read() == raw
    # a plain reader of snapshots does not take it for one
    with pytest.raises(ValueError):
        ea.read_snapshot(path)


def test_an_off_record_round_trips(tmp_path):
    st = su.forged_state()
    st["heat"] = {"on": False, "record": ea.heat_default().reshape(1), "boxes": np.zeros(0, ea.HEAT_BOX_DTYPE), "field": None}
    st["tracers"] = np.zeros(0, ea.TRACER_DTYPE)
    st["bodies"] = {"bodies": np.zeros(0, ea.BODY_DTYPE), "origins": np.zeros((0, 2), np.int32)}
    st["forcing"] = {"record": ea.forcing_default().reshape(1), "boxes": np.zeros(0, ea.FORCE_BOX_DTYPE)}
    st["reseed"] = {"record": ea.reseed().reshape(1), "stats": np.zeros(1, ea.RESEED_STATS_DTYPE)}
    path = str(tmp_path / "off.session")
    ea.write_session(path, st)
    st["n_markers"] = len(st["markers"])
    assert su.same_entries(ea.read_session(path), st)
    rc, why = su.parse_with_library(open(path, "rb").read(), st["X"], st["Y"])
    assert rc == 0, why


def test_the_library_refuses_forged_corruptions_with_its_codes(tmp_path):
    st = su.forged_state()
    X, Y = st["X"], st["Y"]
    good = ea.session_bytes(st)
    good += struct.pack("<Q", ea._fnv1a64(good))

    def refused(raw, code, *words, **kw):
        rc, why = su.parse_with_library(raw, X, Y, **kw)
        assert rc == code and all(w in why for w in words), (rc, why)

    assert su.parse_with_library(good, X, Y)[0] == 0
    refused(good[:-9] + good[-8:], su.EIO)                                   # a byte missing
    refused(good[:len(good) // 2], su.EIO)                                   # truncated
    flipped = bytearray(good); flipped[300] ^= 0x40
    refused(bytes(flipped), su.EIO, "checksum")
    wrong = dict(st, X=X + 1)
    raw = ea.session_bytes(wrong); refused(raw + struct.pack("<Q", ea._fnv1a64(raw)), su.EINVAL, "13x9")
    refused(good, su.EINVAL, "capacity", max_markers=len(st["markers"]) - 1)
    refused(good, su.EINVAL, "dye", dye=1)
    pay = ea.session_payloads(st)
    chunks = [(t, 1, p) for t, p in zip(ea.SESSION_TAGS, pay)]

    def forged(ch):
        raw = ea.session_bytes(st, ch)
        return raw + struct.pack("<Q", ea._fnv1a64(raw))

    refused(forged(chunks[:5] + [(b"WIND", 1, b"\0" * 8)] + chunks[5:]), su.EINVAL, "WIND")
    refused(forged([chunks[1], chunks[0]] + chunks[2:]), su.EINVAL, "FORC")
    refused(forged(chunks[:2] + chunks[1:]), su.EINVAL)
    refused(forged(chunks[:-1]), su.EINVAL, "END")
    refused(forged(chunks[:3] + [(b"TRAC", 2, pay[3])] + chunks[4:]), su.EINVAL, "TRAC", "version 2")
    refused(forged(chunks[:3] + [(b"TRAC", 1, struct.pack("<Q", 1 << 40) + pay[3][8:])] + chunks[4:]), su.EINVAL, "TRAC")
    # records the host checks refuse: a heat value beyond 1e4, a body over an open cell, an unflagged tracer without a position
    hot = dict(st, heat=dict(st["heat"], field=st["heat"]["field"].copy()))
    hot["heat"]["field"][4, 7] = 10001.0
    raw = ea.session_bytes(hot); refused(raw + struct.pack("<Q", ea._fnv1a64(raw)), su.EINVAL, "HEAT", "1e4")
    opened = dict(st, solid=st["solid"].copy())
    opened["solid"][4, 5] = 0
    raw = ea.session_bytes(opened); refused(raw + struct.pack("<Q", ea._fnv1a64(raw)), su.EINVAL, "BODY", "open")
    lost = dict(st, tracers=st["tracers"].copy())
    lost["tracers"]["flags"][2] = ea.TRACER_RETIRED
    raw = ea.session_bytes(lost); refused(raw + struct.pack("<Q", ea._fnv1a64(raw)), su.EINVAL, "TRAC")


def test_the_sett_record_and_the_chunk_constants_are_the_structs(tmp_path):
    d = ea.SESSION_SETTINGS_DTYPE
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "euler_host.h"\nint main(void) {\n'
                   '  printf("%zu %d %d", sizeof(eu_session_settings), EU_SESSION_OPTS, EULER_OPT__COUNT);\n'
                   + "".join('  printf(" %%zu", offsetof(eu_session_settings, %s));\n' % n for n in d.names)
                   + '  printf(" %zu %zu %zu %zu %zu %zu %zu %zu", sizeof(euler_forcing), sizeof(euler_force_box), sizeof(euler_heat), sizeof(euler_heat_box), sizeof(euler_tracer),'
                     ' sizeof(euler_body), sizeof(euler_reseed), sizeof(euler_reseed_stats));\n'
                   '  printf(" %d %zu", EULER_SESSION_IGNORE_SETTINGS, sizeof(eu_session));\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "euler_amd", "csrc"), str(src), "-o", str(exe)])
    out = [int(t) for t in subprocess.check_output([str(exe)]).split()]
    assert out[:3] == [320, ea.SESSION_OPTS, 24] and d.itemsize == 320
    n = len(d.names)
    assert out[3:3 + n] == [d.fields[k][1] for k in d.names]
    assert out[3 + n:11 + n] == [ea.FORCING_DTYPE.itemsize, ea.FORCE_BOX_DTYPE.itemsize, ea.HEAT_DTYPE.itemsize, ea.HEAT_BOX_DTYPE.itemsize, ea.TRACER_DTYPE.itemsize,
                                 ea.BODY_DTYPE.itemsize, ea.RESEED_DTYPE.itemsize, ea.RESEED_STATS_DTYPE.itemsize] == [48, 24, 32, 24, 32, 64, 32, 32]
    assert out[11 + n] == ea.SESSION_IGNORE_SETTINGS and out[12 + n] < (1 << 16)      # (session_util.parse_with_library's output buffer holds an eu_session)
    assert struct.calcsize(ea.SESSION_STAT_FORMAT) == 40 and d.fields["opt"][0].shape == (ea.SESSION_OPTS,)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not available")
def test_host_code_is_clean_under_asan_ubsan(tmp_path):
    """a stand-alone program: a valid 12 x 9 session, every truncation, byte flips of the header, the chunk headers and the counts, oversized counts, chunks out of
    order, a duplicate, a missing END, an unknown tag, a body over an open cell - run directly, nothing preloaded"""
    probe = tmp_path / "probe.c"      # are the sanitizers' runtimes installed at all?  Asked before any work, so that no failure of the real build is taken for it
    probe.write_text("int main(void) { return 0; }\n")
    if subprocess.run(["gcc", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("libasan / libubsan not installed")
    exe = str(tmp_path / "sanitize_session")
    cmd = ["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "euler_amd", "csrc"), "-I" + os.path.join(ROOT, "euler_amd", "cli"),
           os.path.join(ROOT, "tests", "c", "sanitize_session.c"), os.path.join(ROOT, "euler_amd", "csrc", "euler_host.c"), "-lm", "-lpthread", "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "clean" in r.stdout, (r.stdout[-1000:], r.stderr[-4000:])
