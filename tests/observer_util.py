"""What the GPU tests of the read-only observer passes share (test_gpu_overview, test_gpu_diagnostics, test_gpu_viewport, test_gpu_observers)."""
import os

import euler_amd as ea
from test_gpu_parity import assert_bits

EULER_EINVAL, EULER_ESTATE = -1, -5      # include/euler.h
DYE = (ea.F_DYE_R, ea.F_DYE_G, ea.F_DYE_B)
EXE = os.path.join(os.path.dirname(ea.LIB_PATH), "..", "bin", "euler")
STATE_FIELDS = (ea.F_U, ea.F_V, ea.F_UTMP, ea.F_VTMP, ea.F_COUNT, ea.F_PREV_COUNT, ea.F_MARKERS, ea.F_PRESSURE)


def read_back(sim, dye):
    g = [sim.get(f) for f in (ea.F_SOLID, ea.F_SINK, ea.F_COUNT, ea.F_U, ea.F_V)]
    return g + [tuple(sim.get(f) for f in DYE) if dye else None]


def dumped_frames(stdout):
    """the frames of `euler --dump`"""
    out = []
    for chunk in stdout.split(b"--- frame ")[1:]:
        header, body = chunk.split(b"\n", 1)
        out.append(body[: int(header.split(b"(")[1].split()[0])])
    return out


def no_trace_pair(make, look, between_stages=None, fields=STATE_FIELDS, frames=20, compare_every=1):
    """Two handles of make() side by side; look(b, stepped) looks at one of them before (stepped = False) and after every frame, and in the middle
    frame after each of the six stages of one more substep (between_stages(b, stage) in its place where given).  `fields` are compared bit for bit every
    compare_every-th frame and at the middle one, the four counters at the end.  Returns the handles, still open."""
    a, b = make(), make()
    mid = frames // 2
    for f in range(frames):
        look(b, False)
        a.step(); b.step()
        look(b, True)
        if f == mid:      # once between the stages of a substep
            dt = a.timestep(0.1)
            assert b.timestep(0.1) == dt
            for st in range(6):
                a.stage(st, dt); b.stage(st, dt)
                if between_stages:
                    between_stages(b, st)
                else:
                    look(b, True)
        if f % compare_every == compare_every - 1 or f == mid:
            for fld in fields:
                assert_bits(b.get(fld), a.get(fld), "frame %d field %d" % (f, fld))
    sa, sb = a.stats(), b.stats()
    assert (sa.total_substeps, sa.total_pcg_iterations, sa.n_markers, sa.rng_state) == (sb.total_substeps, sb.total_pcg_iterations, sb.n_markers, sb.rng_state)
    return a, b
