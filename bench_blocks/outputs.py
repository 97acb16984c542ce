"""bench_blocks.outputs - `--dump-outputs DIR`: what the timed path computed in its last step, as .npy files, so that two builds can be compared output for output.

The arrays are what a caller of sim_step() reads back (euler_get_field / euler_get_stats): velocities, pressure, the fluid count grid, the markers and the counters.
Arrays larger than SAMPLE elements are written as a fixed, seeded sample of their elements (the same indices for the same size), everything in float32 or
float64, about 28 MB in all at most; the headline's inputs are fixed by the arguments (deterministic scenario, fixed marker seed).  Nothing here is imported by the product."""
import os

import numpy as np

SAMPLE = 1 << 20      # elements per array at most (markers: rows of (x, y))
SEED = 20261016


def _sample(a, rows=False):
    """the whole array when it is small, else SAMPLE elements (rows for the markers) at seeded random positions, in index order"""
    n = a.shape[0] if rows else a.size
    if n <= SAMPLE:
        return a if rows else a.reshape(-1)
    idx = np.sort(np.random.default_rng(SEED).choice(n, SAMPLE, replace=False))
    return a[idx] if rows else a.reshape(-1)[idx]


def dump_outputs(sim, ea, out_dir):
    """write DIR/<name>.npy for the handle's state after the step just taken -> {name: shape}"""
    os.makedirs(out_dir, exist_ok=True)
    st = sim.stats()
    written = {}

    def put(name, a):
        np.save(os.path.join(out_dir, name + ".npy"), a)
        written[name] = list(a.shape)

    put("u", _sample(sim.get(ea.F_U)).astype(np.float32))
    put("v", _sample(sim.get(ea.F_V)).astype(np.float32))
    put("pressure", _sample(sim.get(ea.F_PRESSURE)).astype(np.float64))
    put("fluid_count", _sample(sim.get(ea.F_COUNT)).astype(np.float32))
    put("markers", _sample(sim.get(ea.F_MARKERS), rows=True).astype(np.float32))
    put("stats", np.array([st.frames, st.total_substeps, st.total_pcg_iterations, st.last_substeps, st.last_pcg_iterations, st.last_residual,
                           st.last_dt, st.n_markers, st.fluid_cells], np.float64))
    return written
