"""What the *_cost.py tools share: the handle of a workload and the timing loop of one kernel class."""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import euler_amd as ea  # noqa: E402
from euler_amd import scenarios  # noqa: E402


def make(size, workload, max_iterations, rainbow=False):
    s = ea.Simulation(size, size, dot_mode=ea.DOT_TREE, precond=ea.PRECOND_IC0_TILE, max_iterations=max_iterations, rainbow=rainbow)
    if workload == "half_tank":
        return s.load_half_tank()
    return s.load_text(getattr(scenarios, workload)(), upscale=True)


def kernel_ms(sim, call, calls, cls="misc"):
    """3 untimed calls, then `calls` timed ones with only the profile class `cls` enabled (a HIP event pair around each of its launches).
    Returns (median, min, max) of the class's milliseconds per call and the median wall milliseconds of the whole call."""
    for _ in range(3):
        call()
    sim.profile_enable([cls])
    kern, whole = [], []
    for _ in range(calls):
        sim.profile_reset()
        t0 = time.perf_counter()
        call()
        whole.append((time.perf_counter() - t0) * 1e3)
        kern.append(sim.profile()[cls][0])
    sim.L.euler_profile_enable(sim.h, 0)
    return statistics.median(kern), min(kern), max(kern), statistics.median(whole)
