#!/usr/bin/env python3
"""What dual time stepping (mgcfd_set_dual_time) costs on the bench level (bench.py's 67^3 lattice, 300,763 nodes) and on the
4-level hierarchy of bench.py's V-cycle:

  * the time_step launch, dual time on (k_time_step_src<2, false>: BDF2) against off (k_time_step), each bracketed by its own
    event pair inside unfused sweeps (MGCFD_OPT_TIMING = 1, MGCFD_OPT_FUSE_UPDATE = 0): the same bracket on both, so the
    difference is the kernels';
  * time per sweep and per V-cycle, dual time on against off, without and with residual smoothing (0.5, 2).  "off" is what a
    caller gets by default (fused stages); "off, unfused" runs the launches dual time replaces one for one.

Clocks warm (a warm-up batch before every measurement), alternated batches and their median; sweeps and cycles are host-timed
around a batch (what a caller pays).  The state is re-initialised before every batch and the time levels set by two
begin_steps, so BDF2 runs.  Writes the figures to --out (default profiles/dual_time_cost.txt) and prints them.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mg-cfd-app-plain_amd"))

import mgcfd                                                   # noqa: E402
from mgcfd import meshgen                                      # noqa: E402


def timed(s, run, n, warmup):
    run(warmup); s.synchronize()
    t0 = time.perf_counter(); run(n); s.synchronize()
    return (time.perf_counter() - t0) / n


def prepare(s, dual, smoothing, fuse, dt):
    mach, alpha = s.free_stream()
    s.set_dual_time(0.0)
    s.set_option("fuse_update", fuse)
    s.set_residual_smoothing(*smoothing)
    s.set_free_stream(mach, alpha, reinitialise=True)
    if dual:
        s.set_dual_time(dt)
        s.begin_step(); s.begin_step()


def alternated(s, settings, run, n, warmup, batches, dt):
    t = {k: [] for k in settings}
    for b in range(batches + 1):
        for k in settings:
            prepare(s, *k, dt)
            v = timed(s, run, n, warmup)
            if b > 0:                                          # (the first round warms up)
                t[k].append(v)
    return {k: statistics.median(v) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lattice", type=int, default=67)
    ap.add_argument("--sizes", default="67,55,48,43")
    ap.add_argument("--sweeps", type=int, default=300)
    ap.add_argument("--cycles", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--cfl", type=float, default=1.0)
    ap.add_argument("--dt", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dual_time_cost.txt"))
    a = ap.parse_args()
    irs, none = (0.5, 2), (0.0, 0)
    # (dual, smoothing, fuse_update)
    settings = [(False, none, 1), (False, none, 0), (True, none, 1), (False, irs, 1), (True, irs, 1)]
    names = ["off (fused stages)", "off, unfused", "dual time on", "smoothing (0.5, 2), dual time off", "smoothing (0.5, 2), dual time on"]
    lines = [f"dual time stepping, BDF2, dt = {a.dt}, clamp 2/3, local steps at CFL {a.cfl}; medians of {a.batches} alternated batches"]

    mg = meshgen.make_multigrid((a.lattice,), "m6wing", seed=0, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    lines.append(f"bench level {a.lattice}^3 = {s.nel(0)} nodes, {s.tiling(0)['tiles']} tiles:")
    per_launch = {}
    for dual in (False, True):
        v = []
        for _ in range(a.batches):
            prepare(s, dual, none, 0, a.dt)
            s.smooth(0, a.warmup)
            s.set_option("timing", 1)
            s.reset_monitoring()
            s.smooth(0, 100)
            v.append(s.loop_times(0)["time_step"] / 300.0)
            s.set_option("timing", 0)
        per_launch[dual] = statistics.median(v)
    lines.append(f"  time_step launch, dual time off   {1e6 * per_launch[False]:8.2f} us   (k_time_step, one event pair per launch, 300 launches)")
    lines.append(f"  time_step launch, dual time on    {1e6 * per_launch[True]:8.2f} us   (k_time_step_src<2, false>, the same way)")
    lines.append(f"  ratio                             {per_launch[True] / per_launch[False]:8.2f}")
    t = alternated(s, settings, lambda n: s.smooth(0, n), a.sweeps, a.warmup, a.batches, a.dt)
    for k, name in zip(settings, names):
        lines.append(f"  time per sweep, {name:34s} {1e6 * t[k]:8.2f} us")
    s.close()

    sizes = tuple(int(x) for x in a.sizes.split(","))
    mg = meshgen.make_multigrid(sizes, "m6wing", seed=0, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    t = alternated(s, settings, lambda n: s.run_cycles(n), a.cycles, a.warmup, a.batches, a.dt)
    lines.append(f"{len(sizes)}-level hierarchy {'/'.join(str(n) + '^3' for n in sizes)}:")
    for k, name in zip(settings, names):
        lines.append(f"  time per V-cycle, {name:34s} {1e3 * t[k]:8.4f} ms")
    s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
