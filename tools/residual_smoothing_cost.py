#!/usr/bin/env python3
"""What implicit residual smoothing (mgcfd_set_residual_smoothing) costs, for (eps, iterations) = (0.5, 2) by default, on the
bench level (bench.py's 67^3 lattice, 300,763 nodes) and on the 4-level hierarchy of bench.py's V-cycle:

  * time per smoothing launch, each kind (first / middle / last iteration) as back-to-back launches under one event pair
    (mgcfd_bench_residual_smoothing), beside the level's standalone bit-identical flux launch measured the same way in the
    same process (mgcfd_bench_flux);
  * time per sweep of the bench level, smoothing on and off;
  * time per V-cycle of the hierarchy, smoothing on and off;
  * the cost ratio per cycle.

Clocks warm (a warm-up batch before every measurement), many launches per measurement (one event pair, or one synchronisation
per batch of sweeps or cycles), alternated batches and their median.  Sweeps and cycles are host-timed around a batch: that
is what a caller pays, launch overhead included.  The state is re-initialised before every batch so that on and off
time the same flow.  Writes the figures to --out (default profiles/residual_smoothing_cost.txt) and prints them.
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


def alternated(s, settings, run, n, warmup, batches):
    """median seconds per call of `run` under every (eps, iterations) of `settings`, in alternated batches"""
    t = {k: [] for k in settings}
    mach, alpha = s.free_stream()
    for b in range(batches + 1):
        for k in settings:
            s.set_residual_smoothing(*k)
            s.set_free_stream(mach, alpha, reinitialise=True)
            dt = timed(s, run, n, warmup)
            if b > 0:                                          # (the first round warms up)
                t[k].append(dt)
    return {k: statistics.median(v) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--eps", type=float, default=0.5)
    ap.add_argument("--iterations", type=int, default=2)
    ap.add_argument("--lattice", type=int, default=67)
    ap.add_argument("--sizes", default="67,55,48,43")
    ap.add_argument("--sweeps", type=int, default=300)
    ap.add_argument("--cycles", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200, help="launches per event pair")
    ap.add_argument("--cfl", type=float, default=1.0, help="local steps at this CFL number, smoothing on and off (the flow stays at the far field)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "residual_smoothing_cost.txt"))
    a = ap.parse_args()
    on, off = (a.eps, a.iterations), (0.0, 0)
    lines = [f"implicit residual smoothing, (eps, iterations) = {on}; medians of {a.batches} alternated batches"]

    mg = meshgen.make_multigrid((a.lattice,), "m6wing", seed=0, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    t = alternated(s, [on, off], lambda n: s.smooth(0, n), a.sweeps, a.warmup, a.batches)
    s.set_residual_smoothing(*on)
    s.smooth(0, a.warmup)
    launch, flux = {k: [] for k in range(3)}, []
    for _ in range(a.batches):                                 # alternated: flux, first, middle, last
        flux.append(s.bench_flux(0, a.launches))
        for k in launch:
            launch[k].append(s.bench_residual_smoothing(0, k, a.launches))
    flux = statistics.median(flux)
    lines.append(f"bench level {a.lattice}^3 = {s.nel(0)} nodes, {s.tiling(0)['tiles']} tiles:")
    for k, name in enumerate(("first iteration ", "middle iteration", "last iteration  ")):
        lines.append(f"  smoothing launch, {name}  {1e6 * statistics.median(launch[k]):8.2f} us   ({a.launches} launches per event pair)")
    lines.append(f"  standalone bit-identical flux     {1e6 * flux:8.2f} us   (mgcfd_bench_flux, same process, same way)")
    lines.append(f"  time per sweep, smoothing on      {1e6 * t[on]:8.2f} us")
    lines.append(f"  time per sweep, smoothing off     {1e6 * t[off]:8.2f} us   (fused stages)")
    lines.append(f"  ratio per sweep                   {t[on] / t[off]:8.2f}")
    s.close()

    sizes = tuple(int(x) for x in a.sizes.split(","))
    mg = meshgen.make_multigrid(sizes, "m6wing", seed=0, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    t = alternated(s, [on, off], lambda n: s.run_cycles(n), a.cycles, a.warmup, a.batches)
    lines.append(f"{len(sizes)}-level hierarchy {'/'.join(str(n) + '^3' for n in sizes)}:")
    lines.append(f"  time per V-cycle, smoothing on    {1e3 * t[on]:8.4f} ms")
    lines.append(f"  time per V-cycle, smoothing off   {1e3 * t[off]:8.4f} ms")
    lines.append(f"  cost ratio per cycle              {t[on] / t[off]:8.2f}")
    s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
