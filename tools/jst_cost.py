#!/usr/bin/env python3
"""What the JST dissipation (mgcfd_set_jst) costs, for (kappa2, kappa4) = (2.5, 0.15625) on level 0 by default, on the bench
level (bench.py's 67^3 lattice, 300,763 nodes) and on the 4-level hierarchy of bench.py's V-cycle:

  * time per sensor launch and per dissipation launch, each as back-to-back launches under one event pair (mgcfd_bench_jst),
    beside the level's standalone bit-identical flux launch measured the same way in the same process (mgcfd_bench_flux), with
    the spread (min .. max) of the batches;
  * time per sweep of the bench level, JST on and off;
  * time per V-cycle of the hierarchy, JST on (level 0) and off;
  * the cost ratio per sweep and per cycle.

The method of tools/residual_smoothing_cost.py: clocks warm (a warm-up batch before every measurement), many launches per
measurement (one event pair, or one synchronisation per batch of sweeps or cycles), alternated batches and their median.
Sweeps and cycles are host-timed around a batch: that is what a caller pays, launch overhead included.  The state is
re-initialised before every batch so that on and off time the same flow.  With --fvcorr DIR (the input directory of the
fvcorr_1lvl golden case) it also records, in profiles/jst_fvcorr.txt, the CL/CD and RMS history of that case over --fvcorr-cycles
cycles with JST off and with the defaults.  Writes the figures to --out (default profiles/jst_cost.txt) and prints them.
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
    """median seconds per call of `run` under every (kappa2, kappa4, levels) of `settings`, in alternated batches"""
    t = {k: [] for k in settings}
    mach, alpha = s.free_stream()
    for b in range(batches + 1):
        for k in settings:
            s.set_jst(*k)
            s.set_free_stream(mach, alpha, reinitialise=True)
            dt = timed(s, run, n, warmup)
            if b > 0:                                          # (the first round warms up)
                t[k].append(dt)
    return {k: statistics.median(v) for k, v in t.items()}


def fvcorr_record(directory, cycles, on, out):
    """RMS, CD and CL of fvcorr_1lvl at every `cycles / 20`-th cycle, JST off and on, under the reference's time step."""
    lines = [f"fvcorr_1lvl, {cycles} cycles under the reference's time step: JST off against (kappa2, kappa4, levels) = {on}",
             "cycle |        RMS off         CD off         CL off |         RMS on          CD on          CL on"]
    hist = {}
    for setting in ((0.0, 0.0, 0), on):
        mesh = mgcfd.Mesh("input.dat", directory, 1)
        s = mgcfd.Solver.from_mesh(mesh)
        s.set_jst(*setting)
        try:
            rms, loads = s.run_cycles(cycles, loads=True)
            coeff = s.load_coefficients(loads)                  # [cycles, 6]: CD CL CS CMx CMy CMz
            hist[setting] = (rms, coeff, None)
        except mgcfd.MgcfdError as e:
            hist[setting] = (None, None, f"{e} (cycle {s.invalid_state_location()[1] + 1})")
        s.close(); mesh.close()
    for setting, (rms, coeff, err) in hist.items():
        if err:
            lines.append(f"{setting}: the run went invalid: {err}")
    if all(h[2] is None for h in hist.values()):
        (r0, c0, _), (r1, c1, _) = hist[(0.0, 0.0, 0)], hist[on]
        step = max(1, cycles // 20)
        for c in list(range(step - 1, cycles, step)):
            lines.append(f"{c + 1:5d} | {r0[c]:14.6e} {c0[c][0]:14.6e} {c0[c][1]:14.6e} | {r1[c]:14.6e} {c1[c][0]:14.6e} {c1[c][1]:14.6e}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kappa2", type=float, default=2.5)
    ap.add_argument("--kappa4", type=float, default=0.15625)
    ap.add_argument("--lattice", type=int, default=67)
    ap.add_argument("--sizes", default="67,55,48,43")
    ap.add_argument("--sweeps", type=int, default=300)
    ap.add_argument("--cycles", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200, help="launches per event pair")
    ap.add_argument("--cfl", type=float, default=1.0, help="local steps at this CFL number, JST on and off (the flow stays at the far field)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jst_cost.txt"))
    ap.add_argument("--fvcorr", default=None, help="input directory of the fvcorr_1lvl golden case: also record profiles/jst_fvcorr.txt")
    ap.add_argument("--fvcorr-cycles", type=int, default=200)
    ap.add_argument("--fvcorr-out", default=os.path.join(ROOT, "profiles", "jst_fvcorr.txt"))
    a = ap.parse_args()
    on, off = (a.kappa2, a.kappa4, 1), (0.0, 0.0, 0)
    lines = [f"JST dissipation, (kappa2, kappa4, levels) = {on}; medians of {a.batches} alternated batches"]

    mg = meshgen.make_multigrid((a.lattice,), "m6wing", seed=0, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    t = alternated(s, [on, off], lambda n: s.smooth(0, n), a.sweeps, a.warmup, a.batches)
    s.set_jst(*on)
    s.smooth(0, a.warmup)
    launch, flux = {k: [] for k in range(2)}, []
    for _ in range(a.batches):                                 # alternated: flux, sensor, dissipation
        flux.append(s.bench_flux(0, a.launches))
        for k in launch:
            launch[k].append(s.bench_jst(0, k, a.launches))
    lines.append(f"bench level {a.lattice}^3 = {s.nel(0)} nodes, {s.tiling(0)['tiles']} tiles:")
    for k, name in enumerate(("sensor launch     ", "dissipation launch")):
        lines.append(f"  JST {name}            {1e6 * statistics.median(launch[k]):8.2f} us   (min {1e6 * min(launch[k]):.2f} .. max {1e6 * max(launch[k]):.2f}; "
                     f"{a.launches} launches per event pair)")
    lines.append(f"  standalone bit-identical flux     {1e6 * statistics.median(flux):8.2f} us   (min {1e6 * min(flux):.2f} .. max {1e6 * max(flux):.2f}; "
                 f"mgcfd_bench_flux, same process, same way)")
    lines.append(f"  time per sweep, JST on            {1e6 * t[on]:8.2f} us")
    lines.append(f"  time per sweep, JST off           {1e6 * t[off]:8.2f} us   (fused stages)")
    lines.append(f"  ratio per sweep                   {t[on] / t[off]:8.2f}")
    s.close()

    sizes = tuple(int(x) for x in a.sizes.split(","))
    mg = meshgen.make_multigrid(sizes, "m6wing", seed=0, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    t = alternated(s, [on, off], lambda n: s.run_cycles(n), a.cycles, a.warmup, a.batches)
    lines.append(f"{len(sizes)}-level hierarchy {'/'.join(str(n) + '^3' for n in sizes)}:")
    lines.append(f"  time per V-cycle, JST on level 0  {1e3 * t[on]:8.4f} ms")
    lines.append(f"  time per V-cycle, JST off         {1e3 * t[off]:8.4f} ms")
    lines.append(f"  cost ratio per cycle              {t[on] / t[off]:8.2f}")
    s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if a.fvcorr:
        fvcorr_record(a.fvcorr, a.fvcorr_cycles, on, a.fvcorr_out)


if __name__ == "__main__":
    main()
