#!/usr/bin/env python3
"""What the upwind flux (mgcfd_set_upwind) costs, Venkatakrishnan's limiter at the defaults on level 0 by default, on the bench
level (bench.py's 67^3 lattice, 300,763 nodes) and on the 4-level hierarchy of bench.py's V-cycle:

  * time per gradient launch (pass 1) and per flux launch (pass 2) in both instantiations, each as back-to-back launches under
    one event pair (mgcfd_bench_upwind), beside the level's standalone bit-identical flux launch (mgcfd_bench_flux) and JST's
    two launches (mgcfd_bench_jst) measured the same way in the same process, with the spread (min .. max) of the batches;
  * the bytes each launch moves at least, per node and per internal edge;
  * time per sweep of the bench level and per V-cycle of the hierarchy, upwind on (level 0, MUSCL) against off.

The method of tools/jst_cost.py: clocks warm (a warm-up batch before every measurement), many launches per measurement (one
event pair, or one synchronisation per batch of sweeps or cycles), alternated batches and their median.  Sweeps and cycles are
host-timed around a batch: that is what a caller pays, launch overhead included.  The state is re-initialised before every
batch so that on and off time the same flow.  With --fvcorr DIR (the input directory of the fvcorr_1lvl golden case) it also
records, in profiles/upwind_fvcorr.txt, the RMS, CL and CD history of that case over --fvcorr-cycles cycles under the reference
scheme, the JST defaults and the upwind flux (the level's coordinates are read from its .coords file here: the mesh loader
leaves them out of a single-level fvcorr input).  Writes the figures to --out (default profiles/upwind_cost.txt) and prints them.
"""
import argparse
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mg-cfd-app-plain_amd"))

import numpy as np                                             # noqa: E402

import mgcfd                                                   # noqa: E402
from mgcfd import meshgen                                      # noqa: E402

ON, OFF = (1, 1, "venkatakrishnan"), (0, 0, "none")
# what a launch moves at least, in bytes: per node its own loads and stores (halo copies come on top), per internal edge the two
# ends' row entries (a 2-byte code and three 8-byte weights; pass 1 reads the codes a second time for the limiter)
TRAFFIC = (("gradient (pass 1)", 8 * (5 + 3 + 1) + 8 * 20, 2 * (26 + 2)),
           ("flux, MUSCL (pass 2)", 8 * (5 + 3 + 15) + 8 * 10, 2 * 26),
           ("flux, first order (pass 2)", 8 * 5 + 8 * 10, 2 * 26))


def timed(s, run, n, warmup):
    run(warmup); s.synchronize()
    t0 = time.perf_counter(); run(n); s.synchronize()
    return (time.perf_counter() - t0) / n


def alternated(s, settings, run, n, warmup, batches):
    """median seconds per call of `run` under every (levels, muscl_levels, limiter) of `settings`, in alternated batches"""
    t = {k: [] for k in settings}
    mach, alpha = s.free_stream()
    for b in range(batches + 1):
        for k in settings:
            s.set_upwind(*k)
            s.set_free_stream(mach, alpha, reinitialise=True)
            dt = timed(s, run, n, warmup)
            if b > 0:                                          # (the first round warms up)
                t[k].append(dt)
    return {k: statistics.median(v) for k, v in t.items()}


def fvcorr_record(directory, cycles, out):
    """RMS, CD and CL of fvcorr_1lvl at every `cycles / 20`-th cycle under the three schemes, the reference's time step."""
    names = ("reference", "JST", "upwind")
    lines = [f"fvcorr_1lvl, {cycles} cycles under the reference's time step: the reference's scheme, the JST defaults on level 0 and "
             f"the upwind flux (levels, muscl_levels, limiter) = {ON} at k = {mgcfd.api.UPWIND_VENKAT_K}, entropy_fix = {mgcfd.api.UPWIND_ENTROPY_FIX}",
             "cycle | " + " | ".join(f"{'RMS ' + n:>16s} {'CD ' + n:>16s} {'CL ' + n:>16s}" for n in names)]
    hist = {}
    step = max(1, cycles // 20)
    for name in names:
        mesh = mgcfd.Mesh("input.dat", directory, 1)
        level = dict(mesh.level(0))
        if level.get("coords") is None or len(level["coords"]) == 0:      # (a single-level fvcorr input is loaded without its .coords file)
            files = glob.glob(os.path.join(directory, "*.coords"))
            assert len(files) == 1, "one .coords file beside the single level"
            level["coords"] = np.loadtxt(files[0]).reshape(level["nel"], 3)
        s = mgcfd.Solver.from_arrays([level], mesh.variant)
        if name == "JST":
            s.set_jst()
        if name == "upwind":
            s.set_upwind(*ON)
        rms_all, coeff_all, err = [], [], None
        try:
            for c0 in range(0, cycles, step):                   # (in chunks: a run that goes invalid keeps its history up to there)
                rms, loads = s.run_cycles(min(step, cycles - c0), loads=True)
                rms_all += list(rms)
                coeff_all += list(s.load_coefficients(loads))   # rows of 6: CD CL CS CMx CMy CMz
        except mgcfd.MgcfdError as e:
            err = f"{e}"
        hist[name] = (rms_all, coeff_all, err)
        s.close(); mesh.close()
    for name, (rms, _, err) in hist.items():
        if err:
            lines.append(f"{name}: the run went invalid after {len(rms) // step * step} recorded cycles, within the next {step}: {err}")
    for c in range(step - 1, cycles, step):
        cells = []
        for name in names:
            rms, coeff, _ = hist[name]
            cells.append(" " * 50 if c >= len(rms) else f"{rms[c]:16.6e} {coeff[c][0]:16.6e} {coeff[c][1]:16.6e}")
        lines.append(f"{c + 1:5d} | " + " | ".join(cells))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lattice", type=int, default=67)
    ap.add_argument("--sizes", default="67,55,48,43")
    ap.add_argument("--sweeps", type=int, default=300)
    ap.add_argument("--cycles", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200, help="launches per event pair")
    ap.add_argument("--cfl", type=float, default=1.0, help="local steps at this CFL number, on and off (the flow stays at the far field)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upwind_cost.txt"))
    ap.add_argument("--fvcorr", default=None, help="input directory of the fvcorr_1lvl golden case: also record profiles/upwind_fvcorr.txt")
    ap.add_argument("--fvcorr-only", action="store_true", help="record the fvcorr history alone (needs --fvcorr)")
    ap.add_argument("--fvcorr-cycles", type=int, default=200)
    ap.add_argument("--fvcorr-out", default=os.path.join(ROOT, "profiles", "upwind_fvcorr.txt"))
    a = ap.parse_args()
    if a.fvcorr_only:
        fvcorr_record(a.fvcorr, a.fvcorr_cycles, a.fvcorr_out)
        return
    lines = [f"Upwind flux, (levels, muscl_levels, limiter) = {ON}; medians of {a.batches} alternated batches"]

    mg = meshgen.make_multigrid((a.lattice,), "m6wing", seed=0, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    t = alternated(s, [ON, OFF], lambda n: s.smooth(0, n), a.sweeps, a.warmup, a.batches)
    s.set_upwind(*ON)
    s.smooth(0, a.warmup)
    names = ("upwind gradient launch (pass 1)   ", "upwind flux launch, MUSCL         ", "upwind flux launch, first order   ",
             "standalone bit-identical flux     ", "JST sensor launch                 ", "JST dissipation launch            ")
    got = {k: [] for k in names}
    for _ in range(a.batches):                                 # alternated: the six launches in turn
        s.set_upwind(*ON)
        got[names[0]].append(s.bench_upwind(0, 0, a.launches))
        got[names[1]].append(s.bench_upwind(0, 1, a.launches))
        s.set_upwind(1, 0, "none")
        got[names[2]].append(s.bench_upwind(0, 1, a.launches))
        s.set_upwind(0)
        got[names[3]].append(s.bench_flux(0, a.launches))
        s.set_jst()
        got[names[4]].append(s.bench_jst(0, 0, a.launches))
        got[names[5]].append(s.bench_jst(0, 1, a.launches))
        s.set_jst(levels=0)
    lines.append(f"bench level {a.lattice}^3 = {s.nel(0)} nodes, {s.tiling(0)['tiles']} tiles:")
    for k in names:
        lines.append(f"  {k}{1e6 * statistics.median(got[k]):8.2f} us   (min {1e6 * min(got[k]):.2f} .. max {1e6 * max(got[k]):.2f}; "
                     f"{a.launches} launches per event pair)")
    lines.append("  bytes moved at least (own loads and stores per node; row entries per internal edge, both ends):")
    for name, per_node, per_edge in TRAFFIC:
        lines.append(f"    {name:28s}{per_node:4d} B per node  {per_edge:3d} B per edge")
    lines.append(f"  time per sweep, upwind on         {1e6 * t[ON]:8.2f} us   (per stage: memset, boundary faces, pass 1, pass 2, update)")
    lines.append(f"  time per sweep, upwind off        {1e6 * t[OFF]:8.2f} us   (fused stages)")
    lines.append(f"  ratio per sweep                   {t[ON] / t[OFF]:8.2f}")
    s.close()

    sizes = tuple(int(x) for x in a.sizes.split(","))
    mg = meshgen.make_multigrid(sizes, "m6wing", seed=0, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    t = alternated(s, [ON, OFF], lambda n: s.run_cycles(n), a.cycles, a.warmup, a.batches)
    lines.append(f"{len(sizes)}-level hierarchy {'/'.join(str(n) + '^3' for n in sizes)}:")
    lines.append(f"  time per V-cycle, upwind on level 0 {1e3 * t[ON]:8.4f} ms")
    lines.append(f"  time per V-cycle, upwind off        {1e3 * t[OFF]:8.4f} ms")
    lines.append(f"  cost ratio per cycle                {t[ON] / t[OFF]:8.2f}")
    s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    if a.fvcorr:
        fvcorr_record(a.fvcorr, a.fvcorr_cycles, a.fvcorr_out)


if __name__ == "__main__":
    main()
