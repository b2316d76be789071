#!/usr/bin/env python3
"""What the laminar viscous terms (mgcfd_set_viscous) cost, on the bench level (bench.py's 67^3 lattice, 300,763 nodes) and on
the 4-level hierarchy of bench.py's V-cycle, with the method of tools/jst_cost.py:

  * time per stress launch and per viscous-flux launch, each as back-to-back launches under one event pair
    (mgcfd_bench_viscous), beside the level's standalone bit-identical flux launch (mgcfd_bench_flux) and the JST dissipation
    launch (mgcfd_bench_jst) measured the same way in the same process, each with its algorithmic bytes;
  * time per sweep of the bench level, viscous terms on and off;
  * time per V-cycle of the hierarchy, viscous terms on (level 0) and off;
  * all of it --runs times over (a fresh solver each), the median and the spread (min .. max) of the runs;
  * with --baseline DIR (the mg-cfd-app-plain_amd directory of another build, the parent commit's say): that build's V-cycle,
    timed by a child process per run in alternation with this build's V-cycle with the terms off.

Clocks warm (a warm-up batch before every measurement), many launches per measurement (one event pair, or one synchronisation per
batch of sweeps or cycles), alternated batches and their median.  Sweeps and cycles are host-timed around a batch: that is what a
caller pays, launch overhead included.  The state is re-initialised before every batch so that on and off time the same flow (the
uniform far field: the launches do the same work on any state).  Writes the figures to --out (default
profiles/viscous_cost.txt) and prints them.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(s, run, n, warmup):
    run(warmup); s.synchronize()
    t0 = time.perf_counter(); run(n); s.synchronize()
    return (time.perf_counter() - t0) / n


def vcycle_off(mgcfd, meshgen, a):
    """median seconds per V-cycle of the hierarchy with every optional term off (what a build without them runs too)"""
    sizes = tuple(int(x) for x in a.sizes.split(","))
    mg = meshgen.make_multigrid(sizes, "m6wing", seed=0, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    mach, alpha = s.free_stream()
    t = []
    for b in range(a.batches + 1):
        s.set_free_stream(mach, alpha, reinitialise=True)
        dt = timed(s, lambda n: s.run_cycles(n), a.cycles, a.warmup)
        if b > 0:
            t.append(dt)
    s.close()
    return statistics.median(t)


def alternated(s, settings, apply, run, n, warmup, batches):
    """median seconds per call of `run` under every setting of `settings` (applied by `apply`), in alternated batches"""
    t = {k: [] for k in settings}
    mach, alpha = s.free_stream()
    for b in range(batches + 1):
        for k in settings:
            apply(k)
            s.set_free_stream(mach, alpha, reinitialise=True)
            dt = timed(s, run, n, warmup)
            if b > 0:                                          # (the first round warms up)
                t[k].append(dt)
    return {k: statistics.median(v) for k, v in t.items()}


def one_run(mgcfd, meshgen, a):
    """every figure of one run, in seconds (and the level's node, edge and tile counts)"""
    out = {}
    on, off = (a.mu, a.prandtl, bool(a.no_slip), a.viscous_cfl, 1), None

    def apply(s):
        return lambda k: s.set_viscous(*k) if k else s.set_viscous(0.0, levels=0)

    mg = meshgen.make_multigrid((a.lattice,), "m6wing", seed=0, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    levels = mgcfd.generated_to_levels(mg)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    t = alternated(s, [on, off], apply(s), lambda n: s.smooth(0, n), a.sweeps, a.warmup, a.batches)
    out["sweep_on"], out["sweep_off"] = t[on], t[off]
    s.set_viscous(*on)
    s.set_jst(levels=1)
    s.smooth(0, a.warmup)
    kinds = {"flux": lambda: s.bench_flux(0, a.launches), "stress": lambda: s.bench_viscous(0, 0, a.launches),
             "vflux": lambda: s.bench_viscous(0, 1, a.launches), "jst": lambda: s.bench_jst(0, 1, a.launches)}
    got = {k: [] for k in kinds}
    for _ in range(a.batches):                                 # alternated
        for k, f in kinds.items():
            got[k].append(f())
    for k in kinds:
        out[k] = statistics.median(got[k])
    out["nodes"], out["edges"], out["tiles"] = s.nel(0), int(levels[0]["n_internal"]), s.tiling(0)["tiles"]
    s.close()

    sizes = tuple(int(x) for x in a.sizes.split(","))
    mg = meshgen.make_multigrid(sizes, "m6wing", seed=0, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    t = alternated(s, [on, off], apply(s), lambda n: s.run_cycles(n), a.cycles, a.warmup, a.batches)
    out["cycle_on"], out["cycle_off"] = t[on], t[off]
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mu", type=float, default=1e-3)
    ap.add_argument("--prandtl", type=float, default=0.72)
    ap.add_argument("--viscous-cfl", type=float, default=0.25)
    ap.add_argument("--no-slip", action="store_true")
    ap.add_argument("--lattice", type=int, default=67)
    ap.add_argument("--sizes", default="67,55,48,43")
    ap.add_argument("--sweeps", type=int, default=300)
    ap.add_argument("--cycles", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200, help="launches per event pair")
    ap.add_argument("--cfl", type=float, default=1.0, help="local steps at this CFL number, on and off (the flow stays at the far field)")
    ap.add_argument("--baseline", default=None, help="the mg-cfd-app-plain_amd directory of another build: its V-cycle, alternated with this one's")
    ap.add_argument("--package", default=os.path.join(ROOT, "mg-cfd-app-plain_amd"), help=argparse.SUPPRESS)
    ap.add_argument("--child-vcycle", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "viscous_cost.txt"))
    a = ap.parse_args()
    sys.path.insert(0, a.package)
    import mgcfd
    from mgcfd import meshgen
    if a.child_vcycle:
        print("VCYCLE_SECONDS", repr(vcycle_off(mgcfd, meshgen, a)))
        return

    runs, base = [], []
    for _ in range(a.runs):
        runs.append(one_run(mgcfd, meshgen, a))
        if a.baseline:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-vcycle", "--package", a.baseline, "--sizes", a.sizes,
                                "--cycles", str(a.cycles), "--warmup", str(a.warmup), "--batches", str(a.batches), "--cfl", str(a.cfl)],
                               capture_output=True, text=True, check=True, timeout=600)
            base.append(float([l for l in r.stdout.splitlines() if l.startswith("VCYCLE_SECONDS")][0].split()[1]))

    def line(name, vals, scale, unit, extra=""):
        return f"  {name:<44s}{scale * statistics.median(vals):9.3f} {unit}   (runs: min {scale * min(vals):.3f} .. max {scale * max(vals):.3f}){extra}"

    n, e = runs[0]["nodes"], runs[0]["edges"]
    mb = {"flux": (40 * e + 80 * n) / 1e6, "jst": (176 * n + 20 * e) / 1e6, "stress": (144 * n + 52 * e) / 1e6, "vflux": (160 * n + 52 * e) / 1e6}
    col = lambda k: [r[k] for r in runs]
    lines = [f"laminar viscous terms, (mu, prandtl, wall, cfl_v, levels) = ({a.mu}, {a.prandtl}, {int(a.no_slip)}, {a.viscous_cfl}, 1); "
             f"{a.runs} runs of a fresh solver each, per run medians of {a.batches} alternated batches; below: median of the runs and their spread",
             f"bench level {a.lattice}^3 = {n} nodes, {e} internal edges, {runs[0]['tiles']} tiles; {a.launches} launches per event pair:",
             line("viscous stress launch", col("stress"), 1e6, "us", f"; {mb['stress']:.1f} MB: 144 B per node (W, volume, S) + 52 B per edge (2 x (code + three weights))"),
             line("viscous flux launch", col("vflux"), 1e6, "us", f"; {mb['vflux']:.1f} MB: 160 B per node (S, four fluxes read and written) + 52 B per edge"),
             line("standalone bit-identical flux launch", col("flux"), 1e6, "us", f"; {mb['flux']:.1f} MB: 80 B per node + 40 B per edge (as bench.py prices it)"),
             line("JST dissipation launch", col("jst"), 1e6, "us", f"; {mb['jst']:.1f} MB: 176 B per node + 20 B per edge"),
             f"  viscous flux launch / JST dissipation launch   time {statistics.median(col('vflux')) / statistics.median(col('jst')):.2f}, bytes {mb['vflux'] / mb['jst']:.2f}",
             line("time per sweep, viscous on", col("sweep_on"), 1e6, "us"),
             line("time per sweep, viscous off (fused stages)", col("sweep_off"), 1e6, "us"),
             f"  ratio per sweep                             {statistics.median(col('sweep_on')) / statistics.median(col('sweep_off')):9.2f}",
             f"{len(a.sizes.split(','))}-level hierarchy {'/'.join(x + '^3' for x in a.sizes.split(','))}:",
             line("time per V-cycle, viscous on level 0", col("cycle_on"), 1e3, "ms"),
             line("time per V-cycle, viscous off", col("cycle_off"), 1e3, "ms")]
    if base:
        lines.append(line("time per V-cycle, the baseline build", base, 1e3, "ms", "; a child process per run, alternated with the runs above"))
    lines.append(f"  cost ratio per cycle                        {statistics.median(col('cycle_on')) / statistics.median(col('cycle_off')):9.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
