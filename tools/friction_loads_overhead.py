#!/usr/bin/env python3
"""What the viscous surface loads (mgcfd_surface_loads_viscous, mgcfd_run_cycles_loads_viscous) cost, with the methods of
tools/loads_overhead.py and tools/viscous_cost.py, all in one process and session.

On bench.py's 4-level M6-like hierarchy (67^3/55^3/48^3/43^3 lattices) built with cavity_radius = 0.2, so that level 0 has solid
walls, with the viscous terms on level 0:
  * the time per launch of k_wall_stress, k_surface_loads_viscous and, beside them, k_surface_loads and the tile stress launch
    (k_viscous_stress_tile): from `rocprofv3 --kernel-trace --stats` in a child run of its own (--no-profile skips it), and as
    back-to-back launches under one event pair (mgcfd_bench_friction_loads, mgcfd_bench_viscous), the four alternated batch by
    batch, median and spread of the batches — for kernels this short the second is the rate at which launches can follow one
    another more than the kernel's own time;
  * the V-cycle with the friction loads recorded, with the pressure loads recorded and with no loads, alternated batch by batch
    (median and best batch);
  * with --baseline DIR (the mg-cfd-app-plain_amd directory of another build, the parent commit's say): the V-cycle with
    everything off of this build and of that one, a child process per run, alternated, with the batch-to-batch spread of each.
Writes the figures to --out (default profiles/friction_loads_cost.txt) and prints them.
"""
import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(mgcfd, meshgen, a):
    sizes = tuple(int(x) for x in a.sizes.split(","))
    mg = meshgen.make_multigrid(sizes, "m6wing", seed=0, cavity_radius=a.cavity_radius, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    levels = mgcfd.generated_to_levels(mg)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    return s, levels


def batch_times(s, run, a):
    """seconds per cycle of every timed batch of `run` (the state re-initialised before each, one warm-up batch first)"""
    mach, alpha = s.free_stream()
    t = []
    for b in range(a.batches + 1):
        s.set_free_stream(mach, alpha, reinitialise=True)
        run(a.warmup)
        t0 = time.perf_counter()
        run(a.cycles)
        if b > 0:
            t.append((time.perf_counter() - t0) / a.cycles)
    return t


def spread(vals, scale):
    return f"{scale * statistics.median(vals):9.4f}   (min {scale * min(vals):.4f} .. max {scale * max(vals):.4f})"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="67,55,48,43")
    ap.add_argument("--cavity-radius", type=float, default=0.2)
    ap.add_argument("--mu", type=float, default=1e-3)
    ap.add_argument("--no-slip", action="store_true")
    ap.add_argument("--cfl", type=float, default=1.0, help="local steps at this CFL number")
    ap.add_argument("--cycles", type=int, default=25, help="cycles per timed batch")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, default=20, help="timed batches of each kind, alternated")
    ap.add_argument("--launches", type=int, default=200, help="launches per event pair")
    ap.add_argument("--runs", type=int, default=3, help="child runs of each build for the V-cycle with everything off")
    ap.add_argument("--baseline", default=None, help="the mg-cfd-app-plain_amd directory of another build")
    ap.add_argument("--package", default=os.path.join(ROOT, "mg-cfd-app-plain_amd"), help=argparse.SUPPRESS)
    ap.add_argument("--child-vcycle", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--kernel-only", action="store_true", help="(the profiled child) cycles with friction and with pressure loads, then exit")
    ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "friction_loads_cost.txt"))
    a = ap.parse_args()
    sys.path.insert(0, a.package)
    import mgcfd
    from mgcfd import meshgen

    if a.child_vcycle:
        s, _ = build(mgcfd, meshgen, a)
        print("VCYCLE_BATCHES", " ".join(repr(t) for t in batch_times(s, lambda n: s.run_cycles(n), a)))
        s.close()
        return

    s, levels = build(mgcfd, meshgen, a)
    ref = (0.5, 0.5, 0.5)
    s.set_viscous(a.mu, wall=a.no_slip, levels=1)
    if a.kernel_only:
        s.run_cycles(a.cycles, loads=True, ref_point=ref, friction=True)
        s.run_cycles(a.cycles, loads=True, ref_point=ref)
        s.close()
        return
    s.run_cycles(a.warmup)
    kinds = {"k_wall_stress": lambda: s.bench_friction_loads(0, 0, a.launches),
             "k_surface_loads_viscous": lambda: s.bench_friction_loads(0, 1, a.launches),
             "k_surface_loads": lambda: s.bench_friction_loads(0, 2, a.launches),
             "k_viscous_stress_tile": lambda: s.bench_viscous(0, 0, a.launches)}
    for f in kinds.values():
        f()
    kernel = {k: [] for k in kinds}
    for _ in range(a.batches):
        for k, f in kinds.items():
            kernel[k].append(f())
    cycle = {"friction": [], "pressure": [], "none": []}
    runs = {"friction": lambda n: s.run_cycles(n, loads=True, ref_point=ref, friction=True),
            "pressure": lambda n: s.run_cycles(n, loads=True, ref_point=ref), "none": lambda n: s.run_cycles(n)}
    mach, alpha = s.free_stream()
    order = list(runs)
    for b in range(a.batches + 1):
        for k in (order if b % 2 == 0 else order[::-1]):
            s.set_free_stream(mach, alpha, reinitialise=True)
            runs[k](a.warmup)
            t0 = time.perf_counter()
            runs[k](a.cycles)
            if b > 0:
                cycle[k].append((time.perf_counter() - t0) / a.cycles)
    n_wall, n_nodes = int(levels[0]["n_boundary"]), s.wall_node_count(0)
    s.close()

    off = {"this": [], "baseline": []}
    if a.baseline:
        for _ in range(a.runs):
            for who, package in (("this", a.package), ("baseline", a.baseline)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-vcycle", "--package", package, "--sizes", a.sizes,
                                    "--cavity-radius", str(a.cavity_radius), "--cycles", str(a.cycles), "--warmup", str(a.warmup),
                                    "--batches", str(a.batches), "--cfl", str(a.cfl)], capture_output=True, text=True, check=True, timeout=600)
                off[who] += [float(x) for x in [l for l in r.stdout.splitlines() if l.startswith("VCYCLE_BATCHES")][0].split()[1:]]

    profiled = None
    kernels = ("k_wall_stress", "k_surface_loads_viscous", "k_surface_loads", "k_viscous_stress_tile")
    if not a.no_profile and shutil.which("rocprofv3"):
        d = tempfile.mkdtemp(prefix="friction_prof_")
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--kernel-only", "--sizes", a.sizes, "--cavity-radius", str(a.cavity_radius), "--cycles", str(a.cycles), "--mu", str(a.mu),
               "--cfl", str(a.cfl)] + (["--no-slip"] if a.no_slip else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        profiled = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                for k in kernels:
                    if row["Name"].split("(")[0].split("<")[0].split("::")[-1].split()[-1] == k:
                        c, t, lo, hi = profiled.get(k, (0, 0.0, float("inf"), 0.0))
                        profiled[k] = (c + int(row["Calls"]), t + float(row["AverageNs"]) * int(row["Calls"]),
                                       min(lo, float(row.get("MinNs", "inf"))), max(hi, float(row.get("MaxNs", 0.0))))
        if r.returncode != 0 or not profiled:
            profiled = {"error": f"rocprofv3 exit {r.returncode}: {r.stderr[-300:]}"}
        shutil.rmtree(d, ignore_errors=True)

    med = lambda v: statistics.median(v)
    pair = med(kernel["k_wall_stress"]) + med(kernel["k_surface_loads_viscous"])
    old = med(kernel["k_viscous_stress_tile"]) + med(kernel["k_surface_loads"])
    lines = [f"viscous surface loads on the {'/'.join(x + '^3' for x in a.sizes.split(','))} hierarchy, cavity_radius {a.cavity_radius}: level 0 has "
             f"{levels[0]['nel']} nodes, {n_wall} solid-wall edges on {n_nodes} wall nodes; viscous terms on level 0 (mu {a.mu}, "
             f"{'no-slip' if a.no_slip else 'slip'} walls), local steps at CFL {a.cfl}, bit-identical mode",
             "kernel time, rocprofv3 --kernel-trace --stats in a child run of its own (us): mean (min .. max), launches"] + \
            ([f"  {profiled['error']}"] if profiled is not None and "error" in profiled else
             ["  not measured"] if profiled is None else
             [f"  {k:<44s}{v[1] / v[0] / 1e3:9.3f}   ({v[2] / 1e3:.3f} .. {v[3] / 1e3:.3f}), {v[0]}" for k, v in profiled.items()]) + [
             f"time per launch, {a.launches} back-to-back launches per event pair, median of {a.batches} alternated batches (us):"]
    lines += [f"  {k:<44s}{spread(v, 1e6)}" for k, v in kernel.items()]
    lines += [f"  k_wall_stress + k_surface_loads_viscous     {1e6 * pair:9.4f}",
              f"  k_viscous_stress_tile + k_surface_loads     {1e6 * old:9.4f}   (what the friction loads would cost through the tile stress launch)",
              f"time per V-cycle, {a.cycles} cycles per batch, median of {a.batches} alternated batches (ms):"]
    names = {"friction": "pressure and friction loads recorded", "pressure": "pressure loads recorded", "none": "no loads"}
    lines += [f"  {names[k]:<44s}{spread(cycle[k], 1e3)}   best {1e3 * min(cycle[k]):.4f}" for k in cycle]
    lines += [f"  friction loads against pressure loads       {100.0 * (med(cycle['friction']) / med(cycle['pressure']) - 1.0):+9.2f} %",
              f"  friction loads against no loads             {100.0 * (med(cycle['friction']) / med(cycle['none']) - 1.0):+9.2f} %"]
    if a.baseline:
        lines += [f"time per V-cycle with everything off, {a.runs} child runs of each build, alternated, {a.batches} batches each (ms):",
                  f"  this build                                  {spread(off['this'], 1e3)}",
                  f"  the baseline build                          {spread(off['baseline'], 1e3)}",
                  f"  this build against the baseline             {100.0 * (med(off['this']) / med(off['baseline']) - 1.0):+9.2f} %"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
