#!/usr/bin/env python3
"""What the wall distance (mgcfd_compute_wall_distance, mgcfd_set_wall_damping) costs, on bench.py's 4-level hierarchy
(67^3/55^3/48^3/43^3) built with cavity_radius = 0.2 so that every level has solid walls, with the method of
tools/variable_viscosity_cost.py:

  * k_wall_distance per level: back-to-back launches under one event pair (mgcfd_bench_wall_distance), the pair evaluations
    nel x m per second, and that rate as fp64 vector instructions per second (8 arithmetic + 1 compare per pair) against the
    card's vector fp64 peak;
  * the stress launch on level 0 under (constant, smagorinsky), damped against undamped, alternated in one process
    (mgcfd_bench_viscous kind 0): the two read the same bytes per node;
  * all of it --runs times over (a fresh solver each): the median and the spread (min .. max) of the runs;
  * with --baseline DIR (the mg-cfd-app-plain_amd directory of another build, the parent commit's say): the V-cycle with every
    optional term off, this build's and that build's, a child process per run, alternated.

--resources appends the compiler's resource report of the new kernels and the stress kernel (tools/kernel_resources.py; needs hipcc
and no GPU) to --out.  Writes the figures to --out (default profiles/wall_distance_cost.txt) and prints them.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# fp64 vector peak of the card: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3e12 instructions/s (78.6 TFLOP/s counts an FMA as two;
# half the FP32 vector figure of the micro-architecture tables)
FP64_VECTOR_INSTRUCTIONS = 256 * 4 * 16 * 2.4e9
FP64_PER_PAIR = 9          # 3 subtractions, 3 products, 2 additions, 1 compare (the select of best / near is three 32-bit moves more)


def hierarchy(meshgen, a):
    sizes = tuple(int(x) for x in a.sizes.split(","))
    return meshgen.make_multigrid(sizes, "m6wing", seed=0, cavity_radius=a.cavity_radius, jitter=0.2, area_noise=0.02, volume_noise=0.02)


def vcycle_off(mgcfd, meshgen, a):
    """median seconds per V-cycle with every optional term off (what a build without them runs too)"""
    mg = hierarchy(meshgen, a)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    mach, alpha = s.free_stream()
    t = []
    for b in range(a.batches + 1):
        s.set_free_stream(mach, alpha, reinitialise=True)
        s.run_cycles(a.warmup); s.synchronize()
        t0 = time.perf_counter(); s.run_cycles(a.cycles); s.synchronize()
        if b > 0:
            t.append((time.perf_counter() - t0) / a.cycles)
    s.close()
    return statistics.median(t)


def one_run(mgcfd, meshgen, a):
    out = {}
    mg = hierarchy(meshgen, a)
    levels = mgcfd.generated_to_levels(mg)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    t0 = time.perf_counter()
    s.compute_wall_distance()
    out["compute_all"] = time.perf_counter() - t0          # (with the host's permutation, the uploads and the frees)
    out["shape"] = [(s.nel(l), s.wall_node_count(l), int(levels[l]["n_boundary"])) for l in range(s.num_levels)]
    for l in range(s.num_levels):
        s.bench_wall_distance(l, a.launches)               # (warm)
        out["distance", l] = statistics.median(s.bench_wall_distance(l, a.launches) for _ in range(a.batches))
    s.set_viscous(a.mu, levels=1)
    s.set_viscosity_model(eddy="smagorinsky")
    got = {False: [], True: []}
    for _ in range(a.batches):                             # alternated
        for damped in (False, True):
            s.set_wall_damping(damped)
            s.smooth(0, 2)
            got[damped].append(s.bench_viscous(0, 0, a.launches))
    out["stress", False], out["stress", True] = statistics.median(got[False]), statistics.median(got[True])
    s.close()
    return out


def resources():
    lines = ["compiler's resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; tools/kernel_resources.py), the exact build:"]
    for flt in ("k_wall_distance", "k_wall_spacing", "k_wall_length", "k_viscous_stress_tile"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), flt], capture_output=True, text=True, check=True)
        rows = r.stdout.splitlines()
        lines += [("  " + l.split("(")[0]) for l in (rows if flt == "k_wall_distance" else rows[1:])]
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mu", type=float, default=1e-3)
    ap.add_argument("--sizes", default="67,55,48,43")
    ap.add_argument("--cavity-radius", type=float, default=0.2)
    ap.add_argument("--cycles", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50, help="launches per event pair")
    ap.add_argument("--cfl", type=float, default=1.0, help="local steps at this CFL number (the flow stays at the far field)")
    ap.add_argument("--baseline", default=None, help="the mg-cfd-app-plain_amd directory of another build: its V-cycle, alternated with this one's")
    ap.add_argument("--package", default=os.path.join(ROOT, "mg-cfd-app-plain_amd"), help=argparse.SUPPRESS)
    ap.add_argument("--child-vcycle", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--resources", action="store_true", help="append the compiler's resource report to --out and stop (no GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wall_distance_cost.txt"))
    a = ap.parse_args()
    if a.resources:
        text = "\n".join(resources()) + "\n"
        print(text, end="")
        with open(a.out, "a") as f:
            f.write(text)
        return
    sys.path.insert(0, a.package)
    import mgcfd
    from mgcfd import meshgen
    if a.child_vcycle:
        print("VCYCLE_SECONDS", repr(vcycle_off(mgcfd, meshgen, a)))
        return

    def child(package):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-vcycle", "--package", package, "--sizes", a.sizes,
                            "--cavity-radius", str(a.cavity_radius), "--cycles", str(a.cycles), "--warmup", str(a.warmup),
                            "--batches", str(a.batches), "--cfl", str(a.cfl)], capture_output=True, text=True, check=True, timeout=600)
        return float([l for l in r.stdout.splitlines() if l.startswith("VCYCLE_SECONDS")][0].split()[1])

    runs, here, base = [], [], []
    for _ in range(a.runs):
        runs.append(one_run(mgcfd, meshgen, a))
        if a.baseline:
            here.append(child(a.package))
            base.append(child(a.baseline))

    def line(name, vals, scale, unit, extra=""):
        return f"  {name:<46s}{scale * statistics.median(vals):9.3f} {unit}   (runs: min {scale * min(vals):.3f} .. max {scale * max(vals):.3f}){extra}"

    col = lambda k: [r[k] for r in runs]
    shape = runs[0]["shape"]
    lines = [f"wall distance on the {'/'.join(x + '^3' for x in a.sizes.split(','))} hierarchy, cavity_radius {a.cavity_radius}; {a.runs} runs of a "
             f"fresh solver each, per run medians of {a.batches} batches of {a.launches} launches per event pair; below: median of the runs and their spread",
             "k_wall_distance (nodes x wall nodes = pair evaluations; fp64 vector instructions at 9 per pair against the card's "
             f"{FP64_VECTOR_INSTRUCTIONS / 1e12:.1f}e12 per second):"]
    for l, (nel, m, nb) in enumerate(shape):
        t = statistics.median(col(("distance", l)))
        pairs = nel * m
        lines.append(line(f"level {l}: {nel} x {m} ({nb} solid-wall edges)", col(("distance", l)), 1e6, "us",
                          f"; {pairs / t / 1e12:.3f}e12 pairs/s, {100 * FP64_PER_PAIR * pairs / t / FP64_VECTOR_INSTRUCTIONS:.1f} % of the fp64 vector peak"))
    lines.append(line("mgcfd_compute_wall_distance, all levels, whole call", col("compute_all"), 1e3, "ms", "; host permutation, uploads, launches, frees"))
    lines.append(f"stress launch on level 0 ({shape[0][0]} nodes) under (constant, smagorinsky), mu = {a.mu}:")
    lines.append(line("undamped", col(("stress", False)), 1e6, "us"))
    lines.append(line("damped", col(("stress", True)), 1e6, "us"))
    u = col(("stress", False))
    lines.append(f"  damped / undamped: {statistics.median(col(('stress', True))) / statistics.median(u):.4f} (run-to-run spread of the undamped launch "
                 f"{100 * (max(u) - min(u)) / statistics.median(u):.2f} %)")
    if base:
        lines.append("time per V-cycle, everything off; a child process per run and build, alternated:")
        lines.append(line("this build", here, 1e3, "ms"))
        lines.append(line("the baseline build", base, 1e3, "ms"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
