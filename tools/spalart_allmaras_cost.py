#!/usr/bin/env python3
"""What the Spalart-Allmaras model (mgcfd_set_viscosity_model with MGCFD_EDDY_SPALART_ALLMARAS) costs, on bench.py's 4-level
hierarchy (67^3/55^3/48^3/43^3) built with cavity_radius = 0.2 so that every level has solid walls, with the method of
tools/wall_distance_cost.py:

  * pass 1 (k_sa_gradient_tile) and pass 2 (k_sa_transport_tile) on level 0 and k_sa_restrict into level 1: back-to-back launches
    under one event pair (mgcfd_bench_sa), against the stress launch under (constant, none) in the same process
    (mgcfd_bench_viscous kind 0), each with its algorithmic bytes: per node what the kernel reads and writes of its own node, per
    edge the two incidences' code and weights (2 x (2 + 24) B); halo staging is not counted;
  * a sweep of level 0 and a V-cycle, all levels viscous with no-slip walls, under the model against constant viscosity;
  * all of it --runs times over (a fresh solver each): the median and the spread (min .. max) of the runs;
  * with --baseline DIR (the mg-cfd-app-plain_amd directory of another build, the parent commit's say): the V-cycle with every
    optional term off, this build's and that build's, a child process per run, alternated.

--resources appends the compiler's resource report of the new kernels and the stress kernel (tools/kernel_resources.py; needs hipcc
and no GPU) to --out.  Writes the figures to --out (default profiles/spalart_allmaras_cost.txt) and prints them.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_BYTES = 2 * (2 + 24)
# own-node bytes: stress reads W (40) and vol (8), writes S (96); pass 1 reads W (40), nt (8), vol (8), writes sa_gradient (40) and
# mut (8); pass 2 reads rho and the momentum (32), nt (8), sa_gradient (40), d, vol, g, sf, nt_old (40), writes nt (8)
NODE_BYTES = {"stress": 144, "gradient": 104, "transport": 128}


def hierarchy(meshgen, a):
    sizes = tuple(int(x) for x in a.sizes.split(","))
    return meshgen.make_multigrid(sizes, "m6wing", seed=0, cavity_radius=a.cavity_radius, jitter=0.2, area_noise=0.02, volume_noise=0.02)


def timed_cycles(s, a, what):
    """median seconds per V-cycle (what = "cycle") or per sweep of level 0 ("sweep") over the batches"""
    mach, alpha = s.free_stream()
    t = []
    for b in range(a.batches + 1):
        s.set_free_stream(mach, alpha, reinitialise=True)
        run = (lambda n: s.run_cycles(n)) if what == "cycle" else (lambda n: s.smooth(0, n))
        run(a.warmup); s.synchronize()
        t0 = time.perf_counter(); run(a.cycles); s.synchronize()
        if b > 0:
            t.append((time.perf_counter() - t0) / a.cycles)
    return statistics.median(t)


def vcycle_off(mgcfd, meshgen, a):
    mg = hierarchy(meshgen, a)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    t = timed_cycles(s, a, "cycle")
    s.close()
    return t


def one_run(mgcfd, meshgen, a):
    out = {}
    mg = hierarchy(meshgen, a)
    levels = mgcfd.generated_to_levels(mg)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    out["shape"] = [(s.nel(l), int(levels[l]["n_internal"])) for l in range(s.num_levels)]
    s.set_viscous(a.mu, wall=True, levels=s.num_levels)
    got = {k: [] for k in ("stress", "gradient", "transport", "restrict")}
    for _ in range(a.batches):                             # alternated
        s.set_viscosity_model()
        s.smooth(0, 2)
        got["stress"].append(s.bench_viscous(0, 0, a.launches))
        s.set_viscosity_model(eddy="spalart-allmaras")
        s.smooth(0, 2)
        got["gradient"].append(s.bench_sa(0, "gradient", a.launches))
        got["transport"].append(s.bench_sa(0, "transport", a.launches))
        got["restrict"].append(s.bench_sa(1, "restrict", a.launches))
    for k, v in got.items():
        out[k] = statistics.median(v)
    for model in ("none", "spalart-allmaras"):
        s.set_viscosity_model(eddy=model)
        out["sweep", model] = timed_cycles(s, a, "sweep")
        out["cycle", model] = timed_cycles(s, a, "cycle")
    s.close()
    return out


def resources():
    lines = ["compiler's resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; tools/kernel_resources.py):"]
    for k, flt in enumerate(("k_sa_gradient_tile", "k_sa_transport_tile", "k_sa_restrict", "k_sa_init", "k_viscous_stress_tile")):
        env = dict(os.environ, NS="sa" if flt.startswith("k_sa_") else "exact")       # (the model's kernels are kernels_sa.hip's)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), flt], capture_output=True, text=True, check=True, env=env)
        rows = r.stdout.splitlines()
        lines += [("  " + l.split("(")[0]) for l in (rows if k == 0 else rows[1:])]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spalart_allmaras_cost.txt"))
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
    nel, n_int = runs[0]["shape"][0]
    nbytes = {k: v * nel + EDGE_BYTES * n_int for k, v in NODE_BYTES.items()}
    stress = statistics.median(col("stress"))
    spread = 100 * (max(col("stress")) - min(col("stress"))) / stress
    lines = [f"Spalart-Allmaras model on the {'/'.join(x + '^3' for x in a.sizes.split(','))} hierarchy, cavity_radius {a.cavity_radius}, mu = {a.mu}, "
             f"no-slip walls, all levels viscous; {a.runs} runs of a fresh solver each, per run medians of {a.batches} batches; below: median of the "
             "runs and their spread",
             f"launches on level 0 ({nel} nodes, {n_int} internal edges), {a.launches} per event pair; bytes: own node + {EDGE_BYTES} per edge:",
             line(f"stress launch, (constant, none): {NODE_BYTES['stress']} B/node", col("stress"), 1e6, "us", f"; {nbytes['stress'] / 1e6:.1f} MB; run-to-run spread {spread:.2f} %")]
    for k, label in (("gradient", "pass 1, k_sa_gradient_tile"), ("transport", "pass 2, k_sa_transport_tile")):
        t = statistics.median(col(k))
        lines.append(line(f"{label}: {NODE_BYTES[k]} B/node", col(k), 1e6, "us",
                          f"; {nbytes[k] / 1e6:.1f} MB; time ratio to the stress launch {t / stress:.3f}, byte ratio {nbytes[k] / nbytes['stress']:.3f}"))
    lines.append(line(f"k_sa_restrict into level 1 ({runs[0]['shape'][1][0]} nodes)", col("restrict"), 1e6, "us"))
    for what, label, scale, unit in (("sweep", "sweep of level 0", 1e6, "us"), ("cycle", "V-cycle", 1e3, "ms")):
        lines.append(f"{label}, all levels viscous:")
        lines.append(line("constant viscosity", col((what, "none")), scale, unit))
        lines.append(line("Spalart-Allmaras", col((what, "spalart-allmaras")), scale, unit,
                          f"; ratio {statistics.median(col((what, 'spalart-allmaras'))) / statistics.median(col((what, 'none'))):.3f}"))
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
