#!/usr/bin/env python3
"""What the unsteady Spalart-Allmaras model (mgcfd_set_sa_unsteady) costs, on bench.py's 4-level hierarchy (67^3/55^3/48^3/43^3)
built with cavity_radius = 0.2 so that every level has solid walls, with the method of tools/spalart_allmaras_cost.py:

  * the timed pass 2 (k_sa_transport_tile<.., SaStepTimed>, BDF2) against the plain pass 2 of the same build, and the shielded pass 1
    (k_sa_gradient_tile<.., true>) against the plain pass 1: back-to-back launches under one event pair (mgcfd_bench_sa), alternated
    in one process, each with its algorithmic bytes: per node what the kernel reads and writes of its own node, per edge the two
    incidences' code and weights (2 x (2 + 24) B); halo staging is not counted;
  * a sweep of level 0 and a V-cycle, all levels viscous with no-slip walls, under the model with each setting: RANS, DES97, delayed
    DES, and each of them with dual time stepping and time_accurate;
  * all of it --runs times over (a fresh solver each): the median and the spread (min .. max) of the runs;
  * with --baseline DIR (the mg-cfd-app-plain_amd directory of another build, the parent commit's say): the V-cycle with every
    optional term off, this build's and that build's, a child process per run, alternated.

--resources appends the compiler's resource report of the model's kernels (tools/kernel_resources.py; needs hipcc and no GPU) to
--out.  Writes the figures to --out (default profiles/sa_unsteady_cost.txt) and prints them.  Nothing is gated on.
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import spalart_allmaras_cost as sac  # noqa: E402

EDGE_BYTES = sac.EDGE_BYTES
# own-node bytes: pass 1 as tools/spalart_allmaras_cost.py counts it (104), shielded also d and delta read and d~ written (24 more);
# pass 2 (128), timed also ntn and ntn1 under BDF2 (16 more)
NODE_BYTES = {"gradient": 104, "gradient_shield": 128, "transport": 128, "transport_timed": 144}
DT = 0.05
SETTINGS = (("RANS", False, "wall"), ("DES97", False, "des"), ("delayed DES", False, "ddes"),
            ("RANS, dual time", True, "wall"), ("DES97, dual time", True, "des"), ("delayed DES, dual time", True, "ddes"))


def one_run(mgcfd, meshgen, a):
    out = {}
    mg = sac.hierarchy(meshgen, a)
    levels = mgcfd.generated_to_levels(mg)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    out["shape"] = [(s.nel(l), int(levels[l]["n_internal"])) for l in range(s.num_levels)]
    s.set_viscous(a.mu, wall=True, levels=s.num_levels)
    s.set_viscosity_model(eddy="spalart-allmaras")
    got = {k: [] for k in NODE_BYTES}
    for _ in range(a.batches):                             # alternated
        s.set_dual_time(0.0)
        s.set_sa_unsteady(False, "wall")
        s.smooth(0, 2)
        got["gradient"].append(s.bench_sa(0, "gradient", a.launches))
        got["transport"].append(s.bench_sa(0, "transport", a.launches))
        s.set_sa_unsteady(True, "ddes")
        s.set_dual_time(DT)
        s.advance(2, 1)                                    # (two time levels held: BDF2)
        assert s.dual_time()["levels"] == 2
        got["gradient_shield"].append(s.bench_sa(0, "gradient", a.launches))
        s.set_sa_unsteady(True, "wall")
        got["transport_timed"].append(s.bench_sa(0, "transport", a.launches))
    for k, v in got.items():
        out[k] = statistics.median(v)
    for name, timed, length in SETTINGS:
        s.set_dual_time(0.0)
        s.set_sa_unsteady(timed, length)
        if timed:
            s.set_dual_time(DT)
        out["sweep", name] = sac.timed_cycles(s, a, "sweep")
        out["cycle", name] = sac.timed_cycles(s, a, "cycle")
    s.close()
    return out


def resources():
    lines = ["compiler's resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; tools/kernel_resources.py):"]
    for k, flt in enumerate(("k_sa_gradient_tile", "k_sa_transport_tile", "k_sa_length")):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), flt], capture_output=True, text=True, check=True,
                           env=dict(os.environ, NS="sa"))
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sa_unsteady_cost.txt"))
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
        print("VCYCLE_SECONDS", repr(sac.vcycle_off(mgcfd, meshgen, a)))
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
        return f"  {name:<58s}{scale * statistics.median(vals):9.3f} {unit}   (runs: min {scale * min(vals):.3f} .. max {scale * max(vals):.3f}){extra}"

    col = lambda k: [r[k] for r in runs]
    nel, n_int = runs[0]["shape"][0]
    nbytes = {k: v * nel + EDGE_BYTES * n_int for k, v in NODE_BYTES.items()}
    lines = [f"Unsteady Spalart-Allmaras model on the {'/'.join(x + '^3' for x in a.sizes.split(','))} hierarchy, cavity_radius {a.cavity_radius}, "
             f"mu = {a.mu}, no-slip walls, all levels viscous; {a.runs} runs of a fresh solver each, per run medians of {a.batches} batches; "
             "below: median of the runs and their spread",
             f"launches on level 0 ({nel} nodes, {n_int} internal edges), {a.launches} per event pair; bytes: own node + {EDGE_BYTES} per edge:"]
    for plain, new, label in (("transport", "transport_timed", "pass 2"), ("gradient", "gradient_shield", "pass 1")):
        tp, tn = statistics.median(col(plain)), statistics.median(col(new))
        spread = 100 * (max(col(plain)) - min(col(plain))) / tp
        lines.append(line(f"{label}, plain: {NODE_BYTES[plain]} B/node", col(plain), 1e6, "us", f"; {nbytes[plain] / 1e6:.1f} MB; run-to-run spread {spread:.2f} %"))
        lines.append(line(f"{label}, {'timed (BDF2)' if plain == 'transport' else 'shielded (delayed DES)'}: {NODE_BYTES[new]} B/node", col(new), 1e6, "us",
                          f"; {nbytes[new] / 1e6:.1f} MB; time ratio to the plain launch {tn / tp:.3f}, byte ratio {nbytes[new] / nbytes[plain]:.3f}"))
    for what, label, scale, unit in (("sweep", "sweep of level 0", 1e6, "us"), ("cycle", "V-cycle", 1e3, "ms")):
        lines.append(f"{label}, all levels viscous, (constant, SA):")
        ref = statistics.median(col((what, SETTINGS[0][0])))
        for name, _, _ in SETTINGS:
            lines.append(line(name, col((what, name)), scale, unit, f"; ratio to RANS {statistics.median(col((what, name))) / ref:.3f}"))
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
