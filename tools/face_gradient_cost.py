#!/usr/bin/env python3
"""What the corrected face gradient (mgcfd_set_face_gradient) costs, on bench.py's 4-level hierarchy (67^3/55^3/48^3/43^3) built
with cavity_radius = 0.2 so that level 0 has solid walls, with the viscous terms and no-slip walls on level 0, by the method of
tools/wall_heat_cost.py (event pairs over back-to-back launches, alternated batches, medians):

  * the node-gradient launch and the correction launch (mgcfd_bench_face_gradient kinds 0, 1) against the stress launch and the
    viscous-flux launch (mgcfd_bench_viscous kinds 0, 1) of the same session, with the bytes each moves per node and per edge;
  * the Spalart-Allmaras transport launch (mgcfd_bench_sa kind 1) with and without Qdc;
  * a level-0 sweep (mgcfd_smooth) and a V-cycle, corrected against averaged, both at MGCFD_VISCOUS_CFL_CORRECTED;
  * all of it --runs times over (a fresh solver each): the median and the spread (min .. max) of the runs;
  * with --baseline DIR (the repository root of another build, the parent commit's say): the V-cycle with every optional term
    off, this build's and that build's, a child process per run, alternated; and with --bench as well, bench.py --gpus 1
    --steps 2000 --warmup 200 of both builds, alternated in the same way.

Writes the figures to --out (default profiles/face_gradient_cost.txt) and prints them.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFL_V = 0.2                                                  # MGCFD_VISCOUS_CFL_CORRECTED, for either mode: the same step limit
LAUNCHES = ("stress launch", "viscous-flux launch", "node-gradient launch", "correction launch")
# doubles a launch reads + writes per node (the state's five or the staged fields, the sums' targets), and per incidence-row
# entry: a 2-byte code and three 8-byte weights; an internal edge has two entries
NODE_DOUBLES = {"stress launch": 5 + 1 + 12, "viscous-flux launch": 12 + 4 + 4, "node-gradient launch": 5 + 1 + 14,
                "correction launch": 5 + 14 + 3 + 4 + 4}
ENTRY_BYTES = 2 + 3 * 8


def hierarchy(meshgen, a):
    sizes = tuple(int(x) for x in a.sizes.split(","))
    return meshgen.make_multigrid(sizes, "m6wing", seed=0, cavity_radius=a.cavity_radius, jitter=0.2, area_noise=0.02, volume_noise=0.02)


def timed(s, a, run, n):
    """median seconds per unit of ``run(n)`` over the batches, each from the far field"""
    mach, alpha = s.free_stream()
    t = []
    for b in range(a.batches + 1):
        s.set_free_stream(mach, alpha, reinitialise=True)
        run(max(n // 3, 1)); s.synchronize()
        t0 = time.perf_counter(); run(n); s.synchronize()
        if b > 0:
            t.append((time.perf_counter() - t0) / n)
    return statistics.median(t)


def vcycle_off(mgcfd, meshgen, a):
    mg = hierarchy(meshgen, a)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    t = timed(s, a, lambda n: s.run_cycles(n), a.cycles)
    s.close()
    return t


def one_run(mgcfd, meshgen, a):
    out = {}
    mg = hierarchy(meshgen, a)
    levels = mgcfd.generated_to_levels(mg)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    s.set_viscous(a.mu, wall=True, cfl_v=CFL_V, levels=1)
    s.set_face_gradient("corrected")
    out["shape"] = (s.nel(0), int(levels[0]["n_internal"]))
    got = {name: [] for name in LAUNCHES}
    s.run_cycles(2)
    for _ in range(a.batches):                             # alternated
        got["stress launch"].append(s.bench_viscous(0, 0, a.launches))
        got["viscous-flux launch"].append(s.bench_viscous(0, 1, a.launches))
        got["node-gradient launch"].append(s.bench_face_gradient(0, "nodes", a.launches))
        got["correction launch"].append(s.bench_face_gradient(0, "correction", a.launches))
    s.zero_fluxes(0)
    for k, v in got.items():
        out[k] = statistics.median(v)
    for mode in ("averaged", "corrected"):
        s.set_face_gradient(mode)
        out["sweep", mode] = timed(s, a, lambda n: s.smooth(0, n), a.cycles)
        out["cycle", mode] = timed(s, a, lambda n: s.run_cycles(n), a.cycles)
    # the Spalart-Allmaras transport launch, with and without Qdc
    s.set_viscosity_model(law="sutherland", eddy="spalart-allmaras")
    sa = {"averaged": [], "corrected": []}
    for _ in range(a.batches):
        for mode in sa:
            s.set_face_gradient(mode)
            sa[mode].append(s.bench_sa(0, "transport", a.launches))
    for mode, v in sa.items():
        out["sa", mode] = statistics.median(v)
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mu", type=float, default=1e-3)
    ap.add_argument("--sizes", default="67,55,48,43")
    ap.add_argument("--cavity-radius", type=float, default=0.2)
    ap.add_argument("--cycles", type=int, default=60)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50, help="launches per event pair")
    ap.add_argument("--cfl", type=float, default=1.0, help="local steps at this CFL number")
    ap.add_argument("--baseline", default=None, help="the repository root of another build: its V-cycle with everything off, alternated with this one's")
    ap.add_argument("--bench", action="store_true", help="with --baseline: bench.py --gpus 1 --steps 2000 --warmup 200 of both builds too")
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--child-vcycle", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "face_gradient_cost.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.root, "mg-cfd-app-plain_amd"))
    import mgcfd
    from mgcfd import meshgen
    if a.child_vcycle:
        print("VCYCLE_SECONDS", repr(vcycle_off(mgcfd, meshgen, a)))
        return

    def child(root):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-vcycle", "--root", os.path.abspath(root), "--sizes", a.sizes,
                            "--cavity-radius", str(a.cavity_radius), "--cycles", str(a.cycles), "--batches", str(a.batches), "--cfl", str(a.cfl)],
                           capture_output=True, text=True, check=True, timeout=600)
        return float([l for l in r.stdout.splitlines() if l.startswith("VCYCLE_SECONDS")][0].split()[1])

    def bench(root):
        root = os.path.abspath(root)
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2000", "--warmup", "200"], capture_output=True,
                           text=True, check=True, timeout=900, cwd=root)
        return float(json.loads([l for l in r.stdout.splitlines() if l.startswith("{") and '"metric"' in l][-1])["value"])

    runs, here, base, bench_here, bench_base = [], [], [], [], []
    for _ in range(a.runs):
        runs.append(one_run(mgcfd, meshgen, a))
        if a.baseline:
            here.append(child(a.root))
            base.append(child(a.baseline))
            if a.bench:
                bench_here.append(bench(a.root))
                bench_base.append(bench(a.baseline))

    def line(name, vals, scale, unit, extra=""):
        return f"  {name:<46s}{scale * statistics.median(vals):9.3f} {unit}   (runs: min {scale * min(vals):.3f} .. max {scale * max(vals):.3f}){extra}"

    col = lambda k: [r[k] for r in runs]
    med = lambda k: statistics.median(col(k))
    nel, n_int = runs[0]["shape"]
    lines = [f"Corrected face gradient on the {'/'.join(x + '^3' for x in a.sizes.split(','))} hierarchy, cavity_radius {a.cavity_radius}, mu = {a.mu}, "
             f"cfl_v = {CFL_V}, the viscous terms with no-slip walls on level 0; {a.runs} runs of a fresh solver each, per run medians of {a.batches} "
             "batches; below: median of the runs and their spread",
             f"launches on level 0 ({nel} nodes, {n_int} internal edges), {a.launches} per event pair; bytes: per node the doubles read and "
             f"written, per edge two row entries of {ENTRY_BYTES} B (neighbour fields come from LDS):"]
    for name in LAUNCHES:
        node_bytes = 8 * NODE_DOUBLES[name]
        total = node_bytes * nel + 2 * ENTRY_BYTES * n_int
        lines.append(line(name, col(name), 1e6, "us", f"; {node_bytes} B/node + {2 * ENTRY_BYTES} B/edge = {total / 1e6:.1f} MB, "
                                                      f"{total / med(name) / 1e12:.2f} TB/s"))
    lines.append(f"  the two new launches together against stress + viscous flux: "
                 f"{(med('node-gradient launch') + med('correction launch')) / (med('stress launch') + med('viscous-flux launch')):.3f}")
    lines.append("Spalart-Allmaras transport launch (k_sa_transport_tile), Sutherland:")
    lines.append(line("without Qdc (averaged)", col(("sa", "averaged")), 1e6, "us"))
    lines.append(line("with Qdc (corrected)", col(("sa", "corrected")), 1e6, "us", f"; ratio {med(('sa', 'corrected')) / med(('sa', 'averaged')):.3f}"))
    lines.append("time per level-0 sweep and per V-cycle, level 0 viscous:")
    for key, unit in (("sweep", "level-0 sweep"), ("cycle", "V-cycle")):
        lines.append(line(f"{unit}, averaged", col((key, "averaged")), 1e3, "ms"))
        lines.append(line(f"{unit}, corrected", col((key, "corrected")), 1e3, "ms", f"; ratio {med((key, 'corrected')) / med((key, 'averaged')):.3f}"))
    if base:
        inside = min(base) <= statistics.median(here) <= max(base)
        lines.append("time per V-cycle, everything off; a child process per run and build, alternated:")
        lines.append(line("this build", here, 1e3, "ms"))
        lines.append(line("the baseline build", base, 1e3, "ms", f"; this build's median lies {'inside' if inside else 'outside'} the baseline's own range"))
    if bench_base:
        inside = min(bench_base) <= statistics.median(bench_here) <= max(bench_base)
        lines.append("bench.py --gpus 1 --steps 2000 --warmup 200, alternated in the same way:")
        lines.append(line("this build", bench_here, 1.0, "Medges/s", "; " + ", ".join(f"{v:.0f}" for v in bench_here)))
        lines.append(line("the baseline build", bench_base, 1.0, "Medges/s", "; " + ", ".join(f"{v:.0f}" for v in bench_base) +
                          f"; this build's median lies {'inside' if inside else 'outside'} the baseline's own range"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
