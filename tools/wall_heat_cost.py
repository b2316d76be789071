#!/usr/bin/env python3
"""What the wall thermal conditions and the heat loads (mgcfd_set_wall_temperature, mgcfd_surface_loads_heat, mgcfd_wall_heat)
cost, on bench.py's 4-level hierarchy (67^3/55^3/48^3/43^3) built with cavity_radius = 0.2 so that level 0 has solid walls, with
the viscous terms and no-slip walls on level 0, by the method of tools/friction_loads_overhead.py (event pairs over back-to-back
launches, alternated batches, medians):

  * the isothermal wall launch against the adiabatic one, and the heat-flux wall's launch (mgcfd_bench_wall_heat kinds 0, 1, 2);
  * the fourteen-column loads kernel against the twelve-column one (mgcfd_bench_wall_heat kind 3, mgcfd_bench_friction_loads
    kind 1), and k_wall_heat (kind 4);
  * a V-cycle under the adiabatic, the isothermal and the heat-flux wall, without loads and with the heat loads recorded every cycle;
  * all of it --runs times over (a fresh solver each): the median and the spread (min .. max) of the runs;
  * with --baseline DIR (the repository root of another build, the parent commit's say): the V-cycle with every optional term
    off, this build's and that build's, a child process per run, alternated; and with --bench as well, bench.py --gpus 1
    --steps 2000 --warmup 200 of both builds, alternated in the same way.

Writes the figures to --out (default profiles/wall_heat_cost.txt) and prints them.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (("adiabatic", 0.0), ("isothermal", None), ("heat-flux", 0.05))     # (None: 1.5 times the static free-stream temperature)
KINDS = (("isothermal wall launch", 0), ("adiabatic wall launch", 1), ("heat-flux wall launch", 2), ("fourteen-column loads", 3), ("k_wall_heat", 4))


def hierarchy(meshgen, a):
    sizes = tuple(int(x) for x in a.sizes.split(","))
    return meshgen.make_multigrid(sizes, "m6wing", seed=0, cavity_radius=a.cavity_radius, jitter=0.2, area_noise=0.02, volume_noise=0.02)


def timed_cycles(s, a, heat=False):
    """median seconds per V-cycle over the batches, each from the far field"""
    mach, alpha = s.free_stream()
    t = []
    run = (lambda n: s.run_cycles(n, loads=True, heat=True)) if heat else (lambda n: s.run_cycles(n))
    for b in range(a.batches + 1):
        s.set_free_stream(mach, alpha, reinitialise=True)
        run(a.warmup); s.synchronize()
        t0 = time.perf_counter(); run(a.cycles); s.synchronize()
        if b > 0:
            t.append((time.perf_counter() - t0) / a.cycles)
    return statistics.median(t)


def vcycle_off(mgcfd, meshgen, a):
    mg = hierarchy(meshgen, a)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    t = timed_cycles(s, a)
    s.close()
    return t


def one_run(mgcfd, meshgen, a):
    out = {}
    mg = hierarchy(meshgen, a)
    levels = mgcfd.generated_to_levels(mg)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    s.set_viscous(a.mu, wall=True, levels=1)
    out["shape"] = (s.nel(0), int(levels[0]["n_boundary"]), s.wall_node_count(0))
    t_wall = 1.5 * mgcfd.free_stream_temperature(s.far_field())[0]
    got = {name: [] for name, _ in KINDS}
    got["twelve-column loads"] = []
    s.run_cycles(2)
    for _ in range(a.batches):                             # alternated
        for name, kind in KINDS:
            got[name].append(s.bench_wall_heat(0, kind, a.launches))
        got["twelve-column loads"].append(s.bench_friction_loads(0, 1, a.launches))
    s.zero_fluxes(0)
    for k, v in got.items():
        out[k] = statistics.median(v)
    for mode, value in MODES:
        s.set_wall_temperature(mode, t_wall if value is None else value)
        for key, heat in (("cycle", False), ("cycle+loads", True)):
            try:
                out[key, mode] = timed_cycles(s, a, heat=heat)
            except mgcfd.MgcfdError as e:                  # (an invalid state is reported as such, not timed)
                print(f"{mode} wall: {e}", file=sys.stderr)
                out[key, mode] = float("nan")
    s.close()
    return out


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
    ap.add_argument("--cfl", type=float, default=1.0, help="local steps at this CFL number")
    ap.add_argument("--baseline", default=None, help="the repository root of another build: its V-cycle with everything off, alternated with this one's")
    ap.add_argument("--bench", action="store_true", help="with --baseline: bench.py --gpus 1 --steps 2000 --warmup 200 of both builds too")
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    ap.add_argument("--child-vcycle", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wall_heat_cost.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(a.root, "mg-cfd-app-plain_amd"))
    import mgcfd
    from mgcfd import meshgen
    if a.child_vcycle:
        print("VCYCLE_SECONDS", repr(vcycle_off(mgcfd, meshgen, a)))
        return

    def child(root):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-vcycle", "--root", os.path.abspath(root), "--sizes", a.sizes,
                            "--cavity-radius", str(a.cavity_radius), "--cycles", str(a.cycles), "--warmup", str(a.warmup),
                            "--batches", str(a.batches), "--cfl", str(a.cfl)], capture_output=True, text=True, check=True, timeout=600)
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
    nel, n_edges, n_nodes = runs[0]["shape"]
    lines = [f"Wall thermal conditions on the {'/'.join(x + '^3' for x in a.sizes.split(','))} hierarchy, cavity_radius {a.cavity_radius}, mu = {a.mu}, "
             f"the viscous terms with no-slip walls on level 0; {a.runs} runs of a fresh solver each, per run medians of {a.batches} batches; below: median "
             "of the runs and their spread",
             f"launches on level 0 ({nel} nodes, {n_edges} solid-wall edges on {n_nodes} wall nodes), {a.launches} per event pair:",
             line("adiabatic wall launch (k_viscous_wall)", col("adiabatic wall launch"), 1e6, "us"),
             line("isothermal wall launch", col("isothermal wall launch"), 1e6, "us", f"; ratio {med('isothermal wall launch') / med('adiabatic wall launch'):.3f}"),
             line("heat-flux wall launch (k_wall_heat_flux)", col("heat-flux wall launch"), 1e6, "us"),
             line("twelve-column loads", col("twelve-column loads"), 1e6, "us"),
             line("fourteen-column loads", col("fourteen-column loads"), 1e6, "us", f"; ratio {med('fourteen-column loads') / med('twelve-column loads'):.3f}"),
             line("k_wall_heat", col("k_wall_heat"), 1e6, "us"),
             "time per V-cycle, level 0 viscous:"]
    for mode, _ in MODES:
        lines.append(line(f"{mode} wall", col(("cycle", mode)), 1e3, "ms", f"; ratio to adiabatic {med(('cycle', mode)) / med(('cycle', 'adiabatic')):.3f}"))
        lines.append(line(f"{mode} wall, heat loads every cycle", col(("cycle+loads", mode)), 1e3, "ms", f"; ratio to the same wall without {med(('cycle+loads', mode)) / med(('cycle', mode)):.3f}"))
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
