#!/usr/bin/env python3
"""What the viscosity model (mgcfd_set_viscosity_model) costs, on the bench level (bench.py's 67^3 lattice) and on the 4-level
hierarchy of bench.py's V-cycle, with the method of tools/viscous_cost.py, all in one process:

  * time per stress launch under (constant, none) — the yardstick — and under each of the three models (sutherland, none),
    (constant, smagorinsky), (sutherland, smagorinsky), each as back-to-back launches under one event pair (mgcfd_bench_viscous
    kind 0), alternated, with the algorithmic bytes: 144 B per node + 52 B per edge, and 8 B per node more where the eddy
    viscosity is written;
  * the two step-limit kernels the same way (kind 2): k_viscous_clamp and k_viscous_clamp_variable;
  * time per sweep of the bench level and per V-cycle of the hierarchy with the terms on level 0, per model;
  * all of it --runs times over (a fresh solver each): the median and the spread (min .. max) of the runs;
  * with --baseline DIR (the mg-cfd-app-plain_amd directory of another build, the parent commit's say): that build's V-cycle
    with everything off, timed by a child process per run in alternation with this build's.

--resources appends the compiler's resource report of the stress and limit kernels (tools/kernel_resources.py; needs hipcc and no
GPU) to --out.  Clocks warm, many launches per measurement, alternated batches and their median; the state is re-initialised
before every batch.  Writes the figures to --out (default profiles/variable_viscosity_cost.txt) and prints them.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = (("constant", "none"), ("sutherland", "none"), ("constant", "smagorinsky"), ("sutherland", "smagorinsky"))


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
    """median seconds per call of `run` under every setting, in alternated batches"""
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
    out = {}
    mg = meshgen.make_multigrid((a.lattice,), "m6wing", seed=0, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    levels = mgcfd.generated_to_levels(mg)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    s.set_viscous(a.mu, levels=1)
    apply = lambda m: s.set_viscosity_model(law=m[0], eddy=m[1])
    t = alternated(s, MODELS, apply, lambda n: s.smooth(0, n), a.sweeps, a.warmup, a.batches)
    for m in MODELS:
        out["sweep", m] = t[m]
    got = {}
    for _ in range(a.batches):                                 # alternated
        for m in MODELS:
            apply(m)
            s.smooth(0, 2)
            got.setdefault(("stress", m), []).append(s.bench_viscous(0, 0, a.launches))
            if m in (MODELS[0], MODELS[3]):
                got.setdefault(("clamp", m), []).append(s.bench_viscous(0, 2, a.launches))
    for k, v in got.items():
        out[k] = statistics.median(v)
    out["nodes"], out["edges"], out["tiles"] = s.nel(0), int(levels[0]["n_internal"]), s.tiling(0)["tiles"]
    s.close()

    sizes = tuple(int(x) for x in a.sizes.split(","))
    mg = meshgen.make_multigrid(sizes, "m6wing", seed=0, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s.set_time_step("local", a.cfl)

    def apply_cycle(k):
        if k == "off":
            s.set_viscous(0.0, levels=0)
            s.set_viscosity_model()
        else:
            s.set_viscous(a.mu, levels=1)
            s.set_viscosity_model(law=k[0], eddy=k[1])

    t = alternated(s, MODELS + ("off",), apply_cycle, lambda n: s.run_cycles(n), a.cycles, a.warmup, a.batches)
    for k, v in t.items():
        out["cycle", k] = v
    s.close()
    return out


def resources():
    """the compiler's figures of the kernels the model touches"""
    lines = ["compiler's resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; tools/kernel_resources.py), the exact build;",
             "k_viscous_stress_tile<TAIL, VAR>: VAR = true is the variable instantiation, <*, false> the constant one (its instructions are the parent's):"]
    for flt in ("k_viscous_stress_tile", "k_viscous_clamp", "k_wall_stress"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), flt], capture_output=True, text=True, check=True)
        rows = r.stdout.splitlines()
        lines += [("  " + l.split("(")[0]) for l in (rows if flt == "k_viscous_stress_tile" else rows[1:])]
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mu", type=float, default=1e-3)
    ap.add_argument("--lattice", type=int, default=67)
    ap.add_argument("--sizes", default="67,55,48,43")
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--cycles", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200, help="launches per event pair")
    ap.add_argument("--cfl", type=float, default=1.0, help="local steps at this CFL number (the flow stays at the far field)")
    ap.add_argument("--baseline", default=None, help="the mg-cfd-app-plain_amd directory of another build: its V-cycle, alternated with this one's")
    ap.add_argument("--package", default=os.path.join(ROOT, "mg-cfd-app-plain_amd"), help=argparse.SUPPRESS)
    ap.add_argument("--child-vcycle", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--resources", action="store_true", help="append the compiler's resource report to --out and stop (no GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variable_viscosity_cost.txt"))
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

    runs, base = [], []
    for _ in range(a.runs):
        runs.append(one_run(mgcfd, meshgen, a))
        if a.baseline:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-vcycle", "--package", a.baseline, "--sizes", a.sizes,
                                "--cycles", str(a.cycles), "--warmup", str(a.warmup), "--batches", str(a.batches), "--cfl", str(a.cfl)],
                               capture_output=True, text=True, check=True, timeout=600)
            base.append(float([l for l in r.stdout.splitlines() if l.startswith("VCYCLE_SECONDS")][0].split()[1]))

    def line(name, vals, scale, unit, extra=""):
        return f"  {name:<52s}{scale * statistics.median(vals):9.3f} {unit}   (runs: min {scale * min(vals):.3f} .. max {scale * max(vals):.3f}){extra}"

    n, e = runs[0]["nodes"], runs[0]["edges"]
    col = lambda k: [r[k] for r in runs]
    med = lambda k: statistics.median(col(k))
    name = lambda m: f"({m[0]}, {m[1]})"
    lines = [f"viscosity model, mu = {a.mu}, defaults otherwise; {a.runs} runs of a fresh solver each, per run medians of {a.batches} alternated "
             f"batches; below: median of the runs and their spread",
             f"bench level {a.lattice}^3 = {n} nodes, {e} internal edges, {runs[0]['tiles']} tiles; {a.launches} launches per event pair:"]
    base_bytes = 144 * n + 52 * e
    for m in MODELS:
        b = base_bytes + (8 * n if m[1] != "none" else 0)
        lines.append(line("stress launch " + name(m), col(("stress", m)), 1e6, "us", f"; {b / 1e6:.1f} MB"))
    spread = (max(col(("stress", MODELS[0]))) - min(col(("stress", MODELS[0])))) / med(("stress", MODELS[0]))
    for m in MODELS[1:]:
        b = base_bytes + (8 * n if m[1] != "none" else 0)
        lines.append(f"  stress launch {name(m)} / (constant, none): time {med(('stress', m)) / med(('stress', MODELS[0])):.3f}, bytes {b / base_bytes:.3f}"
                     f" (run-to-run spread of the yardstick {100 * spread:.1f} %)")
    lines += [line("k_viscous_clamp", col(("clamp", MODELS[0])), 1e6, "us", f"; {32 * n / 1e6:.1f} MB: 32 B per node"),
              line("k_viscous_clamp_variable " + name(MODELS[3]), col(("clamp", MODELS[3])), 1e6, "us", f"; {72 * n / 1e6:.1f} MB: 72 B per node")]
    for m in MODELS:
        lines.append(line("time per sweep " + name(m), col(("sweep", m)), 1e6, "us"))
    lines.append(f"{len(a.sizes.split(','))}-level hierarchy {'/'.join(x + '^3' for x in a.sizes.split(','))}, the terms on level 0:")
    for m in MODELS:
        lines.append(line("time per V-cycle " + name(m), col(("cycle", m)), 1e3, "ms"))
    lines.append(line("time per V-cycle, everything off", col(("cycle", "off")), 1e3, "ms"))
    if base:
        lines.append(line("time per V-cycle, the baseline build", base, 1e3, "ms", "; a child process per run, alternated with the runs above"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
