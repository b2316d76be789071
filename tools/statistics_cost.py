#!/usr/bin/env python3
"""What the flow statistics (mgcfd_set_statistics) cost, on bench.py's 4-level hierarchy (67^3/55^3/48^3/43^3) built with
cavity_radius = 0.2 so that every level has solid walls, with the method of tools/spalart_allmaras_cost.py:

  * the volume sample launch (k_statistics_sample<false>: 248 B per node) against dual time's update launch of the same build
    (k_time_step_src<2, false>, BDF2: the same bytes).  The update launch is only reachable inside a sweep, where MGCFD_OPT_TIMING = 1
    brackets every launch with an event pair of its own (tools/dual_time_cost.py's method); so the sample is timed the same way, one
    launch per event pair, and also back to back, --launches per event pair (mgcfd_bench_statistics), which is what a run pays;
  * the wall accumulation launch, back to back;
  * a physical step of advance at --cycles-per-step cycles under delayed DES (all levels viscous, no-slip walls, (constant, SA),
    time_accurate, BDF2) with the statistics off, in mode 1 and in mode 2, alternated;
  * all of it --runs times over (a fresh solver each): the median and the spread (min .. max) of the runs;
  * with --baseline DIR (the checkout of another build, the parent commit's say, built): the V-cycle with every optional term off and
    bench.py's number, this build's and that build's, a child process per run, alternated.

--resources appends the compiler's resource report of the new kernels (tools/kernel_resources.py's method; needs hipcc and no GPU)
to --out.  Writes the figures to --out (default profiles/statistics_cost.txt) and prints them.  Nothing is gated on.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import spalart_allmaras_cost as sac  # noqa: E402

NODE_BYTES = {"sample": 248, "sample_mut": 256, "time_step_src": 256}
DT = 0.05


def per_pair(s, launches):
    """seconds per volume sample launch, one launch per event pair"""
    return statistics.median(s.bench_statistics("volume", 1) for _ in range(launches))


def update_launch(s, a):
    """seconds per k_time_step_src<2, false> launch on level 0: unfused sweeps under MGCFD_OPT_TIMING = 1"""
    mach, alpha = s.free_stream()
    s.set_free_stream(mach, alpha, reinitialise=True)
    s.set_dual_time(DT)
    s.begin_step(); s.begin_step()
    s.set_option("fuse_update", 0)
    s.smooth(0, 10)
    s.set_option("timing", 1)
    s.reset_monitoring()
    s.smooth(0, a.launches)
    t = s.loop_times(0)["time_step"] / (3.0 * a.launches)
    s.set_option("timing", 0)
    s.set_option("fuse_update", 1)
    s.set_dual_time(0.0)
    return t


def one_run(mgcfd, levels, variant, a):
    out = {}
    s = mgcfd.Solver.from_arrays(levels, variant)
    s.set_time_step("local", a.cfl)
    out["shape"] = (s.nel(0), s.wall_node_count(0))
    got = {k: [] for k in ("sample", "sample_pair", "update_pair", "wall")}
    for _ in range(a.batches):                             # alternated
        got["update_pair"].append(update_launch(s, a))
        s.set_statistics("wall")
        s.statistics_sample(1.0)
        got["sample"].append(s.bench_statistics("volume", a.launches))
        got["sample_pair"].append(per_pair(s, a.launches))
        got["wall"].append(s.bench_statistics("wall", a.launches))
        s.set_statistics("off")
    for k, v in got.items():
        out[k] = statistics.median(v)
    s.set_viscous(a.mu, wall=True, levels=s.num_levels)
    s.set_sa_unsteady(True, "ddes")
    s.set_viscosity_model(eddy="spalart-allmaras")
    s.set_dual_time(DT)
    s.advance(2, a.cycles_per_step)
    t = {m: [] for m in ("off", "volume", "wall")}
    for b in range(a.batches + 1):
        for m in t:
            s.set_statistics(m)
            s.advance(2, a.cycles_per_step); s.synchronize()
            t0 = time.perf_counter(); s.advance(a.steps, a.cycles_per_step); s.synchronize()
            if b > 0:
                t[m].append((time.perf_counter() - t0) / a.steps)
    for m, v in t.items():
        out["step", m] = statistics.median(v)
    s.close()
    return out


def resources():
    cs = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-Wno-unused-result",
                        "-mllvm", "-amdgpu-kernarg-preload-count=16", "-ffp-contract=off", f"-I{ROOT}/include", f"-I{cs}",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(cs, "kernels_statistics.hip"), "-o", os.devnull],
                       capture_output=True, text=True)
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)
    names = subprocess.run(["c++filt"], input="\n".join(b.split("\n")[0].strip() for b in blocks[1:]), capture_output=True, text=True).stdout.split("\n")
    lines = ["compiler's resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, kernels_statistics.hip):",
             "  VGPR SGPR scratch occ    LDS  kernel"]
    for b, d in zip(blocks[1:], names):
        g = lambda k: int(m.group(1)) if (m := re.search(k + r": (\d+)", b)) else -1
        sc, occ, lds = g(r"ScratchSize \[bytes/lane\]"), g(r"Occupancy \[waves/SIMD\]"), g(r"LDS Size \[bytes/block\]")
        lines.append(f"  {g('VGPRs'):4d} {g('SGPRs'):4d} {sc:7d} {occ:3d} {lds:6d}  {d.split('(')[0]}")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mu", type=float, default=1e-3)
    ap.add_argument("--sizes", default="67,55,48,43")
    ap.add_argument("--cavity-radius", type=float, default=0.2)
    ap.add_argument("--cycles", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10, help="physical steps per timed advance")
    ap.add_argument("--cycles-per-step", type=int, default=4)
    ap.add_argument("--launches", type=int, default=50, help="launches per event pair")
    ap.add_argument("--cfl", type=float, default=1.0, help="local steps at this CFL number")
    ap.add_argument("--baseline", default=None, help="the checkout of another build (built): its V-cycle and bench.py, alternated with this one's")
    ap.add_argument("--bench-steps", type=int, default=2000)
    ap.add_argument("--package", default=os.path.join(ROOT, "mg-cfd-app-plain_amd"), help=argparse.SUPPRESS)
    ap.add_argument("--child-vcycle", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--resources", action="store_true", help="append the compiler's resource report to --out and stop (no GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "statistics_cost.txt"))
    a = ap.parse_args()
    if a.resources:
        text = "\n".join(resources()) + "\n"
        print(text, end="")
        with open(a.out, "a") as f:
            f.write(text)
        return
    a.baseline = os.path.abspath(a.baseline) if a.baseline else None
    sys.path.insert(0, a.package)
    import mgcfd
    from mgcfd import meshgen
    if a.child_vcycle:
        print("VCYCLE_SECONDS", repr(sac.vcycle_off(mgcfd, meshgen, a)))
        return

    def child_vcycle(package):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-vcycle", "--package", package, "--sizes", a.sizes,
                            "--cavity-radius", str(a.cavity_radius), "--cycles", str(a.cycles), "--warmup", str(a.warmup),
                            "--batches", str(a.batches), "--cfl", str(a.cfl)], capture_output=True, text=True, check=True, timeout=600)
        return float([l for l in r.stdout.splitlines() if l.startswith("VCYCLE_SECONDS")][0].split()[1])

    def child_bench(root):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "200",
                            "--no-vcycle", "--cpu-seconds", "0"], capture_output=True, text=True, check=True, timeout=600, cwd=root)
        return float(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["value"])

    mg = sac.hierarchy(meshgen, a)
    levels = mgcfd.generated_to_levels(mg)
    runs, here, base, bench_here, bench_base = [], [], [], [], []
    for k in range(a.runs):
        runs.append(one_run(mgcfd, levels, mg.mesh_variant, a))
        print(f"[statistics_cost] run {k + 1} of {a.runs}: this build's launches and steps done", file=sys.stderr, flush=True)
        if a.baseline:
            here.append(child_vcycle(a.package))
            base.append(child_vcycle(os.path.join(a.baseline, "mg-cfd-app-plain_amd")))
            print(f"[statistics_cost] run {k + 1}: V-cycle children done", file=sys.stderr, flush=True)
            bench_here.append(child_bench(ROOT))
            bench_base.append(child_bench(a.baseline))
            print(f"[statistics_cost] run {k + 1}: bench.py children done", file=sys.stderr, flush=True)

    def line(name, vals, scale, unit, extra=""):
        return f"  {name:<66s}{scale * statistics.median(vals):9.3f} {unit}   (runs: min {scale * min(vals):.3f} .. max {scale * max(vals):.3f}){extra}"

    col = lambda k: [r[k] for r in runs]
    nel, n_wall = runs[0]["shape"]
    med = lambda k: statistics.median(col(k))
    lines = [f"Flow statistics on the {'/'.join(x + '^3' for x in a.sizes.split(','))} hierarchy, cavity_radius {a.cavity_radius}; {a.runs} runs of a fresh "
             f"solver each, per run medians of {a.batches} batches; below: median of the runs and their spread.  Measured on an MI355X.",
             f"launches on level 0 ({nel} nodes, {n_wall} wall nodes):",
             line(f"volume sample, {a.launches} back to back per event pair: {NODE_BYTES['sample']} B/node", col("sample"), 1e6, "us",
                  f"; {NODE_BYTES['sample'] * nel / 1e6:.1f} MB, {NODE_BYTES['sample'] * nel / med('sample') / 1e12:.2f} TB/s"),
             line("volume sample, one launch per event pair", col("sample_pair"), 1e6, "us"),
             line(f"k_time_step_src<2, false>, one launch per event pair: {NODE_BYTES['time_step_src']} B/node", col("update_pair"), 1e6, "us",
                  f"; sample / update, both one launch per event pair: {med('sample_pair') / med('update_pair'):.3f}"),
             line(f"wall accumulation, {a.launches} back to back per event pair: 64 B in, 64 B out per wall node", col("wall"), 1e6, "us"),
             f"a physical step of advance, {a.cycles_per_step} cycles per step, delayed DES, all levels viscous, (constant, SA), BDF2, dt = {DT}:"]
    off = med(("step", "off"))
    spread = 100 * (max(col(("step", "off"))) - min(col(("step", "off")))) / off
    for m, label in (("off", "statistics off"), ("volume", "mode 1 (volume)"), ("wall", "mode 2 (volume and wall)")):
        extra = f"; run-to-run spread {spread:.2f} %" if m == "off" else f"; difference to off {100 * (med(('step', m)) / off - 1):+.2f} %"
        lines.append(line(label, col(("step", m)), 1e3, "ms", extra))
    if base:
        lines.append("against the baseline build; a child process per run and build, alternated:")
        lines.append(line("V-cycle, everything off, this build", here, 1e3, "ms"))
        lines.append(line("V-cycle, everything off, the baseline build", base, 1e3, "ms",
                          f"; difference {100 * (statistics.median(here) / statistics.median(base) - 1):+.2f} %, "
                          f"baseline spread {100 * (max(base) - min(base)) / statistics.median(base):.2f} %"))
        lines.append(line(f"bench.py --gpus 1 --steps {a.bench_steps}, this build", bench_here, 1.0, "Medges/s"))
        lines.append(line(f"bench.py --gpus 1 --steps {a.bench_steps}, the baseline build", bench_base, 1.0, "Medges/s",
                          f"; difference {100 * (statistics.median(bench_here) / statistics.median(bench_base) - 1):+.2f} %, "
                          f"baseline spread {100 * (max(bench_base) - min(bench_base)) / statistics.median(bench_base):.2f} %"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
