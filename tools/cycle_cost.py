#!/usr/bin/env python3
"""What the shaped multigrid cycles (mgcfd_set_cycle) and the state prolongation (mgcfd_prolong_state) cost on the 4-level
hierarchy of tools/vcycle_bench.py (67^3 / 55^3 / 48^3 / 43^3), local steps at CFL 1.0:

  * ms per cycle for V, W and F, without and with one post-sweep on level 0, with the reference's transfers and with FAS, and each
    one's ratio to the default V-cycle of the same transfers;
  * the state-prolongation launch onto level 0 beside FAS's prolongation launch (k_prolong_tile in its STATE and FAS modes)
    between the same levels: both inside event pairs (MGCFD_OPT_TIMING = 1, one pair per launch), with the bytes each moves;
  * with --baseline DIR (a checkout of another commit with its library built, the parent commit's say): the default V-cycle and
    bench.py of that build and of this one, a child process per run, alternated, so that both see the same session.

The method of tools/fas_cost.py: a warm-up batch before every measurement, many cycles per measurement (host-timed around a
batch: what a caller pays), the state re-initialised before every batch, alternated batches, median and min .. max.  Writes the
figures to --out (default profiles/cycle_cost.txt) and prints them.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(v, scale, unit):
    return f"{scale * statistics.median(v):9.4f} {unit}   (min {scale * min(v):.4f} .. max {scale * max(v):.4f})"


def timed(s, run, n, warmup):
    run(warmup); s.synchronize()
    t0 = time.perf_counter(); run(n); s.synchronize()
    return (time.perf_counter() - t0) / n


def make_solver(sizes, package=None):
    sys.path.insert(0, package or os.path.join(ROOT, "mg-cfd-app-plain_amd"))
    import mgcfd
    from mgcfd import meshgen
    mg = meshgen.make_multigrid(sizes, "m6wing", seed=0, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    return mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)


def child_vcycle(a, sizes):
    """one fresh solver of the build in --package: seconds per default V-cycle, per batch"""
    s = make_solver(sizes, a.package)
    s.set_time_step("local", a.cfl)
    mach, alpha = s.free_stream()
    out = []
    for b in range(a.batches + 1):
        s.set_free_stream(mach, alpha, reinitialise=True)
        dt = timed(s, lambda k: s.run_cycles(k), a.cycles, a.warmup)
        if b > 0:
            out.append(dt)
    s.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="67,55,48,43")
    ap.add_argument("--cycles", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", type=int, default=3, help="repeats of every measurement (at least 3)")
    ap.add_argument("--launches", type=int, default=200, help="launches per measurement of a prolongation kernel")
    ap.add_argument("--cfl", type=float, default=1.0)
    ap.add_argument("--baseline", default=None, help="the root of another build (its mg-cfd-app-plain_amd and bench.py): alternated with this one")
    ap.add_argument("--bench-args", default="--gpus 1 --steps 2000 --warmup 200", help="bench.py's arguments in the comparison")
    ap.add_argument("--runs", type=int, default=3, help="child runs per build in the comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cycle_cost.txt"))
    ap.add_argument("--child-vcycle", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--package", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert a.batches >= 3
    sizes = tuple(int(x) for x in a.sizes.split(","))
    if a.child_vcycle:
        return child_vcycle(a, sizes)
    s = make_solver(sizes)
    n = s.num_levels
    s.set_time_step("local", a.cfl)
    mach, alpha = s.free_stream()
    lines = [f"multigrid cycle control on the {n}-level hierarchy {'/'.join(str(k) + '^3' for k in sizes)} "
             f"({' / '.join(str(s.nel(l)) for l in range(n))} nodes), local steps at CFL {a.cfl}; medians of {a.batches} alternated batches of {a.cycles} cycles (min .. max)"]
    configs = [(shape, p0) for p0 in (0, 1) for shape in "VWF"]
    for fas in (False, True):
        s.set_fas(fas)
        t = {c: [] for c in configs}
        for b in range(a.batches + 1):
            for shape, p0 in configs:
                s.set_cycle(shape, None, [p0] + [1] * (n - 1))
                s.set_free_stream(mach, alpha, reinitialise=True)
                dt = timed(s, lambda k: s.run_cycles(k), a.cycles, a.warmup)
                if b > 0:                                      # (the first round warms up)
                    t[shape, p0].append(dt)
        base = statistics.median(t["V", 0])
        lines.append("FAS on:" if fas else "the reference's transfers:")
        for shape, p0 in configs:
            lines.append(f"  {shape}{', post[0] = 1' if p0 else '':16s} {spread(t[shape, p0], 1e3, 'ms')}   x {statistics.median(t[shape, p0]) / base:.2f} of V")
    # the two prolongation launches onto level 0, one event pair per launch
    s.set_cycle()
    s.set_fas(True)
    s.set_free_stream(mach, alpha, reinitialise=True)
    s.run_cycles(a.warmup)
    s.set_option("timing", 1)
    t = {"state": [], "fas": []}
    for b in range(a.batches + 1):
        for kind, call in (("state", s.prolong_state), ("fas", s.fas_prolong)):
            s.reset_monitoring()
            for _ in range(a.launches):
                call(0)
            s.synchronize()
            if b > 0:
                t[kind].append(s.loop_times(0)["prolong"] / a.launches)
        s.set_free_stream(mach, alpha, reinitialise=True)      # (FAS's launch moves the state: start again)
        s.set_option("timing", 0)
        s.run_cycles(a.warmup)
        s.set_option("timing", 1)
    s.set_option("timing", 0)
    fine, coarse, edges = s.nel(0), s.nel(1), s.num_internal_edges(0)
    nbytes = {"state": 2 * edges * 20 + 16 * fine + 40 * coarse + 40 * fine, "fas": 2 * edges * 20 + 16 * fine + 80 * coarse + 80 * fine}
    lines.append(f"prolongation onto level 0 ({coarse} -> {fine} nodes), {a.launches} launches, one event pair each; bytes: algorithmic, every array once")
    for kind, name in (("state", "state (mgcfd_prolong_state)"), ("fas", "FAS (mgcfd_fas_prolong)")):
        med = statistics.median(t[kind])
        lines.append(f"  {name:30s} {spread(t[kind], 1e6, 'us')}   {nbytes[kind] / 1e6:7.2f} MB   {nbytes[kind] / med / 1e9:6.0f} GB/s")
    s.close()
    if a.baseline:
        here = os.path.abspath(__file__)
        builds = (("this build", ROOT), ("the baseline build", os.path.abspath(a.baseline)))
        vc = {name: [] for name, _ in builds}
        bench = {name: [] for name, _ in builds}
        for _ in range(a.runs):
            for name, root in builds:
                r = subprocess.run([sys.executable, here, "--child-vcycle", "--package", os.path.join(root, "mg-cfd-app-plain_amd"), "--sizes", a.sizes,
                                    "--cycles", str(a.cycles), "--warmup", str(a.warmup), "--batches", str(a.batches), "--cfl", str(a.cfl)],
                                   capture_output=True, text=True, check=True)
                vc[name] += json.loads(r.stdout.strip().splitlines()[-1])
                r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + a.bench_args.split(), capture_output=True, text=True, check=True, cwd=root)
                row = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
                bench[name].append(row)
        lines.append(f"the default V-cycle, a child process per run, {a.runs} runs per build alternated, {a.batches} batches per run:")
        for name, _ in builds:
            lines.append(f"  {name:20s} {spread(vc[name], 1e3, 'ms')}")
        lines.append(f"bench.py {a.bench_args}, the same runs; its 'value' ({bench['this build'][0]['unit']}):")
        for name, _ in builds:
            v = [row["value"] for row in bench[name]]
            lines.append(f"  {name:20s} median {statistics.median(v):.6g}   (min {min(v):.6g} .. max {max(v):.6g})")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
