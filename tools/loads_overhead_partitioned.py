#!/usr/bin/env python3
"""What the surface loads cost on partitioned levels (mgcfd_group_cycles_loads against mgcfd_group_cycles) — the sibling
of tools/loads_overhead.py, on the same hierarchy (bench.py's 4-level M6-like lattices built with cavity_radius = 0.2).

One JSON line with
  * Group.cycles with and without loads, `--ranks` ranks SHARING this one device, the two alternated batch by batch in one
    process (best and median batch).  Ranks that share a device time the call pattern — launches, event records and
    waits — not xGMI: nothing here runs on more than one GPU;
  * from `rocprofv3 --kernel-trace --stats` in a separate child run (--no-profile skips it; --kernel-only is that child):
    k_loads_terms + k_loads_reduce of ONE rank that holds every node, beside k_surface_loads of a whole solver on the same
    level in the same process.
"""
import argparse, csv, glob, json, os, shutil, statistics, subprocess, sys, tempfile, time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mg-cfd-app-plain_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="67,55,48,43")
ap.add_argument("--cavity-radius", type=float, default=0.2)
ap.add_argument("--ranks", type=int, default=3)
ap.add_argument("--cycles", type=int, default=25, help="cycles per timed batch")
ap.add_argument("--batches", type=int, default=20, help="timed batches of each kind, alternated")
ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 run")
ap.add_argument("--kernel-only", action="store_true", help="(the profiled child) one rank and a whole solver, cycles with loads")
a = ap.parse_args()
REF = (0.5, 0.5, 0.5)


def hierarchy():
    import mgcfd
    from mgcfd import meshgen
    sizes = tuple(int(x) for x in a.sizes.split(","))
    mg = meshgen.make_multigrid(sizes, "m6wing", seed=0, cavity_radius=a.cavity_radius, jitter=0.2, area_noise=0.02,
                                volume_noise=0.02)
    return mgcfd.generated_to_levels(mg), mg.mesh_variant


def group_over(levels, variant, part0):
    import mgcfd
    from mgcfd.partition import partition_hierarchy
    H = partition_hierarchy(levels, part0)
    solvers = []
    for h in H:
        lv, owned, keys = h.solver_args()
        solvers.append(mgcfd.Solver.from_arrays(lv, variant, n_owned=owned, order_keys=keys))
    g = mgcfd.Group(solvers)
    for h, s in zip(H, solvers):
        for l in range(len(levels)):
            s.rank_set_halo(l, h.levels[l])
            s.rank_set_wall_slots(l, h.levels[l])
    for l in range(len(levels)):
        g.exchange(l)
    return solvers, g


levels, variant = hierarchy()

if a.kernel_only:
    import mgcfd
    solvers, g = group_over(levels, variant, np.zeros(levels[0]["nel"], dtype=np.int64))
    g.cycles(2 * a.cycles, loads=True, ref_point=REF)
    g.close()
    solvers[0].close()
    whole = mgcfd.Solver.from_arrays(levels, variant)
    whole.run_cycles(2 * a.cycles, loads=True, ref_point=REF)
    whole.close()
    sys.exit(0)

from mgcfd.partition import rcb_partition
solvers, g = group_over(levels, variant, rcb_partition(np.asarray(levels[0]["coords"]), a.ranks))
g.cycles(a.cycles)
g.cycles(a.cycles, loads=True, ref_point=REF)
t_plain, t_loads = [], []
for b in range(a.batches):
    for loads in ((False, True) if b % 2 == 0 else (True, False)):
        t0 = time.perf_counter()
        if loads:
            g.cycles(a.cycles, loads=True, ref_point=REF)
        else:
            g.cycles(a.cycles)
        (t_loads if loads else t_plain).append((time.perf_counter() - t0) / a.cycles)
g.close()
for s in solvers:
    s.close()
out = {"workload": f"M6-like 4-level hierarchy, cavity_radius {a.cavity_radius}: {[L['nel'] for L in levels]} nodes, "
                   f"{a.ranks} ranks sharing one device",
       "solid_wall_edges_level0": levels[0]["n_boundary"], "cycles_per_batch": a.cycles, "batches": a.batches,
       "group_cycle_ms_plain": {"best": min(t_plain) * 1e3, "median": statistics.median(t_plain) * 1e3},
       "group_cycle_ms_loads": {"best": min(t_loads) * 1e3, "median": statistics.median(t_loads) * 1e3}}
out["added_pct_median"] = 100.0 * (statistics.median(t_loads) / statistics.median(t_plain) - 1.0)
out["added_pct_best"] = 100.0 * (min(t_loads) / min(t_plain) - 1.0)

if not a.no_profile:
    prof = shutil.which("rocprofv3")
    if prof is None:
        out["kernels"] = {"error": "rocprofv3 not found"}
    else:
        d = tempfile.mkdtemp(prefix="loads_part_prof_")
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--kernel-only", "--sizes", a.sizes, "--cavity-radius", str(a.cavity_radius),
               "--cycles", str(a.cycles)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            rows += list(csv.DictReader(open(f)))
        out["kernels"] = {}
        for name in ("k_surface_loads", "k_loads_terms", "k_loads_reduce"):
            mine = [row for row in rows if name in row["Name"]]
            if r.returncode != 0 or not mine:
                out["kernels"][name] = {"error": f"rocprofv3 exit {r.returncode}, {len(mine)} rows", "stderr_tail": r.stderr[-300:]}
                continue
            calls = sum(int(row["Calls"]) for row in mine)
            total = sum(float(row["AverageNs"]) * int(row["Calls"]) for row in mine)
            k = {"calls": calls, "avg_us": total / calls / 1e3}
            if all("MinNs" in row and "MaxNs" in row for row in mine):
                k["min_us"] = min(float(row["MinNs"]) for row in mine) / 1e3
                k["max_us"] = max(float(row["MaxNs"]) for row in mine) / 1e3
            out["kernels"][name] = k
        shutil.rmtree(d, ignore_errors=True)
print(json.dumps(out))
