#!/usr/bin/env python3
"""What recording the surface loads costs a V-cycle (mgcfd_run_cycles_loads against mgcfd_run_cycles).

On bench.py's 4-level M6-like hierarchy (67^3/55^3/48^3/43^3 lattices) built with cavity_radius = 0.2, so that every level
has solid walls, it prints one JSON line with
  * the V-cycle time with and without loads, the two alternated batch by batch in one process (best and median batch), and
  * the loads kernel's own time (k_surface_loads) from `rocprofv3 --kernel-trace --stats` in a separate child run
    (--no-profile skips it; --kernel-only is that child).
"""
import argparse, csv, glob, json, os, shutil, statistics, subprocess, sys, tempfile, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mg-cfd-app-plain_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="67,55,48,43")
ap.add_argument("--cavity-radius", type=float, default=0.2)
ap.add_argument("--cycles", type=int, default=25, help="cycles per timed batch")
ap.add_argument("--batches", type=int, default=20, help="timed batches of each kind, alternated")
ap.add_argument("--fast", action="store_true", help="MGCFD_OPT_EXACT = 0")
ap.add_argument("--graph", type=int, default=0, help="MGCFD_OPT_GRAPH")
ap.add_argument("--no-profile", action="store_true", help="skip the rocprofv3 run")
ap.add_argument("--kernel-only", action="store_true", help="(the profiled child) run cycles with loads and exit")
a = ap.parse_args()


def build():
    import mgcfd
    from mgcfd import meshgen
    sizes = tuple(int(x) for x in a.sizes.split(","))
    mg = meshgen.make_multigrid(sizes, "m6wing", seed=0, cavity_radius=a.cavity_radius, jitter=0.2, area_noise=0.02,
                                volume_noise=0.02)
    levels = mgcfd.generated_to_levels(mg)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    s.set_option("exact", 0 if a.fast else 1)
    s.set_option("graph", a.graph)
    return s, [L["nel"] for L in levels], [L["n_boundary"] for L in levels]


if a.kernel_only:
    s, _, _ = build()
    s.run_cycles(2 * a.cycles, loads=True)
    s.close()
    sys.exit(0)

s, nel, walls = build()
ref = (0.5, 0.5, 0.5)
s.run_cycles(a.cycles)
s.run_cycles(a.cycles, loads=True, ref_point=ref)
t_plain, t_loads = [], []
for b in range(a.batches):
    for loads in ((False, True) if b % 2 == 0 else (True, False)):
        t0 = time.perf_counter()
        if loads:
            s.run_cycles(a.cycles, loads=True, ref_point=ref)
        else:
            s.run_cycles(a.cycles)
        (t_loads if loads else t_plain).append((time.perf_counter() - t0) / a.cycles)
s.close()
out = {"workload": f"M6-like 4-level hierarchy, cavity_radius {a.cavity_radius}: {nel} nodes",
       "solid_wall_edges_level0": walls[0], "solid_wall_edges_per_level": walls,
       "mode": "fast" if a.fast else "bit-identical", "graph": a.graph, "cycles_per_batch": a.cycles, "batches": a.batches,
       "vcycle_ms_plain": {"best": min(t_plain) * 1e3, "median": statistics.median(t_plain) * 1e3},
       "vcycle_ms_loads": {"best": min(t_loads) * 1e3, "median": statistics.median(t_loads) * 1e3}}
out["added_pct_median"] = 100.0 * (statistics.median(t_loads) / statistics.median(t_plain) - 1.0)
out["added_pct_best"] = 100.0 * (min(t_loads) / min(t_plain) - 1.0)

if not a.no_profile:
    prof = shutil.which("rocprofv3")
    if prof is None:
        out["kernel"] = {"error": "rocprofv3 not found"}
    else:
        d = tempfile.mkdtemp(prefix="loads_prof_")
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--kernel-only", "--sizes", a.sizes, "--cavity-radius", str(a.cavity_radius),
               "--cycles", str(a.cycles), "--graph", str(a.graph)] + (["--fast"] if a.fast else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        rows = []
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            rows += [row for row in csv.DictReader(open(f)) if "k_surface_loads" in row["Name"]]
        if r.returncode != 0 or not rows:
            out["kernel"] = {"error": f"rocprofv3 exit {r.returncode}, {len(rows)} rows", "stderr_tail": r.stderr[-400:]}
        else:
            calls = sum(int(row["Calls"]) for row in rows)
            total = sum(float(row["AverageNs"]) * int(row["Calls"]) for row in rows)
            out["kernel"] = {"name": "k_surface_loads", "calls": calls, "avg_us": total / calls / 1e3}
            if all("MinNs" in row and "MaxNs" in row for row in rows):
                out["kernel"]["min_us"] = min(float(row["MinNs"]) for row in rows) / 1e3
                out["kernel"]["max_us"] = max(float(row["MaxNs"]) for row in rows) / 1e3
            out["kernel_pct_of_plain_vcycle"] = 100.0 * (total / calls * 1e-9) / statistics.median(t_plain)
        shutil.rmtree(d, ignore_errors=True)
print(json.dumps(out))
