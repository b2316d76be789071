#!/usr/bin/env python3
"""What the time-step modes of mgcfd_set_time_step cost and buy (INTEGRATION.md §8 quotes the figures):

(a) convergence: V-cycles until the level-0 RMS has fallen to --drop times its first cycle's value, global against local
    steps at equal CFL numbers, on the generated 4-level hierarchy (bench.py's V-cycle lattices, or --sizes) and on the golden
    fvcorr_1lvl case.  Capped at --max-cycles; a run that turns invalid says so.
(b) time per sweep of a level split over ranks, global against local: Group.sweeps on --ranks parts and mgcfd_rank_sweeps on
    an RCCL communicator of one rank, as alternated batches (global, local, global, ...), the median of the batches reported.
    The ranks share ONE GPU here, so this times the call pattern (launches, events, the all-reduce's host and device
    overhead), not a flight between devices: never run on more than one GPU.

Prints one JSON line per figure.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mg-cfd-app-plain_amd"))

import mgcfd                                                   # noqa: E402
from mgcfd import meshgen                                      # noqa: E402
from mgcfd.partition import partition_level, rcb_partition    # noqa: E402


def cycles_to_drop(make_solver, mode, cfl, drop, max_cycles, batch=10):
    s = make_solver()
    s.set_time_step(mode, cfl)
    rms = []
    try:
        while len(rms) < max_cycles:
            rms.extend(s.run_cycles(batch).tolist())
            hit = [k for k, r in enumerate(rms) if r <= drop * rms[0]]
            if hit:
                return {"cycles": hit[0] + 1, "rms_first": rms[0], "rms_there": rms[hit[0]]}
    except mgcfd.MgcfdError as e:
        return {"cycles": None, "invalid_after": len(rms), "error": str(e)[:80]}
    finally:
        s.close()
    return {"cycles": None, "rms_first": rms[0], "rms_last": rms[-1], "ran": len(rms)}


def convergence(a):
    sizes = tuple(int(x) for x in a.sizes.split(","))
    mg = meshgen.make_multigrid(sizes, "m6wing", seed=0, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    levels = mgcfd.generated_to_levels(mg)
    golden = os.path.join(ROOT, "tests", "golden", "fvcorr_1lvl", "input")
    mesh = mgcfd.Mesh("input.dat", golden)
    cases = [(f"generated {len(sizes)}-level hierarchy {'/'.join(str(n) + '^3' for n in sizes)}", lambda: mgcfd.Solver.from_arrays(levels, mg.mesh_variant)),
             ("fvcorr_1lvl", lambda: mgcfd.Solver.from_mesh(mesh))]
    for name, make in cases:
        for cfl in (float(x) for x in a.cfls.split(",")):
            for mode in ("global", "local"):
                r = cycles_to_drop(make, mode, cfl, a.drop, a.max_cycles)
                print(json.dumps({"figure": "cycles_to_rms_drop", "case": name, "drop": a.drop, "mode": mode, "cfl": cfl, **r}), flush=True)
    mesh.close()


def median_us(batches):
    return round(1e6 * statistics.median(batches), 2)


def sweep_times(a):
    mg = meshgen.make_multigrid((a.lattice,), "m6wing", seed=4, cavity_radius=0.15, jitter=0.2, area_noise=0.05, volume_noise=0.05)
    L = mgcfd.generated_to_levels(mg)[0]
    # in-process group
    parts = partition_level(L, rcb_partition(np.asarray(L["coords"]), a.ranks))
    solvers = [mgcfd.Solver.from_arrays([P.level], mg.mesh_variant, n_owned=[P.n_owned]) for P in parts]
    g = mgcfd.Group(solvers)
    for P, s in zip(parts, solvers):
        s.rank_set_halo(0, P)
    g.exchange(0)
    # one RCCL rank
    P1 = partition_level(L, np.zeros(L["nel"], dtype=np.int64))[0]
    r = mgcfd.Solver.from_arrays([P1.level], mg.mesh_variant, n_owned=[P1.n_owned])
    r.rank_attach_rccl(0, 1, mgcfd.rccl_unique_id())
    r.rank_set_halo(0, P1)
    r.rank_exchange(0)
    forms = {"Group.sweeps, %d ranks on one GPU" % a.ranks: (g.set_time_step, lambda n: g.sweeps(0, n), g.synchronize),
             "rank_sweeps, one RCCL rank": (r.set_time_step, lambda n: r.rank_sweeps(0, n), r.synchronize)}
    for name, (set_mode, run, sync) in forms.items():
        t = {"global": [], "local": []}
        for b in range(2 * a.batches + 2):
            mode = ("global", "local")[b % 2]
            set_mode(mode, 0.5)
            run(a.warmup); sync()
            t0 = time.perf_counter(); run(a.sweeps); sync(); t1 = time.perf_counter()
            if b >= 2:                                        # (the first batch of each mode warms up)
                t[mode].append((t1 - t0) / a.sweeps)
        print(json.dumps({"figure": "us_per_sweep", "form": name, "nodes": int(L["nel"]), "batches": a.batches, "sweeps_per_batch": a.sweeps,
                          "global_median": median_us(t["global"]), "local_median": median_us(t["local"]),
                          "global_range": [round(1e6 * min(t["global"]), 2), round(1e6 * max(t["global"]), 2)],
                          "local_range": [round(1e6 * min(t["local"]), 2), round(1e6 * max(t["local"]), 2)],
                          "note": "ranks share one GPU: the call pattern only"}), flush=True)
    r.rank_detach()
    r.close()
    g.close()
    for s in solvers:
        s.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="67,55,48,43", help="lattices of the generated hierarchy (bench.py's V-cycle)")
    ap.add_argument("--cfls", default="0.5,1.0")
    ap.add_argument("--drop", type=float, default=0.1, help="RMS relative to the first cycle's")
    ap.add_argument("--max-cycles", type=int, default=300)
    ap.add_argument("--lattice", type=int, default=48, help="(b): the level that is split")
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--batches", type=int, default=7)
    ap.add_argument("--sweeps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--skip", default="", choices=["", "convergence", "sweeps"])
    a = ap.parse_args()
    if a.skip != "convergence":
        convergence(a)
    if a.skip != "sweeps":
        sweep_times(a)


if __name__ == "__main__":
    main()
