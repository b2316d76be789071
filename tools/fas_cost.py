#!/usr/bin/env python3
"""What FAS multigrid (mgcfd_set_fas) costs on the 4-level hierarchy of bench.py's V-cycle (67^3 / 55^3 / 48^3 / 43^3):

  * per level pair: time per k_restrict_fas, forcing, forced update (k_time_step_src<0, true>) and FAS prolongation launch, each
    as back-to-back launches under one event pair (mgcfd_bench_fas), beside k_restrict, k_time_step and the reference's
    prolongation between the same levels, measured the same way in the same process, with the spread (min .. max) of the
    repeats and the bytes each launch moves (algorithmic: what it must read and write once, ids included);
  * time per V-cycle with FAS on and off, plain and with residual smoothing (0.5, 2), and the cost ratios.

The method of tools/jst_cost.py: clocks warm (a warm-up batch before every measurement), many launches per measurement (one event
pair, or one synchronisation per batch of cycles), alternated batches and their median with the spread.  Cycles are host-timed
around a batch: that is what a caller pays, launch overhead included.  The state is re-initialised before every batch so that on
and off time the same flow.  Writes the figures to --out (default profiles/fas_cost.txt) and prints them.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mg-cfd-app-plain_amd"))

import mgcfd                                                   # noqa: E402
from mgcfd import meshgen                                      # noqa: E402

PAIRS = (("restrict_fas", "restrict"), ("forcing", None), ("time_step_fas", "time_step"), ("prolong_fas", "prolong"))


def launch_bytes(kind, fine, coarse, edges, forced_fine):
    """Bytes a launch between a fine level of `fine` nodes and `edges` internal edges and a coarse level of `coarse` nodes
    reads and writes, every array once."""
    return {"restrict": 40 * fine + 4 * fine + 24 * coarse + 40 * coarse,
            "restrict_fas": (120 if forced_fine else 80) * fine + 4 * fine + 24 * coarse + 120 * coarse,
            "forcing": 8 * coarse + 120 * coarse,
            "time_step": 8 * coarse + 120 * coarse,
            "time_step_fas": 8 * coarse + 160 * coarse,
            "prolong": 2 * edges * 20 + 16 * fine + 40 * coarse + 120 * fine,
            "prolong_fas": 2 * edges * 20 + 16 * fine + 80 * coarse + 80 * fine}[kind]


def timed(s, run, n, warmup):
    run(warmup); s.synchronize()
    t0 = time.perf_counter(); run(n); s.synchronize()
    return (time.perf_counter() - t0) / n


def cycles_alternated(s, n, warmup, batches):
    """seconds per V-cycle with FAS off and on, in alternated batches: {on: [per batch]}"""
    t = {False: [], True: []}
    mach, alpha = s.free_stream()
    for b in range(batches + 1):
        for on in (False, True):
            s.set_fas(on)
            s.set_free_stream(mach, alpha, reinitialise=True)
            dt = timed(s, lambda k: s.run_cycles(k), n, warmup)
            if b > 0:                                          # (the first round warms up)
                t[on].append(dt)
    s.set_fas(False)
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="67,55,48,43")
    ap.add_argument("--cycles", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batches", type=int, default=3, help="repeats of every measurement (at least 3)")
    ap.add_argument("--launches", type=int, default=200, help="launches per event pair")
    ap.add_argument("--cfl", type=float, default=1.0, help="local steps at this CFL number, FAS on and off")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fas_cost.txt"))
    a = ap.parse_args()
    assert a.batches >= 3
    sizes = tuple(int(x) for x in a.sizes.split(","))
    mg = meshgen.make_multigrid(sizes, "m6wing", seed=0, jitter=0.2, area_noise=0.02, volume_noise=0.02)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s.set_time_step("local", a.cfl)
    mach, alpha = s.free_stream()
    lines = [f"FAS multigrid on the {len(sizes)}-level hierarchy {'/'.join(str(n) + '^3' for n in sizes)} "
             f"({' / '.join(str(s.nel(l)) for l in range(s.num_levels))} nodes), local steps at CFL {a.cfl}; medians of {a.batches} repeats (min .. max)",
             f"launches: {a.launches} back-to-back per event pair (mgcfd_bench_fas); bytes: algorithmic, every array once"]
    s.set_fas(True)
    s.run_cycles(a.warmup)
    for fine in range(s.num_levels - 1):
        lines.append(f"levels {fine} -> {fine + 1} ({s.nel(fine)} -> {s.nel(fine + 1)} nodes):")
        t = {k: [] for pair in PAIRS for k in pair if k}
        for _ in range(a.batches):                             # alternated: every kind once per repeat
            for k in t:
                if k == "prolong":
                    continue
                t[k].append(s.bench_fas(fine, k, a.launches))
        for _ in range(a.batches):                             # (the reference's prolongation moves the state: last, then start again)
            t["prolong"].append(s.bench_fas(fine, "prolong", a.launches))
        s.set_free_stream(mach, alpha, reinitialise=True)
        s.run_cycles(a.warmup)
        for new, old in PAIRS:
            for k in (new, old):
                if not k:
                    continue
                nbytes = launch_bytes(k, s.nel(fine), s.nel(fine + 1), s.num_internal_edges(fine), fine >= 1)
                med = statistics.median(t[k])
                lines.append(f"  {k:14s} {1e6 * med:8.2f} us   (min {1e6 * min(t[k]):.2f} .. max {1e6 * max(t[k]):.2f})   {nbytes / 1e6:8.2f} MB   {nbytes / med / 1e9:7.0f} GB/s")
    s.set_fas(False)
    for name, smoothing in (("plain", None), ("residual smoothing (0.5, 2)", (0.5, 2))):
        s.set_residual_smoothing(*(smoothing or (0.0, 0)))
        t = cycles_alternated(s, a.cycles, a.warmup, a.batches)
        on, off = statistics.median(t[True]), statistics.median(t[False])
        lines.append(f"V-cycle, {name}:")
        lines.append(f"  FAS off   {1e3 * off:8.4f} ms   (min {1e3 * min(t[False]):.4f} .. max {1e3 * max(t[False]):.4f})")
        lines.append(f"  FAS on    {1e3 * on:8.4f} ms   (min {1e3 * min(t[True]):.4f} .. max {1e3 * max(t[True]):.4f})")
        lines.append(f"  cost ratio per cycle {on / off:6.2f}")
    s.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
