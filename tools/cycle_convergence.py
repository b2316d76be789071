#!/usr/bin/env python3
"""Convergence of the shaped multigrid cycles (mgcfd_set_cycle, mgcfd_full_multigrid) on the CPU, with the numpy emulator
tests/cycle_emulator.py: FAS, local steps, from the far field, on the undamped generated lattices A (13, 9, 6) and C (17, 13, 9, 6),
plain at CFL 1.0 and with residual smoothing (0.5, 2) at CFL 2.0.

Per configuration — V, W, F, each with and without one post-sweep on level 0, and W with the post-sweep behind a full-multigrid
start of --fmg-cycles cycles per coarse level — the RMS of the density component of F_0 / vol after --cycles level-0 cycles, the
cycles it needs to reach 1e-1, 1e-2 and 1e-3, and the work that is: sweeps weighted by nel_l / nel_0, the FMG start's included.
Writes the table to --out (default profiles/cycle_convergence.txt) and prints it.
"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle", "mg-cfd-app-plain_amd", ""):
    sys.path.insert(0, os.path.join(ROOT, p))

import oracle_py                                               # noqa: E402
import cycle_emulator as ce                                    # noqa: E402
import fas_emulator as fe                                      # noqa: E402

THRESHOLDS = (1e-1, 1e-2, 1e-3)
CONFIGS = (("V (default)", "V", 0, False), ("W", "W", 0, False), ("F", "F", 0, False), ("V, post[0] = 1", "V", 1, False),
           ("W, post[0] = 1", "W", 1, False), ("F, post[0] = 1", "F", 1, False), ("FMG, then W, post[0] = 1", "W", 1, True))


def history(case, cfl, smoothing, shape, post0, fmg, cycles, fmg_cycles):
    """(metric after every cycle or None from the invalid cycle on, work after every cycle, the FMG start's work)"""
    em = ce.CycleOracle(oracle_py, case, "local", cfl, *smoothing, fas=True)
    pre, post = ce.default_sweeps(em.n)
    em.set_cycle(shape, pre, [post0] + post[1:])
    if fmg:
        rc, _ = em.full_multigrid([0] + [fmg_cycles] * (em.n - 1))
        assert rc == 0
    start = em.work
    metric, work = [], []
    for _ in range(cycles):
        rc, _ = em.cycles(1)
        if rc:
            break
        metric.append(em.density_residual_rms())
        work.append(em.work)
    em.close()
    return metric, work, start


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cycles", type=int, default=60)
    ap.add_argument("--fmg-cycles", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cycle_convergence.txt"))
    a = ap.parse_args()
    oracle_py.load()
    lines = [f"FAS multigrid under local steps from the far field, {a.cycles} level-0 cycles; metric: RMS of component 0 of F_0 / vol (the numpy emulator, CPU)",
             f"work: sweeps weighted by nel_l / nel_0; an FMG start is {a.fmg_cycles} cycles from every coarse level and its work counts",
             "to 1e-N: the first cycle after which the metric is at or below it, and the work up to there ('-': not within the run)"]
    with tempfile.TemporaryDirectory() as d:
        for name in ("A", "C"):
            case = ce.write_lattice(name, d)
            for label, cfl, smoothing in (("CFL 1.0, no smoothing", 1.0, (0.0, 0)), (f"CFL {fe.CONV_SMOOTHING_CFL}, smoothing {fe.CONV_SMOOTHING}", fe.CONV_SMOOTHING_CFL, fe.CONV_SMOOTHING)):
                lines.append(f"lattice {name} {ce.LATTICES[name]}, {label}:")
                lines.append(f"  {'cycle':26s} {'work/cycle':>10s} {'final':>10s}" + "".join(f" {'to %.0e' % t:>16s}" for t in THRESHOLDS))
                for title, shape, post0, fmg in CONFIGS:
                    metric, work, start = history(case, cfl, smoothing, shape, post0, fmg, a.cycles, a.fmg_cycles)
                    per_cycle = (work[-1] - start) / len(work) if work else float("nan")
                    cells = []
                    for t in THRESHOLDS:
                        hit = next((k for k, m in enumerate(metric) if m <= t), None)
                        cells.append(f" {'-':>16s}" if hit is None else f" {'%d (%.1f)' % (hit + 1, work[hit]):>16s}")
                    final = "%.3e" % metric[-1] if len(metric) == a.cycles else "invalid@%d" % (len(metric) + 1)
                    lines.append(f"  {title:26s} {per_cycle:10.2f} {final:>10s}" + "".join(cells))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
