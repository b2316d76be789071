#!/usr/bin/env python3
"""The convergence histories of FAS multigrid on the CPU (the numpy emulator, tests/fas_emulator.py; no GPU): on the two
generated lattices of tests/test_host_fas.py under local steps, the RMS of component 0 of F_0(W) / vol after every cycle for the
FAS cycle, for sweeps of level 0 alone and for the reference's cycle, and the cycles each needs to bring it below a tolerance.
Writes profiles/fas_convergence.txt (tests/test_host_fas.py asserts the bounds; tests/test_gpu_fas.py requires the GPU to
reproduce the emulator's state bit for bit).
"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "mg-cfd-app-plain_amd", "oracle", ""):
    sys.path.insert(0, os.path.join(ROOT, p))

import oracle_py                                               # noqa: E402
import fas_emulator as fe                                      # noqa: E402

TOLERANCES = (1e-1, 1e-2, 1e-3)


def history(case, cfl, smoothing, kind, cycles):
    """(metric after every cycle, the cycle in which the run went invalid or None)"""
    em = fe.FasOracle(oracle_py, case, "local", cfl, *smoothing, fas=(kind == "fas"))
    out = []
    for c in range(cycles):
        rc = em.sweeps(0, 1) if kind == "level0" else em.cycles(1)[0]
        if rc:
            em.close()
            return out, c + 1
        out.append(em.density_residual_rms())
    em.close()
    return out, None


def first_below(h, tol):
    for c, v in enumerate(h):
        if v <= tol:
            return str(c + 1)
    return "-"


def main():
    oracle_py.load()
    tmp = tempfile.mkdtemp()
    lines = ["FAS multigrid: convergence on the CPU (tests/fas_emulator.py; tools/fas_convergence.py writes this file).",
             "Metric: the RMS of component 0 of F_0(W) / vol on level 0, after every cycle (FAS, reference) or sweep (level 0 alone);",
             "local steps; lattices of meshgen.make_multigrid(sizes, 'fvcorr', seed=11, cavity_radius=0.12, jitter=0.25, area_noise=0.08,",
             "volume_noise=0.1): undamped edge weights, from the far field.", ""]
    runs = (("A", 1.0, (0.0, 0), fe.CONV_CYCLES), ("A", fe.CONV_SMOOTHING_CFL, fe.CONV_SMOOTHING, fe.CONV_CYCLES), ("B", 1.0, (0.0, 0), fe.FIXED_CYCLES))
    for name, cfl, smoothing, cycles in runs:
        case = fe.write_lattice(name, tempfile.mkdtemp(dir=tmp))
        h = {k: history(case, cfl, smoothing, k, cycles) for k in ("fas", "level0", "reference")}
        lines.append(f"lattice {name} {fe.LATTICES[name]}, CFL {cfl}, residual smoothing {smoothing if smoothing[1] else 'off'}, {cycles} cycles")
        lines.append("cycle        FAS cycle   level 0 alone  reference cycle")
        step = max(1, cycles // 12)
        for c in list(range(step - 1, cycles, step)):
            row = [("%14.4e" % h[k][0][c]) if c < len(h[k][0]) else "       invalid" for k in ("fas", "level0", "reference")]
            lines.append(f"{c + 1:5d} {row[0]} {row[1]}  {row[2]}")
        for k, label in (("fas", "FAS cycle"), ("level0", "level 0 alone"), ("reference", "reference cycle")):
            hist, bad = h[k]
            end = f"invalid state in cycle {bad} (0-based, as mgcfd_invalid_state_location counts: {bad - 1})" if bad else f"final {hist[-1]:.4e}"
            lines.append(f"  {label:15s}: {end}; cycles to reach " + ", ".join(f"{t:g}: {first_below(hist, t)}" for t in TOLERANCES))
        if h["fas"][1] is None and h["level0"][1] is None:
            lines.append(f"  level 0 alone / FAS at the end: {h['level0'][0][-1] / h['fas'][0][-1]:.1f}")
        lines.append("")
    text = "\n".join(lines)
    print(text, end="")
    with open(os.path.join(ROOT, "profiles", "fas_convergence.txt"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
