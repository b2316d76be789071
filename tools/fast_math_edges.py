#!/usr/bin/env python3
"""What the fast mode's 1/x and sqrt(x) (kernels.hip: fast_rcp, fast_sqrt, fast_sqrt_pos; mgcfd_diag_fast_math) do OUTSIDE the
range tests/test_gpu_fast_accuracy.py holds them to faithful rounding on ([1e-290, 1e290]): towards the ends of the double
range and on subnormals.  Nothing is asserted; the lines go into profiles/fast_mode_accuracy.txt.

    python3 tools/fast_math_edges.py            (needs the GPU)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mg-cfd-app-plain_amd"))

import mgcfd                                     # noqa: E402
from mgcfd import meshgen                        # noqa: E402

LD = np.longdouble


def main():
    mg = meshgen.make_multigrid((5,), "m6wing", seed=1)
    s = mgcfd.Solver.from_arrays(mgcfd.generated_to_levels(mg), mg.mesh_variant)
    bands = [("1e-308 .. 1e-290", np.logspace(-307.6, -290, 512)), ("1e290 .. 1.7e308", np.logspace(290, 308.2, 512)),
             ("subnormals 5e-324 .. 2e-308", np.logspace(-323.3, -307.7, 512))]
    for kind in ("rcp", "sqrt", "sqrt_pos"):
        for name, x in bands:
            got = s.diag_fast_math(kind, x)
            want = LD(1.0) / x.astype(LD) if kind == "rcp" else np.sqrt(x.astype(LD))
            want64 = want.astype(np.float64)
            ok = np.isfinite(got) & np.isfinite(want64) & (want64 != 0)
            err = np.abs(got[ok].astype(LD) - want[ok]) / want[ok]
            worst = float(err.max()) * 2.0 ** 53 if ok.any() else float("nan")
            print("fast_%-8s %-28s finite %3d of %3d, NaN %3d, inf %3d, zero %3d; max relative error of the finite ones %.3g x 2^-53"
                  % (kind, name, int(np.isfinite(got).sum()), len(x), int(np.isnan(got).sum()), int(np.isinf(got).sum()),
                     int((got == 0).sum()), worst))
    s.close()


if __name__ == "__main__":
    main()
