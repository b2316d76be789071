"""Child process of tests/test_gpu_fast_accuracy.py: the order-free launches of one level under a switch that the library reads
once per process (MGCFD_FREE_WG3, MGCFD_FREE_NO_ROLES: the parent sets one in this process's environment).

  python fast_accuracy_children.py INPUT_DIR LEVEL OUT.npz

For the `perturbed` and the `wide` state: the internal class onto the non-zero f0 and all classes from zero, each twice, and one
sweep under the reference's and under local steps (state, residual, step factors).  Nothing is judged here: the parent
measures the arrays against its long-double reference.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("mg-cfd-app-plain_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import fast_accuracy_reference as far     # noqa: E402


def main(input_dir, l, out):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", input_dir)
    s = mgcfd.Solver.from_mesh(mesh)
    s.set_option("exact", 0)
    s.set_option("flux_variant", 64 | 1)
    assert s.has_order_free(l)
    case = f"mesh3_L{l}"
    nel = s.nel(l)
    import oracle_py
    ff_var = np.array(list(oracle_py.farfield().var))                         # (as the parent's RefLevel.ff_var)
    f0 = np.random.default_rng(17 + l).normal(size=(nel, 5)) * 1e-7          # far.f0_for
    res = {}
    for kind in ("perturbed", "wide"):
        q = far.make_state(kind, nel, ff_var, far.state_seed(case, kind))
        res[f"{kind}/q"] = q
        s.set(l, "variables", q)
        for run in (1, 2):
            s.set(l, "fluxes", f0)
            s.compute_flux_edge(l)
            res[f"{kind}/internal/{run}"] = s.get(l, "fluxes")
            s.zero_fluxes(l)
            s.compute_fluxes(l)
            res[f"{kind}/all/{run}"] = s.get(l, "fluxes")
        for mode in ("reference", "local"):
            s.set_time_step(mode, far.sweep_cfl(case, kind, mode))
            s.set(l, "variables", q)
            s.zero_fluxes(l)
            s.smooth(l, 1)
            res[f"{kind}/{mode}/W"] = s.get(l, "variables")
            res[f"{kind}/{mode}/res"] = s.get(l, "residuals")
            res[f"{kind}/{mode}/sf"] = s.get(l, "step_factors")
    s.close()
    mesh.close()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), sys.argv[3])
