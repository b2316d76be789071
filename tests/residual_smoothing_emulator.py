"""The yardstick of implicit residual smoothing (mgcfd_set_residual_smoothing): ``ResidualSmoothingOracle``, the composed oracle
of tests/time_step_emulator.py with time_step replaced by numpy written from the definition in include/mgcfd.h / INTEGRATION.md
§9.  Every other kernel stays the oracle's entry point.

With ``iterations = M >= 1`` stage j of every sweep computes its fluxes F as before and then, in place of time_step(j):

    D[i][v]  = sf[i] * F[i][v]
    den[i]   = 1.0 + eps * n_i                  n_i: internal edges with i as an end point
    Db0 = D; S[i][v] = sum over the internal edges at i, in edge order from +0.0, of Db(m-1)[other end][v]
             Db(m)[i][v] = (D[i][v] + eps * S[i][v]) / den[i]                                     m = 1 .. M
    variables[i][v] = old_variables[i][v] + Db(M)[i][v] / (RK + 1 - j);   fluxes = 0

Every numpy operation is one IEEE-754 double operation per element (numpy never contracts to FMA); ``np.add.at`` is unbuffered
and adds in index order, so with the index arrays interleaved (a0, b0, a1, b1, ...) a node's sum runs over its edges in the
level's original edge order — the order in which the reference adds into ``fluxes[i]``.  ``iterations = 0`` is
``TimeStepOracle`` itself (tests/test_host_residual_smoothing.py checks the bits).
"""
import ctypes as C

import numpy as np

import free_stream_emulator as fse
import time_step_emulator as tse

RK = 3
MAX_ITERATIONS = 8

# What the GPU tests run (tests/test_gpu_residual_smoothing.py): every case below under every combination below, GPU_CYCLES
# cycles, none skipped.  tests/test_host_residual_smoothing.py asserts on the CPU that each one stays valid.
GPU_CASES = fse.GPU_CASES
GPU_MODES = ("local", "global")
GPU_CFLS = (1.5, 2.5)
GPU_SMOOTHINGS = ((0.5, 2), (1.0, 2))
GPU_CYCLES = 3
# the point of the feature: (case, mode, cfl, cycles); unsmoothed the run goes invalid, with POINT_SMOOTHING it completes
POINT_CASE, POINT_CYCLES, POINT_SMOOTHING = "fvcorr_1lvl", 12, (0.5, 2)
POINT_RUNS = (("local", 2.5), ("global", 4.0))


def gpu_combinations():
    return [(case, mode, cfl, eps, m) for case in GPU_CASES for mode in GPU_MODES for cfl in GPU_CFLS for eps, m in GPU_SMOOTHINGS]


class ResidualSmoothingOracle(tse.TimeStepOracle):
    """TimeStepOracle with the coefficient and the Jacobi iterations of mgcfd_set_residual_smoothing."""

    def __init__(self, oracle, case, mode="reference", cfl=0.5, eps=0.0, iterations=0, ff17=None):
        super().__init__(oracle, case, mode, cfl, ff17)
        self.to, self.frm, self.n_i = [], [], []
        for l in range(self.n):
            L = self.oc.levels[l]
            e = self.oc.edges(l)[L.internal_start:L.internal_start + L.n_internal]
            a, b = np.asarray(e["a"], dtype=np.int64), np.asarray(e["b"], dtype=np.int64)
            assert (a >= 0).all() and (b >= 0).all()
            to = np.empty(2 * len(a), dtype=np.int64)
            to[0::2], to[1::2] = a, b
            frm = np.empty_like(to)
            frm[0::2], frm[1::2] = b, a
            self.to.append(to)
            self.frm.append(frm)
            self.n_i.append(np.bincount(to, minlength=L.nel).astype(np.float64))
        self.set_residual_smoothing(eps, iterations)

    def set_residual_smoothing(self, eps, iterations=2):
        assert 0 <= iterations <= MAX_ITERATIONS and (iterations == 0 or (np.isfinite(eps) and eps > 0.0))
        self.eps, self.iterations = (np.float64(eps) if iterations else np.float64(0.0)), int(iterations)

    def smoothed_update(self, l, sf, fluxes):
        """Db(M) of level ``l`` from the step factors [nel] and the stage's fluxes [nel, 5]."""
        D = sf[:, None] * fluxes
        den = (1.0 + self.eps * self.n_i[l])[:, None]
        Db = D
        for _ in range(self.iterations):
            S = np.zeros_like(D)
            np.add.at(S, self.to[l], Db[self.frm[l]])
            Db = (D + self.eps * S) / den
        return Db

    def _sweep(self, l):
        if self.iterations == 0:
            return super()._sweep(l)
        lib, L = self.lib, self.oc.levels[l]
        C.memmove(L.old_variables, L.variables, 8 * L.nel * 5)
        sf = self.oc.array(l, "step_factors")
        sf[:] = tse.step_factors(self.mode, self.cfl, self.oc.array(l, "variables"), self.oc.array(l, "volumes"),
                                 self.cbrt_vol[l], self.variant)
        if self.on_step_factors:
            self.on_step_factors(l, sf)
        fluxes = self.oc.array(l, "fluxes").reshape(-1, 5)
        old = self.oc.array(l, "old_variables").reshape(-1, 5)
        var = self.oc.array(l, "variables").reshape(-1, 5)
        for j in range(RK):
            lib.ora_compute_flux_edge(L.internal_start, L.n_internal, L.edges, L.variables, L.fluxes)
            lib.ora_compute_boundary_flux_edge(L.boundary_start, L.n_boundary, L.edges, L.variables, L.fluxes)
            lib.ora_compute_wall_flux_edge(L.wall_start, L.n_wall, L.edges, L.variables, L.fluxes, C.byref(self.ff))
            var[:] = old + self.smoothed_update(l, sf, fluxes) / np.float64(RK + 1 - j)
            fluxes[:] = 0.0
            rc = lib.ora_check_for_invalid_variables(L.variables, L.nel, None)
            if rc:
                return rc
        lib.ora_residual(L.nel, L.old_variables, L.variables, L.residuals)
        return 0
