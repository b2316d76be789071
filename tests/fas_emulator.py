"""The yardstick of FAS multigrid (mgcfd_set_fas): ``FasOracle``, the composed oracle of tests/jst_emulator.py (and so of the
dual-time, residual-smoothing and time-step emulators below it) with the forcing terms and the coarse-grid corrections written
in numpy from the definition in include/mgcfd.h / INTEGRATION.md §12.  Every flux, the state restriction and the prolongation
stay the oracle's entry points; step factors, the Jacobi iterations, the dual-time source and the JST correction stay the
emulators' it is built on.

    R_l(W)      the fluxes of level l from zero (+ C where JST covers l: jst_emulator's wrapper adds it), - src under dual time
    forced      on a level l >= 1 every stage takes F' = R_l(W) + P_l, the forcing last
    down leg    T_l = R_l(variables[l]) (+ P_l for l >= 1);  mg_restrict of the state;  W0 = a copy of variables[l+1];
                Q[c] += T_l[child] over the children in ascending fine id, from +0.0;
                P_{l+1} = Q - R_{l+1}(W0) where a coarse node has children, +0.0 where it has none
    up leg      D = W0 - variables[l+1];  prolong_residuals_interpolate_proper with residuals1 = D and residuals2 = +0.0

Every numpy operation is one IEEE-754 double operation per element (numpy never contracts to FMA); ``np.add.at`` is unbuffered
and adds in index order, so with the fine ids ascending a coarse node's sum runs over its children in ascending fine id — the
order of mg_restrict.  While FAS is on the RMS of a cycle is summed in dual time stepping's fixed order
(``dual_time_emulator.ordered_sumsq``).  With FAS off every method is the parent's (tests/test_host_fas.py checks the bits).
"""
import ctypes as C
import os

import numpy as np

import dual_time_emulator as dte
import jst_emulator as jse
import time_step_emulator as tse

RK = 3

# The two generated lattices of the tests (tests/test_host_fas.py, tests/test_gpu_fas.py): undamped (mesh_name = fvcorr), non-nested,
# with a cavity, so that the cycle's fixed point matters.  2,178 / 728 / 215 and 728 / 124 nodes.
LATTICE_ARGS = dict(seed=11, cavity_radius=0.12, jitter=0.25, area_noise=0.08, volume_noise=0.1)
LATTICES = {"A": (13, 9, 6), "B": (9, 5)}
GPU_GOLDENS = ("m6_3lvl", "mixed_2lvl", "tet_2lvl")
GPU_CYCLES = 4
GPU_LATTICE_STEPS = (("reference", 0.5), ("local", 1.0), ("global", 1.0))
# convergence (lattice A) and fixed point (lattice B): local steps at CFL 1.0
CONV_CYCLES, CONV_BOUND = 60, 0.1
CONV_SMOOTHING, CONV_SMOOTHING_CFL = (0.5, 2), 2.0
FIXED_CYCLES, FIXED_BOUND = 200, 1e-8
# the composed runs of tests/test_gpu_fas.py, all on lattice A: (name, mode, cfl, (eps, iterations), JST levels, BDF order or None).
# With a BDF order the run is advance(DUAL_STEPS, DUAL_CYCLES) at dual_time_emulator.pick_dt's physical step, else GPU_CYCLES cycles.
COMPOSED = (("smoothing", "local", 2.0, (0.5, 2), 0, None),
            ("jst_level0", "local", 1.0, (0.0, 0), 1, None),
            ("jst_all", "local", 1.0, (0.0, 0), "all", None),
            ("dual_bdf1", "local", 1.0, (0.0, 0), 0, 1),
            ("dual_bdf2", "local", 1.0, (0.0, 0), 0, 2),
            ("all_three", "local", 2.0, (0.5, 2), "all", 2))
DUAL_STEPS, DUAL_CYCLES = 3, 4


def composed_run(oracle, case, mode, cfl, smoothing, jst_levels, order):
    """One run of COMPOSED on the emulator: (emulator at its end, rc, rms, dt or None)."""
    em = FasOracle(oracle, case, mode, cfl, *smoothing, kappa2=jse.KAPPA2 if jst_levels else 0.0, kappa4=jse.KAPPA4 if jst_levels else 0.0,
                   levels=jst_levels, fas=True)
    if order is None:
        rc, rms = em.cycles(GPU_CYCLES)
        return em, rc, rms, None
    dt = dte.pick_dt(oracle, case, mode, cfl)
    em.set_dual_time(dt)
    em.set_order(order)
    rc, rms = em.advance(DUAL_STEPS, DUAL_CYCLES)
    return em, rc, rms, dt


def write_lattice(name, directory):
    """Lattice ``name`` as a case directory of the emulators' kind — ``<directory>/input/input.dat`` and ``case.txt`` — whose
    path serves wherever a golden case's name does (``free_stream_emulator.case_input`` joins an absolute path unchanged)."""
    from mgcfd import meshgen
    d = os.path.join(str(directory), "lattice_" + name)
    os.makedirs(os.path.join(d, "input"))
    meshgen.write_input(meshgen.make_multigrid(LATTICES[name], "fvcorr", **LATTICE_ARGS), os.path.join(d, "input"))
    with open(os.path.join(d, "case.txt"), "w") as f:
        f.write("duplicate = 1\n")
    return d


class FasOracle(jse.JstOracle):
    """JstOracle with the switch of mgcfd_set_fas."""

    def __init__(self, oracle, case, mode="reference", cfl=0.5, eps=0.0, iterations=0, ff17=None, kappa2=0.0, kappa4=0.0, levels=0,
                 fas=False):
        super().__init__(oracle, case, mode, cfl, eps, iterations, ff17, kappa2, kappa4, levels)
        self.fas = False
        self.P, self.W0 = [None] * self.n, [None] * self.n
        self.max_abs_D = [0.0] * self.n                  # per level >= 1: max |W0 - W| of the last up leg
        self.set_fas(fas)

    def set_fas(self, on=True):
        assert not on or self.n >= 2
        for l in range(1, self.n):
            shape = (self.oc.levels[l].nel, 5)
            self.P[l] = np.zeros(shape) if on else None                      # (zeroed by every enabling call)
            self.W0[l] = (np.zeros(shape) if self.W0[l] is None else self.W0[l]) if on else None
        self.fas = bool(on)

    def set_far_field(self, ff17, reinitialise):
        super().set_far_field(ff17, reinitialise)
        if reinitialise and getattr(self, "fas", False):
            for l in range(1, self.n):
                self.P[l][:] = 0.0

    def total_residual(self, l):
        """R_l of level ``l``'s current variables [nel, 5], from zero fluxes, which stay zero."""
        L = self.oc.levels[l]
        fluxes = self.oc.array(l, "fluxes").reshape(-1, 5)
        assert not fluxes.any()
        self.lib.ora_compute_flux_edge(L.internal_start, L.n_internal, L.edges, L.variables, L.fluxes)
        self.lib.ora_compute_boundary_flux_edge(L.boundary_start, L.n_boundary, L.edges, L.variables, L.fluxes)
        self.lib.ora_compute_wall_flux_edge(L.wall_start, L.n_wall, L.edges, L.variables, L.fluxes, C.byref(self.ff))    # (+ C on a JST level)
        r = fluxes.copy()
        fluxes[:] = 0.0
        if self.dt != 0.0:
            r = r - self.stage_source(l, self._var(l))
        return r

    def _sweep(self, l):
        if not self.fas or l == 0:
            return super()._sweep(l)
        lib, L = self.lib, self.oc.levels[l]
        C.memmove(L.old_variables, L.variables, 8 * L.nel * 5)
        vol = self.oc.array(l, "volumes")
        sf = self.oc.array(l, "step_factors")
        sf[:] = tse.step_factors(self.mode, self.cfl, self.oc.array(l, "variables"), vol, self.cbrt_vol[l], self.variant)
        if self.dt != 0.0:
            sf[:] = dte.clamp_step_factors(sf.copy(), vol, self.dt, self.clamp)
        if self.on_step_factors:
            self.on_step_factors(l, sf)
        fluxes = self.oc.array(l, "fluxes").reshape(-1, 5)
        old = self.oc.array(l, "old_variables").reshape(-1, 5)
        var = self._var(l)
        for j in range(RK):
            lib.ora_compute_flux_edge(L.internal_start, L.n_internal, L.edges, L.variables, L.fluxes)
            lib.ora_compute_boundary_flux_edge(L.boundary_start, L.n_boundary, L.edges, L.variables, L.fluxes)
            lib.ora_compute_wall_flux_edge(L.wall_start, L.n_wall, L.edges, L.variables, L.fluxes, C.byref(self.ff))
            fp = fluxes.copy()
            if self.dt != 0.0:
                fp = fp - self.stage_source(l, var)
            fp = fp + self.P[l]                          # the forcing is the last addition
            if self.iterations:
                var[:] = old + self.smoothed_update(l, sf, fp) / np.float64(RK + 1 - j)
            else:
                factor = sf / np.float64(RK + 1 - j)
                var[:] = old + factor[:, None] * fp
            fluxes[:] = 0.0
            rc = lib.ora_check_for_invalid_variables(L.variables, L.nel, None)
            if rc:
                return rc
        lib.ora_residual(L.nel, L.old_variables, L.variables, L.residuals)
        return 0

    def fas_restrict(self, l):
        """Down-leg steps 1-4 from level ``l``."""
        assert self.fas
        L = self.oc.levels
        T = self.total_residual(l)
        if l >= 1:
            T = T + self.P[l]
        self.lib.ora_mg_restrict(L[l].variables, L[l + 1].variables, L[l + 1].nel, L[l].mg_map, self.O.ptr(self.scratch), L[l].mgc)
        self.W0[l + 1] = self._var(l + 1).copy()
        parent = np.asarray(self.oc.mg_map(l), dtype=np.int64)
        assert len(parent) == L[l].nel
        Q = np.zeros((L[l + 1].nel, 5))
        np.add.at(Q, parent, T)
        has_children = np.bincount(parent, minlength=L[l + 1].nel) > 0
        self.P[l + 1] = np.where(has_children[:, None], Q - self.total_residual(l + 1), 0.0)

    def fas_prolong(self, l):
        """Up-leg steps 1-2 onto level ``l``; the residuals of both levels are saved and restored."""
        assert self.fas
        L = self.oc.levels
        res_c, res_f = self.oc.array(l + 1, "residuals"), self.oc.array(l, "residuals")
        keep_c, keep_f = res_c.copy(), res_f.copy()
        D = self.W0[l + 1] - self._var(l + 1)
        self.max_abs_D[l + 1] = float(np.abs(D).max())
        res_c[:] = D.ravel()
        res_f[:] = 0.0
        self.lib.ora_prolong_residuals_interpolate_proper(L[l].edges, L[l].n_internal, L[l + 1].residuals, L[l].residuals,
                                                          L[l].variables, L[l].nel, L[l].mg_map, L[l + 1].coords, L[l].coords)
        res_c[:] = keep_c
        res_f[:] = keep_f

    def cycles(self, count):
        if not self.fas:
            return super().cycles(count)
        L, n = self.oc.levels, self.n
        rms = []
        for _ in range(count):
            for l in range(n):
                rc = self._sweep(l)
                if rc:
                    return rc, np.array(rms)
                if l == 0:
                    rms.append(float(np.sqrt(dte.ordered_sumsq(self.oc.array(0, "residuals")) / np.float64(L[0].nel))))
                if l + 1 < n:
                    self.fas_restrict(l)
            for l in range(n - 2, -1, -1):
                self.fas_prolong(l)
                if l > 0:
                    rc = self._sweep(l)
                    if rc:
                        return rc, np.array(rms)
        return 0, np.array(rms)

    def density_residual_rms(self):
        """The metric of the convergence tests: the RMS of component 0 of F_0(W) / vol."""
        L = self.oc.levels[0]
        fluxes = self.oc.array(0, "fluxes").reshape(-1, 5)
        assert not fluxes.any()
        self.lib.ora_compute_flux_edge(L.internal_start, L.n_internal, L.edges, L.variables, L.fluxes)
        self.lib.ora_compute_boundary_flux_edge(L.boundary_start, L.n_boundary, L.edges, L.variables, L.fluxes)
        self.lib.ora_compute_wall_flux_edge(L.wall_start, L.n_wall, L.edges, L.variables, L.fluxes, C.byref(self.ff))
        r = fluxes[:, 0] / self.oc.array(0, "volumes")
        fluxes[:] = 0.0
        return float(np.sqrt(np.mean(r * r)))
