"""The yardstick of multigrid cycle control (mgcfd_set_cycle, mgcfd_run_cycles_from, mgcfd_prolong_state, mgcfd_full_multigrid):
``CycleOracle``, the composed oracle of tests/viscous_emulator.py (and so of the FAS, JST, dual-time, residual-smoothing and
time-step emulators below it) with the recursion of include/mgcfd.h / INTEGRATION.md §15 written out.  Every sweep, transfer and
FAS leg stays the emulators' it is built on; nothing in their definitions changes.

    visit(l, kind):
        pre[l] times: sweep(l)              l == top: the cycle's RMS after the LAST of these
        if l == n-1: return
        down(l)                             ora_mg_restrict; with FAS on, FasOracle.fas_restrict's steps
        visit(l+1, kind)
        if l+1 < n-1:  W: visit(l+1, W);  F: visit(l+1, V)
        up(l)                               ora_prolong_residuals_interpolate_proper; with FAS on, FasOracle.fas_prolong
        post[l] times: sweep(l)

    top > 0 (cycles_from): level ``top`` plays level 0's part and is unforced under FAS — its sweeps take R_top(W) without P_top,
        down(top) uses T = R_top, and the stored P_top is neither read nor written.  The RMS is sqrt(S / nel_top) with S summed
        in dual_time_emulator.ordered_sumsq's order over the level's original numbering, whatever the other settings are.
    prolong_state(fine): through the oracle's own ora_prolong_residuals_interpolate_proper with the fine variables and residuals
        +0.0 and the coarse residuals holding the coarse state, then 0.0 - result; the residual arrays are saved and restored.
    full_multigrid(cycles): ora_mg_restrict(l) for l = 0 .. n-2, then for top = n-1 .. 1 cycles_from(top, cycles[top]) and
        prolong_state(top - 1).

With the default configuration ``cycles`` is the parent's method itself (tests/test_host_cycle.py checks the bits).  ``work`` adds
up the sweeps run, each weighted by nel_l / nel_0: the unit of profiles/cycle_convergence.txt.
"""
import numpy as np

import dual_time_emulator as dte
import fas_emulator as fe
import viscous_emulator as ve

SHAPES = ("V", "W", "F")
MAX_SWEEPS = 8
MAX_CYCLES = dte.MAX_ADVANCE_CYCLES

# What the tests run.  Lattice C has four levels (4,886 / 2,178 / 728 / 215 nodes), so that F and W differ; lattice A has three,
# on which they are the same cycle.
LATTICES = dict(fe.LATTICES, C=(17, 13, 9, 6))
GPU_GOLDENS = fe.GPU_GOLDENS
GPU_LATTICES = ("A", "C")
NUM_LEVELS = {"m6_3lvl": 3, "mixed_2lvl": 2, "tet_2lvl": 2, "A": 3, "C": 4}
GPU_CYCLES = 4
VALID_CYCLES = 6
GPU_POST0 = (0, 1)
GPU_STEPS = fe.GPU_LATTICE_STEPS                 # (mode, cfl) under FAS on the lattices: reference 0.5, local 1.0, global 1.0
GPU_GLOBAL_STEP = ("global", 0.5)                # ... and with the reference's transfers there, beside ("reference", 0.5)
SMALLEST_CASE = "tet_2lvl"                       # 420 / 90 nodes: pre and post at MAX_SWEEPS run once here
# convergence on lattice C (tests/test_host_cycle.py): FAS, local steps at CFL 1.0, from the far field
CONV_CYCLES, CONV_SHAPED_BOUND, CONV_V_FLOOR = 60, 1e-4, 1e-2


# the composed run, on lattice A: viscous_emulator.COMPOSED's "all" — local steps at CFL 2.0, smoothing (0.5, 2), JST on level 0,
# FAS, the viscous terms at cell Reynolds number 2 with no-slip walls on all levels, from viscous_emulator.start_state — under
# W with post[0] = 1.  Without dual time's source this composition does not settle on the emulator whatever the cycle (the default V
# goes invalid in its sixth cycle, W with the post-sweep in its third, at CFL 1.0 as at 2.0: the viscous limit binds), so the
# steady run is two cycles; under BDF2 it is advance(DUAL_STEPS, DUAL_CYCLES) as that file's runs.
COMPOSED_MODE, COMPOSED_CFL, COMPOSED_SMOOTHING, COMPOSED_JST_LEVELS = "local", 2.0, (0.5, 2), 1
COMPOSED_CYCLES, COMPOSED_STEPS, COMPOSED_STEP_CYCLES = 2, ve.DUAL_STEPS, ve.DUAL_CYCLES


def composed_run(oracle, case, dual):
    """(emulator at its end, rc, rms, dt or None) of the composed run; ``dual``: inside advance with BDF2."""
    import jst_emulator as jse
    em = CycleOracle(oracle, case, COMPOSED_MODE, COMPOSED_CFL, *COMPOSED_SMOOTHING, kappa2=jse.KAPPA2, kappa4=jse.KAPPA4,
                     levels=COMPOSED_JST_LEVELS, fas=True)
    v = em._var(0)
    v[:] = ve.start_state(len(v), em.ff17[:5])
    em.set_viscous(ve.CELL_RE_MU, ve.PRANDTL, 1, ve.VISCOUS_CFL, "all")
    pre, post = default_sweeps(em.n)
    em.set_cycle("W", pre, [1] + post[1:])
    if not dual:
        rc, rms = em.cycles(COMPOSED_CYCLES)
        return em, rc, rms, None
    dt = dte.pick_dt(oracle, case, COMPOSED_MODE, COMPOSED_CFL)
    em.set_dual_time(dt)
    em.set_order(2)
    rc, rms = em.advance(COMPOSED_STEPS, COMPOSED_STEP_CYCLES)
    return em, rc, rms, dt


def write_lattice(name, directory):
    """fas_emulator.write_lattice for the lattices of this file (C included)."""
    import os
    from mgcfd import meshgen
    d = os.path.join(str(directory), "lattice_" + name)
    os.makedirs(os.path.join(d, "input"))
    meshgen.write_input(meshgen.make_multigrid(LATTICES[name], "fvcorr", **fe.LATTICE_ARGS), os.path.join(d, "input"))
    with open(os.path.join(d, "case.txt"), "w") as f:
        f.write("duplicate = 1\n")
    return d


def default_sweeps(n):
    """(pre, post) of the default cycle on n levels; post[n-1] is ignored and reported as its default."""
    return [1] * n, [0] + [1] * (n - 1)


def gpu_configurations(n):
    """(shape, pre, post) of the bit-for-bit runs on n levels: every shape x post[0] in GPU_POST0, and pre = (2, 1, ...) under W."""
    pre, post = default_sweeps(n)
    out = [(shape, list(pre), [p0] + post[1:]) for shape in SHAPES for p0 in GPU_POST0]
    out.append(("W", [2] + pre[1:], list(post)))
    return out


class CycleOracle(ve.ViscousOracle):
    """ViscousOracle with the settings of mgcfd_set_cycle and the three calls built on the cycle."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.shape = "V"
        self.pre, self.post = default_sweeps(self.n)
        self.top = 0
        self.work = 0.0

    def set_cycle(self, shape="V", pre=None, post=None):
        d_pre, d_post = default_sweeps(self.n)
        pre = d_pre if pre is None else [int(x) for x in pre]
        post = d_post if post is None else [int(x) for x in post]
        assert shape in SHAPES and len(pre) == self.n and len(post) == self.n
        assert all(1 <= x <= MAX_SWEEPS for x in pre) and all(0 <= x <= MAX_SWEEPS for x in post[:self.n - 1])
        post[self.n - 1] = d_post[self.n - 1]
        self.shape, self.pre, self.post = shape, pre, post

    def get_cycle(self):
        return self.shape, list(self.pre), list(self.post)

    def default_cycle(self):
        return (self.shape, self.pre, self.post) == ("V",) + tuple(default_sweeps(self.n))

    # ---- the top-level rule: level ``top`` > 0 is unforced while a run of cycles starts from it ----
    def _sweep(self, l):
        self.work += self.oc.levels[l].nel / self.oc.levels[0].nel
        if self.fas and 0 < l == self.top:
            self.fas = False                             # (the sweep of a solver with FAS off: R_top(W) without P_top)
            try:
                return super()._sweep(l)
            finally:
                self.fas = True
        return super()._sweep(l)

    def fas_restrict(self, l):
        if l != self.top or l == 0:
            return super().fas_restrict(l)
        keep = self.P[l]
        self.P[l] = None                                 # neither read ...
        try:
            L = self.oc.levels
            T = self.total_residual(l)                   # T = R_top
            self.lib.ora_mg_restrict(L[l].variables, L[l + 1].variables, L[l + 1].nel, L[l].mg_map, self.O.ptr(self.scratch), L[l].mgc)
            self.W0[l + 1] = self._var(l + 1).copy()
            parent = np.asarray(self.oc.mg_map(l), dtype=np.int64)
            Q = np.zeros((L[l + 1].nel, 5))
            np.add.at(Q, parent, T)
            has_children = np.bincount(parent, minlength=L[l + 1].nel) > 0
            self.P[l + 1] = np.where(has_children[:, None], Q - self.total_residual(l + 1), 0.0)
        finally:
            self.P[l] = keep                             # ... nor written

    # ---- the recursion ----
    def _down(self, l):
        L = self.oc.levels
        if self.fas:
            self.fas_restrict(l)
        else:
            self.lib.ora_mg_restrict(L[l].variables, L[l + 1].variables, L[l + 1].nel, L[l].mg_map, self.O.ptr(self.scratch), L[l].mgc)

    def _up(self, l):
        L = self.oc.levels
        if self.fas:
            self.fas_prolong(l)
        else:
            self.lib.ora_prolong_residuals_interpolate_proper(L[l].edges, L[l].n_internal, L[l + 1].residuals, L[l].residuals,
                                                              L[l].variables, L[l].nel, L[l].mg_map, L[l + 1].coords, L[l].coords)

    def _rms(self):
        L = self.oc.levels
        if self.top > 0 or self.fas:
            return float(np.sqrt(dte.ordered_sumsq(self.oc.array(self.top, "residuals")) / np.float64(L[self.top].nel)))
        return self.lib.ora_calc_rms(L[0].nel, L[0].residuals)              # (the wrappers below fix its order where an option does)

    def _visit(self, l, kind, rms):
        for k in range(self.pre[l]):
            rc = self._sweep(l)
            if rc:
                return rc
            if l == self.top and k == self.pre[l] - 1:
                rms.append(self._rms())
        if l == self.n - 1:
            return 0
        self._down(l)
        rc = self._visit(l + 1, kind, rms)
        if rc:
            return rc
        if l + 1 < self.n - 1 and kind != "V":
            rc = self._visit(l + 1, "W" if kind == "W" else "V", rms)
            if rc:
                return rc
        self._up(l)
        for _ in range(self.post[l]):
            rc = self._sweep(l)
            if rc:
                return rc
        return 0

    def cycles(self, count):
        if self.default_cycle() and self.top == 0:
            return super().cycles(count)
        rms = []
        for _ in range(count):
            rc = self._visit(self.top, self.shape, rms)
            if rc:
                return rc, np.array(rms)
        return 0, np.array(rms)

    def cycles_from(self, top, count):
        """mgcfd_run_cycles_from: (rc, rms [count])."""
        assert 0 <= top < self.n and count <= MAX_CYCLES and (top == 0 or self.dt == 0.0)
        self.top = top
        try:
            return self.cycles(count)
        finally:
            self.top = 0

    def prolong_state(self, fine):
        """mgcfd_prolong_state: variables[fine] = 0.0 - (0.0 - wavg(variables[fine + 1])); the wall rule follows (the wrapper)."""
        L = self.oc.levels
        res_c, res_f = self.oc.array(fine + 1, "residuals"), self.oc.array(fine, "residuals")
        keep_c, keep_f = res_c.copy(), res_f.copy()
        var = self._var(fine)
        var[:] = 0.0
        res_f[:] = 0.0
        res_c[:] = self.oc.array(fine + 1, "variables")
        self.lib.ora_prolong_residuals_interpolate_proper(L[fine].edges, L[fine].n_internal, L[fine + 1].residuals, L[fine].residuals,
                                                          L[fine].variables, L[fine].nel, L[fine].mg_map, L[fine + 1].coords, L[fine].coords)
        var[:] = 0.0 - var
        res_c[:] = keep_c
        res_f[:] = keep_f

    def full_multigrid(self, cycles):
        """mgcfd_full_multigrid: (rc, the concatenated RMS histories); cycles [n], cycles[0] ignored."""
        L = self.oc.levels
        assert len(cycles) == self.n
        for l in range(self.n - 1):
            self.lib.ora_mg_restrict(L[l].variables, L[l + 1].variables, L[l + 1].nel, L[l].mg_map, self.O.ptr(self.scratch), L[l].mgc)
        hist = []
        for top in range(self.n - 1, 0, -1):
            rc, rms = self.cycles_from(top, int(cycles[top]))
            hist.append(rms)
            if rc:
                return rc, np.concatenate(hist)
            self.prolong_state(top - 1)
        return 0, np.concatenate(hist) if hist else np.array([])
