"""The yardstick of the JST dissipation (mgcfd_set_jst): ``JstOracle``, the composed oracle of tests/dual_time_emulator.py (and so
of tests/residual_smoothing_emulator.py and tests/time_step_emulator.py) with the correction ``C`` written in numpy from the
definition in include/mgcfd.h / INTEGRATION.md §11 and added to every stage's fluxes on levels ``0 .. levels-1``.  Every flux,
transfer and residual stays the oracle's entry point; step factors, the Jacobi iterations and the dual-time source stay the
emulators' it is built on, and see ``F + C``.

Over the internal edges of a level, in the level's original edge order, with W the state the fluxes were computed from:

    pass 1   p_i, r_i = |v_i| + c_i            the reference's pressure and speeds (time_step_emulator.speed_plus_c's operations)
             L_i[v] += W_j[v] - W_i[v];   Pm_i += p_j - p_i;   Pp_i += p_j + p_i      from +0.0, one addition per edge at i
             nu_i = |Pm_i| / Pp_i         (0.0 for a node with no internal edge)
    pass 2   fac = k_e * (r_i + r_j),  k_e = -|e| * (double)0.2f * 0.5
             nu = max(nu_i, nu_j);  e2 = min(kappa2 * nu, 1.0);  e4 = max(kappa4 - e2, 0.0)
             C_i[v] += fac * ((e2 - 1.0) * (W_i[v] - W_j[v]) - e4 * (L_i[v] - L_j[v]))    from +0.0, same edges, same order
             F[i][v] = F[i][v] + C_i[v]

Every numpy operation is one IEEE-754 double operation per element (numpy never contracts to FMA); ``np.add.at`` is unbuffered
and adds in index order, so with the index arrays interleaved (a0, b0, a1, b1, ...) a node's sum runs over its edges in edge
order.  The correction is added behind the far-field faces of a stage — the last of the three flux calls of every emulator
below this one — by a wrapper around the oracle library, so that every ``_sweep`` of the parents composes unchanged.  While JST
is on for level 0 the RMS of a cycle is summed in dual time stepping's fixed order (``dual_time_emulator.ordered_sumsq``).
``levels = 0`` is ``DualTimeOracle`` itself: the wrapper passes everything through (tests/test_host_jst.py checks the bits).
"""
import numpy as np

import dual_time_emulator as dte
import free_stream_emulator as fse
import time_step_emulator as tse

GAMMA = 1.4
SMOOTHING = np.float64(np.float32(0.2))          # src/Base/common.h: a float literal widened to double
KAPPA2, KAPPA4 = 2.5, 0.15625                    # the textbook k2 = 1/2, k4 = 1/32 in units of the reference's 0.2

# What the GPU tests run (tests/test_gpu_jst.py): every case below with every pair of coefficients below on level 0 alone and
# on all levels, under the reference's time step and under local steps at LOCAL_CFL, GPU_CYCLES cycles, none skipped.
# tests/test_host_jst.py asserts on the CPU that each one stays valid, and that LOCAL_CFL is the largest of LOCAL_CFLS at which
# every case does.
GPU_CASES = fse.GPU_CASES
GPU_PAIRS = ((KAPPA2, KAPPA4), (0.0, KAPPA4))
GPU_LEVELS = (1, "all")
GPU_CYCLES = 3
LOCAL_CFLS = (1.0, 1.5)
LOCAL_CFL = 1.5
GPU_STEPS = (("reference", 0.5), ("local", LOCAL_CFL))
# the composed runs: residual smoothing under local steps, and dual time (BDF2) under dual_time_emulator's own setting
COMPOSED_CASE = "m6_2lvl"
COMPOSED_SMOOTHING = ("local", 1.5, (0.5, 2))
COMPOSED_DUAL = ("local15_smooth1", "local", 1.5, (0.5, 1), 2)      # one of dte.GPU_SETTINGS
COMPOSED_DUAL_STEPS, COMPOSED_DUAL_CYCLES = 2, 3


def gpu_combinations():
    return [(case, mode, cfl, k2, k4, lv) for case in GPU_CASES for mode, cfl in GPU_STEPS for k2, k4 in GPU_PAIRS for lv in GPU_LEVELS]


def pressure(variables):
    """derive()'s pressure per node, in the oracle's order of operations (oracle/mgcfd_oracle.c: load_point)."""
    q = np.asarray(variables, dtype=np.float64).reshape(-1, 5)
    rho, en = q[:, 0], q[:, 4]
    vx, vy, vz = q[:, 1] / rho, q[:, 2] / rho, q[:, 3] / rho
    speed_sqd = vx * vx + vy * vy + vz * vz
    return (GAMMA - 1.0) * (en - 0.5 * rho * speed_sqd)


def edge_weights(edges):
    """k_e per edge: -|e| * (double)0.2f * 0.5, left to right."""
    x, y, z = (np.asarray(edges[n], dtype=np.float64) for n in "xyz")
    return -np.sqrt(x * x + y * y + z * z) * SMOOTHING * 0.5


def sensor(W, a, b):
    """Pass 1 over the internal edges (a[k], b[k]) of a level in order: (L [nel, 5], nu [nel], r [nel])."""
    W = np.asarray(W, dtype=np.float64).reshape(-1, 5)
    to = np.empty(2 * len(a), dtype=np.int64)
    to[0::2], to[1::2] = a, b
    frm = np.empty_like(to)
    frm[0::2], frm[1::2] = b, a
    p = pressure(W)
    L = np.zeros_like(W)
    np.add.at(L, to, W[frm] - W[to])
    Pm, Pp = np.zeros(len(W)), np.zeros(len(W))
    np.add.at(Pm, to, p[frm] - p[to])
    np.add.at(Pp, to, p[frm] + p[to])
    has_edge = np.bincount(to, minlength=len(W)) > 0
    with np.errstate(all="ignore"):
        nu = np.where(has_edge, np.abs(Pm) / Pp, 0.0)
        r = tse.speed_plus_c(W)
    return L, nu, r


def switches(nu_i, nu_j, kappa2, kappa4):
    """(e2, e4) of an edge from its ends' sensors."""
    nu = np.where(nu_i > nu_j, nu_i, nu_j)
    e2 = np.float64(kappa2) * nu
    e2 = np.where(e2 < 1.0, e2, 1.0)
    e4 = np.float64(kappa4) - e2
    return e2, np.where(e4 > 0.0, e4, 0.0)


def edge_terms(W, L, nu, r, a, b, k_e, kappa2, kappa4):
    """Pass 2 per edge: (c_ab, c_ba) [n_edges, 5] each, the edge's contributions to its a end and to its b end."""
    W = np.asarray(W, dtype=np.float64).reshape(-1, 5)

    def side(i, j):
        fac = k_e * (r[i] + r[j])
        e2, e4 = switches(nu[i], nu[j], kappa2, kappa4)
        return fac[:, None] * ((e2 - 1.0)[:, None] * (W[i] - W[j]) - e4[:, None] * (L[i] - L[j]))

    with np.errstate(all="ignore"):
        return side(a, b), side(b, a)


def correction(W, a, b, k_e, kappa2, kappa4):
    """(C [nel, 5], L, nu, r) of one stage from its input state."""
    L, nu, r = sensor(W, a, b)
    c_ab, c_ba = edge_terms(W, L, nu, r, a, b, k_e, kappa2, kappa4)
    to = np.empty(2 * len(a), dtype=np.int64)
    to[0::2], to[1::2] = a, b
    terms = np.empty((2 * len(a), 5))
    terms[0::2], terms[1::2] = c_ab, c_ba
    Cn = np.zeros_like(L)
    np.add.at(Cn, to, terms)
    return Cn, L, nu, r


class _JstFluxes:
    """The oracle library with C added behind a stage's far-field faces on JST levels and, while level 0 is one, calc_rms in the
    fixed order (everything else, and everything while JST is off, passes through)."""

    def __init__(self, lib, owner):
        self._lib, self._owner = lib, owner

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def ora_compute_wall_flux_edge(self, start, n, edges, variables, fluxes, ff):
        rc = self._lib.ora_compute_wall_flux_edge(start, n, edges, variables, fluxes, ff)
        em = self._owner
        for l in range(min(em.jst_levels, em.n)):
            if em.oc.levels[l].fluxes == fluxes:
                assert em.oc.levels[l].variables == variables
                em.add_correction(l)
        return rc

    def ora_calc_rms(self, nel, residuals):
        em = self._owner
        if em.jst_levels == 0:
            return self._lib.ora_calc_rms(nel, residuals)
        assert residuals == em.oc.levels[0].residuals
        return float(np.sqrt(dte.ordered_sumsq(em.oc.array(0, "residuals")) / np.float64(nel)))


class JstOracle(dte.DualTimeOracle):
    """DualTimeOracle with the coefficients and levels of mgcfd_set_jst."""

    def __init__(self, oracle, case, mode="reference", cfl=0.5, eps=0.0, iterations=0, ff17=None, kappa2=0.0, kappa4=0.0, levels=0):
        super().__init__(oracle, case, mode, cfl, eps, iterations, ff17)
        self.ea, self.eb, self.k_e = [], [], []
        for l in range(self.n):
            L = self.oc.levels[l]
            e = self.oc.edges(l)[L.internal_start:L.internal_start + L.n_internal]
            self.ea.append(np.asarray(e["a"], dtype=np.int64))
            self.eb.append(np.asarray(e["b"], dtype=np.int64))
            self.k_e.append(edge_weights(e))
        self.lib = _JstFluxes(self.lib, self)
        self.last = [None] * self.n                      # per level: (C, L, nu, r) of the last stage
        self.set_jst(kappa2, kappa4, levels)

    def set_jst(self, kappa2=KAPPA2, kappa4=KAPPA4, levels=1):
        levels = self.n if levels == "all" else int(levels)
        assert levels >= 0 and np.isfinite(kappa2) and kappa2 >= 0.0 and np.isfinite(kappa4) and kappa4 >= 0.0
        assert levels == 0 or kappa2 > 0.0 or kappa4 > 0.0
        self.jst_levels = min(levels, self.n)
        self.kappa2, self.kappa4 = (float(kappa2), float(kappa4)) if self.jst_levels else (0.0, 0.0)

    def terms(self, l, W=None):
        """(C, L, nu, r) of level ``l`` for the state ``W`` (default: its current variables)."""
        W = self.oc.array(l, "variables").reshape(-1, 5) if W is None else W
        return correction(W, self.ea[l], self.eb[l], self.k_e[l], self.kappa2, self.kappa4)

    def add_correction(self, l):
        self.last[l] = self.terms(l)
        fluxes = self.oc.array(l, "fluxes").reshape(-1, 5)
        fluxes[:] = fluxes + self.last[l][0]

    def stage_fluxes(self, l):
        """F + C of level ``l``'s current variables [nel, 5] (mgcfd_compute_fluxes from zero fluxes); the fluxes stay zero."""
        import ctypes as C
        L = self.oc.levels[l]
        fluxes = self.oc.array(l, "fluxes").reshape(-1, 5)
        assert not fluxes.any()
        self.lib.ora_compute_flux_edge(L.internal_start, L.n_internal, L.edges, L.variables, L.fluxes)
        self.lib.ora_compute_boundary_flux_edge(L.boundary_start, L.n_boundary, L.edges, L.variables, L.fluxes)
        self.lib.ora_compute_wall_flux_edge(L.wall_start, L.n_wall, L.edges, L.variables, L.fluxes, C.byref(self.ff))
        out = fluxes.copy()
        fluxes[:] = 0.0
        return out
