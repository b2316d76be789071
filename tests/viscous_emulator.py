"""The yardstick of the laminar viscous terms (mgcfd_set_viscous): ``ViscousOracle``, the composed oracle of tests/fas_emulator.py
(and so of the JST, dual-time, residual-smoothing and time-step emulators below it) with the node stresses ``S``, the viscous flux
``V``, the viscous step limit and the no-slip wall written in numpy from the definition in include/mgcfd.h / INTEGRATION.md §13.
Every inviscid flux, transfer and residual stays the oracle's entry point.

Over the internal edges (a, b, e) of a level, in the level's original edge order, with W the state the fluxes were computed from;
the normal seen from end a is n = +e, from end b n = -e:

    pass 1   u, v, w = momentum / rho;  T = p / rho (jst_emulator.pressure)
             A[phi][d] += (phi_j - phi_i) * n_d    from +0.0, one addition per edge at i;    G = (0.5 * A) / vol
             div = (G[u][x] + G[v][y]) + G[w][z];  t = (2.0/3.0) * div;  txx = mu * (2.0 * G[u][x] - t) ...;  txy = mu * (G[u][y] + G[v][x]) ...
             q_d = kappa * G[T][d],  kappa = (mu * GAMMA) / ((GAMMA - 1.0) * prandtl)
             S_i = (u, v, w, txx, tyy, tzz, txy, txz, tyz, qx, qy, qz)
    pass 2   bars = 0.5 * (S_i + S_j);  fx = (txx*nx + txy*ny) + txz*nz ...;  ex = ((u*txx + v*txy) + w*txz) + qx ...
             fe = (ex*nx + ey*ny) + ez*nz;   V_i[1..4] += (fx, fy, fz, fe)    from +0.0, same edges, same order
             F[i][v] = F[i][v] + V_i[v], v = 1..4
    limit    sf_i = min(sf_i, (k0 * rho_i) * g_i),  g_i = (cbrt(vol_i) * cbrt(vol_i)) / vol_i,  k0 = cfl_v / (max(4.0/3.0, GAMMA / prandtl) * mu)
    wall     variables[i][1..3] = +0.0 at the distinct b ends of the solid-wall (class -1) edges, behind every writer of variables

Every numpy operation is one IEEE-754 double operation per element (numpy never contracts to FMA); ``np.add.at`` is unbuffered
and adds in index order, so with the index arrays interleaved (a0, b0, a1, b1, ...) a node's sum runs over its edges in edge
order.  The hooks are subclassing and one more wrapper around the oracle library, behind JST's: V is added behind the far-field
faces of a stage (after C); the wall rule follows mg_restrict, the prolongation and, behind the invalid-state check of every stage,
the update; a viscous level's sweep is written out here because the limit sits between the step factors and dual time's clamp.
FasOracle.total_residual gains V through the wrapper.  While the terms are on for level 0 the RMS of a cycle is summed in dual
time stepping's fixed order.  ``levels = 0`` is ``FasOracle`` itself (tests/test_host_viscous.py checks the bits).

What the GPU tests run (tests/test_gpu_viscous.py), fixed by tests/test_host_viscous.py on the CPU.  Every run starts from
``start_state``: level 0 holds conftest's perturbed far field (seed START_SEED) — from the uniform far field itself the gradients,
and so V, are exactly zero in the first stage — written before the terms are switched on, so that the enabling call applies the
wall rule to it.  Chosen values and margins:

    GPU_MU       per case the smallest power of ten at which F + V differs in bits from F at more than half of level 0's nodes in
                 the first stage (fraction of nodes that differ at the chosen power / at the next smaller one):
                 lattice A 1e-16 (0.937 / 0.219), lattice B 1e-16 (0.762 / 0.095), m6_3lvl 1e-9 (0.729 / 0.114),
                 mixed_2lvl 1e-9 (0.641 / 0.117), tet_2lvl 1e-9 (0.979 / 0.390).  The condition only guards against a correction
                 that the addition absorbs; the goldens' weights are damped at load, which is why their power is larger.
    CELL_RE_MU   lattice A's second viscosity: cell Reynolds number rho_inf |V_inf| h / mu = 2 with h = 1/12 at the default far
                 field (rho 1.4, |V| 1.2): 0.07.
    VISCOUS_CFL  0.25 = MGCFD_VISCOUS_CFL.  Every combination (both steps, wall 0 and 1, level 0 alone and all levels, every
                 case at GPU_MU and lattice A at CELL_RE_MU too) stays valid for GPU_CYCLES cycles at each of (0.1, 0.25, 0.5).
                 "The viscous limit the binding one on lattice A" is read as: at CELL_RE_MU under local steps at CFL 1.0 the
                 limit is below the policy's step factor at EVERY node of level 0 in every sweep.  That holds at 0.1 and 0.25
                 (6,534 of 6,534 node-sweeps bound) and not at 0.5 (6,196 to 6,233 of 6,534), so 0.25 is the largest.  Under the
                 reference's step (CFL 0.5, legacy formula) the limit never binds at 0.25.
"""
import ctypes as C

import numpy as np

import dual_time_emulator as dte
import fas_emulator as fe
import jst_emulator as jse
import time_step_emulator as tse

GAMMA = 1.4
RK = 3
PRANDTL = 0.72
VISCOUS_CFLS = (0.1, 0.25, 0.5)
VISCOUS_CFL = 0.25

GPU_CYCLES = 3
GPU_STEPS = (("reference", 0.5), ("local", 1.0))
GPU_WALLS = (0, 1)
GPU_LEVELS = (1, "all")
GPU_LATTICES = ("A", "B")
GPU_GOLDENS = fe.GPU_GOLDENS
GPU_MU = {"A": 1e-16, "B": 1e-16, "m6_3lvl": 1e-9, "mixed_2lvl": 1e-9, "tet_2lvl": 1e-9}
CELL_RE, LATTICE_A_H = 2.0, 1.0 / 12.0
CELL_RE_MU = 0.07
START_SEED = 7
# the drop-in binary's runs (tests/test_gpu_viscous.py::test_driver_flags): from the far field, no-slip walls, all levels
DRIVER_CASES = ("fvcorr_1lvl", "m6_2lvl")
DRIVER_MU, DRIVER_REYNOLDS = 0.01, 168.0          # rho_inf |V_inf| L / Re = 1.4 * 1.2 * 1 / 168 = 0.01 up to rounding
# the composed runs, all on lattice A at CELL_RE_MU with wall = 1 on all levels:
# (name, mode, cfl, (eps, iterations), JST levels, BDF order or None, FAS)
COMPOSED = (("smoothing", "local", 2.0, (0.5, 2), 0, None, False),
            ("jst_level0", "local", 1.0, (0.0, 0), 1, None, False),
            ("dual_bdf2", "local", 1.0, (0.0, 0), 0, 2, False),
            ("fas", "local", 1.0, (0.0, 0), 0, None, True),
            ("all", "local", 2.0, (0.5, 2), 1, 2, True))
DUAL_STEPS, DUAL_CYCLES = 2, 3


def cell_re_mu(ff17):
    """mu at which rho_inf |V_inf| h / mu = CELL_RE on lattice A (h = 1/12), rounded to two digits."""
    ff = np.asarray(ff17, dtype=np.float64)
    speed = float(np.sqrt(((ff[1:4] / ff[0]) ** 2).sum()))
    return float("%.2e" % (float(ff[0]) * speed * LATTICE_A_H / CELL_RE))


def gpu_combinations():
    """(case key, mu, mode, cfl, wall, levels) of the bit-for-bit runs; a lattice's key is its letter, and lattice A runs at
    CELL_RE_MU as well."""
    out = []
    for case in GPU_LATTICES + GPU_GOLDENS:
        for mu in (GPU_MU[case], CELL_RE_MU) if case == "A" else (GPU_MU[case],):
            out += [(case, mu, mode, cfl, wall, lv) for mode, cfl in GPU_STEPS for wall in GPU_WALLS for lv in GPU_LEVELS]
    return out


def start_state(nel, ff_var):
    """Level 0's start state of the GPU runs."""
    from conftest import perturbed_state
    return perturbed_state(nel, ff_var, START_SEED)


def configured(oracle, case, mu, mode, cfl, wall, levels, smoothing=(0.0, 0), jst_levels=0, fas=False, cfl_v=VISCOUS_CFL):
    """The emulator as tests/test_gpu_viscous.py configures the solver: the start state, then the terms switched on."""
    em = ViscousOracle(oracle, case, mode, cfl, *smoothing, kappa2=jse.KAPPA2 if jst_levels else 0.0,
                       kappa4=jse.KAPPA4 if jst_levels else 0.0, levels=jst_levels, fas=fas)
    v = em._var(0)
    v[:] = start_state(len(v), em.ff17[:5])
    em.set_viscous(mu, PRANDTL, wall, cfl_v, levels)
    return em


def conductivity(mu, prandtl):
    return (np.float64(mu) * GAMMA) / ((GAMMA - 1.0) * np.float64(prandtl))


def interleaved(a, b, e):
    """(to, frm, N): per edge end in the order (a0, b0, a1, b1, ...) the node, the other node and the normal seen from the node."""
    to = np.empty(2 * len(a), dtype=np.int64)
    to[0::2], to[1::2] = a, b
    frm = np.empty_like(to)
    frm[0::2], frm[1::2] = b, a
    N = np.empty((2 * len(a), 3))
    for d, name in enumerate("xyz"):
        x = np.asarray(e[name], dtype=np.float64)
        N[0::2, d], N[1::2, d] = x, -x
    return to, frm, N


def primitives(W):
    """(u, v, w, T) [nel, 4] of a state [nel, 5]."""
    q = np.asarray(W, dtype=np.float64).reshape(-1, 5)
    rho = q[:, 0]
    return np.stack([q[:, 1] / rho, q[:, 2] / rho, q[:, 3] / rho, jse.pressure(q) / rho], axis=1)


def gradients(phi, to, frm, N, vol):
    """G [nel, n_phi, 3] of the fields phi [nel, n_phi]: pass 1's sums and division."""
    A = np.zeros((len(phi), phi.shape[1], 3))
    d = phi[frm] - phi[to]
    for k in range(phi.shape[1]):
        np.add.at(A[:, k, :], to, d[:, k][:, None] * N)
    return (0.5 * A) / np.asarray(vol, dtype=np.float64)[:, None, None]


def stresses(W, to, frm, N, vol, mu, kappa):
    """Pass 1: S [nel, 12]."""
    with np.errstate(all="ignore"):
        phi = primitives(W)
        G = gradients(phi, to, frm, N, vol)
        mu, kappa = np.float64(mu), np.float64(kappa)
        ux, uy, uz = G[:, 0, 0], G[:, 0, 1], G[:, 0, 2]
        vx, vy, vz = G[:, 1, 0], G[:, 1, 1], G[:, 1, 2]
        wx, wy, wz = G[:, 2, 0], G[:, 2, 1], G[:, 2, 2]
        div = (ux + vy) + wz
        t = (2.0 / 3.0) * div
        S = np.empty((len(phi), 12))
        S[:, 0:3] = phi[:, 0:3]
        S[:, 3], S[:, 4], S[:, 5] = mu * (2.0 * ux - t), mu * (2.0 * vy - t), mu * (2.0 * wz - t)
        S[:, 6], S[:, 7], S[:, 8] = mu * (uy + vx), mu * (uz + wx), mu * (vz + wy)
        S[:, 9:12] = kappa * G[:, 3, :]
    return S


def viscous_flux(S, to, frm, N):
    """Pass 2: V [nel, 5] (column 0 stays +0.0)."""
    with np.errstate(all="ignore"):
        b = 0.5 * (S[to] + S[frm])
        u, v, w, txx, tyy, tzz, txy, txz, tyz, qx, qy, qz = (b[:, k] for k in range(12))
        nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
        fx = (txx * nx + txy * ny) + txz * nz
        fy = (txy * nx + tyy * ny) + tyz * nz
        fz = (txz * nx + tyz * ny) + tzz * nz
        ex = ((u * txx + v * txy) + w * txz) + qx
        ey = ((u * txy + v * tyy) + w * tyz) + qy
        ez = ((u * txz + v * tyz) + w * tzz) + qz
        fe_ = (ex * nx + ey * ny) + ez * nz
        V = np.zeros((len(S), 5))
        for col, f in ((1, fx), (2, fy), (3, fz), (4, fe_)):
            np.add.at(V[:, col], to, f)
    return V


def limit_step_factors(sf, rho, g, mu, prandtl, cfl_v):
    """sf = min(sf, (k0 * rho) * g); a NaN factor stays NaN."""
    kv = max(4.0 / 3.0, GAMMA / float(prandtl))
    k0 = np.float64(float(cfl_v) / (kv * float(mu)))
    with np.errstate(all="ignore"):
        cap = (k0 * rho) * g
    return np.where(cap < sf, cap, sf)


class _ViscousLib:
    """The oracle library (behind JST's wrapper) with V added behind a stage's far-field faces on viscous levels, the wall rule
    behind the writers of variables and, while level 0 is viscous, calc_rms in the fixed order.  Everything else, and
    everything while the terms are off, passes through."""

    def __init__(self, lib, owner):
        self._lib, self._owner = lib, owner

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def _level_of(self, attr, pointer):
        em = self._owner
        for l in range(min(em.visc_levels, em.n)):
            if getattr(em.oc.levels[l], attr) == pointer:
                return l
        return None

    def ora_compute_wall_flux_edge(self, start, n, edges, variables, fluxes, ff):
        rc = self._lib.ora_compute_wall_flux_edge(start, n, edges, variables, fluxes, ff)      # (+ C on a JST level)
        l = self._level_of("fluxes", fluxes)
        if l is not None:
            assert self._owner.oc.levels[l].variables == variables
            self._owner.add_viscous_flux(l)
        return rc

    def ora_check_for_invalid_variables(self, variables, nel, bad):
        rc = self._lib.ora_check_for_invalid_variables(variables, nel, bad)          # the check looks at the update's result
        l = self._level_of("variables", variables)
        if l is not None:
            self._owner.apply_wall(l)
        return rc

    def ora_mg_restrict(self, fine, coarse, *rest):
        rc = self._lib.ora_mg_restrict(fine, coarse, *rest)
        l = self._level_of("variables", coarse)
        if l is not None:
            self._owner.apply_wall(l)
        return rc

    def ora_prolong_residuals_interpolate_proper(self, edges, n_internal, res_c, res_f, var_f, *rest):
        rc = self._lib.ora_prolong_residuals_interpolate_proper(edges, n_internal, res_c, res_f, var_f, *rest)
        l = self._level_of("variables", var_f)
        if l is not None:
            self._owner.apply_wall(l)
        return rc

    def ora_calc_rms(self, nel, residuals):
        em = self._owner
        if em.visc_levels == 0:
            return self._lib.ora_calc_rms(nel, residuals)
        assert residuals == em.oc.levels[0].residuals
        return float(np.sqrt(dte.ordered_sumsq(em.oc.array(0, "residuals")) / np.float64(nel)))


class ViscousOracle(fe.FasOracle):
    """FasOracle with the settings of mgcfd_set_viscous."""

    def __init__(self, oracle, case, mode="reference", cfl=0.5, eps=0.0, iterations=0, ff17=None, kappa2=0.0, kappa4=0.0, levels=0,
                 fas=False, mu=0.0, prandtl=PRANDTL, wall=0, cfl_v=VISCOUS_CFL, viscous_levels=0):
        self.visc_levels = 0
        super().__init__(oracle, case, mode, cfl, eps, iterations, ff17, kappa2, kappa4, levels, fas)
        self.vto, self.vfrm, self.vN, self.g, self.wall_nodes = [], [], [], [], []
        for l in range(self.n):
            L = self.oc.levels[l]
            edges = self.oc.edges(l)
            to, frm, N = interleaved(self.ea[l], self.eb[l], edges[L.internal_start:L.internal_start + L.n_internal])
            self.vto.append(to)
            self.vfrm.append(frm)
            self.vN.append(N)
            cb = self.cbrt_vol[l]
            self.g.append((cb * cb) / self.oc.array(l, "volumes"))
            self.wall_nodes.append(np.unique(np.asarray(edges[L.boundary_start:L.boundary_start + L.n_boundary]["b"], dtype=np.int64)))
        self.lib = _ViscousLib(self.lib, self)
        self.last_S, self.last_V = [None] * self.n, [None] * self.n      # per level: S and V of the last stage
        self.limited = [[0, 0] for _ in range(self.n)]                   # per level: nodes the viscous limit bound / left alone
        self.mu, self.prandtl, self.wall, self.cfl_v = 0.0, 0.0, 0, 0.0
        self.set_viscous(mu, prandtl, wall, cfl_v, viscous_levels)

    def set_viscous(self, mu, prandtl=PRANDTL, wall=0, cfl_v=VISCOUS_CFL, levels=1):
        levels = self.n if levels == "all" else int(levels)
        assert levels >= 0
        if levels:
            assert np.isfinite(mu) and mu > 0.0 and np.isfinite(prandtl) and prandtl > 0.0 and np.isfinite(cfl_v) and cfl_v > 0.0
            assert wall in (0, 1)
        self.visc_levels = min(levels, self.n)
        on = self.visc_levels > 0
        self.mu, self.prandtl, self.cfl_v = (float(mu), float(prandtl), float(cfl_v)) if on else (0.0, 0.0, 0.0)
        self.wall = int(wall) if on else 0
        for l in range(self.visc_levels):
            self.apply_wall(l)

    def viscous_on(self, l):
        return l < self.visc_levels

    def apply_wall(self, l):
        if self.viscous_on(l) and self.wall:
            self._var(l)[self.wall_nodes[l], 1:4] = 0.0

    def set_far_field(self, ff17, reinitialise):
        super().set_far_field(ff17, reinitialise)
        if reinitialise:
            for l in range(getattr(self, "visc_levels", 0)):
                self.apply_wall(l)

    def viscous_terms(self, l, W=None):
        """(S [nel, 12], V [nel, 5]) of level ``l`` for the state ``W`` (default: its current variables)."""
        W = self._var(l) if W is None else W
        S = stresses(W, self.vto[l], self.vfrm[l], self.vN[l], self.oc.array(l, "volumes"), self.mu, conductivity(self.mu, self.prandtl))
        return S, viscous_flux(S, self.vto[l], self.vfrm[l], self.vN[l])

    def add_viscous_flux(self, l):
        self.last_S[l], self.last_V[l] = self.viscous_terms(l)
        fluxes = self.oc.array(l, "fluxes").reshape(-1, 5)
        fluxes[:, 1:5] = fluxes[:, 1:5] + self.last_V[l][:, 1:5]

    def final_step_factors(self, l):
        """The step factors of a sweep of a viscous level from its current variables: policy, viscous limit, dual-time clamp."""
        vol = self.oc.array(l, "volumes")
        free = tse.step_factors(self.mode, self.cfl, self.oc.array(l, "variables"), vol, self.cbrt_vol[l], self.variant)
        sf = limit_step_factors(free, self._var(l)[:, 0], self.g[l], self.mu, self.prandtl, self.cfl_v)
        n_bound = int((sf < free).sum())
        self.limited[l][0] += n_bound
        self.limited[l][1] += len(sf) - n_bound
        if self.dt != 0.0:
            sf = dte.clamp_step_factors(sf, vol, self.dt, self.clamp)
        return sf

    def _sweep(self, l):
        if not self.viscous_on(l):
            return super()._sweep(l)
        lib, L = self.lib, self.oc.levels[l]
        C.memmove(L.old_variables, L.variables, 8 * L.nel * 5)
        sf = self.oc.array(l, "step_factors")
        sf[:] = self.final_step_factors(l)
        if self.on_step_factors:
            self.on_step_factors(l, sf)
        fluxes = self.oc.array(l, "fluxes").reshape(-1, 5)
        old = self.oc.array(l, "old_variables").reshape(-1, 5)
        var = self._var(l)
        forced = self.fas and l >= 1
        for j in range(RK):
            lib.ora_compute_flux_edge(L.internal_start, L.n_internal, L.edges, L.variables, L.fluxes)
            lib.ora_compute_boundary_flux_edge(L.boundary_start, L.n_boundary, L.edges, L.variables, L.fluxes)
            lib.ora_compute_wall_flux_edge(L.wall_start, L.n_wall, L.edges, L.variables, L.fluxes, C.byref(self.ff))     # (+ C, + V)
            if self.dt == 0.0 and not forced and not self.iterations:
                lib.ora_time_step(j, L.nel, L.step_factors, L.fluxes, L.old_variables, L.variables)
            else:
                fp = fluxes.copy()
                if self.dt != 0.0:
                    fp = fp - self.stage_source(l, var)
                if forced:
                    fp = fp + self.P[l]                  # the forcing is the last addition
                if self.iterations:
                    var[:] = old + self.smoothed_update(l, sf, fp) / np.float64(RK + 1 - j)
                else:
                    factor = sf / np.float64(RK + 1 - j)
                    var[:] = old + factor[:, None] * fp
                fluxes[:] = 0.0
            rc = lib.ora_check_for_invalid_variables(L.variables, L.nel, None)          # (then the wall rule: the wrapper)
            if rc:
                return rc
        lib.ora_residual(L.nel, L.old_variables, L.variables, L.residuals)
        return 0
