"""The yardstick of the Spalart-Allmaras model (mgcfd_set_viscosity_model with MGCFD_EDDY_SPALART_ALLMARAS): ``SaOracle``,
tests/wall_distance_emulator.py's ``WallDampedOracle`` (``VariableViscosityOracle`` plus the wall distance) with the definition of
INTEGRATION.md §18 written in numpy, line by line.  Every numpy operation is one IEEE-754 double operation per element (numpy
never contracts to FMA, its sqrt is correctly rounded); ``np.add.at`` adds in index order, so with the edge ends interleaved
(a0, b0, a1, b1, ...) a node's sum runs over its internal edges in the level's original edge order, from +0.0.

    root6(t)   s = sqrt(t);  y = from_bits(int64_bits(s) // 3 + 0x2A9F7893782DA1CE);  four times: y3 = (y*y)*y; y = y * ((y3 + (s + s)) / ((y3 + y3) + s))
    pass 1     G of (u, v, w, nt) as §13 forms G;  om = |curl v|;  nu = mu_i / rho;  chi = nt / nu;  fv1 = chi3 / (chi3 + cv1_3)
               mut = (rho * nt) * fv1 -> eddy_viscosity;  sa_gradient = (G[nt], om, nu)
    pass 2     per edge Qc += min(phi, 0) * (nt_i - nt_j), Qd += nb * (grad_bar . n); per node the source, the point-implicit
               destruction, the capped step; nt_out = max(nt_old + dn, +0.0); +0.0 where d == 0.0
    coarse     nt_I = (sum of the children's nt in ascending fine id) * (1 / count);  mut_I = (rho_I * nt_I) * fv1

The model is the viscosity model's eddy mode 1 to everything that reads ``eddy_viscosity`` (the stress pass, the wall stresses, the
step limit): ``SaOracle`` keeps ``model.eddy == 1`` and writes ``self.mut`` itself.  ``transport`` also reports which branches of
the definition each node took; tests/test_host_sa.py counts them.

The parameters of the GPU runs (tests/test_gpu_sa.py), which tests/test_host_sa.py keeps valid on the CPU, are at the end.
"""
import numpy as np

import cycle_emulator as ce
import time_step_emulator as tse
import variable_viscosity_emulator as vve
import viscous_emulator as ve
import wall_distance_emulator as wde

RK = ve.RK
CB1, CB2, SIGMA, KAPPA = np.float64(0.1355), np.float64(0.622), np.float64(2.0 / 3.0), np.float64(0.41)
CW2, CW3, CV1, CV2, CV3, RLIM = np.float64(0.3), np.float64(2.0), np.float64(7.1), np.float64(0.7), np.float64(0.9), np.float64(10.0)
CW1 = CB1 / (KAPPA * KAPPA) + (1.0 + CB2) / SIGMA
CV1_3 = (CV1 * CV1) * CV1
C6 = np.float64(64.0)
INV_SIGMA = 1.0 / SIGMA
KS = (1.0 + CB2) / SIGMA
SA_RATIO = 3.0
SA = "spalart-allmaras"
EDDY_SA = 4                          # MGCFD_EDDY_SPALART_ALLMARAS (3 stays an unknown mode)
ARR_SA_NU_TILDE, ARR_SA_GRADIENT = 17, 18
BRANCHES = ("s_tilde_second", "r_capped", "jac_clamped", "cap_binds", "clipped", "wall")


def root6(t):
    """The definition's sixth root of t > 0."""
    s = np.sqrt(np.asarray(t, dtype=np.float64))
    y = (s.view(np.int64) // 3 + np.int64(0x2A9F7893782DA1CE)).view(np.float64)
    for _ in range(4):
        y3 = (y * y) * y
        y = y * ((y3 + (s + s)) / ((y3 + y3) + s))
    return y


def fv1(chi):
    chi3 = (chi * chi) * chi
    return chi3 / (chi3 + CV1_3)


def fv2(chi):
    return 1.0 - chi / (1.0 + chi * fv1(chi))


def s_tilde(om, sb):
    """The 2012 limiter: om + sb where sb >= -cv2 om, the rational branch below."""
    with np.errstate(all="ignore"):
        second = om + (om * ((CV2 * CV2) * om + CV3 * sb)) / ((CV3 - 2.0 * CV2) * om - sb)
        return np.where(sb >= -(CV2 * om), om + sb, second)


def fw(r):
    r2 = r * r
    r6 = (r2 * r2) * r2
    g = r + CW2 * (r6 - r)
    g2 = g * g
    g6 = (g2 * g2) * g2
    return g * root6((1.0 + C6) / (g6 + C6))


def velocities(W):
    q = np.asarray(W, dtype=np.float64).reshape(-1, 5)
    rho = q[:, 0]
    return np.stack([q[:, 1] / rho, q[:, 2] / rho, q[:, 3] / rho], axis=1)


def node_viscosity(W, mu, model):
    """nu_i [nel] and rho_i: mu_i by the law of §16 from T = p / rho."""
    q = np.asarray(W, dtype=np.float64).reshape(-1, 5)
    rho = q[:, 0]
    mu_i = vve.viscosity(model, mu, ve.jse.pressure(q) / rho)
    return mu_i / rho, rho


def eddy_viscosity(W, nt, mu, model):
    """mut = (rho * nt) * fv1, the expression pass 1, the coarse levels and the start value share."""
    with np.errstate(all="ignore"):
        nu, rho = node_viscosity(W, mu, model)
        return (rho * nt) * fv1(nt / nu)


def gradient(W, nt, to, frm, N, vol, mu, model):
    """Pass 1: (sa_gradient [nel, 5], mut [nel])."""
    with np.errstate(all="ignore"):
        phi = np.concatenate([velocities(W), np.asarray(nt, dtype=np.float64)[:, None]], axis=1)
        G = ve.gradients(phi, to, frm, N, vol)
        ox = G[:, 2, 1] - G[:, 1, 2]
        oy = G[:, 0, 2] - G[:, 2, 0]
        oz = G[:, 1, 0] - G[:, 0, 1]
        om = np.sqrt((ox * ox + oy * oy) + oz * oz)
        nu, rho = node_viscosity(W, mu, model)
        mut = (rho * nt) * fv1(nt / nu)
        return np.stack([G[:, 3, 0], G[:, 3, 1], G[:, 3, 2], om, nu], axis=1), mut


def edge_sums(W, nt, grad, to, frm, N):
    """Pass 2's (Qc, Qd) [nel] each."""
    with np.errstate(all="ignore"):
        v = velocities(W)
        nu = grad[:, 4]
        nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
        b = 0.5 * (v[to] + v[frm])
        phi = (b[:, 0] * nx + b[:, 1] * ny) + b[:, 2] * nz
        pm = np.where(phi < 0.0, phi, 0.0)
        nb = 0.5 * ((nu[to] + nt[to]) + (nu[frm] + nt[frm]))
        gb = 0.5 * (grad[to, 0:3] + grad[frm, 0:3])
        Qc, Qd = np.zeros(len(nt)), np.zeros(len(nt))
        np.add.at(Qc, to, pm * (nt[to] - nt[frm]))
        np.add.at(Qd, to, nb * ((gb[:, 0] * nx + gb[:, 1] * ny) + gb[:, 2] * nz))
    return Qc, Qd


def node_source(nt, nu, om, gg, d):
    """(src, st, fw, r-capped mask, second-branch mask) of the node terms."""
    with np.errstate(all="ignore"):
        chi = nt / nu
        kd2 = (KAPPA * d) * (KAPPA * d)
        sb = (nt * fv2(chi)) / kd2
        st = s_tilde(om, sb)
        den = st * kd2
        ok = (den > 0.0) & (nt < RLIM * den)
        r = np.where(ok, nt / den, RLIM)
        f = fw(r)
        nd = nt / d
        src = ((CB1 * st) * nt - (CW1 * f) * (nd * nd)) + (CB2 * INV_SIGMA) * gg
    return src, st, f, ~ok, ~(sb >= -(CV2 * om))


def transport(W, nt, nt_old, grad, to, frm, N, vol, d, g, sf, cfl_v, j):
    """Pass 2 of stage j: (nt_out [nel], {branch: mask [nel]}); the masks cover non-wall nodes, ``wall`` the others."""
    with np.errstate(all="ignore"):
        nt = np.asarray(nt, dtype=np.float64)
        Qc, Qd = edge_sums(W, nt, grad, to, frm, N)
        nu, om = grad[:, 4], grad[:, 3]
        gg = (grad[:, 0] * grad[:, 0] + grad[:, 1] * grad[:, 1]) + grad[:, 2] * grad[:, 2]
        src, st, f, capped, second = node_source(nt, nu, om, gg, d)
        Q = (Qc + INV_SIGMA * Qd) + vol * src
        jac = ((2.0 * CW1) * f) * (nt / (d * d)) - CB1 * st
        clamped = ~(jac > 0.0)
        jac = np.where(jac > 0.0, jac, 0.0)
        cap = (np.float64(cfl_v) * g) / (KS * (nu + nt))
        binds = cap < sf
        sft = np.where(binds, cap, sf)
        fac = sft / np.float64(RK + 1 - j)
        dn = (fac * Q) / (1.0 + (fac * vol) * jac)
        x = nt_old + dn
        clipped = x < 0.0
        out = np.where(clipped, 0.0, x)
        wall = d == 0.0
        out = np.where(wall, 0.0, out)
        free = ~wall
    return out, {"s_tilde_second": second & free, "r_capped": capped & free, "jac_clamped": clamped & free, "cap_binds": binds & free,
                 "clipped": clipped & free, "wall": wall}


def restrict(nt_fine, nt_coarse, parent):
    """nt of the coarse level behind a restriction: the children's average, a node without children keeps its value."""
    parent = np.asarray(parent, dtype=np.int64)
    s = np.zeros(len(nt_coarse))
    np.add.at(s, parent, nt_fine)
    count = np.bincount(parent, minlength=len(nt_coarse))
    with np.errstate(all="ignore"):
        avg = s * (1.0 / count.astype(np.float64))
    return np.where(count > 0, avg, nt_coarse)


def start_value(ratio, mu, rho_inf, d):
    """nt at enable: (ratio * mu) / rho_inf, +0.0 where d == 0.0."""
    return np.where(np.asarray(d) == 0.0, 0.0, (np.float64(ratio) * np.float64(mu)) / np.float64(rho_inf))


class _SaLib:
    """The oracle library behind ViscousOracle's wrapper, with the model's restriction behind mg_restrict (and its wall rule)."""

    def __init__(self, lib, owner):
        self._lib, self._owner = lib, owner

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def ora_mg_restrict(self, fine, coarse, *rest):
        rc = self._lib.ora_mg_restrict(fine, coarse, *rest)
        em = self._owner
        for l in range(1, em.n):
            if em.oc.levels[l].variables == coarse and em.sa_on(l):
                em.sa_restrict(l)
        return rc


class SaOracle(wde.WallDampedOracle, ce.CycleOracle):
    """WallDampedOracle (and CycleOracle's cycle control) with the Spalart-Allmaras eddy mode."""

    def __init__(self, *args, **kwargs):
        self.sa, self.eddy_id, self.sa_ratio, self.nt = False, 0, SA_RATIO, None
        super().__init__(*args, **kwargs)
        self.nt = [None] * self.n
        self.nt_old, self.sa_grad = None, None
        self.branches = {k: 0 for k in BRANCHES}
        self.max_move = 0.0                                   # the largest relative change of nt at a non-wall node of level 0 in a stage
        self.lib = _SaLib(self.lib, self)

    # ---- the setting ----
    def sa_on(self, l):
        return self.sa and self.viscous_on(l)

    def _form_mut(self, l):
        self.mut[l][:] = eddy_viscosity(self._var(l), self.nt[l], self.mu, self.model)

    def _initialise(self, l):
        self.nt[l] = start_value(self.sa_ratio, self.mu, self.ff17[0], self.wall_distance(l)[0])
        self._form_mut(l)
        if l == 0:
            self.nt_old = self.nt[0].copy()

    def _settle_sa(self, everything):
        if self.nt is None:
            return
        for l in range(self.n):
            if not self.sa_on(l):
                self.nt[l] = None
            elif self.nt[l] is None or everything:
                self._initialise(l)

    def set_viscous(self, *args, **kwargs):
        super().set_viscous(*args, **kwargs)
        self._settle_sa(False)

    def set_viscosity_model(self, law="constant", t_ref=None, s=vve.SUTHERLAND_S, eddy="none", cs=vve.SMAGORINSKY_CS, prandtl_t=vve.PRANDTL_TURBULENT):
        sa = eddy in (SA, EDDY_SA)
        new_id = EDDY_SA if sa else vve.EDDIES.get(eddy, eddy)
        assert not sa or self.dt == 0.0
        changed = new_id != self.eddy_id
        self.sa, self.eddy_id = sa, new_id
        super().set_viscosity_model(law, t_ref, s, "field" if sa else eddy, cs, prandtl_t)
        if changed:
            for l in range(self.n):
                self.mut[l][:] = 0.0
        self._settle_sa(changed)

    def set_dual_time(self, dt, *args, **kwargs):
        assert not (self.sa and dt != 0.0)
        super().set_dual_time(dt, *args, **kwargs)

    def set_far_field(self, ff17, reinitialise):
        super().set_far_field(ff17, reinitialise)
        if reinitialise and self.nt is not None:
            for l in range(self.n):
                if self.sa_on(l):
                    self._initialise(l)

    def set_sa_free_stream(self, ratio=SA_RATIO, reinitialise=False):
        assert np.isfinite(ratio) and ratio > 0.0
        self.sa_ratio = float(ratio)
        if reinitialise:
            for l in range(self.n):
                if self.sa_on(l):
                    self._initialise(l)

    def nu_tilde(self, l):
        assert self.sa_on(l)
        return self.nt[l].copy()

    def set_nu_tilde(self, l, values):
        """A write of MGCFD_ARR_SA_NU_TILDE: mut is formed again from the new nt and the level's state."""
        assert self.sa_on(l)
        self.nt[l] = np.array(values, dtype=np.float64).ravel().copy()
        self._form_mut(l)

    def copy_old(self):
        """mgcfd_copy_old_variables on level 0: nt_old beside old_variables."""
        self.oc.array(0, "old_variables")[:] = self.oc.array(0, "variables")
        self.nt_old = self.nt[0].copy()

    # ---- the hooks ----
    def add_viscous_flux(self, l):
        if l == 0 and self.sa_on(0):
            self.sa_grad, mut = gradient(self._var(0), self.nt[0], self.vto[0], self.vfrm[0], self.vN[0], self.oc.array(0, "volumes"),
                                         self.mu, self.model)
            self.mut[0][:] = mut
        super().add_viscous_flux(l)

    def sa_restrict(self, l):
        self.nt[l] = restrict(self.nt[l - 1], self.nt[l], self.oc.mg_map(l - 1))
        self._form_mut(l)

    def sa_transport(self, j, sf):
        """Pass 2 of stage j on level 0, from the state the stage's fluxes were computed from."""
        out, masks = transport(self._var(0), self.nt[0], self.nt_old, self.sa_grad, self.vto[0], self.vfrm[0], self.vN[0],
                               self.oc.array(0, "volumes"), self.wall_distance(0)[0], self.g[0], sf, self.cfl_v, j)
        for k in BRANCHES:
            self.branches[k] += int(masks[k].sum())
        free = ~masks["wall"] & (self.nt[0] > 0.0)
        if free.any():
            with np.errstate(all="ignore"):
                self.max_move = max(self.max_move, float(np.nanmax(np.abs(out[free] - self.nt[0][free]) / self.nt[0][free])))
        self.nt[0] = out

    def _sweep(self, l):
        if l != 0 or not self.sa_on(0):
            return super()._sweep(l)
        # ViscousOracle._sweep of level 0 with nt_old beside old_variables and pass 2 before every update
        import ctypes as C
        self.work += 1.0
        lib, L = self.lib, self.oc.levels[0]
        C.memmove(L.old_variables, L.variables, 8 * L.nel * 5)
        self.nt_old = self.nt[0].copy()
        sf = self.oc.array(0, "step_factors")
        sf[:] = self.final_step_factors(0)
        if self.on_step_factors:
            self.on_step_factors(0, sf)
        fluxes = self.oc.array(0, "fluxes").reshape(-1, 5)
        old = self.oc.array(0, "old_variables").reshape(-1, 5)
        var = self._var(0)
        for j in range(RK):
            lib.ora_compute_flux_edge(L.internal_start, L.n_internal, L.edges, L.variables, L.fluxes)
            lib.ora_compute_boundary_flux_edge(L.boundary_start, L.n_boundary, L.edges, L.variables, L.fluxes)
            lib.ora_compute_wall_flux_edge(L.wall_start, L.n_wall, L.edges, L.variables, L.fluxes, C.byref(self.ff))     # (+ C, pass 1, + V)
            self.sa_transport(j, sf.copy())
            if not self.iterations:
                lib.ora_time_step(j, L.nel, L.step_factors, L.fluxes, L.old_variables, L.variables)
            else:
                fp = fluxes.copy()
                var[:] = old + self.smoothed_update(0, sf, fp) / np.float64(RK + 1 - j)
                fluxes[:] = 0.0
            rc = lib.ora_check_for_invalid_variables(L.variables, L.nel, None)          # (then the wall rule: the wrapper)
            if rc:
                return rc
        lib.ora_residual(L.nel, L.old_variables, L.variables, L.residuals)
        return 0

    # ---- mgcfd_compute_fluxes then mgcfd_time_step(0, j), from fluxes of +0.0 ----
    def kernel_level(self, j, sf):
        """(sa_gradient, mut, S, F + V, nt_out, masks) of level 0's current state, nt and nt_old, with step factors ``sf``."""
        f = self.stage_fluxes(0)
        grad, mut, S = self.sa_grad.copy(), self.mut[0].copy(), self.last_S[0].copy()
        out, masks = transport(self._var(0), self.nt[0], self.nt_old, self.sa_grad, self.vto[0], self.vfrm[0], self.vN[0],
                               self.oc.array(0, "volumes"), self.wall_distance(0)[0], self.g[0], sf, self.cfl_v, j)
        return grad, mut, S, f, out, masks


# ---- what the GPU tests run ----
GPU_CYCLES = ve.GPU_CYCLES
MODELS = (("constant", SA), ("sutherland", SA))
RUN_CASES = ("A", "B", "tet_2lvl")
RUN_MU = {"A": ve.CELL_RE_MU, "B": ve.CELL_RE_MU, "tet_2lvl": ve.GPU_MU["tet_2lvl"]}
RUN_STEP = ("local", 1.0)
NT_SEED = 23
NT_MAX = 10.0                        # the kernel-level nt: uniform in [0, NT_MAX * nu_inf], as §16's eddy_field is seeded
# (name, (eps, iterations), JST levels, FAS, cycle shape) on lattice A, all levels, no-slip walls, (sutherland, SA)
COMPOSED = (("smoothing", (0.5, 2), 0, False, "V"), ("jst", (0.0, 0), 1, False, "V"), ("fas", (0.0, 0), 0, True, "V"),
            ("w_cycle", (0.0, 0), 0, False, "W"), ("all", (0.5, 2), 1, True, "W"))


def gpu_runs():
    """(case key, mu, mode, cfl, wall, levels, model) of the bit-for-bit runs."""
    return [(case, RUN_MU[case]) + RUN_STEP + (wall, lv, m) for case in RUN_CASES for m in MODELS for wall in ve.GPU_WALLS for lv in ve.GPU_LEVELS]


def random_nt(mu, rho_inf, nel, seed=NT_SEED):
    return (np.float64(mu) / np.float64(rho_inf)) * np.random.default_rng(seed).uniform(0.0, NT_MAX, nel)


def kernel_level_case(oracle, case, mu, cfl, start):
    """The kernel-level case of tests/test_gpu_sa.py on the emulator: the state ``start``, no-slip walls, (sutherland, SA) on level
    0; nt_old = a random nt (seed NT_SEED + 1) through copy_old, nt = another (seed NT_SEED); the step factors of that state; then
    mgcfd_compute_fluxes and mgcfd_time_step(0, 0).  (the emulator, nt_old, nt, sf, kernel_level's tuple)."""
    em = SaOracle(oracle, case, "local", cfl)
    v = em._var(0)
    v[:] = start
    em.set_viscous(mu, ve.PRANDTL, 1, ve.VISCOUS_CFL, 1)
    em.set_viscosity_model(law="sutherland", eddy=SA)
    old, new = random_nt(mu, em.ff17[0], len(v), NT_SEED + 1), random_nt(mu, em.ff17[0], len(v))
    em.set_nu_tilde(0, old)
    em.copy_old()
    em.set_nu_tilde(0, new)
    sf = em.final_step_factors(0)
    return em, old, new, sf, em.kernel_level(0, sf)


def configured(oracle, case, mu, mode, cfl, wall, levels, model, smoothing=(0.0, 0), jst_levels=0, fas=False, shape="V"):
    """The emulator as tests/test_gpu_sa.py configures the solver: the start state, the terms switched on, then the model."""
    em = SaOracle(oracle, case, mode, cfl, *smoothing, kappa2=ve.jse.KAPPA2 if jst_levels else 0.0,
                  kappa4=ve.jse.KAPPA4 if jst_levels else 0.0, levels=jst_levels, fas=fas)
    if shape != "V":
        em.set_cycle(shape)
    v = em._var(0)
    v[:] = ve.start_state(len(v), em.ff17[:5])
    em.set_viscous(mu, ve.PRANDTL, wall, ve.VISCOUS_CFL, levels)
    em.set_viscosity_model(law=model[0], eddy=model[1])
    return em
