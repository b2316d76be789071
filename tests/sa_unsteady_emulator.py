"""The yardstick of the unsteady Spalart-Allmaras model (mgcfd_set_sa_unsteady): ``SaUnsteadyOracle``, tests/sa_emulator.py's
``SaOracle`` (through tests/face_gradient_emulator.py's ``FaceGradientOracle``, so that the wall thermal conditions and the
corrected face gradient compose) with the definition of INTEGRATION.md §21 written in numpy, line by line.  Every numpy operation
is one IEEE-754 double operation per element.

    time levels  ntn, ntn1 on level 0 while the model, dual time and time_accurate are all in effect: both = nt when the
                 combination takes effect, on reset and on a reinitialising free stream; begin_step shifts them beside the state's
                 and forms mut of every covered level again from nt and the state, as a write of nt does
    pass 2       a = nt - ntn;  b = ntn - ntn1;  ts = (3.0 * a - b) / (2.0 * dt) (order 2) or a / dt (order 1)
                 Q' = Q - vol * ts;  dn = (fac * Q') / (1.0 + (fac * vol) * (jac + cj)),  cj = 1.5 / dt or 1.0 / dt
    delta        the longest internal edge at the node, sqrt((dx*dx + dy*dy) + dz*dz); +inf at a node without one
    DES97        d == 0.0: +0.0;  d <= lim: d;  otherwise lim          (lim = c_des * delta)
    delayed DES  pass 1 writes d == 0.0: +0.0;  d == +inf: lim;  d <= lim: d;  otherwise d - fd * (d - lim),  fd = 1.0 - tanh_fixed(z)

``transport`` reports which branches each node took; tests/test_host_sa_unsteady.py counts them.
"""
import ctypes as C

import numpy as np

import face_gradient_emulator as fge
import sa_emulator as sae
import viscous_emulator as ve
import wall_heat_emulator as whe

RK = ve.RK
SA_CDES = 0.65
WALL, DES, DDES = 0, 1, 2
LENGTHS = {"wall": WALL, "des": DES, "ddes": DDES}
ARR_SA_TIME_N, ARR_SA_TIME_N1, ARR_SA_LENGTH = 20, 21, 22
BRANCHES = ("bdf1", "bdf2", "d_le_lim", "blend", "fd_zero", "fd_one", "d_inf", "wall")
FACTORIALS = (1.0, 1.0, 2.0, 6.0, 24.0, 120.0, 720.0, 5040.0, 40320.0)


def tanh_fixed(z):
    """The definition's tanh of z in [0, 20]: exp(z / 512) by its Taylor polynomial of degree 8, squared ten times."""
    z = np.asarray(z, dtype=np.float64)
    q = z * np.float64(1.0 / 512.0)
    p = np.full(z.shape, np.float64(1.0) / np.float64(FACTORIALS[8]))
    for k in range(7, 0, -1):
        p = np.float64(1.0) / np.float64(FACTORIALS[k]) + q * p
    p = 1.0 + q * p
    for _ in range(10):
        p = p * p
    return (p - 1.0) / (p + 1.0)


def time_source(nt, ntn, ntn1, dt, order):
    """(ts [nel], cj): the differences first, so nt == ntn == ntn1 gives +0.0."""
    dt = np.float64(dt)
    a = nt - ntn
    if order == 1:
        return a / dt, np.float64(1.0) / dt
    b = ntn - ntn1
    return (3.0 * a - b) / (2.0 * dt), np.float64(1.5) / dt


def edge_lengths(X, a, b):
    d = X[b] - X[a]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def delta_of(X, a, b):
    """The longest internal edge at every node; +inf where there is none."""
    L = edge_lengths(X, a, b)
    longest = np.full(len(X), -1.0)
    np.maximum.at(longest, a, L)
    np.maximum.at(longest, b, L)
    return np.where(longest >= 0.0, longest, np.inf)


def des_length(d, lim):
    with np.errstate(all="ignore"):
        return np.where(d == 0.0, 0.0, np.where(d <= lim, d, lim))


def shield(G, nt, nu, d):
    """(fd, z) of delayed DES from the nine velocity gradients G [nel, 3, 3], nt, nu and the wall distance."""
    with np.errstate(all="ignore"):
        f1 = sae.fv1(nt / nu)
        s = [(G[:, k, 0] * G[:, k, 0] + G[:, k, 1] * G[:, k, 1]) + G[:, k, 2] * G[:, k, 2] for k in range(3)]
        sq = np.sqrt((s[0] + s[1]) + s[2])
        kd = sae.KAPPA * d
        kd2 = kd * kd
        rd = (nt * f1 + nu) / (sq * kd2)
        e = 8.0 * rd
        z = (e * e) * e
        z = np.where(z < 20.0, z, 20.0)
        return 1.0 - tanh_fixed(z), z


def ddes_length(d, lim, fd):
    """(d~, {branch: mask})."""
    with np.errstate(all="ignore"):
        wall, inf = d == 0.0, np.isposinf(d)
        le = ~wall & ~inf & (d <= lim)
        rest = ~wall & ~inf & ~le
        out = np.where(wall, 0.0, np.where(inf, lim, np.where(le, d, d - fd * (d - lim))))
    return out, {"d_le_lim": le, "blend": rest & (fd > 0.0) & (fd < 1.0), "fd_zero": rest & (fd == 0.0), "fd_one": rest & (fd == 1.0),
                 "d_inf": inf, "wall": wall}


def transport(W, nt, nt_old, grad, to, frm, N, vol, d, g, sf, cfl_v, j, time=None, X=None):
    """Pass 2 of stage j with the model length ``d`` and, with ``time = (ntn, ntn1, dt, order)``, the physical-time source;
    ``X``: the coordinates under the corrected face gradient.  sae.transport's lines, Q' and cj added."""
    with np.errstate(all="ignore"):
        nt = np.asarray(nt, dtype=np.float64)
        Qc, Qd = sae.edge_sums(W, nt, grad, to, frm, N)
        if X is not None:
            Qd = Qd + fge.sa_qdc(nt, grad, X, to, frm, N)
        nu, om = grad[:, 4], grad[:, 3]
        gg = (grad[:, 0] * grad[:, 0] + grad[:, 1] * grad[:, 1]) + grad[:, 2] * grad[:, 2]
        src, st, f, _, _ = sae.node_source(nt, nu, om, gg, d)
        Q = (Qc + sae.INV_SIGMA * Qd) + vol * src
        jac = ((2.0 * sae.CW1) * f) * (nt / (d * d)) - sae.CB1 * st
        jac = np.where(jac > 0.0, jac, 0.0)
        cap = (np.float64(cfl_v) * g) / (sae.KS * (nu + nt))
        sft = np.where(cap < sf, cap, sf)
        fac = sft / np.float64(RK + 1 - j)
        if time is None:
            dn = (fac * Q) / (1.0 + (fac * vol) * jac)
        else:
            ntn, ntn1, dt, order = time
            ts, cj = time_source(nt, ntn, ntn1, dt, order)
            Qt = Q - vol * ts
            dn = (fac * Qt) / (1.0 + (fac * vol) * (jac + cj))
        x = nt_old + dn
        out = np.where(x < 0.0, 0.0, x)
        return np.where(d == 0.0, 0.0, out)


class SaUnsteadyOracle(fge.FaceGradientOracle):
    """SaOracle (with the wall thermal conditions and the face gradient) and the setting of mgcfd_set_sa_unsteady."""

    def __init__(self, *args, **kwargs):
        self.time_accurate, self.length, self.c_des = False, WALL, np.float64(SA_CDES)
        self.ntn, self.ntn1, self.delta, self.sa_len = None, None, None, None
        self.ubranches = {k: 0 for k in BRANCHES}
        self._ready = False
        super().__init__(*args, **kwargs)
        self._ready = True
        self._settle_unsteady()

    # ---- the setting ----
    def sa_timed(self):
        return bool(self.time_accurate) and self.dt > 0.0 and self.sa_on(0)

    def _settle_unsteady(self, length_changed=False):
        if not self._ready or self.nt is None:
            return
        if not self.sa_timed():
            self.ntn, self.ntn1 = None, None
        elif self.ntn is None:
            self.ntn, self.ntn1 = self.nt[0].copy(), self.nt[0].copy()
        if self.length == WALL or not self.sa_on(0):
            self.delta, self.sa_len = None, None
        elif self.sa_len is None or length_changed:
            if self.delta is None:
                self.delta = delta_of(self.oc.array(0, "coords").reshape(-1, 3), self.ea[0], self.eb[0])
            self.sa_len = des_length(self.wall_distance(0)[0], self.c_des * self.delta)

    def set_sa_unsteady(self, time_accurate=False, length="wall", c_des=SA_CDES):
        length = LENGTHS.get(length, length)
        assert length in (WALL, DES, DDES) and np.isfinite(c_des) and c_des > 0.0
        assert time_accurate or not (self.dt > 0.0 and self.sa_on(0))
        changed = length != self.length or np.float64(c_des) != self.c_des
        self.time_accurate, self.length, self.c_des = bool(time_accurate), length, np.float64(c_des)
        self._settle_unsteady(changed)

    def set_dual_time(self, dt, *args, **kwargs):
        assert self.time_accurate or not (self.sa and dt != 0.0)
        super(sae.SaOracle, self).set_dual_time(dt, *args, **kwargs)          # (past SaOracle's assertion)
        self._settle_unsteady()

    def set_viscosity_model(self, law="constant", t_ref=None, s=sae.vve.SUTHERLAND_S, eddy="none", cs=sae.vve.SMAGORINSKY_CS,
                            prandtl_t=sae.vve.PRANDTL_TURBULENT):
        dt = self.dt
        if self.time_accurate:
            self.dt = 0.0                                                      # (SaOracle asserts the old refusal)
        try:
            super().set_viscosity_model(law, t_ref, s, eddy, cs, prandtl_t)
        finally:
            self.dt = dt
        self._settle_unsteady()

    def set_viscous(self, *args, **kwargs):
        super().set_viscous(*args, **kwargs)
        self._settle_unsteady()

    def set_far_field(self, ff17, reinitialise):
        super().set_far_field(ff17, reinitialise)
        if reinitialise and self.ntn is not None:
            self.ntn, self.ntn1 = self.nt[0].copy(), self.nt[0].copy()

    def reset(self):
        super().reset()
        if self.ntn is not None:
            self.ntn, self.ntn1 = self.nt[0].copy(), self.nt[0].copy()

    def begin_step(self):
        first = self.levels == 0
        super().begin_step()
        if self.ntn is not None:
            now = self.nt[0].copy()
            self.ntn, self.ntn1 = now, (now.copy() if first else self.ntn)
            for l in range(self.n):                       # mut as a write of nt forms it: the step is a function of the six arrays
                if self.sa_on(l):
                    self._form_mut(l)

    def set_nt_time_levels(self, ntn=None, ntn1=None):
        """mgcfd_set_array on MGCFD_ARR_SA_TIME_N / _SA_TIME_N1: a level written is a level held."""
        assert self.ntn is not None
        if ntn is not None:
            self.ntn = np.array(ntn, dtype=np.float64).ravel().copy()
            self.levels = max(self.levels, 1)
        if ntn1 is not None:
            self.ntn1 = np.array(ntn1, dtype=np.float64).ravel().copy()
            self.levels = 2

    def model_length(self):
        """MGCFD_ARR_SA_LENGTH."""
        assert self.sa_len is not None
        return self.sa_len.copy()

    def _d(self):
        return self.wall_distance(0)[0] if self.sa_len is None else self.sa_len

    # ---- the hooks ----
    def add_viscous_flux(self, l):
        super().add_viscous_flux(l)
        if l == 0 and self.sa_on(0) and self.length == DDES:
            G = ve.gradients(sae.velocities(self._var(0)), self.vto[0], self.vfrm[0], self.vN[0], self.oc.array(0, "volumes"))
            d = self.wall_distance(0)[0]
            fd, _ = shield(G, self.nt[0], self.sa_grad[:, 4], d)
            self.sa_len, masks = ddes_length(d, self.c_des * self.delta, fd)
            for k, m in masks.items():
                self.ubranches[k] += int(m.sum())

    def _transport(self, j, sf):
        time = None
        if self.ntn is not None:
            order = self.effective_order()
            time = (self.ntn, self.ntn1, self.dt, order)
            self.ubranches["bdf%d" % order] += len(self.ntn)
        return transport(self._var(0), self.nt[0], self.nt_old, self.sa_grad, self.vto[0], self.vfrm[0], self.vN[0],
                         self.oc.array(0, "volumes"), self._d(), self.g[0], sf, self.cfl_v, j, time, self.X[0] if self.fg_on(0) else None)

    def sa_transport(self, j, sf):
        self.nt[0] = self._transport(j, sf)

    def kernel_level(self, j, sf):
        """(sa_gradient, mut, S, F + V, d~ or None, nt_out) of level 0's current state, nt and nt_old, with step factors ``sf``."""
        f = self.stage_fluxes(0)
        grad, mut, S = self.sa_grad.copy(), self.mut[0].copy(), self.last_S[0].copy()
        length = None if self.sa_len is None else self.sa_len.copy()
        return grad, mut, S, f, length, self._transport(j, sf)

    def _sweep(self, l):
        if l != 0 or not self.sa_on(0) or self.dt == 0.0:
            return super()._sweep(l)
        # SaOracle._sweep of level 0 with the physical-time source of the five variables, as ViscousOracle._sweep takes it
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
            fp = fluxes - self.stage_source(0, var)
            if self.iterations:
                var[:] = old + self.smoothed_update(0, sf, fp) / np.float64(RK + 1 - j)
            else:
                factor = sf / np.float64(RK + 1 - j)
                var[:] = old + factor[:, None] * fp
            fluxes[:] = 0.0
            rc = lib.ora_check_for_invalid_variables(L.variables, L.nel, None)          # (then the wall rule: the wrapper)
            if rc:
                return rc
        lib.ora_residual(L.nel, L.old_variables, L.variables, L.residuals)
        return 0


# ---- what the GPU tests run (tests/test_gpu_sa_unsteady.py), which tests/test_host_sa_unsteady.py keeps valid on the CPU ----
RUN_CASES = sae.RUN_CASES
RUN_MU = sae.RUN_MU
MODEL = sae.MODELS[1]                     # (sutherland, SA)
RUN_LENGTHS = ("wall", "des", "ddes")
DUAL_STEPS, DUAL_CYCLES = ve.DUAL_STEPS + 1, ve.DUAL_CYCLES
# the physical step of the runs: the largest of (0.2, 0.1, 0.05, 0.02) at which every run below stays valid on the CPU (under DES97
# the smaller eddy viscosity leaves lattice B at 0.05 in the third step; tests/test_host_sa_unsteady.py keeps the choice valid)
DUAL_DT = 0.02
KERNEL_CDES = 2.0                         # the kernel-level case at which the first layer of a uniform lattice has d <= lim
TIME_SEED = 31


def configured(oracle, case, mu, length="wall", time_accurate=True, dt=DUAL_DT, c_des=SA_CDES, smoothing=(0.0, 0), jst_levels=0, fas=False,
               shape="V", face_gradient=None, tw_ratio=None, cfl=1.0):
    """The emulator as tests/test_gpu_sa_unsteady.py configures the solver: local steps, the start state, no-slip walls on all
    levels (``tw_ratio``: isothermal at that multiple of the free-stream temperature), (sutherland, SA), the setting, then dual
    time (dt = 0: off)."""
    em = SaUnsteadyOracle(oracle, case, "local", cfl, *smoothing, kappa2=ve.jse.KAPPA2 if jst_levels else 0.0,
                          kappa4=ve.jse.KAPPA4 if jst_levels else 0.0, levels=jst_levels, fas=fas)
    if shape != "V":
        em.set_cycle(shape)
    v = em._var(0)
    v[:] = ve.start_state(len(v), em.ff17[:5])
    if face_gradient:
        em.set_face_gradient(face_gradient)
    em.set_viscous(mu, ve.PRANDTL, 1, ve.VISCOUS_CFL, "all")
    if tw_ratio:
        em.set_wall_temperature(whe.ISOTHERMAL, whe.setting_value(em.ff17, whe.ISOTHERMAL, tw_ratio))
    em.set_viscosity_model(law=MODEL[0], eddy=MODEL[1])
    em.set_sa_unsteady(time_accurate, length, c_des)
    if dt:
        em.set_dual_time(dt)
    return em


def random_levels(em, seed=TIME_SEED):
    """Seeded random ntn and ntn1 of the kernel-level cases: nt scaled by factors in [0.5, 1.5], +0.0 kept on the wall."""
    rng = np.random.default_rng(seed)
    nt = em.nt[0]
    return nt * rng.uniform(0.5, 1.5, len(nt)), nt * rng.uniform(0.5, 1.5, len(nt))


def kernel_variants(name):
    """(length, c_des, BDF order, corrected face gradient, mu or None for the case's own) of the kernel-level runs of case ``name``
    (tests/test_gpu_sa.py's six): delayed DES under BDF2 and DES97 under BDF1 everywhere; on lattice A also c_des = KERNEL_CDES (the
    first layer then has d <= lim), with and without the corrected face gradient; on the tetrahedral level also a viscosity so small
    that rd underflows the shielding (fd = 1)."""
    out = [("ddes", SA_CDES, 2, False, None), ("des", SA_CDES, 1, False, None)]
    if name == "lattice_A":
        out += [("ddes", KERNEL_CDES, 2, True, None), ("ddes", KERNEL_CDES, 1, False, None), ("wall", SA_CDES, 2, True, None)]
    if name == "tet":
        out += [("ddes", SA_CDES, 2, False, 1e-12)]
    return out


def kernel_level_case(oracle, case, mu, cfl, start, length="wall", c_des=SA_CDES, order=None, corrected=False, dt=DUAL_DT):
    """The kernel-level case of tests/test_gpu_sa_unsteady.py on the emulator: sae.kernel_level_case's state and nt on level 0 with
    the setting; ``order`` 1 or 2: dual time on with seeded random time levels of nt (order 1: ntn alone is written, so one level is
    held and BDF1 runs); then mgcfd_compute_fluxes and mgcfd_time_step(0, 0).
    (the emulator, nt_old, nt, (ntn, ntn1) or None, sf, kernel_level's tuple)."""
    em = SaUnsteadyOracle(oracle, case, "local", cfl)
    v = em._var(0)
    v[:] = start
    if corrected:
        em.set_face_gradient("corrected")
    em.set_viscous(mu, ve.PRANDTL, 1, ve.VISCOUS_CFL, 1)
    em.set_viscosity_model(law="sutherland", eddy=sae.SA)
    em.set_sa_unsteady(order is not None, length, c_des)
    old, new = sae.random_nt(mu, em.ff17[0], len(v), sae.NT_SEED + 1), sae.random_nt(mu, em.ff17[0], len(v))
    em.set_nu_tilde(0, old)
    em.copy_old()
    em.set_nu_tilde(0, new)
    levels = None
    if order is not None:
        em.set_dual_time(dt)
        levels = random_levels(em)
        em.set_nt_time_levels(levels[0], levels[1] if order == 2 else None)
        assert em.effective_order() == order
    sf = em.final_step_factors(0)
    return em, old, new, levels, sf, em.kernel_level(0, sf)


def composed_settings():
    """sae.COMPOSED's "all" settings as ``configured``'s keywords, alone and with the corrected face gradient and an isothermal wall."""
    name, smoothing, jst_levels, fas, shape = sae.COMPOSED[-1]
    assert name == "all"
    base = dict(smoothing=smoothing, jst_levels=jst_levels, fas=fas, shape=shape, cfl=2.0)
    return (("all", base), ("all_corrected_isothermal", dict(base, face_gradient="corrected", tw_ratio=whe.TW_RATIOS[0])))
