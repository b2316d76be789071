"""The yardstick of the viscosity model (mgcfd_set_viscosity_model): ``VariableViscosityOracle``, tests/viscous_emulator.py's
``ViscousOracle`` with pass 1 of the viscous terms and the viscous step limit replaced by the definition in include/mgcfd.h /
INTEGRATION.md §16, written in numpy.  Pass 2, the wall rule, the sweep and everything below stay ViscousOracle's.

    law 0    mu_i = mu
    law 1    r = T_i / t_ref;   mu_i = ((mu * (r * sqrt(r))) * (1.0 + s)) / (r + s)
    eddy 0   mut_i = +0.0
    eddy 1   mut_i = eddy_viscosity[i]                  (the caller's array of the level, read)
    eddy 2   sxy = 0.5 * (G[u][y] + G[v][x]);  sxz = 0.5 * (G[u][z] + G[w][x]);  syz = 0.5 * (G[v][z] + G[w][y])
             ss  = ((G[u][x]^2 + G[v][y]^2) + G[w][z]^2) + 2.0 * ((sxy^2 + sxz^2) + syz^2)
             mut_i = ((c2 * d2_i) * rho_i) * sqrt(2.0 * ss)      (written to eddy_viscosity[i] by every stress launch)
    me_i = mu_i + mut_i;   kap_i = CP * (mu_i / prandtl + mut_i / prandtl_t);   txx = me_i * (2.0 * G[u][x] - t) ...;   q_d = kap_i * G[T][d]
    limit    a = (4.0/3.0) * (mu_i + mut_i);  b = GAMMA * (mu_i / prandtl + mut_i / prandtl_t);  d_i = a < b ? b : a
             sf_i = min(sf_i, ((cfl_v * rho_i) * g_i) / d_i)     mu_i from the level's variables at that moment, mut_i as the array stands

c2 = cs * cs, CP = GAMMA / (GAMMA - 1.0), d2_i = cbrt(vol_i) * cbrt(vol_i) with libm's cbrt.  numpy's elementwise operations are one
IEEE-754 double operation each and its sqrt is correctly rounded, as the device's is.  The eddy-viscosity array of a level exists
while the viscous terms cover the level and the model is not the default; it holds +0.0 when it comes into being and whenever
the eddy mode changes.  The wall stresses of the friction loads (tests/friction_loads_emulator.py) go through ``stresses`` too:
``wall_stresses``, ``surface_loads12`` and ``distribution`` below hand its S to that module's own edge terms and sums.

The parameters of the GPU runs (tests/test_gpu_variable_viscosity.py), which tests/test_host_variable_viscosity.py keeps valid on
the CPU: Sutherland with t_ref from the far field and s = 0.3831, cs = 0.17, prandtl_t = 0.9, the three models of ``MODELS``, and
for eddy 1 the field ``mu * uniform(0, 10)`` of seed FIELD_SEED + level.  Cases, viscosities, start state, cycles and the step and
wall combinations are viscous_emulator's own (``ve.gpu_combinations()``).
"""
import numpy as np

import friction_loads_emulator as fle
import surface_loads_emulator as sle
import time_step_emulator as tse
import dual_time_emulator as dte
import viscous_emulator as ve

GAMMA = ve.GAMMA
CP = GAMMA / (GAMMA - 1.0)
SUTHERLAND_S = 0.3831
SMAGORINSKY_CS = 0.17
PRANDTL_TURBULENT = 0.9
LAWS = {"constant": 0, "sutherland": 1}
EDDIES = {"none": 0, "field": 1, "smagorinsky": 2}
# (law, eddy) of the bit-for-bit runs; the last one is "the combined model"
MODELS = (("sutherland", "none"), ("constant", "smagorinsky"), ("sutherland", "smagorinsky"))
COMBINED = MODELS[2]
FIELD_SEED = 11
FIELD_MAX = 10.0


class Model:
    """The settings of mgcfd_set_viscosity_model as the kernels get them."""

    def __init__(self, law="constant", t_ref=1.0, s=SUTHERLAND_S, eddy="none", cs=SMAGORINSKY_CS, prandtl_t=PRANDTL_TURBULENT):
        self.law, self.eddy = LAWS.get(law, law), EDDIES.get(eddy, eddy)
        assert self.law in (0, 1) and self.eddy in (0, 1, 2)
        self.t_ref, self.s, self.cs, self.prandtl_t = np.float64(t_ref), np.float64(s), np.float64(cs), np.float64(prandtl_t)
        self.c2 = self.cs * self.cs

    def variable(self):
        return self.law != 0 or self.eddy != 0


def far_field_t_ref(ff17):
    """p_inf / rho_inf with derive()'s pressure, as the library evaluates it on the far field."""
    ff = np.asarray(ff17, dtype=np.float64)
    return sle.pressure(ff[:5])[0] / ff[0]


def viscosity(model, mu, T):
    """mu_i [nel] by the law."""
    T = np.asarray(T, dtype=np.float64)
    if model.law == 0:
        return np.full(len(T), np.float64(mu))
    with np.errstate(all="ignore"):
        r = T / model.t_ref
        return ((np.float64(mu) * (r * np.sqrt(r))) * (1.0 + model.s)) / (r + model.s)


def smagorinsky(model, G, d2, rho):
    """mut_i [nel] from pass 1's gradients G [nel, 4, 3]."""
    ux, uy, uz = G[:, 0, 0], G[:, 0, 1], G[:, 0, 2]
    vx, vy, vz = G[:, 1, 0], G[:, 1, 1], G[:, 1, 2]
    wx, wy, wz = G[:, 2, 0], G[:, 2, 1], G[:, 2, 2]
    with np.errstate(all="ignore"):
        sxy, sxz, syz = 0.5 * (uy + vx), 0.5 * (uz + wx), 0.5 * (vz + wy)
        ss = ((ux * ux + vy * vy) + wz * wz) + 2.0 * ((sxy * sxy + sxz * sxz) + syz * syz)
        return ((model.c2 * d2) * rho) * np.sqrt(2.0 * ss)


def stresses(W, to, frm, N, vol, mu, prandtl, model, d2=None, field=None):
    """Pass 1 under ``model``: (S [nel, 12], mut [nel]); ``field`` is the level's eddy_viscosity array (read under eddy 1)."""
    with np.errstate(all="ignore"):
        q = np.asarray(W, dtype=np.float64).reshape(-1, 5)
        phi = ve.primitives(q)
        G = ve.gradients(phi, to, frm, N, vol)
        mu_i = viscosity(model, mu, phi[:, 3])
        if model.eddy == 0:
            mut = np.zeros(len(q))
        elif model.eddy == 1:
            mut = np.asarray(field, dtype=np.float64).copy()
        else:
            mut = smagorinsky(model, G, np.asarray(d2, dtype=np.float64), q[:, 0])
        me = mu_i + mut
        kap = CP * (mu_i / np.float64(prandtl) + mut / model.prandtl_t)
        ux, uy, uz = G[:, 0, 0], G[:, 0, 1], G[:, 0, 2]
        vx, vy, vz = G[:, 1, 0], G[:, 1, 1], G[:, 1, 2]
        wx, wy, wz = G[:, 2, 0], G[:, 2, 1], G[:, 2, 2]
        div = (ux + vy) + wz
        t = (2.0 / 3.0) * div
        S = np.empty((len(q), 12))
        S[:, 0:3] = phi[:, 0:3]
        S[:, 3], S[:, 4], S[:, 5] = me * (2.0 * ux - t), me * (2.0 * vy - t), me * (2.0 * wz - t)
        S[:, 6], S[:, 7], S[:, 8] = me * (uy + vx), me * (uz + wx), me * (vz + wy)
        S[:, 9:12] = kap[:, None] * G[:, 3, :]
    return S, mut


def limit_step_factors(sf, W, g, mu, prandtl, cfl_v, model, field):
    """The limit under a non-default model; a NaN factor stays NaN."""
    with np.errstate(all="ignore"):
        q = np.asarray(W, dtype=np.float64).reshape(-1, 5)
        rho = q[:, 0]
        mu_i = viscosity(model, mu, ve.jse.pressure(q) / rho)
        mut = np.zeros(len(q)) if model.eddy == 0 else np.asarray(field, dtype=np.float64)
        a = (4.0 / 3.0) * (mu_i + mut)
        b = GAMMA * (mu_i / np.float64(prandtl) + mut / model.prandtl_t)
        d = np.where(a < b, b, a)
        cap = ((np.float64(cfl_v) * rho) * g) / d
    return np.where(cap < sf, cap, sf)


def eddy_field(mu, nel, level):
    """The caller's field of the eddy-1 runs on a level."""
    return np.float64(mu) * np.random.default_rng(FIELD_SEED + level).uniform(0.0, FIELD_MAX, nel)


class VariableViscosityOracle(ve.ViscousOracle):
    """ViscousOracle with the settings of mgcfd_set_viscosity_model."""

    def __init__(self, *args, **kwargs):
        self.model, self.mut, self._held = Model(), None, None
        super().__init__(*args, **kwargs)
        self.d2 = [self.cbrt_vol[l] * self.cbrt_vol[l] for l in range(self.n)]
        self.mut = [np.zeros(self.oc.levels[l].nel) for l in range(self.n)]
        self._held = [False] * self.n
        self.last_mut = [None] * self.n
        self._settle(False)

    def _settle(self, zero):
        """The arrays' lifetime: held while the terms cover the level and the model is not the default."""
        if self.mut is None:
            return
        for l in range(self.n):
            need = self.viscous_on(l) and self.model.variable()
            if not need or not self._held[l] or zero:
                self.mut[l][:] = 0.0
            self._held[l] = need

    def set_viscous(self, *args, **kwargs):
        super().set_viscous(*args, **kwargs)
        self._settle(False)

    def set_viscosity_model(self, law="constant", t_ref=None, s=SUTHERLAND_S, eddy="none", cs=SMAGORINSKY_CS, prandtl_t=PRANDTL_TURBULENT):
        new = Model(law, far_field_t_ref(self.ff17) if t_ref is None else t_ref, s, eddy, cs, prandtl_t)
        changed = new.eddy != self.model.eddy
        self.model = new
        self._settle(changed)

    def eddy_viscosity(self, l):
        assert self._held[l] and self.model.eddy != 0
        return self.mut[l].copy()

    def set_eddy_viscosity(self, l, values):
        assert self._held[l] and self.model.eddy == 1
        self.mut[l][:] = values

    def stresses_of(self, l, W=None):
        """(S, mut) of level ``l`` for the state ``W`` (default: its current variables); nothing is stored."""
        W = self._var(l) if W is None else W
        return stresses(W, self.vto[l], self.vfrm[l], self.vN[l], self.oc.array(l, "volumes"), self.mu, self.prandtl, self.model,
                        self.d2[l], self.mut[l])

    def viscous_terms(self, l, W=None):
        if not self.model.variable():
            return super().viscous_terms(l, W)
        S, self._mut_of_terms = self.stresses_of(l, W)
        return S, ve.viscous_flux(S, self.vto[l], self.vfrm[l], self.vN[l])

    def add_viscous_flux(self, l):
        super().add_viscous_flux(l)                       # (a stress launch: under eddy 2 it writes the array)
        if self.model.eddy == 2:
            self.mut[l][:] = self._mut_of_terms
        if self.model.variable():
            self.last_mut[l] = self.mut[l].copy()

    def final_step_factors(self, l):
        if not self.model.variable():
            return super().final_step_factors(l)
        vol = self.oc.array(l, "volumes")
        free = tse.step_factors(self.mode, self.cfl, self.oc.array(l, "variables"), vol, self.cbrt_vol[l], self.variant)
        sf = limit_step_factors(free, self._var(l), self.g[l], self.mu, self.prandtl, self.cfl_v, self.model, self.mut[l])
        n_bound = int((sf < free).sum())
        self.limited[l][0] += n_bound
        self.limited[l][1] += len(sf) - n_bound
        if self.dt != 0.0:
            sf = dte.clamp_step_factors(sf, vol, self.dt, self.clamp)
        return sf


def configured(oracle, case, mu, mode, cfl, wall, levels, model, smoothing=(0.0, 0), jst_levels=0, fas=False, field=False):
    """The emulator as tests/test_gpu_variable_viscosity.py configures the solver: the start state, the terms switched on, then
    the model (law, eddy) with the parameters above; ``field``: the eddy-1 field written on every covered level."""
    em = VariableViscosityOracle(oracle, case, mode, cfl, *smoothing, kappa2=ve.jse.KAPPA2 if jst_levels else 0.0,
                                 kappa4=ve.jse.KAPPA4 if jst_levels else 0.0, levels=jst_levels, fas=fas)
    v = em._var(0)
    v[:] = ve.start_state(len(v), em.ff17[:5])
    em.set_viscous(mu, ve.PRANDTL, wall, ve.VISCOUS_CFL, levels)
    em.set_viscosity_model(law=model[0], eddy=model[1])
    if field:
        for l in range(em.visc_levels):
            em.set_eddy_viscosity(l, eddy_field(mu, em.oc.levels[l].nel, l))
    return em


# ---- the friction loads under a model: friction_loads_emulator's edge terms and sums on this module's S ----
def node_stresses(variables, edges, level, mu, prandtl, model, field=None):
    """S [nel, 12] of a level dict (friction_loads_emulator's kind) for ``variables``; eddy 2 is formed locally."""
    internal, _ = fle.slices(level)
    e = edges[internal]
    to, frm, N = ve.interleaved(np.asarray(e["a"], dtype=np.int64), np.asarray(e["b"], dtype=np.int64), e)
    vol = np.asarray(level["volumes"], dtype=np.float64)
    cb = tse.libm_cbrt(vol)
    return stresses(variables, to, frm, N, vol, mu, prandtl, model, cb * cb, field)[0]


def wall_stresses(variables, edges, level, S):
    _, wall = fle.slices(level)
    ids = fle.wall_nodes(edges[wall])
    return ids, S[ids]


def surface_loads12(variables, edges, level, ff17, ref_point, S):
    _, wall = fle.slices(level)
    walls = edges[wall]
    pressure = sle.edge_terms(variables, walls, level.get("coords"), ff17, ref_point)
    friction = fle.friction_terms(S, walls, level.get("coords"), ref_point)
    return sle.reduce_loads(np.concatenate([pressure, friction], axis=1))


def distribution(variables, edges, level, ff17, S):
    """friction_loads_emulator.distribution with the stresses given."""
    _, wall = fle.slices(level)
    walls = edges[wall]
    ids = fle.wall_nodes(walls)
    at = np.searchsorted(ids, np.asarray(walls["b"], dtype=np.int64))
    a = np.zeros((len(ids), 3))
    for d, k in enumerate("xyz"):
        np.add.at(a[:, d], at, np.asarray(walls[k], dtype=np.float64))
    q = np.asarray(variables, dtype=np.float64).reshape(-1, 5)
    dp = sle.pressure(q[ids]) - sle.pressure(np.asarray(ff17[:5], dtype=np.float64))[0]
    txx, tyy, tzz, txy, txz, tyz = (S[ids, k] for k in range(3, 9))
    t = np.zeros((len(ids), 3))
    t[:, 0] = -((txx * a[:, 0] + txy * a[:, 1]) + txz * a[:, 2])
    t[:, 1] = -((txy * a[:, 0] + tyy * a[:, 1]) + tyz * a[:, 2])
    t[:, 2] = -((txz * a[:, 0] + tyz * a[:, 1]) + tzz * a[:, 2])
    return ids, np.concatenate([a, dp[:, None], t], axis=1)
