"""The yardstick of the wall thermal conditions and the heat loads (mgcfd_set_wall_temperature, mgcfd_surface_loads_heat,
mgcfd_wall_heat): ``WallHeatOracle``, tests/sa_emulator.py's ``SaOracle`` with the wall rule and the heat-flux
addition of the definition written in numpy, and the heat loads on top of tests/friction_loads_emulator.py and
tests/surface_loads_emulator.py.  Every numpy operation is one IEEE-754 double operation per element, never contracted; numpy's
sqrt is correctly rounded.

    isothermal   ew = Tw / (GAMMA - 1.0) once;  at the wall nodes, wherever the no-slip rule runs: momentum +0.0,
                 variables[i][4] = variables[i][0] * ew  (FAS's W0 is a copy of the state the rule has been applied to: its own density)
                 residuals[i][4] = variables[i][4] - old_variables[i][4]  (the oracle's residual runs behind the last stage's rule)
    heat flux    a_i = the sum of the node's solid-wall weights from +0.0 in B order;  area_i = sqrt((ax*ax + ay*ay) + az*az)
                 behind every addition of V:  fluxes[i][4] = fluxes[i][4] + qw * area_i
    heat loads   edge e of B, node b, weights (x, y, z), q from Sw_b:  h_e = -((qx*x + qy*y) + qz*z),  s_e = sqrt((x*x + y*y) + z*z)
                 out14 = reduce_loads of the twelve columns of §14 with (h_e, s_e) behind them;  h = +0.0 on a non-viscous level
    table        per wall node  h_i = -((qx*ax + qy*ay) + qz*az),  T_i = p_i / rho_i,  area_i

The setting is in effect on the levels the viscous terms cover, and only while their wall is the no-slip one.

What the GPU tests run (tests/test_gpu_wall_heat.py), kept valid on the CPU by tests/test_host_wall_heat.py, is at the end.
"""
import numpy as np

import friction_loads_emulator as fle
import sa_emulator as sae
import surface_loads_emulator as sle
import variable_viscosity_emulator as vve
import viscous_emulator as ve

GAMMA = ve.GAMMA
ADIABATIC, ISOTHERMAL, HEAT_FLUX = 0, 1, 2
MODES = {"adiabatic": ADIABATIC, "isothermal": ISOTHERMAL, "heat-flux": HEAT_FLUX}


def wall_energy(tw):
    """ew of the isothermal wall."""
    return np.float64(tw) / (GAMMA - 1.0)


def node_areas(wall_edges):
    """(ids [n], a [n, 3], area [n]) of the wall nodes of the solid-wall slice ``wall_edges``."""
    ids = fle.wall_nodes(wall_edges)
    at = np.searchsorted(ids, np.asarray(wall_edges["b"], dtype=np.int64))
    a = np.zeros((len(ids), 3))
    for d, k in enumerate("xyz"):
        np.add.at(a[:, d], at, np.asarray(wall_edges[k], dtype=np.float64))           # (one addition per edge, in B order)
    return ids, a, np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def free_stream_temperature(ff17):
    """(t_static, t_total) as mgcfd_free_stream_temperature forms them."""
    ff = np.asarray(ff17, dtype=np.float64)
    rho = ff[0]
    vx, vy, vz = ff[1] / rho, ff[2] / rho, ff[3] / rho
    speed_sqd = vx * vx + vy * vy + vz * vz
    p = (GAMMA - 1.0) * (ff[4] - 0.5 * rho * speed_sqd)
    t = p / rho
    m2 = speed_sqd / (GAMMA * t)
    return float(t), float(t * (1.0 + 0.2 * m2))


def heat_coefficients(ff17, table, t_wall=None):
    """(qw [n], St [n]) by the formula of INTEGRATION.md §19."""
    ff = np.asarray(ff17, dtype=np.float64)
    v = ff[1:4] / ff[0]
    speed = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    tab = np.asarray(table, dtype=np.float64).reshape(-1, 3)
    tw = tab[:, 1] if t_wall is None else np.float64(t_wall)
    with np.errstate(all="ignore"):
        qw = tab[:, 0] / tab[:, 2]
        return qw, qw / (ff[0] * speed * (GAMMA / (GAMMA - 1.0)) * (free_stream_temperature(ff)[1] - tw))


# ---- the heat loads of a level dict (friction_loads_emulator's kind) ----
def node_stresses(variables, edges, level, mu, prandtl, model=None, field=None):
    """S [nel, 12] with the conductivity of whatever model is on: §13's under the default model, §16's otherwise."""
    if model is None or not model.variable():
        internal, _ = fle.slices(level)
        return fle.node_stresses(variables, edges[internal], level["volumes"], mu, prandtl)
    return vve.node_stresses(variables, edges, level, mu, prandtl, model, field)


def heat_terms(S, wall_edges):
    """[n, 2] per-edge (h_e, s_e); S None: h_e = +0.0."""
    x, y, z = (np.asarray(wall_edges[k], dtype=np.float64) for k in "xyz")
    s = np.sqrt((x * x + y * y) + z * z)
    if S is None:
        return np.stack([np.zeros(len(s)), s], axis=1)
    b = np.asarray(wall_edges["b"], dtype=np.int64)
    qx, qy, qz = S[b, 9], S[b, 10], S[b, 11]
    return np.stack([-((qx * x + qy * y) + qz * z), s], axis=1)


def surface_loads14(variables, edges, level, ff17, ref_point, S):
    """out14 = Fp Mp | Fv Mv | Q A of a level's current variables; ``S`` None on a level the terms are not on for."""
    _, wall = fle.slices(level)
    walls = edges[wall]
    if len(walls) == 0:
        return np.zeros(14)
    pressure = sle.edge_terms(variables, walls, level.get("coords"), ff17, ref_point)
    friction = fle.friction_terms(S, walls, level.get("coords"), ref_point)
    return sle.reduce_loads(np.concatenate([pressure, friction, heat_terms(S, walls)], axis=1))


def wall_heat(variables, edges, level, S):
    """(ids [n], table [n, 3]): h | T | area per wall node."""
    _, wall = fle.slices(level)
    ids, a, area = node_areas(edges[wall])
    q = np.asarray(variables, dtype=np.float64).reshape(-1, 5)
    T = sle.pressure(q[ids]) / q[ids, 0]
    h = np.zeros(len(ids))
    if S is not None:
        qx, qy, qz = S[ids, 9], S[ids, 10], S[ids, 11]
        h = -((qx * a[:, 0] + qy * a[:, 1]) + qz * a[:, 2])
    return ids, np.stack([h, T, area], axis=1)


class WallHeatOracle(sae.SaOracle):
    """SaOracle with the setting of mgcfd_set_wall_temperature."""

    def __init__(self, *args, **kwargs):
        self.wt_mode, self.wt_value, self.ew = ADIABATIC, 0.0, np.float64(0.0)
        super().__init__(*args, **kwargs)
        self.area = []
        for l in range(self.n):
            L = self.oc.levels[l]
            ids, _, area = node_areas(self.oc.edges(l)[L.boundary_start:L.boundary_start + L.n_boundary])
            assert np.array_equal(ids, self.wall_nodes[l])
            self.area.append(area)

    def thermal(self, mode):
        return self.wt_mode == mode and bool(self.wall) and self.visc_levels > 0

    def set_wall_temperature(self, mode="adiabatic", value=0.0):
        mode = MODES.get(mode, mode)
        assert mode in (ADIABATIC, ISOTHERMAL, HEAT_FLUX)
        assert mode != ISOTHERMAL or (np.isfinite(value) and value > 0.0)
        assert mode != HEAT_FLUX or np.isfinite(value)
        self.wt_mode, self.wt_value = mode, 0.0 if mode == ADIABATIC else float(value)
        self.ew = wall_energy(value) if mode == ISOTHERMAL else np.float64(0.0)
        if self.thermal(ISOTHERMAL):                 # (going back to adiabatic leaves the state as it stands)
            for l in range(self.visc_levels):
                self.apply_wall(l)

    def apply_wall(self, l):
        super().apply_wall(l)
        if self.viscous_on(l) and self.wall and self.wt_mode == ISOTHERMAL:
            v = self._var(l)
            v[self.wall_nodes[l], 4] = v[self.wall_nodes[l], 0] * self.ew

    def add_viscous_flux(self, l):
        super().add_viscous_flux(l)
        if self.thermal(HEAT_FLUX) and self.viscous_on(l):
            fluxes = self.oc.array(l, "fluxes").reshape(-1, 5)
            w = self.wall_nodes[l]
            fluxes[w, 4] = fluxes[w, 4] + np.float64(self.wt_value) * self.area[l]

    def wall_temperatures(self, l):
        """T = p / rho of level l's wall nodes."""
        q = self._var(l)[self.wall_nodes[l]]
        return sle.pressure(q) / q[:, 0]

    def level_dict(self, l):
        """Level l as the heat loads above take it (the oracle's arrays)."""
        L = self.oc.levels[l]
        return {"nel": L.nel, "internal_start": L.internal_start, "n_internal": L.n_internal, "boundary_start": L.boundary_start,
                "n_boundary": L.n_boundary, "volumes": self.oc.array(l, "volumes"), "coords": self.oc.array(l, "coords").reshape(-1, 3)}

    def wall_stress_rows(self, l):
        """S of level l's current variables under the model that is on (mut as the array holds it); None on a non-viscous level."""
        return self.viscous_terms(l)[0] if self.viscous_on(l) else None

    def heat_loads(self, l, ref_point=(0.0, 0.0, 0.0)):
        return surface_loads14(self._var(l), self.oc.edges(l), self.level_dict(l), self.ff17, ref_point, self.wall_stress_rows(l))

    def heat_table(self, l):
        return wall_heat(self._var(l), self.oc.edges(l), self.level_dict(l), self.wall_stress_rows(l))


# ---- what the GPU tests run ----
GPU_CYCLES = ve.GPU_CYCLES
# Wall temperatures as multiples of the static free-stream temperature and the heat flux of mode 2: a hot and a cold wall well
# away from the free stream (so that the sign of Q is not a matter of rounding) and inside what every mesh below stands for
# GPU_CYCLES cycles from the perturbed start state without a NaN or a negative energy (tests/test_host_wall_heat.py runs them all).
TW_RATIOS = (1.5, 0.5)
QW = 0.05
# the second wall temperature of the mid-run change
TW_RATIO_CHANGED = 1.25
RUN_STEP = ("reference", 0.5)               # the step tests/friction_loads_emulator.py validated GPU_MU under
RUN_MU = dict(fle.GPU_MU)                         # A, box17, hull9, mixed_2lvl, tet_2lvl
RUN_CASES = ("A", "hull9", "box17", "tet_2lvl")
GENERATED = fle.GPU_GENERATED
MULTI_LEVEL = ("A", "tet_2lvl")                   # (hull9 and box17 are one level: "one level" and "all levels" are the same run)
# (name, (eps, iterations), JST levels, FAS) on lattice A, all levels: one at a time
COMPOSED = (("smoothing", (0.5, 2), 0, False), ("jst_level0", (0.0, 0), 1, False), ("fas", (0.0, 0), 0, True))
SA_MODEL = ("sutherland", sae.SA)
DUAL_DT, DUAL_STEPS, DUAL_CYCLES = 0.05, ve.DUAL_STEPS, ve.DUAL_CYCLES


def thermal_settings(ff17):
    """The (mode, value) pairs of the plain runs for a far field: two isothermal walls and the heat-flux wall."""
    t = free_stream_temperature(ff17)[0]
    return tuple((ISOTHERMAL, r * t) for r in TW_RATIOS) + ((HEAT_FLUX, QW),)


def gpu_runs():
    """(case key, levels, mode, ratio-or-flux) of the plain bit-for-bit runs."""
    return [(case, lv, mode, x) for case in RUN_CASES for lv in (ve.GPU_LEVELS if case in MULTI_LEVEL else (1,))
            for mode, x in ((ISOTHERMAL, TW_RATIOS[0]), (ISOTHERMAL, TW_RATIOS[1]), (HEAT_FLUX, QW))]


def setting_value(ff17, mode, x):
    return x * free_stream_temperature(ff17)[0] if mode == ISOTHERMAL else x


def configured(oracle, case, mu, levels, mode, x, smoothing=(0.0, 0), jst_levels=0, fas=False, model=None, step=RUN_STEP, order=(0, 1)):
    """The emulator as tests/test_gpu_wall_heat.py configures the solver: the start state, then the viscous terms with no-slip
    walls and the thermal setting in ``order``, then the viscosity model."""
    cfl = 2.0 if smoothing[1] else step[1]
    em = WallHeatOracle(oracle, case, step[0], cfl, *smoothing, kappa2=ve.jse.KAPPA2 if jst_levels else 0.0,
                        kappa4=ve.jse.KAPPA4 if jst_levels else 0.0, levels=jst_levels, fas=fas)
    v = em._var(0)
    v[:] = ve.start_state(len(v), em.ff17[:5])
    setters = (lambda: em.set_viscous(mu, ve.PRANDTL, 1, ve.VISCOUS_CFL, levels),
               lambda: em.set_wall_temperature(mode, setting_value(em.ff17, mode, x)))
    for k in order:
        setters[k]()
    if model is not None:
        em.set_viscosity_model(law=model[0], eddy=model[1])
    return em
