"""The yardstick of the wall distance (mgcfd_compute_wall_distance, mgcfd_wall_spacing, mgcfd_set_wall_damping): the
definition of include/mgcfd.h / INTEGRATION.md §17 in numpy, and ``WallDampedOracle``, tests/variable_viscosity_emulator.py's
``VariableViscosityOracle`` with the wall-limited Smagorinsky length scale.

    wall nodes   W_0 < W_1 < .. < W_{m-1}: the distinct b ends of the level's solid-wall edges, ascending original id
    distance     best = +inf; near = -1
                 for j = 0 .. m-1:  dx = x_i - x_Wj; dy = y_i - y_Wj; dz = z_i - z_Wj;  r2 = (dx*dx + dy*dy) + dz*dz
                                    if r2 < best: best = r2; near = j
                 d_i = sqrt(best);  nearest_i = near < 0 ? -1 : W_near
    spacing      h_k = min of d_n over the other ends n of W_k's internal incidences with d_n > 0.0; +0.0 where there is none
    damping      a = c2 * d2_i;  kd = kappa * d_i;  w2 = kd * kd;  l2_i = w2 < a ? w2 : a;   mut_i = (l2_i * rho_i) * sqrt(2.0 * ss)

The loop over j is the definition's, in its order, with the strict <; every step is vectorised over i, and numpy's elementwise
operations are one IEEE-754 double operation each (its sqrt is correctly rounded, as the device's is).  A NaN r2 compares false and
is never taken.  The damped eddy viscosity goes through variable_viscosity_emulator.stresses with c2 = 1.0 and l2 in d2's place:
(1.0 * l2_i) * rho_i is (l2_i * rho_i) bit for bit, since a product with 1.0 is exact.
"""
import copy

import numpy as np

import friction_loads_emulator as fle
import time_step_emulator as tse
import variable_viscosity_emulator as vve
import viscous_emulator as ve

WALL_KAPPA = 0.41
ARR_WALL_DISTANCE = 16


def wall_distance(coords, wall_ids):
    """(d [nel], nearest [nel] original ids or -1) of the nodes at ``coords [nel, 3]`` against the wall nodes ``wall_ids`` (ascending)."""
    x = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
    ids = np.asarray(wall_ids, dtype=np.int64)
    assert np.all(np.diff(ids) > 0)
    best = np.full(len(x), np.inf)
    near = np.full(len(x), -1, dtype=np.int64)
    with np.errstate(all="ignore"):
        for j in range(len(ids)):
            w = x[ids[j]]
            dx, dy, dz = x[:, 0] - w[0], x[:, 1] - w[1], x[:, 2] - w[2]
            r2 = (dx * dx + dy * dy) + dz * dz
            take = r2 < best
            best = np.where(take, r2, best)
            near = np.where(take, j, near)
        d = np.sqrt(best)
    return d, np.where(near < 0, -1, ids[np.maximum(near, 0)] if len(ids) else -1)


def tied_nodes(coords, wall_ids):
    """How many nodes have their minimal r2 at more than one wall node (the tie rule decides their ``nearest``)."""
    x = np.asarray(coords, dtype=np.float64).reshape(-1, 3)
    ids = np.asarray(wall_ids, dtype=np.int64)
    if len(ids) == 0:
        return 0
    best = np.full(len(x), np.inf)
    count = np.zeros(len(x), dtype=np.int64)
    for j in range(len(ids)):
        w = x[ids[j]]
        dx, dy, dz = x[:, 0] - w[0], x[:, 1] - w[1], x[:, 2] - w[2]
        r2 = (dx * dx + dy * dy) + dz * dz
        count = np.where(r2 < best, 1, np.where(r2 == best, count + 1, count))
        best = np.minimum(best, r2)
    return int((count > 1).sum())


def wall_spacing(d, internal_edges, wall_ids):
    """h [m]: the walk over the internal edges in their order, an a end before a b end as the wall rows are built."""
    ids = np.asarray(wall_ids, dtype=np.int64)
    a, b = np.asarray(internal_edges["a"], dtype=np.int64), np.asarray(internal_edges["b"], dtype=np.int64)
    h = np.zeros(len(ids))
    found = np.zeros(len(ids), dtype=bool)
    at = {int(w): k for k, w in enumerate(ids)}
    for ea, eb in zip(a.tolist(), b.tolist()):
        for me, other in ((ea, eb), (eb, ea)):
            k = at.get(me)
            if k is None:
                continue
            dn = d[other]
            if dn > 0.0 and (not found[k] or dn < h[k]):
                h[k], found[k] = dn, True
    return h


def length_scale(c2, d2, kappa, d):
    """l2 [nel]."""
    with np.errstate(all="ignore"):
        a = np.float64(c2) * np.asarray(d2, dtype=np.float64)
        kd = np.float64(kappa) * np.asarray(d, dtype=np.float64)
        w2 = kd * kd
        return np.where(w2 < a, w2, a)


def level_wall_nodes(level_mesh):
    """The wall nodes of a meshgen.LevelMesh: the nodes with a solid-wall face (code -1), ascending."""
    node = np.repeat(np.arange(level_mesh.nel, dtype=np.int64), np.diff(level_mesh.nbr_ptr))
    return np.unique(node[np.asarray(level_mesh.nbr_idx) == -1])


def _unit(model):
    m = copy.copy(model)
    m.c2 = np.float64(1.0)
    return m


class WallDampedOracle(vve.VariableViscosityOracle):
    """VariableViscosityOracle with mgcfd_set_wall_damping: d per level from the case's coordinates, l2 formed by every setter."""

    def __init__(self, *args, **kwargs):
        self.wd_on, self.wd_kappa, self.l2, self.dist = False, np.float64(WALL_KAPPA), None, None
        super().__init__(*args, **kwargs)
        self.dist = [None] * self.n
        self.l2 = [None] * self.n
        self._settle_damping()

    def wall_distance(self, l):
        if self.dist[l] is None:
            self.dist[l] = wall_distance(self.oc.array(l, "coords").reshape(-1, 3), self.wall_nodes[l])
        return self.dist[l]

    def damped(self, l):
        return bool(self.wd_on) and self.model.eddy == 2 and self.viscous_on(l)

    def _settle_damping(self):
        if self.l2 is None:
            return
        for l in range(self.n):
            self.l2[l] = length_scale(self.model.c2, self.d2[l], self.wd_kappa, self.wall_distance(l)[0]) if self.damped(l) else None

    def set_viscous(self, *args, **kwargs):
        super().set_viscous(*args, **kwargs)
        self._settle_damping()

    def set_viscosity_model(self, *args, **kwargs):
        super().set_viscosity_model(*args, **kwargs)
        self._settle_damping()

    def set_wall_damping(self, on=True, kappa=WALL_KAPPA):
        self.wd_on, self.wd_kappa = bool(on), np.float64(kappa)
        self._settle_damping()

    def stresses_of(self, l, W=None):
        if not self.damped(l):
            return super().stresses_of(l, W)
        W = self._var(l) if W is None else W
        return vve.stresses(W, self.vto[l], self.vfrm[l], self.vN[l], self.oc.array(l, "volumes"), self.mu, self.prandtl,
                            _unit(self.model), self.l2[l], self.mut[l])


def configured(oracle, case, mu, mode, cfl, wall, levels, model, kappa=WALL_KAPPA, smoothing=(0.0, 0), jst_levels=0, fas=False):
    """The emulator as tests/test_gpu_wall_distance.py configures the solver: vve.configured's order, then the damping."""
    em = WallDampedOracle(oracle, case, mode, cfl, *smoothing, kappa2=ve.jse.KAPPA2 if jst_levels else 0.0,
                          kappa4=ve.jse.KAPPA4 if jst_levels else 0.0, levels=jst_levels, fas=fas)
    v = em._var(0)
    v[:] = ve.start_state(len(v), em.ff17[:5])
    em.set_viscous(mu, ve.PRANDTL, wall, ve.VISCOUS_CFL, levels)
    em.set_viscosity_model(law=model[0], eddy=model[1])
    em.set_wall_damping(True, kappa)
    return em


# The damped runs of tests/test_gpu_wall_distance.py, which tests/test_host_wall_distance.py keeps valid on the CPU: the cases,
# viscosities and steps of tests/test_gpu_variable_viscosity.py's bit-for-bit runs (ve.gpu_combinations()) with no-slip walls on
# all levels, under (constant, smagorinsky) and the combined model, kappa = WALL_KAPPA, ve.GPU_CYCLES cycles; and one composed run.
DAMPED_MODELS = (("constant", "smagorinsky"), vve.COMBINED)
DAMPED_CASES = ("A", "B", "tet_2lvl")
COMPOSED = ve.COMPOSED[-1]          # residual smoothing, JST on level 0, dual time (BDF2) and FAS together


def gpu_runs():
    """(case key, mu, mode, cfl, wall, levels, model) of the damped bit-for-bit runs."""
    return [c + (m,) for m in DAMPED_MODELS for c in ve.gpu_combinations() if c[0] in DAMPED_CASES and c[4] == 1 and c[5] == "all"]


# ---- §14's wall stresses under the damped model, on a level dict (friction_loads_emulator's kind) ----
def damped_stresses(variables, edges, level, mu, prandtl, model, kappa, wall_ids):
    """(S [nel, 12], mut [nel]) of a level dict for ``variables`` with eddy 2 damped: vve.node_stresses with l2 in d2's place."""
    internal, _ = fle.slices(level)
    e = edges[internal]
    to, frm, N = ve.interleaved(np.asarray(e["a"], dtype=np.int64), np.asarray(e["b"], dtype=np.int64), e)
    vol = np.asarray(level["volumes"], dtype=np.float64)
    cb = tse.libm_cbrt(vol)
    d, _ = wall_distance(level["coords"], wall_ids)
    l2 = length_scale(model.c2, cb * cb, kappa, d)
    return vve.stresses(variables, to, frm, N, vol, mu, prandtl, _unit(model), l2, None)


def node_stresses(variables, edges, level, mu, prandtl, model, kappa, wall_ids):
    return damped_stresses(variables, edges, level, mu, prandtl, model, kappa, wall_ids)[0]
