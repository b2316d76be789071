"""The yardstick of the corrected face gradient (mgcfd_set_face_gradient): ``FaceGradientOracle``,
tests/wall_heat_emulator.py's ``WallHeatOracle`` (and so ``SaOracle`` and everything below it) with the definition written in numpy,
line by line.  Every numpy operation is one IEEE-754 double operation per element (numpy never contracts to FMA, its sqrt and
its division are correctly rounded); ``np.add.at`` adds in index order, so with the edge ends interleaved (a0, b0, a1, b1, ...)
a node's sum runs over its internal edges in the level's original edge order, from +0.0.

    per edge end (node i, other node j, normal n seen from i), x the level's coordinates as given at creation:
        dx = x_j - x_i;  L = sqrt((dx.x*dx.x + dx.y*dx.y) + dx.z*dx.z);  t = dx / L;    L == 0.0: the edge contributes nothing
        gb[phi][d] = 0.5 * (G_i[phi][d] + G_j[phi][d]),  G: §13 pass 1's gradients of phi = (u, v, w, T)
        c_phi = (phi_j - phi_i) / L - ((gb[phi][x]*t.x + gb[phi][y]*t.y) + gb[phi][z]*t.z)
        mf = 0.5 * (me_i + me_j);  kf = 0.5 * (kap_i + kap_j)     (me, kap: pass 1's, mut as it stands behind the stress launch)
        dv = (c_u*t.x + c_v*t.y) + c_w*t.z;  tt = (2.0/3.0) * dv
        txx = mf*(2.0*(c_u*t.x) - tt) ...;  txy = mf*(c_u*t.y + c_v*t.x) ...;  q_d = kf*(c_T*t_d)
        Vc_i[1..3] += tau . n;   Wk_i += (tau . vb) . n,  vb = 0.5 * (v_i + v_j);   Hc_i += q . n
    F[i][1..3] = F[i][1..3] + Vc_i[1..3];  F[i][4] = (F[i][4] + Wk_i) + Hc_i      directly behind F = F + V; §19's heat-flux wall follows
    Spalart-Allmaras pass 2:  c_nt likewise from nt and G[nt];  tn = (t.x*nx + t.y*ny) + t.z*nz;  Qdc += nb * (c_nt * tn);
                              Qd + Qdc stands where Qd stood

The parameters of the GPU runs (tests/test_gpu_face_gradient.py), which tests/test_host_face_gradient.py keeps valid on the CPU, are
at the end.
"""
import numpy as np

import sa_emulator as sae
import variable_viscosity_emulator as vve
import viscous_emulator as ve
import wall_heat_emulator as whe

AVERAGED, CORRECTED = 0, 1
MODES = {"averaged": AVERAGED, "corrected": CORRECTED}
ARR_VISCOUS_GRADIENT = 19
VISCOUS_CFL_CORRECTED = 0.2          # MGCFD_VISCOUS_CFL_CORRECTED


def edge_geometry(X, to, frm):
    """(t [2E, 3], L [2E]) per edge end; t is NaN where L == 0.0 (such ends are masked out of every sum)."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 3)
    dx = X[frm] - X[to]
    L = np.sqrt((dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]) + dx[:, 2] * dx[:, 2])
    with np.errstate(all="ignore"):
        return dx / L[:, None], L


def along_edge(phi, G, to, frm, t, L):
    """c_phi [2E]: the two-point difference minus the along-edge component of the averaged gradient G [nel, 3] of phi [nel]."""
    with np.errstate(all="ignore"):
        gb = 0.5 * (G[to] + G[frm])
        return (phi[frm] - phi[to]) / L - ((gb[:, 0] * t[:, 0] + gb[:, 1] * t[:, 1]) + gb[:, 2] * t[:, 2])


def edge_terms(phi, G, me, kap, X, to, frm, N):
    """(terms [2E, 5] = the edge end's additions to Vc[1], Vc[2], Vc[3], Wk, Hc; ok [2E] = L != 0.0)."""
    with np.errstate(all="ignore"):
        t, L = edge_geometry(X, to, frm)
        tx, ty, tz = t[:, 0], t[:, 1], t[:, 2]
        nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
        cu, cv, cw, cT = (along_edge(phi[:, k], G[:, k, :], to, frm, t, L) for k in range(4))
        mf = 0.5 * (me[to] + me[frm])
        kf = 0.5 * (kap[to] + kap[frm])
        dv = (cu * tx + cv * ty) + cw * tz
        tt = (2.0 / 3.0) * dv
        txx, tyy, tzz = mf * (2.0 * (cu * tx) - tt), mf * (2.0 * (cv * ty) - tt), mf * (2.0 * (cw * tz) - tt)
        txy, txz, tyz = mf * (cu * ty + cv * tx), mf * (cu * tz + cw * tx), mf * (cv * tz + cw * ty)
        qx, qy, qz = kf * (cT * tx), kf * (cT * ty), kf * (cT * tz)
        b = 0.5 * (phi[to, 0:3] + phi[frm, 0:3])
        ub, vb, wb = b[:, 0], b[:, 1], b[:, 2]
        wx = (ub * txx + vb * txy) + wb * txz
        wy = (ub * txy + vb * tyy) + wb * tyz
        wz = (ub * txz + vb * tyz) + wb * tzz
        terms = np.stack([(txx * nx + txy * ny) + txz * nz, (txy * nx + tyy * ny) + tyz * nz, (txz * nx + tyz * ny) + tzz * nz,
                          (wx * nx + wy * ny) + wz * nz, (qx * nx + qy * ny) + qz * nz], axis=1)
    return terms, L != 0.0


def node_sums(terms, ok, to, nel):
    """[nel, 5]: Vc[1..3], Wk, Hc from +0.0, one addition per edge end with L != 0.0, in edge order."""
    out = np.zeros((nel, terms.shape[1]))
    with np.errstate(all="ignore"):
        for k in range(terms.shape[1]):
            np.add.at(out[:, k], to[ok], terms[ok, k])
    return out


def correction(W, vol, me, kap, X, to, frm, N):
    """(G [nel, 4, 3], sums [nel, 5], terms [2E, 5], ok [2E]) of the state W."""
    with np.errstate(all="ignore"):
        phi = ve.primitives(W)
        G = ve.gradients(phi, to, frm, N, vol)
    nel = len(phi)
    me = np.broadcast_to(np.asarray(me, dtype=np.float64), (nel,))
    kap = np.broadcast_to(np.asarray(kap, dtype=np.float64), (nel,))
    terms, ok = edge_terms(phi, G, me, kap, X, to, frm, N)
    return G, node_sums(terms, ok, to, nel), terms, ok


def add_correction(F, sums):
    """F [nel, 5] behind F = F + V: the definition's two lines."""
    F[:, 1:4] = F[:, 1:4] + sums[:, 0:3]
    F[:, 4] = (F[:, 4] + sums[:, 3]) + sums[:, 4]


def sa_edge_terms(nt, grad, X, to, frm, N):
    """(per-end additions to Qdc [2E], ok [2E]); grad: sa_gradient [nel, 5] = G[nt] | om | nu."""
    with np.errstate(all="ignore"):
        t, L = edge_geometry(X, to, frm)
        nu = grad[:, 4]
        nb = 0.5 * ((nu[to] + nt[to]) + (nu[frm] + nt[frm]))
        c = along_edge(nt, grad[:, 0:3], to, frm, t, L)
        tn = (t[:, 0] * N[:, 0] + t[:, 1] * N[:, 1]) + t[:, 2] * N[:, 2]
        return nb * (c * tn), L != 0.0


def sa_qdc(nt, grad, X, to, frm, N):
    terms, ok = sa_edge_terms(np.asarray(nt, dtype=np.float64), grad, X, to, frm, N)
    out = np.zeros(len(nt))
    with np.errstate(all="ignore"):
        np.add.at(out, to[ok], terms[ok])
    return out


def transport(W, nt, nt_old, grad, to, frm, N, vol, d, g, sf, cfl_v, j, X):
    """sa_emulator.transport with Qd + Qdc (one addition) where Qd stood: its edge sums are wrapped for the call."""
    plain = sae.edge_sums

    def corrected(W_, nt_, grad_, to_, frm_, N_):
        Qc, Qd = plain(W_, nt_, grad_, to_, frm_, N_)
        with np.errstate(all="ignore"):
            return Qc, Qd + sa_qdc(nt_, grad_, X, to_, frm_, N_)

    sae.edge_sums = corrected
    try:
        return sae.transport(W, nt, nt_old, grad, to, frm, N, vol, d, g, sf, cfl_v, j)
    finally:
        sae.edge_sums = plain


class FaceGradientOracle(whe.WallHeatOracle):
    """WallHeatOracle with the setting of mgcfd_set_face_gradient."""

    def __init__(self, *args, **kwargs):
        self.fg_mode = AVERAGED
        super().__init__(*args, **kwargs)
        self.X = [self.oc.array(l, "coords").reshape(-1, 3).copy() for l in range(self.n)]
        self.last_G, self.last_sums, self.last_terms = [None] * self.n, [None] * self.n, [None] * self.n

    def set_face_gradient(self, mode="corrected"):
        mode = MODES.get(mode, mode)
        assert mode in (AVERAGED, CORRECTED)
        self.fg_mode = mode

    def fg_on(self, l):
        return self.fg_mode == CORRECTED and self.viscous_on(l)

    def node_coefficients(self, l):
        """(me, kap) of level l's nodes: the constants without a viscosity model; §16/§18's expressions with mut as the array
        holds it (behind the stress launch) otherwise."""
        nel = self.oc.levels[l].nel
        if not self.model.variable():
            return np.full(nel, np.float64(self.mu)), np.full(nel, ve.conductivity(self.mu, self.prandtl))
        with np.errstate(all="ignore"):
            mu_i = vve.viscosity(self.model, self.mu, ve.primitives(self._var(l))[:, 3])
            mut = np.zeros(nel) if self.model.eddy == 0 else self.mut[l].copy()
            return mu_i + mut, vve.CP * (mu_i / np.float64(self.prandtl) + mut / self.model.prandtl_t)

    def face_correction(self, l):
        me, kap = self.node_coefficients(l)
        return correction(self._var(l), self.oc.array(l, "volumes"), me, kap, self.X[l], self.vto[l], self.vfrm[l], self.vN[l])

    def add_viscous_flux(self, l):
        if not self.fg_on(l):
            return super().add_viscous_flux(l)
        sae.SaOracle.add_viscous_flux(self, l)            # pass 1 of the model, S, F = F + V (the stress launch leaves mut)
        self.last_G[l], self.last_sums[l], self.last_terms[l], _ = self.face_correction(l)
        fluxes = self.oc.array(l, "fluxes").reshape(-1, 5)
        add_correction(fluxes, self.last_sums[l])
        if self.thermal(whe.HEAT_FLUX):                   # §19's heat-flux wall, behind the correction
            w = self.wall_nodes[l]
            fluxes[w, 4] = fluxes[w, 4] + np.float64(self.wt_value) * self.area[l]

    def viscous_gradient(self, l):
        """MGCFD_ARR_VISCOUS_GRADIENT [nel, 12] of the last flux launch of level l."""
        assert self.fg_on(l) and self.last_G[l] is not None
        return self.last_G[l].reshape(-1, 12).copy()

    def _transport(self, j, sf):
        args = (self._var(0), self.nt[0], self.nt_old, self.sa_grad, self.vto[0], self.vfrm[0], self.vN[0],
                self.oc.array(0, "volumes"), self.wall_distance(0)[0], self.g[0], sf, self.cfl_v, j)
        return transport(*args, self.X[0]) if self.fg_on(0) else sae.transport(*args)

    def sa_transport(self, j, sf):
        if not self.fg_on(0):
            return super().sa_transport(j, sf)
        out, masks = self._transport(j, sf)
        for k in sae.BRANCHES:
            self.branches[k] += int(masks[k].sum())
        self.nt[0] = out

    def kernel_level(self, j, sf):
        f = self.stage_fluxes(0)
        grad, mut, S = self.sa_grad.copy(), self.mut[0].copy(), self.last_S[0].copy()
        out, masks = self._transport(j, sf)
        return grad, mut, S, f, out, masks


# ---- what the GPU tests run ----
GPU_CYCLES = ve.GPU_CYCLES
RUN_CASES = ("A", "B", "tet_2lvl")
RUN_MU = dict(sae.RUN_MU)                       # lattices at the cell-Reynolds viscosity, tet_2lvl at its GPU_MU
RUN_STEP = ("local", 1.0)
SA_MODEL = ("sutherland", sae.SA)
TW_RATIO, QW = whe.TW_RATIOS[0], whe.QW
DUAL_DT, DUAL_STEPS, DUAL_CYCLES = whe.DUAL_DT, ve.DUAL_STEPS, ve.DUAL_CYCLES
# (name, keyword arguments of ``configured``): each option of the viscous path in turn, then all that combine.  The Spalart-Allmaras
# model and dual time stepping exclude each other, and one eddy model and one wall condition are in effect at a time, so there
# are two: "all_sa" takes residual smoothing, JST, FAS, the W cycle, Sutherland with SA and the heat-flux wall; "all_dual" takes
# residual smoothing, JST, FAS, the W cycle, Sutherland with the damped Smagorinsky model, the isothermal wall and mgcfd_advance.
# ``dual``: the run is mgcfd_advance (BDF2 from the second step on) and not GPU_CYCLES cycles.
COMPOSED = (("smoothing", dict(smoothing=(0.5, 2))),
            ("jst_level0", dict(jst_levels=1)),
            ("fas", dict(fas=True)),
            ("w_cycle", dict(shape="W")),
            ("advance_bdf2", dict(dual=True)),
            ("sutherland", dict(model=("sutherland", "none"))),
            ("smagorinsky_damped", dict(model=("constant", "smagorinsky"), damping=True)),
            ("sa", dict(model=SA_MODEL)),
            ("isothermal", dict(thermal=(whe.ISOTHERMAL, TW_RATIO))),
            ("heat_flux", dict(thermal=(whe.HEAT_FLUX, QW))),
            ("all_sa", dict(smoothing=(0.5, 2), jst_levels=1, fas=True, shape="W", model=SA_MODEL, thermal=(whe.HEAT_FLUX, QW))),
            ("all_dual", dict(smoothing=(0.5, 2), jst_levels=1, fas=True, shape="W", model=("sutherland", "smagorinsky"), damping=True,
                              thermal=(whe.ISOTHERMAL, TW_RATIO), dual=True)))


def gpu_runs():
    """(case key, wall, levels) of the plain bit-for-bit runs."""
    return [(case, wall, lv) for case in RUN_CASES for wall in ve.GPU_WALLS for lv in ve.GPU_LEVELS]


# Composed runs left out: FAS with the no-slip terms on level 0 of lattice A alone (the coarse levels then run slip walls against
# level 0's no-slip state) leaves the valid states in the second cycle under the averaged gradient at MGCFD_VISCOUS_CFL as well
# (tests/test_host_face_gradient.py asserts that), so there is no state to compare.
COMPOSED_INVALID = (("fas", "A", 1, 1), ("all_sa", "A", 1, 1))
# mgcfd_advance on lattice B (jitter 0.25 h: edges down to half a lattice step) runs at cfl_v = 0.05: at 0.2 and 0.1 the corrected
# run leaves the valid states in the fifth or sixth of its six cycles, where the averaged one at 0.25 survives them.
COMPOSED_CFL_V = {("advance_bdf2", "B"): 0.05}


def composed_runs():
    """(name, keyword arguments, case key, wall, levels): every plain run composed with every entry of COMPOSED, but for
    COMPOSED_INVALID; the keywords carry the run's cfl_v."""
    return [(name, dict(kw, cfl_v=COMPOSED_CFL_V.get((name, case), VISCOUS_CFL_CORRECTED)), case, wall, lv)
            for name, kw in COMPOSED for case, wall, lv in gpu_runs() if (name, case, wall, lv) not in COMPOSED_INVALID]


def run(em, dual=False):
    """(rc, rms) of a configured emulator's run: GPU_CYCLES cycles, or under dual time DUAL_STEPS steps of DUAL_CYCLES cycles."""
    if dual:
        rc, rms = em.advance(DUAL_STEPS, DUAL_CYCLES)
        return rc, np.asarray(rms, dtype=np.float64).reshape(DUAL_STEPS, DUAL_CYCLES)
    return em.cycles(GPU_CYCLES)


def configured(oracle, case, mu, wall, levels, smoothing=(0.0, 0), jst_levels=0, fas=False, shape="V", model=None, damping=False,
               thermal=None, dual=False, order=(0, 1), mode="corrected", cfl_v=VISCOUS_CFL_CORRECTED, step=RUN_STEP):
    """The emulator as tests/test_gpu_face_gradient.py configures the solver: the start state, then the viscous terms and the
    face-gradient mode in ``order``, then the thermal setting, the wall damping, the viscosity model and dual time stepping."""
    cfl = 2.0 if smoothing[1] else step[1]
    em = FaceGradientOracle(oracle, case, step[0], cfl, *smoothing, kappa2=ve.jse.KAPPA2 if jst_levels else 0.0,
                            kappa4=ve.jse.KAPPA4 if jst_levels else 0.0, levels=jst_levels, fas=fas)
    if shape != "V":
        em.set_cycle(shape)
    v = em._var(0)
    v[:] = ve.start_state(len(v), em.ff17[:5])
    setters = (lambda: em.set_viscous(mu, ve.PRANDTL, wall, cfl_v, levels), lambda: em.set_face_gradient(mode))
    for k in order:
        setters[k]()
    if thermal is not None:
        em.set_wall_temperature(thermal[0], whe.setting_value(em.ff17, *thermal))
    if damping:
        em.set_wall_damping(True)
    if model is not None:
        em.set_viscosity_model(law=model[0], eddy=model[1])
    if dual:
        em.set_dual_time(DUAL_DT)
    return em
