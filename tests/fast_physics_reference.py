"""The yardstick of the fast flavour (MGCFD_OPT_EXACT = 0) of the launchers behind the flux kernels: the two viscous passes
(constant viscosity, Sutherland's law, an eddy-viscosity field), the two JST passes, the source terms of one smoothing sweep
(viscous step limit, dual time's source and clamp, the Jacobi iterations of residual smoothing) and the weighted sums of the FAS
restriction and the prolongations, in numpy ``longdouble``, written from the definitions in INTEGRATION.md (§9 - §13, §15, §16)
and the docstring formulas of the emulators — not from the kernels.  ``LD``, ``U``, ``K``, ``K_sweep``, ``rel_units``,
``RefLevel`` and ``make_state`` are tests/fast_accuracy_reference.py's, imported, not copied.

Every evaluation returns its value S and its MAGNITUDE A.  In tests/fast_accuracy_reference.py A is "the sum of the absolute
values of the products S is made of", because there every product is formed from the launch's exact input.  Here most sums are
formed from values that were themselves computed in the same launch — a gradient sums differences of u = mx / rho, a stress sums
gradients — so a magnitude is carried along with every value, by the rules of a first-order rounding analysis:

    an input of the launch        A = |x|                      (exact: x - y of two inputs has A = |x - y|)
    x + y, x - y                  A = A_x + A_y                (a cancellation never makes the unit smaller)
    x * y, x / y                  A = A_x * A_y,  A_x / |y|    (y an input or a sum of positive terms)
    sqrt(x), Sutherland's law     A = |f(x)| * max(1, |x f'(x) / f(x)|) * A_x / |x|

so that ``U * A`` is the size of one rounding of the largest thing that went into S, wherever in the launch it was rounded.
With these, txx = mu * (2 G[u][x] - t) has A = A_mu * (2 A_G[u][x] + (2/3) (A_G[u][x] + A_G[v][y] + A_G[w][z])): every term
counted separately, with the gradients' own magnitudes in place of their absolute values (A_G >= |G|: on a nearly uniform field
a gradient is a hundred times smaller than the products it was summed from, and its absolute value would be no unit for it).

Each pass is evaluated on its own input: pass 2 of the viscous terms takes the rows S a launch of pass 1 WROTE (doubles, exact
as input), the JST correction takes L, nu and r as read back, so no bound has to absorb the launch before.  Inside ``sweep`` the
stages chain, and the chained magnitudes are handed on instead (``S_mag``, ``L_mag``, ``r_mag``).

Host only: numpy and what tests/fast_accuracy_reference.py needs.  tests/test_host_fast_physics.py and
tests/test_gpu_fast_physics.py share it.
"""
import os

import numpy as np

import fast_accuracy_reference as far
from fast_accuracy_reference import LD, U, K, K_sweep, rel_units, RefLevel, make_state, GAMMA, K_SMOOTHING, CLASSES, RK  # noqa: F401

TWO_THIRDS = LD(np.float64(2.0 / 3.0))
FOUR_THIRDS = LD(np.float64(4.0 / 3.0))
CP = LD(np.float64(1.4 / (1.4 - 1.0)))
MARGIN = 3.0                                         # the GPU bound: K <= 3 * max(K_ref, 1)

# What the GPU tests run (tests/test_gpu_fast_physics.py), and tests/test_host_fast_physics.py keeps valid on the CPU
MESHES = ("lattice_A", "tet", "hub", "isolated")
AMPLITUDE = {"lattice_A": 0.01, "tet": 0.002, "hub": 0.002, "isolated": 0.002}
LOCAL_CFL = {"lattice_A": 1.0, "tet": 0.02, "hub": 0.02, "isolated": 0.02}
MU = {"lattice_A": 0.07, "tet": 1e-3, "hub": 1e-9, "isolated": 1e-9}          # lattice A: viscous_emulator.CELL_RE_MU
STATE_SEED = 7
PRANDTL, VISCOUS_CFL = 0.72, 0.25                    # viscous_emulator.PRANDTL, VISCOUS_CFL
JST_PAIRS = ((2.5, 0.15625), (0.0, 0.15625), (600.0, 0.0))                   # jst_emulator.GPU_PAIRS + the saturated switch
SMOOTHING = (0.5, 2)
SWEEP_MESHES = ("lattice_A", "tet")
DUAL_DT_QUANTILE = 0.5                               # the physical step: the clamp binds at half of the nodes
SUTHERLAND_S, PRANDTL_TURBULENT, FIELD_SEED, FIELD_MAX = 0.3831, 0.9, 11, 10.0  # variable_viscosity_emulator's


def isolated_level():
    """Eight nodes of which 1, 4 and 6 have no internal edge (tests/test_gpu_viscous.py::_isolated_level, the same seed)."""
    from mgcfd import meshgen
    rng = np.random.default_rng(4)
    internal = [(0, 5), (2, 5), (2, 7), (3, 7)]
    faces = [(-1, 4), (-2, 6), (-1, 5), (-2, 0), (-1, 2)]
    nel, lists = 8, [[] for _ in range(8)]
    for a, b in internal:
        w = rng.normal(size=3) * 1e-3
        lists[a].append((b, w))
        lists[b].append((a, -w))
    for code, node in faces:
        lists[node].append((code, rng.normal(size=3) * 1e-3))
    ptr = np.zeros(nel + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    return meshgen.LevelMesh(nel=nel, volumes=rng.uniform(1e-6, 2e-6, nel), coords=rng.random((nel, 3)), nbr_ptr=ptr,
                             nbr_idx=np.array([n for x in lists for n, _ in x], dtype=np.int64),
                             nbr_w=np.array([w for x in lists for _, w in x], dtype=np.float64).reshape(-1, 3))


def write_cases(directory):
    """{mesh: case directory} of MESHES (the emulators' kind: ``<dir>/input/input.dat`` and ``case.txt``)."""
    import fas_emulator as fe
    from mgcfd import meshgen
    out = {"lattice_A": fe.write_lattice("A", directory)}
    for name, level in (("tet", meshgen.make_tet_level(30000, seed=0, wall_below=2.0)),
                        ("hub", meshgen.make_hub_level(600, scale=1e-4, seed=5)), ("isolated", isolated_level())):
        mg = meshgen.MultigridMesh(mesh_name="fvcorr")
        mg.levels.append(level)
        d = os.path.join(str(directory), name)
        os.makedirs(os.path.join(d, "input"))
        meshgen.write_input(mg, os.path.join(d, "input"))
        with open(os.path.join(d, "case.txt"), "w") as f:
            f.write("duplicate = 1\n")
        out[name] = d
    return out


def start_state(mesh, nel, ff_var):
    from conftest import perturbed_state
    return perturbed_state(nel, ff_var, seed=STATE_SEED, amplitude=AMPLITUDE[mesh])


def ref_level(em, l=0):
    """The RefLevel of an emulator's level (its edge records are already adjusted and damped where the variant asks for it)."""
    L = em.oc.levels[l]
    assert (L.internal_start, L.boundary_start, L.wall_start) == (0, L.n_internal, L.n_internal + L.n_boundary)
    return RefLevel(L.nel, em.oc.edges(l).copy(), L.n_internal, L.n_boundary, L.n_wall, em.oc.array(l, "volumes").copy(), em.ff, em.variant)


def wall_nodes(level):
    s, n = level.span("wall")
    return np.unique(np.asarray(level.edges["b"][s:s + n], dtype=np.int64))


def ends(level):
    """(to, frm, N): per internal edge end the node, the other node and the normal seen from the node (+e at a, -e at b)."""
    e = level.edges
    s, n = level.span("internal")
    a, b = np.asarray(e["a"][s:s + n], dtype=np.int64), np.asarray(e["b"][s:s + n], dtype=np.int64)
    w = np.stack([e["x"][s:s + n], e["y"][s:s + n], e["z"][s:s + n]], axis=1).astype(LD)
    return np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([w, -w])


def _scatter(to, terms, nel):
    out = np.zeros((nel,) + terms.shape[1:], dtype=LD)
    np.add.at(out, to, terms)
    return out


# ------------------------------------------------------------------------------------------------------------------
# Viscous terms (§13, §16)
# ------------------------------------------------------------------------------------------------------------------
class Viscosity:
    """mu, the Prandtl number and the model of mgcfd_set_viscosity_model: ``law`` 0 constant, 1 Sutherland (t_ref, s);
    ``field`` the eddy-viscosity array of eddy mode 1, or None."""

    def __init__(self, mu, prandtl=PRANDTL, law=0, t_ref=1.0, s=SUTHERLAND_S, field=None, prandtl_t=PRANDTL_TURBULENT, cfl_v=VISCOUS_CFL):
        self.mu, self.prandtl, self.law = LD(np.float64(mu)), LD(np.float64(prandtl)), int(law)
        self.t_ref, self.s, self.prandtl_t, self.cfl_v = LD(np.float64(t_ref)), LD(np.float64(s)), LD(np.float64(prandtl_t)), LD(np.float64(cfl_v))
        self.field = None if field is None else np.asarray(field, dtype=np.float64).astype(LD)

    def node_viscosity(self, T, A_T):
        """(mu_i, A_mu): Sutherland's law mu * r sqrt(r) (1 + s) / (r + s), r = T / t_ref, has d ln mu / d ln T = 1.5 - r / (r + s),
        between 0.5 and 1.5."""
        if self.law == 0:
            m = np.full(len(T), self.mu, dtype=LD)
            return m, m.copy()
        r = T / self.t_ref
        m = ((self.mu * (r * np.sqrt(r))) * (LD(1.0) + self.s)) / (r + self.s)
        cond = np.maximum(LD(1.0), np.abs(LD(1.5) - r / (r + self.s)))
        return m, np.abs(m) * cond * (A_T / np.abs(T))

    def coefficients(self, T, A_T):
        """(me, A_me, kap, A_kap, mu_i): mu_i + mut and CP * (mu_i / prandtl + mut / prandtl_t)."""
        mu_i, A_mu = self.node_viscosity(T, A_T)
        mut = np.zeros(len(T), dtype=LD) if self.field is None else self.field
        me, A_me = mu_i + mut, A_mu + np.abs(mut)
        kap = CP * (mu_i / self.prandtl + mut / self.prandtl_t)
        A_kap = CP * (A_mu / self.prandtl + np.abs(mut) / self.prandtl_t)
        return me, A_me, kap, A_kap, mu_i


def primitives(q):
    """(phi, A_phi) [nel, 4] of (u, v, w, T = p / rho) with the reference's pressure, and rho."""
    q = np.asarray(q).astype(LD).reshape(-1, 5)
    rho, m, en = q[:, 0], q[:, 1:4], q[:, 4]
    v = m / rho[:, None]
    sq = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
    p = (GAMMA - LD(1.0)) * (en - LD(0.5) * rho * sq)
    A_p = (GAMMA - LD(1.0)) * (np.abs(en) + LD(0.5) * rho * sq)
    phi = np.concatenate([v, (p / rho)[:, None]], axis=1)
    A_phi = np.concatenate([np.abs(v), (A_p / rho)[:, None]], axis=1)
    return phi, A_phi, rho, p, A_p, np.sqrt(sq)


def gradients(level, phi, A_phi):
    """(G, A_G) [nel, n_phi, 3]: G = (0.5 * sum (phi_j - phi_i) n) / vol."""
    to, frm, N = ends(level)
    vol = level.volumes.astype(LD)[:, None, None]
    G = _scatter(to, (phi[frm] - phi[to])[:, :, None] * N[:, None, :], level.nel)
    A = _scatter(to, (A_phi[frm] + A_phi[to])[:, :, None] * np.abs(N)[:, None, :], level.nel)
    return (LD(0.5) * G) / vol, (LD(0.5) * A) / vol


def viscous_pass1(level, q, visc):
    """(S, A) [nel, 12] of the node stresses (u, v, w, txx, tyy, tzz, txy, txz, tyz, qx, qy, qz) and a dict of the
    intermediates ("G", "A_G", "mu", "div")."""
    phi, A_phi, rho, _, _, _ = primitives(q)
    G, AG = gradients(level, phi, A_phi)
    me, A_me, kap, A_kap, mu_i = visc.coefficients(phi[:, 3], A_phi[:, 3])
    ux, uy, uz, vx, vy, vz, wx, wy, wz = (G[:, i, d] for i in range(3) for d in range(3))
    aux, auy, auz, avx, avy, avz, awx, awy, awz = (AG[:, i, d] for i in range(3) for d in range(3))
    div = (ux + vy) + wz
    t, a_t = TWO_THIRDS * div, TWO_THIRDS * ((aux + avy) + awz)
    S, A = np.empty((level.nel, 12), dtype=LD), np.empty((level.nel, 12), dtype=LD)
    S[:, 0:3], A[:, 0:3] = phi[:, 0:3], A_phi[:, 0:3]
    for k, (g, ag) in enumerate(((ux, aux), (vy, avy), (wz, awz))):
        S[:, 3 + k], A[:, 3 + k] = me * (LD(2.0) * g - t), A_me * (LD(2.0) * ag + a_t)
    for k, (g1, g2, a1, a2) in enumerate(((uy, vx, auy, avx), (uz, wx, auz, awx), (vz, wy, avz, awy))):
        S[:, 6 + k], A[:, 6 + k] = me * (g1 + g2), A_me * (a1 + a2)
    S[:, 9:12], A[:, 9:12] = kap[:, None] * G[:, 3, :], A_kap[:, None] * AG[:, 3, :]
    return S, A, {"G": G, "A_G": AG, "mu": mu_i, "div": div}


def viscous_pass2(level, S, S_mag=None):
    """(V, A) [nel, 5] from the rows S [nel, 12]: as given they are exact (S_mag None: |S|); column 0 stays zero."""
    S = np.asarray(S).astype(LD).reshape(-1, 12)
    M = np.abs(S) if S_mag is None else np.asarray(S_mag).astype(LD)
    to, frm, N = ends(level)
    b, m = LD(0.5) * (S[to] + S[frm]), LD(0.5) * (M[to] + M[frm])
    u, v, w, txx, tyy, tzz, txy, txz, tyz, qx, qy, qz = (b[:, k] for k in range(12))
    mu_, mv, mw, mxx, myy, mzz, mxy, mxz, myz, mqx, mqy, mqz = (m[:, k] for k in range(12))
    nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
    ax, ay, az = np.abs(nx), np.abs(ny), np.abs(nz)
    terms, mags = np.zeros((len(to), 5), dtype=LD), np.zeros((len(to), 5), dtype=LD)
    terms[:, 1], mags[:, 1] = (txx * nx + txy * ny) + txz * nz, (mxx * ax + mxy * ay) + mxz * az
    terms[:, 2], mags[:, 2] = (txy * nx + tyy * ny) + tyz * nz, (mxy * ax + myy * ay) + myz * az
    terms[:, 3], mags[:, 3] = (txz * nx + tyz * ny) + tzz * nz, (mxz * ax + myz * ay) + mzz * az
    ex, mex = ((u * txx + v * txy) + w * txz) + qx, ((mu_ * mxx + mv * mxy) + mw * mxz) + mqx
    ey, mey = ((u * txy + v * tyy) + w * tyz) + qy, ((mu_ * mxy + mv * myy) + mw * myz) + mqy
    ez, mez = ((u * txz + v * tyz) + w * tzz) + qz, ((mu_ * mxz + mv * myz) + mw * mzz) + mqz
    terms[:, 4], mags[:, 4] = (ex * nx + ey * ny) + ez * nz, (mex * ax + mey * ay) + mez * az
    return _scatter(to, terms, level.nel), _scatter(to, mags, level.nel)


def onto(f0, S, A):
    """(f0 + S, |f0| + A): a launch's sums added onto the fluxes that were there."""
    f0 = np.asarray(f0).astype(LD).reshape(S.shape)
    return f0 + S, np.abs(f0) + A


def viscous_limit(level, q, visc):
    """The cap of the viscous step limit per node: (k0 * rho) * g, or ((cfl_v * rho) * g) / d under a model (§16)."""
    phi, A_phi, rho, _, _, _ = primitives(q)
    vol = level.volumes.astype(LD)
    cb = np.cbrt(vol)
    g = (cb * cb) / vol
    if visc.law == 0 and visc.field is None:
        kv = max(FOUR_THIRDS, GAMMA / visc.prandtl)
        return ((visc.cfl_v / (kv * visc.mu)) * rho) * g
    _, _, _, _, mu_i = visc.coefficients(phi[:, 3], A_phi[:, 3])
    mut = np.zeros(level.nel, dtype=LD) if visc.field is None else visc.field
    a = FOUR_THIRDS * (mu_i + mut)
    b = GAMMA * (mu_i / visc.prandtl + mut / visc.prandtl_t)
    return ((visc.cfl_v * rho) * g) / np.maximum(a, b)


# ------------------------------------------------------------------------------------------------------------------
# JST (§11)
# ------------------------------------------------------------------------------------------------------------------
def jst_sensor(level, q):
    """{"L": (L, A) [nel, 5], "nu": (nu, A) [nel], "r": (r, A) [nel]} of pass 1.  nu = |Pm| / Pp is a quotient of two sums of
    pressures, each with the magnitude of the reference's pressure expression; r = |v| + sqrt(GAMMA p / rho)."""
    W = np.asarray(q).astype(LD).reshape(-1, 5)
    _, _, rho, p, A_p, speed = primitives(W)
    to, frm, _ = ends(level)
    L, A_L = _scatter(to, W[frm] - W[to], level.nel), _scatter(to, np.abs(W[frm] - W[to]), level.nel)
    Pm, Pp = _scatter(to, p[frm] - p[to], level.nel), _scatter(to, p[frm] + p[to], level.nel)
    A_P = _scatter(to, A_p[frm] + A_p[to], level.nel)
    has = np.bincount(to, minlength=level.nel) > 0
    nu, A_nu = np.zeros(level.nel, dtype=LD), np.zeros(level.nel, dtype=LD)
    nu[has] = np.abs(Pm[has]) / Pp[has]
    A_nu[has] = (A_P[has] + nu[has] * A_P[has]) / np.abs(Pp[has])
    c = np.sqrt(GAMMA * p / rho)
    return {"L": (L, A_L), "nu": (nu, A_nu), "r": (speed + c, speed + c * (A_p / np.abs(p)))}


def jst_edge_weights(level):
    e = level.edges
    s, n = level.span("internal")
    x, y, z = (e[k][s:s + n].astype(LD) for k in "xyz")
    return -np.sqrt(x * x + y * y + z * z) * K_SMOOTHING * LD(0.5)


def jst_switches(nu_i, nu_j, kappa2, kappa4):
    nu = np.maximum(nu_i, nu_j)
    e2 = np.minimum(LD(np.float64(kappa2)) * nu, LD(1.0))
    return e2, np.maximum(LD(np.float64(kappa4)) - e2, LD(0.0))


def jst_correction(level, q, L, nu, r, kappa2, kappa4, L_mag=None, r_mag=None):
    """(C, A) [nel, 5] of pass 2 from the state and the L, nu, r GIVEN (as read back they are exact, and so is W: the
    differences W_i - W_j and L_i - L_j then carry their own absolute value; chained inside a sweep the magnitudes of L and r
    are given)."""
    W = np.asarray(q).astype(LD).reshape(-1, 5)
    L, nu, r = np.asarray(L).astype(LD).reshape(-1, 5), np.asarray(nu).astype(LD).ravel(), np.asarray(r).astype(LD).ravel()
    to, frm, _ = ends(level)
    k_e = np.tile(jst_edge_weights(level), 2)
    fac = k_e * (r[to] + r[frm])
    A_fac = np.abs(fac) if r_mag is None else np.abs(k_e) * (r_mag[to] + r_mag[frm])
    e2, e4 = jst_switches(nu[to], nu[frm], kappa2, kappa4)
    dW = np.abs(W[to] - W[frm])
    dL = np.abs(L[to] - L[frm]) if L_mag is None else L_mag[to] + L_mag[frm]
    terms = fac[:, None] * ((e2 - LD(1.0))[:, None] * (W[to] - W[frm]) - e4[:, None] * (L[to] - L[frm]))
    # e2 = kappa2 * nu is a rounded product: e2 - 1.0 and kappa4 - e2 are sums of two terms, each counted
    A_e4 = np.where(e4 > 0, LD(np.float64(kappa4)) + e2, LD(0.0))
    mags = A_fac[:, None] * ((e2 + LD(1.0))[:, None] * dW + A_e4[:, None] * dL)
    return _scatter(to, terms, level.nel), _scatter(to, mags, level.nel)


# ------------------------------------------------------------------------------------------------------------------
# One sweep with any of V, C, the dual-time source and residual smoothing (§9, §10)
# ------------------------------------------------------------------------------------------------------------------
class DualTime:
    """The physical step, the clamp, the BDF order and the two time levels [nel, 5] of mgcfd_set_dual_time.  (§10's source is
    explicit — the definition has no point-implicit factor; the clamp of the pseudo step stands in its place.)"""

    def __init__(self, dt, Wn, Wn1, order=2, clamp=2.0 / 3.0):
        self.dt, self.clamp, self.order = LD(np.float64(dt)), LD(np.float64(clamp)), int(order)
        self.Wn, self.Wn1 = np.asarray(Wn).astype(LD).reshape(-1, 5), np.asarray(Wn1).astype(LD).reshape(-1, 5)

    def source(self, level, W):
        """(src, A): vol * ((3 a - b) / (2 dt)) with a = W - Wn, b = Wn - Wn1, or vol * (a / dt) under BDF1."""
        vol = level.volumes.astype(LD)[:, None]
        a = W - self.Wn
        A_a = np.abs(a)
        if self.order == 1:
            return vol * (a / self.dt), vol * (A_a / self.dt)
        b = self.Wn - self.Wn1
        return vol * ((LD(3.0) * a - b) / (LD(2.0) * self.dt)), vol * ((LD(3.0) * A_a + np.abs(b)) / (LD(2.0) * self.dt))


def smoothed(level, D, A_D, eps, iterations):
    """(Db(M), A): Db(m) = (D + eps * sum over the internal edges at i of Db(m-1)[other end]) / (1 + eps * n_i)."""
    to, frm, _ = ends(level)
    eps = LD(np.float64(eps))
    den = (LD(1.0) + eps * np.bincount(to, minlength=level.nel).astype(LD))[:, None]
    Db, A = D, A_D
    for _ in range(iterations):
        Db, A = (D + eps * _scatter(to, Db[frm], level.nel)) / den, (A_D + eps * _scatter(to, A[frm], level.nel)) / den
    return Db, A


def sweep(level, q, mode="reference", cfl=0.5, viscous=None, wall=False, jst=None, smoothing=None, dual=None):
    """far.sweep() with a stage's sum F plus any of C (``jst`` = (kappa2, kappa4)), V (``viscous`` a Viscosity; ``wall``: the
    no-slip rule behind every stage), minus the dual-time source (``dual`` a DualTime) and with ``smoothing`` = (eps, M) Jacobi
    iterations in place of the plain update.  D accumulates |sf / rk_div_j| * A_j of every stage as far.sweep's does (smoothed,
    the Jacobi iterations are applied to the magnitudes with the same positive weights); as there, a stage takes the state it starts from as
    its exact input.  With every option off the operations
    are far.sweep's own, in its order: tests/test_host_fast_physics.py asserts the same long-double bits."""
    old = np.asarray(q).astype(LD).reshape(-1, 5)
    sf = far.step_factor(level, old, mode, cfl)
    if viscous is not None:
        sf = np.minimum(sf, viscous_limit(level, old, viscous))
    if dual is not None:
        sf = np.minimum(sf, (dual.clamp * dual.dt) / level.volumes.astype(LD))
    walls = wall_nodes(level) if (viscous is not None and wall) else None
    W, D, valid = old, np.abs(old), True
    for j in range(RK):
        S, A = far.accumulate(far.class_sums(level, W), CLASSES)
        if jst is not None:
            s = jst_sensor(level, W)
            C_, A_C = jst_correction(level, W, s["L"][0], s["nu"][0], s["r"][0], jst[0], jst[1], L_mag=s["L"][1], r_mag=s["r"][1])
            S, A = S + C_, A + A_C
        if viscous is not None:
            rows, rows_mag, _ = viscous_pass1(level, W, viscous)
            V, A_V = viscous_pass2(level, rows, rows_mag)
            S, A = S + V, A + A_V
        if dual is not None:
            src, A_src = dual.source(level, W)
            S, A = S - src, A + A_src
        if smoothing is not None:
            Db, A_Db = smoothed(level, sf[:, None] * S, np.abs(sf)[:, None] * A, *smoothing)
            W = old + Db / LD(RK + 1 - j)
            D = D + A_Db / LD(RK + 1 - j)
        else:
            fac = sf / LD(RK + 1 - j)
            W = old + fac[:, None] * S
            D = D + np.abs(fac)[:, None] * A
        valid = valid and bool(np.isfinite(W).all() and (W[:, 0] >= 0).all() and (W[:, 4] >= 0).all())
        if walls is not None:
            W = W.copy()
            W[walls, 1:4] = LD(0.0)
    return {"sf": sf, "W": W, "res": W - old, "D": D, "valid": valid}


# ------------------------------------------------------------------------------------------------------------------
# Numpy models of faulty kernels (tests/test_host_fast_physics.py): applied to the emulator's double output
# ------------------------------------------------------------------------------------------------------------------
def old_metric(got, want):
    """The whole-array metric of the test_fast_mode tests: max |difference| / max |value|."""
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max() / max(np.abs(want).max(), 1e-300))


def k_bound(k_ref):
    """3 * max(K_ref, 1) per component."""
    return MARGIN * np.maximum(np.atleast_1d(np.asarray(k_ref, dtype=np.float64)), 1.0)


# ------------------------------------------------------------------------------------------------------------------
# Transfers (§12, §15): the weighted sums of the FAS restriction and of the prolongations, each on the launch's own input
# ------------------------------------------------------------------------------------------------------------------
def restrict_state(parent, W_fine, W_coarse_before):
    """(S, A) of the restricted state: the mean over a coarse node's children (the sum times 1 / count); a coarse node without
    children keeps what it held (A = 0 there: K demands that value exactly)."""
    Wf = np.asarray(W_fine).astype(LD).reshape(-1, 5)
    before = np.asarray(W_coarse_before).astype(LD).reshape(-1, 5)
    count = np.bincount(parent, minlength=len(before))
    has = count > 0
    avg = LD(1.0) / np.maximum(count, 1).astype(LD)
    S, A = _scatter(parent, Wf, len(before)) * avg[:, None], _scatter(parent, np.abs(Wf), len(before)) * avg[:, None]
    S[~has], A[~has] = before[~has], LD(0.0)
    return S, A


def restrict_forcing(parent, T_fine, R_coarse):
    """(P, A): Q - R_{l+1}(W0) with Q the children's summed total residual; exactly +0.0 (A = 0) without children."""
    T, R = np.asarray(T_fine).astype(LD).reshape(-1, 5), np.asarray(R_coarse).astype(LD).reshape(-1, 5)
    has = np.bincount(parent, minlength=len(R)) > 0
    S, A = _scatter(parent, T, len(R)) - R, _scatter(parent, np.abs(T), len(R)) + np.abs(R)
    S[~has], A[~has] = LD(0.0), LD(0.0)
    return S, A


class Interpolation:
    """wavg_i of mgcfd_prolong (prolong_residuals_interpolate_proper, mg_loops.cpp:730-851) for the internal edges (a2, b2) of a
    fine level: a node that coincides with its parent takes the parent's value; every other node the inverse-distance weighted
    mean of, per edge at its a end, its own parent and the other end's parent and, per edge at its b end, its own parent twice
    (the reference's b-end quirk: the second weight is the distance to the a end's parent, the value still the own parent's)."""

    def __init__(self, level_fine, parent, coords_fine, coords_coarse):
        e = level_fine.edges
        s, n = level_fine.span("internal")
        a2, b2 = np.asarray(e["a"][s:s + n], dtype=np.int64), np.asarray(e["b"][s:s + n], dtype=np.int64)
        parent = np.asarray(parent, dtype=np.int64)
        cf, cc = np.asarray(coords_fine, dtype=np.float64).reshape(-1, 3), np.asarray(coords_coarse, dtype=np.float64).reshape(-1, 3)
        a1, b1 = parent[a2], parent[b2]

        def inv_dist(p, q):
            d = p.astype(LD) - q.astype(LD)
            return LD(1.0) / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])

        self.nel = level_fine.nel
        self.coincident = (cf == cc[parent]).all(axis=1)
        self.parent = parent
        with np.errstate(divide="ignore"):
            self.to = np.concatenate([a2, a2, b2, b2])
            self.frm = np.concatenate([a1, b1, b1, b1])
            self.w = np.concatenate([inv_dist(cf[a2], cc[a1]), inv_dist(cc[b1], cf[a2]), inv_dist(cf[b2], cc[b1]), inv_dist(cc[a1], cf[b2])])
        keep = ~self.coincident[self.to]
        self.to, self.frm, self.w = self.to[keep], self.frm[keep], self.w[keep]
        self.w_sum = _scatter(self.to, self.w, self.nel)
        self.has_edge = np.bincount(np.concatenate([a2, b2]), minlength=self.nel) > 0

    def __call__(self, X):
        """(wavg, A) [nel_fine, 5] of the coarse values X [nel_coarse, 5]."""
        X = np.asarray(X).astype(LD).reshape(-1, 5)
        S = _scatter(self.to, self.w[:, None] * X[self.frm], self.nel)
        A = _scatter(self.to, self.w[:, None] * np.abs(X[self.frm]), self.nel)
        free = ~self.coincident
        S[free], A[free] = S[free] / self.w_sum[free][:, None], A[free] / self.w_sum[free][:, None]
        S[self.coincident], A[self.coincident] = X[self.parent[self.coincident]], np.abs(X[self.parent[self.coincident]])
        return S, A


def fas_correction(interp, W_fine, W0, W_coarse):
    """(S, A) of the up leg: variables[l] + (0.0 - wavg(W0 - variables[l+1]))."""
    Wf = np.asarray(W_fine).astype(LD).reshape(-1, 5)
    D = np.asarray(W0).astype(LD).reshape(-1, 5) - np.asarray(W_coarse).astype(LD).reshape(-1, 5)
    wavg, A = interp(D)
    return Wf - wavg, np.abs(Wf) + A


def emulated_wavg(em, fine, X):
    """wavg(X) [nel_fine, 5] in double with the oracle's own prolongation (the emulators' way: residuals1 = X, residuals2 = +0.0,
    variables = +0.0, so that the call leaves 0.0 - wavg); the emulator's arrays are restored."""
    L = em.oc.levels
    res_c, res_f, var = em.oc.array(fine + 1, "residuals"), em.oc.array(fine, "residuals"), em.oc.array(fine, "variables")
    keep = res_c.copy(), res_f.copy(), var.copy()
    res_c[:], res_f[:], var[:] = np.asarray(X, dtype=np.float64).ravel(), 0.0, 0.0
    em.lib.ora_prolong_residuals_interpolate_proper(L[fine].edges, L[fine].n_internal, L[fine + 1].residuals, L[fine].residuals,
                                                    L[fine].variables, L[fine].nel, L[fine].mg_map, L[fine + 1].coords, L[fine].coords)
    out = 0.0 - var.reshape(-1, 5)
    res_c[:], res_f[:], var[:] = keep
    return out


def emulated_restriction(em, fine, W_fine, W_coarse_before):
    """mg_restrict of a given fine state in double (the oracle's entry point); the emulator's arrays are restored."""
    L = em.oc.levels
    vf, vc = em.oc.array(fine, "variables"), em.oc.array(fine + 1, "variables")
    keep = vf.copy(), vc.copy()
    vf[:], vc[:] = np.asarray(W_fine, dtype=np.float64).ravel(), np.asarray(W_coarse_before, dtype=np.float64).ravel()
    em.lib.ora_mg_restrict(L[fine].variables, L[fine + 1].variables, L[fine + 1].nel, L[fine].mg_map, em.O.ptr(em.scratch), L[fine].mgc)
    out = vc.reshape(-1, 5).copy()
    vf[:], vc[:] = keep
    return out


def emulated_forcing(parent, T_fine, R_coarse):
    """fas_emulator.FasOracle.fas_restrict's steps 3 and 4 in double on given T and R(W0)."""
    T, R = np.asarray(T_fine, dtype=np.float64).reshape(-1, 5), np.asarray(R_coarse, dtype=np.float64).reshape(-1, 5)
    Q = np.zeros_like(R)
    np.add.at(Q, parent, T)
    return np.where((np.bincount(parent, minlength=len(R)) > 0)[:, None], Q - R, 0.0)


# ------------------------------------------------------------------------------------------------------------------
# The emulators' own double evaluation of the same things, on the same input: what sets K_ref
# ------------------------------------------------------------------------------------------------------------------
def make_emulator(oracle, case, mesh, fas=False):
    """The composed emulator (variable_viscosity_emulator.VariableViscosityOracle: viscous, JST, dual time, smoothing and FAS
    below it) under local steps at the mesh's CFL number, everything off, level 0 at the start state."""
    import variable_viscosity_emulator as vve
    em = vve.VariableViscosityOracle(oracle, case, "local", LOCAL_CFL[mesh], fas=fas)
    em._var(0)[:] = start_state(mesh, em.oc.levels[0].nel, em.ff17[:5])
    return em


def eddy_field(mu, nel):
    """variable_viscosity_emulator.eddy_field of level 0."""
    return np.float64(mu) * np.random.default_rng(FIELD_SEED).uniform(0.0, FIELD_MAX, nel)


def viscous_setup(em, mesh, variable=False, mu=None):
    """Switches the viscous terms on (no-slip walls, level 0) and, ``variable``, Sutherland's law with the far field's t_ref
    plus the eddy-viscosity field; returns (the state with the wall rule applied, the Viscosity of the reference, the field)."""
    import variable_viscosity_emulator as vve
    mu = MU[mesh] if mu is None else mu
    em.set_viscous(mu, PRANDTL, 1, VISCOUS_CFL, 1)
    if not variable:
        em.set_viscosity_model()
        return em.variables(0), Viscosity(mu), None
    field = eddy_field(mu, em.oc.levels[0].nel)
    em.set_viscosity_model(law="sutherland", eddy="field")
    em.set_eddy_viscosity(0, field)
    return em.variables(0), Viscosity(mu, law=1, t_ref=vve.far_field_t_ref(em.ff17), field=field), field


def emulated_viscous_flux(em, S, l=0):
    import viscous_emulator as ve
    return ve.viscous_flux(np.asarray(S, dtype=np.float64), em.vto[l], em.vfrm[l], em.vN[l])


def emulated_correction(em, W, L, nu, r, kappa2, kappa4, l=0):
    """jst_emulator's pass 2 on given L, nu and r: C [nel, 5]."""
    import jst_emulator as jse
    a, b = em.ea[l], em.eb[l]
    c_ab, c_ba = jse.edge_terms(W, np.asarray(L, dtype=np.float64), np.asarray(nu, dtype=np.float64), np.asarray(r, dtype=np.float64),
                                a, b, em.k_e[l], kappa2, kappa4)
    to = np.empty(2 * len(a), dtype=np.int64)
    to[0::2], to[1::2] = a, b
    terms = np.empty((2 * len(a), 5))
    terms[0::2], terms[1::2] = c_ab, c_ba
    Cn = np.zeros((em.oc.levels[l].nel, 5))
    np.add.at(Cn, to, terms)
    return Cn


SWEEP_OPTIONS = ("viscous", "jst", "smoothing", "dual")


def dual_time_levels(em, mesh):
    """(dt, Wn, Wn1): the physical step at which the clamp binds on half of level 0's nodes at the start state (the median of
    sf * vol / clamp, two digits), and two time levels distinct from the state (the start state's recipe, other seeds)."""
    import dual_time_emulator as dte
    import time_step_emulator as tse
    from conftest import perturbed_state
    vol = em.oc.array(0, "volumes")
    free = tse.step_factors("local", LOCAL_CFL[mesh], start_state(mesh, len(vol), em.ff17[:5]), vol, em.cbrt_vol[0], em.variant)
    dt = float("%.2g" % np.quantile(free * vol / dte.CLAMP, DUAL_DT_QUANTILE))
    Wn, Wn1 = (perturbed_state(len(vol), em.ff17[:5], seed=STATE_SEED + k, amplitude=AMPLITUDE[mesh]) for k in (1, 2))
    return dt, Wn, Wn1


def sweep_setup(em, mesh, options, order=2):
    """Configures the emulator for one sweep of level 0 with ``options`` (a subset of SWEEP_OPTIONS; ``order``: dual time's BDF
    order) and returns (the state the sweep starts from, the keywords of ``sweep``, the settings as the solver takes them)."""
    kw, settings = {}, {}
    if "viscous" in options:
        _, kw["viscous"], _ = viscous_setup(em, mesh)
        kw["wall"] = True
        settings["viscous"] = (MU[mesh], PRANDTL, True, VISCOUS_CFL, 1)
    if "jst" in options:
        em.set_jst(*JST_PAIRS[0], 1)
        kw["jst"] = settings["jst"] = JST_PAIRS[0]
    if "smoothing" in options:
        em.set_residual_smoothing(*SMOOTHING)
        kw["smoothing"] = settings["smoothing"] = SMOOTHING
    if "dual" in options:
        dt, Wn, Wn1 = dual_time_levels(em, mesh)
        em.set_dual_time(dt)
        em.set_order(order)
        em.set_time_levels(0, Wn, Wn1)
        kw["dual"] = DualTime(dt, Wn, Wn1, order=order, clamp=em.clamp)
        settings["dual"] = (dt, Wn, Wn1)
    return em.variables(0), kw, settings


def emulated_sweep(em):
    """One sweep of level 0 on the emulator: (rc, {"W", "res", "sf"})."""
    rc = em.sweeps(0, 1)
    return rc, {"W": em.variables(0), "res": em.oc.array(0, "residuals").reshape(-1, 5).copy(), "sf": em.step_factors(0)}


def transfer_setup(em, mesh):
    """The inputs of the transfer checks on a hierarchy's levels 0 and 1: the fine start state, the coarse level's state before
    the restriction (the far field), the map, the interpolation, and the coarse state the up leg starts from (the start
    state's recipe on level 1, another seed: distinct from W0, so that the correction is of the perturbation's size)."""
    from conftest import perturbed_state
    n1 = em.oc.levels[1].nel
    parent = np.asarray(em.oc.mg_map(0), dtype=np.int64).copy()
    assert len(parent) == em.oc.levels[0].nel
    interp = Interpolation(ref_level(em, 0), parent, em.oc.array(0, "coords"), em.oc.array(1, "coords"))
    return {"W_fine": em.variables(0), "coarse_before": em.variables(1), "parent": parent, "interp": interp,
            "W_coarse": perturbed_state(n1, em.ff17[:5], seed=STATE_SEED + 3, amplitude=AMPLITUDE[mesh])}
