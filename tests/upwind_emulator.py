"""The yardstick of the upwind flux (mgcfd_set_upwind): ``UpwindOracle``, the composed oracle of tests/cycle_emulator.py (and so of
the viscous, FAS, JST, dual-time, residual-smoothing and time-step emulators below it) with limited MUSCL reconstruction and
Roe's flux written in numpy from the definition in include/mgcfd.h / INTEGRATION.md §23.  The wall and far-field fluxes, every
transfer and residual stay the oracle's entry points.

On an upwind level the oracle's internal flux call is a no-op and ``U`` is added behind the far-field call — before JST's and
the viscous wrappers add theirs — so that a stage's fluxes are ``F = B + U`` (+ V ...).  Per edge end (node i, other node j,
normal n seen from i), in the order (a0, b0, a1, b1, ...) of the level's internal edges, q = (rho, u, v, w, p):

    pass 1   G = Green-Gauss on q (viscous_emulator.gradients);  qmax, qmin over q_i and the q_j
             d2 = 0.5 * ((G[v][0]*dx + G[v][1]*dy) + G[v][2]*dz),  dx = x_j - x_i;  d1 = qmax - q_i (d2 > 0) | qmin - q_i (d2 < 0)
             Barth-Jespersen t = min(1, d1/d2);  Venkatakrishnan t = ((d1*d1 + e2)*d2 + ((2*d2)*d2)*d1) / (d2*(((d1*d1 + (2*d2)*d2) + d1*d2) + e2))
             psi = min over the ends from 1.0;  Gl = psi * G
    pass 2   qL = q_i + 0.5*(Gl_i . dx);  qR = q_j - 0.5*(Gl_j . dx);  first order where a density or pressure is not > 0
             s = sign of the first non-zero component of n;  m = s*n;  (qa, qb) = (qL, qR) if s > 0 else (qR, qL)
             U_i = U_i - s * Phi(qa, qb, m)          from +0.0, one addition per end, in edge order

Every numpy operation is one IEEE-754 double operation per element; ``np.add.at`` is unbuffered and adds in index order.  The
extrema and the limiter's minimum are taken by comparison in the ends' order (``ranked``), as the kernels take them, so that a
tie between +0.0 and -0.0 falls the same way.  While level 0 is an upwind level the RMS of a cycle is summed in dual time
stepping's fixed order.  ``levels = 0`` is ``CycleOracle`` itself (tests/test_host_upwind.py checks the bits).
"""
import numpy as np

import cycle_emulator as ce
import dual_time_emulator as dte
import fas_emulator as fe
import jst_emulator as jse
import viscous_emulator as ve

GAMMA = 1.4
NONE, BARTH_JESPERSEN, VENKATAKRISHNAN = 0, 1, 2
LIMITERS = {"none": NONE, "barth-jespersen": BARTH_JESPERSEN, "venkatakrishnan": VENKATAKRISHNAN}
VENKAT_K, ENTROPY_FIX = 5.0, 0.1                 # MGCFD_UPWIND_VENKAT_K, MGCFD_UPWIND_ENTROPY_FIX
ARR_UPWIND_GRADIENT, ARR_UPWIND_LIMITER = 25, 26

# ---- what the GPU tests run (tests/test_gpu_upwind.py); tests/test_host_upwind.py asserts on the CPU that every run below stays
# valid for its cycles and that LOCAL_CFL is the largest of LOCAL_CFLS at which all do ----
GPU_LATTICES = ("A", "B")
GPU_GOLDENS = ("tet_2lvl", "mixed_2lvl")
GPU_CASES = GPU_LATTICES + GPU_GOLDENS
GPU_CYCLES = 3
LOCAL_CFLS = (0.5, 1.0, 1.5)
LOCAL_CFL = 1.0
GPU_STEPS = (("reference", 0.5), ("local", LOCAL_CFL))
GPU_LEVELS = (1, "all")
GPU_MUSCL = (0, 1, "all")
GPU_LIMITERS = ("none", "barth-jespersen", "venkatakrishnan")
RUN_LIMITER = "venkatakrishnan"
START_SEED, START_AMPLITUDE = 7, 0.01
SUPERSONIC_MACH = 2.0
# the composed runs, all on lattice A with the upwind flux (Venkatakrishnan) on all levels, MUSCL on level 0:
# (name, mode, cfl, (eps, iterations), BDF order or None, FAS, viscous, cycle)
COMPOSED = (("smoothing", "local", 2.0, (0.5, 2), None, False, False, None),
            ("dual_bdf2", "local", 0.5, (0.0, 0), 2, False, False, None),
            ("fas", "local", 1.0, (0.0, 0), None, True, False, None),
            ("viscous", "local", 1.0, (0.0, 0), None, False, True, None),
            ("cycle", "local", 0.5, (0.0, 0), None, False, False, ("W", 1)))
DUAL_STEPS, DUAL_CYCLES = 2, 3
# the unsmoothed composed runs' local CFL is the largest of these at which the run stays valid on the emulator: at 1.0 the
# dual-time run goes invalid in its second step and the W cycle in the post-sweep of its third cycle
COMPOSED_CFLS = (0.5, 1.0)
# ... and the smoothed run's of these (residual smoothing is there to raise the CFL number: at 2.5 the run goes invalid)
SMOOTHED_CFLS = (1.5, 2.0, 2.5)
# ("reference", 0.5) has no candidates: the mode is the reference's own step with the literal 0.5 it hard-codes, tested as it is)


def gpu_runs():
    """(case, mode, cfl, levels, muscl) of the whole runs; muscl <= levels."""
    out = []
    for case in GPU_CASES:
        for mode, cfl in GPU_STEPS:
            for lv in GPU_LEVELS:
                for m in GPU_MUSCL:
                    if lv == 1 and m == "all":
                        continue                             # (the same run as muscl = 1)
                    out.append((case, mode, cfl, lv, m))
    return out


def start_state(nel, ff_var):
    from conftest import perturbed_state
    return perturbed_state(nel, ff_var, START_SEED, START_AMPLITUDE)


def supersonic_state(nel, ff_var):
    """The perturbed start state with its momentum scaled to about Mach 2 (the energy follows, the pressure stays)."""
    W = start_state(nel, ff_var)
    p = jse.pressure(W)
    c = np.sqrt(GAMMA * p / W[:, 0])
    speed = np.sqrt((W[:, 1:4] ** 2).sum(axis=1)) / W[:, 0]
    W[:, 1:4] *= (SUPERSONIC_MACH * c / speed)[:, None]
    W[:, 4] = p / (GAMMA - 1.0) + 0.5 * (W[:, 1:4] ** 2).sum(axis=1) / W[:, 0]
    return W


# ---- the definition ----
def primitives5(W):
    """q = (rho, u, v, w, p) [nel, 5] of a state [nel, 5]."""
    W = np.asarray(W, dtype=np.float64).reshape(-1, 5)
    rho = W[:, 0]
    with np.errstate(all="ignore"):
        return np.stack([rho, W[:, 1] / rho, W[:, 2] / rho, W[:, 3] / rho, jse.pressure(W)], axis=1)


def ranked(to):
    """Per edge end its rank among the ends of its node, in order: the rounds in which a sequential walk visits them."""
    order = np.argsort(to, kind="stable")
    sorted_to = to[order]
    first = np.r_[0, np.nonzero(np.diff(sorted_to))[0] + 1]
    start = np.repeat(first, np.diff(np.r_[first, len(to)]))
    rank = np.empty(len(to), dtype=np.int64)
    rank[order] = np.arange(len(to)) - start
    return [np.nonzero(rank == r)[0] for r in range(int(rank.max()) + 1 if len(to) else 0)]


def dot3(g, dx):
    return (g[..., 0] * dx[..., 0] + g[..., 1] * dx[..., 1]) + g[..., 2] * dx[..., 2]


def gradient_pass(q, X, to, frm, N, vol, limiter, k, rounds=None):
    """Pass 1: (Gl [nel, 5, 3], psi [nel, 5], G [nel, 5, 3], qmin, qmax)."""
    rounds = ranked(to) if rounds is None else rounds
    vol = np.asarray(vol, dtype=np.float64)
    with np.errstate(all="ignore"):
        G = ve.gradients(q, to, frm, N, vol)
        qmax, qmin = q.copy(), q.copy()
        for sel in rounds:
            i, o = to[sel], q[frm[sel]]
            qmax[i] = np.where(o > qmax[i], o, qmax[i])
            qmin[i] = np.where(o < qmin[i], o, qmin[i])
        psi = np.ones_like(q)
        if limiter != NONE:
            dx = X[frm] - X[to]
            d2 = 0.5 * dot3(G[to], dx[:, None, :])
            d1 = np.where(d2 > 0.0, qmax[to], qmin[to]) - q[to]
            if limiter == BARTH_JESPERSEN:
                r = d1 / d2
                t = np.where(r < 1.0, r, 1.0)
            else:
                e2 = (((np.float64(k) * np.float64(k)) * np.float64(k)) * vol)[to][:, None]
                d11, d22 = d1 * d1, (2.0 * d2) * d2
                t = ((d11 + e2) * d2 + d22 * d1) / (d2 * (((d11 + d22) + d1 * d2) + e2))
            t = np.where((d2 > 0.0) | (d2 < 0.0), t, 1.0)
            for sel in rounds:
                i = to[sel]
                psi[i] = np.where(t[sel] < psi[i], t[sel], psi[i])
        return psi[:, :, None] * G, psi, G, qmin, qmax


def reconstruct(q, Gl, X, to, frm):
    """(qL, qR, fallback) per edge end; Gl None: first order."""
    qL, qR = q[to].copy(), q[frm].copy()
    if Gl is None:
        return qL, qR, np.zeros(len(to), dtype=bool)
    with np.errstate(all="ignore"):
        dx = (X[frm] - X[to])[:, None, :]
        rL = q[to] + 0.5 * dot3(Gl[to], dx)
        rR = q[frm] - 0.5 * dot3(Gl[frm], dx)
        ok = (rL[:, 0] > 0.0) & (rL[:, 4] > 0.0) & (rR[:, 0] > 0.0) & (rR[:, 4] > 0.0)
    return np.where(ok[:, None], rL, qL), np.where(ok[:, None], rR, qR), ~ok


def normal_flux(q, nh):
    """(Fn [n, 5], un, H) of the states q through the unit normals nh."""
    rho, u, v, w, p = (q[:, k] for k in range(5))
    un = (u * nh[:, 0] + v * nh[:, 1]) + w * nh[:, 2]
    E = p / (GAMMA - 1.0) + (0.5 * rho) * ((u * u + v * v) + w * w)
    ru = rho * un
    F = np.stack([ru, ru * u + p * nh[:, 0], ru * v + p * nh[:, 1], ru * w + p * nh[:, 2], (E + p) * un], axis=1)
    return F, un, (E + p) / rho


def roe(qa, qb, m, entropy_fix, parts=False):
    """Phi(qa, qb, m) [n, 5]; with ``parts`` also (area, Fn_a, Fn_b, D)."""
    with np.errstate(all="ignore"):
        area = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        nh = m / area[:, None]
        Fa, una, Ha = normal_flux(qa, nh)
        Fb, unb, Hb = normal_flux(qb, nh)
        ra, rb = np.sqrt(qa[:, 0]), np.sqrt(qb[:, 0])
        den = ra + rb
        ut, vt, wt = ((ra * qa[:, k] + rb * qb[:, k]) / den for k in (1, 2, 3))
        Ht = (ra * Ha + rb * Hb) / den
        q2 = (ut * ut + vt * vt) + wt * wt
        c2 = (GAMMA - 1.0) * (Ht - 0.5 * q2)
        ct = np.sqrt(c2)
        unt = (ut * nh[:, 0] + vt * nh[:, 1]) + wt * nh[:, 2]
        rt = ra * rb
        drho, du, dv, dw, dp = (qb[:, k] - qa[:, k] for k in range(5))
        dun = (du * nh[:, 0] + dv * nh[:, 1]) + dw * nh[:, 2]
        l1, l2, l3 = np.abs(unt - ct), np.abs(unt), np.abs(unt + ct)
        d = np.float64(entropy_fix) * (l2 + ct)
        dd, d2 = d * d, 2.0 * d
        l1 = np.where(l1 < d, (l1 * l1 + dd) / d2, l1)
        l3 = np.where(l3 < d, (l3 * l3 + dd) / d2, l3)
        l2 = np.where(l2 < d, (l2 * l2 + dd) / d2, l2)
        rc, t2c = rt * ct, 2.0 * c2
        a1, a2, a3 = (dp - rc * dun) / t2c, drho - dp / c2, (dp + rc * dun) / t2c
        k1, k2, ks, k3 = l1 * a1, l2 * a2, l2 * rt, l3 * a3
        D = np.empty_like(Fa)
        D[:, 0] = (k1 + k2) + k3
        for col, (vel, dvel) in enumerate(((ut, du), (vt, dv), (wt, dw))):
            h = nh[:, col]
            D[:, 1 + col] = ((k1 * (vel - ct * h) + k2 * vel) + ks * (dvel - dun * h)) + k3 * (vel + ct * h)
        D[:, 4] = ((k1 * (Ht - ct * unt) + k2 * (0.5 * q2)) + ks * (((ut * du + vt * dv) + wt * dw) - unt * dun)) + k3 * (Ht + ct * unt)
        Phi = area[:, None] * (0.5 * (Fa + Fb) - 0.5 * D)
        Phi = np.where((area == 0.0)[:, None], 0.0, Phi)
    return (Phi, area, Fa, Fb, D) if parts else Phi


def orientation(N):
    """pos [2E]: s = +1 (the first non-zero component of n is positive)."""
    nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
    return np.where(nx != 0.0, nx > 0.0, np.where(ny != 0.0, ny > 0.0, nz > 0.0))


def edge_terms(qL, qR, N, entropy_fix):
    """The ends' additions to U [2E, 5]: -s * Phi(qa, qb, s*n)."""
    pos = orientation(N)
    qa, qb = np.where(pos[:, None], qL, qR), np.where(pos[:, None], qR, qL)
    Phi = roe(qa, qb, np.where(pos[:, None], N, -N), entropy_fix)
    return np.where(pos[:, None], -Phi, Phi)


def upwind_sum(W, X, to, frm, N, vol, muscl, limiter, k, entropy_fix, rounds=None):
    """(U [nel, 5], Gl or None, psi or None, terms [2E, 5], fallback [2E]) of one stage from its input state."""
    q = primitives5(W)
    Gl = psi = None
    if muscl:
        Gl, psi, _, _, _ = gradient_pass(q, X, to, frm, N, vol, limiter, k, rounds)
    qL, qR, fb = reconstruct(q, Gl, X, to, frm)
    terms = edge_terms(qL, qR, N, entropy_fix)
    U = np.zeros((len(q), 5))
    with np.errstate(all="ignore"):
        np.add.at(U, to, terms)
    return U, Gl, psi, terms, fb


class _UpwindLib:
    """The oracle library, innermost of the wrappers: on upwind levels the internal flux call does nothing and U follows the
    far-field faces; while level 0 is an upwind level calc_rms runs in the fixed order.  Everything else passes through."""

    def __init__(self, lib, owner):
        self._lib, self._owner = lib, owner

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def _level_of(self, fluxes):
        em = self._owner
        for l in range(min(em.up_levels, em.n)):
            if em.oc.levels[l].fluxes == fluxes:
                return l
        return None

    def ora_compute_flux_edge(self, start, n, edges, variables, fluxes):
        if self._level_of(fluxes) is not None:
            return 0
        return self._lib.ora_compute_flux_edge(start, n, edges, variables, fluxes)

    def ora_compute_wall_flux_edge(self, start, n, edges, variables, fluxes, ff):
        rc = self._lib.ora_compute_wall_flux_edge(start, n, edges, variables, fluxes, ff)
        l = self._level_of(fluxes)
        if l is not None:
            assert self._owner.oc.levels[l].variables == variables
            self._owner.add_upwind(l)
        return rc

    def ora_calc_rms(self, nel, residuals):
        em = self._owner
        if em.up_levels == 0:
            return self._lib.ora_calc_rms(nel, residuals)
        assert residuals == em.oc.levels[0].residuals
        return float(np.sqrt(dte.ordered_sumsq(em.oc.array(0, "residuals")) / np.float64(nel)))


class UpwindOracle(ce.CycleOracle):
    """CycleOracle with the settings of mgcfd_set_upwind."""

    def __init__(self, *args, **kwargs):
        self.up_levels = self.up_muscl = 0
        super().__init__(*args, **kwargs)
        w = self.lib
        while not isinstance(w, jse._JstFluxes):             # below JST's wrapper: U comes before C and V
            w = w._lib
        w._lib = _UpwindLib(w._lib, self)
        self.X = [self.oc.array(l, "coords").reshape(-1, 3).copy() for l in range(self.n)]
        self.rounds = [None] * self.n
        self.last_U, self.last_Gl, self.last_psi = [None] * self.n, [None] * self.n, [None] * self.n
        self.fallbacks = [0] * self.n
        self.limiter, self.k, self.entropy_fix = NONE, 0.0, 0.0

    def set_upwind(self, levels=1, muscl_levels=None, limiter="venkatakrishnan", k=VENKAT_K, entropy_fix=ENTROPY_FIX):
        levels = self.n if levels == "all" else int(levels)
        muscl = levels if muscl_levels is None else (self.n if muscl_levels == "all" else int(muscl_levels))
        limiter = LIMITERS.get(limiter, limiter)
        assert 0 <= muscl <= levels and limiter in (NONE, BARTH_JESPERSEN, VENKATAKRISHNAN)
        assert np.isfinite(k) and k > 0.0 and np.isfinite(entropy_fix) and 0.0 <= entropy_fix <= 1.0
        assert levels == 0 or self.jst_levels == 0
        self.up_levels = min(levels, self.n)
        self.up_muscl = min(muscl, self.up_levels)
        on = self.up_levels > 0
        self.limiter, self.k, self.entropy_fix = (limiter, float(k), float(entropy_fix)) if on else (NONE, 0.0, 0.0)

    def upwind_terms(self, l, W=None):
        """upwind_sum of level ``l`` for the state ``W`` (default: its current variables)."""
        W = self._var(l) if W is None else W
        if self.rounds[l] is None:
            self.rounds[l] = ranked(self.vto[l])
        return upwind_sum(W, self.X[l], self.vto[l], self.vfrm[l], self.vN[l], self.oc.array(l, "volumes"), l < self.up_muscl,
                          self.limiter, self.k, self.entropy_fix, self.rounds[l])

    def add_upwind(self, l):
        U, Gl, psi, _, fb = self.upwind_terms(l)
        self.last_U[l], self.last_Gl[l], self.last_psi[l] = U, Gl, psi
        self.fallbacks[l] += int(fb.sum())
        fluxes = self.oc.array(l, "fluxes").reshape(-1, 5)
        fluxes[:] = fluxes + U

    def upwind_gradient(self, l):
        """MGCFD_ARR_UPWIND_GRADIENT [nel, 15] of the last flux launch of level l."""
        return self.last_Gl[l].reshape(-1, 15).copy()


def configured(oracle, case, mode, cfl, levels, muscl, limiter=RUN_LIMITER, state="perturbed", smoothing=(0.0, 0), fas=False):
    """The emulator as tests/test_gpu_upwind.py configures the solver: level 0's start state, then the flux switched on."""
    em = UpwindOracle(oracle, case, mode, cfl, *smoothing, fas=fas)
    v = em._var(0)
    if state == "perturbed":
        v[:] = start_state(len(v), em.ff17[:5])
    elif state == "supersonic":
        v[:] = supersonic_state(len(v), em.ff17[:5])
    em.set_upwind(levels, muscl, limiter)
    return em


def write_lattice(name, directory):
    return fe.write_lattice(name, directory)
