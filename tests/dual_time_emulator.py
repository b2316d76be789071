"""The yardstick of dual time stepping (mgcfd_set_dual_time): ``DualTimeOracle``, the composed oracle of
tests/residual_smoothing_emulator.py with the physical-time source, the clamp of the pseudo step and the shift of the time
levels written in numpy from the definition in include/mgcfd.h / INTEGRATION.md §10.  Every flux, transfer, residual and RMS
stays the oracle's entry point; step factors and the Jacobi iterations stay the emulators' it is built on.

With dual time on and physical step dt, stage j of every sweep of every level computes its fluxes F as before and then

    a = W - Wn;  b = Wn - Wn1                              W: the state the fluxes were computed from
    BDF2:  src = vol * ((3.0 * a - b) / (2.0 * dt))        BDF1:  src = vol * (a / dt)
    F' = F - src

and the update proceeds with F' in place of F (time_step(j), or D = sf * F' into the Jacobi iterations).  Before stage 0
``sf = min(sf, (clamp * dt) / vol)``.  ``begin_step`` does Wn1 <- Wn, Wn <- variables on every level; the first one after
switching on or ``reset`` sets both to variables and BDF1 runs until the second.  While dual time is on the RMS of a cycle
is summed in the order the definition fixes on the original numbering (``ordered_sumsq``).  Every numpy operation is one IEEE-754 double
operation per element (numpy never contracts to FMA).
"""
import ctypes as C

import numpy as np

import residual_smoothing_emulator as rse
import time_step_emulator as tse

RK = 3
CLAMP = 2.0 / 3.0
MAX_ADVANCE_CYCLES = 4096

# What the GPU tests run (tests/test_gpu_dual_time.py): GPU_STEPS physical steps x GPU_CYCLES cycles (BDF1, then BDF2 twice) on
# every case below under every setting below.  dt per case is chosen so that the clamp binds on some nodes and not on others
# under every setting (asserted on the emulator's step factors by the host and the GPU tests).
GPU_CASES = ("fvcorr_1lvl", "m6_2lvl", "mixed_2lvl")
GPU_STEPS, GPU_CYCLES = 3, 2
# (name, time-step mode, cfl, (eps, iterations), bdf order)
GPU_SETTINGS = (("global05", "global", 0.5, (0.0, 0), 2),
                ("local25_smooth2", "local", 2.5, (0.5, 2), 2),
                ("local15_smooth1", "local", 1.5, (0.5, 1), 2),
                ("bdf1", "local", 1.5, (0.0, 0), 1))
# The physical step per (case, setting): with sf the unclamped step factors, the clamp binds where dt < sf * vol / clamp.  Under
# local steps that product spreads over a factor of two on a level and dt sits near level 0's median; under global steps it is
# one number per level (min_j(cfl * dt_j)), so on two levels dt sits between the levels' numbers (the clamp binds on the whole
# coarse level and nowhere on the fine one) and on the single-level case it can only bind everywhere or nowhere: it binds.
GPU_DT = {"fvcorr_1lvl": {"global05": 0.02, "local25_smooth2": 0.19, "local15_smooth1": 0.12, "bdf1": 0.12},
          "m6_2lvl": {"global05": 0.04, "local25_smooth2": 0.23, "local15_smooth1": 0.14, "bdf1": 0.14},
          "mixed_2lvl": {"global05": 0.03, "local25_smooth2": 0.17, "local15_smooth1": 0.10, "bdf1": 0.10}}
START_SEED = 7
# the point of the feature (test 3): m6_2lvl from conftest.perturbed_state(seed POINT_SEED), one cycle with dual time off (the
# coarse level then holds the restricted state), then POINT_STEPS x POINT_CYCLES at POINT_DT under local steps with smoothing.
# The figures below are what the emulator gives on the CPU (tests/test_host_dual_time.py prints and asserts them,
# profiles/dual_time_convergence.txt records them); the tests assert them with a margin of a factor 2.
POINT_CASE, POINT_MODE, POINT_CFL, POINT_SMOOTHING, POINT_SEED = "m6_2lvl", "local", 2.5, (0.5, 2), 7
POINT_DT, POINT_STEPS, POINT_CYCLES = 2.0, 3, 24
POINT_RMS_DROP = (3.53, 7.23, 7.26)              # rms[first cycle] / rms[last cycle] per physical step
POINT_RESIDUAL_RATIO = (0.429, 0.253, 0.256)       # max |(F - src) / vol| after the step's cycles / before them


def source(W, Wn, Wn1, vol, dt, order):
    """src [nel, 5] of one stage; vol [nel].  The differences first: W == Wn == Wn1 gives +0.0 exactly."""
    dt = np.float64(dt)
    vol = np.asarray(vol, dtype=np.float64)[:, None]
    a = W - Wn
    if order == 1:
        return vol * (a / dt)
    b = Wn - Wn1
    return vol * ((3.0 * a - b) / (2.0 * dt))


def clamp_step_factors(sf, vol, dt, clamp):
    """sf = min(sf, (clamp * dt) / vol); a NaN factor stays NaN."""
    cap = (np.float64(clamp) * np.float64(dt)) / vol
    return np.where(cap < sf, cap, sf)


def _tree64(v):
    """[..., 64] -> [...]: v[i] + v[i + 32] for i < 32, then + 16, 8, 4, 2, 1."""
    for half in (32, 16, 8, 4, 2, 1):
        v = v[..., :half] + v[..., half:]
    return v[..., 0]


def _group256(v):
    """[n, 256] -> [n]: four trees of 64, added one after another from +0.0."""
    b = _tree64(v.reshape(-1, 4, 64))
    t = np.zeros(len(b))
    for w in range(4):
        t = t + b[:, w]
    return t


def ordered_sumsq(residuals):
    """S of the definition (include/mgcfd.h, "The RMS of a cycle while dual time is on") for residuals [nel, 5]."""
    r = np.asarray(residuals, dtype=np.float64).reshape(-1, 5)
    q = np.zeros(len(r))
    for f in range(5):
        q = q + r[:, f] * r[:, f]
    q = np.concatenate([q, np.zeros(-len(q) % 256)])
    p = _group256(q.reshape(-1, 256))
    p = np.concatenate([p, np.zeros(-len(p) % 256)]).reshape(-1, 256)
    t = np.zeros(256)
    for row in p:
        t = t + row
    return _group256(t.reshape(1, 256))[0]


class _OrderedRms:
    """The oracle library with calc_rms in the definition's order while dual time is on (everything else passes through)."""

    def __init__(self, lib, owner):
        self._lib, self._owner = lib, owner

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def ora_calc_rms(self, nel, residuals):
        em = self._owner
        if em.dt == 0.0:
            return self._lib.ora_calc_rms(nel, residuals)
        assert residuals == em.oc.levels[0].residuals
        return float(np.sqrt(ordered_sumsq(em.oc.array(0, "residuals")) / np.float64(nel)))


def shift(variables, Wn, Wn1, first):
    """The time levels after begin_step: (Wn, Wn1)."""
    now = np.array(variables, dtype=np.float64, copy=True)
    return now, (now.copy() if first else Wn)


class DualTimeOracle(rse.ResidualSmoothingOracle):
    """ResidualSmoothingOracle with the physical step, the clamp and the time levels of mgcfd_set_dual_time."""

    def __init__(self, oracle, case, mode="reference", cfl=0.5, eps=0.0, iterations=0, ff17=None):
        super().__init__(oracle, case, mode, cfl, eps, iterations, ff17)
        self.lib = _OrderedRms(self.lib, self)
        self.dt, self.clamp, self.order, self.levels = 0.0, 0.0, 2, 0
        self.Wn, self.Wn1 = [None] * self.n, [None] * self.n
        self.bound = [[0, 0] for _ in range(self.n)]     # per level: nodes the clamp bound / left alone, over all sweeps
        self.max_abs_src = 0.0
        self.src_bits = set()                            # the distinct bit patterns of src while ``record_src_bits``
        self.record_src_bits = False

    def _var(self, l):
        return self.oc.array(l, "variables").reshape(-1, 5)

    def set_dual_time(self, dt, clamp=CLAMP):
        assert np.isfinite(dt) and dt >= 0.0 and (dt == 0.0 or (np.isfinite(clamp) and clamp > 0.0))
        if dt > 0.0 and self.dt == 0.0:
            for l in range(self.n):
                self.Wn[l], self.Wn1[l] = shift(self._var(l), None, None, True)
            self.levels = 0
        if dt == 0.0:
            self.Wn, self.Wn1, self.levels = [None] * self.n, [None] * self.n, 0
        self.dt, self.clamp = float(dt), (float(clamp) if dt > 0.0 else 0.0)

    def set_order(self, order):
        assert order in (1, 2)
        self.order = order

    def reset(self):
        self.levels = 0

    def set_time_levels(self, l, Wn=None, Wn1=None):
        """mgcfd_set_array on MGCFD_ARR_TIME_N / _TIME_N1: a level written is a level held."""
        if Wn is not None:
            self.Wn[l] = np.array(Wn, dtype=np.float64).reshape(-1, 5)
            self.levels = max(self.levels, 1)
        if Wn1 is not None:
            self.Wn1[l] = np.array(Wn1, dtype=np.float64).reshape(-1, 5)
            self.levels = 2

    def begin_step(self):
        assert self.dt > 0.0
        for l in range(self.n):
            self.Wn[l], self.Wn1[l] = shift(self._var(l), self.Wn[l], self.Wn1[l], self.levels == 0)
        self.levels = 1 if self.levels == 0 else 2

    def effective_order(self):
        return 2 if (self.order == 2 and self.levels == 2) else 1

    def stage_source(self, l, W):
        return source(W, self.Wn[l], self.Wn1[l], self.oc.array(l, "volumes"), self.dt, self.effective_order())

    def _sweep(self, l):
        if self.dt == 0.0:
            return super()._sweep(l)
        lib, L = self.lib, self.oc.levels[l]
        C.memmove(L.old_variables, L.variables, 8 * L.nel * 5)
        vol = self.oc.array(l, "volumes")
        sf = self.oc.array(l, "step_factors")
        free = tse.step_factors(self.mode, self.cfl, self.oc.array(l, "variables"), vol, self.cbrt_vol[l], self.variant)
        sf[:] = clamp_step_factors(free, vol, self.dt, self.clamp)
        n_bound = int((sf < free).sum())
        self.bound[l][0] += n_bound
        self.bound[l][1] += int(L.nel) - n_bound
        if self.on_step_factors:
            self.on_step_factors(l, sf)
        fluxes = self.oc.array(l, "fluxes").reshape(-1, 5)
        old = self.oc.array(l, "old_variables").reshape(-1, 5)
        var = self._var(l)
        for j in range(RK):
            lib.ora_compute_flux_edge(L.internal_start, L.n_internal, L.edges, L.variables, L.fluxes)
            lib.ora_compute_boundary_flux_edge(L.boundary_start, L.n_boundary, L.edges, L.variables, L.fluxes)
            lib.ora_compute_wall_flux_edge(L.wall_start, L.n_wall, L.edges, L.variables, L.fluxes, C.byref(self.ff))
            src = self.stage_source(l, var)
            if self.record_src_bits:
                self.src_bits.update(np.unique(src.view(np.int64)).tolist())
            if np.isfinite(src).all():
                self.max_abs_src = max(self.max_abs_src, float(np.abs(src).max()))
            fp = fluxes - src
            if self.iterations:
                var[:] = old + self.smoothed_update(l, sf, fp) / np.float64(RK + 1 - j)
            else:
                factor = sf / np.float64(RK + 1 - j)
                var[:] = old + factor[:, None] * fp
            fluxes[:] = 0.0
            rc = lib.ora_check_for_invalid_variables(L.variables, L.nel, None)
            if rc:
                return rc
        lib.ora_residual(L.nel, L.old_variables, L.variables, L.residuals)
        return 0

    def advance(self, steps, cycles_per_step):
        """mgcfd_advance: (rc, rms [steps * cycles_per_step], NaN from the failing cycle on)."""
        assert steps * cycles_per_step <= MAX_ADVANCE_CYCLES
        out = np.full(steps * cycles_per_step, np.nan)
        for step in range(steps):
            self.begin_step()
            rc, rms = self.cycles(cycles_per_step)
            out[step * cycles_per_step:step * cycles_per_step + len(rms)] = rms
            if rc:
                return rc, out
        return 0, out

    def bdf_residual(self, l=0):
        """(F - src) / vol of level ``l``'s current variables [nel, 5]: what a converged physical step drives to zero."""
        L = self.oc.levels[l]
        fluxes = self.oc.array(l, "fluxes").reshape(-1, 5)
        assert not fluxes.any()
        self.lib.ora_compute_flux_edge(L.internal_start, L.n_internal, L.edges, L.variables, L.fluxes)
        self.lib.ora_compute_boundary_flux_edge(L.boundary_start, L.n_boundary, L.edges, L.variables, L.fluxes)
        self.lib.ora_compute_wall_flux_edge(L.wall_start, L.n_wall, L.edges, L.variables, L.fluxes, C.byref(self.ff))
        r = (fluxes - self.stage_source(l, self._var(l))) / self.oc.array(l, "volumes")[:, None]
        fluxes[:] = 0.0
        return r


def pick_dt(oracle, case, mode, cfl, clamp=CLAMP, quantile=0.5):
    """A physical step at which the clamp binds on about ``quantile`` of level 0's nodes at the far-field start state:
    sf_i > clamp * dt / vol_i  <=>  dt < sf_i * vol_i / clamp, so the quantile of sf * vol / clamp, rounded to two digits."""
    em = tse.TimeStepOracle(oracle, case, mode, cfl)
    vol = em.oc.array(0, "volumes")
    sf = tse.step_factors(mode, cfl, em.oc.array(0, "variables"), vol, em.cbrt_vol[0], em.variant)
    dt = float(np.quantile(sf * vol / clamp, quantile))
    em.close()
    return float("%.2e" % dt)


def clamp_is_all_or_none(case, mode):
    """Global steps on a single level: sf * vol is one number, so the clamp binds on every node or on none."""
    return mode == "global" and case.endswith("_1lvl")


def start_state(case, ff_var, nel):
    """Level 0's start state of the GPU cases: fvcorr_1lvl develops a flow from its far field; the others get conftest's
    perturbation (seed START_SEED), or nothing would move."""
    from conftest import perturbed_state
    if case == "fvcorr_1lvl":
        return np.tile(np.asarray(ff_var, dtype=np.float64), (nel, 1))
    return perturbed_state(nel, ff_var, START_SEED)


def configured(oracle, case, name, mode, cfl, smoothing, order):
    """The emulator as tests/test_gpu_dual_time.py configures the solver for setting ``name``."""
    em = DualTimeOracle(oracle, case, mode, cfl, *smoothing)
    v = em.oc.array(0, "variables").reshape(-1, 5)
    v[:] = start_state(case, em.ff17[:5], len(v))
    em.set_dual_time(GPU_DT[case][name])
    em.set_order(order)
    return em


def point_run(oracle):
    """The run of test 3: (emulator at its end, [(rms [POINT_CYCLES], max |BDF residual| before, after) per physical step])."""
    from conftest import perturbed_state
    em = DualTimeOracle(oracle, POINT_CASE, POINT_MODE, POINT_CFL, *POINT_SMOOTHING)
    v = em.oc.array(0, "variables").reshape(-1, 5)
    v[:] = perturbed_state(len(v), em.ff17[:5], POINT_SEED)
    rc, _ = em.cycles(1)
    assert rc == 0
    em.set_dual_time(POINT_DT)
    hist = []
    for _ in range(POINT_STEPS):
        em.begin_step()
        r0 = float(np.abs(em.bdf_residual(0)).max())
        rc, rms = em.cycles(POINT_CYCLES)
        assert rc == 0
        hist.append((rms, r0, float(np.abs(em.bdf_residual(0)).max())))
    return em, hist
