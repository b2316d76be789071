"""The yardstick of the flow statistics (mgcfd_set_statistics): the definition of INTEGRATION.md §22 written in numpy, line by line.
Every numpy operation is one IEEE-754 double operation per element, in the definition's association; nothing is contracted.

    sample values  u = mx / rho, v = my / rho, w_ = mz / rho; speed_sqd = u*u + v*v + w_*w_; p = (gamma - 1) * (en - 0.5 * rho * speed_sqd)
                   x = (rho, u, v, w_, p, mut), mut = the eddy viscosity in effect on level 0, else +0.0
    host           wsum_new = wsum + w; a = w / wsum_new
    per node       d = x - m (old mean); m = m + a * d; e = x - m (new mean); c[pair(r, s)] = c[pair(r, s)] + (w * d[r]) * e[s]
                   over the pairs uu vv ww uv uw vw pp
    wall           the dp | tx ty tz columns of mgcfd_wall_distribution's table by the same recurrence with the same a and w:
                   [n][8] = mean dp tx ty tz | M2 dp tx ty tz

``Accumulator`` holds samples, wsum, m and c (and the wall table); ``StatisticsOracle`` is tests/sa_unsteady_emulator.py's
``SaUnsteadyOracle`` whose ``advance`` takes one sample of weight dt behind every completed physical step.
"""
import numpy as np

import dual_time_emulator as dte
import sa_unsteady_emulator as sue
import viscous_emulator as ve
import wall_heat_emulator as whe

GAMMA = 1.4
ARR_STATISTICS_MEAN, ARR_STATISTICS_MOMENTS = 23, 24
MEAN_COLUMNS, MOMENT_COLUMNS, WALL_COLUMNS = 6, 7, 8
PAIRS = ((1, 1), (2, 2), (3, 3), (1, 2), (1, 3), (2, 3), (4, 4))          # uu vv ww uv uw vw pp as columns of x
KERNEL_WEIGHTS = (0.02, 0.02, 0.05, 0.02, 0.013)                          # the kernel-level samples of tests/test_gpu_statistics.py
KERNEL_SEEDS = (7, 8, 9, 10, 11)


def sample_values(W, mut=None):
    """x [nel, 6] of a state W [nel, 5] by k_wall_distribution's expressions; mut None: the column is +0.0."""
    W = np.asarray(W, dtype=np.float64).reshape(-1, 5)
    rho, mx, my, mz, en = (W[:, k] for k in range(5))
    with np.errstate(all="ignore"):
        u, v, w_ = mx / rho, my / rho, mz / rho
        speed_sqd = u * u + v * v + w_ * w_
        p = (GAMMA - 1.0) * (en - 0.5 * rho * speed_sqd)
    m = np.zeros(len(W)) if mut is None else np.asarray(mut, dtype=np.float64).ravel()
    return np.stack([rho, u, v, w_, p, m], axis=1)


def update(x, m, c, a, w, pairs):
    """One step of the recurrence on columns: (m, c) after the sample x."""
    a, w = np.float64(a), np.float64(w)
    with np.errstate(all="ignore"):
        d = x - m
        m = m + a * d
        e = x - m
        c = c.copy()
        for k, (r, s) in enumerate(pairs):
            c[:, k] = c[:, k] + (w * d[:, r]) * e[:, s]
    return m, c


class Accumulator:
    """samples, wsum, m [nel, 6], c [nel, 7] from +0.0 and, once a wall table has been sampled, wall [n, 8]."""

    def __init__(self, nel, n_wall=None):
        self.samples, self.wsum, self.a, self.w = 0, np.float64(0.0), None, None
        self.m, self.c = np.zeros((nel, MEAN_COLUMNS)), np.zeros((nel, MOMENT_COLUMNS))
        self.wall = None if n_wall is None else np.zeros((n_wall, WALL_COLUMNS))

    def factors(self, w):
        """(wsum_new, a) of a sample of weight w, on the host."""
        w = np.float64(w)
        assert np.isfinite(w) and w > 0.0
        wsum_new = self.wsum + w
        return wsum_new, w / wsum_new

    def sample_x(self, x, w):
        """One sample of the values x [nel, 6]."""
        wsum_new, a = self.factors(w)
        self.m, self.c = update(np.asarray(x, dtype=np.float64), self.m, self.c, a, w, PAIRS)
        self.wsum, self.a, self.w = wsum_new, a, np.float64(w)
        self.samples += 1

    def sample(self, W, mut, w):
        self.sample_x(sample_values(W, mut), w)

    def wall_sample(self, table, w):
        """The wall half of the sample just taken (the same a and w): ``table`` [n, 7] is mgcfd_wall_distribution's."""
        assert self.a is not None and np.float64(w) == self.w
        t = np.asarray(table, dtype=np.float64).reshape(-1, 7)[:, 3:7]
        if self.wall is None:
            self.wall = np.zeros((len(t), WALL_COLUMNS))
        m, m2 = update(t, self.wall[:, :4], self.wall[:, 4:], self.a, w, ((0, 0), (1, 1), (2, 2), (3, 3)))
        self.wall = np.concatenate([m, m2], axis=1)

    def reset(self):
        self.__init__(len(self.m), None if self.wall is None else len(self.wall))


def derive(wsum, c):
    """mgcfd_statistics_derive: [n, 8] = Ruu Rvv Rww Ruv Ruw Rvw | p_rms | k."""
    c = np.asarray(c, dtype=np.float64).reshape(-1, MOMENT_COLUMNS)
    wsum = np.float64(wsum)
    R = c[:, :6] / wsum
    return np.concatenate([R, np.sqrt(c[:, 6] / wsum)[:, None], (0.5 * ((R[:, 0] + R[:, 1]) + R[:, 2]))[:, None]], axis=1)


def two_pass(X, weights, dtype):
    """The textbook evaluation in ``dtype``: the weighted means of the samples X [n_samples, 6], then the weighted sums of the
    products of the deviations for the seven pairs.  (mean [6], c [7])."""
    X = np.asarray(X).astype(dtype)
    w = np.asarray(weights).astype(dtype)
    wsum = w.sum()
    mean = (w[:, None] * X).sum(axis=0) / wsum
    D = X - mean
    return mean, np.array([(w * D[:, r] * D[:, s]).sum() for r, s in PAIRS], dtype=dtype)


class StatisticsOracle(sue.SaUnsteadyOracle):
    """SaUnsteadyOracle whose ``advance`` samples behind every completed physical step while ``statistics`` is on."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.stat = None

    def set_statistics(self, on=True):
        self.stat = Accumulator(self.oc.levels[0].nel) if on else None

    def mut_in_effect(self):
        """Level 0's eddy viscosity where one is in effect, else None."""
        if self.mut is None or not self._held[0] or self.model.eddy == 0:
            return None
        return self.mut[0]

    def statistics_sample(self, w):
        self.stat.sample(self._var(0), self.mut_in_effect(), w)

    def advance(self, steps, cycles_per_step):
        assert steps * cycles_per_step <= dte.MAX_ADVANCE_CYCLES
        out = np.full(steps * cycles_per_step, np.nan)
        for step in range(steps):
            self.begin_step()
            rc, rms = self.cycles(cycles_per_step)
            out[step * cycles_per_step:step * cycles_per_step + len(rms)] = rms
            if rc:
                return rc, out
            if self.stat is not None:
                self.statistics_sample(self.dt)
        return 0, out


def configured(oracle, case, mu, length="ddes", time_accurate=True, dt=sue.DUAL_DT, c_des=sue.SA_CDES, smoothing=(0.0, 0), jst_levels=0, fas=False,
               shape="V", face_gradient=None, tw_ratio=None, cfl=1.0):
    """sue.configured's setup, line by line, on a StatisticsOracle with the statistics on."""
    em = StatisticsOracle(oracle, case, "local", cfl, *smoothing, kappa2=ve.jse.KAPPA2 if jst_levels else 0.0,
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
    em.set_viscosity_model(law=sue.MODEL[0], eddy=sue.MODEL[1])
    em.set_sa_unsteady(time_accurate, length, c_des)
    if dt:
        em.set_dual_time(dt)
    em.set_statistics(True)
    return em


# ---- the invalid-step run of tests/test_gpu_statistics.py: tests/test_gpu_dual_time.py's choice of case ----
INVALID_CASE, INVALID_CFL, INVALID_DT, INVALID_STEPS, INVALID_CYCLES = "fvcorr_1lvl", 6.0, 10.0, 3, 4
# ... which fails in its first step; so that the accumulators have something to keep, VALID_STEPS steps at VALID_DT come first, from
# tests/dual_time_emulator.py's start state of the case at its seed (tests/test_host_statistics.py keeps the choice valid on the CPU)
VALID_DT, VALID_STEPS, VALID_CFL = 0.02, 2, 1.0


def invalid_start(nel, ff_var):
    from conftest import perturbed_state
    return perturbed_state(nel, ff_var, dte.START_SEED)


def invalid_run(oracle):
    """(rc and rms of the valid steps, rc and rms of the run that goes invalid, the emulator): local steps at CFL 1 and dt 0.02 for
    two steps, then CFL 6 with a physical step of 10."""
    em = StatisticsOracle(oracle, INVALID_CASE, "local", VALID_CFL)
    v = em._var(0)
    v[:] = invalid_start(len(v), em.ff17[:5])
    em.set_dual_time(VALID_DT)
    em.set_statistics(True)
    rc0, rms0 = em.advance(VALID_STEPS, INVALID_CYCLES)
    em.cfl = INVALID_CFL
    em.set_dual_time(INVALID_DT)
    rc, rms = em.advance(INVALID_STEPS, INVALID_CYCLES)
    return rc0, rms0, rc, rms, em
