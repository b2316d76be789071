"""Host tests of the flow statistics (no GPU): the numpy emulator (tests/statistics_emulator.py) against what the definition in
INTEGRATION.md §22 implies — its exact invariants, its accuracy against a two-pass evaluation in long double — then
mgcfd_statistics_derive against numpy, the ABI surface, and the runs tests/test_gpu_statistics.py emulates, which stay valid."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fas_emulator as fe
import sa_unsteady_emulator as sue
import statistics_emulator as ste

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
N_SAMPLES, N_NODES = 64, 256


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("statistics_lattices")
    return {name: fe.write_lattice(name, d) for name in fe.LATTICES}


# ---- the invariants, exact ----
def test_a_constant_signal():
    """m == x bitwise after any number of samples of any weights, and every co-moment is +0.0."""
    rng = np.random.default_rng(1)
    x = rng.uniform(-2.0, 2.0, (97, 6))
    acc = ste.Accumulator(len(x))
    for w in (0.02, 0.02, 0.05, 1e-9, 3.0, 0.013, 0.02):
        acc.sample_x(x, w)
        assert np.array_equal(_bits(acc.m), _bits(x))
        assert np.array_equal(_bits(acc.c), _bits(np.zeros_like(acc.c)))
    assert acc.samples == 7


def test_the_first_sample_and_two_equal_weights():
    """The first sample gives m = x and c = +0.0; two samples of equal weight give m = x1 + 0.5 * (x2 - x1)."""
    rng = np.random.default_rng(2)
    x1, x2 = rng.normal(size=(50, 6)), rng.normal(size=(50, 6))
    acc = ste.Accumulator(50)
    acc.sample_x(x1, 0.37)
    assert acc.a == 1.0 and np.array_equal(_bits(acc.m), _bits(x1)) and np.array_equal(_bits(acc.c), _bits(np.zeros((50, 7))))
    acc.sample_x(x2, 0.37)
    assert acc.a == 0.5
    assert np.array_equal(_bits(acc.m), _bits(x1 + 0.5 * (x2 - x1)))
    assert acc.wsum == np.float64(0.37) + np.float64(0.37) and acc.samples == 2


def test_rescaled_weights_give_the_same_means():
    """Weights (w, w, w) and all weights rescaled by a power of two give the same sequence of a, so the same means bitwise; the
    co-moments scale with the weights exactly."""
    rng = np.random.default_rng(3)
    X = rng.normal(size=(3, 40, 6))
    one, two = ste.Accumulator(40), ste.Accumulator(40)
    for k in range(3):
        one.sample_x(X[k], 0.02)
        two.sample_x(X[k], 0.02 * 4.0)
        assert one.a == two.a
    assert np.array_equal(_bits(one.m), _bits(two.m))
    assert np.array_equal(_bits(4.0 * one.c), _bits(two.c))


# ---- accuracy against a two-pass evaluation in long double ----
def _signal(ratio, seed):
    """[N_SAMPLES, N_NODES, 6]: per node and column a mean of order one, a sinusoid and noise of relative size ``ratio``."""
    rng = np.random.default_rng(seed)
    mean = rng.uniform(0.5, 2.0, (1, N_NODES, 6)) * rng.choice([-1.0, 1.0], (1, N_NODES, 6))
    t = np.arange(N_SAMPLES, dtype=np.float64)[:, None, None]
    phase = rng.uniform(0.0, 2.0 * np.pi, (1, N_NODES, 6))
    return mean * (1.0 + ratio * (np.sin(0.37 * t + phase) + 0.5 * rng.normal(size=(N_SAMPLES, N_NODES, 6))))


MEASURED = {}


@pytest.mark.parametrize("weights", ("equal", "unequal"))
@pytest.mark.parametrize("ratio", (1e-1, 1e-6))
def test_accuracy_against_long_double(ratio, weights):
    """64 samples of a seeded signal at 256 nodes, fluctuation over mean ``ratio``, equal (0.02) or unequal (uniform in 0.005 ..
    0.05) weights.  The yardstick per quantity (six means, seven co-moments) is what numpy's two-pass DOUBLE evaluation of the same
    samples loses against the two-pass evaluation in np.longdouble, the largest loss over the nodes; the emulator's largest error
    over the nodes is asserted within 8 x that (an incremental form does one rounding chain per sample where the two-pass form
    does two per sample) plus a floor of 64 ulp of the largest term.

    The largest term, from the rounding of the format and not from what the emulator gives: a stored mean carries a rounding
    error of up to an ulp of |x| per sample, so for a mean the term is |x|.  A co-moment's update (w * d[r]) * e[s] forms d and e
    against that mean, so the mean's error enters it multiplied by w |d|: the term is w |x| |d|, one ulp of it per sample, 64 over
    the run (max w, the larger |x| and the larger |d| of the pair, over samples and nodes).  This is the condition number of the
    incremental forms (Chan, Golub and LeVeque 1983: error ~ n kappa eps with kappa = |mean| / rms): the two-pass form's
    first-order error in the mean cancels in sum w (x - mean), so at a fluctuation of 1e-6 its co-moments are about a million
    times more accurate than any one-pass form's, and there the floor and not the factor 8 carries the assertion.

    Measured on the CPU, largest emulator error over the two-pass double loss | over the floor, per group of quantities:
        ratio 1e-1, equal weights    means 1.2 | 0.03   co-moments 11      | 0.2
        ratio 1e-1, unequal weights  means 1.1 | 0.03   co-moments 8.9     | 0.07
        ratio 1e-6, equal weights    means 1.0 | 0.04   co-moments 9.7e+05 | 0.2
        ratio 1e-6, unequal weights  means 1.0 | 0.04   co-moments 9.2e+05 | 0.1
    """
    X = _signal(ratio, seed=11)
    rng = np.random.default_rng(5)
    w = np.full(N_SAMPLES, 0.02) if weights == "equal" else rng.uniform(0.005, 0.05, N_SAMPLES)
    acc = ste.Accumulator(N_NODES)
    for k in range(N_SAMPLES):
        acc.sample_x(X[k], w[k])
    ref_m, ref_c, dbl_m, dbl_c = (np.zeros((N_NODES, 6), np.longdouble), np.zeros((N_NODES, 7), np.longdouble),
                                  np.zeros((N_NODES, 6)), np.zeros((N_NODES, 7)))
    for i in range(N_NODES):
        ref_m[i], ref_c[i] = ste.two_pass(X[:, i, :], w, np.longdouble)
        dbl_m[i], dbl_c[i] = ste.two_pass(X[:, i, :], w, np.float64)
    loss_m = np.abs(dbl_m.astype(np.longdouble) - ref_m).max(axis=0).astype(np.float64)
    loss_c = np.abs(dbl_c.astype(np.longdouble) - ref_c).max(axis=0).astype(np.float64)
    err_m = np.abs(acc.m.astype(np.longdouble) - ref_m).max(axis=0).astype(np.float64)
    err_c = np.abs(acc.c.astype(np.longdouble) - ref_c).max(axis=0).astype(np.float64)
    floor_m = 64 * EPS * np.abs(X).max(axis=(0, 1))
    D = X - np.asarray(ref_m, dtype=np.float64)[None]
    ax, ad = np.abs(X).max(axis=(0, 1)), np.abs(D).max(axis=(0, 1))
    floor_c = 64 * EPS * w.max() * np.array([max(ax[r], ax[s]) * max(ad[r], ad[s]) for r, s in ste.PAIRS])
    ratio_m, ratio_c = float((err_m / loss_m).max()), float((err_c / loss_c).max())
    MEASURED[(ratio, weights)] = (ratio_m, ratio_c)
    print(f"ratio {ratio:g} {weights}: emulator error over two-pass double loss: means {ratio_m:.2g}, co-moments {ratio_c:.2g}; "
          f"over the floor: means {float((err_m / floor_m).max()):.1g}, co-moments {float((err_c / floor_c).max()):.1g}")
    print("  two-pass double loss, means", loss_m, "co-moments", loss_c)
    print("  emulator error,       means", err_m, "co-moments", err_c)
    assert (err_m <= 8.0 * loss_m + floor_m).all(), (err_m, loss_m, floor_m)
    assert (err_c <= 8.0 * loss_c + floor_c).all(), (err_c, loss_c, floor_c)
    assert acc.wsum > 0.0 and np.abs(np.float64(acc.wsum) - w.sum()) <= 64 * EPS * w.sum()


def test_sample_values_against_the_primitives():
    """x of a state built from primitives returns them to rounding; the mut column is +0.0 without an eddy viscosity."""
    rng = np.random.default_rng(4)
    rho, p = rng.uniform(0.5, 2.0, 30), rng.uniform(0.5, 2.0, 30)
    vel = rng.normal(size=(30, 3))
    en = p / (ste.GAMMA - 1.0) + 0.5 * rho * (vel * vel).sum(axis=1)
    W = np.concatenate([rho[:, None], rho[:, None] * vel, en[:, None]], axis=1)
    x = ste.sample_values(W)
    assert np.array_equal(_bits(x[:, 0]), _bits(rho)) and np.array_equal(_bits(x[:, 5]), _bits(np.zeros(30)))
    assert np.abs(x[:, 1:4] - vel).max() <= 4 * EPS * np.abs(vel).max() and np.abs(x[:, 4] - p).max() <= 64 * EPS * np.abs(en).max()
    mut = rng.uniform(0.0, 1e-3, 30)
    assert np.array_equal(_bits(ste.sample_values(W, mut)[:, 5]), _bits(mut))


def test_the_wall_half_follows_the_same_factors():
    """wall_sample takes the a and w of the sample just taken: columns 3 .. 6 of the table, means and second moments."""
    rng = np.random.default_rng(6)
    acc = ste.Accumulator(4)
    tables = rng.normal(size=(3, 9, 7))
    for k, w in enumerate((0.02, 0.05, 0.013)):
        acc.sample_x(rng.normal(size=(4, 6)), w)
        acc.wall_sample(tables[k], w)
    W = np.array([0.02, 0.05, 0.013])
    mean = (W[:, None, None] * tables[:, :, 3:7]).sum(axis=0) / W.sum()
    m2 = (W[:, None, None] * (tables[:, :, 3:7] - mean) ** 2).sum(axis=0)
    assert acc.wall.shape == (9, 8)
    assert np.allclose(acc.wall[:, :4], mean, rtol=1e-13, atol=0) and np.allclose(acc.wall[:, 4:], m2, rtol=1e-12, atol=0)


# ---- the library's host-only call ----
def test_derive_against_numpy():
    """mgcfd_statistics_derive: c / wsum, sqrt(cpp / wsum) and 0.5 * ((Ruu + Rvv) + Rww), bit for bit numpy's; refusals."""
    import mgcfd
    lib = mgcfd.load_library()
    rng = np.random.default_rng(8)
    c = np.ascontiguousarray(rng.normal(size=(101, 7)))
    c[:, [0, 1, 2, 6]] = np.abs(c[:, [0, 1, 2, 6]])
    out = np.zeros((101, 8))
    wsum = 0.173
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.mgcfd_statistics_derive(wsum, ptr(c), 101, ptr(out)) == 0
    assert np.array_equal(_bits(out), _bits(ste.derive(wsum, c)))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.mgcfd_statistics_derive(bad, ptr(c), 101, ptr(out)) == 1
    assert lib.mgcfd_statistics_derive(wsum, ptr(c), -1, ptr(out)) == 1


def test_abi_surface():
    """The header declares the ids, the modes and the calls; the Python tables know them; the ABI version stays 1 and the array
    enum still ends with MGCFD_ARR_EDDY_VISCOSITY."""
    import mgcfd
    from mgcfd import api
    h = open(os.path.join(ROOT, "include", "mgcfd.h")).read()
    for pattern in (r"#define MGCFD_ARR_STATISTICS_MEAN\s+23\b", r"#define MGCFD_ARR_STATISTICS_MOMENTS\s+24\b", r"#define MGCFD_STATISTICS_OFF 0\b",
                    r"#define MGCFD_STATISTICS_VOLUME 1\b", r"#define MGCFD_STATISTICS_VOLUME_AND_WALL 2\b", r"#define MGCFD_WALL_STATISTICS_COLUMNS 8\b",
                    r"int mgcfd_set_statistics\(mgcfd_solver \*s, int mode\);",
                    r"int mgcfd_get_statistics\(const mgcfd_solver \*s, int \*mode, int64_t \*samples, double \*wsum\);",
                    r"int mgcfd_statistics_reset\(mgcfd_solver \*s\);", r"int mgcfd_statistics_sample\(mgcfd_solver \*s, double weight\);",
                    r"int mgcfd_statistics_restore\(mgcfd_solver \*s, int64_t samples, double wsum\);",
                    r"int mgcfd_wall_statistics\(mgcfd_solver \*s, int64_t \*node_ids, double \*out\);",
                    r"int mgcfd_set_wall_statistics\(mgcfd_solver \*s, const double \*in\);",
                    r"int mgcfd_statistics_derive\(double wsum, const double \*moments7, int64_t n, double \*out8\);",
                    r"int mgcfd_bench_statistics\(mgcfd_solver \*s, int kind, int launches, double \*avg_seconds\);",
                    r"MGCFD_ARR_EDDY_VISCOSITY /\*[^/]*\*/ \};"):
        assert re.search(pattern, h), pattern
    assert (api.ARR["statistics_mean"], api.ARR["statistics_moments"]) == (ste.ARR_STATISTICS_MEAN, ste.ARR_STATISTICS_MOMENTS)
    assert (api.NCOLS["statistics_mean"], api.NCOLS["statistics_moments"]) == (ste.MEAN_COLUMNS, ste.MOMENT_COLUMNS)
    assert api.WALL_STATISTICS_COLUMNS == ste.WALL_COLUMNS and api._STATISTICS_MODES == {"off": 0, "volume": 1, "wall": 2}
    lib = mgcfd.load_library()
    for name in ("mgcfd_set_statistics", "mgcfd_get_statistics", "mgcfd_statistics_reset", "mgcfd_statistics_sample", "mgcfd_statistics_restore",
                 "mgcfd_wall_statistics", "mgcfd_set_wall_statistics", "mgcfd_statistics_derive", "mgcfd_bench_statistics"):
        assert name in mgcfd.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.mgcfd_abi_version() == 1


# ---- the runs of tests/test_gpu_statistics.py stay valid on the CPU ----
@pytest.mark.parametrize("key", ("A", "B"))
def test_the_gpu_runs_stay_valid(key, oracle, lattices):
    """Delayed DES under BDF2 on lattices A and B through advance: finite, nt >= 0, one sample per step with wsum = the sum of dt in
    the order taken; the statistics leave the state alone (the run with them off gives the same bits); the mut column is in use."""
    em = ste.configured(oracle, lattices[key], sue.RUN_MU[key], "ddes")
    rc, rms = em.advance(sue.DUAL_STEPS, sue.DUAL_CYCLES)
    assert rc == 0 and np.isfinite(rms).all()
    plain = sue.configured(oracle, lattices[key], sue.RUN_MU[key], "ddes")
    rc0, rms0 = plain.advance(sue.DUAL_STEPS, sue.DUAL_CYCLES)
    assert rc0 == 0 and np.array_equal(_bits(rms), _bits(rms0)) and np.array_equal(_bits(em.variables(0)), _bits(plain.variables(0)))
    wsum = np.float64(0.0)
    for _ in range(sue.DUAL_STEPS):
        wsum = wsum + np.float64(sue.DUAL_DT)
    assert em.stat.samples == sue.DUAL_STEPS and em.stat.wsum == wsum
    assert np.isfinite(em.stat.m).all() and np.isfinite(em.stat.c).all()
    assert (em.stat.c[:, [0, 1, 2, 6]] >= 0.0).all() and em.stat.c[:, 0].max() > 0.0
    assert em.stat.m[:, 5].max() > 0.0 and (em.stat.m[:, 0] > 0.0).all() and (em.stat.m[:, 4] > 0.0).all()
    em.close(); plain.close()


def test_the_composed_run_and_the_changed_step_stay_valid(oracle, lattices):
    """Lattice A composed with residual smoothing, JST, FAS and a W cycle; and two advance calls with different dt."""
    name, kw = sue.composed_settings()[0]
    em = ste.configured(oracle, lattices["A"], sue.RUN_MU["A"], "ddes", **kw)
    rc, rms = em.advance(sue.DUAL_STEPS, sue.DUAL_CYCLES)
    assert rc == 0 and np.isfinite(rms).all() and np.isfinite(em.stat.c).all() and em.stat.samples == sue.DUAL_STEPS
    em.close()
    em = ste.configured(oracle, lattices["A"], sue.RUN_MU["A"], "ddes")
    rc, _ = em.advance(2, sue.DUAL_CYCLES)
    em.set_dual_time(sue.DUAL_DT / 2)
    rc2, _ = em.advance(2, sue.DUAL_CYCLES)
    assert rc == 0 and rc2 == 0 and em.stat.samples == 4
    assert em.stat.wsum == ((np.float64(sue.DUAL_DT) + sue.DUAL_DT) + sue.DUAL_DT / 2) + sue.DUAL_DT / 2
    em.close()


def test_the_invalid_run_goes_invalid_in_a_known_step(oracle):
    """tests/test_gpu_dual_time.py's invalid case behind two valid steps: the valid steps are sampled, the failing step is not."""
    rc0, rms0, rc, rms, em = ste.invalid_run(oracle)
    failed = int(np.isnan(rms).argmax()) // ste.INVALID_CYCLES
    print("invalid run: rc", rc, "fails in step", failed, "of the second call; samples", em.stat.samples)
    assert rc0 == 0 and np.isfinite(rms0).all()
    assert rc != 0 and np.isnan(rms[-1]) and failed < ste.INVALID_STEPS
    assert em.stat.samples == ste.VALID_STEPS + failed >= ste.VALID_STEPS
    assert np.isfinite(em.stat.m).all() and np.isfinite(em.stat.c).all() and em.stat.c[:, 0].max() > 0.0
    em.close()
