"""Host tests of implicit residual smoothing (no GPU): the numpy emulator (tests/residual_smoothing_emulator.py) with the
smoothing off against TimeStepOracle bit for bit, the validity of every combination the GPU tests run, the stability facts the
feature rests on, and the new symbols."""
import os

import numpy as np
import pytest

import residual_smoothing_emulator as rse
import time_step_emulator as tse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("case", rse.GPU_CASES)
def test_iterations_zero_is_the_time_step_oracle(case, oracle):
    """iterations = 0 (whatever eps): TimeStepOracle's bits on every level and its RMS history, under the default policy and
    under local steps."""
    for mode, cfl in (("reference", 0.5), ("local", 1.5)):
        want = tse.TimeStepOracle(oracle, case, mode, cfl)
        em = rse.ResidualSmoothingOracle(oracle, case, mode, cfl, 0.7, 0)
        rc_w, rms_w = want.cycles(rse.GPU_CYCLES)
        rc, rms = em.cycles(rse.GPU_CYCLES)
        assert rc == rc_w == 0 and np.array_equal(_bits(rms), _bits(rms_w))
        for l in range(em.n):
            assert np.array_equal(_bits(em.variables(l)), _bits(want.variables(l))), (case, mode, l)
        em.close(); want.close()


def test_the_sum_runs_in_edge_order_from_plus_zero(oracle):
    """The emulator's S against a plain Python loop over the edges (the definition read literally) on one level."""
    em = rse.ResidualSmoothingOracle(oracle, "tet_2lvl", "local", 1.5, 0.5, 2)
    L = em.oc.levels[0]
    e = em.oc.edges(0)[L.internal_start:L.internal_start + L.n_internal]
    rng = np.random.default_rng(5)
    sf, F = rng.uniform(0.5, 2.0, L.nel), rng.standard_normal((L.nel, 5))
    D = sf[:, None] * F
    n = np.zeros(L.nel)
    for a, b in zip(e["a"], e["b"]):
        n[a] += 1.0; n[b] += 1.0
    Db = D.copy()
    for _ in range(2):
        S = np.zeros_like(D)
        for a, b in zip(e["a"], e["b"]):
            S[a] = S[a] + Db[b]
            S[b] = S[b] + Db[a]
        Db = (D + np.float64(0.5) * S) / (1.0 + np.float64(0.5) * n)[:, None]
    assert np.array_equal(_bits(em.smoothed_update(0, sf, F)), _bits(Db))
    em.close()


@pytest.mark.parametrize("case,mode,cfl,eps,m", rse.gpu_combinations())
def test_every_gpu_combination_stays_valid(case, mode, cfl, eps, m, oracle):
    em = rse.ResidualSmoothingOracle(oracle, case, mode, cfl, eps, m)
    rc, rms = em.cycles(rse.GPU_CYCLES)
    print(case, mode, cfl, eps, m, "rc", rc, "rms", rms)
    assert rc == 0 and len(rms) == rse.GPU_CYCLES and np.isfinite(rms).all()
    for l in range(em.n):
        assert np.isfinite(em.variables(l)).all()
    em.close()


def _cycles_completed(oracle, mode, cfl, smoothing, cycles=rse.POINT_CYCLES):
    em = rse.ResidualSmoothingOracle(oracle, rse.POINT_CASE, mode, cfl, *smoothing)
    with np.errstate(all="ignore"):
        rc, rms = em.cycles(cycles)
    em.close()
    return rc, len(rms), rms


def test_stability_facts(oracle):
    """fvcorr_1lvl, the one golden case with a real flow in it.  Unsmoothed, `local` steps go invalid after 8, 2 and 1 completed
    cycles at CFL 2.0, 2.5 and 3.0 and `global` steps at CFL 4.0 after 7; with (0.5, 2) every one of them runs 12 cycles and the
    RMS falls below 1e-2."""
    for mode, cfl, done in (("local", 2.0, 8), ("local", 2.5, 2), ("local", 3.0, 1), ("global", 4.0, 7)):
        rc, n, _ = _cycles_completed(oracle, mode, cfl, (0.0, 0))
        print(mode, cfl, "unsmoothed: rc", rc, "after", n, "cycles")
        assert rc != 0 and n == done, (mode, cfl, rc, n)
    for mode, cfl in (("local", 2.0), ("local", 2.5), ("local", 3.0), ("global", 4.0)):
        rc, n, rms = _cycles_completed(oracle, mode, cfl, rse.POINT_SMOOTHING)
        print(mode, cfl, "smoothed: rc", rc, "rms", rms[-1] if n else None)
        assert rc == 0 and n == rse.POINT_CYCLES
        if mode == "local":
            assert 0.0 < rms[-1] < 1e-2
    assert set(rse.POINT_RUNS) <= {("local", 2.5), ("global", 4.0)}


def test_new_symbols_are_exported_and_typed():
    """(mgcfd_abi_version stays 1: the two calls are additions, and the existing host tests pin the number.)"""
    import mgcfd
    lib = mgcfd.load_library()
    header = open(os.path.join(ROOT, "include", "mgcfd.h")).read()
    for name in ("mgcfd_set_residual_smoothing", "mgcfd_get_residual_smoothing", "mgcfd_bench_residual_smoothing"):
        assert name in mgcfd.EXPORTED_SYMBOLS and hasattr(lib, name) and name + "(" in header
    assert "MGCFD_MAX_SMOOTHING_ITERATIONS 8" in header
    for name in ("set_residual_smoothing", "residual_smoothing"):
        assert callable(getattr(mgcfd.Solver, name))
    import inspect
    assert "residual_smoothing" in inspect.signature(mgcfd.Solver.polar).parameters
