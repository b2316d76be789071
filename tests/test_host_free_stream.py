"""Host tests of the run-time free stream (no GPU): mgcfd_free_stream_constants against the oracle, the goldens' far field and
the Python emulator, bit for bit; its argument errors; the composed oracle (tests/free_stream_emulator.py) against
ora_solve; and that the composed oracle stays valid for every (golden case, pair) combination the GPU tests run."""
import itertools
import math
import os

import numpy as np
import pytest

import free_stream_emulator as fse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_default_pair_is_the_reference_far_field(oracle):
    import mgcfd
    got = mgcfd.free_stream_constants(1.2, 0.0)
    assert got.shape == (17,)
    assert np.array_equal(_bits(got), _bits(fse.oracle_default_ff17(oracle)))
    # today's Solver.far_field() values, written out (mgcfd_get_far_field of a solver nobody set: the GPU tests pin that
    # these are what a fresh solver returns): rho = 1.4, |V| = 1.2, p = 1
    assert got[0] == 1.4 and got[1] == 1.4 * 1.2 and got[2] == 0.0 and got[3] == 0.0
    assert got[4] == 1.4 * (0.5 * (1.2 * 1.2)) + (1.0 / (1.4 - 1.0))
    assert got[5] == 1.2 * (1.4 * 1.2) + 1.0 and got[9] == 1.0 and got[13] == 1.0
    assert got[14] == 1.2 * (got[4] + 1.0) and got[15] == 0.0 and got[16] == 0.0


def test_pair_table_covers_the_regimes():
    machs = [m for m, _ in fse.PAIRS]
    alphas = [a for _, a in fse.PAIRS]
    assert min(machs) < 1.0 < max(machs) and min(alphas) < 0.0 < max(alphas)
    assert fse.DEFAULT in fse.PAIRS
    gm, ga = [m for m, _ in fse.GPU_PAIRS], [a for _, a in fse.GPU_PAIRS]
    assert min(gm) < 1.0 < max(gm) and min(ga) < 0.0 < max(ga) and fse.DEFAULT not in fse.GPU_PAIRS


@pytest.mark.parametrize("mach,alpha", fse.PAIRS + fse.GPU_PAIRS)
def test_constants_equal_the_emulator_bit_for_bit(mach, alpha):
    import mgcfd
    got = mgcfd.free_stream_constants(mach, alpha)
    want = fse.free_stream_constants(mach, alpha)
    assert np.array_equal(_bits(got), _bits(want)), (got - want)
    # and they mean what they say: |V| = M c with c = 1, the velocity turned by alpha, p = 1
    v = got[1:4] / got[0]
    assert math.isclose(math.hypot(v[0], v[1]), mach, rel_tol=1e-14) and v[2] == 0.0
    assert math.isclose(math.degrees(math.atan2(v[1], v[0])), alpha, rel_tol=1e-12, abs_tol=1e-15)


@pytest.mark.parametrize("mach,alpha", [(float("nan"), 0.0), (1.2, float("nan")), (float("inf"), 0.0), (1.2, float("-inf")),
                                        (0.0, 0.0), (-0.5, 1.0), (1.2, 90.0), (1.2, -90.0), (0.8, 135.0)])
def test_argument_errors(mach, alpha):
    import mgcfd
    with pytest.raises(mgcfd.MgcfdError) as e:
        mgcfd.free_stream_constants(mach, alpha)
    assert e.value.code == 1 and "free stream" in str(e.value)


def test_new_symbols_are_exported_and_typed():
    import mgcfd
    lib = mgcfd.load_library()
    for name in ("mgcfd_free_stream_constants", "mgcfd_set_free_stream", "mgcfd_get_free_stream", "mgcfd_group_set_free_stream"):
        assert name in mgcfd.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.mgcfd_abi_version() == 1
    header = open(os.path.join(ROOT, "include", "mgcfd.h")).read()
    for name in ("mgcfd_free_stream_constants", "mgcfd_set_free_stream", "mgcfd_get_free_stream", "mgcfd_group_set_free_stream"):
        assert name + "(" in header


@pytest.mark.parametrize("case", fse.GPU_CASES)
def test_composed_oracle_reproduces_ora_solve(case, oracle):
    """Default far field: final `variables` of every level and the RMS list, bit for bit, after 1..3 cycles."""
    for cycles in (1, 2, 3):
        oc = oracle.OracleCase.from_input_dat(os.path.join(fse.case_input(case), "input.dat"), fse.case_duplicate(case))
        rc, want_rms, _ = oc.solve(cycles)
        assert rc == 0
        co = fse.ComposedOracle(oracle, case)
        rc, rms = co.cycles(cycles)
        assert rc == 0
        assert np.array_equal(_bits(rms), _bits(want_rms))
        for l in range(oc.nlevels):
            assert np.array_equal(_bits(co.variables(l)), _bits(oc.array(l, "variables").reshape(-1, 5))), f"level {l}"
        # one batch of 3 and three batches of 1 are the same thing
        if cycles == 3:
            co2 = fse.ComposedOracle(oracle, case)
            parts = [co2.cycles(1) for _ in range(3)]
            assert all(p[0] == 0 for p in parts)
            assert np.array_equal(_bits(np.concatenate([p[1] for p in parts])), _bits(want_rms))
            assert np.array_equal(_bits(co2.variables(0)), _bits(co.variables(0)))
            co2.close()
        co.close()
        oc.close()


@pytest.mark.parametrize("case,pair", list(itertools.product(fse.GPU_CASES, fse.GPU_PAIRS)))
def test_composed_oracle_stays_valid_for_every_gpu_combination(case, pair, oracle):
    """Cold start at the pair for GPU_CYCLES cycles, and the warm-start sequences the GPU tests drive: pair -> the other
    pair, default -> pair, each leg GPU_CYCLES cycles.  Return code 0 and finite RMS in every cycle."""
    other = [p for p in fse.GPU_PAIRS if p != pair][0]
    for first, second in ((pair, None), (pair, other), (fse.DEFAULT, pair)):
        co = fse.ComposedOracle(oracle, case, fse.free_stream_constants(*first))
        rc, rms = co.cycles(fse.GPU_CYCLES)
        assert rc == 0 and len(rms) == fse.GPU_CYCLES and np.all(np.isfinite(rms)), (first, rc, rms)
        if second is not None:
            co.set_far_field(fse.free_stream_constants(*second), reinitialise=False)
            rc, rms = co.cycles(fse.GPU_CYCLES)
            assert rc == 0 and len(rms) == fse.GPU_CYCLES and np.all(np.isfinite(rms)), (first, second, rc, rms)
        co.close()


@pytest.mark.parametrize("case", fse.GPU_CASES)
def test_level0_sweep_sequences_stay_valid(case, oracle):
    """What the sweep-graph test drives: fse.SWEEPS sweeps of level 0 alone at one pair from its far field, then as many at the other."""
    a, b = fse.GPU_PAIRS
    co = fse.ComposedOracle(oracle, case, fse.free_stream_constants(*a))
    assert all(co._sweep(0) == 0 for _ in range(fse.SWEEPS))
    co.set_far_field(fse.free_stream_constants(*b), reinitialise=False)
    assert all(co._sweep(0) == 0 for _ in range(fse.SWEEPS))
    co.close()


@pytest.mark.parametrize("warm", [True, False])
def test_polar_sequence_stays_valid(warm, oracle):
    co = fse.ComposedOracle(oracle, fse.POLAR_CASE)
    for k, alpha in enumerate(fse.POLAR_ALPHAS):
        co.set_far_field(fse.free_stream_constants(fse.POLAR_MACH, alpha), reinitialise=(k == 0 or not warm))
        rc, rms = co.cycles(fse.GPU_CYCLES)
        assert rc == 0 and np.all(np.isfinite(rms))
    co.close()


def test_a_changed_far_field_changes_the_flow(oracle):
    a = fse.ComposedOracle(oracle, "m6_2lvl")
    b = fse.ComposedOracle(oracle, "m6_2lvl", fse.free_stream_constants(*fse.GPU_PAIRS[0]))
    a.cycles(2)
    b.cycles(2)
    assert not np.array_equal(a.variables(0), b.variables(0))
    a.close()
    b.close()


def test_driver_rejects_bad_free_stream_arguments():
    import subprocess
    exe = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
    # (the message of each: an unknown option or a missing setting ends with status 1 and "ERROR" too, so the words are checked)
    for extra, words in ((["--mach", "0"], "free stream: the Mach number must be positive"),
                         (["--alpha", "90"], "free stream: the angle of attack must lie inside (-90, 90) degrees"),
                         (["--mach", "abc"], "--mach=abc: expected a number"),
                         (["--alpha", "1.5x"], "--alpha=1.5x: expected a number"),
                         (["--mach", "nan"], "--mach=nan: expected a number"),
                         (["--polar", "0:4"], "--polar=0:4: expected A0:A1:N"),
                         (["--polar", "0:4:0"], "--polar=0:4:0: expected A0:A1:N"),
                         (["--polar", "0:95:3"], "free stream: the angle of attack must lie inside (-90, 90) degrees")):
        r = subprocess.run([exe, "-i", "input.dat", "-d", fse.case_input("m6_2lvl")] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and ("ERROR: " + words) in r.stderr, (extra, r.stdout, r.stderr)
