"""Host tests of the run-time time step (no GPU): the numpy emulator (tests/time_step_emulator.py) against the oracle's two
step-factor kernels bit for bit in every sweep, the validity of every (case, mode, CFL) combination the GPU tests run, what
local steps do to convergence, the argument errors that need no device, and the new symbols."""
import ctypes as C
import os

import numpy as np
import pytest

import free_stream_emulator as fse
import time_step_emulator as tse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CYCLES = 5
STREAMS = [(1.2, 0.0), (0.8, 3.0)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _ff(stream):
    return fse.free_stream_constants(*stream)


def test_libm_cbrt_is_the_emulators():
    """The emulator's cbrt is the host libm's (the function the reference and the library call), not numpy's own, which may
    differ from it in the last bits (neither is correctly rounded): the two agree to a few ulp, and the identities below hold
    with libm's."""
    x = np.linspace(1e-4, 3.0, 20001)
    a, b = tse.libm_cbrt(x), np.cbrt(x)
    print("np.cbrt differs from libm's cbrt in", int((_bits(a) != _bits(b)).sum()), "of", x.size, "values")
    assert np.allclose(a, b, rtol=1e-15, atol=0.0)


@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("case", tse.GPU_CASES)
def test_global_and_legacy_equal_the_oracle_every_sweep(case, stream, oracle):
    """global at cfl = 0.5 gives ora_compute_step_factor's bits and local_legacy ora_compute_step_factor_legacy's, on the
    state of every sweep of 5 cycles — so "reference" at 0.5 is today's run whatever the mesh name."""
    for mode, fn in (("global", "ora_compute_step_factor"), ("local_legacy", "ora_compute_step_factor_legacy")):
        em = tse.TimeStepOracle(oracle, case, mode, 0.5, _ff(stream))
        seen = []

        def check(l, sf, em=em, fn=fn, seen=seen):
            L = em.oc.levels[l]
            want = np.zeros(L.nel)
            getattr(em.lib, fn)(L.nel, L.variables, L.volumes, oracle.ptr(want))
            assert np.array_equal(_bits(sf), _bits(want)), (case, mode, l, len(seen))
            seen.append(l)

        em.on_step_factors = check
        rc, rms = em.cycles(CYCLES)
        assert rc == 0 and len(rms) == CYCLES
        assert len(seen) == CYCLES * (em.n + max(0, em.n - 2))        # sweeps per cycle: levels 0..n-1, then n-2..1
        em.close()


@pytest.mark.parametrize("case", tse.GPU_CASES)
def test_reference_mode_is_the_composed_oracle(case, oracle):
    """mode "reference" at 0.5 = tests/free_stream_emulator.py's ComposedOracle (itself ora_solve), every level, bit for bit."""
    a = tse.TimeStepOracle(oracle, case)
    b = fse.ComposedOracle(oracle, case)
    (rca, rmsa), (rcb, rmsb) = a.cycles(3), b.cycles(3)
    assert rca == 0 and rcb == 0 and np.array_equal(_bits(rmsa), _bits(rmsb))
    for l in range(a.n):
        assert np.array_equal(_bits(a.variables(l)), _bits(b.variables(l)))
    a.close(); b.close()


@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("mode,cfl", [("local", 0.8), ("local", 1.0), ("local", 1.5), ("global", 0.8), ("global", 1.5)])
@pytest.mark.parametrize("case", tse.GPU_CASES)
def test_modes_stay_valid(case, mode, cfl, stream, oracle):
    em = tse.TimeStepOracle(oracle, case, mode, cfl, _ff(stream))
    rc, rms = em.cycles(CYCLES)
    assert rc == 0 and len(rms) == CYCLES and np.all(np.isfinite(rms)), (case, mode, cfl, stream, rc)
    em.close()


@pytest.mark.parametrize("case,mode,cfl", tse.gpu_combinations())
def test_every_gpu_combination_stays_valid(case, mode, cfl, oracle):
    """The table tests/test_gpu_time_step.py runs, none skipped: return code 0 in every cycle at the default free stream."""
    em = tse.TimeStepOracle(oracle, case, mode, cfl)
    rc, rms = em.cycles(tse.GPU_CYCLES)
    assert rc == 0 and len(rms) == tse.GPU_CYCLES
    em.close()


def test_gpu_table_covers_what_the_issue_names():
    combos = tse.gpu_combinations()
    assert len(combos) == (5 * 3 + 2) * 3
    assert ("fvcorr_1lvl", "global", 0.8) in combos and ("m6_2lvl", "local_legacy", 1.5) in combos
    assert all((c, "local", k) in combos for c in tse.GPU_CASES for k in tse.GPU_CFLS)


def test_local_steps_converge_faster_on_fvcorr(oracle):
    """fvcorr_1lvl, 5 cycles.  The RMS (of the change one sweep makes) after the fifth cycle is 1.19e-2 at local 1.5 and
    1.57e-2 at local 0.5, the formula at the reference's CFL number — the two figures the issue quotes; the run as the
    reference does it (local_legacy 0.5) stands at 1.07e-2 there, having fallen from its first cycle by a factor 0.71 where
    local 1.5 falls by 0.14: the larger steps change more per sweep and die away faster."""
    runs = {}
    for name, mode, cfl in (("today", "reference", 0.5), ("local 0.5", "local", 0.5), ("local 1.5", "local", 1.5)):
        em = tse.TimeStepOracle(oracle, "fvcorr_1lvl", mode, cfl)
        rc, rms = em.cycles(CYCLES)
        print("fvcorr_1lvl", name, "RMS per cycle", rms)
        assert rc == 0 and len(rms) == CYCLES
        runs[name] = rms
        em.close()
    assert abs(runs["local 1.5"][-1] - 1.19e-2) < 0.005e-2 and abs(runs["local 0.5"][-1] - 1.57e-2) < 0.005e-2    # to their three digits
    assert abs(runs["today"][-1] - 1.07e-2) < 0.005e-2
    assert runs["local 1.5"][-1] < runs["local 0.5"][-1]
    assert runs["local 1.5"][-1] / runs["local 1.5"][0] < 0.2 < 0.6 < runs["today"][-1] / runs["today"][0]


@pytest.mark.parametrize("case", [c for c in tse.GPU_CASES if c.startswith("m6")])
def test_damped_m6_cases_stay_near_the_far_field(case, oracle):
    for mode, cfl in (("global", 1.5), ("local", 1.5)):
        em = tse.TimeStepOracle(oracle, case, mode, cfl)
        rc, rms = em.cycles(CYCLES)
        print(case, mode, cfl, "RMS", rms[-1])
        assert rc == 0 and 0.0 < rms[-1] < 1e-5
        em.close()


def test_new_symbols_are_exported_and_typed():
    import mgcfd
    lib = mgcfd.load_library()
    names = ("mgcfd_set_time_step", "mgcfd_get_time_step", "mgcfd_group_set_time_step")
    header = open(os.path.join(ROOT, "include", "mgcfd.h")).read()
    for name in names:
        assert name in mgcfd.EXPORTED_SYMBOLS and hasattr(lib, name) and name + "(" in header
    assert lib.mgcfd_abi_version() == 1
    for k, name in enumerate(("MGCFD_DT_REFERENCE", "MGCFD_DT_GLOBAL", "MGCFD_DT_LOCAL", "MGCFD_DT_LOCAL_LEGACY")):
        assert f"{name} = {k}" in header
    assert mgcfd.api.DT_MODE == {"reference": 0, "global": 1, "local": 2, "local_legacy": 3}


def test_argument_errors_without_a_device():
    """What can be refused before any device is touched: a null handle (MGCFD_ERR_ARG), an unknown mode name in Python."""
    import mgcfd
    lib = mgcfd.load_library()
    assert lib.mgcfd_set_time_step(None, 2, 0.8) == 1
    assert lib.mgcfd_get_time_step(None, None, None) == 1
    assert lib.mgcfd_group_set_time_step(None, 2, 0.8) == 1
    with pytest.raises(ValueError):
        mgcfd.api._dt_mode("implicit")
    assert mgcfd.api._dt_mode("local-legacy") == 3 and mgcfd.api._dt_mode("local") == 2


def test_driver_refuses_bad_values_right_after_parsing(tmp_path):
    """euler3d_gpu_double: --time-step / --cfl with a bad value exit with status 1 before any file or device is touched."""
    import subprocess
    exe = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
    for args in (["--time-step=implicit"], ["--cfl", "0"], ["--cfl", "-1"], ["--cfl", "nan"], ["--cfl", "abc"], ["--time-step=local", "--cfl", "inf"]):
        r = subprocess.run([exe, "-i", "missing.dat", "-d", str(tmp_path)] + args, capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1, (args, r.returncode, r.stderr)
        assert "time-step" in r.stderr or "cfl" in r.stderr, (args, r.stderr)
    for k, text in enumerate(("time_step = implicit\n", "cfl = 0\n", "time_step = local\ncfl = minus\n")):      # ... and from a config file
        conf = tmp_path / f"bad{k}.conf"
        conf.write_text(text)
        r = subprocess.run([exe, "-i", "missing.dat", "-d", str(tmp_path), "-c", str(conf)], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 1 and ("time_step" in r.stderr or "cfl" in r.stderr), (text, r.returncode, r.stderr)
