"""Host tests of dual time stepping (no GPU): the emulator (tests/dual_time_emulator.py) against a hand-worked 3-node example,
src = +0.0 for uniform input, the emulator with dual time off against the emulator it is built on, the validity of every
combination the GPU tests run and where their clamp binds, the recorded convergence figures, and the new symbols."""
import os

import numpy as np
import pytest

import dual_time_emulator as dte
import residual_smoothing_emulator as rse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_hand_worked_three_nodes():
    """Three nodes, numbers whose arithmetic is exact in binary: every entry worked by hand from the definition."""
    W = np.array([[2.0] * 5, [1.0, 3.0, 5.0, 7.0, 9.0], [4.0] * 5])
    Wn = np.array([[1.0] * 5, [1.0, 2.0, 3.0, 4.0, 5.0], [4.0] * 5])
    Wn1 = np.array([[0.5] * 5, [1.0, 1.0, 1.0, 1.0, 1.0], [2.0] * 5])
    vol, dt = np.array([2.0, 0.5, 4.0]), 0.25
    # BDF2: vol * ((3 a - b) / (2 dt)), 2 dt = 0.5
    #   node 0: a = 1, b = 0.5: 2 * (2.5 / 0.5) = 10
    #   node 1: a = (0 1 2 3 4), b = (0 1 2 3 4): 3a - b = (0 2 4 6 8): 0.5 * (. / 0.5) = (0 2 4 6 8)
    #   node 2: a = 0, b = 2: 4 * (-2 / 0.5) = -16
    want2 = np.array([[10.0] * 5, [0.0, 2.0, 4.0, 6.0, 8.0], [-16.0] * 5])
    assert np.array_equal(_bits(dte.source(W, Wn, Wn1, vol, dt, 2)), _bits(want2))
    # BDF1: vol * (a / dt): node 0: 2 * 4 = 8; node 1: 0.5 * (0 4 8 12 16) = (0 2 4 6 8); node 2: 4 * 0 = +0
    want1 = np.array([[8.0] * 5, [0.0, 2.0, 4.0, 6.0, 8.0], [0.0] * 5])
    assert np.array_equal(_bits(dte.source(W, Wn, Wn1, vol, dt, 1)), _bits(want1))
    # the clamp: clamp * dt = 0.5 * 0.25 = 0.125; caps 0.0625, 0.25, 0.03125
    sf = np.array([0.05, 1.0, np.nan])
    got = dte.clamp_step_factors(sf, vol, dt, 0.5)
    assert got[0] == 0.05 and got[1] == 0.25 and np.isnan(got[2])
    # the shift: the first step stores the state twice, a later one moves Wn down
    n, n1 = dte.shift(W, None, None, True)
    assert np.array_equal(n, W) and np.array_equal(n1, W) and n is not W and n1 is not n
    n, n1 = dte.shift(W, Wn, Wn1, False)
    assert np.array_equal(n, W) and n1 is Wn


def test_uniform_input_gives_plus_zero():
    rng = np.random.default_rng(3)
    W = rng.standard_normal((64, 5)) * 10.0 ** rng.integers(-200, 200, (64, 1))
    vol = rng.uniform(1e-9, 1e9, 64)
    for order in (1, 2):
        for dt in (1e-300, 1e-3, 1.0, 1e300):
            src = dte.source(W, W.copy(), W.copy(), vol, dt, order)
            assert np.array_equal(_bits(src), np.zeros(src.shape, dtype=np.int64)), (order, dt)      # +0.0, never -0.0


def test_ordered_sum_of_squares_against_the_definition_read_literally():
    """ordered_sumsq against plain Python loops over the definition's sentences, on 700 nodes (three groups, the last one short)
    and on 70,000 (more than 256 groups)."""
    def tree64(v):
        v = list(v)
        for half in (32, 16, 8, 4, 2, 1):
            v = [v[i] + v[i + half] for i in range(half)]
        return v[0]

    def group(v):
        t = 0.0
        for w in range(4):
            t = t + tree64(v[64 * w:64 * w + 64])
        return t

    rng = np.random.default_rng(11)
    for nel in (700, 70000):
        r = rng.standard_normal((nel, 5)) * 10.0 ** rng.integers(-8, 2, (nel, 1))
        q = []
        for o in range(nel):
            acc = 0.0
            for f in range(5):
                acc = acc + float(r[o, f]) * float(r[o, f])
            q.append(acc)
        q += [0.0] * (-nel % 256)
        p = [group(q[256 * g:256 * g + 256]) for g in range(len(q) // 256)]
        t = [0.0] * 256
        for k, x in enumerate(p):
            t[k % 256] = t[k % 256] + x
        assert float(dte.ordered_sumsq(r)).hex() == group(t).hex(), nel


@pytest.mark.parametrize("case", dte.GPU_CASES)
def test_dual_time_off_is_the_smoothing_oracle(case, oracle):
    """dt = 0 (never switched on, or on and off again): ResidualSmoothingOracle's bits."""
    want = rse.ResidualSmoothingOracle(oracle, case, "local", 1.5, 0.5, 2)
    em = dte.DualTimeOracle(oracle, case, "local", 1.5, 0.5, 2)
    em.set_dual_time(0.1); em.set_dual_time(0.0)
    rc_w, rms_w = want.cycles(3)
    rc, rms = em.cycles(3)
    assert rc == rc_w == 0 and np.array_equal(_bits(rms), _bits(rms_w))
    for l in range(em.n):
        assert np.array_equal(_bits(em.variables(l)), _bits(want.variables(l)))
    em.close(); want.close()


@pytest.mark.parametrize("case", dte.GPU_CASES)
@pytest.mark.parametrize("name,mode,cfl,smoothing,order", dte.GPU_SETTINGS)
def test_every_gpu_combination_stays_valid_and_the_clamp_binds(case, name, mode, cfl, smoothing, order, oracle):
    em = dte.configured(oracle, case, name, mode, cfl, smoothing, order)
    rc, rms = em.advance(dte.GPU_STEPS, dte.GPU_CYCLES)
    print(case, name, "rc", rc, "rms", rms, "bound / free per level", em.bound, "max |src|", em.max_abs_src)
    assert rc == 0 and np.isfinite(rms).all() and em.levels == 2 and em.max_abs_src > 0.0
    bound, free = sum(b[0] for b in em.bound), sum(b[1] for b in em.bound)
    assert bound > 0 and (free > 0 or dte.clamp_is_all_or_none(case, mode))
    assert em.effective_order() == order
    for l in range(em.n):
        assert np.isfinite(em.variables(l)).all()
        assert not np.array_equal(em.Wn[l], em.Wn1[l])
    em.close()


def test_recorded_convergence_figures(oracle):
    """The figures tests/test_gpu_dual_time.py rests its physical claim on, as recorded in profiles/dual_time_convergence.txt."""
    em, hist = dte.point_run(oracle)
    em.close()
    for step, (rms, r0, r1) in enumerate(hist):
        print("step", step, "rms", rms[0], rms[-1], "drop", rms[0] / rms[-1], "residual", r0, r1, "ratio", r1 / r0)
        assert (np.diff(rms) < 0).all()
        assert abs(rms[0] / rms[-1] / dte.POINT_RMS_DROP[step] - 1.0) < 0.01
        assert abs(r1 / r0 / dte.POINT_RESIDUAL_RATIO[step] - 1.0) < 0.01


def test_new_symbols_are_exported_and_typed():
    import mgcfd
    lib = mgcfd.load_library()
    header = open(os.path.join(ROOT, "include", "mgcfd.h")).read()
    for name in ("mgcfd_set_dual_time", "mgcfd_get_dual_time", "mgcfd_dual_time_set_order", "mgcfd_dual_time_reset",
                 "mgcfd_dual_time_begin_step", "mgcfd_advance"):
        assert name in mgcfd.EXPORTED_SYMBOLS and hasattr(lib, name) and name + "(" in header
    assert "MGCFD_MAX_ADVANCE_CYCLES 4096" in header and "MGCFD_ARR_TIME_N, MGCFD_ARR_TIME_N1" in header
    assert mgcfd.api.ARR["time_n"] == 7 and mgcfd.api.ARR["time_n1"] == 8
    for name in ("set_dual_time", "dual_time", "dual_time_order", "dual_time_reset", "begin_step", "advance"):
        assert callable(getattr(mgcfd.Solver, name))
    import inspect
    assert inspect.signature(mgcfd.Solver.set_dual_time).parameters["clamp"].default == 2.0 / 3.0 == dte.CLAMP
    assert lib.mgcfd_abi_version() == 1


def test_driver_argument_parsing(tmp_path):
    """The driver's dual-time flags and config keys are checked before any file is read or any GPU touched: every bad value, a
    companion without --physical-time-step, -g out of range, --gpus-partition and --polar end with code 1 and a message that
    names the flag; good values get as far as the missing input file; --help lists the four flags."""
    import subprocess

    def run(args):
        r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
        return r.returncode, r.stdout + r.stderr

    for args, word in ((["--physical-time-step", "0"], "--physical-time-step"), (["--physical-time-step", "nan"], "--physical-time-step"),
                       (["--physical-time-step=-1"], "--physical-time-step"), (["--physical-time-step", "0.1", "--time-steps", "0"], "--time-steps"),
                       (["--physical-time-step", "0.1", "--time-steps", "2.5"], "--time-steps"),
                       (["--physical-time-step", "0.1", "--dual-time-clamp", "0"], "--dual-time-clamp"),
                       (["--physical-time-step", "0.1", "--bdf-order", "3"], "--bdf-order"),
                       (["--time-steps", "3"], "need --physical-time-step"), (["--bdf-order", "1"], "need --physical-time-step"),
                       (["--dual-time-clamp", "0.5"], "need --physical-time-step"),
                       (["--physical-time-step", "0.1", "-g", "0"], "cycles per physical step"),
                       (["--physical-time-step", "0.1", "-g", "4097"], "cycles per physical step"),
                       (["--physical-time-step", "0.1", "-i", "none.dat", "--gpus", "2", "--gpus-partition"], "--gpus-partition"),
                       (["--physical-time-step", "0.1", "-i", "none.dat", "--polar", "0:1:2"], "--polar")):
        rc, out = run(args)
        assert rc == 1 and word in out, (args, out)
    for key, bad in (("physical_time_step", "-2"), ("time_steps", "x"), ("dual_time_clamp", "inf"), ("bdf_order", "0")):
        conf = tmp_path / "bad.conf"
        conf.write_text(f"physical_time_step = 0.1\n{key} = {bad}\n")
        rc, out = run(["-c", str(conf)])
        assert rc == 1 and f"{key} = '{bad}'" in out, (key, out)
    conf = tmp_path / "good.conf"
    conf.write_text("physical_time_step = 0.1\ntime_steps = 4\ndual_time_clamp = 0.5\nbdf_order = 1\n")
    for args in (["-c", str(conf)], ["--physical-time-step=0.1", "--time-steps=4", "--dual-time-clamp=0.5", "--bdf-order=2", "-g", "4096"]):
        rc, out = run(args)
        assert rc == 1 and "input_file not set" in out, (args, out)
    rc, out = run(["--help"])
    for flag in ("--physical-time-step=DT", "--time-steps=N", "--dual-time-clamp=X", "--bdf-order=1|2", "cycles PER PHYSICAL STEP"):
        assert flag in out
