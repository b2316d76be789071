"""GPU tests of the run-time time step (mgcfd_set_time_step) on ONE solver and in the drop-in binary: every case of
tse.GPU_CASES under every (mode, CFL) of tse.gpu_combinations() against the numpy emulator (tests/time_step_emulator.py), bit
for bit; the same bits on every path (fused, kernel-granular, graphs, stage_wg4); the setter between runs and mid-sweep; the
fast mode; the defaults against the golden dumps; --time-step / --cfl; loads and polars under local steps.  Groups and ranks:
tests/test_gpu_time_step_ranks.py.  tests/test_host_time_step.py asserts on the CPU that every combination stays valid."""
import os
import subprocess

import numpy as np
import pytest

import free_stream_emulator as fse
import surface_loads_emulator as emu
import time_step_emulator as tse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
CASES, K = tse.GPU_CASES, tse.GPU_CYCLES
REF = (0.25, -0.125, 0.375)
REL_RUN = 1e-10          # tests/test_gpu_order_free.py: level `variables` after whole cycles, max |difference| / max |value|
RMS_FAST = 1e-9          # ... and its RMS tolerance


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(np.asarray(got) - np.asarray(want)).max():.3e}"


def _solver(case, graph=0, exact=1, stage_wg4=1, fuse=1):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    s.set_option("graph", graph)
    s.set_option("exact", exact)
    s.set_option("stage_wg4", stage_wg4)
    s.set_option("fuse_update", fuse)
    return mesh, s


def _emulate(oracle, case, mode, cfl, cycles=K):
    em = tse.TimeStepOracle(oracle, case, mode, cfl)
    rc, rms = em.cycles(cycles)
    assert rc == 0
    out = (rms, [em.variables(l) for l in range(em.n)], [em.step_factors(l) for l in range(em.n)])
    em.close()
    return out


@pytest.mark.parametrize("case,mode,cfl", tse.gpu_combinations())
def test_state_and_step_factors_equal_the_emulator(case, mode, cfl, oracle):
    """After K cycles: `variables` of every level and every level's step_factors bitwise the emulator's, the RMS history
    within tests/test_gpu_parity.py's rtol 1e-12 — with graphs off and on."""
    want_rms, want_v, want_sf = _emulate(oracle, case, mode, cfl)
    for graph in (0, 1):
        mesh, s = _solver(case, graph)
        s.set_time_step(mode, cfl)
        assert s.time_step_control() == (mode, cfl)
        rms = s.run_cycles(K)
        what = f"{case} {mode} {cfl} graph={graph}"
        print(what, "rms", rms, "want", want_rms)
        for l in range(s.num_levels):
            _same(s.get(l, "variables"), want_v[l], f"{what}: variables, level {l}")
            _same(s.get(l, "step_factors"), want_sf[l], f"{what}: step_factors, level {l}")
        assert np.allclose(rms, want_rms, rtol=1e-12, atol=0), what
        s.close()
        mesh.close()


def _kernel_granular_cycle(s):
    """One V-cycle call by call (src/euler3d_cpu_double.cpp:371-694), every loop its own launch."""
    n = s.num_levels

    def sweep(l):
        s.copy_old_variables(l)
        s.compute_step_factor(l)
        for j in range(3):
            s.compute_fluxes(l)
            s.time_step(l, j)
        s.residual(l)

    for l in range(n):
        sweep(l)
        if l + 1 < n:
            s.restrict(l)
    for l in range(n - 2, -1, -1):
        s.prolong(l)
        if l > 0:
            sweep(l)


@pytest.mark.parametrize("mode,cfl", [("global", 0.8), ("local", 0.8), ("local_legacy", 1.5), ("local", 1.5)])
@pytest.mark.parametrize("case", CASES)
def test_same_bits_on_every_path(case, mode, cfl, oracle):
    """Fused stages with graphs on / off and stage_wg4 on / off, one launch per loop (fuse_update = 0), the kernel-granular
    calls and the split sweep (sweep_begin / sweep_stage): all the emulator's bits."""
    _, want_v, want_sf = _emulate(oracle, case, mode, cfl)
    for graph, wg4, fuse in ((0, 1, 1), (1, 1, 1), (0, 0, 1), (1, 0, 1), (0, 1, 0)):
        mesh, s = _solver(case, graph, stage_wg4=wg4, fuse=fuse)
        s.set_time_step(mode, cfl)
        s.run_cycles(K)
        for l in range(s.num_levels):
            _same(s.get(l, "variables"), want_v[l], f"{case} {mode} {cfl} graph={graph} wg4={wg4} fuse={fuse}: level {l}")
            _same(s.get(l, "step_factors"), want_sf[l], f"{case} {mode} {cfl} graph={graph} wg4={wg4} fuse={fuse}: step_factors {l}")
        s.close()
        mesh.close()
    mesh, s = _solver(case)
    s.set_time_step(mode, cfl)
    for _ in range(K):
        _kernel_granular_cycle(s)
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), want_v[l], f"{case} {mode} {cfl} kernel-granular: level {l}")
        _same(s.get(l, "step_factors"), want_sf[l], f"{case} {mode} {cfl} kernel-granular: step_factors {l}")
    s.close()
    mesh.close()
    # sweeps of level 0 alone: mgcfd_smooth (with its look-ahead on a single level) against the split sweep, stage by stage
    em = tse.TimeStepOracle(oracle, case, mode, cfl)
    assert em.sweeps(0, fse.SWEEPS) == 0
    for how in ("smooth", "smooth_graph", "stages", "begin_end"):
        mesh, s = _solver(case, graph=1 if how == "smooth_graph" else 0)
        s.set_time_step(mode, cfl)
        if how.startswith("smooth"):
            s.smooth(0, fse.SWEEPS)
        for _ in range(0 if how.startswith("smooth") else fse.SWEEPS):
            s.sweep_begin(0)
            if how == "stages":
                for j in range(3):
                    s.sweep_stage(0, j, partials=False)
            else:
                s.sweep_end(0)
        _same(s.get(0, "variables"), em.variables(0), f"{case} {mode} {cfl} {how}: sweeps of level 0")
        _same(s.get(0, "step_factors"), em.step_factors(0), f"{case} {mode} {cfl} {how}: step factors of the last sweep")
        s.close()
        mesh.close()
    em.close()


@pytest.mark.parametrize("case", CASES)
def test_switching_between_runs(case, oracle):
    """K cycles under one policy, the setter, K cycles under another — the state is kept, graphs are captured again — equals
    the emulator driven the same way, with graphs off and on; sweeps of level 0 alone likewise (the look-ahead's sf_alt and
    partial minima of the old policy are discarded)."""
    legs = [("reference", 0.5), ("local", 1.5), ("global", 0.8), ("local_legacy", 0.8), ("local", 0.5), ("reference", 0.5)]
    em = tse.TimeStepOracle(oracle, case)
    want = []
    for mode, cfl in legs:
        em.set_time_step(mode, cfl)
        rc, rms = em.cycles(K)
        assert rc == 0
        want.append((rms, [em.variables(l) for l in range(em.n)]))
    for mode, cfl in legs:
        em.set_time_step(mode, cfl)
        assert em.sweeps(0, fse.SWEEPS) == 0
        want.append((None, [em.variables(0)]))
    em.close()
    for graph in (0, 1):
        mesh, s = _solver(case, graph)
        for k, (mode, cfl) in enumerate(legs):
            before = s.get(0, "variables")
            s.set_time_step(mode, cfl)
            _same(s.get(0, "variables"), before, "the setter keeps the state")
            rms = s.run_cycles(K)
            for l in range(s.num_levels):
                _same(s.get(l, "variables"), want[k][1][l], f"{case} graph={graph} leg {k} {mode} {cfl}: level {l}")
            assert np.allclose(rms, want[k][0], rtol=1e-12, atol=0)
        for k, (mode, cfl) in enumerate(legs):
            s.set_time_step(mode, cfl)
            s.smooth(0, fse.SWEEPS)
            _same(s.get(0, "variables"), want[len(legs) + k][1][0], f"{case} graph={graph} sweeps leg {k} {mode} {cfl}")
        s.close()
        mesh.close()


def test_setter_is_refused_mid_sweep_and_on_bad_arguments():
    import mgcfd
    mesh, s = _solver("m6_2lvl")
    ref_mesh, ref = _solver("m6_2lvl")
    for t in (s, ref):
        t.set_time_step("local", 0.8)
    for mode, cfl in ((7, 0.5), (-1, 0.5), ("local", 0.0), ("local", -0.5), ("global", float("nan")), ("reference", float("inf"))):
        with pytest.raises(mgcfd.MgcfdError) as e:
            s.set_time_step(mode, cfl)
        assert e.value.code == 1 and "time step" in str(e.value)
    with pytest.raises(ValueError):
        s.set_time_step("implicit", 0.5)
    assert s.time_step_control() == ("local", 0.8)           # a refused call changes nothing
    with pytest.raises(mgcfd.MgcfdError) as e:               # a local step: nothing to reduce
        s.step_factor_local(0)
    assert e.value.code == 1
    s.sweep_begin(0)
    s.sweep_stage(0, 0, partials=False)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_time_step("global", 0.5)
    assert e.value.code == 1 and "sweep is under way" in str(e.value)
    assert s.time_step_control() == ("local", 0.8)
    s.sweep_stage(0, 1, partials=False)
    s.sweep_stage(0, 2, partials=False)
    ref.smooth(0, 1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "the sweep the refused call interrupted")
    s.sweep_begin(0)
    s.sweep_flux0(0)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_time_step("global", 0.5)
    assert e.value.code == 1
    s.sweep_end(0)
    ref.smooth(0, 1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "the second sweep")
    for t in (s, ref):
        t.set_time_step("global", 1.5)
        t.run_cycles(1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "a cycle after the change")
    s.close(); ref.close()
    mesh.close(); ref_mesh.close()


@pytest.mark.parametrize("mode,cfl", [("global", 0.8), ("local", 0.8), ("local", 1.5), ("local_legacy", 1.5)])
@pytest.mark.parametrize("case", CASES)
def test_fast_mode(case, mode, cfl, oracle):
    """exact = 0 (FMA contraction, the order-free stages) against the same emulator within the bound
    tests/test_gpu_order_free.py applies to whole cycles: 1e-10 of the largest value per level, RMS rtol 1e-9."""
    want_rms, want_v, _ = _emulate(oracle, case, mode, cfl)
    mesh, s = _solver(case, exact=0)
    s.set_time_step(mode, cfl)
    rms = s.run_cycles(K)
    assert np.allclose(rms, want_rms, rtol=RMS_FAST, atol=0)
    for l in range(s.num_levels):
        rel = np.abs(s.get(l, "variables") - want_v[l]).max() / max(np.abs(want_v[l]).max(), 1e-300)
        print(case, mode, cfl, "level", l, "rel", rel)
        assert rel <= REL_RUN, f"{case} {mode} {cfl} level {l}: {rel:.3e}"
    s.close()
    mesh.close()


def _golden_cycles(case):
    meta = dict(l.strip().split(" = ") for l in open(os.path.join(fse.GOLDEN, case, "case.txt")))
    return int(meta["cycles"])


def _run_driver(tmp, case, extra, cycles):
    os.makedirs(tmp / "out", exist_ok=True)
    cmd = [EXE, "-i", "input.dat", "-d", fse.case_input(case), "-o", "out/", "-g", str(cycles), "-m", str(fse.case_duplicate(case))] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tmp)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _loop_iters(d):
    """LoopNumIters.csv of a driver run as {column: count}: the per-level loop columns, without the identification columns
    in front of them (the last of which, CpuId, is the core the process happened to run on)."""
    f = [n for n in os.listdir(d / "out") if n.startswith("LoopNumIters")][0]
    header, line = [l.rstrip(",").split(",") for l in (d / "out" / f).read_text().splitlines()[:2]]
    assert len(header) == len(line)
    at = header.index("CpuId") + 1
    assert header[at] == "flux0" and len(header) > at
    return dict(zip(header[at:], (int(x) for x in line[at:])))


def _strip(out):
    return [l for l in out.splitlines() if not l.startswith("Total runtime = ")]


@pytest.mark.parametrize("case", CASES)
def test_defaults_reproduce_the_golden_dumps(case, tmp_path):
    """Without the options, and with --time-step=reference --cfl 0.5 spelled out: variables.level0.txt of the golden case byte
    for byte, the same stdout and the same LoopNumIters.csv."""
    cycles, dup = _golden_cycles(case), fse.case_duplicate(case)
    golden = open(os.path.join(fse.GOLDEN, case, "variables.level0.txt"), "rb").read()
    name = f"variables.size={dup}x.cycles={cycles}.level=0"
    plain = _run_driver(tmp_path / "plain", case, ["--output-variables"], cycles)
    assert (tmp_path / "plain" / "out" / name).read_bytes() == golden
    said = _run_driver(tmp_path / "said", case, ["--output-variables", "--time-step=reference", "--cfl", "0.5"], cycles)
    assert (tmp_path / "said" / "out" / name).read_bytes() == golden
    assert _strip(said.stdout) == _strip(plain.stdout)
    assert sorted(os.listdir(tmp_path / "said" / "out")) == sorted(os.listdir(tmp_path / "plain" / "out"))
    assert _loop_iters(tmp_path / "said") == _loop_iters(tmp_path / "plain")
    # ... and the Python API's default is that run too
    mesh, s = _solver(case)
    assert s.time_step_control() == ("reference", 0.5)
    s.run_cycles(cycles)
    assert fse.render_variables(s.get(0, "variables")).encode() == golden
    s.close()
    mesh.close()


@pytest.mark.parametrize("case", ["m6_2lvl", "fvcorr_1lvl"])
def test_driver_flags(case, oracle, tmp_path):
    """--time-step=local --cfl 0.8: the dump is the %.17e rendering of the emulator's state, on one GPU, from a config file and
    with --gpus 2 --gpus-partition --gpus-share-device; stdout has the plain run's lines and LoopNumIters.csv its counts
    (compute_step: nel per sweep in every mode)."""
    dup = fse.case_duplicate(case)
    name = f"variables.size={dup}x.cycles={K}.level=0"
    want_rms, want_v, _ = _emulate(oracle, case, "local", 0.8)
    want = fse.render_variables(want_v[0]).encode()
    plain = _run_driver(tmp_path / "plain", case, ["--output-variables"], K)
    conf = tmp_path / "run.conf"
    conf.write_text("time_step = local\ncfl = 0.8\n")
    flags = ["--time-step=local", "--cfl", "0.8"]
    for tag, extra in (("one", flags), ("conf", ["-c", str(conf)]), ("two", flags + ["--gpus", "2", "--gpus-partition", "--gpus-share-device"]),
                       ("loads", flags + ["--output-loads"])):
        d = tmp_path / tag
        r = _run_driver(d, case, ["--output-variables"] + extra, K)
        assert (d / "out" / name).read_bytes() == want, f"{case} {tag}"
        lines, plain_lines = _strip(r.stdout), _strip(plain.stdout)
        assert len(lines) == len(plain_lines)
        rms_lines = [l for l in lines if "(RMS = " in l]
        assert rms_lines == [(f"Cycle {i + 1} / {K}" if len(want_v) <= 1 else f"MG cycle {i + 1} / {K}") + " (RMS = %.3e)" % want_rms[i] for i in range(K)]
        if tag in ("one", "conf"):
            assert _loop_iters(d) == _loop_iters(tmp_path / "plain")
    # the same flow under --time-step=local-legacy / global: other dumps, each the emulator's
    for mode, flag in (("local_legacy", "local-legacy"), ("global", "global")):
        _, v, _ = _emulate(oracle, case, mode, 1.5)
        d = tmp_path / flag
        _run_driver(d, case, ["--output-variables", f"--time-step={flag}", "--cfl=1.5"], K)
        assert (d / "out" / name).read_bytes() == fse.render_variables(v[0]).encode(), f"{case} {flag}"


@pytest.mark.parametrize("case", CASES)
def test_loads_under_local_steps(case, oracle):
    """surface_loads and the run_cycles(loads=True) history under LOCAL equal the loads emulator on the emulator's states."""
    em = tse.TimeStepOracle(oracle, case, "local", 0.8)
    states = []
    for _ in range(K):
        rc, _ = em.cycles(1)
        assert rc == 0
        states.append(em.variables(0))
    em.close()
    mesh, s = _solver(case)
    s.set_time_step("local", 0.8)
    d = mesh.level(0)
    walls = s.get_edges(0, d["n_edges"])[d["boundary_start"]:d["boundary_start"] + d["n_boundary"]]
    ff = s.far_field()
    _, hist = s.run_cycles(K, loads=True, ref_point=REF)
    want = np.array([emu.surface_loads(v, walls, d["coords"], ff, REF) for v in states])
    _same(hist, want, f"{case}: loads history under local steps")
    _same(s.surface_loads(0, REF), want[-1], f"{case}: surface_loads")
    s.close()
    mesh.close()


def test_polar_under_local_steps(oracle):
    """Solver.polar(time_step="local", cfl=0.8) = set_time_step once, then the polar by hand; the last angle's state is the
    emulator's driven the same way; the solver keeps the policy."""
    import mgcfd
    case, alphas, mach = fse.POLAR_CASE, fse.POLAR_ALPHAS, fse.POLAR_MACH
    mesh, s = _solver(case)
    pol = s.polar(alphas, K, mach=mach, ref_point=REF, time_step="local", cfl=0.8)
    assert s.time_step_control() == ("local", 0.8)
    em = tse.TimeStepOracle(oracle, case, "local", 0.8)
    for k, (al, p) in enumerate(zip(alphas, pol)):
        em.set_far_field(fse.free_stream_constants(mach, al), reinitialise=(k == 0))
        rc, rms = em.cycles(K)
        assert rc == 0 and np.allclose(p["rms"], rms, rtol=1e-12, atol=0)
    _same(s.get(0, "variables"), em.variables(0), "the polar's last state")
    em.close()
    mesh2, t = _solver(case)
    t.set_time_step("local", 0.8)
    for k, (al, p) in enumerate(zip(alphas, pol)):
        t.set_free_stream(mach, al, reinitialise=(k == 0))
        rms, hist = t.run_cycles(K, loads=True, ref_point=REF)
        _same(p["rms"], rms, "polar RMS")
        _same(p["loads"], hist, "polar loads")
    pol2 = s.polar([1.0], 1, cfl=1.5)                         # cfl alone keeps the mode
    assert s.time_step_control() == ("local", 1.5) and len(pol2) == 1
    t.close(); s.close()
    mesh.close(); mesh2.close()
