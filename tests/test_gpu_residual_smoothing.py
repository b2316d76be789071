"""GPU tests of implicit residual smoothing (mgcfd_set_residual_smoothing) on one solver and in the drop-in binary: every
combination of rse.gpu_combinations() against the numpy emulator (tests/residual_smoothing_emulator.py) bit for bit; the same
bits on every path; the kernel's tile paths (several tiles, halo beyond LDS, long rows); the runs that only complete smoothed;
switching; refusals; the fast mode; the driver's flags; device allocations.  tests/test_host_residual_smoothing.py asserts on
the CPU that every combination stays valid."""
import os
import subprocess

import numpy as np
import pytest

import free_stream_emulator as fse
import residual_smoothing_emulator as rse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
CASES, K = rse.GPU_CASES, rse.GPU_CYCLES
REL_RUN = 1e-10          # tests/test_gpu_order_free.py: level `variables` after whole cycles, max |difference| / max |value|
RMS_FAST = 1e-9          # ... and its RMS tolerance
PATHS = [("m6_3lvl", "global", 1.5, 0.5, 2), ("tet_2lvl", "local", 2.5, 1.0, 2), ("fvcorr_1lvl", "local", 2.5, 0.5, 2),
         ("mixed_2lvl", "global", 2.5, 0.5, 1), ("m6_2lvl_dup2", "local", 1.5, 0.5, 3)]      # (one and three iterations too)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(np.asarray(got) - np.asarray(want)).max():.3e}"


def _solver(case, graph=0, exact=1, stage_wg4=1, fuse=1):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    for name, v in (("graph", graph), ("exact", exact), ("stage_wg4", stage_wg4), ("fuse_update", fuse)):
        s.set_option(name, v)
    return mesh, s


_emulated = {}


def _emulate(oracle, case, mode, cfl, eps, m, cycles=K):
    """(rms, variables per level) of `cycles` cycles: computed once per combination, shared and left unchanged."""
    key = (case, mode, cfl, eps, m, cycles)
    if key not in _emulated:
        em = rse.ResidualSmoothingOracle(oracle, case, mode, cfl, eps, m)
        rc, rms = em.cycles(cycles)
        assert rc == 0
        _emulated[key] = (rms, [em.variables(l) for l in range(em.n)])
        em.close()
    return _emulated[key]


@pytest.mark.parametrize("case,mode,cfl,eps,m", rse.gpu_combinations())
def test_state_equals_the_emulator(case, mode, cfl, eps, m, oracle):
    """After K cycles: `variables` of every level bitwise the emulator's, the RMS history within rtol 1e-12 — graphs off and on.
    (Smoothed sweeps are launched directly whatever MGCFD_OPT_GRAPH says: graph = 1 checks that the option is routed to the
    same launches and that nothing captured earlier is replayed, not a capture of the smoothing launches.)"""
    want_rms, want_v = _emulate(oracle, case, mode, cfl, eps, m)
    for graph in (0, 1):
        mesh, s = _solver(case, graph)
        s.set_time_step(mode, cfl)
        s.set_residual_smoothing(eps, m)
        assert s.residual_smoothing() == (eps, m)
        rms = s.run_cycles(K)
        what = f"{case} {mode} {cfl} ({eps}, {m}) graph={graph}"
        print(what, "rms", rms, "want", want_rms)
        for l in range(s.num_levels):
            _same(s.get(l, "variables"), want_v[l], f"{what}: variables, level {l}")
            assert not s.get(l, "fluxes").any(), f"{what}: fluxes, level {l}"
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


@pytest.mark.parametrize("case,mode,cfl,eps,m", PATHS)
def test_same_bits_on_every_path(case, mode, cfl, eps, m, oracle):
    """fuse_update 0 / 1, graph 0 / 1, stage_wg4 0 / 1, timing modes 1 and 4, the kernel-granular cycle and smooth(0, n): all
    the emulator's bits; the loop counts are those of the unsmoothed run."""
    _, want_v = _emulate(oracle, case, mode, cfl, eps, m)
    mesh, plain = _solver(case)
    plain.set_time_step(mode, min(cfl, 1.5))
    plain.run_cycles(K)
    want_iters = [plain.loop_iters(l) for l in range(plain.num_levels)]
    plain.close(); mesh.close()
    for graph, wg4, fuse, timing in ((0, 1, 1, 0), (1, 1, 1, 0), (0, 0, 1, 0), (1, 0, 1, 0), (0, 1, 0, 0), (1, 1, 0, 0), (0, 1, 1, 1), (0, 1, 1, 4)):
        mesh, s = _solver(case, graph, stage_wg4=wg4, fuse=fuse)
        s.set_option("timing", timing)
        s.set_time_step(mode, cfl)
        s.set_residual_smoothing(eps, m)
        s.run_cycles(K)
        what = f"{case} {mode} {cfl} ({eps}, {m}) graph={graph} wg4={wg4} fuse={fuse} timing={timing}"
        for l in range(s.num_levels):
            _same(s.get(l, "variables"), want_v[l], f"{what}: level {l}")
            assert s.loop_iters(l) == want_iters[l], what
        if timing:
            t = s.loop_times(0)
            assert t["time_step"] > 0.0 and t["flux"] > 0.0, what
        s.close()
        mesh.close()
    mesh, s = _solver(case)
    s.set_time_step(mode, cfl)
    s.set_residual_smoothing(eps, m)
    for _ in range(K):
        _kernel_granular_cycle(s)
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), want_v[l], f"{case} {mode} {cfl} kernel-granular: level {l}")
    s.close()
    mesh.close()
    em = rse.ResidualSmoothingOracle(oracle, case, mode, cfl, eps, m)
    assert em.sweeps(0, fse.SWEEPS) == 0
    for graph in (0, 1):
        mesh, s = _solver(case, graph)
        s.set_time_step(mode, cfl)
        s.set_residual_smoothing(eps, m)
        s.smooth(0, fse.SWEEPS)
        _same(s.get(0, "variables"), em.variables(0), f"{case} {mode} {cfl} smooth graph={graph}")
        _same(s.get(0, "step_factors"), em.step_factors(0), f"{case} {mode} {cfl} smooth graph={graph}: step factors")
        _same(s.get(0, "residuals"), em.oc.array(0, "residuals").reshape(-1, 5), f"{case} {mode} {cfl} smooth graph={graph}: residuals")
        s.close()
        mesh.close()
    em.close()


def test_kernel_paths(oracle, tmp_path):
    """The shapes at which the gather can go wrong: more than one tile, halo nodes beyond the LDS table (out[4] > 0) and long
    rows (out[8] > 0).  The goldens have several tiles; a generated tetrahedral level (30,000 nodes, the smallest size
    tests/test_gpu_parity.py knows to overflow) has the other two.  Sweeps of that level against the emulator, bit for bit,
    with one, two and three iterations under both kinds of step."""
    import mgcfd
    from mgcfd import meshgen
    tilings = {}
    for case in CASES:
        mesh, s = _solver(case)
        for l in range(s.num_levels):
            tilings[(case, l)] = s.tiling(l)
        s.close(); mesh.close()
    mg = meshgen.MultigridMesh(mesh_name="fvcorr")
    mg.levels.append(meshgen.make_tet_level(30000, seed=0, wall_below=2.0))
    d = tmp_path / "tet"
    os.makedirs(d / "input")
    meshgen.write_input(mg, str(d / "input"))
    (d / "case.txt").write_text("duplicate = 1\n")
    mesh = mgcfd.Mesh("input.dat", str(d / "input"))
    s = mgcfd.Solver.from_mesh(mesh)
    tilings[("tet30000", 0)] = s.tiling(0)
    for k, t in tilings.items():
        print(k, t)
    assert any(t["tiles"] > 1 for t in tilings.values())
    assert any(t["overflow_refs"] > 0 for t in tilings.values())
    assert any(t["list_entries"] > 0 for t in tilings.values())
    assert tilings[("tet30000", 0)]["overflow_refs"] > 0 and tilings[("tet30000", 0)]["list_entries"] > 0
    from conftest import perturbed_state
    start = perturbed_state(s.nel(0), s.far_field()[:5], seed=7, amplitude=0.002)
    em = rse.ResidualSmoothingOracle(oracle, str(d), "local", 0.1)
    # (this level's cells are small against its faces: a perturbed state survives local steps at these CFL numbers, checked on the CPU)
    for mode, cfl, eps, m in (("local", 0.1, 0.5, 2), ("global", 1.5, 1.0, 1), ("local", 0.2, 0.5, 3)):
        em.oc.array(0, "variables")[:] = start.ravel()
        em.set_time_step(mode, cfl)
        em.set_residual_smoothing(eps, m)
        assert em.sweeps(0, 2) == 0
        s.set(0, "variables", start)
        s.set_time_step(mode, cfl)
        s.set_residual_smoothing(eps, m)
        s.smooth(0, 2)
        _same(s.get(0, "variables"), em.variables(0), f"tetrahedral level {mode} {cfl} ({eps}, {m})")
        assert s.pending_invalid_state()[0] == 0
    em.close()
    s.close(); mesh.close()


@pytest.mark.parametrize("mode,cfl", rse.POINT_RUNS)
def test_the_point_of_the_feature(mode, cfl, oracle):
    """fvcorr_1lvl, 12 cycles: without smoothing run_cycles raises the emulator's error code in the emulator's cycle; with
    (0.5, 2) all 12 complete and the state is the emulator's bit for bit."""
    import mgcfd
    case, n = rse.POINT_CASE, rse.POINT_CYCLES
    em = rse.ResidualSmoothingOracle(oracle, case, mode, cfl)
    with np.errstate(all="ignore"):
        rc, rms = em.cycles(n)
    em.close()
    assert rc != 0
    mesh, s = _solver(case)
    s.set_time_step(mode, cfl)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.run_cycles(n)
    print(mode, cfl, "unsmoothed:", e.value, "emulator: rc", rc, "after", len(rms), "cycles")
    assert e.value.code == {1: 4, 2: 5, 3: 6}[rc]             # ora_check_for_invalid_variables' code as MGCFD_ERR_NAN / _NEG_DENSITY / _NEG_ENERGY
    assert s.invalid_state_location()[1] == len(rms)          # 0-based cycle = the emulator's completed cycles
    s.close(); mesh.close()
    want_rms, want_v = _emulate(oracle, case, mode, cfl, *rse.POINT_SMOOTHING, cycles=n)
    mesh, s = _solver(case)
    s.set_time_step(mode, cfl)
    s.set_residual_smoothing(*rse.POINT_SMOOTHING)
    got = s.run_cycles(n)
    print(mode, cfl, "smoothed rms", got)
    _same(s.get(0, "variables"), want_v[0], f"{case} {mode} {cfl} smoothed, {n} cycles")
    assert np.allclose(got, want_rms, rtol=1e-12, atol=0)
    s.close(); mesh.close()


@pytest.mark.parametrize("case", CASES)
def test_switching_between_runs(case, oracle):
    """On, off and on again between runs keeps the state and equals the emulator driven the same way (graphs off and on); after
    switching off, the rest of the run equals an unsmoothed solver started from that state."""
    legs = [(0.5, 2), (0.0, 0), (1.0, 3), (0.0, 0), (0.5, 1)]
    em = rse.ResidualSmoothingOracle(oracle, case, "local", 1.5)
    want = []
    for eps, m in legs:
        em.set_residual_smoothing(eps, m)
        rc, rms = em.cycles(K)
        assert rc == 0
        want.append((rms, [em.variables(l) for l in range(em.n)]))
    em.close()
    for graph in (0, 1):
        mesh, s = _solver(case, graph)
        s.set_time_step("local", 1.5)
        for k, (eps, m) in enumerate(legs):
            before = s.get(0, "variables")
            s.set_residual_smoothing(eps, m)
            assert s.residual_smoothing() == (eps, m)
            _same(s.get(0, "variables"), before, "the setter keeps the state")
            if k == 1:
                ref_mesh, ref = _solver(case, graph)
                ref.set_time_step("local", 1.5)
                for l in range(s.num_levels):
                    ref.set(l, "variables", s.get(l, "variables"))
                ref.run_cycles(K)
            rms = s.run_cycles(K)
            for l in range(s.num_levels):
                _same(s.get(l, "variables"), want[k][1][l], f"{case} graph={graph} leg {k} ({eps}, {m}): level {l}")
            assert np.allclose(rms, want[k][0], rtol=1e-12, atol=0)
            if k == 1:
                for l in range(s.num_levels):
                    _same(s.get(l, "variables"), ref.get(l, "variables"), f"{case} graph={graph}: against a never-smoothed solver, level {l}")
                ref.close(); ref_mesh.close()
        s.close()
        mesh.close()


def test_refusals():
    """Bad arguments, mid-sweep, a partitioned solver, a group member, the sweep_* calls and group creation while on: error
    code 1, "residual smoothing" in the message, nothing changed."""
    import mgcfd
    mesh, s = _solver("m6_2lvl")
    ref_mesh, ref = _solver("m6_2lvl")
    for t in (s, ref):
        t.set_residual_smoothing(0.5, 2)
    for eps, m in ((0.0, 2), (-0.5, 1), (float("nan"), 2), (float("inf"), 1), (0.5, -1), (0.5, 9)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            s.set_residual_smoothing(eps, m)
        assert e.value.code == 1 and "residual smoothing" in str(e.value)
    assert s.residual_smoothing() == (0.5, 2)
    for call in (lambda: s.sweep_begin(0), lambda: s.sweep_begin_partials(0), lambda: s.sweep_flux0(0), lambda: s.sweep_stage(0, 0),
                 lambda: s.sweep_end(0), lambda: s.sweep_end_partials(0)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1 and "residual smoothing" in str(e.value)
    with pytest.raises(mgcfd.MgcfdError) as e:
        mgcfd.Group([s])
    assert e.value.code == 1 and "residual smoothing" in str(e.value)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.rank_attach_plain(0, 1)
    assert e.value.code == 1 and "residual smoothing" in str(e.value)
    for t in (s, ref):
        t.run_cycles(1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "a cycle after the refused calls")
    # mid-sweep: the split sweep runs with smoothing off; the setter is refused until its last stage has run
    for t in (s, ref):
        t.set_residual_smoothing(0.0, 0)
    s.sweep_begin(0)
    s.sweep_stage(0, 0, partials=False)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_residual_smoothing(0.5, 2)
    assert e.value.code == 1 and "residual smoothing" in str(e.value) and "sweep is under way" in str(e.value)
    assert s.residual_smoothing() == (0.0, 0)
    s.sweep_stage(0, 1, partials=False)
    s.sweep_stage(0, 2, partials=False)
    ref.smooth(0, 1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "the sweep the refused call interrupted")
    # a group member, and a partitioned solver
    g = mgcfd.Group([s])
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_residual_smoothing(0.5, 2)
    assert e.value.code == 1 and "residual smoothing" in str(e.value)
    s.set_residual_smoothing(0.0, 0)                          # switching off is always allowed
    g.close()
    s.close(); ref.close()
    mesh.close(); ref_mesh.close()
    from mgcfd.partition import partition_hierarchy, rcb_partition
    mesh = mgcfd.Mesh("input.dat", fse.case_input("m6_2lvl"), 1)
    levels = [mesh.level(l) for l in range(mesh.num_levels)]
    H = partition_hierarchy(levels, rcb_partition(np.asarray(levels[0]["coords"]).reshape(-1, 3), 2))
    lv, owned, keys = H[0].solver_args()
    t = mgcfd.Solver.from_arrays(lv, mesh.variant, n_owned=owned, order_keys=keys)
    with pytest.raises(mgcfd.MgcfdError) as e:
        t.set_residual_smoothing(0.5, 2)
    assert e.value.code == 1 and "residual smoothing" in str(e.value)
    assert t.residual_smoothing() == (0.0, 0)
    t.set_residual_smoothing(0.0, 0)
    t.close()
    mesh.close()


@pytest.mark.parametrize("case,mode,cfl,eps,m", PATHS)
def test_fast_mode(case, mode, cfl, eps, m, oracle):
    """exact = 0 (FMA contraction, the order-free flux kernel) within the bound tests/test_gpu_order_free.py applies to whole
    cycles: 1e-10 of the largest value per level, RMS rtol 1e-9."""
    want_rms, want_v = _emulate(oracle, case, mode, cfl, eps, m)
    mesh, s = _solver(case, exact=0)
    s.set_time_step(mode, cfl)
    s.set_residual_smoothing(eps, m)
    rms = s.run_cycles(K)
    assert np.allclose(rms, want_rms, rtol=RMS_FAST, atol=0)
    for l in range(s.num_levels):
        rel = np.abs(s.get(l, "variables") - want_v[l]).max() / max(np.abs(want_v[l]).max(), 1e-300)
        print(case, mode, cfl, eps, m, "level", l, "rel", rel)
        assert rel <= REL_RUN, f"{case} level {l}: {rel:.3e}"
    s.close()
    mesh.close()


def _golden_cycles(case):
    meta = dict(l.strip().split(" = ") for l in open(os.path.join(fse.GOLDEN, case, "case.txt")))
    return int(meta["cycles"])


def _run_driver(tmp, case, extra, cycles, ok=True):
    os.makedirs(tmp / "out", exist_ok=True)
    cmd = [EXE, "-i", "input.dat", "-d", fse.case_input(case), "-o", "out/", "-g", str(cycles), "-m", str(fse.case_duplicate(case))] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tmp)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


def _loop_iters(d):
    f = [n for n in os.listdir(d / "out") if n.startswith("LoopNumIters")][0]
    header, line = [l.rstrip(",").split(",") for l in (d / "out" / f).read_text().splitlines()[:2]]
    at = header.index("CpuId") + 1
    return dict(zip(header[at:], (int(x) for x in line[at:])))


def _csv_row(path):
    rows = [l.rstrip(",\n").split(",") for l in open(path) if l.strip()]
    return dict(zip(rows[0], rows[1]))


def _strip(out):
    return [l for l in out.splitlines() if not l.startswith("Total runtime = ")]


@pytest.mark.parametrize("case", ["m6_2lvl", "fvcorr_1lvl"])
def test_driver_flags(case, oracle, tmp_path):
    """--residual-smoothing 0.5 (two iterations by default), --smoothing-iterations, the config keys and --gpus 2 mesh copies: the
    dump is the %.17e rendering of the emulator's state, the RMS lines its history, LoopNumIters.csv the plain run's counts;
    without the flags the golden dump; with --gpus-partition an error before any GPU work."""
    dup = fse.case_duplicate(case)
    name = f"variables.size={dup}x.cycles={K}.level=0"
    want_rms, want_v = _emulate(oracle, case, "local", 2.5, 0.5, 2)
    want = fse.render_variables(want_v[0]).encode()
    plain = _run_driver(tmp_path / "plain", case, ["--output-variables"], K)
    conf = tmp_path / "run.conf"
    conf.write_text("time_step = local\ncfl = 2.5\nresidual_smoothing = 0.5\nsmoothing_iterations = 2\n")
    flags = ["--time-step=local", "--cfl", "2.5", "--residual-smoothing", "0.5"]
    for tag, extra in (("default", flags), ("said", flags + ["--smoothing-iterations", "2"]), ("conf", ["-c", str(conf)]),
                       ("two", flags + ["--gpus", "2", "--gpus-share-device"])):
        d = tmp_path / tag
        if tag == "two" and len(want_v) == 1:                  # (a single level on two GPUs is split over them: refused by the library)
            r = _run_driver(d, case, ["--output-variables"] + extra, K, ok=False)
            assert "residual smoothing" in (r.stdout + r.stderr)
            continue
        r = _run_driver(d, case, ["--output-variables"] + extra, K)
        assert (d / "out" / name).read_bytes() == want, f"{case} {tag}"
        lines, plain_lines = _strip(r.stdout), _strip(plain.stdout)
        if tag != "two":
            assert len(lines) == len(plain_lines)
            rms_lines = [l for l in lines if "(RMS = " in l]
            assert rms_lines == [(f"Cycle {i + 1} / {K}" if len(want_v) <= 1 else f"MG cycle {i + 1} / {K}") + " (RMS = %.3e)" % want_rms[i] for i in range(K)]
            assert _loop_iters(d) == _loop_iters(tmp_path / "plain")
    _, v3 = _emulate(oracle, case, "local", 2.5, 1.0, 3)
    d = tmp_path / "three"
    _run_driver(d, case, ["--output-variables", "--time-step=local", "--cfl=2.5", "--residual-smoothing=1.0", "--smoothing-iterations=3"], K)
    assert (d / "out" / name).read_bytes() == fse.render_variables(v3[0]).encode()
    r = _run_driver(tmp_path / "part", case, flags + ["--gpus", "2", "--gpus-partition", "--gpus-share-device"], K, ok=False)
    assert "residual smoothing" in (r.stdout + r.stderr).lower()
    assert not [n for n in os.listdir(tmp_path / "part" / "out") if n.startswith("variables")]
    for bad in (["--residual-smoothing", "-1"], ["--residual-smoothing", "0.5", "--smoothing-iterations", "9"], ["--smoothing-iterations", "2"]):
        _run_driver(tmp_path / "bad", case, bad, K, ok=False)


@pytest.mark.parametrize("case", CASES)
def test_defaults_reproduce_the_golden_dumps(case, tmp_path):
    """Without the flags: variables.level0.txt of the golden case byte for byte and the golden LoopNumIters.csv's counts (as
    tests/test_gpu_parity.py compares them); --smoothing-iterations 0 spelled out is that run too, and so is the Python
    API's default."""
    cycles, dup = _golden_cycles(case), fse.case_duplicate(case)
    golden = open(os.path.join(fse.GOLDEN, case, "variables.level0.txt"), "rb").read()
    name = f"variables.size={dup}x.cycles={cycles}.level=0"
    plain = _run_driver(tmp_path / "plain", case, ["--output-variables"], cycles)
    assert (tmp_path / "plain" / "out" / name).read_bytes() == golden
    off = _run_driver(tmp_path / "off", case, ["--output-variables", "--residual-smoothing", "0.5", "--smoothing-iterations", "0"], cycles)
    assert (tmp_path / "off" / "out" / name).read_bytes() == golden
    assert _strip(off.stdout) == _strip(plain.stdout)
    want = _csv_row(os.path.join(fse.GOLDEN, case, "LoopNumIters.csv"))
    for d in (tmp_path / "plain", tmp_path / "off"):
        got = _csv_row(d / "out" / [n for n in os.listdir(d / "out") if n.startswith("LoopNumIters")][0])
        assert list(got.keys()) == list(want.keys())                      # same schema, same column order
        for k in want:
            if k[:-1] in ("flux", "update", "compute_step", "time_step", "restrict", "prolong", "indirect_rw") or k in ("Size", "Mesh", "MG cycles"):
                assert got[k] == want[k], (case, k)
    mesh, s = _solver(case)
    assert s.residual_smoothing() == (0.0, 0)
    s.set_residual_smoothing(0.5, 2)
    s.set_residual_smoothing(0.0, 0)                          # on and off again before the run: the default run
    s.run_cycles(cycles)
    assert fse.render_variables(s.get(0, "variables")).encode() == golden
    s.close()
    mesh.close()


def test_polar_with_residual_smoothing(oracle):
    """Solver.polar(residual_smoothing=(eps, iterations)) = set_residual_smoothing once, then the polar; the solver keeps it."""
    case, alphas, mach = fse.POLAR_CASE, fse.POLAR_ALPHAS, fse.POLAR_MACH
    mesh, s = _solver(case)
    pol = s.polar(alphas, K, mach=mach, time_step="local", cfl=2.5, residual_smoothing=(0.5, 2))
    assert s.residual_smoothing() == (0.5, 2) and s.time_step_control() == ("local", 2.5)
    em = rse.ResidualSmoothingOracle(oracle, case, "local", 2.5, 0.5, 2)
    for k, (al, p) in enumerate(zip(alphas, pol)):
        em.set_far_field(fse.free_stream_constants(mach, al), reinitialise=(k == 0))
        rc, rms = em.cycles(K)
        assert rc == 0 and np.allclose(p["rms"], rms, rtol=1e-12, atol=0)
    _same(s.get(0, "variables"), em.variables(0), "the polar's last state")
    em.close()
    s.close(); mesh.close()


def test_device_resources():
    """A solver that never enables the smoothing holds what it holds today; enabling adds two arrays per level, once; destroy
    returns to the baseline."""
    import mgcfd
    base = mgcfd.live_device_resources()
    mesh, a = _solver("m6_3lvl")
    never = mgcfd.live_device_resources()
    a.run_cycles(1)
    a.set_residual_smoothing(0.0, 0)
    after_run = mgcfd.live_device_resources()
    mesh_b, b = _solver("m6_3lvl")
    b.run_cycles(1)
    both = mgcfd.live_device_resources()
    assert both["allocations"] - after_run["allocations"] == after_run["allocations"] - base["allocations"], "a never-enabled solver: today's count"
    b.set_residual_smoothing(0.5, 2)
    on = mgcfd.live_device_resources()
    assert on["allocations"] - both["allocations"] == 2 * b.num_levels
    assert on["bytes"] - both["bytes"] >= sum(2 * 5 * 8 * b.nel(l) for l in range(b.num_levels))
    b.set_residual_smoothing(0.0, 0)
    b.set_residual_smoothing(1.0, 3)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"], "allocated once"
    b.run_cycles(1)
    b.close(); mesh_b.close()
    assert mgcfd.live_device_resources()["allocations"] == after_run["allocations"]
    a.close(); mesh.close()
    end = mgcfd.live_device_resources()
    assert end["allocations"] == base["allocations"] and end["bytes"] == base["bytes"]
    assert never["allocations"] > base["allocations"]
