"""GPU tests of the JST dissipation (mgcfd_set_jst) on one solver and in the drop-in binary: every combination of
jse.gpu_combinations() against the numpy emulator (tests/jst_emulator.py) bit for bit — state, stage fluxes F + C and RMS history;
the same bits on every path; the kernels' tile paths (several tiles, halo beyond LDS, long rows) with L, nu, r and C read back;
composition with residual smoothing and dual time; switching; refusals; the fast mode; the driver's flags; device allocations.
tests/test_host_jst.py asserts on the CPU that every combination stays valid."""
import os
import subprocess

import numpy as np
import pytest

import dual_time_emulator as dte
import free_stream_emulator as fse
import jst_emulator as jse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
CASES, K = jse.GPU_CASES, jse.GPU_CYCLES
REL_RUN = 1e-10          # tests/test_gpu_residual_smoothing.py::test_fast_mode (from tests/test_gpu_order_free.py): level `variables`
RMS_FAST = 1e-9          # after whole cycles, max |difference| / max |value|; and its RMS tolerance
# (case, mode, cfl, kappa2, kappa4, levels): three, two and one level; both pairs; level 0 alone and all levels
PATHS = [("m6_3lvl", "reference", 0.5, 2.5, 0.15625, 1), ("tet_2lvl", "local", 1.5, 0.0, 0.15625, "all"),
         ("fvcorr_1lvl", "local", 1.5, 2.5, 0.15625, 1), ("mixed_2lvl", "reference", 0.5, 2.5, 0.15625, "all")]


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


def _levels(s, lv):
    return s.num_levels if lv == "all" else lv


_emulated = {}


def _emulate(oracle, case, mode, cfl, k2, k4, lv, cycles=K):
    """(rms, variables per level, F + C of the final state per level) of `cycles` cycles: computed once per combination,
    shared and left unchanged."""
    key = (case, mode, cfl, k2, k4, lv, cycles)
    if key not in _emulated:
        em = jse.JstOracle(oracle, case, mode, cfl, kappa2=k2, kappa4=k4, levels=lv)
        rc, rms = em.cycles(cycles)
        assert rc == 0
        _emulated[key] = (rms, [em.variables(l) for l in range(em.n)], [em.stage_fluxes(l) for l in range(em.n)])
        em.close()
    return _emulated[key]


@pytest.mark.parametrize("case,mode,cfl,k2,k4,lv", jse.gpu_combinations())
def test_state_fluxes_and_rms_equal_the_emulator(case, mode, cfl, k2, k4, lv, oracle):
    """After K cycles: `variables` of every level, the RMS history and F + C of the final state on every level (one
    mgcfd_compute_fluxes from zero fluxes, read back) bitwise the emulator's."""
    want_rms, want_v, want_f = _emulate(oracle, case, mode, cfl, k2, k4, lv)
    mesh, s = _solver(case)
    s.set_time_step(mode, cfl)
    s.set_jst(k2, k4, _levels(s, lv))
    assert s.jst() == (k2, k4, _levels(s, lv))
    rms = s.run_cycles(K)
    what = f"{case} {mode} {cfl} ({k2}, {k4}, {lv})"
    print(what, "rms", rms, "want", want_rms)
    _same(rms, want_rms, f"{what}: RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), want_v[l], f"{what}: variables, level {l}")
        assert not s.get(l, "fluxes").any(), f"{what}: fluxes after the run, level {l}"
        s.compute_fluxes(l)
        _same(s.get(l, "fluxes"), want_f[l], f"{what}: F + C, level {l}")
        s.zero_fluxes(l)
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


@pytest.mark.parametrize("case,mode,cfl,k2,k4,lv", PATHS)
def test_same_bits_on_every_path(case, mode, cfl, k2, k4, lv, oracle):
    """fuse_update 0 / 1, graph 0 / 1, stage_wg4 0 / 1, timing modes 1 and 4, the kernel-granular cycle and smooth(0, n): all the
    emulator's bits; the loop counts are those of the run without JST."""
    want_rms, want_v, _ = _emulate(oracle, case, mode, cfl, k2, k4, lv)
    mesh, plain = _solver(case)
    plain.set_time_step(mode, cfl)
    plain.run_cycles(K)
    want_iters = [plain.loop_iters(l) for l in range(plain.num_levels)]
    plain.close(); mesh.close()
    for graph, wg4, fuse, timing in ((0, 1, 1, 0), (1, 1, 1, 0), (0, 0, 1, 0), (1, 0, 1, 0), (0, 1, 0, 0), (1, 1, 0, 0), (0, 1, 1, 1), (0, 1, 1, 4)):
        mesh, s = _solver(case, graph, stage_wg4=wg4, fuse=fuse)
        s.set_option("timing", timing)
        s.set_time_step(mode, cfl)
        s.set_jst(k2, k4, _levels(s, lv))
        rms = s.run_cycles(K)
        what = f"{case} {mode} {cfl} ({k2}, {k4}, {lv}) graph={graph} wg4={wg4} fuse={fuse} timing={timing}"
        _same(rms, want_rms, f"{what}: RMS history")
        for l in range(s.num_levels):
            _same(s.get(l, "variables"), want_v[l], f"{what}: level {l}")
            assert s.loop_iters(l) == want_iters[l], what
        if timing:
            assert s.loop_times(0)["flux"] > 0.0, what
        s.close()
        mesh.close()
    mesh, s = _solver(case)
    s.set_time_step(mode, cfl)
    s.set_jst(k2, k4, _levels(s, lv))
    for _ in range(K):
        _kernel_granular_cycle(s)
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), want_v[l], f"{case} {mode} {cfl} kernel-granular: level {l}")
    s.close()
    mesh.close()
    em = jse.JstOracle(oracle, case, mode, cfl, kappa2=k2, kappa4=k4, levels=lv)
    assert em.sweeps(0, fse.SWEEPS) == 0
    for graph in (0, 1):
        mesh, s = _solver(case, graph)
        s.set_time_step(mode, cfl)
        s.set_jst(k2, k4, _levels(s, lv))
        s.smooth(0, fse.SWEEPS)
        _same(s.get(0, "variables"), em.variables(0), f"{case} {mode} {cfl} smooth graph={graph}")
        _same(s.get(0, "residuals"), em.oc.array(0, "residuals").reshape(-1, 5), f"{case} {mode} {cfl} smooth graph={graph}: residuals")
        s.close()
        mesh.close()
    em.close()


def test_kernel_paths(oracle, tmp_path):
    """The shapes at which the gathers can go wrong, as tests/test_gpu_residual_smoothing.py::test_kernel_paths finds them: more
    than one tile (the goldens), halo nodes beyond the LDS table and long rows (a generated tetrahedral level of 30,000 nodes).
    On that level and on a golden one, from a perturbed state: L, nu and r (MGCFD_ARR_JST_*), F + C after mgcfd_compute_fluxes,
    and F(internal) + C after mgcfd_compute_flux_edge, with F(internal) from the same call with JST off, so that C itself is
    compared in one addition — all bitwise the emulator's; then two sweeps.  (JST leaves the noise of a perturbed state almost
    undamped: the tetrahedral level runs at local CFL 0.02, where the emulator stays valid; tests/test_host_jst.py has no part in
    this generated level, so the emulator's return code is asserted here.)"""
    import mgcfd
    from mgcfd import meshgen
    from conftest import perturbed_state
    mg = meshgen.MultigridMesh(mesh_name="fvcorr")
    mg.levels.append(meshgen.make_tet_level(30000, seed=0, wall_below=2.0))
    d = tmp_path / "tet"
    os.makedirs(d / "input")
    meshgen.write_input(mg, str(d / "input"))
    (d / "case.txt").write_text("duplicate = 1\n")
    for case, amplitude, cfl in ((str(d), 0.002, 0.02), ("mixed_2lvl", 0.01, 0.5)):
        mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
        s = mgcfd.Solver.from_mesh(mesh)
        t = s.tiling(0)
        print(case, t)
        if case == str(d):
            assert t["tiles"] > 1 and t["overflow_refs"] > 0 and t["list_entries"] > 0
        else:
            assert t["tiles"] > 1
        start = perturbed_state(s.nel(0), s.far_field()[:5], seed=7, amplitude=amplitude)
        em = jse.JstOracle(oracle, case, "local", cfl)
        for k2, k4 in jse.GPU_PAIRS + ((600.0, 0.0),):         # (the last: the second-difference switch alone, saturated on some edges)
            em.set_jst(k2, k4, 1)
            s.set_jst(k2, k4, 1)
            s.set_time_step("local", cfl)
            em.oc.array(0, "variables")[:] = start.ravel()
            s.set(0, "variables", start)
            Cn, L, nu, r = em.terms(0)
            want_f = em.stage_fluxes(0)
            s.zero_fluxes(0)
            s.compute_fluxes(0)
            what = f"{os.path.basename(case)} ({k2}, {k4})"
            _same(s.get(0, "jst_laplacian"), L, f"{what}: L")
            _same(s.get(0, "jst_sensor"), nu, f"{what}: nu")
            _same(s.get(0, "jst_radius"), r, f"{what}: r")
            _same(s.get(0, "fluxes"), want_f, f"{what}: F + C")
            assert Cn.any() and np.isfinite(Cn).all()
            if k2 == 600.0:
                e2, _ = jse.switches(nu[em.ea[0]], nu[em.eb[0]], k2, k4)
                assert (e2 == 1.0).any() and (e2 < 1.0).any()
            # C alone: the internal fluxes of a solver without JST, then the same call with JST: the difference of the two
            # launches' results is C added to F(internal) in one addition
            s.zero_fluxes(0)
            s.set_jst(0.0, 0.0, 0)
            s.compute_flux_edge(0)
            f_int = s.get(0, "fluxes")
            s.zero_fluxes(0)
            s.set_jst(k2, k4, 1)
            s.compute_flux_edge(0)
            _same(s.get(0, "fluxes"), f_int + Cn, f"{what}: F(internal) + C")
            s.zero_fluxes(0)
            assert em.sweeps(0, 2) == 0
            s.smooth(0, 2)
            _same(s.get(0, "variables"), em.variables(0), f"{what}: two sweeps")
            assert s.pending_invalid_state()[0] == 0
        em.close()
        s.close(); mesh.close()


def test_composition_with_residual_smoothing(oracle):
    """JST on all levels with residual smoothing (0.5, 2) under local steps: the composed emulator's bits."""
    case = jse.COMPOSED_CASE
    mode, cfl, smoothing = jse.COMPOSED_SMOOTHING
    em = jse.JstOracle(oracle, case, mode, cfl, *smoothing, kappa2=jse.KAPPA2, kappa4=jse.KAPPA4, levels="all")
    rc, want_rms = em.cycles(K)
    assert rc == 0
    for graph in (0, 1):
        mesh, s = _solver(case, graph)
        s.set_time_step(mode, cfl)
        s.set_residual_smoothing(*smoothing)
        s.set_jst(levels=s.num_levels)
        assert s.jst() == (jse.KAPPA2, jse.KAPPA4, s.num_levels)
        rms = s.run_cycles(K)
        _same(rms, want_rms, f"smoothing + JST graph={graph}: RMS history")
        for l in range(s.num_levels):
            _same(s.get(l, "variables"), em.variables(l), f"smoothing + JST graph={graph}: level {l}")
        s.close(); mesh.close()
    em.close()


def test_composition_with_dual_time(oracle):
    """JST on all levels with dual time stepping (BDF1 then BDF2, with one smoothing iteration): 2 steps x 3 cycles, the composed
    emulator's state, time levels and RMS history."""
    case = jse.COMPOSED_CASE
    name, mode, cfl, smoothing, order = jse.COMPOSED_DUAL
    steps, cycles = jse.COMPOSED_DUAL_STEPS, jse.COMPOSED_DUAL_CYCLES
    em = jse.JstOracle(oracle, case, mode, cfl, *smoothing, kappa2=jse.KAPPA2, kappa4=jse.KAPPA4, levels="all")
    v = em.oc.array(0, "variables").reshape(-1, 5)
    v[:] = dte.start_state(case, em.ff17[:5], len(v))
    em.set_dual_time(dte.GPU_DT[case][name])
    em.set_order(order)
    rc, want_rms = em.advance(steps, cycles)
    assert rc == 0 and em.effective_order() == 2
    mesh, s = _solver(case)
    s.set_time_step(mode, cfl)
    s.set_residual_smoothing(*smoothing)
    s.set_jst(levels=s.num_levels)
    s.set(0, "variables", dte.start_state(case, s.far_field()[:5], s.nel(0)))
    s.set_dual_time(dte.GPU_DT[case][name])
    s.dual_time_order(order)
    rms = s.advance(steps, cycles).ravel()
    _same(rms, want_rms, "dual time + JST: RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), em.variables(l), f"dual time + JST: level {l}")
        _same(s.get(l, "time_n"), em.Wn[l], f"dual time + JST: Wn, level {l}")
        _same(s.get(l, "time_n1"), em.Wn1[l], f"dual time + JST: Wn1, level {l}")
    # switching dual time off keeps the JST order of the RMS; switching JST off as well returns to the plain solver
    s.set_dual_time(0.0)
    em.set_dual_time(0.0)
    rc, want_rms = em.cycles(1)
    _same(s.run_cycles(1), want_rms, "JST after dual time was switched off: RMS")
    s.close(); mesh.close()
    em.close()


@pytest.mark.parametrize("case", CASES)
def test_switching_between_runs(case, oracle):
    """On, off and on again between runs keeps the state and equals the emulator driven the same way (graphs off and on); after
    switching off, the rest of the run equals a solver that never had it on, started from that state."""
    legs = [(2.5, 0.15625, 1), (0.0, 0.0, 0), (0.0, 0.15625, "all"), (0.0, 0.0, 0), (2.5, 0.0, 1)]
    em = jse.JstOracle(oracle, case, "local", 1.5)
    want = []
    for k2, k4, lv in legs:
        em.set_jst(k2, k4, lv)
        rc, rms = em.cycles(K)
        assert rc == 0
        want.append((rms, [em.variables(l) for l in range(em.n)]))
    em.close()
    for graph in (0, 1):
        mesh, s = _solver(case, graph)
        s.set_time_step("local", 1.5)
        for k, (k2, k4, lv) in enumerate(legs):
            before = s.get(0, "variables")
            s.set_jst(k2, k4, _levels(s, lv))
            assert s.jst() == (k2, k4, _levels(s, lv))
            _same(s.get(0, "variables"), before, "the setter keeps the state")
            if k == 1:
                ref_mesh, ref = _solver(case, graph)
                ref.set_time_step("local", 1.5)
                for l in range(s.num_levels):
                    ref.set(l, "variables", s.get(l, "variables"))
                ref.run_cycles(K)
            rms = s.run_cycles(K)
            for l in range(s.num_levels):
                _same(s.get(l, "variables"), want[k][1][l], f"{case} graph={graph} leg {k} ({k2}, {k4}, {lv}): level {l}")
            if lv:
                _same(rms, want[k][0], f"{case} graph={graph} leg {k}: RMS history")
            else:
                assert np.allclose(rms, want[k][0], rtol=1e-12, atol=0)    # (off: the library's own order of the sum, as ever)
            if k == 1:
                for l in range(s.num_levels):
                    _same(s.get(l, "variables"), ref.get(l, "variables"), f"{case} graph={graph}: against a solver that never had it, level {l}")
                ref.close(); ref_mesh.close()
        s.close()
        mesh.close()


def _golden_cycles(case):
    meta = dict(l.strip().split(" = ") for l in open(os.path.join(fse.GOLDEN, case, "case.txt")))
    return int(meta["cycles"])


def test_refusals():
    """Bad numbers, mid-sweep, a partitioned solver, a group member, the sweep_* calls, group creation and rank attachment while
    on: error code 1, "JST" in the message, nothing changed."""
    import mgcfd
    mesh, s = _solver("m6_2lvl")
    ref_mesh, ref = _solver("m6_2lvl")
    for t in (s, ref):
        t.set_jst(2.5, 0.15625, 1)
    for k2, k4, lv in ((-1.0, 0.1, 1), (2.5, -0.1, 1), (float("nan"), 0.1, 1), (2.5, float("inf"), 1), (2.5, 0.1, -1), (0.0, 0.0, 1),
                       (float("nan"), 0.1, 0)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            s.set_jst(k2, k4, lv)
        assert e.value.code == 1 and "JST" in str(e.value)
    assert s.jst() == (2.5, 0.15625, 1)
    for call in (lambda: s.sweep_begin(0), lambda: s.sweep_begin_partials(0), lambda: s.sweep_flux0(0), lambda: s.sweep_stage(0, 0),
                 lambda: s.sweep_end(0), lambda: s.sweep_end_partials(0), lambda: s.sweep_begin(1)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1 and "JST" in str(e.value)
    with pytest.raises(mgcfd.MgcfdError) as e:
        mgcfd.Group([s])
    assert e.value.code == 1 and "JST" in str(e.value)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.rank_attach_plain(0, 1)
    assert e.value.code == 1 and "JST" in str(e.value)
    with pytest.raises(mgcfd.MgcfdError):
        s.set(0, "jst_sensor", np.zeros(s.nel(0)))
    with pytest.raises(mgcfd.MgcfdError):
        s.get(1, "jst_sensor")                                # (never on for level 1)
    for t in (s, ref):
        t.run_cycles(1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "a cycle after the refused calls")
    # mid-sweep: the split sweep runs with JST off; the setter is refused until its last stage has run
    for t in (s, ref):
        t.set_jst(0.0, 0.0, 0)
    assert s.jst() == (0.0, 0.0, 0)
    s.sweep_begin(0)
    s.sweep_stage(0, 0, partials=False)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_jst(2.5, 0.15625, 1)
    assert e.value.code == 1 and "JST" in str(e.value) and "sweep is under way" in str(e.value)
    assert s.jst() == (0.0, 0.0, 0)
    s.sweep_stage(0, 1, partials=False)
    s.sweep_stage(0, 2, partials=False)
    ref.smooth(0, 1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "the sweep the refused call interrupted")
    # a group member, and a partitioned solver
    g = mgcfd.Group([s])
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_jst(2.5, 0.15625, 1)
    assert e.value.code == 1 and "JST" in str(e.value)
    s.set_jst(0.0, 0.0, 0)                                    # switching off is always allowed
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
        t.set_jst(2.5, 0.15625, 1)
    assert e.value.code == 1 and "JST" in str(e.value)
    assert t.jst() == (0.0, 0.0, 0)
    t.set_jst(2.5, 0.15625, 0)
    t.close()
    mesh.close()


@pytest.mark.parametrize("case,mode,cfl,k2,k4,lv", PATHS)
def test_fast_mode(case, mode, cfl, k2, k4, lv, oracle):
    """exact = 0 (FMA contraction, the order-free flux kernel for F) within the bound
    tests/test_gpu_residual_smoothing.py::test_fast_mode uses: 1e-10 of the largest value per level, RMS rtol 1e-9."""
    want_rms, want_v, _ = _emulate(oracle, case, mode, cfl, k2, k4, lv)
    mesh, s = _solver(case, exact=0)
    s.set_time_step(mode, cfl)
    s.set_jst(k2, k4, _levels(s, lv))
    rms = s.run_cycles(K)
    assert np.allclose(rms, want_rms, rtol=RMS_FAST, atol=0)
    for l in range(s.num_levels):
        rel = np.abs(s.get(l, "variables") - want_v[l]).max() / max(np.abs(want_v[l]).max(), 1e-300)
        print(case, mode, cfl, k2, k4, lv, "level", l, "rel", rel)
        assert rel <= REL_RUN, f"{case} level {l}: {rel:.3e}"
    s.close()
    mesh.close()


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
    """--jst (the Python defaults), the three value flags (each implies --jst), the config keys and --gpus 2 mesh copies: the dump
    is the %.17e rendering of the emulator's state, the RMS lines its history, LoopNumIters.csv the plain run's counts; with
    --gpus-partition an error before any GPU work."""
    dup = fse.case_duplicate(case)
    name = f"variables.size={dup}x.cycles={K}.level=0"
    want_rms, want_v, _ = _emulate(oracle, case, "reference", 0.5, jse.KAPPA2, jse.KAPPA4, 1)
    want = fse.render_variables(want_v[0]).encode()
    plain = _run_driver(tmp_path / "plain", case, ["--output-variables"], K)
    conf = tmp_path / "run.conf"
    conf.write_text("jst = Y\n")
    conf2 = tmp_path / "run2.conf"
    conf2.write_text("jst_kappa2 = 2.5\njst_kappa4 = 0.15625\njst_levels = 1\n")
    for tag, extra in (("default", ["--jst"]), ("said", ["--jst-kappa2", "2.5", "--jst-kappa4=0.15625", "--jst-levels", "1"]),
                       ("one", ["--jst-kappa2=2.5"]), ("conf", ["-c", str(conf)]), ("conf2", ["-c", str(conf2)]),
                       ("two", ["--jst", "--gpus", "2", "--gpus-share-device"])):
        d = tmp_path / tag
        if tag == "two" and len(want_v) == 1:                  # (a single level on two GPUs is split over them: refused by the library)
            r = _run_driver(d, case, ["--output-variables"] + extra, K, ok=False)
            assert "JST" in (r.stdout + r.stderr)
            continue
        r = _run_driver(d, case, ["--output-variables"] + extra, K)
        assert (d / "out" / name).read_bytes() == want, f"{case} {tag}"
        lines, plain_lines = _strip(r.stdout), _strip(plain.stdout)
        if tag != "two":
            assert len(lines) == len(plain_lines)
            rms_lines = [l for l in lines if "(RMS = " in l]
            assert rms_lines == [(f"Cycle {i + 1} / {K}" if len(want_v) <= 1 else f"MG cycle {i + 1} / {K}") + " (RMS = %.3e)" % want_rms[i] for i in range(K)]
            assert _loop_iters(d) == _loop_iters(tmp_path / "plain")
    _, v_all, _ = _emulate(oracle, case, "local", jse.LOCAL_CFL, 0.0, jse.KAPPA4, "all")
    d = tmp_path / "all"
    _run_driver(d, case, ["--output-variables", "--time-step=local", f"--cfl={jse.LOCAL_CFL}", "--jst-kappa2=0", "--jst-levels=8"], K)
    assert (d / "out" / name).read_bytes() == fse.render_variables(v_all[0]).encode()
    r = _run_driver(tmp_path / "part", case, ["--jst", "--gpus", "2", "--gpus-partition", "--gpus-share-device"], K, ok=False)
    assert "jst" in (r.stdout + r.stderr).lower()
    assert not [n for n in os.listdir(tmp_path / "part" / "out") if n.startswith("variables")]
    for bad in (["--jst-kappa2", "-1"], ["--jst-kappa4", "nan"], ["--jst-levels", "-1"], ["--jst-kappa2", "0", "--jst-kappa4", "0"]):
        _run_driver(tmp_path / "bad", case, bad, K, ok=False)


@pytest.mark.parametrize("case", CASES)
def test_defaults_reproduce_the_golden_output(case, tmp_path):
    """Without the flags: variables.level0.txt of the golden case byte for byte and the golden LoopNumIters.csv's counts (as
    tests/test_gpu_parity.py compares them); --jst-levels 0 spelled out is that run too, stdout included, and so is the Python
    API after on and off again."""
    cycles, dup = _golden_cycles(case), fse.case_duplicate(case)
    golden = open(os.path.join(fse.GOLDEN, case, "variables.level0.txt"), "rb").read()
    name = f"variables.size={dup}x.cycles={cycles}.level=0"
    plain = _run_driver(tmp_path / "plain", case, ["--output-variables"], cycles)
    assert (tmp_path / "plain" / "out" / name).read_bytes() == golden
    off = _run_driver(tmp_path / "off", case, ["--output-variables", "--jst", "--jst-levels", "0"], cycles)
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
    assert s.jst() == (0.0, 0.0, 0)
    s.set_jst()
    s.set_jst(levels=0)                                       # on and off again before the run: the default run
    s.run_cycles(cycles)
    assert fse.render_variables(s.get(0, "variables")).encode() == golden
    s.close()
    mesh.close()


def test_polar_with_jst(oracle):
    """Solver.polar(jst=(kappa2, kappa4, levels)) = set_jst once, then the polar; the solver keeps it."""
    case, alphas, mach = fse.POLAR_CASE, fse.POLAR_ALPHAS, fse.POLAR_MACH
    mesh, s = _solver(case)
    pol = s.polar(alphas, K, mach=mach, jst=(jse.KAPPA2, jse.KAPPA4, 1))
    assert s.jst() == (jse.KAPPA2, jse.KAPPA4, 1)
    em = jse.JstOracle(oracle, case, kappa2=jse.KAPPA2, kappa4=jse.KAPPA4, levels=1)
    for k, (al, p) in enumerate(zip(alphas, pol)):
        em.set_far_field(fse.free_stream_constants(mach, al), reinitialise=(k == 0))
        rc, rms = em.cycles(K)
        assert rc == 0
        _same(p["rms"], rms, f"polar, angle {al}: RMS history")
    _same(s.get(0, "variables"), em.variables(0), "the polar's last state")
    em.close()
    s.close(); mesh.close()


def test_device_resources():
    """A solver that never enables it holds what it holds today; enabling adds the seven arrays of a level (one allocation) per
    JST level and level 0's numbering for the RMS, once; destroy returns to the baseline."""
    import mgcfd
    base = mgcfd.live_device_resources()
    mesh, a = _solver("m6_3lvl")
    a.run_cycles(1)
    a.set_jst(levels=0)
    after_run = mgcfd.live_device_resources()
    mesh_b, b = _solver("m6_3lvl")
    b.run_cycles(1)
    both = mgcfd.live_device_resources()
    assert both["allocations"] - after_run["allocations"] == after_run["allocations"] - base["allocations"], "a never-enabled solver: today's count"
    b.set_jst(levels=2)
    on = mgcfd.live_device_resources()
    assert on["allocations"] - both["allocations"] == 2 + 1
    assert on["bytes"] - both["bytes"] >= sum(7 * 8 * b.nel(l) for l in range(2))
    b.set_jst(levels=0)
    b.set_jst(0.0, 0.3, 2)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"], "allocated once"
    b.set_jst(levels=3)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"] + 1, "a further level: its seven arrays"
    b.run_cycles(1)
    assert b.bench_jst(0, 0, 3) > 0.0 and b.bench_jst(0, 1, 3) > 0.0
    b.close(); mesh_b.close()
    assert mgcfd.live_device_resources()["allocations"] == after_run["allocations"]
    a.close(); mesh.close()
    end = mgcfd.live_device_resources()
    assert end["allocations"] == base["allocations"] and end["bytes"] == base["bytes"]
