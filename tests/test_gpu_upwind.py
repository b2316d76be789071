"""GPU tests of the upwind flux (mgcfd_set_upwind) on one solver and in the drop-in binary, everything bit for bit against the numpy
emulator (tests/upwind_emulator.py): the kernels' results (Gl, psi, F = B + U, U alone) per limiter and instantiation from a
perturbed and from a supersonic state; whole runs (state of every level, RMS history); composition with residual smoothing, dual
time, FAS, the viscous terms and the cycle control; switching; the JST exclusion and the other refusals; allocations; the fast mode;
polar; the driver's flags.  tests/test_host_upwind.py asserts on the CPU that every run here stays valid."""
import os
import subprocess

import numpy as np
import pytest

import dual_time_emulator as dte
import free_stream_emulator as fse
import upwind_emulator as ue
import viscous_emulator as ve

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
K = ue.GPU_CYCLES


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape or got.size == want.size, what
    assert np.array_equal(_bits(got).ravel(), _bits(want).ravel()), \
        f"{what}: {int((_bits(got).ravel() != _bits(want).ravel()).sum())} of {got.size} differ, max |difference| {np.nanmax(np.abs(got.ravel() - want.ravel())):.3e}"


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("upwind_lattices")
    return {name: ue.write_lattice(name, d) for name in ue.GPU_LATTICES}


def _case(lattices, key):
    return lattices.get(key, key)


def _solver(case, graph=0, exact=1):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    s.set_option("graph", graph)
    s.set_option("exact", exact)
    return mesh, s


def _n(s, lv):
    return s.num_levels if lv == "all" else lv


def _state(kind, nel, ff):
    return ue.start_state(nel, ff) if kind == "perturbed" else ue.supersonic_state(nel, ff)


@pytest.mark.parametrize("state", ["perturbed", "supersonic"])
@pytest.mark.parametrize("key", ue.GPU_CASES)
def test_kernels(key, state, oracle, lattices):
    """Level 0 (several tiles with halos on lattice A, long rows and overflow lists on tet_2lvl, degrees 3-14 on mixed_2lvl) and the
    coarsest level, every limiter and both flux instantiations: Gl and psi as read back, F = B + U after mgcfd_compute_fluxes
    and U alone after mgcfd_compute_flux_edge from zero fluxes."""
    case = _case(lattices, key)
    mesh, s = _solver(case)
    em = ue.UpwindOracle(oracle, case)
    n = s.num_levels
    for l in (0, n - 1):
        W = _state(state, s.nel(l), s.far_field()[:5])
        s.set(l, "variables", W)
        em._var(l)[:] = W
    if state == "supersonic":
        q = ue.primitives5(em._var(0))
        mach = np.sqrt((q[:, 1:4] ** 2).sum(axis=1)) / np.sqrt(ue.GAMMA * q[:, 4] / q[:, 0])
        assert mach.min() > 1.5
    for limiter in ue.GPU_LIMITERS:
        for muscl in (0, n):
            s.set_upwind(n, muscl, limiter)
            em.set_upwind(n, muscl, limiter)
            assert s.upwind() == (n, muscl, limiter, ue.VENKAT_K, ue.ENTROPY_FIX)
            for l in (0, n - 1):
                what = f"{key} {state} {limiter} muscl={muscl} level {l}"
                want_f = em.stage_fluxes(l)
                s.zero_fluxes(l)
                s.compute_fluxes(l)
                _same(s.get(l, "fluxes"), want_f, f"{what}: B + U")
                U = em.last_U[l]
                assert np.isfinite(U).all() and U.any()
                if muscl:
                    _same(s.get(l, "upwind_gradient"), em.upwind_gradient(l), f"{what}: Gl")
                    _same(s.get(l, "upwind_limiter"), em.last_psi[l], f"{what}: psi")
                    # (the inputs exercise the limiter: Barth-Jespersen binds somewhere on every level; on the goldens, whose
                    #  weights are damped at load, Venkatakrishnan's e2 swamps the differences and psi stays within rounding of 1)
                    assert (em.last_psi[l] <= 1.0).all()
                    if limiter == "barth-jespersen":
                        assert (em.last_psi[l] < 1.0).any()
                s.zero_fluxes(l)
                s.compute_flux_edge(l)
                _same(s.get(l, "fluxes"), 0.0 + U, f"{what}: U alone")
                s.zero_fluxes(l)
    em.close()
    s.close(); mesh.close()


def test_kernel_paths(oracle, tmp_path):
    """The shapes at which the gathers can go wrong and the small cases do not reach, as tests/test_gpu_jst.py::test_kernel_paths
    finds them: halo nodes beyond the LDS table (the overflow list) and long rows (the tail lists), on a generated tetrahedral
    level of 30,000 nodes.  From a perturbed state, first order and every limiter under MUSCL: Gl, psi and B + U."""
    import mgcfd
    from mgcfd import meshgen
    mg = meshgen.MultigridMesh(mesh_name="fvcorr")
    mg.levels.append(meshgen.make_tet_level(30000, seed=0, wall_below=2.0))
    d = tmp_path / "tet"
    os.makedirs(d / "input")
    meshgen.write_input(mg, str(d / "input"))
    (d / "case.txt").write_text("duplicate = 1\n")
    em = ue.UpwindOracle(oracle, str(d))
    # (the mesh loader leaves the coordinates out of a single-level fvcorr input: the level is handed over with them)
    mesh = mgcfd.Mesh("input.dat", fse.case_input(str(d)), 1)
    level = dict(mesh.level(0))
    level["coords"] = em.X[0]
    s = mgcfd.Solver.from_arrays([level], mesh.variant)
    t = s.tiling(0)
    print(t)
    assert t["tiles"] > 1 and t["overflow_refs"] > 0 and t["list_entries"] > 0
    from conftest import perturbed_state
    W = perturbed_state(s.nel(0), s.far_field()[:5], seed=7, amplitude=0.002)
    s.set(0, "variables", W)
    em._var(0)[:] = W
    for limiter, muscl in (("none", 0), ("none", 1), ("barth-jespersen", 1), ("venkatakrishnan", 1)):   # (first order reads no limiter)
        s.set_upwind(1, muscl, limiter)
        em.set_upwind(1, muscl, limiter)
        want_f = em.stage_fluxes(0)
        assert np.isfinite(em.last_U[0]).all() and em.last_U[0].any()
        s.zero_fluxes(0)
        s.compute_fluxes(0)
        what = f"tet 30000 {limiter} muscl={muscl}"
        _same(s.get(0, "fluxes"), want_f, f"{what}: B + U")
        if muscl:
            _same(s.get(0, "upwind_gradient"), em.upwind_gradient(0), f"{what}: Gl")
            _same(s.get(0, "upwind_limiter"), em.last_psi[0], f"{what}: psi")
        s.zero_fluxes(0)
    em.close()
    s.close(); mesh.close()


_emulated = {}


def _emulate(oracle, case, key, mode, cfl, lv, muscl):
    """(rms, variables per level) of K cycles: computed once per combination, shared and left unchanged."""
    k = (key, mode, cfl, lv, muscl)
    if k not in _emulated:
        em = ue.configured(oracle, case, mode, cfl, lv, muscl)
        rc, rms = em.cycles(K)
        assert rc == 0
        _emulated[k] = (rms, [em.variables(l) for l in range(em.n)])
        em.close()
    return _emulated[k]


def _configure(s, mode, cfl, lv, muscl, limiter=ue.RUN_LIMITER):
    s.set_time_step(mode, cfl)
    s.set(0, "variables", ue.start_state(s.nel(0), s.far_field()[:5]))
    s.set_upwind(_n(s, lv), _n(s, muscl), limiter)


@pytest.mark.parametrize("key,mode,cfl,lv,muscl", ue.gpu_runs())
def test_runs(key, mode, cfl, lv, muscl, oracle, lattices):
    """K cycles under the reference step and under local steps, upwind on level 0 alone and on all levels, reconstruction on
    none, level 0 and all: the state of every level and the RMS history."""
    case = _case(lattices, key)
    want_rms, want_v = _emulate(oracle, case, key, mode, cfl, lv, muscl)
    mesh, s = _solver(case, graph=1)                           # (MGCFD_OPT_GRAPH is accepted: the launches run directly)
    _configure(s, mode, cfl, lv, muscl)
    rms = s.run_cycles(K)
    what = f"{key} {mode} {cfl} levels={lv} muscl={muscl}"
    print(what, "rms", rms)
    _same(rms, want_rms, f"{what}: RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), want_v[l], f"{what}: level {l}")
    assert s.pending_invalid_state()[0] == 0
    s.close(); mesh.close()


def test_loop_counts_and_timing(oracle, lattices):
    """The iteration counts are those of the run without the upwind flux; the launches are timed as the flux loop."""
    case = lattices["B"]
    mesh, plain = _solver(case)
    plain.set_time_step("local", ue.LOCAL_CFL)
    plain.run_cycles(K)
    want = [plain.loop_iters(l) for l in range(plain.num_levels)]
    plain.close(); mesh.close()
    mesh, s = _solver(case)
    s.set_option("timing", 1)
    _configure(s, "local", ue.LOCAL_CFL, "all", 1)
    s.run_cycles(K)
    for l in range(s.num_levels):
        assert s.loop_iters(l) == want[l]
    assert s.loop_times(0)["flux"] > 0.0
    s.close(); mesh.close()


@pytest.mark.parametrize("name,mode,cfl,smoothing,order,fas,viscous,cycle", ue.COMPOSED, ids=[c[0] for c in ue.COMPOSED])
def test_composition(name, mode, cfl, smoothing, order, fas, viscous, cycle, oracle, lattices):
    """Lattice A, upwind on all levels with MUSCL on level 0, with residual smoothing, dual time (BDF2), FAS, the viscous terms
    with no-slip walls, and a W cycle with a post-sweep on level 0: the composed emulator's state and RMS history."""
    case = lattices["A"]
    em = ue.configured(oracle, case, mode, cfl, "all", 1, smoothing=smoothing, fas=fas)
    mesh, s = _solver(case)
    if smoothing[1]:
        s.set_residual_smoothing(*smoothing)
    if fas:
        s.set_fas(True)
    _configure(s, mode, cfl, "all", 1)
    if viscous:
        em.set_viscous(ve.CELL_RE_MU, ve.PRANDTL, 1, ve.VISCOUS_CFL, "all")
        s.set_viscous(ve.CELL_RE_MU, ve.PRANDTL, True, ve.VISCOUS_CFL, s.num_levels)
    if cycle:
        pre, post = [1] * em.n, [cycle[1]] + [1] * (em.n - 1)
        em.set_cycle(cycle[0], pre, post)
        s.set_cycle(cycle[0], pre, post)
    if order is None:
        rc, want_rms = em.cycles(K)
        rms = s.run_cycles(K)
    else:
        dt = dte.pick_dt(oracle, case, mode, cfl)
        em.set_dual_time(dt)
        em.set_order(order)
        rc, want_rms = em.advance(ue.DUAL_STEPS, ue.DUAL_CYCLES)
        s.set_dual_time(dt)
        s.dual_time_order(order)
        rms = s.advance(ue.DUAL_STEPS, ue.DUAL_CYCLES).ravel()
    assert rc == 0
    _same(rms, want_rms, f"{name}: RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), em.variables(l), f"{name}: level {l}")
        if fas and l >= 1:
            _same(s.get(l, "fas_forcing"), em.P[l], f"{name}: P, level {l}")
    em.close()
    s.close(); mesh.close()


def test_on_then_off_equals_the_parent(oracle):
    """A solver that had the upwind flux on for K cycles and then off runs the rest as one that never had it, started from that
    state (graphs off and on); a solver it was switched on and off again on before the run gives the golden run's bits."""
    case = "tet_2lvl"
    for graph in (0, 1):
        mesh, s = _solver(case, graph)
        s.set_upwind(s.num_levels, 1)
        s.run_cycles(K)
        before = s.get(0, "variables")
        s.set_upwind(0)
        assert s.upwind() == (0, 0, "none", 0.0, 0.0)
        _same(s.get(0, "variables"), before, "the setter keeps the state")
        ref_mesh, ref = _solver(case, graph)
        for l in range(s.num_levels):
            ref.set(l, "variables", s.get(l, "variables"))
        s.run_cycles(K)
        ref.run_cycles(K)
        for l in range(s.num_levels):
            _same(s.get(l, "variables"), ref.get(l, "variables"), f"graph={graph}: level {l}")
        ref.close(); ref_mesh.close()
        s.close(); mesh.close()
    mesh, s = _solver(case)
    s.set_upwind(1)
    s.set_upwind(0)
    got = s.run_cycles(K)
    ref_mesh, ref = _solver(case)
    _same(got, ref.run_cycles(K), "on and off again before the run: RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), ref.get(l, "variables"), f"on and off again before the run: level {l}")
    ref.close(); ref_mesh.close()
    s.close(); mesh.close()


def test_jst_and_upwind_exclude_each_other():
    """Either setter first: the second is refused with nothing changed; after the first is switched off the second is taken."""
    import mgcfd
    mesh, s = _solver("m6_2lvl")
    s.set_upwind(1, 0, "none")
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_jst(levels=1)
    assert e.value.code == 1 and "upwind" in str(e.value)
    assert s.jst() == (0.0, 0.0, 0) and s.upwind()[0] == 1
    s.set_upwind(0)
    s.set_jst(levels=2)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_upwind(1, 0, "none")
    assert e.value.code == 1 and "JST" in str(e.value)
    assert s.upwind()[0] == 0 and s.jst()[2] == 2
    s.set_upwind(0)                                            # switching off is always allowed
    s.set_jst(levels=0)
    s.set_upwind(2, 1)
    assert s.upwind()[:3] == (2, 1, "venkatakrishnan")
    s.close(); mesh.close()


def test_refusals(tmp_path):
    """Bad numbers, muscl_levels > levels, an unknown limiter, a level without coordinates, mid-sweep, a group member, a partitioned
    solver; the sweep_* calls, group creation and rank attachment while on: error code 1, nothing changed."""
    import mgcfd
    mesh, s = _solver("m6_2lvl")
    ref_mesh, ref = _solver("m6_2lvl")
    for t in (s, ref):
        t.set_upwind(1, 1)
    nan, inf = float("nan"), float("inf")
    for args in ((-1, 0, "none", 5.0, 0.1), (1, -1, "none", 5.0, 0.1), (1, 2, "none", 5.0, 0.1), (1, 1, 3, 5.0, 0.1), (1, 1, -1, 5.0, 0.1),
                 (1, 1, "none", nan, 0.1), (1, 1, "none", inf, 0.1), (1, 1, "none", 0.0, 0.1), (1, 1, "none", -5.0, 0.1),
                 (1, 1, "none", 5.0, nan), (1, 1, "none", 5.0, -0.1), (1, 1, "none", 5.0, inf), (1, 1, "none", 5.0, 1.5), (0, 0, "none", nan, 0.1)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            s.set_upwind(*args)
        assert e.value.code == 1 and "upwind" in str(e.value), args
    assert s.upwind() == (1, 1, "venkatakrishnan", ue.VENKAT_K, ue.ENTROPY_FIX)
    for call in (lambda: s.sweep_begin(0), lambda: s.sweep_begin_partials(0), lambda: s.sweep_flux0(0), lambda: s.sweep_stage(0, 0),
                 lambda: s.sweep_end(0), lambda: s.sweep_end_partials(0), lambda: s.sweep_begin(1)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1 and "upwind" in str(e.value)
    with pytest.raises(mgcfd.MgcfdError) as e:
        mgcfd.Group([s])
    assert e.value.code == 1 and "upwind" in str(e.value)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.rank_attach_plain(0, 1)
    assert e.value.code == 1 and "upwind" in str(e.value)
    with pytest.raises(mgcfd.MgcfdError):
        s.set(0, "upwind_limiter", np.zeros((s.nel(0), 5)))
    with pytest.raises(mgcfd.MgcfdError):
        s.get(1, "upwind_gradient")                           # (level 1 never reconstructed)
    with pytest.raises(mgcfd.MgcfdError):
        s.bench_upwind(1, 1, 2)
    for t in (s, ref):
        t.run_cycles(1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "a cycle after the refused calls")
    # mid-sweep: the split sweep runs with the flux off; the setter is refused until its last stage has run
    for t in (s, ref):
        t.set_upwind(0)
    s.sweep_begin(0)
    s.sweep_stage(0, 0, partials=False)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_upwind(1)
    assert e.value.code == 1 and "upwind" in str(e.value) and "sweep is under way" in str(e.value)
    assert s.upwind()[0] == 0
    s.sweep_stage(0, 1, partials=False)
    s.sweep_stage(0, 2, partials=False)
    ref.smooth(0, 1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "the sweep the refused call interrupted")
    g = mgcfd.Group([s])
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_upwind(1)
    assert e.value.code == 1 and "upwind" in str(e.value)
    s.set_upwind(0)
    g.close()
    s.close(); ref.close()
    mesh.close(); ref_mesh.close()
    # a partitioned solver
    from mgcfd.partition import partition_hierarchy, rcb_partition
    mesh = mgcfd.Mesh("input.dat", fse.case_input("m6_2lvl"), 1)
    levels = [mesh.level(l) for l in range(mesh.num_levels)]
    H = partition_hierarchy(levels, rcb_partition(np.asarray(levels[0]["coords"]).reshape(-1, 3), 2))
    lv, owned, keys = H[0].solver_args()
    t = mgcfd.Solver.from_arrays(lv, mesh.variant, n_owned=owned, order_keys=keys)
    with pytest.raises(mgcfd.MgcfdError) as e:
        t.set_upwind(1, 0)
    assert e.value.code == 1 and "upwind" in str(e.value)
    assert t.upwind()[0] == 0
    t.close()
    # a level created without coordinates: first order is taken, reconstruction refused
    mesh.close()
    mesh = mgcfd.Mesh("input.dat", fse.case_input("fvcorr_1lvl"), 1)
    assert len(mesh.level(0)["coords"]) == 0                  # (a single-level fvcorr input is loaded without its .coords file)
    t = mgcfd.Solver.from_arrays([mesh.level(0)], mesh.variant)
    with pytest.raises(mgcfd.MgcfdError) as e:
        t.set_upwind(1, 1)
    assert e.value.code == 1 and "coordinates" in str(e.value)
    assert t.upwind()[0] == 0
    t.set_upwind(1, 0)
    t.run_cycles(1)
    t.close()
    mesh.close()


def test_device_resources():
    """A solver that never enables it holds what it holds today; a first-order level allocates nothing; a MUSCL level adds Gl with
    psi (one allocation) and its coordinates; level 0's numbering for the RMS comes once; destroy returns to the baseline."""
    import mgcfd
    base = mgcfd.live_device_resources()
    mesh, a = _solver("m6_3lvl")
    a.run_cycles(1)
    a.set_upwind(0)
    after_run = mgcfd.live_device_resources()
    mesh_b, b = _solver("m6_3lvl")
    b.run_cycles(1)
    both = mgcfd.live_device_resources()
    assert both["allocations"] - after_run["allocations"] == after_run["allocations"] - base["allocations"], "a never-enabled solver: today's count"
    b.set_upwind(3, 0, "none")
    first = mgcfd.live_device_resources()
    assert first["allocations"] - both["allocations"] == 1, "first order: level 0's numbering alone"
    b.set_upwind(3, 2)
    on = mgcfd.live_device_resources()
    assert on["allocations"] - first["allocations"] == 2 * 2, "per MUSCL level: Gl with psi, and the coordinates"
    assert on["bytes"] - first["bytes"] >= sum(23 * 8 * b.nel(l) for l in range(2))
    b.set_upwind(3, 0)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"] - 2, "the coordinates go with the MUSCL levels"
    b.set_upwind(3, 2, "barth-jespersen")
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"], "Gl and psi: allocated once"
    b.run_cycles(1)
    assert b.bench_upwind(0, "gradient", 3) > 0.0 and b.bench_upwind(0, "flux", 3) > 0.0 and b.bench_upwind(2, "flux", 3) > 0.0
    b.close(); mesh_b.close()
    assert mgcfd.live_device_resources()["allocations"] == after_run["allocations"]
    a.close(); mesh.close()
    end = mgcfd.live_device_resources()
    assert end["allocations"] == base["allocations"] and end["bytes"] == base["bytes"]


def test_fast_mode_gives_the_same_u(oracle):
    """MGCFD_OPT_EXACT = 0 changes nothing in the upwind kernels: Gl, psi and U alone carry the exact mode's bits."""
    case = "mixed_2lvl"
    em = ue.UpwindOracle(oracle, case)
    mesh, s = _solver(case, exact=0)
    W = ue.start_state(s.nel(0), s.far_field()[:5])
    s.set(0, "variables", W)
    em._var(0)[:] = W
    s.set_upwind(1, 1)
    em.set_upwind(1, 1)
    U, Gl, psi, _, _ = em.upwind_terms(0)
    s.zero_fluxes(0)
    s.compute_flux_edge(0)
    _same(s.get(0, "fluxes"), 0.0 + U, "U under the fast mode")
    _same(s.get(0, "upwind_gradient"), Gl.reshape(-1, 15), "Gl under the fast mode")
    _same(s.get(0, "upwind_limiter"), psi, "psi under the fast mode")
    em.close()
    s.close(); mesh.close()


def test_polar_with_upwind(oracle):
    """Solver.polar(upwind=...) = set_upwind once, then the polar; the solver keeps it."""
    case, alphas, mach = fse.POLAR_CASE, fse.POLAR_ALPHAS, fse.POLAR_MACH
    mesh, s = _solver(case)
    pol = s.polar(alphas, K, mach=mach, upwind=dict(levels=1, limiter="venkatakrishnan"))
    assert s.upwind() == (1, 1, "venkatakrishnan", ue.VENKAT_K, ue.ENTROPY_FIX)
    em = ue.UpwindOracle(oracle, case)
    em.set_upwind(1, 1)
    for k, (al, p) in enumerate(zip(alphas, pol)):
        em.set_far_field(fse.free_stream_constants(mach, al), reinitialise=(k == 0))
        rc, rms = em.cycles(K)
        assert rc == 0
        _same(p["rms"], rms, f"polar, angle {al}: RMS history")
    _same(s.get(0, "variables"), em.variables(0), "the polar's last state")
    em.close()
    s.close(); mesh.close()


def _run_driver(tmp, case, extra, cycles, ok=True):
    os.makedirs(tmp / "out", exist_ok=True)
    cmd = [EXE, "-i", "input.dat", "-d", fse.case_input(case), "-o", "out/", "-g", str(cycles), "-m", str(fse.case_duplicate(case))] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tmp)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    if not ok:
        assert r.returncode == 1, r.stdout + r.stderr
    return r


def _strip(out):
    return [l for l in out.splitlines() if not l.startswith("Total runtime = ")]


def test_driver_flags(oracle, tmp_path):
    """--upwind (the Python defaults), the value flags (each implies --upwind) and the config keys: the dump is the %.17e rendering
    of the emulator's state and the RMS lines its history; --upwind-levels 0 is the plain run, stdout included; with --jst on the
    same level, with --gpus-partition, or reconstructing on a mesh without coordinates, status 1 before any dump."""
    case = "m6_2lvl"
    dup = fse.case_duplicate(case)
    name = f"variables.size={dup}x.cycles={K}.level=0"
    em = ue.UpwindOracle(oracle, case)
    em.set_upwind(1, 1)
    rc, want_rms = em.cycles(K)
    assert rc == 0
    want = fse.render_variables(em.variables(0)).encode()
    em.close()
    em = ue.UpwindOracle(oracle, case)
    em.set_upwind(2, 1, "barth-jespersen", 5.0, 0.0)
    rc, _ = em.cycles(K)
    assert rc == 0
    want_bj = fse.render_variables(em.variables(0)).encode()
    em.close()
    plain = _run_driver(tmp_path / "plain", case, ["--output-variables"], K)
    conf = tmp_path / "run.conf"
    conf.write_text("upwind = Y\n")
    conf2 = tmp_path / "run2.conf"
    conf2.write_text("upwind_levels = 2\nmuscl_levels = 1\nlimiter = barth-jespersen\nentropy_fix = 0\n")
    for tag, extra, w in (("default", ["--upwind"], want), ("said", ["--upwind-levels", "1", "--muscl-levels=1", "--limiter", "venkatakrishnan",
                                                                       "--venkat-k=5", "--entropy-fix", "0.1"], want),
                          ("one", ["--venkat-k=5"], want), ("conf", ["-c", str(conf)], want), ("conf2", ["-c", str(conf2)], want_bj),
                          ("bj", ["--upwind-levels=2", "--muscl-levels=1", "--limiter=barth-jespersen", "--entropy-fix=0"], want_bj)):
        d = tmp_path / tag
        r = _run_driver(d, case, ["--output-variables"] + extra, K)
        assert (d / "out" / name).read_bytes() == w, tag
        lines, plain_lines = _strip(r.stdout), _strip(plain.stdout)
        assert len(lines) == len(plain_lines)
        if w is want:
            assert [l for l in lines if "(RMS = " in l] == [f"MG cycle {i + 1} / {K}" + " (RMS = %.3e)" % want_rms[i] for i in range(K)]
    off = _run_driver(tmp_path / "off", case, ["--output-variables", "--upwind", "--upwind-levels", "0"], K)
    assert (tmp_path / "off" / "out" / name).read_bytes() == (tmp_path / "plain" / "out" / name).read_bytes()
    assert _strip(off.stdout) == _strip(plain.stdout)
    # a single-level input without its .coords file: first order runs, reconstruction is refused
    from mgcfd import meshgen
    bare = tmp_path / "bare"
    os.makedirs(bare / "input")
    meshgen.write_input(meshgen.make_multigrid((7,), "fvcorr", seed=5, cavity_radius=0.01, volume_noise=0.02), str(bare / "input"))
    (bare / "case.txt").write_text("duplicate = 1\n")
    for n in os.listdir(bare / "input"):
        if n.endswith(".coords"):
            os.remove(bare / "input" / n)
    _run_driver(tmp_path / "bare_first", str(bare), ["--upwind", "--muscl-levels", "0"], 1)
    for tag, c, extra, word in (("jst", case, ["--upwind", "--jst"], "jst"),
                                ("part", case, ["--upwind", "--gpus", "2", "--gpus-partition", "--gpus-share-device"], "upwind"),
                                ("nocoords", str(bare), ["--upwind"], "coords")):
        r = _run_driver(tmp_path / tag, c, ["--output-variables"] + extra, K, ok=False)
        assert word in (r.stdout + r.stderr).lower(), tag
        assert not [n for n in os.listdir(tmp_path / tag / "out") if n.startswith("variables")]
    for bad in (["--limiter", "minmod"], ["--venkat-k", "0"], ["--entropy-fix", "2"], ["--upwind-levels", "-1"], ["--upwind-levels", "1", "--muscl-levels", "2"]):
        _run_driver(tmp_path / "bad", case, bad, K, ok=False)
