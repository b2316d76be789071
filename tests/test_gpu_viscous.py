"""GPU tests of the laminar viscous terms (mgcfd_set_viscous) on one solver and in the drop-in binary: every combination of
ve.gpu_combinations() against the numpy emulator (tests/viscous_emulator.py) bit for bit — state on every level, the node stresses
S, F + V after mgcfd_compute_fluxes, the step factors after the limit and the RMS history; the same bits on every path; the kernels'
tile paths (a last partial tile, several tiles, halo nodes beyond the LDS table, long rows, nodes without internal edges);
composition with residual smoothing, JST, dual time and FAS; switching off mid-run; refusals; the fast mode; the driver's flags;
polar(viscous=...); device allocations.  tests/test_host_viscous.py asserts on the CPU that every combination stays valid."""
import os
import subprocess

import numpy as np
import pytest

import dual_time_emulator as dte
import fas_emulator as fe
import free_stream_emulator as fse
import jst_emulator as jse
import viscous_emulator as ve

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
K = ve.GPU_CYCLES
REL_RUN = 1e-10          # tests/test_gpu_jst.py::test_fast_mode: level `variables` after whole cycles, max |difference| / max |value|
RMS_FAST = 1e-9          # ... and its RMS tolerance
# (case key, mu, mode, cfl, wall, levels): three and two levels; both walls; level 0 alone and all levels; both kinds of viscosity
PATHS = [("A", ve.CELL_RE_MU, "local", 1.0, 1, "all"), ("m6_3lvl", ve.GPU_MU["m6_3lvl"], "reference", 0.5, 1, 1),
         ("tet_2lvl", ve.GPU_MU["tet_2lvl"], "local", 1.0, 0, "all"), ("B", ve.GPU_MU["B"], "reference", 0.5, 1, "all")]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(np.asarray(got) - np.asarray(want)).max():.3e}"


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("viscous_lattices")
    return {name: fe.write_lattice(name, d) for name in fe.LATTICES}


def _case(lattices, key):
    return lattices.get(key, key)


def _solver(case, graph=0, exact=1, stage_wg4=1, fuse=1):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    for name, v in (("graph", graph), ("exact", exact), ("stage_wg4", stage_wg4), ("fuse_update", fuse)):
        s.set_option(name, v)
    return mesh, s


def _levels(s, lv):
    return s.num_levels if lv == "all" else lv


def _configure(s, mu, mode, cfl, wall, lv, smoothing=(0.0, 0), jst_levels=0, fas=False):
    """The solver as ve.configured sets the emulator up: the start state, then the terms switched on."""
    s.set_time_step(mode, cfl)
    if smoothing[1]:
        s.set_residual_smoothing(*smoothing)
    if jst_levels:
        s.set_jst(levels=jst_levels)
    if fas:
        s.set_fas(True)
    s.set(0, "variables", ve.start_state(s.nel(0), s.far_field()[:5]))
    s.set_viscous(mu, ve.PRANDTL, bool(wall), ve.VISCOUS_CFL, _levels(s, lv))
    assert s.viscous() == (mu, ve.PRANDTL, bool(wall), ve.VISCOUS_CFL, _levels(s, lv))


_emulated = {}


def _emulate(oracle, case, mu, mode, cfl, wall, lv):
    """(rms, variables per level, step factors per level, (S, F + V) of the final state per level) of K cycles: computed once
    per combination, shared and left unchanged."""
    key = (case, mu, mode, cfl, wall, lv)
    if key not in _emulated:
        em = ve.configured(oracle, case, mu, mode, cfl, wall, lv)
        rc, rms = em.cycles(K)
        assert rc == 0
        v = [em.variables(l) for l in range(em.n)]
        sf = [em.step_factors(l) for l in range(em.n)]
        sfl = []
        for l in range(em.n):
            f = em.stage_fluxes(l)
            sfl.append((em.last_S[l].copy() if em.viscous_on(l) else None, f))
        _emulated[key] = (rms, v, sf, sfl)
        em.close()
    return _emulated[key]


def _check_run(s, want, what, fluxes=True):
    want_rms, want_v, want_sf, want_sfl = want
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), want_v[l], f"{what}: variables, level {l}")
        if not fluxes:
            continue
        _same(s.get(l, "step_factors"), want_sf[l], f"{what}: step factors, level {l}")
        assert not s.get(l, "fluxes").any(), f"{what}: fluxes after the run, level {l}"
        s.compute_fluxes(l)
        _same(s.get(l, "fluxes"), want_sfl[l][1], f"{what}: F + V, level {l}")
        if want_sfl[l][0] is not None:
            _same(s.get(l, "viscous_stress"), want_sfl[l][0], f"{what}: S, level {l}")
        s.zero_fluxes(l)


@pytest.mark.parametrize("key,mu,mode,cfl,wall,lv", ve.gpu_combinations())
def test_state_stresses_fluxes_step_factors_and_rms_equal_the_emulator(key, mu, mode, cfl, wall, lv, oracle, lattices):
    """After K cycles from the perturbed start state: `variables` of every level, the step factors of every level's last sweep
    (after the viscous limit), the RMS history, and S and F + V of the final state on every level (one mgcfd_compute_fluxes from
    zero fluxes, read back), bitwise the emulator's."""
    case = _case(lattices, key)
    want = _emulate(oracle, case, mu, mode, cfl, wall, lv)
    mesh, s = _solver(case)
    _configure(s, mu, mode, cfl, wall, lv)
    rms = s.run_cycles(K)
    what = f"{key} mu={mu} {mode} {cfl} wall={wall} levels={lv}"
    print(what, "rms", rms, "want", want[0])
    _same(rms, want[0], f"{what}: RMS history")
    _check_run(s, want, what)
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


@pytest.mark.parametrize("key,mu,mode,cfl,wall,lv", PATHS)
def test_same_bits_on_every_path(key, mu, mode, cfl, wall, lv, oracle, lattices):
    """graph 0 / 1, stage_wg4 0 / 1, fuse_update 0 / 1, timing modes 1 and 4 and the kernel-granular cycle: all the emulator's
    bits; the loop counts are those of the run without the terms."""
    case = _case(lattices, key)
    want = _emulate(oracle, case, mu, mode, cfl, wall, lv)
    mesh, plain = _solver(case)
    plain.set_time_step(mode, cfl)
    plain.set(0, "variables", ve.start_state(plain.nel(0), plain.far_field()[:5]))
    plain.run_cycles(K)
    want_iters = [plain.loop_iters(l) for l in range(plain.num_levels)]
    plain.close(); mesh.close()
    for graph, wg4, fuse, timing in ((1, 1, 1, 0), (0, 0, 1, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 1, 1, 1), (0, 1, 1, 4)):
        mesh, s = _solver(case, graph, stage_wg4=wg4, fuse=fuse)
        s.set_option("timing", timing)
        _configure(s, mu, mode, cfl, wall, lv)
        rms = s.run_cycles(K)
        what = f"{key} graph={graph} wg4={wg4} fuse={fuse} timing={timing}"
        _same(rms, want[0], f"{what}: RMS history")
        _check_run(s, want, what, fluxes=False)
        for l in range(s.num_levels):
            assert s.loop_iters(l) == want_iters[l], what
        if timing:
            assert s.loop_times(0)["flux"] > 0.0, what
        s.close()
        mesh.close()
    mesh, s = _solver(case)
    _configure(s, mu, mode, cfl, wall, lv)
    for _ in range(K):
        _kernel_granular_cycle(s)
    _check_run(s, want, f"{key} kernel-granular")
    s.close()
    mesh.close()


def _isolated_level():
    """Eight nodes of which 1, 4 and 6 have no internal edge (1 has nothing at all, 4 a solid-wall face, 6 a far-field face),
    beside a chain 0 - 5 - 2 - 7 - 3 with a solid-wall and a far-field face: small random weights, as a hub level has them."""
    from mgcfd import meshgen
    rng = np.random.default_rng(4)
    internal = [(0, 5), (2, 5), (2, 7), (3, 7)]
    faces = [(-1, 4), (-2, 6), (-1, 5), (-2, 0), (-1, 2)]
    nel, lists = 8, [[] for _ in range(8)]
    for a, b in internal:
        w = rng.normal(size=3) * 1e-3
        lists[a].append((b, w))
        lists[b].append((a, -w))
    for code, node in faces:
        lists[node].append((code, rng.normal(size=3) * 1e-3))
    ptr = np.zeros(nel + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=ptr[1:])
    return meshgen.LevelMesh(nel=nel, volumes=rng.uniform(1e-6, 2e-6, nel), coords=rng.random((nel, 3)), nbr_ptr=ptr,
                             nbr_idx=np.array([n for x in lists for n, _ in x], dtype=np.int64),
                             nbr_w=np.array([w for x in lists for _, w in x], dtype=np.float64).reshape(-1, 3))


def test_kernel_paths(oracle, lattices, tmp_path):
    """The shapes at which the gathers can go wrong: a last partial tile and more than one tile (lattice A: 2,178 nodes; the
    goldens run in the test above), halo nodes beyond the LDS table and long rows (the generated tetrahedral level of 30,000 nodes
    that tests/test_gpu_jst.py::test_kernel_paths uses), a hub whose row is longer than a tile is wide, and nodes without an
    internal edge.  On each, from a perturbed state and with no-slip walls: S, F + V after mgcfd_compute_fluxes and F(internal)
    + V after mgcfd_compute_flux_edge, with F(internal) from the same call with the terms off, so that V itself is compared in
    one addition — all bitwise the emulator's; then two sweeps.  (The generated levels have no part in tests/test_host_viscous.py:
    the emulator's return code is asserted here; the generated levels run at local CFL 0.02 as in the JST test: undamped, they go invalid within two sweeps at 0.5.)"""
    import mgcfd
    from mgcfd import meshgen
    from conftest import perturbed_state
    cases = [(lattices["A"], 0.01, 1.0, ve.CELL_RE_MU)]
    for name, level, amplitude, cfl, mu in (("tet", meshgen.make_tet_level(30000, seed=0, wall_below=2.0), 0.002, 0.02, 1e-3),
                                            ("hub", meshgen.make_hub_level(600, scale=1e-4, seed=5), 0.002, 0.02, 1e-9),
                                            ("isolated", _isolated_level(), 0.002, 0.02, 1e-9)):
        mg = meshgen.MultigridMesh(mesh_name="fvcorr")
        mg.levels.append(level)
        d = tmp_path / name
        os.makedirs(d / "input")
        meshgen.write_input(mg, str(d / "input"))
        (d / "case.txt").write_text("duplicate = 1\n")
        cases.append((str(d), amplitude, cfl, mu))
    for case, amplitude, cfl, mu in cases:
        mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
        s = mgcfd.Solver.from_mesh(mesh)
        t = s.tiling(0)
        name = os.path.basename(case)
        print(name, t)
        if name == "tet":
            assert t["tiles"] > 1 and t["overflow_refs"] > 0 and t["list_entries"] > 0
        elif name == "hub":
            assert t["list_entries"] > 0
        elif name == "lattice_A":
            assert t["tiles"] > 1 and s.nel(0) % 256 != 0
        start = perturbed_state(s.nel(0), s.far_field()[:5], seed=7, amplitude=amplitude)
        em = ve.ViscousOracle(oracle, case, "local", cfl)
        em._var(0)[:] = start
        em.set_viscous(mu, ve.PRANDTL, 1, ve.VISCOUS_CFL, 1)
        s.set_time_step("local", cfl)
        s.set(0, "variables", start)
        s.set_viscous(mu, wall=True)
        _same(s.get(0, "variables"), em.variables(0), f"{name}: the start state with the wall rule applied")
        S, V = em.viscous_terms(0)
        want_f = em.stage_fluxes(0)
        s.compute_fluxes(0)
        _same(s.get(0, "viscous_stress"), S, f"{name}: S")
        _same(s.get(0, "fluxes"), want_f, f"{name}: F + V")
        assert np.isfinite(S).all() and np.isfinite(V).all() and V[:, 1:].any() and not V[:, 0].any()
        if name == "isolated":
            assert not S[[1, 4, 6], 3:].any() and not V[[1, 4, 6]].any() and S[[1, 6], 0].all()
        # V alone: the internal fluxes with the terms off, then the same call with them on
        s.zero_fluxes(0)
        s.set_viscous(0.0, levels=0)
        s.compute_flux_edge(0)
        f_int = s.get(0, "fluxes")
        s.zero_fluxes(0)
        s.set_viscous(mu, wall=True)
        s.compute_flux_edge(0)
        _same(s.get(0, "fluxes"), f_int + V, f"{name}: F(internal) + V")
        s.zero_fluxes(0)
        assert em.sweeps(0, 2) == 0
        s.smooth(0, 2)
        _same(s.get(0, "variables"), em.variables(0), f"{name}: two sweeps")
        _same(s.get(0, "residuals"), em.oc.array(0, "residuals").reshape(-1, 5), f"{name}: residuals")
        _same(s.get(0, "step_factors"), em.step_factors(0), f"{name}: step factors")
        assert s.pending_invalid_state()[0] == 0
        em.close()
        s.close(); mesh.close()


@pytest.mark.parametrize("name,mode,cfl,smoothing,jst_levels,order,fas", ve.COMPOSED, ids=[c[0] for c in ve.COMPOSED])
def test_composition(name, mode, cfl, smoothing, jst_levels, order, fas, oracle, lattices):
    """Lattice A at cell Reynolds number 2, no-slip walls, all levels, with residual smoothing (0.5, 2), JST (defaults, level 0),
    dual time (2 steps x 3 cycles, BDF2), FAS, and all of them: the composed emulator's state and RMS history (FAS: P and W0 too)."""
    case = lattices["A"]
    em = ve.configured(oracle, case, ve.CELL_RE_MU, mode, cfl, 1, "all", smoothing, jst_levels, fas)
    mesh, s = _solver(case)
    _configure(s, ve.CELL_RE_MU, mode, cfl, 1, "all", smoothing, jst_levels, fas)
    if order is None:
        rc, want_rms = em.cycles(K)
        rms = s.run_cycles(K)
    else:
        dt = dte.pick_dt(oracle, case, mode, cfl)
        em.set_dual_time(dt)
        em.set_order(order)
        rc, want_rms = em.advance(ve.DUAL_STEPS, ve.DUAL_CYCLES)
        s.set_dual_time(dt)
        s.dual_time_order(order)
        rms = s.advance(ve.DUAL_STEPS, ve.DUAL_CYCLES).ravel()
    assert rc == 0
    _same(rms, want_rms, f"{name}: RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), em.variables(l), f"{name}: level {l}")
        if fas and l >= 1:
            _same(s.get(l, "fas_forcing"), em.P[l], f"{name}: P, level {l}")
            _same(s.get(l, "fas_start"), em.W0[l], f"{name}: W0, level {l}")
        if order is not None:
            _same(s.get(l, "time_n"), em.Wn[l], f"{name}: Wn, level {l}")
    em.close()
    s.close(); mesh.close()


@pytest.mark.parametrize("key", ["A", "m6_3lvl"])
def test_switching_off_mid_run(key, oracle, lattices):
    """On for K cycles, off for K, on again (graphs off and on): the emulator driven the same way; after switching off the rest
    of the run equals a solver that never had the terms on, started from that state."""
    case = _case(lattices, key)
    mu = ve.CELL_RE_MU if key == "A" else ve.GPU_MU[key]
    em = ve.configured(oracle, case, mu, "local", 1.0, 1, "all")
    want = []
    for on in (True, False, True):
        if not on:
            em.set_viscous(0.0, levels=0)
        elif want:
            em.set_viscous(mu, ve.PRANDTL, 1, ve.VISCOUS_CFL, "all")
        rc, rms = em.cycles(K)
        assert rc == 0
        want.append((rms, [em.variables(l) for l in range(em.n)]))
    em.close()
    for graph in (0, 1):
        mesh, s = _solver(case, graph)
        _configure(s, mu, "local", 1.0, 1, "all")
        for k in range(3):
            if k == 1:
                before = s.get(0, "variables")
                s.set_viscous(0.0, levels=0)
                assert s.viscous() == (0.0, 0.0, False, 0.0, 0)
                _same(s.get(0, "variables"), before, "switching off keeps the state")
                ref_mesh, ref = _solver(case, graph)
                ref.set_time_step("local", 1.0)
                for l in range(s.num_levels):
                    ref.set(l, "variables", s.get(l, "variables"))
                ref.run_cycles(K)
            if k == 2:
                s.set_viscous(mu, ve.PRANDTL, True, ve.VISCOUS_CFL, s.num_levels)
            rms = s.run_cycles(K)
            for l in range(s.num_levels):
                _same(s.get(l, "variables"), want[k][1][l], f"{key} graph={graph} leg {k}: level {l}")
            if k != 1:
                _same(rms, want[k][0], f"{key} graph={graph} leg {k}: RMS history")
            else:
                assert np.allclose(rms, want[k][0], rtol=1e-12, atol=0)    # (off: the library's own order of the sum, as ever)
                for l in range(s.num_levels):
                    _same(s.get(l, "variables"), ref.get(l, "variables"), f"{key} graph={graph}: against a solver that never had them, level {l}")
                ref.close(); ref_mesh.close()
        s.close()
        mesh.close()


def test_refusals():
    """Bad numbers, mid-sweep, a partitioned solver, a group member, the sweep_* calls, group creation and rank attachment while
    on: error code 1, "viscous" in the message, nothing changed."""
    import mgcfd
    mesh, s = _solver("m6_2lvl")
    ref_mesh, ref = _solver("m6_2lvl")
    for t in (s, ref):
        t.set_viscous(1e-3, levels=1)
    good = (1e-3, ve.PRANDTL, False, ve.VISCOUS_CFL, 1)
    for mu, pr, wall, cv, lv in ((0.0, 0.72, 0, 0.25, 1), (-1.0, 0.72, 0, 0.25, 1), (float("nan"), 0.72, 0, 0.25, 1), (1e-3, 0.0, 0, 0.25, 1),
                                 (1e-3, float("inf"), 0, 0.25, 1), (1e-3, 0.72, 0, 0.0, 1), (1e-3, 0.72, 0, float("nan"), 1),
                                 (1e-3, 0.72, 2, 0.25, 1), (1e-3, 0.72, -1, 0.25, 1), (1e-3, 0.72, 0, 0.25, -1)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            s._c(s.lib.mgcfd_set_viscous(s.handle, mu, pr, wall, cv, lv))
        assert e.value.code == 1 and "viscous" in str(e.value), (mu, pr, wall, cv, lv)
    assert s.viscous() == good
    for call in (lambda: s.sweep_begin(0), lambda: s.sweep_begin_partials(0), lambda: s.sweep_flux0(0), lambda: s.sweep_stage(0, 0),
                 lambda: s.sweep_end(0), lambda: s.sweep_end_partials(0), lambda: s.sweep_begin(1)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1 and "viscous" in str(e.value)
    with pytest.raises(mgcfd.MgcfdError) as e:
        mgcfd.Group([s])
    assert e.value.code == 1 and "viscous" in str(e.value)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.rank_attach_plain(0, 1)
    assert e.value.code == 1 and "viscous" in str(e.value)
    with pytest.raises(mgcfd.MgcfdError):
        s.set(0, "viscous_stress", np.zeros((s.nel(0), 12)))
    with pytest.raises(mgcfd.MgcfdError):
        s.get(1, "viscous_stress")                            # (not on for level 1)
    with pytest.raises(mgcfd.MgcfdError):
        s.bench_viscous(1, 0, 1)
    for t in (s, ref):
        t.run_cycles(1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "a cycle after the refused calls")
    # mid-sweep: the split sweep runs with the terms off; the setter is refused until its last stage has run
    for t in (s, ref):
        t.set_viscous(0.0, levels=0)
    s.sweep_begin(0)
    s.sweep_stage(0, 0, partials=False)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_viscous(1e-3, levels=1)
    assert e.value.code == 1 and "viscous" in str(e.value) and "sweep is under way" in str(e.value)
    assert s.viscous() == (0.0, 0.0, False, 0.0, 0)
    s.sweep_stage(0, 1, partials=False)
    s.sweep_stage(0, 2, partials=False)
    ref.smooth(0, 1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "the sweep the refused call interrupted")
    # a group member, and a partitioned solver
    g = mgcfd.Group([s])
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_viscous(1e-3, levels=1)
    assert e.value.code == 1 and "viscous" in str(e.value)
    s.set_viscous(0.0, levels=0)                              # switching off is always allowed
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
        t.set_viscous(1e-3, levels=1)
    assert e.value.code == 1 and "viscous" in str(e.value)
    assert t.viscous() == (0.0, 0.0, False, 0.0, 0)
    t.set_viscous(1e-3, levels=0)
    t.close()
    mesh.close()


@pytest.mark.parametrize("key,mu,mode,cfl,wall,lv", PATHS)
def test_fast_mode(key, mu, mode, cfl, wall, lv, oracle, lattices):
    """exact = 0 (FMA contraction, the order-free flux kernel for F) within the bound tests/test_gpu_jst.py::test_fast_mode uses:
    1e-10 of the largest value per level, RMS rtol 1e-9."""
    case = _case(lattices, key)
    want_rms, want_v, _, _ = _emulate(oracle, case, mu, mode, cfl, wall, lv)
    mesh, s = _solver(case, exact=0)
    _configure(s, mu, mode, cfl, wall, lv)
    rms = s.run_cycles(K)
    assert np.allclose(rms, want_rms, rtol=RMS_FAST, atol=0)
    for l in range(s.num_levels):
        rel = np.abs(s.get(l, "variables") - want_v[l]).max() / max(np.abs(want_v[l]).max(), 1e-300)
        print(key, mode, cfl, wall, lv, "level", l, "rel", rel)
        assert rel <= REL_RUN, f"{key} level {l}: {rel:.3e}"
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


def _strip(out):
    return [l for l in out.splitlines() if not l.startswith("Total runtime = ")]


@pytest.mark.parametrize("case", ve.DRIVER_CASES)
def test_driver_flags(case, oracle, tmp_path):
    """--viscosity with its companions, --reynolds (resolved against the free stream in use), the config keys: the dump is the
    %.17e rendering of the emulator's state, the RMS lines its history, LoopNumIters.csv the plain run's counts; --gpus 2
    with a level per GPU gives the same dump; with --gpus-partition an error before any GPU work; bad values and companions without a viscosity are refused."""
    dup = fse.case_duplicate(case)
    name = f"variables.size={dup}x.cycles={K}.level=0"
    em = ve.ViscousOracle(oracle, case, mu=ve.DRIVER_MU, wall=1, viscous_levels="all")
    rc, want_rms = em.cycles(K)
    assert rc == 0
    want, n_levels = fse.render_variables(em.variables(0)).encode(), em.n
    em.close()
    plain = _run_driver(tmp_path / "plain", case, ["--output-variables"], K)
    assert (tmp_path / "plain" / "out" / name).read_bytes() != want
    conf = tmp_path / "run.conf"
    conf.write_text(f"viscosity = {ve.DRIVER_MU!r}\nno_slip = Y\nviscous_levels = 8\nprandtl = {ve.PRANDTL!r}\nviscous_cfl = {ve.VISCOUS_CFL!r}\n")
    for tag, extra in (("said", ["--viscosity", repr(ve.DRIVER_MU), "--no-slip", "--viscous-levels=8", "--prandtl", repr(ve.PRANDTL),
                                 f"--viscous-cfl={ve.VISCOUS_CFL!r}"]),
                       ("short", [f"--viscosity={ve.DRIVER_MU!r}", "--no-slip", "--viscous-levels", "8"]),
                       ("conf", ["-c", str(conf)])):
        d = tmp_path / tag
        r = _run_driver(d, case, ["--output-variables"] + extra, K)
        assert (d / "out" / name).read_bytes() == want, f"{case} {tag}"
        lines, plain_lines = _strip(r.stdout), _strip(plain.stdout)
        assert len(lines) == len(plain_lines)
        rms_lines = [l for l in lines if "(RMS = " in l]
        assert rms_lines == [(f"Cycle {i + 1} / {K}" if n_levels <= 1 else f"MG cycle {i + 1} / {K}") + " (RMS = %.3e)" % want_rms[i] for i in range(K)]
        assert _loop_iters(d) == _loop_iters(tmp_path / "plain")
    # --gpus 2 with one multigrid level per GPU: the same bits; a single level would be split over the two: refused by the library
    two = ["--output-variables", f"--viscosity={ve.DRIVER_MU!r}", "--no-slip", "--viscous-levels", "8", "--gpus", "2", "--gpus-share-device"]
    if n_levels == 1:
        r = _run_driver(tmp_path / "two", case, two, K, ok=False)
        assert "viscous" in (r.stdout + r.stderr).lower()
    else:
        _run_driver(tmp_path / "two", case, two, K)
        assert (tmp_path / "two" / "out" / name).read_bytes() == want, f"{case} --gpus 2"
    # --reynolds against the free stream of --mach / --alpha: mu = rho_inf |V_inf| L / Re
    import mgcfd
    mach, alpha, reynolds, length = 0.8, 2.0, 500.0, 0.5
    ff = mgcfd.free_stream_constants(mach, alpha)
    mu = mgcfd.viscosity_from_reynolds(ff, reynolds, length)
    em = ve.ViscousOracle(oracle, case, mu=mu, wall=0, viscous_levels=1)
    em.set_far_field(ff, reinitialise=True)
    rc, _ = em.cycles(K)
    assert rc == 0
    d = tmp_path / "reynolds"
    _run_driver(d, case, ["--output-variables", "--mach", str(mach), "--alpha", str(alpha), "--reynolds", str(reynolds), "--ref-length", str(length)], K)
    assert (d / "out" / name).read_bytes() == fse.render_variables(em.variables(0)).encode()
    em.close()
    r = _run_driver(tmp_path / "part", case, ["--viscosity", "0.01", "--gpus", "2", "--gpus-partition", "--gpus-share-device"], K, ok=False)
    assert "viscous" in (r.stdout + r.stderr).lower()
    assert not [n for n in os.listdir(tmp_path / "part" / "out") if n.startswith("variables")]
    for bad in (["--viscosity", "0"], ["--viscosity", "-1"], ["--reynolds", "nan"], ["--viscosity", "0.01", "--reynolds", "100"],
                ["--prandtl", "0.72"], ["--no-slip"], ["--viscous-levels", "1"], ["--viscosity", "0.01", "--viscous-levels", "-1"],
                ["--viscosity", "0.01", "--viscous-cfl", "0"], ["--reynolds", "100", "--ref-length", "0"]):
        _run_driver(tmp_path / "bad", case, bad, K, ok=False)


def _golden_cycles(case):
    meta = dict(l.strip().split(" = ") for l in open(os.path.join(fse.GOLDEN, case, "case.txt")))
    return int(meta["cycles"])


@pytest.mark.parametrize("case", fse.GPU_CASES)
def test_defaults_reproduce_the_golden_output(case, tmp_path):
    """With the flags absent: variables.level0.txt of the golden case byte for byte; --viscous-levels 0 spelled out is that run too,
    stdout included, and so is the Python API after on and off again."""
    cycles, dup = _golden_cycles(case), fse.case_duplicate(case)
    golden = open(os.path.join(fse.GOLDEN, case, "variables.level0.txt"), "rb").read()
    name = f"variables.size={dup}x.cycles={cycles}.level=0"
    plain = _run_driver(tmp_path / "plain", case, ["--output-variables"], cycles)
    assert (tmp_path / "plain" / "out" / name).read_bytes() == golden
    off = _run_driver(tmp_path / "off", case, ["--output-variables", "--viscosity", "0.01", "--viscous-levels", "0"], cycles)
    assert (tmp_path / "off" / "out" / name).read_bytes() == golden
    assert _strip(off.stdout) == _strip(plain.stdout)
    assert _loop_iters(tmp_path / "off") == _loop_iters(tmp_path / "plain")
    mesh, s = _solver(case)
    assert s.viscous() == (0.0, 0.0, False, 0.0, 0)
    s.set_viscous(0.01, wall=False)
    s.set_viscous(0.0, levels=0)                              # on and off again before the run: the default run
    s.run_cycles(cycles)
    assert fse.render_variables(s.get(0, "variables")).encode() == golden
    s.close()
    mesh.close()


def test_polar_with_viscous(oracle):
    """Solver.polar(viscous=...) = set_viscous once, then the polar; the solver keeps it; every angle that starts from its far
    field starts with the wall rule applied."""
    case, alphas, mach = fse.POLAR_CASE, fse.POLAR_ALPHAS, fse.POLAR_MACH
    mesh, s = _solver(case)
    pol = s.polar(alphas, K, mach=mach, viscous={"mu": ve.DRIVER_MU, "wall": True, "levels": 2})
    assert s.viscous() == (ve.DRIVER_MU, ve.PRANDTL, True, ve.VISCOUS_CFL, 2)
    em = ve.ViscousOracle(oracle, case, mu=ve.DRIVER_MU, wall=1, viscous_levels=2)
    for k, (al, p) in enumerate(zip(alphas, pol)):
        em.set_far_field(fse.free_stream_constants(mach, al), reinitialise=(k == 0))
        rc, rms = em.cycles(K)
        assert rc == 0
        _same(p["rms"], rms, f"polar, angle {al}: RMS history")
    _same(s.get(0, "variables"), em.variables(0), "the polar's last state")
    em.close()
    s.close(); mesh.close()
    mesh, s = _solver(case)
    s.polar(alphas[:1], 1, mach=mach, viscous=(ve.DRIVER_MU, ve.PRANDTL, False, 0.1, 1))
    assert s.viscous() == (ve.DRIVER_MU, ve.PRANDTL, False, 0.1, 1)
    s.close(); mesh.close()


def test_device_resources():
    """A solver that never enables them holds what it holds today; enabling adds S, g and the wall-node list per viscous level
    and level 0's numbering for the RMS, once; switching off releases them; destroy returns to the baseline."""
    import mgcfd
    base = mgcfd.live_device_resources()
    mesh, a = _solver("m6_3lvl")
    a.run_cycles(1)
    a.set_viscous(0.0, levels=0)
    after_run = mgcfd.live_device_resources()
    mesh_b, b = _solver("m6_3lvl")
    b.run_cycles(1)
    both = mgcfd.live_device_resources()
    assert both["allocations"] - after_run["allocations"] == after_run["allocations"] - base["allocations"], "a never-enabled solver: today's count"
    b.set_viscous(1e-3, levels=2)
    on = mgcfd.live_device_resources()
    assert on["allocations"] - both["allocations"] == 2 * 3 + 1
    assert on["bytes"] - both["bytes"] >= sum(13 * 8 * b.nel(l) for l in range(2))
    b.set_viscous(2e-3, wall=True, levels=2)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"], "allocated once"
    b.set_viscous(1e-3, levels=3)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"] + 3, "a further level: its three arrays"
    b.run_cycles(1)
    assert b.bench_viscous(0, 0, 3) > 0.0 and b.bench_viscous(0, 1, 3) > 0.0
    b.set_viscous(0.0, levels=0)
    off = mgcfd.live_device_resources()
    assert off["allocations"] == both["allocations"] and off["bytes"] == both["bytes"], "switching off releases"
    b.close(); mesh_b.close()
    assert mgcfd.live_device_resources()["allocations"] == after_run["allocations"]
    a.close(); mesh.close()
    end = mgcfd.live_device_resources()
    assert end["allocations"] == base["allocations"] and end["bytes"] == base["bytes"]
