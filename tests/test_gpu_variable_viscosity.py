"""GPU tests of the viscosity model (mgcfd_set_viscosity_model: Sutherland's law, a caller's eddy-viscosity field, Smagorinsky)
on one solver and in the drop-in binary, against the numpy emulator (tests/variable_viscosity_emulator.py) bit for bit: the state
on every level, the step factors after the variable limit, the RMS history, and S, eddy_viscosity and F + V after
mgcfd_compute_fluxes; the stress kernel's tile paths; the same bits on every path; composition with residual smoothing, JST, dual
time and FAS; the friction loads under every model; the behaviour of the setting and its refusals; the fast mode; the driver's
flags; polar(viscosity_model=...); device allocations.  tests/test_host_variable_viscosity.py asserts on the CPU that every
combination stays valid."""
import os
import subprocess

import numpy as np
import pytest

import dual_time_emulator as dte
import fas_emulator as fe
import free_stream_emulator as fse
import friction_loads_emulator as fle
import variable_viscosity_emulator as vve
import viscous_emulator as ve

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
K = ve.GPU_CYCLES
REL_RUN = 1e-10          # tests/test_gpu_viscous.py::test_fast_mode's tolerances
RMS_FAST = 1e-9
REF = (0.25, -0.125, 0.375)
FIELD = ("constant", "field")
BITWISE_CASES = ("A", "B", "tet_2lvl")
# test_gpu_viscous.py's PATHS: three and two levels; both walls; level 0 alone and all levels; both kinds of viscosity
PATHS = [("A", ve.CELL_RE_MU, "local", 1.0, 1, "all"), ("m6_3lvl", ve.GPU_MU["m6_3lvl"], "reference", 0.5, 1, 1),
         ("tet_2lvl", ve.GPU_MU["tet_2lvl"], "local", 1.0, 0, "all"), ("B", ve.GPU_MU["B"], "reference", 0.5, 1, "all")]
LATTICE_A = ("A", ve.CELL_RE_MU, "local", 1.0, 1, "all")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(got - want).max():.3e}"


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("variable_viscosity_lattices")
    return {name: fe.write_lattice(name, d) for name in fe.LATTICES}


def _case(lattices, key):
    return lattices.get(key, key)


def _solver(case, graph=0, exact=1, fuse=1):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    for name, v in (("graph", graph), ("exact", exact), ("fuse_update", fuse)):
        s.set_option(name, v)
    return mesh, s


def _levels(s, lv):
    return s.num_levels if lv == "all" else lv


def _set_model(s, model):
    s.set_viscosity_model(law=model[0], eddy=model[1])
    got = s.viscosity_model()
    assert (got["law"], got["eddy"]) == tuple(model)
    assert (got["s"], got["cs"], got["prandtl_t"]) == (vve.SUTHERLAND_S, vve.SMAGORINSKY_CS, vve.PRANDTL_TURBULENT)
    _same([got["t_ref"]], [vve.far_field_t_ref(s.far_field())], "t_ref taken from the far field")


def _write_field(s, mu, lv):
    for l in range(_levels(s, lv)):
        assert not s.get(l, "eddy_viscosity").any(), "the array holds +0.0 at allocation"
        s.set(l, "eddy_viscosity", vve.eddy_field(mu, s.nel(l), l))


def _configure(s, mu, mode, cfl, wall, lv, model, smoothing=(0.0, 0), jst_levels=0, fas=False):
    """The solver as vve.configured sets the emulator up: the start state, the terms switched on, then the model."""
    s.set_time_step(mode, cfl)
    if smoothing[1]:
        s.set_residual_smoothing(*smoothing)
    if jst_levels:
        s.set_jst(levels=jst_levels)
    if fas:
        s.set_fas(True)
    s.set(0, "variables", ve.start_state(s.nel(0), s.far_field()[:5]))
    s.set_viscous(mu, ve.PRANDTL, bool(wall), ve.VISCOUS_CFL, _levels(s, lv))
    _set_model(s, model)
    if tuple(model) == FIELD:
        _write_field(s, mu, lv)


_emulated = {}


def _emulate(oracle, case, mu, mode, cfl, wall, lv, model):
    """(rms, variables, step factors, eddy viscosity after the run, (S, mut, F + V) of the final state) per level of K cycles:
    computed once per combination, shared and left unchanged."""
    key = (case, mu, mode, cfl, wall, lv, tuple(model))
    if key not in _emulated:
        em = vve.configured(oracle, case, mu, mode, cfl, wall, lv, model, field=tuple(model) == FIELD)
        rc, rms = em.cycles(K)
        assert rc == 0
        v = [em.variables(l) for l in range(em.n)]
        sf = [em.step_factors(l) for l in range(em.n)]
        held = [em.viscous_on(l) and em.model.eddy != 0 for l in range(em.n)]
        mut_run = [em.eddy_viscosity(l) if held[l] else None for l in range(em.n)]
        sfl = []
        for l in range(em.n):
            f = em.stage_fluxes(l)
            sfl.append((em.last_S[l].copy() if em.viscous_on(l) else None, em.eddy_viscosity(l) if held[l] else None, f))
        _emulated[key] = (rms, v, sf, mut_run, sfl)
        em.close()
    return _emulated[key]


def _check_run(s, want, what, fluxes=True):
    want_rms, want_v, want_sf, want_mut, want_sfl = want
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), want_v[l], f"{what}: variables, level {l}")
        if not fluxes:
            continue
        _same(s.get(l, "step_factors"), want_sf[l], f"{what}: step factors, level {l}")
        if want_mut[l] is not None:
            _same(s.get(l, "eddy_viscosity"), want_mut[l], f"{what}: eddy viscosity after the run, level {l}")
        assert not s.get(l, "fluxes").any(), f"{what}: fluxes after the run, level {l}"
        s.compute_fluxes(l)
        S, mut, f = want_sfl[l]
        _same(s.get(l, "fluxes"), f, f"{what}: F + V, level {l}")
        if S is not None:
            _same(s.get(l, "viscous_stress"), S, f"{what}: S, level {l}")
        if mut is not None:
            _same(s.get(l, "eddy_viscosity"), mut, f"{what}: eddy viscosity, level {l}")
        s.zero_fluxes(l)


def _bitwise_runs():
    out = [c + (m,) for m in vve.MODELS for c in ve.gpu_combinations() if c[0] in BITWISE_CASES]
    out.append(LATTICE_A + (FIELD,))
    out += [(key, ve.GPU_MU[key], "local", 1.0, 1, "all", vve.COMBINED) for key in ("m6_3lvl", "mixed_2lvl")]
    return out


@pytest.mark.parametrize("key,mu,mode,cfl,wall,lv,model", _bitwise_runs())
def test_state_stresses_eddy_viscosity_fluxes_step_factors_and_rms_equal_the_emulator(key, mu, mode, cfl, wall, lv, model, oracle, lattices):
    """After K cycles from the perturbed start state: `variables` of every level, the step factors of every level's last sweep
    (after k_viscous_clamp_variable), the RMS history, the eddy viscosity the last stage left, and S, eddy_viscosity and F + V
    of the final state (one mgcfd_compute_fluxes from zero fluxes), bitwise the emulator's."""
    case = _case(lattices, key)
    want = _emulate(oracle, case, mu, mode, cfl, wall, lv, model)
    mesh, s = _solver(case)
    _configure(s, mu, mode, cfl, wall, lv, model)
    rms = s.run_cycles(K)
    what = f"{key} mu={mu} {mode} {cfl} wall={wall} levels={lv} {model}"
    print(what, "rms", rms, "want", want[0])
    _same(rms, want[0], f"{what}: RMS history")
    _check_run(s, want, what)
    s.close()
    mesh.close()


def _isolated_level():
    """tests/test_gpu_viscous.py's level, rebuilt: eight nodes of which 1, 4 and 6 have no internal edge (1 has nothing at all, 4
    a solid-wall face, 6 a far-field face), beside a chain 0 - 5 - 2 - 7 - 3 with a solid-wall and a far-field face."""
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
    """The shapes at which the stress kernel's gathers can go wrong, as tests/test_gpu_viscous.py::test_kernel_paths has them: a
    last partial tile and more than one tile (lattice A), halo nodes beyond the LDS table and long rows (the generated tetrahedral
    level of 30,000 nodes), a hub whose row is longer than a tile, and nodes without an internal edge.  From a perturbed state,
    no-slip walls, the combined model: S, eddy_viscosity and F + V bitwise the emulator's, eddy_viscosity +0.0 at the isolated
    nodes; then two sweeps (CFL 0.02 on the generated levels, as there), compared sweep by sweep.  On the tetrahedral level the
    emulator itself finds a negative energy in the second sweep (undamped Smagorinsky at its no-slip wall grows to 27 mu within
    a sweep while the limit still holds the 1.7 mu of the sweep before; without an eddy viscosity the level stays valid, and the
    perturbation's amplitude does not matter): there the library must report the same finding."""
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
        em = vve.VariableViscosityOracle(oracle, case, "local", cfl)
        em._var(0)[:] = start
        em.set_viscous(mu, ve.PRANDTL, 1, ve.VISCOUS_CFL, 1)
        em.set_viscosity_model(law=vve.COMBINED[0], eddy=vve.COMBINED[1])
        s.set_time_step("local", cfl)
        s.set(0, "variables", start)
        s.set_viscous(mu, wall=True)
        _set_model(s, vve.COMBINED)
        assert not s.get(0, "eddy_viscosity").any(), f"{name}: +0.0 from the enabling call"
        want_f = em.stage_fluxes(0)
        S, mut = em.last_S[0], em.eddy_viscosity(0)
        s.compute_fluxes(0)
        _same(s.get(0, "viscous_stress"), S, f"{name}: S")
        _same(s.get(0, "eddy_viscosity"), mut, f"{name}: eddy viscosity")
        _same(s.get(0, "fluxes"), want_f, f"{name}: F + V")
        assert np.isfinite(S).all() and np.isfinite(mut).all() and (mut >= 0.0).all() and mut.any()
        if name == "isolated":
            assert not _bits(s.get(0, "eddy_viscosity")[[1, 4, 6]]).any() and not S[[1, 4, 6], 3:].any()
        s.zero_fluxes(0)
        for sweep in (1, 2):
            rc = em.sweeps(0, 1)
            s.smooth(0, 1)
            if rc != 0:
                # the reference itself leaves the valid states here (it stops at that stage, the library finishes the sweep):
                # the library has to report the same finding; there is no state left to compare
                assert name == "tet" and sweep == 2, f"{name}: the emulator's sweep {sweep} returned {rc}"
                assert s.pending_invalid_state()[0] == rc + 3, f"{name}: sweep {sweep}"
                break
            _same(s.get(0, "variables"), em.variables(0), f"{name}: sweep {sweep}")
            _same(s.get(0, "step_factors"), em.step_factors(0), f"{name}: step factors, sweep {sweep}")
            _same(s.get(0, "eddy_viscosity"), em.eddy_viscosity(0), f"{name}: eddy viscosity after sweep {sweep}")
            assert s.pending_invalid_state()[0] == 0
        em.close()
        s.close(); mesh.close()


def _kernel_granular_cycle(s):
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


def test_same_bits_on_every_path(oracle, lattices):
    """run_cycles with MGCFD_OPT_GRAPH set (accepted, runs directly) and fuse_update 0 / 1, and the kernel-granular cycle: the
    emulator's bits."""
    key, mu, mode, cfl, wall, lv = LATTICE_A
    case = lattices[key]
    want = _emulate(oracle, case, mu, mode, cfl, wall, lv, vve.COMBINED)
    for graph, fuse in ((1, 1), (0, 0), (1, 0)):
        mesh, s = _solver(case, graph, fuse=fuse)
        _configure(s, mu, mode, cfl, wall, lv, vve.COMBINED)
        rms = s.run_cycles(K)
        what = f"graph={graph} fuse={fuse}"
        _same(rms, want[0], f"{what}: RMS history")
        _check_run(s, want, what, fluxes=False)
        s.close()
        mesh.close()
    mesh, s = _solver(case)
    _configure(s, mu, mode, cfl, wall, lv, vve.COMBINED)
    for _ in range(K):
        _kernel_granular_cycle(s)
    _check_run(s, want, "kernel-granular")
    s.close()
    mesh.close()


@pytest.mark.parametrize("name,mode,cfl,smoothing,jst_levels,order,fas", ve.COMPOSED, ids=[c[0] for c in ve.COMPOSED])
def test_composition(name, mode, cfl, smoothing, jst_levels, order, fas, oracle, lattices):
    """Lattice A at cell Reynolds number 2, no-slip walls, all levels, the combined model, with residual smoothing, JST, dual time
    (BDF2), FAS, and all of them: the composed emulator's state, eddy viscosity and RMS history."""
    case = lattices["A"]
    em = vve.configured(oracle, case, ve.CELL_RE_MU, mode, cfl, 1, "all", vve.COMBINED, smoothing, jst_levels, fas)
    mesh, s = _solver(case)
    _configure(s, ve.CELL_RE_MU, mode, cfl, 1, "all", vve.COMBINED, smoothing, jst_levels, fas)
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
        _same(s.get(l, "eddy_viscosity"), em.eddy_viscosity(l), f"{name}: eddy viscosity, level {l}")
        if fas and l >= 1:
            _same(s.get(l, "fas_forcing"), em.P[l], f"{name}: P, level {l}")
    em.close()
    s.close(); mesh.close()


@pytest.mark.parametrize("model", vve.MODELS + (FIELD,), ids=lambda m: "-".join(m))
def test_friction_loads(model):
    """With each model on lattice A (all levels, no-slip walls, after K cycles), on every level: surface_loads(friction=True),
    wall_stress and wall_distribution are bitwise the emulator's on the state read back; the wall_stress rows equal the wall rows
    of S after compute_fluxes; eddy_viscosity is unchanged by the loads calls."""
    import mgcfd
    mg = fle.generated("A")
    levels = mgcfd.generated_to_levels(mg)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    mu = ve.CELL_RE_MU
    s.set(0, "variables", ve.start_state(s.nel(0), s.far_field()[:5]))
    s.set_viscous(mu, ve.PRANDTL, True, ve.VISCOUS_CFL, s.num_levels)
    _set_model(s, model)
    if model == FIELD:
        _write_field(s, mu, "all")
    s.run_cycles(K)
    m = vve.Model(model[0], vve.far_field_t_ref(s.far_field()), eddy=model[1])
    for l in range(s.num_levels):
        what = f"{model} level {l}"
        v, e = s.get(l, "variables"), s.get_edges(l, len(levels[l]["edges"]))
        mut_before = s.get(l, "eddy_viscosity") if m.eddy else None
        S = vve.node_stresses(v, e, levels[l], mu, ve.PRANDTL, m, mut_before)
        want12 = vve.surface_loads12(v, e, levels[l], s.far_field(), REF, S)
        want_ids, want_table = vve.distribution(v, e, levels[l], s.far_field(), S)
        assert want12[6:9].all(), f"{what}: the friction force should not vanish"
        _same(s.surface_loads(l, REF, friction=True), want12, f"{what}: loads")
        ids, table = s.wall_distribution(l)
        assert np.array_equal(ids, want_ids)
        _same(table, want_table, f"{what}: distribution")
        ids, sw = s.wall_stress(l)
        assert np.array_equal(ids, want_ids)
        _same(sw, S[want_ids], f"{what}: Sw")
        if m.eddy:
            _same(s.get(l, "eddy_viscosity"), mut_before, f"{what}: eddy viscosity after the loads calls")
        s.compute_fluxes(l)
        _same(sw, s.get(l, "viscous_stress")[ids], f"{what}: Sw against the wall rows of S")
        s.zero_fluxes(l)
    s.close()


def test_switching(oracle, lattices):
    """The model off mid-run: the constant-viscosity bits from there on (the emulator driven the same way, and a solver that never
    had a model started from that state).  The viscous terms off and on again: the model is kept."""
    key, mu, mode, cfl, wall, lv = LATTICE_A
    case = lattices[key]
    em = vve.configured(oracle, case, mu, mode, cfl, wall, lv, vve.COMBINED)
    want = []
    for leg in range(3):
        if leg == 1:
            em.set_viscosity_model()
        if leg == 2:
            em.set_viscosity_model(law=vve.COMBINED[0], eddy=vve.COMBINED[1])
            em.set_viscous(0.0, levels=0)
            em.set_viscous(mu, ve.PRANDTL, wall, ve.VISCOUS_CFL, lv)
        rc, rms = em.cycles(K)
        assert rc == 0
        want.append((rms, [em.variables(l) for l in range(em.n)], [em.eddy_viscosity(l) for l in range(em.n)] if leg != 1 else None))
    em.close()
    mesh, s = _solver(case)
    _configure(s, mu, mode, cfl, wall, lv, vve.COMBINED)
    for leg in range(3):
        if leg == 1:
            s.set_viscosity_model()
            assert (s.viscosity_model()["law"], s.viscosity_model()["eddy"]) == ("constant", "none")
            ref_mesh, ref = _solver(case)
            ref.set_time_step(mode, cfl)
            for l in range(s.num_levels):
                ref.set(l, "variables", s.get(l, "variables"))
            ref.set_viscous(mu, ve.PRANDTL, bool(wall), ve.VISCOUS_CFL, s.num_levels)
            ref.run_cycles(K)
        if leg == 2:
            _set_model(s, vve.COMBINED)
            s.set_viscous(0.0, levels=0)
            assert (s.viscosity_model()["law"], s.viscosity_model()["eddy"]) == vve.COMBINED
            s.set_viscous(mu, ve.PRANDTL, bool(wall), ve.VISCOUS_CFL, s.num_levels)
            assert not s.get(0, "eddy_viscosity").any()
        rms = s.run_cycles(K)
        _same(rms, want[leg][0], f"leg {leg}: RMS history")
        for l in range(s.num_levels):
            _same(s.get(l, "variables"), want[leg][1][l], f"leg {leg}: level {l}")
            if leg == 1:
                _same(s.get(l, "variables"), ref.get(l, "variables"), f"against a solver that never had a model, level {l}")
            else:
                _same(s.get(l, "eddy_viscosity"), want[leg][2][l], f"leg {leg}: eddy viscosity, level {l}")
        if leg == 1:
            ref.close(); ref_mesh.close()
    s.close()
    mesh.close()


def test_refusals():
    """Unknown law or eddy, bad numbers where used, mid-sweep, a group member and a partitioned solver; the array's access rules:
    error code 1, nothing changed."""
    import mgcfd
    mesh, s = _solver("m6_2lvl")
    ref_mesh, ref = _solver("m6_2lvl")
    for t in (s, ref):
        t.set_viscous(1e-3, levels=1)
        t.set_viscosity_model(law="sutherland", eddy="smagorinsky", t_ref=0.8)
    good = s.viscosity_model()
    assert good == {"law": "sutherland", "t_ref": 0.8, "s": vve.SUTHERLAND_S, "eddy": "smagorinsky", "cs": vve.SMAGORINSKY_CS,
                    "prandtl_t": vve.PRANDTL_TURBULENT}
    nan, inf = float("nan"), float("inf")
    for law, t_ref, sr, eddy, cs, pt in ((2, 0.0, 0.4, 0, 0.17, 0.9), (-1, 0.0, 0.4, 0, 0.17, 0.9), (0, 0.0, 0.4, 3, 0.17, 0.9), (0, 0.0, 0.4, -1, 0.17, 0.9),
                                         (1, -1.0, 0.4, 0, 0.17, 0.9), (0, nan, 0.4, 0, 0.17, 0.9), (1, inf, 0.4, 0, 0.17, 0.9),
                                         (1, 0.0, 0.0, 0, 0.17, 0.9), (1, 0.0, -0.1, 0, 0.17, 0.9), (1, 0.0, nan, 0, 0.17, 0.9), (1, 0.0, inf, 0, 0.17, 0.9),
                                         (0, 0.0, 0.4, 2, 0.0, 0.9), (0, 0.0, 0.4, 2, nan, 0.9), (0, 0.0, 0.4, 2, -1.0, 0.9),
                                         (0, 0.0, 0.4, 2, 0.17, 0.0), (0, 0.0, 0.4, 1, 0.17, nan), (0, 0.0, 0.4, 1, 0.17, -1.0), (0, 0.0, 0.4, 1, 0.17, inf)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            s._c(s.lib.mgcfd_set_viscosity_model(s.handle, law, t_ref, sr, eddy, cs, pt))
        assert e.value.code == 1 and "viscosity model" in str(e.value), (law, t_ref, sr, eddy, cs, pt)
    assert s.viscosity_model() == good
    # a value the model does not use is not looked at
    s._c(s.lib.mgcfd_set_viscosity_model(s.handle, 0, 0.8, nan, 2, 0.17, 0.9))
    s._c(s.lib.mgcfd_set_viscosity_model(s.handle, 1, 0.8, vve.SUTHERLAND_S, 2, 0.17, 0.9))
    # the array: read-only under Smagorinsky, absent on an uncovered level and without an eddy mode
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set(0, "eddy_viscosity", np.zeros(s.nel(0)))
    assert e.value.code == 1
    with pytest.raises(mgcfd.MgcfdError):
        s.get(1, "eddy_viscosity")
    for t in (s, ref):
        t.run_cycles(1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "a cycle after the refused calls")
    s.set_viscosity_model(law="sutherland")
    with pytest.raises(mgcfd.MgcfdError):
        s.get(0, "eddy_viscosity")
    s.set_viscosity_model(eddy="field")
    s.set(0, "eddy_viscosity", np.full(s.nel(0), 1e-3))
    assert (s.get(0, "eddy_viscosity") == 1e-3).all()
    s.set_viscous(0.0, levels=0)
    with pytest.raises(mgcfd.MgcfdError):
        s.get(0, "eddy_viscosity")
    # mid-sweep: the setter is refused until the sweep's last stage has run
    s.sweep_begin(0)
    s.sweep_stage(0, 0, partials=False)
    before = s.viscosity_model()
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_viscosity_model(law="sutherland")
    assert e.value.code == 1 and "sweep is under way" in str(e.value)
    assert s.viscosity_model() == before
    s.sweep_stage(0, 1, partials=False)
    s.sweep_stage(0, 2, partials=False)
    # a group member, and a partitioned solver: a non-default model is refused, the default is not
    s.set_viscosity_model()
    g = mgcfd.Group([s])
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_viscosity_model(law="sutherland")
    assert e.value.code == 1 and "viscosity model" in str(e.value)
    s.set_viscosity_model()
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
        t.set_viscosity_model(eddy="smagorinsky")
    assert e.value.code == 1 and "viscosity model" in str(e.value)
    assert (t.viscosity_model()["law"], t.viscosity_model()["eddy"]) == ("constant", "none")
    t.set_viscosity_model()
    t.close()
    mesh.close()


@pytest.mark.parametrize("key,mu,mode,cfl,wall,lv", PATHS)
def test_fast_mode(key, mu, mode, cfl, wall, lv, oracle, lattices):
    """exact = 0 within tests/test_gpu_viscous.py::test_fast_mode's bounds: 1e-10 of the largest value per level, RMS rtol 1e-9."""
    case = _case(lattices, key)
    want_rms, want_v = _emulate(oracle, case, mu, mode, cfl, wall, lv, vve.COMBINED)[:2]
    mesh, s = _solver(case, exact=0)
    _configure(s, mu, mode, cfl, wall, lv, vve.COMBINED)
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
    if not ok:
        assert r.returncode == 1, r.stdout + r.stderr
    return r


def _strip(out):
    return [l for l in out.splitlines() if not l.startswith("Total runtime = ")]


def test_driver_flags(oracle, tmp_path):
    """--sutherland and --smagorinsky with their companions and the config keys on fvcorr_1lvl: the dump is the %.17e rendering
    of the emulator's state, and not the constant-viscosity run's; without --viscosity / --reynolds, and with --gpus-partition,
    exit status 1 and no dump."""
    case = "fvcorr_1lvl"
    dup = fse.case_duplicate(case)
    name = f"variables.size={dup}x.cycles={K}.level=0"
    em = vve.VariableViscosityOracle(oracle, case, mu=ve.DRIVER_MU, wall=1, viscous_levels="all")
    em.set_viscosity_model(law="sutherland", eddy="smagorinsky")
    t_ref = float(em.model.t_ref)
    rc, want_rms = em.cycles(K)
    assert rc == 0
    want = fse.render_variables(em.variables(0)).encode()
    em.close()
    base = ["--output-variables", "--viscosity", repr(ve.DRIVER_MU), "--no-slip", "--viscous-levels", "8"]
    constant = _run_driver(tmp_path / "constant", case, base, K)
    assert (tmp_path / "constant" / "out" / name).read_bytes() != want
    conf = tmp_path / "run.conf"
    conf.write_text(f"viscosity = {ve.DRIVER_MU!r}\nno_slip = Y\nviscous_levels = 8\nsutherland = Y\nsutherland_tref = {t_ref!r}\n"
                    f"sutherland_s = {vve.SUTHERLAND_S!r}\nsmagorinsky = {vve.SMAGORINSKY_CS!r}\nprandtl_turbulent = {vve.PRANDTL_TURBULENT!r}\n")
    for tag, extra in (("short", base + ["--sutherland", "--smagorinsky"]),
                       ("said", base + ["--sutherland", "--sutherland-tref", repr(t_ref), f"--sutherland-s={vve.SUTHERLAND_S!r}",
                                        "--smagorinsky", repr(vve.SMAGORINSKY_CS), "--prandtl-turbulent", repr(vve.PRANDTL_TURBULENT)]),
                       ("equals", base + [f"--smagorinsky={vve.SMAGORINSKY_CS!r}", "--sutherland"]),
                       ("conf", ["--output-variables", "-c", str(conf)])):
        d = tmp_path / tag
        r = _run_driver(d, case, extra, K)
        assert (d / "out" / name).read_bytes() == want, tag
        lines = _strip(r.stdout)
        assert len(lines) == len(_strip(constant.stdout))
        assert [l for l in lines if "(RMS = " in l] == [f"Cycle {i + 1} / {K}" + " (RMS = %.3e)" % want_rms[i] for i in range(K)]
    for tag, bad in (("no_viscosity", ["--sutherland"]), ("no_viscosity2", ["--smagorinsky", "0.2"]), ("no_viscosity3", ["--prandtl-turbulent", "0.9"]),
                     ("partition", base + ["--smagorinsky", "--gpus", "2", "--gpus-partition", "--gpus-share-device"]),
                     ("bad_cs", base + ["--smagorinsky=-1"]), ("bad_s", base + ["--sutherland", "--sutherland-s", "0"])):
        r = _run_driver(tmp_path / tag, case, ["--output-variables"] + bad, K, ok=False)
        assert not [n for n in os.listdir(tmp_path / tag / "out") if n.startswith("variables")], tag


def test_defaults_reproduce_the_golden_output(tmp_path):
    """With the flags absent the golden variables.level0.txt byte for byte, and so the Python API after a model set and unset."""
    case = "m6_2lvl"
    meta = dict(l.strip().split(" = ") for l in open(os.path.join(fse.GOLDEN, case, "case.txt")))
    cycles, dup = int(meta["cycles"]), fse.case_duplicate(case)
    golden = open(os.path.join(fse.GOLDEN, case, "variables.level0.txt"), "rb").read()
    _run_driver(tmp_path / "plain", case, ["--output-variables"], cycles)
    assert (tmp_path / "plain" / "out" / f"variables.size={dup}x.cycles={cycles}.level=0").read_bytes() == golden
    mesh, s = _solver(case)
    assert s.viscosity_model() == {"law": "constant", "t_ref": 0.0, "s": vve.SUTHERLAND_S, "eddy": "none", "cs": vve.SMAGORINSKY_CS,
                                   "prandtl_t": vve.PRANDTL_TURBULENT}
    s.set_viscosity_model(law="sutherland", eddy="smagorinsky")            # (without the viscous terms: no effect)
    s.run_cycles(cycles)
    assert fse.render_variables(s.get(0, "variables")).encode() == golden
    s.close()
    mesh.close()


def test_polar_with_viscosity_model(oracle):
    """Solver.polar(viscous=..., viscosity_model=...) = the two setters once, then the polar; the solver keeps both."""
    case, alphas, mach = fse.POLAR_CASE, fse.POLAR_ALPHAS, fse.POLAR_MACH
    mesh, s = _solver(case)
    t_ref = float(vve.far_field_t_ref(s.far_field()))
    pol = s.polar(alphas, K, mach=mach, viscous={"mu": ve.DRIVER_MU, "wall": True, "levels": 2},
                  viscosity_model={"law": "sutherland", "eddy": "smagorinsky"})
    got = s.viscosity_model()
    assert (got["law"], got["eddy"], got["t_ref"]) == ("sutherland", "smagorinsky", t_ref)
    em = vve.VariableViscosityOracle(oracle, case, mu=ve.DRIVER_MU, wall=1, viscous_levels=2)
    em.set_viscosity_model(law="sutherland", eddy="smagorinsky")
    for k, (al, p) in enumerate(zip(alphas, pol)):
        em.set_far_field(fse.free_stream_constants(mach, al), reinitialise=(k == 0))
        rc, rms = em.cycles(K)
        assert rc == 0
        _same(p["rms"], rms, f"polar, angle {al}: RMS history")
    _same(s.get(0, "variables"), em.variables(0), "the polar's last state")
    em.close()
    s.close(); mesh.close()


def test_device_resources():
    """A non-default model adds the eddy viscosity and d2 per covered level, once; either setting going off releases them;
    destroy returns to the baseline."""
    import mgcfd
    base = mgcfd.live_device_resources()
    mesh, s = _solver("m6_3lvl")
    s.run_cycles(1)
    s.set_viscosity_model(law="sutherland")                    # (the viscous terms are off: nothing is allocated)
    plain = mgcfd.live_device_resources()
    s.set_viscous(1e-3, levels=2)
    on = mgcfd.live_device_resources()
    assert on["allocations"] - plain["allocations"] == 2 * 3 + 1 + 2 * 2
    s.set_viscosity_model()
    viscous_only = mgcfd.live_device_resources()
    assert viscous_only["allocations"] == on["allocations"] - 2 * 2
    s.set_viscosity_model(eddy="smagorinsky")
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"]
    assert mgcfd.live_device_resources()["bytes"] - viscous_only["bytes"] >= sum(2 * 8 * s.nel(l) for l in range(2))
    s.set_viscosity_model(law="sutherland", eddy="field")
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"], "allocated once"
    s.set_viscous(1e-3, levels=3)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"] + 3 + 2, "a further level: its five arrays"
    s.run_cycles(1)
    s.set_viscous(0.0, levels=0)
    off = mgcfd.live_device_resources()
    assert off["allocations"] == plain["allocations"] and off["bytes"] == plain["bytes"], "switching the terms off releases"
    s.close(); mesh.close()
    end = mgcfd.live_device_resources()
    assert end["allocations"] == base["allocations"] and end["bytes"] == base["bytes"]
