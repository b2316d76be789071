"""GPU tests of the wall distance (mgcfd_compute_wall_distance, mgcfd_wall_nearest, mgcfd_wall_spacing, mgcfd_set_wall_damping)
against the numpy emulator (tests/wall_distance_emulator.py) bit for bit: d, nearest and h on the shapes at which the all-pairs
kernel can go wrong; numbering; the damped Smagorinsky runs (state, step factors, RMS history, S, eddy_viscosity, F + V, the
friction loads); a composed run; the fast mode; the setting and its refusals; device allocations; the driver's flag.
tests/test_host_wall_distance.py checks the emulator itself and asserts on the CPU that every damped run stays valid."""
import ctypes
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
import wall_distance_emulator as wde

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
K = ve.GPU_CYCLES
REL_RUN = 1e-10          # tests/test_gpu_viscous.py::test_fast_mode's tolerances
RMS_FAST = 1e-9
REF = (0.25, -0.125, 0.375)
LATTICE_A = ("A", ve.CELL_RE_MU, "local", 1.0, 1, "all")
SMAGORINSKY = wde.DAMPED_MODELS[0]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(got - want).max():.3e}"


# ---- geometry: d, nearest and h bit for bit ----
# The smallest shapes at which k_wall_distance can go wrong (tile 256, chunk 256; tests/test_host_wall_distance.py counts them):
#   A      2,178 / 728 / 215 nodes, 38 / 6 / 6 wall nodes: a last partial tile, fewer wall nodes than a wavefront, ties on levels 1, 2
#   box17  4,452 nodes, 278 wall nodes: more than one chunk, a partial last chunk, 1,404 tied nodes
#   box21  7,866 nodes, 546 wall nodes: three chunks
#   tet    30,000 nodes, 19 wall nodes: the tetrahedral plan's node order
#   box9   no wall: +inf / -1 everywhere, h empty
def _generated(name):
    from mgcfd import meshgen
    if name == "A":
        return meshgen.make_multigrid(fe.LATTICES["A"], "fvcorr", **fe.LATTICE_ARGS)
    level = {"box17": lambda: meshgen.make_box_level(17, seed=3, cavity_radius=0.3),
             "box21": lambda: meshgen.make_box_level(21, seed=3, cavity_radius=0.35),
             "tet": lambda: meshgen.make_tet_level(30000, seed=0),
             "box9": lambda: meshgen.make_box_level(9)}[name]()
    return meshgen.MultigridMesh(mesh_name="fvcorr", levels=[level])


def _device_doubles(ptr, count):
    """``count`` doubles at a device address, through the runtime the library is linked against."""
    hip = ctypes.CDLL("libamdhip64.so")
    out = np.empty(count)
    rc = hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(8 * count), ctypes.c_int(2))
    assert rc == 0
    return out


@pytest.mark.parametrize("name", ["A", "box17", "box21", "tet", "box9"])
def test_distance_nearest_and_spacing_equal_the_emulator(name):
    import mgcfd
    mg = _generated(name)
    levels = mgcfd.generated_to_levels(mg)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    assert s.wall_distance_levels() == 0
    with pytest.raises(mgcfd.MgcfdError):
        s.get(0, "wall_distance")
    s.compute_wall_distance()
    assert s.wall_distance_levels() == s.num_levels
    for l, lv in enumerate(mg.levels):
        w = wde.level_wall_nodes(lv)
        want_d, want_near = wde.wall_distance(lv.coords, w)
        d, near = s.get(l, "wall_distance").ravel(), s.wall_nearest(l)
        what = f"{name} level {l}"
        print(what, lv.nel, "nodes", len(w), "wall nodes", "d max", want_d.max())
        assert s.wall_node_count(l) == len(w)
        _same(d, want_d, f"{what}: d")
        assert np.array_equal(near, want_near), f"{what}: nearest"
        ids, h = s.wall_spacing(l)
        assert np.array_equal(ids, w)
        internal, _ = fle.slices(levels[l])
        _same(h, wde.wall_spacing(want_d, s.get_edges(l, len(levels[l]["edges"]))[internal], w), f"{what}: h")
        if len(w):
            assert np.array_equal(_bits(d[w]), _bits(np.zeros(len(w)))) and np.array_equal(near[w], w) and (h > 0.0).any()
        else:
            assert np.isposinf(d).all() and (near == -1).all() and len(h) == 0
        # numbering: the device holds d in the library's numbering ([1][stride], pad lanes +inf), get hands it out in original order
        ptr, count = s.array_devptr(l, "wall_distance")
        dev = _device_doubles(ptr, count)
        assert count >= lv.nel and count % 256 == 0 and np.isposinf(dev[lv.nel:]).all()
        assert np.array_equal(np.sort(_bits(dev[:lv.nel])), np.sort(_bits(d)))
        if len(w):
            assert not np.array_equal(_bits(dev[:lv.nel]), _bits(d)), f"{what}: the level is renumbered"
        with pytest.raises(mgcfd.MgcfdError) as e:
            s.set(l, "wall_distance", d)
        assert e.value.code == 1
    s.close()


# ---- damped runs ----
@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("wall_distance_lattices")
    return {name: fe.write_lattice(name, d) for name in fe.LATTICES}


def _solver(case, exact=1):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    s.set_option("exact", exact)
    return mesh, s


def _configure(s, mu, mode, cfl, wall, model, smoothing=(0.0, 0), jst_levels=0, fas=False, order=(0, 1, 2)):
    """The solver as wde.configured sets the emulator up; ``order``: the order of the three setters that make the damping effective."""
    s.set_time_step(mode, cfl)
    if smoothing[1]:
        s.set_residual_smoothing(*smoothing)
    if jst_levels:
        s.set_jst(levels=jst_levels)
    if fas:
        s.set_fas(True)
    s.set(0, "variables", ve.start_state(s.nel(0), s.far_field()[:5]))
    setters = (lambda: s.set_viscous(mu, ve.PRANDTL, bool(wall), ve.VISCOUS_CFL, s.num_levels),
               lambda: s.set_viscosity_model(law=model[0], eddy=model[1]),
               lambda: s.set_wall_damping(True, wde.WALL_KAPPA))
    for k in order:
        setters[k]()
    assert s.wall_damping() == (True, wde.WALL_KAPPA) and s.wall_distance_levels() == s.num_levels


_emulated = {}


def _emulate(oracle, case, mu, mode, cfl, wall, lv, model):
    """(rms, variables, step factors, eddy viscosity after the run, (S, mut, F + V) of the final state) per level of K cycles:
    computed once per combination, shared and left unchanged."""
    key = (case, mu, mode, cfl, wall, lv, tuple(model))
    if key not in _emulated:
        em = wde.configured(oracle, case, mu, mode, cfl, wall, lv, model)
        rc, rms = em.cycles(K)
        assert rc == 0
        v = [em.variables(l) for l in range(em.n)]
        sf = [em.step_factors(l) for l in range(em.n)]
        mut_run = [em.eddy_viscosity(l) for l in range(em.n)]
        sfl = []
        for l in range(em.n):
            f = em.stage_fluxes(l)
            sfl.append((em.last_S[l].copy(), em.eddy_viscosity(l), f))
        _emulated[key] = (rms, v, sf, mut_run, sfl, [w.copy() for w in em.wall_nodes])
        em.close()
    return _emulated[key]


def _check_run(s, want, what):
    want_rms, want_v, want_sf, want_mut, want_sfl, walls = want
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), want_v[l], f"{what}: variables, level {l}")
        _same(s.get(l, "step_factors"), want_sf[l], f"{what}: step factors, level {l}")
        mut = s.get(l, "eddy_viscosity").ravel()
        _same(mut, want_mut[l], f"{what}: eddy viscosity after the run, level {l}")
        assert not _bits(mut[walls[l]]).any(), f"{what}: eddy viscosity is +0.0 at the wall nodes, level {l}"
        s.compute_fluxes(l)
        S, m, f = want_sfl[l]
        _same(s.get(l, "fluxes"), f, f"{what}: F + V, level {l}")
        _same(s.get(l, "viscous_stress"), S, f"{what}: S, level {l}")
        _same(s.get(l, "eddy_viscosity").ravel(), m, f"{what}: eddy viscosity, level {l}")
        s.zero_fluxes(l)


@pytest.mark.parametrize("key,mu,mode,cfl,wall,lv,model", wde.gpu_runs())
def test_damped_runs_equal_the_emulator(key, mu, mode, cfl, wall, lv, model, oracle, lattices):
    """After K cycles from the perturbed start state with the damping on: `variables` and step factors of every level, the RMS
    history, the eddy viscosity the last stage left (+0.0 at every wall node), and S, eddy_viscosity and F + V of the final
    state, bitwise the emulator's."""
    case = lattices.get(key, key)
    want = _emulate(oracle, case, mu, mode, cfl, wall, lv, model)
    mesh, s = _solver(case)
    _configure(s, mu, mode, cfl, wall, model)
    rms = s.run_cycles(K)
    what = f"{key} mu={mu} {mode} {cfl} {model}"
    print(what, "rms", rms, "want", want[0])
    _same(rms, want[0], f"{what}: RMS history")
    _check_run(s, want, what)
    s.close()
    mesh.close()


def test_a_level_without_walls_runs_as_the_undamped_model(oracle, tmp_path):
    """d = +inf everywhere: l2 = c2 * d2 and the run is bit for bit the undamped model's (two solvers, and the emulator)."""
    import mgcfd
    from mgcfd import meshgen
    mg = meshgen.MultigridMesh(mesh_name="fvcorr", levels=[meshgen.make_box_level(9, seed=2, jitter=0.2)])
    got = []
    for damped in (False, True):
        s = mgcfd.Solver.from_generated(mg)
        s.set_time_step("local", 1.0)
        s.set(0, "variables", ve.start_state(s.nel(0), s.far_field()[:5]))
        s.set_viscous(0.05, ve.PRANDTL, True, ve.VISCOUS_CFL, 1)
        s.set_viscosity_model(law=vve.COMBINED[0], eddy=vve.COMBINED[1])
        if damped:
            s.set_wall_damping()
            assert np.isposinf(s.get(0, "wall_distance")).all() and (s.wall_nearest(0) == -1).all()
        rms = s.run_cycles(K)
        got.append((rms, s.get(0, "variables"), s.get(0, "eddy_viscosity")))
        s.close()
    assert got[0][2].any()
    for a, b, what in zip(got[0], got[1], ("RMS history", "variables", "eddy viscosity")):
        _same(b, a, f"no wall: {what}")


@pytest.mark.parametrize("model", wde.DAMPED_MODELS, ids=lambda m: "-".join(m))
def test_friction_loads(model):
    """Damped, on lattice A (all levels, no-slip walls, after K cycles), on every level: surface_loads(friction=True), wall_stress
    and wall_distribution are bitwise the emulator's on the state read back, the wall rows of S included."""
    import mgcfd
    mg = fle.generated("A")
    levels = mgcfd.generated_to_levels(mg)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    mu = ve.CELL_RE_MU
    s.set(0, "variables", ve.start_state(s.nel(0), s.far_field()[:5]))
    s.set_wall_damping()
    s.set_viscous(mu, ve.PRANDTL, True, ve.VISCOUS_CFL, s.num_levels)
    s.set_viscosity_model(law=model[0], eddy=model[1])
    s.run_cycles(K)
    m = vve.Model(model[0], vve.far_field_t_ref(s.far_field()), eddy=model[1])
    for l in range(s.num_levels):
        what = f"{model} level {l}"
        v, e = s.get(l, "variables"), s.get_edges(l, len(levels[l]["edges"]))
        w = wde.level_wall_nodes(mg.levels[l])
        S = wde.node_stresses(v, e, levels[l], mu, ve.PRANDTL, m, wde.WALL_KAPPA, w)
        free = vve.node_stresses(v, e, levels[l], mu, ve.PRANDTL, m)
        assert not np.array_equal(_bits(S[w]), _bits(free[w])), f"{what}: the damping changes the wall stresses"
        want12 = vve.surface_loads12(v, e, levels[l], s.far_field(), REF, S)
        want_ids, want_table = vve.distribution(v, e, levels[l], s.far_field(), S)
        _same(s.surface_loads(l, REF, friction=True), want12, f"{what}: loads")
        ids, table = s.wall_distribution(l)
        assert np.array_equal(ids, want_ids) and np.array_equal(ids, w)
        _same(table, want_table, f"{what}: distribution")
        ids, sw = s.wall_stress(l)
        _same(sw, S[want_ids], f"{what}: Sw")
        s.compute_fluxes(l)
        _same(sw, s.get(l, "viscous_stress")[ids], f"{what}: Sw against the wall rows of S")
        s.zero_fluxes(l)
    s.close()


def test_composition(oracle, lattices):
    """Lattice A, the combined model, damped, with residual smoothing, JST, dual time (BDF2) and FAS together."""
    name, mode, cfl, smoothing, jst_levels, order, fas = wde.COMPOSED
    case = lattices["A"]
    em = wde.configured(oracle, case, ve.CELL_RE_MU, mode, cfl, 1, "all", vve.COMBINED, smoothing=smoothing, jst_levels=jst_levels, fas=fas)
    mesh, s = _solver(case)
    _configure(s, ve.CELL_RE_MU, mode, cfl, 1, vve.COMBINED, smoothing, jst_levels, fas)
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
        _same(s.get(l, "eddy_viscosity").ravel(), em.eddy_viscosity(l), f"{name}: eddy viscosity, level {l}")
    em.close()
    s.close(); mesh.close()


def test_fast_mode(oracle, lattices):
    """exact = 0: d is bitwise (geometry does not depend on MGCFD_OPT_EXACT); the damped state is within
    tests/test_gpu_viscous.py::test_fast_mode's bounds: 1e-10 of the largest value per level, RMS rtol 1e-9."""
    key, mu, mode, cfl, wall, lv = LATTICE_A
    case = lattices[key]
    want_rms, want_v = _emulate(oracle, case, mu, mode, cfl, wall, lv, vve.COMBINED)[:2]
    mesh, s = _solver(case, exact=0)
    _configure(s, mu, mode, cfl, wall, vve.COMBINED)
    em = wde.configured(oracle, case, mu, mode, cfl, wall, lv, vve.COMBINED)
    for l in range(s.num_levels):
        _same(s.get(l, "wall_distance").ravel(), em.wall_distance(l)[0], f"fast mode: d, level {l}")
        assert np.array_equal(s.wall_nearest(l), em.wall_distance(l)[1])
    em.close()
    rms = s.run_cycles(K)
    assert np.allclose(rms, want_rms, rtol=RMS_FAST, atol=0)
    for l in range(s.num_levels):
        rel = np.abs(s.get(l, "variables") - want_v[l]).max() / max(np.abs(want_v[l]).max(), 1e-300)
        print("fast mode: level", l, "rel", rel)
        assert rel <= REL_RUN, f"level {l}: {rel:.3e}"
    s.close()
    mesh.close()


# ---- the setting ----
def test_any_order_of_the_setters_reaches_the_same_bits(oracle, lattices):
    import itertools
    key, mu, mode, cfl, wall, lv = LATTICE_A
    case = lattices[key]
    want = _emulate(oracle, case, mu, mode, cfl, wall, lv, vve.COMBINED)
    for order in itertools.permutations((0, 1, 2)):
        mesh, s = _solver(case)
        _configure(s, mu, mode, cfl, wall, vve.COMBINED, order=order)
        rms = s.run_cycles(K)
        _same(rms, want[0], f"order {order}: RMS history")
        for l in range(s.num_levels):
            _same(s.get(l, "variables"), want[1][l], f"order {order}: level {l}")
        s.close()
        mesh.close()
    # kappa and cs changed by a later setter: l2 is formed again
    mesh, s = _solver(case)
    _configure(s, mu, mode, cfl, wall, vve.COMBINED)
    s.set_wall_damping(True, 0.3)
    s.set_viscosity_model(law=vve.COMBINED[0], eddy=vve.COMBINED[1], cs=0.2)
    em = wde.configured(oracle, case, mu, mode, cfl, wall, lv, vve.COMBINED)
    em.set_wall_damping(True, 0.3)
    em.set_viscosity_model(law=vve.COMBINED[0], eddy=vve.COMBINED[1], cs=0.2)
    rc, want_rms = em.cycles(K)
    assert rc == 0
    _same(s.run_cycles(K), want_rms, "kappa 0.3, cs 0.2: RMS history")
    _same(s.get(0, "variables"), em.variables(0), "kappa 0.3, cs 0.2: level 0")
    # off again: the undamped model's bits from the same state
    s.set_wall_damping(False)
    em.set_wall_damping(False)
    rc, want_rms = em.cycles(1)
    _same(s.run_cycles(1), want_rms, "damping off: RMS history")
    _same(s.get(0, "variables"), em.variables(0), "damping off: level 0")
    em.close()
    s.close(); mesh.close()


def test_refusals_and_device_resources():
    """MGCFD_ERR_ARG with the getters unchanged: levels out of range, a level without coordinates, a bad kappa, release while the
    damping is in effect, mid-sweep, a group member and a partitioned solver, NULL outputs; the allocation count returns."""
    import mgcfd
    mesh, s = _solver("m6_2lvl")
    s.run_cycles(1)
    s.wall_node_count(0); s.wall_node_count(1)                       # (the wall plans go with the solver, as §14 has it)
    plain = mgcfd.live_device_resources()

    def refused(call, text="wall"):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1 and text in str(e.value), str(e.value)

    for levels in (0, -1, 3):
        refused(lambda: s.compute_wall_distance(levels))
    assert s.wall_distance_levels() == 0
    refused(lambda: s.wall_nearest(0))
    refused(lambda: s.wall_spacing(0))
    s.compute_wall_distance(1)
    assert s.wall_distance_levels() == 1
    held = mgcfd.live_device_resources()
    assert held["allocations"] == plain["allocations"] + 2 and held["bytes"] - plain["bytes"] >= 12 * s.nel(0)
    s.compute_wall_distance(1)
    assert mgcfd.live_device_resources()["allocations"] == held["allocations"], "a held level is not computed again"
    refused(lambda: s.get(1, "wall_distance"), "WALL_DISTANCE")
    refused(lambda: s._c(s.lib.mgcfd_wall_nearest(s.handle, 0, None)), "null")
    refused(lambda: s._c(s.lib.mgcfd_wall_spacing(s.handle, 0, None, None)), "null")
    for kappa in (0.0, -0.41, float("nan"), float("inf")):
        refused(lambda: s.set_wall_damping(True, kappa))
    assert s.wall_damping() == (False, wde.WALL_KAPPA)
    # in effect: both levels hold d, l2 per level; release is refused
    s.set_viscous(1e-3, wall=True, levels=2)
    viscous_only = mgcfd.live_device_resources()
    s.set_viscosity_model(eddy="smagorinsky")
    before = mgcfd.live_device_resources()
    s.set_wall_damping(True, 0.4)
    assert s.wall_distance_levels() == 2 and s.wall_damping() == (True, 0.4)
    assert mgcfd.live_device_resources()["allocations"] == before["allocations"] + 2 + 2
    refused(s.release_wall_distance)
    assert s.wall_distance_levels() == 2
    # the settings go off, then release: the count returns
    s.set_viscosity_model()
    assert mgcfd.live_device_resources()["allocations"] == viscous_only["allocations"] + 2, "l2 is gone, level 1's d and nearest stay"
    s.set_viscous(0.0, levels=0)
    s.set_wall_damping(False)
    s.release_wall_distance()
    assert s.wall_distance_levels() == 0
    end = mgcfd.live_device_resources()
    assert end["allocations"] == plain["allocations"] and end["bytes"] == plain["bytes"]
    # mid-sweep
    s.sweep_begin(0)
    s.sweep_stage(0, 0, partials=False)
    refused(lambda: s.set_wall_damping(True, 0.4), "sweep is under way")
    refused(lambda: s.compute_wall_distance(2), "sweep is under way")
    assert s.wall_damping() == (False, wde.WALL_KAPPA) and s.wall_distance_levels() == 0
    s.sweep_stage(0, 1, partials=False)
    s.sweep_stage(0, 2, partials=False)
    # a group member
    g = mgcfd.Group([s])
    refused(lambda: s.compute_wall_distance(1))
    refused(lambda: s.set_wall_damping(True))
    assert s.wall_damping() == (False, wde.WALL_KAPPA) and s.wall_distance_levels() == 0
    g.close()
    s.close(); mesh.close()
    # a solver created without coordinates: compute is refused, and so is the setter that would make the damping effective
    # (a single undamped level: its creation needs none)
    flat = mgcfd.Mesh("input.dat", fse.case_input("fvcorr_1lvl"), 1)
    levels = [dict(flat.level(l)) for l in range(flat.num_levels)]
    for lv in levels:
        lv["coords"] = None
    t = mgcfd.Solver.from_arrays(levels, flat.variant)
    refused(lambda: t.compute_wall_distance(1), "coordinates")
    t.set_viscous(1e-3, levels=1)
    t.set_wall_damping(True)                                         # (not effective yet: kept)
    refused(lambda: t.set_viscosity_model(eddy="smagorinsky"), "coordinates")
    assert t.viscosity_model()["eddy"] == "none" and t.wall_distance_levels() == 0
    t.set_wall_damping(False)
    t.set_viscosity_model(eddy="smagorinsky")
    refused(lambda: t.set_wall_damping(True), "coordinates")
    assert t.wall_damping() == (False, wde.WALL_KAPPA)
    t.close()
    flat.close()
    # a partitioned solver
    from mgcfd.partition import partition_hierarchy, rcb_partition
    mesh = mgcfd.Mesh("input.dat", fse.case_input("m6_2lvl"), 1)
    levels = [mesh.level(l) for l in range(mesh.num_levels)]
    H = partition_hierarchy(levels, rcb_partition(np.asarray(levels[0]["coords"]).reshape(-1, 3), 2))
    lv, owned, keys = H[0].solver_args()
    t = mgcfd.Solver.from_arrays(lv, mesh.variant, n_owned=owned, order_keys=keys)
    refused(lambda: t.compute_wall_distance(1))
    refused(lambda: t.set_wall_damping(True))
    refused(t.release_wall_distance)
    assert t.wall_damping() == (False, wde.WALL_KAPPA)
    t.close()
    mesh.close()


def test_polar_with_wall_damping():
    import mgcfd
    mesh, s = _solver(fse.POLAR_CASE)
    s.polar(fse.POLAR_ALPHAS[:1], 1, mach=fse.POLAR_MACH, viscous={"mu": ve.DRIVER_MU, "wall": True, "levels": 2},
            viscosity_model={"eddy": "smagorinsky"}, wall_damping={"kappa": 0.4})
    assert s.wall_damping() == (True, 0.4) and s.wall_distance_levels() == 2
    s.close(); mesh.close()


# ---- the drop-in binary ----
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


def test_driver_flag(oracle, tmp_path):
    """--wall-damping and --wall-damping=0.41 (and the config key) on m6_2lvl, which has solid walls on both levels (18 and 6 wall
    nodes): the dump is the %.17e rendering of the emulator's state and not the undamped run's; without --smagorinsky, and with
    --gpus 2, exit status 1 and no dump; so on fvcorr_1lvl, whose single undamped level the reader loads without coordinates."""
    case = "m6_2lvl"
    dup = fse.case_duplicate(case)
    name = f"variables.size={dup}x.cycles={K}.level=0"
    em = wde.WallDampedOracle(oracle, case, mu=ve.DRIVER_MU, wall=1, viscous_levels="all")
    assert [len(w) for w in em.wall_nodes] == [18, 6]
    em.set_viscosity_model(law="constant", eddy="smagorinsky")
    em.set_wall_damping(True)
    rc, want_rms = em.cycles(K)
    assert rc == 0
    want = fse.render_variables(em.variables(0)).encode()
    em.close()
    base = ["--output-variables", "--viscosity", repr(ve.DRIVER_MU), "--no-slip", "--viscous-levels", "8", "--smagorinsky"]
    undamped = _run_driver(tmp_path / "undamped", case, base, K)
    assert (tmp_path / "undamped" / "out" / name).read_bytes() != want
    conf = tmp_path / "run.conf"
    conf.write_text(f"viscosity = {ve.DRIVER_MU!r}\nno_slip = Y\nviscous_levels = 8\nsmagorinsky = Y\nwall_damping = {wde.WALL_KAPPA!r}\n")
    for tag, extra in (("short", base + ["--wall-damping"]), ("equals", base + ["--wall-damping=0.41"]),
                       ("conf", ["--output-variables", "-c", str(conf)])):
        d = tmp_path / tag
        r = _run_driver(d, case, extra, K)
        assert (d / "out" / name).read_bytes() == want, tag
        lines = _strip(r.stdout)
        assert len(lines) == len(_strip(undamped.stdout))
        assert [l for l in lines if "(RMS = " in l] == [f"MG cycle {i + 1} / {K}" + " (RMS = %.3e)" % want_rms[i] for i in range(K)]
    no_model = ["--output-variables", "--viscosity", repr(ve.DRIVER_MU), "--no-slip"]
    for tag, bad in (("no_smagorinsky", no_model + ["--wall-damping"]), ("no_viscosity", ["--output-variables", "--wall-damping"]),
                     ("gpus", base + ["--wall-damping", "--gpus", "2", "--gpus-share-device"]),
                     ("gpus_no_model", no_model + ["--wall-damping", "--gpus", "2", "--gpus-share-device"]),
                     ("bad_kappa", base + ["--wall-damping=-1"])):
        _run_driver(tmp_path / tag, case, bad, K, ok=False)
        assert not [n for n in os.listdir(tmp_path / tag / "out") if n.startswith("variables")], tag
    r = _run_driver(tmp_path / "no_coords", "fvcorr_1lvl", base + ["--wall-damping"], K, ok=False)
    assert "without coordinates" in r.stderr and not [n for n in os.listdir(tmp_path / "no_coords" / "out") if n.startswith("variables")]


def test_defaults_reproduce_the_golden_output(tmp_path):
    """With the flag absent the golden variables.level0.txt byte for byte, and so the Python API with the damping set while the
    viscous terms are off (no effect, nothing computed)."""
    case = "m6_2lvl"
    meta = dict(l.strip().split(" = ") for l in open(os.path.join(fse.GOLDEN, case, "case.txt")))
    cycles, dup = int(meta["cycles"]), fse.case_duplicate(case)
    golden = open(os.path.join(fse.GOLDEN, case, "variables.level0.txt"), "rb").read()
    _run_driver(tmp_path / "plain", case, ["--output-variables"], cycles)
    assert (tmp_path / "plain" / "out" / f"variables.size={dup}x.cycles={cycles}.level=0").read_bytes() == golden
    mesh, s = _solver(case)
    assert s.wall_damping() == (False, wde.WALL_KAPPA)
    s.set_wall_damping(True)
    s.set_viscosity_model(eddy="smagorinsky")
    assert s.wall_distance_levels() == 0
    s.run_cycles(cycles)
    assert fse.render_variables(s.get(0, "variables")).encode() == golden
    s.close()
    mesh.close()
