"""GPU tests of the Spalart-Allmaras model (mgcfd_set_viscosity_model with MGCFD_EDDY_SPALART_ALLMARAS, mgcfd_set_sa_free_stream)
against the numpy emulator (tests/sa_emulator.py) bit for bit: the three kernels on the shapes at which their gathers can go wrong;
the runs (state, nu_tilde and eddy viscosity of every covered level, step factors, RMS history); the composed runs; the friction
loads; a restart; the setters in either order; the refusals and the device allocations; polar; the driver's flag; the fast mode.
tests/test_host_sa.py checks the emulator itself and asserts on the CPU that every run here stays valid."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import fas_emulator as fe
import free_stream_emulator as fse
import friction_loads_emulator as fle
import sa_emulator as sae
import variable_viscosity_emulator as vve
import viscous_emulator as ve
import wall_distance_emulator as wde

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
K = sae.GPU_CYCLES
REL_RUN = 1e-10          # tests/test_gpu_viscous.py::test_fast_mode's tolerances
RMS_FAST = 1e-9
REF = (0.25, -0.125, 0.375)
LATTICE_A = ("A", ve.CELL_RE_MU, "local", 1.0, 1, "all", sae.MODELS[1])


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(got - want).max():.3e}"


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("sa_lattices")
    return {name: fe.write_lattice(name, d) for name in fe.LATTICES}


def _solver(case, exact=1):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    s.set_option("exact", exact)
    return mesh, s


def _levels(s, lv):
    return s.num_levels if lv == "all" else lv


def _configure(s, mu, mode, cfl, wall, lv, model, smoothing=(0.0, 0), jst_levels=0, fas=False, shape="V", order=(0, 1)):
    """The solver as sae.configured sets the emulator up; ``order``: the order of the two setters that make the model effective."""
    s.set_time_step(mode, cfl)
    if smoothing[1]:
        s.set_residual_smoothing(*smoothing)
    if jst_levels:
        s.set_jst(levels=jst_levels)
    if fas:
        s.set_fas(True)
    if shape != "V":
        s.set_cycle(shape)
    s.set(0, "variables", ve.start_state(s.nel(0), s.far_field()[:5]))
    setters = (lambda: s.set_viscous(mu, ve.PRANDTL, bool(wall), ve.VISCOUS_CFL, _levels(s, lv)),
               lambda: s.set_viscosity_model(law=model[0], eddy=model[1]))
    for k in order:
        setters[k]()
    got = s.viscosity_model()
    assert (got["law"], got["eddy"]) == tuple(model) and s.wall_distance_levels() >= _levels(s, lv)


# ---- kernel level ----
def _kernel_cases(lattices, tmp_path):
    """(name, case directory, perturbation amplitude, CFL, mu): lattices A and B (a last partial tile, more than one tile), the
    generated tetrahedral level (halo nodes beyond the LDS table: the overflow list; long rows: the TAIL instantiation), the hub
    (a row longer than a tile), nodes without an internal edge, and a level without walls (d = +inf)."""
    from mgcfd import meshgen
    from test_gpu_variable_viscosity import _isolated_level
    cases = [("lattice_A", lattices["A"], 0.01, 1.0, ve.CELL_RE_MU), ("lattice_B", lattices["B"], 0.01, 1.0, ve.CELL_RE_MU)]
    for name, level, amplitude, cfl, mu in (("tet", meshgen.make_tet_level(30000, seed=0), 0.002, 0.02, 1e-3),
                                            ("hub", meshgen.make_hub_level(600, scale=1e-4, seed=5), 0.002, 0.02, 1e-9),
                                            ("isolated", _isolated_level(), 0.002, 0.02, 1e-9),
                                            ("no_wall", meshgen.make_box_level(9, seed=2, jitter=0.2), 0.01, 1.0, 0.05)):
        mg = meshgen.MultigridMesh(mesh_name="fvcorr")
        mg.levels.append(level)
        d = tmp_path / name
        os.makedirs(d / "input")
        meshgen.write_input(mg, str(d / "input"))
        (d / "case.txt").write_text("duplicate = 1\n")
        cases.append((name, str(d), amplitude, cfl, mu))
    return cases


def test_kernel_level(oracle, lattices, tmp_path):
    """A perturbed W, a random nt_old (through mgcfd_copy_old_variables) and a random nt, the step factors of that state; then
    mgcfd_compute_fluxes and mgcfd_time_step(0, 0): sa_gradient, eddy_viscosity, S, F + V and the new nt bitwise the emulator's."""
    import mgcfd
    from conftest import perturbed_state
    total = {k: 0 for k in sae.BRANCHES}
    for name, case, amplitude, cfl, mu in _kernel_cases(lattices, tmp_path):
        mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
        levels = [dict(mesh.level(l)) for l in range(mesh.num_levels)]
        if levels[0].get("coords") is None or len(levels[0]["coords"]) == 0:
            # (the reader loads a single undamped level without coordinates: the ones the emulator reads)
            em0 = sae.SaOracle(oracle, case, "local", cfl)
            levels[0]["coords"] = em0.oc.array(0, "coords").reshape(-1, 3).copy()
            em0.close()
        s = mgcfd.Solver.from_arrays(levels, mesh.variant)
        t = s.tiling(0)
        print(name, t)
        if name == "tet":
            assert t["tiles"] > 1 and t["overflow_refs"] > 0 and t["list_entries"] > 0
        elif name == "hub":
            assert t["list_entries"] > 0
        elif name == "lattice_A":
            assert t["tiles"] > 1 and s.nel(0) % 256 != 0
        start = perturbed_state(s.nel(0), s.far_field()[:5], seed=7, amplitude=amplitude)
        em, old, new, sf, (grad, mut, S, f, out, masks) = sae.kernel_level_case(oracle, case, mu, cfl, start)
        for k in sae.BRANCHES:
            total[k] += int(masks[k].sum())
        s.set_time_step("local", cfl)
        s.set(0, "variables", start)
        s.set_viscous(mu, wall=True)
        s.set_viscosity_model(law="sutherland", eddy=sae.SA)
        d = s.get(0, "wall_distance").ravel()
        _same(d, em.wall_distance(0)[0], f"{name}: d")
        if name == "no_wall":
            assert np.isposinf(d).all()
        _same(s.get(0, "sa_nu_tilde").ravel(), sae.start_value(sae.SA_RATIO, mu, s.far_field()[0], d), f"{name}: the start value")
        s.set(0, "sa_nu_tilde", old)
        s.copy_old_variables(0)
        s.set(0, "sa_nu_tilde", new)
        s.compute_step_factor(0)
        _same(s.get(0, "step_factors").ravel(), sf, f"{name}: step factors")
        s.compute_fluxes(0)
        _same(s.get(0, "sa_gradient"), grad, f"{name}: sa_gradient")
        _same(s.get(0, "eddy_viscosity").ravel(), mut, f"{name}: eddy viscosity")
        _same(s.get(0, "viscous_stress"), S, f"{name}: S")
        _same(s.get(0, "fluxes"), f, f"{name}: F + V")
        s.time_step(0, 0)
        _same(s.get(0, "sa_nu_tilde").ravel(), out, f"{name}: nt after the stage")
        assert np.isfinite(out).all() and (out >= 0.0).all()
        if name == "isolated":
            assert not grad[[1, 4, 6], :4].any()
        em.close()
        s.close(); mesh.close()
    print("branches over the kernel-level cases:", total)
    assert all(total[k] >= 1 for k in sae.BRANCHES), total


# ---- runs ----
_emulated = {}


def _emulate(oracle, case, mu, mode, cfl, wall, lv, model, **composed):
    """(rms, variables, step factors, nt, mut) per level of K cycles: computed once per combination, shared and left unchanged."""
    key = (case, mu, mode, cfl, wall, lv, tuple(model), tuple(sorted(composed.items())))
    if key not in _emulated:
        em = sae.configured(oracle, case, mu, mode, cfl, wall, lv, model, **composed)
        rc, rms = em.cycles(K)
        assert rc == 0
        cov = range(em.visc_levels)
        _emulated[key] = (rms, [em.variables(l) for l in range(em.n)], [em.step_factors(l) for l in range(em.n)],
                          [em.nu_tilde(l) for l in cov], [em.eddy_viscosity(l) for l in cov])
        em.close()
    return _emulated[key]


def _check_run(s, rms, want, what):
    want_rms, want_v, want_sf, want_nt, want_mut = want
    _same(rms, want_rms, f"{what}: RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), want_v[l], f"{what}: variables, level {l}")
        _same(s.get(l, "step_factors"), want_sf[l], f"{what}: step factors, level {l}")
    for l in range(len(want_nt)):
        _same(s.get(l, "sa_nu_tilde").ravel(), want_nt[l], f"{what}: nu_tilde, level {l}")
        _same(s.get(l, "eddy_viscosity").ravel(), want_mut[l], f"{what}: eddy viscosity, level {l}")


@pytest.mark.parametrize("key,mu,mode,cfl,wall,lv,model", sae.gpu_runs())
def test_runs_equal_the_emulator(key, mu, mode, cfl, wall, lv, model, oracle, lattices):
    case = lattices.get(key, key)
    want = _emulate(oracle, case, mu, mode, cfl, wall, lv, model)
    mesh, s = _solver(case)
    _configure(s, mu, mode, cfl, wall, lv, model)
    rms = s.run_cycles(K)
    what = f"{key} mu={mu} wall={wall} levels={lv} {model}"
    print(what, "rms", rms, "want", want[0])
    _check_run(s, rms, want, what)
    s.close(); mesh.close()


@pytest.mark.parametrize("name,smoothing,jst_levels,fas,shape", sae.COMPOSED, ids=[c[0] for c in sae.COMPOSED])
def test_composition(name, smoothing, jst_levels, fas, shape, oracle, lattices):
    """Lattice A, (sutherland, SA), all levels, no-slip walls, with residual smoothing, JST, FAS, a W cycle, and all of them."""
    key, mu, mode, _, wall, lv, model = LATTICE_A
    cfl = 2.0 if smoothing[1] else 1.0
    composed = dict(smoothing=smoothing, jst_levels=jst_levels, fas=fas, shape=shape)
    want = _emulate(oracle, lattices[key], mu, mode, cfl, wall, lv, model, **composed)
    mesh, s = _solver(lattices[key])
    _configure(s, mu, mode, cfl, wall, lv, model, **composed)
    rms = s.run_cycles(K)
    _check_run(s, rms, want, name)
    s.close(); mesh.close()


def test_friction_loads():
    """Lattice A after K cycles, on every level: surface_loads(friction=True), wall_stress and wall_distribution are bitwise the
    emulator's on the state and the eddy viscosity read back (the wall-stress pass reads mut as under the caller's field)."""
    import mgcfd
    mg = fle.generated("A")
    levels = mgcfd.generated_to_levels(mg)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    mu = ve.CELL_RE_MU
    s.set(0, "variables", ve.start_state(s.nel(0), s.far_field()[:5]))
    s.set_viscous(mu, ve.PRANDTL, True, ve.VISCOUS_CFL, s.num_levels)
    s.set_viscosity_model(law="sutherland", eddy=sae.SA)
    s.run_cycles(K)
    m = vve.Model("sutherland", vve.far_field_t_ref(s.far_field()), eddy="field")
    for l in range(s.num_levels):
        v, e, mut = s.get(l, "variables"), s.get_edges(l, len(levels[l]["edges"])), s.get(l, "eddy_viscosity").ravel()
        assert mut.any()
        S = vve.node_stresses(v, e, levels[l], mu, ve.PRANDTL, m, mut)
        want12 = vve.surface_loads12(v, e, levels[l], s.far_field(), REF, S)
        want_ids, want_table = vve.distribution(v, e, levels[l], s.far_field(), S)
        _same(s.surface_loads(l, REF, friction=True), want12, f"level {l}: loads")
        ids, table = s.wall_distribution(l)
        assert np.array_equal(ids, want_ids)
        _same(table, want_table, f"level {l}: distribution")
        ids, sw = s.wall_stress(l)
        _same(sw, S[want_ids], f"level {l}: Sw")
    s.close()


def _device_copy(ptr, host, to_device):
    hip = ctypes.CDLL("libamdhip64.so")
    rc = hip.hipMemcpy(ctypes.c_void_p(ptr if to_device else host.ctypes.data), ctypes.c_void_p(host.ctypes.data if to_device else ptr),
                       ctypes.c_size_t(8 * host.size), ctypes.c_int(1 if to_device else 2))
    assert rc == 0


@pytest.mark.parametrize("through", ["set_array", "devptr"])
def test_restart(through, oracle, lattices):
    """K cycles, nt of every covered level written again (mgcfd_set_array, or through the device pointer with
    mgcfd_array_written), K more: the emulator's bits with the same writes, each of which forms mut again."""
    key, mu, mode, cfl, wall, lv, model = LATTICE_A
    em = sae.configured(oracle, lattices[key], mu, mode, cfl, wall, lv, model)
    mesh, s = _solver(lattices[key])
    _configure(s, mu, mode, cfl, wall, lv, model)
    rc, rms0 = em.cycles(K)
    assert rc == 0
    _same(s.run_cycles(K), rms0, "before the restart: RMS history")
    scale = 1.25                                              # (a write that changes something)
    for l in range(s.num_levels):
        nt = s.get(l, "sa_nu_tilde").ravel()
        _same(nt, em.nu_tilde(l), f"level {l}: nt before the restart")
        em.set_nu_tilde(l, scale * nt)
        if through == "set_array":
            s.set(l, "sa_nu_tilde", scale * nt)
        else:
            ptr, count = s.array_devptr(l, "sa_nu_tilde")
            dev = np.empty(count)
            _device_copy(ptr, dev, False)
            dev *= scale
            _device_copy(ptr, dev, True)
            s.array_written(l, "sa_nu_tilde")
        _same(s.get(l, "eddy_viscosity").ravel(), em.eddy_viscosity(l), f"level {l}: mut formed from the written nt")
    rc, rms1 = em.cycles(K)
    assert rc == 0
    _same(s.run_cycles(K), rms1, "after the restart: RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), em.variables(l), f"after the restart: level {l}")
        _same(s.get(l, "sa_nu_tilde").ravel(), em.nu_tilde(l), f"after the restart: nt, level {l}")
    em.close()
    s.close(); mesh.close()


def test_setters_in_either_order_and_the_free_stream(oracle, lattices):
    key, mu, mode, cfl, wall, lv, model = LATTICE_A
    want = _emulate(oracle, lattices[key], mu, mode, cfl, wall, lv, model)
    mesh, s = _solver(lattices[key])
    _configure(s, mu, mode, cfl, wall, lv, model, order=(1, 0))
    _check_run(s, s.run_cycles(K), want, "model first")
    # the free-stream ratio, and a reinitialising set_free_stream: the start value on every covered level
    em = sae.configured(oracle, lattices[key], mu, mode, cfl, wall, lv, model)
    assert s.sa_free_stream() == sae.SA_RATIO
    s.set_sa_free_stream(5.0)
    em.set_sa_free_stream(5.0)
    assert s.sa_free_stream() == 5.0
    s.set_free_stream(0.8, 2.0, reinitialise=True)
    em.set_far_field(s.far_field(), True)
    for l in range(s.num_levels):
        _same(s.get(l, "sa_nu_tilde").ravel(), em.nu_tilde(l), f"reinitialised: nt, level {l}")
        _same(s.get(l, "eddy_viscosity").ravel(), em.eddy_viscosity(l), f"reinitialised: mut, level {l}")
    rc, rms = em.cycles(K)
    assert rc == 0
    _same(s.run_cycles(K), rms, "after the new free stream: RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "sa_nu_tilde").ravel(), em.nu_tilde(l), f"after the new free stream: nt, level {l}")
    s.set_sa_free_stream(2.0, reinitialise=True)
    em.set_sa_free_stream(2.0, True)
    for l in range(s.num_levels):
        _same(s.get(l, "sa_nu_tilde").ravel(), em.nu_tilde(l), f"ratio 2: nt, level {l}")
    em.close()
    s.close(); mesh.close()


def test_refusals_and_device_resources():
    """MGCFD_ERR_ARG with nothing changed; the allocation count returns when the mode, or the viscous terms, go off."""
    import mgcfd
    mesh, s = _solver("m6_2lvl")
    s.run_cycles(1)
    s.compute_wall_distance()
    plain = mgcfd.live_device_resources()

    def refused(call, text=""):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1 and text in str(e.value), str(e.value)

    for ratio in (0.0, -3.0, float("nan"), float("inf")):
        refused(lambda: s.set_sa_free_stream(ratio), "ratio")
    assert s.sa_free_stream() == sae.SA_RATIO
    # the mode's value is 4; 3 stays an unknown eddy mode, as tests/test_gpu_variable_viscosity.py::test_refusals has it
    refused(lambda: s._c(s.lib.mgcfd_set_viscosity_model(s.handle, 0, 0.0, 0.4, 3, 0.17, 0.9)), "viscosity model")
    s._c(s.lib.mgcfd_set_viscosity_model(s.handle, 0, 0.0, 0.4, sae.EDDY_SA, 0.17, 0.9))
    assert s.viscosity_model()["eddy"] == sae.SA
    s.set_viscosity_model()
    refused(lambda: s.get(0, "sa_nu_tilde"), "SA_NU_TILDE")
    refused(lambda: s.bench_sa(0, "gradient", 1))
    s.set_viscous(1e-3, wall=True, levels=2)
    viscous_only = mgcfd.live_device_resources()
    s.set_viscosity_model(eddy=sae.SA)
    on = mgcfd.live_device_resources()
    # mut on two levels; nt on two levels; nt_old, the spare buffer and sa_gradient on level 0
    assert on["allocations"] == viscous_only["allocations"] + 2 * 2 + 2 + 3
    refused(s.release_wall_distance, "Spalart-Allmaras")
    refused(lambda: s.set_dual_time(0.1), "Spalart-Allmaras")
    assert s.dual_time()["dt"] == 0.0
    refused(lambda: s.set(0, "eddy_viscosity", np.zeros(s.nel(0))), "read-only")
    refused(lambda: s.set(0, "sa_gradient", np.zeros((s.nel(0), 5))), "read-only")
    refused(lambda: s.get(1, "sa_gradient"), "SA_GRADIENT")
    assert s.get(1, "sa_nu_tilde").shape[0] == s.nel(1) and s.get(0, "sa_gradient").shape == (s.nel(0), 5)
    assert s.bench_sa(0, "gradient", 2) > 0.0 and s.bench_sa(0, "transport", 2) > 0.0 and s.bench_sa(1, "restrict", 2) > 0.0
    refused(lambda: s.bench_sa(0, "restrict", 1))
    s.set_viscous(1e-3, wall=True, levels=1)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"] - 2 - 2 - 2, "level 1's S, g, wall list, mut, d2 and nt are gone"
    refused(lambda: s.get(1, "sa_nu_tilde"), "SA_NU_TILDE")
    s.set_viscous(1e-3, wall=True, levels=2)
    s.set_viscosity_model()
    now = mgcfd.live_device_resources()
    assert now["allocations"] == viscous_only["allocations"] and now["bytes"] == viscous_only["bytes"]
    s.set_viscosity_model(eddy=sae.SA)
    s.set_viscous(0.0, levels=0)
    now = mgcfd.live_device_resources()
    assert now["allocations"] == plain["allocations"] and now["bytes"] == plain["bytes"]
    assert s.viscosity_model()["eddy"] == sae.SA, "the model is kept while the terms are off"
    s.set_viscosity_model()
    # dual time first: the mode is refused
    s.set_dual_time(0.1)
    refused(lambda: s.set_viscosity_model(eddy=sae.SA), "dual time")
    assert s.viscosity_model()["eddy"] == "none"
    s.set_dual_time(0.0)
    # mid-sweep
    s.sweep_begin(0)
    s.sweep_stage(0, 0, partials=False)
    refused(lambda: s.set_viscosity_model(eddy=sae.SA), "sweep is under way")
    refused(lambda: s.set_sa_free_stream(2.0), "sweep is under way")
    assert s.viscosity_model()["eddy"] == "none" and s.sa_free_stream() == sae.SA_RATIO
    s.sweep_stage(0, 1, partials=False)
    s.sweep_stage(0, 2, partials=False)
    # a group member
    g = mgcfd.Group([s])
    refused(lambda: s.set_viscosity_model(eddy=sae.SA))
    assert s.viscosity_model()["eddy"] == "none"
    g.close()
    s.close(); mesh.close()
    # a covered level created without coordinates
    flat = mgcfd.Mesh("input.dat", fse.case_input("fvcorr_1lvl"), 1)
    levels = [dict(flat.level(l)) for l in range(flat.num_levels)]
    for lv in levels:
        lv["coords"] = None
    t = mgcfd.Solver.from_arrays(levels, flat.variant)
    t.set_viscous(1e-3, levels=1)
    refused(lambda: t.set_viscosity_model(eddy=sae.SA), "coordinates")
    assert t.viscosity_model()["eddy"] == "none"
    t.set_viscous(0.0, levels=0)
    t.set_viscosity_model(eddy=sae.SA)                               # (not effective yet: kept)
    refused(lambda: t.set_viscous(1e-3, levels=1), "coordinates")
    assert t.viscous()[4] == 0
    t.close()
    flat.close()
    # a partitioned solver
    from mgcfd.partition import partition_hierarchy, rcb_partition
    mesh = mgcfd.Mesh("input.dat", fse.case_input("m6_2lvl"), 1)
    levels = [mesh.level(l) for l in range(mesh.num_levels)]
    H = partition_hierarchy(levels, rcb_partition(np.asarray(levels[0]["coords"]).reshape(-1, 3), 2))
    lv, owned, keys = H[0].solver_args()
    t = mgcfd.Solver.from_arrays(lv, mesh.variant, n_owned=owned, order_keys=keys)
    refused(lambda: t.set_viscosity_model(eddy=sae.SA))
    assert t.viscosity_model()["eddy"] == "none"
    t.close()
    mesh.close()


def test_polar(oracle):
    """polar(..., viscosity_model={"eddy": "spalart-allmaras"}) is set_free_stream + run_cycles with the model on: the emulator's
    RMS history of the first angle."""
    import mgcfd
    case = fse.POLAR_CASE
    mesh, s = _solver(case)
    rows = s.polar(fse.POLAR_ALPHAS[:1], K, mach=fse.POLAR_MACH, warm_start=False, viscous={"mu": ve.DRIVER_MU, "wall": True, "levels": 2},
                   viscosity_model={"eddy": sae.SA})
    assert s.viscosity_model()["eddy"] == sae.SA and s.wall_distance_levels() == 2 and len(rows) == 1
    em = sae.SaOracle(oracle, case, mu=ve.DRIVER_MU, wall=1, viscous_levels="all")
    em.set_viscosity_model(eddy=sae.SA)
    em.set_far_field(s.far_field(), True)
    rc, rms = em.cycles(K)
    assert rc == 0
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), em.variables(l), f"polar: level {l}")
        _same(s.get(l, "sa_nu_tilde").ravel(), em.nu_tilde(l), f"polar: nt, level {l}")
    em.close()
    s.close(); mesh.close()


def test_fast_mode(oracle, lattices):
    """exact = 0: the model's kernels are never contracted, the flux, stress and update kernels are; against the exact-mode run
    (the emulator's bits) the state is within tests/test_gpu_viscous.py::test_fast_mode's bounds — 1e-10 of the largest value per
    level, RMS rtol 1e-9 — and nt within the same bound of its largest value.  Measured on an MI355X: the state differs by
    6.4e-16 of the largest value, nt by 1.9e-16, the RMS history by 1.1e-16 relative, so the model needs no wider bound."""
    key, mu, mode, cfl, wall, lv, model = LATTICE_A
    want_rms, want_v, _, want_nt, _ = _emulate(oracle, lattices[key], mu, mode, cfl, wall, lv, model)
    mesh, s = _solver(lattices[key], exact=0)
    _configure(s, mu, mode, cfl, wall, lv, model)
    rms = s.run_cycles(K)
    print("fast mode: RMS relative", np.abs(rms / want_rms - 1.0).max())
    for l in range(s.num_levels):
        rel = np.abs(s.get(l, "variables") - want_v[l]).max() / max(np.abs(want_v[l]).max(), 1e-300)
        rel_nt = np.abs(s.get(l, "sa_nu_tilde").ravel() - want_nt[l]).max() / np.abs(want_nt[l]).max()
        print("fast mode: level", l, "rel", rel, "nt rel", rel_nt)
    assert np.allclose(rms, want_rms, rtol=RMS_FAST, atol=0)
    for l in range(s.num_levels):
        rel = np.abs(s.get(l, "variables") - want_v[l]).max() / max(np.abs(want_v[l]).max(), 1e-300)
        rel_nt = np.abs(s.get(l, "sa_nu_tilde").ravel() - want_nt[l]).max() / np.abs(want_nt[l]).max()
        assert rel <= REL_RUN and rel_nt <= REL_RUN, f"level {l}: {rel:.3e} {rel_nt:.3e}"
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


def test_driver_flag(oracle, tmp_path):
    """--spalart-allmaras, --spalart-allmaras=3 and the config key on m6_2lvl: the dump is the %.17e rendering of the emulator's
    state; another ratio gives another state; without a viscosity, with --smagorinsky, with --gpus 2 and with
    --physical-time-step: exit status 1 and no dump."""
    case = "m6_2lvl"
    dup = fse.case_duplicate(case)
    name = f"variables.size={dup}x.cycles={K}.level=0"
    em = sae.SaOracle(oracle, case, mu=ve.DRIVER_MU, wall=1, viscous_levels="all")
    em.set_viscosity_model(law="constant", eddy=sae.SA)
    rc, want_rms = em.cycles(K)
    assert rc == 0
    want = fse.render_variables(em.variables(0)).encode()
    em.close()
    base = ["--output-variables", "--viscosity", repr(ve.DRIVER_MU), "--no-slip", "--viscous-levels", "8"]
    laminar = _run_driver(tmp_path / "laminar", case, base, K)
    assert (tmp_path / "laminar" / "out" / name).read_bytes() != want
    conf = tmp_path / "run.conf"
    conf.write_text(f"viscosity = {ve.DRIVER_MU!r}\nno_slip = Y\nviscous_levels = 8\nspalart_allmaras = Y\n")
    for tag, extra in (("short", base + ["--spalart-allmaras"]), ("equals", base + ["--spalart-allmaras=3"]),
                       ("conf", ["--output-variables", "-c", str(conf)])):
        d = tmp_path / tag
        r = _run_driver(d, case, extra, K)
        assert (d / "out" / name).read_bytes() == want, tag
        lines = [l for l in r.stdout.splitlines() if "(RMS = " in l]
        assert lines == [f"MG cycle {i + 1} / {K}" + " (RMS = %.3e)" % want_rms[i] for i in range(K)]
    _run_driver(tmp_path / "ratio", case, base + ["--spalart-allmaras=30"], K)
    assert (tmp_path / "ratio" / "out" / name).read_bytes() != want
    for tag, bad in (("no_viscosity", ["--output-variables", "--spalart-allmaras"]),
                     ("smagorinsky", base + ["--spalart-allmaras", "--smagorinsky"]),
                     ("gpus", base + ["--spalart-allmaras", "--gpus", "2", "--gpus-share-device"]),
                     ("dual", base + ["--spalart-allmaras", "--physical-time-step", "0.1"]),
                     ("bad_ratio", base + ["--spalart-allmaras=-1"])):
        _run_driver(tmp_path / tag, case, bad, K, ok=False)
        assert not [n for n in os.listdir(tmp_path / tag / "out") if n.startswith("variables")], tag


def test_defaults_reproduce_the_golden_output(tmp_path):
    """With the flag absent the golden variables.level0.txt byte for byte, and so the Python API with the model selected while
    the viscous terms are off (no effect, nothing allocated)."""
    import mgcfd
    case = "m6_2lvl"
    meta = dict(l.strip().split(" = ") for l in open(os.path.join(fse.GOLDEN, case, "case.txt")))
    cycles, dup = int(meta["cycles"]), fse.case_duplicate(case)
    golden = open(os.path.join(fse.GOLDEN, case, "variables.level0.txt"), "rb").read()
    _run_driver(tmp_path / "plain", case, ["--output-variables"], cycles)
    assert (tmp_path / "plain" / "out" / f"variables.size={dup}x.cycles={cycles}.level=0").read_bytes() == golden
    mesh, s = _solver(case)
    before = mgcfd.live_device_resources()["allocations"]
    s.set_viscosity_model(eddy=sae.SA)
    s.set_sa_free_stream(4.0)
    assert mgcfd.live_device_resources()["allocations"] == before and s.wall_distance_levels() == 0
    s.run_cycles(cycles)
    assert fse.render_variables(s.get(0, "variables")).encode() == golden
    s.close(); mesh.close()
