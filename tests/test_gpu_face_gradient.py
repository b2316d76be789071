"""GPU tests of the corrected face gradient (mgcfd_set_face_gradient) against the numpy emulator (tests/face_gradient_emulator.py)
bit for bit: the kernels on the shapes at which their gathers can go wrong (and a level with two coincident nodes); the runs
(state and step factors of every level, RMS history); the runs composed with every other option of the viscous path; dual time
stepping; the fast mode; the setters in either order, the mode switched on, off and on, a solver that never calls the setter; the
refusals and the device allocations; polar; the driver's flag.  tests/test_host_face_gradient.py checks the emulator itself and
asserts on the CPU that every run here stays valid."""
import os
import subprocess

import numpy as np
import pytest

import face_gradient_emulator as fge
import fas_emulator as fe
import free_stream_emulator as fse
import sa_emulator as sae
import viscous_emulator as ve
import wall_heat_emulator as whe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
K = fge.GPU_CYCLES
REL_RUN = 1e-10          # tests/test_gpu_viscous.py::test_fast_mode's tolerances
RMS_FAST = 1e-9
CFL_V = fge.VISCOUS_CFL_CORRECTED


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(got - want).max():.3e}"


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("face_gradient_lattices")
    return {name: fe.write_lattice(name, d) for name in fe.LATTICES}


def _solver(case, exact=1):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    s.set_option("exact", exact)
    return mesh, s


def _levels(s, lv):
    return s.num_levels if lv == "all" else lv


def _configure(s, mu, wall, lv, smoothing=(0.0, 0), jst_levels=0, fas=False, shape="V", model=None, damping=False, thermal=None,
               dual=False, order=(0, 1), mode="corrected", cfl_v=CFL_V, step=fge.RUN_STEP):
    """The solver as fge.configured sets the emulator up."""
    s.set_time_step(step[0], 2.0 if smoothing[1] else step[1])
    if smoothing[1]:
        s.set_residual_smoothing(*smoothing)
    if jst_levels:
        s.set_jst(levels=jst_levels)
    if fas:
        s.set_fas(True)
    if shape != "V":
        s.set_cycle(shape)
    s.set(0, "variables", ve.start_state(s.nel(0), s.far_field()[:5]))
    setters = (lambda: s.set_viscous(mu, ve.PRANDTL, bool(wall), cfl_v, _levels(s, lv)), lambda: s.set_face_gradient(mode))
    for k in order:
        setters[k]()
    assert s.face_gradient() == mode
    if thermal is not None:
        s.set_wall_temperature(thermal[0], whe.setting_value(s.far_field(), *thermal))
    if damping:
        s.set_wall_damping(True)
    if model is not None:
        s.set_viscosity_model(law=model[0], eddy=model[1])
    if dual:
        s.set_dual_time(fge.DUAL_DT)


def _run(s, dual=False):
    """The RMS history of the run fge.run emulates."""
    return s.advance(fge.DUAL_STEPS, fge.DUAL_CYCLES) if dual else s.run_cycles(K)


# ---- kernel level ----
def _single_level_case(level, directory):
    from mgcfd import meshgen
    mg = meshgen.MultigridMesh(mesh_name="fvcorr")
    mg.levels.append(level)
    os.makedirs(os.path.join(directory, "input"))
    meshgen.write_input(mg, os.path.join(directory, "input"))
    with open(os.path.join(directory, "case.txt"), "w") as f:
        f.write("duplicate = 1\n")
    return str(directory)


def _kernel_cases(lattices, tmp_path):
    """(name, case directory, perturbation amplitude, CFL, mu): tests/test_gpu_sa.py's six — lattices A and B (a last partial tile,
    more than one tile), the generated tetrahedral level (the overflow list and the TAIL instantiation), the hub (a row longer than
    a tile), nodes without an internal edge, a level without walls — and lattice A's level 0 with one node moved onto its
    neighbour along the first internal edge (L == 0.0)."""
    from mgcfd import meshgen
    from test_gpu_variable_viscosity import _isolated_level
    cases = [("lattice_A", lattices["A"], 0.01, 1.0, ve.CELL_RE_MU), ("lattice_B", lattices["B"], 0.01, 1.0, ve.CELL_RE_MU)]
    merged = meshgen.make_multigrid(fe.LATTICES["A"], "fvcorr", **fe.LATTICE_ARGS).levels[0]
    edges, n_int, _, _ = meshgen.to_edge_arrays(merged, meshgen.MESH_CODES["fvcorr"])
    merged.coords[int(edges["b"][0])] = merged.coords[int(edges["a"][0])]
    for name, level, amplitude, cfl, mu in (("tet", meshgen.make_tet_level(30000, seed=0), 0.002, 0.02, 1e-3),
                                            ("hub", meshgen.make_hub_level(600, scale=1e-4, seed=5), 0.002, 0.02, 1e-9),
                                            ("isolated", _isolated_level(), 0.002, 0.02, 1e-9),
                                            ("no_wall", meshgen.make_box_level(9, seed=2, jitter=0.2), 0.01, 1.0, 0.05),
                                            ("coincident", merged, 0.01, 1.0, ve.CELL_RE_MU)):
        cases.append((name, _single_level_case(level, tmp_path / name), amplitude, cfl, mu))
    return cases


def test_kernel_level(oracle, lattices, tmp_path):
    """tests/test_gpu_sa.py's kernel-level case (a perturbed W, random nt_old and nt, Sutherland with SA, no-slip walls) under the
    corrected gradient: viscous_gradient, S (the averaged run's bits as well), F + V + Vc and the new nt bitwise the emulator's."""
    import mgcfd
    from conftest import perturbed_state
    skipped = 0
    for name, case, amplitude, cfl, mu in _kernel_cases(lattices, tmp_path):
        mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
        levels = [dict(mesh.level(l)) for l in range(mesh.num_levels)]
        em = fge.FaceGradientOracle(oracle, case, "local", cfl)
        if levels[0].get("coords") is None or len(levels[0]["coords"]) == 0:
            levels[0]["coords"] = em.X[0].copy()      # (the reader loads a single undamped level without coordinates: the emulator's)
        s = mgcfd.Solver.from_arrays(levels, mesh.variant)
        t = s.tiling(0)
        print(name, t)
        if name == "tet":
            assert t["tiles"] > 1 and t["overflow_refs"] > 0 and t["list_entries"] > 0
        elif name == "hub":
            assert t["list_entries"] > 0
        start = perturbed_state(s.nel(0), s.far_field()[:5], seed=7, amplitude=amplitude)
        v = em._var(0)
        v[:] = start
        em.set_viscous(mu, ve.PRANDTL, 1, CFL_V, 1)
        em.set_viscosity_model(law="sutherland", eddy=sae.SA)
        old, new = sae.random_nt(mu, em.ff17[0], len(v), sae.NT_SEED + 1), sae.random_nt(mu, em.ff17[0], len(v))
        em.set_nu_tilde(0, old)
        em.copy_old()
        em.set_nu_tilde(0, new)
        sf = em.final_step_factors(0)
        em.stage_fluxes(0)
        S_averaged = em.last_S[0].copy()
        em.set_face_gradient("corrected")
        grad, mut, S, f, out, masks = em.kernel_level(0, sf)
        _same(S, S_averaged, f"{name}: the emulator's S under either gradient")
        terms_ok = fge.edge_geometry(em.X[0], em.vto[0], em.vfrm[0])[1] != 0.0
        if name == "coincident":
            assert (~terms_ok).sum() == 2
        else:
            skipped += int((~terms_ok).sum())
        s.set_time_step("local", cfl)
        s.set(0, "variables", start)
        s.set_viscous(mu, ve.PRANDTL, True, CFL_V, 1)
        s.set_viscosity_model(law="sutherland", eddy=sae.SA)
        s.set_face_gradient("corrected")
        s.set(0, "sa_nu_tilde", old)
        s.copy_old_variables(0)
        s.set(0, "sa_nu_tilde", new)
        s.compute_step_factor(0)
        _same(s.get(0, "step_factors").ravel(), sf, f"{name}: step factors")
        s.compute_fluxes(0)
        _same(s.get(0, "viscous_gradient"), em.viscous_gradient(0), f"{name}: viscous_gradient")
        _same(s.get(0, "sa_gradient"), grad, f"{name}: sa_gradient")
        _same(s.get(0, "eddy_viscosity").ravel(), mut, f"{name}: eddy viscosity")
        _same(s.get(0, "viscous_stress"), S, f"{name}: S")
        _same(s.get(0, "fluxes"), f, f"{name}: F + V + Vc")
        assert np.isfinite(f).all() and np.abs(em.last_sums[0]).max() > 0.0
        s.time_step(0, 0)
        _same(s.get(0, "sa_nu_tilde").ravel(), out, f"{name}: nt after the stage")
        assert np.isfinite(out).all() and (out >= 0.0).all()
        with pytest.raises(mgcfd.MgcfdError):
            s.set(0, "viscous_gradient", em.viscous_gradient(0))
        em.close()
        s.close(); mesh.close()
    assert skipped == 0


# ---- runs ----
_emulated = {}


def _emulate(oracle, case, mu, wall, lv, **kw):
    """(rms, variables, step factors, nt and mut under SA, P and W0 under FAS) of the run: computed once per combination, shared
    and left unchanged."""
    key = (case, mu, wall, lv, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _emulated:
        em = fge.configured(oracle, case, mu, wall, lv, **kw)
        rc, rms = fge.run(em, kw.get("dual", False))
        assert rc == 0
        extra = {}
        if kw.get("fas"):
            extra = {"P": [None] + [em.P[l].copy() for l in range(1, em.n)], "W0": [None] + [em.W0[l].copy() for l in range(1, em.n)]}
        if em.sa:
            extra.update({"nt": [em.nu_tilde(l) for l in range(em.visc_levels)], "mut": [em.eddy_viscosity(l) for l in range(em.visc_levels)]})
        _emulated[key] = (rms, [em.variables(l) for l in range(em.n)], [em.step_factors(l) for l in range(em.n)], extra)
        em.close()
    return _emulated[key]


def _check_run(s, rms, want, what):
    want_rms, want_v, want_sf, extra = want
    _same(rms, want_rms, f"{what}: RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), want_v[l], f"{what}: variables, level {l}")
        _same(s.get(l, "step_factors"), want_sf[l], f"{what}: step factors, level {l}")
    for l, nt in enumerate(extra.get("nt", [])):
        _same(s.get(l, "sa_nu_tilde").ravel(), nt, f"{what}: nu_tilde, level {l}")
        _same(s.get(l, "eddy_viscosity").ravel(), extra["mut"][l], f"{what}: eddy viscosity, level {l}")
    for l in range(1, len(extra.get("P", []))):
        _same(s.get(l, "fas_forcing"), extra["P"][l], f"{what}: P, level {l}")
        _same(s.get(l, "fas_start"), extra["W0"][l], f"{what}: W0, level {l}")


@pytest.mark.parametrize("key,wall,lv", fge.gpu_runs())
def test_runs_equal_the_emulator(key, wall, lv, oracle, lattices):
    case, mu = lattices.get(key, key), fge.RUN_MU[key]
    want = _emulate(oracle, case, mu, wall, lv)
    mesh, s = _solver(case)
    _configure(s, mu, wall, lv)
    rms = s.run_cycles(K)
    print(key, wall, lv, "rms", rms, "want", want[0])
    _check_run(s, rms, want, f"{key} wall={wall} levels={lv}")
    s.close(); mesh.close()


@pytest.mark.parametrize("name,kw,key,wall,lv", fge.composed_runs(), ids=[f"{c[0]}-{c[2]}-wall{c[3]}-{c[4]}" for c in fge.composed_runs()])
def test_composition(name, kw, key, wall, lv, oracle, lattices):
    """Every plain run — A, B and tet_2lvl, wall 0 and 1, one and all levels covered — composed in turn with residual smoothing,
    JST, FAS (P and W0 too), a W cycle, mgcfd_advance (BDF2), Sutherland, the damped Smagorinsky model, SA (nt, mut), the
    isothermal and the heat-flux wall, and with the two sets of all that combine (fge.COMPOSED)."""
    case, mu = lattices.get(key, key), fge.RUN_MU[key]
    want = _emulate(oracle, case, mu, wall, lv, **kw)
    mesh, s = _solver(case)
    _configure(s, mu, wall, lv, **kw)
    rms = _run(s, kw.get("dual", False))
    _check_run(s, rms, want, f"{name} {key} wall={wall} levels={lv}")
    s.close(); mesh.close()


@pytest.mark.parametrize("key", fge.RUN_CASES)
def test_fast_mode(key, oracle, lattices):
    """MGCFD_OPT_EXACT = 0 (the flux, stress and viscous-flux launches may contract; the new launches never do) against the exact
    run inside tests/test_gpu_viscous.py::test_fast_mode's bounds: 1e-10 of the largest value per level, RMS rtol 1e-9.
    The measured differences are printed."""
    case, mu = lattices.get(key, key), fge.RUN_MU[key]
    want_rms, want_v, _, _ = _emulate(oracle, case, mu, 1, "all")
    mesh, s = _solver(case, exact=0)
    _configure(s, mu, 1, "all")
    rms = s.run_cycles(K)
    print(key, "RMS relative", np.abs(rms / want_rms - 1.0).max())
    assert np.allclose(rms, want_rms, rtol=RMS_FAST, atol=0)
    for l in range(s.num_levels):
        rel = np.abs(s.get(l, "variables") - want_v[l]).max() / max(np.abs(want_v[l]).max(), 1e-300)
        print(key, "level", l, "rel", rel)
        assert rel <= REL_RUN, f"{key} level {l}: {rel:.3e}"
    s.close(); mesh.close()


# ---- the setting ----
def test_setters_in_either_order_and_on_off_on(oracle, lattices):
    """The mode before the viscous terms; then K cycles corrected, K averaged, K corrected within one run: the emulator driven the
    same way, bit for bit; the getter follows; the mode survives the terms going off."""
    mu = fge.RUN_MU["A"]
    want = _emulate(oracle, lattices["A"], mu, 1, "all")
    mesh, s = _solver(lattices["A"])
    _configure(s, mu, 1, "all", order=(1, 0))
    _check_run(s, s.run_cycles(K), want, "mode first")
    em = fge.configured(oracle, lattices["A"], mu, 1, "all", order=(1, 0))
    assert em.cycles(K)[0] == 0
    for mode in ("averaged", "corrected"):
        em.set_face_gradient(mode)
        s.set_face_gradient(mode)
        assert s.face_gradient() == mode
        rc, rms = em.cycles(K)
        assert rc == 0
        _same(s.run_cycles(K), rms, f"then {mode}: RMS history")
        for l in range(s.num_levels):
            _same(s.get(l, "variables"), em.variables(l), f"then {mode}: variables, level {l}")
    s.set_viscous(0.0, levels=0)
    assert s.face_gradient() == "corrected"
    em.close()
    s.close(); mesh.close()


def test_a_solver_that_never_calls_the_setter_keeps_its_bits(oracle, lattices):
    """tests/test_gpu_viscous.py's run on lattice A: a solver that never calls the setter, one that sets "averaged", and one that
    went to "corrected" and back before the run all give the viscous emulator's bits."""
    em = ve.configured(oracle, lattices["A"], ve.CELL_RE_MU, "local", 1.0, 1, "all")
    rc, want_rms = em.cycles(K)
    assert rc == 0
    for touched in (0, 1, 2):
        mesh, s = _solver(lattices["A"])
        s.set_time_step("local", 1.0)
        s.set(0, "variables", ve.start_state(s.nel(0), s.far_field()[:5]))
        s.set_viscous(ve.CELL_RE_MU, ve.PRANDTL, True, ve.VISCOUS_CFL, s.num_levels)
        if touched == 2:
            s.set_face_gradient("corrected")
        if touched:
            s.set_face_gradient("averaged")
        assert s.face_gradient() == "averaged"
        _same(s.run_cycles(K), want_rms, f"touched={touched}: RMS history")
        for l in range(s.num_levels):
            _same(s.get(l, "variables"), em.variables(l), f"touched={touched}: variables, level {l}")
        s.close(); mesh.close()
    em.close()


def test_refusals_and_device_resources(lattices):
    """An unknown mode, a level without coordinates (from either setter), mid-sweep, a group member and a partitioned solver: error
    code 1 and nothing changed; G and the coordinates are held exactly while the mode is in effect on a level."""
    import mgcfd
    base = mgcfd.live_device_resources()
    mu = fge.RUN_MU["A"]
    mesh, s = _solver(lattices["A"])

    def refused(call, text=""):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1 and text in str(e.value), str(e.value)

    for mode in (2, -1, 7):
        refused(lambda: s.set_face_gradient(mode), "face gradient")
    assert s.face_gradient() == "averaged"
    s.set_viscous(mu, ve.PRANDTL, True, CFL_V, 2)
    refused(lambda: s.get(0, "viscous_gradient"), "VISCOUS_GRADIENT")
    on = mgcfd.live_device_resources()
    s.set_face_gradient("corrected")
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"] + 4, "G and the coordinates of the two covered levels"
    s.set_face_gradient("corrected")
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"] + 4, "allocated once"
    refused(lambda: s.get(2, "viscous_gradient"), "VISCOUS_GRADIENT")
    assert s.get(1, "viscous_gradient").shape == (s.nel(1), 12)
    s.set_viscous(mu, ve.PRANDTL, True, CFL_V, 3)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"] + 3 + 6, "a further level: its three arrays, G and x"
    s.set_viscous(mu, ve.PRANDTL, True, CFL_V, 2)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"] + 4
    s.set_face_gradient("averaged")
    off = mgcfd.live_device_resources()
    assert off["allocations"] == on["allocations"] and off["bytes"] == on["bytes"], "the mode off releases"
    s.set_viscous(0.0, levels=0)
    terms_off = mgcfd.live_device_resources()
    s.set_viscous(mu, ve.PRANDTL, True, CFL_V, 2)
    s.set_face_gradient("corrected")
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"] + 4
    s.set_viscous(0.0, levels=0)
    assert s.face_gradient() == "corrected", "kept while the terms are off"
    off = mgcfd.live_device_resources()
    assert off["allocations"] == terms_off["allocations"] and off["bytes"] == terms_off["bytes"], "the terms off release G and x as well"
    s.set_viscous(mu, ve.PRANDTL, True, CFL_V, 2)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"] + 4
    # the diagnostics run and leave the state alone
    before = s.get(0, "variables")
    assert all(s.bench_face_gradient(0, kind, 3) > 0.0 for kind in ("nodes", "correction"))
    _same(s.get(0, "variables"), before, "the state after the diagnostics")
    s.zero_fluxes(0)
    for kind, level in ((2, 0), (-1, 0), (0, 2)):
        refused(lambda: s.bench_face_gradient(level, kind, 1))
    # mid-sweep (the split sweep runs with the terms off)
    s.set_viscous(0.0, levels=0)
    s.set_face_gradient("averaged")
    s.sweep_begin(0)
    s.sweep_stage(0, 0, partials=False)
    refused(lambda: s.set_face_gradient("corrected"), "sweep is under way")
    assert s.face_gradient() == "averaged"
    s.sweep_stage(0, 1, partials=False)
    s.sweep_stage(0, 2, partials=False)
    # a group member
    g = mgcfd.Group([s])
    refused(lambda: s.set_face_gradient("corrected"))
    assert s.face_gradient() == "averaged"
    g.close()
    s.close(); mesh.close()
    assert mgcfd.live_device_resources()["allocations"] == base["allocations"]
    # a level created without coordinates: whichever setter would make the mode effective refuses
    flat = mgcfd.Mesh("input.dat", fse.case_input("fvcorr_1lvl"), 1)
    lvs = [dict(flat.level(l)) for l in range(flat.num_levels)]
    for lv in lvs:
        lv["coords"] = None
    t = mgcfd.Solver.from_arrays(lvs, flat.variant)
    t.set_viscous(1e-3, levels=1)
    refused(lambda: t.set_face_gradient("corrected"), "without coordinates")
    assert t.face_gradient() == "averaged"
    t.set_viscous(0.0, levels=0)
    t.set_face_gradient("corrected")                                   # (not effective yet: kept)
    refused(lambda: t.set_viscous(1e-3, levels=1), "without coordinates")
    assert t.viscous()[4] == 0 and t.face_gradient() == "corrected"
    t.close()
    flat.close()
    # a partitioned solver
    from mgcfd.partition import partition_hierarchy, rcb_partition
    mesh = mgcfd.Mesh("input.dat", fse.case_input("m6_2lvl"), 1)
    lvs = [mesh.level(l) for l in range(mesh.num_levels)]
    H = partition_hierarchy(lvs, rcb_partition(np.asarray(lvs[0]["coords"]).reshape(-1, 3), 2))
    lv, owned, keys = H[0].solver_args()
    t = mgcfd.Solver.from_arrays(lv, mesh.variant, n_owned=owned, order_keys=keys)
    refused(lambda: t.set_face_gradient("corrected"), "partitioned")
    t.set_face_gradient("averaged")
    assert t.face_gradient() == "averaged"
    t.close()
    mesh.close()
    assert mgcfd.live_device_resources()["allocations"] == base["allocations"]


def test_polar_with_the_corrected_gradient(oracle):
    """Solver.polar(face_gradient="corrected") = set_face_gradient once, then the viscous terms at MGCFD_VISCOUS_CFL_CORRECTED (no
    cfl_v named), then the polar."""
    case, alphas, mach = fse.POLAR_CASE, fse.POLAR_ALPHAS, fse.POLAR_MACH
    mesh, s = _solver(case)
    pol = s.polar(alphas, K, mach=mach, viscous={"mu": ve.DRIVER_MU, "wall": True, "levels": 2}, face_gradient="corrected")
    assert s.face_gradient() == "corrected" and s.viscous()[3] == CFL_V
    em = fge.FaceGradientOracle(oracle, case, mu=ve.DRIVER_MU, wall=1, cfl_v=CFL_V, viscous_levels=2)
    em.set_face_gradient("corrected")
    for k, (al, p) in enumerate(zip(alphas, pol)):
        em.set_far_field(fse.free_stream_constants(mach, al), reinitialise=(k == 0))
        rc, rms = em.cycles(K)
        assert rc == 0
        _same(p["rms"], rms, f"polar, angle {al}: RMS history")
    _same(s.get(0, "variables"), em.variables(0), "the polar's last state")
    em.close()
    s.close(); mesh.close()


# ---- the drop-in binary ----
def _run_driver(tmp, case, extra, cycles, ok=True):
    os.makedirs(tmp / "out", exist_ok=True)
    cmd = [EXE, "-i", "input.dat", "-d", fse.case_input(case), "-o", "out/", "-g", str(cycles), "-m", str(fse.case_duplicate(case))] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tmp)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


def test_driver_flag(oracle, tmp_path):
    """--face-gradient corrected (and the config key): the dump is the %.17e rendering of the emulator's state at the corrected
    mode's default cfl_v, and at a --viscous-cfl given beside it; --face-gradient averaged and no flag write the viscous run's
    bytes; the flag errors exit with status 1 right after parsing (no file written)."""
    case = "m6_2lvl"
    dup = fse.case_duplicate(case)
    name = f"variables.size={dup}x.cycles={K}.level=0"
    viscous = [f"--viscosity={ve.DRIVER_MU!r}", "--no-slip", "--viscous-levels", "8", "--output-variables"]

    def emulated(mode, cfl_v):
        em = fge.FaceGradientOracle(oracle, case, mu=ve.DRIVER_MU, wall=1, cfl_v=cfl_v, viscous_levels="all")
        em.set_face_gradient(mode)
        rc, _ = em.cycles(K)
        assert rc == 0
        out = fse.render_variables(em.variables(0)).encode()
        em.close()
        return out

    corrected, averaged = emulated("corrected", CFL_V), emulated("averaged", ve.VISCOUS_CFL)
    assert corrected != averaged
    conf = tmp_path / "run.conf"
    conf.write_text(f"viscosity = {ve.DRIVER_MU!r}\nno_slip = Y\nviscous_levels = 8\nface_gradient = corrected\n")
    for tag, extra, want in (("flag", viscous + ["--face-gradient", "corrected"], corrected),
                             ("equals", viscous + ["--face-gradient=corrected"], corrected),
                             ("conf", ["-c", str(conf), "--output-variables"], corrected),
                             ("cfl", viscous + ["--face-gradient", "corrected", "--viscous-cfl", "0.1"], emulated("corrected", 0.1)),
                             ("averaged", viscous + ["--face-gradient", "averaged"], averaged),
                             ("plain", viscous, averaged)):
        _run_driver(tmp_path / tag, case, extra, K)
        assert (tmp_path / tag / "out" / name).read_bytes() == want, tag
    for bad in (["--face-gradient", "corrected"], ["--face-gradient", "averaged"], viscous + ["--face-gradient", "compact"],
                [f"--viscosity={ve.DRIVER_MU!r}", "--viscous-levels", "0", "--face-gradient", "corrected"],
                viscous + ["--face-gradient", "corrected", "--gpus", "2", "--gpus-share-device"]):
        r = _run_driver(tmp_path / "bad", case, bad, K, ok=False)
        assert r.returncode == 1 and "ERROR" in r.stderr, bad
        assert not os.listdir(tmp_path / "bad" / "out"), bad
