"""GPU tests of the viscous surface loads (mgcfd_surface_loads_viscous, mgcfd_run_cycles_loads_viscous,
mgcfd_advance_loads_viscous, mgcfd_wall_distribution, euler3d_gpu_double --loads-friction / --output-surface): everything bit
for bit against the numpy emulator of the definition (tests/friction_loads_emulator.py) evaluated on the state read back from
the GPU.  The meshes and viscosities are fle.GPU_MU's (tests/test_host_friction_loads.py counts their walls and checks on the
CPU that the runs stay valid): lattice A of fas_emulator on levels 0, 1 and 2 (54, 6 and 6 solid-wall edges; nodes with 1 and
3 of them), the fvcorr 17^3 box (414 edges: two chunks and stage B; 278 wall nodes with 1, 2 and 3 edges), the hull-wall 9^3
box (81 edges, a flat wall) and the goldens mixed_2lvl and tet_2lvl (rows of non-uniform degree)."""
import os
import subprocess

import numpy as np
import pytest

import dual_time_emulator as dte
import fas_emulator as fe
import free_stream_emulator as fse
import friction_loads_emulator as fle
import viscous_emulator as ve

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
REF = (0.25, -0.125, 0.375)
K = fe.GPU_CYCLES
KEYS = list(fle.GPU_MU)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(got - want).max():.3e}\n{got}\n{want}"


_generated = {}


def _open(key, **options):
    """(levels, solver): the level dicts of the emulator and a fresh solver."""
    import mgcfd
    if key in fle.GPU_GENERATED:
        if key not in _generated:
            mg = fle.generated(key)
            _generated[key] = (mgcfd.generated_to_levels(mg), mg.mesh_variant)
        levels, variant = _generated[key]
        s = mgcfd.Solver.from_arrays(levels, variant)
    else:
        mesh = mgcfd.Mesh("input.dat", fse.case_input(key), fse.case_duplicate(key))
        levels = [mesh.level(l) for l in range(mesh.num_levels)]
        s = mgcfd.Solver.from_mesh(mesh)
        mesh.close()                            # (mgcfd_create_from_mesh copies what it needs)
    for name, v in options.items():
        s.set_option(name, v)
    return levels, s


def _start(s, key, wall, levels="all"):
    """The start of every run: the perturbed state on level 0, then the terms on at the case's viscosity."""
    s.set(0, "variables", ve.start_state(s.nel(0), s.far_field()[:5]))
    s.set_viscous(fle.GPU_MU[key], ve.PRANDTL, bool(wall), ve.VISCOUS_CFL, s.num_levels if levels == "all" else levels)


def _edges(s, levels, l):
    return s.get_edges(l, len(levels[l]["edges"]))


def _want(s, levels, l, key, viscous=True, ref=REF):
    """(out12, (ids, table)) of the emulator on level l's state as the GPU holds it."""
    v, e, visc = s.get(l, "variables"), _edges(s, levels, l), (fle.GPU_MU[key], ve.PRANDTL) if viscous else None
    return fle.surface_loads12(v, e, levels[l], s.far_field(), ref, visc), fle.distribution(v, e, levels[l], s.far_field(), visc)


@pytest.mark.parametrize("wall", ve.GPU_WALLS)
@pytest.mark.parametrize("key", KEYS)
def test_loads_stresses_and_distribution_equal_the_emulator(key, wall):
    """After K cycles with the terms on every level, on every level: the twelve loads and the distribution are the emulator's
    bits; the pressure six are mgcfd_surface_loads'; Sw is the emulator's and, after mgcfd_compute_fluxes on the same state, the
    wall rows of MGCFD_ARR_VISCOUS_STRESS; S is what it was before the loads calls; a second call gives the same (the ticket)."""
    levels, s = _open(key)
    _start(s, key, wall)
    s.run_cycles(K)
    for l in range(s.num_levels):
        what = f"{key} wall={wall} level {l}"
        want12, (want_ids, want_table) = _want(s, levels, l, key)
        if levels[l]["n_boundary"] == 0:            # (a golden's coarse level without solid walls: twelve zeros, no wall node)
            assert l > 0
            _same(s.surface_loads(l, REF, friction=True), np.zeros(12), f"{what}: loads")
            assert s.wall_node_count(l) == 0
            continue
        assert want12[6:9].all(), f"{what}: the friction force should not vanish"
        s_before = s.get(l, "viscous_stress")
        got = s.surface_loads(l, REF, friction=True)
        print(what, "Fp", got[:3], "Fv", got[6:9])
        _same(got, want12, f"{what}: loads")
        _same(got[:6], s.surface_loads(l, REF), f"{what}: pressure six")
        _same(s.surface_loads(l, REF, friction=True), want12, f"{what}: loads, second call")
        ids, table = s.wall_distribution(l)
        assert np.array_equal(ids, want_ids) and s.wall_node_count(l) == len(want_ids), what
        _same(table, want_table, f"{what}: distribution")
        ids, sw = s.wall_stress(l)
        assert np.array_equal(ids, want_ids)
        _same(sw, fle.wall_stresses(s.get(l, "variables"), _edges(s, levels, l), levels[l], (fle.GPU_MU[key], ve.PRANDTL))[1], f"{what}: Sw")
        _same(s.get(l, "viscous_stress"), s_before, f"{what}: S after the loads calls")
        s.compute_fluxes(l)
        _same(sw, s.get(l, "viscous_stress")[ids], f"{what}: Sw against the wall rows of S")
        s.zero_fluxes(l)
    s.close()


@pytest.mark.parametrize("key", ["A", "box17"])
def test_cycle_history_equals_the_synchronous_call(key):
    """Row c of mgcfd_run_cycles_loads_viscous is the synchronous call after cycle c on a twin stepped one cycle at a time; the RMS
    and the final state are mgcfd_run_cycles' bits; MGCFD_OPT_GRAPH is accepted."""
    runs = {}
    for name in ("plain", "twin", "history", "graph"):
        levels, s = _open(key, graph=1 if name == "graph" else 0)
        _start(s, key, 1)
        if name == "plain":
            rms, rows = s.run_cycles(K), None
        elif name == "twin":
            rms, rows = np.zeros(K), np.zeros((K, 12))
            for c in range(K):
                rms[c] = s.run_cycles(1)[0]
                rows[c] = s.surface_loads(0, REF, friction=True)
        else:
            rms, rows = s.run_cycles(K, loads=True, ref_point=REF, friction=True)
            assert rows.shape == (K, 12)
            _same(rows[-1], _want(s, levels, 0, key)[0], f"{key} {name}: the last row against the emulator")
        runs[name] = (rms, rows, [s.get(l, "variables") for l in range(s.num_levels)])
        s.close()
    for name in ("twin", "history", "graph"):
        _same(runs[name][0], runs["plain"][0], f"{key} {name}: RMS")
        for l, v in enumerate(runs[name][2]):
            _same(v, runs["plain"][2][l], f"{key} {name}: variables, level {l}")
    _same(runs["history"][1], runs["twin"][1], f"{key}: history rows")
    _same(runs["graph"][1], runs["twin"][1], f"{key}: history rows with MGCFD_OPT_GRAPH")


def test_graph_cycles_without_viscosity_keep_their_bits():
    """No viscous level: the friction six of every row are +0.0, the pressure six mgcfd_run_cycles_loads', the RMS and the state
    those of the captured cycle."""
    import mgcfd
    results = []
    for friction in (False, True):
        mesh = mgcfd.Mesh("input.dat", fse.case_input("m6_3lvl"), fse.case_duplicate("m6_3lvl"))
        s = mgcfd.Solver.from_mesh(mesh)
        s.set_option("graph", 1)
        rms, rows = s.run_cycles(K, loads=True, ref_point=REF, friction=friction)
        results.append((rms, rows, s.get(0, "variables")))
        s.close(); mesh.close()
    (rms0, rows0, v0), (rms1, rows1, v1) = results
    _same(rms1, rms0, "RMS")
    _same(v1, v0, "variables")
    _same(rows1[:, :6], rows0, "pressure six")
    _same(rows1[:, 6:], np.zeros((K, 6)), "friction six")


def test_advance_history_with_bdf2_on_lattice_a(oracle, tmp_path):
    """mgcfd_advance_loads_viscous under dual time stepping, BDF2: row k is the synchronous call after physical step k on a twin;
    RMS and final state are mgcfd_advance's bits."""
    steps, cycles = ve.DUAL_STEPS + 1, ve.DUAL_CYCLES
    dt = dte.pick_dt(oracle, fe.write_lattice("A", tmp_path), "local", 1.0)
    runs = {}
    for name in ("plain", "twin", "history"):
        levels, s = _open("A")
        s.set_time_step("local", 1.0)
        _start(s, "A", 1)
        s.set_dual_time(dt)
        s.dual_time_order(2)
        if name == "plain":
            rms, rows = s.advance(steps, cycles), None
        elif name == "twin":
            rms, rows = np.zeros((steps, cycles)), np.zeros((steps, 12))
            for k in range(steps):
                rms[k] = s.advance(1, cycles)[0]
                rows[k] = s.surface_loads(0, REF, friction=True)
        else:
            rms, rows = s.advance(steps, cycles, loads=True, ref_point=REF, friction=True)
            _same(rows[-1], _want(s, levels, 0, "A")[0], "advance: the last row against the emulator")
        assert s.dual_time()["levels"] == 2
        runs[name] = (rms, rows, [s.get(l, "variables") for l in range(s.num_levels)])
        s.close()
    for name in ("twin", "history"):
        _same(runs[name][0], runs["plain"][0], f"advance {name}: RMS")
        for l, v in enumerate(runs[name][2]):
            _same(v, runs["plain"][2][l], f"advance {name}: variables, level {l}")
    _same(runs["history"][1], runs["twin"][1], "advance: history rows")
    assert runs["history"][1][:, 6:9].all()


@pytest.mark.parametrize("key", ["A", "tet_2lvl"])
def test_fast_mode_gives_the_emulators_bits_on_its_own_state(key):
    """MGCFD_OPT_EXACT = 0: the cycles may contract, the loads, the wall stresses and the distribution never do."""
    levels, s = _open(key, exact=0)
    _start(s, key, 1)
    _, rows = s.run_cycles(K, loads=True, ref_point=REF, friction=True)
    for l in range(s.num_levels):
        want12, (want_ids, want_table) = _want(s, levels, l, key)
        _same(s.surface_loads(l, REF, friction=True), want12, f"{key} fast, level {l}: loads")
        _same(s.wall_distribution(l)[1], want_table, f"{key} fast, level {l}: distribution")
    _same(rows[-1], _want(s, levels, 0, key)[0], f"{key} fast: the last history row")
    s.close()


def test_a_level_the_terms_are_not_on_for():
    """Lattice A with the terms on level 0 alone: on levels 1 and 2 the friction six and the distribution's t are +0.0 in bits and
    the pressure six are unchanged; on a solver that never was viscous the same holds on level 0, and mgcfd_wall_stress refuses."""
    import mgcfd
    levels, s = _open("A")
    _start(s, "A", 1, levels=1)
    s.run_cycles(K)
    for l in (1, 2):
        got = s.surface_loads(l, REF, friction=True)
        want12, (want_ids, want_table) = _want(s, levels, l, "A", viscous=False)
        _same(got, want12, f"level {l}: loads")
        _same(got[6:], np.zeros(6), f"level {l}: friction six")
        _same(got[:6], s.surface_loads(l, REF), f"level {l}: pressure six")
        ids, table = s.wall_distribution(l)
        assert np.array_equal(ids, want_ids)
        _same(table, want_table, f"level {l}: distribution")
        _same(table[:, 4:], np.zeros((len(ids), 3)), f"level {l}: t")
        with pytest.raises(mgcfd.MgcfdError) as e:
            s.wall_stress(l)
        assert e.value.code == 1
    assert s.surface_loads(0, REF, friction=True)[6:9].all()
    s.close()
    levels, s = _open("A")
    s.run_cycles(2)
    got = s.surface_loads(0, REF, friction=True)
    _same(got, _want(s, levels, 0, "A", viscous=False)[0], "never viscous: loads")
    _same(got[6:], np.zeros(6), "never viscous: friction six")
    s.close()


def test_a_level_without_solid_wall_gives_twelve_zeros():
    import mgcfd
    from mgcfd import meshgen
    mg = meshgen.make_multigrid((9, 5), "fvcorr", seed=4, cavity_radius=0.0, jitter=0.2)
    levels = mgcfd.generated_to_levels(mg)
    assert all(L["n_boundary"] == 0 for L in levels)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    s.set_viscous(0.05, levels=2)
    _same(s.surface_loads(0, REF, friction=True), np.zeros(12), "loads")
    assert s.wall_node_count(0) == 0
    ids, table = s.wall_distribution(0)
    assert ids.shape == (0,) and table.shape == (0, 7)
    rms, rows = s.run_cycles(2, loads=True, ref_point=REF, friction=True)
    _same(rows, np.zeros((2, 12)), "history")
    s.close()


def test_a_partitioned_solver_is_refused():
    import mgcfd
    from mgcfd import meshgen
    mg = meshgen.make_multigrid((9,), "m6wing", seed=3, cavity_radius=0.15)
    levels = mgcfd.generated_to_levels(mg)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant, n_owned=[levels[0]["nel"]])
    for call in (lambda: s.surface_loads(0, friction=True), lambda: s.run_cycles(1, loads=True, friction=True),
                 lambda: s.wall_node_count(0), lambda: s.wall_distribution(0)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1 and "partitioned" in str(e.value)
    s.close()


def test_device_resources_return_to_their_start_values():
    import mgcfd
    levels, s = _open("box17")
    s.close()                                   # (the runtime and the library are up)
    before = mgcfd.live_device_resources()
    levels, s = _open("box17")
    _start(s, "box17", 1)
    s.run_cycles(1, loads=True, friction=True)
    s.wall_distribution(0)
    assert mgcfd.live_device_resources()["allocations"] > before["allocations"]
    s.close()
    assert mgcfd.live_device_resources() == before


def _run_driver(tmp, extra, ok=True):
    os.makedirs(tmp / "out", exist_ok=True)
    cmd = [EXE, "-i", "input.dat", "-d", fse.case_input("m6_2lvl"), "-o", "out/", "-g", str(K)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=tmp)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


def _csv(path):
    lines = path.read_text().splitlines()
    return lines[0], np.array([[float(v) for v in l.split(",")] for l in lines[1:]])


def test_driver_flags(tmp_path):
    """--loads-friction: the thirteen columns come from Fp + Fv and the friction loads and their coefficients follow, in
    surface_loads.* and polar.csv, all equal to the C calls'; --output-surface writes the distribution as Cp and Cf; without the
    new flags the loads file is the one mgcfd_run_cycles_loads gives; the flags' conditions are checked right after parsing."""
    import mgcfd
    S, c, ref = 0.7532, 0.64607, (0.5, 0.25, -0.125)
    visc = [f"--viscosity={ve.DRIVER_MU!r}", "--no-slip", "--viscous-levels", "8"]
    loads = ["--output-loads", f"--loads-reference={S},{c},{ref[0]},{ref[1]},{ref[2]}"]
    name = f"surface_loads.size=1x.cycles={K}.level=0"
    old_header = "cycle,Fx,Fy,Fz,Mx,My,Mz,CD,CL,CS,CMx,CMy,CMz"
    mesh = mgcfd.Mesh("input.dat", fse.case_input("m6_2lvl"), 1)
    s = mgcfd.Solver.from_mesh(mesh)
    s.set_viscous(ve.DRIVER_MU, ve.PRANDTL, True, ve.VISCOUS_CFL, 8)
    _, hist = s.run_cycles(K, loads=True, ref_point=ref, friction=True)
    ids, table = s.wall_distribution(0)
    coords = mesh.level(0)["coords"]
    ff = s.far_field()
    # without the new flags: the file of the pressure loads, as before
    _run_driver(tmp_path / "pressure", visc + loads)
    header, got = _csv(tmp_path / "pressure" / "out" / name)
    assert header == old_header and got.shape == (K, 13)
    _same(got[:, 1:7], hist[:, :6], "pressure loads file")
    _same(got[:, 7:], s.load_coefficients(hist[:, :6], S, c), "pressure loads file: coefficients")
    assert not [n for n in os.listdir(tmp_path / "pressure" / "out") if n.startswith("surface.")]
    # with them
    _run_driver(tmp_path / "friction", visc + loads + ["--loads-friction", "--output-surface"])
    header, got = _csv(tmp_path / "friction" / "out" / name)
    assert header == old_header + ",Fxv,Fyv,Fzv,Mxv,Myv,Mzv,CDv,CLv,CSv,CMxv,CMyv,CMzv" and got.shape == (K, 25)
    total = hist[:, :6] + hist[:, 6:]
    _same(got[:, 1:7], total, "total loads")
    _same(got[:, 7:13], s.load_coefficients(total, S, c), "total coefficients")
    _same(got[:, 13:19], hist[:, 6:], "friction loads")
    _same(got[:, 19:25], s.load_coefficients(hist[:, 6:], S, c), "friction coefficients")
    assert hist[:, 6:9].all()
    header, surf = _csv(tmp_path / "friction" / "out" / "surface.size=1x.level=0")
    assert header == "node,x,y,z,ax,ay,az,Cp,Cfx,Cfy,Cfz" and surf.shape == (len(ids), 11)
    assert np.array_equal(surf[:, 0].astype(np.int64), ids)
    _same(surf[:, 1:4], coords[ids], "surface: coordinates")
    _same(surf[:, 4:7], table[:, 0:3], "surface: a")
    cp, cf = mgcfd.surface_coefficients(ff, table)
    assert np.allclose(surf[:, 7], cp, rtol=1e-14, atol=0) and np.allclose(surf[:, 8:11], cf, rtol=1e-12, atol=1e-18)
    # polar.csv: the same appended columns, each angle's last cycle
    s.close()
    alphas = (0.0, 2.0)
    _run_driver(tmp_path / "polar", visc + ["--polar", "0:2:2", "--loads-friction", f"--loads-reference={S},{c},{ref[0]},{ref[1]},{ref[2]}"])
    header, got = _csv(tmp_path / "polar" / "out" / "polar.csv")
    assert header == "alpha,mach,rms_last,Fx,Fy,Fz,Mx,My,Mz,CD,CL,CS,CMx,CMy,CMz,Fxv,Fyv,Fzv,Mxv,Myv,Mzv,CDv,CLv,CSv,CMxv,CMyv,CMzv"
    s = mgcfd.Solver.from_mesh(mesh)
    s.set_viscous(ve.DRIVER_MU, ve.PRANDTL, True, ve.VISCOUS_CFL, 8)
    for k, alpha in enumerate(alphas):
        s.set_free_stream(1.2, alpha, reinitialise=(k == 0))
        _, h = s.run_cycles(K, loads=True, ref_point=ref, friction=True)
        _same(got[k, 3:9], h[-1, :6] + h[-1, 6:], f"polar, alpha {alpha}: total loads")
        _same(got[k, 15:21], h[-1, 6:], f"polar, alpha {alpha}: friction loads")
        _same(got[k, 21:27], s.load_coefficients(h[-1, 6:], S, c), f"polar, alpha {alpha}: friction coefficients")
    s.close(); mesh.close()
    # the conditions, decided right after parsing: exit status 1 and no output
    for extra in (loads + ["--loads-friction"], visc + ["--loads-friction"], visc + loads + ["--loads-friction", "--gpus", "2", "--gpus-partition"],
                  ["--output-surface", "--gpus", "2"]):
        r = _run_driver(tmp_path / "refused", extra, ok=False)
        assert r.returncode == 1 and "ERROR" in r.stderr and not os.listdir(tmp_path / "refused" / "out")
