"""GPU tests of the wall thermal conditions and the heat loads (mgcfd_set_wall_temperature, mgcfd_surface_loads_heat,
mgcfd_wall_heat and their neighbours) against the numpy emulator (tests/wall_heat_emulator.py) bit for bit:
the runs under the isothermal and the heat-flux wall (state and step factors of every level, RMS history), composed with residual
smoothing, JST, FAS, the Spalart-Allmaras model and dual time stepping; the fourteen loads and the heat table on every level,
evaluated by the emulator on the state read back; the histories; the fast mode; the setters in either order, a change of the wall
temperature mid-run and the return to adiabatic; the refusals and the device allocations; polar; the driver.
tests/test_host_wall_heat.py checks the emulator itself and asserts on the CPU that every run here stays valid."""
import os
import subprocess

import numpy as np
import pytest

import dual_time_emulator as dte
import fas_emulator as fe
import free_stream_emulator as fse
import friction_loads_emulator as fle
import sa_emulator as sae
import variable_viscosity_emulator as vve
import viscous_emulator as ve
import wall_heat_emulator as whe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
K = whe.GPU_CYCLES
REF = (0.25, -0.125, 0.375)
MODE_NAMES = {whe.ISOTHERMAL: "isothermal", whe.HEAT_FLUX: "heat-flux", whe.ADIABATIC: "adiabatic"}
LATTICE_MODES = [(whe.ISOTHERMAL, whe.TW_RATIOS[0]), (whe.HEAT_FLUX, whe.QW)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(got - want).max():.3e}"


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("wall_heat_cases")
    out = {key: fle.write_case(key, d) for key in whe.GENERATED if key != "A"}
    out["A"] = fe.write_lattice("A", d)
    return out


def _solver(case, exact=1):
    """(level dicts, solver) of a case directory or a golden's name."""
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    levels = [dict(mesh.level(l)) for l in range(mesh.num_levels)]
    s = mgcfd.Solver.from_mesh(mesh)
    mesh.close()                                # (mgcfd_create_from_mesh copies what it needs)
    s.set_option("exact", exact)
    return levels, s


def _levels(s, lv):
    return s.num_levels if lv == "all" else lv


def _configure(s, mu, lv, mode, x, smoothing=(0.0, 0), jst_levels=0, fas=False, model=None, step=whe.RUN_STEP, order=(0, 1)):
    """The solver as whe.configured sets the emulator up; ``order``: the order of the two setters that make the mode effective."""
    s.set_time_step(step[0], 2.0 if smoothing[1] else step[1])
    if smoothing[1]:
        s.set_residual_smoothing(*smoothing)
    if jst_levels:
        s.set_jst(levels=jst_levels)
    if fas:
        s.set_fas(True)
    s.set(0, "variables", ve.start_state(s.nel(0), s.far_field()[:5]))
    value = whe.setting_value(s.far_field(), mode, x)
    setters = (lambda: s.set_viscous(mu, ve.PRANDTL, True, ve.VISCOUS_CFL, _levels(s, lv)),
               lambda: s.set_wall_temperature(MODE_NAMES[mode], value))
    for k in order:
        setters[k]()
    assert s.wall_temperature() == (MODE_NAMES[mode], value)
    if model is not None:
        s.set_viscosity_model(law=model[0], eddy=model[1])


_emulated = {}


def _emulate(oracle, case, mu, lv, mode, x, **composed):
    """(rms, variables, step factors, nt, mut) per level of K cycles: computed once per combination, shared and left unchanged."""
    key = (case, mu, lv, mode, x, tuple(sorted((k, str(v)) for k, v in composed.items())))
    if key not in _emulated:
        em = whe.configured(oracle, case, mu, lv, mode, x, **composed)
        rc, rms = em.cycles(K)
        assert rc == 0
        sa = [l for l in range(em.visc_levels) if em.sa_on(l)]
        _emulated[key] = (rms, [em.variables(l) for l in range(em.n)], [em.step_factors(l) for l in range(em.n)],
                          [em.nu_tilde(l) for l in sa], [em.eddy_viscosity(l) for l in sa])
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


def _stresses(s, levels, l, mu, model=None):
    """S of level l's state as the GPU holds it, under the model that is on; None on a level the terms are not on for."""
    if l >= s.viscous()[4]:
        return None
    v, e = s.get(l, "variables"), s.get_edges(l, len(levels[l]["edges"]))
    if model is None:
        return whe.node_stresses(v, e, levels[l], mu, ve.PRANDTL)
    m = vve.Model(model[0], vve.far_field_t_ref(s.far_field()), eddy="field" if model[1] == sae.SA else model[1])
    return whe.node_stresses(v, e, levels[l], mu, ve.PRANDTL, m, s.get(l, "eddy_viscosity").ravel())


def _check_heat_loads(s, levels, mu, what, model=None):
    """On every level: out14 and the heat table are the emulator's bits on the state read back; the first twelve are
    mgcfd_surface_loads_viscous'; a second call gives the same (the ticket)."""
    for l in range(s.num_levels):
        v, e = s.get(l, "variables"), s.get_edges(l, len(levels[l]["edges"]))
        got = s.surface_loads(l, REF, heat=True)
        ids, table = s.wall_heat(l)
        if levels[l]["n_boundary"] == 0:            # (a coarse level without solid walls: fourteen zeros, no wall node)
            _same(got, np.zeros(14), f"{what}: loads, level {l}")
            assert len(ids) == 0 and table.shape == (0, 3)
            continue
        S = _stresses(s, levels, l, mu, model)
        want14 = whe.surface_loads14(v, e, levels[l], s.far_field(), REF, S)
        want_ids, want_table = whe.wall_heat(v, e, levels[l], S)
        print(what, "level", l, "Q", got[12], "A", got[13])
        _same(got, want14, f"{what}: out14, level {l}")
        _same(got[:12], s.surface_loads(l, REF, friction=True), f"{what}: the first twelve, level {l}")
        _same(s.surface_loads(l, REF, heat=True), want14, f"{what}: out14, second call, level {l}")
        assert np.array_equal(ids, want_ids) and np.array_equal(ids, s.wall_distribution(l)[0])
        _same(table, want_table, f"{what}: heat table, level {l}")
        if S is None:
            _same(got[12:13], np.zeros(1), f"{what}: Q on a level the terms are not on for, level {l}")
            _same(table[:, 0], np.zeros(len(ids)), f"{what}: h on a level the terms are not on for, level {l}")
            assert got[13] > 0.0
        else:
            assert got[12] != 0.0 and got[13] > 0.0 and table[:, 0].any()


# ---- runs ----
@pytest.mark.parametrize("key,lv,mode,x", whe.gpu_runs())
def test_runs_equal_the_emulator(key, lv, mode, x, oracle, cases):
    """K cycles from the perturbed start state under the isothermal wall (hot and cold) and the heat-flux wall, one level and all
    levels covered: state and step factors of every level and the RMS history are the emulator's bits; then the fourteen loads
    and the heat table of every level (a level the terms are not on for and a level without walls among them)."""
    case, mu = cases.get(key, key), whe.RUN_MU[key]
    want = _emulate(oracle, case, mu, lv, mode, x)
    levels, s = _solver(case)
    _configure(s, mu, lv, mode, x)
    rms = s.run_cycles(K)
    what = f"{key} levels={lv} {MODE_NAMES[mode]} {x}"
    print(what, "rms", rms, "want", want[0])
    _check_run(s, rms, want, what)
    _check_heat_loads(s, levels, mu, what)
    if key == "box17":
        assert levels[0]["n_boundary"] == 414 and s.wall_node_count(0) == 278       # two chunks of edges, two workgroups of nodes
    if mode == whe.ISOTHERMAL:
        ew = np.float64(whe.setting_value(s.far_field(), mode, x)) / (ve.GAMMA - 1.0)
        for l in range(s.viscous()[4]):
            v, w = s.get(l, "variables"), s.wall_heat(l)[0]
            _same(v[w, 4], v[w, 0] * ew, f"{what}: wall energy, level {l}")
            assert not v[w, 1:4].any()
    s.close()


@pytest.mark.parametrize("mode,x", LATTICE_MODES, ids=["isothermal", "heat-flux"])
@pytest.mark.parametrize("name,smoothing,jst_levels,fas", whe.COMPOSED, ids=[c[0] for c in whe.COMPOSED])
def test_composition(name, smoothing, jst_levels, fas, mode, x, oracle, cases):
    """Lattice A, all levels, with residual smoothing (0.5, 2), with JST on level 0 and with FAS (P and W0 too), one at a time."""
    mu = whe.RUN_MU["A"]
    composed = dict(smoothing=smoothing, jst_levels=jst_levels, fas=fas)
    em = whe.configured(oracle, cases["A"], mu, "all", mode, x, **composed)
    rc, want_rms = em.cycles(K)
    assert rc == 0
    levels, s = _solver(cases["A"])
    _configure(s, mu, "all", mode, x, **composed)
    _same(s.run_cycles(K), want_rms, f"{name}: RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), em.variables(l), f"{name}: variables, level {l}")
        _same(s.get(l, "step_factors"), em.step_factors(l), f"{name}: step factors, level {l}")
        if fas and l >= 1:
            _same(s.get(l, "fas_forcing"), em.P[l], f"{name}: P, level {l}")
            _same(s.get(l, "fas_start"), em.W0[l], f"{name}: W0, level {l}")
    em.close()
    s.close()


@pytest.mark.parametrize("mode,x", LATTICE_MODES, ids=["isothermal", "heat-flux"])
def test_spalart_allmaras_with_sutherland(mode, x, oracle, cases):
    """Lattice A, all levels, (sutherland, SA): state, step factors, nu_tilde, eddy viscosity and RMS; the heat loads with the
    conductivity of the model that is on."""
    mu = whe.RUN_MU["A"]
    want = _emulate(oracle, cases["A"], mu, "all", mode, x, model=whe.SA_MODEL)
    levels, s = _solver(cases["A"])
    _configure(s, mu, "all", mode, x, model=whe.SA_MODEL)
    rms = s.run_cycles(K)
    _check_run(s, rms, want, f"SA {MODE_NAMES[mode]}")
    assert len(want[3]) == s.num_levels
    _check_heat_loads(s, levels, mu, f"SA {MODE_NAMES[mode]}", model=whe.SA_MODEL)
    s.close()


def test_dual_time_bdf2_and_the_advance_history(oracle, cases):
    """The isothermal wall under mgcfd_advance (BDF2) on lattice A: the emulator's RMS, state and time level; row k of
    mgcfd_advance_loads_heat is the synchronous call after physical step k on a twin; same RMS and final state."""
    mu, (mode, x), step = whe.RUN_MU["A"], LATTICE_MODES[0], ("local", 1.0)
    dt = dte.pick_dt(oracle, cases["A"], *step)
    steps, cycles = whe.DUAL_STEPS, whe.DUAL_CYCLES
    em = whe.configured(oracle, cases["A"], mu, "all", mode, x, step=step)
    em.set_dual_time(dt)
    em.set_order(2)
    rc, want_rms = em.advance(steps, cycles)
    assert rc == 0
    runs = {}
    for name in ("twelve", "plain", "twin", "history"):
        levels, s = _solver(cases["A"])
        _configure(s, mu, "all", mode, x, step=step)
        s.set_dual_time(dt)
        s.dual_time_order(2)
        if name == "twelve":
            rms, rows = s.advance(steps, cycles, loads=True, ref_point=REF, friction=True)
        elif name == "plain":
            rms, rows = s.advance(steps, cycles), None
            _same(rms.ravel(), want_rms, "advance: RMS history against the emulator")
            for l in range(s.num_levels):
                _same(s.get(l, "variables"), em.variables(l), f"advance: variables, level {l}")
                _same(s.get(l, "time_n"), em.Wn[l], f"advance: Wn, level {l}")
        elif name == "twin":
            rms, rows = np.zeros((steps, cycles)), np.zeros((steps, 14))
            for k in range(steps):
                rms[k] = s.advance(1, cycles)[0]
                rows[k] = s.surface_loads(0, REF, heat=True)
        else:
            rms, rows = s.advance(steps, cycles, loads=True, ref_point=REF, heat=True)
            assert rows.shape == (steps, 14)
            _same(rows[:, :12], runs["twelve"][1], "advance: the first twelve against mgcfd_advance_loads_viscous")
        runs[name] = (rms, rows, [s.get(l, "variables") for l in range(s.num_levels)])
        s.close()
    em.close()
    for name in ("twelve", "twin", "history"):
        _same(runs[name][0], runs["plain"][0], f"advance {name}: RMS")
        for l, v in enumerate(runs[name][2]):
            _same(v, runs["plain"][2][l], f"advance {name}: variables, level {l}")
    _same(runs["history"][1], runs["twin"][1], "advance: history rows")
    assert runs["history"][1][:, 12].all()


@pytest.mark.parametrize("key", ["A", "box17"])
def test_cycle_history_equals_the_synchronous_call(key, cases):
    """Row c of mgcfd_run_cycles_loads_heat is the synchronous call after cycle c on a twin stepped one cycle at a time; the RMS,
    the final state and the first twelve columns are mgcfd_run_cycles_loads_viscous'."""
    mu, (mode, x) = whe.RUN_MU[key], LATTICE_MODES[0]
    runs = {}
    for name in ("twelve", "twin", "history"):
        levels, s = _solver(cases[key])
        _configure(s, mu, "all", mode, x)
        if name == "twelve":
            rms, rows = s.run_cycles(K, loads=True, ref_point=REF, friction=True)
        elif name == "twin":
            rms, rows = np.zeros(K), np.zeros((K, 14))
            for c in range(K):
                rms[c] = s.run_cycles(1)[0]
                rows[c] = s.surface_loads(0, REF, heat=True)
        else:
            rms, rows = s.run_cycles(K, loads=True, ref_point=REF, heat=True)
            assert rows.shape == (K, 14)
        runs[name] = (rms, rows, [s.get(l, "variables") for l in range(s.num_levels)])
        s.close()
    for name in ("twin", "history"):
        _same(runs[name][0], runs["twelve"][0], f"{key} {name}: RMS")
        for l, v in enumerate(runs[name][2]):
            _same(v, runs["twelve"][2][l], f"{key} {name}: variables, level {l}")
    _same(runs["history"][1], runs["twin"][1], f"{key}: history rows")
    _same(runs["history"][1][:, :12], runs["twelve"][1], f"{key}: the first twelve columns")


@pytest.mark.parametrize("mode,x", LATTICE_MODES, ids=["isothermal", "heat-flux"])
def test_fast_mode_gives_the_emulators_bits_on_its_own_state(mode, x, cases):
    """MGCFD_OPT_EXACT = 0: the cycles may contract; the wall launches, the loads and the heat table never do."""
    mu = whe.RUN_MU["A"]
    levels, s = _solver(cases["A"], exact=0)
    _configure(s, mu, "all", mode, x)
    _, rows = s.run_cycles(K, loads=True, ref_point=REF, heat=True)
    _check_heat_loads(s, levels, mu, f"fast {MODE_NAMES[mode]}")
    _same(rows[-1], s.surface_loads(0, REF, heat=True), "fast: the last history row")
    if mode == whe.ISOTHERMAL:
        ew = np.float64(whe.setting_value(s.far_field(), mode, x)) / (ve.GAMMA - 1.0)
        for l in range(s.num_levels):
            v, w = s.get(l, "variables"), s.wall_heat(l)[0]
            _same(v[w, 4], v[w, 0] * ew, f"fast: wall energy, level {l}")
    s.close()


def test_a_level_the_terms_are_not_on_for_and_a_solver_without_them(cases):
    """Lattice A with the terms on level 0 alone: on levels 1 and 2 Q and every h are +0.0 in bits and A is still summed (inside
    _check_heat_loads); the same on level 0 of a solver that never was viscous."""
    levels, s = _solver(cases["A"])
    _configure(s, whe.RUN_MU["A"], 1, *LATTICE_MODES[0])
    s.run_cycles(K)
    _check_heat_loads(s, levels, whe.RUN_MU["A"], "level 0 alone")
    s.close()
    levels, s = _solver(cases["A"])
    s.run_cycles(1)
    _check_heat_loads(s, levels, 0.0, "never viscous")
    s.close()


# ---- the setting ----
def test_setter_order_a_change_mid_run_and_the_return_to_adiabatic(oracle, cases):
    """The thermal setter before the viscous one; K cycles; another wall temperature (applied at once); K cycles; the heat-flux
    wall; K cycles; adiabatic again (the state stays); K cycles: the emulator driven the same way, bit for bit."""
    mu, (mode, x) = whe.RUN_MU["A"], LATTICE_MODES[0]
    em = whe.configured(oracle, cases["A"], mu, "all", mode, x, order=(1, 0))
    levels, s = _solver(cases["A"])
    _configure(s, mu, "all", mode, x, order=(1, 0))
    t_inf = whe.free_stream_temperature(s.far_field())[0]
    for leg, (name, value) in enumerate(((None, None), ("isothermal", whe.TW_RATIO_CHANGED * t_inf), ("heat-flux", whe.QW), ("adiabatic", 0.0))):
        if name is not None:
            before = s.get(0, "variables")
            em.set_wall_temperature(name, value)
            s.set_wall_temperature(name, value)
            assert s.wall_temperature() == (name, value)
            if name != "isothermal":
                _same(s.get(0, "variables"), before, f"leg {leg}: the setter keeps the state")
            for l in range(s.num_levels):
                _same(s.get(l, "variables"), em.variables(l), f"leg {leg}: the state behind the setter, level {l}")
        rc, want_rms = em.cycles(K)
        assert rc == 0
        _same(s.run_cycles(K), want_rms, f"leg {leg}: RMS history")
        for l in range(s.num_levels):
            _same(s.get(l, "variables"), em.variables(l), f"leg {leg}: variables, level {l}")
    em.close()
    s.close()


def test_a_solver_that_never_calls_the_setter_keeps_its_bits(oracle, cases):
    """tests/test_gpu_viscous.py's run on lattice A (cell Reynolds number 2, local steps, no-slip walls, all levels): a solver that
    never calls the setter and one that went to the heat-flux wall and back before the run both give that run's bits, which are
    the viscous emulator's."""
    em = ve.configured(oracle, cases["A"], ve.CELL_RE_MU, "local", 1.0, 1, "all")
    rc, want_rms = em.cycles(K)
    assert rc == 0
    for touched in (False, True):
        levels, s = _solver(cases["A"])
        s.set_time_step("local", 1.0)
        s.set(0, "variables", ve.start_state(s.nel(0), s.far_field()[:5]))
        s.set_viscous(ve.CELL_RE_MU, ve.PRANDTL, True, ve.VISCOUS_CFL, s.num_levels)
        if touched:
            s.set_wall_temperature("heat-flux", whe.QW)
            s.set_wall_temperature("adiabatic")
        assert s.wall_temperature() == ("adiabatic", 0.0)
        _same(s.run_cycles(K), want_rms, f"touched={touched}: RMS history")
        for l in range(s.num_levels):
            _same(s.get(l, "variables"), em.variables(l), f"touched={touched}: variables, level {l}")
        s.close()
    em.close()


def test_refusals_and_device_resources(cases):
    """An unknown mode, bad values, mid-sweep, a group member and a partitioned solver: error code 1 and nothing changed; the areas
    are held exactly while the heat-flux wall is in effect, and closing returns every allocation."""
    import mgcfd
    base = mgcfd.live_device_resources()
    levels, s = _solver(cases["A"])
    s.set_viscous(whe.RUN_MU["A"], ve.PRANDTL, True, ve.VISCOUS_CFL, 2)
    s.set_wall_temperature("isothermal", 1.0)
    for mode, value in ((3, 1.0), (-1, 1.0), (1, 0.0), (1, -1.0), (1, float("nan")), (1, float("inf")), (2, float("nan")), (2, float("inf"))):
        with pytest.raises(mgcfd.MgcfdError) as e:
            s._c(s.lib.mgcfd_set_wall_temperature(s.handle, mode, value))
        assert e.value.code == 1 and "wall temperature" in str(e.value), (mode, value)
    assert s.wall_temperature() == ("isothermal", 1.0)
    s.set_wall_temperature("heat-flux", -whe.QW)            # (either sign)
    s.set_wall_temperature("isothermal", 1.0)
    on = mgcfd.live_device_resources()
    s.set_wall_temperature("heat-flux", whe.QW)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"] + 2, "the areas of the two covered levels"
    s.set_wall_temperature("heat-flux", 2.0 * whe.QW)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"] + 2, "allocated once"
    s.set_viscous(whe.RUN_MU["A"], ve.PRANDTL, True, ve.VISCOUS_CFL, 3)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"] + 3 + 3, "a further level: its three arrays and its areas"
    s.set_viscous(whe.RUN_MU["A"], ve.PRANDTL, False, ve.VISCOUS_CFL, 2)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"], "slip walls: the mode is not in effect"
    s.set_viscous(whe.RUN_MU["A"], ve.PRANDTL, True, ve.VISCOUS_CFL, 2)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"] + 2
    s.set_wall_temperature("adiabatic")
    off = mgcfd.live_device_resources()
    assert off["allocations"] == on["allocations"] and off["bytes"] == on["bytes"], "the mode off releases"
    s.set_wall_temperature("heat-flux", whe.QW)
    s.set_viscous(0.0, levels=0)
    assert s.wall_temperature() == ("heat-flux", whe.QW), "kept while the terms are off"
    s.set_wall_temperature("adiabatic")
    # the diagnostics run and leave the state alone
    s.set_viscous(whe.RUN_MU["A"], ve.PRANDTL, True, ve.VISCOUS_CFL, 2)
    before = s.get(0, "variables")
    assert all(s.bench_wall_heat(0, kind, 3) > 0.0 for kind in range(5))
    _same(s.get(0, "variables"), before, "the state after the diagnostics")
    s.zero_fluxes(0)
    for kind, level in ((5, 0), (-1, 0), (0, 2)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            s.bench_wall_heat(level, kind, 1)
        assert e.value.code == 1
    # mid-sweep (the split sweep runs with the terms off)
    s.set_viscous(0.0, levels=0)
    s.sweep_begin(0)
    s.sweep_stage(0, 0, partials=False)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_wall_temperature("isothermal", 1.0)
    assert e.value.code == 1 and "sweep is under way" in str(e.value) and s.wall_temperature() == ("adiabatic", 0.0)
    s.sweep_stage(0, 1, partials=False)
    s.sweep_stage(0, 2, partials=False)
    # a group member
    g = mgcfd.Group([s])
    for call in (lambda: s.set_wall_temperature("isothermal", 1.0), lambda: s.surface_loads(0, heat=True), lambda: s.wall_heat(0),
                 lambda: s.run_cycles(1, loads=True, heat=True)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1
    g.close()
    s.close()
    assert mgcfd.live_device_resources()["allocations"] == base["allocations"]
    # a partitioned solver
    from mgcfd.partition import partition_hierarchy, rcb_partition
    mesh = mgcfd.Mesh("input.dat", fse.case_input("m6_2lvl"), 1)
    lvs = [mesh.level(l) for l in range(mesh.num_levels)]
    H = partition_hierarchy(lvs, rcb_partition(np.asarray(lvs[0]["coords"]).reshape(-1, 3), 2))
    lv, owned, keys = H[0].solver_args()
    t = mgcfd.Solver.from_arrays(lv, mesh.variant, n_owned=owned, order_keys=keys)
    for call in (lambda: t.set_wall_temperature("isothermal", 1.0), lambda: t.surface_loads(0, heat=True), lambda: t.wall_heat(0)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1
    assert t.wall_temperature() == ("adiabatic", 0.0)
    t.close()
    mesh.close()
    assert mgcfd.live_device_resources()["allocations"] == base["allocations"]


def test_polar_with_a_wall_temperature(oracle):
    """Solver.polar(wall_temperature=...) = set_wall_temperature once, then the polar; every angle that starts from its far field
    starts with the isothermal wall applied."""
    case, alphas, mach = fse.POLAR_CASE, fse.POLAR_ALPHAS, fse.POLAR_MACH
    tw = whe.TW_RATIOS[0] * whe.free_stream_temperature(fse.free_stream_constants(mach, alphas[0]))[0]
    levels, s = _solver(case)
    pol = s.polar(alphas, K, mach=mach, viscous={"mu": ve.DRIVER_MU, "wall": True, "levels": 2}, wall_temperature=("isothermal", tw))
    assert s.wall_temperature() == ("isothermal", tw)
    em = whe.WallHeatOracle(oracle, case, mu=ve.DRIVER_MU, wall=1, viscous_levels=2)
    em.set_wall_temperature("isothermal", tw)
    for k, (al, p) in enumerate(zip(alphas, pol)):
        em.set_far_field(fse.free_stream_constants(mach, al), reinitialise=(k == 0))
        rc, rms = em.cycles(K)
        assert rc == 0
        _same(p["rms"], rms, f"polar, angle {al}: RMS history")
    _same(s.get(0, "variables"), em.variables(0), "the polar's last state")
    em.close()
    s.close()
    levels, s = _solver(case)
    s.polar(alphas[:1], 1, mach=mach, viscous={"mu": ve.DRIVER_MU, "wall": True, "levels": 1}, wall_temperature={"mode": "heat-flux", "value": whe.QW})
    assert s.wall_temperature() == ("heat-flux", whe.QW)
    s.close()


# ---- the drop-in binary ----
def _run_driver(tmp, case, extra, cycles, ok=True):
    os.makedirs(tmp / "out", exist_ok=True)
    cmd = [EXE, "-i", "input.dat", "-d", fse.case_input(case), "-o", "out/", "-g", str(cycles), "-m", str(fse.case_duplicate(case))] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tmp)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


def _out_file(d, prefix):
    return (d / "out" / [n for n in os.listdir(d / "out") if n.startswith(prefix)][0]).read_text()


def test_driver_flags(oracle, tmp_path):
    """--wall-temperature-ratio against the free stream of --mach / --alpha: the dump is the %.17e rendering of the emulator's
    state; --wall-temperature and the config keys likewise; --loads-heat appends Q, A, St_mean to surface_loads.* and qw, T, St to
    surface.* and changes no other byte; without the new flags every file is what it was; the flag errors exit with status 1
    before any GPU work (no file written)."""
    import mgcfd
    case = "m6_2lvl"
    dup = fse.case_duplicate(case)
    name = f"variables.size={dup}x.cycles={K}.level=0"
    mach, alpha, ratio = 0.8, 2.0, whe.TW_RATIOS[0]
    ff = mgcfd.free_stream_constants(mach, alpha)
    tw = ratio * mgcfd.free_stream_temperature(ff)[0]
    em = whe.WallHeatOracle(oracle, case, mu=ve.DRIVER_MU, wall=1, viscous_levels="all")
    em.set_wall_temperature("isothermal", tw)
    em.set_far_field(ff, reinitialise=True)
    rc, _ = em.cycles(K)
    assert rc == 0
    want = fse.render_variables(em.variables(0)).encode()
    em.close()
    viscous = [f"--viscosity={ve.DRIVER_MU!r}", "--no-slip", "--viscous-levels", "8", "--mach", str(mach), "--alpha", str(alpha)]
    conf = tmp_path / "run.conf"
    conf.write_text(f"viscosity = {ve.DRIVER_MU!r}\nno_slip = Y\nviscous_levels = 8\nwall_temperature = {tw!r}\nff_mach = {mach}\nangle_of_attack = {alpha}\n")
    for tag, extra in (("ratio", viscous + ["--wall-temperature-ratio", repr(ratio)]), ("value", viscous + [f"--wall-temperature={tw!r}"]),
                       ("conf", ["-c", str(conf)])):
        _run_driver(tmp_path / tag, case, ["--output-variables"] + extra, K)
        assert (tmp_path / tag / "out" / name).read_bytes() == want, tag
    # the appended columns: the other bytes stay
    loads = viscous + ["--wall-temperature-ratio", repr(ratio), "--output-loads", "--loads-friction", "--output-surface", "--output-variables"]
    _run_driver(tmp_path / "twelve", case, loads, K)
    _run_driver(tmp_path / "heat", case, loads + ["--loads-heat"], K)
    assert (tmp_path / "heat" / "out" / name).read_bytes() == want == (tmp_path / "twelve" / "out" / name).read_bytes()
    levels, s = _solver(case)
    s.set_free_stream(mach, alpha, reinitialise=True)
    s.set_viscous(ve.DRIVER_MU, ve.PRANDTL, True, ve.VISCOUS_CFL, s.num_levels)
    s.set_wall_temperature("isothermal", tw)
    _, rows = s.run_cycles(K, loads=True, heat=True)
    ids, table = s.wall_heat(0)
    qw, st = mgcfd.heat_coefficients(ff, table, t_wall=tw)
    s.close()
    for prefix, extra_header, n_extra in (("surface_loads", ",Q,A,St_mean", 3), ("surface.", ",qw,T,St", 3)):
        old, new = _out_file(tmp_path / "twelve", prefix).splitlines(), _out_file(tmp_path / "heat", prefix).splitlines()
        assert len(old) == len(new) and new[0] == old[0] + extra_header
        for a, b in zip(old[1:], new[1:]):
            assert b.startswith(a + ",") and len(b[len(a) + 1:].split(",")) == n_extra
    got = np.array([[float(x) for x in line.split(",")[-3:]] for line in _out_file(tmp_path / "heat", "surface_loads").splitlines()[1:]])
    _same(got[:, :2], rows[:, 12:], "surface_loads.*: Q and A")
    t_total = mgcfd.free_stream_temperature(ff)[1]
    scale = ff[0] * np.sqrt(((ff[1:4] / ff[0]) ** 2).sum()) * (1.4 / 0.4) * (t_total - tw)
    assert np.allclose(got[:, 2], (rows[:, 12] / rows[:, 13]) / scale, rtol=1e-13, atol=0)
    got = np.array([[float(x) for x in line.split(",")[-3:]] for line in _out_file(tmp_path / "heat", "surface.").splitlines()[1:]])
    assert len(got) == len(ids)
    _same(got[:, 1], table[:, 1], "surface.*: T")
    assert np.allclose(got[:, 0], qw, rtol=1e-14, atol=0) and np.allclose(got[:, 2], st, rtol=1e-13, atol=0)
    # without the new flags: byte for byte what the viscous run writes
    plain_flags = [f"--viscosity={ve.DRIVER_MU!r}", "--no-slip", "--viscous-levels", "8", "--output-variables", "--output-loads", "--loads-friction", "--output-surface"]
    _run_driver(tmp_path / "plain", case, plain_flags, K)
    em = ve.ViscousOracle(oracle, case, mu=ve.DRIVER_MU, wall=1, viscous_levels="all")
    rc, _ = em.cycles(K)
    assert rc == 0 and (tmp_path / "plain" / "out" / name).read_bytes() == fse.render_variables(em.variables(0)).encode()
    em.close()
    assert _out_file(tmp_path / "plain", "surface_loads").splitlines()[0].endswith(",CMzv")
    assert _out_file(tmp_path / "plain", "surface.").splitlines()[0].endswith(",Cfz")
    # the errors: status 1 right after parsing
    base = [f"--viscosity={ve.DRIVER_MU!r}", "--no-slip"]
    for bad in (["--wall-temperature", "1.0"], [f"--viscosity={ve.DRIVER_MU!r}", "--wall-temperature", "1.0"], base + ["--wall-temperature", "0"],
                base + ["--wall-temperature-ratio", "-1"], base + ["--wall-heat-flux", "nan"], base + ["--wall-temperature", "1.0", "--wall-heat-flux", "0.1"],
                base + ["--wall-temperature", "1.0", "--wall-temperature-ratio", "1.5"], base + ["--output-loads", "--loads-heat"],
                base + ["--viscous-levels", "0", "--wall-heat-flux", "0.1"],
                base + ["--wall-heat-flux", "0.1", "--gpus", "2", "--gpus-share-device"],
                base + ["--output-loads", "--loads-friction", "--loads-heat", "--gpus", "2", "--gpus-share-device"]):
        r = _run_driver(tmp_path / "bad", case, ["--output-variables"] + bad, K, ok=False)
        assert r.returncode == 1 and "ERROR" in r.stderr, bad
        assert not os.listdir(tmp_path / "bad" / "out"), bad
