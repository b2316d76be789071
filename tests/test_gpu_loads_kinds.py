"""GPU tests of what the three loads kinds share on one solver (the pressure six, the twelve with the friction six, the fourteen
with Q and A): the reference point and a synchronous call's result in one device buffer, one history per kind, one launch and
one read-back path, and mgcfd_advance's six-wide rows through the same held rows as the wider ones.  Everything bit for bit
against a twin solver brought to the same state; the kinds against the emulators are tests/test_gpu_surface_loads.py,
tests/test_gpu_friction_loads.py and tests/test_gpu_wall_heat.py.  Lattice A of fas_emulator at fle.GPU_MU's viscosity (54
solid-wall edges on level 0), whose runs tests/test_host_friction_loads.py and tests/test_host_wall_heat.py keep valid."""
import numpy as np
import pytest

import dual_time_emulator as dte
import fas_emulator as fe
import free_stream_emulator as fse
import friction_loads_emulator as fle
import viscous_emulator as ve
import wall_heat_emulator as whe

pytestmark = pytest.mark.gpu

REF = (0.25, -0.125, 0.375)
K = 2                                   # cycles per history: two rows, so a row index that stays at 0 shows
KINDS = {6: {}, 12: {"friction": True}, 14: {"heat": True}}
RING = 4096                             # mgcfd_solver::kRmsRing, the rows a history holds


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(got - want).max():.3e}\n{got}\n{want}"


_lattice = {}


def _lattice_a(isothermal=False, step=whe.RUN_STEP):
    """A fresh solver on lattice A from the perturbed start state with the viscous terms and no-slip walls on every level;
    isothermal: a hot wall, so that Q does not vanish."""
    import mgcfd
    if not _lattice:
        mg = fle.generated("A")
        _lattice["A"] = (mgcfd.generated_to_levels(mg), mg.mesh_variant)
    s = mgcfd.Solver.from_arrays(*_lattice["A"])
    s.set_time_step(*step)
    s.set(0, "variables", ve.start_state(s.nel(0), s.far_field()[:5]))
    s.set_viscous(fle.GPU_MU["A"], ve.PRANDTL, True, ve.VISCOUS_CFL, s.num_levels)
    if isothermal:
        s.set_wall_temperature("isothermal", whe.setting_value(s.far_field(), whe.ISOTHERMAL, whe.TW_RATIOS[0]))
    return s


def _state(s):
    return [s.get(l, "variables") for l in range(s.num_levels)]


def test_kinds_interleaved_on_one_solver():
    """Synchronous loads of six, fourteen, twelve and six, then run_cycles(K, loads=True) of six, fourteen, twelve and six on ONE
    solver: every result is the same call's on a fresh twin brought to the same state (which made no call of another kind before
    it), the twelve are the first twelve of the fourteen and the pressure six columns 0 to 5 of both."""
    s = _lattice_a(isothermal=True)
    s.run_cycles(1)
    # the twin of a synchronous call: the same cycle, then that call alone
    sync = {}
    for width in (6, 14, 12):
        t = _lattice_a(isothermal=True)
        t.run_cycles(1)
        sync[width] = t.surface_loads(0, REF, **KINDS[width])
        t.close()
    assert sync[14][:3].all() and sync[14][6:9].all() and sync[14][12] != 0.0 and sync[14][13] > 0.0, "every column family should be there"
    for width in (6, 14, 12, 6):
        _same(s.surface_loads(0, REF, **KINDS[width]), sync[width], f"synchronous {width} between the other kinds")
    _same(sync[12], sync[14][:12], "the twelve against the first twelve of the fourteen")
    _same(sync[6], sync[14][:6], "the pressure six against the fourteen's")
    # the histories: call number n starts from the state 1 + n * K cycles leave
    calls = (6, 14, 12, 6)
    rows, rms = [], []
    for width in calls:
        r, h = s.run_cycles(K, loads=True, ref_point=REF, **KINDS[width])
        assert h.shape == (K, width)
        rms.append(r); rows.append(h)
    final = _state(s)
    s.close()
    for n, width in enumerate(calls):
        t = _lattice_a(isothermal=True)
        t.run_cycles(1 + n * K)
        r, h = t.run_cycles(K, loads=True, ref_point=REF, **KINDS[width])
        _same(rms[n], r, f"history call {n} ({width} wide): RMS")
        _same(rows[n], h, f"history call {n} ({width} wide): rows")
        if width < 14:
            # ... and the narrower kinds' rows are the front columns of the fourteen-wide rows of the same cycles
            wide = _lattice_a(isothermal=True)
            wide.run_cycles(1 + n * K)
            _, h14 = wide.run_cycles(K, loads=True, ref_point=REF, heat=True)
            _same(rows[n], h14[:, :width], f"history call {n} ({width} wide): against the fourteen-wide rows of the same cycles")
            wide.close()
        if n == len(calls) - 1:
            for l, v in enumerate(_state(t)):
                _same(final[l], v, f"final state, level {l}")
        t.close()


def test_six_wide_advance_history_with_bdf2(oracle, tmp_path):
    """mgcfd_advance with loads under BDF2 (the run of tests/test_gpu_friction_loads.py's twelve-wide test): row k is
    mgcfd_surface_loads after physical step k on a twin stepped one step at a time; RMS and final state are the twin's and those of
    mgcfd_advance without loads."""
    steps, cycles = ve.DUAL_STEPS + 1, ve.DUAL_CYCLES
    dt = dte.pick_dt(oracle, fe.write_lattice("A", tmp_path), "local", 1.0)
    runs = {}
    for name in ("plain", "twin", "history"):
        s = _lattice_a(step=("local", 1.0))
        s.set_dual_time(dt)
        s.dual_time_order(2)
        if name == "plain":
            rms, rows = s.advance(steps, cycles), None
        elif name == "twin":
            rms, rows = np.zeros((steps, cycles)), np.zeros((steps, 6))
            for k in range(steps):
                rms[k] = s.advance(1, cycles)[0]
                rows[k] = s.surface_loads(0, REF)
        else:
            rms, rows = s.advance(steps, cycles, loads=True, ref_point=REF)
            assert rows.shape == (steps, 6)
            _same(rows[-1], s.surface_loads(0, REF), "advance: the last row against the synchronous call")
        assert s.dual_time()["levels"] == 2
        runs[name] = (rms, rows, _state(s))
        s.close()
    for name in ("twin", "history"):
        _same(runs[name][0], runs["plain"][0], f"advance {name}: RMS")
        for l, v in enumerate(runs[name][2]):
            _same(v, runs["plain"][2][l], f"advance {name}: variables, level {l}")
    _same(runs["history"][1], runs["twin"][1], "advance: history rows")
    assert runs["history"][1][:, :3].all()


def _fvcorr(mode, cfl, dt):
    """The single-level golden from its far field, as tests/test_gpu_dual_time.py starts it."""
    import mgcfd
    case = "fvcorr_1lvl"
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    mesh.close()
    s.set_time_step(mode, cfl)
    s.set(0, "variables", dte.start_state(case, s.far_field()[:5], s.nel(0)))
    s.set_dual_time(dt)
    return s


def test_six_wide_advance_history_fills_the_ring():
    """As many steps of one cycle as the history holds rows — the most one call takes: MGCFD_MAX_ADVANCE_CYCLES is the history's
    length, so a call never holds more rows than fit and one step more is refused before anything runs.  The rows are read back
    when the history is full: the last row is the synchronous call on the final state and row 0 a twin's first step."""
    import mgcfd
    mode, cfl, dt = "global", 0.5, dte.GPU_DT["fvcorr_1lvl"]["global05"]
    s = _fvcorr(mode, cfl, dt)
    start = s.get(0, "variables")
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.advance(RING + 1, 1, loads=True, ref_point=REF)
    assert e.value.code == 1 and f"at most {RING} cycles per call" in str(e.value)
    _same(s.get(0, "variables"), start, "the state after the refusal")
    rms, rows = s.advance(RING, 1, loads=True, ref_point=REF)
    assert rows.shape == (RING, 6) and rms.shape == (RING, 1) and np.isfinite(rms).all()
    _same(rows[RING - 1], s.surface_loads(0, REF), "the history's last row against the synchronous call on the final state")
    s.close()
    t = _fvcorr(mode, cfl, dt)
    t.advance(1, 1)
    first = t.surface_loads(0, REF)
    t.close()
    assert first[:3].any() and np.isfinite(rows).all()
    _same(rows[0], first, "row 0 against the twin's first step")
    assert not np.array_equal(_bits(rows[RING - 1]), _bits(rows[0])), "the flow should have moved"


@pytest.mark.parametrize("cfl,steps,cycles,failing", [(6.0, 3, 4, 0), (2.5, 4, 2, 1)])
def test_six_wide_advance_keeps_completed_rows_on_an_invalid_state(cfl, steps, cycles, failing):
    """The invalid state of tests/test_gpu_dual_time.py inside advance with loads (local CFL 6.0: the first step fails), and the
    same at local CFL 2.5, where the dual-time emulator finds the second step invalid: the steps that completed keep their rows (a
    twin's synchronous calls), the failing step and every later one are NaN, and .step names the failing step."""
    import mgcfd
    s = _fvcorr("local", cfl, 10.0)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.advance(steps, cycles, loads=True, ref_point=REF)
    step = e.value.step
    assert e.value.code in (4, 5, 6) and step == failing and step == s.dual_time()["invalid_step"]
    assert e.value.loads.shape == (steps, 6) and e.value.rms.shape == (steps, cycles)
    s.close()
    assert np.isnan(e.value.loads[step:]).all() and np.isnan(e.value.rms[step, -1]) and np.isnan(e.value.rms[step + 1:]).all()
    assert np.isfinite(e.value.loads[:step]).all() and (step == 0 or e.value.loads[:step, :3].any())
    t = _fvcorr("local", cfl, 10.0)
    for k in range(step):
        _same(e.value.rms[k], t.advance(1, cycles)[0], f"step {k}: RMS")
        _same(e.value.loads[k], t.surface_loads(0, REF), f"step {k}: row")
    with pytest.raises(mgcfd.MgcfdError) as again:
        t.advance(1, cycles)
    assert again.value.code == e.value.code
    t.close()
