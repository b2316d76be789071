"""Host tests of the wall thermal conditions and the heat loads (no GPU): what the numpy emulator (tests/wall_heat_emulator.py)
computes on cases with a derived answer — a gas at rest with a linear temperature over a flat wall — the isothermal wall's bits
behind every writer of a covered level's state, the signs of the heat rate, the free-stream temperatures and the Stanton number
against the package's host functions, and that every run of tests/test_gpu_wall_heat.py stays valid on the CPU."""
import numpy as np
import pytest

import dual_time_emulator as dte
import fas_emulator as fe
import friction_loads_emulator as fle
import sa_emulator as sae
import viscous_emulator as ve
import wall_heat_emulator as whe

MU, PRANDTL = 0.3, 0.72
RHO, T0, SLOPE = 1.3, 0.9, 0.37
K = whe.GPU_CYCLES


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _far_field():
    import mgcfd
    return mgcfd.free_stream_constants(1.2, 0.0)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("wall_heat_cases")
    out = {key: fle.write_case(key, d) for key in whe.GENERATED if key != "A"}
    out["A"] = fe.write_lattice("A", d)
    return out


def test_linear_temperature_over_a_flat_wall():
    """Derived: on the 9^3 hull-wall box every wall edge has weights (0, 0, +A_e) (fvcorr: into the fluid); a gas at rest with
    T = T0 + c z has q = (0, 0, kappa c) at every node, so Q = -kappa c A with A = 1: the heat the fluid receives from the wall.
    To 1e-12 relative, the tolerance tests/test_host_friction_loads.py holds Fv to on the same box; the table's h add up to Q."""
    import mgcfd
    level = mgcfd.generated_to_levels(fle.hull_wall_box(9))[0]
    T = T0 + SLOPE * level["coords"][:, 2]
    W = np.zeros((level["nel"], 5))
    W[:, 0] = RHO
    W[:, 4] = (RHO * T) / (ve.GAMMA - 1.0)
    S = whe.node_stresses(W, level["edges"], level, MU, PRANDTL)
    out = whe.surface_loads14(W, level["edges"], level, _far_field(), (0.0, 0.0, 0.0), S)
    want = -float(ve.conductivity(MU, PRANDTL)) * SLOPE
    print("Q", out[12], "against", want, "A", out[13])
    assert abs(out[13] - 1.0) <= 1e-12
    assert abs(out[12] - want) <= 1e-12 * abs(want)
    assert not out[6:12].any(), "a gas at rest has no friction"
    ids, table = whe.wall_heat(W, level["edges"], level, S)
    assert table.shape == (81, 3) and np.array_equal(ids, np.flatnonzero(level["coords"][:, 2] == 0.0))
    assert abs(table[:, 0].sum() - out[12]) <= 1e-12 * abs(want)
    assert abs(table[:, 2].sum() - 1.0) <= 1e-12 and np.abs(table[:, 1] - T0).max() <= 1e-14
    # the first twelve are the friction loads' bits; without the stresses Q is +0.0 and A is still summed
    want12 = fle.surface_loads12(W, level["edges"], level, _far_field(), (0.0, 0.0, 0.0), (MU, PRANDTL))
    assert np.array_equal(_bits(out[:12]), _bits(want12))
    off = whe.surface_loads14(W, level["edges"], level, _far_field(), (0.0, 0.0, 0.0), None)
    assert np.array_equal(_bits(off[6:13]), _bits(np.zeros(7))) and np.array_equal(_bits(off[13:]), _bits(out[13:]))
    # the wall heat flux and the Stanton number of the package against the emulator's
    qw, st = mgcfd.heat_coefficients(_far_field(), table, t_wall=T0)
    want_qw, want_st = whe.heat_coefficients(_far_field(), table, t_wall=T0)
    assert np.allclose(qw, want_qw, rtol=1e-15, atol=0) and np.allclose(st, want_st, rtol=1e-14, atol=0)
    assert np.abs(qw - want).max() <= 1e-11 * abs(want)


def test_free_stream_temperature():
    """t_static = p / rho of the far field, t_total = t_static (1 + 0.2 M^2): the package's host call gives the emulator's bits,
    and M recovers the Mach number the constants were made from."""
    import mgcfd
    for mach, alpha in ((1.2, 0.0), (0.8, 2.0), (3.0, -1.0), (0.05, 0.0)):
        ff = mgcfd.free_stream_constants(mach, alpha)
        got, want = mgcfd.free_stream_temperature(ff), whe.free_stream_temperature(ff)
        assert np.array_equal(_bits(got), _bits(want)), (mach, alpha)
        assert abs(got[1] / got[0] - (1.0 + 0.2 * mach * mach)) <= 1e-14 * (1.0 + 0.2 * mach * mach)


class _Checked(whe.WallHeatOracle):
    """WallHeatOracle that checks the definition behind every application of the wall rule and every sweep."""

    applied = swept = 0

    def apply_wall(self, l):
        super().apply_wall(l)
        if self.viscous_on(l) and self.wall and self.wt_mode == whe.ISOTHERMAL:
            v, w = self._var(l), self.wall_nodes[l]
            assert np.array_equal(_bits(v[w, 4]), _bits(v[w, 0] * (np.float64(self.wt_value) / (ve.GAMMA - 1.0))))
            assert np.array_equal(_bits(v[w, 1:4]), _bits(np.zeros((len(w), 3))))
            self.applied += 1

    def _sweep(self, l):
        rc = super()._sweep(l)
        if rc == 0 and self.viscous_on(l) and self.wall and self.wt_mode == whe.ISOTHERMAL:
            w = self.wall_nodes[l]
            v, old = self._var(l), self.oc.array(l, "old_variables").reshape(-1, 5)
            res = self.oc.array(l, "residuals").reshape(-1, 5)
            assert np.array_equal(_bits(res[w, 4]), _bits(v[w, 4] - old[w, 4]))
            assert np.array_equal(_bits(res[w, 1:4]), _bits(0.0 - old[w, 1:4]))
            self.swept += 1
        return rc


@pytest.mark.parametrize("fas", [False, True])
def test_isothermal_wall_bits_after_every_writer(fas, oracle, cases):
    """Lattice A, all levels: the energy of every isothermal wall node is density * ew in bits, and its momentum +0.0, behind every
    stage, restriction and prolongation (the plain legs and FAS's, W0 included); the energy residual of a sweep is
    variables - old_variables in bits."""
    em = _Checked(oracle, cases["A"], "local", 1.0, fas=fas)
    v = em._var(0)
    v[:] = ve.start_state(len(v), em.ff17[:5])
    em.set_viscous(ve.CELL_RE_MU, ve.PRANDTL, 1, ve.VISCOUS_CFL, "all")
    tw = whe.TW_RATIOS[0] * whe.free_stream_temperature(em.ff17)[0]
    em.set_wall_temperature("isothermal", tw)
    rc, rms = em.cycles(K)
    assert rc == 0 and np.isfinite(rms).all()
    # the setter on three levels; per cycle the sweeps of levels 0, 1, 2, 1 (three stages each), two restrictions, two prolongations
    assert em.applied == 3 + K * (4 * 3 + 4) and em.swept == K * 4
    ew = np.float64(tw) / (ve.GAMMA - 1.0)
    for l in range(em.n):
        w = em.wall_nodes[l]
        assert np.array_equal(_bits(em._var(l)[w, 4]), _bits(em._var(l)[w, 0] * ew)), f"level {l}"
        assert np.array_equal(_bits(em.wall_temperatures(l)), _bits(em.wall_temperatures(l))) and np.abs(em.wall_temperatures(l) - tw).max() <= 4e-16 * tw
        if fas and l >= 1:
            assert np.array_equal(_bits(em.W0[l][w, 4]), _bits(em.W0[l][w, 0] * ew)) and not em.W0[l][w, 1:4].any()
    em.close()


def _hull_run(oracle, case, mode, value):
    em = whe.WallHeatOracle(oracle, case, *whe.RUN_STEP)
    em.set_viscous(whe.RUN_MU["hull9"], ve.PRANDTL, 1, ve.VISCOUS_CFL, "all")
    em.set_wall_temperature(mode, value)
    rc, rms = em.cycles(K)
    assert rc == 0 and np.isfinite(rms).all()
    out = em.heat_loads(0), em.heat_table(0)[1], em.wall_temperatures(0).mean()
    em.close()
    return out


def test_signs_on_the_hull_wall_box(oracle, cases):
    """From the free stream: a wall at 1.5 T_inf heats the gas (Q > 0), one at 0.5 T_inf cools it (Q < 0); a positive wall heat
    flux raises the wall nodes' mean temperature above the adiabatic run's.  The table's h add up to Q."""
    t_inf = whe.free_stream_temperature(_far_field())[0]
    hot, table_hot, _ = _hull_run(oracle, cases["hull9"], "isothermal", whe.TW_RATIOS[0] * t_inf)
    cold, table_cold, _ = _hull_run(oracle, cases["hull9"], "isothermal", whe.TW_RATIOS[1] * t_inf)
    adiabatic, _, t_adiabatic = _hull_run(oracle, cases["hull9"], "adiabatic", 0.0)
    flux, _, t_flux = _hull_run(oracle, cases["hull9"], "heat-flux", whe.QW)
    print("Q hot", hot[12], "cold", cold[12], "adiabatic", adiabatic[12], "A", hot[13], "mean wall T", t_adiabatic, t_flux)
    assert hot[12] > 0.0 and cold[12] < 0.0
    assert abs(hot[13] - 1.0) <= 1e-12 and hot[13] == cold[13] == adiabatic[13]
    assert abs(table_hot[:, 0].sum() - hot[12]) <= 1e-12 * abs(hot[12]) and abs(table_cold[:, 0].sum() - cold[12]) <= 1e-12 * abs(cold[12])
    assert t_flux > t_adiabatic


def test_going_back_to_adiabatic_and_the_setter_order(oracle, cases):
    """Either order of the two setters gives the same bits; going back to adiabatic leaves the state as it stands; the setting has
    no effect under slip walls."""
    a = whe.configured(oracle, cases["A"], ve.CELL_RE_MU, "all", whe.ISOTHERMAL, whe.TW_RATIOS[0], order=(0, 1))
    b = whe.configured(oracle, cases["A"], ve.CELL_RE_MU, "all", whe.ISOTHERMAL, whe.TW_RATIOS[0], order=(1, 0))
    for l in range(a.n):
        assert np.array_equal(_bits(a.variables(l)), _bits(b.variables(l)))
    before = [a.variables(l) for l in range(a.n)]
    a.set_wall_temperature("adiabatic")
    for l in range(a.n):
        assert np.array_equal(_bits(a.variables(l)), _bits(before[l]))
    a.close(); b.close()
    slip = whe.WallHeatOracle(oracle, cases["A"], "local", 1.0)
    slip._var(0)[:] = ve.start_state(len(slip._var(0)), slip.ff17[:5])
    start = slip.variables(0)
    slip.set_viscous(ve.CELL_RE_MU, ve.PRANDTL, 0, ve.VISCOUS_CFL, "all")
    slip.set_wall_temperature("isothermal", 1.0)
    assert np.array_equal(_bits(slip.variables(0)), _bits(start))
    slip.close()


def _valid(em, what):
    rc, rms = em.cycles(K)
    assert rc == 0 and np.isfinite(rms).all(), what
    for l in range(em.n):
        v = em.variables(l)
        assert np.isfinite(v).all() and (v[:, 0] > 0.0).all() and (v[:, 4] > 0.0).all(), f"{what}: level {l}"
    em.close()


@pytest.mark.parametrize("key,lv,mode,x", whe.gpu_runs())
def test_the_plain_gpu_runs_stay_valid(key, lv, mode, x, oracle, cases):
    _valid(whe.configured(oracle, cases.get(key, key), whe.RUN_MU[key], lv, mode, x), f"{key} levels={lv} mode={mode} {x}")


@pytest.mark.parametrize("mode,x", [(whe.ISOTHERMAL, whe.TW_RATIOS[0]), (whe.HEAT_FLUX, whe.QW)])
def test_the_composed_gpu_runs_stay_valid(mode, x, oracle, cases):
    for name, smoothing, jst_levels, fas in whe.COMPOSED:
        _valid(whe.configured(oracle, cases["A"], whe.RUN_MU["A"], "all", mode, x, smoothing, jst_levels, fas), f"{name} mode={mode}")
    _valid(whe.configured(oracle, cases["A"], whe.RUN_MU["A"], "all", mode, x, model=whe.SA_MODEL), f"SA mode={mode}")


def test_the_dual_time_gpu_run_stays_valid(oracle, cases):
    em = whe.configured(oracle, cases["A"], whe.RUN_MU["A"], "all", whe.ISOTHERMAL, whe.TW_RATIOS[0], step=("local", 1.0))
    em.set_dual_time(dte.pick_dt(oracle, cases["A"], "local", 1.0))
    em.set_order(2)
    rc, rms = em.advance(whe.DUAL_STEPS, whe.DUAL_CYCLES)
    assert rc == 0 and np.isfinite(rms).all()
    em.close()


def test_the_polar_and_the_driver_runs_stay_valid(oracle):
    """tests/test_gpu_wall_heat.py's polar and drop-in binary runs on the golden m6_2lvl: from the far field of Mach 0.8, a wall at
    TW_RATIOS[0] times its static temperature."""
    import free_stream_emulator as fse
    import mgcfd
    case, alphas, mach = fse.POLAR_CASE, fse.POLAR_ALPHAS, fse.POLAR_MACH
    tw = whe.TW_RATIOS[0] * whe.free_stream_temperature(fse.free_stream_constants(mach, alphas[0]))[0]
    em = whe.WallHeatOracle(oracle, case, mu=ve.DRIVER_MU, wall=1, viscous_levels=2)
    em.set_wall_temperature("isothermal", tw)
    for k, al in enumerate(alphas):
        em.set_far_field(fse.free_stream_constants(mach, al), reinitialise=(k == 0))
        rc, rms = em.cycles(K)
        assert rc == 0 and np.isfinite(rms).all(), al
    em.close()
    ff = mgcfd.free_stream_constants(0.8, 2.0)
    em = whe.WallHeatOracle(oracle, "m6_2lvl", mu=ve.DRIVER_MU, wall=1, viscous_levels="all")
    em.set_wall_temperature("isothermal", whe.TW_RATIOS[0] * mgcfd.free_stream_temperature(ff)[0])
    em.set_far_field(ff, reinitialise=True)
    _valid(em, "driver")


def test_wall_counts_of_the_gpu_meshes(oracle, cases):
    """What tests/test_gpu_wall_heat.py relies on: hull9 has 81 wall nodes (one chunk, one workgroup), box17 414 wall edges on 278
    wall nodes (two chunks of 256 edges, two workgroups of the node kernels); lattice A has walls on levels 0 and 1."""
    for key, edges, nodes in (("hull9", 81, 81), ("box17", 414, 278)):
        em = whe.WallHeatOracle(oracle, cases[key])
        assert em.oc.levels[0].n_boundary == edges and len(em.wall_nodes[0]) == nodes and (em.area[0] > 0.0).all()
        em.close()
    em = whe.WallHeatOracle(oracle, cases["A"])
    assert [em.oc.levels[l].n_boundary for l in range(em.n)][:2] == [54, 6]
    em.close()
