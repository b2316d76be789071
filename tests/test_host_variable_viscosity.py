"""Host tests of the viscosity model (no GPU): the numpy emulator (tests/variable_viscosity_emulator.py) keeps every combination
tests/test_gpu_variable_viscosity.py runs valid and changes S at every node; on the uniform fvcorr lattice of
tests/test_host_viscous.py Sutherland's law, a Couette field, a pure shear under Smagorinsky and a uniform field give the derived
values; the viscous flux still sums to zero; an all-zero caller's field under the constant law reproduces ViscousOracle's
stresses in bits; and the ABI surface is in the header, the library and the Python table."""
import os
import re

import numpy as np
import pytest

import fas_emulator as fe
import variable_viscosity_emulator as vve
import viscous_emulator as ve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MU = 0.3
RHO, P0 = 1.3, 0.9
REL = 1e-12          # exact-arithmetic identities evaluated in a few dozen roundings: a factor ~1e3 over that


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("variable_viscosity_lattices")
    return {name: fe.write_lattice(name, d) for name in fe.LATTICES}


@pytest.fixture(scope="module")
def box():
    """tests/test_host_viscous.py's lattice: unjittered, unpermuted 9^3 with fvcorr weights; h = 1/8."""
    from mgcfd import meshgen
    n = 9
    level = meshgen.make_box_level(n, permute=False)
    edges, n_int, _, _ = meshgen.to_edge_arrays(level, meshgen.MESH_CODES["fvcorr"])
    e = edges[:n_int]
    to, frm, N = ve.interleaved(np.asarray(e["a"], dtype=np.int64), np.asarray(e["b"], dtype=np.int64), e)
    ijk = np.rint(level.coords * (n - 1)).astype(np.int64)
    layer = np.minimum(ijk, n - 1 - ijk).min(axis=1)
    cb = vve.tse.libm_cbrt(level.volumes)
    return level.coords, level.volumes, to, frm, N, layer, cb * cb


def _state(vel, T):
    p = RHO * T
    W = np.empty((len(vel), 5))
    W[:, 0] = RHO
    W[:, 1:4] = RHO * vel
    W[:, 4] = p / (ve.GAMMA - 1.0) + 0.5 * RHO * (vel * vel).sum(axis=1)
    return W


def _mu_of(T, t_ref, s=vve.SUTHERLAND_S, mu=MU):
    r = float(T) / float(t_ref)
    return mu * r ** 1.5 * (1.0 + s) / (r + s)


def test_sutherland_formula():
    """mu(T) equals the formula in Python floats at T = t_ref (where it is mu) and at 2 t_ref."""
    t_ref = 0.7
    m = vve.Model("sutherland", t_ref)
    got = vve.viscosity(m, MU, np.array([t_ref, 2.0 * t_ref]))
    assert abs(got[0] - MU) <= REL * MU
    assert abs(got[0] - _mu_of(t_ref, t_ref)) <= REL * MU and abs(got[1] - _mu_of(2.0 * t_ref, t_ref)) <= REL * MU
    assert got[1] > got[0]
    assert np.array_equal(_bits(vve.viscosity(vve.Model(), MU, np.array([0.3, 5.0]))), _bits(np.full(2, MU)))


def test_couette_with_a_temperature_gradient(box):
    """u = a y with T = T0 (1 + c y): txy_i = mu(T_i) a at interior nodes."""
    xyz, vol, to, frm, N, layer, d2 = box
    a, T0, c = 0.4, P0 / RHO, 0.5
    y = xyz[:, 1]
    vel = np.zeros((len(xyz), 3))
    vel[:, 0] = a * y
    T = T0 * (1.0 + c * y)
    m = vve.Model("sutherland", T0)
    S, mut = vve.stresses(_state(vel, T), to, frm, N, vol, MU, ve.PRANDTL, m, d2)
    inner = layer >= 1
    want = np.array([_mu_of(t, T0) for t in T]) * a
    rel = np.abs(S[inner, 6] - want[inner]).max() / np.abs(want[inner]).max()
    print("Couette: txy against mu(T) a, relative", rel)
    assert rel <= REL and not mut.any()
    assert np.ptp(want[inner]) > 0.01 * want[inner].max()


def test_pure_shear_under_smagorinsky(box):
    """u = a y at uniform rho and T: mut_i = rho (cs h)^2 |a| with h the lattice spacing, at interior nodes."""
    xyz, vol, to, frm, N, layer, d2 = box
    h = 1.0 / 8.0
    inner = layer >= 1
    for a in (0.4, -0.4):
        vel = np.zeros((len(xyz), 3))
        vel[:, 0] = a * xyz[:, 1]
        m = vve.Model("constant", 1.0, eddy="smagorinsky")
        S, mut = vve.stresses(_state(vel, np.full(len(xyz), P0 / RHO)), to, frm, N, vol, MU, ve.PRANDTL, m, d2)
        want = RHO * (vve.SMAGORINSKY_CS * h) ** 2 * abs(a)
        rel = np.abs(mut[inner] - want).max() / want
        print("pure shear: mut against rho (cs h)^2 |a|, relative", rel)
        assert rel <= REL
        assert np.abs(S[inner, 6] - (MU + want) * a).max() <= REL * (MU + want) * abs(a)


def test_uniform_field_gives_zero(box):
    """A uniform field: mut = +0.0 and zero stresses in bits."""
    xyz, vol, to, frm, N, layer, d2 = box
    vel = np.tile(np.array([0.3, -0.2, 0.1]), (len(xyz), 1))
    m = vve.Model("sutherland", P0 / RHO, eddy="smagorinsky")
    S, mut = vve.stresses(_state(vel, np.full(len(xyz), P0 / RHO)), to, frm, N, vol, MU, ve.PRANDTL, m, d2)
    assert not _bits(mut).any() and not _bits(S[:, 3:]).any()


def test_conservation(oracle, lattices):
    """The viscous flux still sums to zero over a level in each component, relative to the sum of magnitudes."""
    em = vve.configured(oracle, lattices["A"], 0.05, "local", 1.0, 0, 1, vve.COMBINED)
    S, V = em.viscous_terms(0)
    total, size = np.abs(V.sum(axis=0)), np.abs(V).sum(axis=0)
    print("sum V", V.sum(axis=0), "sum |V|", size)
    assert (size[1:] > 0.0).all() and (total[1:] <= REL * size[1:]).all() and not V[:, 0].any()
    em.close()


def test_zero_field_under_the_constant_law_is_viscous_oracle(oracle, lattices):
    """eddy 1 with an all-zero field under law 0: S[:, 3:9] equals ViscousOracle's in bits (mu + 0.0 = mu); the heat flux agrees
    to a rounding or two (kappa is formed differently)."""
    want = ve.configured(oracle, lattices["A"], ve.CELL_RE_MU, "local", 1.0, 1, "all")
    em = vve.configured(oracle, lattices["A"], ve.CELL_RE_MU, "local", 1.0, 1, "all", ("constant", "field"))
    for l in range(em.n):
        assert not em.eddy_viscosity(l).any()
        S, _ = em.viscous_terms(l)
        S0, _ = want.viscous_terms(l)
        assert np.array_equal(_bits(S[:, :9]), _bits(S0[:, :9])) and S0[:, 3:9].any()
        assert np.allclose(S[:, 9:], S0[:, 9:], rtol=1e-15, atol=0)
    em.close(); want.close()


def _constant_S(oracle, case, mu, mode, cfl, wall, lv):
    em = ve.configured(oracle, case, mu, mode, cfl, wall, lv)
    S = em.viscous_terms(0)[0]
    em.close()
    return S


def test_every_gpu_combination(oracle, lattices):
    """Every combination of the GPU runs (ve.gpu_combinations() x MODELS) stays valid for GPU_CYCLES cycles, and from the start
    state S[:, 3:] differs in bits from the constant-viscosity S at more than half of level 0's nodes (measured: all of them).  On
    lattice A at CELL_RE_MU the limit binds at every node-sweep and the state differs from the constant-viscosity run's."""
    combos = ve.gpu_combinations()
    assert len(combos) * len(vve.MODELS) == 144
    plain_state = {}
    for key, mu, mode, cfl, wall, lv in combos:
        case = lattices.get(key, key)
        S0 = _constant_S(oracle, case, mu, mode, cfl, wall, lv)
        for model in vve.MODELS:
            em = vve.configured(oracle, case, mu, mode, cfl, wall, lv, model)
            S = em.viscous_terms(0)[0]
            frac = float((_bits(S[:, 3:]) != _bits(S0[:, 3:])).any(axis=1).mean())
            rc, rms = em.cycles(ve.GPU_CYCLES)
            assert rc == 0 and np.isfinite(rms).all(), (key, mu, mode, wall, lv, model)
            assert frac > 0.5, (key, mu, model, frac)
            if key == "A" and mu == ve.CELL_RE_MU and mode == "local":
                assert em.limited[0][1] == 0 and em.limited[0][0] == ve.GPU_CYCLES * em.oc.levels[0].nel, (model, em.limited)
                k = (mode, cfl, wall, lv)
                if k not in plain_state:
                    p = ve.configured(oracle, case, mu, mode, cfl, wall, lv)
                    assert p.cycles(ve.GPU_CYCLES)[0] == 0
                    plain_state[k] = p.variables(0)
                    p.close()
                assert (_bits(em.variables(0)) != _bits(plain_state[k])).any(axis=1).all(), model
            em.close()
    # the eddy-1 field on lattice A, and the composed runs with the combined model
    em = vve.configured(oracle, lattices["A"], ve.CELL_RE_MU, "local", 1.0, 1, "all", ("constant", "field"), field=True)
    assert em.cycles(ve.GPU_CYCLES)[0] == 0
    em.close()


def test_composed_runs_stay_valid(oracle, lattices):
    import dual_time_emulator as dte
    for name, mode, cfl, smoothing, jst_levels, order, fas in ve.COMPOSED:
        em = vve.configured(oracle, lattices["A"], ve.CELL_RE_MU, mode, cfl, 1, "all", vve.COMBINED, smoothing, jst_levels, fas)
        if order is None:
            rc, rms = em.cycles(ve.GPU_CYCLES)
        else:
            em.set_dual_time(dte.pick_dt(oracle, lattices["A"], mode, cfl))
            em.set_order(order)
            rc, rms = em.advance(ve.DUAL_STEPS, ve.DUAL_CYCLES)
        assert rc == 0 and np.isfinite(rms).all(), name
        em.close()


def test_array_lifetime_in_the_emulator(oracle, lattices):
    """The eddy-viscosity array holds +0.0 when it comes into being and when the eddy mode changes; a stress launch writes it
    under Smagorinsky; switching the terms off and on keeps the model and starts from +0.0 again."""
    em = vve.configured(oracle, lattices["A"], ve.CELL_RE_MU, "local", 1.0, 1, 1, vve.COMBINED)
    assert not em.eddy_viscosity(0).any()
    em.stage_fluxes(0)
    first = em.eddy_viscosity(0)
    assert first.all()
    em.set_viscous(0.0, levels=0)
    em.set_viscous(ve.CELL_RE_MU, ve.PRANDTL, 1, ve.VISCOUS_CFL, 1)
    assert em.model.eddy == 2 and not em.eddy_viscosity(0).any()
    em.set_viscosity_model(eddy="field")
    em.set_eddy_viscosity(0, first)
    em.set_viscosity_model(law="sutherland", eddy="field")
    assert np.array_equal(em.eddy_viscosity(0), first)
    em.set_viscosity_model(eddy="smagorinsky")
    assert not em.eddy_viscosity(0).any()
    em.close()


def test_symbols_defaults_and_array_id():
    import mgcfd
    from mgcfd import api
    header = open(os.path.join(ROOT, "include", "mgcfd.h")).read()
    lib = mgcfd.load_library()
    for name in ("mgcfd_set_viscosity_model", "mgcfd_get_viscosity_model"):
        assert name in mgcfd.EXPORTED_SYMBOLS and hasattr(lib, name) and f"int {name}(" in header
    for macro, value, mine in (("MGCFD_SUTHERLAND_S", api.SUTHERLAND_S, vve.SUTHERLAND_S), ("MGCFD_SMAGORINSKY_CS", api.SMAGORINSKY_CS, vve.SMAGORINSKY_CS),
                               ("MGCFD_PRANDTL_TURBULENT", api.PRANDTL_TURBULENT, vve.PRANDTL_TURBULENT)):
        assert float(re.search(rf"#define {macro} (\S+)", header).group(1)) == value == mine
    assert vve.SUTHERLAND_S == float("%.4f" % (110.4 / 288.15))
    for names, table in ((("MGCFD_VISCOSITY_CONSTANT", "MGCFD_VISCOSITY_SUTHERLAND"), vve.LAWS),
                         (("MGCFD_EDDY_NONE", "MGCFD_EDDY_FIELD", "MGCFD_EDDY_SMAGORINSKY"), vve.EDDIES)):
        for name, value in zip(names, sorted(table.values())):
            assert re.search(rf"{name} = {value}\b", header), name
    assert api._VISCOSITY_LAWS == vve.LAWS and api._EDDY_MODES == vve.EDDIES
    enum = header[header.index("enum { MGCFD_ARR_VARIABLES"):]
    enum = re.sub(r"/\*.*?\*/", "", enum[:enum.index("};")], flags=re.S)
    ids = re.findall(r"MGCFD_ARR_[A-Z0-9_]+", enum)
    assert ids.index("MGCFD_ARR_EDDY_VISCOSITY") == api.ARR["eddy_viscosity"] == 15 == len(ids) - 1
    assert api.NCOLS["eddy_viscosity"] == 1
    assert lib.mgcfd_abi_version() == 1
