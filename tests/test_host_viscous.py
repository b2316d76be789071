"""Host tests of the laminar viscous terms (no GPU): the numpy emulator (tests/viscous_emulator.py) is FasOracle bit for bit with
the terms off; on a uniform lattice the node gradients of a linear field are exact at every node, hull included, the viscous
flux of a constant stress vanishes, quadratic fields give the derived second derivatives, the viscous flux sums to zero over the
level, and the no-slip wall holds behind every writer of variables; and the parameters of tests/test_gpu_viscous.py are fixed
here: every combination stays valid, each case's viscosity is the smallest power of ten at which F + V differs from F at more
than half of level 0's nodes, and MGCFD_VISCOUS_CFL is the largest of (0.1, 0.25, 0.5) that keeps the limit binding on lattice A."""
import os
import re

import numpy as np
import pytest

import dual_time_emulator as dte
import fas_emulator as fe
import free_stream_emulator as fse
import viscous_emulator as ve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MU, KAPPA = 0.3, 0.7
RHO, P0 = 1.3, 0.9


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("viscous_lattices")
    return {name: fe.write_lattice(name, d) for name in fe.LATTICES}


def _case(lattices, key):
    return lattices.get(key, key)


@pytest.fixture(scope="module")
def box():
    """An unjittered, unpermuted 9^3 lattice with fvcorr weights: (coords, volumes, to, frm, N, layer [nel]: a node's distance
    from the hull in lattice steps)."""
    from mgcfd import meshgen
    n = 9
    level = meshgen.make_box_level(n, permute=False)
    edges, n_int, _, _ = meshgen.to_edge_arrays(level, meshgen.MESH_CODES["fvcorr"])
    e = edges[:n_int]
    to, frm, N = ve.interleaved(np.asarray(e["a"], dtype=np.int64), np.asarray(e["b"], dtype=np.int64), e)
    ijk = np.rint(level.coords * (n - 1)).astype(np.int64)
    layer = np.minimum(ijk, n - 1 - ijk).min(axis=1)
    return level.coords, level.volumes, to, frm, N, layer


def _state(vel, T):
    """Conserved variables of uniform density RHO, the velocities vel [nel, 3] and the temperatures T [nel] (p = RHO * T)."""
    p = RHO * T
    W = np.empty((len(vel), 5))
    W[:, 0] = RHO
    W[:, 1:4] = RHO * vel
    W[:, 4] = p / (ve.GAMMA - 1.0) + 0.5 * RHO * (vel * vel).sum(axis=1)
    return W


def test_off_is_fas_oracle(oracle):
    """levels = 0 — never on, and switched on and off again before the run — gives FasOracle's bits with FAS on, and the golden
    variables.level0.txt byte for byte with everything off."""
    case = "m6_3lvl"
    want = fe.FasOracle(oracle, case, fas=True)
    rc_w, rms_w = want.cycles(fe.GPU_CYCLES)
    for toggle in (False, True):
        em = ve.ViscousOracle(oracle, case, fas=True)
        if toggle:
            em.set_viscous(1e-3, levels="all", wall=0)
            em.set_viscous(0.0, levels=0)
        rc, rms = em.cycles(fe.GPU_CYCLES)
        assert rc == rc_w == 0 and np.array_equal(_bits(rms), _bits(rms_w))
        for l in range(em.n):
            assert np.array_equal(_bits(em.variables(l)), _bits(want.variables(l)))
            assert np.array_equal(_bits(em.P[l]), _bits(want.P[l])) if l else True
        em.close()
    want.close()
    meta = dict(l.strip().split(" = ") for l in open(os.path.join(fse.GOLDEN, case, "case.txt")))
    em = ve.ViscousOracle(oracle, case)
    assert em.cycles(int(meta["cycles"]))[0] == 0
    assert fse.render_variables(em.variables(0)).encode() == open(os.path.join(fse.GOLDEN, case, "variables.level0.txt"), "rb").read()
    em.close()


def test_linear_velocity_field(box):
    """u = M x + c: G equals M at EVERY node, hull included, to 1e-12 relative; at interior nodes the stress is constant, so
    V[1..3] is below 1e-10 of mu |grad u| h^2 and V[4] = vol * (tau : grad u) to 1e-10 relative."""
    xyz, vol, to, frm, N, layer = box
    M = np.array([[0.3, -0.7, 0.2], [0.5, 0.4, -0.6], [-0.1, 0.8, 0.9]])
    vel = xyz @ M.T + np.array([0.2, -0.3, 0.1])
    W = _state(vel, np.full(len(xyz), P0 / RHO))
    G = ve.gradients(ve.primitives(W)[:, 0:3], to, frm, N, vol)
    err = np.abs(G - M[None, :, :]).max() / np.abs(M).max()
    print("linear field: max |G - M| / max |M| =", err)
    assert err <= 1e-12
    S = ve.stresses(W, to, frm, N, vol, MU, KAPPA)
    V = ve.viscous_flux(S, to, frm, N)
    h = 1.0 / 8.0
    inner = layer >= 1
    scale = MU * np.sqrt((M * M).sum()) * h * h
    print("linear field: max |V[1..3]| / (mu |grad u| h^2) =", np.abs(V[inner, 1:4]).max() / scale)
    assert np.abs(V[inner, 1:4]).max() <= 1e-10 * scale
    div = np.trace(M)
    tau = MU * (M + M.T) - MU * (2.0 / 3.0) * div * np.eye(3)
    want = vol * (tau * M).sum()
    rel = np.abs(V[inner, 4] - want[inner]).max() / np.abs(want[inner]).max()
    print("linear field: V[4] against vol * (tau : grad u), relative", rel)
    assert rel <= 1e-10
    assert not V[:, 0].any()


def test_quadratic_fields(box):
    """Derived, not measured: u = (y^2, 0, 0) at uniform rho and p gives tau_xy = 2 mu y and V[1] = 2 mu vol; T = 1 + y^2 at
    u = 0 gives q_y = 2 kappa y and V[4] = 2 kappa vol, at nodes two or more layers from the hull (the averaged central
    difference is exact for quadratics on a uniform lattice, the hull's one-sided difference is not), to 1e-10 relative."""
    xyz, vol, to, frm, N, layer = box
    deep = layer >= 2
    assert deep.sum() == 5 ** 3
    y = xyz[:, 1]
    vel = np.zeros((len(xyz), 3))
    vel[:, 0] = y * y
    V = ve.viscous_flux(ve.stresses(_state(vel, np.full(len(xyz), P0 / RHO)), to, frm, N, vol, MU, KAPPA), to, frm, N)
    rel = np.abs(V[deep, 1] - 2.0 * MU * vol[deep]).max() / (2.0 * MU * vol[deep]).max()
    print("u = y^2: V[1] against 2 mu vol, relative", rel)
    assert rel <= 1e-10
    V = ve.viscous_flux(ve.stresses(_state(np.zeros((len(xyz), 3)), 1.0 + y * y), to, frm, N, vol, MU, KAPPA), to, frm, N)
    rel = np.abs(V[deep, 4] - 2.0 * KAPPA * vol[deep]).max() / (2.0 * KAPPA * vol[deep]).max()
    print("T = 1 + y^2: V[4] against 2 kappa vol, relative", rel)
    assert rel <= 1e-10
    assert np.abs(V[deep, 1:4]).max() <= 1e-10 * (2.0 * KAPPA * vol[deep]).max()


def test_conservation(oracle, lattices):
    """The two ends of an edge receive exactly opposite terms: the sum of V over all nodes is below 1e-12 of the sum of |V|
    (a perturbed state on lattice A, whose jitter, cavity and noise leave nothing symmetric)."""
    em = ve.configured(oracle, lattices["A"], 0.05, "local", 1.0, 0, 1)
    S, V = em.viscous_terms(0)
    total, size = np.abs(V.sum(axis=0)), np.abs(V).sum(axis=0)
    print("sum V", V.sum(axis=0), "sum |V|", size)
    assert (size[1:] > 0.0).all() and (total[1:] <= 1e-12 * size[1:]).all() and not V[:, 0].any()
    # per edge the two ends' terms are exact negatives: the interleaved terms of pass 2 cancel pairwise
    b = 0.5 * (S[em.vto[0]] + S[em.vfrm[0]])
    f = (b[:, 3] * em.vN[0][:, 0] + b[:, 6] * em.vN[0][:, 1]) + b[:, 7] * em.vN[0][:, 2]
    assert np.array_equal(_bits(f[0::2]), _bits(-f[1::2]))
    em.close()


class _WallWatch:
    """The outermost wrapper of a test: behind every writer of variables the wall nodes' momentum is +0.0 in bits."""

    def __init__(self, lib, em):
        self._lib, self._em, self.seen = lib, em, {"stage": 0, "restrict": 0, "prolong": 0}

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def _look(self, kind):
        em = self._em
        for l in range(em.visc_levels):
            m = em._var(l)[em.wall_nodes[l], 1:4]
            assert len(m) and not _bits(m).any(), (kind, l)
        self.seen[kind] += 1

    def ora_check_for_invalid_variables(self, *a):
        rc = self._lib.ora_check_for_invalid_variables(*a)
        self._look("stage")
        return rc

    def ora_mg_restrict(self, *a):
        rc = self._lib.ora_mg_restrict(*a)
        self._look("restrict")
        return rc

    def ora_prolong_residuals_interpolate_proper(self, *a):
        rc = self._lib.ora_prolong_residuals_interpolate_proper(*a)
        self._look("prolong")
        return rc


@pytest.mark.parametrize("fas", [False, True])
def test_no_slip_wall_on_lattice_a(fas, oracle, lattices):
    """wall = 1 on all levels of lattice A: wall momentum is exactly +0.0 after every stage, prolongation and restriction of 3
    cycles (the reference's transfers and FAS's), the wall residual is +0.0 - old, density and energy move."""
    em = ve.configured(oracle, lattices["A"], ve.CELL_RE_MU, "local", 1.0, 1, "all", fas=fas)
    assert all(len(em.wall_nodes[l]) > 0 for l in range(em.n))
    before = em.variables(0)[em.wall_nodes[0]]
    assert not _bits(before[:, 1:4]).any() and (before[:, 0] > 0).all()
    watch = _WallWatch(em.lib, em)
    em.lib = watch
    rc, rms = em.cycles(3)
    assert rc == 0 and np.isfinite(rms).all()
    assert watch.seen == {"stage": 3 * 3 * (1 + 2 + 1), "restrict": 3 * 2, "prolong": 3 * 2}
    after = em.variables(0)[em.wall_nodes[0]]
    assert not np.array_equal(after[:, 0], before[:, 0]) and not np.array_equal(after[:, 4], before[:, 4])
    if fas:
        for l in range(1, em.n):
            assert not _bits(em.W0[l][em.wall_nodes[l], 1:4]).any()
    em.close()
    # the residual of the clamped state: one sweep from a state whose wall momentum is not zero
    em = ve.configured(oracle, lattices["A"], ve.CELL_RE_MU, "local", 1.0, 0, 1)
    em.wall = 1
    old = em.variables(0)
    assert old[em.wall_nodes[0], 1:4].all()
    assert em._sweep(0) == 0
    res = em.oc.array(0, "residuals").reshape(-1, 5)
    assert np.array_equal(_bits(res[em.wall_nodes[0], 1:4]), _bits(0.0 - old[em.wall_nodes[0], 1:4]))
    em.close()


def _differing_fraction(oracle, case, mu):
    """The fraction of level 0's nodes at which F + V differs in bits from F in the first stage of a GPU run."""
    em = ve.configured(oracle, case, mu, "reference", 0.5, 0, 1)
    with_v = em.stage_fluxes(0)
    em.set_viscous(0.0, levels=0)
    frac = float((_bits(with_v) != _bits(em.stage_fluxes(0))).any(axis=1).mean())
    em.close()
    return frac


def test_gpu_viscosities(oracle, lattices):
    """GPU_MU[case] is the smallest power of ten at which F + V differs from F at more than half of level 0's nodes in the first
    stage: the condition holds at it and fails at the next smaller power; lattice A's second viscosity is cell Reynolds 2."""
    for key, mu in ve.GPU_MU.items():
        assert mu == 10.0 ** round(np.log10(mu))
        at, below = _differing_fraction(oracle, _case(lattices, key), mu), _differing_fraction(oracle, _case(lattices, key), mu / 10.0)
        print(key, mu, "fraction", at, "at the next smaller power", below)
        assert at > 0.5 >= below, key
    em = ve.ViscousOracle(oracle, lattices["A"])
    assert ve.cell_re_mu(em.ff17) == ve.CELL_RE_MU
    em.close()
    assert ve.CELL_RE_MU > ve.GPU_MU["A"] and _differing_fraction(oracle, lattices["A"], ve.CELL_RE_MU) > 0.5


def test_viscous_cfl_and_every_gpu_combination(oracle, lattices):
    """Every combination tests/test_gpu_viscous.py runs returns code 0 here at every candidate of VISCOUS_CFLS, and VISCOUS_CFL is
    the largest of them at which the viscous limit binds at every node of lattice A's level 0 in every sweep at CELL_RE_MU under
    local steps (the reading recorded in the emulator's header)."""
    binds = {}
    for cfl_v in ve.VISCOUS_CFLS:
        for key, mu, mode, cfl, wall, lv in ve.gpu_combinations():
            em = ve.configured(oracle, _case(lattices, key), mu, mode, cfl, wall, lv, cfl_v=cfl_v)
            rc, rms = em.cycles(ve.GPU_CYCLES)
            assert rc == 0 and np.isfinite(rms).all(), (cfl_v, key, mu, mode, wall, lv)
            if key == "A" and mu == ve.CELL_RE_MU and mode == "local":
                binds[cfl_v] = binds.get(cfl_v, True) and em.limited[0][1] == 0 and em.limited[0][0] == ve.GPU_CYCLES * em.oc.levels[0].nel
                print(cfl_v, wall, lv, "limited", em.limited)
            em.close()
    assert ve.VISCOUS_CFL == max(c for c in ve.VISCOUS_CFLS if binds[c]) and not binds[max(ve.VISCOUS_CFLS)]


def test_composed_and_driver_runs_stay_valid(oracle, lattices):
    """The composed runs (residual smoothing, JST, dual time, FAS, all of them) and the drop-in binary's cases return code 0."""
    for name, mode, cfl, smoothing, jst_levels, order, fas in ve.COMPOSED:
        em = ve.configured(oracle, lattices["A"], ve.CELL_RE_MU, mode, cfl, 1, "all", smoothing, jst_levels, fas)
        if order is None:
            rc, rms = em.cycles(ve.GPU_CYCLES)
        else:
            em.set_dual_time(dte.pick_dt(oracle, lattices["A"], mode, cfl))
            em.set_order(order)
            rc, rms = em.advance(ve.DUAL_STEPS, ve.DUAL_CYCLES)
            assert em.effective_order() == 2
        assert rc == 0 and np.isfinite(rms).all(), name
        em.close()
    for case in ve.DRIVER_CASES:
        plain = ve.ViscousOracle(oracle, case)
        assert plain.cycles(ve.GPU_CYCLES)[0] == 0
        em = ve.ViscousOracle(oracle, case, mu=ve.DRIVER_MU, wall=1, viscous_levels="all")
        rc, rms = em.cycles(ve.GPU_CYCLES)
        assert rc == 0 and np.isfinite(rms).all(), case
        assert not np.array_equal(em.variables(0), plain.variables(0)), case
        em.close(); plain.close()


def test_symbols_defaults_and_array_id():
    import mgcfd
    from mgcfd import api
    header = open(os.path.join(ROOT, "include", "mgcfd.h")).read()
    lib = mgcfd.load_library()
    for name in ("mgcfd_set_viscous", "mgcfd_get_viscous", "mgcfd_viscosity_from_reynolds", "mgcfd_bench_viscous"):
        assert name in mgcfd.EXPORTED_SYMBOLS and hasattr(lib, name) and f"int {name}(" in header
    assert float(re.search(r"#define MGCFD_VISCOUS_CFL (\S+)", header).group(1)) == ve.VISCOUS_CFL == api.VISCOUS_CFL
    assert float(re.search(r"#define MGCFD_VISCOUS_PRANDTL (\S+)", header).group(1)) == ve.PRANDTL == api.VISCOUS_PRANDTL
    enum = header[header.index("enum { MGCFD_ARR_VARIABLES"):]
    enum = re.sub(r"/\*.*?\*/", "", enum[:enum.index("};")], flags=re.S)
    assert re.findall(r"MGCFD_ARR_[A-Z0-9_]+", enum).index("MGCFD_ARR_VISCOUS_STRESS") == api.ARR["viscous_stress"]
    # host only: mu = rho_inf |V_inf| L / Re, refused for bad numbers
    ff = mgcfd.free_stream_constants(1.2, 3.0)
    assert abs(mgcfd.viscosity_from_reynolds(ff, 1000.0, 2.0) - 1.4 * 1.2 * 2.0 / 1000.0) <= 1e-15
    assert abs(mgcfd.viscosity_from_reynolds(mgcfd.free_stream_constants(1.2, 0.0), ve.DRIVER_REYNOLDS) - ve.DRIVER_MU) <= 1e-17
    for re_, length in ((0.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0), (100.0, 0.0), (100.0, float("inf"))):
        with pytest.raises(mgcfd.MgcfdError):
            mgcfd.viscosity_from_reynolds(ff, re_, length)
