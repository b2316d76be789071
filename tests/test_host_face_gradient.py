"""Host tests of the corrected face gradient (no GPU): the numpy emulator (tests/face_gradient_emulator.py) against what the
definition in INTEGRATION.md §20 implies on the uniform 9^3 lattice of tests/test_host_viscous.py — the checkerboard the averaged
gradient cannot see and the correction damps, linear and quadratic fields left alone, the sine's two transfer factors, exact
antisymmetry of every edge term, coincident nodes — the measured per-sweep amplification of the odd-even temperature mode that
fixes MGCFD_VISCOUS_CFL_CORRECTED, and the parameters of tests/test_gpu_face_gradient.py: every run stays valid."""
import ctypes
import os
import re

import numpy as np
import pytest

import face_gradient_emulator as fge
import fas_emulator as fe
import free_stream_emulator as fse
import sa_emulator as sae
import viscous_emulator as ve
import wall_heat_emulator as whe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MU, KAPPA = 0.3, 0.7
RHO, P0 = 1.3, 0.9
H = 1.0 / 8.0
REL = 1e-10


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("face_gradient_lattices")
    return {name: fe.write_lattice(name, d) for name in fe.LATTICES}


@pytest.fixture(scope="module")
def box():
    """tests/test_host_viscous.py's lattice: unjittered, unpermuted 9^3 with fvcorr weights; h = 1/8.  (coords, volumes, to,
    frm, N, layer, sign): layer = a node's distance from the hull in lattice steps, sign = (-1)^(i+j+k)."""
    from mgcfd import meshgen
    n = 9
    level = meshgen.make_box_level(n, permute=False)
    edges, n_int, _, _ = meshgen.to_edge_arrays(level, meshgen.MESH_CODES["fvcorr"])
    e = edges[:n_int]
    to, frm, N = ve.interleaved(np.asarray(e["a"], dtype=np.int64), np.asarray(e["b"], dtype=np.int64), e)
    ijk = np.rint(level.coords * (n - 1)).astype(np.int64)
    layer = np.minimum(ijk, n - 1 - ijk).min(axis=1)
    sign = 1.0 - 2.0 * (ijk.sum(axis=1) % 2)
    return level.coords, level.volumes, to, frm, N, layer, sign


def _state(vel, T):
    p = RHO * T
    W = np.empty((len(vel), 5))
    W[:, 0] = RHO
    W[:, 1:4] = RHO * vel
    W[:, 4] = p / (ve.GAMMA - 1.0) + 0.5 * RHO * (vel * vel).sum(axis=1)
    return W


def _terms(box, W):
    """(V [nel, 5], sums [nel, 5] = Vc[1..3] Wk Hc, per-end terms, ok) at constant MU and KAPPA."""
    xyz, vol, to, frm, N, _, _ = box
    V = ve.viscous_flux(ve.stresses(W, to, frm, N, vol, MU, KAPPA), to, frm, N)
    _, sums, terms, ok = fge.correction(W, vol, MU, KAPPA, xyz, to, frm, N)
    return V, sums, terms, ok


def test_checkerboard_in_u(box):
    """u = u0 + eps (-1)^(i+j+k) at uniform rho and p: V[deep, 1] == 0.0 in bits — the averaged gradient does not see the mode —
    and Vc[deep, 1] = -(40/3) mu eps h s_i to 1e-10 relative."""
    xyz, vol, to, frm, N, layer, sign = box
    deep = layer >= 2
    eps = 1e-3
    vel = np.zeros((len(xyz), 3))
    vel[:, 0] = 0.25 + eps * sign
    V, sums, _, ok = _terms(box, _state(vel, np.full(len(xyz), P0 / RHO)))
    assert ok.all()
    assert not _bits(V[deep, 1]).any()
    want = -(40.0 / 3.0) * MU * eps * H * sign[deep]
    rel = np.abs(sums[deep, 0] - want).max() / np.abs(want).max()
    print("checkerboard in u: Vc[1] against -(40/3) mu eps h s, relative", rel)
    assert rel <= REL


def test_checkerboard_in_T_and_nt(box):
    """T = T0 (1 + eps s_i) at rest: V[deep, 4] == 0.0 in bits and Hc[deep] = -12 kappa (T0 eps) h s_i; nt = nt0 + eps s_i at a
    uniform nu: Qd[deep] == 0.0 in bits and Qdc[deep] = -12 nb eps h s_i, nb = nu + nt0 to first order in eps."""
    xyz, vol, to, frm, N, layer, sign = box
    deep = layer >= 2
    T0, eps = P0 / RHO, 1e-3
    V, sums, _, _ = _terms(box, _state(np.zeros((len(xyz), 3)), T0 + eps * sign))
    assert not _bits(V[deep, 4]).any()
    want = -12.0 * KAPPA * eps * H * sign[deep]
    rel = np.abs(sums[deep, 4] - want).max() / np.abs(want).max()
    print("checkerboard in T: Hc against -12 kappa eps h s, relative", rel)
    assert rel <= REL
    assert not sums[deep, 0:4].any()                       # (a gas at rest: no stress work)
    nu, nt0 = 0.05, 0.2
    nt = nt0 + eps * sign
    W = _state(np.zeros((len(xyz), 3)), np.full(len(xyz), T0))
    G = ve.gradients(nt[:, None], to, frm, N, vol)[:, 0, :]
    grad = np.concatenate([G, np.zeros((len(nt), 1)), np.full((len(nt), 1), nu)], axis=1)
    _, Qd = sae.edge_sums(W, nt, grad, to, frm, N)
    Qdc = fge.sa_qdc(nt, grad, xyz, to, frm, N)
    assert not _bits(Qd[deep]).any()
    # nb of an edge is nu + nt0 exactly in the mean of its two ends: (nu + nt0 + eps s) and (nu + nt0 - eps s)
    want = -12.0 * (nu + nt0) * eps * H * sign[deep]
    rel = np.abs(Qdc[deep] - want).max() / np.abs(want).max()
    print("checkerboard in nt: Qdc against -12 nb eps h s, relative", rel)
    assert rel <= REL


def test_linear_field(box):
    """u = M x + c: the averaged gradient is exact along every edge, so |Vc[1..3]| <= 1e-10 mu |grad u| h^2 at every node, hull
    included."""
    xyz = box[0]
    M = np.array([[0.3, -0.7, 0.2], [0.5, 0.4, -0.6], [-0.1, 0.8, 0.9]])
    vel = xyz @ M.T + np.array([0.2, -0.3, 0.1])
    _, sums, _, _ = _terms(box, _state(vel, np.full(len(xyz), P0 / RHO)))
    scale = MU * np.sqrt((M * M).sum()) * H * H
    print("linear field: max |Vc[1..3]| / (mu |grad u| h^2) =", np.abs(sums[:, 0:3]).max() / scale)
    assert np.abs(sums[:, 0:3]).max() <= REL * scale


def test_quadratic_fields(box):
    """u = (y^2, 0, 0) and T = 1 + y^2: the averaged central difference is exact along the edges of a uniform lattice, Vc and Hc
    vanish two layers from the hull (against the 2 mu vol and 2 kappa vol of §13, which stand)."""
    xyz, vol, to, frm, N, layer, _ = box
    deep = layer >= 2
    y = xyz[:, 1]
    vel = np.zeros((len(xyz), 3))
    vel[:, 0] = y * y
    V, sums, _, _ = _terms(box, _state(vel, np.full(len(xyz), P0 / RHO)))
    assert np.abs(V[deep, 1] - 2.0 * MU * vol[deep]).max() <= REL * 2.0 * MU * vol[deep].max()
    print("u = y^2: max |Vc[1]| / (2 mu vol) =", np.abs(sums[deep, 0]).max() / (2.0 * MU * vol[deep].max()))
    assert np.abs(sums[deep, 0:3]).max() <= REL * 2.0 * MU * vol[deep].max()
    V, sums, _, _ = _terms(box, _state(np.zeros((len(xyz), 3)), 1.0 + y * y))
    assert np.abs(V[deep, 4] - 2.0 * KAPPA * vol[deep]).max() <= REL * 2.0 * KAPPA * vol[deep].max()
    assert np.abs(sums[deep, 4]).max() <= REL * 2.0 * KAPPA * vol[deep].max()


def test_sine_transfer_factors(box):
    """u = 0.1 sin(k y), k h = pi/4: V[1] / exact = sin^2(kh) / (kh)^2 = 0.8106 and (V + Vc)[1] / exact = 4 sin^2(kh/2) / (kh)^2 =
    0.9496, the compact second difference's, where |u| > 0.05, two layers from the hull."""
    xyz, vol, to, frm, N, layer, _ = box
    kh = np.pi / 4.0
    k = kh / H
    u = 0.1 * np.sin(k * xyz[:, 1])
    vel = np.zeros((len(xyz), 3))
    vel[:, 0] = u
    V, sums, _, _ = _terms(box, _state(vel, np.full(len(xyz), P0 / RHO)))
    at = (layer >= 2) & (np.abs(u) > 0.05)
    assert at.sum() > 0
    exact = MU * (-k * k * u[at]) * vol[at]
    wide, compact = V[at, 1] / exact, (V[at, 1] + sums[at, 0]) / exact
    print("sine: averaged", wide.min(), wide.max(), "corrected", compact.min(), compact.max())
    assert np.abs(wide - np.sin(kh) ** 2 / kh ** 2).max() <= REL
    assert np.abs(compact - 4.0 * np.sin(kh / 2.0) ** 2 / kh ** 2).max() <= REL
    assert abs(np.sin(kh) ** 2 / kh ** 2 - 0.8106) < 5e-5 and abs(4.0 * np.sin(kh / 2.0) ** 2 / kh ** 2 - 0.9496) < 5e-5


def test_conservation(box):
    """Every edge term is the exact negative of its other end's (the ends are interleaved), and the level sums to rounding."""
    xyz = box[0]
    rng = np.random.default_rng(5)
    vel = 0.3 * rng.standard_normal((len(xyz), 3))
    T = P0 / RHO * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, len(xyz)))
    _, sums, terms, ok = _terms(box, _state(vel, T))
    assert ok.all() and np.abs(terms).max() > 0.0
    assert np.array_equal(_bits(terms[0::2]), _bits(-terms[1::2]))
    scale = np.abs(terms).sum(axis=0)
    print("conservation: |level sum| / sum |terms|", np.abs(sums.sum(axis=0)) / scale)
    assert (np.abs(sums.sum(axis=0)) <= 1e-13 * scale).all()


def test_coincident_nodes(box):
    """An edge between two nodes given equal coordinates contributes nothing (as if it were not there) and the run stays finite."""
    xyz, vol, to, frm, N, _, _ = box
    X = xyz.copy()
    a, b = int(to[0]), int(frm[0])
    X[b] = X[a]
    rng = np.random.default_rng(6)
    W = _state(0.3 * rng.standard_normal((len(xyz), 3)), P0 / RHO * (1.0 + 0.1 * rng.uniform(-1.0, 1.0, len(xyz))))
    _, sums, terms, ok = fge.correction(W, vol, MU, KAPPA, X, to, frm, N)
    dead = ((to == a) & (frm == b)) | ((to == b) & (frm == a))
    assert dead.sum() == 2 and np.array_equal(ok, ~dead)
    assert np.isfinite(sums).all()
    keep = ~dead
    _, without, _, _ = fge.correction(W, vol, MU, KAPPA, X, to[keep], frm[keep], N[keep])
    # (the node gradients still see the edge: compare against the sums of the remaining ends' terms)
    assert np.array_equal(_bits(sums), _bits(fge.node_sums(terms, ok, to, len(X))))
    assert np.array_equal(_bits(fge.node_sums(terms[keep], np.ones(int(keep.sum()), dtype=bool), to[keep], len(X))), _bits(sums))
    assert np.isfinite(without).all()
    nt = 0.2 + 0.01 * rng.uniform(-1.0, 1.0, len(X))
    grad = np.concatenate([ve.gradients(nt[:, None], to, frm, N, vol)[:, 0, :], np.zeros((len(nt), 1)), np.full((len(nt), 1), 0.05)], axis=1)
    assert np.isfinite(fge.sa_qdc(nt, grad, X, to, frm, N)).all()


# ---- the step limit ----
STABILITY_N = 17
STABILITY_MU = 1.0


def _amplification(oracle, directory, mode, cfl_v):
    """The per-sweep amplification of an odd-even T perturbation on a uniform 17^3 far-field box holding a gas at rest (the far
    field at Mach 0), local steps at CFL 1.0 with mu so large that the viscous limit binds at every node: the projection of
    T - T0 onto (-1)^(i+j+k) over the nodes six or more layers from the hull, after one sweep over before it."""
    em = fge.FaceGradientOracle(oracle, directory, "local", 1.0)
    em.set_far_field(fse.free_stream_constants(0.0, 0.0), True)
    n = STABILITY_N
    ijk = np.rint(em.X[0] * (n - 1)).astype(np.int64)
    layer = np.minimum(ijk, n - 1 - ijk).min(axis=1)
    sign = 1.0 - 2.0 * (ijk.sum(axis=1) % 2)
    deep = layer >= 6
    v = em._var(0)
    rho, T0 = v[0, 0], ve.primitives(v)[0, 3]
    v[:] = 0.0
    v[:, 0] = rho
    v[:, 4] = rho * (T0 * (1.0 + 1e-6 * sign)) / (ve.GAMMA - 1.0)
    em.set_face_gradient(mode)
    em.set_viscous(STABILITY_MU, ve.PRANDTL, 0, cfl_v, 1)
    before = float((sign[deep] * (ve.primitives(v)[deep, 3] - T0)).sum())
    assert em._sweep(0) == 0
    assert em.limited[0] == [len(v), 0], em.limited
    after = float((sign[deep] * (ve.primitives(em._var(0))[deep, 3] - T0)).sum())
    em.close()
    return after / before


def _stages(z):
    """The sweep's amplification of an eigenmode with dt * lambda = z: stage j updates old + (dt / (RK + 1 - j)) * R, so the three
    stages give 1 + z/2 + z^2/6 + z^3/24, which stays inside [-1, 1] on the real axis down to z = -4."""
    return 1.0 + z / 2.0 + z * z / 6.0 + z ** 3 / 24.0


def test_stability_of_the_odd_even_mode(oracle, tmp_path):
    """dt * lambda = 12 cfl_v for pure conduction under the corrected gradient; the averaged one leaves the mode to the inviscid
    dissipation alone, whose small z_i = 2 (amplification - 1) the averaged run measures.  Printed per cfl_v and mode, and
    asserted: the corrected mode decays at MGCFD_VISCOUS_CFL_CORRECTED; it follows 1 + z/2 + z^2/6 + z^3/24 at z = -12 cfl_v + z_i
    to 1e-3 of max(1, |z|^3 / 24) (z_i enters to second order only through that sum); it grows at 0.5.

    Measured here (profiles/face_gradient_stability.txt): 0.1: 0.99462 / 0.56498; 0.2: 0.98928 / 0.17487;
    0.25: 0.98662 / -0.14203; 0.5: 0.97348 / -5.16371 (averaged / corrected).  The textbook three-stage polynomial
    1 + z + z^2/2 + z^3/6 would give -0.82 at 0.2 and -2 at 0.25; the sweep's own is the one above, so 0.25 decays as well and
    the real-axis bound is cfl_v = 1/3."""
    from mgcfd import meshgen
    mg = meshgen.MultigridMesh(mesh_name="fvcorr")
    mg.levels.append(meshgen.make_box_level(STABILITY_N, permute=False))
    os.makedirs(tmp_path / "input")
    meshgen.write_input(mg, str(tmp_path / "input"))
    (tmp_path / "case.txt").write_text("duplicate = 1\n")
    got = {}
    cfls = tuple(sorted(set(ve.VISCOUS_CFLS + (fge.VISCOUS_CFL_CORRECTED,))))
    for cfl_v in cfls:
        for mode in ("averaged", "corrected"):
            got[mode, cfl_v] = _amplification(oracle, str(tmp_path), mode, cfl_v)
        z_i = 2.0 * (got["averaged", cfl_v] - 1.0)
        print(f"cfl_v {cfl_v:5.2f}  averaged {got['averaged', cfl_v]: .6f}  corrected {got['corrected', cfl_v]: .6f}  "
              f"1 + z/2 + z^2/6 + z^3/24 at z = {-12.0 * cfl_v + z_i:.4f}: {_stages(-12.0 * cfl_v + z_i): .6f}")
    assert abs(got["corrected", fge.VISCOUS_CFL_CORRECTED]) < 1.0
    for cfl_v in cfls:
        assert 0.95 < got["averaged", cfl_v] <= 1.0                      # (the mode is invisible to the averaged gradient)
        z = -12.0 * cfl_v + 2.0 * (got["averaged", cfl_v] - 1.0)
        assert abs(got["corrected", cfl_v] - _stages(z)) <= 1e-3 * max(1.0, abs(z) ** 3 / 24.0)
    assert abs(got["corrected", 0.5]) > 1.0


# ---- the parameters of the GPU tests ----
def _valid(em, cycles=fge.GPU_CYCLES):
    rc, rms = em.cycles(cycles)
    assert rc == 0 and np.isfinite(rms).all()
    for l in range(em.n):
        assert np.isfinite(em.variables(l)).all()


@pytest.mark.parametrize("key,wall,lv", fge.gpu_runs())
def test_the_plain_gpu_runs_stay_valid(key, wall, lv, oracle, lattices):
    em = fge.configured(oracle, lattices.get(key, key), fge.RUN_MU[key], wall, lv)
    _valid(em)
    assert em.last_sums[0] is not None and np.abs(em.last_sums[0]).max() > 0.0
    em.close()


@pytest.mark.parametrize("name,kw,key,wall,lv", fge.composed_runs(), ids=[f"{c[0]}-{c[2]}-wall{c[3]}-{c[4]}" for c in fge.composed_runs()])
def test_the_composed_gpu_runs_stay_valid(name, kw, key, wall, lv, oracle, lattices):
    em = fge.configured(oracle, lattices.get(key, key), fge.RUN_MU[key], wall, lv, **kw)
    rc, rms = fge.run(em, kw.get("dual", False))
    assert rc == 0 and np.isfinite(rms).all()
    for l in range(em.n):
        assert np.isfinite(em.variables(l)).all()
    assert np.abs(em.last_sums[0]).max() > 0.0
    em.close()


def test_the_composed_runs_left_out_are_invalid_under_the_averaged_gradient_too(oracle, lattices):
    """fge.COMPOSED_INVALID: the same settings under the averaged gradient at MGCFD_VISCOUS_CFL leave the valid states within
    GPU_CYCLES cycles, so the combination has no state to compare in either mode; and nothing else is left out."""
    composed = dict(fge.COMPOSED)
    for name, key, wall, lv in fge.COMPOSED_INVALID:
        em = fge.configured(oracle, lattices.get(key, key), fge.RUN_MU[key], wall, lv, mode="averaged", cfl_v=ve.VISCOUS_CFL, **composed[name])
        rc, _ = fge.run(em, composed[name].get("dual", False))
        em.close()
        assert rc != 0, (name, key, wall, lv)
    assert len(fge.composed_runs()) == len(fge.COMPOSED) * len(fge.gpu_runs()) - len(fge.COMPOSED_INVALID)


def test_averaged_mode_is_the_wall_heat_oracle(oracle, lattices):
    """The mode off — never set, and set and unset before the run — gives WallHeatOracle's bits."""
    want = whe.configured(oracle, lattices["A"], fge.RUN_MU["A"], "all", whe.HEAT_FLUX, whe.QW, model=fge.SA_MODEL, step=fge.RUN_STEP)
    rc_w, rms_w = want.cycles(fge.GPU_CYCLES)
    for toggle in (False, True):
        em = fge.configured(oracle, lattices["A"], fge.RUN_MU["A"], 1, "all", model=fge.SA_MODEL, thermal=(whe.HEAT_FLUX, whe.QW),
                            mode="corrected" if toggle else "averaged", cfl_v=ve.VISCOUS_CFL)
        em.set_face_gradient("averaged")
        rc, rms = em.cycles(fge.GPU_CYCLES)
        assert rc == rc_w == 0 and np.array_equal(_bits(rms), _bits(rms_w))
        for l in range(em.n):
            assert np.array_equal(_bits(em.variables(l)), _bits(want.variables(l)))
        em.close()
    want.close()


def test_symbols_defaults_and_array_id():
    import mgcfd
    from mgcfd import api
    header = open(os.path.join(ROOT, "include", "mgcfd.h")).read()
    lib = mgcfd.load_library()
    for name in ("mgcfd_set_face_gradient", "mgcfd_get_face_gradient", "mgcfd_bench_face_gradient"):
        assert name in mgcfd.EXPORTED_SYMBOLS and hasattr(lib, name) and f"int {name}(" in header
        assert getattr(lib, name).restype is ctypes.c_int and getattr(lib, name).argtypes
    for macro, value in (("MGCFD_FACE_GRADIENT_AVERAGED", fge.AVERAGED), ("MGCFD_FACE_GRADIENT_CORRECTED", fge.CORRECTED),
                         ("MGCFD_ARR_VISCOUS_GRADIENT", fge.ARR_VISCOUS_GRADIENT)):
        assert int(re.search(rf"#define {macro} (\S+)", header).group(1)) == value
    assert float(re.search(r"#define MGCFD_VISCOUS_CFL_CORRECTED (\S+)", header).group(1)) == api.VISCOUS_CFL_CORRECTED == fge.VISCOUS_CFL_CORRECTED
    assert api._FACE_GRADIENTS == fge.MODES
    assert api.ARR["viscous_gradient"] == fge.ARR_VISCOUS_GRADIENT == 19 and api.NCOLS["viscous_gradient"] == 12
    assert lib.mgcfd_abi_version() == 1


def test_refusals_without_a_device():
    """A NULL solver is MGCFD_ERR_ARG from every entry point of the section; so is a NULL result pointer of the bench call."""
    import mgcfd
    lib = mgcfd.load_library()
    mode, t = ctypes.c_int(7), ctypes.c_double(-1.0)
    assert lib.mgcfd_set_face_gradient(None, fge.CORRECTED) == 1
    assert lib.mgcfd_get_face_gradient(None, ctypes.byref(mode)) == 1 and mode.value == 7
    assert lib.mgcfd_bench_face_gradient(None, 0, 0, 1, ctypes.byref(t)) == 1 and t.value == -1.0


def test_the_polar_and_the_driver_runs_stay_valid(oracle):
    """tests/test_gpu_face_gradient.py's polar and driver runs on m6_2lvl from the far field, at the corrected mode's default cfl_v
    and at 0.1; the corrected run differs from the averaged one."""
    case, alphas, mach = fse.POLAR_CASE, fse.POLAR_ALPHAS, fse.POLAR_MACH
    em = fge.FaceGradientOracle(oracle, case, mu=ve.DRIVER_MU, wall=1, cfl_v=fge.VISCOUS_CFL_CORRECTED, viscous_levels=2)
    em.set_face_gradient("corrected")
    for k, al in enumerate(alphas):
        em.set_far_field(fse.free_stream_constants(mach, al), reinitialise=(k == 0))
        _valid(em)
    em.close()
    states = {}
    for mode, cfl_v in (("corrected", fge.VISCOUS_CFL_CORRECTED), ("corrected", 0.1), ("averaged", fge.VISCOUS_CFL_CORRECTED)):
        em = fge.FaceGradientOracle(oracle, "m6_2lvl", mu=ve.DRIVER_MU, wall=1, cfl_v=cfl_v, viscous_levels="all")
        em.set_face_gradient(mode)
        _valid(em)
        states[mode, cfl_v] = em.variables(0)
        em.close()
    assert not np.array_equal(states["corrected", fge.VISCOUS_CFL_CORRECTED], states["averaged", fge.VISCOUS_CFL_CORRECTED])


def test_the_kernel_level_case_with_coincident_nodes(oracle, tmp_path):
    """Lattice A's level 0 with one node moved onto its neighbour, as tests/test_gpu_face_gradient.py builds it: two edge ends have
    L == 0.0, S is the averaged run's in bits, F + V + Vc and the new nt stay finite, and the correction is there."""
    from conftest import perturbed_state
    from mgcfd import meshgen
    level = meshgen.make_multigrid(fe.LATTICES["A"], "fvcorr", **fe.LATTICE_ARGS).levels[0]
    edges, _, _, _ = meshgen.to_edge_arrays(level, meshgen.MESH_CODES["fvcorr"])
    level.coords[int(edges["b"][0])] = level.coords[int(edges["a"][0])]
    mg = meshgen.MultigridMesh(mesh_name="fvcorr")
    mg.levels.append(level)
    os.makedirs(tmp_path / "input")
    meshgen.write_input(mg, str(tmp_path / "input"))
    (tmp_path / "case.txt").write_text("duplicate = 1\n")
    mu = ve.CELL_RE_MU
    em = fge.FaceGradientOracle(oracle, str(tmp_path), "local", 1.0)
    v = em._var(0)
    v[:] = perturbed_state(len(v), em.ff17[:5], seed=7, amplitude=0.01)
    em.set_viscous(mu, ve.PRANDTL, 1, fge.VISCOUS_CFL_CORRECTED, 1)
    em.set_viscosity_model(law="sutherland", eddy=sae.SA)
    em.set_nu_tilde(0, sae.random_nt(mu, em.ff17[0], len(v), sae.NT_SEED + 1))
    em.copy_old()
    em.set_nu_tilde(0, sae.random_nt(mu, em.ff17[0], len(v)))
    sf = em.final_step_factors(0)
    averaged = em.kernel_level(0, sf)
    em.set_face_gradient("corrected")
    corrected = em.kernel_level(0, sf)
    assert (fge.edge_geometry(em.X[0], em.vto[0], em.vfrm[0])[1] == 0.0).sum() == 2
    assert np.array_equal(_bits(averaged[2]), _bits(corrected[2]))
    assert np.isfinite(corrected[3]).all() and np.isfinite(corrected[4]).all()
    assert not np.array_equal(averaged[3], corrected[3]) and not np.array_equal(averaged[4], corrected[4])
    assert em.viscous_gradient(0).shape == (len(v), 12)
    em.close()
