"""Host tests of the Spalart-Allmaras model (no GPU): the numpy emulator (tests/sa_emulator.py) against what the definition in
INTEGRATION.md §18 implies — the sixth root against long double, the closure functions' continuity and fw(1) = 1, the log-layer
identity that defines cw1, the convection, diffusion and gradient terms of a linear nt on the uniform lattice of
tests/test_host_viscous.py, a uniform field that stays put in bits — and the parameters of tests/test_gpu_sa.py: every run stays
valid, moves nt, and together with the kernel-level case reaches every branch of the definition."""
import os
import re

import numpy as np
import pytest

import fas_emulator as fe
import sa_emulator as sae
import variable_viscosity_emulator as vve
import viscous_emulator as ve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO, P0 = 1.3, 0.9


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("sa_lattices")
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
    return level.coords, level.volumes, to, frm, N, layer


def _state(vel, T):
    p = RHO * T
    W = np.empty((len(vel), 5))
    W[:, 0] = RHO
    W[:, 1:4] = RHO * vel
    W[:, 4] = p / (ve.GAMMA - 1.0) + 0.5 * RHO * (vel * vel).sum(axis=1)
    return W


def test_root6_against_long_double():
    """Within 4 ulp of the long-double t**(1/6) on 1e6 points, log-uniform over [1e-32, 1.02]."""
    rng = np.random.default_rng(1)
    t = np.exp(rng.uniform(np.log(1e-32), np.log(1.02), 1_000_000))
    t[:2] = (1e-32, 1.02)
    got = sae.root6(t)
    want = t.astype(np.longdouble) ** (np.longdouble(1) / np.longdouble(6))
    ulp = np.spacing(want.astype(np.float64)).astype(np.longdouble)
    err = np.abs(got.astype(np.longdouble) - want) / ulp
    print("root6: max error", float(err.max()), "ulp; long double eps", np.finfo(np.longdouble).eps)
    assert np.finfo(np.longdouble).eps < 1e-18, "long double is wider than double here"
    assert float(err.max()) <= 4.0
    assert sae.root6(np.float64(1.0)) == 1.0


def test_closure_functions():
    """fv1, fv2 and the limiter of S~ are continuous at sb = -cv2 om to 1e-14; fw(1) = 1 to 1e-15."""
    om = np.array([0.3, 1.0, 7.5, 1234.5])
    sb0 = -(sae.CV2 * om)
    below, above = np.nextafter(sb0, -np.inf), sb0
    a, b = sae.s_tilde(om, below), sae.s_tilde(om, above)
    assert (below < sb0).all()
    rel = np.abs(a - b) / np.abs(b)
    print("S~ across the switch, relative", rel)
    assert (rel <= 1e-14).all()
    assert np.abs(b - (1.0 - sae.CV2) * om).max() <= 1e-14 * om.max()
    # (fv1 and fv2 are rational in chi: continuous wherever their denominators are positive, which is chi >= 0)
    chi = np.array([0.0, 1e-8, 1.0, 7.1, 18.4, 1e3, 1e8])
    for f in (sae.fv1, sae.fv2):
        lo, hi = f(chi), f(np.nextafter(chi, np.inf))
        assert np.isfinite(lo).all() and (np.abs(hi - lo) <= 1e-14).all()
    assert sae.fv1(np.float64(0.0)) == 0.0 and sae.fv2(np.float64(0.0)) == 1.0
    assert abs(sae.fv1(np.float64(7.1)) - 0.5) <= 1e-15
    assert abs(float(sae.fw(np.float64(1.0))) - 1.0) <= 1e-15
    # the far limit of fw: (1 + cw3^6)^(1/6)
    assert abs(float(sae.fw(np.float64(1e6))) - 65.0 ** (1.0 / 6.0)) <= 1e-9


def test_log_layer_identity():
    """nt = kappa ut d, om = ut / (kappa d), |grad nt| = kappa ut, nu = 1e-12 nt: the node source plus (1/sigma) kappa^2 ut^2 —
    the diffusion of a linear nt with a linear diffusivity — vanishes to 1e-9 of cb1 ut^2: the identity that defines cw1."""
    ut = 0.05
    d = np.array([1e-3, 0.01, 0.1, 1.0, 10.0])
    nt = sae.KAPPA * ut * d
    om = ut / (sae.KAPPA * d)
    gg = np.full(len(d), (sae.KAPPA * ut) ** 2)
    src, st, f, capped, second = sae.node_source(nt, 1e-12 * nt, om, gg, d)
    rest = src + sae.INV_SIGMA * sae.KAPPA ** 2 * ut ** 2
    print("log layer: residual", rest, "of", sae.CB1 * ut ** 2)
    assert (np.abs(rest) <= 1e-9 * sae.CB1 * ut ** 2).all()
    assert not capped.any() and not second.any()


def test_linear_nt_on_the_uniform_lattice(box):
    """Uniform velocity (U, 0, Wz), Wz > 0, and nt = z: Qc = -vol Wz, Qd = vol, gg = 1, two layers from the hull, to 1e-12."""
    xyz, vol, to, frm, N, layer = box
    U, Wz, mu = 0.3, 0.2, 0.05
    vel = np.tile(np.array([U, 0.0, Wz]), (len(xyz), 1))
    W = _state(vel, np.full(len(xyz), P0 / RHO))
    nt = xyz[:, 2].copy()
    grad, mut = sae.gradient(W, nt, to, frm, N, vol, mu, vve.Model())
    Qc, Qd = sae.edge_sums(W, nt, grad, to, frm, N)
    deep = layer >= 2
    assert deep.sum() == 5 ** 3
    gg = (grad[:, 0] ** 2 + grad[:, 1] ** 2) + grad[:, 2] ** 2
    for got, want, what in ((Qc[deep], -vol[deep] * Wz, "Qc"), (Qd[deep], vol[deep], "Qd"), (gg[deep], np.ones(deep.sum()), "gg")):
        rel = np.abs(got - want).max() / np.abs(want).max()
        print(what, "relative", rel)
        assert rel <= 1e-12
    assert np.abs(grad[deep, 3]).max() <= 1e-12 and np.array_equal(_bits(grad[:, 4]), _bits(np.full(len(xyz), mu / RHO)))


def test_uniform_field_stays_put_in_bits(box):
    """A uniform state and a uniform nt with d = +inf: nt is bit-identical after three cycles of three stages."""
    xyz, vol, to, frm, N, layer = box
    n = len(xyz)
    W = _state(np.tile(np.array([0.3, -0.2, 0.1]), (n, 1)), np.full(n, P0 / RHO))
    mu = 0.05
    nt0 = np.full(n, 3.0 * mu / RHO)
    cb = vve.tse.libm_cbrt(vol)
    g, d, sf = (cb * cb) / vol, np.full(n, np.inf), np.full(n, 0.7) / vol
    nt = nt0.copy()
    for cycle in range(3):
        old = nt.copy()
        for j in range(sae.RK):
            grad, mut = sae.gradient(W, nt, to, frm, N, vol, mu, vve.Model("sutherland", P0 / RHO))
            nt, masks = sae.transport(W, nt, old, grad, to, frm, N, vol, d, g, sf, ve.VISCOUS_CFL, j)
            assert not masks["wall"].any() and not masks["clipped"].any()
    assert np.array_equal(_bits(nt), _bits(nt0))


# ---- the parameters of the GPU runs ----
_runs = {}


def _run(oracle, lattices, key, mu, mode, cfl, wall, lv, model):
    k = (key, mu, mode, cfl, wall, lv, tuple(model))
    if k not in _runs:
        em = sae.configured(oracle, lattices.get(key, key), mu, mode, cfl, wall, lv, model)
        start = [em.nu_tilde(l) for l in range(em.visc_levels)]
        rc, rms = em.cycles(sae.GPU_CYCLES)
        _runs[k] = (rc, rms, [em.variables(l) for l in range(em.n)], start, [em.nu_tilde(l) for l in range(em.visc_levels)],
                    [em.eddy_viscosity(l) for l in range(em.visc_levels)], dict(em.branches), em.max_move,
                    [w.copy() for w in em.wall_nodes])
        em.close()
    return _runs[k]


@pytest.mark.parametrize("key,mu,mode,cfl,wall,lv,model", sae.gpu_runs())
def test_gpu_runs_stay_valid(key, mu, mode, cfl, wall, lv, model, oracle, lattices):
    rc, rms, v, start, nt, mut, branches, move, walls = _run(oracle, lattices, key, mu, mode, cfl, wall, lv, model)
    assert rc == 0 and np.isfinite(rms).all()
    for l in range(len(v)):
        assert np.isfinite(v[l]).all()
    for l in range(len(nt)):
        assert np.isfinite(nt[l]).all() and (nt[l] >= 0.0).all() and np.isfinite(mut[l]).all() and (mut[l] >= 0.0).all()
    assert not _bits(nt[0][walls[0]]).any(), "nt is +0.0 on level 0's wall (a coarse level holds its children's average)"
    print(key, model, wall, lv, "branches", branches, "largest relative move of nt in a stage", move)


@pytest.mark.parametrize("name,smoothing,jst_levels,fas,shape", sae.COMPOSED, ids=[c[0] for c in sae.COMPOSED])
def test_composed_runs_stay_valid(name, smoothing, jst_levels, fas, shape, oracle, lattices):
    em = sae.configured(oracle, lattices["A"], ve.CELL_RE_MU, "local", 2.0 if smoothing[1] else 1.0, 1, "all", sae.MODELS[1],
                        smoothing=smoothing, jst_levels=jst_levels, fas=fas, shape=shape)
    rc, rms = em.cycles(sae.GPU_CYCLES)
    assert rc == 0 and np.isfinite(rms).all()
    for l in range(em.n):
        assert np.isfinite(em.variables(l)).all() and np.isfinite(em.nu_tilde(l)).all() and (em.nu_tilde(l) >= 0.0).all()
    em.close()


def _kernel_level_masks(oracle, case, mu):
    from conftest import perturbed_state
    em0 = sae.SaOracle(oracle, case, "local", 1.0)
    start = ve.start_state(len(em0._var(0)), em0.ff17[:5])
    em0.close()
    em, old, new, sf, out = sae.kernel_level_case(oracle, case, mu, 1.0, start)
    em.close()
    return out


def test_every_branch_is_reached(oracle, lattices):
    """Over the plain runs and the kernel-level case (a seeded random nt in [0, 10 nu], lattice A) together: at least one node in
    the second branch of S~, with r capped, with jac clamped, with the cap below the step factor, clipped at zero, and on the wall."""
    total = {k: 0 for k in sae.BRANCHES}
    for c in sae.gpu_runs():
        for k, n in _run(oracle, lattices, *c)[6].items():
            total[k] += n
    print("plain runs:", total)
    grad, mut, S, f, out, masks = _kernel_level_masks(oracle, lattices["A"], ve.CELL_RE_MU)
    kernel = {k: int(masks[k].sum()) for k in sae.BRANCHES}
    print("kernel-level case:", kernel)
    assert np.isfinite(out).all() and (out >= 0.0).all() and np.isfinite(grad).all() and np.isfinite(f).all()
    for k in sae.BRANCHES:
        assert total[k] + kernel[k] >= 1, f"no node takes the branch {k}"


def test_plain_run_moves_nt(oracle, lattices):
    """A plain run on lattice A moves nt by more than 1e-3 relative at some non-wall node."""
    c = [r for r in sae.gpu_runs() if r[0] == "A"][0]
    rc, rms, v, start, nt, mut, branches, move, walls = _run(oracle, lattices, *c)
    free = start[0] > 0.0
    rel = np.abs(nt[0][free] - start[0][free]) / start[0][free]
    print("lattice A: nt moved by at most", rel.max(), "relative over the run")
    assert rel.max() > 1e-3


def test_abi_surface():
    """The header declares the mode, the arrays and the calls; the Python table knows them."""
    import mgcfd
    from mgcfd import api
    h = open(os.path.join(ROOT, "include", "mgcfd.h")).read()
    for pattern in (r"#define MGCFD_EDDY_SPALART_ALLMARAS 4\b", r"#define MGCFD_ARR_SA_NU_TILDE 17\b", r"#define MGCFD_ARR_SA_GRADIENT 18\b",
                    r"#define MGCFD_SA_RATIO 3\.0\b", r"int mgcfd_set_sa_free_stream\(mgcfd_solver \*s, double ratio, int reinitialise\);",
                    r"int mgcfd_get_sa_free_stream\(", r"int mgcfd_bench_sa\(mgcfd_solver \*s, int level, int kind, int launches, double \*avg_seconds\);"):
        assert re.search(pattern, h), pattern
    assert api.ARR["sa_nu_tilde"] == sae.ARR_SA_NU_TILDE and api.ARR["sa_gradient"] == sae.ARR_SA_GRADIENT
    assert api.NCOLS["sa_nu_tilde"] == 1 and api.NCOLS["sa_gradient"] == 5
    assert api._ALL_EDDY_MODES[sae.SA] == sae.EDDY_SA and api.SA_RATIO == sae.SA_RATIO
    for name in ("mgcfd_set_sa_free_stream", "mgcfd_get_sa_free_stream", "mgcfd_bench_sa"):
        assert name in mgcfd.EXPORTED_SYMBOLS
