"""Host tests of the unsteady Spalart-Allmaras model (no GPU): the numpy emulator (tests/sa_unsteady_emulator.py) against what the
definition in INTEGRATION.md §21 implies — tanh_fixed against long double, the BDF source of a linear and a quadratic nt, a uniform
field that stays put in bits under dual time, delta and the DES97 length on the uniform lattice, the log-layer identity of the
delayed-DES shielding — and the parameters of tests/test_gpu_sa_unsteady.py: every run stays finite with nt >= 0, every branch is
reached, DES and delayed DES move nt away from the RANS run; the ABI surface."""
import os
import re

import numpy as np
import pytest

import fas_emulator as fe
import sa_emulator as sae
import sa_unsteady_emulator as sue
import variable_viscosity_emulator as vve
import viscous_emulator as ve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHO, P0 = 1.3, 0.9


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("sa_unsteady_lattices")
    return {name: fe.write_lattice(name, d) for name in fe.LATTICES}


@pytest.fixture(scope="module")
def box():
    """tests/test_host_viscous.py's lattice: unjittered, unpermuted 9^3 with fvcorr weights; h = 1/8."""
    from mgcfd import meshgen
    n = 9
    level = meshgen.make_box_level(n, permute=False)
    edges, n_int, _, _ = meshgen.to_edge_arrays(level, meshgen.MESH_CODES["fvcorr"])
    e = edges[:n_int]
    a, b = np.asarray(e["a"], dtype=np.int64), np.asarray(e["b"], dtype=np.int64)
    to, frm, N = ve.interleaved(a, b, e)
    return level.coords, level.volumes, to, frm, N, a, b


def test_tanh_fixed_against_long_double():
    """3 M points over [0, 20]: within 1e-12 absolute of the long-double tanh (ten squarings each double the relative error of p
    and add half an ulp: about 1024 x 5 x 1.1e-16, 3e-13 in the quotient), the ends exact, every value in [0, 1]."""
    z = np.random.default_rng(2).uniform(0.0, 20.0, 3_000_000)
    z[:2] = (0.0, 20.0)
    got = sue.tanh_fixed(z)
    err = float(np.abs(got.astype(np.longdouble) - np.tanh(z.astype(np.longdouble))).max())
    print("tanh_fixed: largest absolute error", err)
    assert err <= 1e-12
    assert got[0] == 0.0 and not np.signbit(got[0]) and got[1] == 1.0
    assert (got >= 0.0).all() and (got <= 1.0).all()


def test_bdf_source():
    """nt = a + b t sampled at three levels: BDF2's and BDF1's ts equal b to a few roundings; for a quadratic BDF2 stays exact to
    rounding and BDF1 is off by c dt."""
    a, b, c, dt = 0.3, 0.7, 0.9, 0.01
    t = np.array([1.0, 2.0, 5.0])
    lin = lambda s: a + b * s
    for order in (1, 2):
        ts, cj = sue.time_source(lin(t), lin(t - dt), lin(t - 2.0 * dt), dt, order)
        assert np.abs(ts - b).max() <= 64 * np.finfo(float).eps * np.abs(lin(t)).max() / dt, (order, ts)
        assert cj == (1.5 if order == 2 else 1.0) / np.float64(dt)
    quad = lambda s: a + b * s + c * s * s
    exact = b + 2.0 * c * t
    ts2, _ = sue.time_source(quad(t), quad(t - dt), quad(t - 2.0 * dt), dt, 2)
    ts1, _ = sue.time_source(quad(t), quad(t - dt), quad(t - 2.0 * dt), dt, 1)
    bound = 64 * np.finfo(float).eps * np.abs(quad(t)).max() / dt
    print("BDF2 error", np.abs(ts2 - exact).max(), "BDF1 error", np.abs(ts1 - exact).max(), "c dt", c * dt)
    assert np.abs(ts2 - exact).max() <= bound
    assert np.abs((exact - ts1) - c * dt).max() <= bound
    same = np.full(4, 0.37)
    for order in (1, 2):
        ts, _ = sue.time_source(same, same, same, dt, order)
        assert np.array_equal(_bits(ts), _bits(np.zeros(4)))


def test_uniform_field_stays_put_in_bits(box):
    """A uniform state and nt = ntn = ntn1 uniform with d = +inf: bit-identical over ve.DUAL_STEPS + 1 physical steps of
    ve.DUAL_CYCLES cycles of three stages, BDF1 first and BDF2 after."""
    xyz, vol, to, frm, N, _, _ = box
    n = len(xyz)
    W = np.empty((n, 5))
    vel = np.tile(np.array([0.3, -0.2, 0.1]), (n, 1))
    W[:, 0], W[:, 1:4] = RHO, RHO * vel
    W[:, 4] = P0 / (ve.GAMMA - 1.0) + 0.5 * RHO * (vel * vel).sum(axis=1)
    mu = 0.05
    nt0 = np.full(n, 3.0 * mu / RHO)
    cb = vve.tse.libm_cbrt(vol)
    g, d, sf = (cb * cb) / vol, np.full(n, np.inf), np.full(n, 0.7) / vol
    nt, ntn, ntn1 = nt0.copy(), nt0.copy(), nt0.copy()
    for step in range(ve.DUAL_STEPS + 1):
        ntn1, ntn = (nt.copy(), nt.copy()) if step == 0 else (ntn, nt.copy())
        for cycle in range(ve.DUAL_CYCLES):
            old = nt.copy()
            for j in range(sae.RK):
                grad, mut = sae.gradient(W, nt, to, frm, N, vol, mu, vve.Model("sutherland", P0 / RHO))
                nt = sue.transport(W, nt, old, grad, to, frm, N, vol, d, g, sf, ve.VISCOUS_CFL, j, (ntn, ntn1, 0.05, 1 if step == 0 else 2))
    assert np.array_equal(_bits(nt), _bits(nt0))


def test_delta_and_des_length_on_the_uniform_lattice(box):
    """delta = h at every node of the uniform lattice, and d~ = min(d, c_des h) under DES97 (+0.0 on the wall)."""
    xyz, vol, to, frm, N, a, b = box
    h = 1.0 / 8.0
    delta = sue.delta_of(xyz, a, b)
    assert np.array_equal(_bits(delta), _bits(np.full(len(xyz), h)))
    d = xyz[:, 2].copy()                                   # a wall at z = 0
    got = sue.des_length(d, np.float64(sue.SA_CDES) * delta)
    assert np.array_equal(_bits(got), _bits(np.minimum(d, np.float64(sue.SA_CDES) * h)))
    assert (got[d == 0.0] == 0.0).all() and not np.signbit(got[d == 0.0]).any()
    lone = sue.delta_of(xyz, a[:1], b[:1])
    assert np.isposinf(lone).sum() == len(xyz) - 2


def test_log_layer_identity_under_ddes():
    """nt = kappa ut d and sqrt(U_ij U_ij) = ut / (kappa d): rd = 1, z caps at 20, fd = +0.0 and d~ = d exactly (full shielding);
    nt -> 0 at zero shear and a small nu: fd = 1 and d~ = lim."""
    ut = 0.05
    d = np.array([1e-3, 0.01, 0.1, 1.0, 10.0])
    nt = sae.KAPPA * ut * d
    G = np.zeros((len(d), 3, 3))
    G[:, 0, 2] = ut / (sae.KAPPA * d)
    fd, z = sue.shield(G, nt, 1e-12 * nt, d)
    assert (z == 20.0).all() and np.array_equal(_bits(fd), _bits(np.zeros(len(d))))
    lim = 0.5 * d
    got, masks = sue.ddes_length(d, lim, fd)
    assert np.array_equal(_bits(got), _bits(d)) and masks["fd_zero"].all()
    fd, z = sue.shield(np.zeros((len(d), 3, 3)) + 1.0, np.zeros(len(d)), np.full(len(d), 1e-12), d)
    assert (fd == 1.0).all()
    got, masks = sue.ddes_length(d, lim, fd)
    assert np.array_equal(_bits(got), _bits(lim)) and masks["fd_one"].all()


# ---- the parameters of the GPU runs ----
_runs = {}


def _run(oracle, lattices, key, length, dt=sue.DUAL_DT, **composed):
    k = (key, length, dt, repr(sorted(composed.items())))
    if k not in _runs:
        em = sue.configured(oracle, lattices.get(key, key), sue.RUN_MU[key], length, dt=dt, **composed)
        if dt:
            rc, rms = em.advance(sue.DUAL_STEPS, sue.DUAL_CYCLES)
        else:
            rc, rms = em.cycles(sae.GPU_CYCLES)
        _runs[k] = (rc, rms, [em.variables(l) for l in range(em.n)], [em.nu_tilde(l) for l in range(em.visc_levels)], dict(em.ubranches))
        em.close()
    return _runs[k]


@pytest.mark.parametrize("length", sue.RUN_LENGTHS)
@pytest.mark.parametrize("key", sue.RUN_CASES)
def test_gpu_runs_stay_valid(key, length, oracle, lattices):
    for dt in (sue.DUAL_DT, 0.0):                          # (the dual-time runs and, under des and ddes, the steady ones)
        if dt == 0.0 and (length == "wall" or key != "A"):
            continue
        rc, rms, v, nt, br = _run(oracle, lattices, key, length, dt)
        assert rc == 0 and np.isfinite(rms).all()
        assert all(np.isfinite(x).all() for x in v) and all(np.isfinite(x).all() and (x >= 0.0).all() for x in nt)


@pytest.mark.parametrize("name,kw", sue.composed_settings(), ids=[c[0] for c in sue.composed_settings()])
def test_composed_runs_stay_valid(name, kw, oracle, lattices):
    rc, rms, v, nt, br = _run(oracle, lattices, "A", "ddes", **kw)
    assert rc == 0 and np.isfinite(rms).all() and all(np.isfinite(x).all() and (x >= 0.0).all() for x in nt)


def test_every_branch_is_reached(oracle, lattices, tmp_path):
    """Over the GPU cases together — the runs on lattice A and the kernel-level cases of tests/test_gpu_sa_unsteady.py, each of
    which stays finite with nt >= 0: c_des = 2.0 puts lattice A's first layer at d <= lim, the box without walls has d = +inf, the
    tetrahedral level at mu = 1e-12 has fd = 1."""
    from conftest import perturbed_state
    from test_gpu_sa import _kernel_cases
    total = {k: 0 for k in sue.BRANCHES}
    for length in sue.RUN_LENGTHS:
        for k, n in _run(oracle, lattices, "A", length)[4].items():
            total[k] += n
    counts = {}
    for name, case, amplitude, cfl, mu in _kernel_cases(lattices, tmp_path):
        for length, c_des, order, corrected, mu_v in sue.kernel_variants(name):
            em0 = sue.SaUnsteadyOracle(oracle, case, "local", cfl)
            start = perturbed_state(len(em0._var(0)), em0.ff17[:5], seed=7, amplitude=amplitude)
            em0.close()
            em, old, new, levels, sf, (grad, mut, S, f, d_model, out) = sue.kernel_level_case(oracle, case, mu_v or mu, cfl, start, length, c_des,
                                                                                            order, corrected)
            assert np.isfinite(out).all() and (out >= 0.0).all(), (name, length)
            if name == "lattice_A" and length == "ddes":
                d, lim = em.wall_distance(0)[0], np.float64(c_des) * em.delta
                counts[c_des] = int(((d > 0.0) & (d <= lim)).sum())
                print("lattice A, c_des", c_des, "off-wall nodes with d <= lim:", counts[c_des], "of", int((d > 0.0).sum()))
            print(name, length, c_des, order, corrected, mu_v, em.ubranches)
            for k, n in em.ubranches.items():
                total[k] += n
            em.close()
    # (lattice A is jittered, so a few nodes sit within 0.65 of their longest edge of the wall; at 2.0 the whole first layer does)
    assert counts[sue.KERNEL_CDES] > 4 * max(counts[sue.SA_CDES], 1)
    print("branches:", total)
    assert all(total[k] >= 1 for k in sue.BRANCHES), total


def test_des_and_ddes_move_nt(oracle, lattices):
    """A DES run and a delayed-DES run each move level 0's nt away from the RANS run's by more than rounding at some node."""
    rans = _run(oracle, lattices, "A", "wall")[3][0]
    for length in ("des", "ddes"):
        nt = _run(oracle, lattices, "A", length)[3][0]
        rel = float(np.abs(nt - rans).max() / np.abs(rans).max())
        print(length, "against RANS: largest difference of nt over its largest value", rel)
        assert rel > 1e-10


def test_restart_from_the_six_arrays(oracle, lattices):
    """Two steps, then variables, Wn, Wn1, nt, ntn and ntn1 written into a fresh emulator and one more step: the bits of the
    uninterrupted run (begin_step forms mut again, so nothing else carries over)."""
    rc, want_rms, want_v, want_nt, _ = _run(oracle, lattices, "A", "ddes")
    a = sue.configured(oracle, lattices["A"], sue.RUN_MU["A"], "ddes")
    rc, r0 = a.advance(2, sue.DUAL_CYCLES)
    assert rc == 0
    saved = [(a.variables(l), a.Wn[l].copy(), a.Wn1[l].copy(), a.nu_tilde(l)) for l in range(a.n)]
    ntn, ntn1 = a.ntn.copy(), a.ntn1.copy()
    a.close()
    b = sue.configured(oracle, lattices["A"], sue.RUN_MU["A"], "ddes")
    for l, (v, wn, wn1, nt) in enumerate(saved):
        b._var(l)[:] = v
        b.set_time_levels(l, wn, wn1)
        b.set_nu_tilde(l, nt)
    b.set_nt_time_levels(ntn, ntn1)
    rc, r1 = b.advance(sue.DUAL_STEPS - 2, sue.DUAL_CYCLES)
    assert rc == 0
    assert np.array_equal(_bits(np.concatenate([r0, r1])), _bits(want_rms))
    assert np.array_equal(_bits(b.variables(0)), _bits(want_v[0])) and np.array_equal(_bits(b.nu_tilde(0)), _bits(want_nt[0]))
    b.close()


def test_abi_surface():
    """The header declares the setting, the arrays and the calls; the Python table knows them."""
    import mgcfd
    from mgcfd import api
    h = open(os.path.join(ROOT, "include", "mgcfd.h")).read()
    for pattern in (r"#define MGCFD_SA_LENGTH_WALL 0\b", r"#define MGCFD_SA_LENGTH_DES  1\b", r"#define MGCFD_SA_LENGTH_DDES 2\b",
                    r"#define MGCFD_SA_CDES 0\.65\b", r"#define MGCFD_ARR_SA_TIME_N 20\b", r"#define MGCFD_ARR_SA_TIME_N1 21\b",
                    r"#define MGCFD_ARR_SA_LENGTH 22\b",
                    r"int mgcfd_set_sa_unsteady\(mgcfd_solver \*s, int time_accurate, int length, double c_des\);",
                    r"int mgcfd_get_sa_unsteady\(const mgcfd_solver \*s, int \*time_accurate, int \*length, double \*c_des\);"):
        assert re.search(pattern, h), pattern
    assert (api.ARR["sa_time_n"], api.ARR["sa_time_n1"], api.ARR["sa_length"]) == (sue.ARR_SA_TIME_N, sue.ARR_SA_TIME_N1, sue.ARR_SA_LENGTH)
    assert api.NCOLS["sa_time_n"] == api.NCOLS["sa_time_n1"] == api.NCOLS["sa_length"] == 1
    assert api.SA_CDES == sue.SA_CDES and api._SA_LENGTHS == sue.LENGTHS
    for name in ("mgcfd_set_sa_unsteady", "mgcfd_get_sa_unsteady"):
        assert name in mgcfd.EXPORTED_SYMBOLS
