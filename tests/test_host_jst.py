"""Host tests of the JST dissipation (no GPU): the numpy emulator (tests/jst_emulator.py) with JST off against its parent bit for
bit, the sums read literally, the reduction to the reference's dissipation, conservation, what the scheme is for (a linear field
loses its dissipation), the validity of every combination the GPU tests run, and the new symbols."""
import os

import numpy as np
import pytest

import dual_time_emulator as dte
import jst_emulator as jse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -52


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _random_state(em, l, seed, amplitude=0.05):
    from conftest import perturbed_state
    return perturbed_state(em.oc.levels[l].nel, em.ff17[:5], seed, amplitude)


@pytest.mark.parametrize("case", jse.GPU_CASES)
def test_levels_zero_is_the_parent_emulator(case, oracle):
    """levels = 0 (whatever the coefficients): DualTimeOracle's bits on every level and its RMS history, plain and with
    residual smoothing under local steps."""
    for mode, cfl, smoothing in (("reference", 0.5, (0.0, 0)), ("local", 1.5, (0.5, 2))):
        want = dte.DualTimeOracle(oracle, case, mode, cfl, *smoothing)
        em = jse.JstOracle(oracle, case, mode, cfl, *smoothing, kappa2=2.5, kappa4=0.15625, levels=0)
        assert (em.kappa2, em.kappa4, em.jst_levels) == (0.0, 0.0, 0)
        rc_w, rms_w = want.cycles(jse.GPU_CYCLES)
        rc, rms = em.cycles(jse.GPU_CYCLES)
        assert rc == rc_w == 0 and np.array_equal(_bits(rms), _bits(rms_w))
        for l in range(em.n):
            assert np.array_equal(_bits(em.variables(l)), _bits(want.variables(l))), (case, mode, l)
        em.close(); want.close()


def test_the_sums_run_in_edge_order_from_plus_zero(oracle):
    """The emulator's L, nu, r and C against a plain Python loop over the edges (the definition read literally) on one level."""
    em = jse.JstOracle(oracle, "tet_2lvl", kappa2=2.5, kappa4=0.15625, levels=1)
    W = _random_state(em, 1, seed=5)
    a, b, k_e = em.ea[1], em.eb[1], em.k_e[1]
    e = em.oc.edges(1)[em.oc.levels[1].internal_start:][:len(a)]
    p = jse.pressure(W)
    n = len(W)
    L, Pm, Pp, deg = np.zeros((n, 5)), np.zeros(n), np.zeros(n), np.zeros(n, dtype=int)
    for i, j in zip(a, b):
        L[i] = L[i] + (W[j] - W[i]); Pm[i] = Pm[i] + (p[j] - p[i]); Pp[i] = Pp[i] + (p[j] + p[i]); deg[i] += 1
        L[j] = L[j] + (W[i] - W[j]); Pm[j] = Pm[j] + (p[i] - p[j]); Pp[j] = Pp[j] + (p[i] + p[j]); deg[j] += 1
    nu = np.array([abs(Pm[i]) / Pp[i] if deg[i] else 0.0 for i in range(n)])
    rho = W[:, 0]
    vx, vy, vz = W[:, 1] / rho, W[:, 2] / rho, W[:, 3] / rho
    ssq = vx * vx + vy * vy + vz * vz
    r = np.sqrt(ssq) + np.sqrt(1.4 * p / rho)
    Cn = np.zeros((n, 5))
    k2, k4 = np.float64(2.5), np.float64(0.15625)
    for (i, j), E in zip(zip(a, b), e):
        k = -np.sqrt(E["x"] * E["x"] + E["y"] * E["y"] + E["z"] * E["z"]) * np.float64(np.float32(0.2)) * 0.5
        for me, ot in ((i, j), (j, i)):
            fac = k * (r[me] + r[ot])
            m = nu[me] if nu[me] > nu[ot] else nu[ot]
            e2 = k2 * m
            e2 = e2 if e2 < 1.0 else np.float64(1.0)
            e4 = k4 - e2
            e4 = e4 if e4 > 0.0 else np.float64(0.0)
            Cn[me] = Cn[me] + fac * ((e2 - 1.0) * (W[me] - W[ot]) - e4 * (L[me] - L[ot]))
    got = em.terms(1, W)
    for name, g, w in zip(("C", "L", "nu", "r"), got, (Cn, L, nu, r)):
        assert np.array_equal(_bits(g), _bits(w)), name
    assert np.array_equal(_bits(k_e), _bits([-np.sqrt(E["x"] * E["x"] + E["y"] * E["y"] + E["z"] * E["z"]) * np.float64(np.float32(0.2)) * 0.5 for E in e]))
    em.close()


@pytest.mark.parametrize("case", ["m6_2lvl", "tet_2lvl"])
def test_reduction_to_the_reference(case, oracle):
    """Where e2 = 1 the edge's correction is exactly +-0.0: checked per edge at a kappa2 so large that the sensor saturates on
    every edge of a randomly perturbed state (asserted), and per edge on the saturated subset at the default kappa2."""
    em = jse.JstOracle(oracle, case, levels=0)
    W = _random_state(em, 0, seed=11)
    a, b, k_e = em.ea[0], em.eb[0], em.k_e[0]
    L, nu, r = jse.sensor(W, a, b)
    edge_nu = np.maximum(nu[a], nu[b])
    assert edge_nu.min() > 0.0
    big = 2.0 / edge_nu.min()
    e2, e4 = jse.switches(nu[a], nu[b], big, jse.KAPPA4)
    assert (e2 == 1.0).all() and (e4 == 0.0).all()
    for terms in jse.edge_terms(W, L, nu, r, a, b, k_e, big, jse.KAPPA4):
        assert not terms.any()                              # +0.0 or -0.0, nothing else
    Cn, _, _, _ = jse.correction(W, a, b, k_e, big, jse.KAPPA4)
    assert not Cn.any()
    # the default pair on a state with a pressure jump across half of the nodes: saturated edges contribute zero, others do not
    W2 = W.copy()
    W2[::2, 4] *= 3.0
    L, nu, r = jse.sensor(W2, a, b)
    e2, _ = jse.switches(nu[a], nu[b], jse.KAPPA2, jse.KAPPA4)
    sat = e2 == 1.0
    assert sat.any() and (~sat).any()
    c_ab, c_ba = jse.edge_terms(W2, L, nu, r, a, b, k_e, jse.KAPPA2, jse.KAPPA4)
    assert not c_ab[sat].any() and not c_ba[sat].any()
    assert c_ab[~sat].any(axis=1).all()
    em.close()


@pytest.mark.parametrize("case", ["m6_2lvl", "mixed_2lvl", "tet_2lvl"])
def test_conservation(case, oracle):
    """An edge gives its two ends exact negatives, so the sum of C over all nodes is at round-off: below n_terms * u * the
    largest |term| per variable (a sum of n_terms numbers that cancel pairwise loses at most that in any order)."""
    em = jse.JstOracle(oracle, case, levels=0)
    for k2, k4 in jse.GPU_PAIRS:
        W = _random_state(em, 0, seed=3)
        a, b, k_e = em.ea[0], em.eb[0], em.k_e[0]
        L, nu, r = jse.sensor(W, a, b)
        c_ab, c_ba = jse.edge_terms(W, L, nu, r, a, b, k_e, k2, k4)
        assert c_ab.any()
        assert np.array_equal(_bits(c_ab), _bits(-c_ba))
        Cn, _, _, _ = jse.correction(W, a, b, k_e, k2, k4)
        bound = 2 * len(a) * U * np.abs(c_ab).max(axis=0)
        print(case, k2, k4, "sum of C", Cn.sum(axis=0), "bound", bound)
        assert (np.abs(Cn.sum(axis=0)) <= bound).all()
    em.close()


def test_a_linear_field_loses_its_dissipation(oracle, tmp_path):
    """The point of the scheme, on a generated 9^3 box level (lattice connectivity, noisy areas and volumes): a state whose five
    variables are linear in the lattice indices, kappa2 = 0, kappa4 = 0.15625.

    * At every node none of whose edges reaches a hull node the undivided Laplacian is round-off: |L_i[v]| <= 64 u max|W[v]| —
      six neighbours, each difference within u max|W| of its exact value and five additions of partial sums below 6 |slope|,
      so 11 u max|W| would do; 64 leaves slack.
    * There the dissipation JST leaves, D1 + C with D1_i = sum k_e (r_i + r_j) (W_i - W_j) the first-difference term, is below
      1e-10 of that term's magnitude M_i = sum |k_e (r_i + r_j) (W_i - W_j)| (the magnitude of what is summed, not of the sum,
      which on a lattice largely cancels by itself): what is left is fac * 0.15625 * (L_i - L_j) <= fac * 0.15625 * 128 u max|W|
      against fac * |slope| with |slope| >= 1e-3 max|W| here, 4e-12, plus the rounding of the products.
    * The parent's flux carries the whole term: F(parent) - F(JST) = -C equals D1 to that accuracy, through the oracle's own
      flux kernels (up to the rounding of F itself, 64 u max|F|)."""
    import mgcfd  # noqa: F401  (the package's mesh generator)
    from mgcfd import meshgen
    n = 9
    mg = meshgen.MultigridMesh(mesh_name="fvcorr")
    mg.levels.append(meshgen.make_box_level(n, seed=4, area_noise=0.05, volume_noise=0.05))
    d = tmp_path / "box"
    os.makedirs(d / "input")
    meshgen.write_input(mg, str(d / "input"))
    (d / "case.txt").write_text("duplicate = 1\n")
    em = jse.JstOracle(oracle, str(d), kappa2=0.0, kappa4=jse.KAPPA4, levels=1)
    ijk = np.rint(em.oc.array(0, "coords").reshape(-1, 3) * (n - 1))
    assert np.abs(ijk / (n - 1) - em.oc.array(0, "coords").reshape(-1, 3)).max() < 1e-12
    ff = em.ff17[:5]
    slopes = np.array([[0.010, 0.020, -0.005], [0.020, -0.010, 0.015], [0.004, 0.008, 0.012], [-0.006, 0.010, 0.005], [0.030, 0.020, -0.010]])
    base = np.array([ff[0], ff[1], 0.3, 0.2, ff[4]])
    W = base[None, :] + ijk @ slopes.T
    assert (W[:, 0] > 0.0).all() and (jse.pressure(W) > 0.0).all()
    a, b, k_e = em.ea[0], em.eb[0], em.k_e[0]
    hull = ((ijk == 0) | (ijk == n - 1)).any(axis=1)
    touches = hull.copy()
    np.logical_or.at(touches, a, hull[b])
    np.logical_or.at(touches, b, hull[a])
    inner = ~touches
    assert inner.sum() == (n - 4) ** 3
    var = em.oc.array(0, "variables").reshape(-1, 5)
    var[:] = W
    Cn, L, nu, r = em.terms(0)
    wmax = np.abs(W).max(axis=0)
    print("max |L| / max |W| at the inner nodes, in u:", np.abs(L[inner]).max(axis=0) / wmax / U)
    assert (np.abs(L[inner]) <= 64 * U * wmax).all()
    assert (np.abs(L[hull]).max(axis=0) > 1e-3 * wmax).all()           # (... and it is not zero everywhere)
    fac = k_e * (r[a] + r[b])
    d1_ab = fac[:, None] * (W[a] - W[b])
    D1, M = np.zeros_like(W), np.zeros_like(W)
    np.add.at(D1, a, d1_ab); np.add.at(D1, b, -d1_ab)
    np.add.at(M, a, np.abs(d1_ab)); np.add.at(M, b, np.abs(d1_ab))
    left = np.abs(D1 + Cn)[inner] / M[inner]
    print("dissipation left / first-difference magnitude, max per variable:", left.max(axis=0))
    assert (left < 1e-10).all()
    f_jst = em.stage_fluxes(0)
    em.set_jst(0.0, 0.0, 0)
    f_parent = em.stage_fluxes(0)
    assert np.array_equal(_bits(f_jst), _bits(f_parent + Cn))
    carried = np.abs((f_parent - f_jst) - D1)[inner]
    slack = 1e-10 * M[inner] + 64 * U * np.abs(f_parent).max(axis=0)
    print("parent - JST against the first-difference term, max per variable:", carried.max(axis=0), "term", np.abs(D1[inner]).max(axis=0))
    assert (carried <= slack).all()
    assert (M[inner].min(axis=0) > 1e3 * slack.max(axis=0)).all()      # the term is far above what the check lets through
    em.close()


def test_local_cfl_is_the_largest_valid_one(oracle):
    """Local steps: LOCAL_CFL is the largest of LOCAL_CFLS at which every GPU case, pair and level choice stays valid."""
    valid = {}
    for cfl in jse.LOCAL_CFLS:
        ok = True
        for case in jse.GPU_CASES:
            for k2, k4 in jse.GPU_PAIRS:
                for lv in jse.GPU_LEVELS:
                    em = jse.JstOracle(oracle, case, "local", cfl, kappa2=k2, kappa4=k4, levels=lv)
                    with np.errstate(all="ignore"):
                        rc, rms = em.cycles(jse.GPU_CYCLES)
                    em.close()
                    if rc:
                        print("local", cfl, case, k2, k4, lv, "rc", rc, "after", len(rms), "cycles")
                    ok = ok and rc == 0
        valid[cfl] = ok
    print(valid)
    assert valid[jse.LOCAL_CFL]
    assert jse.LOCAL_CFL == max(c for c in jse.LOCAL_CFLS if valid[c])


@pytest.mark.parametrize("case,mode,cfl,k2,k4,lv", jse.gpu_combinations())
def test_every_gpu_combination_stays_valid(case, mode, cfl, k2, k4, lv, oracle):
    em = jse.JstOracle(oracle, case, mode, cfl, kappa2=k2, kappa4=k4, levels=lv)
    rc, rms = em.cycles(jse.GPU_CYCLES)
    print(case, mode, cfl, k2, k4, lv, "rc", rc, "rms", rms)
    assert rc == 0 and len(rms) == jse.GPU_CYCLES and np.isfinite(rms).all()
    for l in range(em.n):
        assert np.isfinite(em.variables(l)).all()
        if l < em.jst_levels:
            assert em.last[l] is not None and em.last[l][0].any()          # the correction ran on the level and is not trivially zero
        else:
            assert em.last[l] is None
    em.close()


def test_composed_runs_stay_valid(oracle):
    """The two composed runs of tests/test_gpu_jst.py: with residual smoothing, and with dual time (BDF2)."""
    mode, cfl, smoothing = jse.COMPOSED_SMOOTHING
    em = jse.JstOracle(oracle, jse.COMPOSED_CASE, mode, cfl, *smoothing, kappa2=jse.KAPPA2, kappa4=jse.KAPPA4, levels="all")
    rc, rms = em.cycles(jse.GPU_CYCLES)
    assert rc == 0 and np.isfinite(rms).all()
    em.close()
    name, mode, cfl, smoothing, order = jse.COMPOSED_DUAL
    assert (name, mode, cfl, smoothing, order) in dte.GPU_SETTINGS
    em = jse.JstOracle(oracle, jse.COMPOSED_CASE, mode, cfl, *smoothing, kappa2=jse.KAPPA2, kappa4=jse.KAPPA4, levels="all")
    v = em.oc.array(0, "variables").reshape(-1, 5)
    v[:] = dte.start_state(jse.COMPOSED_CASE, em.ff17[:5], len(v))
    em.set_dual_time(dte.GPU_DT[jse.COMPOSED_CASE][name])
    em.set_order(order)
    rc, rms = em.advance(jse.COMPOSED_DUAL_STEPS, jse.COMPOSED_DUAL_CYCLES)
    assert rc == 0 and np.isfinite(rms).all() and em.effective_order() == 2
    em.close()


def test_new_symbols_are_exported_and_typed():
    """(mgcfd_abi_version stays 1: the calls are additions, and the existing host tests pin the number.)"""
    import inspect
    import mgcfd
    lib = mgcfd.load_library()
    header = open(os.path.join(ROOT, "include", "mgcfd.h")).read()
    for name in ("mgcfd_set_jst", "mgcfd_get_jst", "mgcfd_bench_jst"):
        assert name in mgcfd.EXPORTED_SYMBOLS and hasattr(lib, name) and name + "(" in header
    assert "MGCFD_JST_KAPPA2 2.5" in header and "MGCFD_JST_KAPPA4 0.15625" in header
    sig = inspect.signature(mgcfd.Solver.set_jst).parameters
    assert [sig[k].default for k in ("kappa2", "kappa4", "levels")] == [jse.KAPPA2, jse.KAPPA4, 1]
    assert callable(mgcfd.Solver.jst) and "jst" in inspect.signature(mgcfd.Solver.polar).parameters
