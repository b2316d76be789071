"""Host tests of the upwind flux (no GPU): the numpy emulator (tests/upwind_emulator.py) with the flux off against its parent bit for
bit, the sums read literally, consistency and conservation of Roe's flux, what reconstruction is for (a linear field loses its
dissipation; second order by Richardson), the limiters' properties, the positivity fallback, the validity of every run the GPU
tests make, and the new symbols."""
import os

import numpy as np
import pytest

import cycle_emulator as ce
import dual_time_emulator as dte
import jst_emulator as jse
import upwind_emulator as ue
import viscous_emulator as ve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -52


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("upwind_host_lattices")
    return {name: ue.write_lattice(name, d) for name in ue.GPU_LATTICES}


def _case(lattices, key):
    return lattices.get(key, key)


def _box(tmp_path, n, name="box"):
    """A uniform n^3 lattice (no jitter, no noise) as a single-level case directory."""
    from mgcfd import meshgen
    mg = meshgen.MultigridMesh(mesh_name="fvcorr")
    mg.levels.append(meshgen.make_box_level(n, seed=4))
    d = tmp_path / f"{name}{n}"
    os.makedirs(d / "input")
    meshgen.write_input(mg, str(d / "input"))
    (d / "case.txt").write_text("duplicate = 1\n")
    return str(d)


def _inner(em, l, n, rings):
    """Nodes of the uniform lattice at least ``rings`` cells away from the hull, and the lattice indices of all nodes."""
    ijk = np.rint(em.X[l] * (n - 1)).astype(np.int64)
    assert np.abs(ijk / (n - 1) - em.X[l]).max() < 1e-12
    return ((ijk >= rings) & (ijk <= n - 1 - rings)).all(axis=1), ijk


def _conserved(q):
    rho, u, v, w, p = (q[:, k] for k in range(5))
    return np.stack([rho, rho * u, rho * v, rho * w, p / (ue.GAMMA - 1.0) + 0.5 * rho * (u * u + v * v + w * w)], axis=1)


def _random_states(nel, seed, mach):
    """Random positive states around Mach ``mach`` in a random direction per node."""
    rng = np.random.default_rng(seed)
    rho, p = rng.uniform(0.5, 2.0, nel), rng.uniform(0.5, 2.0, nel)
    c = np.sqrt(ue.GAMMA * p / rho)
    d = rng.normal(size=(nel, 3))
    vel = d / np.linalg.norm(d, axis=1)[:, None] * (mach * c * rng.uniform(0.8, 1.2, nel))[:, None]
    return _conserved(np.column_stack([rho, vel, p]))


@pytest.mark.parametrize("key", ue.GPU_CASES)
def test_levels_zero_is_the_parent_emulator(key, oracle, lattices):
    """levels = 0 (whatever the other arguments): CycleOracle's bits on every level and its RMS history, plain and with residual
    smoothing under local steps."""
    case = _case(lattices, key)
    for mode, cfl, smoothing in (("reference", 0.5, (0.0, 0)), ("local", 1.0, (0.5, 2))):
        want = ce.CycleOracle(oracle, case, mode, cfl, *smoothing)
        em = ue.UpwindOracle(oracle, case, mode, cfl, *smoothing)
        em.set_upwind(0, 0, "barth-jespersen", 3.0, 0.2)
        assert (em.up_levels, em.up_muscl, em.limiter, em.k, em.entropy_fix) == (0, 0, ue.NONE, 0.0, 0.0)
        rc_w, rms_w = want.cycles(ue.GPU_CYCLES)
        rc, rms = em.cycles(ue.GPU_CYCLES)
        assert rc == rc_w == 0 and np.array_equal(_bits(rms), _bits(rms_w))
        for l in range(em.n):
            assert np.array_equal(_bits(em.variables(l)), _bits(want.variables(l))), (key, mode, l)
        em.close(); want.close()


def test_the_sums_run_in_edge_order_from_plus_zero(oracle):
    """The emulator's extrema, psi and U against a plain Python loop over the edge ends (the definition read literally) on one
    level, Barth-Jespersen."""
    em = ue.UpwindOracle(oracle, "tet_2lvl")
    em.set_upwind(2, 2, "barth-jespersen")
    l = 1
    W = ue.start_state(em.oc.levels[l].nel, em.ff17[:5])
    q = ue.primitives5(W)
    to, frm, N, X = em.vto[l], em.vfrm[l], em.vN[l], em.X[l]
    vol = em.oc.array(l, "volumes")
    Ut, Gl, psi, terms, _ = em.upwind_terms(l, W)
    nel = len(q)
    A = np.zeros((nel, 5, 3))
    qmax, qmin = q.copy(), q.copy()
    for e in range(len(to)):
        i, j = to[e], frm[e]
        for v in range(5):
            A[i, v] = A[i, v] + (q[j, v] - q[i, v]) * N[e]
            if q[j, v] > qmax[i, v]: qmax[i, v] = q[j, v]
            if q[j, v] < qmin[i, v]: qmin[i, v] = q[j, v]
    G = (0.5 * A) / vol[:, None, None]
    want_psi = np.ones((nel, 5))
    for e in range(len(to)):
        i, j = to[e], frm[e]
        dx = X[j] - X[i]
        for v in range(5):
            d2 = 0.5 * ((G[i, v, 0] * dx[0] + G[i, v, 1] * dx[1]) + G[i, v, 2] * dx[2])
            t = 1.0
            if d2 > 0.0 or d2 < 0.0:
                d1 = (qmax[i, v] if d2 > 0.0 else qmin[i, v]) - q[i, v]
                r = d1 / d2
                t = r if r < 1.0 else 1.0
            if t < want_psi[i, v]: want_psi[i, v] = t
    assert np.array_equal(_bits(psi), _bits(want_psi))
    assert np.array_equal(_bits(Gl), _bits(want_psi[:, :, None] * G))
    want_U = np.zeros((nel, 5))
    for e in range(len(to)):
        want_U[to[e]] = want_U[to[e]] + terms[e]
    assert np.array_equal(_bits(Ut), _bits(want_U))
    em.close()


def test_consistency():
    """Phi(q, q, m) = area * Fn(q).  With qa = qb every difference is exactly +0.0, so a1, a2, a3 and the shear factors multiply
    exact zeros: D is +-0.0 and Phi = area * (0.5 * (Fn + Fn) - 0.5 * 0.0) — the doubling, the halving and the subtraction of zero
    are exact, so the two sides agree BIT FOR BIT with the emulator's own Fn (bound 0).  Against the Euler flux evaluated
    independently in long double from the same states the difference is the rounding of Fn's operations: per component at most
    12 roundings on the chain area -> nh -> un -> rho*un -> product -> sum -> area * ..., each relative to a term bounded by the
    magnitude M = area * (rho (|u nhx| + |v nhy| + |w nhz|) (1 + |u| + |v| + |w| + |H|) + |p|), so 16 u M is a bound with slack."""
    rng = np.random.default_rng(2)
    n = 4000
    for mach in (0.3, 2.5):
        W = _random_states(n, 5, mach)
        q = ue.primitives5(W)
        m = rng.normal(size=(n, 3)) * 1e-2
        for fix in (0.0, 0.1):
            Phi, area, Fa, Fb, D = ue.roe(q, q, m, fix, parts=True)
            assert not D.any()
            assert np.array_equal(_bits(Phi), _bits(area[:, None] * Fa))
        L = np.longdouble
        ql, ml = q.astype(L), m.astype(L)
        ar = np.sqrt((ml ** 2).sum(axis=1))
        nh = ml / ar[:, None]
        un = (ql[:, 1:4] * nh).sum(axis=1)
        E = ql[:, 4] / L(ue.GAMMA - 1.0) + L(0.5) * ql[:, 0] * (ql[:, 1:4] ** 2).sum(axis=1)
        exact = ar[:, None] * np.column_stack([ql[:, 0] * un, (ql[:, 0] * un)[:, None] * ql[:, 1:4] + ql[:, 4][:, None] * nh, (E + ql[:, 4]) * un])
        H = np.abs((E + ql[:, 4]) / ql[:, 0])
        una = (np.abs(ql[:, 1:4] * nh)).sum(axis=1)                # (un's own rounding is relative to the magnitude of its three products)
        M = ar * (ql[:, 0] * una * (1.0 + np.abs(ql[:, 1:4]).sum(axis=1) + H) + np.abs(ql[:, 4]))
        err = (np.abs(Phi.astype(L) - exact) / M[:, None]).max()
        print("mach", mach, "max |Phi - exact| / M in u:", float(err / U))
        assert err <= 16 * U


def test_the_sign_of_u_is_the_references(oracle, tmp_path):
    """The reference's fluxes hold MINUS the outflow, so U must enter with the sign of its internal loop.  Kernel and emulator
    would agree bit for bit with either sign, and consistency, conservation and the order would pass; this pins it.  On a closed
    uniform lattice (9^3, h = 1/8, every dual face an exact power of two) at the uniform far field the far-field faces' B and the
    internal edges' U cancel: every node's F = B + U is a sum of at most seven terms of size <= max|U| that cancel exactly in
    exact arithmetic, so |F| <= 16 u max|U| per variable (eight roundings of partial sums below 2 max|U|).  With the other sign
    F would be 2 B, as large as max|U| itself at the hull.  The reference's own scheme closes the same way; first order and
    MUSCL alike."""
    em = ue.UpwindOracle(oracle, _box(tmp_path, 9))
    for muscl in (0, 1):
        em.set_upwind(1, muscl, "venkatakrishnan")
        F = em.stage_fluxes(0)
        Ut = em.last_U[0]
        umax = np.abs(Ut).max(axis=0)
        print("muscl", muscl, "max |B + U|", np.abs(F).max(axis=0), "max |U|", umax)
        assert (umax > 1e-3).all()                              # (the hull nodes' U is not small: the check has something to cancel)
        assert (np.abs(F).max(axis=0) <= 16 * U * umax).all()
        assert (np.abs((F - Ut) - Ut).max(axis=0) > 0.5 * umax).all()      # B - U, what the other sign would leave
    em.set_upwind(0)
    assert (np.abs(em.stage_fluxes(0)).max(axis=0) <= 16 * U * umax).all()
    em.close()


def test_an_empty_coordinate_array_is_no_coordinates():
    """mgcfd.Mesh.level hands out coords of shape (0, 3) for a level loaded without its .coords file; the level descriptors
    built from such a dict carry a null pointer (the library then knows the level has none), never the address of an empty
    buffer that the library would read 3 * nel doubles from."""
    from mgcfd import api
    L = {"nel": 2, "volumes": np.ones(2), "edges": np.zeros(0, dtype=api.EDGE_DTYPE), "n_internal": 0, "n_boundary": 0, "n_wall": 0}
    for coords, null in ((np.zeros((0, 3)), True), (None, True), (np.zeros((2, 3)), False)):
        descs, keep = api._level_descs([dict(L, coords=coords)])
        assert (not descs[0].coords) == null


@pytest.mark.parametrize("key", ["B", "tet_2lvl"])
def test_conservation(key, oracle, lattices):
    """On random sub- and supersonic states the two ends of every edge carry exact negatives — every limiter, first order and
    MUSCL — so the sum of U over the nodes is at round-off (below n_terms * u * the largest |term| per variable)."""
    em = ue.UpwindOracle(oracle, _case(lattices, key))
    nel = em.oc.levels[0].nel
    for mach in (0.4, 2.0):
        W = _random_states(nel, 9, mach)
        for limiter in ue.GPU_LIMITERS:
            for muscl in (0, 1):
                em.set_upwind(1, muscl, limiter)
                Ut, _, _, terms, fb = em.upwind_terms(0, W)
                assert np.isfinite(terms).all() and terms.any()
                assert np.array_equal(_bits(terms[0::2]), _bits(-terms[1::2])), (key, mach, limiter, muscl)
                bound = len(terms) * U * np.abs(terms).max(axis=0)
                assert (np.abs(Ut.sum(axis=0)) <= bound).all()
    em.close()


def _linear_state(X):
    slopes = np.array([[0.10, 0.20, -0.05], [0.20, -0.10, 0.15], [0.04, 0.08, 0.12], [-0.06, 0.10, 0.05], [0.30, 0.20, -0.10]])
    base = np.array([1.4, 0.9, 0.3, 0.2, 1.0])
    return base[None, :] + X @ slopes.T, slopes


def test_a_linear_field_is_reconstructed_exactly(oracle, tmp_path):
    """A uniform 9^3 lattice (h = 1/8), q linear in the coordinates, no limiter.

    * At every node one cell or more from the hull G is exact to rounding: six differences of size |slope| h, each within
      u max|q| of its exact value, times n (exact powers of two here), five additions, one halving and one division:
      |G - slope| <= 64 u max|q| / h, with slack, as tests/test_host_jst.py bounds its Laplacian.
    * At every edge between two such nodes qL and qR agree to rounding: both are q at the midpoint, each off by at most
      0.5 h * 3 * (64 u max|q| / h) + 4 u max|q|, so |qR - qL| <= 256 u max|q|.
    * There the dissipation is that of a jump of 256 u max|q| in place of one of |slope| h: D(MUSCL) <= B * D_first with
      B = 256 u max|q| / (min|slope| h) * kappa, kappa = 64 covering the ratio of the largest to the smallest wave strength per
      unit jump (the state is subsonic: |lambda| between 0.1 c and 2 c after the entropy fix) — B is about 1e-9 here; measured in
      the sum of the edge's |D| components against the first-order sum.
    * Venkatakrishnan on the same field: psi <= 1 everywhere and psi -> 1 at the inner nodes: there d1 = 2 d2 up to rounding,
      where the function is (4 + 4 + e) / (4 + 4 + e) with e = e2 / d2^2 in both, 1 up to the rounding of its nine operations
      (16 u).  Barth-Jespersen is exactly 1 there (min(1, 2))."""
    n = 9
    em = ue.UpwindOracle(oracle, _box(tmp_path, n))
    inner, _ = _inner(em, 0, n, 1)
    assert inner.sum() == (n - 2) ** 3
    q, slopes = _linear_state(em.X[0])
    W = _conserved(q)
    q = ue.primitives5(W)                                       # (what the scheme sees: linear up to the rounding of W)
    to, frm, N, X = em.vto[0], em.vfrm[0], em.vN[0], em.X[0]
    vol = em.oc.array(0, "volumes")
    h = 1.0 / (n - 1)
    qm = np.abs(q).max(axis=0)
    Gl, psi, G, _, _ = ue.gradient_pass(q, X, to, frm, N, vol, ue.NONE, ue.VENKAT_K)
    errG = np.abs(G[inner] - slopes[None]).max(axis=(0, 2))
    print("max |G - slope| h / max|q| at the inner nodes, in u:", errG * h / qm / U)
    assert (errG <= 64 * U * qm / h).all()
    both = inner[to] & inner[frm]
    qL, qR, fb = ue.reconstruct(q, Gl, X, to, frm)
    assert not fb.any()
    jump = np.abs(qR - qL)[both].max(axis=0)
    print("max |qR - qL| / max|q| at the inner edges, in u:", jump / qm / U)
    assert (jump <= 256 * U * qm).all()
    pos = ue.orientation(N)
    m = np.where(pos[:, None], N, -N)

    def dissipation(a, b):
        _, _, _, _, D = ue.roe(np.where(pos[:, None], a, b), np.where(pos[:, None], b, a), m, ue.ENTROPY_FIX, parts=True)
        return np.abs(D).sum(axis=1)

    d_first, d_muscl = dissipation(q[to], q[frm])[both], dissipation(qL, qR)[both]
    B = 256 * U * qm.max() / (np.abs(slopes).min() * h) * 64
    print("D(MUSCL) / D(first order) at the inner edges: max", (d_muscl / d_first).max(), "bound", B)
    assert d_first.min() > 0.0 and (d_muscl <= B * d_first).all() and B < 1e-8
    for limiter in (ue.BARTH_JESPERSEN, ue.VENKATAKRISHNAN):
        _, psi, _, _, _ = ue.gradient_pass(q, X, to, frm, N, vol, limiter, ue.VENKAT_K)
        assert (psi <= 1.0).all() and (psi > 0.0).all()
        print("limiter", limiter, "min psi at the inner nodes", psi[inner].min(), "overall", psi.min())
        if limiter == ue.BARTH_JESPERSEN:
            # d1 / d2 is 2 up to rounding along every edge of a linear field: the neighbour's value against the midpoint's
            assert (psi[inner] == 1.0).all()
        else:
            assert (1.0 - psi[inner]).max() <= 16 * U
    em.close()


def test_barth_jespersen_keeps_the_reconstruction_inside_the_extrema(oracle, lattices):
    """A step profile (two constant states, the jump across x = 0.5, on the jittered lattice B): every reconstructed value of a
    node lies inside its [qmin, qmax] up to the rounding of the reconstruction itself (4 u max|q|: the dot product's three
    roundings and the addition); unlimited reconstruction leaves the interval by far more than that."""
    em = ue.UpwindOracle(oracle, lattices["B"])
    X, to, frm, N = em.X[0], em.vto[0], em.vfrm[0], em.vN[0]
    vol = em.oc.array(0, "volumes")
    left, right = np.array([1.4, 0.9, 0.1, 0.0, 1.0]), np.array([0.7, 1.3, -0.1, 0.2, 0.4])
    q = ue.primitives5(_conserved(np.where((X[:, 0] < 0.5)[:, None], left, right)))
    tol = 4 * U * np.abs(q).max(axis=0)
    out = {}
    for limiter in (ue.BARTH_JESPERSEN, ue.NONE):
        Gl, psi, _, qmin, qmax = ue.gradient_pass(q, X, to, frm, N, vol, limiter, ue.VENKAT_K)
        dx = (X[frm] - X[to])[:, None, :]
        rec = q[to] + 0.5 * ue.dot3(Gl[to], dx)
        out[limiter] = np.maximum(rec - qmax[to], qmin[to] - rec).max(axis=0)
    print("overshoot, Barth-Jespersen:", out[ue.BARTH_JESPERSEN], "unlimited:", out[ue.NONE])
    assert (out[ue.BARTH_JESPERSEN] <= tol).all()
    assert (out[ue.NONE] > 1e6 * tol).all()
    em.close()


def test_venkatakrishnan_never_exceeds_one(oracle, lattices):
    """psi <= 1 on the perturbed and the supersonic start states of every GPU case, and below 1 somewhere on the lattices."""
    for key in ue.GPU_CASES:
        em = ue.UpwindOracle(oracle, _case(lattices, key))
        em.set_upwind(1, 1, "venkatakrishnan")
        for W in (ue.start_state(em.oc.levels[0].nel, em.ff17[:5]), ue.supersonic_state(em.oc.levels[0].nel, em.ff17[:5])):
            _, _, psi, _, _ = em.upwind_terms(0, W)
            assert (psi <= 1.0).all() and np.isfinite(psi).all()
            if key in ue.GPU_LATTICES:
                assert (psi < 1.0).any()
        em.close()


def _smooth_state(X):
    s = np.sin(2.0 * np.pi * X)
    c = np.cos(2.0 * np.pi * X)
    q = np.column_stack([1.4 + 0.2 * s[:, 0] * c[:, 1], 0.8 + 0.1 * c[:, 0] * s[:, 2], 0.3 + 0.1 * s[:, 1], 0.2 + 0.1 * c[:, 2] * s[:, 0],
                         1.0 + 0.2 * c[:, 0] * c[:, 1] * s[:, 2]])
    return _conserved(q)


def test_observed_order(oracle, tmp_path):
    """The residual per volume U_i / vol_i of a smooth non-linear state on three nested uniform lattices (9^3, 17^3, 33^3), at the
    nodes of the coarsest one two of its cells or more from the hull, by Richardson: p = log2(|R_h - R_h/2| / |R_h/2 - R_h/4|)
    in the root mean square over those nodes and the five variables.  First order stays below 1.5 and unlimited MUSCL above it —
    the midpoint of the theoretical 1 and 2."""
    sizes = (9, 17, 33)
    R = {0: [], 1: []}
    for n in sizes:
        em = ue.UpwindOracle(oracle, _box(tmp_path, n))
        step = (n - 1) // (sizes[0] - 1)
        inner, ijk = _inner(em, 0, n, 2 * step)
        pick = inner & (ijk % step == 0).all(axis=1)
        order = np.lexsort((ijk[pick, 2], ijk[pick, 1], ijk[pick, 0]))
        assert pick.sum() == (sizes[0] - 4) ** 3
        W = _smooth_state(em.X[0])
        vol = em.oc.array(0, "volumes")
        for muscl in (0, 1):
            em.set_upwind(1, muscl, "none")
            Ut, _, _, _, fb = em.upwind_terms(0, W)
            assert not fb.any()
            R[muscl].append((Ut / vol[:, None])[pick][order])
        em.close()
    p = {}
    for muscl in (0, 1):
        d1 = np.sqrt(((R[muscl][0] - R[muscl][1]) ** 2).mean())
        d2 = np.sqrt(((R[muscl][1] - R[muscl][2]) ** 2).mean())
        p[muscl] = float(np.log2(d1 / d2))
    print("observed order: first order", p[0], "unlimited MUSCL", p[1])
    assert p[0] < 1.5 < p[1]


def test_the_positivity_fallback(oracle, lattices):
    """A constructed edge: one node of lattice B with a density a thousand times its neighbours'.  Unlimited reconstruction takes
    the density at some of its edges below zero: exactly those ends (and their twins) fall back to qL = q_i, qR = q_j in ALL
    variables; the others keep their reconstruction; U stays finite; with Barth-Jespersen no end falls back."""
    em = ue.UpwindOracle(oracle, lattices["B"])
    X, to, frm, N = em.X[0], em.vto[0], em.vfrm[0], em.vN[0]
    vol = em.oc.array(0, "volumes")
    nel = em.oc.levels[0].nel
    qc = np.tile(np.array([1.4, 0.9, 0.1, 0.0, 1.0]), (nel, 1))
    centre = int(np.argmin(np.linalg.norm(X - 0.5 + 0.11, axis=1)))
    qc[centre, 0] *= 1000.0
    q = ue.primitives5(_conserved(qc))
    Gl, _, _, _, _ = ue.gradient_pass(q, X, to, frm, N, vol, ue.NONE, ue.VENKAT_K)
    qL, qR, fb = ue.reconstruct(q, Gl, X, to, frm)
    dx = (X[frm] - X[to])[:, None, :]
    rL, rR = q[to] + 0.5 * ue.dot3(Gl[to], dx), q[frm] - 0.5 * ue.dot3(Gl[frm], dx)
    bad = ~((rL[:, 0] > 0) & (rL[:, 4] > 0) & (rR[:, 0] > 0) & (rR[:, 4] > 0))
    assert bad.any() and not bad.all() and np.array_equal(fb, bad)
    assert np.array_equal(fb[0::2], fb[1::2])                   # both ends of an edge decide alike
    assert np.array_equal(_bits(qL[fb]), _bits(q[to][fb])) and np.array_equal(_bits(qR[fb]), _bits(q[frm][fb]))
    assert np.array_equal(_bits(qL[~fb]), _bits(rL[~fb])) and np.array_equal(_bits(qR[~fb]), _bits(rR[~fb]))
    W = _conserved(qc)
    em.set_upwind(1, 1, "none")
    Ut, _, _, terms, fb2 = em.upwind_terms(0, W)
    assert np.array_equal(fb2, fb) and np.isfinite(Ut).all()
    em.set_upwind(1, 1, "barth-jespersen")
    assert not em.upwind_terms(0, W)[4].any()
    em.close()


def test_local_cfl_is_the_largest_valid_one(oracle, lattices):
    """Local steps: LOCAL_CFL is the largest of LOCAL_CFLS at which every run of gpu_runs()'s cases and level choices stays valid."""
    valid = {}
    for cfl in ue.LOCAL_CFLS:
        ok = True
        for key in ue.GPU_CASES:
            for lv in ue.GPU_LEVELS:
                for m in ue.GPU_MUSCL:
                    if lv == 1 and m == "all":
                        continue
                    em = ue.configured(oracle, _case(lattices, key), "local", cfl, lv, m)
                    with np.errstate(all="ignore"):
                        rc, rms = em.cycles(ue.GPU_CYCLES)
                    em.close()
                    if rc:
                        print("local", cfl, key, lv, m, "rc", rc, "after", len(rms), "cycles")
                    ok = ok and rc == 0
        valid[cfl] = ok
    print(valid)
    assert valid[ue.LOCAL_CFL]
    assert ue.LOCAL_CFL == max(c for c in ue.LOCAL_CFLS if valid[c])


@pytest.mark.parametrize("key,mode,cfl,lv,muscl", ue.gpu_runs())
def test_every_gpu_run_stays_valid(key, mode, cfl, lv, muscl, oracle, lattices):
    em = ue.configured(oracle, _case(lattices, key), mode, cfl, lv, muscl)
    rc, rms = em.cycles(ue.GPU_CYCLES)
    assert rc == 0 and len(rms) == ue.GPU_CYCLES and np.isfinite(rms).all()
    for l in range(em.n):
        assert np.isfinite(em.variables(l)).all()
        assert (em.last_U[l] is not None and em.last_U[l].any()) == (l < em.up_levels)
        assert (em.last_Gl[l] is not None) == (l < em.up_muscl)
    em.close()


@pytest.mark.parametrize("name,mode,cfl,smoothing,order,fas,viscous,cycle", ue.COMPOSED, ids=[c[0] for c in ue.COMPOSED])
def test_composed_runs_stay_valid(name, mode, cfl, smoothing, order, fas, viscous, cycle, oracle, lattices):
    rc, rms = _composed_run(oracle, lattices["A"], mode, cfl, smoothing, order, fas, viscous, cycle)
    assert rc == 0 and np.isfinite(rms).all()


def _composed_run(oracle, case, mode, cfl, smoothing, order, fas, viscous, cycle):
    em = ue.configured(oracle, case, mode, cfl, "all", 1, smoothing=smoothing, fas=fas)
    if viscous:
        em.set_viscous(ve.CELL_RE_MU, ve.PRANDTL, 1, ve.VISCOUS_CFL, "all")
    if cycle:
        em.set_cycle(cycle[0], [1] * em.n, [cycle[1]] + [1] * (em.n - 1))
    with np.errstate(all="ignore"):
        if order is None:
            rc, rms = em.cycles(ue.GPU_CYCLES)
        else:
            em.set_dual_time(dte.pick_dt(oracle, case, mode, cfl))
            em.set_order(order)
            rc, rms = em.advance(ue.DUAL_STEPS, ue.DUAL_CYCLES)
    em.close()
    return rc, rms


def test_composed_cfls_are_the_largest_valid_ones(oracle, lattices):
    """Every composed run's CFL is the largest of its candidate list at which it stays valid: COMPOSED_CFLS for the unsmoothed
    runs, SMOOTHED_CFLS for the smoothed one.  (The whole runs' ("reference", 0.5) is no choice: that mode is the reference's own
    step with the literal 0.5 it hard-codes; their local CFL is test_local_cfl_is_the_largest_valid_one's.)"""
    for name, mode, cfl, smoothing, order, fas, viscous, cycle in ue.COMPOSED:
        candidates = ue.SMOOTHED_CFLS if smoothing[1] else ue.COMPOSED_CFLS
        valid = {c: _composed_run(oracle, lattices["A"], mode, c, smoothing, order, fas, viscous, cycle)[0] == 0 for c in candidates}
        print(name, valid)
        assert cfl in candidates and cfl == max(c for c in candidates if valid[c]), name


def test_kernel_states_are_valid(oracle, lattices):
    """The two start states of tests/test_gpu_upwind.py::test_kernels on every case and on the coarsest level: positive, finite U,
    the supersonic one above Mach 1.5 everywhere."""
    for key in ue.GPU_CASES:
        em = ue.UpwindOracle(oracle, _case(lattices, key))
        for l in (0, em.n - 1):
            for W in (ue.start_state(em.oc.levels[l].nel, em.ff17[:5]), ue.supersonic_state(em.oc.levels[l].nel, em.ff17[:5])):
                q = ue.primitives5(W)
                assert (q[:, 0] > 0).all() and (q[:, 4] > 0).all()
                for limiter in ue.GPU_LIMITERS:
                    em.set_upwind(em.n, em.n, limiter)
                    assert np.isfinite(em.upwind_terms(l, W)[0]).all()
            assert (np.sqrt((q[:, 1:4] ** 2).sum(axis=1)) / np.sqrt(ue.GAMMA * q[:, 4] / q[:, 0])).min() > 1.5
        em.close()


def test_the_setter_refuses_without_a_device():
    """What needs no device: a null solver is refused by every entry point, and the symbols, constants and array names exist."""
    import ctypes as C
    import mgcfd
    from mgcfd import api
    lib = mgcfd.load_library()
    for name in ("mgcfd_set_upwind", "mgcfd_get_upwind", "mgcfd_bench_upwind"):
        assert name in mgcfd.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.mgcfd_set_upwind(None, 1, 1, 2, 5.0, 0.1) == 1
    assert lib.mgcfd_get_upwind(None, None, None, None, None, None) == 1
    t = C.c_double(0.0)
    assert lib.mgcfd_bench_upwind(None, 0, 0, 1, C.byref(t)) == 1
    assert api.ARR["upwind_gradient"] == ue.ARR_UPWIND_GRADIENT and api.ARR["upwind_limiter"] == ue.ARR_UPWIND_LIMITER
    assert api.NCOLS["upwind_gradient"] == 15 and api.NCOLS["upwind_limiter"] == 5
    assert api.LIMITERS == ue.LIMITERS and (api.UPWIND_VENKAT_K, api.UPWIND_ENTROPY_FIX) == (ue.VENKAT_K, ue.ENTROPY_FIX)
    header = open(os.path.join(ROOT, "include", "mgcfd.h")).read()
    for text in ("#define MGCFD_LIMITER_NONE 0", "#define MGCFD_LIMITER_BARTH_JESPERSEN 1", "#define MGCFD_LIMITER_VENKATAKRISHNAN 2",
                 "#define MGCFD_UPWIND_VENKAT_K 5.0", "#define MGCFD_UPWIND_ENTROPY_FIX 0.1", "#define MGCFD_ARR_UPWIND_GRADIENT 25",
                 "#define MGCFD_ARR_UPWIND_LIMITER 26"):
        assert text in header
