"""The yardstick of the fast mode's accuracy (MGCFD_OPT_EXACT = 0): the flux sums and one smoothing sweep of a level in numpy
``longdouble`` (64 significand bits on x86: 2^-11 of a double's rounding unit), written from the expressions of
oracle/mgcfd_oracle.c — not from the kernels — with every product of the reference's expressions kept apart, so that beside each
node's sum S there is its MAGNITUDE A: the sum of the absolute values of the products S is made of.

    K(got)       = |got - S| / (2^-53 * A)      per node and component
    K_sweep(got) = |got - W_3| / (2^-53 * D)    D = |old| + sum_j |sf / rk_div_j| * A_j

K is the error in units of "one rounding of the largest thing that was added": a correctly rounded evaluation of an n-term sum
stays below n, the oracle's double evaluation measures 3 to 5 on the levels the tests use (tests/test_host_fast_accuracy.py
asserts <= 8), and a kernel whose reciprocal lost three digits measures a thousand — where the whole-array metric of the other
fast-mode tests, max |difference| / max |value|, still reads 1e-13.

The three edge classes, in the oracle's names: "internal" (ora_compute_flux_edge), "wall" (solid wall, neighbour code -1:
ora_compute_boundary_flux_edge) and "far" (far field, code -2: ora_compute_wall_flux_edge).

Host only: numpy, the CPU oracle and libm.  tests/test_host_fast_accuracy.py and tests/test_gpu_fast_accuracy.py share it.
"""
import ctypes as C

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, ("numpy.longdouble has %d significand bits here: it is no high-precision reference for fp64 "
                                  "(the accuracy tests need an extended type, 63 bits or more)" % np.finfo(LD).nmant)

U = LD(2.0) ** -53                                  # a double's rounding unit
GAMMA = LD(np.float64(1.4))                         # the reference's constants are doubles (src/Base/const.h:9)
K_SMOOTHING = LD(np.float64(np.float32(0.2)))       # src/Base/common.h:24: a float literal widened to double
CLASSES = ("internal", "wall", "far")
STATES = ("perturbed", "uniform", "wide", "at_rest")
RK = 3


# ------------------------------------------------------------------------------------------------------------------
# A level as the kernels see it
# ------------------------------------------------------------------------------------------------------------------
class RefLevel:
    """One level: edge records AFTER ora_adjust_ewt / ora_dampen_ewt (m6wing: damping 5e-8; fvcorr: neither), volumes, far
    field.  ``from_dict`` takes what mgcfd.generated_to_levels / Mesh.level give and adjusts the weights with the oracle."""

    def __init__(self, nel, edges, n_internal, n_boundary, n_wall, volumes, ff, variant):
        self.nel, self.edges, self.variant = int(nel), np.ascontiguousarray(edges), int(variant)
        self.n_internal, self.n_boundary, self.n_wall = int(n_internal), int(n_boundary), int(n_wall)
        self.volumes = np.ascontiguousarray(volumes, dtype=np.float64)
        self.ff = ff
        self.ff_var = np.array(list(ff.var))
        # the far field's three-vectors per component: momenta for the density, then fc_mx, fc_my, fc_mz, fc_de
        self.ff_T = np.array([list(ff.var[1:4]), list(ff.fc_mx), list(ff.fc_my), list(ff.fc_mz), list(ff.fc_de)]).astype(LD)

    @classmethod
    def from_dict(cls, oracle, L, variant):
        lib = oracle.load()
        edges = np.ascontiguousarray(L["edges"]).copy()
        damping = {2: 5e-8, 3: 1e-7, 4: 2e-7}.get(int(variant), 0.0)           # euler3d_cpu_double.cpp:337-352
        if damping:
            coords = np.ascontiguousarray(L["coords"], dtype=np.float64)
            lib.ora_adjust_ewt(oracle.ptr(coords), len(edges), oracle.ptr(edges))
            lib.ora_dampen_ewt(len(edges), oracle.ptr(edges), damping)
        return cls(L["nel"], edges, L["n_internal"], L["n_boundary"], L["n_wall"], L["volumes"], oracle.farfield(), variant)

    def span(self, cls_name):
        ni, nb, nw = self.n_internal, self.n_boundary, self.n_wall
        return {"internal": (0, ni), "wall": (ni, nb), "far": (ni + nb, nw)}[cls_name]


# ------------------------------------------------------------------------------------------------------------------
# States
# ------------------------------------------------------------------------------------------------------------------
def make_state(kind, nel, ff_var, seed):
    """The four states of the accuracy tests, seeded; each passes ora_check_for_invalid_variables."""
    ff_var = np.asarray(ff_var, dtype=np.float64)
    if kind == "perturbed":
        from conftest import perturbed_state
        return perturbed_state(nel, ff_var, seed)
    if kind == "uniform":
        return np.tile(ff_var, (nel, 1))
    rng = np.random.default_rng(seed)
    if kind == "at_rest":
        q = np.tile(ff_var, (nel, 1)) * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, (nel, 5)))
        q[:, 1:4] = 0.0                                # +0.0: fast_sqrt's x == 0 branch
        return q
    assert kind == "wide"
    g = 1.4
    rho = 10.0 ** rng.uniform(-2.0, 2.0, nel)
    p = 10.0 ** rng.uniform(-2.0, 2.0, nel)
    mach = rng.uniform(0.0, 3.0, nel)
    d = rng.normal(size=(nel, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    v = d * (mach * np.sqrt(g * p / rho))[:, None]
    v[::7] = 0.0                                       # every seventh node exactly at rest
    q = np.empty((nel, 5))
    q[:, 0] = rho
    q[:, 1:4] = rho[:, None] * v
    q[:, 4] = p / (g - 1.0) + 0.5 * rho * (v * v).sum(axis=1)
    return q


# ------------------------------------------------------------------------------------------------------------------
# The reference, in long double
# ------------------------------------------------------------------------------------------------------------------
def point(q):
    """load_point + sound_speed + flux_contributions (oracle/mgcfd_oracle.c:37-78): T[n, component, axis]."""
    q = np.asarray(q).astype(LD).reshape(-1, 5)
    rho, m, en = q[:, 0], q[:, 1:4], q[:, 4]
    v = m / rho[:, None]
    speed_sqd = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
    p = (GAMMA - LD(1.0)) * (en - LD(0.5) * rho * speed_sqd)
    c = np.sqrt(GAMMA * p / rho)
    T = np.empty((len(q), 5, 3), dtype=LD)
    T[:, 0, :] = m                                                   # density: the momentum
    for k in range(3):                                               # momentum k: v_k * m + p on the diagonal
        T[:, 1 + k, :] = v[:, k][:, None] * m
        T[:, 1 + k, k] += p
    T[:, 4, :] = v * (en + p)[:, None]                               # energy: v * (E + p)
    return {"q": q, "p": p, "c": c, "speed": np.sqrt(speed_sqd), "T": T}


def class_sums(level, q):
    """{class: (S, A)}: per node and component the sum of the class's contributions and of the magnitudes of their products."""
    P = point(q)
    Q, T = P["q"], P["T"]
    out = {}
    e = level.edges
    # internal edges, flux_kernel.elemfunc.c:130-189: end a gets factor * (A - B) + f . (T_a + T_b), end b the negative
    s, n = level.span("internal")
    a, b = e["a"][s:s + n], e["b"][s:s + n]
    w = np.stack([e["x"][s:s + n], e["y"][s:s + n], e["z"][s:s + n]], axis=1).astype(LD)
    ewt = np.sqrt(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2])
    factor = -ewt * K_SMOOTHING * LD(0.5) * (P["speed"][a] + P["speed"][b] + P["c"][a] + P["c"][b])
    f = LD(-0.5) * w
    diss = factor[:, None] * (Q[a] - Q[b])
    ta = f[:, None, :] * T[a]                                        # [edge, component, axis]
    tb = f[:, None, :] * T[b]
    contrib = diss + ta.sum(axis=2) + tb.sum(axis=2)
    mag = np.abs(diss) + np.abs(ta).sum(axis=2) + np.abs(tb).sum(axis=2)
    S, A = np.zeros((level.nel, 5), dtype=LD), np.zeros((level.nel, 5), dtype=LD)
    np.add.at(S, a, contrib)
    np.subtract.at(S, b, contrib)
    np.add.at(A, a, mag)
    np.add.at(A, b, mag)
    out["internal"] = (S, A)
    # solid walls, flux_boundary_kernel.elemfunc.c:37-64: e * p on the momenta, 0.0 on density and energy
    s, n = level.span("wall")
    b = e["b"][s:s + n]
    w = np.stack([e["x"][s:s + n], e["y"][s:s + n], e["z"][s:s + n]], axis=1).astype(LD)
    contrib = np.zeros((n, 5), dtype=LD)
    contrib[:, 1:4] = w * P["p"][b][:, None]
    S, A = np.zeros((level.nel, 5), dtype=LD), np.zeros((level.nel, 5), dtype=LD)
    np.add.at(S, b, contrib)
    np.add.at(A, b, np.abs(contrib))
    out["wall"] = (S, A)
    # far-field faces, flux_wall_kernel.elemfunc.c:51-88: f . (T_ff + T_b) with f = 0.5 e
    s, n = level.span("far")
    b = e["b"][s:s + n]
    f = LD(0.5) * np.stack([e["x"][s:s + n], e["y"][s:s + n], e["z"][s:s + n]], axis=1).astype(LD)
    tf = f[:, None, :] * level.ff_T[None, :, :]
    tb = f[:, None, :] * T[b]
    S, A = np.zeros((level.nel, 5), dtype=LD), np.zeros((level.nel, 5), dtype=LD)
    np.add.at(S, b, tf.sum(axis=2) + tb.sum(axis=2))
    np.add.at(A, b, np.abs(tf).sum(axis=2) + np.abs(tb).sum(axis=2))
    out["far"] = (S, A)
    return out


def accumulate(sums, classes, f0=None):
    """(S, A) of the classes of ``classes`` added onto ``f0`` (None: from zero)."""
    nel = len(sums["internal"][0])
    S = np.zeros((nel, 5), dtype=LD) if f0 is None else np.asarray(f0).astype(LD).reshape(nel, 5).copy()
    A = np.abs(S)
    for c in classes:
        S = S + sums[c][0]
        A = A + sums[c][1]
    return S, A


def K(got, S, A, f0=None):
    """|got - S| / (2^-53 A) as float64 [nel, 5].  Where A = 0 nothing was added: got must be f0 (or zero) exactly, which
    reads 0 there when it holds and inf when it does not."""
    got = np.asarray(got, dtype=np.float64).reshape(S.shape)
    err = np.abs(got.astype(LD) - S)
    k = np.zeros(S.shape, dtype=np.float64)
    pos = A > 0
    k[pos] = (err[pos] / (U * A[pos])).astype(np.float64)
    base = np.zeros(S.shape) if f0 is None else np.asarray(f0, dtype=np.float64).reshape(S.shape)
    k[~pos & (got != base)] = np.inf
    return k


def step_factor(level, q, mode, cfl=0.5):
    """compute_step_factor (oracle/mgcfd_oracle.c:213-242) in long double.  ``mode``: "reference" (what the mesh name selects:
    the global minimum, or fvcorr's local formula) or "local" (sf_i = cfl * cbrt(vol_i) / (speed_i + c_i) / vol_i)."""
    P = point(q)
    vol = level.volumes.astype(LD)
    s = P["speed"] + P["c"]
    cfl = LD(np.float64(cfl))
    if mode == "reference" and level.variant == 0:
        return cfl / (np.sqrt(vol) * s)
    dt = cfl * (np.cbrt(vol) / s)
    if mode == "local":
        return dt / vol
    assert mode == "reference"
    return dt.min() / vol


def sweep(level, q, mode="reference", cfl=0.5):
    """One smoothing sweep (euler3d_cpu_double.cpp:383-508): W_j = old + sf / rk_div_j * F(W_{j-1}), residual W_3 - old.
    Returns sf, W (the state after the sweep), res, D and whether every stage's state stayed valid in the reference."""
    old = np.asarray(q).astype(LD).reshape(-1, 5)
    sf = step_factor(level, old, mode, cfl)
    W, D, valid = old, np.abs(old), True
    for j in range(RK):
        S, A = accumulate(class_sums(level, W), CLASSES)
        fac = sf / LD(RK + 1 - j)
        W = old + fac[:, None] * S
        D = D + np.abs(fac)[:, None] * A
        valid = valid and bool(np.isfinite(W).all() and (W[:, 0] >= 0).all() and (W[:, 4] >= 0).all())
    return {"sf": sf, "W": W, "res": W - old, "D": D, "valid": valid}


def K_sweep(got, want, D):
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    return (np.abs(got.astype(LD) - want) / (U * D)).astype(np.float64)


def rel_units(got, want):
    """Plain relative error in units of 2^-53 (the step factors)."""
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    return (np.abs(got.astype(LD) - want) / (U * np.abs(want))).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------
# The oracle's own double evaluation of the same things: what sets K_ref
# ------------------------------------------------------------------------------------------------------------------
def oracle_class(oracle, level, cls_name, q, f):
    """One class's loop of the oracle, accumulating into the double array ``f`` [nel, 5]."""
    lib = oracle.load()
    s, n = level.span(cls_name)
    q = np.ascontiguousarray(q, dtype=np.float64)
    if cls_name == "internal":
        lib.ora_compute_flux_edge(s, n, oracle.ptr(level.edges), oracle.ptr(q), oracle.ptr(f))
    elif cls_name == "wall":
        lib.ora_compute_boundary_flux_edge(s, n, oracle.ptr(level.edges), oracle.ptr(q), oracle.ptr(f))
    else:
        lib.ora_compute_wall_flux_edge(s, n, oracle.ptr(level.edges), oracle.ptr(q), oracle.ptr(f), C.byref(level.ff))
    return f


def oracle_sweep(oracle, level, q, mode="reference", cfl=0.5):
    """One sweep with the oracle's loops; the step factor from tests/time_step_emulator.py (the oracle's own bits in
    "reference" mode at cfl = 0.5).  Returns sf, W, res and the code of ora_check_for_invalid_variables after the sweep."""
    import time_step_emulator as tse
    lib = oracle.load()
    old = np.ascontiguousarray(q, dtype=np.float64).reshape(-1, 5).copy()
    v, f = old.copy(), np.zeros_like(old)
    sf = np.ascontiguousarray(tse.step_factors(mode, cfl, old, level.volumes, tse.libm_cbrt(level.volumes), level.variant))
    rc = 0
    for j in range(RK):
        for c in CLASSES:
            oracle_class(oracle, level, c, v, f)
        lib.ora_time_step(j, level.nel, oracle.ptr(sf), oracle.ptr(f), oracle.ptr(old), oracle.ptr(v))
        rc = rc or lib.ora_check_for_invalid_variables(oracle.ptr(v), level.nel, None)
    return {"sf": sf, "W": v, "res": v - old, "rc": rc}


def state_is_valid(oracle, q):
    q = np.ascontiguousarray(q, dtype=np.float64)
    return oracle.load().ora_check_for_invalid_variables(oracle.ptr(q), len(q), None) == 0


# ------------------------------------------------------------------------------------------------------------------
# What the GPU tests run: the levels (the smallest that reach each instantiation of k_flux_free) and the states on each
# ------------------------------------------------------------------------------------------------------------------
def f0_for(level, seed):
    """The non-zero flux array the accumulating launches start from."""
    return np.random.default_rng(seed).normal(size=(level.nel, 5)) * 1e-7


def build_cases(oracle, mesh3_dir, fvcorr_dir):
    """{name: (levels as mgcfd dicts, mesh variant, level index, states)} of tests/test_gpu_fast_accuracy.py; at_rest and
    uniform run on the smallest level only (the coarsest level of the 3-level hierarchy)."""
    import mgcfd
    from mgcfd import meshgen

    def from_dir(d):
        mesh = mgcfd.Mesh("input.dat", d)
        lv = [mesh.level(l) for l in range(mesh.num_levels)]
        variant = mesh.variant
        mesh.close()
        return lv, variant

    cases = {}
    lv3, v3 = from_dir(mesh3_dir)
    for l in range(3):
        cases[f"mesh3_L{l}"] = (lv3, v3, l, STATES if l == 2 else ("perturbed", "wide"))
    lvf, vf = from_dir(fvcorr_dir)
    cases["fvcorr"] = (lvf, vf, 0, ("perturbed", "wide"))
    m1 = meshgen.make_multigrid((9,), "m6wing", seed=3, cavity_radius=0.15, jitter=0.2, area_noise=0.05, volume_noise=0.05)
    cases["m6wing_1lvl"] = (mgcfd.generated_to_levels(m1), m1.mesh_variant, 0, ("perturbed", "wide"))
    # (the (11, 6) lattice has long rows — a tail list — and its plan does not tell whether a lane holds more than five half rows;
    #  (12, 6) is the smallest without a tail whose plan is not uniform (has_half_rows false), which leaves that one reason)
    mx = meshgen.make_mixed_multigrid((12, 6), "m6wing", seed=2, jitter=0.2, area_noise=0.05, volume_noise=0.05)
    cases["mixed"] = (mgcfd.generated_to_levels(mx), mx.mesh_variant, 0, ("perturbed", "wide"))
    tet = meshgen.MultigridMesh(mesh_name="m6wing")
    tet.levels.append(meshgen.make_tet_level(30000, seed=1))
    cases["tet"] = (mgcfd.generated_to_levels(tet), tet.mesh_variant, 0, ("perturbed", "wide"))
    return cases


def sweep_cfl(case, kind, mode):
    """The CFL number of the one sweep a state is put through.  0.5, the reference's, except for the `wide` state: neighbours
    there differ by factors up to 1e4 in density and pressure, and an explicit step at CFL 0.5 leaves negative energies — the
    reference itself would abort in check_for_invalid_variables.  The long-double sweep stays valid from 0.1 down under local
    steps on the damped (m6wing) levels and from 1e-7 down on the undamped fvcorr level, whose local step is its reference step;
    a factor 5 to 10 below that is taken, so that no rounding decides.  tests/test_host_fast_accuracy.py asserts that every
    combination stays valid, in long double and in the oracle."""
    if kind != "wide":
        return 0.5
    if case == "fvcorr":
        return 1e-8
    return 0.02 if mode == "local" else 0.5


def state_seed(case, kind):
    return 1000 + 7 * sorted(CASE_NAMES).index(case) + STATES.index(kind)


CASE_NAMES = ("mesh3_L0", "mesh3_L1", "mesh3_L2", "fvcorr", "m6wing_1lvl", "mixed", "tet")


# ------------------------------------------------------------------------------------------------------------------
# A numpy model of the fast kernel's algebra (kernels.hip: make_nodef, make_ownf, edge_flux_neg_f), internal edges only,
# with the faults tests/test_host_fast_accuracy.py injects.  float64 throughout; numpy never contracts, so every FMA of the
# kernel is two roundings here: the model is no more accurate than the kernel.
# ------------------------------------------------------------------------------------------------------------------
def fast_model_internal(level, q, rcp_error=0.0, c_root_error=0.0, drop_share_at=None):
    """Internal-edge flux sums as the order-free kernel forms them: velocities from a reciprocal (relative error
    ``rcp_error``), |v| + c kept as one number (the sound speed's root off by ``c_root_error``), the regrouped negated flux per
    edge, subtracted at the evaluating end and added at the other.  ``drop_share_at``: a node whose first mirrored share is lost."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 5)
    g, ks = np.float64(1.4), np.float64(np.float32(0.2))
    rho, en = q[:, 0], q[:, 4]
    inv = (1.0 / rho) * (1.0 + rcp_error)
    v = q[:, 1:4] * inv[:, None]
    sq = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
    p = (g - 1.0) * (en - 0.5 * rho * sq)
    sc = np.sqrt(sq) + np.sqrt(g * p * inv) * (1.0 + c_root_error)
    m = rho[:, None] * v                                             # the momentum re-formed from the velocity
    H = en + p
    e = level.edges
    s, n = level.span("internal")
    a, b = e["a"][s:s + n], e["b"][s:s + n]
    f = -0.5 * np.stack([e["x"][s:s + n], e["y"][s:s + n], e["z"][s:s + n]], axis=1)
    half_ewt = np.sqrt(np.maximum(f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1] + f[:, 2] * f[:, 2], 1e-300))
    factor = (half_ewt * ks) * (sc[a] + sc[b])
    fva = f[:, 0] * v[a, 0] + f[:, 1] * v[a, 1] + f[:, 2] * v[a, 2]
    fvb = f[:, 0] * v[b, 0] + f[:, 1] * v[b, 1] + f[:, 2] * v[b, 2]
    da, db = rho[a] * fva, rho[b] * fvb
    ps = p[a] + p[b]
    G = np.empty((n, 5))
    G[:, 0] = factor * (rho[a] - rho[b]) - (da + db)
    for k in range(3):
        G[:, 1 + k] = factor * (m[a, k] - m[b, k]) - v[a, k] * da - v[b, k] * db - ps * f[:, k]
    G[:, 4] = factor * (en[a] - en[b]) - H[a] * fva - (en[b] + p[b]) * fvb
    mine, mirrored = G, G
    if drop_share_at is not None:
        # (which end evaluates an edge is the plan's choice: the share this node is handed by the first edge that lists it)
        hit = np.flatnonzero(b == drop_share_at)
        if len(hit):
            mirrored = G.copy()
            mirrored[hit[0]] = 0.0
        else:
            mine = G.copy()
            mine[np.flatnonzero(a == drop_share_at)[0]] = 0.0
    out = np.zeros((level.nel, 5))
    np.subtract.at(out, a, mine)
    np.add.at(out, b, mirrored)
    return out
