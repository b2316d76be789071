"""The yardstick of tests/test_gpu_fast_physics.py on the CPU (tests/fast_physics_reference.py; nothing here needs a GPU).

1. YARDSTICK.  For every array the GPU tests measure, K_ref: the double emulator's K against the long-double evaluation, on the
   inputs the GPU tests use (there the emulator is evaluated on what the GPU wrote; here on what the emulator itself wrote).
   These are reference-against-reference figures: the cap, twice the largest figure measured here rounded up to an integer, only
   guards the yardstick — a magnitude that forgot terms would inflate K_ref and loosen every GPU bound, 3 * max(K_ref, 1).
   Measured (the maximum over nodes and components; MEASURED and CAPS below are read off these lines):

    K_ref  lattice_A jst L                                              0.00
    K_ref  lattice_A jst nu                                             0.82
    K_ref  lattice_A jst r                                              1.37
    K_ref  lattice_A jst C (2.5, 0.15625)                               1.52
    K_ref  lattice_A jst F_int + C (2.5, 0.15625)                       0.96
    K_ref  lattice_A jst C (0.0, 0.15625)                               1.89
    K_ref  lattice_A jst F_int + C (0.0, 0.15625)                       0.98
    K_ref  lattice_A jst C (600.0, 0.0)                                 0.70
    K_ref  lattice_A jst F_int + C (600.0, 0.0)                         0.91
    K_ref  lattice_A viscous S constant                                 1.91
    K_ref  lattice_A viscous V constant                                 3.00
    K_ref  lattice_A viscous F_int + V constant                         2.02
    K_ref  lattice_A viscous S sutherland+field                         2.74
    K_ref  lattice_A viscous mu_i (relative)                            4.45
    K_ref  lattice_A viscous V sutherland+field                         2.28
    K_ref  lattice_A viscous F_int + V sutherland+field                 2.22
    K_ref  tet jst L                                                    0.00
    K_ref  tet jst nu                                                   0.84
    K_ref  tet jst r                                                    1.54
    K_ref  tet jst C (2.5, 0.15625)                                     3.82
    K_ref  tet jst F_int + C (2.5, 0.15625)                             3.05
    K_ref  tet jst C (0.0, 0.15625)                                     3.82
    K_ref  tet jst F_int + C (0.0, 0.15625)                             3.95
    K_ref  tet jst C (600.0, 0.0)                                       2.31
    K_ref  tet jst F_int + C (600.0, 0.0)                               1.44
    K_ref  tet viscous S constant                                       0.84
    K_ref  tet viscous V constant                                       4.84
    K_ref  tet viscous F_int + V constant                               3.57
    K_ref  hub jst L                                                    0.00
    K_ref  hub jst nu                                                   0.79
    K_ref  hub jst r                                                    1.38
    K_ref  hub jst C (2.5, 0.15625)                                     4.62
    K_ref  hub jst F_int + C (2.5, 0.15625)                             3.47
    K_ref  hub jst C (0.0, 0.15625)                                     6.37
    K_ref  hub jst F_int + C (0.0, 0.15625)                             3.65
    K_ref  hub jst C (600.0, 0.0)                                       1.32
    K_ref  hub jst F_int + C (600.0, 0.0)                               0.99
    K_ref  hub viscous S constant                                       1.00
    K_ref  hub viscous V constant                                       2.55
    K_ref  hub viscous F_int + V constant                               0.98
    K_ref  isolated jst L                                               0.00
    K_ref  isolated jst nu                                              0.49
    K_ref  isolated jst r                                               0.63
    K_ref  isolated jst C (2.5, 0.15625)                                1.95
    K_ref  isolated jst F_int + C (2.5, 0.15625)                        0.80
    K_ref  isolated jst C (0.0, 0.15625)                                1.34
    K_ref  isolated jst F_int + C (0.0, 0.15625)                        0.80
    K_ref  isolated jst C (600.0, 0.0)                                  0.51
    K_ref  isolated jst F_int + C (600.0, 0.0)                          0.70
    K_ref  isolated viscous S constant                                  1.24
    K_ref  isolated viscous V constant                                  1.20
    K_ref  isolated viscous F_int + V constant                          0.88
    K_ref  lattice_A sweep viscous state                                0.73
    K_ref  lattice_A sweep viscous residual                             0.73
    K_ref  lattice_A sweep viscous step factor                         10.44
    K_ref  lattice_A sweep jst state                                    0.95
    K_ref  lattice_A sweep jst residual                                 0.95
    K_ref  lattice_A sweep jst step factor                              5.22
    K_ref  lattice_A sweep smoothing state                              0.41
    K_ref  lattice_A sweep smoothing residual                           0.41
    K_ref  lattice_A sweep smoothing step factor                        5.22
    K_ref  lattice_A sweep dual state                                   1.10
    K_ref  lattice_A sweep dual residual                                1.10
    K_ref  lattice_A sweep dual step factor                             5.22
    K_ref  lattice_A sweep dual BDF1 state                              1.19
    K_ref  lattice_A sweep dual BDF1 residual                           1.19
    K_ref  lattice_A sweep dual BDF1 step factor                        5.22
    K_ref  lattice_A sweep viscous+jst+smoothing+dual state             0.56
    K_ref  lattice_A sweep viscous+jst+smoothing+dual residual          0.56
    K_ref  lattice_A sweep viscous+jst+smoothing+dual step factor      10.44
    K_ref  tet sweep viscous state                                      0.77
    K_ref  tet sweep viscous residual                                   0.77
    K_ref  tet sweep viscous step factor                                7.45
    K_ref  tet sweep jst state                                          1.88
    K_ref  tet sweep jst residual                                       1.88
    K_ref  tet sweep jst step factor                                    7.45
    K_ref  tet sweep smoothing state                                    0.75
    K_ref  tet sweep smoothing residual                                 0.75
    K_ref  tet sweep smoothing step factor                              7.45
    K_ref  tet sweep dual state                                         1.21
    K_ref  tet sweep dual residual                                      1.21
    K_ref  tet sweep dual step factor                                   5.79
    K_ref  lattice_A fas_restrict coarse state                          2.23
    K_ref  lattice_A fas_restrict P                                     1.35
    K_ref  lattice_A fas_prolong fine state                             0.85
    K_ref  lattice_A prolong_state fine state                           6.72

2. SENSITIVITY.  Numpy models of faulty kernels, applied to the emulator.  "Old metric": what the test_fast_mode tests assert,
   max |difference| / max |value| <= 1e-10 of level 0's state, here after GPU_CYCLES sweeps of level 0 with the fault in every
   stage.  "New": the K of the faulty launch on the start state against 3 * max(K_ref, 1).  Measured:

    fault                                                   old metric   K        bound
    one neighbour dropped from a gradient sum (lattice A)   6.9e-17      1.6e13   3.6
    one weight halved on the hub's long row (601 entries)   1.2e-11      2.5e10   3
    three digits of txx lost (lattice A)                    0            901      4.6
    V zeroed at mu = 1e-16 (lattice A)                      2.8e-16      2.6e3    3
    nu off by 1e-6 at one node (lattice A)                  1.1e-9 (!)   2.6e6    3
    nu off by 1e-8 at one node (lattice A)                  1.1e-11      2.6e4    3
    one Jacobi iteration skipped, CFL 1.0 (lattice A)       0.19 (!)     3.4e14   3
    one Jacobi iteration skipped, CFL 1e-10 (lattice A)     3.3e-11      9.9e4    3

   (!): above 1e-10, the old metric sees that fault as well on these inputs; the row below it is the size it passes.
   The three-digit loss of one stress component exceeds the bound at 119 of lattice A's 2,178 nodes: those next to a no-slip
   wall, where the velocity differences are of the velocity's own size.  In the interior of the 1 % perturbed field a gradient
   is a small fraction of the products it was summed from, in double as in long double, and the detectable relative error of
   a stress, K_bound * 2^-53 * A / |txx|, is 4.7e-13 at the median node (5.1e-16 at the best).
   V zeroed: the unit is a rounding of |F| + A_V, and the detectable relative error of V, K_bound * 2^-53 * A / |V|, is 6.5 at
   the median node at this viscosity: a V lost whole (a relative error of 1) is found at 740 of the 2,178 nodes.
   (ve.GPU_MU was chosen so that F + V differs from F in BITS at most nodes; 3 roundings is more.)
   The sensor: on the perturbed states of these tests the old metric is linear in the fault and reads 1.1e-9 for 1e-6 at one
   node; it passes from 9e-8 down; K falls to the bound at about 1e-12.
   The skipped Jacobi iteration changes the update by a tenth of itself.  At CFL 1.0 the update is a tenth of the state and the
   old metric finds the fault too; it measures against the STATE, so it passes once the update is below 1e-9 of the state
   (shown at CFL 1e-10; a run near its steady state is in the same position), where K_sweep still reads 1e5.

3. INPUTS.  Every input of the GPU tests is valid in the emulator (the states pass the invalid-state check, every sweep that
   is run returns code 0 and stays valid in long double, every emulated array is finite), and every
   branch occurs: the saturated and the unsaturated JST switch, wall nodes, nodes without an internal edge, the viscous limit
   binding and not binding, the dual-time clamp binding and not binding, coarse nodes' children, coincident nodes.
"""
import numpy as np
import pytest

import fast_accuracy_reference as far
import fast_physics_reference as fpr
import viscous_emulator as ve

OLD_REL_RUN = 1e-10         # tests/test_gpu_viscous.py::test_fast_mode and its siblings: REL_RUN
OLD_CYCLES = 3              # ve.GPU_CYCLES
GPU_MU_LATTICE = 1e-16      # ve.GPU_MU["A"]

MEASURED = {line[11:69].strip(): float(line[69:]) for line in __doc__.splitlines() if line.startswith("    K_ref  ")}
CAPS = {label: max(1, int(np.ceil(2.0 * figure))) for label, figure in MEASURED.items()}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return fpr.write_cases(tmp_path_factory.mktemp("fast_physics"))


_FIGURES = {}


def _record(label, k, figures=_FIGURES):
    """Prints a K_ref and asserts its cap."""
    k = float(np.max(k))
    figures[label] = k
    print("KREF %-52s %8.2f   cap %s" % (label, k, CAPS.get(label)))
    return k


def _assert_caps(figures):
    missing = [l for l in figures if l not in CAPS]
    assert not missing, f"no cap for {missing}"
    over = {l: (k, CAPS[l]) for l, k in figures.items() if not k <= CAPS[l]}
    assert not over, f"the emulator is further from long double than twice what was measured: {over}"


def test_long_double_sweep_with_every_option_off_is_the_plain_sweep(oracle, cases):
    """fpr.sweep without options against far.sweep: the same long-double bits in every array."""
    em = fpr.make_emulator(oracle, cases["lattice_A"], "lattice_A")
    level, W = fpr.ref_level(em), em.variables(0)
    for mode, cfl in (("local", 1.0), ("reference", 0.5)):
        a, b = far.sweep(level, W, mode, cfl), fpr.sweep(level, W, mode, cfl)
        for name in ("sf", "W", "res", "D"):
            assert a[name].dtype == b[name].dtype == fpr.LD and np.array_equal(a[name], b[name]), f"{mode}: {name}"
        assert a["valid"] and b["valid"]
    em.close()


@pytest.mark.parametrize("mesh", fpr.MESHES)
def test_yardstick_of_the_launches(oracle, cases, mesh):
    """Viscous pass 1 (constant mu; on lattice A Sutherland + field too, and mu_i by rel_units), pass 2 and F(internal) + V;
    JST's L, nu, r, C and F(internal) + C for every pair."""
    import jst_emulator as jse
    import variable_viscosity_emulator as vve
    figures = {}
    em = fpr.make_emulator(oracle, cases[mesh], mesh)
    level, start = fpr.ref_level(em), em.variables(0)
    nel = level.nel
    assert far.state_is_valid(oracle, start)
    # JST on the start state
    L, nu, r = jse.sensor(start, em.ea[0], em.eb[0])
    s = fpr.jst_sensor(level, start)
    for name, got in (("L", L), ("nu", nu), ("r", r)):
        _record(f"{mesh} jst {name}", far.K(got, *s[name]), figures)
    f_int = far.oracle_class(oracle, level, "internal", start, np.zeros((nel, 5)))
    for k2, k4 in fpr.JST_PAIRS:
        Cn = fpr.emulated_correction(em, start, L, nu, r, k2, k4)
        C_, A_C = fpr.jst_correction(level, start, L, nu, r, k2, k4)
        _record(f"{mesh} jst C ({k2}, {k4})", far.K(Cn, C_, A_C), figures)
        _record(f"{mesh} jst F_int + C ({k2}, {k4})", far.K(f_int + Cn, *fpr.onto(f_int, C_, A_C), f0=f_int), figures)
        assert np.isfinite(Cn).all() and Cn.any()
    # the viscous terms, no-slip walls
    for variable in ((False, True) if mesh == "lattice_A" else (False,)):
        W, visc, _ = fpr.viscous_setup(em, mesh, variable)
        tag = "sutherland+field" if variable else "constant"
        S_em = em.viscous_terms(0)[0]
        S, A, mid = fpr.viscous_pass1(level, W, visc)
        assert np.isfinite(S_em).all()
        _record(f"{mesh} viscous S {tag}", far.K(S_em, S, A), figures)
        if variable:
            _record(f"{mesh} viscous mu_i (relative)", far.rel_units(vve.viscosity(em.model, em.mu, ve.primitives(W)[:, 3]), mid["mu"]), figures)
        V_em = fpr.emulated_viscous_flux(em, S_em)
        V, A_V = fpr.viscous_pass2(level, S_em)
        _record(f"{mesh} viscous V {tag}", far.K(V_em, V, A_V), figures)
        f_int = far.oracle_class(oracle, level, "internal", W, np.zeros((nel, 5)))
        got = f_int.copy()
        got[:, 1:5] = got[:, 1:5] + V_em[:, 1:5]
        _record(f"{mesh} viscous F_int + V {tag}", far.K(got, *fpr.onto(f_int, V, A_V), f0=f_int), figures)
        assert V_em[:, 1:].any() and not V_em[:, 0].any()
    em.close()
    _FIGURES.update(figures)
    _assert_caps(figures)


def _sweep_cases(mesh):
    """(options, BDF order): each option alone (dual time under BDF2, which the GPU tests run, and on lattice A under BDF1 too)
    and, on lattice A, all together."""
    alone = [((o,), 2) for o in fpr.SWEEP_OPTIONS]
    return alone + ([(("dual",), 1), (fpr.SWEEP_OPTIONS, 2)] if mesh == "lattice_A" else [])


@pytest.mark.parametrize("mesh", fpr.SWEEP_MESHES)
def test_yardstick_of_one_sweep(oracle, cases, mesh):
    """smooth(0, 1) with each option alone and, on lattice A, all together: state, residual, step factors."""
    figures = {}
    for options, order in _sweep_cases(mesh):
        em = fpr.make_emulator(oracle, cases[mesh], mesh)
        level = fpr.ref_level(em)
        W, kw, _ = fpr.sweep_setup(em, mesh, options, order)
        assert "dual" not in options or em.effective_order() == order
        rc, got = fpr.emulated_sweep(em)
        ref = fpr.sweep(level, W, "local", fpr.LOCAL_CFL[mesh], **kw)
        tag = f"{mesh} sweep {'+'.join(options)}{' BDF1' if order == 1 else ''}"
        assert rc == 0 and ref["valid"], f"{tag}: the state does not survive one sweep"
        _record(f"{tag} state", far.K_sweep(got["W"], ref["W"], ref["D"]), figures)
        _record(f"{tag} residual", far.K_sweep(got["res"], ref["res"], ref["D"]), figures)
        _record(f"{tag} step factor", far.rel_units(got["sf"], ref["sf"]), figures)
        em.close()
    _FIGURES.update(figures)
    _assert_caps(figures)


def test_yardstick_of_the_transfers(oracle, cases):
    """fas_restrict(0) (coarse state, W0, P), fas_prolong(0) and prolong_state(0) on lattice A's hierarchy."""
    figures = {}
    mesh = "lattice_A"
    em = fpr.make_emulator(oracle, cases[mesh], mesh, fas=True)
    t = fpr.transfer_setup(em, mesh)
    T0 = em.total_residual(0)
    coarse = fpr.emulated_restriction(em, 0, t["W_fine"], t["coarse_before"])
    _record(f"{mesh} fas_restrict coarse state", far.K(coarse, *fpr.restrict_state(t["parent"], t["W_fine"], t["coarse_before"]), f0=t["coarse_before"]), figures)
    em._var(1)[:] = coarse
    R1 = em.total_residual(1)
    P = fpr.emulated_forcing(t["parent"], T0, R1)
    _record(f"{mesh} fas_restrict P", far.K(P, *fpr.restrict_forcing(t["parent"], T0, R1)), figures)
    em.fas_restrict(0)
    assert np.array_equal(em.P[1], P) and np.array_equal(em.W0[1], coarse), "the pieces are the emulator's own down leg"
    new = t["W_fine"] + (0.0 - fpr.emulated_wavg(em, 0, coarse - t["W_coarse"]))
    _record(f"{mesh} fas_prolong fine state", far.K(new, *fpr.fas_correction(t["interp"], t["W_fine"], coarse, t["W_coarse"])), figures)
    em._var(1)[:] = t["W_coarse"]
    em.fas_prolong(0)
    assert np.array_equal(em.variables(0), new), "... and its own up leg"
    _record(f"{mesh} prolong_state fine state", far.K(0.0 - (0.0 - fpr.emulated_wavg(em, 0, t["W_coarse"])), *t["interp"](t["W_coarse"])), figures)
    em.close()
    _FIGURES.update(figures)
    _assert_caps(figures)


# ------------------------------------------------------------------------------------------------------------------
# Sensitivity
# ------------------------------------------------------------------------------------------------------------------
def _old_metric_after_sweeps(em_plain, em_faulty):
    """max |difference| / max |value| of level 0's state after OLD_CYCLES sweeps of level 0 on both emulators."""
    assert em_plain.sweeps(0, OLD_CYCLES) == 0 and em_faulty.sweeps(0, OLD_CYCLES) == 0
    return fpr.old_metric(em_faulty.variables(0), em_plain.variables(0))


def _drop_one_end(em, node, halve=False):
    """The index arrays of ve.stresses with the first edge end of ``node`` removed (or its normal halved)."""
    to, frm, N = em.vto[0].copy(), em.vfrm[0].copy(), em.vN[0].copy()
    at = np.flatnonzero(to == node)[0]
    if halve:
        N[at] *= 0.5
        return to, frm, N
    keep = np.ones(len(to), dtype=bool)
    keep[at] = False
    return to[keep], frm[keep], N[keep]


def _viscous_fault(em, kind, node=None):
    """Replaces ``em.viscous_terms`` by a faulty model: (S, V) with the fault in pass 1 or pass 2."""
    plain = type(em).viscous_terms

    def faulty(l, W=None):
        W_ = em._var(l) if W is None else W
        vol, kappa = em.oc.array(l, "volumes"), ve.conductivity(em.mu, em.prandtl)
        if kind in ("neighbour dropped", "weight halved"):
            S = ve.stresses(W_, *_drop_one_end(em, node, halve=(kind == "weight halved")), vol, em.mu, kappa)
            return S, ve.viscous_flux(S, em.vto[l], em.vfrm[l], em.vN[l])
        S, V = plain(em, l, W)
        if kind == "three digits of txx lost":
            S = S.copy()
            S[:, 3] *= 1.0 + 1e-13
            return S, ve.viscous_flux(S, em.vto[l], em.vfrm[l], em.vN[l])
        assert kind == "V zeroed"
        return S, np.zeros_like(V)

    em.viscous_terms = faulty


def _report(name, old, k, bound):
    k, bound = np.atleast_1d(k), np.atleast_1d(bound)
    print("FAULT %-44s old metric %.2e   K %.3g against %.3g" % (name, old, k.max(), bound[np.argmax(k / bound)]))


@pytest.mark.parametrize("kind,mesh", [("neighbour dropped", "lattice_A"), ("weight halved", "hub"), ("three digits of txx lost", "lattice_A")])
def test_faults_of_viscous_pass_1_pass_the_old_metric_and_exceed_the_new_bound(oracle, cases, kind, mesh):
    mu = GPU_MU_LATTICE if mesh == "lattice_A" else fpr.MU[mesh]
    em, bad = fpr.make_emulator(oracle, cases[mesh], mesh), fpr.make_emulator(oracle, cases[mesh], mesh)
    level = fpr.ref_level(em)
    W, visc, _ = fpr.viscous_setup(em, mesh, mu=mu)
    fpr.viscous_setup(bad, mesh, mu=mu)
    degree = np.bincount(em.vto[0], minlength=level.nel)
    node = int(np.argmax(degree)) if mesh == "hub" else int(np.argsort(degree)[len(degree) // 2])
    if mesh == "hub":
        assert degree[node] > 256, "the hub's row was meant to be longer than a tile is wide"
    _viscous_fault(bad, kind, node)
    S, A, _ = fpr.viscous_pass1(level, W, visc)
    k_ref = far.K(em.viscous_terms(0)[0], S, A).max(axis=0)
    k = far.K(bad.viscous_terms(0)[0], S, A)
    old = _old_metric_after_sweeps(em, bad)
    _report(f"{kind} ({mesh}, mu {mu:g})", old, k.max(axis=0), fpr.k_bound(k_ref))
    if kind == "three digits of txx lost":
        detect = (fpr.k_bound(k_ref)[3] * fpr.U * A[:, 3] / np.abs(S[:, 3])).astype(np.float64)
        print("      detectable relative error of txx: median %.2e, smallest %.2e; nodes above the bound: %d of %d"
              % (np.median(detect), detect.min(), int((k[:, 3] > fpr.k_bound(k_ref)[3]).sum()), level.nel))
    assert old <= OLD_REL_RUN, "the whole-run metric was meant to pass this fault"
    assert (k.max(axis=0) > fpr.k_bound(k_ref)).any(), "the per-node bound was meant to catch it"
    em.close(); bad.close()


def test_zeroed_viscous_flux_at_the_lattices_gpu_viscosity(oracle, cases):
    """mu = 1e-16 on lattice A: F(internal) + V with V written as zeros.  The unit is a rounding of |F| + A_V."""
    mesh, mu = "lattice_A", GPU_MU_LATTICE
    em, bad = fpr.make_emulator(oracle, cases[mesh], mesh), fpr.make_emulator(oracle, cases[mesh], mesh)
    level = fpr.ref_level(em)
    W, visc, _ = fpr.viscous_setup(em, mesh, mu=mu)
    fpr.viscous_setup(bad, mesh, mu=mu)
    _viscous_fault(bad, "V zeroed")
    S_em, V_em = em.viscous_terms(0)
    V, A_V = fpr.viscous_pass2(level, S_em)
    f_int = far.oracle_class(oracle, level, "internal", W, np.zeros((level.nel, 5)))
    target = fpr.onto(f_int, V, A_V)
    good = f_int.copy()
    good[:, 1:5] = good[:, 1:5] + V_em[:, 1:5]
    k_ref = far.K(good, *target, f0=f_int).max(axis=0)
    k = far.K(f_int, *target, f0=f_int)
    bound = fpr.k_bound(k_ref)
    old = _old_metric_after_sweeps(em, bad)
    _report(f"V zeroed ({mesh}, mu {mu:g})", old, k.max(axis=0), bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        detect = (bound[None, 1:] * fpr.U * target[1][:, 1:] / np.abs(V[:, 1:])).astype(np.float64)
    found = (k[:, 1:] > bound[None, 1:]).any(axis=1)
    print("      detectable relative error of V: median %.2e; a V lost whole is found at %d of %d nodes (%.3f)"
          % (np.median(detect), int(found.sum()), level.nel, found.mean()))
    assert old <= OLD_REL_RUN, "the whole-run metric was meant to pass this fault"
    assert (k.max(axis=0) > bound).any(), "the per-node bound was meant to catch it"
    em.close(); bad.close()


@pytest.mark.parametrize("size", [1e-6, 1e-8])
def test_sensor_off_at_one_node(oracle, cases, size):
    """nu_i * (1 + size) at one node of lattice A.  The switch multiplies differences of the state, and on the perturbed state
    of these tests the old metric is linear in the fault: 1.1e-9 for 1e-6 (it sees that one too), 1.1e-11 for 1e-8, which it
    passes; K reads 2.6e6 and 2.6e4 against a bound of 3."""
    import jst_emulator as jse
    mesh = "lattice_A"
    em, bad = fpr.make_emulator(oracle, cases[mesh], mesh), fpr.make_emulator(oracle, cases[mesh], mesh)
    level, W = fpr.ref_level(em), em.variables(0)
    node = level.nel // 2
    for e in (em, bad):
        e.set_jst(*fpr.JST_PAIRS[0], 1)

    def faulty(l, W=None):
        W_ = bad._var(l) if W is None else W
        L, nu, r = jse.sensor(W_, bad.ea[l], bad.eb[l])
        nu = nu.copy()
        nu[node] *= 1.0 + size
        return fpr.emulated_correction(bad, W_, L, nu, r, bad.kappa2, bad.kappa4, l), L, nu, r

    bad.terms = faulty
    s = fpr.jst_sensor(level, W)
    k_ref = far.K(em.terms(0)[2], *s["nu"]).max()
    k = far.K(bad.terms(0)[2], *s["nu"])
    old = _old_metric_after_sweeps(em, bad)
    _report(f"nu off by {size:g} at one node ({mesh})", old, k.max(), fpr.k_bound(k_ref))
    if size == 1e-6:
        assert old > OLD_REL_RUN, "on this state the whole-run metric sees a fault of this size as well"
    else:
        assert old <= OLD_REL_RUN, "the whole-run metric was meant to pass this fault"
    assert k.max() > fpr.k_bound(k_ref)[0] and int(np.argmax(k)) == node
    em.close(); bad.close()


@pytest.mark.parametrize("cfl", [1.0, 1e-10])
def test_one_jacobi_iteration_skipped(oracle, cases, cfl):
    """Residual smoothing (0.5, 2) with one iteration run.  A missing iteration changes the update by a tenth of itself: at the
    GPU tests' CFL 1.0 the update is a tenth of the state and the old metric finds the fault too.  The old metric measures the
    update's error against the STATE, so it passes the fault once the update is below 1e-9 of the state (shown at CFL 1e-10; a run
    near its steady state is in the same position), where K_sweep still reads 1e4."""
    mesh = "lattice_A"
    em, bad = fpr.make_emulator(oracle, cases[mesh], mesh), fpr.make_emulator(oracle, cases[mesh], mesh)
    level, W = fpr.ref_level(em), em.variables(0)
    for e in (em, bad):
        e.set_time_step("local", cfl)
        e.set_residual_smoothing(*fpr.SMOOTHING)
    bad.set_residual_smoothing(fpr.SMOOTHING[0], fpr.SMOOTHING[1] - 1)
    ref = fpr.sweep(level, W, "local", cfl, smoothing=fpr.SMOOTHING)
    assert em.sweeps(0, 1) == 0 and bad.sweeps(0, 1) == 0
    k_ref = far.K_sweep(em.variables(0), ref["W"], ref["D"]).max(axis=0)
    k = far.K_sweep(bad.variables(0), ref["W"], ref["D"]).max(axis=0)
    assert em.sweeps(0, OLD_CYCLES - 1) == 0 and bad.sweeps(0, OLD_CYCLES - 1) == 0
    old = fpr.old_metric(bad.variables(0), em.variables(0))
    _report(f"one Jacobi iteration skipped (CFL {cfl:g})", old, k, fpr.k_bound(k_ref))
    assert (k > fpr.k_bound(k_ref)).all(), "the per-node bound was meant to catch it"
    if cfl == 1.0:
        assert old > OLD_REL_RUN, "on the perturbed state the whole-run metric sees a skipped iteration as well"
    else:
        assert old <= OLD_REL_RUN, "with an update this small the whole-run metric was meant to pass this fault"
        assert k.max() > 1e3
    em.close(); bad.close()


# ------------------------------------------------------------------------------------------------------------------
# Inputs
# ------------------------------------------------------------------------------------------------------------------
def test_every_branch_occurs_on_the_inputs_of_the_gpu_tests(oracle, cases):
    import jst_emulator as jse
    saturated = unsaturated = 0
    for mesh in fpr.MESHES:
        em = fpr.make_emulator(oracle, cases[mesh], mesh)
        level, start = fpr.ref_level(em), em.variables(0)
        _, nu, _ = jse.sensor(start, em.ea[0], em.eb[0])
        e2, _ = jse.switches(nu[em.ea[0]], nu[em.eb[0]], *fpr.JST_PAIRS[2])
        saturated, unsaturated = saturated + int((e2 == 1.0).sum()), unsaturated + int((e2 < 1.0).sum())
        walls = fpr.wall_nodes(level)
        assert np.array_equal(walls, em.wall_nodes[0]) and (len(walls) > 0) == (mesh in ("lattice_A", "isolated")), f"{mesh}: wall nodes"
        isolated = np.flatnonzero(np.bincount(em.vto[0], minlength=level.nel) == 0)
        if mesh == "isolated":
            assert list(isolated) == [1, 4, 6]
            W, visc, _ = fpr.viscous_setup(em, mesh)
            S, A, _ = fpr.viscous_pass1(level, W, visc)
            assert not A[isolated, 3:].any() and not S[isolated, 3:].any(), "no internal edge: A = 0, the stresses exactly zero"
            V, A_V = fpr.viscous_pass2(level, em.viscous_terms(0)[0])
            assert not A_V[isolated].any()
            s = fpr.jst_sensor(level, start)
            assert not s["nu"][1][isolated].any() and not s["L"][1][isolated].any()
        else:
            assert len(isolated) == 0
        assert far.state_is_valid(oracle, start), f"{mesh}: the start state"
        W, _, _ = fpr.viscous_setup(em, mesh)
        assert far.state_is_valid(oracle, W), f"{mesh}: the start state with the wall rule applied"
        em.close()
    assert saturated > 0 and unsaturated > 0
    # the limits: the viscous one binds on lattice A and not on the tet level; the clamp binds on some nodes and not on others
    for mesh in fpr.SWEEP_MESHES:
        em = fpr.make_emulator(oracle, cases[mesh], mesh)
        fpr.sweep_setup(em, mesh, ("viscous",))
        assert em.sweeps(0, 1) == 0
        assert (em.limited[0][0] > 0) == (mesh == "lattice_A") and sum(em.limited[0]) == em.oc.levels[0].nel
        em.close()
        em = fpr.make_emulator(oracle, cases[mesh], mesh)
        fpr.sweep_setup(em, mesh, ("dual",))
        assert em.sweeps(0, 1) == 0
        assert em.bound[0][0] > 0 and em.bound[0][1] > 0, f"{mesh}: the clamp was meant to bind on some nodes and not on others"
        em.close()
    em = fpr.make_emulator(oracle, cases["lattice_A"], "lattice_A", fas=True)
    t = fpr.transfer_setup(em, "lattice_A")
    assert t["interp"].coincident.any() and not t["interp"].coincident.all() and t["interp"].has_edge.all()
    assert (np.bincount(t["parent"], minlength=em.oc.levels[1].nel) > 0).all()
    em.close()
