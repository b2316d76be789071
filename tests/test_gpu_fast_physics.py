"""The fast flavour (MGCFD_OPT_EXACT = 0) of the launchers behind the flux kernels, per node and component against long double:
viscous_stress and viscous_flux (constant viscosity; Sutherland's law with an eddy-viscosity field), jst_sensor and
jst_dissipation, one sweep with each of the viscous terms, JST, residual smoothing and dual time (time_step_src, dual_source,
smooth, the viscous step limit and dual time's clamp), and the transfers restrict_fas, prolong_fas and prolong_state.

The whole-run test_fast_mode tests compare the state after a few cycles with the emulator's, max |difference| / max |value| <=
1e-10: tests/test_host_fast_physics.py shows what that lets through.  Here every launch is measured on its OWN input, in units
of one rounding of the magnitudes that went into each node's value (tests/fast_physics_reference.py):

    K <= 3 * max(K_ref, 1)      per array and component

K_ref is the double emulator's K on the same input, computed here; the input of a second pass is what the GPU's first pass
wrote (S read back for the viscous flux; L, nu and r read back for the JST correction; T and R(W0) for the FAS forcing), so no
bound absorbs the launch before.  The 3 is tests/test_gpu_fast_accuracy.py's: contraction only removes roundings, a faithful
reciprocal or root adds one; the floor of 1 because no double evaluation guarantees better than one rounding of the magnitude.
No launch needed a model-based bound.

F is the deterministic flux variant's (flux_variant 1), so that F(internal) of one launch is the f0 of the next.  The meshes
are the smallest that reach each path of the tile walk, those of the exact-flavour test_kernel_paths, with their tilings
asserted as there:

    lattice_A   2,178 nodes: several tiles, the last one partial           mu 0.07 (cell Reynolds number 2), local CFL 1.0
    tet         30,000 tetrahedral nodes: overflow references, row lists   mu 1e-3, local CFL 0.02
    hub         600 spokes: a row longer than a tile is wide               mu 1e-9, local CFL 0.02
    isolated    8 nodes, three without an internal edge (A = 0: exact)     mu 1e-9, local CFL 0.02

Every figure is printed before anything is asserted, in lines that begin with FASTACC (profiles/fast_mode_accuracy.txt).
"""
import numpy as np
import pytest

import fast_accuracy_reference as far
import fast_physics_reference as fpr
import free_stream_emulator as fse

pytestmark = pytest.mark.gpu

DETERMINISTIC = 1       # flux_variant: the contracted node gather, the same bits in every launch


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return fpr.write_cases(tmp_path_factory.mktemp("fast_physics"))


def _solver(case):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    for name, v in (("graph", 0), ("exact", 0), ("flux_variant", DETERMINISTIC)):
        s.set_option(name, v)
    return mesh, s


def _path(name, s):
    """The tile walk's paths on level 0, asserted as the exact-flavour test_kernel_paths assert them."""
    t = s.tiling(0)
    if name == "tet":
        assert t["tiles"] > 1 and t["overflow_refs"] > 0 and t["list_entries"] > 0
    elif name == "hub":
        assert t["list_entries"] > 0
    elif name == "lattice_A":
        assert t["tiles"] > 1 and s.nel(0) % 256 != 0
    else:
        assert s.nel(0) == 8
    return "%d tiles, %d overflow refs, %d list entries" % (t["tiles"], t["overflow_refs"], t["list_entries"])


def check(label, k, k_ref):
    """K <= 3 * max(K_ref, 1) per component; the figures are printed before anything is asserted."""
    k = np.asarray(k, dtype=np.float64)
    k = k.reshape(len(k), -1)
    kmax, k_ref = k.max(axis=0), np.atleast_1d(np.asarray(k_ref, dtype=np.float64))
    print("FASTACC %-86s K %s | emulator %s" % (label, np.array2string(kmax, precision=2, floatmode="fixed", max_line_width=400),
                                               np.array2string(k_ref, precision=2, floatmode="fixed", max_line_width=400)))
    bound = fpr.k_bound(k_ref)
    if not (kmax <= bound).all():
        node, comp = np.unravel_index(np.argmax(k / bound), k.shape)
        raise AssertionError(f"{label}: K {kmax} above 3 x max({k_ref}, 1); worst at node {int(node)}, component {int(comp)}")


def _same(got, want, what):
    assert np.array_equal(np.asarray(got).view(np.int64), np.asarray(want).view(np.int64)), what


@pytest.mark.parametrize("mesh", fpr.MESHES)
def test_viscous_launches_per_node(oracle, cases, mesh):
    """After compute_fluxes: viscous_stress against pass 1.  Then F(internal) from compute_flux_edge with the terms off and the
    same call with them on: F(internal) + V against F(internal) as read + pass 2 in long double ON THE S THE GPU WROTE."""
    msh, s = _solver(cases[mesh])
    em = fpr.make_emulator(oracle, cases[mesh], mesh)
    level, start, path = fpr.ref_level(em), em.variables(0), _path(mesh, s)
    s.set_time_step("local", fpr.LOCAL_CFL[mesh])
    for variable in ((False, True) if mesh == "lattice_A" else (False,)):
        W, visc, field = fpr.viscous_setup(em, mesh, variable)
        tag = "Sutherland + eddy field" if variable else "constant mu"

        def switch_on():
            s.set_viscous(fpr.MU[mesh], fpr.PRANDTL, True, fpr.VISCOUS_CFL, 1)
            if variable:
                s.set_viscosity_model(law="sutherland", eddy="field")
                s.set(0, "eddy_viscosity", field)
            else:
                s.set_viscosity_model()

        s.set(0, "variables", start)
        switch_on()
        _same(s.get(0, "variables"), W, f"{mesh}: the start state with the wall rule applied")
        s.zero_fluxes(0)
        s.compute_fluxes(0)
        S_got = s.get(0, "viscous_stress")
        S, A, _ = fpr.viscous_pass1(level, W, visc)
        check(f"{mesh} viscous_stress [{tag}; {path}] S", far.K(S_got, S, A), far.K(em.viscous_terms(0)[0], S, A).max(axis=0))
        # V alone: the internal fluxes with the terms off, then the same call with them on
        s.zero_fluxes(0)
        s.set_viscous(0.0, levels=0)
        s.compute_flux_edge(0)
        f_int = s.get(0, "fluxes")
        s.zero_fluxes(0)
        switch_on()
        s.compute_flux_edge(0)
        got = s.get(0, "fluxes")
        S_in = s.get(0, "viscous_stress")
        _same(S_in, S_got, f"{mesh}: pass 1 keeps row order: the same bits in every launch")
        V, A_V = fpr.viscous_pass2(level, S_in)
        target = fpr.onto(f_int, V, A_V)
        ref = f_int.copy()
        ref[:, 1:5] = ref[:, 1:5] + fpr.emulated_viscous_flux(em, S_in)[:, 1:5]
        check(f"{mesh} viscous_flux [{tag}; {path}] F(internal) + V", far.K(got, *target, f0=f_int), far.K(ref, *target, f0=f_int).max(axis=0))
        assert np.isfinite(S_got).all() and V[:, 1:].any()
        s.zero_fluxes(0)
    em.close()
    s.close(); msh.close()


@pytest.mark.parametrize("mesh", fpr.MESHES)
def test_jst_launches_per_node(oracle, cases, mesh):
    """After compute_fluxes: jst_laplacian, jst_sensor and jst_radius against pass 1.  Then F(internal) with JST off and the same
    call with it on: F(internal) + C against F(internal) as read + pass 2 in long double ON THE L, nu AND r THE GPU WROTE."""
    import jst_emulator as jse
    msh, s = _solver(cases[mesh])
    em = fpr.make_emulator(oracle, cases[mesh], mesh)
    level, start, path = fpr.ref_level(em), em.variables(0), _path(mesh, s)
    s.set_time_step("local", fpr.LOCAL_CFL[mesh])
    s.set(0, "variables", start)
    sensor = fpr.jst_sensor(level, start)
    emulated = dict(zip(("L", "nu", "r"), jse.sensor(start, em.ea[0], em.eb[0])))
    for k2, k4 in fpr.JST_PAIRS:
        s.set_jst(k2, k4, 1)
        s.zero_fluxes(0)
        s.compute_fluxes(0)
        got = {"L": s.get(0, "jst_laplacian"), "nu": s.get(0, "jst_sensor"), "r": s.get(0, "jst_radius")}
        for name in ("L", "nu", "r"):
            k_ref = far.K(emulated[name], *sensor[name])
            check(f"{mesh} jst_sensor [({k2}, {k4}); {path}] {name}", far.K(got[name], *sensor[name]), k_ref.reshape(len(k_ref), -1).max(axis=0))
        s.zero_fluxes(0)
        s.set_jst(0.0, 0.0, 0)
        s.compute_flux_edge(0)
        f_int = s.get(0, "fluxes")
        s.zero_fluxes(0)
        s.set_jst(k2, k4, 1)
        s.compute_flux_edge(0)
        f_c = s.get(0, "fluxes")
        L, nu, r = s.get(0, "jst_laplacian"), s.get(0, "jst_sensor"), s.get(0, "jst_radius")
        _same(L, got["L"], f"{mesh}: pass 1 keeps row order: the same bits in every launch")
        C_, A_C = fpr.jst_correction(level, start, L, nu, r, k2, k4)
        target = fpr.onto(f_int, C_, A_C)
        ref = f_int + fpr.emulated_correction(em, start, L, nu, r, k2, k4)
        check(f"{mesh} jst_dissipation [({k2}, {k4}); {path}] F(internal) + C", far.K(f_c, *target, f0=f_int), far.K(ref, *target, f0=f_int).max(axis=0))
        s.zero_fluxes(0)
    em.close()
    s.close(); msh.close()


SWEEPS = [(m, (o,)) for m in fpr.SWEEP_MESHES for o in fpr.SWEEP_OPTIONS] + [("lattice_A", fpr.SWEEP_OPTIONS)]


@pytest.mark.parametrize("mesh,options", SWEEPS, ids=[f"{m}-{'+'.join(o)}" for m, o in SWEEPS])
def test_one_sweep_per_node(oracle, cases, mesh, options):
    """smooth(0, 1) with each option alone and, on lattice A, all together: state and residual by K_sweep, the step factors
    (after the viscous limit and dual time's clamp) by their relative error."""
    msh, s = _solver(cases[mesh])
    em = fpr.make_emulator(oracle, cases[mesh], mesh)
    level, start, path = fpr.ref_level(em), em.variables(0), _path(mesh, s)
    W, kw, settings = fpr.sweep_setup(em, mesh, options)
    s.set_time_step("local", fpr.LOCAL_CFL[mesh])
    s.set(0, "variables", start)
    if "viscous" in settings:
        s.set_viscous(*settings["viscous"])
    if "jst" in settings:
        s.set_jst(*settings["jst"], 1)
    if "smoothing" in settings:
        s.set_residual_smoothing(*settings["smoothing"])
    if "dual" in settings:
        dt, Wn, Wn1 = settings["dual"]
        s.set_dual_time(dt)
        s.dual_time_order(2)
        s.set(0, "time_n", Wn)
        s.set(0, "time_n1", Wn1)
    _same(s.get(0, "variables"), W, f"{mesh}: the state the sweep starts from")
    rc, emu = fpr.emulated_sweep(em)
    ref = fpr.sweep(level, W, "local", fpr.LOCAL_CFL[mesh], **kw)
    assert rc == 0 and ref["valid"]
    s.zero_fluxes(0)
    s.smooth(0, 1)
    what = f"{mesh} sweep [{' + '.join(options)}; {path}]"
    check(f"{what} state", far.K_sweep(s.get(0, "variables"), ref["W"], ref["D"]), far.K_sweep(emu["W"], ref["W"], ref["D"]).max(axis=0))
    check(f"{what} residual", far.K_sweep(s.get(0, "residuals"), ref["res"], ref["D"]), far.K_sweep(emu["res"], ref["res"], ref["D"]).max(axis=0))
    check(f"{what} step factor", far.rel_units(s.get(0, "step_factors"), ref["sf"]), far.rel_units(emu["sf"], ref["sf"]).max())
    assert s.pending_invalid_state()[0] == 0
    em.close()
    s.close(); msh.close()


def test_transfers_per_node(oracle, cases):
    """Lattice A's hierarchy with FAS on: fas_restrict(0) — the coarse state and W0 against the children's mean, P against the
    children's summed T minus R(W0), with T and R(W0) the GPU's own (compute_fluxes from zero on the same states) —, then
    fas_prolong(0) and prolong_state(0) from a coarse state distinct from W0, against the interpolation in long double."""
    mesh = "lattice_A"
    msh, s = _solver(cases[mesh])
    em = fpr.make_emulator(oracle, cases[mesh], mesh, fas=True)
    t = fpr.transfer_setup(em, mesh)
    parent, interp, W_fine, W_coarse = t["parent"], t["interp"], t["W_fine"], t["W_coarse"]
    s.set_time_step("local", fpr.LOCAL_CFL[mesh])
    s.set_fas(True)
    s.set(0, "variables", W_fine)
    before = s.get(1, "variables")
    _same(before, t["coarse_before"], "level 1 before the restriction: the far field")
    s.zero_fluxes(0)
    s.compute_fluxes(0)
    T = s.get(0, "fluxes")
    s.zero_fluxes(0)
    s.fas_restrict(0)
    coarse, W0, P = s.get(1, "variables"), s.get(1, "fas_start"), s.get(1, "fas_forcing")
    _same(W0, coarse, "W0 is a copy of the restricted state")
    target = fpr.restrict_state(parent, W_fine, before)
    check(f"{mesh} restrict_fas coarse state and W0", far.K(coarse, *target, f0=before),
          far.K(fpr.emulated_restriction(em, 0, W_fine, before), *target, f0=before).max(axis=0))
    s.zero_fluxes(1)
    s.compute_fluxes(1)
    R = s.get(1, "fluxes")
    s.zero_fluxes(1)
    target = fpr.restrict_forcing(parent, T, R)
    check(f"{mesh} restrict_fas + fas_forcing P", far.K(P, *target), far.K(fpr.emulated_forcing(parent, T, R), *target).max(axis=0))
    s.set(1, "variables", W_coarse)
    s.fas_prolong(0)
    target = fpr.fas_correction(interp, W_fine, W0, W_coarse)
    ref = W_fine + (0.0 - fpr.emulated_wavg(em, 0, W0 - W_coarse))
    check(f"{mesh} prolong_fas fine state", far.K(s.get(0, "variables"), *target), far.K(ref, *target).max(axis=0))
    s.prolong_state(0)
    target = interp(W_coarse)
    ref = 0.0 - (0.0 - fpr.emulated_wavg(em, 0, W_coarse))
    check(f"{mesh} prolong_state fine state", far.K(s.get(0, "variables"), *target), far.K(ref, *target).max(axis=0))
    em.close()
    s.close(); msh.close()
