"""The fast mode (MGCFD_OPT_EXACT = 0, MGCFD_OPT_FLUX_VARIANT = 64 | 1) per node and component against long double.

The other fast-mode tests compare whole arrays (max |difference| / max |value| <= 1e-12 per launch), on the far field +-1 %:
a kernel may lose three digits of a reciprocal or a root under that metric (tests/test_host_fast_accuracy.py shows it).  Here
every node's result is measured in units of one rounding of the magnitudes that were added into it
(tests/fast_accuracy_reference.py: K and K_sweep), and the bound is

    K <= 3 * K_ref        per component; K_ref = the oracle's own maximum K on the same input, computed here

The 3 covers estimate-based 1/x and sqrt(x) that are faithful, not correctly rounded; momenta re-formed from velocities; and an
unordered sum.  (A numpy model of that algebra stays within 1.5 x the oracle; FMA contraction only removes roundings.)

Which instantiation of k_flux_free a level reaches is read off the plan — has_order_free, has_half_rows, tiling() — and
printed with every figure (lines that begin with FASTACC: profiles/fast_mode_accuracy.txt is made of them):

    mesh3_L0..2    3-level lattice hierarchy: 546-node LDS image; standalone <F, ACC> and <F, from zero>; stage roles 0, 1, 2
                   (global steps) and 1, 1, 2 (local steps)
    m6wing_1lvl    one level: its last stage looks ahead — role 3 under global steps, the generic epilogue under local steps
    fvcorr         one level, fvcorr's local step: roles 1, 1 and the generic epilogue for the look-ahead
    mixed          (12, 6) mixed elements: more than five half rows per lane (LONG), generic epilogue
    tet            30,000 tetrahedral nodes: halos beyond the shared table (WIDE), generic epilogue
    children       MGCFD_FREE_WG3=1: the kTileCap image on mesh3_L0; MGCFD_FREE_NO_ROLES=1: the generic epilogue with the
                   546-node image (both read once per process: tests/fast_accuracy_children.py)
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import fast_accuracy_reference as far

pytestmark = pytest.mark.gpu

FREE = 64 | 1           # order-free accumulation, edge-length factor recomputed
GATHER = 1              # the contracted node gather
MARGIN = 3.0
FREE_CAP4_HALO = 290    # preprocess.hpp: kFreeCap4Halo
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cases(oracle, mesh3_dir, fvcorr_dir):
    return far.build_cases(oracle, mesh3_dir, fvcorr_dir)


_REF = {}


def reference(oracle, cases, case, kind):
    """Level, state, long-double sums and the oracle's K on them: computed once per (case, state), shared, never modified."""
    key = (case, kind)
    if key not in _REF:
        levels, variant, l, _ = cases[case]
        level = _REF.get(case) or far.RefLevel.from_dict(oracle, levels[l], variant)
        _REF[case] = level
        q = far.make_state(kind, level.nel, level.ff_var, far.state_seed(case, kind))
        sums = far.class_sums(level, q)
        f0 = far.f0_for(level, 17 + l)
        r = {"level": level, "q": q, "f0": f0, "target": {}, "k_ref": {}}
        for c in far.CLASSES:
            S, A = far.accumulate(sums, (c,), f0)
            r["target"][c] = (S, A)
            r["k_ref"][c] = far.K(far.oracle_class(oracle, level, c, q, f0.copy()), S, A, f0=f0).max(axis=0)
        S, A = far.accumulate(sums, far.CLASSES)
        got = np.zeros((level.nel, 5))
        for c in far.CLASSES:
            far.oracle_class(oracle, level, c, q, got)
        r["target"]["all"] = (S, A)
        r["k_ref"]["all"] = far.K(got, S, A).max(axis=0)
        _REF[key] = r
    return _REF[key]


def sweep_reference(oracle, cases, case, kind, mode):
    key = (case, kind, mode)
    if key not in _REF:
        r = reference(oracle, cases, case, kind)
        cfl = far.sweep_cfl(case, kind, mode)
        ref = far.sweep(r["level"], r["q"], mode, cfl)
        ora = far.oracle_sweep(oracle, r["level"], r["q"], mode, cfl)
        assert ref["valid"] and ora["rc"] == 0
        _REF[key] = {"cfl": cfl, "ref": ref,
                     "k_W": far.K_sweep(ora["W"], ref["W"], ref["D"]).max(axis=0),
                     "k_res": far.K_sweep(ora["res"], ref["res"], ref["D"]).max(axis=0),
                     "k_sf": far.rel_units(ora["sf"], ref["sf"]).max()}
    return _REF[key]


def node_class_of_worst(k):
    """Where the largest K lies: (node, component)."""
    node, comp = np.unravel_index(np.argmax(k), k.shape)
    return int(node), int(comp)


def check(label, k, k_ref):
    """K <= 3 K_ref per component; the figures are printed before anything is asserted."""
    kmax = np.atleast_1d(np.max(k, axis=0))
    k_ref = np.atleast_1d(k_ref)
    print("FASTACC %-78s K %s | oracle %s" % (label, np.array2string(kmax, precision=2, floatmode="fixed"),
                                             np.array2string(k_ref, precision=2, floatmode="fixed")))
    if not (kmax <= MARGIN * k_ref).all():
        node, comp = node_class_of_worst(np.asarray(k).reshape(len(k), -1) / np.maximum(MARGIN * k_ref, 1e-300))
        raise AssertionError(f"{label}: K {kmax} above 3 x {k_ref}; worst at node {node}, component {comp}")


def instantiation(s, l, wg3=False, no_roles=False):
    """(description, fast path) of the k_flux_free instantiation level l launches, from the plan."""
    assert s.has_order_free(l), "this level has no half-row plan: k_flux_free never runs"
    til = s.tiling(l)
    wide = til["halo_max"] > til["halo_capacity"]
    cap4 = til["halo_max"] <= FREE_CAP4_HALO and not wg3 and not wide
    # (has_half_rows is false on a level without long rows or wide halos only for more than five half rows per lane)
    long_rows = (not wide) and til["list_entries"] == 0 and not s.has_half_rows(l)
    cap = "WIDE(768)" if wide else ("CAP546" if cap4 else "CAP559")
    name = f"{cap}{' LONG' if long_rows and not wide else ''}"
    return name, (cap4 and not long_rows and not no_roles), wide, long_rows


def stage_roles(fast_path, single_level, variant, mode):
    """The ROLE of the three fused stages (kernels.hip: stage_role, free_stage_role), -1 the generic epilogue."""
    if not fast_path:
        return "generic,generic,generic"
    global_dt = mode == "reference" and variant != 0
    first = "0" if global_dt else "1"
    last = ("3" if global_dt else "generic") if single_level else "2"
    return f"{first},1,{last}"


def run_flux_checks(oracle, cases, case, s, l, what, variant_name):
    _, _, _, states = cases[case]
    for kind in states:
        r = reference(oracle, cases, case, kind)
        s.set(l, "variables", r["q"])
        launch = {"internal": s.compute_flux_edge, "wall": s.compute_boundary_flux_edge, "far": s.compute_wall_flux_edge}
        for c in far.CLASSES:                                        # each class alone onto a non-zero f0, twice
            for run in (1, 2):
                s.set(l, "fluxes", r["f0"])
                launch[c](l)
                k = far.K(s.get(l, "fluxes"), *r["target"][c], f0=r["f0"])
                check(f"{case} {kind} {variant_name} [{what}, ACC] {c} += run {run}", k, r["k_ref"][c])
        for run in (1, 2):                                           # all classes from zero, twice
            s.zero_fluxes(l)
            s.compute_fluxes(l)
            k = far.K(s.get(l, "fluxes"), *r["target"]["all"])
            check(f"{case} {kind} {variant_name} [{what}] all from zero run {run}", k, r["k_ref"]["all"])


@pytest.mark.parametrize("case", far.CASE_NAMES)
def test_flux_launches_per_node(oracle, cases, case):
    """Each class alone onto a non-zero f0 and all classes from zero, each launch twice (LDS atomics: the runs need not be
    equal, both lie inside the bound), with the order-free kernel and with the contracted node gather."""
    import mgcfd
    levels, variant, l, _ = cases[case]
    assert mgcfd.plan_audit(levels, variant) == "", "an index of the plan is out of range: nothing is launched"
    s = mgcfd.Solver.from_arrays(levels, variant)
    s.set_option("exact", 0)
    s.set_option("flux_variant", FREE)
    name, _, wide, long_rows = instantiation(s, l)
    if case.startswith("mesh3") or case in ("fvcorr", "m6wing_1lvl"):
        assert name == "CAP546", f"{case} was meant to take the 546-node image, got {name}"
    if case == "mixed":
        assert long_rows and not wide, "the mixed level was meant to have more than five half rows per lane and no wide halo"
    if case == "tet":
        assert wide, "the tetrahedral level was meant to have halos beyond the shared table"
    run_flux_checks(oracle, cases, case, s, l, name, "k_flux_free")
    s.set_option("flux_variant", GATHER)
    run_flux_checks(oracle, cases, case, s, l, "node gather", "k_flux_tile")
    s.close()


def run_sweep_checks(oracle, cases, case, s, l, label, kinds=None):
    levels, variant, _, states = cases[case]
    for kind in (kinds or states):
        r = reference(oracle, cases, case, kind)
        for mode in ("reference", "local"):
            w = sweep_reference(oracle, cases, case, kind, mode)
            s.set_time_step(mode, w["cfl"])
            s.set(l, "variables", r["q"])
            s.zero_fluxes(l)
            s.smooth(l, 1)
            ref = w["ref"]
            got = s.get(l, "variables")
            what = label(mode)
            check(f"{case} {kind} sweep/{mode} [{what}] state", far.K_sweep(got, ref["W"], ref["D"]), w["k_W"])
            check(f"{case} {kind} sweep/{mode} [{what}] residual", far.K_sweep(s.get(l, "residuals"), ref["res"], ref["D"]), w["k_res"])
            check(f"{case} {kind} sweep/{mode} [{what}] step factor", far.rel_units(s.get(l, "step_factors"), ref["sf"]), w["k_sf"])
            if len(levels) == 1:
                # the last stage left the next sweep's step-factor work behind (look-ahead): the next sweep's factors, against
                # the definition on the state this sweep produced
                level = r["level"]
                want = far.step_factor(level, got, mode, w["cfl"])
                import time_step_emulator as tse
                ora = tse.step_factors(mode, w["cfl"], got, level.volumes, tse.libm_cbrt(level.volumes), level.variant)
                s.smooth(l, 1)
                check(f"{case} {kind} sweep/{mode} [{what}] step factor of the sweep after (look-ahead)",
                      far.rel_units(s.get(l, "step_factors"), want), far.rel_units(ora, want).max())
    s.set_time_step("reference", 0.5)


@pytest.mark.parametrize("case", far.CASE_NAMES)
def test_one_sweep_per_node(oracle, cases, case):
    """smooth(l, 1) under the reference's and under local steps: state, residual and step factors."""
    import mgcfd
    levels, variant, l, _ = cases[case]
    assert mgcfd.plan_audit(levels, variant) == ""
    s = mgcfd.Solver.from_arrays(levels, variant)
    s.set_option("exact", 0)
    s.set_option("flux_variant", FREE)
    name, fast_path, _, _ = instantiation(s, l)
    if case in ("mesh3_L0", "mesh3_L1", "mesh3_L2", "fvcorr", "m6wing_1lvl"):
        assert fast_path, f"{case} was meant to run the role-specialised stages"
    else:
        assert not fast_path, f"{case} was meant to run the generic epilogue"
    run_sweep_checks(oracle, cases, case, s, l,
                     lambda mode: f"{name} FUSE roles {stage_roles(fast_path, len(levels) == 1, variant, mode)}")
    s.close()


@pytest.mark.parametrize("env,what", [("MGCFD_FREE_WG3", "CAP559"), ("MGCFD_FREE_NO_ROLES", "CAP546")])
def test_instantiations_behind_process_wide_switches(oracle, cases, mesh3_dir, tmp_path, env, what):
    """The kTileCap image on a level that would take the small one, and the generic epilogue in place of the roles: both
    switches are read once per process, so a child runs the launches and this process measures what it wrote."""
    case = "mesh3_L0"
    out = str(tmp_path / "child.npz")
    e = dict(os.environ)
    e.pop("MGCFD_FREE_WG3", None)
    e.pop("MGCFD_FREE_NO_ROLES", None)
    e[env] = "1"
    p = subprocess.run([sys.executable, os.path.join(HERE, "fast_accuracy_children.py"), mesh3_dir, "0", out],
                       env=e, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = np.load(out)
    for kind in ("perturbed", "wide"):
        r = reference(oracle, cases, case, kind)
        assert np.array_equal(got[f"{kind}/q"], r["q"])
        for run in (1, 2):
            check(f"{case} {kind} k_flux_free [{what}, ACC; {env}=1] internal += run {run}",
                  far.K(got[f"{kind}/internal/{run}"], *r["target"]["internal"], f0=r["f0"]), r["k_ref"]["internal"])
            check(f"{case} {kind} k_flux_free [{what}; {env}=1] all from zero run {run}",
                  far.K(got[f"{kind}/all/{run}"], *r["target"]["all"]), r["k_ref"]["all"])
        for mode in ("reference", "local"):
            w = sweep_reference(oracle, cases, case, kind, mode)
            ref = w["ref"]
            label = f"{case} {kind} sweep/{mode} [{what} FUSE roles generic,generic,generic; {env}=1]"
            check(label + " state", far.K_sweep(got[f"{kind}/{mode}/W"], ref["W"], ref["D"]), w["k_W"])
            check(label + " residual", far.K_sweep(got[f"{kind}/{mode}/res"], ref["res"], ref["D"]), w["k_res"])
            check(label + " step factor", far.rel_units(got[f"{kind}/{mode}/sf"], ref["sf"]), w["k_sf"])


# ------------------------------------------------------------------------------------------------------------------
# The approximations on their own (mgcfd_diag_fast_math)
# ------------------------------------------------------------------------------------------------------------------
FAITHFUL = 2.0 ** -52


def _neighbours(x, n=64):
    """The n doubles below x, x, and the n doubles above."""
    bits = np.array([x], dtype=np.float64).view(np.int64)[0]
    return (bits + np.arange(-n, n + 1, dtype=np.int64)).view(np.float64)


def _fast_math_arguments(oracle, cases):
    pts = [np.logspace(-290, 290, 4096), _neighbours(1.0), _neighbours(2.0), _neighbours(4.0)]
    r = reference(oracle, cases, "mesh3_L0", "wide")
    P = far.point(r["q"])
    e = r["level"].edges
    half = 0.25 * (e["x"] ** 2 + e["y"] ** 2 + e["z"] ** 2)
    rho = r["q"][:, 0]
    sq = (P["speed"] ** 2).astype(np.float64)
    c2 = (P["c"] ** 2).astype(np.float64)
    return {"rcp": np.concatenate(pts + [rho]),
            "sqrt": np.concatenate(pts + [sq[sq > 0], c2]),
            "sqrt_pos": np.concatenate(pts + [sq[sq > 0], c2, half[half > 0]])}


def test_reciprocal_and_root_are_faithfully_rounded(oracle, cases, mesh3_dir):
    """fast_rcp, fast_sqrt and fast_sqrt_pos over [1e-290, 1e290], around 1, 2 and 4, and on what the `wide` state feeds them:
    relative error <= 2^-52 against long double; and the special values the flux kernel relies on."""
    import mgcfd
    s = mgcfd.Solver.from_mesh(mgcfd.Mesh("input.dat", mesh3_dir))
    LD = np.longdouble
    worst = {}
    for kind, x in _fast_math_arguments(oracle, cases).items():
        got = s.diag_fast_math(kind, x)
        want = LD(1.0) / x.astype(LD) if kind == "rcp" else np.sqrt(x.astype(LD))
        err = (np.abs(got.astype(LD) - want) / want).astype(np.float64)
        worst[kind] = err.max()
        print("FASTACC %-14s %5d arguments: max relative error %.3f x 2^-53 at x = %r" % ("fast_" + kind, len(x), err.max() * 2.0 ** 53, float(x[np.argmax(err)])))
    inf, nan = np.inf, np.nan
    root = s.diag_fast_math("sqrt", np.array([0.0, inf, -1.0, -0.0, -inf, nan, -1e-300]))
    rcp = s.diag_fast_math("rcp", np.array([0.0, -0.0]))
    s.close()
    for kind, e in worst.items():
        assert e <= FAITHFUL, f"fast_{kind}: relative error {e:.3e} above 2^-52"
    assert root[0] == 0.0 and not np.signbit(root[0]), "fast_sqrt(+0.0) must be +0.0"
    assert root[1] == inf, "fast_sqrt(inf) must be inf"
    assert np.isnan(root[2]) and np.isnan(root[4]) and np.isnan(root[5]) and np.isnan(root[6]), "negative and NaN arguments give NaN"
    assert root[3] == 0.0, "fast_sqrt(-0.0) is a zero"
    assert not np.isfinite(rcp).any(), "fast_rcp(0) is not finite"
