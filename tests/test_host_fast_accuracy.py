"""The fast mode's accuracy yardstick on the CPU (tests/fast_accuracy_reference.py; nothing here needs a GPU).

1. A condition on the INPUTS of tests/test_gpu_fast_accuracy.py: on every level / state pair it runs, the oracle's own double
   evaluation lies within K <= 8 (flux sums) and K_sweep <= 8 (one sweep) of the long-double reference, every state passes
   ora_check_for_invalid_variables and stays valid through the sweep.  The GPU bound is 3 x the oracle's K on the same input:
   this keeps that bound a small multiple of rounding.
2. The power of the new metric, on a numpy model of the kernel's algebra: a reciprocal one Newton step short (1e-13), one off by
   1e-14 and a sound speed whose root is off by 1e-13 pass the whole-array metric of the older tests (1e-12) and exceed the GPU
   bound on the `wide` state; so does one mirrored share lost at the node with the smallest magnitude.
"""
import numpy as np
import pytest

import fast_accuracy_reference as far

K_MAX_ORACLE = 8.0          # the oracle against long double: measured <= 4.6 on the levels used
MARGIN = 3.0                # the GPU bound: 3 x the oracle's K on the same input (tests/test_gpu_fast_accuracy.py)
OLD_REL_LAUNCH = 1e-12      # tests/test_gpu_order_free.py: max |difference| / max |reference value| per array


@pytest.fixture(scope="module")
def cases(oracle, mesh3_dir, fvcorr_dir):
    return far.build_cases(oracle, mesh3_dir, fvcorr_dir)


def test_long_double_is_an_extended_type():
    assert np.finfo(np.longdouble).nmant >= 63


def test_case_names_are_the_cases(cases):
    assert tuple(cases) == far.CASE_NAMES


@pytest.mark.parametrize("case", far.CASE_NAMES)
def test_oracle_is_within_the_bound_on_every_input_of_the_gpu_tests(oracle, cases, case):
    levels, variant, l, states = cases[case]
    level = far.RefLevel.from_dict(oracle, levels[l], variant)
    for kind in states:
        q = far.make_state(kind, level.nel, level.ff_var, far.state_seed(case, kind))
        assert far.state_is_valid(oracle, q), f"{case} {kind}: the state itself is invalid"
        sums = far.class_sums(level, q)
        f0 = far.f0_for(level, 17 + l)
        for c in far.CLASSES:                                    # each class alone onto a non-zero f0
            got = far.oracle_class(oracle, level, c, q, f0.copy())
            k = far.K(got, *far.accumulate(sums, (c,), f0), f0=f0)
            print(f"{case} {kind} {c}+=: oracle K max per component {k.max(axis=0)}")
            assert k.max() <= K_MAX_ORACLE, f"{case} {kind}: class {c}"
        got = np.zeros((level.nel, 5))
        for c in far.CLASSES:
            far.oracle_class(oracle, level, c, q, got)
        k = far.K(got, *far.accumulate(sums, far.CLASSES))
        print(f"{case} {kind} all: oracle K max per component {k.max(axis=0)}")
        assert k.max() <= K_MAX_ORACLE, f"{case} {kind}: all classes from zero"
        for mode in ("reference", "local"):
            cfl = far.sweep_cfl(case, kind, mode)
            ref = far.sweep(level, q, mode, cfl)
            ora = far.oracle_sweep(oracle, level, q, mode, cfl)
            assert ref["valid"] and ora["rc"] == 0, f"{case} {kind} {mode}: the state does not survive one sweep"
            kw, kr = far.K_sweep(ora["W"], ref["W"], ref["D"]), far.K_sweep(ora["res"], ref["res"], ref["D"])
            ks = far.rel_units(ora["sf"], ref["sf"])
            print(f"{case} {kind} sweep/{mode}: oracle K_sweep state {kw.max(axis=0)} residual {kr.max(axis=0)} step factor {ks.max():.2f}")
            assert kw.max() <= K_MAX_ORACLE and kr.max() <= K_MAX_ORACLE, f"{case} {kind}: sweep under {mode} steps"
            assert ks.max() <= K_MAX_ORACLE, f"{case} {kind}: step factors under {mode} steps"


def test_magnitude_is_zero_exactly_where_nothing_is_added(oracle, cases):
    """A node without a far-field face has A = 0 for that class from zero: K reads 0 for an untouched value, inf otherwise."""
    levels, variant, l, _ = cases["mesh3_L2"]
    level = far.RefLevel.from_dict(oracle, levels[l], variant)
    q = far.make_state("perturbed", level.nel, level.ff_var, 1)
    S, A = far.accumulate(far.class_sums(level, q), ("far",))
    untouched = np.flatnonzero((A == 0).all(axis=1))
    assert len(untouched) > 0
    got = S.astype(np.float64)
    assert far.K(got, S, A).max() <= 1.0
    got[untouched[0], 2] = 1e-300
    assert np.isinf(far.K(got, S, A)[untouched[0], 2])


@pytest.fixture(scope="module")
def wide_level0(oracle, cases):
    levels, variant, l, _ = cases["mesh3_L0"]
    level = far.RefLevel.from_dict(oracle, levels[l], variant)
    q = far.make_state("wide", level.nel, level.ff_var, far.state_seed("mesh3_L0", "wide"))
    S, A = far.accumulate(far.class_sums(level, q), ("internal",))
    want = far.oracle_class(oracle, level, "internal", q, np.zeros((level.nel, 5)))
    return level, q, S, A, want, far.K(want, S, A).max(axis=0)


def _old_metric(got, want):
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)


def test_model_of_the_fast_algebra_is_inside_the_gpu_bound(wide_level0):
    level, q, S, A, want, k_ref = wide_level0
    k = far.K(far.fast_model_internal(level, q), S, A).max(axis=0)
    print(f"oracle K {k_ref}\nmodel  K {k}")
    assert (k <= 1.5 * k_ref).all(), "the regrouped algebra itself stays within 1.5 x the oracle"


@pytest.mark.parametrize("name,fault", [
    ("reciprocal one Newton step short (1e-13)", {"rcp_error": 1e-13}),
    ("reciprocal off by 1e-14", {"rcp_error": 1e-14}),
    ("sound speed's root off by 1e-13", {"c_root_error": 1e-13}),
])
def test_faults_the_old_metric_passes_exceed_the_new_bound(wide_level0, name, fault):
    level, q, S, A, want, k_ref = wide_level0
    got = far.fast_model_internal(level, q, **fault)
    k = far.K(got, S, A).max(axis=0)
    old = _old_metric(got, want)
    print(f"{name}: K {k} against 3 x {k_ref}; old metric {old:.2e}")
    assert old <= OLD_REL_LAUNCH, "the whole-array metric was meant to pass this fault"
    assert (k > MARGIN * k_ref).any(), "the per-node bound was meant to catch it"


def test_a_dropped_mirrored_share_exceeds_the_new_bound(wide_level0):
    level, q, S, A, want, k_ref = wide_level0
    node = int(np.argmin(A.sum(axis=1)))
    got = far.fast_model_internal(level, q, drop_share_at=node)
    k = far.K(got, S, A)
    print(f"share dropped at node {node}: K there {k[node]}, old metric {_old_metric(got, want):.2e}")
    assert (k.max(axis=0) > MARGIN * k_ref).any()
    assert k[node].max() > 1e6, "a whole term is missing at that node"
