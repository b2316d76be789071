"""Host tests of multigrid cycle control (no GPU): the numpy emulator (tests/cycle_emulator.py) with the default configuration is
its parents bit for bit, F and W are the same cycle on three levels and differ on four, W and F converge on lattice C where
the default V stalls, the state interpolation reproduces a uniform state and writes +0.0 for zeros, everything tests/test_gpu_cycle.py
runs stays valid, and the new symbols are declared.  The measured histories are recorded in profiles/cycle_convergence.txt."""
import ctypes as C
import os

import numpy as np
import pytest

import cycle_emulator as ce
import fas_emulator as fe
import viscous_emulator as ve

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mgcfd_set_cycle", "mgcfd_get_cycle", "mgcfd_run_cycles_from", "mgcfd_prolong_state", "mgcfd_full_multigrid")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("cycle_lattices")
    return {name: ce.write_lattice(name, d) for name in ("A", "C")}


def test_symbols_are_exported_and_typed():
    import mgcfd
    header = open(os.path.join(ROOT, "include", "mgcfd.h")).read()
    lib = mgcfd.load_library()
    for name in NEW_SYMBOLS:
        assert name in mgcfd.EXPORTED_SYMBOLS and hasattr(lib, name) and f"int {name}(" in header
        assert getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes
    assert lib.mgcfd_abi_version() == 1
    for name, value in (("MGCFD_CYCLE_V", 0), ("MGCFD_CYCLE_W", 1), ("MGCFD_CYCLE_F", 2)):
        assert f"{name} = {value}" in header
    assert "#define MGCFD_MAX_CYCLE_SWEEPS 8" in header and ce.MAX_SWEEPS == 8
    from mgcfd import api
    assert api.CYCLE_SHAPES == {"V": 0, "W": 1, "F": 2} and api.MAX_CYCLE_SWEEPS == 8
    for method in ("set_cycle", "get_cycle", "run_cycles_from", "prolong_state", "full_multigrid"):
        assert callable(getattr(api.Solver, method))


def test_lattice_c_sizes(oracle, lattices):
    em = ce.CycleOracle(oracle, lattices["C"])
    assert [em.oc.levels[l].nel for l in range(em.n)] == [4886, 2178, 728, 215] and em.variant == 0
    assert em.get_cycle() == ("V", [1, 1, 1, 1], [0, 1, 1, 1]) and em.default_cycle()
    em.close()


@pytest.mark.parametrize("case", ["A", "m6_3lvl"])
@pytest.mark.parametrize("fas", [False, True])
def test_defaults_are_the_parents(case, fas, oracle, lattices):
    """Never configured, and the default configuration set explicitly: ViscousOracle's and FasOracle's RMS history and state on
    every level, bit for bit."""
    where = lattices.get(case, case)
    mode, cfl = ("local", 1.0) if case == "A" else ("reference", 0.5)
    wants = []
    for cls in (ve.ViscousOracle, fe.FasOracle):
        em = cls(oracle, where, mode, cfl, fas=fas)
        rc, rms = em.cycles(ce.GPU_CYCLES)
        assert rc == 0
        wants.append((rms, [em.variables(l) for l in range(em.n)]))
        em.close()
    for explicit in (False, True):
        em = ce.CycleOracle(oracle, where, mode, cfl, fas=fas)
        if explicit:
            em.set_cycle("V", *ce.default_sweeps(em.n))
        rc, rms = em.cycles(ce.GPU_CYCLES)
        assert rc == 0
        for want_rms, want_vars in wants:
            assert np.array_equal(_bits(rms), _bits(want_rms))
            assert all(np.array_equal(_bits(em.variables(l)), _bits(want_vars[l])) for l in range(em.n))
        em.close()


def _shaped(oracle, where, shape, fas, cycles, post0=0, mode="local", cfl=1.0):
    em = ce.CycleOracle(oracle, where, mode, cfl, fas=fas)
    pre, post = ce.default_sweeps(em.n)
    em.set_cycle(shape, pre, [post0] + post[1:])
    rc, rms = em.cycles(cycles)
    return em, rc, rms


@pytest.mark.parametrize("fas", [False, True])
def test_f_is_w_on_three_levels_and_not_on_four(fas, oracle, lattices):
    out = {}
    for name in ("A", "C"):
        for shape in ("W", "F"):
            mode, cfl = ("local", 1.0) if fas else ("reference", 0.5)
            em, rc, rms = _shaped(oracle, lattices[name], shape, fas, ce.GPU_CYCLES, mode=mode, cfl=cfl)
            assert rc == 0
            out[name, shape] = (rms, [em.variables(l) for l in range(em.n)])
            em.close()
    assert np.array_equal(_bits(out["A", "W"][0]), _bits(out["A", "F"][0]))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(out["A", "W"][1], out["A", "F"][1]))
    assert not np.array_equal(_bits(out["C", "W"][1][0]), _bits(out["C", "F"][1][0]))


def test_convergence_on_lattice_c(oracle, lattices):
    """FAS, local steps at CFL 1.0, 60 cycles from the far field, the RMS of component 0 of F_0 / vol: W <= 1e-4 and F <= 1e-4
    where the default V stays above 1e-2."""
    metric = {}
    for shape in ce.SHAPES:
        em, rc, _ = _shaped(oracle, lattices["C"], shape, True, ce.CONV_CYCLES)
        assert rc == 0, shape
        metric[shape] = em.density_residual_rms()
        print("lattice C, FAS, local 1.0,", shape, "after", ce.CONV_CYCLES, "cycles:", metric[shape], "work per cycle", em.work / ce.CONV_CYCLES)
        em.close()
    assert metric["W"] <= ce.CONV_SHAPED_BOUND
    assert metric["F"] <= ce.CONV_SHAPED_BOUND
    assert metric["V"] > ce.CONV_V_FLOOR


def test_prolong_state_of_a_uniform_state_and_of_zeros(oracle, lattices):
    """A uniform coarse state comes out exactly: with every component a power of two (or zero) each product w * u is the
    weight scaled exactly, so the sum is u * w_sum bit for bit and the division gives u.  (For other values the sums round
    differently from the weight sum and the result is u only to a few ulp.)  Zeros of either sign come out as +0.0; whatever
    the fine level held is overwritten; residuals are untouched."""
    em = ce.CycleOracle(oracle, lattices["A"])
    uniform = np.array([1.0, -0.25, 0.0, 2.0, 4.0])
    for l in (1, 0):
        em._var(l + 1)[:] = uniform
        em._var(l)[:] = 7.0
        res = [em.oc.array(k, "residuals").copy() for k in (l, l + 1)]
        em.oc.array(l, "residuals")[:] = 0.5
        em.prolong_state(l)
        got = em.variables(l)
        assert np.array_equal(_bits(got), _bits(np.tile(uniform, (len(got), 1))))
        assert (em.oc.array(l, "residuals") == 0.5).all()
        em.oc.array(l, "residuals")[:] = res[0]
        em._var(l + 1)[:] = -0.0
        em.prolong_state(l)
        assert np.array_equal(_bits(em.variables(l)), np.zeros((len(got), 5), dtype=np.int64))
    em.close()


def test_full_multigrid_is_its_parts(oracle, lattices):
    em = ce.CycleOracle(oracle, lattices["A"], "local", 1.0, fas=True)
    parts = ce.CycleOracle(oracle, lattices["A"], "local", 1.0, fas=True)
    rc, hist = em.full_multigrid([0, 3, 2])
    L = parts.oc.levels
    for l in range(2):
        parts.lib.ora_mg_restrict(L[l].variables, L[l + 1].variables, L[l + 1].nel, L[l].mg_map, parts.O.ptr(parts.scratch), L[l].mgc)
    r2 = parts.cycles_from(2, 2)[1]
    parts.prolong_state(1)
    r1 = parts.cycles_from(1, 3)[1]
    parts.prolong_state(0)
    assert rc == 0 and np.array_equal(_bits(hist), _bits(np.concatenate([r2, r1]))) and len(hist) == 5
    assert all(np.array_equal(_bits(em.variables(l)), _bits(parts.variables(l))) for l in range(3))
    em.close()
    parts.close()


def test_every_gpu_run_stays_valid(oracle, lattices):
    """What tests/test_gpu_cycle.py runs against this emulator returns code 0 here: (V, W, F) x post[0] in {0, 1} x {reference
    transfers, FAS}, six cycles each, on all five cases, the FMG starts, the composed runs, the global step on the lattices and
    the run at eight sweeps per level."""
    for case in ce.GPU_GOLDENS + ce.GPU_LATTICES:
        where = lattices.get(case, case)
        for fas in (False, True):
            mode, cfl = ("local", 1.0) if (fas and case in lattices) else ("reference", 0.5)
            for shape in ce.SHAPES:
                for post0 in ce.GPU_POST0:
                    em, rc, rms = _shaped(oracle, where, shape, fas, ce.VALID_CYCLES, post0, mode, cfl)
                    assert rc == 0 and np.isfinite(rms).all() and len(rms) == ce.VALID_CYCLES, (case, fas, shape, post0)
                    em.close()
    for case in ("A", "C", "m6_3lvl"):
        for fas in (False, True):
            em = ce.CycleOracle(oracle, lattices.get(case, case), fas=fas)
            rc, rms = em.full_multigrid([0] + [2] * (em.n - 1))
            assert rc == 0 and np.isfinite(rms).all() and len(rms) == 2 * (em.n - 1), (case, fas)
            em.close()
    for dual in (False, True):
        em, rc, rms, _ = ce.composed_run(oracle, lattices["A"], dual)
        assert rc == 0 and np.isfinite(rms).all(), dual
        em.close()
    for case in ce.GPU_LATTICES:                          # the reference's transfers under a global step on the lattices
        for shape, pre, post in ce.gpu_configurations(len(ce.LATTICES[case])):
            em = ce.CycleOracle(oracle, lattices[case], *ce.GPU_GLOBAL_STEP)
            em.set_cycle(shape, pre, post)
            assert em.cycles(ce.VALID_CYCLES)[0] == 0, (case, shape, pre, post)
            em.close()
    em = ce.CycleOracle(oracle, ce.SMALLEST_CASE, fas=True)
    em.set_cycle("W", [ce.MAX_SWEEPS] * em.n, [ce.MAX_SWEEPS] * em.n)
    assert em.cycles(1)[0] == 0
    em.close()
