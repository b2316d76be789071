"""Host tests of FAS multigrid (no GPU): the numpy emulator (tests/fas_emulator.py) converges where the reference's cycle goes
invalid and level-0 sweeps alone crawl, its fixed point is the fine grid's, with FAS off it is its parent bit for bit (the golden
output), coarse nodes without children get no forcing, and the new symbols are declared.  The measured histories are recorded in
profiles/fas_convergence.txt."""
import os

import numpy as np
import pytest

import fas_emulator as fe
import free_stream_emulator as fse
import jst_emulator as jse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("fas_lattices")
    return {name: fe.write_lattice(name, d) for name in fe.LATTICES}


def _metric_after(oracle, case, cfl, smoothing, fas, cycles, level0_only=False):
    """(rc, metric or None) after `cycles` FAS cycles / reference cycles / sweeps of level 0 alone under local steps."""
    em = fe.FasOracle(oracle, case, "local", cfl, *smoothing, fas=fas)
    rc = em.sweeps(0, cycles) if level0_only else em.cycles(cycles)[0]
    out = em.density_residual_rms() if rc == 0 else None
    em.close()
    return rc, out


def test_lattice_sizes(oracle, lattices):
    for name, sizes in (("A", [2178, 728, 215]), ("B", [728, 124])):
        em = fe.FasOracle(oracle, lattices[name])
        assert [em.oc.levels[l].nel for l in range(em.n)] == sizes and em.variant == 0
        em.close()


@pytest.mark.parametrize("cfl,smoothing", [(1.0, (0.0, 0)), (fe.CONV_SMOOTHING_CFL, fe.CONV_SMOOTHING)])
def test_convergence_on_lattice_a(cfl, smoothing, oracle, lattices):
    """60 FAS cycles reach at most 1/10 of what 60 sweeps of level 0 alone reach (the RMS of component 0 of F_0 / vol), plain at
    CFL 1.0 and with smoothing (0.5, 2) at CFL 2.0."""
    rc, fas = _metric_after(oracle, lattices["A"], cfl, smoothing, True, fe.CONV_CYCLES)
    rc0, alone = _metric_after(oracle, lattices["A"], cfl, smoothing, False, fe.CONV_CYCLES, level0_only=True)
    print("lattice A, local", cfl, smoothing, ": FAS", fas, "level 0 alone", alone, "ratio 1 /", alone / fas)
    assert rc == 0 and rc0 == 0
    assert fas <= fe.CONV_BOUND * alone


def test_the_reference_cycle_goes_invalid_on_lattice_a(oracle, lattices):
    rc, _ = _metric_after(oracle, lattices["A"], 1.0, (0.0, 0), False, fe.CONV_CYCLES)
    assert rc in (1, 2, 3)


def test_fixed_point_on_lattice_b(oracle, lattices):
    """After 200 FAS cycles the metric is <= 1e-8; one more cycle's coarse correction D is <= 1e-8 of max |W| on level 1: the
    cycle's fixed point is the fine grid's steady state."""
    em = fe.FasOracle(oracle, lattices["B"], "local", 1.0, fas=True)
    rc, _ = em.cycles(fe.FIXED_CYCLES)
    metric = em.density_residual_rms()
    rc1, _ = em.cycles(1)
    d, w = em.max_abs_D[1], float(np.abs(em.variables(1)).max())
    print("lattice B: metric", metric, "max |D|", d, "max |W|", w)
    assert rc == 0 and rc1 == 0
    assert metric <= fe.FIXED_BOUND
    assert d <= fe.FIXED_BOUND * w
    em.close()


@pytest.mark.parametrize("case", ["m6_3lvl", "tet_2lvl"])
def test_off_is_the_golden_output(case, oracle):
    """With FAS off — never on, and switched on and off again before the run — the golden variables.level0.txt byte for byte and
    JstOracle's RMS history bit for bit."""
    meta = dict(l.strip().split(" = ") for l in open(os.path.join(fse.GOLDEN, case, "case.txt")))
    golden = open(os.path.join(fse.GOLDEN, case, "variables.level0.txt"), "rb").read()
    want = jse.JstOracle(oracle, case)
    rc_w, rms_w = want.cycles(int(meta["cycles"]))
    want.close()
    for toggle in (False, True):
        em = fe.FasOracle(oracle, case)
        if toggle:
            em.set_fas(True)
            em.set_fas(False)
        rc, rms = em.cycles(int(meta["cycles"]))
        assert rc == rc_w == 0 and np.array_equal(_bits(rms), _bits(rms_w))
        assert fse.render_variables(em.variables(0)).encode() == golden
        em.close()


def test_childless_coarse_nodes(oracle):
    """tet_2lvl has 3 coarse nodes without children: P is +0.0 there and W0 holds the values they kept; everywhere else
    P = Q - R(W0) with Q the children's sum read literally."""
    em = fe.FasOracle(oracle, "tet_2lvl", fas=True)
    parent = np.asarray(em.oc.mg_map(0), dtype=np.int64)
    childless = np.flatnonzero(np.bincount(parent, minlength=em.oc.levels[1].nel) == 0)
    assert len(childless) == 3
    from conftest import perturbed_state
    em.oc.array(1, "variables")[:] = perturbed_state(em.oc.levels[1].nel, em.ff17[:5], seed=3).ravel()
    kept = em.variables(1)[childless]
    assert em._sweep(0) == 0
    T = em.total_residual(0)
    em.fas_restrict(0)
    assert np.array_equal(_bits(em.P[1][childless]), np.zeros((3, 5), dtype=np.int64))
    assert np.array_equal(_bits(em.W0[1][childless]), _bits(kept))
    assert np.array_equal(_bits(em.W0[1]), _bits(em.variables(1)))
    Q = np.zeros_like(em.P[1])
    for i in range(len(parent)):                      # ascending fine id, one addition per child, from +0.0
        Q[parent[i]] = Q[parent[i]] + T[i]
    R0 = em.total_residual(1)
    with_children = np.setdiff1d(np.arange(len(Q)), childless)
    assert np.array_equal(_bits(em.P[1][with_children]), _bits((Q - R0)[with_children]))
    assert em.P[1].any()
    em.close()


def test_every_gpu_combination_stays_valid(oracle, lattices):
    """What tests/test_gpu_fas.py runs against this emulator returns code 0 here, so none of its cases is skipped there."""
    for name in fe.LATTICES:
        for mode, cfl in fe.GPU_LATTICE_STEPS:
            em = fe.FasOracle(oracle, lattices[name], mode, cfl, fas=True)
            rc, rms = em.cycles(fe.GPU_CYCLES)
            assert rc == 0 and np.isfinite(rms).all() and all(em.P[l].any() for l in range(1, em.n)), (name, mode, cfl)
            em.close()
    for case in fe.GPU_GOLDENS:
        em = fe.FasOracle(oracle, case, fas=True)
        assert em.cycles(fe.GPU_CYCLES)[0] == 0, case
        em.close()
    for name, mode, cfl, smoothing, jst_levels, order in fe.COMPOSED:
        em, rc, rms, dt = fe.composed_run(oracle, lattices["A"], mode, cfl, smoothing, jst_levels, order)
        assert rc == 0 and np.isfinite(rms).all(), name
        if order == 2:
            assert em.effective_order() == 2
        em.close()


def test_symbols_and_array_ids():
    import mgcfd
    header = open(os.path.join(ROOT, "include", "mgcfd.h")).read()
    lib = mgcfd.load_library()
    for name in ("mgcfd_set_fas", "mgcfd_get_fas", "mgcfd_fas_restrict", "mgcfd_fas_prolong", "mgcfd_bench_fas"):
        assert name in mgcfd.EXPORTED_SYMBOLS and hasattr(lib, name) and f"int {name}(" in header
    import re
    from mgcfd import api
    enum = header[header.index("enum { MGCFD_ARR_VARIABLES"):]
    enum = re.sub(r"/\*.*?\*/", "", enum[:enum.index("};")], flags=re.S)
    ids = re.findall(r"MGCFD_ARR_[A-Z0-9_]+", enum)
    assert ids.index("MGCFD_ARR_FAS_FORCING") == api.ARR["fas_forcing"] and ids.index("MGCFD_ARR_FAS_START") == api.ARR["fas_start"]
