"""GPU tests of multigrid cycle control (mgcfd_set_cycle, mgcfd_run_cycles_from, mgcfd_prolong_state, mgcfd_full_multigrid) on one
solver and in the drop-in binary, against the numpy emulator (tests/cycle_emulator.py) bit for bit: state on every level, RMS
history (where an option fixes the order of its sum; to 1e-12 otherwise) and, under FAS, P and W0, for every shape with and without a level-0 post-sweep on three golden cases and two generated
lattices; the same bits with graphs asked for and with unfused stages; a composed run; the default configuration set explicitly;
cycles from every coarser level, the state interpolation and the full-multigrid start; the fast mode; refusals; the driver's
flags.  tests/test_host_cycle.py asserts on the CPU that every run here stays valid on the emulator."""
import os
import subprocess

import numpy as np
import pytest

import cycle_emulator as ce
import free_stream_emulator as fse
import viscous_emulator as ve

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
K = ce.GPU_CYCLES
REL_RUN = 1e-10          # tests/test_gpu_fas.py::test_fast_mode: level `variables` after whole cycles, max |difference| / max |value|
RMS_FAST = 1e-9          # ... and its RMS tolerance
RMS_FREE_ORDER = 1e-12   # tests/test_gpu_parity.py: the RMS of a cycle while no option fixes the order of its sum


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(np.asarray(got) - np.asarray(want)).max():.3e}"


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("cycle_lattices")
    return {name: ce.write_lattice(name, d) for name in ce.GPU_LATTICES}


def _solver(case, graph=0, exact=1, stage_wg4=1, fuse=1):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    for name, v in (("graph", graph), ("exact", exact), ("stage_wg4", stage_wg4), ("fuse_update", fuse)):
        s.set_option(name, v)
    return mesh, s


def _compare(s, em, what, rms=None, want_rms=None, ordered=None):
    """State (and P, W0) bit for bit.  The RMS history bit for bit where its sum has a fixed order — FAS, JST or the viscous
    terms on level 0, dual time (mgcfd_solver's ordered_rms), or a cycle from a coarser level (``ordered=True``) — and otherwise,
    where the definition leaves the order of the sum free, within tests/test_gpu_parity.py's rtol for it."""
    if rms is not None:
        if ordered if ordered is not None else (em.fas or em.dt != 0.0 or em.visc_levels > 0 or em.jst_levels > 0):
            _same(rms, want_rms, f"{what}: RMS history")
        else:
            assert len(rms) == len(want_rms) and np.allclose(rms, want_rms, rtol=RMS_FREE_ORDER, atol=0), f"{what}: RMS history {rms} {want_rms}"
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), em.variables(l), f"{what}: variables, level {l}")
        if em.fas and l >= 1:
            _same(s.get(l, "fas_forcing"), em.P[l], f"{what}: P, level {l}")
            _same(s.get(l, "fas_start"), em.W0[l], f"{what}: W0, level {l}")


# (case, FAS, mode, cfl): the goldens under the reference's step (a global one: their meshes are not fvcorr), the lattices under
# the reference's (a local one) and a global step with the reference's transfers, and under all three of GPU_STEPS with FAS
RUNS = [(c, fas, "reference", 0.5) for c in ce.GPU_GOLDENS for fas in (False, True)]
RUNS += [(c, False) + step for c in ce.GPU_LATTICES for step in (("reference", 0.5), ce.GPU_GLOBAL_STEP)]
RUNS += [(c, True) + step for c in ce.GPU_LATTICES for step in ce.GPU_STEPS]


@pytest.mark.parametrize("case,fas,mode,cfl", RUNS)
def test_shaped_cycles_equal_the_emulator(case, fas, mode, cfl, oracle, lattices):
    """(V, W, F) x post[0] in {0, 1}, and W with pre = (2, 1, ...): after K cycles `variables` of every level, the RMS history and,
    under FAS, P and W0 are the emulator's bits.  The first configuration is the default one set explicitly."""
    where = lattices.get(case, case)
    for shape, pre, post in ce.gpu_configurations(ce.NUM_LEVELS[case]):
        em = ce.CycleOracle(oracle, where, mode, cfl, fas=fas)
        em.set_cycle(shape, pre, post)
        rc, want_rms = em.cycles(K)
        assert rc == 0
        mesh, s = _solver(where)
        s.set_time_step(mode, cfl)
        if fas:
            s.set_fas()
        s.set_cycle(shape, pre, post)
        assert s.get_cycle() == em.get_cycle()
        rms = s.run_cycles(K)
        print(case, fas, mode, cfl, shape, pre, post, "rms", rms)
        _compare(s, em, f"{case} fas={fas} {mode} {shape} pre={pre} post={post}", rms, want_rms)
        assert s.pending_invalid_state()[0] == 0
        em.close()
        s.close(); mesh.close()


@pytest.mark.parametrize("case,fas,mode,cfl", [("m6_3lvl", False, "reference", 0.5), ("C", False, "global", 0.5), ("C", True, "global", 1.0),
                                               ("A", True, "local", 1.0)])
def test_same_bits_on_every_path(case, fas, mode, cfl, oracle, lattices):
    """W with a level-0 post-sweep with MGCFD_OPT_GRAPH = 1 (accepted, the launches run directly), unfused stages, three
    workgroups per CU, one cycle per call, and after a run of default cycles on the same solver (whose look-ahead and captured
    graphs must not leak into the shaped cycle): the emulator's bits."""
    where = lattices.get(case, case)
    em = ce.CycleOracle(oracle, where, mode, cfl, fas=fas)
    pre, post = ce.default_sweeps(em.n)
    post[0] = 1
    em.set_cycle("W", pre, post)
    rc, want_rms = em.cycles(K)
    assert rc == 0
    for graph, wg4, fuse in ((1, 1, 1), (0, 1, 0), (0, 0, 1), (1, 0, 0)):
        mesh, s = _solver(where, graph, stage_wg4=wg4, fuse=fuse)
        s.set_time_step(mode, cfl)
        if fas:
            s.set_fas()
        s.set_cycle("W", pre, post)
        _compare(s, em, f"{case} graph={graph} wg4={wg4} fuse={fuse}", s.run_cycles(K), want_rms)
        s.close(); mesh.close()
    mesh, s = _solver(where)
    s.set_time_step(mode, cfl)
    if fas:
        s.set_fas()
    s.set_cycle("W", pre, post)
    _compare(s, em, f"{case} one cycle per call", np.concatenate([s.run_cycles(1) for _ in range(K)]), want_rms)
    s.close(); mesh.close()
    # default cycles first (graph = 1: captured where the options allow), then the shaped ones, then default ones again
    em2 = ce.CycleOracle(oracle, where, mode, cfl, fas=fas)
    mesh, s = _solver(where, graph=1)
    s.set_time_step(mode, cfl)
    if fas:
        s.set_fas()
    for shape, q in (("V", None), ("W", post), ("V", None)):
        em2.set_cycle(shape, None, q)
        s.set_cycle(shape, None, q)
        rc, want = em2.cycles(2)
        assert rc == 0
        _compare(s, em2, f"{case} {shape} in a row", s.run_cycles(2), want)
    em.close(); em2.close()
    s.close(); mesh.close()


@pytest.mark.parametrize("dual", [False, True], ids=["steady", "advance_bdf2"])
def test_composition(dual, oracle, lattices):
    """Lattice A: FAS + residual smoothing + JST + the viscous terms with no-slip walls on all levels under W with post[0] = 1,
    and the same inside mgcfd_advance with BDF2: the composed emulator's bits."""
    case = lattices["A"]
    em, rc, want_rms, dt = ce.composed_run(oracle, case, dual)
    assert rc == 0
    mesh, s = _solver(case)
    s.set_time_step(ce.COMPOSED_MODE, ce.COMPOSED_CFL)
    s.set_residual_smoothing(*ce.COMPOSED_SMOOTHING)
    s.set_jst(levels=ce.COMPOSED_JST_LEVELS)
    s.set_fas()
    s.set(0, "variables", ve.start_state(s.nel(0), s.far_field()[:5]))
    s.set_viscous(ve.CELL_RE_MU, ve.PRANDTL, True, ve.VISCOUS_CFL, s.num_levels)
    s.set_cycle(*em.get_cycle())
    if dual:
        s.set_dual_time(dt)
        s.dual_time_order(2)
        rms = s.advance(ce.COMPOSED_STEPS, ce.COMPOSED_STEP_CYCLES).ravel()
    else:
        rms = s.run_cycles(ce.COMPOSED_CYCLES)
    _compare(s, em, f"composed, dual={dual}", rms, want_rms)
    if dual:
        for l in range(s.num_levels):
            _same(s.get(l, "time_n"), em.Wn[l], f"composed: Wn, level {l}")
    assert s.pending_invalid_state()[0] == 0
    em.close()
    s.close(); mesh.close()


@pytest.mark.parametrize("case", ["m6_3lvl", "C"])
@pytest.mark.parametrize("graph", [0, 1])
def test_default_set_explicitly_is_a_solver_never_configured(case, graph, lattices):
    """State, RMS history, LoopNumIters and the library's live device resources."""
    import mgcfd
    where = lattices.get(case, case)
    mesh_r, ref = _solver(where, graph)
    mesh, s = _solver(where, graph)
    before = mgcfd.live_device_resources()
    s.set_cycle("V", *ce.default_sweeps(s.num_levels))
    s.set_cycle()
    s.set_cycle("W", None, None)
    s.set_cycle("V", None, [0] + [1] * (s.num_levels - 2) + [5])          # (post[n-1] is ignored)
    after = mgcfd.live_device_resources()
    assert (after["allocations"], after["bytes"]) == (before["allocations"], before["bytes"])
    assert s.get_cycle() == ("V",) + tuple(ce.default_sweeps(s.num_levels)) == ref.get_cycle()
    _same(s.run_cycles(K), ref.run_cycles(K), "RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), ref.get(l, "variables"), f"level {l}")
        assert s.loop_iters(l) == ref.loop_iters(l), l
    s.close(); mesh.close()
    ref.close(); mesh_r.close()


def _state_run_setup(oracle, where, fas, viscous):
    mode, cfl = ("local", 1.0) if fas else ("reference", 0.5)
    em = ce.CycleOracle(oracle, where, mode, cfl, fas=fas)
    mesh, s = _solver(where)
    s.set_time_step(mode, cfl)
    if fas:
        s.set_fas()
    if viscous:
        em.set_viscous(ve.GPU_MU["A"], ve.PRANDTL, 1, ve.VISCOUS_CFL, "all")
        s.set_viscous(ve.GPU_MU["A"], ve.PRANDTL, True, ve.VISCOUS_CFL, s.num_levels)
    return em, mesh, s


@pytest.mark.parametrize("case,fas,viscous", [("A", False, False), ("A", True, False), ("A", True, True), ("C", False, False), ("C", True, False),
                                              ("m6_3lvl", False, False), ("m6_3lvl", True, False)])
def test_cycles_from_prolong_state_and_full_multigrid(case, fas, viscous, oracle, lattices):
    """After two level-0 cycles: mgcfd_prolong_state onto every level (the fine level poisoned first: it is only written; both
    levels' residuals stay), mgcfd_run_cycles_from for every top level with its RMS history (the levels below untouched, P_top
    untouched under FAS), and on a fresh solver mgcfd_full_multigrid followed by level-0 cycles: the emulator's bits.  One run has
    no-slip walls on every level."""
    where = lattices.get(case, case)
    em, mesh, s = _state_run_setup(oracle, where, fas, viscous)
    n = em.n
    rc, want = em.cycles(2)
    assert rc == 0
    _compare(s, em, "two cycles", s.run_cycles(2), want)
    for top in range(n - 1, 0, -1):
        below = [s.get(l, "variables") for l in range(top)]
        p_top = s.get(top, "fas_forcing") if fas else None
        rc, want = em.cycles_from(top, 2)
        assert rc == 0
        rms = s.run_cycles_from(top, 2)
        print(case, fas, "from level", top, "rms", rms)
        _compare(s, em, f"{case}: cycles from level {top}", rms, want, ordered=True)
        for l in range(top):
            _same(s.get(l, "variables"), below[l], f"cycles from level {top}: level {l} is untouched")
        if fas:
            _same(s.get(top, "fas_forcing"), p_top, f"cycles from level {top}: P_top is untouched")
    _compare(s, em, "top = 0 is run_cycles", s.run_cycles_from(0, 1), em.cycles_from(0, 1)[1])
    for fine in range(n - 2, -1, -1):
        res = [s.get(l, "residuals") for l in (fine, fine + 1)]
        s.set(fine, "variables", np.full((s.nel(fine), 5), np.nan))
        em.prolong_state(fine)
        s.prolong_state(fine)
        _compare(s, em, f"{case}: state prolonged onto level {fine}")
        for k, l in enumerate((fine, fine + 1)):
            _same(s.get(l, "residuals"), res[k], f"prolong_state({fine}): residuals of level {l}")
    if viscous:
        assert all(len(em.wall_nodes[l]) and not s.get(l, "variables")[em.wall_nodes[l], 1:4].any() for l in range(n))
    rc, want = em.cycles(2)                                   # (the look-ahead the last launch left is taken, or was not left)
    assert rc == 0
    _compare(s, em, "cycles after the state prolongation", s.run_cycles(2), want)
    em.close()
    s.close(); mesh.close()
    em, mesh, s = _state_run_setup(oracle, where, fas, viscous)
    cycles = [0] + [3, 2, 2][:n - 1]
    it0 = [s.loop_iters(l)["prolong"] for l in range(n)]
    rc, want = em.full_multigrid(cycles)
    assert rc == 0
    rms = s.full_multigrid(cycles)
    assert len(rms) == sum(cycles)
    _compare(s, em, f"{case}: full multigrid", rms, want, ordered=True)
    assert all(s.loop_iters(l)["prolong"] > it0[l] for l in range(n - 1))         # (counted as MGCFD_LOOP_PROLONG)
    rc, want = em.cycles(2)
    assert rc == 0
    _compare(s, em, f"{case}: level-0 cycles after full multigrid", s.run_cycles(2), want)
    em.close()
    s.close(); mesh.close()


def test_global_step_after_state_prolongation(oracle, lattices):
    """Under MGCFD_DT_GLOBAL a fused sweep takes the step-factor minima the state prolongation left: full multigrid, W-cycles
    from every level, then level-0 cycles, with the reference's transfers and with FAS."""
    for fas in (False, True):
        em = ce.CycleOracle(oracle, lattices["C"], "global", 0.5, fas=fas)
        mesh, s = _solver(lattices["C"])
        s.set_time_step("global", 0.5)
        if fas:
            s.set_fas()
        pre, post = ce.default_sweeps(em.n)
        post[0] = 1
        em.set_cycle("W", pre, post)
        s.set_cycle("W", pre, post)
        rc, want = em.full_multigrid([0, 2, 2, 2])
        assert rc == 0
        _compare(s, em, f"global step, fas={fas}: full multigrid", s.full_multigrid([0, 2, 2, 2]), want, ordered=True)
        rc, want = em.cycles(3)
        assert rc == 0
        _compare(s, em, f"global step, fas={fas}: cycles after it", s.run_cycles(3), want)
        em.close()
        s.close(); mesh.close()


@pytest.mark.parametrize("case,fas,mode,cfl", [("A", True, "local", 1.0), ("m6_3lvl", False, "reference", 0.5)])
def test_fast_mode(case, fas, mode, cfl, oracle, lattices):
    """exact = 0, flux variant 1 (the deterministic one) within the bounds tests/test_gpu_fas.py::test_fast_mode uses: 1e-10 of the
    largest value per level, RMS rtol 1e-9; full multigrid, then W-cycles with a level-0 post-sweep."""
    where = lattices.get(case, case)
    em = ce.CycleOracle(oracle, where, mode, cfl, fas=fas)
    mesh, s = _solver(where, exact=0)
    s.set_option("flux_variant", 1)
    s.set_time_step(mode, cfl)
    if fas:
        s.set_fas()
    pre, post = ce.default_sweeps(em.n)
    post[0] = 1
    em.set_cycle("W", pre, post)
    s.set_cycle("W", pre, post)
    rc, want_fmg = em.full_multigrid([0, 2, 2])
    rc2, want_rms = em.cycles(K)
    assert rc == 0 and rc2 == 0
    assert np.allclose(s.full_multigrid([0, 2, 2]), want_fmg, rtol=RMS_FAST, atol=0)
    assert np.allclose(s.run_cycles(K), want_rms, rtol=RMS_FAST, atol=0)
    for l in range(s.num_levels):
        want = em.variables(l)
        rel = np.abs(s.get(l, "variables") - want).max() / max(np.abs(want).max(), 1e-300)
        print(case, "level", l, "rel", rel)
        assert rel <= REL_RUN, f"{case} level {l}: {rel:.3e}"
    em.close()
    s.close(); mesh.close()


def test_refusals(lattices):
    """Every MGCFD_ERR_ARG case: error code 1, the configuration and the state unchanged afterwards; group creation and rank
    attachment refuse a solver with a non-default cycle."""
    import mgcfd
    mesh, s = _solver("m6_3lvl")
    ref_mesh, ref = _solver("m6_3lvl")
    s.set_cycle("W", [1, 2, 1], [1, 1, 0])
    held = s.get_cycle()
    assert held == ("W", [1, 2, 1], [1, 1, 1])
    bad = (lambda: s.set_cycle(3), lambda: s.set_cycle(-1), lambda: s.set_cycle("V", [1, 0, 1]), lambda: s.set_cycle("V", [1, 9, 1]),
           lambda: s.set_cycle("V", None, [0, -1, 1]), lambda: s.set_cycle("V", None, [9, 1, 1]),
           lambda: s.run_cycles_from(3, 1), lambda: s.run_cycles_from(-1, 1), lambda: s.run_cycles_from(1, 4097),
           lambda: s.prolong_state(2), lambda: s.prolong_state(-1), lambda: s.full_multigrid([0, 1, -1]), lambda: s.full_multigrid([0, 4097, 1]),
           lambda: mgcfd.Group([s]), lambda: s.rank_attach_plain(0, 1), lambda: s.rank_attach_rccl(0, 1, bytes(128)))
    s.run_cycles(1)
    ref.set_cycle(*held)
    ref.run_cycles(1)
    state = [s.get(l, "variables") for l in range(3)]
    for k, call in enumerate(bad):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1, k
        assert s.get_cycle() == held, k
        for l in range(3):
            _same(s.get(l, "variables"), state[l], f"refused call {k}: level {l}")
    for t in (s, ref):
        t.set_cycle("W", [1, 2, 1], [1, 1, 0])
    _same(s.run_cycles(2), ref.run_cycles(2), "cycles after the refused calls: RMS history")
    for l in range(3):
        _same(s.get(l, "variables"), ref.get(l, "variables"), f"cycles after the refused calls: level {l}")
    # dual time: no coarser start level, so no full multigrid either
    s.set_dual_time(0.1)
    state = [s.get(l, "variables") for l in range(3)]
    for call in (lambda: s.run_cycles_from(1, 1), lambda: s.full_multigrid([0, 1, 1])):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1
        for l in range(3):
            _same(s.get(l, "variables"), state[l], f"refused under dual time: level {l}")
    s.set_dual_time(0.0)
    # mid-sweep: the setter is refused until the sweep's last stage has run
    for t in (s, ref):
        t.set_cycle()
    s.sweep_begin(0)
    s.sweep_stage(0, 0, partials=False)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_cycle("W")
    assert e.value.code == 1 and "sweep is under way" in str(e.value) and s.get_cycle()[0] == "V"
    s.sweep_stage(0, 1, partials=False)
    s.sweep_stage(0, 2, partials=False)
    ref.smooth(0, 1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "the sweep the refused call interrupted")
    # a group member: only the default cycle; the other calls are refused
    g = mgcfd.Group([s])
    for call in (lambda: s.set_cycle("W"), lambda: s.set_cycle("V", None, [1, 1, 1]), lambda: s.run_cycles_from(1, 1), lambda: s.prolong_state(0)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1
    s.set_cycle()                                             # the default one is always allowed
    g.close()
    s.close(); ref.close()
    mesh.close(); ref_mesh.close()
    from mgcfd.partition import partition_hierarchy, rcb_partition
    mesh = mgcfd.Mesh("input.dat", fse.case_input("m6_2lvl"), 1)
    levels = [mesh.level(l) for l in range(mesh.num_levels)]
    H = partition_hierarchy(levels, rcb_partition(np.asarray(levels[0]["coords"]).reshape(-1, 3), 2))
    lv, owned, keys = H[0].solver_args()
    t = mgcfd.Solver.from_arrays(lv, mesh.variant, n_owned=owned, order_keys=keys)
    for call in (lambda: t.set_cycle("V", None, [1, 1]), lambda: t.run_cycles_from(1, 1), lambda: t.prolong_state(0)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1
    t.set_cycle()
    assert t.get_cycle() == ("V", [1, 1], [0, 1])
    t.close()
    mesh.close()


def test_loads_follow_the_post_sweeps_and_loop_counts(oracle):
    """mgcfd_run_cycles_loads under W with post[0] = 1 on m6_3lvl: every cycle's row is mgcfd_surface_loads of the state that
    cycle leaves, behind its level-0 post-sweep.  LoopNumIters of the shaped cycle against the default one's: with three levels W
    with the post-sweep runs level 0 twice per cycle (1 in V), level 1 four times (2), level 2 twice (1), restricts onto level 1
    once (once) and onto level 2 twice (once), prolongs onto level 0 once (once) and onto level 1 twice (once)."""
    case = "m6_3lvl"
    em = ce.CycleOracle(oracle, case)
    em.set_cycle("W", [1, 1, 1], [1, 1, 1])
    mesh, s = _solver(case)
    s.set_cycle("W", [1, 1, 1], [1, 1, 1])
    for c in range(2):
        rc, want = em.cycles(1)
        assert rc == 0
        rms, loads = s.run_cycles(1, loads=True)
        _compare(s, em, f"cycle {c} with loads", rms, want)
        assert loads.shape == (1, 6) and loads.any()
        _same(loads[0], s.surface_loads(0), f"cycle {c}: the loads row is the final state's")
    s.reset_monitoring()
    s.run_cycles(K)
    mesh_v, v = _solver(case)
    v.run_cycles(K)
    sweeps, down, up = (2, 2, 2), (None, 1, 2), (1, 2, None)
    for l in range(3):
        got, base = s.loop_iters(l), v.loop_iters(l)
        for loop in ("flux", "compute_step", "time_step"):
            assert got[loop] == sweeps[l] * base[loop] > 0, (l, loop, got, base)
        if down[l]:
            assert got["restrict"] == down[l] * base["restrict"] > 0, (l, got, base)
        if up[l]:
            assert got["prolong"] == up[l] * base["prolong"] > 0, (l, got, base)
    em.close()
    s.close(); mesh.close()
    v.close(); mesh_v.close()


def test_eight_sweeps_per_level(oracle):
    """pre and post at MGCFD_MAX_CYCLE_SWEEPS on the smallest case, one W-cycle under FAS."""
    em = ce.CycleOracle(oracle, ce.SMALLEST_CASE, fas=True)
    em.set_cycle("W", [ce.MAX_SWEEPS] * em.n, [ce.MAX_SWEEPS] * em.n)
    rc, want = em.cycles(1)
    assert rc == 0
    mesh, s = _solver(ce.SMALLEST_CASE)
    s.set_fas()
    s.set_cycle("W", [ce.MAX_SWEEPS] * em.n, [ce.MAX_SWEEPS] * em.n)
    _compare(s, em, "eight sweeps per level", s.run_cycles(1), want)
    em.close()
    s.close(); mesh.close()


def _run_driver(tmp, case, extra, cycles, ok=True):
    os.makedirs(tmp / "out", exist_ok=True)
    cmd = [EXE, "-i", "input.dat", "-d", fse.case_input(case), "-o", "out/", "-g", str(cycles), "-m", str(fse.case_duplicate(case))] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tmp)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


def test_driver(oracle, tmp_path):
    """--cycle, --pre-sweeps, --post-sweeps and --fmg-cycles on m6_3lvl against the emulator's dump, byte for byte, and its RMS
    lines; without the flags the golden output; with --gpus 2 the flags are refused."""
    case = "m6_3lvl"
    meta = dict(l.strip().split(" = ") for l in open(os.path.join(fse.GOLDEN, case, "case.txt")))
    golden = open(os.path.join(fse.GOLDEN, case, "variables.level0.txt"), "rb").read()
    dup = fse.case_duplicate(case)
    runs = ((["--cycle", "W", "--post-sweeps", "1"], False, "W", [1, 1, 1], [1, 1, 1], None),
            (["--cycle=F", "--pre-sweeps", "2,1,1", "--post-sweeps", "0,2,1", "--fas"], True, "F", [2, 1, 1], [0, 2, 1], None),
            (["--cycle", "W", "--post-sweeps", "1", "--fmg-cycles", "3", "--fas"], True, "W", [1, 1, 1], [1, 1, 1], [0, 3, 3]),
            (["--fmg-cycles", "2,4"], False, "V", [1, 1, 1], [0, 1, 1], [0, 2, 4]))
    for k, (flags, fas, shape, pre, post, fmg) in enumerate(runs):
        em = ce.CycleOracle(oracle, case, fas=fas)
        em.set_cycle(shape, pre, post)
        if fmg:
            assert em.full_multigrid(fmg)[0] == 0
        rc, rms = em.cycles(K)
        assert rc == 0
        r = _run_driver(tmp_path / str(k), case, ["--output-variables"] + flags, K)
        got = (tmp_path / str(k) / "out" / f"variables.size={dup}x.cycles={K}.level=0").read_bytes()
        assert got == fse.render_variables(em.variables(0)).encode(), flags
        assert [l for l in r.stdout.splitlines() if "(RMS = " in l] == [f"MG cycle {i + 1} / {K}" + " (RMS = %.3e)" % rms[i] for i in range(K)]
        em.close()
    cycles = int(meta["cycles"])
    _run_driver(tmp_path / "plain", case, ["--output-variables"], cycles)
    assert (tmp_path / "plain" / "out" / f"variables.size={dup}x.cycles={cycles}.level=0").read_bytes() == golden
    for flags in (["--cycle", "W"], ["--fmg-cycles", "2"], ["--post-sweeps", "1"]):
        r = _run_driver(tmp_path / "two", case, ["--output-variables", "--gpus", "2", "--gpus-share-device"] + flags, K, ok=False)
        assert "one GPU" in r.stderr
        assert not [n for n in os.listdir(tmp_path / "two" / "out") if n.startswith("variables")]
    for flags in (["--cycle", "X"], ["--pre-sweeps", "0"], ["--post-sweeps", "1,2"], ["--fmg-cycles", "1,2,3"]):
        _run_driver(tmp_path / "bad", case, flags, K, ok=False)
