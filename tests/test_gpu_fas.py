"""GPU tests of FAS multigrid (mgcfd_set_fas) on one solver and in the drop-in binary, against the numpy emulator
(tests/fas_emulator.py) bit for bit: state, forcing P, start state W0 and RMS history on the two generated lattices and three golden
cases; the same bits on every path; composition with residual smoothing, JST and dual time; a forced stage from read-back arrays;
switching; refusals; the fast mode; the driver's flag; convergence on the device.  tests/test_host_fas.py asserts on the CPU that
every combination stays valid and that the emulator meets the convergence bounds."""
import os
import subprocess

import numpy as np
import pytest

import fas_emulator as fe
import free_stream_emulator as fse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
K = fe.GPU_CYCLES
REL_RUN = 1e-10          # tests/test_gpu_jst.py::test_fast_mode: level `variables` after whole cycles, max |difference| / max |value|
RMS_FAST = 1e-9          # ... and its RMS tolerance


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(np.asarray(got) - np.asarray(want)).max():.3e}"


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("fas_lattices")
    return {name: fe.write_lattice(name, d) for name in fe.LATTICES}


def _case(name, lattices):
    return lattices.get(name, name)


def _solver(case, graph=0, exact=1, stage_wg4=1, fuse=1):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    for name, v in (("graph", graph), ("exact", exact), ("stage_wg4", stage_wg4), ("fuse_update", fuse)):
        s.set_option(name, v)
    return mesh, s


_emulated = {}


def _emulate(oracle, lattices, name, mode, cfl, cycles=K):
    """(rms, variables per level, P per level, W0 per level) of `cycles` FAS cycles from the far field: computed once per
    combination, shared and left unchanged."""
    key = (name, mode, cfl, cycles)
    if key not in _emulated:
        em = fe.FasOracle(oracle, _case(name, lattices), mode, cfl, fas=True)
        rc, rms = em.cycles(cycles)
        assert rc == 0
        _emulated[key] = (rms, [em.variables(l) for l in range(em.n)], [None] + [em.P[l].copy() for l in range(1, em.n)],
                          [None] + [em.W0[l].copy() for l in range(1, em.n)])
        em.close()
    return _emulated[key]


def _compare(s, want, what, rms=None):
    want_rms, want_v, want_p, want_w0 = want
    if rms is not None:
        _same(rms, want_rms, f"{what}: RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), want_v[l], f"{what}: variables, level {l}")
        if l >= 1:
            _same(s.get(l, "fas_forcing"), want_p[l], f"{what}: P, level {l}")
            _same(s.get(l, "fas_start"), want_w0[l], f"{what}: W0, level {l}")
        assert not s.get(l, "fluxes").any(), f"{what}: fluxes after the run, level {l}"


COMBINATIONS = [(name, mode, cfl) for name in fe.LATTICES for mode, cfl in fe.GPU_LATTICE_STEPS] + [(c, "reference", 0.5) for c in fe.GPU_GOLDENS]


@pytest.mark.parametrize("name,mode,cfl", COMBINATIONS)
def test_state_forcing_and_rms_equal_the_emulator(name, mode, cfl, oracle, lattices):
    """After K cycles: `variables` of every level, P and W0 of every level >= 1 and the RMS history bitwise the emulator's.
    Every case has coarse nodes with more than four children (asserted: the gather's fifth-child loop runs)."""
    want = _emulate(oracle, lattices, name, mode, cfl)
    mesh, s = _solver(_case(name, lattices))
    parents = np.asarray(mesh.level(0)["mg_map"]).ravel()
    assert np.bincount(parents).max() > 4
    s.set_time_step(mode, cfl)
    assert not s.fas()
    s.set_fas()
    assert s.fas()
    rms = s.run_cycles(K)
    print(name, mode, cfl, "rms", rms, "want", want[0])
    _compare(s, want, f"{name} {mode} {cfl}", rms)
    assert s.pending_invalid_state()[0] == 0
    s.close(); mesh.close()


def _granular_sweep(s, l, with_smooth):
    if with_smooth:
        s.smooth(l, 1)
        return
    s.copy_old_variables(l)
    s.compute_step_factor(l)
    for j in range(3):
        s.compute_fluxes(l)
        s.time_step(l, j)
    s.residual(l)


def _granular_cycle(s, with_smooth):
    """One FAS cycle call by call: mgcfd_fas_restrict / mgcfd_fas_prolong around mgcfd_smooth, or around the kernel-granular sweep."""
    n = s.num_levels
    for l in range(n):
        _granular_sweep(s, l, with_smooth)
        if l + 1 < n:
            s.fas_restrict(l)
    for l in range(n - 2, -1, -1):
        s.fas_prolong(l)
        if l > 0:
            _granular_sweep(s, l, with_smooth)


@pytest.mark.parametrize("name,mode,cfl", [("A", "local", 1.0), ("A", "global", 1.0), ("m6_3lvl", "reference", 0.5), ("tet_2lvl", "reference", 0.5)])
def test_same_bits_on_every_path(name, mode, cfl, oracle, lattices):
    """run_cycles with graph = 1, fuse_update = 0 and stage_wg4 = 0, run_cycles one cycle at a time, and the cycle call by call
    (with mgcfd_smooth, and with compute_fluxes / time_step): all the emulator's bits."""
    want = _emulate(oracle, lattices, name, mode, cfl)
    case = _case(name, lattices)
    for graph, wg4, fuse in ((1, 1, 1), (0, 1, 0), (0, 0, 1), (1, 0, 0)):
        mesh, s = _solver(case, graph, stage_wg4=wg4, fuse=fuse)
        s.set_time_step(mode, cfl)
        s.set_fas()
        rms = s.run_cycles(K)
        _compare(s, want, f"{name} {mode} graph={graph} wg4={wg4} fuse={fuse}", rms)
        s.close(); mesh.close()
    mesh, s = _solver(case)
    s.set_time_step(mode, cfl)
    s.set_fas()
    rms = np.concatenate([s.run_cycles(1) for _ in range(K)])
    _compare(s, want, f"{name} {mode} one cycle per call", rms)
    s.close(); mesh.close()
    for with_smooth in (True, False):
        mesh, s = _solver(case)
        s.set_time_step(mode, cfl)
        s.set_fas()
        for _ in range(K):
            _granular_cycle(s, with_smooth)
        _compare(s, want, f"{name} {mode} call by call, smooth={with_smooth}")
        s.close(); mesh.close()


@pytest.mark.parametrize("name,mode,cfl,smoothing,jst_levels,order", fe.COMPOSED, ids=[c[0] for c in fe.COMPOSED])
def test_composition(name, mode, cfl, smoothing, jst_levels, order, oracle, lattices):
    """Residual smoothing, JST on level 0 and on all levels, dual time under BDF1 and BDF2, and all three together, on lattice A:
    bitwise the composed emulator, and valid."""
    import jst_emulator as jse
    case = lattices["A"]
    em, rc, want_rms, dt = fe.composed_run(oracle, case, mode, cfl, smoothing, jst_levels, order)
    assert rc == 0
    mesh, s = _solver(case)
    s.set_time_step(mode, cfl)
    if smoothing[1]:
        s.set_residual_smoothing(*smoothing)
    if jst_levels:
        s.set_jst(jse.KAPPA2, jse.KAPPA4, s.num_levels if jst_levels == "all" else jst_levels)
    s.set_fas()
    if order is None:
        rms = s.run_cycles(K)
    else:
        s.set_dual_time(dt)
        s.dual_time_order(order)
        rms = s.advance(fe.DUAL_STEPS, fe.DUAL_CYCLES).ravel()
    want = (want_rms, [em.variables(l) for l in range(em.n)], em.P, em.W0)
    _compare(s, want, name, rms)
    assert s.pending_invalid_state()[0] == 0
    if order is not None:
        for l in range(s.num_levels):
            _same(s.get(l, "time_n"), em.Wn[l], f"{name}: Wn, level {l}")
    em.close()
    s.close(); mesh.close()


def test_forced_stages_from_read_back_arrays(lattices):
    """mgcfd_time_step(1, j) after mgcfd_fas_restrict(0): variables = old + sf / (RK + 1 - j) * (F + P), every operand read back;
    the coarse fluxes read back zero afterwards."""
    for mode, cfl in (("local", 1.0), ("global", 1.0)):
        mesh, s = _solver(lattices["A"])
        s.set_time_step(mode, cfl)
        s.set_fas()
        s.smooth(0, 2)
        s.fas_restrict(0)
        P = s.get(1, "fas_forcing")
        assert P.any() and not s.get(1, "fluxes").any()
        _same(s.get(1, "fas_start"), s.get(1, "variables"), "W0 is the restricted state")
        s.copy_old_variables(1)
        s.compute_step_factor(1)
        old, sf = s.get(1, "old_variables"), s.get(1, "step_factors")
        for j in range(3):
            s.compute_fluxes(1)
            F = s.get(1, "fluxes")
            s.time_step(1, j)
            factor = sf / np.float64(3 + 1 - j)
            _same(s.get(1, "variables"), old + factor[:, None] * (F + P), f"{mode}: forced stage {j}")
            assert not s.get(1, "fluxes").any()
        _same(s.get(1, "fas_forcing"), P, "the stages leave P alone")
        s.close(); mesh.close()


def _golden(case):
    meta = dict(l.strip().split(" = ") for l in open(os.path.join(fse.GOLDEN, case, "case.txt")))
    return int(meta["cycles"]), open(os.path.join(fse.GOLDEN, case, "variables.level0.txt"), "rb").read()


@pytest.mark.parametrize("name", ["A", "m6_3lvl", "tet_2lvl"])
def test_switching(name, oracle, lattices):
    """Off -> on -> off between runs: the off runs are a never-switched solver's bits (for a golden case: the golden output), the on
    run the emulator's, and after switching off the library holds what it held before switching on."""
    import mgcfd
    case = _case(name, lattices)
    mode, cfl = "reference", 0.5
    if name != "A":
        cycles, golden = _golden(name)
        mesh, s = _solver(case)
        s.set_fas(True)
        s.set_fas(False)
        s.run_cycles(cycles)
        assert fse.render_variables(s.get(0, "variables")).encode() == golden
        s.close(); mesh.close()
    mesh, s = _solver(case)
    s.set_time_step(mode, cfl)
    ref_mesh, ref = _solver(case)
    ref.set_time_step(mode, cfl)
    rms, rms_ref = s.run_cycles(K), ref.run_cycles(K)
    _same(rms, rms_ref, "off, leg 0: RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), ref.get(l, "variables"), f"off, leg 0: level {l}")
    em = fe.FasOracle(oracle, case, mode, cfl)
    assert em.cycles(K)[0] == 0
    before = mgcfd.live_device_resources()
    state = [s.get(l, "variables") for l in range(s.num_levels)]
    s.set_fas(True)
    em.set_fas(True)
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), state[l], "the setter keeps the state")
    rc, want_rms = em.cycles(K)
    assert rc == 0
    _compare(s, (want_rms, [em.variables(l) for l in range(em.n)], em.P, em.W0), f"{name}: on", s.run_cycles(K))
    s.set_fas(False)
    after = mgcfd.live_device_resources()
    assert (after["allocations"], after["bytes"]) == (before["allocations"], before["bytes"])
    for l in range(s.num_levels):
        ref.set(l, "variables", s.get(l, "variables"))
    rms, rms_ref = s.run_cycles(K), ref.run_cycles(K)
    _same(rms, rms_ref, "off, leg 2: RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), ref.get(l, "variables"), f"off, leg 2: level {l}")
    with pytest.raises(mgcfd.MgcfdError):
        s.get(1, "fas_forcing")
    em.close()
    s.close(); ref.close()
    mesh.close(); ref_mesh.close()


def test_refusals(lattices):
    """A one-level solver, mid-sweep, a partitioned solver, a group member; while on: the sweep_* calls, group creation and rank
    attachment; the legs while off; writes to P and W0: error code 1, "FAS" in the message, nothing changed."""
    import mgcfd
    mesh1, one = _solver("fvcorr_1lvl")
    with pytest.raises(mgcfd.MgcfdError) as e:
        one.set_fas()
    assert e.value.code == 1 and "FAS" in str(e.value) and not one.fas()
    one.set_fas(False)
    one.close(); mesh1.close()
    mesh, s = _solver("m6_2lvl")
    ref_mesh, ref = _solver("m6_2lvl")
    for call in (lambda: s.fas_restrict(0), lambda: s.fas_prolong(0), lambda: s.get(1, "fas_forcing"), lambda: s.get(1, "fas_start")):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1 and "FAS" in str(e.value)
    for t in (s, ref):
        t.set_fas()
    for call in (lambda: s.sweep_begin(0), lambda: s.sweep_begin_partials(0), lambda: s.sweep_flux0(0), lambda: s.sweep_stage(0, 0),
                 lambda: s.sweep_end(0), lambda: s.sweep_end_partials(0), lambda: s.sweep_begin(1), lambda: mgcfd.Group([s]),
                 lambda: s.rank_attach_plain(0, 1), lambda: s.set(1, "fas_forcing", np.zeros((s.nel(1), 5))),
                 lambda: s.set(1, "fas_start", np.zeros((s.nel(1), 5))), lambda: s.get(0, "fas_forcing")):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1 and "FAS" in str(e.value)
    assert s.fas()
    s.set_option("graph", 1)                                  # accepted: the launches run directly
    rms, rms_ref = s.run_cycles(2), ref.run_cycles(2)
    _same(rms, rms_ref, "cycles after the refused calls: RMS history")
    for l in range(2):
        _same(s.get(l, "variables"), ref.get(l, "variables"), f"cycles after the refused calls: level {l}")
        _same(s.get(1, "fas_forcing"), ref.get(1, "fas_forcing"), "cycles after the refused calls: P")
    # mid-sweep: the split sweep runs with FAS off; the setter is refused until its last stage has run
    for t in (s, ref):
        t.set_fas(False)
    s.sweep_begin(0)
    s.sweep_stage(0, 0, partials=False)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_fas()
    assert e.value.code == 1 and "FAS" in str(e.value) and "sweep is under way" in str(e.value) and not s.fas()
    s.sweep_stage(0, 1, partials=False)
    s.sweep_stage(0, 2, partials=False)
    ref.smooth(0, 1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "the sweep the refused call interrupted")
    # a group member, and a partitioned solver
    g = mgcfd.Group([s])
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_fas()
    assert e.value.code == 1 and "FAS" in str(e.value) and not s.fas()
    s.set_fas(False)                                          # switching off is always allowed
    g.close()
    s.close(); ref.close()
    mesh.close(); ref_mesh.close()
    from mgcfd.partition import partition_hierarchy, rcb_partition
    mesh = mgcfd.Mesh("input.dat", fse.case_input("m6_2lvl"), 1)
    levels = [mesh.level(l) for l in range(mesh.num_levels)]
    H = partition_hierarchy(levels, rcb_partition(np.asarray(levels[0]["coords"]).reshape(-1, 3), 2))
    lv, owned, keys = H[0].solver_args()
    t = mgcfd.Solver.from_arrays(lv, mesh.variant, n_owned=owned, order_keys=keys)
    with pytest.raises(mgcfd.MgcfdError) as e:
        t.set_fas()
    assert e.value.code == 1 and "FAS" in str(e.value) and not t.fas()
    t.close()
    mesh.close()


@pytest.mark.parametrize("name,mode,cfl", [("A", "local", 1.0), ("m6_3lvl", "reference", 0.5)])
def test_fast_mode(name, mode, cfl, oracle, lattices):
    """exact = 0 (FMA contraction, the order-free flux kernel for F) within the bounds tests/test_gpu_jst.py::test_fast_mode uses:
    1e-10 of the largest value per level, RMS rtol 1e-9."""
    want_rms, want_v, _, _ = _emulate(oracle, lattices, name, mode, cfl)
    mesh, s = _solver(_case(name, lattices), exact=0)
    s.set_time_step(mode, cfl)
    s.set_fas()
    rms = s.run_cycles(K)
    assert np.allclose(rms, want_rms, rtol=RMS_FAST, atol=0)
    for l in range(s.num_levels):
        rel = np.abs(s.get(l, "variables") - want_v[l]).max() / max(np.abs(want_v[l]).max(), 1e-300)
        print(name, mode, cfl, "level", l, "rel", rel)
        assert rel <= REL_RUN, f"{name} level {l}: {rel:.3e}"
    s.close(); mesh.close()


def test_loop_counts_and_bench_hook(lattices):
    """LoopNumIters: restrict, prolong, compute_step and time_step count as in the run without FAS; flux counts the two extra
    residual evaluations per level pair and cycle.  mgcfd_bench_fas times every kind of launch and leaves a state the next run
    can start from again."""
    import mgcfd
    mesh, plain = _solver(lattices["A"])
    plain.set_time_step("local", 1.0)
    plain.run_cycles(K)
    mesh_s, s = _solver(lattices["A"])
    s.set_time_step("local", 1.0)
    with pytest.raises(mgcfd.MgcfdError):
        s.bench_fas(0, "restrict_fas", 2)                     # (off)
    s.set_fas()
    s.run_cycles(K)
    n = s.num_levels
    extra = [0] * n
    for l in range(n - 1):
        extra[l] += K * s.num_internal_edges(l)
        extra[l + 1] += K * s.num_internal_edges(l + 1)
    for l in range(n):
        got, want = s.loop_iters(l), plain.loop_iters(l)
        assert got["flux"] == want["flux"] + extra[l], (l, got, want)
        for loop in ("restrict", "prolong", "compute_step", "time_step", "update", "indirect_rw"):
            assert got[loop] == want[loop], (l, loop, got, want)
    for fine in range(n - 1):
        for kind in mgcfd.Solver.FAS_LAUNCHES:
            assert s.bench_fas(fine, kind, 3) > 0.0, (fine, kind)
    s.set_free_stream(*s.free_stream(), reinitialise=True)
    assert not s.get(1, "fas_forcing").any()                  # (the forcing belonged to the state that has gone)
    mesh_r, ref = _solver(lattices["A"])
    ref.set_time_step("local", 1.0)
    ref.set_fas()
    _same(s.run_cycles(K), ref.run_cycles(K), "after the bench launches and a re-initialisation: RMS history")
    for l in range(n):
        _same(s.get(l, "variables"), ref.get(l, "variables"), f"after the bench launches and a re-initialisation: level {l}")
    for t, m in ((plain, mesh), (s, mesh_s), (ref, mesh_r)):
        t.close(); m.close()


def _run_driver(tmp, case, extra, cycles, ok=True):
    os.makedirs(tmp / "out", exist_ok=True)
    cmd = [EXE, "-i", "input.dat", "-d", fse.case_input(case), "-o", "out/", "-g", str(cycles), "-m", str(fse.case_duplicate(case))] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tmp)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


def test_driver(oracle, lattices, tmp_path):
    """--fas and the config key on m6_3lvl: the dump is the Python run's, byte for byte (and the emulator's), the RMS lines its
    history; without the flag the golden output; --fas --gpus 2 and a one-level input are refused with a message that says why."""
    case = "m6_3lvl"
    cycles, golden = _golden(case)
    dup = fse.case_duplicate(case)
    mesh, s = _solver(case)
    s.set_fas()
    rms = s.run_cycles(K)
    want = fse.render_variables(s.get(0, "variables")).encode()
    s.close(); mesh.close()
    assert want == fse.render_variables(_emulate(oracle, lattices, case, "reference", 0.5)[1][0]).encode()
    conf = tmp_path / "run.conf"
    conf.write_text("fas = Y\n")
    for tag, extra in (("flag", ["--fas"]), ("conf", ["-c", str(conf)])):
        r = _run_driver(tmp_path / tag, case, ["--output-variables"] + extra, K)
        assert (tmp_path / tag / "out" / f"variables.size={dup}x.cycles={K}.level=0").read_bytes() == want, tag
        assert [l for l in r.stdout.splitlines() if "(RMS = " in l] == [f"MG cycle {i + 1} / {K}" + " (RMS = %.3e)" % rms[i] for i in range(K)]
    _run_driver(tmp_path / "plain", case, ["--output-variables"], cycles)
    assert (tmp_path / "plain" / "out" / f"variables.size={dup}x.cycles={cycles}.level=0").read_bytes() == golden
    for extra in (["--fas", "--gpus", "2", "--gpus-share-device"], ["--fas", "--gpus", "2", "--gpus-partition", "--gpus-share-device"]):
        r = _run_driver(tmp_path / "two", case, ["--output-variables"] + extra, K, ok=False)
        assert "FAS" in r.stderr and "one GPU" in r.stderr
        assert not [n for n in os.listdir(tmp_path / "two" / "out") if n.startswith("variables")]
    r = _run_driver(tmp_path / "one", "fvcorr_1lvl", ["--output-variables", "--fas"], K, ok=False)
    assert "FAS" in r.stderr and "two levels" in r.stderr
    assert not [n for n in os.listdir(tmp_path / "one" / "out") if n.startswith("variables")]


def test_convergence_on_the_device(oracle, lattices):
    """Lattice A, local steps at CFL 1.0, 60 cycles: the final state and the RMS history are the emulator's bit for bit, so the
    bound tests/test_host_fas.py asserts on the emulator holds for the device."""
    want = _emulate(oracle, lattices, "A", "local", 1.0, fe.CONV_CYCLES)
    mesh, s = _solver(lattices["A"])
    s.set_time_step("local", 1.0)
    s.set_fas()
    rms = s.run_cycles(fe.CONV_CYCLES)
    _compare(s, want, "lattice A, 60 cycles", rms)
    s.close(); mesh.close()
