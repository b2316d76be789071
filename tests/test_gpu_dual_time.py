"""GPU tests of dual time stepping (mgcfd_set_dual_time, mgcfd_advance) on one solver: the state, the time levels and the RMS
history against the numpy emulator (tests/dual_time_emulator.py) on int64 views of the doubles; the same bits on every path;
convergence within a physical step; the free stream; switching; refusals; the fast mode.
tests/test_host_dual_time.py asserts on the CPU that every combination stays valid and that the clamp binds as stated."""
import os
import subprocess

import numpy as np
import pytest

import dual_time_emulator as dte
import free_stream_emulator as fse
from conftest import perturbed_state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")

STEPS, K = dte.GPU_STEPS, dte.GPU_CYCLES
REL_RUN = 1e-10          # tests/test_gpu_order_free.py: level `variables` after whole cycles, max |difference| / max |value|
RMS_FAST = 1e-9          # ... and its RMS tolerance
COMBOS = [(case,) + setting for case in dte.GPU_CASES for setting in dte.GPU_SETTINGS]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(np.asarray(got) - np.asarray(want)).max():.3e}"


def _solver(case, graph=0, exact=1, fuse=1):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    for name, v in (("graph", graph), ("exact", exact), ("fuse_update", fuse)):
        s.set_option(name, v)
    return mesh, s


def _configure(s, case, name, mode, cfl, smoothing, order):
    s.set_time_step(mode, cfl)
    s.set_residual_smoothing(*smoothing)
    s.set(0, "variables", dte.start_state(case, s.far_field()[:5], s.nel(0)))
    s.set_dual_time(dte.GPU_DT[case][name])
    s.dual_time_order(order)


_emulated = {}


def _emulate(oracle, case, name, mode, cfl, smoothing, order):
    """What STEPS x K leave behind: computed once per combination, shared and left unchanged."""
    key = (case, name)
    if key not in _emulated:
        em = dte.configured(oracle, case, name, mode, cfl, smoothing, order)
        rc, rms = em.advance(STEPS, K)
        assert rc == 0
        _emulated[key] = {"rms": rms, "v": [em.variables(l) for l in range(em.n)], "wn": [w.copy() for w in em.Wn],
                          "wn1": [w.copy() for w in em.Wn1], "bound": [tuple(b) for b in em.bound]}
        em.close()
    return _emulated[key]


def _check_state(s, want, what):
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), want["v"][l], f"{what}: variables, level {l}")
        _same(s.get(l, "time_n"), want["wn"][l], f"{what}: Wn, level {l}")
        _same(s.get(l, "time_n1"), want["wn1"][l], f"{what}: Wn1, level {l}")
        assert not s.get(l, "fluxes").any(), f"{what}: fluxes, level {l}"


@pytest.mark.parametrize("case,name,mode,cfl,smoothing,order", COMBOS)
def test_state_equals_the_emulator(case, name, mode, cfl, smoothing, order, oracle):
    """After 3 physical steps x 2 cycles (BDF1, then BDF2 twice; `bdf1`: BDF1 throughout): variables of every level, Wn and Wn1
    and the RMS history bitwise the emulator's; the clamp bound some nodes and left others alone (the emulator's step factors)."""
    want = _emulate(oracle, case, name, mode, cfl, smoothing, order)
    bound, free = sum(b[0] for b in want["bound"]), sum(b[1] for b in want["bound"])
    print(case, name, "clamp bound / free per level", want["bound"])
    assert bound > 0 and (free > 0 or dte.clamp_is_all_or_none(case, mode)), (case, name, want["bound"])
    mesh, s = _solver(case)
    _configure(s, case, name, mode, cfl, smoothing, order)
    rms = s.advance(STEPS, K).ravel()
    print(case, name, "rms", rms, "want", want["rms"])
    _check_state(s, want, f"{case} {name}")
    info = s.dual_time()
    assert info["dt"] == dte.GPU_DT[case][name] and info["clamp"] == dte.CLAMP and info["order"] == order and info["levels"] == 2
    _same(rms, want["rms"], f"{case} {name}: RMS history")
    s.close(); mesh.close()


def _kernel_granular_cycle(s):
    """One V-cycle call by call (src/euler3d_cpu_double.cpp:371-694), every loop its own launch."""
    n = s.num_levels

    def sweep(l):
        s.copy_old_variables(l)
        s.compute_step_factor(l)
        for j in range(3):
            s.compute_fluxes(l)
            s.time_step(l, j)
        s.residual(l)

    for l in range(n):
        sweep(l)
        if l + 1 < n:
            s.restrict(l)
    for l in range(n - 2, -1, -1):
        s.prolong(l)
        if l > 0:
            sweep(l)


@pytest.mark.parametrize("case,name,mode,cfl,smoothing,order", [c for c in COMBOS if c[1] in ("global05", "local25_smooth2")])
def test_same_bits_on_every_path(case, name, mode, cfl, smoothing, order, oracle):
    """advance; begin_step + run_cycles; begin_step + the kernel-granular calls; MGCFD_OPT_GRAPH 0 / 1 and MGCFD_OPT_FUSE_UPDATE
    0 / 1: all the emulator's bits."""
    want = _emulate(oracle, case, name, mode, cfl, smoothing, order)
    for graph, fuse in ((0, 1), (1, 1), (0, 0), (1, 0)):
        mesh, s = _solver(case, graph, fuse=fuse)
        _configure(s, case, name, mode, cfl, smoothing, order)
        s.advance(STEPS, K)
        _check_state(s, want, f"{case} {name} advance graph={graph} fuse={fuse}")
        s.close(); mesh.close()
    for path in ("run_cycles", "granular"):
        mesh, s = _solver(case)
        _configure(s, case, name, mode, cfl, smoothing, order)
        for _ in range(STEPS):
            s.begin_step()
            if path == "run_cycles":
                s.run_cycles(K)
            else:
                for _ in range(K):
                    _kernel_granular_cycle(s)
        _check_state(s, want, f"{case} {name} begin_step + {path}")
        s.close(); mesh.close()


def test_inner_iterations_converge(oracle):
    """The point of the feature, on m6_2lvl from conftest.perturbed_state: within every physical step the RMS falls from its
    first cycle to its last and the BDF residual (F - src) / vol falls.  No tolerance was fixed in advance: the figures are the
    emulator's own on the CPU (profiles/dual_time_convergence.txt: at dt = 2.0 and 24 cycles per step the RMS falls by factors
    of 3.53 / 7.23 / 7.26 in the three steps, monotonically, and max |BDF residual| goes 3.24e-5 -> 1.39e-5, 4.17e-5 -> 1.06e-5,
    4.28e-5 -> 1.09e-5), asserted on the emulator with a margin of a factor 2; the GPU has to give the emulator's state bitwise
    and the same residual from its own arrays."""
    em, hist = dte.point_run(oracle)
    for step, (rms, r0, r1) in enumerate(hist):
        print("step", step, "rms first / last", rms[0], rms[-1], "max |BDF residual| before / after", r0, r1)
        assert rms[0] / rms[-1] > dte.POINT_RMS_DROP[step] / 2.0
        assert r1 / r0 < dte.POINT_RESIDUAL_RATIO[step] * 2.0
    mesh, s = _solver(dte.POINT_CASE)
    s.set_time_step(dte.POINT_MODE, dte.POINT_CFL)
    s.set_residual_smoothing(*dte.POINT_SMOOTHING)
    s.set(0, "variables", perturbed_state(s.nel(0), s.far_field()[:5], dte.POINT_SEED))
    s.run_cycles(1)
    s.set_dual_time(dte.POINT_DT)
    rms = s.advance(dte.POINT_STEPS, dte.POINT_CYCLES)
    want_rms = np.array([h[0] for h in hist])
    _same(rms, want_rms, "point run: RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), em.variables(l), f"point run: variables, level {l}")
    # the BDF2 equation from the library's own arrays, after one more flux evaluation
    s.compute_fluxes(0)
    F, W, Wn, Wn1 = (s.get(0, n).reshape(-1, 5) for n in ("fluxes", "variables", "time_n", "time_n1"))
    vol = s.get(0, "volumes")
    r = (F - dte.source(W, Wn, Wn1, vol, dte.POINT_DT, 2)) / vol[:, None]
    _same(r, em.bdf_residual(0), "BDF residual from get_array")
    assert np.abs(r).max() / hist[-1][1] < dte.POINT_RESIDUAL_RATIO[-1] * 2.0
    s.close(); mesh.close(); em.close()


def test_free_stream_stays_the_free_stream(oracle):
    """From the uniform far field on fvcorr_1lvl the source is +0.0 everywhere (W == Wn == Wn1), so the update takes F - (+0.0):
    with a physical step long enough that the clamp binds nowhere, the first stage gives the bits it gives with dual time off.
    (The golden case's far field is no steady state — its first cycle moves it by an RMS of 2e-2 — so from the second stage on
    W differs from Wn and the two runs part, as they must; 2 steps x 2 cycles on and off are compared against the emulator.)"""
    case = "fvcorr_1lvl"
    em = dte.DualTimeOracle(oracle, case, "global", 0.5)
    em.set_dual_time(1.0)
    em.begin_step()
    src = em.stage_source(0, em.oc.array(0, "variables").reshape(-1, 5))
    assert np.array_equal(_bits(src), np.zeros(src.shape, dtype=np.int64))          # +0.0, not -0.0
    em.reset()                                  # (nothing has run: the advance below starts as the solver's, with BDF1)
    rc, want_rms = em.advance(2, 2)
    assert rc == 0 and em.bound[0][0] == 0                                           # the clamp bound nowhere
    (mesh, off), (mesh2, on) = _solver(case), _solver(case)
    for t in (off, on):
        t.set_time_step("global", 0.5)
    on.set_dual_time(1.0)
    on.begin_step()
    _same(on.get(0, "time_n"), off.get(0, "variables"), "Wn at the start")
    _same(on.get(0, "time_n1"), off.get(0, "variables"), "Wn1 at the start")
    for t in (off, on):
        t.copy_old_variables(0); t.compute_step_factor(0); t.compute_fluxes(0); t.time_step(0, 0)
    _same(on.get(0, "step_factors"), off.get(0, "step_factors"), "step factors: the clamp binds nowhere")
    _same(on.get(0, "variables"), off.get(0, "variables"), "the first stage with src = +0.0")
    on.close(); mesh2.close(); off.close(); mesh.close()
    mesh, s = _solver(case)
    s.set_time_step("global", 0.5)
    s.set_dual_time(1.0)
    rms = s.advance(2, 2).ravel()
    _same(s.get(0, "variables"), em.variables(0), "2 steps x 2 cycles from the far field")
    _same(rms, want_rms, "2 steps x 2 cycles from the far field: RMS history")
    s.close(); mesh.close(); em.close()


def test_switching_and_resources(oracle):
    """on -> off -> cycles equal to a solver that never had it -> on again with reset; mgcfd_live_device_resources is back at its
    starting figures after off and after destroy."""
    import mgcfd
    case, name, mode, cfl = "m6_2lvl", "global05", "global", 0.5
    dt = dte.GPU_DT[case][name]
    before = mgcfd.live_device_resources()
    mesh, s = _solver(case)
    s.set_time_step(mode, cfl)
    s.set(0, "variables", dte.start_state(case, s.far_field()[:5], s.nel(0)))
    s.run_cycles(1)
    held = mgcfd.live_device_resources()
    s.set_dual_time(dt)
    grown = mgcfd.live_device_resources()
    assert grown["allocations"] == held["allocations"] + 2 * s.num_levels + 1      # Wn, Wn1 per level; level 0's numbering
    assert grown["bytes"] > held["bytes"] and grown["bytes"] > held["bytes"]
    s.advance(2, 2)
    s.set_dual_time(0.0)
    assert mgcfd.live_device_resources() == held
    assert s.dual_time()["dt"] == 0.0 and s.dual_time()["levels"] == 0
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.get(0, "time_n")
    assert e.value.code == 1 and "dual time" in str(e.value)
    # a solver that never had it on, given the same state: the same cycles, the same bits
    mesh2, never = _solver(case)
    never.set_time_step(mode, cfl)
    for l in range(s.num_levels):
        never.set(l, "variables", s.get(l, "variables"))
    got, want = s.run_cycles(3), never.run_cycles(3)
    _same(got, want, "RMS of the cycles after switching off")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), never.get(l, "variables"), f"cycles after switching off, level {l}")
    assert s.loop_iters(0)["flux"] > 0
    never.close(); mesh2.close()
    # on again, a step, then reset: the next step starts with both levels equal to the state, BDF1
    s.set_dual_time(dt)
    assert s.dual_time()["levels"] == 0
    s.begin_step(); s.run_cycles(1); s.begin_step(); s.run_cycles(1)
    assert s.dual_time()["levels"] == 2
    s.dual_time_reset()
    assert s.dual_time()["levels"] == 0
    s.begin_step()
    assert s.dual_time()["levels"] == 1
    for l in range(s.num_levels):
        _same(s.get(l, "time_n"), s.get(l, "variables"), f"Wn after reset, level {l}")
        _same(s.get(l, "time_n1"), s.get(l, "variables"), f"Wn1 after reset, level {l}")
    s.close(); mesh.close()
    assert mgcfd.live_device_resources() == before


def test_refusals():
    """Bad dt or clamp, mid-sweep, the sweep_* calls and group creation while on, a group member, a rank, a partitioned solver,
    more than 4096 cycles per advance: error code 1, "dual time" in the message, nothing changed."""
    import mgcfd
    dt = dte.GPU_DT["m6_2lvl"]["global05"]
    mesh, s = _solver("m6_2lvl")
    ref_mesh, ref = _solver("m6_2lvl")
    for t in (s, ref):
        t.set_dual_time(dt)
    state = s.dual_time()
    for bad_dt, bad_clamp in ((-1.0, dte.CLAMP), (float("nan"), dte.CLAMP), (float("inf"), dte.CLAMP), (dt, 0.0), (dt, -0.5),
                              (dt, float("nan")), (dt, float("inf"))):
        with pytest.raises(mgcfd.MgcfdError) as e:
            s.set_dual_time(bad_dt, bad_clamp)
        assert e.value.code == 1 and "dual time" in str(e.value), (bad_dt, bad_clamp)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.dual_time_order(3)
    assert e.value.code == 1 and "dual time" in str(e.value)
    assert s.dual_time() == state
    for call in (lambda: s.sweep_begin(0), lambda: s.sweep_begin_partials(0), lambda: s.sweep_flux0(0), lambda: s.sweep_stage(0, 0),
                 lambda: s.sweep_end(0), lambda: s.sweep_end_partials(0), lambda: mgcfd.Group([s]), lambda: s.rank_attach_plain(0, 1),
                 lambda: s.advance(4097, 1), lambda: s.advance(2, 2049), lambda: s.advance(1, 0)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1 and "dual time" in str(e.value)
    assert s.dual_time() == state
    for t in (s, ref):
        t.advance(1, 1)
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), ref.get(l, "variables"), "a step after the refused calls")
        _same(s.get(l, "time_n"), ref.get(l, "time_n"), "Wn after the refused calls")
    # mid-sweep: the split sweep runs with dual time off; the setter is refused until its last stage has run
    for t in (s, ref):
        t.set_dual_time(0.0)
    for call in (lambda: s.begin_step(), lambda: s.advance(1, 1), lambda: s.dual_time_reset(), lambda: s.dual_time_order(1)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1 and "dual time" in str(e.value)
    s.sweep_begin(0)
    s.sweep_stage(0, 0, partials=False)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_dual_time(dt)
    assert e.value.code == 1 and "dual time" in str(e.value) and "sweep is under way" in str(e.value)
    assert s.dual_time()["dt"] == 0.0
    s.sweep_stage(0, 1, partials=False)
    s.sweep_stage(0, 2, partials=False)
    ref.smooth(0, 1)
    _same(s.get(0, "variables"), ref.get(0, "variables"), "the sweep the refused call interrupted")
    # a group member, and a partitioned solver
    g = mgcfd.Group([s])
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.set_dual_time(dt)
    assert e.value.code == 1 and "dual time" in str(e.value)
    s.set_dual_time(0.0)                                      # switching off is always allowed
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
        t.set_dual_time(dt)
    assert e.value.code == 1 and "dual time" in str(e.value)
    assert t.dual_time()["dt"] == 0.0
    t.close()
    mesh.close()


@pytest.mark.parametrize("case,name,mode,cfl,smoothing,order", [c for c in COMBOS if c[1] in ("global05", "local25_smooth2")])
def test_fast_mode(case, name, mode, cfl, smoothing, order, oracle):
    """exact = 0 (FMA contraction, the order-free flux kernel) within the bound tests/test_gpu_order_free.py applies to whole
    cycles: 1e-10 of the largest value per level, RMS rtol 1e-9."""
    want = _emulate(oracle, case, name, mode, cfl, smoothing, order)
    mesh, s = _solver(case, exact=0)
    _configure(s, case, name, mode, cfl, smoothing, order)
    rms = s.advance(STEPS, K).ravel()
    assert np.allclose(rms, want["rms"], rtol=RMS_FAST, atol=0)
    for l in range(s.num_levels):
        for name_, w in (("variables", want["v"][l]), ("time_n", want["wn"][l]), ("time_n1", want["wn1"][l])):
            rel = np.abs(s.get(l, name_) - w).max() / max(np.abs(w).max(), 1e-300)
            print(case, name, "level", l, name_, "rel", rel)
            assert rel < REL_RUN, (case, name, l, name_, rel)
    s.close(); mesh.close()


def _run_driver(tmp, case, extra, cycles, ok=True):
    os.makedirs(tmp / "out", exist_ok=True)
    cmd = [EXE, "-i", "input.dat", "-d", fse.case_input(case), "-o", "out/", "-g", str(cycles), "-m", str(fse.case_duplicate(case))] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tmp)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


@pytest.mark.parametrize("case", dte.GPU_CASES)
def test_driver(case, oracle, tmp_path):
    """--physical-time-step / --time-steps / --dual-time-clamp / --bdf-order and the config keys, -g as the cycles per physical
    step: the dump is the %.17e rendering of the emulator's final state, the RMS lines its history (one per cycle), the loads
    file has one row per physical step (the solver's own loads of those states); --gpus 2 mesh copies agree (a single level on
    two GPUs is split: refused); --gpus-partition errors before any GPU work."""
    import mgcfd
    dt, n_lv = dte.GPU_DT[case]["local25_smooth2"], (1 if case.endswith("_1lvl") else 2)
    name = f"variables.size={fse.case_duplicate(case)}x.cycles={K}.level=0"
    flags = ["--time-step=local", "--cfl", "2.5", "--residual-smoothing", "0.5", "--physical-time-step", repr(dt), "--time-steps", str(STEPS)]
    dual_only = ["--physical-time-step", repr(dt), "--time-steps", str(STEPS)]
    conf = tmp_path / "run.conf"
    conf.write_text(f"time_step = local\ncfl = 2.5\nresidual_smoothing = 0.5\nphysical_time_step = {dt!r}\ntime_steps = {STEPS}\n"
                    f"dual_time_clamp = 0.5\nbdf_order = 1\n")
    for tag, clamp, order, extra in (("flags", dte.CLAMP, 2, flags), ("said", 0.5, 1, flags + ["--dual-time-clamp", "0.5", "--bdf-order=1"]),
                                     ("conf", 0.5, 1, ["-c", str(conf)]), ("two", dte.CLAMP, 2, flags + ["--gpus", "2", "--gpus-share-device"])):
        d = tmp_path / tag
        if tag == "two" and n_lv == 1:
            # (without the smoothing flags, whose own refusal of a split level would come first)
            r = _run_driver(d, case, ["--output-variables"] + dual_only + ["--gpus", "2", "--gpus-share-device"], K, ok=False)
            assert "dual time" in (r.stdout + r.stderr)
            continue
        em = dte.DualTimeOracle(oracle, case, "local", 2.5, 0.5, 2)
        em.set_dual_time(dt, clamp); em.set_order(order)
        rc, want_rms = em.advance(STEPS, K)
        assert rc == 0
        r = _run_driver(d, case, ["--output-variables"] + extra + ([] if tag == "two" else ["--output-loads"]), K)
        assert (d / "out" / name).read_bytes() == fse.render_variables(em.variables(0)).encode(), f"{case} {tag}"
        em.close()
        total = STEPS * K
        rms_lines = [l for l in r.stdout.splitlines() if "(RMS = " in l]
        assert rms_lines == [(f"Cycle {i + 1} / {total}" if n_lv == 1 else f"MG cycle {i + 1} / {total}") + " (RMS = %.3e)" % want_rms[i]
                             for i in range(total)], f"{case} {tag}"
        if tag == "flags":
            rows = [l.split(",") for l in (d / "out" / f"surface_loads.size={fse.case_duplicate(case)}x.cycles={K}.level=0").read_text().splitlines()]
            assert len(rows) == 1 + STEPS and [row[0] for row in rows[1:]] == [str(k + 1) for k in range(STEPS)]
            mesh, s = _solver(case)
            s.set_time_step("local", 2.5); s.set_residual_smoothing(0.5, 2); s.set_dual_time(dt)
            _, loads = s.advance(STEPS, K, loads=True)
            assert [[float(x) for x in row[1:7]] for row in rows[1:]] == loads.tolist()
            s.close(); mesh.close()
    r = _run_driver(tmp_path / "part", case, dual_only + ["--output-variables", "--gpus", "2", "--gpus-partition", "--gpus-share-device"], K, ok=False)
    assert "dual time" in (r.stdout + r.stderr).lower()
    assert not [n for n in os.listdir(tmp_path / "part" / "out") if n.startswith("variables")]


def test_driver_without_the_flags_gives_the_golden_dump(tmp_path):
    """Without the new flags the golden dumps come out byte for byte."""
    for case in dte.GPU_CASES:
        meta = dict(l.strip().split(" = ") for l in open(os.path.join(fse.GOLDEN, case, "case.txt")))
        cycles, dup = int(meta["cycles"]), fse.case_duplicate(case)
        _run_driver(tmp_path / case, case, ["--output-variables"], cycles)
        golden = open(os.path.join(fse.GOLDEN, case, "variables.level0.txt"), "rb").read()
        assert (tmp_path / case / "out" / f"variables.size={dup}x.cycles={cycles}.level=0").read_bytes() == golden, case


def test_advance_keeps_its_histories_on_an_invalid_state():
    """An invalid state inside advance: the error carries the RMS (NaN from the failing cycle on) and the physical step."""
    import mgcfd
    mesh, s = _solver("fvcorr_1lvl")
    s.set_time_step("local", 6.0)
    s.set_dual_time(10.0)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.advance(3, 4)
    assert e.value.code in (4, 5, 6) and e.value.rms.shape == (3, 4) and np.isnan(e.value.rms[-1, -1])
    assert e.value.step == s.dual_time()["invalid_step"] >= 0
    s.close(); mesh.close()
