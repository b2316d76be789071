"""GPU tests of the unsteady Spalart-Allmaras model (mgcfd_set_sa_unsteady) against the numpy emulator
(tests/sa_unsteady_emulator.py) bit for bit: the timed pass 2, the shielded pass 1 and the DES97 length on the shapes at which
tests/test_gpu_sa.py's gathers can go wrong; the dual-time runs under the three lengths; the composed runs; steady DES; a restart;
the setters in several orders; the refusals and the device allocations; the driver's flags; the fast mode.
tests/test_host_sa_unsteady.py checks the emulator itself and asserts on the CPU that every run here stays valid."""
import os
import subprocess

import numpy as np
import pytest

import fas_emulator as fe
import free_stream_emulator as fse
import sa_emulator as sae
import sa_unsteady_emulator as sue
import viscous_emulator as ve
import wall_heat_emulator as whe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
K = sae.GPU_CYCLES
STEPS, CYCLES, DT = sue.DUAL_STEPS, sue.DUAL_CYCLES, sue.DUAL_DT
REL_RUN = 1e-10          # tests/test_gpu_viscous.py::test_fast_mode's tolerances
RMS_FAST = 1e-9


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(got - want).max():.3e}"


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("sa_unsteady_lattices")
    return {name: fe.write_lattice(name, d) for name in fe.LATTICES}


def _solver(case, exact=1):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    s.set_option("exact", exact)
    return mesh, s


def _configure(s, mu, length="wall", time_accurate=True, dt=DT, c_des=sue.SA_CDES, smoothing=(0.0, 0), jst_levels=0, fas=False, shape="V",
               face_gradient=None, tw_ratio=None, cfl=1.0, order=(0, 1, 2, 3)):
    """The solver as sue.configured sets the emulator up; ``order``: the order of the four setters that complete the combination
    (viscous terms, model, unsteady setting, dual time), which must respect the refusals: the setting before whichever of the model
    and dual time comes second."""
    s.set_time_step("local", cfl)
    if smoothing[1]:
        s.set_residual_smoothing(*smoothing)
    if jst_levels:
        s.set_jst(levels=jst_levels)
    if fas:
        s.set_fas(True)
    if shape != "V":
        s.set_cycle(shape)
    s.set(0, "variables", ve.start_state(s.nel(0), s.far_field()[:5]))
    if face_gradient:
        s.set_face_gradient(face_gradient)

    def viscous():
        s.set_viscous(mu, ve.PRANDTL, True, ve.VISCOUS_CFL, s.num_levels)
        if tw_ratio:
            s.set_wall_temperature("isothermal", whe.setting_value(s.far_field(), whe.ISOTHERMAL, tw_ratio))

    setters = (viscous, lambda: s.set_viscosity_model(law=sue.MODEL[0], eddy=sue.MODEL[1]),
               lambda: s.set_sa_unsteady(time_accurate, length, c_des), lambda: s.set_dual_time(dt) if dt else None)
    for k in order:
        setters[k]()
    assert s.sa_unsteady() == {"time_accurate": bool(time_accurate), "length": length, "c_des": c_des}


# ---- kernel level ----
def test_kernel_level(oracle, lattices, tmp_path):
    """tests/test_gpu_sa.py's kernel-level cases under sue.kernel_variants: a perturbed W, random nt_old, nt and time levels; then
    mgcfd_compute_fluxes and mgcfd_time_step(0, 0): the step factors, sa_gradient, eddy_viscosity, the model length and the new nt
    bitwise the emulator's."""
    import mgcfd
    from conftest import perturbed_state
    from test_gpu_sa import _kernel_cases
    for name, case, amplitude, cfl, mu0 in _kernel_cases(lattices, tmp_path):
        mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
        levels = [dict(mesh.level(l)) for l in range(mesh.num_levels)]
        if levels[0].get("coords") is None or len(levels[0]["coords"]) == 0:
            em0 = sae.SaOracle(oracle, case, "local", cfl)
            levels[0]["coords"] = em0.oc.array(0, "coords").reshape(-1, 3).copy()
            em0.close()
        for length, c_des, order, corrected, mu_v in sue.kernel_variants(name):
            mu = mu_v or mu0
            what = f"{name} {length} c_des={c_des} bdf{order} corrected={corrected} mu={mu}"
            s = mgcfd.Solver.from_arrays(levels, mesh.variant)
            start = perturbed_state(s.nel(0), s.far_field()[:5], seed=7, amplitude=amplitude)
            em, old, new, tl, sf, (grad, mut, S, f, d_model, out) = sue.kernel_level_case(oracle, case, mu, cfl, start, length, c_des, order, corrected)
            s.set_time_step("local", cfl)
            s.set(0, "variables", start)
            if corrected:
                s.set_face_gradient("corrected")
            s.set_viscous(mu, ve.PRANDTL, True, ve.VISCOUS_CFL, 1)
            s.set_viscosity_model(law="sutherland", eddy=sae.SA)
            s.set_sa_unsteady(True, length, c_des)
            s.set(0, "sa_nu_tilde", old)
            s.copy_old_variables(0)
            s.set(0, "sa_nu_tilde", new)
            s.set_dual_time(DT)
            _same(s.get(0, "sa_time_n").ravel(), new, f"{what}: ntn at switch-on")
            _same(s.get(0, "sa_time_n1").ravel(), new, f"{what}: ntn1 at switch-on")
            s.set(0, "sa_time_n", tl[0])
            if order == 2:
                s.set(0, "sa_time_n1", tl[1])
            assert s.dual_time()["levels"] == order
            if length != "wall":
                _same(s.get(0, "sa_length").ravel(), sue.des_length(em.wall_distance(0)[0], np.float64(c_des) * em.delta), f"{what}: d~ at enable")
            s.compute_step_factor(0)
            _same(s.get(0, "step_factors").ravel(), sf, f"{what}: step factors")
            s.compute_fluxes(0)
            _same(s.get(0, "sa_gradient"), grad, f"{what}: sa_gradient")
            _same(s.get(0, "eddy_viscosity").ravel(), mut, f"{what}: eddy viscosity")
            if length != "wall":
                _same(s.get(0, "sa_length").ravel(), d_model, f"{what}: d~")
            s.time_step(0, 0)
            _same(s.get(0, "sa_nu_tilde").ravel(), out, f"{what}: nt after the stage")
            assert np.isfinite(out).all() and (out >= 0.0).all()
            print(what, "ok", em.ubranches)
            em.close()
            s.close()
        mesh.close()


# ---- runs ----
_emulated = {}


def _emulate(oracle, case, mu, length, dt=DT, **kw):
    """(rms, variables per level, nt and mut per covered level, ntn, ntn1, d~) of the run: computed once, shared, left unchanged."""
    key = (case, mu, length, dt, repr(sorted(kw.items())))
    if key not in _emulated:
        em = sue.configured(oracle, case, mu, length, dt=dt, **kw)
        rc, rms = em.advance(STEPS, CYCLES) if dt else em.cycles(K)
        assert rc == 0
        cov = range(em.visc_levels)
        _emulated[key] = (rms, [em.variables(l) for l in range(em.n)], [em.nu_tilde(l) for l in cov], [em.eddy_viscosity(l) for l in cov],
                          None if em.ntn is None else em.ntn.copy(), None if em.ntn1 is None else em.ntn1.copy(),
                          None if em.sa_len is None else em.model_length())
        em.close()
    return _emulated[key]


def _check_run(s, rms, want, what):
    want_rms, want_v, want_nt, want_mut, ntn, ntn1, d_model = want
    _same(np.asarray(rms).ravel(), want_rms, f"{what}: RMS history")
    for l in range(s.num_levels):
        _same(s.get(l, "variables"), want_v[l], f"{what}: variables, level {l}")
    for l in range(len(want_nt)):
        _same(s.get(l, "sa_nu_tilde").ravel(), want_nt[l], f"{what}: nu_tilde, level {l}")
        _same(s.get(l, "eddy_viscosity").ravel(), want_mut[l], f"{what}: eddy viscosity, level {l}")
    if ntn is not None:
        _same(s.get(0, "sa_time_n").ravel(), ntn, f"{what}: sa_time_n")
        _same(s.get(0, "sa_time_n1").ravel(), ntn1, f"{what}: sa_time_n1")
    if d_model is not None:
        _same(s.get(0, "sa_length").ravel(), d_model, f"{what}: sa_length")


@pytest.mark.parametrize("length", sue.RUN_LENGTHS)
@pytest.mark.parametrize("key", sue.RUN_CASES)
def test_runs_equal_the_emulator(key, length, oracle, lattices):
    """ve.DUAL_STEPS + 1 physical steps of ve.DUAL_CYCLES cycles through advance (BDF1, then BDF2 twice)."""
    case = lattices.get(key, key)
    want = _emulate(oracle, case, sue.RUN_MU[key], length)
    mesh, s = _solver(case)
    _configure(s, sue.RUN_MU[key], length)
    rms = s.advance(STEPS, CYCLES)
    print(key, length, "rms", np.asarray(rms).ravel())
    _check_run(s, rms, want, f"{key} {length}")
    s.close(); mesh.close()


@pytest.mark.parametrize("name,kw", sue.composed_settings(), ids=[c[0] for c in sue.composed_settings()])
def test_composition(name, kw, oracle, lattices):
    """Lattice A under delayed DES and dual time with residual smoothing, JST, FAS and a W cycle; and with the corrected face
    gradient and an isothermal wall as well."""
    want = _emulate(oracle, lattices["A"], sue.RUN_MU["A"], "ddes", **kw)
    mesh, s = _solver(lattices["A"])
    _configure(s, sue.RUN_MU["A"], "ddes", **kw)
    _check_run(s, s.advance(STEPS, CYCLES), want, name)
    s.close(); mesh.close()


@pytest.mark.parametrize("length", ("des", "ddes"))
def test_steady_des(length, oracle, lattices):
    """run_cycles with dual time off: the model length alone."""
    want = _emulate(oracle, lattices["A"], sue.RUN_MU["A"], length, dt=0.0)
    mesh, s = _solver(lattices["A"])
    _configure(s, sue.RUN_MU["A"], length, dt=0.0)
    _check_run(s, s.run_cycles(K), want, f"steady {length}")
    import mgcfd
    with pytest.raises(mgcfd.MgcfdError):
        s.get(0, "sa_time_n")
    s.close(); mesh.close()


def test_restart(oracle, lattices):
    """Stop after step 2, read variables, Wn, Wn1, nt, ntn, ntn1 of every level that holds them; a fresh solver, written, continues
    with BDF2: bit for bit the uninterrupted run."""
    want = _emulate(oracle, lattices["A"], sue.RUN_MU["A"], "ddes")
    mesh, s = _solver(lattices["A"])
    _configure(s, sue.RUN_MU["A"], "ddes")
    rms0 = s.advance(2, CYCLES)
    saved = {(l, n): s.get(l, n) for l in range(s.num_levels) for n in ("variables", "time_n", "time_n1", "sa_nu_tilde")}
    saved[(0, "sa_time_n")], saved[(0, "sa_time_n1")] = s.get(0, "sa_time_n"), s.get(0, "sa_time_n1")
    s.close(); mesh.close()
    mesh, s = _solver(lattices["A"])
    _configure(s, sue.RUN_MU["A"], "ddes")
    for l in range(s.num_levels):                       # (the state first: a written nt forms mut from it)
        for n in ("variables", "time_n", "time_n1", "sa_nu_tilde"):
            s.set(l, n, saved[(l, n)])
    s.set(0, "sa_time_n", saved[(0, "sa_time_n")])
    s.set(0, "sa_time_n1", saved[(0, "sa_time_n1")])
    assert s.dual_time()["levels"] == 2
    rms1 = s.advance(STEPS - 2, CYCLES)
    _check_run(s, np.concatenate([np.asarray(rms0).ravel(), np.asarray(rms1).ravel()]), want, "restart")
    s.close(); mesh.close()


@pytest.mark.parametrize("order", [(1, 0, 2, 3), (2, 3, 0, 1), (2, 0, 3, 1), (3, 2, 1, 0), (0, 2, 1, 3)], ids=lambda o: "".join(map(str, o)))
def test_setters_in_several_orders(order, oracle, lattices):
    """Whichever of set_viscous, set_viscosity_model, set_sa_unsteady and set_dual_time completes the combination, the same bits."""
    want = _emulate(oracle, lattices["A"], sue.RUN_MU["A"], "ddes")
    mesh, s = _solver(lattices["A"])
    _configure(s, sue.RUN_MU["A"], "ddes", order=order)
    _check_run(s, s.advance(STEPS, CYCLES), want, f"order {order}")
    s.close(); mesh.close()


def test_reset_and_free_stream(oracle, lattices):
    """dual_time_reset and a reinitialising set_free_stream set both time levels of nt to nt; BDF1 runs again after the reset."""
    em = sue.configured(oracle, lattices["A"], sue.RUN_MU["A"], "wall")
    mesh, s = _solver(lattices["A"])
    _configure(s, sue.RUN_MU["A"], "wall")
    rc, rms = em.advance(2, CYCLES)
    assert rc == 0
    _same(np.asarray(s.advance(2, CYCLES)).ravel(), rms, "before the reset")
    em.reset(); s.dual_time_reset()
    _same(s.get(0, "sa_time_n").ravel(), em.nt[0], "reset: ntn")
    _same(s.get(0, "sa_time_n1").ravel(), em.nt[0], "reset: ntn1")
    rc, rms = em.advance(1, CYCLES)
    assert rc == 0 and em.effective_order() == 1
    _same(np.asarray(s.advance(1, CYCLES)).ravel(), rms, "after the reset")
    _same(s.get(0, "sa_nu_tilde").ravel(), em.nt[0], "after the reset: nt")
    s.set_free_stream(0.8, 2.0, reinitialise=True)
    em.set_far_field(s.far_field(), True)
    _same(s.get(0, "sa_time_n").ravel(), em.ntn, "reinitialised: ntn")
    _same(s.get(0, "sa_time_n1").ravel(), em.ntn1, "reinitialised: ntn1")
    _same(s.get(0, "sa_nu_tilde").ravel(), em.nt[0], "reinitialised: nt")
    em.close()
    s.close(); mesh.close()


def test_refusals_and_device_resources():
    """MGCFD_ERR_ARG with nothing changed; the two old refusals stand with time_accurate = 0; the allocation count goes up and returns."""
    import mgcfd
    mesh, s = _solver("m6_2lvl")
    default = {"time_accurate": False, "length": "wall", "c_des": sue.SA_CDES}
    assert s.sa_unsteady() == default

    def refused(call, text=""):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1 and text in str(e.value), str(e.value)

    for bad in (-1, 3):
        refused(lambda: s._c(s.lib.mgcfd_set_sa_unsteady(s.handle, 1, bad, 0.65)), "length")
    for c_des in (0.0, -1.0, float("nan"), float("inf")):
        refused(lambda: s.set_sa_unsteady(True, "des", c_des), "c_des")
    assert s.sa_unsteady() == default
    for l, n in ((0, "sa_time_n"), (0, "sa_time_n1"), (0, "sa_length")):
        refused(lambda: s.get(l, n), "SA_")
    # the old refusals with time_accurate = 0
    s.set_viscous(1e-3, wall=True, levels=2)
    s.set_viscosity_model(eddy=sae.SA)
    refused(lambda: s.set_dual_time(0.1), "Spalart-Allmaras")
    s.set_viscosity_model()
    s.set_dual_time(0.1)
    refused(lambda: s.set_viscosity_model(eddy=sae.SA), "dual time")
    s.set_dual_time(0.0)
    s.set_viscosity_model(eddy=sae.SA)
    sa_only = mgcfd.live_device_resources()
    # the length: delta and d~ on level 0
    s.set_sa_unsteady(False, "des")
    assert mgcfd.live_device_resources()["allocations"] == sa_only["allocations"] + 2
    refused(lambda: s.set(0, "sa_length", np.zeros(s.nel(0))), "read-only")
    refused(lambda: s.get(1, "sa_length"), "SA_LENGTH")
    refused(lambda: s.set_dual_time(0.1), "Spalart-Allmaras")
    # the time levels: ntn and ntn1 on level 0 beside Wn and Wn1 of both levels
    s.set_sa_unsteady(True, "des")
    with_length = mgcfd.live_device_resources()
    s.set_dual_time(0.1)
    on = mgcfd.live_device_resources()
    assert on["allocations"] >= with_length["allocations"] + 2 + 4
    assert s.get(0, "sa_time_n").shape[0] == s.nel(0)
    refused(lambda: s.get(1, "sa_time_n"), "SA_TIME_N")
    refused(lambda: s.set_sa_unsteady(False, "des"), "time_accurate")
    assert s.sa_unsteady()["time_accurate"]
    assert s.bench_sa(0, "gradient", 2) > 0.0 and s.bench_sa(0, "transport", 2) > 0.0
    s.set_sa_unsteady(True, "ddes", 0.5)
    assert mgcfd.live_device_resources()["allocations"] == on["allocations"]
    assert s.bench_sa(0, "gradient", 2) > 0.0
    s.set_dual_time(0.0)
    now = mgcfd.live_device_resources()
    assert now["allocations"] == with_length["allocations"] and now["bytes"] == with_length["bytes"]
    s.set_sa_unsteady(False, "wall")
    now = mgcfd.live_device_resources()
    assert now["allocations"] == sa_only["allocations"] and now["bytes"] == sa_only["bytes"]
    # kept while the model or the viscous terms are off; released with either
    s.set_sa_unsteady(True, "ddes")
    s.set_dual_time(0.1)
    s.set_viscosity_model()
    refused(lambda: s.get(0, "sa_length"), "SA_LENGTH")
    refused(lambda: s.get(0, "sa_time_n"), "SA_TIME_N")
    s.set_viscosity_model(eddy=sae.SA)                    # (dual time is on: time_accurate lets the model in)
    assert s.get(0, "sa_time_n").shape[0] == s.nel(0)
    s.set_viscous(0.0, levels=0)
    refused(lambda: s.get(0, "sa_length"), "SA_LENGTH")
    assert s.sa_unsteady() == {"time_accurate": True, "length": "ddes", "c_des": sue.SA_CDES}
    s.set_dual_time(0.0)
    s.set_viscosity_model()
    s.set_sa_unsteady()
    # mid-sweep
    s.sweep_begin(0)
    s.sweep_stage(0, 0, partials=False)
    refused(lambda: s.set_sa_unsteady(True, "des"), "sweep is under way")
    assert s.sa_unsteady() == default
    s.sweep_stage(0, 1, partials=False)
    s.sweep_stage(0, 2, partials=False)
    # a group member
    g = mgcfd.Group([s])
    refused(lambda: s.set_sa_unsteady(True, "des"))
    assert s.sa_unsteady() == default
    g.close()
    s.close(); mesh.close()
    # a partitioned solver
    from mgcfd.partition import partition_hierarchy, rcb_partition
    mesh = mgcfd.Mesh("input.dat", fse.case_input("m6_2lvl"), 1)
    levels = [mesh.level(l) for l in range(mesh.num_levels)]
    H = partition_hierarchy(levels, rcb_partition(np.asarray(levels[0]["coords"]).reshape(-1, 3), 2))
    lv, owned, keys = H[0].solver_args()
    t = mgcfd.Solver.from_arrays(lv, mesh.variant, n_owned=owned, order_keys=keys)
    refused(lambda: t.set_sa_unsteady(True, "des"))
    assert t.sa_unsteady() == default
    t.close()
    mesh.close()


def test_fast_mode(oracle, lattices):
    """exact = 0 on lattice A under delayed DES and dual time: the model's kernels are never contracted, so against the exact-mode
    run (the emulator's bits) the state and nt stay within tests/test_gpu_viscous.py::test_fast_mode's bounds — 1e-10 of the largest
    value per level, RMS rtol 1e-9."""
    want_rms, want_v, want_nt, *_ = _emulate(oracle, lattices["A"], sue.RUN_MU["A"], "ddes")
    mesh, s = _solver(lattices["A"], exact=0)
    _configure(s, sue.RUN_MU["A"], "ddes")
    rms = np.asarray(s.advance(STEPS, CYCLES)).ravel()
    print("fast mode: RMS relative", np.abs(rms / want_rms - 1.0).max())
    rels = []
    for l in range(s.num_levels):
        rel = np.abs(s.get(l, "variables") - want_v[l]).max() / max(np.abs(want_v[l]).max(), 1e-300)
        rel_nt = np.abs(s.get(l, "sa_nu_tilde").ravel() - want_nt[l]).max() / np.abs(want_nt[l]).max()
        print("fast mode: level", l, "rel", rel, "nt rel", rel_nt)
        rels.append((rel, rel_nt))
    assert np.allclose(rms, want_rms, rtol=RMS_FAST, atol=0)
    for l, (rel, rel_nt) in enumerate(rels):
        assert rel <= REL_RUN and rel_nt <= REL_RUN, f"level {l}: {rel:.3e} {rel_nt:.3e}"
    s.close(); mesh.close()


# ---- the drop-in binary ----
def _run_driver(tmp, case, extra, cycles, ok=True):
    os.makedirs(tmp / "out", exist_ok=True)
    cmd = [EXE, "-i", "input.dat", "-d", fse.case_input(case), "-o", "out/", "-g", str(cycles), "-m", str(fse.case_duplicate(case))] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tmp)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    if not ok:
        assert r.returncode == 1, r.stdout + r.stderr
    return r


def test_driver_flags(oracle, tmp_path):
    """--sa-time-accurate, --sa-length and --sa-cdes (and the config keys) on m6_2lvl with --physical-time-step: the dump is the
    %.17e rendering of the emulator's state; without --spalart-allmaras, and --spalart-allmaras --physical-time-step without
    --sa-time-accurate: exit status 1 and no dump."""
    case = "m6_2lvl"
    dup = fse.case_duplicate(case)
    name = f"variables.size={dup}x.cycles={CYCLES}.level=0"
    dt = 0.1
    em = sue.SaUnsteadyOracle(oracle, case, mu=ve.DRIVER_MU, wall=1, viscous_levels="all")
    em.set_sa_unsteady(True, "des", 0.5)
    em.set_viscosity_model(law="constant", eddy=sae.SA)
    em.set_dual_time(dt)
    rc, want_rms = em.advance(STEPS, CYCLES)
    assert rc == 0
    want = fse.render_variables(em.variables(0)).encode()
    em.close()
    base = ["--output-variables", "--viscosity", repr(ve.DRIVER_MU), "--no-slip", "--viscous-levels", "8", "--spalart-allmaras"]
    dual = ["--physical-time-step", repr(dt), "--time-steps", str(STEPS)]
    conf = tmp_path / "run.conf"
    conf.write_text(f"viscosity = {ve.DRIVER_MU!r}\nno_slip = Y\nviscous_levels = 8\nspalart_allmaras = Y\nsa_time_accurate = Y\nsa_length = des\n"
                    f"sa_cdes = 0.5\nphysical_time_step = {dt!r}\ntime_steps = {STEPS}\n")
    for tag, extra in (("flags", base + dual + ["--sa-time-accurate", "--sa-length", "des", "--sa-cdes", "0.5"]),
                       ("conf", ["--output-variables", "-c", str(conf)])):
        d = tmp_path / tag
        r = _run_driver(d, case, extra, CYCLES)
        assert (d / "out" / name).read_bytes() == want, tag
        lines = [l for l in r.stdout.splitlines() if "(RMS = " in l]
        total = STEPS * CYCLES
        assert lines == [f"MG cycle {i + 1} / {total}" + " (RMS = %.3e)" % want_rms[i] for i in range(total)], tag
    _run_driver(tmp_path / "rans", case, base + dual + ["--sa-time-accurate"], CYCLES)
    assert (tmp_path / "rans" / "out" / name).read_bytes() != want      # (the wall distance: another state, if only in the last bits)
    for tag, bad in (("no_model", ["--output-variables", "--viscosity", repr(ve.DRIVER_MU), "--sa-length", "des"]),
                     ("no_model_time", ["--output-variables", "--viscosity", repr(ve.DRIVER_MU), "--sa-time-accurate"]),
                     ("no_model_cdes", ["--output-variables", "--viscosity", repr(ve.DRIVER_MU), "--sa-cdes", "0.5"]),
                     ("dual_without", base + dual), ("dual_length_only", base + dual + ["--sa-length", "ddes"]),
                     ("bad_length", base + ["--sa-length", "iddes"]), ("bad_cdes", base + ["--sa-cdes", "-1"])):
        _run_driver(tmp_path / tag, case, bad, CYCLES, ok=False)
        assert not [n for n in os.listdir(tmp_path / tag / "out") if n.startswith("variables")], tag


def test_defaults_reproduce_the_golden_output(tmp_path):
    """With the new flags absent the golden variables.level0.txt byte for byte, and so the Python API with the setting made while
    the model is off (no effect, nothing allocated)."""
    import mgcfd
    case = "m6_2lvl"
    meta = dict(l.strip().split(" = ") for l in open(os.path.join(fse.GOLDEN, case, "case.txt")))
    cycles, dup = int(meta["cycles"]), fse.case_duplicate(case)
    golden = open(os.path.join(fse.GOLDEN, case, "variables.level0.txt"), "rb").read()
    _run_driver(tmp_path / "plain", case, ["--output-variables"], cycles)
    assert (tmp_path / "plain" / "out" / f"variables.size={dup}x.cycles={cycles}.level=0").read_bytes() == golden
    mesh, s = _solver(case)
    before = mgcfd.live_device_resources()["allocations"]
    s.set_sa_unsteady(True, "ddes", 0.5)
    assert mgcfd.live_device_resources()["allocations"] == before
    s.run_cycles(cycles)
    assert fse.render_variables(s.get(0, "variables")).encode() == golden
    s.close(); mesh.close()
