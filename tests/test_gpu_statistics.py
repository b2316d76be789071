"""GPU tests of the flow statistics (mgcfd_set_statistics) against the numpy emulator (tests/statistics_emulator.py) bit for bit:
the volume sample on a partial last block, more than one block and the tetrahedral level, without an eddy viscosity, with the
caller's field and under Spalart-Allmaras; the wall table; the dual-time runs through advance, alone, composed, with loads and
with a changed step; a restart; a step that goes invalid; the mode changes, refusals and device allocations; the fast mode; the
driver's flags.  tests/test_host_statistics.py checks the emulator itself and asserts on the CPU that every run here stays valid."""
import os
import subprocess

import numpy as np
import pytest

import fas_emulator as fe
import free_stream_emulator as fse
import friction_loads_emulator as fle
import sa_emulator as sae
import sa_unsteady_emulator as sue
import statistics_emulator as ste
import variable_viscosity_emulator as vve
import viscous_emulator as ve

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
STEPS, CYCLES, DT = sue.DUAL_STEPS, sue.DUAL_CYCLES, sue.DUAL_DT
KERNEL_CASES = (("B", 0.01), ("A", 0.01), ("tet_2lvl", 0.002))         # (case, tests/test_gpu_sa.py's perturbation amplitude)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: max |difference| {np.abs(got - want).max():.3e}"


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("statistics_lattices")
    out = {name: fe.write_lattice(name, d) for name in fe.LATTICES}
    out["box17"] = fle.write_case("box17", d)
    return out


def _solver(case, exact=1):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    s.set_option("exact", exact)
    return mesh, s


def _configure(s, mu, **kw):
    from test_gpu_sa_unsteady import _configure as configure
    configure(s, mu, "ddes", **kw)


def _check_volume(s, acc, what):
    st = s.statistics()
    assert st["samples"] == acc.samples, f"{what}: samples {st['samples']} != {acc.samples}"
    _same(np.float64(st["wsum"]), np.float64(acc.wsum), f"{what}: wsum")
    _same(s.get(0, "statistics_mean"), acc.m, f"{what}: statistics_mean")
    _same(s.get(0, "statistics_moments"), acc.c, f"{what}: statistics_moments")


def _mut(s):
    import mgcfd
    try:
        return s.get(0, "eddy_viscosity").ravel()
    except mgcfd.MgcfdError:
        return None


# ---- kernel level ----
@pytest.mark.parametrize("eddy", ("none", "field", "spalart-allmaras"))
@pytest.mark.parametrize("key,amplitude", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_kernel_level(key, amplitude, eddy, lattices):
    """Five seeded perturbed states through set, a sample of each with the weights (0.02, 0.02, 0.05, 0.02, 0.013): after each the
    two arrays, samples and wsum are the emulator's.  Without the viscous terms the mut column stays +0.0; with the caller's field
    and under Spalart-Allmaras (a new nu_tilde per sample, which forms mut again) it averages MGCFD_ARR_EDDY_VISCOSITY as the
    library holds it.  The first sample alone gives m = x and c = +0.0."""
    from conftest import perturbed_state
    case = lattices.get(key, key)
    mesh, s = _solver(case)
    nel, ff = s.nel(0), s.far_field()
    mu = sue.RUN_MU[key]
    if eddy != "none":
        s.set_viscous(mu, ve.PRANDTL, True, ve.VISCOUS_CFL, 1)
        s.set_viscosity_model(law="sutherland" if eddy == sae.SA else "constant", eddy=eddy)
    s.set_statistics("volume")
    assert s.statistics() == {"mode": "volume", "samples": 0, "wsum": 0.0}
    _same(s.get(0, "statistics_mean"), np.zeros((nel, 6)), "zeroed means")
    _same(s.get(0, "statistics_moments"), np.zeros((nel, 7)), "zeroed co-moments")
    acc = ste.Accumulator(nel)
    for k, (seed, w) in enumerate(zip(ste.KERNEL_SEEDS, ste.KERNEL_WEIGHTS)):
        state = perturbed_state(nel, ff[:5], seed=seed, amplitude=amplitude)
        s.set(0, "variables", state)
        if eddy == "field":
            s.set(0, "eddy_viscosity", vve.eddy_field(mu, nel, k))
        if eddy == sae.SA:
            s.set(0, "sa_nu_tilde", sae.random_nt(mu, ff[0], nel, sae.NT_SEED + k))
        mut = _mut(s)
        assert (mut is None) == (eddy == "none")
        if mut is not None:
            assert mut.max() > 0.0
        s.statistics_sample(w)
        acc.sample(state, mut, w)
        _check_volume(s, acc, f"{key} {eddy} sample {k}")
        if k == 0:
            x = ste.sample_values(state, mut)
            assert np.array_equal(s.get(0, "statistics_mean"), x)              # (up to the sign of a zero)
            _same(s.get(0, "statistics_moments"), np.zeros((nel, 7)), "first sample: c")
    if eddy == "none":
        _same(s.get(0, "statistics_mean")[:, 5], np.zeros(nel), "the mut column without an eddy viscosity")
    s.close(); mesh.close()


def test_identical_states_give_exact_zeros(lattices):
    """Five samples of one state: m == x bitwise, every co-moment +0.0."""
    from conftest import perturbed_state
    mesh, s = _solver(lattices["B"])
    nel = s.nel(0)
    state = perturbed_state(nel, s.far_field()[:5], seed=7)
    s.set(0, "variables", state)
    s.set_statistics("volume")
    for w in ste.KERNEL_WEIGHTS:
        s.statistics_sample(w)
    _same(s.get(0, "statistics_mean"), ste.sample_values(state), "constant signal: m")
    _same(s.get(0, "statistics_moments"), np.zeros((nel, 7)), "constant signal: c")
    assert s.statistics()["samples"] == 5
    s.close(); mesh.close()


def test_fast_mode(lattices):
    """exact = 0: the statistics kernels are never contracted, so samples of states written through set are still the emulator's."""
    from conftest import perturbed_state
    mesh, s = _solver(lattices["B"], exact=0)
    nel = s.nel(0)
    s.set_statistics("volume")
    acc = ste.Accumulator(nel)
    for seed, w in zip(ste.KERNEL_SEEDS[:3], ste.KERNEL_WEIGHTS[:3]):
        state = perturbed_state(nel, s.far_field()[:5], seed=seed)
        s.set(0, "variables", state)
        s.statistics_sample(w)
        acc.sample(state, None, w)
    _check_volume(s, acc, "fast mode")
    s.close(); mesh.close()


# ---- the wall table ----
@pytest.mark.parametrize("viscous", (True, False), ids=("viscous", "inviscid"))
@pytest.mark.parametrize("key", ("A", "box17"))
def test_wall_table(key, viscous, lattices):
    """Three samples in mode 2: the table equals the emulator run on wall_distribution's tables of the same states (t = +0.0 with
    the viscous terms off), in wall_distribution's order; the volume arrays as in mode 1."""
    from conftest import perturbed_state
    mesh, s = _solver(lattices[key])
    nel = s.nel(0)
    if viscous:
        s.set_viscous(fle.GPU_MU[key], ve.PRANDTL, True, ve.VISCOUS_CFL, 1)
    s.set_statistics("wall")
    ids0, table0 = s.wall_statistics()
    assert len(ids0) == s.wall_node_count(0) > 0 and (key != "box17" or len(ids0) == 278)
    _same(table0, np.zeros((len(ids0), 8)), "zeroed wall table")
    acc = ste.Accumulator(nel)
    for k, w in enumerate(ste.KERNEL_WEIGHTS[2:5]):
        state = perturbed_state(nel, s.far_field()[:5], seed=ste.KERNEL_SEEDS[k])
        s.set(0, "variables", state)
        ids, dist = s.wall_distribution(0)
        assert viscous == bool(dist[:, 4:7].any())
        s.statistics_sample(w)
        acc.sample(state, None, w)
        acc.wall_sample(dist, w)
        got_ids, got = s.wall_statistics()
        assert np.array_equal(got_ids, ids)
        _same(got, acc.wall, f"{key} wall table, sample {k}")
        _same(s.wall_distribution(0)[1], dist, "wall_distribution's own result")
        _check_volume(s, acc, f"{key} volume arrays in mode 2, sample {k}")
    if not viscous:
        _same(acc.wall[:, [1, 2, 3, 5, 6, 7]], np.zeros((len(ids0), 6)), "t = +0.0 with the viscous terms off")
    assert s.bench_statistics("volume", 2) > 0.0 and s.bench_statistics("wall", 2) > 0.0
    _same(s.wall_statistics()[1], acc.wall, "the wall table behind the bench launches")
    s.close(); mesh.close()


def test_a_mesh_without_solid_walls(tmp_path):
    """Mode 2 on a level without walls: n = 0, nothing launched, no error; the volume sample runs."""
    from mgcfd import meshgen
    mg = meshgen.MultigridMesh(mesh_name="fvcorr")
    mg.levels.append(meshgen.make_box_level(9, seed=2, jitter=0.2))
    d = tmp_path / "no_wall"
    os.makedirs(d / "input")
    meshgen.write_input(mg, str(d / "input"))
    (d / "case.txt").write_text("duplicate = 1\n")
    mesh, s = _solver(str(d))
    s.set_statistics("wall")
    s.statistics_sample(0.5)
    ids, table = s.wall_statistics()
    assert len(ids) == 0 and table.shape == (0, 8)
    s.set_wall_statistics(np.zeros((0, 8)))
    assert s.statistics()["samples"] == 1
    _same(s.get(0, "statistics_mean"), ste.sample_values(s.get(0, "variables")), "the volume sample")
    s.close(); mesh.close()


# ---- runs ----
_emulated = {}


def _emulate(oracle, case, mu, second_dt=None, **kw):
    """(rms, variables of level 0, m, c, samples, wsum) of the run: computed once, shared, left unchanged."""
    key = (case, mu, second_dt, repr(sorted(kw.items())))
    if key not in _emulated:
        em = ste.configured(oracle, case, mu, "ddes", **kw)
        if second_dt is None:
            rc, rms = em.advance(STEPS, CYCLES)
        else:
            rc, rms = em.advance(2, CYCLES)
            em.set_dual_time(second_dt)
            rc2, rms2 = em.advance(STEPS - 2, CYCLES)
            rc, rms = rc or rc2, np.concatenate([rms, rms2])
        assert rc == 0
        _emulated[key] = (rms, em.variables(0), em.stat.m.copy(), em.stat.c.copy(), em.stat.samples, em.stat.wsum, em.nu_tilde(0))
        em.close()
    return _emulated[key]


def _check_run(s, rms, want, what):
    want_rms, want_v, m, c, samples, wsum, nt = want
    _same(np.asarray(rms).ravel(), want_rms, f"{what}: RMS history")
    _same(s.get(0, "variables"), want_v, f"{what}: variables")
    _same(s.get(0, "sa_nu_tilde").ravel(), nt, f"{what}: nu_tilde")
    st = s.statistics()
    assert st["samples"] == samples
    _same(np.float64(st["wsum"]), np.float64(wsum), f"{what}: wsum")
    _same(s.get(0, "statistics_mean"), m, f"{what}: statistics_mean")
    _same(s.get(0, "statistics_moments"), c, f"{what}: statistics_moments")


@pytest.mark.parametrize("key", ("A", "B"))
def test_runs_equal_the_emulator(key, oracle, lattices):
    """sue.DUAL_STEPS steps of sue.DUAL_CYCLES cycles under delayed DES with BDF2 through advance: the state, nt and the RMS
    history are those of the same run with the statistics off, and the two arrays the emulator's."""
    want = _emulate(oracle, lattices[key], sue.RUN_MU[key])
    mesh, s = _solver(lattices[key])
    s.set_statistics("volume")
    _configure(s, sue.RUN_MU[key])
    rms = s.advance(STEPS, CYCLES)
    _check_run(s, rms, want, f"lattice {key}")
    mesh0, s0 = _solver(lattices[key])
    _configure(s0, sue.RUN_MU[key])
    _same(s0.advance(STEPS, CYCLES), rms, "RMS history with the statistics off")
    _same(s0.get(0, "variables"), s.get(0, "variables"), "state with the statistics off")
    fs = s.flow_statistics()
    _same(np.concatenate([fs["reynolds"], fs["p_rms"][:, None], fs["k"][:, None]], axis=1), ste.derive(want[5], want[3]), "flow_statistics")
    _same(fs["mean"], want[2], "flow_statistics: mean")
    s0.close(); mesh0.close()
    s.close(); mesh.close()


def test_composition(oracle, lattices):
    """Lattice A composed with residual smoothing, JST, FAS and a W cycle."""
    name, kw = sue.composed_settings()[0]
    want = _emulate(oracle, lattices["A"], sue.RUN_MU["A"], **kw)
    mesh, s = _solver(lattices["A"])
    _configure(s, sue.RUN_MU["A"], **kw)
    s.set_statistics("volume")
    _check_run(s, s.advance(STEPS, CYCLES), want, name)
    s.close(); mesh.close()


def test_a_changed_step_changes_the_weights(oracle, lattices):
    """Two steps at dt, two at dt / 2: wsum and the a sequence follow."""
    want = _emulate(oracle, lattices["A"], sue.RUN_MU["A"], second_dt=DT / 2)
    mesh, s = _solver(lattices["A"])
    _configure(s, sue.RUN_MU["A"])
    s.set_statistics("volume")
    rms = np.asarray(s.advance(2, CYCLES)).ravel()
    s.set_dual_time(DT / 2)
    rms = np.concatenate([rms, np.asarray(s.advance(STEPS - 2, CYCLES)).ravel()])
    _check_run(s, rms, want, "changed step")
    s.close(); mesh.close()


@pytest.mark.parametrize("order", ("first", "before_dual_time", "last"))
def test_setters_in_three_orders(order, oracle, lattices):
    """set_statistics before the other setters, between the model and dual time, and behind them all: the same bits."""
    want = _emulate(oracle, lattices["A"], sue.RUN_MU["A"])
    mesh, s = _solver(lattices["A"])
    if order == "first":
        s.set_statistics("volume")
        _configure(s, sue.RUN_MU["A"], order=(2, 3, 0, 1))
    elif order == "before_dual_time":
        _configure(s, sue.RUN_MU["A"], dt=0.0)
        s.set_statistics("volume")
        s.set_dual_time(DT)
    else:
        _configure(s, sue.RUN_MU["A"])
        s.set_statistics("volume")
    _check_run(s, s.advance(STEPS, CYCLES), want, f"order {order}")
    s.close(); mesh.close()


def test_advance_with_friction_loads_and_the_wall_table(oracle, lattices):
    """advance_loads_viscous in mode 2: the loads rows are those of the run without statistics, taken step by step, and the wall
    table is the emulator's on that run's wall_distribution tables; the volume arrays the emulated run's."""
    want = _emulate(oracle, lattices["A"], sue.RUN_MU["A"])
    mesh, s = _solver(lattices["A"])
    _configure(s, sue.RUN_MU["A"])
    s.set_statistics("wall")
    rms, loads = s.advance(STEPS, CYCLES, loads=True, friction=True)
    _check_run(s, rms, want, "with friction loads")
    mesh0, s0 = _solver(lattices["A"])
    _configure(s0, sue.RUN_MU["A"])
    acc = ste.Accumulator(s0.nel(0))
    for step in range(STEPS):
        _, row = s0.advance(1, CYCLES, loads=True, friction=True)
        _same(row[0], loads[step], f"loads row {step}")
        acc.sample(s0.get(0, "variables"), s0.get(0, "eddy_viscosity").ravel(), DT)
        acc.wall_sample(s0.wall_distribution(0)[1], DT)
    ids, table = s.wall_statistics()
    assert np.array_equal(ids, s0.wall_distribution(0)[0])
    _same(table, acc.wall, "wall table")
    assert table[:, 4:].max() > 0.0 and np.abs(table[:, 1:4]).max() > 0.0
    s0.close(); mesh0.close()
    s.close(); mesh.close()


def test_restart(oracle, lattices):
    """Two steps; the state, the time levels, nt and its levels, both statistics arrays, the wall table, samples and wsum written
    into a fresh solver; two more steps: bitwise the uninterrupted four-step run."""
    want = _emulate(oracle, lattices["A"], sue.RUN_MU["A"])
    mesh, s = _solver(lattices["A"])
    _configure(s, sue.RUN_MU["A"])
    s.set_statistics("wall")
    rms_all = s.advance(STEPS, CYCLES)
    _check_run(s, rms_all, want, "uninterrupted")
    wall_all = s.wall_statistics()[1]
    s.close(); mesh.close()
    mesh, s = _solver(lattices["A"])
    _configure(s, sue.RUN_MU["A"])
    s.set_statistics("wall")
    rms0 = s.advance(2, CYCLES)
    saved = {(l, n): s.get(l, n) for l in range(s.num_levels) for n in ("variables", "time_n", "time_n1", "sa_nu_tilde")}
    for n in ("sa_time_n", "sa_time_n1", "statistics_mean", "statistics_moments"):
        saved[(0, n)] = s.get(0, n)
    wall, st = s.wall_statistics()[1], s.statistics()
    assert st["samples"] == 2
    s.close(); mesh.close()
    mesh, s = _solver(lattices["A"])
    _configure(s, sue.RUN_MU["A"])
    s.set_statistics("wall")
    for l in range(s.num_levels):                       # (the state first: a written nt forms mut from it)
        for n in ("variables", "time_n", "time_n1", "sa_nu_tilde"):
            s.set(l, n, saved[(l, n)])
    for n in ("sa_time_n", "sa_time_n1", "statistics_mean", "statistics_moments"):
        s.set(0, n, saved[(0, n)])
    s.statistics_restore(st["samples"], st["wsum"])
    s.set_wall_statistics(wall)
    assert s.statistics() == st
    rms1 = s.advance(STEPS - 2, CYCLES)
    _check_run(s, np.concatenate([np.asarray(rms0).ravel(), np.asarray(rms1).ravel()]), want, "restart")
    _same(s.wall_statistics()[1], wall_all, "restart: wall table")
    s.close(); mesh.close()


def test_an_invalid_step_is_not_sampled(oracle):
    """tests/test_gpu_dual_time.py's invalid case behind two valid steps: samples counts the completed steps and the arrays are the
    emulator's after them."""
    import mgcfd
    rc0, rms0, rc, rms, em = ste.invalid_run(oracle)
    assert rc0 == 0 and rc != 0
    mesh, s = _solver(ste.INVALID_CASE)
    s.set_time_step("local", ste.VALID_CFL)
    s.set(0, "variables", ste.invalid_start(s.nel(0), s.far_field()[:5]))
    s.set_dual_time(ste.VALID_DT)
    s.set_statistics("volume")
    _same(np.asarray(s.advance(ste.VALID_STEPS, ste.INVALID_CYCLES)).ravel(), rms0, "the valid steps' RMS")
    s.set_time_step("local", ste.INVALID_CFL)
    s.set_dual_time(ste.INVALID_DT)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.advance(ste.INVALID_STEPS, ste.INVALID_CYCLES)
    assert e.value.code in (4, 5, 6) and e.value.step >= 0
    assert s.statistics()["samples"] == ste.VALID_STEPS + e.value.step == em.stat.samples
    _check_volume(s, em.stat, "after the invalid step")
    em.close()
    s.close(); mesh.close()


# ---- housekeeping ----
def test_reset_modes_and_device_resources(lattices):
    """reset; 1 -> 2 -> 1 -> 0; the allocation count goes up by what the modes hold and returns, with and without a wall plan made
    before; the arrays read in place through torch equal get."""
    import torch
    import mgcfd
    from mgcfd.distributed import DevArrayView
    from conftest import perturbed_state
    mesh, s = _solver(lattices["A"])
    nel = s.nel(0)
    s.set(0, "variables", perturbed_state(nel, s.far_field()[:5], seed=7))       # (at the far field dp is an exact zero)
    fresh = mgcfd.live_device_resources()
    s.set_statistics("wall")                           # (makes the wall plan, which goes with the mode again)
    s.statistics_sample(1.0)
    s.set_statistics("off")
    now = mgcfd.live_device_resources()
    assert now["allocations"] == fresh["allocations"] and now["bytes"] == fresh["bytes"]
    s.wall_distribution(0)                             # (the plan is the caller's from here on)
    before = mgcfd.live_device_resources()
    s.set_statistics("volume")
    assert mgcfd.live_device_resources()["allocations"] == before["allocations"] + 2
    s.statistics_sample(0.5)
    s.statistics_sample(0.25)
    assert s.statistics() == {"mode": "volume", "samples": 2, "wsum": 0.75}
    kept = s.get(0, "statistics_mean")
    s.set_statistics("wall")
    assert mgcfd.live_device_resources()["allocations"] == before["allocations"] + 4
    assert s.statistics() == {"mode": "wall", "samples": 2, "wsum": 0.75}
    _same(s.get(0, "statistics_mean"), kept, "1 -> 2 keeps the volume accumulators")
    s.statistics_sample(0.5)
    assert s.wall_statistics()[1].any()
    s.set_statistics("volume")
    assert mgcfd.live_device_resources()["allocations"] == before["allocations"] + 2
    s.set_statistics("wall")
    _same(s.wall_statistics()[1], np.zeros((s.wall_node_count(0), 8)), "2 -> 1 -> 2 zeroes the wall table")
    # in place through torch: [ncols][stride] in the library's numbering
    marker = np.arange(nel * 6, dtype=np.float64).reshape(nel, 6)
    s.set(0, "statistics_mean", marker)
    ptr, count = s.array_devptr(0, "statistics_mean")
    dev = DevArrayView(ptr, count).tensor(torch.device("cuda", 0)).cpu().numpy().reshape(6, -1)[:, :nel]
    node = (dev[0] / 6).astype(np.int64)
    assert np.array_equal(np.sort(node), np.arange(nel))
    _same(dev.T, s.get(0, "statistics_mean")[node], "devptr through torch against get")
    s.array_written(0, "statistics_mean")
    ptr7, count7 = s.array_devptr(0, "statistics_moments")
    assert count7 * 6 == count * 7
    # reset
    s.statistics_reset()
    assert s.statistics() == {"mode": "wall", "samples": 0, "wsum": 0.0}
    _same(s.get(0, "statistics_mean"), np.zeros((nel, 6)), "reset: means")
    _same(s.get(0, "statistics_moments"), np.zeros((nel, 7)), "reset: co-moments")
    _same(s.wall_statistics()[1], np.zeros((s.wall_node_count(0), 8)), "reset: wall table")
    s.set_statistics("off")
    now = mgcfd.live_device_resources()
    assert now["allocations"] == before["allocations"] and now["bytes"] == before["bytes"]
    assert s.statistics() == {"mode": "off", "samples": 0, "wsum": 0.0}
    s.close(); mesh.close()


def test_refusals():
    """MGCFD_ERR_ARG with nothing changed."""
    import mgcfd
    mesh, s = _solver("m6_2lvl")
    off = {"mode": "off", "samples": 0, "wsum": 0.0}
    assert s.statistics() == off

    def refused(call, text=""):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1 and text in str(e.value), str(e.value)

    # while the mode is off
    for name in ("statistics_mean", "statistics_moments"):
        refused(lambda: s.get(0, name), "STATISTICS")
        refused(lambda: s.set(0, name, np.zeros((s.nel(0), 6 if name.endswith("mean") else 7))), "STATISTICS")
        refused(lambda: s.array_devptr(0, name), "STATISTICS")
    refused(lambda: s.statistics_sample(0.1), "off")
    refused(s.statistics_reset, "off")
    refused(lambda: s.statistics_restore(1, 0.1), "off")
    refused(s.wall_statistics, "off")
    refused(lambda: s.bench_statistics("volume", 1), "off")
    for bad in (-1, 3):
        refused(lambda: s.set_statistics(bad), "mode")
    assert s.statistics() == off
    # mode 1
    s.set_statistics("volume")
    on = {"mode": "volume", "samples": 0, "wsum": 0.0}
    for w in (0.0, -1.0, float("nan"), float("inf")):
        refused(lambda: s.statistics_sample(w), "weight")
    for samples, wsum in ((-1, 1.0), (1, -1.0), (1, float("nan")), (1, float("inf")), (0, 1.0), (1, 0.0)):
        refused(lambda: s.statistics_restore(samples, wsum), "restore")
    refused(s.wall_statistics, "wall statistics")
    refused(lambda: s.set_wall_statistics(np.zeros((s.wall_node_count(0), 8))), "wall statistics")
    refused(lambda: s.bench_statistics("wall", 1), "wall statistics")
    refused(lambda: s.bench_statistics(2, 1), "kind")
    refused(lambda: s.get(1, "statistics_mean"), "STATISTICS")
    assert s.statistics() == on
    s.statistics_restore(0, 0.0)
    s.statistics_restore(3, 0.5)
    assert s.statistics() == {"mode": "volume", "samples": 3, "wsum": 0.5}
    s.statistics_reset()
    # a kernel-granular sweep under way
    s.sweep_begin(0)
    s.sweep_stage(0, 0, partials=False)
    refused(lambda: s.statistics_sample(0.1), "sweep is under way")
    refused(lambda: s.set_statistics("off"), "sweep is under way")
    refused(s.statistics_reset, "sweep is under way")
    s.sweep_stage(0, 1, partials=False)
    s.sweep_stage(0, 2, partials=False)
    s.statistics_sample(0.1)
    assert s.statistics()["samples"] == 1
    # the setting survives the other setters, and the mut column follows the eddy viscosity in effect
    s.set_viscous(1e-3, wall=True, levels=2)
    s.set_viscosity_model(eddy="field")
    s.set(0, "eddy_viscosity", np.full(s.nel(0), 2e-3))
    s.set_dual_time(0.1)
    s.set_free_stream(0.8, 2.0, reinitialise=False)
    assert s.statistics()["samples"] == 1
    s.statistics_reset()
    s.statistics_sample(0.1)
    _same(s.get(0, "statistics_mean")[:, 5], np.full(s.nel(0), 2e-3), "the mut column under the caller's field")
    s.set_dual_time(0.0)
    s.set_viscosity_model()
    s.set_viscous(0.0, levels=0)
    s.statistics_reset()
    s.statistics_sample(0.1)
    _same(s.get(0, "statistics_mean")[:, 5], np.zeros(s.nel(0)), "the mut column with the model off")
    s.set_statistics("off")
    # a group member
    g = mgcfd.Group([s])
    refused(lambda: s.set_statistics("volume"), "flow statistics")
    assert s.statistics() == off
    g.close()
    s.close(); mesh.close()
    # a partitioned solver
    from mgcfd.partition import partition_hierarchy, rcb_partition
    mesh = mgcfd.Mesh("input.dat", fse.case_input("m6_2lvl"), 1)
    levels = [mesh.level(l) for l in range(mesh.num_levels)]
    H = partition_hierarchy(levels, rcb_partition(np.asarray(levels[0]["coords"]).reshape(-1, 3), 2))
    lv, owned, keys = H[0].solver_args()
    t = mgcfd.Solver.from_arrays(lv, mesh.variant, n_owned=owned, order_keys=keys)
    refused(lambda: t.set_statistics("volume"), "flow statistics")
    refused(lambda: t.statistics_sample(0.1), "flow statistics")
    assert t.statistics() == off
    t.close()
    mesh.close()


# ---- the drop-in binary ----
def _run_driver(tmp, case, extra, cycles, ok=True):
    os.makedirs(tmp / "out", exist_ok=True)
    cmd = [EXE, "-i", "input.dat", "-d", fse.case_input(case), "-o", "out/", "-g", str(cycles), "-m", str(fse.case_duplicate(case))] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tmp)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    if not ok:
        assert r.returncode == 1, r.stdout + r.stderr
    return r


def _rows(path):
    lines = open(path).read().splitlines()
    assert lines[-1].startswith("# samples = ")
    return lines[0].split(","), np.array([[float(t) for t in l.split(",")] for l in lines[1:-1]]), lines[-1]


def test_driver_flags(lattices, tmp_path):
    """--output-statistics --statistics-start 1 (with --output-surface) on lattice A: the rows are the Python run's flow_statistics()
    at the file's %.17e, which reads back to the same doubles; the refusals exit with status 1 and write nothing."""
    import mgcfd
    case, steps = lattices["A"], 3
    dual = ["--physical-time-step", repr(DT), "--time-steps", str(steps)]
    r = _run_driver(tmp_path / "run", case, dual + ["--output-statistics", "--statistics-start", "1", "--output-surface"], CYCLES)
    plain = _run_driver(tmp_path / "plain", case, dual, CYCLES)
    strip = lambda out: [l for l in out.splitlines() if not l.startswith("Total runtime")]
    assert strip(r.stdout) == strip(plain.stdout)
    mesh, s = _solver(case)
    s.set_dual_time(DT)
    s.advance(1, CYCLES)
    s.set_statistics("wall")
    s.advance(steps - 1, CYCLES)
    fs, st = s.flow_statistics(), s.statistics()
    head, rows, last = _rows(tmp_path / "run" / "out" / "statistics.size=1x.level=0")
    assert head == "node,x,y,z,rho,u,v,w,p,mut,Ruu,Rvv,Rww,Ruv,Ruw,Rvw,p_rms,k".split(",")
    assert last == "# samples = %d, wsum = %.17e" % (st["samples"], st["wsum"]) and st["samples"] == steps - 1
    assert np.array_equal(rows[:, 0], np.arange(s.nel(0)))
    _same(rows[:, 4:10], fs["mean"], "driver: means")
    _same(rows[:, 10:16], fs["reynolds"], "driver: Reynolds stresses")
    _same(rows[:, 16], fs["p_rms"], "driver: p_rms")
    _same(rows[:, 17], fs["k"], "driver: k")
    assert fs["k"].max() > 0.0
    ids, table = s.wall_statistics()
    ff = s.far_field()
    v = ff[1:4] / ff[0]
    q = 0.5 * ff[0] * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    head, rows, last = _rows(tmp_path / "run" / "out" / "surface_statistics.size=1x.level=0")
    assert head == "node,x,y,z,Cp_mean,Cfx_mean,Cfy_mean,Cfz_mean,Cp_rms,Cfx_rms,Cfy_rms,Cfz_rms".split(",")
    assert np.array_equal(rows[:, 0].astype(np.int64), ids)
    _same(rows[:, 4], table[:, 0] / q, "driver: mean Cp")
    _same(rows[:, 8], np.sqrt(table[:, 4] / np.float64(st["wsum"])) / q, "driver: rms Cp")
    s.close(); mesh.close()
    assert not [n for n in os.listdir(tmp_path / "plain" / "out") if "statistics" in n]
    for tag, bad in (("no_dual_time", ["--output-statistics"]), ("start_without", dual + ["--statistics-start", "1"]),
                     ("start_too_late", dual + ["--output-statistics", "--statistics-start", str(steps)]),
                     ("bad_start", dual + ["--output-statistics", "--statistics-start", "-1"]),
                     ("several_gpus", dual + ["--output-statistics", "--gpus", "2"])):
        _run_driver(tmp_path / tag, case, bad, CYCLES, ok=False)
        assert not [n for n in os.listdir(tmp_path / tag / "out") if "statistics" in n], tag
