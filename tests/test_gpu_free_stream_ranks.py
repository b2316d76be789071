"""GPU tests of the run-time free stream on partitioned levels and in the drop-in binary: an in-process group of three parts
on this one GPU against ONE solver, the group's agreement rule, a one-rank RCCL solver replaying its sweep graphs after a
change, and euler3d_gpu_double --mach / --alpha / --polar against the composed oracle (tests/free_stream_emulator.py) and
Solver.polar."""
import os
import subprocess

import numpy as np
import pytest

import free_stream_emulator as fse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
CASES, PAIRS, K = fse.GPU_CASES, fse.GPU_PAIRS, fse.GPU_CYCLES
REF = (0.25, -0.125, 0.375)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: {got} != {want}"


def _levels(case):
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    levels = [mesh.level(l) for l in range(mesh.num_levels)]
    for L in levels:
        if np.size(L["coords"]) == 0:                         # (a single-level fvcorr input has no .coords file)
            L["coords"] = None
    return mesh, levels, mesh.variant


def _group(levels, variant, part0):
    import mgcfd
    from mgcfd.partition import partition_hierarchy
    H = partition_hierarchy(levels, part0)
    solvers = []
    for h in H:
        lv, owned, keys = h.solver_args()
        solvers.append(mgcfd.Solver.from_arrays(lv, variant, n_owned=owned, order_keys=keys))
    g = mgcfd.Group(solvers)
    for h, s in zip(H, solvers):
        for l in range(len(levels)):
            s.rank_set_halo(l, h.levels[l])
            s.rank_set_wall_slots(l, h.levels[l])
    for l in range(len(levels)):
        g.exchange(l)
    return H, solvers, g


def _part3(levels):
    from mgcfd.partition import rcb_partition
    c = levels[0].get("coords")
    if c is None:
        return (np.arange(levels[0]["nel"]) * 3) // levels[0]["nel"]
    return rcb_partition(np.asarray(c).reshape(-1, 3), 3)


@pytest.mark.parametrize("case", CASES)
def test_group_of_three_parts_equals_one_solver(case):
    """Group.set_free_stream then Group.cycles(loads=True): owned nodes of every level and the loads history bitwise the
    one-solver run's, cold at A and warm at B.  (The RMS of a group is summed rank by rank: the parity tolerance, as in
    tests/test_gpu_partitioned_loads.py.)"""
    import mgcfd
    a, b = PAIRS
    mesh, levels, variant = _levels(case)
    whole = mgcfd.Solver.from_arrays(levels, variant)
    H, solvers, g = _group(levels, variant, _part3(levels))
    for pair, reinit in ((a, True), (b, False)):
        whole.set_free_stream(*pair, reinitialise=reinit)
        g.set_free_stream(*pair, reinitialise=reinit)
        for s in solvers:
            assert s.free_stream() == pair
            _same(s.far_field(), whole.far_field(), "a rank's far field")
        want_rms, want = whole.run_cycles(K, loads=True, ref_point=REF)
        rms, hist = g.cycles(K, loads=True, ref_point=REF)
        _same(hist, want, f"{case} {pair}: loads history")
        assert np.allclose(rms, want_rms, rtol=1e-12, atol=0)
        for h, s in zip(H, solvers):
            for l in range(len(levels)):
                P = h.levels[l]
                _same(s.get(l, "variables")[:P.n_owned], whole.get(l, "variables")[P.global_ids[:P.n_owned]], f"{case} {pair}: rank {h.rank} level {l}")
        _same(g.surface_loads(0, REF), whole.surface_loads(0, REF), f"{case} {pair}: surface_loads")
    g.close()
    for s in solvers:
        s.close()
    whole.close()
    mesh.close()


def test_group_refuses_ranks_that_disagree():
    import mgcfd
    mesh, levels, variant = _levels("m6_2lvl")
    H, solvers, g = _group(levels, variant, _part3(levels))
    g.set_free_stream(*PAIRS[0])
    g.cycles(1)
    solvers[1].set_free_stream(*PAIRS[1], reinitialise=False)
    for call in (lambda: g.cycles(1), lambda: g.cycles(1, loads=True), lambda: g.sweeps(0, 1), lambda: g.sweeps_rms(0, 1),
                 lambda: g.surface_loads(0)):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1 and "rank 1" in str(e.value) and "free stream" in str(e.value)
    with pytest.raises(mgcfd.MgcfdError) as e:
        g.set_free_stream(0.0, 0.0)
    assert e.value.code == 1
    solvers[1].set_free_stream(*PAIRS[0], reinitialise=False)
    g.cycles(1)                                               # in line again
    g.close()
    for s in solvers:
        s.close()
    mesh.close()


def test_one_rank_rccl_solver_replays_its_graphs_after_a_change():
    """MGCFD_OPT_GRAPH on an RCCL rank: sweeps at A, set B, sweeps again — bitwise the same sequence on a plain solver without
    graphs; mgcfd_rank_graph_status shows the graphs dropped by the change, captured again, and sweeps replayed after it."""
    import mgcfd
    from mgcfd.partition import partition_level, rcb_partition
    a, b = PAIRS
    mesh, levels, variant = _levels("fvcorr_1lvl")
    L = levels[0]
    n = fse.SWEEPS
    ref = mgcfd.Solver.from_arrays([L], variant)
    ref.set_free_stream(*a)
    ref.smooth(0, n)
    want_a = ref.get(0, "variables")
    ref.set_free_stream(*b, reinitialise=False)
    ref.smooth(0, n)
    want_b = ref.get(0, "variables")
    ref.close()
    P = partition_level(L, np.zeros(L["nel"], dtype=np.int64))[0]
    s = mgcfd.Solver.from_arrays([P.level], variant, n_owned=[P.n_owned])
    s.rank_attach_rccl(0, 1, mgcfd.rccl_unique_id())
    s.rank_set_halo(0, P)
    s.set_option("graph", 1)
    s.set_free_stream(*a)
    s.rank_exchange(0)
    s.rank_sweeps(0, n)
    _same(s.get(0, "variables")[:P.n_owned], want_a[P.global_ids[:P.n_owned]], "sweeps at A")
    st_a = s.rank_graph_status(0)
    assert st_a["graphs"] >= 1 and not st_a["capture_refused"] and st_a["sweeps_replayed"] >= 1, st_a
    s.set_free_stream(*b, reinitialise=False)
    assert s.rank_graph_status(0)["graphs"] == 0, "the change of free stream drops the rank's sweep graphs"
    s.rank_sweeps(0, n)
    st_b = s.rank_graph_status(0)
    assert st_b["graphs"] >= 1 and not st_b["capture_refused"] and st_b["sweeps_replayed"] > st_a["sweeps_replayed"], (st_a, st_b)
    _same(s.get(0, "variables")[:P.n_owned], want_b[P.global_ids[:P.n_owned]], "sweeps replayed at B")
    s.rank_detach()
    s.close()
    mesh.close()


def _child(mode, out, env=None):
    """tests/free_stream_children.py in a process of its own (it makes a process group of its own)."""
    import sys
    r = subprocess.run([sys.executable, "-s", os.path.join(ROOT, "tests", "free_stream_children.py"), mode, str(out)],
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


def test_distributed_helper_under_the_nccl_backend(tmp_path):
    """distributed.set_free_stream_all on a one-rank RCCL process group (backend "nccl" refuses host tensors): the solver gets
    the far field of rank 0's pair.  (Two ranks: tests/test_distributed_free_stream.py, on gloo.)"""
    got = _child("nccl_helper", tmp_path / "ff.npy")
    _same(got, fse.free_stream_constants(*PAIRS[0]), "far field set through the nccl backend")


def _run_driver(tmp, case, extra, cycles=K):
    os.makedirs(tmp / "out", exist_ok=True)
    cmd = [EXE, "-i", "input.dat", "-d", fse.case_input(case), "-o", "out/", "-g", str(cycles), "-m", str(fse.case_duplicate(case))] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tmp)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _strip(out):
    return [l for l in out.splitlines() if not l.startswith("Total runtime = ")]


@pytest.mark.parametrize("case", CASES)
def test_driver_dump_equals_the_composed_oracle(case, oracle, tmp_path):
    """--mach M --alpha A --output-variables --output-loads: the dump is the %.17e rendering of the composed oracle's state,
    byte for byte, on one GPU and with --gpus 2 --gpus-partition --gpus-share-device; stdout has the plain run's lines."""
    dup = fse.case_duplicate(case)
    name = f"variables.size={dup}x.cycles={K}.level=0"
    plain = _run_driver(tmp_path / "plain", case, ["--output-variables"])
    for pair in PAIRS:
        co = fse.ComposedOracle(oracle, case, fse.free_stream_constants(*pair))
        rc, want_rms = co.cycles(K)
        assert rc == 0
        want = fse.render_variables(co.variables(0)).encode()
        co.close()
        opts = ["--mach", repr(pair[0]), "--alpha", repr(pair[1]), "--output-variables", "--output-loads"]
        for tag, extra in (("one", []), ("two", ["--gpus", "2", "--gpus-partition", "--gpus-share-device"])):
            d = tmp_path / f"{tag}_{pair[0]}"
            r = _run_driver(d, case, opts + extra)
            assert (d / "out" / name).read_bytes() == want, f"{case} {pair} {tag}"
            lines, plain_lines = _strip(r.stdout), _strip(plain.stdout)
            assert len(lines) == len(plain_lines)
            for got, ref in zip(lines, plain_lines):           # the reference's lines, nothing added (the RMS figures are this flow's)
                assert got.split("(RMS")[0] == ref.split("(RMS")[0]
            rms_lines = [l for l in lines if "(RMS = " in l]
            assert rms_lines == [(f"Cycle {i + 1} / {K}" if co.n <= 1 else f"MG cycle {i + 1} / {K}") + " (RMS = %.3e)" % want_rms[i] for i in range(K)]
            assert sorted(os.listdir(d / "out")) == sorted(os.listdir(tmp_path / "plain" / "out") + [f"surface_loads.size={dup}x.cycles={K}.level=0"])


def test_driver_without_the_new_options_is_the_golden_run(tmp_path):
    golden = os.path.join(ROOT, "tests", "golden", "m6_2lvl", "variables.level0.txt")
    _run_driver(tmp_path, "m6_2lvl", ["--output-variables"])
    assert (tmp_path / "out" / f"variables.size=1x.cycles={K}.level=0").read_bytes() == open(golden, "rb").read()
    assert "polar.csv" not in os.listdir(tmp_path / "out")


@pytest.mark.parametrize("gpus", [[], ["--gpus", "2", "--gpus-partition", "--gpus-share-device"]])
def test_driver_polar_equals_solver_polar(gpus, tmp_path):
    import mgcfd
    case, mach, alphas = fse.POLAR_CASE, fse.POLAR_MACH, fse.POLAR_ALPHAS
    a0, a1, n = alphas[0], alphas[-1], len(alphas)
    assert alphas == [a0 + (a1 - a0) * k / (n - 1) for k in range(n)]
    S, c, ref = 0.7532, 0.64607, (0.5, 0.25, -0.125)
    plain = _run_driver(tmp_path / "plain", case, ["--output-variables"])
    r = _run_driver(tmp_path / "polar", case, ["--mach", repr(mach), f"--polar={a0}:{a1}:{n}", "--output-variables",
                                                f"--loads-reference={S},{c},{ref[0]},{ref[1]},{ref[2]}"] + gpus)
    assert len(_strip(r.stdout)) == len(_strip(plain.stdout))
    out = tmp_path / "polar" / "out"
    assert sorted(os.listdir(out)) == sorted(os.listdir(tmp_path / "plain" / "out") + ["polar.csv"])
    lines = (out / "polar.csv").read_text().splitlines()
    assert lines[0] == "alpha,mach,rms_last,Fx,Fy,Fz,Mx,My,Mz,CD,CL,CS,CMx,CMy,CMz"
    rows = np.array([[float(v) for v in l.split(",")] for l in lines[1:]])
    assert rows.shape == (n, 15)
    mesh = mgcfd.Mesh("input.dat", fse.case_input(case), fse.case_duplicate(case))
    s = mgcfd.Solver.from_mesh(mesh)
    pol = s.polar(alphas, K, mach=mach, warm_start=True, ref_point=ref, ref_area=S, ref_length=c)
    for row, p in zip(rows, pol):
        _same(row[:2], [p["alpha"], p["mach"]], "alpha, mach")
        _same(row[3:9], p["loads"][-1], "loads of the last cycle")
        _same(row[9:], p["coefficients"], "coefficients")
        if gpus:
            assert np.isclose(row[2], p["rms"][-1], rtol=1e-12, atol=0)
        else:
            _same(row[2:3], p["rms"][-1:], "rms_last")
    # the dump is the last angle's state
    assert (out / f"variables.size=1x.cycles={K}.level=0").read_bytes() == fse.render_variables(s.get(0, "variables")).encode()
    s.close()
    mesh.close()
