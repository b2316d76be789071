"""GPU tests of the surface loads (mgcfd_surface_loads, mgcfd_run_cycles_loads, euler3d_gpu_double --output-loads): bit for
bit against the numpy emulator of the definition (tests/surface_loads_emulator.py) applied to the oracle's state, and
the cycles themselves unchanged by recording them."""
import os
import subprocess

import numpy as np
import pytest

import surface_loads_emulator as emu
from conftest import perturbed_state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
CASES = ["m6_2lvl", "m6_3lvl", "m6_2lvl_dup2", "mixed_2lvl", "tet_2lvl", "fvcorr_1lvl"]
REF = (0.25, -0.125, 0.375)


def _dup(case):
    meta = dict(l.strip().split(" = ") for l in open(os.path.join(GOLDEN, case, "case.txt")))
    return int(meta["duplicate"])


def _input(case):
    return os.path.join(GOLDEN, case, "input")


def _solver(mgcfd, case):
    mesh = mgcfd.Mesh("input.dat", _input(case), _dup(case))
    return mesh, mgcfd.Solver.from_mesh(mesh)


def _walls(solver, mesh, level):
    """The level's solid-wall edges as mgcfd_get_edges returns them, and its coordinates."""
    d = mesh.level(level)
    e = solver.get_edges(level, d["n_edges"])
    return e[d["boundary_start"]:d["boundary_start"] + d["n_boundary"]], d["coords"]


def _emulate(solver, mesh, level, variables, ref=REF):
    walls, coords = _walls(solver, mesh, level)
    return emu.surface_loads(variables, walls, coords, solver.far_field(), ref)


def _oracle_state(oracle, case, cycles):
    oc = oracle.OracleCase.from_input_dat(os.path.join(_input(case), "input.dat"), _dup(case))
    rc, _, _ = oc.solve(cycles)
    assert rc == 0
    v = oc.array(0, "variables").reshape(-1, 5).copy()
    oc.close()
    return v


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("case", CASES)
def test_loads_history_matches_the_emulator_on_the_oracle_state(case, oracle):
    import mgcfd
    states = [_oracle_state(oracle, case, c + 1) for c in range(3)]
    mesh, probe = _solver(mgcfd, case)
    want = np.array([_emulate(probe, mesh, 0, states[c]) for c in range(3)])
    probe.close()
    if case != "fvcorr_1lvl":
        assert np.any(want != 0.0), "the case should carry solid-wall loads"
    for k in range(1, 4):
        mesh, s = _solver(mgcfd, case)
        rms, hist = s.run_cycles(k, loads=True, ref_point=REF)
        assert rms.shape == (k,) and hist.shape == (k, 6)
        for c in range(k):
            assert np.array_equal(hist[c], want[c]), f"k={k} cycle {c}: {hist[c]} != {want[c]}"
        s.close()


@pytest.mark.parametrize("case", CASES)
def test_loads_leave_the_solve_alone(case):
    import mgcfd
    k = 3
    histories = []
    for graph in (0, 1):
        for timing in (0, 4):
            runs = []
            for loads in (False, True):
                mesh, s = _solver(mgcfd, case)
                s.set_option("graph", graph)
                s.set_option("timing", timing)
                if loads:
                    rms, hist = s.run_cycles(k, loads=True, ref_point=REF)
                    histories.append(hist)
                else:
                    rms = s.run_cycles(k)
                runs.append((rms, [s.get(l, "variables") for l in range(s.num_levels)]))
                s.close()
            (rms0, v0), (rms1, v1) = runs
            assert np.array_equal(_bits(rms0), _bits(rms1)), f"graph={graph} timing={timing}: RMS differs"
            for l in range(len(v0)):
                assert np.array_equal(_bits(v0[l]), _bits(v1[l])), f"graph={graph} timing={timing}: level {l} differs"
    for h in histories[1:]:
        assert np.array_equal(_bits(h), _bits(histories[0]))


@pytest.mark.parametrize("case", ["m6_2lvl", "m6_3lvl", "tet_2lvl"])
def test_fast_mode_loads_match_the_emulator_on_the_gpu_state(case):
    import mgcfd
    mesh, s = _solver(mgcfd, case)
    s.set_option("exact", 0)
    for c in range(3):
        _, hist = s.run_cycles(1, loads=True, ref_point=REF)
        want = _emulate(s, mesh, 0, s.get(0, "variables"))
        assert np.array_equal(hist[0], want), f"cycle {c}"
        assert np.array_equal(s.surface_loads(0, REF), want)
    s.close()


def test_surface_loads_of_a_coarse_level():
    import mgcfd
    mesh, s = _solver(mgcfd, "m6_3lvl")
    s.run_cycles(2)
    for level in (1, 2):
        got = s.surface_loads(level, REF)
        assert np.array_equal(got, _emulate(s, mesh, level, s.get(level, "variables")))
        assert np.any(got != 0.0)
    # the default reference point is the origin
    assert np.array_equal(s.surface_loads(1), _emulate(s, mesh, 1, s.get(1, "variables"), (0.0, 0.0, 0.0)))
    s.close()


def test_a_level_without_solid_wall_gives_exact_zeros():
    import mgcfd
    from mgcfd import meshgen
    mg = meshgen.make_multigrid((9, 5), "m6wing", seed=4, cavity_radius=0.0, jitter=0.2)
    levels = mgcfd.generated_to_levels(mg)
    assert all(L["n_boundary"] == 0 for L in levels)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    got = s.surface_loads(0, REF)
    assert np.array_equal(_bits(got), _bits(np.zeros(6)))
    rms_plain = mgcfd.Solver.from_arrays(levels, mg.mesh_variant).run_cycles(2)
    rms, hist = s.run_cycles(2, loads=True, ref_point=REF)
    assert np.array_equal(_bits(hist), _bits(np.zeros((2, 6))))
    assert np.array_equal(_bits(rms), _bits(rms_plain))
    s.close()


def test_more_than_65536_solid_wall_edges_take_three_tree_stages(oracle):
    import mgcfd
    from mgcfd import meshgen
    mg = meshgen.make_multigrid((40,), "m6wing", seed=8, cavity_radius=0.2, jitter=0.2, area_noise=0.05)
    L = mgcfd.generated_to_levels(mg)[0]
    e, ni, nb, nw = L["edges"], L["n_internal"], L["n_boundary"], L["n_wall"]
    rng = np.random.default_rng(21)
    extra = np.zeros(2 * L["nel"], dtype=e.dtype)          # every node two more solid-wall faces
    extra["a"] = -1
    extra["b"] = np.tile(np.arange(L["nel"]), 2)
    for f in ("x", "y", "z"):
        extra[f] = rng.uniform(-1e-3, 1e-3, len(extra))
    L["edges"] = np.concatenate([e[:ni], e[ni:ni + nb], extra, e[ni + nb:]])
    L["n_boundary"] = nb + len(extra)
    assert L["n_boundary"] > 65536 and -(-L["n_boundary"] // 256) > 256
    s = mgcfd.Solver.from_arrays([L], mg.mesh_variant)
    ff = s.far_field()
    q = perturbed_state(L["nel"], ff[:5], seed=17)
    s.set(0, "variables", q)
    walls = s.get_edges(0, len(L["edges"]))[ni:ni + L["n_boundary"]]
    want = emu.surface_loads(q, walls, L["coords"], ff, REF)
    got = s.surface_loads(0, REF)
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(s.surface_loads(0, REF), got)          # and again: the arrival ticket reset itself
    s.close()


def test_a_partitioned_solver_refuses_loads():
    import mgcfd
    from mgcfd import meshgen
    mg = meshgen.make_multigrid((9,), "m6wing", seed=3, cavity_radius=0.15)
    levels = mgcfd.generated_to_levels(mg)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant, n_owned=[levels[0]["nel"]])
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.surface_loads(0)
    assert e.value.code == 1 and "partitioned" in str(e.value)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.run_cycles(1, loads=True)
    assert e.value.code == 1 and "partitioned" in str(e.value)
    s.close()


def _run_driver(tmp, extra):
    # (the same relative output prefix in two directories: the stdout lines that name the files are the same)
    os.makedirs(tmp / "out", exist_ok=True)
    cmd = [EXE, "-i", "input.dat", "-d", _input("m6_2lvl"), "-o", "out/", "-g", "3", "--output-variables"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=tmp)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_driver_output_loads(tmp_path):
    import mgcfd
    S, c, ref = 0.7532, 0.64607, (0.5, 0.25, -0.125)
    plain = _run_driver(tmp_path / "plain", [])
    with_loads = _run_driver(tmp_path / "loads", ["--output-loads", f"--loads-reference={S},{c},{ref[0]},{ref[1]},{ref[2]}"])
    # stdout and every dump as without the flag (the total runtime aside, which no two runs share)
    strip = lambda out: [l for l in out.splitlines() if not l.startswith("Total runtime = ")]
    assert strip(with_loads.stdout) == strip(plain.stdout)
    name = "variables.size=1x.cycles=3.level=0"
    plain_out, loads_out = tmp_path / "plain" / "out", tmp_path / "loads" / "out"
    assert (loads_out / name).read_bytes() == (plain_out / name).read_bytes()
    # LoopNumIters.csv: the same bytes but for CpuId, the host core each run happened to be on
    def iters(path):
        head, row = [l.split(",") for l in path.read_text().splitlines()]
        return [(h, v) for h, v in zip(head, row) if h != "CpuId"]
    assert iters(loads_out / "LoopNumIters.csv") == iters(plain_out / "LoopNumIters.csv")
    assert sorted(os.listdir(loads_out)) == sorted(os.listdir(plain_out) + ["surface_loads.size=1x.cycles=3.level=0"])
    lines = (loads_out / "surface_loads.size=1x.cycles=3.level=0").read_text().splitlines()
    assert lines[0] == "cycle,Fx,Fy,Fz,Mx,My,Mz,CD,CL,CS,CMx,CMy,CMz"
    rows = [l.split(",") for l in lines[1:]]
    assert [int(r[0]) for r in rows] == [1, 2, 3]
    assert all(len(r) == 13 and all("e" in v for v in r[1:]) for r in rows)
    got = np.array([[float(v) for v in r[1:]] for r in rows])
    mesh, s = _solver(mgcfd, "m6_2lvl")
    _, hist = s.run_cycles(3, loads=True, ref_point=ref)
    assert np.array_equal(got[:, :6], hist)
    assert np.array_equal(got[:, 6:], s.load_coefficients(hist, S, c))
    assert np.allclose(got[:, 6:], np.array([emu.coefficients(s.far_field(), h, S, c) for h in hist]), rtol=1e-14, atol=0)
    s.close()
