"""GPU tests of the surface loads over a partitioned level (mgcfd_rank_set_wall_slots, mgcfd_group_surface_loads,
mgcfd_group_cycles_loads, mgcfd_rank_surface_loads, mgcfd_rank_cycles_loads, euler3d_gpu_double --gpus N --gpus-partition
--output-loads): the ranks of a group on this one GPU against ONE solver that holds the whole hierarchy and against the numpy
emulator of the definition (tests/surface_loads_emulator.py).  Every comparison is on the int64 views of the doubles: the
loads of a level split over ranks are the whole level's bit for bit, the sign of a zero included."""
import os
import subprocess
import types

import numpy as np
import pytest

import surface_loads_emulator as emu
from conftest import perturbed_state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")
REF = (0.25, -0.125, 0.375)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(got, want, what):
    assert np.array_equal(_bits(got), _bits(want)), f"{what}: {got} != {want}"


def _hierarchy(sizes=(24, 12, 6), cavity_radius=0.3, seed=4):
    import mgcfd
    from mgcfd import meshgen
    mg = meshgen.make_multigrid(sizes, "m6wing", seed=seed, jitter=0.2, area_noise=0.05, volume_noise=0.05, cavity_radius=cavity_radius)
    return mgcfd.generated_to_levels(mg), mg.mesh_variant


def _part0(levels, split, n_parts):
    from mgcfd.partition import rcb_partition, slab_partition
    return {"rcb": rcb_partition, "slab": slab_partition}[split](np.asarray(levels[0]["coords"]), n_parts)


def _group_over(levels, mesh_variant, part0, slots=True, exact=True):
    import mgcfd
    from mgcfd.partition import partition_hierarchy
    H = partition_hierarchy(levels, part0)
    solvers = []
    for h in H:
        lv, owned, keys = h.solver_args()
        s = mgcfd.Solver.from_arrays(lv, mesh_variant, n_owned=owned, order_keys=keys)
        s.set_option("exact", int(exact))
        solvers.append(s)
    g = mgcfd.Group(solvers)
    for h, s in zip(H, solvers):
        for l in range(len(levels)):
            s.rank_set_halo(l, h.levels[l])
            if slots:
                s.rank_set_wall_slots(l, h.levels[l])
    for l in range(len(levels)):
        g.exchange(l)
    return H, solvers, g


def _close(g, solvers):
    g.close()
    for s in solvers:
        s.close()


def _emulate(whole, levels, l, ref=REF):
    L = levels[l]
    ni, nb = L["n_internal"], L["n_boundary"]
    walls = whole.get_edges(l, len(L["edges"]))[ni:ni + nb]
    return emu.surface_loads(whole.get(l, "variables"), walls, L["coords"], whole.far_field(), ref)


def _owned_state(H, solvers, n_levels):
    return [[(s.get(l, "variables")[:h.levels[l].n_owned], s.get(l, "residuals")[:h.levels[l].n_owned]) for l in range(n_levels)]
            for h, s in zip(H, solvers)]


@pytest.mark.parametrize("threads", ["0", "1"])
@pytest.mark.parametrize("split,n_parts", [("rcb", 3), ("rcb", 5), ("slab", 6)])
def test_group_loads_history_and_every_level_equal_the_whole(monkeypatch, threads, split, n_parts):
    import mgcfd
    monkeypatch.setenv("MGCFD_GROUP_THREADS", threads)
    levels, variant = _hierarchy()
    part0 = _part0(levels, split, n_parts)
    # what makes the case a test of the ORDER: several chunks of 256, a chunk whose edges belong to several ranks — and, in
    # slabs, a rank that owns no solid-wall edge at all
    L0 = levels[0]
    ni, nb = L0["n_internal"], L0["n_boundary"]
    owner = part0[L0["edges"]["b"][ni:ni + nb]]
    assert -(-nb // 256) >= 2
    assert max(len(np.unique(owner[k:k + 256])) for k in range(0, nb, 256)) >= 2
    if split == "slab":
        assert len(np.unique(owner)) < n_parts, "a rank without a solid-wall edge"

    whole = mgcfd.Solver.from_arrays(levels, variant)
    want_rms, want = whole.run_cycles(3, loads=True, ref_point=REF)
    assert np.any(want != 0.0)

    H, solvers, g = _group_over(levels, variant, part0)
    rms, hist = g.cycles(3, loads=True, ref_point=REF)
    assert hist.shape == (3, 6)
    print("loads of the group", hist, "of the whole", want)
    _same_bits(hist, want, f"{split} {n_parts}, threads {threads}: history")
    assert np.allclose(rms, want_rms, rtol=1e-12, atol=0.0)

    # every level, the ticket resetting itself
    for l in range(len(levels)):
        one = whole.surface_loads(l, REF)
        _same_bits(one, _emulate(whole, levels, l), f"level {l}: the whole solver against the emulator")
        for again in range(2):
            _same_bits(g.surface_loads(l, REF), one, f"level {l}, call {again}")
    _same_bits(g.surface_loads(1), whole.surface_loads(1), "the default reference point")
    with pytest.raises(mgcfd.MgcfdError) as e:
        solvers[0].surface_loads(0)
    assert e.value.code == 1 and "partitioned" in str(e.value)
    state = _owned_state(H, solvers, len(levels))
    _close(g, solvers)
    whole.close()

    # recording the loads leaves the cycles alone
    H, solvers, g = _group_over(levels, variant, part0, slots=False)
    _same_bits(g.cycles(3), rms, "RMS with and without loads")
    plain = _owned_state(H, solvers, len(levels))
    for r in range(n_parts):
        for l in range(len(levels)):
            _same_bits(state[r][l][0], plain[r][l][0], f"rank {r} level {l}: variables")
            _same_bits(state[r][l][1], plain[r][l][1], f"rank {r} level {l}: residuals")
    _close(g, solvers)


def test_three_tree_stages_across_ranks():
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
    whole = mgcfd.Solver.from_arrays([L], mg.mesh_variant)
    ff = whole.far_field()
    walls = whole.get_edges(0, len(L["edges"]))[ni:ni + L["n_boundary"]]
    whole.close()
    q = perturbed_state(L["nel"], ff[:5], seed=17)
    want = emu.surface_loads(q, walls, L["coords"], ff, REF)
    H, solvers, g = _group_over([L], mg.mesh_variant, _part0([L], "rcb", 3))
    for h, s in zip(H, solvers):
        s.set(0, "variables", q[h.levels[0].global_ids])
    for again in range(2):
        _same_bits(g.surface_loads(0, REF), want, f"call {again}")
    _close(g, solvers)


def test_fast_mode_histories_are_equal():
    """MGCFD_OPT_EXACT = 0 on every rank against the whole hierarchy swept by the kernel the partitioned stages run (variant 1):
    the same operations, so the same state — and the loads are never contracted, whatever the option says."""
    import mgcfd
    levels, variant = _hierarchy((12, 6, 3), seed=9)
    whole = mgcfd.Solver.from_arrays(levels, variant)
    whole.set_option("exact", 0)
    whole.set_option("flux_variant", 1)
    _, want = whole.run_cycles(2, loads=True, ref_point=REF)
    _same_bits(whole.surface_loads(0, REF), _emulate(whole, levels, 0), "the whole solver against the emulator")
    whole.close()
    assert np.any(want != 0.0)
    H, solvers, g = _group_over(levels, variant, _part0(levels, "rcb", 3), exact=False)
    _, hist = g.cycles(2, loads=True, ref_point=REF)
    _same_bits(hist, want, "fast mode")
    _close(g, solvers)


def test_no_solid_wall_gives_positive_zeros():
    levels, variant = _hierarchy((9, 5), cavity_radius=0.0)
    assert all(L["n_boundary"] == 0 for L in levels)
    part0 = _part0(levels, "rcb", 3)
    H, solvers, g = _group_over(levels, variant, part0)
    rms, hist = g.cycles(2, loads=True, ref_point=REF)
    _same_bits(hist, np.zeros((2, 6)), "history")
    _same_bits(g.surface_loads(0, REF), np.zeros(6), "one call")
    _close(g, solvers)
    H, solvers, g = _group_over(levels, variant, part0, slots=False)
    _same_bits(g.cycles(2), rms, "RMS as without loads")
    _close(g, solvers)


def test_refusals_name_the_wall_slots_and_leave_the_group_usable():
    import mgcfd
    levels, variant = _hierarchy((12, 6, 3))
    H, solvers, g = _group_over(levels, variant, _part0(levels, "rcb", 3), slots=False)
    parts = [h.levels[0] for h in H]
    assert all(len(P.wall_slots) >= 2 for P in parts)
    fake = lambda slots, total: types.SimpleNamespace(wall_slots=np.asarray(slots, dtype=np.int64), wall_total=total)

    def refused(call):
        with pytest.raises(mgcfd.MgcfdError) as e:
            call()
        assert e.value.code == 1 and "wall slots" in str(e.value), str(e.value)
        assert g.cycles(1).shape == (1,)                  # the group goes on

    def set_all():
        for P, s in zip(parts, solvers):
            s.rank_set_wall_slots(0, P)

    # no slots on one rank
    solvers[0].rank_set_wall_slots(0, parts[0])
    solvers[2].rank_set_wall_slots(0, parts[2])
    refused(lambda: g.cycles(1, loads=True))
    refused(lambda: g.surface_loads(0))
    set_all()
    # a count that differs from the local n_boundary, slots not ascending or outside the whole level
    P = parts[1]
    refused(lambda: solvers[1].rank_set_wall_slots(0, fake(P.wall_slots[:-1], P.wall_total)))
    swapped = P.wall_slots.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    refused(lambda: solvers[1].rank_set_wall_slots(0, fake(swapped, P.wall_total)))
    refused(lambda: solvers[1].rank_set_wall_slots(0, fake(P.wall_slots, int(P.wall_slots[-1]))))
    # two ranks naming one slot
    k = next(k for k in range(len(P.wall_slots)) if P.wall_slots[k] > 0 and P.wall_slots[k] - 1 not in P.wall_slots)
    twice = P.wall_slots.copy()
    twice[k] -= 1
    solvers[1].rank_set_wall_slots(0, fake(twice, P.wall_total))
    refused(lambda: g.cycles(1, loads=True))
    set_all()
    # different n_total
    solvers[2].rank_set_wall_slots(0, fake(parts[2].wall_slots, parts[2].wall_total + 1))
    refused(lambda: g.surface_loads(0))
    set_all()
    # a whole solver takes no slots; a member still refuses the one-solver call
    with pytest.raises(mgcfd.MgcfdError) as e:
        solvers[0].surface_loads(0)
    assert e.value.code == 1 and "partitioned" in str(e.value)
    rms, hist = g.cycles(1, loads=True, ref_point=REF)
    assert np.all(np.isfinite(hist)) and np.any(hist != 0.0)
    _close(g, solvers)
    whole = mgcfd.Solver.from_arrays(levels, variant)
    with pytest.raises(mgcfd.MgcfdError) as e:
        whole.rank_set_wall_slots(0, parts[0])
    assert e.value.code == 1 and "wall slots" in str(e.value)
    whole.close()


def test_rank_loads_over_rccl_with_one_rank():
    """The RCCL form with the one rank this box offers: the agreement on the counts, the terms, the reduce (no message)."""
    import mgcfd
    from mgcfd.partition import partition_hierarchy
    levels, variant = _hierarchy((12, 6, 3))
    whole = mgcfd.Solver.from_arrays(levels, variant)
    want_rms, want = whole.run_cycles(3, loads=True, ref_point=REF)
    want_levels = [whole.surface_loads(l, REF) for l in range(len(levels))]
    whole.close()
    H = partition_hierarchy(levels, np.zeros(levels[0]["nel"], dtype=np.int64))
    lv, owned, keys = H[0].solver_args()
    s = mgcfd.Solver.from_arrays(lv, variant, n_owned=owned, order_keys=keys)
    s.rank_attach_rccl(0, 1, mgcfd.rccl_unique_id())
    for l in range(len(levels)):
        s.rank_set_halo(l, H[0].levels[l])
        s.rank_exchange(l)
    with pytest.raises(mgcfd.MgcfdError) as e:
        s.rank_cycles(1, loads=True)
    assert e.value.code == 1 and "wall slots" in str(e.value)
    for l in range(len(levels)):
        s.rank_set_wall_slots(l, H[0].levels[l])
    rms, hist = s.rank_cycles(3, loads=True, ref_point=REF)
    _same_bits(hist, want, "history")
    assert np.allclose(rms, want_rms, rtol=1e-12, atol=0.0)
    for l in range(len(levels)):
        for again in range(2):
            _same_bits(s.rank_surface_loads(l, REF), want_levels[l], f"level {l}, call {again}")
    s.rank_detach()
    s.close()


def _case(case):
    meta = dict(l.strip().split(" = ") for l in open(os.path.join(GOLDEN, case, "case.txt")))
    return os.path.join(GOLDEN, case, "input"), int(meta["duplicate"])


def _run_driver(tmp, case, extra):
    # (the same relative output prefix in every directory: the stdout lines that name the files are the same)
    d, dup = case if isinstance(case, tuple) else _case(case)
    os.makedirs(tmp / "out", exist_ok=True)
    cmd = [EXE, "-i", "input.dat", "-d", d, "-o", "out/", "-g", "3", "-m", str(dup), "--output-variables"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=tmp)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _driver_three_ways(case, tmp_path):
    """One GPU with loads, three ranks without, three ranks with: the loads file is the one-GPU run's byte for byte, stdout and
    the variables dump those of the three ranks without the flag.  Returns the six loads of every cycle."""
    loads = ["--output-loads", "--loads-reference=0.7532,0.64607,0.5,0.25,-0.125"]
    gpus = ["--gpus", "3", "--gpus-share-device", "--gpus-partition"]
    one = _run_driver(tmp_path / "one", case, loads)
    plain = _run_driver(tmp_path / "plain", case, gpus)
    both = _run_driver(tmp_path / "both", case, gpus + loads)
    assert "3 ranks" in both.stderr and "partitioned" in both.stderr
    strip = lambda out: [l for l in out.splitlines() if not l.startswith("Total runtime = ")]
    assert strip(both.stdout) == strip(plain.stdout)
    out = {k: tmp_path / k / "out" for k in ("one", "plain", "both")}
    names = [n for n in os.listdir(out["one"]) if n.startswith("surface_loads.")]
    assert len(names) == 1
    assert sorted(os.listdir(out["both"])) == sorted(os.listdir(out["plain"]) + names)
    assert (out["both"] / names[0]).read_bytes() == (out["one"] / names[0]).read_bytes()
    dumps = [n for n in os.listdir(out["plain"]) if n.startswith("variables.")]
    assert len(dumps) == 1
    assert (out["both"] / dumps[0]).read_bytes() == (out["plain"] / dumps[0]).read_bytes()
    rows = np.array([[float(v) for v in l.split(",")[1:7]] for l in (out["both"] / names[0]).read_text().splitlines()[1:]])
    assert rows.shape == (3, 6)
    return rows


@pytest.mark.parametrize("case", ["m6_3lvl", "m6_2lvl_dup2", "fvcorr_1lvl"])
def test_driver_output_loads_on_partitioned_levels(case, tmp_path):
    """fvcorr_1lvl is the single-level input (mgcfd_group_cycles_loads on a hierarchy of one level).  Its level has six
    solid-wall edges (tests/golden/fvcorr_1lvl/kernels.npz: L0_sizes), so its rows are not zeros: they are the one-GPU run's,
    byte for byte.  The level without any solid wall is the next test's."""
    assert np.any(_driver_three_ways(case, tmp_path) != 0.0)


def test_driver_on_a_single_level_without_solid_wall_writes_zeros(tmp_path):
    from mgcfd import meshgen
    mg = meshgen.make_multigrid((9,), "m6wing", seed=4, cavity_radius=0.0, jitter=0.2)
    assert mg.levels[0].nel > 0
    d = tmp_path / "input"
    os.makedirs(d)
    meshgen.write_input(mg, str(d))
    _same_bits(_driver_three_ways((str(d), 1), tmp_path), np.zeros((3, 6)), "no solid wall")
