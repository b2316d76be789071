"""CPU tests of the surface loads over a partitioned level: the wall slots both Python partitioners hand to
mgcfd_rank_set_wall_slots (every solid-wall edge of the whole level named exactly once, in the whole level's order), and
the driver's command line (--output-loads with --gpus N needs --gpus-partition)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "mg-cfd-app-plain_amd", "csrc", "euler3d_gpu_double")


@pytest.fixture(scope="module")
def mgcfd_mod():
    import mgcfd
    if not os.path.exists(mgcfd.LIB_PATH) or not os.path.exists(EXE):
        import __graft_entry__
        __graft_entry__.build()
    return mgcfd


def _levels():
    import mgcfd
    from mgcfd import meshgen
    mg = meshgen.make_multigrid((24, 12, 6), "m6wing", seed=4, jitter=0.2, area_noise=0.05, volume_noise=0.05, cavity_radius=0.3)
    return mgcfd.generated_to_levels(mg)


def _check_parts(whole, parts):
    """parts: the LevelParts of ONE level, a rank each."""
    ni, nb = int(whole["n_internal"]), int(whole["n_boundary"])
    named = np.zeros(nb, dtype=np.int64)
    for P in parts:
        slots = np.asarray(P.wall_slots)
        assert slots.dtype == np.int64 and P.wall_total == nb
        assert len(slots) == P.level["n_boundary"]
        assert np.all(np.diff(slots) > 0), "strictly ascending"
        assert len(slots) == 0 or (slots[0] >= 0 and slots[-1] < nb)
        named[slots] += 1
        lni = P.level["n_internal"]
        mine = P.level["edges"][lni:lni + len(slots)]
        theirs = whole["edges"][ni + slots]
        for f in mine.dtype.names:
            if f == "b":                                    # the renumbered node: the same node of the whole level
                assert np.array_equal(P.global_ids[mine["b"]], theirs["b"])
            else:
                assert np.array_equal(mine[f], theirs[f]), f
    assert np.array_equal(named, np.ones(nb, dtype=np.int64)), "every solid-wall edge exactly once"


@pytest.mark.parametrize("n_parts", [2, 3, 4, 5, 6])
def test_partition_level_names_every_wall_edge_once(n_parts):
    from mgcfd.partition import partition_level, rcb_partition, slab_partition
    levels = _levels()
    assert levels[0]["n_boundary"] > 256
    for split in (rcb_partition, slab_partition):
        part = split(np.asarray(levels[0]["coords"]), n_parts)
        _check_parts(levels[0], partition_level(levels[0], part))


@pytest.mark.parametrize("n_parts", [2, 3, 4, 5, 6])
def test_partition_hierarchy_names_every_wall_edge_once_on_every_level(n_parts):
    from mgcfd.partition import partition_hierarchy, rcb_partition, slab_partition
    levels = _levels()
    for split in (rcb_partition, slab_partition):
        H = partition_hierarchy(levels, split(np.asarray(levels[0]["coords"]), n_parts))
        for l in range(len(levels)):
            assert levels[l]["n_boundary"] > 0
            _check_parts(levels[l], [h.levels[l] for h in H])


def test_a_level_without_solid_wall_has_no_slots():
    import mgcfd
    from mgcfd import meshgen
    from mgcfd.partition import partition_hierarchy, rcb_partition
    mg = meshgen.make_multigrid((9, 5), "m6wing", seed=4, cavity_radius=0.0, jitter=0.2)
    levels = mgcfd.generated_to_levels(mg)
    for h in partition_hierarchy(levels, rcb_partition(np.asarray(levels[0]["coords"]), 3)):
        for P in h.levels:
            assert P.wall_total == 0 and len(P.wall_slots) == 0


def test_the_new_entry_points_are_bound(mgcfd_mod):
    for name in ("mgcfd_rank_set_wall_slots", "mgcfd_group_surface_loads", "mgcfd_group_cycles_loads", "mgcfd_rank_surface_loads",
                 "mgcfd_rank_cycles_loads"):
        assert name in mgcfd_mod.EXPORTED_SYMBOLS
    assert mgcfd_mod.load_library().mgcfd_abi_version() == 1


def test_driver_accepts_output_loads_on_several_gpus_with_every_level_partitioned(mgcfd_mod):
    # parsed, then the run stops at the missing input file as any run would
    r = subprocess.run([EXE, "--output-loads", "--gpus", "2", "--gpus-partition"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "ERROR: input_file not set" in r.stdout
    assert "--output-loads runs on" not in r.stderr


def test_driver_help_names_the_combination(mgcfd_mod):
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    text = " ".join(r.stderr.split())
    at = text.index("--output-loads ")
    assert "--gpus-partition" in text[at:at + 500]
