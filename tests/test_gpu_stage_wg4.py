"""The bit-identical fused stages at four workgroups per CU (MGCFD_OPT_STAGE_WG4, k_flux_tile's 80-byte-record instantiation)
against the same stages forced onto the 96-byte-record one, bit for bit, in one process: the bench level, the mixed-element
level and a lattice whose tile halos exceed the 254 slots (both fall back), and the 4-level V-cycle."""
import numpy as np
import pytest

from test_gpu_configs import _bits_equal

pytestmark = pytest.mark.gpu


def _sweeps(levels, mesh_variant, q, wg4, sweeps, variant=-1):
    import mgcfd
    s = mgcfd.Solver.from_arrays(levels, mesh_variant)
    s.set_option("stage_wg4", wg4)
    if variant >= 0:
        s.set_option("flux_variant", variant)
    assert s.get_option("stage_wg4") == wg4
    s.set(0, "variables", q)
    s.smooth(0, sweeps)
    out = {a: s.get(0, a) for a in ("variables", "old_variables", "residuals", "step_factors")}
    chosen = s.stage_wg4(0)
    s.close()
    return out, chosen


@pytest.mark.parametrize("variant", [-1, 0])          # the edge-length factor recomputed (default) / streamed
def test_bench_level_four_workgroups_per_cu_same_bits(variant):
    """The level bench.py times (67^3, 300,763 nodes, every tile halo within 254 slots): the automatic choice takes the new
    instantiation, and 5 sweeps (first stage, middle, last with the look-ahead) leave the same bits as the forced-old kernel."""
    import bench
    mg, levels = bench.build_workload(67)
    import mgcfd
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    assert s.tiling(0)["halo_max"] <= 254
    q = bench.perturbed_state(levels[0]["nel"], s.far_field()[:5])
    s.close()
    new, chosen_new = _sweeps(levels, mg.mesh_variant, q, 1, 5, variant)
    old, chosen_old = _sweeps(levels, mg.mesh_variant, q, 0, 5, variant)
    assert chosen_new and not chosen_old
    for a in new:
        _bits_equal(new[a], old[a], f"bench level, variant {variant}: {a}")


@pytest.mark.parametrize("mesh,lattice", [("mixed", 67), ("lattice", 55)])
def test_levels_with_halos_beyond_the_slots_fall_back(mesh, lattice):
    """The mixed-element level (halos up to 289 nodes) and the permuted 55^3 lattice (up to 265): the automatic choice keeps
    the 96-byte records, and the results equal the forced-old run's."""
    import bench
    import mgcfd
    mg, levels = bench.build_workload(lattice, mesh=mesh)
    s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
    halo_max = s.tiling(0)["halo_max"]
    q = bench.perturbed_state(levels[0]["nel"], s.far_field()[:5])
    s.close()
    new, chosen_new = _sweeps(levels, mg.mesh_variant, q, 1, 3)
    old, _ = _sweeps(levels, mg.mesh_variant, q, 0, 3)
    assert halo_max > 254 and not chosen_new, f"{mesh} {lattice}^3: halo_max {halo_max}, new kernel chosen: {chosen_new}"
    for a in new:
        _bits_equal(new[a], old[a], f"{mesh} {lattice}^3: {a}")


def test_four_level_vcycle_same_bits():
    """The (67, 55, 48, 43)^3 hierarchy of bench.py's V-cycle leg: 3 cycles with the automatic choice (some levels new, some
    not) against 3 with the old kernel everywhere; every level's state and residuals, and the RMS history."""
    import bench
    import mgcfd
    mg, levels = bench.build_hierarchy()
    runs = []
    for wg4 in (1, 0):
        s = mgcfd.Solver.from_arrays(levels, mg.mesh_variant)
        s.set_option("stage_wg4", wg4)
        rms = s.run_cycles(3)
        runs.append((np.asarray(rms), [(s.get(l, "variables"), s.get(l, "residuals")) for l in range(len(levels))],
                     [s.stage_wg4(l) for l in range(len(levels))]))
        s.close()
    (rms_n, st_n, ch_n), (rms_o, st_o, ch_o) = runs
    assert ch_n[0] and not any(ch_o), f"choice per level: {ch_n} / {ch_o}"
    _bits_equal(rms_n, rms_o, "RMS history")
    for l in range(len(levels)):
        _bits_equal(st_n[l][0], st_o[l][0], f"level {l} variables")
        _bits_equal(st_n[l][1], st_o[l][1], f"level {l} residuals")
