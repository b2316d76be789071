"""Host tests of the viscous surface loads (no GPU): what the numpy emulator (tests/friction_loads_emulator.py) computes on
cases with a derived answer — a Couette flow over a flat wall, a uniform state — its pressure half against the emulator of the
pressure loads in bits, the surface coefficients, and the wall counts of the meshes tests/test_gpu_friction_loads.py runs."""
import numpy as np
import pytest

import fas_emulator as fe
import friction_loads_emulator as fle
import surface_loads_emulator as sle
import viscous_emulator as ve
from conftest import perturbed_state

MU, PRANDTL, SHEAR = 0.3, 0.72, 0.37
RHO, P0 = 1.3, 0.9


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _level(mg, l=0):
    import mgcfd
    return mgcfd.generated_to_levels(mg)[l]


def _state(vel, p):
    W = np.empty((len(vel), 5))
    W[:, 0] = RHO
    W[:, 1:4] = RHO * vel
    W[:, 4] = p / (ve.GAMMA - 1.0) + 0.5 * RHO * (vel * vel).sum(axis=1)
    return W


def _far_field():
    import mgcfd
    return mgcfd.free_stream_constants(1.2, 0.0)


def _wall_degrees(level):
    _, wall = fle.slices(level)
    return np.unique(np.unique(level["edges"][wall]["b"], return_counts=True)[1]).tolist()


@pytest.fixture(scope="module")
def couette():
    """The 9^3 hull-wall box with u = (SHEAR z, 0, 0) at uniform density and pressure."""
    level = _level(fle.hull_wall_box())
    vel = np.zeros((level["nel"], 3))
    vel[:, 0] = SHEAR * level["coords"][:, 2]
    return level, _state(vel, np.full(level["nel"], P0))


def test_couette_flow_over_a_flat_wall(couette):
    """Derived: every wall edge has weights (0, 0, +A_e) (fvcorr: into the fluid), rz = 0 and tau_xz = MU * SHEAR, so
    Fv = (-MU SHEAR, 0, 0) on a wall of area 1 and, the wall's centroid lying at y = 0.5, Mv about the origin is
    (0, 0, +0.5 MU SHEAR); to 1e-12 relative.  The nodes' t add up to Fv to 1e-12."""
    level, W = couette
    _, wall = fle.slices(level)
    walls = level["edges"][wall]
    assert len(walls) == 81 and not walls["x"].any() and not walls["y"].any() and (walls["z"] > 0.0).all()
    assert abs(walls["z"].sum() - 1.0) <= 1e-14
    out = fle.surface_loads12(W, level["edges"], level, _far_field(), (0.0, 0.0, 0.0), (MU, PRANDTL))
    fv, mv = out[6:9], out[9:12]
    scale = MU * SHEAR
    print("Couette: Fv", fv, "Mv", mv, "against", -scale, 0.5 * scale)
    assert np.abs(fv - np.array([-scale, 0.0, 0.0])).max() <= 1e-12 * scale
    assert np.abs(mv - np.array([0.0, 0.0, 0.5 * scale])).max() <= 1e-12 * scale
    ids, table = fle.distribution(W, level["edges"], level, _far_field(), (MU, PRANDTL))
    assert np.array_equal(ids, np.flatnonzero(level["coords"][:, 2] == 0.0)) and table.shape == (81, 7)
    assert np.abs(table[:, 4:7].sum(axis=0) - fv).max() <= 1e-12 * scale
    # a pressure excess on the same wall pushes along +z: Fp,z = +dp A
    dp = P0 - sle.pressure(_far_field()[:5])[0]
    assert abs(out[2] - dp) <= 1e-12 * abs(dp) and abs(out[0]) <= 1e-12 * abs(dp) and abs(out[1]) <= 1e-12 * abs(dp)
    assert np.abs((table[:, 3:4] * table[:, 0:3]).sum(axis=0) - out[0:3]).max() <= 1e-12 * abs(dp)


def test_surface_coefficients_of_the_couette_flow(couette):
    """Cp = dp / q_inf and Cf = (-MU SHEAR / q_inf, 0, 0) at every wall node (the wall shear is tangential already); the
    package's surface_coefficients gives the emulator's numbers."""
    import mgcfd
    level, W = couette
    ff = _far_field()
    _, table = fle.distribution(W, level["edges"], level, ff, (MU, PRANDTL))
    v = ff[1:4] / ff[0]
    q = 0.5 * ff[0] * float(v @ v)
    cp, cf = mgcfd.surface_coefficients(ff, table)
    want_cp, want_cf = fle.surface_coefficients(ff, table)
    assert np.allclose(cp, want_cp, rtol=1e-15, atol=0) and np.allclose(cf, want_cf, rtol=1e-14, atol=1e-300)
    assert np.abs(cp - (P0 - sle.pressure(ff[:5])[0]) / q).max() <= 1e-12 * np.abs(cp).max()
    assert np.abs(cf - np.array([-MU * SHEAR / q, 0.0, 0.0])).max() <= 1e-12 * MU * SHEAR / q


def test_a_uniform_state_has_no_friction():
    level = _level(fle.fvcorr_box())
    W = np.tile(_far_field()[:5], (level["nel"], 1))
    out = fle.surface_loads12(W, level["edges"], level, _far_field(), (0.1, 0.2, 0.3), (MU, PRANDTL))
    assert (out[6:] == 0.0).all()
    _, table = fle.distribution(W, level["edges"], level, _far_field(), (MU, PRANDTL))
    assert (table[:, 4:] == 0.0).all() and (table[:, 3] == 0.0).all()


@pytest.mark.parametrize("viscous", [None, (MU, PRANDTL)])
def test_the_pressure_six_are_the_pressure_loads(viscous):
    """Bit for bit what surface_loads_emulator.surface_loads gives, with the friction on and off; off, the friction is +0.0."""
    level = _level(fle.fvcorr_box())
    ff = _far_field()
    W = perturbed_state(level["nel"], ff[:5], seed=3)
    ref = (0.25, -0.125, 0.375)
    out = fle.surface_loads12(W, level["edges"], level, ff, ref, viscous)
    _, wall = fle.slices(level)
    want = sle.surface_loads(W, level["edges"][wall], level["coords"], ff, ref)
    assert np.array_equal(_bits(out[:6]), _bits(want))
    if viscous is None:
        assert np.array_equal(_bits(out[6:]), _bits(np.zeros(6)))
    else:
        assert (out[6:] != 0.0).all()


def test_the_wall_rows_equal_the_full_pass():
    """Sw is pass 1 restricted to the wall nodes: the same bits as the rows of S over the whole level."""
    level = _level(fle.fvcorr_box())
    W = perturbed_state(level["nel"], _far_field()[:5], seed=3)
    ids, Sw = fle.wall_stresses(W, level["edges"], level, (MU, PRANDTL))
    internal, _ = fle.slices(level)
    S = fle.node_stresses(W, level["edges"][internal], level["volumes"], MU, PRANDTL)
    assert np.array_equal(_bits(Sw), _bits(S[ids])) and Sw[:, 3:9].any()


def test_wall_counts_of_the_gpu_meshes():
    """What tests/test_gpu_friction_loads.py relies on: the fvcorr 17^3 box has 414 solid-wall edges (two chunks of 256: stage B
    runs) on 278 wall nodes carrying 1, 2 and 3 of them; lattice A has 54 and 6 on levels 0 and 1, on nodes carrying 1 and 3;
    the hull-wall box 81."""
    from mgcfd import meshgen
    box = _level(fle.fvcorr_box())
    _, wall = fle.slices(box)
    assert box["n_boundary"] == 414 and len(fle.wall_nodes(box["edges"][wall])) == 278 and _wall_degrees(box) == [1, 2, 3]
    mg = meshgen.make_multigrid(fe.LATTICES["A"], "fvcorr", **fe.LATTICE_ARGS)
    a0, a1 = _level(mg, 0), _level(mg, 1)
    assert (a0["n_boundary"], a1["n_boundary"]) == (54, 6)
    assert (_wall_degrees(a0), _wall_degrees(a1)) == ([1, 3], [1])
    assert _level(fle.hull_wall_box())["n_boundary"] == 81


@pytest.mark.parametrize("key", list(fle.GPU_MU))
def test_the_gpu_runs_stay_valid(key, oracle, tmp_path):
    """Every run of tests/test_gpu_friction_loads.py — the perturbed start state, the terms on every level at GPU_MU, slip and
    no-slip walls — passes the invalid-state check for fe.GPU_CYCLES cycles on the CPU (the composed oracle of the viscous terms)."""
    case = fle.write_case(key, tmp_path) if key in fle.GPU_GENERATED else key
    for wall in (0, 1):
        em = ve.configured(oracle, case, fle.GPU_MU[key], "reference", 0.5, wall, "all")
        rc, rms = em.cycles(fe.GPU_CYCLES)
        em.close()
        assert rc == 0 and np.isfinite(rms).all(), f"{key} wall={wall}"
