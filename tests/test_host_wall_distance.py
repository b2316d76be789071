"""Host tests of the wall distance (no GPU): the numpy emulator (tests/wall_distance_emulator.py) against a k-d tree on every
mesh tests/test_gpu_wall_distance.py runs, the tie rule, the wall-limited Smagorinsky length scale and y+ on a Couette flow over
a flat wall with a derived answer, the agreement of header, package and emulator, and the validity of every damped GPU run."""
import os
import re

import numpy as np
import pytest

import fas_emulator as fe
import friction_loads_emulator as fle
import variable_viscosity_emulator as vve
import viscous_emulator as ve
import wall_distance_emulator as wde

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MU, PRANDTL, SHEAR = 0.3, 0.72, 0.37
RHO, P0 = 1.3, 0.9


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def geometry_levels():
    """name -> meshgen.LevelMesh: the shapes of the GPU file's bitwise tests."""
    from mgcfd import meshgen
    out = {}
    for name in ("A", "B"):
        for l, lv in enumerate(meshgen.make_multigrid(fe.LATTICES[name], "fvcorr", **fe.LATTICE_ARGS).levels):
            out[f"{name}{l}"] = lv
    out["box17"] = meshgen.make_box_level(17, seed=3, cavity_radius=0.3)
    out["box21"] = meshgen.make_box_level(21, seed=3, cavity_radius=0.35)
    out["tet"] = meshgen.make_tet_level(30000, seed=0)
    out["box9"] = meshgen.make_box_level(9)
    return out


@pytest.fixture(scope="module")
def levels():
    return geometry_levels()


# (nodes, wall nodes, nodes with a tied minimum), counted here on the CPU
SHAPES = {"A0": (2178, 38, 0), "A1": (728, 6, 224), "A2": (215, 6, 53), "B0": (728, 6, 0), "B1": (124, 6, 64),
          "box17": (4452, 278, 1404), "box21": (7866, 546, None), "tet": (30000, 19, None), "box9": (729, 0, 0)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_emulator_against_a_kd_tree_and_the_tie_counts(name, levels):
    """d against scipy's cKDTree over the wall nodes to 1e-14 relative (both are a handful of roundings of the same quantity;
    candidate distances differ by far more, so a wrong index cannot hide), the nearest node at that distance, a wall node its own
    nearest at +0.0, and the shapes the GPU file relies on: sizes, wall counts and how many nodes the tie rule decides."""
    from scipy.spatial import cKDTree
    lv = levels[name]
    w = wde.level_wall_nodes(lv)
    nel, m, ties = SHAPES[name]
    assert (lv.nel, len(w)) == (nel, m)
    d, near = wde.wall_distance(lv.coords, w)
    if m == 0:
        assert np.isposinf(d).all() and (near == -1).all()
        return
    want, idx = cKDTree(lv.coords[w]).query(lv.coords)
    err = np.abs(d - want) / np.where(want > 0.0, want, 1.0)
    print(name, "max relative difference to the k-d tree", err.max(), "tied nodes", wde.tied_nodes(lv.coords, w))
    assert err.max() <= 1e-14
    assert np.array_equal(_bits(d[w]), _bits(np.zeros(m))) and np.array_equal(near[w], w)
    back = np.sqrt(((lv.coords - lv.coords[near]) ** 2).sum(axis=1))
    assert np.abs(back - want).max() <= 1e-14 * want.max()
    if ties is not None:
        assert wde.tied_nodes(lv.coords, w) == ties
    if ties:
        # the lowest wall id wins: no wall node of a lower id is as near
        for i in np.flatnonzero(near != w[idx])[:50]:
            r2 = ((lv.coords[w] - lv.coords[i]) ** 2).sum(axis=1)
            assert near[i] == w[np.flatnonzero(r2 == r2.min())[0]]


def test_a_nan_coordinate_is_never_taken():
    x = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [1.0, 0.0, 0.0], [0.25, 0.0, 0.0]])
    d, near = wde.wall_distance(x, [0, 1, 2])
    assert near.tolist() == [0, -1, 2, 0] and np.isposinf(d[1]) and d[3] == 0.25


def _state(vel, p):
    W = np.empty((len(vel), 5))
    W[:, 0] = RHO
    W[:, 1:4] = RHO * vel
    W[:, 4] = p / (ve.GAMMA - 1.0) + 0.5 * RHO * (vel * vel).sum(axis=1)
    return W


@pytest.fixture(scope="module")
def couette():
    """tests/test_host_friction_loads.py's Couette flow: the 9^3 box whose z = 0 hull faces are solid walls, u = (SHEAR z, 0, 0)
    at uniform density and pressure."""
    import mgcfd
    level = mgcfd.generated_to_levels(fle.hull_wall_box())[0]
    vel = np.zeros((level["nel"], 3))
    vel[:, 0] = SHEAR * level["coords"][:, 2]
    _, wall = fle.slices(level)
    return level, _state(vel, np.full(level["nel"], P0)), fle.wall_nodes(level["edges"][wall])


def test_damped_smagorinsky_in_pure_shear_over_a_flat_wall(couette):
    """Derived: the lattice is aligned with the wall, so d_i = z_i; pass 1 is exact on a linear field, so ss = 0.5 SHEAR^2 and
    mut_i = rho * min(cs delta_i, kappa z_i)^2 * |SHEAR| with delta_i = cbrt(vol_i), to 1e-12; exactly +0.0 on the wall."""
    level, W, wall = couette
    model = vve.Model(eddy="smagorinsky")
    d, near = wde.wall_distance(level["coords"], wall)
    z = level["coords"][:, 2]
    assert np.array_equal(_bits(d), _bits(z)) and np.array_equal(wall, np.flatnonzero(z == 0.0))
    S, mut = wde.damped_stresses(W, level["edges"], level, MU, PRANDTL, model, wde.WALL_KAPPA, wall)
    delta = np.cbrt(level["volumes"])
    want = RHO * np.minimum(vve.SMAGORINSKY_CS * delta, wde.WALL_KAPPA * z) ** 2 * abs(SHEAR)
    print("Couette: max |mut - derived| / max", np.abs(mut - want).max() / want.max(), "limited by the wall at",
          int((wde.WALL_KAPPA * z < vve.SMAGORINSKY_CS * delta).sum()), "of", len(z))
    assert np.abs(mut - want).max() <= 1e-12 * want.max()
    assert np.array_equal(_bits(mut[wall]), _bits(np.zeros(len(wall))))
    assert 0 < (wde.WALL_KAPPA * z < vve.SMAGORINSKY_CS * delta).sum() < len(z), "both branches of the limit are taken"
    # with d = +inf the length scale is the undamped model's, bit for bit
    l2 = wde.length_scale(model.c2, delta * delta, wde.WALL_KAPPA, np.full(len(z), np.inf))
    assert np.array_equal(_bits(l2), _bits(model.c2 * (delta * delta)))


def test_wall_yplus_of_the_couette_flow(couette):
    """y+ = h sqrt(rho tau) / mu with tau = MU SHEAR on the wall (mut is +0.0 there) and h the lattice spacing 1/8: to 1e-12."""
    import mgcfd
    level, W, wall = couette
    S = wde.node_stresses(W, level["edges"], level, MU, PRANDTL, vve.Model(eddy="smagorinsky"), wde.WALL_KAPPA, wall)
    ids, table = vve.distribution(W, level["edges"], level, mgcfd.free_stream_constants(1.2, 0.0), S)
    internal, _ = fle.slices(level)
    h = wde.wall_spacing(wde.wall_distance(level["coords"], wall)[0], level["edges"][internal], wall)
    assert np.array_equal(ids, wall) and np.abs(h - 0.125).max() <= 1e-15
    yplus = mgcfd.wall_yplus(table, h, RHO, MU)
    want = 0.125 * np.sqrt(RHO * MU * SHEAR) / MU
    print("Couette: y+", yplus.min(), yplus.max(), "against", want)
    assert yplus.shape == (81,) and np.abs(yplus - want).max() <= 1e-12 * want


def test_wall_spacing_skips_wall_neighbours_and_is_zero_without_a_fluid_neighbour():
    edges = np.zeros(3, dtype=[("a", np.int64), ("b", np.int64)])
    edges["a"], edges["b"] = [0, 0, 3], [1, 2, 4]
    d = np.array([0.0, 0.0, 0.5, 0.0, 0.0])
    assert wde.wall_spacing(d, edges, [0, 1, 3, 4]).tolist() == [0.5, 0.0, 0.0, 0.0]


def test_header_package_and_emulator_agree():
    import mgcfd
    from mgcfd import api
    header = open(os.path.join(ROOT, "include", "mgcfd.h")).read()
    assert int(re.search(r"#define MGCFD_ARR_WALL_DISTANCE (\d+)", header).group(1)) == api.ARR["wall_distance"] == wde.ARR_WALL_DISTANCE == 16
    assert api.ARR["wall_distance"] == api.ARR["eddy_viscosity"] + 1 and api.NCOLS["wall_distance"] == 1
    assert float(re.search(r"#define MGCFD_WALL_KAPPA (\S+)", header).group(1)) == api.WALL_KAPPA == wde.WALL_KAPPA == 0.41
    assert "int mgcfd_abi_version(void)" in header
    for name in ("mgcfd_compute_wall_distance", "mgcfd_get_wall_distance", "mgcfd_release_wall_distance", "mgcfd_wall_nearest",
                 "mgcfd_wall_spacing", "mgcfd_set_wall_damping", "mgcfd_get_wall_damping"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in mgcfd.EXPORTED_SYMBOLS, name
    for name in ("compute_wall_distance", "wall_distance_levels", "release_wall_distance", "wall_nearest", "wall_spacing",
                 "set_wall_damping", "wall_damping"):
        assert callable(getattr(mgcfd.Solver, name)), name
    import inspect
    assert inspect.signature(mgcfd.Solver.set_wall_damping).parameters["kappa"].default == wde.WALL_KAPPA
    assert "wall_damping" in inspect.signature(mgcfd.Solver.polar).parameters
    assert callable(mgcfd.wall_yplus)


@pytest.fixture(scope="module")
def lattices(tmp_path_factory):
    d = tmp_path_factory.mktemp("wall_distance_lattices")
    return {name: fe.write_lattice(name, d) for name in fe.LATTICES}


@pytest.mark.parametrize("key,mu,mode,cfl,wall,lv,model", wde.gpu_runs())
def test_the_damped_gpu_runs_stay_valid(key, mu, mode, cfl, wall, lv, model, oracle, lattices):
    """Every damped run of tests/test_gpu_wall_distance.py passes the invalid-state check in every cycle on the CPU; the eddy
    viscosity is +0.0 at every wall node and nowhere above the undamped model's on the same final state."""
    em = wde.configured(oracle, lattices.get(key, key), mu, mode, cfl, wall, lv, model)
    for c in range(ve.GPU_CYCLES):
        rc, rms = em.cycles(1)
        assert rc == 0 and np.isfinite(rms).all(), f"cycle {c}"
    for l in range(em.n):
        mut = em.eddy_viscosity(l)
        assert np.array_equal(_bits(mut[em.wall_nodes[l]]), _bits(np.zeros(len(em.wall_nodes[l]))))
        _, damped = em.stresses_of(l)
        _, free = vve.VariableViscosityOracle.stresses_of(em, l)
        assert (damped <= free).all() and (len(em.wall_nodes[l]) == 0 or (damped < free).any())
    em.close()


def test_the_driver_run_stays_valid_and_differs_from_the_undamped_one(oracle):
    """tests/test_gpu_wall_distance.py::test_driver_flag's run: m6_2lvl from the far field at ve.DRIVER_MU, no-slip walls on both
    levels (18 and 6 wall nodes), (constant, smagorinsky)."""
    states = []
    for damped in (True, False):
        em = wde.WallDampedOracle(oracle, "m6_2lvl", mu=ve.DRIVER_MU, wall=1, viscous_levels="all")
        assert [len(w) for w in em.wall_nodes] == [18, 6]
        em.set_viscosity_model(law="constant", eddy="smagorinsky")
        em.set_wall_damping(damped)
        for c in range(ve.GPU_CYCLES):
            rc, rms = em.cycles(1)
            assert rc == 0 and np.isfinite(rms).all()
        states.append(em.variables(0))
        em.close()
    assert not np.array_equal(_bits(states[0]), _bits(states[1]))


def test_the_composed_damped_run_stays_valid(oracle, lattices):
    import dual_time_emulator as dte
    name, mode, cfl, smoothing, jst_levels, order, fas = wde.COMPOSED
    case = lattices["A"]
    em = wde.configured(oracle, case, ve.CELL_RE_MU, mode, cfl, 1, "all", vve.COMBINED, smoothing=smoothing, jst_levels=jst_levels, fas=fas)
    em.set_dual_time(dte.pick_dt(oracle, case, mode, cfl))
    em.set_order(order)
    rc, rms = em.advance(ve.DUAL_STEPS, ve.DUAL_CYCLES)
    em.close()
    assert rc == 0 and np.isfinite(rms).all()
