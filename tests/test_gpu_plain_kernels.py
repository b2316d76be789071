"""What a single-flavour kernel (csrc/kernels_plain.hip) alone produces from a state is the same bits whichever flavour the solver
runs: two solvers on one mesh, MGCFD_OPT_EXACT 1 and 0, the same level-0 state, and the surface loads, the friction loads, the
wall distance with its nearest wall nodes and the invalid-state check compared bit for bit.  Those kernels exist once in the
library and are never contracted (tests/test_host_boundary.py checks the library's symbols)."""
import numpy as np
import pytest

from conftest import perturbed_state

pytestmark = pytest.mark.gpu

MU = 1.0e-3
REF = (0.25, -0.125, 0.375)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def flavours(mesh_dir):
    """(exact solver, fast solver) on the 9^3 / 5^3 m6wing hierarchy, both holding the free stream with a fixed-seed +-1 % noise
    (momentum y and z lifted off zero first), so that no term of the loads vanishes."""
    import mgcfd
    mesh = mgcfd.Mesh("input.dat", mesh_dir)
    pair = []
    for exact in (1, 0):
        s = mgcfd.Solver.from_mesh(mesh, device=0)
        s.set_option("exact", exact)
        pair.append(s)
    state = perturbed_state(pair[0].nel(0), pair[0].far_field()[:5], seed=7)
    for s in pair:
        s.set(0, "variables", state)
    yield pair
    for s in pair:
        s.close()


def test_both_flavours_hold_the_same_state(flavours):
    a, b = flavours
    assert np.array_equal(_bits(a.get(0, "variables")), _bits(b.get(0, "variables")))


def test_pressure_loads_do_not_depend_on_the_flavour(flavours):
    a, b = (s.surface_loads(0, REF) for s in flavours)
    assert np.all(np.isfinite(a)) and np.all(a != 0.0)
    assert np.array_equal(_bits(a), _bits(b)), f"exact {a} fast {b}"


def test_friction_loads_do_not_depend_on_the_flavour(flavours):
    for s in flavours:
        s.set_viscous(MU, levels=1)
    a, b = (s.surface_loads(0, REF, friction=True) for s in flavours)
    assert a.shape == (12,) and np.all(np.isfinite(a)) and np.all(a[6:] != 0.0)
    assert np.array_equal(_bits(a), _bits(b)), f"exact {a} fast {b}"


def test_wall_distance_does_not_depend_on_the_flavour(flavours):
    for s in flavours:
        s.compute_wall_distance()
    d = [s.get(0, "wall_distance") for s in flavours]
    near = [s.wall_nearest(0) for s in flavours]
    assert np.all(np.isfinite(d[0])) and d[0].max() > 0.0 and near[0].min() >= 0
    assert np.array_equal(_bits(d[0]), _bits(d[1]))
    assert np.array_equal(near[0], near[1])


def test_invalid_state_check_does_not_depend_on_the_flavour(flavours):
    a, b = (s.check_for_invalid_variables(0) for s in flavours)
    assert a == b and a[0] == 0
