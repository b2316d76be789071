"""numpy emulator of the viscous surface loads (mgcfd_surface_loads_viscous, mgcfd_wall_distribution): the
yardstick the tests compare the HIP kernels against bit for bit.  It is written from the definition on top of the emulators of
the two halves it joins: ``viscous_emulator.stresses`` (pass 1 of the viscous terms) and ``surface_loads_emulator`` (the pressure
terms, ``tree_stage`` / ``reduce_loads``).  Elementwise float64 operations in the definition's order and association; nothing
here is contracted to FMA.

    wall nodes     the distinct b ends of the solid-wall slice B, ascending original id
    Sw_i           viscous_emulator.stresses on the level's current variables, the rows of the wall nodes
    edge terms     pressure six: surface_loads_emulator.edge_terms;  friction six, tau from Sw_b:
                   gx = -((txx*x + txy*y) + txz*z), gy = -((txy*x + tyy*y) + tyz*z), gz = -((txz*x + tyz*y) + tzz*z),
                   moment (ry*gz - rz*gy, rz*gx - rx*gz, rx*gy - ry*gx);  +0.0 on a level the viscous terms are not on for
    summation      every one of the twelve columns through surface_loads_emulator.reduce_loads
    distribution   per wall node a = the sum of its solid-wall edge weights from +0.0 in B order, dp = p - p_inf, t = -(tau . a)

A level is a dict as ``mgcfd.Mesh.level`` / ``mgcfd.generated_to_levels`` give it; ``edges`` are the weights the solver holds
(``Solver.get_edges``), ``viscous`` is ``(mu, prandtl)`` or None.
"""
import numpy as np

import surface_loads_emulator as sle
import viscous_emulator as ve


def slices(level):
    """(internal, solid-wall) slices of a level's edge list."""
    i0 = int(level.get("internal_start", 0))
    b0 = int(level.get("boundary_start", i0 + int(level["n_internal"])))
    return slice(i0, i0 + int(level["n_internal"])), slice(b0, b0 + int(level["n_boundary"]))


def wall_nodes(wall_edges):
    return np.unique(np.asarray(wall_edges["b"], dtype=np.int64))


def node_stresses(variables, internal_edges, volumes, mu, prandtl):
    """S [nel, 12] of every node: pass 1 on ``variables`` over the internal edges in their order."""
    a, b = np.asarray(internal_edges["a"], dtype=np.int64), np.asarray(internal_edges["b"], dtype=np.int64)
    to, frm, N = ve.interleaved(a, b, internal_edges)
    return ve.stresses(variables, to, frm, N, volumes, mu, ve.conductivity(mu, prandtl))


def friction_terms(S, wall_edges, coords, ref_point):
    """[n, 6] per-edge friction force and moment; S None: +0.0."""
    b = np.asarray(wall_edges["b"], dtype=np.int64)
    if S is None:
        return np.zeros((len(b), 6))
    x, y, z = (np.asarray(wall_edges[k], dtype=np.float64) for k in "xyz")
    txx, tyy, tzz, txy, txz, tyz = (S[b, k] for k in range(3, 9))
    gx = -((txx * x + txy * y) + txz * z)
    gy = -((txy * x + tyy * y) + tyz * z)
    gz = -((txz * x + tyz * y) + tzz * z)
    if coords is None or np.size(coords) == 0:
        c = np.zeros((len(b), 3))
    else:
        c = np.asarray(coords, dtype=np.float64).reshape(-1, 3)[b]
    ref = np.asarray(ref_point, dtype=np.float64)
    rx, ry, rz = c[:, 0] - ref[0], c[:, 1] - ref[1], c[:, 2] - ref[2]
    return np.stack([gx, gy, gz, ry * gz - rz * gy, rz * gx - rx * gz, rx * gy - ry * gx], axis=1)


def _stresses_of(variables, edges, level, viscous):
    if viscous is None:
        return None
    internal, _ = slices(level)
    return node_stresses(variables, edges[internal], level["volumes"], *viscous)


def surface_loads12(variables, edges, level, ff17, ref_point, viscous):
    """out12 = Fp(3) Mp(3) | Fv(3) Mv(3) of a level's current variables."""
    _, wall = slices(level)
    walls = edges[wall]
    if len(walls) == 0:
        return np.zeros(12)
    pressure = sle.edge_terms(variables, walls, level.get("coords"), ff17, ref_point)
    friction = friction_terms(_stresses_of(variables, edges, level, viscous), walls, level.get("coords"), ref_point)
    return sle.reduce_loads(np.concatenate([pressure, friction], axis=1))


def wall_stresses(variables, edges, level, viscous):
    """(ids [n], Sw [n, 12])."""
    _, wall = slices(level)
    ids = wall_nodes(edges[wall])
    return ids, _stresses_of(variables, edges, level, viscous)[ids]


def distribution(variables, edges, level, ff17, viscous):
    """(ids [n], table [n, 7]): ax ay az | dp | tx ty tz per wall node."""
    _, wall = slices(level)
    walls = edges[wall]
    ids = wall_nodes(walls)
    at = np.searchsorted(ids, np.asarray(walls["b"], dtype=np.int64))
    a = np.zeros((len(ids), 3))
    for d, k in enumerate("xyz"):
        np.add.at(a[:, d], at, np.asarray(walls[k], dtype=np.float64))           # (unbuffered: one addition per edge, in B order)
    q = np.asarray(variables, dtype=np.float64).reshape(-1, 5)
    dp = sle.pressure(q[ids]) - sle.pressure(np.asarray(ff17[:5], dtype=np.float64))[0]
    t = np.zeros((len(ids), 3))
    S = _stresses_of(variables, edges, level, viscous)
    if S is not None:
        txx, tyy, tzz, txy, txz, tyz = (S[ids, k] for k in range(3, 9))
        t[:, 0] = -((txx * a[:, 0] + txy * a[:, 1]) + txz * a[:, 2])
        t[:, 1] = -((txy * a[:, 0] + tyy * a[:, 1]) + tyz * a[:, 2])
        t[:, 2] = -((txz * a[:, 0] + tyz * a[:, 1]) + tzz * a[:, 2])
    return ids, np.concatenate([a, dp[:, None], t], axis=1)


def surface_coefficients(ff17, table):
    """(Cp [n], Cf [n, 3]): Cp = dp / q_inf, Cf = (t - (t.n) n) / (|a| q_inf), n = a / |a|."""
    ff = np.asarray(ff17, dtype=np.float64)
    v = ff[1:4] / ff[0]
    q = 0.5 * ff[0] * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    tab = np.asarray(table, dtype=np.float64).reshape(-1, 7)
    a, dp, t = tab[:, 0:3], tab[:, 3], tab[:, 4:7]
    area = np.sqrt((a * a).sum(axis=1))
    n = a / area[:, None]
    return dp / q, (t - (t * n).sum(axis=1)[:, None] * n) / (area * q)[:, None]


# ---- the meshes of the tests (tests/test_host_friction_loads.py counts them on the CPU and checks that the runs stay valid) ----
# Every GPU run: viscous_emulator.start_state on level 0, the terms on every level at GPU_MU, both walls, fas_emulator.GPU_CYCLES
# cycles.  The viscosities: a cell Reynolds number rho_inf |V_inf| h / mu of about 2 on the generated lattices (h = 1/12, 1/16, 1/8
# at the default far field, rho 1.4, |V| 1.2), as viscous_emulator.CELL_RE_MU; 1e-3 on the goldens, whose weights are damped at load.
GPU_MU = {"A": ve.CELL_RE_MU, "box17": 0.05, "hull9": 0.1, "mixed_2lvl": 1e-3, "tet_2lvl": 1e-3}
GPU_GENERATED = ("A", "box17", "hull9")
FVCORR_BOX = dict(sizes=(17,), seed=5, cavity_radius=0.3, jitter=0.2)      # 414 solid-wall edges, 278 wall nodes


def fvcorr_box():
    from mgcfd import meshgen
    return meshgen.make_multigrid(FVCORR_BOX["sizes"], "fvcorr", seed=FVCORR_BOX["seed"], cavity_radius=FVCORR_BOX["cavity_radius"],
                                  jitter=FVCORR_BOX["jitter"])


def hull_wall_box(n=9, permute=False):
    """An n^3 fvcorr box whose z = 0 hull faces are solid walls (-1) and not far field (-2): a flat wall of area 1."""
    from mgcfd import meshgen
    level = meshgen.make_box_level(n, permute=permute)
    node = np.repeat(np.arange(level.nel, dtype=np.int64), np.diff(level.nbr_ptr))
    down = (level.nbr_idx == -2) & (level.nbr_w[:, 2] < 0.0) & (level.coords[node, 2] == 0.0)
    level.nbr_idx = np.where(down, -1, level.nbr_idx)
    return meshgen.MultigridMesh(mesh_name="fvcorr", levels=[level])


def generated(key):
    """The generated meshes of GPU_GENERATED."""
    from mgcfd import meshgen
    import fas_emulator as fe
    if key == "A":
        return meshgen.make_multigrid(fe.LATTICES["A"], "fvcorr", **fe.LATTICE_ARGS)
    return {"box17": fvcorr_box, "hull9": hull_wall_box}[key]()


def write_case(key, directory):
    """A generated mesh as a case directory of the emulators' kind (fas_emulator.write_lattice)."""
    import os
    from mgcfd import meshgen
    d = os.path.join(str(directory), "friction_" + key)
    os.makedirs(os.path.join(d, "input"))
    meshgen.write_input(generated(key), os.path.join(d, "input"))
    with open(os.path.join(d, "case.txt"), "w") as f:
        f.write("duplicate = 1\n")
    return d
