"""numpy emulator of the surface-loads definition ("Surface loads"): the yardstick the loads tests
compare the HIP kernel against bit for bit.  Elementwise float64 operations in the kernel's order and association,
then the fixed summation tree; nothing here is contracted to FMA."""
import numpy as np

CHUNK = 256


def pressure(q):
    """derive()'s pressure (cfd_loops.h:121-148) of every row of q[:, 5]."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 5)
    rho, mx, my, mz, en = (q[:, k] for k in range(5))
    vx, vy, vz = mx / rho, my / rho, mz / rho
    speed_sqd = vx * vx + vy * vy + vz * vz
    return (1.4 - 1.0) * (en - 0.5 * rho * speed_sqd)


def edge_terms(variables, wall_edges, coords, ff17, ref_point):
    """[n, 6] per-edge force and moment of the solid-wall edges (records with fields b, x, y, z)."""
    q = np.asarray(variables, dtype=np.float64).reshape(-1, 5)
    b = np.asarray(wall_edges["b"], dtype=np.int64)
    p_inf = pressure(np.asarray(ff17[:5], dtype=np.float64))[0]
    dp = pressure(q[b]) - p_inf
    fx, fy, fz = dp * wall_edges["x"], dp * wall_edges["y"], dp * wall_edges["z"]
    if coords is None or np.size(coords) == 0:
        c = np.zeros((len(b), 3))
    else:
        c = np.asarray(coords, dtype=np.float64).reshape(-1, 3)[b]
    ref = np.asarray(ref_point, dtype=np.float64)
    rx, ry, rz = c[:, 0] - ref[0], c[:, 1] - ref[1], c[:, 2] - ref[2]
    return np.stack([fx, fy, fz, ry * fz - rz * fy, rz * fx - rx * fz, rx * fy - ry * fx], axis=1)


def tree_stage(a):
    """Stage A: chunks of 256 rows (the last padded with zeros), each reduced by v[t] += v[t+s], s = 128 .. 1."""
    a = np.asarray(a, dtype=np.float64)
    m = -(-len(a) // CHUNK)
    v = np.zeros((m * CHUNK, a.shape[1]))
    v[:len(a)] = a
    v = v.reshape(m, CHUNK, a.shape[1])
    s = CHUNK // 2
    while s >= 1:
        v[:, :s] = v[:, :s] + v[:, s:2 * s]
        s //= 2
    return v[:, 0]


def reduce_loads(terms):
    """Stage A, then stage A again over the partial sums until one row is left; zeros for no edges."""
    terms = np.asarray(terms, dtype=np.float64)
    if len(terms) == 0:
        return np.zeros(terms.shape[1] if terms.ndim == 2 else 6)
    a = tree_stage(terms)
    while len(a) > 1:
        a = tree_stage(a)
    return a[0]


def surface_loads(variables, wall_edges, coords, ff17, ref_point):
    return reduce_loads(edge_terms(variables, wall_edges, coords, ff17, ref_point))


def coefficients(ff17, loads, ref_area=1.0, ref_length=1.0):
    """CD CL CS CMx CMy CMz by the formula of INTEGRATION.md."""
    ff = np.asarray(ff17, dtype=np.float64)
    rho = ff[0]
    v = ff[1:4] / rho
    q = 0.5 * rho * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    a = np.arctan2(v[1], v[0])
    f = np.asarray(loads, dtype=np.float64)
    qs = q * ref_area
    return np.array([(f[0] * np.cos(a) + f[1] * np.sin(a)) / qs, (-f[0] * np.sin(a) + f[1] * np.cos(a)) / qs, f[2] / qs,
                     f[3] / (qs * ref_length), f[4] / (qs * ref_length), f[5] / (qs * ref_length)])
