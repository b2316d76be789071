"""The yardsticks of the run-time free stream (mgcfd_free_stream_constants, mgcfd_set_free_stream):

* ``free_stream_constants`` — the reference's far-field expressions (src/Kernels/cfd_loops.h:85-119, 57-83) in their order, with
  the Mach number and the angle of attack as arguments, in plain Python floats: every operation is one IEEE-754 double
  operation (Python never contracts to FMA), ``math.cos`` / ``math.sin`` / ``math.sqrt`` are the host libm's, the one the
  library calls.
* ``ComposedOracle`` — a V-cycle composed from the oracle's KERNEL entry points in ``ora_solve``'s order
  (oracle/mgcfd_oracle.c, the driver of src/euler3d_cpu_double.cpp:321-694), with the far field handed in instead of
  compiled in.  With the default far field it reproduces ``ora_solve`` bit for bit (tests/test_host_free_stream.py); it
  is the expectation of every GPU test of the free stream.
* the tables the tests run over: ``PAIRS`` (host, against the emulator) and ``GPU_CASES`` x ``GPU_PAIRS``.
"""
import ctypes as C
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

DEFAULT = (1.2, 0.0)

# (mach, alpha_deg): subsonic, transonic and supersonic, both signs of alpha, and the reference's own pair
PAIRS = [(1.2, 0.0), (0.5, 2.0), (0.3, -4.0), (0.8395, 3.06), (0.84, -3.06), (0.95, 0.5), (1.0, -1.0), (1.2, 5.0), (1.5, -2.5),
         (2.0, 10.0), (3.0, -20.0), (0.1, 45.0), (0.7, -60.0), (1.3, 89.0), (6.5, -0.125), (0.05, 1e-3)]

# What the GPU tests run: every golden case below at every pair below, 3 cycles, none skipped.  tests/test_host_free_stream.py
# asserts on the CPU that the composed oracle stays valid (return code 0 in every cycle) for each combination, cold and
# in the warm-start sequences the GPU tests drive.
GPU_CASES = ["m6_2lvl", "m6_3lvl", "m6_2lvl_dup2", "mixed_2lvl", "tet_2lvl", "fvcorr_1lvl"]
GPU_PAIRS = [(0.8, 3.0), (1.5, -2.0)]            # one subsonic, one supersonic; both signs of alpha
GPU_CYCLES = 3
SWEEPS = 4                                       # sweeps of level 0 alone at one pair, then as many at the other (sweep graphs)
# the polar the Python and drop-in tests run on m6_2lvl: GPU_CYCLES cycles per angle, warm-started or not
POLAR_CASE, POLAR_MACH, POLAR_ALPHAS = "m6_2lvl", 0.8, [-2.0, 0.5, 3.0]


def free_stream_constants(mach, alpha_deg):
    """The 17 far-field doubles: ff_variable[5] | ff_flux_contribution_momentum_x/y/z[3] | ..._density_energy[3]."""
    gamma = 1.4
    angle = (3.1415926535897931 / 180.0) * float(alpha_deg)
    rho = 1.4
    pressure = 1.0
    c = math.sqrt(gamma * pressure / rho)
    speed = float(mach) * c
    vx = speed * math.cos(angle)
    vy = speed * math.sin(angle)
    vz = 0.0
    var = [rho, rho * vx, rho * vy, rho * vz, rho * (0.5 * (speed * speed)) + (pressure / (gamma - 1.0))]
    # compute_flux_contribution, cfd_loops.h:57-83
    mx = [vx * var[1] + pressure, vx * var[2], vx * var[3]]
    my = [mx[1], vy * var[2] + pressure, vy * var[3]]
    mz = [mx[2], my[2], vz * var[3] + pressure]
    de_p = var[4] + pressure
    de = [vx * de_p, vy * de_p, vz * de_p]
    return np.array(var + mx + my + mz + de, dtype=np.float64)


def case_input(case):
    return os.path.join(GOLDEN, case, "input")


def case_duplicate(case):
    meta = dict(l.strip().split(" = ") for l in open(os.path.join(GOLDEN, case, "case.txt")))
    return int(meta["duplicate"])


class ComposedOracle:
    """``ora_solve`` taken apart: the same kernel calls in the same order on the same arrays, the far field an argument."""

    def __init__(self, oracle, case, ff17=None):
        self.O = oracle
        self.lib = oracle.load()
        self.oc = oracle.OracleCase.from_input_dat(os.path.join(case_input(case), "input.dat"), case_duplicate(case))
        self.n = self.oc.nlevels
        self.variant = self.oc.mesh_variant
        self.ff = oracle.OraFarfield()
        L = self.oc.levels
        self.scratch = np.zeros(max(L[l].nel for l in range(self.n)), dtype=np.int64)
        damping = {2: 5e-8, 3: 1e-7, 4: 2e-7}.get(self.variant, 0.0)              # euler3d_cpu_double.cpp:337-352
        if damping != 0.0:
            for l in range(self.n):
                self.lib.ora_adjust_ewt(L[l].coords, L[l].n_edges, L[l].edges)
                self.lib.ora_dampen_ewt(L[l].n_edges, L[l].edges, damping)
        for l in range(self.n):
            self.lib.ora_zero_fluxes(L[l].nel, L[l].fluxes)
            self.lib.ora_zero_fluxes(L[l].nel, L[l].residuals)
        self.set_far_field(oracle_default_ff17(oracle) if ff17 is None else ff17, reinitialise=True)

    def set_far_field(self, ff17, reinitialise):
        ff17 = np.asarray(ff17, dtype=np.float64).reshape(17)
        self.ff17 = ff17.copy()
        for k in range(5):
            self.ff.var[k] = ff17[k]
        for name, at in (("fc_mx", 5), ("fc_my", 8), ("fc_mz", 11), ("fc_de", 14)):
            for k in range(3):
                getattr(self.ff, name)[k] = ff17[at + k]
        if reinitialise:
            L = self.oc.levels
            for l in range(self.n):
                self.lib.ora_initialize_variables(L[l].nel, L[l].variables, C.byref(self.ff))

    def _sweep(self, l):
        """euler3d_cpu_double.cpp:383-508; returns check_for_invalid_variables' code of the first failing stage, or 0."""
        lib, L = self.lib, self.oc.levels[l]
        C.memmove(L.old_variables, L.variables, 8 * L.nel * 5)
        if self.variant == 0:
            lib.ora_compute_step_factor_legacy(L.nel, L.variables, L.volumes, L.step_factors)
        else:
            lib.ora_compute_step_factor(L.nel, L.variables, L.volumes, L.step_factors)
        for j in range(3):
            lib.ora_compute_flux_edge(L.internal_start, L.n_internal, L.edges, L.variables, L.fluxes)
            lib.ora_compute_boundary_flux_edge(L.boundary_start, L.n_boundary, L.edges, L.variables, L.fluxes)
            lib.ora_compute_wall_flux_edge(L.wall_start, L.n_wall, L.edges, L.variables, L.fluxes, C.byref(self.ff))
            lib.ora_time_step(j, L.nel, L.step_factors, L.fluxes, L.old_variables, L.variables)
            rc = lib.ora_check_for_invalid_variables(L.variables, L.nel, None)
            if rc:
                return rc
        lib.ora_residual(L.nel, L.old_variables, L.variables, L.residuals)
        return 0

    def cycles(self, count):
        """``count`` cycles from the current state: (rc, rms[count]); stops at the first invalid state as ora_solve does."""
        lib, L, n = self.lib, self.oc.levels, self.n
        rms = []
        for _ in range(count):
            for l in range(n):                                   # up: sweep, restrict
                rc = self._sweep(l)
                if rc:
                    return rc, np.array(rms)
                if l == 0:
                    rms.append(lib.ora_calc_rms(L[0].nel, L[0].residuals))
                if l + 1 < n:
                    lib.ora_mg_restrict(L[l].variables, L[l + 1].variables, L[l + 1].nel, L[l].mg_map,
                                        self.O.ptr(self.scratch), L[l].mgc)
            for l in range(n - 2, -1, -1):                       # down: prolong, sweep (not on level 0: the next cycle's)
                lib.ora_prolong_residuals_interpolate_proper(L[l].edges, L[l].n_internal, L[l + 1].residuals, L[l].residuals,
                                                             L[l].variables, L[l].nel, L[l].mg_map, L[l + 1].coords, L[l].coords)
                if l > 0:
                    rc = self._sweep(l)
                    if rc:
                        return rc, np.array(rms)
        return 0, np.array(rms)

    def variables(self, l=0):
        return self.oc.array(l, "variables").reshape(-1, 5).copy()

    def close(self):
        self.oc.close()


def oracle_default_ff17(oracle):
    ff = oracle.farfield()
    return np.array(list(ff.var) + list(ff.fc_mx) + list(ff.fc_my) + list(ff.fc_mz) + list(ff.fc_de), dtype=np.float64)


def render_variables(v):
    """dump() of src/Base/io.cpp:201-233 as the golden variables.level0.txt files hold it."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 5)
    return "".join(" ".join("%.17e" % x for x in row) + "\n" for row in v)
