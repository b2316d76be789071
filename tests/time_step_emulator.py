"""The yardstick of the run-time time step (mgcfd_set_time_step): ``TimeStepOracle``, the composed oracle of
tests/free_stream_emulator.py with compute_step_factor replaced by numpy written from the definition in include/mgcfd.h /
INTEGRATION.md §8.  Every other kernel stays the oracle's entry point.

With derive()'s speed and c (src/Kernels/cfd_loops.h:121-148) and dt_i = cbrt(vol_i) / (speed_i + c_i):

    global        sf_i = min_j(cfl * dt_j) / vol_i                    cfd_loops.cpp:76-157
    local         sf_i = (cfl * dt_i) / vol_i
    local_legacy  sf_i = cfl / (sqrt(vol_i) * (speed_i + c_i))        cfd_loops.cpp:13-73
    reference     global, or local_legacy for mesh_name = fvcorr      euler3d_cpu_double.cpp:388-395

Every numpy operation below is one IEEE-754 double operation per element (numpy never contracts to FMA) and ``np.sqrt`` is
correctly rounded; ``cbrt`` is NOT taken from numpy, whose cbrt differs from libm's in the last bits, but from the host's
libm through ctypes — the function the reference and the library call.  tests/test_host_time_step.py checks on the CPU that
``global`` and ``local_legacy`` at cfl = 0.5 give ora_compute_step_factor's and ora_compute_step_factor_legacy's bits.
"""
import ctypes as C
import ctypes.util

import numpy as np

import free_stream_emulator as fse

MODES = ("reference", "global", "local", "local_legacy")
GAMMA = 1.4

# What the GPU tests run (tests/test_gpu_time_step.py): every golden case of fse.GPU_CASES under every (mode, cfl) below that
# applies to it, GPU_CYCLES cycles, none skipped.  tests/test_host_time_step.py asserts that each combination stays valid.
GPU_CASES = fse.GPU_CASES
GPU_CFLS = (0.5, 0.8, 1.5)
GPU_CYCLES = 3
RANK_CFL = 0.8                                   # the partitioned forms: local and global at this CFL number


def gpu_modes(case):
    """global everywhere (fvcorr included), local_legacy where the mesh name does not already select it, local everywhere."""
    return ("global", "local") if case.startswith("fvcorr") else ("global", "local_legacy", "local")


def gpu_combinations():
    return [(case, mode, cfl) for case in GPU_CASES for mode in gpu_modes(case) for cfl in GPU_CFLS]


_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cbrt.restype = C.c_double
_libm.cbrt.argtypes = [C.c_double]


def libm_cbrt(a):
    return np.array([_libm.cbrt(float(x)) for x in np.asarray(a, dtype=np.float64).ravel()], dtype=np.float64)


def speed_plus_c(variables):
    """derive() per node, in the oracle's order of operations (oracle/mgcfd_oracle.c: load_point, sound_speed)."""
    q = np.asarray(variables, dtype=np.float64).reshape(-1, 5)
    rho, en = q[:, 0], q[:, 4]
    vx, vy, vz = q[:, 1] / rho, q[:, 2] / rho, q[:, 3] / rho
    speed_sqd = vx * vx + vy * vy + vz * vz
    pressure = (GAMMA - 1.0) * (en - 0.5 * rho * speed_sqd)
    c = np.sqrt(GAMMA * pressure / rho)
    return np.sqrt(speed_sqd) + c


def step_factors(mode, cfl, variables, volumes, cbrt_vol, variant):
    """The step factors of one sweep from the definition; ``mode`` one of MODES, ``variant`` the mesh_name code."""
    assert mode in MODES
    if mode == "reference":
        mode = "local_legacy" if variant == 0 else "global"
    cfl = np.float64(cfl)
    s = speed_plus_c(variables)
    if mode == "local_legacy":
        return cfl / (np.sqrt(volumes) * s)
    dt = cbrt_vol / s
    if mode == "local":
        return (cfl * dt) / volumes
    return (cfl * dt).min() / volumes


class TimeStepOracle(fse.ComposedOracle):
    """ComposedOracle with the time-step mode and CFL number of mgcfd_set_time_step."""

    def __init__(self, oracle, case, mode="reference", cfl=0.5, ff17=None):
        super().__init__(oracle, case, ff17)
        self.cbrt_vol = [libm_cbrt(self.oc.array(l, "volumes")) for l in range(self.n)]
        self.set_time_step(mode, cfl)
        self.on_step_factors = None              # a test's hook: called with (level, step_factors view) every sweep

    def set_time_step(self, mode="reference", cfl=0.5):
        assert mode in MODES and np.isfinite(cfl) and cfl > 0.0
        self.mode, self.cfl = mode, float(cfl)

    def _sweep(self, l):
        """euler3d_cpu_double.cpp:383-508 with the step factor from the definition."""
        lib, L = self.lib, self.oc.levels[l]
        C.memmove(L.old_variables, L.variables, 8 * L.nel * 5)
        sf = self.oc.array(l, "step_factors")
        sf[:] = step_factors(self.mode, self.cfl, self.oc.array(l, "variables"), self.oc.array(l, "volumes"),
                             self.cbrt_vol[l], self.variant)
        if self.on_step_factors:
            self.on_step_factors(l, sf)
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

    def sweeps(self, l, count):
        """``count`` sweeps of level ``l`` alone (mgcfd_smooth): the return code of the first invalid stage, or 0."""
        for _ in range(count):
            rc = self._sweep(l)
            if rc:
                return rc
        return 0

    def step_factors(self, l):
        return self.oc.array(l, "step_factors").copy()
