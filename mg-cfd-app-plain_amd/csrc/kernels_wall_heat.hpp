// kernels_wall_heat.hpp — the launchers of kernels_wall_heat.hip: the wall thermal conditions' kernels, one of each, never contracted.
#pragma once

#include "device_plan.hpp"

namespace mgcfd {

// the isothermal wall launch (k_viscous_wall's place while that mode is in effect), the heat-flux wall's addition into fluxes[][4]
// and the heat table (a.out [n][3] = h T area)
void launch_viscous_wall_isothermal(hipStream_t, int64_t n, int64_t stride, const int32_t *nodes, double ew, double *q, double *q2,
                                    const double *old_variables, double *residuals);
void launch_wall_heat_flux(hipStream_t, int64_t n, int64_t stride, const int32_t *nodes, const double *area, double qw, double *fluxes);
void launch_wall_heat(hipStream_t, int64_t stride, const double *q, const WallDistribution &a);

} // namespace mgcfd
