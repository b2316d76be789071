// kernels_sa.hpp — the launchers of kernels_sa.hip: the Spalart-Allmaras model's kernels, one of each, never contracted.
#pragma once

#include "device_plan.hpp"

namespace mgcfd {

// the Spalart-Allmaras model: pass 1 (sa_gradient, eddy_viscosity), pass 2 (nu_tilde), the coarse levels' nt and mut, the start value
void launch_sa_gradient(hipStream_t, const DevicePlan &p, const SaStep &a);
// (x: the level's coordinates [3][stride] under the corrected face gradient, which adds Qdc; nullptr: the averaged gradient)
void launch_sa_transport(hipStream_t, const DevicePlan &p, const SaStep &a, const double *x = nullptr);
void launch_sa_restrict(hipStream_t, int64_t nel_coarse, int64_t stride_coarse, const int32_t *child_ptr, const int32_t *child,
                        const double *fine_nt, double *coarse_nt, const SaStep &a);
void launch_sa_init(hipStream_t, int64_t nel, int64_t stride, double nt0, const double *d, double *nt, const SaStep &a);

} // namespace mgcfd
