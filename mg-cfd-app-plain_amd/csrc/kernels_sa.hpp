// kernels_sa.hpp — the launchers of kernels_sa.hip: the Spalart-Allmaras model's kernels, one of each, never contracted.
#pragma once

#include "device_plan.hpp"

namespace mgcfd {

// the Spalart-Allmaras model: pass 1 (sa_gradient, eddy_viscosity), pass 2 (nu_tilde), the coarse levels' nt and mut, the start value
// (shield: delayed DES, which writes the model length d~ too; nullptr: the plain pass 1)
void launch_sa_gradient(hipStream_t, const DevicePlan &p, const SaStep &a, const SaShield *shield = nullptr);
// (x: the level's coordinates [3][stride] under the corrected face gradient, which adds Qdc; nullptr: the averaged gradient.
//  time: the physical-time source of nt under dual time stepping; nullptr: none)
void launch_sa_transport(hipStream_t, const DevicePlan &p, const SaStep &a, const double *x = nullptr, const SaTime *time = nullptr);
// the DES97 length d~ = min(d, c_des * delta) per node (delayed DES: until the first pass 1)
void launch_sa_length(hipStream_t, int64_t nel, int64_t stride, const SaShield &a);
void launch_sa_restrict(hipStream_t, int64_t nel_coarse, int64_t stride_coarse, const int32_t *child_ptr, const int32_t *child,
                        const double *fine_nt, double *coarse_nt, const SaStep &a);
void launch_sa_init(hipStream_t, int64_t nel, int64_t stride, double nt0, const double *d, double *nt, const SaStep &a);

} // namespace mgcfd
