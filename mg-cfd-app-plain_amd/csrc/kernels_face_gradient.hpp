// kernels_face_gradient.hpp — the launchers of kernels_face_gradient.hip: the corrected face gradient's kernels, one of each,
// never contracted.
#pragma once

#include "device_plan.hpp"

namespace mgcfd {

// the corrected face gradient (mgcfd_set_face_gradient): the node gradients G with me and kap behind the stress launch, then the
// correction Vc, Wk, Hc into fluxes behind the viscous-flux launch
void launch_face_gradient_nodes(hipStream_t, const DevicePlan &p, const FaceGradientStep &a);
void launch_face_gradient_correction(hipStream_t, const DevicePlan &p, const FaceGradientStep &a);

} // namespace mgcfd
