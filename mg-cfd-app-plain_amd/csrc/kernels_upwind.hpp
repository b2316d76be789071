// kernels_upwind.hpp — the launchers of kernels_upwind.hip: the upwind flux's kernels (limited MUSCL reconstruction and Roe's
// flux-difference splitting; mgcfd_set_upwind), one of each, never contracted.
#pragma once

#include "device_plan.hpp"

namespace mgcfd {

// The launches of the upwind flux (kernels_upwind.hip: k_upwind_gradient_tile, k_upwind_flux_tile; INTEGRATION.md "Upwind
// fluxes"): pass 1 writes gl and psi from w and x; pass 2 reads w (and, reconstructing, x and gl) and adds U into fluxes.
struct UpwindStep {
    const double *w = nullptr;                // the stage's input state W [5][stride]
    const double *x = nullptr;                // [3][stride] the level's coordinates as given at creation (MUSCL levels)
    const double *volumes = nullptr;          // [stride]
    double *gl = nullptr;                     // Gl [15][stride]: the limited gradient of (rho, u, v, w, p), field 3 * v + d
    double *psi = nullptr;                    // [5][stride] the limiter per variable
    double *fluxes = nullptr;                 // the stage's fluxes (pass 2 only): F = F + U
    int limiter = 0;                          // MGCFD_LIMITER_*
    double k3 = 0.0;                          // (k * k) * k, formed on the host (Venkatakrishnan)
    double entropy_fix = 0.0;                 // Harten's fraction; 0: none
};

// static LDS of the reconstructing flux kernel (23 fields of 560 doubles): above the 64 KB every device grants, so the host
// asks the device before the first launch
constexpr int kUpwindMusclLds = 23 * 560 * 8;

void launch_upwind_gradient(hipStream_t, const DevicePlan &p, const UpwindStep &a);
void launch_upwind_flux(hipStream_t, const DevicePlan &p, const UpwindStep &a, bool muscl);

} // namespace mgcfd
