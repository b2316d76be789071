// kernels_wall_heat.hip — the kernels of the wall thermal conditions with their launchers (kernels_wall_heat.hpp: the prototypes
// in namespace mgcfd; INTEGRATION.md "Wall thermal conditions").  Compiled ONCE, with -ffp-contract=off, as kernels_plain.hip is:
// nothing here is ever contracted, whichever flavour the solver runs.  The heat loads' fourteen-column sums are an instantiation
// of k_surface_loads_viscous and live with it in kernels_plain.hip.
#include "kernel_device.hpp"
#include "kernels_wall_heat.hpp"

namespace mgcfd {

// The isothermal no-slip wall (mgcfd_set_wall_temperature, INTEGRATION.md "Wall thermal conditions"): k_viscous_wall's
// launch with the energy held at the wall temperature beside it, energy = density * ew with ew = Tw / (GAMMA - 1.0) from
// the host — q2 from its own density — and the energy residual of the state it leaves.  Density stays.
__global__ void __launch_bounds__(kBlock)
k_viscous_wall_isothermal(int64_t n, int64_t stride, const int32_t *__restrict__ nodes, double ew, double *__restrict__ q,
                          double *__restrict__ q2, const double *__restrict__ old_variables, double *__restrict__ residuals)
{
#pragma clang fp contract(off)
    const int64_t k = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (k >= n) return;
    const int64_t i = nodes[k];
#pragma unroll
    for (int v = 1; v <= 3; v++) {
        q[v * stride + i] = 0.0;
        if (q2) q2[v * stride + i] = 0.0;
        if (residuals) residuals[v * stride + i] = 0.0 - old_variables[v * stride + i];
    }
    const double en = q[i] * ew;
    q[4 * stride + i] = en;
    if (q2) q2[4 * stride + i] = q2[i] * ew;
    if (residuals) residuals[4 * stride + i] = en - old_variables[4 * stride + i];
}

// The heat-flux wall: fluxes[i][4] = fluxes[i][4] + qw * area_i at the n listed wall nodes, behind the viscous-flux launch.
__global__ void __launch_bounds__(kBlock)
k_wall_heat_flux(int64_t n, int64_t stride, const int32_t *__restrict__ nodes, const double *__restrict__ area, double qw,
                 double *__restrict__ fluxes)
{
#pragma clang fp contract(off)
    const int64_t k = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (k >= n) return;
    const int64_t at = 4 * stride + nodes[k];
    fluxes[at] = fluxes[at] + qw * area[k];
}

// The heat table: one lane per wall node, as k_wall_distribution.  a = the sum of its solid-wall weights from +0.0 in record
// order, h = -(q . a) from the node's heat flux in Sw (+0.0 without it), T = p / rho by k_surface_loads' pressure, area = |a|.
__global__ void __launch_bounds__(kBlock)
k_wall_heat(int64_t stride, const double *__restrict__ q, WallDistribution a)
{
#pragma clang fp contract(off)
    const int64_t k = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (k >= a.wn.n) return;
    const int64_t b = a.wn.node[k];
    double ax = 0.0, ay = 0.0, az = 0.0;
    for (int32_t j = a.wn.wall_ptr[k]; j < a.wn.wall_ptr[k + 1]; j++) {
        const WallRecord &r = a.rec[a.wn.wall_edge[j]];
        ax += r.x; ay += r.y; az += r.z;
    }
    const double rho = q[b], mx = q[stride + b], my = q[2 * stride + b], mz = q[3 * stride + b], en = q[4 * stride + b];
    const double vx = mx / rho, vy = my / rho, vz = mz / rho;
    const double speed_sqd = vx * vx + vy * vy + vz * vz;
    const double p = (kGamma - 1.0) * (en - 0.5 * rho * speed_sqd);
    double h = 0.0;
    if (a.sw) {
        const double *s = a.sw + k;
        const double qx = s[9 * a.wn.n], qy = s[10 * a.wn.n], qz = s[11 * a.wn.n];
        h = -((qx * ax + qy * ay) + qz * az);
    }
    double *o = a.out + 3 * k;
    o[0] = h; o[1] = p / rho; o[2] = sqrt((ax * ax + ay * ay) + az * az);
}

// ==========================================================================================
// launchers
// ==========================================================================================
void launch_viscous_wall_isothermal(hipStream_t st, int64_t n, int64_t stride, const int32_t *nodes, double ew, double *q, double *q2,
                                    const double *old_variables, double *residuals)
{ if (n > 0) hipLaunchKernelGGL(k_viscous_wall_isothermal, dim3(grid_for(n)), dim3(kBlock), 0, st, n, stride, nodes, ew, q, q2, old_variables, residuals); }
void launch_wall_heat_flux(hipStream_t st, int64_t n, int64_t stride, const int32_t *nodes, const double *area, double qw, double *fluxes)
{ if (n > 0) hipLaunchKernelGGL(k_wall_heat_flux, dim3(grid_for(n)), dim3(kBlock), 0, st, n, stride, nodes, area, qw, fluxes); }
void launch_wall_heat(hipStream_t st, int64_t stride, const double *q, const WallDistribution &a)
{ if (a.wn.n > 0) hipLaunchKernelGGL(k_wall_heat, dim3(grid_for(a.wn.n)), dim3(kBlock), 0, st, stride, q, a); }

} // namespace mgcfd
