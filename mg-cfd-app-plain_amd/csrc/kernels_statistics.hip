// kernels_statistics.hip — the kernels of the flow statistics with their launchers (kernels_statistics.hpp: the prototypes in
// namespace mgcfd; INTEGRATION.md "Flow statistics").  Compiled ONCE, with -ffp-contract=off, as kernels_sa.hip is: nothing here is
// ever contracted, whichever flavour the solver runs.
#include "kernel_device.hpp"
#include "kernels_statistics.hpp"

namespace mgcfd {

// One weighted sample of a level's state (West's incremental form; the definition is in mgcfd.h): one lane per node, SoA.
//   x = (rho, u, v, w_, p, mut) by k_wall_distribution's expressions;  d = x - m (old mean);  m = m + a * d;  e = x - m (new mean);
//   c[pair(r, s)] = c[pair(r, s)] + (w * d[r]) * e[s]  over  uu vv ww uv uw vw pp.
// Every lane's 18 (MUT: 19) loads are independent of one another and are issued before the first use; the accumulators are
// stored write-through (MGCFD_ST_STAGE): nothing reads them again before the next physical step, and a line left dirty in L2
// would only be written back under the next launch.  Pad lanes nel .. stride are skipped.
// (waves_per_eu 1..4: at the default target of eight waves the compiler keeps to 64 VGPRs and sinks four of the loads behind
// the divisions; with room for 88 it issues them all up front, four workgroups per CU with 19 loads in flight per lane)
template <bool MUT>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, 4)))
k_statistics_sample(int64_t nel, int64_t stride, const double *__restrict__ q, const double *__restrict__ mut,
                    double *__restrict__ mean, double *__restrict__ moments, double a, double w)
{
#pragma clang fp contract(off)
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (i >= nel) return;
    const double rho = q[i], mx = q[stride + i], my = q[2 * stride + i], mz = q[3 * stride + i], en = q[4 * stride + i];
    double x[6], m[6], c[7];
    x[5] = 0.0;
    if constexpr (MUT) x[5] = mut[i];
#pragma unroll
    for (int k = 0; k < 6; k++) m[k] = mean[k * stride + i];
#pragma unroll
    for (int k = 0; k < 7; k++) c[k] = moments[k * stride + i];
    const double u = mx / rho, v = my / rho, w_ = mz / rho;
    const double speed_sqd = u * u + v * v + w_ * w_;
    x[0] = rho; x[1] = u; x[2] = v; x[3] = w_;
    x[4] = (kGamma - 1.0) * (en - 0.5 * rho * speed_sqd);
    double d[6], e[6];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        d[k] = x[k] - m[k];
        m[k] = m[k] + a * d[k];
        e[k] = x[k] - m[k];
    }
    const double wu = w * d[1], wv = w * d[2], ww = w * d[3], wp = w * d[4];
    c[0] = c[0] + wu * e[1];
    c[1] = c[1] + wv * e[2];
    c[2] = c[2] + ww * e[3];
    c[3] = c[3] + wu * e[2];
    c[4] = c[4] + wu * e[3];
    c[5] = c[5] + wv * e[3];
    c[6] = c[6] + wp * e[4];
#pragma unroll
    for (int k = 0; k < 6; k++) MGCFD_ST_STAGE(mean + k * stride + i, m[k]);
#pragma unroll
    for (int k = 0; k < 7; k++) MGCFD_ST_STAGE(moments + k * stride + i, c[k]);
}

// One weighted sample of the wall distribution: one lane per wall node.  Columns 3 .. 6 (dp | tx ty tz) of dist's row into the
// table's row: mean [4] | M2 [4], by the same recurrence, M2[k] = M2[k] + (w * d[k]) * e[k].
__global__ void __launch_bounds__(kBlock)
k_statistics_wall(int64_t n, const double *__restrict__ dist, double *__restrict__ table, double a, double w)
{
#pragma clang fp contract(off)
    const int64_t k = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (k >= n) return;
    const double *x = dist + 7 * k + 3;
    double *t = table + 8 * k;
    double xs[4], m[4], m2[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { xs[j] = x[j]; m[j] = t[j]; m2[j] = t[4 + j]; }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const double d = xs[j] - m[j];
        m[j] = m[j] + a * d;
        const double e = xs[j] - m[j];
        m2[j] = m2[j] + (w * d) * e;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) { t[j] = m[j]; t[4 + j] = m2[j]; }
}

// ==========================================================================================
// launchers
// ==========================================================================================
void launch_statistics_sample(hipStream_t st, int64_t nel, int64_t stride, const double *q, const double *mut, double *mean, double *moments,
                              double a, double w)
{
    if (nel <= 0) return;
    if (mut) hipLaunchKernelGGL(k_statistics_sample<true>, dim3(grid_for(nel)), dim3(kBlock), 0, st, nel, stride, q, mut, mean, moments, a, w);
    else hipLaunchKernelGGL(k_statistics_sample<false>, dim3(grid_for(nel)), dim3(kBlock), 0, st, nel, stride, q, mut, mean, moments, a, w);
}
void launch_statistics_wall(hipStream_t st, int64_t n, const double *dist, double *table, double a, double w)
{ if (n > 0) hipLaunchKernelGGL(k_statistics_wall, dim3(grid_for(n)), dim3(kBlock), 0, st, n, dist, table, a, w); }

} // namespace mgcfd
