// kernels_statistics.hpp — the launchers of kernels_statistics.hip: the flow statistics' kernels, one of each, never contracted.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mgcfd {

// One sample of a level's state into the volume accumulators (INTEGRATION.md "Flow statistics"): q [5][stride], mut [stride] or
// nullptr (the mut column then samples +0.0 and the array is not read), mean [6][stride], moments [7][stride];
// a = w / (wsum + w) and the weight w come from the host.
void launch_statistics_sample(hipStream_t, int64_t nel, int64_t stride, const double *q, const double *mut, double *mean, double *moments,
                              double a, double w);
// One sample of a wall distribution table dist [n][7] (its dp | tx ty tz columns) into the wall table [n][8].
void launch_statistics_wall(hipStream_t, int64_t n, const double *dist, double *table, double a, double w);

} // namespace mgcfd
