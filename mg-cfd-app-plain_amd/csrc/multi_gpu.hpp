// multi_gpu.hpp — euler3d_gpu_double --gpus N (multi_gpu.cpp).
#pragma once

#include <cstdint>
#include <vector>

#include "mgcfd.h"

namespace multi_gpu {

struct Options {
    int gpus = 1;
    int first_device = 0;
    bool share_device = false;        // --gpus-share-device: every rank on `first_device` (a functional rehearsal on a one-GPU box)
    bool fast_math = false;
    bool partition_levels = false;    // --gpus-partition: split EVERY level of a multigrid input over the ranks even when gpus <= levels
};

class Run {
public:
    struct Impl;
    Run(const mgcfd_mesh *mesh, const Options &opt);      // throws std::runtime_error
    ~Run();
    int ranks() const;
    bool partitioned() const;                              // true: the level(s) split over the ranks; false: one multigrid level per rank
    bool partitioned_hierarchy() const;                    // true: every level of a multigrid input split over the ranks (mgcfd_group_cycles)
    int run_cycles(int cycles, double *rms_out);           // MGCFD_OK or MGCFD_ERR_NAN / NEG_*
    // ... and the whole level-0 surface loads of every cycle, loads_out[cycles][6] (partitioned() runs only: mgcfd_group_cycles_loads)
    int run_cycles_loads(int cycles, const double ref_point[3], double *rms_out, double *loads_out);
    void far_field(double ff17[17]) const;
    // mgcfd_set_free_stream on every rank (the group's call where the ranks form one); MGCFD_OK or MGCFD_ERR_ARG
    int set_free_stream(double mach, double alpha_deg, int reinitialise);
    // mgcfd_set_time_step on every rank, likewise
    int set_time_step(int mode, double cfl);
    // mgcfd_set_residual_smoothing on every rank (one multigrid level per rank only: MGCFD_ERR_ARG where a level is split)
    int set_residual_smoothing(double eps, int iterations);
    // mgcfd_set_jst on every rank, likewise
    int set_jst(double kappa2, double kappa4, int levels);
    // mgcfd_set_viscous on every rank, likewise
    int set_viscous(double mu, double prandtl, int wall, double cfl_v, int levels);
    // mgcfd_set_dual_time (+ the BDF order) on every rank, likewise; advance: steps x (mgcfd_dual_time_begin_step on every rank +
    // cycles_per_step cycles), rms_out [steps * cycles_per_step]
    int set_dual_time(double dt, double clamp, int order);
    int advance(int steps, int cycles_per_step, double *rms_out);
    void get_level0(int which, int ncols, double *out) const;   // a level-0 array of the WHOLE mesh, original numbering
    int check_invalid(int level, int64_t *bad_cell) const;      // check_for_invalid_variables on `level` of the whole mesh (original cell id)
    void loop_iters(int level, int cycles, int64_t out[MGCFD_NUM_LOOPS]) const;
private:
    Impl *p;
};

} // namespace multi_gpu
