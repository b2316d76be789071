// kernels.hpp — the launchers of kernels.hip (two numeric flavours each) and of kernels_plain.hip (one of each).
#pragma once

#include "device_plan.hpp"

// The launchers that exist in two flavours, mgcfd::exact:: (-ffp-contract=off) and mgcfd::fast:: (contracted), named ONCE:
// X(member, launcher, (parameters)).  The declarations in both namespaces, struct Launchers and the two tables of
// mgcfd_solver::k() (solver.cpp) are all generated from this list, every table entry by its member's name.
#define MGCFD_L(X, name, params) X(name, launch_##name, params)       /* member `name`, launcher `launch_name` */
#define MGCFD_FLAVOURED_LAUNCHERS(X)                                                                                 \
    MGCFD_L(X, step_factor_local, (hipStream_t, int64_t nel, int64_t stride, const double *q, const double *cbrt_vol, \
                                   double cfl, double *sf, double *partial_min, double *old_variables))              \
    MGCFD_L(X, step_factor_apply, (hipStream_t, int64_t nel, const double *min_dt_scalar, const double *volumes,     \
                                   double *sf))                                                                      \
    MGCFD_L(X, step_factor_legacy, (hipStream_t, int64_t nel, int64_t stride, const double *q, const double *volumes, \
                                    double cfl, double *sf, double *old_variables))                                  \
    MGCFD_L(X, step_factor_nodal, (hipStream_t, int64_t nel, int64_t stride, const double *q, const double *cbrt_vol, \
                                   const double *volumes, double cfl, double *sf, double *old_variables))            \
    MGCFD_L(X, flux, (hipStream_t, const DevicePlan &, const double *q, const FarField &, double *fluxes, int classes, \
                      int accumulate, int variant, const FusedStep *fused, const StagePush *push))                   \
    MGCFD_L(X, indirect_rw, (hipStream_t, const DevicePlan &, const double *q, double *fluxes, int variant))         \
    MGCFD_L(X, time_step, (hipStream_t, int64_t nel, int64_t stride, int j, double *sf, double *fluxes,              \
                           const double *old_variables, double *q, const int32_t *old_of_new,                        \
                           unsigned long long *err, int check, const double *partial_min, int n_partial,             \
                           const double *volumes, double *residuals, int zero_fluxes))                               \
    MGCFD_L(X, time_step_src, (hipStream_t, int64_t nel, int64_t stride, int j, const double *sf,                    \
                               const double *fluxes, const double *forcing, const double *old_variables, double *q, \
                               const int32_t *old_of_new, unsigned long long *err, int check, double *residuals,    \
                               const DualSource &))                                                                  \
    MGCFD_L(X, dual_source, (hipStream_t, int64_t nel, int64_t stride, double *fluxes, const DualSource &))          \
    MGCFD_L(X, smooth, (hipStream_t, const DevicePlan &, const SmoothStep &))                                        \
    MGCFD_L(X, jst_sensor, (hipStream_t, const DevicePlan &, const JstStep &))                                       \
    MGCFD_L(X, jst_dissipation, (hipStream_t, const DevicePlan &, const JstStep &))                                  \
    MGCFD_L(X, viscous_stress, (hipStream_t, const DevicePlan &, const ViscousStep &))                               \
    MGCFD_L(X, viscous_flux, (hipStream_t, const DevicePlan &, const ViscousStep &))                                 \
    MGCFD_L(X, residual, (hipStream_t, int64_t stride, const double *old_variables, const double *q,                 \
                          double *residuals))                                                                        \
    MGCFD_L(X, sumsq, (hipStream_t, int64_t nel, int64_t stride, const double *x, double *partial, int n_partial,    \
                       double *out, const int32_t *old_of_new, int64_t n_owned))                                     \
    X(restrict_, launch_restrict, (hipStream_t, int64_t nel_coarse, int64_t stride_coarse, int64_t stride_fine,      \
                                   const int32_t *child_ptr, const int32_t *child, const int32_t *child4,            \
                                   const double *fine_q, double *coarse_q, const double *cbrt_vol, double cfl,       \
                                   double *partial_min, const SumTask &rms))                                         \
    MGCFD_L(X, restrict_fas, (hipStream_t, int64_t nel_coarse, int64_t stride_coarse, int64_t stride_fine,           \
                              const int32_t *child_ptr, const int32_t *child, const int32_t *child4,                 \
                              const double *fine_q, const double *fine_r, const double *fine_p, double *coarse_q,    \
                              double *w0, double *qsum))                                                             \
    MGCFD_L(X, prolong, (hipStream_t, const DevicePlan &, int64_t stride_coarse, const double *coarse_residuals,     \
                         const double *fine_residuals, double *fine_q, const double *cbrt_vol, double cfl,           \
                         double *partial_min))                                                                       \
    MGCFD_L(X, prolong_fas, (hipStream_t, const DevicePlan &, int64_t stride_coarse, const double *coarse_w0,        \
                             const double *coarse_q, double *fine_q, const double *cbrt_vol, double cfl,             \
                             double *partial_min))                                                                   \
    MGCFD_L(X, prolong_state, (hipStream_t, const DevicePlan &, int64_t stride_coarse, const double *coarse_q,       \
                               double *fine_q, const double *cbrt_vol, double cfl, double *partial_min))

#define MGCFD_DECLARE_LAUNCHER(member, launcher, params) void launcher params;
#define MGCFD_LAUNCHER_MEMBER(member, launcher, params) void (*member) params;
namespace mgcfd {
namespace exact { MGCFD_FLAVOURED_LAUNCHERS(MGCFD_DECLARE_LAUNCHER) }
namespace fast {
MGCFD_FLAVOURED_LAUNCHERS(MGCFD_DECLARE_LAUNCHER)
// The `fast` build only: 1/x and sqrt(x) as the order-free flux kernel computes them (mgcfd_diag_fast_math).
void launch_diag_fast_math(hipStream_t, int kind, int64_t n, const double *in, double *out);
}
// One flavour's launchers; which table a solver uses follows MGCFD_OPT_EXACT (solver.cpp: mgcfd_solver::k()).
struct Launchers { MGCFD_FLAVOURED_LAUNCHERS(MGCFD_LAUNCHER_MEMBER) };
}
#undef MGCFD_DECLARE_LAUNCHER
#undef MGCFD_LAUNCHER_MEMBER

// The launchers of kernels_plain.hip.
namespace mgcfd {
void launch_init_variables(hipStream_t, int64_t stride, const FarField &, double *q);
void launch_min_reduce(hipStream_t, int64_t nel, const double *partial_min, double *out);
void launch_stream_tiles(hipStream_t, int n_tiles, const double *src, double *dst, int64_t rd_total, int64_t wr_total);
void launch_viscous_clamp(hipStream_t, int64_t nel, double k0, const double *rho, const double *g, double *sf);
void launch_viscous_clamp_variable(hipStream_t, int64_t nel, int64_t stride, const ViscousClamp &);
void launch_viscous_wall(hipStream_t, int64_t n, int64_t stride, const int32_t *nodes, double *q, double *q2,
                         const double *old_variables, double *residuals);
void launch_dual_clamp(hipStream_t, int64_t nel, double cdt, const double *volumes, double *sf);
void launch_dual_shift(hipStream_t, int64_t n, const double *q, double *wn, double *wn1, int first);
void launch_check_invalid(hipStream_t, int64_t nel, int64_t stride, const double *q, const int32_t *old_of_new,
                          unsigned long long *err);
void launch_halo_pack(hipStream_t, int64_t n, int64_t stride, const int32_t *idx, const double *field, double *msg);
void launch_halo_unpack(hipStream_t, int64_t n, int64_t stride, const int32_t *idx, const double *msg, double *field);
void launch_halo_push(hipStream_t, int64_t n, int64_t stride, const int32_t *idx, const int32_t *target,
                      const double *field, const PushPeers &peers);
void launch_halo_push_flags(hipStream_t, int64_t n, int64_t stride, const int32_t *idx, const int32_t *target,
                            const double *field, const PushPeers &peers, const PushFlags &flags, unsigned *ticket);
void launch_flags_wait(hipStream_t, const unsigned long long *flags, const FlagRows &rows, int slot,
                       unsigned long long value, int *timed_out);
void launch_min_publish(hipStream_t, const double *my_min, const MinPublish &mp);
void launch_append_scalar(hipStream_t, const double *src, double *ring, int *count, int cap);
void launch_sumsq_original(hipStream_t, int64_t nel, int64_t stride, const double *x, const int32_t *new_of_old,
                           double *partial);
void launch_min_over_peers(hipStream_t, const double *const *scalars, int n, double *out);
void launch_accept_restricted(hipStream_t, int64_t nel_coarse, int64_t stride_coarse, const int32_t *child_ptr,
                              const double *src, double *coarse_q);
void launch_sum_partials_append(hipStream_t, int n, const double *partial, double *out, double *ring, int *count,
                                int cap);
void launch_surface_loads(hipStream_t, int64_t stride, const double *q, const LoadsTask &task);
void launch_wall_stress(hipStream_t, int64_t stride, const double *q, const WallStress &a);
void launch_wall_distance(hipStream_t, int64_t nel, int64_t stride, const WallDistance &a);
void launch_wall_spacing(hipStream_t, const WallSpacing &a);
void launch_wall_length(hipStream_t, int64_t stride, const WallLength &a);
// (columns = 14: the heat loads' Q and A behind the twelve, task.base.partial [14][..], rows of 14)
void launch_surface_loads_viscous(hipStream_t, int64_t stride, const double *q, const LoadsTaskViscous &task, int columns = 12);
void launch_wall_distribution(hipStream_t, int64_t stride, const double *q, const WallDistribution &a);
void launch_loads_terms(hipStream_t, int64_t stride, const double *q, const LoadsTerms &task);
void launch_loads_scatter(hipStream_t, int64_t n, const double *src, int64_t src_row, const int32_t *slot,
                          double *table, int64_t row);
void launch_loads_reduce(hipStream_t, const double *table, int64_t row, const LoadsTask &task);
void launch_fas_forcing(hipStream_t, int64_t nel_coarse, int64_t stride_coarse, const int32_t *child_ptr,
                        const double *fluxes, double *forcing);
void launch_fas_add_forcing(hipStream_t, int64_t stride, double *fluxes, const double *forcing);
}

// The rule: a launcher has two flavours exactly if MGCFD_FLAVOURED_LAUNCHERS lists it (launch_diag_fast_math beside the
// list: fast only).  Everything else exists once, in kernels_plain.hip (the Spalart-Allmaras model's: kernels_sa.hip, kernels_sa.hpp; the wall thermal conditions': kernels_wall_heat.hip, kernels_wall_heat.hpp; the corrected face gradient's: kernels_face_gradient.hip, kernels_face_gradient.hpp), compiled with -ffp-contract=off: never contracted,
// whichever flavour the solver runs.  So an `exact::` or `fast::` at a call site is always a deliberate choice of flavour.
