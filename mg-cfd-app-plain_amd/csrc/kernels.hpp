// kernels.hpp — launchers of kernels.hip, declared once per numeric flavour.
#pragma once

#include "device_plan.hpp"

#define MGCFD_DECLARE_LAUNCHERS(NS)                                                                                  \
    namespace mgcfd { namespace NS {                                                                                 \
    void launch_init_variables(hipStream_t, int64_t stride, const FarField &, double *q);                            \
    void launch_step_factor_local(hipStream_t, int64_t nel, int64_t stride, const double *q, const double *cbrt_vol, \
                                  double cfl, double *sf, double *partial_min, double *old_variables);               \
    void launch_min_reduce(hipStream_t, int64_t nel, const double *partial_min, double *out);                        \
    void launch_step_factor_apply(hipStream_t, int64_t nel, const double *min_dt_scalar,                             \
                                  const double *volumes, double *sf);                                                \
    void launch_step_factor_legacy(hipStream_t, int64_t nel, int64_t stride, const double *q, const double *volumes, \
                                   double cfl, double *sf, double *old_variables);                                   \
    void launch_step_factor_nodal(hipStream_t, int64_t nel, int64_t stride, const double *q, const double *cbrt_vol, \
                                  const double *volumes, double cfl, double *sf, double *old_variables);             \
    void launch_flux(hipStream_t, const DevicePlan &, const double *q, const FarField &, double *fluxes,             \
                     int classes, int accumulate, int variant, const FusedStep *fused, const StagePush *push);       \
    void launch_indirect_rw(hipStream_t, const DevicePlan &, const double *q, double *fluxes, int variant);                       \
    void launch_stream_tiles(hipStream_t, int n_tiles, const double *src, double *dst, int64_t rd_total, int64_t wr_total);      \
    void launch_time_step(hipStream_t, int64_t nel, int64_t stride, int j, double *sf, double *fluxes,               \
                          const double *old_variables, double *q, const int32_t *old_of_new,                         \
                          unsigned long long *err, int check, const double *partial_min, int n_partial,              \
                          const double *volumes, double *residuals, int zero_fluxes);                                \
    void launch_smooth(hipStream_t, const DevicePlan &, const SmoothStep &);                                          \
    void launch_jst_sensor(hipStream_t, const DevicePlan &, const JstStep &);                                        \
    void launch_jst_dissipation(hipStream_t, const DevicePlan &, const JstStep &);                                   \
    void launch_viscous_stress(hipStream_t, const DevicePlan &, const ViscousStep &);                                \
    void launch_viscous_flux(hipStream_t, const DevicePlan &, const ViscousStep &);                                  \
    void launch_viscous_clamp(hipStream_t, int64_t nel, double k0, const double *rho, const double *g, double *sf);  \
    void launch_viscous_clamp_variable(hipStream_t, int64_t nel, int64_t stride, const ViscousClamp &);              \
    void launch_viscous_wall(hipStream_t, int64_t n, int64_t stride, const int32_t *nodes, double *q, double *q2,    \
                             const double *old_variables, double *residuals);                                        \
    void launch_time_step_src(hipStream_t, int64_t nel, int64_t stride, int j, const double *sf,                     \
                              const double *fluxes, const double *forcing, const double *old_variables, double *q,  \
                              const int32_t *old_of_new, unsigned long long *err, int check, double *residuals,     \
                              const DualSource &);                                                                   \
    void launch_dual_source(hipStream_t, int64_t nel, int64_t stride, double *fluxes, const DualSource &);           \
    void launch_dual_clamp(hipStream_t, int64_t nel, double cdt, const double *volumes, double *sf);                 \
    void launch_dual_shift(hipStream_t, int64_t n, const double *q, double *wn, double *wn1, int first);             \
    void launch_check_invalid(hipStream_t, int64_t nel, int64_t stride, const double *q,                             \
                              const int32_t *old_of_new, unsigned long long *err);                                   \
    void launch_residual(hipStream_t, int64_t stride, const double *old_variables, const double *q,                  \
                         double *residuals);                                                                         \
    void launch_sumsq(hipStream_t, int64_t nel, int64_t stride, const double *x, double *partial, int n_partial,     \
                      double *out, const int32_t *old_of_new, int64_t n_owned);                                      \
    void launch_halo_pack(hipStream_t, int64_t n, int64_t stride, const int32_t *idx, const double *field,           \
                          double *msg);                                                                              \
    void launch_halo_unpack(hipStream_t, int64_t n, int64_t stride, const int32_t *idx, const double *msg,           \
                            double *field);                                                                          \
    void launch_halo_push(hipStream_t, int64_t n, int64_t stride, const int32_t *idx, const int32_t *target,         \
                          const double *field, const PushPeers &peers);                                              \
    void launch_halo_push_flags(hipStream_t, int64_t n, int64_t stride, const int32_t *idx, const int32_t *target,   \
                                const double *field, const PushPeers &peers, const PushFlags &flags,                 \
                                unsigned *ticket);                                                                   \
    void launch_flags_wait(hipStream_t, const unsigned long long *flags, const FlagRows &rows, int slot,             \
                           unsigned long long value, int *timed_out);                                                \
    void launch_min_publish(hipStream_t, const double *my_min, const MinPublish &mp);                                \
    void launch_append_scalar(hipStream_t, const double *src, double *ring, int *count, int cap);                    \
    void launch_sumsq_original(hipStream_t, int64_t nel, int64_t stride, const double *x, const int32_t *new_of_old, \
                               double *partial);                                                                     \
    void launch_min_over_peers(hipStream_t, const double *const *scalars, int n, double *out);                       \
    void launch_accept_restricted(hipStream_t, int64_t nel_coarse, int64_t stride_coarse, const int32_t *child_ptr,  \
                                  const double *src, double *coarse_q);                                              \
    void launch_sum_partials_append(hipStream_t, int n, const double *partial, double *out, double *ring,            \
                                    int *count, int cap);                                                            \
    void launch_restrict(hipStream_t, int64_t nel_coarse, int64_t stride_coarse, int64_t stride_fine,                \
                         const int32_t *child_ptr, const int32_t *child, const int32_t *child4, const double *fine_q, \
                         double *coarse_q,                                                                        \
                         const double *cbrt_vol, double cfl, double *partial_min, const SumTask &rms);              \
    void launch_surface_loads(hipStream_t, int64_t stride, const double *q, const LoadsTask &task);                  \
    void launch_wall_stress(hipStream_t, int64_t stride, const double *q, const WallStress &a);                      \
    void launch_wall_distance(hipStream_t, int64_t nel, int64_t stride, const WallDistance &a);                      \
    void launch_wall_spacing(hipStream_t, const WallSpacing &a);                                                     \
    void launch_wall_length(hipStream_t, int64_t stride, const WallLength &a);                                       \
    void launch_surface_loads_viscous(hipStream_t, int64_t stride, const double *q, const LoadsTaskViscous &task);   \
    void launch_wall_distribution(hipStream_t, int64_t stride, const double *q, const WallDistribution &a);          \
    void launch_loads_terms(hipStream_t, int64_t stride, const double *q, const LoadsTerms &task);                   \
    void launch_loads_scatter(hipStream_t, int64_t n, const double *src, int64_t src_row, const int32_t *slot,       \
                              double *table, int64_t row);                                                           \
    void launch_loads_reduce(hipStream_t, const double *table, int64_t row, const LoadsTask &task);                  \
    void launch_prolong(hipStream_t, const DevicePlan &, int64_t stride_coarse, const double *coarse_residuals,      \
                        const double *fine_residuals, double *fine_q, const double *cbrt_vol,                       \
                        double cfl, double *partial_min);                                                            \
    void launch_restrict_fas(hipStream_t, int64_t nel_coarse, int64_t stride_coarse, int64_t stride_fine,            \
                             const int32_t *child_ptr, const int32_t *child, const int32_t *child4,                  \
                             const double *fine_q, const double *fine_r, const double *fine_p, double *coarse_q,     \
                             double *w0, double *qsum);                                                              \
    void launch_fas_forcing(hipStream_t, int64_t nel_coarse, int64_t stride_coarse, const int32_t *child_ptr,        \
                            const double *fluxes, double *forcing);                                                  \
    void launch_fas_add_forcing(hipStream_t, int64_t stride, double *fluxes, const double *forcing);                 \
    void launch_prolong_fas(hipStream_t, const DevicePlan &, int64_t stride_coarse, const double *coarse_w0,         \
                            const double *coarse_q, double *fine_q, const double *cbrt_vol, double cfl,              \
                            double *partial_min);                                                                    \
    void launch_prolong_state(hipStream_t, const DevicePlan &, int64_t stride_coarse, const double *coarse_q,        \
                              double *fine_q, const double *cbrt_vol, double cfl, double *partial_min);              \
    } }

MGCFD_DECLARE_LAUNCHERS(exact)
MGCFD_DECLARE_LAUNCHERS(fast)

// The `fast` build only: 1/x and sqrt(x) as the order-free flux kernel computes them (mgcfd_diag_fast_math).
namespace mgcfd { namespace fast {
void launch_diag_fast_math(hipStream_t, int kind, int64_t n, const double *in, double *out);
} }

// The launchers whose numeric flavour follows MGCFD_OPT_EXACT (solver.cpp: mgcfd_solver::k() holds one table per flavour).
// Everything else is called as exact:: — those kernels do no arithmetic that contraction could change.
namespace mgcfd {
struct Launchers {
    decltype(exact::launch_step_factor_local) *step_factor_local;    decltype(exact::launch_step_factor_apply) *step_factor_apply;
    decltype(exact::launch_step_factor_legacy) *step_factor_legacy;  decltype(exact::launch_flux) *flux;
    decltype(exact::launch_indirect_rw) *indirect_rw;                decltype(exact::launch_time_step) *time_step;
    decltype(exact::launch_residual) *residual;                      decltype(exact::launch_sumsq) *sumsq;
    decltype(exact::launch_restrict) *restrict_;                     decltype(exact::launch_prolong) *prolong;
    decltype(exact::launch_step_factor_nodal) *step_factor_nodal;    decltype(exact::launch_smooth) *smooth;
    decltype(exact::launch_time_step_src) *time_step_src;            decltype(exact::launch_dual_source) *dual_source;
    decltype(exact::launch_jst_sensor) *jst_sensor;                  decltype(exact::launch_jst_dissipation) *jst_dissipation;
    decltype(exact::launch_restrict_fas) *restrict_fas;              decltype(exact::launch_prolong_fas) *prolong_fas;
    decltype(exact::launch_viscous_stress) *viscous_stress;          decltype(exact::launch_viscous_flux) *viscous_flux;
    decltype(exact::launch_prolong_state) *prolong_state;
};
}
