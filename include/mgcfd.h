/*
 * mgcfd.h — C ABI of libmgcfd_hip.so: the MI355X (gfx950) implementation of
 * MG-CFD's edge-flux / multigrid hot path.
 *
 * The reference (warwick-hpsc/MG-CFD-app-plain) has no plugin/FFI layer: its
 * hot path is a set of free functions on caller-owned host arrays
 * (src/Kernels/{flux_loops,cfd_loops,mg_loops,validation}.h) driven by main()
 * (src/euler3d_cpu_double.cpp:371-694).  This header exports that same set at
 * the same granularity behind an opaque handle that keeps the mesh and the
 * state resident in HBM; every entry point names the reference function it
 * replaces.  Plain C types only, no exceptions cross the boundary, no exit():
 * every call returns MGCFD_OK or an error code and mgcfd_last_error() explains.
 *
 * Numbering: callers always see the reference's ORIGINAL node and edge
 * numbering; the library renumbers internally and permutes on the way in/out.
 * Threading: one host thread per solver handle (as the reference's main()).
 */
#ifndef MGCFD_H
#define MGCFD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGCFD_NVAR 5   /* src/Base/const.h:29  (rho, rho*u, rho*v, rho*w, rho*E) */
#define MGCFD_RK 3     /* src/Base/const.h:13 */

/* mesh_name codes — src/Base/const.h:40-43 */
#define MGCFD_MESH_FVCORR 0
#define MGCFD_MESH_M6_WING 2
#define MGCFD_MESH_LA_CASCADE 3
#define MGCFD_MESH_ROTOR_37 4

/* error codes */
#define MGCFD_OK 0
#define MGCFD_ERR_ARG 1        /* bad argument / level out of range */
#define MGCFD_ERR_IO 2         /* file missing or malformed */
#define MGCFD_ERR_HIP 3        /* HIP runtime failure (no device, OOM, launch error) */
#define MGCFD_ERR_NAN 4        /* check_for_invalid_variables: NaN/Inf          (validation.cpp:112-121) */
#define MGCFD_ERR_NEG_DENSITY 5 /* ... negative density                         (validation.cpp:124-128) */
#define MGCFD_ERR_NEG_ENERGY 6  /* ... negative density*energy                  (validation.cpp:130-134) */
#define MGCFD_ERR_VALIDATION 7 /* identify_differences found a value out of tolerance (validation.cpp:140-199) */

/* Loop ids: the columns of Times.csv / LoopNumIters.csv in file order
 * (src/Monitoring/timer.cpp:135-144, src/Base/const.h:31-38 names). */
enum { MGCFD_LOOP_FLUX = 0, MGCFD_LOOP_UPDATE, MGCFD_LOOP_COMPUTE_STEP, MGCFD_LOOP_TIME_STEP,
       MGCFD_LOOP_RESTRICT, MGCFD_LOOP_PROLONG, MGCFD_LOOP_INDIRECT_RW, MGCFD_NUM_LOOPS };

/* Per-level arrays a caller can read back / overwrite (reference: the arrays main() owns,
 * src/euler3d_cpu_double.cpp:138-162). */
enum { MGCFD_ARR_VARIABLES = 0, MGCFD_ARR_OLD_VARIABLES, MGCFD_ARR_FLUXES, MGCFD_ARR_RESIDUALS,
       MGCFD_ARR_STEP_FACTORS, MGCFD_ARR_VOLUMES,
       MGCFD_ARR_STAGE /* the state the last mgcfd_sweep_stage wrote (halo messages between the stages of a split sweep) */,
       MGCFD_ARR_TIME_N, MGCFD_ARR_TIME_N1 /* dual time stepping's time levels Wn and Wn1 (while mgcfd_set_dual_time has it on) */,
       MGCFD_ARR_JST_LAPLACIAN, MGCFD_ARR_JST_SENSOR, MGCFD_ARR_JST_RADIUS /* read-only: L [nel][5], nu [nel] and r [nel] of the last
                                 flux launch of a level the JST dissipation is on for (mgcfd_set_jst) */,
       MGCFD_ARR_FAS_FORCING, MGCFD_ARR_FAS_START /* read-only, levels >= 1 while FAS multigrid is on (mgcfd_set_fas): the forcing P and
                                 the start state W0 [nel][5] of the last mgcfd_fas_restrict onto the level */,
       MGCFD_ARR_VISCOUS_STRESS /* read-only: the node stresses S [nel][12] of the last flux launch of a level the viscous terms are on
                                 for (mgcfd_set_viscous): u v w | txx tyy tzz txy txz tyz | qx qy qz */,
       MGCFD_ARR_EDDY_VISCOSITY /* the eddy viscosity mut [nel] of a viscous level under mgcfd_set_viscosity_model: the caller's to
                                 write under MGCFD_EDDY_FIELD, read-only (the last stress launch's) under MGCFD_EDDY_SMAGORINSKY */ };

/* Solver options (mgcfd_set_option) */
enum {
    MGCFD_OPT_EXACT = 0,       /* 1 (default): kernels compiled without FMA contraction and summing in the
                                  reference's order => bit-identical to the reference built with
                                  -ffp-contract=off, and the same bits from run to run.
                                  0: the fast mode — FMA contraction allowed AND, with MGCFD_OPT_FLUX_VARIANT = -1, the
                                  order-free flux kernel wherever a level has its plan (bit 6 below): within 1e-12 relative
                                  of the reference per sweep (north_star allows 1e-10), but NOT reproducible bit for bit
                                  from run to run, nor between a whole level and the same level partitioned (a launch over
                                  part of a level takes the node gather).  MGCFD_OPT_EXACT = 0 with MGCFD_OPT_FLUX_VARIANT = 1
                                  is the deterministic contracted mode (the node gather only). */
    MGCFD_OPT_TIMING = 1,      /* 1: bracket every loop with hipEvents (Times.csv columns; every loop its own launch, as the
                                  reference's -DTIME build brackets them, src/Monitoring/timer.cpp:58-195); 2: only the flux launches
                                  of every 8th sweep; 3: as 2 for every sweep (reads back as 2);
                                  4: per-loop times by ATTRIBUTION — the cycles run the fused stages; every 32nd sweep and every 32nd
                                  restriction / prolongation of a level runs per loop under events (the indirect_rw probe in
                                  every fourth of those, its column extrapolated at the measured rate), one event pair brackets each batch of cycles, and mgcfd_get_loop_times apportions the
                                  batches' GPU time to (level, loop) by the sampled launches' ratios: all seven columns at
                                  ~1.05x the fused cycle time instead of 2.7x (what euler3d_gpu_double runs by default) */
    MGCFD_OPT_INDIRECT_RW = 2, /* 1: also run the indirect_rw probe each RK stage, as the reference's main() does */
    MGCFD_OPT_CHECK_INVALID = 3, /* 1 (default): NaN / negativity check every RK stage (validation.cpp:107-138) */
    MGCFD_OPT_FLUX_VARIANT = 4, /* -1 (default): automatic — 1 (the edge-length factor recomputed: never slower on an
                                   MI355X, faster once a level's rows outgrow the Infinity Cache).  Otherwise a bit set:
                                   bit 0: 0 edge-length factor streamed, 1 recomputed from the weights;
                                   bit 2 (4): two-phase design point — edge fluxes written to memory, then a node-centred
                                   sum (the reference's FLUX_FISSION idea); kernel-granular and unfused sweeps only;
                                   bit 3 (8): the indirect_rw probe in its L1-gather form (32-bit neighbour codes).
                                   Every variant above gives bit-identical results.
                                   bits 1 (2), 4 (16) and 5 (32): removed, refused.  They selected the edge-once tiles, the
                                   indexed weights and the ordered half-row kernel, three bit-identical layouts that lost to
                                   the node gather (EXPERIMENTS.md); a value >= 0 with one of them set returns MGCFD_ERR_ARG
                                   and leaves the option as it was.
                                   bit 6 (64), with MGCFD_OPT_EXACT = 0 only (the bit-identical kernels ignore it): ORDER-FREE
                                   accumulation over the half-row plan (k_flux_free) — every internal edge of a tile evaluated
                                   once, the other end's share added to its LDS sum with fp64 LDS atomics, no ordered hand-over.
                                   Sums are associated differently from the reference's (src/Kernels/flux_loops.cpp:133-136 adds
                                   in edge order) and are not reproducible bit for bit from run to run: <= 1e-12 relative per
                                   launch, <= 1e-10 after 25 V-cycles, the reference's -v rule (validation.cpp:159-166) passes;
                                   tests/test_gpu_order_free.py.  Levels without a half-row plan run the node gather.
                                   With MGCFD_OPT_EXACT = 0 the automatic choice (-1) sets this bit where the kernel is the faster
                                   one: for every standalone flux launch of a level that has the plan, for the fused stages of
                                   levels with long rows or tile halos beyond the shared table (tetrahedral levels) and — round 4:
                                   role-specialised stages — of levels on the kernel's fast path (halos of at most 290 nodes, at
                                   most five evaluations per lane: the lattice-like levels of the named meshes). */
    MGCFD_OPT_FUSE_UPDATE = 5, /* 1 (default): mgcfd_smooth / mgcfd_run_cycles run each Runge-Kutta stage as ONE
                                  launch (fluxes + time_step, same operations); 0: one launch per loop */
    MGCFD_OPT_GRAPH = 6,       /* 1: replay each smoothing sweep / multigrid cycle from a captured hipGraph (one host
                                  call instead of 3 / ~24 launches).  0 (default): launch the kernels directly — on
                                  ROCm 7.2 / MI355X the graph costs ~1.7 us per kernel node more than direct launches
                                  (sweep 75 us replayed, 70 us launched), so it only pays when the host cannot keep
                                  the queue full */
    MGCFD_OPT_RANK_SPLIT = 7,  /* ranks in different processes, direct stores (mgcfd_rank_ipc_*): 1 (default) a stage runs its
                                  boundary tiles first, sends, then the interior tiles (the message's flight is hidden);
                                  0: all tiles in ONE launch, then the message (two launches less per stage, the flight
                                  exposed); 2: ONE launch that sends its own message — the boundary tiles come first, their
                                  epilogue stores into the neighbours, the last of them raises the flags while the interior
                                  tiles still run.  Which is fastest depends on the flight time: bench.py times all three. */
    MGCFD_OPT_STAGE_WG4 = 8    /* 1 (default): the bit-identical fused stages (MGCFD_OPT_EXACT = 1, roles without a message or an
                                  absorbed stage, levels without long rows) of a level whose every tile halo fits 254 LDS slots and
                                  whose tiles outnumber three per CU run the instantiation with 80-byte node records, four
                                  workgroups per CU instead of three; same bits.  0: always the 96-byte-record instantiation (A/B) */
};

/* Same 40-byte layout as the reference's edge_neighbour (src/Base/definitions.h:83). */
typedef struct { int64_t a, b; double x, y, z; } mgcfd_edge;

/* One multigrid level, as read_grid()/read_mg_connectivity() produce it
 * (src/Base/io.cpp:14-199, src/Base/io_enhanced.cpp:629-650).  All pointers are
 * caller-owned host memory, copied by mgcfd_create(). */
typedef struct {
    int64_t nel;
    int64_t n_edges;                       /* allocated length of edges[] */
    int64_t n_internal, n_boundary, n_wall;
    int64_t internal_start, boundary_start, wall_start;
    const double *volumes;                 /* [nel] */
    const double *coords;                  /* [nel*3] x y z; may be NULL for a single-level fvcorr run */
    const mgcfd_edge *edges;               /* [n_edges]: internal | boundary (a=-1) | wall (a=-2) */
    const int64_t *mg_map;                 /* [mgc] fine -> coarse map to the next level; NULL on the last */
    int64_t mgc;
} mgcfd_level_desc;

typedef struct mgcfd_mesh mgcfd_mesh;      /* host-side multigrid input (files parsed)   */
typedef struct mgcfd_solver mgcfd_solver;  /* device-resident solver                     */

const char *mgcfd_last_error(void);
int mgcfd_abi_version(void);
/* Optional: start bringing up the HIP runtime and `device`'s context on a thread of the library's own and return at once, so
 * that it happens WHILE the caller reads its input files (0.1 s of a drop-in run's start-up); mgcfd_create* waits for it.
 * No reference counterpart (a CPU code has no device to wake).  Errors surface in mgcfd_create*, not here. */
int mgcfd_device_warm_up(int device);
/* What the library holds on the devices in this process right now: out[0] device allocations, out[1] their bytes, out[2]
 * handles (streams, events, graph executables, opened HIP IPC mappings) — of every solver, whatever its device.  Counted by
 * the library itself, so the figures do not move with what else runs on a card; after every solver and group has been
 * destroyed they are back where they were before the first was created.  Touches no device. */
int mgcfd_live_device_resources(int64_t out[3]);

/* ---------------------------------------------------------------------------------
 * File boundary (host only, no GPU needed)
 * --------------------------------------------------------------------------------- */
/* read_input_dat + read_grid + read_mg_connectivity (+ duplicate_mesh when duplicate > 1):
 * src/Base/io_enhanced.cpp:407-579, src/Base/io.cpp:14-199, io_enhanced.cpp:629-650, :89-201.
 * `directory` may be NULL/"" (paths then relative to the cwd, as with no -d). */
int mgcfd_mesh_load(const char *input_dat, const char *directory, int duplicate, mgcfd_mesh **out);
/* The same with flags: MGCFD_MESH_LEGACY_ORDERING sorts every edge class by (a, b, x, y, z) as the
 * reference's -DLEGACY_ORDERING build does (src/Base/io.cpp:183-193, src/Base/common.h:145-157). */
#define MGCFD_MESH_LEGACY_ORDERING 1
int mgcfd_mesh_load_ex(const char *input_dat, const char *directory, int duplicate, int flags, mgcfd_mesh **out);
void mgcfd_mesh_free(mgcfd_mesh *m);
int mgcfd_mesh_num_levels(const mgcfd_mesh *m);
int mgcfd_mesh_variant(const mgcfd_mesh *m);
int mgcfd_mesh_size(const mgcfd_mesh *m);                 /* input.dat "size" x duplicate (euler3d_cpu_double.cpp:259-260) */
/* Borrowed view of level l (valid until mgcfd_mesh_free). */
int mgcfd_mesh_level(const mgcfd_mesh *m, int level, mgcfd_level_desc *out);

/* dump(): "%.17e" x5 per node (src/Base/io.cpp:201-233); generic writer for 1- or 5-column arrays. */
int mgcfd_write_array(const char *path, const double *data, int64_t nel, int ncols);
/* identify_differences(): returns MGCFD_OK or MGCFD_ERR_VALIDATION; *first_bad = flat index or -1. */
int mgcfd_identify_differences(const double *test_values, const double *master_values, int64_t nel,
                               int mesh_variant, int64_t *first_bad);

/* ---------------------------------------------------------------------------------
 * Solver life cycle
 * --------------------------------------------------------------------------------- */
/* Uploads the levels to GPU `device`, applies adjust_ewt/dampen_ewt for the mesh variant
 * (euler3d_cpu_double.cpp:337-352, validation.cpp:28-75), builds the renumbered gather
 * structures, and initialises every level to the far-field state
 * (initialize_far_field_conditions + initialize_variables, cfd_loops.h:44-119;
 * fluxes/residuals zeroed, euler3d_cpu_double.cpp:321-331). */
int mgcfd_create(const mgcfd_level_desc *levels, int nlevels, int mesh_variant, int device,
                 mgcfd_solver **out);
int mgcfd_create_from_mesh(const mgcfd_mesh *m, int device, mgcfd_solver **out);
/* A level PARTITIONED over ranks (multi-GPU "within a level"): every rank passes its own part —
 * its owned nodes numbered first, then ghost copies of the other ranks' nodes its edges touch, and
 * every edge with at least one owned end point (relative order as in the whole mesh, so sums keep
 * the reference's order).  n_owned[l] = number of owned nodes of level l (nodes with id >= n_owned
 * are ghosts: gathered from, never updated; excluded from the RMS). */
int mgcfd_create_partitioned(const mgcfd_level_desc *levels, int nlevels, int mesh_variant, int device,
                             const int64_t *n_owned, mgcfd_solver **out);
/* The same for a partitioned HIERARCHY (every level split over the ranks, mg_map in local numbering: the parent of
 * every local fine node must be a local coarse node).  order_keys[l] (may be NULL) gives, per node of level l, the key by
 * which a coarse node's children are summed in mgcfd_restrict — global ids, so the mean keeps the whole mesh's order.
 * The caller exchanges ghost values where the hierarchy needs them: `variables` after every time_step, after
 * mgcfd_restrict (coarse level) and after mgcfd_prolong (fine level); coarse `residuals` before mgcfd_prolong
 * (mgcfd/partition.py: partition_hierarchy, mgcfd/distributed.py: PartitionedCycle). */
int mgcfd_create_partitioned_mg(const mgcfd_level_desc *levels, int nlevels, int mesh_variant, int device,
                                const int64_t *n_owned, const int64_t *const *order_keys, mgcfd_solver **out);
/* Host only (no device): builds the gather plans the three calls above would build and checks every index the kernels
 * form from them — LDS slots, halo / overflow positions, half-row owners, list entries, children, staged coarse nodes —
 * against the size of what it indexes.  MGCFD_OK, or MGCFD_ERR_ARG with the violations in `report` (may be NULL).
 * n_owned / order_keys as in mgcfd_create_partitioned_mg (NULL: every node owned).  The reference has no counterpart:
 * its loops index the caller's arrays directly (src/Kernels/flux_loops.cpp:133-136). */
int mgcfd_plan_audit(const mgcfd_level_desc *levels, int nlevels, int mesh_variant, const int64_t *n_owned,
                     const int64_t *const *order_keys, char *report, int64_t report_cap);
void mgcfd_destroy(mgcfd_solver *s);
int mgcfd_set_option(mgcfd_solver *s, int option, int value);
/* *yes = 1 when the half-row plan of level `level` is uniform: no long rows, no halo node left outside LDS, at most 5 edges
 * evaluated per lane.  A property of the plan: it tells which instantiation of the order-free kernel the level reaches (the
 * one that requests every half row up front; other levels walk the rows beyond five in a loop or stage wide halos). */
int mgcfd_level_has_half_rows(const mgcfd_solver *s, int level, int *yes);
/* *yes = 1 when level `level` can run the order-free flux kernel (MGCFD_OPT_FLUX_VARIANT bit 6 with MGCFD_OPT_EXACT = 0): no halo
 * node left outside LDS; any number of edges per node (what a lane's five requested rows do not hold is walked in a loop). */
int mgcfd_level_has_order_free(const mgcfd_solver *s, int level, int *yes);
/* *yes = 1 when the bit-identical fused stages of level `level` run the four-workgroups-per-CU instantiation (MGCFD_OPT_STAGE_WG4
 * set, MGCFD_OPT_EXACT = 1, no long rows, every tile halo within 254 LDS slots, more tiles than three per CU; the split sweep's
 * absorbed first stage and a stage that sends its own message keep the other one). */
int mgcfd_level_stage_wg4(const mgcfd_solver *s, int level, int *yes);
/* What the tiling of level `level` looks like (the figures MGCFD_VERBOSE=1 prints at creation):
 * out[0] tiles of 256 nodes, out[1] halo nodes of all tiles together, out[2] the largest halo, out[3] halo nodes a
 * tile can stage in LDS, out[4] incidence-row entries that refer to a halo node beyond that (each a gather from
 * HBM), out[5] incidence-row entries of internal edges (two per edge), out[6] padding entries among them,
 * out[7] 1 when the nodes were ordered by coordinate boxes instead of greedy clusters, out[8] internal-edge entries
 * handed to the workgroups' lists instead of the per-node loops (long rows: entries beyond a tile's row limit, and
 * every entry from a node's first out[4]-kind entry on — so with out[8] > 0 none of out[4] is gathered inside a loop),
 * out[9] rows the per-node loops walk, summed over the 64-node slices. */
int mgcfd_level_tiling(const mgcfd_solver *s, int level, int64_t out[10]);
int mgcfd_get_option(const mgcfd_solver *s, int option, int *value);
/* Run all subsequent work of this solver on an existing HIP stream (hipStream_t as void*), e.g.
 * the cuda_stream of a torch.cuda.Stream() made current with torch.cuda.set_stream(): collectives
 * and copies torch enqueues on that stream are then ordered with the solver's kernels.  NULL restores
 * the solver's own stream, which is created non-blocking: it does NOT synchronise with the legacy
 * default stream, whose handle is also NULL — the default stream cannot be shared this way. */
int mgcfd_set_stream(mgcfd_solver *s, void *hip_stream);
int mgcfd_synchronize(mgcfd_solver *s);
int mgcfd_num_levels(const mgcfd_solver *s);
int64_t mgcfd_level_nel(const mgcfd_solver *s, int level);
int64_t mgcfd_level_num_internal_edges(const mgcfd_solver *s, int level);
/* ff_variable[5] + the four ff_flux_contribution_* vectors (17 doubles), globals.h:11-15. */
int mgcfd_get_far_field(const mgcfd_solver *s, double *out17);
/* The free stream at run time.  The reference fixes it when it is compiled (ff_mach = 1.2, deg_angle_of_attack = 0,
 * src/Base/const.h:14-15); here the caller chooses it.
 * mgcfd_free_stream_constants — host only: the 17 doubles of mgcfd_get_far_field for a Mach number and an angle of attack in
 * degrees, the reference's expressions (src/Kernels/cfd_loops.h:85-119 and 57-83) in their order, never contracted to FMA;
 * gamma = 1.4, p = 1 and rho = 1.4 stay fixed, the velocity is |V| (cos a, sin a, 0).  (1.2, 0.0) gives the reference's values
 * bit for bit.  MGCFD_ERR_ARG for a non-finite value, mach <= 0 or |alpha_deg| >= 90.
 * mgcfd_set_free_stream — synchronises, then replaces the far field every flux, stage, init and loads kernel is given (and the
 * far-field pressure of the surface loads).  reinitialise = 1: `variables` of every level becomes the new far field, as
 * mgcfd_create leaves it, and a pending invalid state (mgcfd_pending_invalid_state) is forgotten; 0: the state stays (a warm
 * start: the next cycles continue from the flow of the previous free stream).  Every captured graph of the solver
 * (MGCFD_OPT_GRAPH: sweeps, cycles, an RCCL rank's sweeps — mgcfd_rank_graph_status out[0] goes back to 0) is dropped, since
 * a captured launch holds the far field as an argument; the next run captures again.  Works on plain, partitioned and
 * rank-attached solvers.  A solver it is never called on behaves as before.  MGCFD_ERR_ARG, and nothing changed, while a
 * kernel-granular sweep is under way on any level (after mgcfd_sweep_flux0, or between mgcfd_sweep_stage 0 and the last
 * stage): its buffers hold half a sweep of the old free stream.
 * Ranks: the ranks of one flow must hold the same far field.  An in-process group checks it (further down); between RCCL
 * ranks in different processes nothing can, so agreement there is the CALLER's duty: call it with the same arguments on
 * every rank (mgcfd/distributed.py: set_free_stream_all broadcasts rank 0's). */
int mgcfd_free_stream_constants(double mach, double alpha_deg, double out17[17]);
int mgcfd_set_free_stream(mgcfd_solver *s, double mach, double alpha_deg, int reinitialise);
int mgcfd_get_free_stream(const mgcfd_solver *s, double *mach, double *alpha_deg);
/* The time step at run time: which step-factor formula every smoothing sweep starts with, and its CFL number.  The reference
 * ties both to the mesh NAME and the literal 0.5 (src/euler3d_cpu_double.cpp:388-395, src/Kernels/cfd_loops.cpp:13-157).
 * With derive()'s speed and c of node i (cfd_loops.h:121-148) and dt_i = cbrt(vol_i) / (speed_i + c_i) — cbrt from the host's
 * libm, as the reference calls it — the step factors of a sweep are, associated as written and never contracted to FMA:
 *   MGCFD_DT_REFERENCE     what the mesh name selects: GLOBAL, or LOCAL_LEGACY for mesh_name = fvcorr (the default)
 *   MGCFD_DT_GLOBAL        sf_i = min_j(cfl * dt_j) / vol_i          compute_step_factor, cfd_loops.cpp:76-157
 *   MGCFD_DT_LOCAL         sf_i = (cfl * dt_i) / vol_i               every node marches at its own step; no reference counterpart
 *   MGCFD_DT_LOCAL_LEGACY  sf_i = cfl / (sqrt(vol_i) * (speed_i + c_i))   compute_step_factor_legacy, cfd_loops.cpp:13-73
 * (MGCFD_DT_REFERENCE, 0.5) is what a solver starts with and launches what it launched before this call existed.  Under a
 * local mode nothing is reduced: a level split over ranks needs no all-reduce of the time step (no RCCL call, no flag round,
 * no event fan-in per sweep) and mgcfd_step_factor_local returns MGCFD_ERR_ARG.  The ghosts of a partitioned level get the
 * factor 0 under MGCFD_DT_LOCAL (their owners compute theirs).
 * mgcfd_set_time_step — synchronises, drops every captured graph of the solver (a captured launch holds the CFL number) and
 * discards step-factor work done ahead under the old policy; the state stays.  MGCFD_ERR_ARG, and nothing changed, for an
 * unknown mode, a non-finite cfl or cfl <= 0, and while a kernel-granular sweep is under way (as mgcfd_set_free_stream).
 * Ranks: the ranks of one flow must hold the same mode and CFL number.  An in-process group checks it
 * (mgcfd_group_set_time_step, further down); between RCCL ranks in different processes agreement is the CALLER's duty
 * (mgcfd/distributed.py: set_time_step_all broadcasts rank 0's). */
enum { MGCFD_DT_REFERENCE = 0, MGCFD_DT_GLOBAL = 1, MGCFD_DT_LOCAL = 2, MGCFD_DT_LOCAL_LEGACY = 3 };
int mgcfd_set_time_step(mgcfd_solver *s, int mode, double cfl);
int mgcfd_get_time_step(const mgcfd_solver *s, int *mode, double *cfl);
/* Implicit residual smoothing (Jameson): every time_step's update D_i = step_factor_i * fluxes_i is replaced by `iterations`
 * Jacobi iterations on (1 + eps * n_i) Db_i - eps * sum_j Db_j = D_i over the level's internal edges, which raises the
 * usable CFL number of the three-stage scheme by a factor of two or more.  No reference counterpart.  With iterations = M >= 1,
 * stage j of every sweep of every level computes its fluxes as before (internal, solid wall, far field) and then, in place
 * of time_step(j), with every operation one IEEE-754 double operation, never contracted to FMA under MGCFD_OPT_EXACT = 1:
 *   D[i][v]   = sf[i] * F[i][v]                       sf: the sweep's step factors under the mgcfd_set_time_step policy
 *   den[i]    = 1.0 + eps * (double)n_i               n_i: internal edges with i as an end point (boundary faces do not count)
 *   Db0 = D;  for m = 1 .. M:   S[i][v] = the sum, started at +0.0, of Db(m-1)[other end][v] over the internal edges at i
 *                               in the level's original edge order, one addition per edge;
 *                               Db(m)[i][v] = (D[i][v] + eps * S[i][v]) / den[i]
 *   variables[i][v] = old_variables[i][v] + Db(M)[i][v] / (double)(MGCFD_RK + 1 - j)
 * fluxes are zero afterwards and check_for_invalid_variables runs inside the last launch, as time_step carries it; residual,
 * RMS and everything behind the sweep are unchanged.  A stage is one standalone flux launch + M smoothing launches (the
 * fused flux + time_step stages and captured graphs are not used while it is on; MGCFD_OPT_GRAPH is accepted and runs the
 * same launches directly); mgcfd_time_step(s, level, j) performs the steps above; LoopNumIters counts are unchanged and the
 * launches are timed as MGCFD_LOOP_TIME_STEP.  iterations = 0 switches it off (eps is then ignored and reported as 0): the
 * solver launches exactly what it launched before this call existed.  The first call with iterations > 0 allocates two
 * [5][stride] arrays per level; a solver it is never called on holds what it held before.
 * mgcfd_set_residual_smoothing synchronises and drops every captured graph; the state stays.  MGCFD_ERR_ARG, and nothing
 * changed: iterations < 0 or > MGCFD_MAX_SMOOTHING_ITERATIONS; with iterations > 0 a non-finite eps or eps <= 0; while a
 * kernel-granular sweep is under way (as mgcfd_set_free_stream); with iterations > 0 on a solver made by
 * mgcfd_create_partitioned* or attached to a group or as a rank — a level split over ranks would need a ghost exchange per
 * Jacobi iteration, which is deliberately out of scope.  While it is on, mgcfd_sweep_begin*, mgcfd_sweep_flux0,
 * mgcfd_sweep_stage and mgcfd_sweep_end* return MGCFD_ERR_ARG, and mgcfd_group_create and mgcfd_rank_attach_* refuse the solver. */
#define MGCFD_MAX_SMOOTHING_ITERATIONS 8
int mgcfd_set_residual_smoothing(mgcfd_solver *s, double eps, int iterations);
int mgcfd_get_residual_smoothing(const mgcfd_solver *s, double *eps, int *iterations);
/* Dual time stepping (Jameson 1991): time-accurate flows.  Physical time is discretised by the second-order backward
 * difference formula (BDF2, BDF1 on the first step) and every physical step is solved as a steady problem in pseudo-time
 * by the machinery above: V-cycles, local or global pseudo steps (mgcfd_set_time_step), residual smoothing.  No reference
 * counterpart.  With dual time on and physical step dt every level l holds two more [5][stride] arrays: Wn, the state at the
 * last physical time level, and Wn1, the one before it.  Stage j of every sweep of every level computes its fluxes F as
 * before (internal, solid wall, far field) and then forms for every node i and variable v, with W the stage's input state
 * (the state the fluxes were computed from), every operation one IEEE-754 double operation, never contracted to FMA under
 * MGCFD_OPT_EXACT = 1:
 *   a = W[i][v] - Wn[i][v]
 *   b = Wn[i][v] - Wn1[i][v]
 *   second order (BDF2):   src = vol[i] * ((3.0 * a - b) / (2.0 * dt))
 *   first order  (BDF1):   src = vol[i] * (a / dt)
 *   F'[i][v] = F[i][v] - src
 * (the differences first: a uniform state gives src = +0.0 exactly).  The update proceeds with F' in place of F and nothing
 * else changes: time_step(j) without residual smoothing, D = sf * F' into the Jacobi iterations with it.  The source is
 * explicit in pseudo-time, so after a sweep's step factors are final under the mgcfd_set_time_step policy and before
 * stage 0:   sf[i] = min(sf[i], (clamp * dt) / vol[i])   (clamp: a run-time number, finite and above zero; the callers' default
 * is 2.0/3.0, MGCFD_DUAL_TIME_CLAMP; vol: the volumes the step factor uses; a node whose factor is NaN keeps it).
 * The RMS of a cycle while dual time is on (mgcfd_run_cycles[_loads], mgcfd_advance) is sqrt(S / nel) with S, the sum of the
 * squares of level 0's residuals, added up in an order fixed by the ORIGINAL node numbering, every operation one IEEE-754
 * double operation, never contracted: node o gives q[o] = ((((+0.0 + r0*r0) + r1*r1) + r2*r2) + r3*r3) + r4*r4; nodes
 * 256 g .. 256 g + 255 (missing ones count +0.0) form group g of four blocks of 64; a block of 64 values is halved five times
 * (v[i] + v[i + 32] for i < 32, then + 16, 8, 4, 2) and its last two values added; the group's sum is ((+0.0 + block 0) +
 * block 1) + block 2) + block 3; the group sums p[g] are added up the same way: t[i] = p[i] + p[i + 256] + ... one after
 * another from +0.0 for i < 256, then t as one group.  (With dual time off the sum keeps the order of the library's own
 * numbering, as before.)
 * Time levels: mgcfd_dual_time_begin_step does Wn1 <- Wn and Wn <- variables[l] on EVERY level l — a coarse level takes its
 * own current `variables` (what mg_restrict of the last cycle left, plus the sweeps and prolongations behind it): no new
 * transfer operator is introduced.  The first step after switching on, and the first after mgcfd_dual_time_reset, sets
 * Wn1 = Wn = variables and runs BDF1; from the second step on BDF2 runs; mgcfd_dual_time_set_order(s, 1) keeps BDF1
 * throughout.  Switching on also sets Wn1 = Wn = variables, so sweeps before the first begin_step are defined (BDF1 against
 * the state at switch-on).  mgcfd_set_array on MGCFD_ARR_TIME_N / _TIME_N1 (a restart) marks one / both levels as held:
 * restore variables, Wn and Wn1 and the next begin_step shifts them and runs BDF2.
 * mgcfd_set_dual_time(s, dt, clamp): dt > 0 and finite switches it on (the arrays are allocated at the first such call; a
 * later one changes dt and clamp and keeps the levels), dt = 0 switches it off: the arrays are released and the solver
 * launches what it launched, and computes the bits it computed, before the call existed.  It synchronises and drops every
 * captured graph; the state stays.  MGCFD_ERR_ARG, and nothing changed: a negative or non-finite dt; with dt > 0 a non-finite
 * clamp or clamp <= 0; while a kernel-granular sweep is under way (as mgcfd_set_time_step); with dt > 0 on a solver made by
 * mgcfd_create_partitioned* or attached to a group or as a rank.  While it is on: mgcfd_smooth, mgcfd_run_cycles[_loads] and
 * mgcfd_compute_step_factor / mgcfd_step_factor_apply / mgcfd_time_step(s, l, j) honour the clamp and the source
 * (mgcfd_time_step with the state mgcfd_compute_fluxes last read as W); a stage is one standalone flux launch + one
 * time_step launch that forms F' in registers (with residual smoothing: + one node-wise source launch + the M smoothing
 * launches); the fused flux + time_step stages and captured graphs are not used (MGCFD_OPT_GRAPH is accepted and runs the
 * launches directly); mgcfd_sweep_begin*, mgcfd_sweep_flux0, mgcfd_sweep_stage and mgcfd_sweep_end* return MGCFD_ERR_ARG, and
 * mgcfd_group_create and mgcfd_rank_attach_* refuse the solver.  Out of scope: levels split over ranks, captured graphs
 * with dual time on, a fused flux + dual-time stage.
 * mgcfd_get_dual_time: any pointer may be NULL; dt = 0 when off; *order as set (2 by default); *levels = time levels held
 * (0, 1 or 2); *invalid_step = the 0-based physical step of the last mgcfd_advance in which an invalid state was found, or -1.
 * mgcfd_dual_time_set_order: 1 or 2.  mgcfd_dual_time_reset: the next begin_step starts again with BDF1.  Both, and
 * mgcfd_dual_time_begin_step, return MGCFD_ERR_ARG while dual time is off.
 * mgcfd_advance: steps x (mgcfd_dual_time_begin_step + cycles_per_step V-cycles).  rms_out (may be NULL)
 * [step * cycles_per_step + c] receives the level-0 RMS as mgcfd_run_cycles gives it, loads_out (may be NULL) [step * 6 ..]
 * the level-0 surface loads (mgcfd_surface_loads about ref_point) of the state each physical step ends with.  Errors and
 * mgcfd_invalid_state_location are those of mgcfd_run_cycles (the cycle counts within the physical step, which
 * mgcfd_get_dual_time reports); entries from the failing cycle on are NaN and later steps do not run.  At most
 * MGCFD_MAX_ADVANCE_CYCLES cycles per call in total (steps * cycles_per_step): MGCFD_ERR_ARG beyond that, for steps < 0 or
 * cycles_per_step < 1, and while dual time is off. */
#define MGCFD_MAX_ADVANCE_CYCLES 4096
#define MGCFD_DUAL_TIME_CLAMP (2.0 / 3.0)
int mgcfd_set_dual_time(mgcfd_solver *s, double dt, double clamp);
int mgcfd_get_dual_time(const mgcfd_solver *s, double *dt, double *clamp, int *order, int *levels, int *invalid_step);
int mgcfd_dual_time_set_order(mgcfd_solver *s, int order);
int mgcfd_dual_time_reset(mgcfd_solver *s);
int mgcfd_dual_time_begin_step(mgcfd_solver *s);
int mgcfd_advance(mgcfd_solver *s, int steps, int cycles_per_step, double *rms_out, double *loads_out, const double ref_point[3]);
/* JST dissipation (Jameson, Schmidt, Turkel 1981): the reference's scalar first-difference dissipation, 0.2 * spectral radius *
 * (W_i - W_j) on every internal edge, is kept only where a pressure sensor sees a shock; elsewhere a small fourth difference
 * takes over.  No reference counterpart.  Per solver: kappa2 >= 0, kappa4 >= 0 (finite, in units of the reference's own
 * dissipation: the textbook pair k2 = 1/2, k4 = 1/32 is MGCFD_JST_KAPPA2 = 2.5, MGCFD_JST_KAPPA4 = 0.15625) and levels >= 0: it
 * runs on levels 0 .. levels-1 (capped at the number of levels; 0 = off).  On such a level stage j of every sweep computes its
 * fluxes F from the stage's input state W as before (internal, solid wall, far field) and then, over the level's internal
 * edges only, in the level's original edge order, every operation one IEEE-754 double operation, never contracted to FMA
 * under MGCFD_OPT_EXACT = 1:
 *   pass 1, node i:   p_i = the reference's pressure (velocities by division, speed_sqd left to right,
 *                     (GAMMA-1)*(en - 0.5*rho*speed_sqd));  r_i = sqrt(speed_sqd_i) + sqrt(GAMMA * p_i / rho_i);
 *                     sums from +0.0, one addition per internal edge (i, j) at i:  L_i[v] += W_j[v] - W_i[v];
 *                     Pm_i += p_j - p_i;  Pp_i += p_j + p_i;   nu_i = fabs(Pm_i) / Pp_i  (no internal edge: 0.0)
 *   pass 2, node i:   C_i[v] from +0.0, over the same edges in the same order, k_e = -|e| * (double)0.2f * 0.5:
 *                     fac = k_e * (r_i + r_j);  nu = nu_i > nu_j ? nu_i : nu_j;
 *                     e2 = kappa2 * nu;  e2 = e2 < 1.0 ? e2 : 1.0;   e4 = kappa4 - e2;  e4 = e4 > 0.0 ? e4 : 0.0;
 *                     C_i[v] += fac * ((e2 - 1.0) * (W_i[v] - W_j[v]) - e4 * (L_i[v] - L_j[v]))
 *                     F[i][v] = F[i][v] + C_i[v]
 * With the first-difference term already inside F the edge's dissipation is fac * (e2 * (W_i - W_j) - e4 * (L_i - L_j)):
 * never more than the reference's, and the reference's where e2 = 1.  Everything behind F sees F + C: time_step, the
 * dual-time source and clamp, the residual smoothing, residual, RMS, loads.  Step factors are unchanged.
 * While it is on for level 0 the RMS of a cycle is summed in the order dual time stepping fixes on the original numbering
 * (above), so a history is reproducible bit for bit.
 * Launches: on a JST level a stage is one standalone flux launch, the sensor launch, the dissipation launch, then the update
 * the other settings select; fused flux + time_step stages, the step-factor look-ahead and captured graphs are not used on
 * that level (MGCFD_OPT_GRAPH is accepted and the launches run directly); other levels launch and compute what they did.
 * mgcfd_compute_fluxes and mgcfd_compute_flux_edge include both passes on a JST level (the boundary and far-field calls do
 * not: call them first, or use mgcfd_compute_fluxes, for F + C as defined).  MGCFD_OPT_EXACT = 0 may contract and may take the
 * order-free kernel for F; the two passes keep edge order.  Timed as MGCFD_LOOP_FLUX; LoopNumIters counts are unchanged.
 * mgcfd_set_jst synchronises and drops every captured graph; the state stays.  The first enabling call allocates seven [stride]
 * arrays (L [5], nu, r) per JST level; a solver it is never called on holds what it held.  MGCFD_ERR_ARG, and nothing
 * changed: a negative or non-finite coefficient; levels < 0; levels > 0 with both coefficients zero; while a kernel-granular
 * sweep is under way; levels > 0 on a solver made by mgcfd_create_partitioned* or attached to a group or as a rank (a split
 * level would need L, nu and r exchanged per stage: out of scope).  While it is on, mgcfd_sweep_begin*, mgcfd_sweep_flux0,
 * mgcfd_sweep_stage and mgcfd_sweep_end* return MGCFD_ERR_ARG, and mgcfd_group_create and mgcfd_rank_attach_* refuse the solver.
 * mgcfd_get_jst: any pointer may be NULL; *levels is the capped number, 0 when off (the coefficients are then reported as 0). */
#define MGCFD_JST_KAPPA2 2.5
#define MGCFD_JST_KAPPA4 0.15625
int mgcfd_set_jst(mgcfd_solver *s, double kappa2, double kappa4, int levels);
int mgcfd_get_jst(const mgcfd_solver *s, double *kappa2, double *kappa4, int *levels);
/* FAS multigrid (Brandt's full approximation storage, as Jameson's multigrid uses it): the coarse equations carry a forcing
 * term and what comes back up is a correction, so the cycle's fixed point is the fine grid's steady state.  The reference's
 * cycle (mgcfd_restrict, unforced coarse sweeps, mgcfd_prolong of one sweep's change of state) has another fixed point; it
 * stays the default.  Per solver, off by default: with it off the solver launches what it launches and computes the bits it
 * computes without this call.  Every operation below is one IEEE-754 double operation, never contracted to FMA under
 * MGCFD_OPT_EXACT = 1; n is the number of levels.
 *   Total residual R_l(W) of level l, formed from zero fluxes in this order, each part only where its feature is on for l:
 *     1. F, the internal, solid-wall and far-field fluxes, as mgcfd_compute_fluxes;
 *     2. + C, the two JST passes, where mgcfd_set_jst covers l;
 *     3. - src, the dual-time source with W as the state, while dual time is on.
 *   Forced stage: on a level l >= 1 every stage of every sweep takes F' = R_l(W) + P_l wherever it took R_l(W) — the forcing is
 *     the last addition; D = sf * F' goes into the Jacobi iterations with residual smoothing on.  Step factors, the dual-time
 *     clamp, the invalid-state check and `residuals` are unchanged.  Level 0 has no forcing: its sweeps are the sweeps of a
 *     solver with FAS off, fused stages included.
 *   Down leg, l = 0 .. n-2, after sweep(l):
 *     1. T_l = R_l(variables[l]); for l >= 1 then T_l[i][v] = R_l[i][v] + P_l[i][v].
 *     2. mg_restrict of the state exactly as mgcfd_restrict(l); W0_{l+1} = a copy of all of variables[l+1], nodes without
 *        children included.
 *     3. Q[c][v], from +0.0, receives one addition per child, T_l[child][v], over the children of c in ascending original fine
 *        id (mg_restrict's order): summed, not averaged.
 *     4. P_{l+1}[c][v] = Q[c][v] - R_{l+1}(W0_{l+1})[c][v] for a coarse node with children, +0.0 for one without.  fluxes[l+1]
 *        is logically zero afterwards.
 *     Then sweep(l+1), forced.
 *   Up leg, l = n-2 .. 0:
 *     1. D[c][v] = W0_{l+1}[c][v] - variables[l+1][c][v].
 *     2. variables[l][i][v] = variables[l][i][v] + (0.0 - wavg_i(D)[v]), wavg_i what mgcfd_prolong applies to the coarse
 *        residuals — the same entries, order and weights, the division by the weight sum, the coincident-node rule and the
 *        reference's b-end quirk (mg_loops.cpp:730-851): prolong_residuals_interpolate_proper with residuals1 = D and
 *        residuals2 = +0.0.
 *     3. The `residuals` arrays of both levels are not touched.
 *     4. For l > 0, sweep(l), forced with the same P_l.
 *   The level-0 RMS of a cycle keeps its definition and, while FAS is on, is summed in the fixed original-numbering order of
 *   dual time stepping and the JST dissipation (above).
 * mgcfd_set_fas(s, on): switching on allocates P and W0, [5][stride] each, on the levels >= 1, both zeroed; every enabling call
 * and mgcfd_set_free_stream(.., reinitialise = 1) zero P again; switching off releases them.  It synchronises and drops every
 * captured graph; the state stays.  MGCFD_ERR_ARG, and nothing changed: a one-level solver; while a kernel-granular sweep is
 * under way; a solver made by mgcfd_create_partitioned* or attached to a group or as a rank (a split level would need T, P and D
 * exchanged: out of scope).  While it is on: mgcfd_group_create and mgcfd_rank_attach_* refuse the solver; mgcfd_sweep_begin*,
 * mgcfd_sweep_flux0, mgcfd_sweep_stage and mgcfd_sweep_end* return MGCFD_ERR_ARG; MGCFD_OPT_GRAPH is accepted and the launches run
 * directly; mgcfd_time_step(s, l, j) and mgcfd_smooth(s, l, k) honour P_l on l >= 1 (a stage there is one standalone flux
 * launch + the forced update); mgcfd_restrict and mgcfd_prolong stay the reference's; mgcfd_run_cycles[_loads] and mgcfd_advance
 * run the cycle above.  mgcfd_fas_restrict(s, fine) does down-leg steps 1-4 (both levels' fluxes must be zero, as after
 * time_step), mgcfd_fas_prolong(s, fine) up-leg steps 1-2; MGCFD_ERR_ARG while FAS is off.  LoopNumIters: the extra residual
 * evaluations count, and are timed, as MGCFD_LOOP_FLUX; restrict and prolong count as before.
 * Out of scope: levels split over ranks or GPUs; captured graphs with FAS on; a fused flux + forced-update stage; a
 * volume-weighted state restriction.  (W- and F-cycles and sweep counts per level: mgcfd_set_cycle, below.) */
int mgcfd_set_fas(mgcfd_solver *s, int on);
int mgcfd_get_fas(const mgcfd_solver *s, int *on);
/* The multigrid cycle: its shape (V, W or F), the sweeps per level before the down leg (pre) and after the up leg (post), cycles
 * that start from a coarser level, the interpolation of a coarse state onto the next finer level, and a full-multigrid (FMG)
 * start built from them.  Per solver; everything is off by default, and a solver on which none of these calls is made launches
 * what it launched and computes the bits it computed.  n is the number of levels.  One cycle is visit(0, shape):
 *   visit(l, kind):
 *     pre[l] times: sweep(l)          l == 0: the cycle's RMS is taken after the LAST of these, defined as without this call
 *     if l == n-1: return
 *     down(l)                         mgcfd_restrict(l); with FAS on, the down leg from l (steps 1-4 above)
 *     visit(l+1, kind)
 *     if l+1 < n-1:                   the coarsest level is visited once per down leg
 *       kind == W: visit(l+1, W);     kind == F: visit(l+1, V)
 *     up(l)                           mgcfd_prolong(l); with FAS on, the up leg onto l (steps 1-2 above)
 *     post[l] times: sweep(l)
 *   A second visit of l+1 works on the same coarse problem: P_{l+1} and W0_{l+1} of the one down(l) stay, its own down(l+1)
 *   forms P_{l+2} and W0_{l+2} anew.  sweep, down, up, forced stages and step factors are the operations defined above on the
 *   arrays as they stand (dual-time source and clamp, JST, viscous terms and the wall launch included); with the reference's
 *   transfers up(l) prolongs whatever residuals[l+1] the last sweep there left.  With three levels F and W are the same cycle.
 * Defaults: shape V, pre[l] = 1, post[0] = 0, post[l] = 1 for 0 < l < n-1; post[n-1] is ignored (mgcfd_get_cycle reports 1 for
 * it, 0 on a one-level solver).  That is the reference's cycle launch for launch, and while the configuration equals it fused
 * stages, the step-factor look-ahead, captured graphs and the RMS folded into the first restriction stay as they are.  With any
 * other configuration MGCFD_OPT_GRAPH is accepted and the launches run directly; the look-ahead is used exactly where the launch
 * that wrote a level's current state left its minima behind.  mgcfd_run_cycles, mgcfd_run_cycles_loads[_viscous] and
 * mgcfd_advance[_loads_viscous] run the configured cycle; loads are those of the state after the post[0] sweeps; one RMS per cycle.
 * mgcfd_set_cycle(s, shape, pre, post): pre and post hold n entries each, NULL = the defaults.  It synchronises, drops every
 * captured graph and allocates nothing.  MGCFD_ERR_ARG, and nothing changed: an unknown shape; pre[l] outside
 * 1..MGCFD_MAX_CYCLE_SWEEPS; post[l] outside 0..MGCFD_MAX_CYCLE_SWEEPS; while a kernel-granular sweep is under way; a non-default
 * configuration on a solver made by mgcfd_create_partitioned* or attached to a group or as a rank.  mgcfd_group_create and
 * mgcfd_rank_attach_* refuse a solver with a non-default cycle.  mgcfd_get_cycle: any pointer may be NULL.
 * mgcfd_run_cycles_from(s, top, cycles, rms_out) runs visit(top, shape) `cycles` times with level `top` in level 0's part; the
 * levels below `top` are untouched.  With FAS on `top` is unforced: its stages take R_top(W) without P_top, down(top) step 1 uses
 * T = R_top, and the stored P_top is neither read nor written.  rms_out[c] = sqrt(S / nel_top), S summed in dual time stepping's
 * fixed order (above) over level top's ORIGINAL numbering whatever the other settings are; that numbering is uploaded at the
 * first such call and goes with the solver.  top = 0 is mgcfd_run_cycles, with its own RMS rule.  MGCFD_ERR_ARG for top > 0:
 * while dual time is on, beyond MGCFD_MAX_ADVANCE_CYCLES cycles, on a partitioned or attached solver.  An invalid state is
 * reported as by mgcfd_run_cycles.
 * mgcfd_prolong_state(s, fine): for every node i of level `fine` and component v
 *     variables[fine][i][v] = 0.0 - (0.0 - wavg_i(variables[fine+1])[v])
 * with wavg_i exactly what mgcfd_prolong and FAS's up leg form (entries, order, weights, the division by the weight sum, the
 * coincident-node rule and the b-end quirk); the two subtractions only turn a -0.0 into +0.0.  The fine state is written, never
 * read; `residuals` of both levels are untouched; on a viscous level with wall = 1 the wall launch follows.  Timed and counted as
 * MGCFD_LOOP_PROLONG.  MGCFD_ERR_ARG on a partitioned or attached solver.
 * mgcfd_full_multigrid(s, cycles, rms_out): mgcfd_restrict(l) for l = 0 .. n-2 (the state only, no sweeps), then for
 * top = n-1 .. 1: mgcfd_run_cycles_from(top, cycles[top]) followed by mgcfd_prolong_state(top - 1).  cycles holds n entries,
 * cycles[0] is ignored; rms_out (may be NULL) receives the concatenated histories.  MGCFD_ERR_ARG, and nothing changed: while
 * dual time is on, on a partitioned or attached solver, a cycles[l] outside 0..MGCFD_MAX_ADVANCE_CYCLES, while a kernel-granular
 * sweep is under way.  An invalid state stops it there and is returned.  The level-0 cycles are the caller's next call.
 * Out of scope: split levels and groups; captured graphs of shaped cycles; FMG under dual time; a volume-weighted or
 * higher-order state interpolation; per-level CFL numbers. */
enum { MGCFD_CYCLE_V = 0, MGCFD_CYCLE_W = 1, MGCFD_CYCLE_F = 2 };
#define MGCFD_MAX_CYCLE_SWEEPS 8
int mgcfd_set_cycle(mgcfd_solver *s, int shape, const int *pre, const int *post);
int mgcfd_get_cycle(const mgcfd_solver *s, int *shape, int *pre, int *post);
int mgcfd_run_cycles_from(mgcfd_solver *s, int top, int cycles, double *rms_out);
int mgcfd_prolong_state(mgcfd_solver *s, int fine_level);
int mgcfd_full_multigrid(mgcfd_solver *s, const int *cycles, double *rms_out);
/* Laminar viscous terms: the Navier-Stokes stresses, heat conduction and a no-slip wall.  No reference counterpart.  Per solver:
 * mu > 0 (dynamic viscosity in the solver's units, constant unless mgcfd_set_viscosity_model sets a law), prandtl > 0, wall (0 = slip, as without the
 * feature; 1 = no-slip, adiabatic), cfl_v > 0 (the viscous step limit, (c)) and levels >= 0: it runs on levels 0 .. levels-1
 * (capped at the number of levels; 0 = off, the other arguments are then ignored), exactly mgcfd_set_jst's levels.  Off by
 * default; with it off the solver launches what it launched and computes the bits it computed.
 * Every operation below is one IEEE-754 double operation, never contracted to FMA under MGCFD_OPT_EXACT = 1.  Both passes run over
 * the level's internal edges only, in the level's original edge order, one addition per edge at each end.  For an edge record
 * (a, b, e) the normal seen from end a is n = (e.x, e.y, e.z) and the other node is b; seen from end b it is n = (-e.x, -e.y, -e.z)
 * (the negation is exact) and the other node is a.  W is the state the stage's fluxes were computed from.
 *   (a) pass 1, node i: the node stresses S_i, twelve doubles.  u = mx / rho, v = my / rho, w = mz / rho; p the reference's
 *       pressure ((GAMMA-1)*(en - 0.5*rho*speed_sqd), speed_sqd = u*u + v*v + w*w left to right); T = p / rho.
 *       For phi in (u, v, w, T) and d in (x, y, z): A[phi][d] from +0.0, A[phi][d] += (phi_j - phi_i) * n_d per edge at i;
 *       G[phi][d] = (0.5 * A[phi][d]) / vol_i with the volumes the step factor uses (Green-Gauss in difference form: wherever a
 *       node's dual surface closes it equals the face-value form with the boundary faces included, it needs no boundary edge
 *       and is exactly zero for a uniform field).
 *       div = (G[u][x] + G[v][y]) + G[w][z];  t = (2.0/3.0) * div;
 *       txx = mu * (2.0 * G[u][x] - t), tyy and tzz likewise;  txy = mu * (G[u][y] + G[v][x]);  txz = mu * (G[u][z] + G[w][x]);
 *       tyz = mu * (G[v][z] + G[w][y]);  q_d = kappa * G[T][d], kappa = (mu * GAMMA) / ((GAMMA - 1.0) * prandtl) formed once on
 *       the host.  S_i = (u, v, w, txx, tyy, tzz, txy, txz, tyz, qx, qy, qz).  A node without internal edges has zero
 *       stresses, heat flux and viscous flux.
 *   (b) pass 2, node i: V_i[1..4] from +0.0 over the same edges in the same order with the same n; barred values are
 *       0.5 * (x_i + x_j) of the twelve components of S:
 *       fx = (txx*nx + txy*ny) + txz*nz;  fy = (txy*nx + tyy*ny) + tyz*nz;  fz = (txz*nx + tyz*ny) + tzz*nz;
 *       ex = ((u*txx + v*txy) + w*txz) + qx, ey and ez likewise with the matching rows of the tensor;
 *       fe = (ex*nx + ey*ny) + ez*nz;   V_i[1] += fx; V_i[2] += fy; V_i[3] += fz; V_i[4] += fe.
 *       Then F[i][v] = F[i][v] + V_i[v] for v = 1..4; F[i][0] is not touched.  The two ends of an edge receive exactly opposite
 *       terms: the viscous flux is conservative.  Faces of the boundary classes carry no viscous flux: a wall (no-slip
 *       adiabatic, or slip) has none by definition, the far field's is neglected.  Where the JST dissipation is on too, V is
 *       added after C; everything behind F sees F + C + V: time_step, the dual-time source, the residual smoothing, FAS's total
 *       residual R_l (step "2b. + V where mgcfd_set_viscous covers l"), residual, RMS, loads.  mgcfd_compute_fluxes and
 *       mgcfd_compute_flux_edge include both passes on a viscous level, as they include JST's.
 *   (c) the viscous step limit: at enable the host forms g_i = (cbrt(vol_i) * cbrt(vol_i)) / vol_i with libm's cbrt,
 *       kv = max(4.0/3.0, GAMMA / prandtl) and k0 = cfl_v / (kv * mu).  After a sweep's step factors are final under the
 *       mgcfd_set_time_step policy and before dual time stepping's clamp: sf[i] = min(sf[i], (k0 * rho_i) * g_i); a NaN factor
 *       stays NaN.
 *   (d) the no-slip wall (wall = 1): the wall nodes of a level are the distinct b ends of its solid-wall (class -1) edges.  A
 *       small launch sets variables[i][1..3] = +0.0 there; density and energy stay.  It runs after every launch that writes a
 *       viscous level's variables: every stage's update on every path, mgcfd_prolong / mgcfd_fas_prolong onto the level,
 *       mgcfd_restrict / mgcfd_fas_restrict into it (W0 too), once at enable, and after mgcfd_set_free_stream(.., reinitialise
 *       = 1).  Where the update wrote residuals the same launch stores residuals[i][v] = +0.0 - old_variables[i][v], v = 1..3:
 *       the residual of the clamped state.  The invalid-state check looks at the update's result, as before.
 * While it is on for level 0 the RMS of a cycle is summed in the order dual time stepping fixes on the original numbering.
 * Launches: on a viscous level a stage is one standalone flux launch, JST's two launches where on, the stress launch and the
 * viscous-flux launch, the update the other settings select and, with wall = 1, the wall launch; fused flux + time_step stages,
 * the step-factor look-ahead and captured graphs are not used on that level (MGCFD_OPT_GRAPH is accepted and the launches run
 * directly); other levels launch and compute what they did.  Timed as MGCFD_LOOP_FLUX; LoopNumIters counts are unchanged.
 * MGCFD_OPT_EXACT = 0 may contract and may take the order-free kernel for F; the two passes keep edge order.
 * mgcfd_set_viscous synchronises and drops every captured graph; the state stays but for the wall nodes' momentum.  The first
 * enabling call allocates per viscous level S [12][stride], g [stride] and the wall-node list; switching off releases them.
 * MGCFD_ERR_ARG, and nothing changed: levels < 0; with levels > 0 a mu, prandtl or cfl_v that is not finite and positive or a
 * wall other than 0 and 1; while a kernel-granular sweep is under way; levels > 0 on a solver made by mgcfd_create_partitioned*
 * or attached to a group or as a rank.  While it is on, mgcfd_sweep_begin*, mgcfd_sweep_flux0, mgcfd_sweep_stage and
 * mgcfd_sweep_end* return MGCFD_ERR_ARG, and mgcfd_group_create and mgcfd_rank_attach_* refuse the solver.
 * Friction in the surface loads: mgcfd_surface_loads_viscous and its neighbours (mgcfd_surface_loads stays the pressure loads).
 * The face gradient is the plain average of the two node gradients unless mgcfd_set_face_gradient selects the corrected one.
 * Out of scope: transported turbulence models (variable viscosity: mgcfd_set_viscosity_model); viscous flux through
 * far-field faces; levels split over ranks; graphs and fused stages with viscosity on.
 * The weights are used as the solver holds them: on meshes whose variant makes the reference rescale them at load (every
 * variant but fvcorr) the viscous terms inherit that rescaling as the inviscid ones do; physical statements are made on
 * fvcorr-variant meshes.
 * mgcfd_get_viscous: any pointer may be NULL; *levels is the capped number, 0 when off (the other values are then 0).
 * mgcfd_viscosity_from_reynolds (host only): mu = rho_inf * |V_inf| * ref_length / reynolds from a far field as
 * mgcfd_free_stream_constants / mgcfd_get_far_field give it; MGCFD_ERR_ARG unless reynolds, ref_length and the result are finite
 * and positive. */
#define MGCFD_VISCOUS_PRANDTL 0.72
#define MGCFD_VISCOUS_CFL 0.25
int mgcfd_set_viscous(mgcfd_solver *s, double mu, double prandtl, int wall, double cfl_v, int levels);
int mgcfd_get_viscous(const mgcfd_solver *s, double *mu, double *prandtl, int *wall, double *cfl_v, int *levels);
int mgcfd_viscosity_from_reynolds(const double ff17[17], double reynolds, double ref_length, double *mu);
/* Viscosity model: Sutherland's law, a caller-supplied eddy-viscosity field, the Smagorinsky model.  No reference counterpart.
 * One setting per solver, off by default (law 0, eddy 0): a solver on which the setter is never called launches and computes
 * what it did.  It applies on exactly the levels mgcfd_set_viscous covers (mu, prandtl, wall, cfl_v and levels stay that
 * call's) and has no effect while the viscous terms are off; either call may come first, and the model is kept while the terms
 * are off.  Every operation below is one IEEE-754 double operation (+ - * / sqrt), never contracted under MGCFD_OPT_EXACT = 1.
 *   law        MGCFD_VISCOSITY_CONSTANT: mu_i = mu;  MGCFD_VISCOSITY_SUTHERLAND: r = T_i / t_ref,
 *              mu_i = ((mu * (r * sqrt(r))) * (1.0 + s_ratio)) / (r + s_ratio), with T = p / rho
 *   t_ref > 0  the T at which mu(T) = mu; 0 on input takes the far field's p_inf / rho_inf in use at the call (the getter reports
 *              the value taken; a later mgcfd_set_free_stream does not change it)
 *   s_ratio    Sutherland's constant over the reference temperature (MGCFD_SUTHERLAND_S = 110.4 K / 288.15 K)
 *   eddy       MGCFD_EDDY_NONE: mut_i = +0.0;  MGCFD_EDDY_FIELD: mut_i = MGCFD_ARR_EDDY_VISCOSITY[i], the caller's array;
 *              MGCFD_EDDY_SMAGORINSKY: with G of pass 1, sxy = 0.5 * (G[u][y] + G[v][x]), sxz, syz likewise,
 *              ss = ((G[u][x]^2 + G[v][y]^2) + G[w][z]^2) + 2.0 * ((sxy^2 + sxz^2) + syz^2),
 *              mut_i = (((cs * cs) * d2_i) * rho_i) * sqrt(2.0 * ss), d2_i = cbrt(vol_i) * cbrt(vol_i) from the host's libm at
 *              enable; written to MGCFD_ARR_EDDY_VISCOSITY[i] by every stress launch (a stage or mgcfd_compute_fluxes).  No wall
 *              damping unless mgcfd_set_wall_damping is on: near a no-slip wall the model overpredicts mut.
 *   prandtl_t  the turbulent Prandtl number
 * Pass 1 of the viscous terms then finishes S_i with me_i = mu_i + mut_i on the six stresses and
 * kap_i = (GAMMA / (GAMMA - 1.0)) * (mu_i / prandtl + mut_i / prandtl_t) on the heat flux; S keeps its twelve columns, pass 2
 * and everything behind it are unchanged.  The wall-stress pass of the friction loads applies the same expressions (eddy 1 read
 * at the wall node, eddy 2 formed locally and stored nowhere), so mgcfd_wall_stress stays the wall rows of S.  The step limit
 * becomes, in the same place: a = (4.0/3.0) * (mu_i + mut_i), b = GAMMA * (mu_i / prandtl + mut_i / prandtl_t), d = a < b ? b : a,
 * sf_i = min(sf_i, ((cfl_v * rho_i) * g_i) / d) with mu_i from the level's variables at that moment and mut_i as the array
 * stands (under Smagorinsky: the last stress launch's values, +0.0 from the enabling call until the first one).
 * MGCFD_ARR_EDDY_VISCOSITY [nel][1] exists per covered level while eddy != 0: +0.0 at allocation and whenever the eddy mode
 * changes; under MGCFD_EDDY_FIELD readable and writable (values are not checked; each level has its own array, nothing is
 * restricted between levels), under MGCFD_EDDY_SMAGORINSKY read-only; otherwise MGCFD_ERR_ARG.  The arrays (and d2) are
 * allocated while both the viscous terms and a non-default model are on and released when either goes off.
 * The setter synchronises and drops captured graphs.  MGCFD_ERR_ARG, and nothing changed: an unknown law or eddy; t_ref negative
 * or not finite; s_ratio (law 1), cs (eddy 2) or prandtl_t (eddy 1, 2) not finite and positive; while a kernel-granular sweep
 * is under way; a non-default model on a solver made by mgcfd_create_partitioned* or attached to a group or as a rank.
 * mgcfd_get_viscosity_model: any pointer may be NULL.
 * The wall-limited length scale of eddy 2 is mgcfd_set_wall_damping's ("Wall distance" below).
 * Out of scope: WALE and dynamic procedures; transported models (the Spalart-Allmaras model below is one); restriction of an eddy field
 * between levels; split levels, groups and ranks; graphs and fused stages with viscosity on. */
enum { MGCFD_VISCOSITY_CONSTANT = 0, MGCFD_VISCOSITY_SUTHERLAND = 1 };
enum { MGCFD_EDDY_NONE = 0, MGCFD_EDDY_FIELD = 1, MGCFD_EDDY_SMAGORINSKY = 2 };
#define MGCFD_SUTHERLAND_S 0.3831
#define MGCFD_SMAGORINSKY_CS 0.17
#define MGCFD_PRANDTL_TURBULENT 0.9
int mgcfd_set_viscosity_model(mgcfd_solver *s, int law, double t_ref, double s_ratio, int eddy, double cs, double prandtl_t);
int mgcfd_get_viscosity_model(const mgcfd_solver *s, int *law, double *t_ref, double *s_ratio, int *eddy, double *cs, double *prandtl_t);
int mgcfd_fas_restrict(mgcfd_solver *s, int fine_level);
int mgcfd_fas_prolong(mgcfd_solver *s, int fine_level);

/* ---------------------------------------------------------------------------------
 * Kernel-granular operations (asynchronous on the solver's stream)
 * --------------------------------------------------------------------------------- */
/* copy<double>(old_variables, variables)                    src/Base/common.h:100-112 */
int mgcfd_copy_old_variables(mgcfd_solver *s, int level);
/* compute_step_factor / compute_step_factor_legacy (chosen by mesh variant exactly as
 * euler3d_cpu_double.cpp:388-395 does, unless mgcfd_set_time_step chose)   src/Kernels/cfd_loops.cpp:13-157 */
int mgcfd_compute_step_factor(mgcfd_solver *s, int level);
/* compute_flux_edge over the level's internal edges: fluxes += …   flux_loops.cpp:78-153 */
int mgcfd_compute_flux_edge(mgcfd_solver *s, int level);
/* compute_boundary_flux_edge (neighbour code -1)                   flux_loops.cpp:10-42 */
int mgcfd_compute_boundary_flux_edge(mgcfd_solver *s, int level);
/* compute_wall_flux_edge (neighbour code -2, far field)            flux_loops.cpp:44-76 */
int mgcfd_compute_wall_flux_edge(mgcfd_solver *s, int level);
/* The three above in one launch (same per-node summation order as calling them in sequence). */
int mgcfd_compute_fluxes(mgcfd_solver *s, int level);
/* time_step(j, …): variables = old + sf/(RK+1-j)*fluxes; fluxes = 0    cfd_loops.cpp:215-280 */
int mgcfd_time_step(mgcfd_solver *s, int level, int j);
/* zero_fluxes                                                       cfd_loops.cpp:282-305 */
int mgcfd_zero_fluxes(mgcfd_solver *s, int level);
/* indirect_rw over the internal edges (fluxes += …)                 indirect_rw_loop.cpp:11-78 */
int mgcfd_indirect_rw(mgcfd_solver *s, int level);
/* residual(): residuals = variables - old_variables                 validation.cpp:77-89 */
int mgcfd_residual(mgcfd_solver *s, int level);
/* calc_rms(): sqrt(sum(r^2)/nel); synchronises                      validation.cpp:91-105 */
int mgcfd_calc_rms(mgcfd_solver *s, int level, double *rms);
/* check_for_invalid_variables(); synchronises; returns MGCFD_OK or MGCFD_ERR_NAN/NEG_*;
 * *bad_cell = first offending cell in original numbering          validation.cpp:107-138 */
int mgcfd_check_for_invalid_variables(mgcfd_solver *s, int level, int64_t *bad_cell);
/* What the checks INSIDE the launches issued so far have found (every time_step / fused stage carries the reference's
 * check_for_invalid_variables; the calls themselves are asynchronous): MGCFD_OK or the first failing launch's class and
 * cell.  Unlike mgcfd_check_for_invalid_variables it does not look at the current state — the reference checks after a
 * time_step only, so a value a prolongation spoils after the last sweep goes unnoticed there too.  Synchronises; clears the flag. */
int mgcfd_pending_invalid_state(mgcfd_solver *s, int64_t *bad_cell);
/* mg_restrict(variables[fine] -> variables[fine+1])                 mg_loops.cpp:30-202 */
int mgcfd_restrict(mgcfd_solver *s, int fine_level);
/* prolong_residuals_interpolate_proper(residuals[fine+1] -> variables[fine])   mg_loops.cpp:678-864 */
int mgcfd_prolong(mgcfd_solver *s, int fine_level);

/* ---------------------------------------------------------------------------------
 * Cycle driver — the state machine of src/euler3d_cpu_double.cpp:371-694
 * --------------------------------------------------------------------------------- */
/* `sweeps` smoothing sweeps on one level, no multigrid transfer: the per-level body of the cycle
 * loop (copy, step factor, RK x [fluxes, time_step], residual; euler3d_cpu_double.cpp:383-508). */
int mgcfd_smooth(mgcfd_solver *s, int level, int sweeps);
/* Runs `cycles` (multigrid) cycles from the solver's current state.  rms_out (may be NULL)
 * receives, per cycle, the level-0 RMS the reference prints.  Synchronises before returning.
 * On an invalid state returns MGCFD_ERR_NAN / NEG_* like the reference's exit().
 * The check runs inside every time_step launch; the earliest failing launch and, within it, the smallest original
 * cell id are what is reported (the reference stops at exactly that cell).  The cycles of the current batch (up to
 * 4096) still run to the end; rms_out entries from the failing cycle on are NaN. */
int mgcfd_run_cycles(mgcfd_solver *s, int cycles, double *rms_out);
/* ---------------------------------------------------------------------------------
 * Surface loads — no reference counterpart: the pressure force and moment on the solid walls (neighbour code -1,
 * src/Base/io.cpp:92-104), the sum over those edges of the momentum term compute_boundary_flux_edge adds
 * (flux_boundary_kernel.elemfunc.c) with the far-field pressure taken off.  For edge (node b, weights w):
 * f = (p_b - p_inf) w, m = (coords[b] - ref_point) x f; summed in a fixed order (chunks of 256 edges, stride-halving
 * tree, then the same over the partial sums), never contracted to FMA: a bitwise function of the state.  INTEGRATION.md
 * gives the whole definition.  Solvers of a partitioned level or attached as ranks: MGCFD_ERR_ARG from the two calls below —
 * the loads of a level split over ranks come from mgcfd_group_surface_loads / mgcfd_group_cycles_loads and
 * mgcfd_rank_surface_loads / mgcfd_rank_cycles_loads (further down), bit for bit the same six numbers.
 * --------------------------------------------------------------------------------- */
/* Loads of level `level`'s current `variables`: out6 = Fx Fy Fz Mx My Mz.  ref_point NULL = the origin.  Synchronises.
 * A level without solid-wall edges gives exact zeros. */
int mgcfd_surface_loads(mgcfd_solver *s, int level, const double ref_point[3], double out6[6]);
/* mgcfd_run_cycles (same RMS, same final state, same errors), and loads_out[c*6 .. c*6+5] = the level-0 loads of the
 * state at the end of cycle c (after its last prolongation), recorded on the device inside the cycle and read back with
 * the RMS.  Rows of cycles that did not complete are NaN, as rms_out's. */
int mgcfd_run_cycles_loads(mgcfd_solver *s, int cycles, const double ref_point[3], double *rms_out, double *loads_out);
/* Host only: coefficients of a loads vector against the far field ff17 (mgcfd_get_far_field): q = 0.5 rho |V|^2,
 * alpha = atan2(Vy, Vx); out6 = CD = F.(cos a, sin a, 0)/(q S), CL = F.(-sin a, cos a, 0)/(q S), CS = Fz/(q S),
 * CMx CMy CMz = M/(q S c).  ref_area S and ref_length c must be positive. */
int mgcfd_load_coefficients(const double ff17[17], const double loads6[6], double ref_area, double ref_length,
                            double out6[6]);
/* ---------------------------------------------------------------------------------
 * Viscous surface loads — the friction half of the loads beside the pressure half, and the distribution along the wall.
 * The wall nodes of a level are the distinct b ends of its solid-wall edges in ascending original id.  On a level the viscous
 * terms are on for (mgcfd_set_viscous), every wall node i gets Sw_i: the twelve node stresses of pass 1 of the viscous terms
 * (u v w | txx tyy tzz txy txz tyz | qx qy qz) evaluated on the level's CURRENT variables, with the expressions, associations and
 * +0.0 starts of that pass, over the internal edges at i in the level's original edge order; MGCFD_ARR_VISCOUS_STRESS is not
 * touched.  For a solid-wall edge (node b, weights (x, y, z)), r = coords[b] - ref_point and tau from Sw_b:
 *   pressure six   exactly mgcfd_surface_loads' terms
 *   friction six   gx = -((txx*x + txy*y) + txz*z),  gy = -((txy*x + tyy*y) + tyz*z),  gz = -((txz*x + tyz*y) + tzz*z),
 *                  moment (ry*gz - rz*gy, rz*gx - rx*gz, rx*gy - ry*gx)
 * and each of the twelve columns goes through mgcfd_surface_loads' summation tree.  Every operation is one IEEE-754 double
 * operation, never contracted to FMA whatever MGCFD_OPT_EXACT says.  out12 = Fp(3) Mp(3) | Fv(3) Mv(3); the pressure six are bit
 * for bit mgcfd_surface_loads'; the total is the caller's, one addition per component.  On a level the viscous terms are not on for
 * the friction six are +0.0; a level without solid-wall edges gives twelve exact zeros and launches nothing.
 * Sign: the friction term takes the convention of the pressure term — both are what the wall face feeds into its node's momentum
 * residual with the boundary weights as the solver holds them, so Fp + Fv is one consistent vector.  On an fvcorr-variant mesh the
 * weights point into the fluid: a shear flow u = (a z, 0, 0) over a wall at z = 0 gives Fv = (-mu a A, 0, 0), a pressure excess
 * on the same wall Fp,z = +dp A.
 * The first call for a level builds its wall plan (host work, allocations); it goes with the solver.  A solver made by
 * mgcfd_create_partitioned* or attached to a group or as a rank: MGCFD_ERR_ARG from every call below.
 * --------------------------------------------------------------------------------- */
/* Pressure and friction loads of level `level`'s current `variables`.  ref_point NULL = the origin.  Synchronises. */
int mgcfd_surface_loads_viscous(mgcfd_solver *s, int level, const double ref_point[3], double out12[12]);
/* mgcfd_run_cycles_loads with rows of twelve: loads_out[c*12 .. c*12+11] = mgcfd_surface_loads_viscous of level 0 for the state at
 * the end of cycle c, recorded on the device in a twelve-wide history and read back with the RMS.  Same RMS, final state, errors
 * and NaN rows as mgcfd_run_cycles_loads.  MGCFD_OPT_GRAPH is accepted and the launches run directly. */
int mgcfd_run_cycles_loads_viscous(mgcfd_solver *s, int cycles, const double ref_point[3], double *rms_out, double *loads_out);
/* mgcfd_advance with rows of twelve (loads_out [steps][12], required): every step's loads are stored into the history on the
 * device and read back once.  Same RMS, final state, errors and NaN rows as mgcfd_advance. */
int mgcfd_advance_loads_viscous(mgcfd_solver *s, int steps, int cycles_per_step, double *rms_out, double *loads_out,
                                const double ref_point[3]);
/* The number of wall nodes of a level (0 where it has no solid-wall edge). */
int mgcfd_wall_node_count(mgcfd_solver *s, int level, int64_t *n);
/* The surface distribution of level `level`'s current `variables`, one row per wall node: node_ids [n] (may be NULL) = the
 * original ids, ascending; out [n][7] = ax ay az | dp | tx ty tz with a = the sum of the node's solid-wall edge weights (from +0.0,
 * one addition per edge in mgcfd_get_edges order), dp = p_i - p_inf, t = -(tau . a) associated as the edge terms above (+0.0 on a
 * level the viscous terms are not on for).  The t of all nodes add up to Fv, the dp a to Fp, up to rounding.  Synchronises. */
#define MGCFD_WALL_COLUMNS 7
int mgcfd_wall_distribution(mgcfd_solver *s, int level, int64_t *node_ids, double *out);
/* Diagnostic: Sw itself, out [n][12] (node_ids as above).  MGCFD_ERR_ARG on a level the viscous terms are not on for.  Under
 * MGCFD_OPT_EXACT = 1 the rows equal the wall nodes' rows of MGCFD_ARR_VISCOUS_STRESS after mgcfd_compute_fluxes on the same state. */
int mgcfd_wall_stress(mgcfd_solver *s, int level, int64_t *node_ids, double *out);
/* Diagnostic: mean GPU time of `launches` back-to-back launches of the wall-stress kernel (kind 0), the twelve-column loads kernel
 * (1) or mgcfd_surface_loads' kernel (2) on a viscous level with solid walls, as mgcfd_bench_viscous times its launches. */
int mgcfd_bench_friction_loads(mgcfd_solver *s, int level, int kind, int launches, double *avg_seconds);
/* ---------------------------------------------------------------------------------
 * Wall distance — every node's distance to the nearest solid-wall NODE of its level, the wall spacing and the wall-limited
 * Smagorinsky length scale.  No reference counterpart.  Off by default: a solver that makes none of these calls launches what
 * it launched and computes the same bits.  Every operation is one IEEE-754 double operation (+ - * / sqrt, compare), never
 * contracted to FMA whatever MGCFD_OPT_EXACT says.
 * With W_0 < W_1 < .. < W_{m-1} the level's wall nodes in ascending original id (the list of mgcfd_wall_node_count and
 * mgcfd_wall_stress) and x the level's coordinates as given at creation, for every node i:
 *   best = +inf; near = -1
 *   for j = 0 .. m-1:   dx = x_i - x_Wj;  dy = y_i - y_Wj;  dz = z_i - z_Wj;  r2 = (dx*dx + dy*dy) + dz*dz
 *                       if r2 < best: best = r2; near = j
 *   d_i = sqrt(best);   nearest_i = near < 0 ? -1 : W_near   (an original id)
 * The strict < gives a tie to the lowest wall id; a NaN r2 is never taken; a level without wall nodes has d = +inf and nearest
 * = -1 everywhere; a wall node has d = +0.0 and is its own nearest node.  The minimum is exact over all wall nodes: no search
 * radius, no approximation.  It is the distance to the nearest wall node, not to a wall face: the mesh format has no wall
 * faces, so d overestimates the face distance by up to the wall's own node spacing.
 * Wall spacing: for wall node W_k, over its internal incidences in the level's original edge order, h_k = the minimum of d_n
 * over the other ends n with d_n > 0.0, +0.0 where there is none (what y+ = h * sqrt(rho_w * tau_w) / mu_w needs).
 * Wall damping of MGCFD_EDDY_SMAGORINSKY (the Mason-Thomson / Smagorinsky-Lilly length-scale limit; there is no exp on the
 * device, hence not van Driest's exponential):
 *   a = (cs*cs) * d2_i;  kd = kappa * d_i;  w2 = kd * kd;  l2_i = w2 < a ? w2 : a      (once per node when the setting takes effect)
 *   mut_i = (l2_i * rho_i) * sqrt(2.0 * ss)
 * With d_i = +inf this is bit for bit the undamped mut_i; at a wall node mut_i = +0.0.  The wall-stress pass of the friction
 * loads applies the same expression; the step limit reads MGCFD_ARR_EDDY_VISCOSITY as before; nothing else of the viscosity
 * model changes.
 * mgcfd_compute_wall_distance: levels 0 .. levels-1 hold d afterwards (12 bytes per node on the device); levels that hold it are
 * not recomputed.  The coordinates go to the device for the computation only.  mgcfd_get_wall_distance: how many leading levels
 * hold it.  mgcfd_release_wall_distance frees it on every level.
 * MGCFD_ARR_WALL_DISTANCE [nel][1]: read-only through mgcfd_get_array (original numbering) and mgcfd_array_devptr (the layout of
 * the other one-column arrays); it exists on a level exactly while the level holds the distance, MGCFD_ERR_ARG otherwise.
 * mgcfd_wall_nearest: nearest [nel] in original numbering, original ids, -1 without a wall.  mgcfd_wall_spacing: node_ids [n]
 * (may be NULL) and h [n] in the order of mgcfd_wall_stress; both need the level to hold the distance.  Both synchronise.
 * mgcfd_set_wall_damping: kept like the viscosity model, either call may come first; no effect unless the viscous terms cover a
 * level and the eddy mode is MGCFD_EDDY_SMAGORINSKY.  Whichever of mgcfd_set_viscous, mgcfd_set_viscosity_model and
 * mgcfd_set_wall_damping makes it effective on a level that does not hold the distance computes it there; every such setter
 * synchronises, drops captured graphs and forms l2 again.  mgcfd_get_wall_damping: any pointer may be NULL.
 * MGCFD_ERR_ARG, and nothing changed: levels outside 1 .. mgcfd_num_levels; a level in range created without coordinates (also
 * from a setter that would make the damping effective there); kappa not finite and positive; mgcfd_release_wall_distance while
 * the damping is in effect on some level; while a kernel-granular sweep is under way; a solver made by mgcfd_create_partitioned*
 * or attached to a group or as a rank (a rank holds part of the wall only); a NULL nearest or h.
 * Out of scope: the distance to wall faces or a projection onto them; van Driest's exponential; transported models (the Spalart-Allmaras model below is one); restricting
 * d between levels; partitioned levels, groups and ranks; graphs and fused stages with viscosity on.
 * --------------------------------------------------------------------------------- */
#define MGCFD_ARR_WALL_DISTANCE 16        /* behind the array enum's last entry */
#define MGCFD_WALL_KAPPA 0.41
int mgcfd_compute_wall_distance(mgcfd_solver *s, int levels);
int mgcfd_get_wall_distance(const mgcfd_solver *s, int *levels);
int mgcfd_release_wall_distance(mgcfd_solver *s);
int mgcfd_wall_nearest(mgcfd_solver *s, int level, int64_t *nearest);
int mgcfd_wall_spacing(mgcfd_solver *s, int level, int64_t *node_ids, double *h);
int mgcfd_set_wall_damping(mgcfd_solver *s, int on, double kappa);
int mgcfd_get_wall_damping(const mgcfd_solver *s, int *on, double *kappa);
/* Diagnostic: mean GPU time of `launches` back-to-back launches of the wall-distance kernel on a level that holds the distance
 * (the coordinates are uploaded for the call), as mgcfd_bench_viscous times its launches. */
int mgcfd_bench_wall_distance(mgcfd_solver *s, int level, int launches, double *avg_seconds);
/* ---------------------------------------------------------------------------------
 * Spalart-Allmaras model: a transported eddy viscosity.  No reference counterpart; INTEGRATION.md "Spalart-Allmaras model"
 * holds the definition, line by line (the noft2 form with the 2012 limiter of S~; every operation one IEEE-754 double
 * operation, never contracted whatever MGCFD_OPT_EXACT says).  Selected as the eddy mode MGCFD_EDDY_SPALART_ALLMARAS of
 * mgcfd_set_viscosity_model (cs is ignored, prandtl_t is used); off by default, and a solver that never selects it launches and
 * computes what it did.  nu_tilde (nt) is a sixth transported quantity beside the state, on the levels mgcfd_set_viscous covers:
 *   level 0         pass 1 (k_sa_gradient_tile) behind the flux launch and the JST pair, before the stress launch: G of
 *                   (u, v, w, nt), the vorticity magnitude, nu_i and mut_i = (rho_i nt_i) fv1 into MGCFD_ARR_EDDY_VISCOSITY, which
 *                   the stress launch, the wall-stress pass and the step limit read as under MGCFD_EDDY_FIELD;
 *                   pass 2 (k_sa_transport_tile) before the stage's update of the five variables: upwind convection, diffusion on
 *                   averaged node gradients, production, destruction (point-implicit), nt_out = max(nt_old + dn, +0.0), +0.0
 *                   where d == 0.0.  mgcfd_compute_fluxes runs pass 1; mgcfd_time_step on level 0 runs pass 2 first.
 *   covered l >= 1  behind every restriction into the level (k_sa_restrict): nt averaged over the children as the state is, mut
 *                   from it and the restricted state; frozen until the next restriction.  Nothing of nt is prolonged.
 * The nt update is not smoothed (residual smoothing) and has no FAS forcing; JST, FAS, residual smoothing and the cycle control
 * compose with the model otherwise.  The wall distance is needed on every covered level: whichever setter makes the mode
 * effective on a level that does not hold it computes it there, and mgcfd_release_wall_distance is refused meanwhile.
 * At enable, and on mgcfd_set_free_stream(.., reinitialise = 1): nt = (ratio * mu) / rho_inf on every node of every covered
 * level, +0.0 where d == 0.0, and mut formed from it.  mgcfd_set_sa_free_stream sets ratio (MGCFD_SA_RATIO by default; kept
 * while the mode is off) and with reinitialise != 0 applies it at once.
 * MGCFD_ARR_SA_NU_TILDE [nel][1]: readable and writable on covered levels (mgcfd_set_array, mgcfd_array_devptr +
 * mgcfd_array_written; a write on level 0 is a restart).  MGCFD_ARR_SA_GRADIENT [nel][5] = G[nt][x] G[nt][y] G[nt][z] | om | nu of
 * the last pass 1: read-only, level 0.  MGCFD_ARR_EDDY_VISCOSITY is read-only under the mode.
 * MGCFD_ERR_ARG, and nothing changed: ratio not finite and positive; the mode requested while dual time stepping is on, and dual
 * time stepping requested while the mode is on (nt has no BDF source); a level the mode would take effect on created without
 * coordinates; a solver made by mgcfd_create_partitioned* or attached to a group or as a rank; while a kernel-granular sweep is
 * under way.
 * Out of scope: SA-neg, ft2, trip terms, rotation corrections; transport on coarse levels; nt in the residual smoothing or the
 * FAS forcing; far-field nt flux.  (nt under dual time and the DES lengths: mgcfd_set_sa_unsteady, below.)
 * --------------------------------------------------------------------------------- */
#define MGCFD_EDDY_SPALART_ALLMARAS 4         /* (3 is left unassigned: mgcfd_set_viscosity_model has always refused it, and callers rely on that) */
#define MGCFD_ARR_SA_NU_TILDE 17
#define MGCFD_ARR_SA_GRADIENT 18
#define MGCFD_SA_RATIO 3.0
int mgcfd_set_sa_free_stream(mgcfd_solver *s, double ratio, int reinitialise);
int mgcfd_get_sa_free_stream(const mgcfd_solver *s, double *ratio);
/* Diagnostic: mean GPU time of `launches` back-to-back launches of one of the model's kernels (kind 0: pass 1, 1: pass 2 into
 * the spare buffer, so nt stays, 2: k_sa_restrict into level `level` from the level below it), as mgcfd_bench_viscous times
 * its launches.  MGCFD_ERR_ARG where the model is not in effect. */
int mgcfd_bench_sa(mgcfd_solver *s, int level, int kind, int launches, double *avg_seconds);
/* ---------------------------------------------------------------------------------
 * Unsteady Spalart-Allmaras: nt under dual time stepping, the DES97 and delayed-DES lengths.  No reference counterpart;
 * INTEGRATION.md "Unsteady Spalart-Allmaras" holds the definition, line by line (every operation one IEEE-754 double operation,
 * never contracted whatever MGCFD_OPT_EXACT says).  One call, per solver, kept like the viscosity model while the model or the
 * viscous terms are off; the default (0, MGCFD_SA_LENGTH_WALL, MGCFD_SA_CDES) launches and computes what the model did, and keeps
 * its refusals.
 *   time_accurate = 1   lifts the two refusals between the model and mgcfd_set_dual_time.  While the model, dual time stepping and
 *                       time_accurate are all in effect, level 0 holds nt at the two last physical time levels (ntn, ntn1) and
 *                       pass 2 takes, behind Q:
 *                           a = nt_i - ntn_i;  b = ntn_i - ntn1_i
 *                           order 2: ts = (3.0 * a - b) / (2.0 * dt), cj = 1.5 / dt;   order 1: ts = a / dt, cj = 1.0 / dt
 *                           Q' = Q - vol_i * ts;   dn = (fac * Q') / (1.0 + (fac * vol_i) * (jac + cj))
 *                       with the order the state's source uses at that moment (cj formed once on the host).  Both levels are set
 *                       to nt when the combination takes effect, on mgcfd_dual_time_reset and on a reinitialising
 *                       mgcfd_set_free_stream; mgcfd_dual_time_begin_step does ntn1 <- ntn, ntn <- nt beside the state's levels
 *                       and forms mut of every covered level again from nt and the state, as a write of nt does, so that a
 *                       physical step is a function of variables, Wn, Wn1, nt, ntn and ntn1 alone.
 *                       MGCFD_ARR_SA_TIME_N / _SA_TIME_N1 [nel][1] (level 0) are readable and writable; a write marks the level
 *                       held, as one of MGCFD_ARR_TIME_N / _TIME_N1 does (a restart).
 *   length              the model length d~ that pass 2 reads wherever it read the wall distance d (the wall test, kd2, nd, jac);
 *                       the start value's wall test, the wall-stress pass and y+ keep d.  With delta_i the longest internal edge
 *                       at node i of level 0, sqrt((dx*dx + dy*dy) + dz*dz) from the coordinates as given (+inf at a node without
 *                       internal edges), and lim_i = c_des * delta_i:
 *       MGCFD_SA_LENGTH_WALL  d~ = d.
 *       MGCFD_SA_LENGTH_DES   DES97: d_i == 0.0: +0.0;  d_i <= lim_i: d_i;  otherwise lim_i.  One node-wise launch (k_sa_length)
 *                             when the setting takes effect and when it changes.
 *       MGCFD_SA_LENGTH_DDES  delayed DES (Spalart et al. 2006): the same launch first, then every pass 1 writes it
 *                             (k_sa_gradient_tile<TAIL, true>, which sums all nine velocity-gradient components):
 *                                 su = (G[u][x]*G[u][x] + G[u][y]*G[u][y]) + G[u][z]*G[u][z];  sv, sw likewise;  sq = sqrt((su + sv) + sw)
 *                                 kd = kappa * d_i;  kd2 = kd * kd;  rd = (nt_i * fv1 + nu_i) / (sq * kd2)
 *                                 e = 8.0 * rd;  z = (e * e) * e;  z = z < 20.0 ? z : 20.0;  fd = 1.0 - tanh_fixed(z)
 *                                 d_i == 0.0: +0.0;  d_i == +inf: lim_i;  d_i <= lim_i: d_i;  otherwise d_i - fd * (d_i - lim_i)
 *                             tanh_fixed(z): q = z * (1.0 / 512.0); p = 1/8!; for k = 7 .. 1: p = 1/k! + q * p; p = 1.0 + q * p;
 *                             ten times p = p * p; (p - 1.0) / (p + 1.0).
 *                       MGCFD_ARR_SA_LENGTH [nel][1] (level 0, read-only) exists while length != WALL and the model is in effect.
 * MGCFD_ERR_ARG, and nothing changed: length outside 0..2; time_accurate not 0 or 1; c_des not finite and positive; while a
 * kernel-granular sweep is under way; a solver made by mgcfd_create_partitioned* or attached to a group or as a rank;
 * time_accurate = 0 while dual time stepping is on and the model is in effect.  The setter synchronises and drops captured graphs.
 * Out of scope: IDDES, SA-neg, ft2, the low-Reynolds correction Psi; transport, time levels or d~ on coarse levels; nt in the
 * residual smoothing or the FAS forcing; partitioned levels, groups and ranks.
 * --------------------------------------------------------------------------------- */
#define MGCFD_SA_LENGTH_WALL 0      /* d~ = d */
#define MGCFD_SA_LENGTH_DES  1      /* DES97 */
#define MGCFD_SA_LENGTH_DDES 2      /* delayed DES (Spalart et al. 2006) */
#define MGCFD_SA_CDES 0.65
#define MGCFD_ARR_SA_TIME_N 20
#define MGCFD_ARR_SA_TIME_N1 21
#define MGCFD_ARR_SA_LENGTH 22
int mgcfd_set_sa_unsteady(mgcfd_solver *s, int time_accurate, int length, double c_des);
int mgcfd_get_sa_unsteady(const mgcfd_solver *s, int *time_accurate, int *length, double *c_des);
/* ---------------------------------------------------------------------------------
 * Flow statistics: time means and resolved Reynolds stresses of level 0, accumulated on the device.  No reference counterpart;
 * INTEGRATION.md "Flow statistics" holds the definition.  Off by default, per solver: a solver that never calls
 * mgcfd_set_statistics allocates nothing and launches what it launched.
 *
 * A sample is level 0's current `variables` taken with a weight w > 0.  For node i, by k_wall_distribution's expressions:
 *     u = mx / rho;  v = my / rho;  w_ = mz / rho;  speed_sqd = u*u + v*v + w_*w_;  p = (gamma - 1) * (en - 0.5 * rho * speed_sqd)
 *     x = (rho, u, v, w_, p, mut),  mut = MGCFD_ARR_EDDY_VISCOSITY[i] where level 0 holds an eddy viscosity in effect, else +0.0
 *     (the array is then not read).
 * Per solver: samples (int64) and wsum (double, from +0.0).  Per node: six means m[0..5] and seven co-moments c[0..6] for the
 * pairs uu vv ww uv uw vw pp, all from +0.0.  On the host, in double, never contracted:
 *     wsum_new = wsum + w;  a = w / wsum_new          (both reach the kernel as arguments: no division by the weight on the device)
 * Per node, every operation one IEEE-754 double operation in this association, never contracted whatever MGCFD_OPT_EXACT says:
 *     d[k] = x[k] - m[k]                 k = 0..5      (against the OLD mean)
 *     m[k] = m[k] + a * d[k]
 *     e[k] = x[k] - m[k]                 k = 1..4      (against the NEW mean)
 *     c[pair(r,s)] = c[pair(r,s)] + (w * d[r]) * e[s]  (r,s) over (u,u) (v,v) (w,w) (u,v) (u,w) (v,w) (p,p)
 * (West's weighted incremental form.)  The first sample gives m = x, up to the sign of a zero, and c = +0.0; a constant signal keeps
 * c at exact zeros.  The Reynolds stresses are c / wsum.  Averages are plain (Reynolds) averages of the primitives, not Favre averages.
 *
 * Wall statistics (MGCFD_STATISTICS_VOLUME_AND_WALL): for every wall node of level 0 the dp | tx ty tz columns of
 * mgcfd_wall_distribution's row for the same state, four means and the four per-column second moments (w * d[k]) * e[k] by the same
 * recurrence with the same a and w: a table [n_wall][8] = mean dp tx ty tz | M2 dp tx ty tz in mgcfd_wall_distribution's order
 * (t = +0.0 where the viscous terms are off).  A sample launches the wall-stress and wall-distribution kernels into a table of the
 * solver's own, then the per-wall-node accumulation.
 *
 * While a mode is on, mgcfd_advance and its _loads_viscous / _loads_heat forms take one sample with weight = dt (the physical step
 * in effect) after every physical step whose cycles completed, behind the loads launch and without a synchronisation of their own; a
 * step that goes invalid is not sampled.  mgcfd_statistics_sample works with or without dual time stepping.  The setting survives
 * mgcfd_set_viscous, mgcfd_set_viscosity_model, mgcfd_set_dual_time and mgcfd_set_free_stream in any order: the mut column follows
 * whether an eddy viscosity is in effect at the sample.
 *
 * MGCFD_ARR_STATISTICS_MEAN / _MOMENTS (level 0, while a mode is on) are readable and writable like the time levels (mgcfd_get_array,
 * mgcfd_set_array, mgcfd_array_devptr + mgcfd_array_written).  A restart: mgcfd_set_statistics, mgcfd_set_array of the two arrays,
 * mgcfd_statistics_restore(samples, wsum) and, in mode 2, mgcfd_set_wall_statistics; the run then continues in bits.
 *
 * MGCFD_ERR_ARG, and nothing changed: a mode outside 0..2; the arrays, a sample, a reset or a restore while the mode is off; a weight
 * not finite or <= 0; a restore with samples < 0, wsum negative or not finite, or exactly one of the two zero; the wall calls outside
 * mode 2 (a level without solid walls: n = 0, nothing launched); a solver made by mgcfd_create_partitioned* or attached to a group or
 * as a rank; a kernel-granular sweep under way.
 * Out of scope: Favre averages; triple correlations and budgets; temperature and nu_tilde means; phase or windowed averages and a
 * sampling interval; point probes and spectra; load statistics; coarse levels; partitioned levels, groups and ranks; captured graphs
 * containing the sample launch.
 * --------------------------------------------------------------------------------- */
#define MGCFD_ARR_STATISTICS_MEAN    23   /* [nel][6]  rho u v w p mut            level 0, while statistics are on */
#define MGCFD_ARR_STATISTICS_MOMENTS 24   /* [nel][7]  uu vv ww uv uw vw pp (co-moments, not yet divided by wsum) */
#define MGCFD_STATISTICS_OFF 0
#define MGCFD_STATISTICS_VOLUME 1
#define MGCFD_STATISTICS_VOLUME_AND_WALL 2
#define MGCFD_WALL_STATISTICS_COLUMNS 8
/* 0 releases everything; 1 / 2 allocate (zeroed, samples = 0, wsum = +0.0); 1 <-> 2 keeps the volume accumulators and (re)zeroes the
 * wall table.  Synchronises. */
int mgcfd_set_statistics(mgcfd_solver *s, int mode);
int mgcfd_get_statistics(const mgcfd_solver *s, int *mode, int64_t *samples, double *wsum);
/* accumulators, samples and wsum back to zero; asynchronous on the solver's stream */
int mgcfd_statistics_reset(mgcfd_solver *s);
/* one sample of level 0's current state; asynchronous on the solver's stream */
int mgcfd_statistics_sample(mgcfd_solver *s, double weight);
/* a restart: after mgcfd_set_array of the two arrays */
int mgcfd_statistics_restore(mgcfd_solver *s, int64_t samples, double wsum);
/* node_ids [n] (may be NULL) and out [n][MGCFD_WALL_STATISTICS_COLUMNS], n = mgcfd_wall_node_count(s, 0); synchronises */
int mgcfd_wall_statistics(mgcfd_solver *s, int64_t *node_ids, double *out);
/* a restart: in [n][MGCFD_WALL_STATISTICS_COLUMNS] in mgcfd_wall_statistics' order */
int mgcfd_set_wall_statistics(mgcfd_solver *s, const double *in);
/* host only: out8 [n][8] = Ruu Rvv Rww Ruv Ruw Rvw | p_rms | k from moments7 [n][7]:
 * R = c / wsum, p_rms = sqrt(cpp / wsum), k = 0.5 * ((Ruu + Rvv) + Rww).  wsum must be finite and positive. */
int mgcfd_statistics_derive(double wsum, const double *moments7, int64_t n, double *out8);
/* Diagnostic: mean GPU time of `launches` back-to-back launches of the volume sample (kind 0) or the wall accumulation (kind 1) on
 * level 0's current state, as mgcfd_bench_viscous times its launches.  The launches run with a = w = 0.0, so the accumulators of a
 * finite state stay as they are (up to the sign of a zero), as do samples and wsum.  Kind 1 needs mode 2 and a solid wall. */
int mgcfd_bench_statistics(mgcfd_solver *s, int kind, int launches, double *avg_seconds);
/* ---------------------------------------------------------------------------------
 * Wall thermal conditions and heat loads.  No reference counterpart; INTEGRATION.md "Wall thermal conditions" holds the
 * definition.  Every operation is one IEEE-754 double operation (+ - * sqrt), never contracted whatever MGCFD_OPT_EXACT says.
 * Off by default: a solver that never calls mgcfd_set_wall_temperature launches what it launched and computes the same bits.
 * mgcfd_set_wall_temperature is kept like the viscosity model: either setter may come first, and the setting is in effect on the
 * levels mgcfd_set_viscous covers, and only while its `wall` is 1.
 *   MGCFD_WALL_ADIABATIC    value ignored: the no-slip wall of mgcfd_set_viscous as it is.
 *   MGCFD_WALL_ISOTHERMAL   value = Tw > 0 in the solver's units (T = p / rho).  ew = Tw / (GAMMA - 1.0), formed once on the host.
 *                           Wherever the no-slip launch runs (behind every writer of a covered level's variables, on FAS's W0, at
 *                           enable, after mgcfd_set_free_stream(.., reinitialise = 1)) one launch (k_viscous_wall_isothermal) takes
 *                           its place: momentum +0.0, variables[i][4] = variables[i][0] * ew (W0: from W0's own density), and
 *                           where the update wrote residuals, residuals[i][4] = variables[i][4] - old_variables[i][4] beside the
 *                           three momentum residuals.  Density stays.  Setting the mode or a new Tw applies the launch at once;
 *                           going back to adiabatic leaves the state as it stands.
 *   MGCFD_WALL_HEAT_FLUX    value = qw, finite, positive heats the fluid.  The wall rule is the adiabatic one.  With a_i the sum of
 *                           wall node i's solid-wall edge weights (mgcfd_wall_distribution's a) and area_i = sqrt((ax*ax + ay*ay)
 *                           + az*az), formed on the host when the mode comes into effect, one launch (k_wall_heat_flux) directly
 *                           behind the viscous-flux launch of every stage does fluxes[i][4] = fluxes[i][4] + qw * area_i
 *                           (mgcfd_compute_fluxes, mgcfd_compute_flux_edge, FAS's total residual included).
 * Heat loads: with Sw of mgcfd_surface_loads_viscous (its qx qy qz carry the conductivity of whatever viscosity model is on), a
 * solid-wall edge (node b, weights (x, y, z)) gives h = -((qx*x + qy*y) + qz*z) and s = sqrt((x*x + y*y) + z*z); the two columns
 * go through the summation tree beside the twelve: out14 = Fp Mp | Fv Mv | Q A, the first twelve bit for bit
 * mgcfd_surface_loads_viscous'.  Q is the heat rate the fluid receives from the wall, A the wall's area: on an fvcorr-variant mesh
 * T = T0 + c z over a wall at z = 0 gives Q = -kappa c A.  On a level the viscous terms are not on for Q = +0.0 (A is still
 * summed); a level without solid-wall edges gives fourteen exact zeros and launches nothing.
 * mgcfd_wall_heat: one row per wall node in mgcfd_wall_distribution's order, out [n][3] = h_i T_i area_i with
 * h_i = -((qx*ax + qy*ay) + qz*az) (+0.0 on a level the viscous terms are not on for), T_i = p_i / rho_i.
 * The cycle and advance forms give the RMS, final state, errors and NaN rows of their twelve-column siblings.
 * mgcfd_free_stream_temperature (host only): t_static = p / rho of the far field by derive()'s expressions, t_total = t_static *
 * (1.0 + 0.2 * M*M) with M*M = speed_sqd / (GAMMA * t_static), from the 17 values alone.  Either pointer may be NULL.
 * MGCFD_ERR_ARG, and nothing changed: an unknown mode; Tw not finite and positive, qw not finite; while a kernel-granular sweep
 * is under way; a solver made by mgcfd_create_partitioned* or attached to a group or as a rank (every call of this section).
 * The setter synchronises and drops captured graphs.  mgcfd_set_array on variables is not followed by the wall launch.
 * Out of scope: a wall temperature per node; radiative or catalytic walls; partitioned levels, groups and ranks; graphs and fused
 * stages with the terms on; thermal conditions on slip walls.
 * --------------------------------------------------------------------------------- */
#define MGCFD_WALL_ADIABATIC 0
#define MGCFD_WALL_ISOTHERMAL 1
#define MGCFD_WALL_HEAT_FLUX 2
int mgcfd_set_wall_temperature(mgcfd_solver *s, int mode, double value);
int mgcfd_get_wall_temperature(const mgcfd_solver *s, int *mode, double *value);
int mgcfd_free_stream_temperature(const double ff17[17], double *t_static, double *t_total);   /* host only */
int mgcfd_surface_loads_heat(mgcfd_solver *s, int level, const double ref_point[3], double out14[14]);
int mgcfd_run_cycles_loads_heat(mgcfd_solver *s, int cycles, const double ref_point[3], double *rms_out, double *loads_out /* [cycles][14] */);
int mgcfd_advance_loads_heat(mgcfd_solver *s, int steps, int cycles_per_step, double *rms_out, double *loads_out /* [steps][14] */,
                             const double ref_point[3]);
#define MGCFD_WALL_HEAT_COLUMNS 3
int mgcfd_wall_heat(mgcfd_solver *s, int level, int64_t *node_ids, double *out /* [n][3] */);
/* Diagnostic: mean GPU time of `launches` back-to-back launches of the isothermal wall launch (kind 0), the adiabatic one (1), the
 * heat-flux launch (2), the fourteen-column loads (3) or k_wall_heat (4) on a no-slip viscous level with solid walls, as
 * mgcfd_bench_viscous times its launches.  Kinds 0 and 2 take the value in effect, or 1.0 where the mode is another. */
int mgcfd_bench_wall_heat(mgcfd_solver *s, int level, int kind, int launches, double *avg_seconds);
/* ---------------------------------------------------------------------------------
 * Corrected face gradients for the viscous and Spalart-Allmaras diffusion.  No reference counterpart; INTEGRATION.md "Corrected
 * face gradients" holds the definition, line by line (every operation one IEEE-754 double operation, never contracted whatever
 * MGCFD_OPT_EXACT says).  The averaged face gradient turns the Laplacian into a wide stencil on a uniform lattice and damps no
 * odd-even mode; MGCFD_FACE_GRADIENT_CORRECTED replaces its along-edge component by the two-point difference, as a correction
 * added to the fluxes directly behind F = F + V:  F[1..3] += Vc,  F[4] = (F[4] + Wk) + Hc  (the heat-flux wall's launch follows),
 * and under the Spalart-Allmaras model Qd + Qdc stands where Qd stood.  Off by default (a solver that never selects it launches
 * and computes what it did); kept like the viscosity model: either setter may come first, the mode survives the terms going
 * off, and it is in effect on the levels mgcfd_set_viscous covers.  Such a level holds G, me, kap [14][stride] and its
 * coordinates [3][stride] on the device exactly while the mode is in effect on it.  Two launches per viscous-flux launch
 * (k_face_gradient_nodes_tile directly behind the stress launch, k_face_gradient_correction_tile directly behind the viscous-flux launch) on every
 * path: the sweeps, mgcfd_compute_fluxes, mgcfd_compute_flux_edge and FAS's total residual.
 * The corrected operator is stiffer: callers that name no cfl_v take MGCFD_VISCOUS_CFL_CORRECTED under the mode
 * (mgcfd_set_viscous itself takes what it is given).
 * MGCFD_ARR_VISCOUS_GRADIENT [nel][12] = G[u][xyz] G[v][xyz] G[w][xyz] G[T][xyz] of the last such launch: read-only, on covered
 * levels while the mode is in effect.
 * The setter synchronises and drops captured graphs.  MGCFD_ERR_ARG, and nothing changed: an unknown mode; a covered level
 * created without coordinates (checked by whichever setter makes the mode effective); the corrected mode on a solver made by
 * mgcfd_create_partitioned* or attached to a group or as a rank; while a kernel-granular sweep is under way.
 * Unchanged: the node gradients, S and the wall-stress pass; the friction and heat loads and the wall tables; coarse-level SA
 * (no transport there); the viscous step limit's formula.
 * Out of scope: correcting the wall-stress pass and the loads; viscous or nt flux through boundary faces; partitioned levels,
 * groups and ranks; graphs and fused stages with the terms on; other non-orthogonal correction variants.
 * --------------------------------------------------------------------------------- */
#define MGCFD_FACE_GRADIENT_AVERAGED 0
#define MGCFD_FACE_GRADIENT_CORRECTED 1
#define MGCFD_VISCOUS_CFL_CORRECTED 0.2
#define MGCFD_ARR_VISCOUS_GRADIENT 19
int mgcfd_set_face_gradient(mgcfd_solver *s, int mode);
int mgcfd_get_face_gradient(const mgcfd_solver *s, int *mode);
/* Diagnostic: mean GPU time of `launches` back-to-back launches of the node-gradient launch (kind 0) or the correction launch
 * (kind 1; the level's fluxes keep accumulating: numbers, not a state) on a level the mode is in effect on, as
 * mgcfd_bench_viscous times its launches. */
int mgcfd_bench_face_gradient(mgcfd_solver *s, int level, int kind, int launches, double *avg_seconds);
/* ---------------------------------------------------------------------------------
 * Upwind fluxes: limited MUSCL reconstruction and Roe's flux-difference splitting on the internal edges, per level.  No
 * reference counterpart; INTEGRATION.md "Upwind fluxes" (§23) holds the same definition with its reasons.  Every operation below
 * is one IEEE-754 double operation in the order written, never contracted whatever MGCFD_OPT_EXACT says.  Off by default: a
 * solver the setter is never called on launches what it launched before and computes the same bits.
 *   levels        levels 0 .. levels-1 take the upwind flux on their internal edges; the others keep the reference's scheme
 *   muscl_levels  levels 0 .. muscl_levels-1 (<= levels) reconstruct; the other upwind levels are first order
 *   limiter       MGCFD_LIMITER_NONE, _BARTH_JESPERSEN or _VENKATAKRISHNAN;  k: Venkatakrishnan's constant
 *   entropy_fix   Harten's fraction, 0 .. 1; 0: none.  (MGCFD_UPWIND_VENKAT_K and _ENTROPY_FIX are conventions, not measurements.)
 * Stage j of an upwind level forms F from its input state W:  B = what the reference's solid-wall and far-field loops leave in
 * zeroed fluxes, in their own order;  F_i = B_i + U_i;  U_i starts at +0.0 and takes one addition per internal edge at i in the
 * level's original edge order.  Per node q = (rho, u, v, w, p): u = W1 / rho ..., p the reference's pressure expression.  Per
 * edge end (i, j, n seen from i: +e at end a, -e at end b), x the coordinates as given at creation, dx = x_j - x_i per component:
 *   pass 1 (MUSCL levels)
 *     A[v][d] += (q_j[v] - q_i[v]) * n[d];  G[v][d] = (0.5 * A[v][d]) / vol_i
 *     qmax[v] = q_j[v] if q_j[v] > qmax[v];  qmin[v] = q_j[v] if q_j[v] < qmin[v]      both from q_i[v]
 *     a second walk over the same ends:  d2 = 0.5 * ((G[v][0]*dx + G[v][1]*dy) + G[v][2]*dz)
 *       d2 > 0: d1 = qmax[v] - q_i[v];  d2 < 0: d1 = qmin[v] - q_i[v];  otherwise (zero, NaN) t = 1.0
 *       Barth-Jespersen   r = d1 / d2;  t = r if r < 1.0, else 1.0
 *       Venkatakrishnan   e2 = ((k*k)*k) * vol_i;  d11 = d1*d1;  d22 = (2.0*d2)*d2
 *                         t = ((d11 + e2)*d2 + d22*d1) / (d2 * (((d11 + d22) + d1*d2) + e2))
 *       psi[v] = t if t < psi[v], from 1.0 (no limiter: no walk, psi = 1.0)
 *     Gl[v][d] = psi[v] * G[v][d]        MGCFD_ARR_UPWIND_GRADIENT [nel][15] (3*v + d), MGCFD_ARR_UPWIND_LIMITER [nel][5]: read-only
 *   pass 2
 *     qL[v] = q_i[v] + 0.5 * ((Gl_i[v][0]*dx + Gl_i[v][1]*dy) + Gl_i[v][2]*dz);  qR[v] = q_j[v] - 0.5 * ((Gl_j[v][0]*dx + ...) + ...)
 *     unless rhoL > 0, pL > 0, rhoR > 0 and pR > 0 (and on a first-order level): qL = q_i, qR = q_j in all variables
 *     s = +1 if the first component of n that is != 0 is > 0, else -1;  m = s * n;  (qa, qb) = (qL, qR) for s > 0, else (qR, qL)
 *     U_i[k] = U_i[k] - s * Phi[k]      (the fluxes hold MINUS the outflow, as the reference's internal loop leaves them: its
 *                                        end a takes -0.5 e . (F_a + F_b)); both ends of an edge evaluate Phi on the same bits
 *   Phi(qa, qb, m):  area = sqrt((mx*mx + my*my) + mz*mz), area == 0: Phi = 0;  nh = m / area
 *     per state: un = (u*nhx + v*nhy) + w*nhz;  E = p / (GAMMA - 1.0) + (0.5*rho) * ((u*u + v*v) + w*w);  ru = rho * un
 *                Fn = (ru, ru*u + p*nhx, ru*v + p*nhy, ru*w + p*nhz, (E + p)*un);  H = (E + p) / rho
 *     ra = sqrt(rho_a), rb = sqrt(rho_b), den = ra + rb;  ut = (ra*u_a + rb*u_b) / den, vt, wt, Ht alike
 *     q2 = (ut*ut + vt*vt) + wt*wt;  c2 = (GAMMA - 1.0) * (Ht - 0.5*q2);  ct = sqrt(c2);  unt = (ut*nhx + vt*nhy) + wt*nhz;  rt = ra*rb
 *     drho, du, dv, dw, dp = b - a;  dun = (du*nhx + dv*nhy) + dw*nhz
 *     l1 = |unt - ct|, l2 = |unt|, l3 = |unt + ct|;  d = entropy_fix * (l2 + ct);  each l < d becomes (l*l + d*d) / (2.0*d)
 *     rc = rt*ct;  a1 = (dp - rc*dun) / (2.0*c2);  a2 = drho - dp / c2;  a3 = (dp + rc*dun) / (2.0*c2)
 *     k1 = l1*a1, k2 = l2*a2, ks = l2*rt, k3 = l3*a3
 *     D[0] = (k1 + k2) + k3
 *     D[1] = ((k1*(ut - ct*nhx) + k2*ut) + ks*(du - dun*nhx)) + k3*(ut + ct*nhx);   D[2], D[3] alike with v, w and nhy, nhz
 *     D[4] = ((k1*(Ht - ct*unt) + k2*(0.5*q2)) + ks*(((ut*du + vt*dv) + wt*dw) - unt*dun)) + k3*(Ht + ct*unt)
 *     Phi[k] = area * (0.5 * (Fn_a[k] + Fn_b[k]) - 0.5 * D[k])
 *   A c2 that is not positive yields NaN or infinities, which the invalid-state check catches as ever.
 * Everything behind F is unchanged and sees B + U: time_step, residual smoothing, the dual-time source, FAS, V, SA, loads, RMS;
 * step factors are unchanged.  While level 0 is an upwind level the RMS is summed in the fixed order (as under JST).
 * On an upwind level op_flux is: settle the fluxes, the flux launch with classes = 6, pass 1 (MUSCL levels), pass 2, then the
 * viscous and SA terms as ever.  No fused stage, no look-ahead and no captured graph on such a level (MGCFD_OPT_GRAPH is accepted;
 * the launches run directly); timed as MGCFD_LOOP_FLUX; iteration counts unchanged.  mgcfd_compute_fluxes gives B + U,
 * mgcfd_compute_flux_edge adds U alone.  Kernels: kernels_upwind.hip, compiled once; MGCFD_OPT_EXACT = 0 changes nothing in them.
 * The setter synchronises, drops captured graphs and keeps the state; a level's Gl and psi are one allocation, made when a MUSCL
 * level first covers it; its coordinates [3][stride] are on the device exactly while a MUSCL level (or the corrected face
 * gradient, which shares the copy) is in effect on it.  MGCFD_ERR_ARG with nothing changed: negative levels, muscl_levels >
 * levels, an unknown limiter, k not finite and positive, entropy_fix not in 0 .. 1; a MUSCL level created without coordinates;
 * JST on (and mgcfd_set_jst refuses while the upwind flux is on); a kernel-granular sweep under way; a solver made by
 * mgcfd_create_partitioned*, in a group or attached as a rank.  While on, the mgcfd_sweep_* split calls, mgcfd_group_create
 * and mgcfd_rank_attach_* refuse the solver.
 * Out of scope: split levels, groups and ranks; graphs and fused stages with it on; HLLC or AUSM; characteristic boundary
 * conditions; reconstruction of nu_tilde; freezing the limiter.
 * --------------------------------------------------------------------------------- */
#define MGCFD_LIMITER_NONE 0
#define MGCFD_LIMITER_BARTH_JESPERSEN 1
#define MGCFD_LIMITER_VENKATAKRISHNAN 2
#define MGCFD_UPWIND_VENKAT_K 5.0
#define MGCFD_UPWIND_ENTROPY_FIX 0.1
#define MGCFD_ARR_UPWIND_GRADIENT 25
#define MGCFD_ARR_UPWIND_LIMITER 26
int mgcfd_set_upwind(mgcfd_solver *s, int levels, int muscl_levels, int limiter, double k, double entropy_fix);
int mgcfd_get_upwind(const mgcfd_solver *s, int *levels, int *muscl_levels, int *limiter, double *k, double *entropy_fix);
/* Diagnostic: mean GPU time of `launches` back-to-back launches of pass 1 (kind 0, a MUSCL level) or pass 2 in the level's
 * instantiation (kind 1; the level's fluxes keep accumulating: numbers, not a state), as mgcfd_bench_jst times its launches. */
int mgcfd_bench_upwind(mgcfd_solver *s, int level, int kind, int launches, double *avg_seconds);
/* Where the last MGCFD_ERR_NAN / NEG_DENSITY / NEG_ENERGY was found: *cell = original cell id (the reference's
 * "Cell %ld"), *cycle = 0-based cycle of the mgcfd_run_cycles call (-1: not known — graph replay, or found by another call). */
int mgcfd_invalid_state_location(const mgcfd_solver *s, int64_t *cell, int *cycle);

/* ---------------------------------------------------------------------------------
 * State access (synchronous; original numbering)
 * --------------------------------------------------------------------------------- */
int mgcfd_get_array(mgcfd_solver *s, int level, int which, double *out);        /* [nel*5] or [nel] */
int mgcfd_set_array(mgcfd_solver *s, int level, int which, const double *in);
/* Edge weights after adjust/dampen, original edge order: [n_edges] records. */
/* Device address of a node array as the library holds it: [ncols][stride] fp64, structure of arrays in the
 * LIBRARY's node numbering (ncols = 5, or 1 for step factors / volumes); *count = ncols * stride elements.
 * For moving a whole level's array between two solvers built from the SAME level data (same numbering), e.g. one
 * multigrid level per GPU: send the coarse `variables` after mgcfd_restrict, the coarse `residuals` before
 * mgcfd_prolong.  The address of `variables` / `old_variables` changes with every smoothing sweep (the state buffers
 * rotate): ask again after each one.  A caller that WRITES through the pointer must say so with
 * mgcfd_array_written before the next library call on that level. */
int mgcfd_array_devptr(mgcfd_solver *s, int level, int which, void **devptr, int64_t *count);
int mgcfd_array_written(mgcfd_solver *s, int level, int which);
int mgcfd_get_edges(mgcfd_solver *s, int level, mgcfd_edge *out);
/* One multigrid level per rank: `dev_src` is the next-coarser level's `variables` as ANOTHER solver built from the same
 * level data holds it after its mgcfd_restrict(fine_level) (its mgcfd_array_devptr, or a received copy of it).  Copies
 * the coarse nodes that HAVE children; a coarse node without children keeps this solver's value, as mg_restrict leaves
 * it (src/Kernels/mg_loops.cpp:63-78,174-189) — only the rank that sweeps the coarse level has that value. */
int mgcfd_accept_restricted(mgcfd_solver *s, int fine_level, const void *dev_src);

/* ---------------------------------------------------------------------------------
 * Monitoring — LoopNumIters.csv / Times.csv contents
 * (src/Monitoring/loop_stats.cpp:48-171, src/Monitoring/timer.cpp:58-195)
 * --------------------------------------------------------------------------------- */
int mgcfd_get_loop_iters(const mgcfd_solver *s, int level, int64_t out[MGCFD_NUM_LOOPS]);
int mgcfd_get_loop_times(mgcfd_solver *s, int level, double out_seconds[MGCFD_NUM_LOOPS]);
int mgcfd_reset_monitoring(mgcfd_solver *s);
/* Average GPU duration (seconds) of the internal-edge flux launches issued since the last
 * reset, measured with hipEvents on the launch stream, and how many launches that covers.
 * Requires MGCFD_OPT_TIMING. */
int mgcfd_get_flux_kernel_time(mgcfd_solver *s, int level, double *avg_seconds, int64_t *launches);

/* Diagnostic: mean GPU time of `launches` back-to-back flux launches (internal + boundary +
 * far field, starting from zero fluxes), hipEvents around the batch on the solver's stream. */
int mgcfd_bench_flux(mgcfd_solver *s, int level, int launches, double *avg_seconds);
/* Diagnostic: the same for `launches` back-to-back launches of one kind of residual-smoothing iteration (kind 0: the first,
 * which forms D on load; 1: a middle one; 2: the last, which applies the update — here into the second state buffer, without
 * check or residual, so the state stays), behind one flux launch.  MGCFD_ERR_ARG while the smoothing is off. */
int mgcfd_bench_residual_smoothing(mgcfd_solver *s, int level, int kind, int launches, double *avg_seconds);
/* Diagnostic: the same for one of the JST dissipation's launches (kind 0: the sensor, 1: the dissipation, which adds into
 * fluxes[] launch after launch; the state stays), behind one flux launch with both passes.  MGCFD_ERR_ARG where it is off. */
int mgcfd_bench_jst(mgcfd_solver *s, int level, int kind, int launches, double *avg_seconds);
/* Diagnostic: the same for one of the viscous terms' launches (kind 0: the stress launch, 1: the viscous-flux launch, which adds
 * into fluxes[] launch after launch; the state stays; 2: the step limit's launch on the level's step factors, k_viscous_clamp or
 * under a non-default viscosity model k_viscous_clamp_variable), behind one flux launch with both passes.  The stress launch is
 * the instantiation the viscosity model selects.  MGCFD_ERR_ARG where they are off. */
int mgcfd_bench_viscous(mgcfd_solver *s, int level, int kind, int launches, double *avg_seconds);
/* Diagnostic: the same for one of FAS multigrid's launches between `fine_level` and the level above it, behind one
 * mgcfd_fas_restrict (kind 0: k_restrict_fas, 1: the forcing launch, 2: the forced update k_time_step_src<0, true> on the
 * coarse level, 3: the FAS prolongation) and for the launches they stand beside (4: k_restrict, 5: k_time_step on the coarse
 * level, 6: the reference's prolongation, which moves the fine state: re-initialise afterwards).  MGCFD_ERR_ARG while FAS is off. */
int mgcfd_bench_fas(mgcfd_solver *s, int fine_level, int kind, int launches, double *avg_seconds);
/* The same for the indirect_rw probe (src/Kernels/indirect_rw_loop.cpp:8-78; fluxes += ..., accumulating over the
 * launches): the empirical data-movement ceiling of the flux kernel on this level's tiles. */
int mgcfd_bench_indirect_rw(mgcfd_solver *s, int level, int launches, double *avg_seconds);
/* ... and for a tile-shaped STREAM of exactly the bytes SURVEY.md §8(d) prices for that launch (40 B per internal edge + 40 B per
 * node read, 40 B per node written; one workgroup per tile, nothing dependent, nothing computed): the practical ceiling of its
 * data movement on this chip, launch included.  Overwrites `fluxes`. */
int mgcfd_bench_stream_ceiling(mgcfd_solver *s, int level, int launches, double *avg_seconds);
/* Diagnostic: out[i] = f(in[i]) for the n host doubles of `in`, with f one of the approximations the MGCFD_OPT_EXACT = 0 build's
 * order-free flux kernel uses in place of division and square root, run on the device from that build (whatever MGCFD_OPT_EXACT
 * is set to): kind 0 its 1/x, kind 1 its sqrt(x) with the special cases (+0 -> +0, +inf -> +inf, negative or NaN -> NaN), kind 2
 * its sqrt(x) for x > 0 without them.  What tests/test_gpu_fast_accuracy.py measures against long double. */
int mgcfd_diag_fast_math(mgcfd_solver *s, int kind, int64_t n, const double *in, double *out);

/* ---------------------------------------------------------------------------------
 * Multi-GPU hooks (one process per GPU; the collectives themselves are issued by the
 * host through RCCL — see INTEGRATION.md).  compute_step_factor's global min
 * (cfd_loops.cpp:137-150) is split so an all-reduce(min) can run between the halves.
 * --------------------------------------------------------------------------------- */
/* First half: per-node cfl*dt (cfl = 0.5 unless mgcfd_set_time_step chose) and the rank-local minimum, left in a device
 * scalar.  MGCFD_ERR_ARG under a local time step. */
int mgcfd_step_factor_local(mgcfd_solver *s, int level);
/* Device address of that fp64 scalar (for an in-place RCCL all-reduce MIN). */
int mgcfd_step_factor_min_devptr(mgcfd_solver *s, int level, void **devptr);
/* Second half: step_factors[i] = min_dt / volumes[i]. */
int mgcfd_step_factor_apply(mgcfd_solver *s, int level);
/* One smoothing sweep (as mgcfd_smooth) split around that all-reduce, with the fused stage
 * kernels: sweep_begin = first half of compute_step_factor (skipped when the launch that produced
 * the variables already left its minima behind) + reduction to the scalar behind
 * mgcfd_step_factor_min_devptr; [all-reduce MIN that scalar across ranks];
 * sweep_end = the RK stages (fluxes + time_step fused, "/ volume" applied in the first) + residual.
 * Optional, to HIDE the all-reduce: sweep_flux0 computes the first stage's fluxes, which do not
 * depend on the time step, and may run while the collective is in flight; sweep_end then starts
 * with time_step on them. */
int mgcfd_sweep_begin(mgcfd_solver *s, int level);
/* The same split with the PARTIAL minima as the exchanged quantity: *devptr = the level's per-workgroup minima
 * (*count fp64 values, a few KB), to be all-reduced (MIN, element-wise) in place of the scalar.  sweep_begin_partials
 * then launches nothing when an earlier launch already left the minima behind, and sweep_end_partials lets the first
 * stage take the minimum over the (now global) partials — one small kernel and 5 us less on the way to the collective.
 * Same results as sweep_begin / sweep_end. */
int mgcfd_step_factor_partials_devptr(mgcfd_solver *s, int level, void **devptr, int *count);
/* The Runge-Kutta stages of such a sweep ONE AT A TIME, for a partitioned level: after mgcfd_sweep_begin[_partials] and
 * the all-reduce, call mgcfd_sweep_stage(s, level, j, partials) for j = 0, 1, 2 — each a single fused launch (fluxes +
 * time_step; the first finishes compute_step_factor, the last writes the residual and ends the sweep) — and between
 * them move the ghosts' new values with mgcfd_halo_pack / _unpack on MGCFD_ARR_STAGE (the state that stage wrote; the
 * ghosts hold no rows, so a stage leaves them at the sweep's start state until the message arrives). */
int mgcfd_sweep_stage(mgcfd_solver *s, int level, int j, int partials);
int mgcfd_sweep_begin_partials(mgcfd_solver *s, int level);
int mgcfd_sweep_end_partials(mgcfd_solver *s, int level);
int mgcfd_sweep_flux0(mgcfd_solver *s, int level);
int mgcfd_sweep_end(mgcfd_solver *s, int level);
/* Halo exchange of a partitioned level.  A plan is a list of local node ids (the nodes this rank
 * sends to one peer, or the ghosts it receives from it, in an order both sides agree on);
 * pack copies their 5 values of array `which` (MGCFD_ARR_*) into a contiguous [n][5] fp64 message
 * in DEVICE memory, unpack writes a received message into them.  The message itself moves by
 * RCCL send/recv (torch.distributed) between the two calls. */
int mgcfd_halo_plan(mgcfd_solver *s, int level, int64_t n, const int64_t *node_ids, int *plan);
int mgcfd_halo_pack(mgcfd_solver *s, int level, int plan, int which, void *dev_buf);
int mgcfd_halo_unpack(mgcfd_solver *s, int level, int plan, int which, const void *dev_buf);
/* Sum of squared residuals of the level, left in a device scalar (all-reduce SUM, then
 * rms = sqrt(sum / global_nel)). */
int mgcfd_residual_sumsq(mgcfd_solver *s, int level, void **devptr);

/* ---------------------------------------------------------------------------------
 * Multi-GPU in the C++ host: a level PARTITIONED over ranks (mgcfd_create_partitioned), the whole
 * sweep loop inside the library.  The reference has no distributed path; what a partitioned level
 * needs follows from its loops: one all-reduce(MIN) of the time step per sweep
 * (src/Kernels/cfd_loops.cpp:137-150) and, because every RK stage reads the neighbours' new state
 * (src/Kernels/flux_loops.cpp:133-136 after cfd_loops.cpp:241-268), one halo message per neighbouring
 * rank after every stage.  Per stage the library runs the tiles next to ghost nodes first, packs every
 * peer's segment with ONE launch, sends (RCCL ncclSend/ncclRecv grouped on a second stream; between the
 * solvers of one process hipMemcpyPeerAsync over xGMI), runs the interior tiles while the message travels,
 * and unpacks with ONE launch before the next stage's boundary tiles.  Results equal the unpartitioned
 * level's bit for bit on owned nodes.  The solvers of one process skip the message buffers altogether: behind its
 * boundary tiles a rank stores the nodes its peers need straight into their ghost slots (one launch, peer access
 * over xGMI) and a peer's next stage waits for that launch's event (MGCFD_GROUP_DIRECT=0 in the environment keeps
 * the buffered form).
 *
 * Two ways to be a rank:
 *   one rank per PROCESS (RCCL):  mgcfd_rccl_unique_id on rank 0, the 128 bytes handed to every rank by the
 *       launcher (MPI, torch.distributed, a file), mgcfd_rank_attach_rccl, mgcfd_rank_set_halo,
 *       mgcfd_rank_exchange once, then mgcfd_rank_sweeps.  librccl is loaded when first needed.
 *   the solvers of ONE process (one per device): mgcfd_group_create, mgcfd_rank_set_halo on each,
 *       mgcfd_group_exchange once, then mgcfd_group_sweeps — what euler3d_gpu_double --gpus N runs.
 * --------------------------------------------------------------------------------- */
typedef struct mgcfd_group mgcfd_group;
int mgcfd_rccl_unique_id(void *out128);
int mgcfd_rank_attach_rccl(mgcfd_solver *s, int rank, int world, const void *id128);
int mgcfd_rank_detach(mgcfd_solver *s);
/* The level's neighbours: peers[k] ascending; send_ids[k] = the OWNED local nodes peer k holds as ghosts, recv_ids[k] =
 * the local GHOSTS peer k owns, both in an order the two ranks agree on (ascending global id).  Also splits the level's
 * tiles into boundary / interior for the overlapped exchange.
 * A level that already has an exchange gets a new one: the call synchronises the solver's stream and the old exchange's
 * message stream and frees the old one.  It is refused (MGCFD_ERR_ARG, nothing changed) while other ranks hold device
 * addresses into the old exchange: while it is attached through HIP IPC (mgcfd_rank_ipc_detach on every rank first), and
 * once a group has run mgcfd_group_exchange, sweeps or cycles on the level (create the solvers and the group anew). */
int mgcfd_rank_set_halo(mgcfd_solver *s, int level, int n_peers, const int *peers, const int64_t *send_counts,
                        const int64_t *const *send_ids, const int64_t *recv_counts, const int64_t *const *recv_ids);
int mgcfd_rank_halo_info(const mgcfd_solver *s, int level, int64_t out[4]);   /* boundary tiles, interior tiles, nodes sent, nodes received */
/* What the solver is a rank of, as the library sees it: out[0] this rank, out[1] the number of ranks, out[2] the transport
 * (0 none, 1 an RCCL communicator, 2 an in-process group, 3 plain attachment: HIP IPC messages only), out[3] the size the RCCL
 * communicator itself reports (ncclCommCount; -1 without one). */
int mgcfd_rank_info(const mgcfd_solver *s, int out[4]);
/* MGCFD_OPT_GRAPH = 1 on an RCCL rank (mgcfd_rank_sweeps): out[0] = sweep graphs instantiated for the level (0..3, one per
 * buffer rotation), out[1] = 1 when a capture was refused — the sweeps then run call by call, with the same results —,
 * out[2] = sweeps replayed from a graph so far.  A caller that times the replayed form asks before it believes the figure. */
int mgcfd_rank_graph_status(const mgcfd_solver *s, int level, int64_t out[3]);
int mgcfd_rank_exchange(mgcfd_solver *s, int level);          /* ghosts of `variables` <- owners (after mgcfd_set_array) */
int mgcfd_rank_sweeps(mgcfd_solver *s, int level, int sweeps); /* the per-level body of the cycle loop, `sweeps` times; asynchronous */
int mgcfd_rank_residual_sumsq(mgcfd_solver *s, int level, double *sum_all_ranks);
/* Ranks in different processes, messages as direct stores (opt-in; rehearsed with two processes on ONE GPU only): every rank
 * publishes HIP IPC handles of its three state buffers and of a few flag words, opens its neighbours', and a stage's message
 * is then ONE launch that stores the nodes the neighbours need straight into their ghost slots (over xGMI between devices)
 * and raises their flags; the neighbour's next stage starts behind a one-wave launch that waits for them.  No message
 * buffers, no second stream, no RCCL call per stage; with EVERY rank attached the all-reduce of a global time step goes
 * through the same flags (every rank stores its minimum into every other rank's memory) and no collective library is needed
 * at all, otherwise it stays on RCCL.
 *   mgcfd_rank_attach_plain (or mgcfd_rank_attach_rccl), mgcfd_rank_set_halo, then mgcfd_rank_ipc_export_size / _export, the
 *   blobs handed round by the launcher, mgcfd_rank_ipc_attach (the other ranks' blobs in any order: at least the neighbours',
 *   at most 16 ranks); from then on mgcfd_rank_exchange / mgcfd_rank_sweeps run the direct form.
 *   mgcfd_rank_ipc_status: waits for a neighbour that gave up (about 2 s each) since the last call; 0 = all messages arrived.
 *   A wait that gave up is an ERROR, not a statistic: the stages behind it ran on stale ghosts.  While the count is not zero
 *   mgcfd_synchronize and mgcfd_get_array return MGCFD_ERR_HIP, and so does the next mgcfd_rank_sweeps after one of them has
 *   seen it; mgcfd_rank_ipc_status reads the count and thereby acknowledges it (mgcfd_rank_ipc_detach clears it too).
 *   The ranks keep each other in step through the flags only WITHIN this form: before the first mgcfd_rank_exchange — and
 *   whenever a rank has touched the level by other means (mgcfd_set_array, another kind of sweep) — the caller synchronises
 *   the ranks (a barrier), or a neighbour's stores may land in a buffer that is still in use. */
int mgcfd_rank_attach_plain(mgcfd_solver *s, int rank, int world);
int mgcfd_rank_ipc_export_size(mgcfd_solver *s, int level, int64_t *bytes);
int mgcfd_rank_ipc_export(mgcfd_solver *s, int level, void *out);
int mgcfd_rank_ipc_attach(mgcfd_solver *s, int level, int n_exports, const void *const *exports);
int mgcfd_rank_ipc_status(mgcfd_solver *s, int level, int *timed_out);
int mgcfd_rank_ipc_detach(mgcfd_solver *s, int level);       /* back to the buffered form; closes the neighbours' mappings */
int mgcfd_group_create(int n, mgcfd_solver *const *solvers, mgcfd_group **out);   /* solvers[r] becomes rank r of n */
void mgcfd_group_destroy(mgcfd_group *g);       /* its solvers are ranks of nothing afterwards; they and the group may be destroyed in either order */
/* mgcfd_set_free_stream on every rank: one pass leaves all ranks idle and without graphs (the group's own sweep graph,
 * MGCFD_GROUP_GRAPH=1, included), a second one sets them; a bad argument or a sweep under way changes no rank.  The group calls that run sweeps, cycles or loads (mgcfd_group_sweeps[_rms],
 * mgcfd_group_cycles[_loads], mgcfd_group_surface_loads) return MGCFD_ERR_ARG while the ranks' far fields differ in any bit;
 * the message names the first rank that differs from rank 0. */
int mgcfd_group_set_free_stream(mgcfd_group *g, double mach, double alpha_deg, int reinitialise);
/* mgcfd_set_time_step on every rank, in the same two passes; a bad argument or a sweep under way changes no rank.  The group
 * calls that run sweeps, cycles or loads return MGCFD_ERR_ARG while the ranks' mode or CFL number differ; the message names the
 * first rank that differs from rank 0. */
int mgcfd_group_set_time_step(mgcfd_group *g, int mode, double cfl);
int mgcfd_group_exchange(mgcfd_group *g, int level);
int mgcfd_group_sweeps(mgcfd_group *g, int level, int sweeps);   /* asynchronous; a host thread per rank issues that rank's launches */
/* The same with calc_rms (src/Kernels/validation.cpp:91-105) after every sweep — the reference's cycle loop prints it per
 * cycle, src/euler3d_cpu_double.cpp:383-508 — gathered on the devices and read back ONCE: rms_of_each[k] = RMS after
 * sweep k.  At most 4096 sweeps per call.  Synchronises. */
int mgcfd_group_sweeps_rms(mgcfd_group *g, int level, int sweeps, double *rms_of_each);
int mgcfd_group_rms(mgcfd_group *g, int level, double *rms);
/* V-cycles on a PARTITIONED HIERARCHY (mgcfd_create_partitioned_mg; mgcfd_rank_set_halo on EVERY level, ghosts current:
 * mgcfd_group_exchange / mgcfd_rank_exchange on every level once): the reference's cycle — sweeps on levels 0 .. n-1, n-2 .. 1,
 * mg_restrict on the way up, prolong_residuals_interpolate_proper on the way down, src/euler3d_cpu_double.cpp:371-694 — with
 * the ghost values moved where the next loop reads them: `variables` after every time_step (one message per Runge-Kutta stage,
 * as in mgcfd_group_sweeps), after mg_restrict (coarse ghosts) and after the prolongation (fine ghosts), the coarse `residuals`
 * before the prolongation; one all-reduce(MIN) of the time step per sweep.  Every level equals mgcfd_run_cycles on the whole
 * hierarchy bit for bit on owned nodes.  rms_out (may be NULL): the level-0 RMS after the level-0 sweep of each cycle, as the
 * reference prints it.  Returns MGCFD_OK or MGCFD_ERR_NAN / NEG_* (check_for_invalid_variables inside every time_step).
 * At most 4096 cycles per call.  Synchronises. */
int mgcfd_group_cycles(mgcfd_group *g, int cycles, double *rms_out);
int mgcfd_rank_cycles(mgcfd_solver *s, int cycles, double *rms_out);      /* one rank per process over RCCL (mgcfd_rank_attach_rccl) */
int mgcfd_group_synchronize(mgcfd_group *g);
/* Surface loads of a level split over ranks: bit for bit what mgcfd_surface_loads returns for the same state on one solver
 * that holds the whole level.  The definition is unchanged — chunks of 256 edges of the WHOLE level's solid-wall slice in the
 * whole level's order, the stride-halving tree, the tree over the partial sums, never contracted — so every rank says where
 * its edges lie in that slice: slot[k] = position, in [boundary_start, boundary_start + n_boundary) of the whole level, of
 * this rank's k-th solid-wall edge (its local boundary-class edges in local order); n_total = the whole level's n_boundary
 * (0 is legal: a level without solid walls), n = how many slots are given.  MGCFD_ERR_ARG unless the solver was made by
 * mgcfd_create_partitioned*, n equals the level's local n_boundary and the slots are strictly ascending in [0, n_total)
 * (local edge lists keep the whole level's order).  Every rank stores its edges' six terms at their slots of a table on
 * rank 0 (stores and copies only, never an arithmetic reduction), rank 0 reduces the table. */
int mgcfd_rank_set_wall_slots(mgcfd_solver *s, int level, int64_t n_total, int64_t n, const int64_t *slot);
/* In-process groups.  Before the first launch the group checks on the host that every rank has slots on the level, that all
 * name the same n_total and that together they name 0 .. n_total-1 exactly once: MGCFD_ERR_ARG otherwise ("wall slots", and
 * the rank).  mgcfd_group_surface_loads: the loads of `level`'s current state; synchronises.  mgcfd_group_cycles_loads:
 * mgcfd_group_cycles (same RMS, same final state on every rank, same errors) and loads_out[c*6 .. c*6+5] = the level-0 loads
 * of the state cycle c leaves (after its last prolongation and the exchange behind it), recorded on rank 0's device inside
 * the cycles, read back once; rows stay NaN when the call fails before the read-back. */
int mgcfd_group_surface_loads(mgcfd_group *g, int level, const double ref_point[3], double out6[6]);
int mgcfd_group_cycles_loads(mgcfd_group *g, int cycles, const double ref_point[3], double *rms_out, double *loads_out);
/* One rank per process over RCCL (mgcfd_rank_attach_rccl): collective, every rank receives the same numbers.  The ranks'
 * edge counts are agreed once, outside the cycles (their sum must be n_total: MGCFD_ERR_ARG), the slots go to rank 0 once;
 * per evaluation every other rank sends its terms to rank 0 (ncclSend / ncclRecv), which places them by slot and reduces.
 * NOTE: exercised with ONE rank only, the most a one-GPU box offers; the messages between several ranks have never run. */
int mgcfd_rank_surface_loads(mgcfd_solver *s, int level, const double ref_point[3], double out6[6]);
int mgcfd_rank_cycles_loads(mgcfd_solver *s, int cycles, const double ref_point[3], double *rms_out, double *loads_out);

#ifdef __cplusplus
}
#endif
#endif /* MGCFD_H */
