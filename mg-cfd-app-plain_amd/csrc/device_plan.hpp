// device_plan.hpp — plain structs shared by the host solver and the HIP kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "preprocess.hpp"

namespace mgcfd {

// Per-node arrays are stored structure-of-arrays with a common padded stride
// (stride = 256 * n_tiles): q[f*stride + i], f = 0..4 = the reference's `variables[i*5 + f]`;
// likewise old_variables, fluxes, residuals.
constexpr int kNumStateFields = 5;
static_assert(sizeof(EdgeW) == 32, "EdgeW must be 32 bytes");
static_assert(sizeof(ProlongW) == 24, "ProlongW must be 24 bytes");

// launch_flux's variant bit for the bit-identical fused stages (never part of a user's MGCFD_OPT_FLUX_VARIANT: solver.cpp adds
// it with MGCFD_OPT_STAGE_WG4): the four-workgroups-per-CU instantiation where the level's tile halos fit kTileCap4 - kTile slots
constexpr int kVariantStageWg4 = 1 << 7;

// ff_variable + ff_flux_contribution_* (src/Base/globals.h:11-15), passed by value.
struct FarField {
    double var[5];
    double fc_mx[3], fc_my[3], fc_mz[3], fc_de[3];
};

// Where a halo "push" stores (kernels_plain.hip: k_halo_push): the state buffers of up to kMaxPushPeers neighbouring ranks
// (peer access over xGMI, or the same device), the peers' segments of the message being consecutive slot ranges.
constexpr int kMaxPushPeers = 8;
struct PushPeers {
    double *base[kMaxPushPeers] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // peer p's state buffer [5][stride[p]]
    int64_t stride[kMaxPushPeers] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t first[kMaxPushPeers + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};     // slots [first[p], first[p+1]) go to peer p
    int n = 0;
};

// The flags a push raises in its peers once its stores are on their way (ranks in different processes: kernels_plain.hip,
// k_halo_push with flags, k_flags_wait): flag[p] = the word in peer p's memory, value = this message's sequence number.
struct PushFlags {
    unsigned long long *flag[kMaxPushPeers] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    unsigned long long value = 0;
    int n = 0;
};
// The message of a stage sent by the stage launch itself (k_flux_tile<..., PUSH>): the launch covers a rank's boundary tiles
// FIRST (workgroups [0, n_boundary)) and its interior tiles behind them; a boundary tile's epilogue stores the nodes the
// neighbours need (per-node lists: send_ptr / send_peer / send_target) into their ghost slots, and the boundary tile that
// finishes last raises the neighbours' flags — while the interior tiles of the same launch are still running.
struct StagePush {
    const int32_t *send_ptr = nullptr;      // [nel + 1] (library numbering): a node's entries
    const int8_t *send_peer = nullptr;      // [entries] position of the destination in peers
    const int32_t *send_target = nullptr;   // [entries] the node's index in that peer's numbering
    PushPeers peers;
    PushFlags flags;
    unsigned *ticket = nullptr;
    int32_t n_boundary = 0;
};

// A rank's flag words are rows of four (one per Runge-Kutta stage + one for the time-step all-reduce), one row per SOURCE rank.
constexpr int kMaxIpcRanks = 16;
struct FlagRows { int row[kMaxIpcRanks] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; int n = 0; };
// The all-reduce(MIN) of the time step between processes without a collective library: every rank stores its minimum into
// slot [parity][its rank] of every other rank's array and raises that rank's flag (k_min_publish); whoever has seen all flags
// holds all minima.
struct MinPublish {
    double *mins[kMaxIpcRanks] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};              // rank p's array [2][kMaxIpcRanks] (own rank: the local one)
    unsigned long long *flag[kMaxIpcRanks] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // rank p's flag word [this rank][3]
    int world = 0, me = 0, parity = 0;
    unsigned long long value = 0;
};

// Arguments of the time_step half of a fused flux + time_step launch (kernels.hip: k_flux_tile<FUSE>).
struct FusedStep {
    double rk_div = 1.0;                      // double(RK+1-j)
    double *step_factors = nullptr;
    const double *old_variables = nullptr;
    double *q_out = nullptr;                  // new variables (must differ from the launch's input state)
    const double *partial_min = nullptr;      // != nullptr on the first stage: finish compute_step_factor here
    int n_partial = 0;
    const double *volumes = nullptr;
    double *residuals = nullptr;              // != nullptr on the last stage: residuals = variables - old
    const int32_t *old_of_new = nullptr;
    unsigned long long *err = nullptr;
    int check = 0;
    // last stage extras
    // role 5 (a middle stage that applies the FIRST stage's time_step while it stages its input): the first stage's
    // fluxes and its divisor RK+1-0; the input state is then old_variables + (min_dt/volume/vin_div) * vin_flux
    const double *vin_flux = nullptr;
    double vin_div = 4.0;
    int check_vin = 0;                        // ... and the check sequence number of that absorbed time_step (earlier than `check`)
    double *sumsq_partial = nullptr;          // != nullptr (last stage): per-tile sums of squares of the residuals (calc_rms, validation.cpp:91-105)
    // look-ahead for the NEXT sweep on this level, from the state this launch produces:
    double *next_partial_min = nullptr;       // first half of compute_step_factor: per-tile minima of 0.5*cbrt(vol)/(|v|+c)
    const double *cbrt_vol = nullptr;
    double *next_legacy_sf = nullptr;         // a local time step: next sweep's step factors go here — cfl/(sqrt(vol)*(|v|+c)) (cfd_loops.cpp:37-61) ...
    int next_nodal = 0;                       // ... or, when set, (cfl*cbrt(vol)/(|v|+c))/vol (MGCFD_DT_LOCAL)
    double cfl = 0.5;                         // the CFL number of whichever look-ahead runs (the reference's literal 0.5)
    // a launch over PART of the level's tiles (a partitioned level: the tiles next to ghost nodes first, so that their
    // results can travel while the others are computed): tile_list[k] = tile of workgroup k; nullptr = all tiles
    const int32_t *tile_list = nullptr;
    int32_t n_list = 0;
    // > 0: the launch treats only nodes [0, nel_active) as present (a partitioned level whose ghosts are numbered last:
    // the ghost slots are then written by halo messages only — a peer may be storing into them during this launch)
    int64_t nel_active = 0;
};

// One Jacobi iteration of the implicit residual smoothing (kernels.hip: k_smooth_tile; mgcfd_set_residual_smoothing).
struct SmoothStep {
    const double *fluxes = nullptr;           // the stage's fluxes F [5][stride] and ...
    const double *step_factors = nullptr;     // ... the sweep's step factors: D = step_factors * F
    const double *prev = nullptr;             // the previous iteration's result [5][stride]; nullptr: the first iteration (starts from D)
    double *next = nullptr;                   // this iteration's result; nullptr: the last iteration, which applies the update instead:
    double eps = 0.0;
    double rk_div = 1.0;                      // double(RK+1-j)
    const double *old_variables = nullptr;
    double *q_out = nullptr;                  // variables = old_variables + result / rk_div
    double *residuals = nullptr;              // != nullptr: residuals = variables - old_variables
    const int32_t *old_of_new = nullptr;
    unsigned long long *err = nullptr;
    int check = 0;
};

// The two launches of the JST dissipation (kernels.hip: k_jst_sensor_tile, k_jst_dissipation_tile; mgcfd_set_jst): the sensor
// writes lap, nu and r from w; the dissipation reads all four and adds the correction C into fluxes.
struct JstStep {
    const double *w = nullptr;                // the stage's input state W [5][stride]: what the fluxes were computed from
    double *lap = nullptr;                    // L [5][stride]: the undivided Laplacian of W over the internal edges
    double *nu = nullptr;                     // [stride] the pressure sensor
    double *r = nullptr;                      // [stride] the spectral radius |v| + c
    double *fluxes = nullptr;                 // the stage's fluxes F [5][stride] (dissipation only): F = F + C
    double kappa2 = 0.0, kappa4 = 0.0;
};

// The viscosity model of a level (mgcfd_set_viscosity_model): how pass 1 of the viscous terms, the wall-stress pass and the
// step limit form a node's viscosity mu_i and eddy viscosity mut_i.  law 0 and eddy 0 is the constant viscosity: nothing
// here is read then.
struct ViscosityModel {
    int law = 0;                              // 0 constant, 1 Sutherland: mu_i = ((mu * (r * sqrt(r))) * one_plus_s) / (r + s), r = T_i / t_ref
    int eddy = 0;                             // 0 none, 1 the caller's field (mut read), 2 Smagorinsky (mut written by the stress launch)
    double t_ref = 1.0, s = 0.0, one_plus_s = 1.0;
    double c2 = 0.0;                          // cs * cs
    double cp = 0.0;                          // GAMMA / (GAMMA - 1.0)
    double prandtl = 1.0, prandtl_t = 1.0;
    double *mut = nullptr;                    // eddy_viscosity [stride]
    const double *d2 = nullptr;               // [stride] cbrt(vol) * cbrt(vol), from the host; damped: l2 (k_wall_length) in its place
    int damped = 0;                           // eddy 2 under wall damping (mgcfd_set_wall_damping): d2 holds l2_i = min(c2 d2_i, (kappa d_i)^2)
    __host__ __device__ bool variable() const { return law != 0 || eddy != 0; }
};

// The two launches of the viscous terms (kernels.hip: k_viscous_stress_tile, k_viscous_flux_tile; mgcfd_set_viscous): the stress
// launch writes s from w; the flux launch reads s and adds the viscous flux V into components 1..4 of fluxes.
struct ViscousStep {
    const double *w = nullptr;                // the stage's input state W [5][stride]: what the fluxes were computed from
    double *s = nullptr;                      // S [12][stride]: u v w | txx tyy tzz txy txz tyz | qx qy qz per node
    const double *volumes = nullptr;          // [stride]
    double *fluxes = nullptr;                 // the stage's fluxes F (+ C) [5][stride] (flux launch only): F = F + V
    double mu = 0.0, kappa = 0.0;             // kappa = (mu * GAMMA) / ((GAMMA - 1) * prandtl), formed on the host
    ViscosityModel model;                     // the stress launch only; constant: the launch reads none of it
};

// The variable step limit (k_viscous_clamp_variable): sf = min(sf, ((cfl_v * rho) * g) / d), d from mu_i and mut_i.
struct ViscousClamp {
    const double *q = nullptr;                // the level's variables [5][stride]
    const double *g = nullptr;                // [stride] cbrt(vol)^2 / vol
    double *step_factors = nullptr;
    double mu = 0.0, cfl_v = 0.0;
    ViscosityModel model;
};

// The Spalart-Allmaras model (kernels_sa.hip: k_sa_gradient_tile, k_sa_transport_tile, k_sa_restrict; eddy mode
// MGCFD_EDDY_SPALART_ALLMARAS): pass 1 writes grad and mut from w and nt; pass 2 reads w, nt, grad and writes nt_out.
struct SaStep {
    const double *w = nullptr;                // the stage's input state W [5][stride]: what the fluxes were computed from
    const double *nt = nullptr;               // [stride] nu_tilde at the stage's input
    double *grad = nullptr;                   // sa_gradient [5][stride]: G[nt][x] G[nt][y] G[nt][z] | om | nu
    double *mut = nullptr;                    // eddy_viscosity [stride] (pass 1 and the restriction write it)
    const double *volumes = nullptr;          // [stride]
    double mu = 0.0;
    ViscosityModel model;                     // the law alone is read (viscosity_of)
    double cv1_3 = 0.0;                       // (cv1 * cv1) * cv1, formed on the host like the four below
    // pass 2
    const double *nt_old = nullptr;           // [stride] nu_tilde at the sweep's start
    double *nt_out = nullptr;                 // [stride] the stage's result (never nt itself: other tiles still stage it)
    const double *d = nullptr;                // [stride] the wall distance
    const double *g = nullptr;                // [stride] cbrt(vol)^2 / vol
    const double *step_factors = nullptr;     // [stride] the sweep's final factors
    double cw1 = 0.0, c6 = 0.0, inv_sigma = 0.0, ks = 0.0;
    double cfl_v = 0.0;
    double rk_div = 1.0;                      // double(RK+1-j)
};
// ... and pass 2 under the corrected face gradient (mgcfd_set_face_gradient): an argument type of its own, so that every kernel
// that takes SaStep keeps its arguments
struct SaStepCorrected : SaStep {
    const double *x = nullptr;                // [3][stride] the level's coordinates as given at creation
};
// ... and pass 2 with the physical-time source of nt (mgcfd_set_sa_unsteady with time_accurate, under dual time stepping):
//   a = nt - ntn;  b = ntn - ntn1;  ts = (3 a - b) / (2 dt)  (order 2)  |  a / dt  (order 1, ntn1 not read);  Q' = Q - vol * ts
//   dn = (fac * Q') / (1.0 + (fac * vol) * (jac + cj))
// Again argument types of their own: the untimed instantiations keep their arguments and their code.
struct SaTime {
    const double *ntn = nullptr, *ntn1 = nullptr;   // [stride] nu_tilde at the last physical time level and the one before it
    double dt = 0.0;                          // the physical step
    double cj = 0.0;                          // 1.5 / dt (order 2) or 1.0 / dt (order 1), formed once on the host
    int order = 1;
};
struct SaStepTimed : SaStep { SaTime t; };
struct SaStepCorrectedTimed : SaStepCorrected { SaTime t; };
// Pass 1 under delayed DES (MGCFD_SA_LENGTH_DDES): the shielded model length d~ per node, written every stage.  The DES97 length
// (k_sa_length) takes the same arguments.
struct SaShield {
    const double *d = nullptr;                // [stride] the wall distance
    const double *delta = nullptr;            // [stride] the longest internal edge at the node (+inf: none)
    double c_des = 0.0;
    double *length = nullptr;                 // [stride] d~
};
struct SaStepShielded : SaStep { SaShield sh; };

// The two launches of the corrected face gradient (kernels_face_gradient.hip: k_face_gradient_nodes_tile,
// k_face_gradient_correction_tile; mgcfd_set_face_gradient): the first writes g from w behind the stress launch, the second reads
// w, g and x and adds the correction into components 1..4 of fluxes behind the viscous-flux launch.
struct FaceGradientStep {
    const double *w = nullptr;                // the stage's input state W [5][stride]: what the fluxes were computed from
    double *g = nullptr;                      // [14][stride]: G[u][xyz] G[v] G[w] G[T] | me | kap per node
    const double *x = nullptr;                // [3][stride] the level's coordinates as given at creation
    const double *volumes = nullptr;          // [stride]
    double *fluxes = nullptr;                 // the stage's fluxes F (+ C + V) [5][stride] (correction only)
    double mu = 0.0, kappa = 0.0;             // as ViscousStep's
    ViscosityModel model;                     // the first launch only; mut is read as it stands behind the stress launch
};

// The physical-time source of dual time stepping (kernels.hip: k_time_step_src, k_dual_source; mgcfd_set_dual_time):
//   src = vol * ((3 (W - Wn) - (Wn - Wn1)) / (2 dt))   order 2 (BDF2);   src = vol * ((W - Wn) / dt)   order 1 (BDF1, Wn1 not read)
struct DualSource {
    const double *w = nullptr;                // the stage's input state W [5][stride]: what the fluxes were computed from
    const double *wn = nullptr, *wn1 = nullptr;   // the last physical time level and the one before it
    const double *volumes = nullptr;          // [stride]
    double dt = 0.0;                          // the physical step
    int order = 1;
};

// "Add up these partial sums" as an argument: k_sum_partials does only that; k_restrict can take it along.
struct SumTask {
    const double *partial = nullptr;      // [n]
    int n = 0;
    double *out = nullptr;                // the total
    double *ring = nullptr;               // nullptr, or: also append the total to the rms history
    int *count = nullptr;
    int cap = 0;
};

// One solid-wall edge (neighbour code -1) as the surface-loads kernel reads it: the edge's weights after adjust/dampen,
// the coordinates of its node and the node's index in the solver's numbering.
struct WallRecord {
    double x, y, z;                       // edge weights
    double cx, cy, cz;                    // coordinates of node b (zeros where the level has none)
    int32_t node;                         // node b, renumbered
    int32_t pad;
};

// The pressure loads of one level's solid walls (k_surface_loads): six sums Fx Fy Fz Mx My Mz over `n` records.
struct LoadsTask {
    const WallRecord *rec = nullptr;      // [n]
    int64_t n = 0;
    double p_inf = 0.0;                   // far-field pressure
    const double *ref = nullptr;          // device [3]: moment reference point
    double *partial = nullptr;            // [6][ceil(n / 256)] per-workgroup sums (stage A), reduced in place (stage B)
    unsigned *ticket = nullptr;           // arrival counter of the workgroups; the last one resets it to 0
    double *out = nullptr;                // nullptr, or: the 6 sums
    double *ring = nullptr;               // nullptr, or: the 6 sums into row (*count - 1) of this [cap][6] history
    const int *count = nullptr;
    int cap = 0;
};

// The loads of a level split over ranks: every rank stores the six terms of its own solid-wall edges at the edges' slots
// of a terms table [6][row] (row = the whole level's edge count rounded up to 256, pad lanes zero) that lives on the
// gathering rank (k_loads_terms), which then reduces the table exactly as k_surface_loads reduces its records
// (k_loads_reduce: LoadsTask with rec = nullptr, n = the whole level's count).
struct LoadsTerms {
    const WallRecord *rec = nullptr;      // [n] this rank's records, local order
    int64_t n = 0;
    double p_inf = 0.0;
    const double *ref = nullptr;          // device [3]
    const int32_t *slot = nullptr;        // [n] position in the whole level's solid-wall slice; nullptr: lane k stores at k
    double *table = nullptr;              // [6][row], on this device or on a peer's (peer access)
    int64_t row = 0;
};

// The wall nodes of a level (the distinct b ends of its solid-wall edges, ascending original id) and, per wall node, its
// internal incidences in the level's original edge order and its solid-wall edges in the order of the records
// (preprocess.hpp: WallRows).  Node ids are the solver's numbering.
struct WallNodes {
    int64_t n = 0;                        // wall nodes
    const int32_t *node = nullptr;        // [n]
    const int32_t *int_ptr = nullptr;     // [n + 1] a wall node's internal incidences ...
    const int32_t *int_nbr = nullptr;     // [entries] ... the other node ...
    const double *int_n = nullptr;        // [entries][3] ... and the normal seen from the wall node: +e at an a end, -e at a b end
    const int32_t *wall_ptr = nullptr;    // [n + 1] a wall node's solid-wall edges ...
    const int32_t *wall_edge = nullptr;   // [records] ... as indices into the level's WallRecord list, ascending
};

// The wall distance of a level (k_wall_distance; mgcfd_compute_wall_distance): every node's distance to the nearest of the m
// wall nodes and that wall node's index in the wall list, an exact all-pairs minimum in ascending list order.
struct WallDistance {
    const double *x = nullptr;            // [3][stride] the nodes' coordinates in the solver's numbering (pad lanes: finite)
    const double *wx = nullptr;           // [3][m] the wall nodes' coordinates in list order
    int32_t m = 0;
    double *d = nullptr;                  // [stride] pad lanes +inf
    int32_t *nearest = nullptr;           // [stride] index into the wall list, -1 without a wall and in pad lanes
};

// The wall spacing (k_wall_spacing): per wall node the smallest positive distance among the other ends of its internal incidences.
struct WallSpacing {
    WallNodes wn;
    const double *d = nullptr;            // [stride] the level's wall distance
    double *h = nullptr;                  // [wn.n]
};

// The wall-limited Smagorinsky length scale (k_wall_length): l2_i = min(c2 d2_i, (kappa d_i)^2) per node.
struct WallLength {
    const double *d2 = nullptr, *d = nullptr;   // [stride] each
    double c2 = 0.0, kappa = 0.0;
    double *l2 = nullptr;                 // [stride]
};

// The node stresses of the wall nodes alone (k_wall_stress): pass 1 of the viscous terms on the level's current state,
// into a compact table sw [12][n].
struct WallStress {
    WallNodes wn;
    const double *volumes = nullptr;      // [stride]
    double mu = 0.0, kappa = 0.0;
    double *sw = nullptr;                 // [12][wn.n]
    ViscosityModel model;                 // as the stress launch applies it; model.mut is read under eddy 1 and never written
};

// Pressure and friction loads in one launch (k_surface_loads_viscous): twelve sums Fp(3) Mp(3) | Fv(3) Mv(3) over the
// records of `base`; base.partial is [12][ceil(n / 256)], base.out 12 sums, base.ring rows of 12.
struct LoadsTaskViscous {
    LoadsTask base;
    const int32_t *wall_of_rec = nullptr; // [n] the wall node (index into sw's columns) of every record
    const double *sw = nullptr;           // [12][nw]; nullptr: the viscous terms are off for the level, the friction six are +0.0
    int64_t nw = 0;
};

// The per-wall-node surface distribution (k_wall_distribution): out [n][7] = ax ay az | dp | tx ty tz.
struct WallDistribution {
    WallNodes wn;
    const WallRecord *rec = nullptr;
    double p_inf = 0.0;
    const double *sw = nullptr;           // as in LoadsTaskViscous
    double *out = nullptr;
};

// Long rows (preprocess.hpp: LevelPlan::tail_*): device arrays of the entries the per-node loop leaves to the workgroup.
struct TailPlan {
    const int32_t *rows_main = nullptr;   // [n_slices] internal rows the per-node loop walks
    const int32_t *tile_ptr = nullptr;    // [n_tiles+1]
    const double2 *rec = nullptr;         // [total][3]: fx fy | fz k | (owner slot | code << 16) -
    const int32_t *begin = nullptr, *count = nullptr;   // [stride] a node's entries
    double2 *flux = nullptr;              // scratch [total][3]: the entry's five flux terms (48-byte records)
};

// Device pointers of one level's gather plan.
struct DevicePlan {
    int64_t nel = 0;
    int64_t stride = 0;                 // 256 * n_tiles
    int32_t n_slices = 0;
    int32_t *slice_row0 = nullptr, *rows_int = nullptr, *rows_bnd = nullptr, *nbr = nullptr;
    double *w = nullptr;                // [row][4 components][64 lanes]: signed, halved edge weights fx,fy,fz and k = -|e|*0.2f*0.5
    int32_t n_tiles = 0;
    int32_t pad_row = 0;                // index of a row of padding after the last row (nbr16, w)
    uint16_t *nbr16 = nullptr;          // [row][64 lanes] tile-local codes
    int32_t *tile_halo = nullptr;        // [n_tiles][kHaloStride] ids of the staged halo nodes, -1 padded
    int32_t *tile_ovf_ptr = nullptr, *tile_ovf = nullptr;
    int vin_ok = 0;                     // no tile has overflow nodes or more than 256 halo nodes: role-5 launches allowed
    int lds_complete = 0;               // every halo node of every tile is staged in LDS (no overflow table entries)
    int32_t halo_max = 0;               // the largest halo of a tile (k_flux_free: how many workgroups may share a CU)
    // half rows (preprocess.hpp: LevelPlan::hr_*), k_flux_free's plan
    int free_rows = 0;                  // the half-row plan is present
    int half = 0;                       // ... and uniform (LevelPlan::half): the level reaches k_flux_free's short-row instantiations
    int32_t hr_max_rows = 0;            // the most half rows a slice holds
    int free_wide = 0;                  // some tile's halo exceeds kHaloStride: k_flux_free stages from free_halo ([n_tiles][kFreeHaloStride])
    int32_t *free_halo = nullptr;
    int32_t hr_pad_row = 0;             // index of a half row of padding after the last one
    int32_t *hr_row0 = nullptr;         // [n_slices+1]
    uint32_t *hr_code = nullptr;        // [half row][64]
    double *hr_w = nullptr;             // [half row][3][64]
    int has_tail = 0;                   // long rows: some tile leaves entries to its workgroup (k_flux_tile<..., TAIL>)
    TailPlan tail;
    // two-phase ("fission") design point: per-edge arrays, edge-flux scratch [5][n_edges_pad], rows' edge references
    int64_t n_edges = 0, n_edges_pad = 0;
    int32_t *fe_ab = nullptr, *row_edge = nullptr;
    double *fe_w = nullptr, *edge_flux = nullptr;
    int32_t *old_of_new = nullptr;
    // transfer to/from the next-coarser level
    int32_t *child_ptr = nullptr, *child = nullptr;
    int32_t *child4 = nullptr;          // [nel_coarse][4] the first four children of every coarse node, -1 padded
    double *pro_w = nullptr;            // [row][w_own | w_other][64 lanes]
    int32_t *pro_p = nullptr;           // [row][64 lanes] coarse NEW id of the other end's parent
    int pro_tiled = 0;                  // k_prolong_tile can run (coarse residuals staged in LDS)
    int32_t *pro_tile_n = nullptr, *pro_tile_ids = nullptr;
    uint16_t *pro_s16 = nullptr, *pro_own16 = nullptr;
    int32_t *pro_parent = nullptr;
    double *pro_wsum = nullptr;
};

// The level can run the stages of kVariantStageWg4: no long rows, every tile's halo within the 80-byte records' slots (so no
// overflow table and no second halo id per thread either)
inline bool stage_wg4_fits(const DevicePlan &p) { return !p.has_tail && p.halo_max <= kTileCap4 - kTile; }

} // namespace mgcfd
