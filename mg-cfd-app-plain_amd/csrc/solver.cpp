// solver.cpp — device-resident solver behind the C ABI of include/mgcfd.h.
//
// Owns, per multigrid level, the state arrays the reference's main() owns
// (src/euler3d_cpu_double.cpp:138-162) in HBM, in the renumbered node order of the
// level's gather plan, and exposes the reference's kernel set one call per loop plus the
// V-cycle state machine (src/euler3d_cpu_double.cpp:371-694).
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <functional>
#include <future>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "device_owner.hpp"
#include "kernels.hpp"
#include "kernels_face_gradient.hpp"
#include "kernels_upwind.hpp"
#include "kernels_sa.hpp"
#include "kernels_statistics.hpp"
#include "kernels_wall_heat.hpp"
#include "mesh.hpp"
#include "mgcfd.h"
#include "preprocess.hpp"

namespace mgcfd {

static thread_local std::string g_last_error;

// A level's device arrays live in ONE block (a creation is one allocation and a destruction one free per level instead
// of 55 of each).  build_solver first lists them — which member points where, from which host array it is filled — with
// no call into the runtime (so that the listing and the repacking into device layouts can run while the device is still
// waking up), then allocates the block, sets the members and copies.
struct LevelStaging {
    struct Item { std::function<void(char *)> place; const void *src; size_t bytes; size_t offset; };
    std::vector<Item> items;
    std::vector<std::shared_ptr<void>> keep;      // arrays repacked for the device, alive until they have been copied
    size_t total = 0;
    static constexpr size_t kAlign = 4096;
    template <typename F> void alloc(F *&field, size_t bytes, const void *src = nullptr)
    {
        const size_t off = total;
        total += (std::max<size_t>(bytes, 1) + kAlign - 1) / kAlign * kAlign;
        F **where = &field;
        items.push_back({[where, off](char *base) { *where = reinterpret_cast<F *>(base + off); }, src, src ? bytes : 0, off});
    }
    template <typename F, typename T> void upload(F *&field, const std::vector<T> &v) { alloc(field, v.size() * sizeof(T), v.data()); }
    template <typename F, typename T> void upload(F *&field, std::vector<T> &&v)
    {
        auto held = std::make_shared<std::vector<T>>(std::move(v));
        keep.push_back(held);
        upload(field, *held);
    }
};

struct EventPair { Event start, stop; int level, loop; bool is_flux_internal; int launches; };

// The halo exchange of one partitioned level as the C++ host runs it (mgcfd_rank_* / mgcfd_group_*): ONE packed message
// per exchange holding every peer's segment (one pack and one unpack launch whatever the number of peers), one buffer
// set per Runge-Kutta stage (a set is reused a whole sweep later), and the level's tiles split into those next to ghost
// nodes ("boundary": they read ghosts, and every node a peer needs lies in one of them) and the rest ("interior"),
// which run while the message travels.
struct HaloExchange {
    static constexpr int kSets = 3;
    DeviceOwner mem;                                     // every device array named below (not the opened mappings)
    std::vector<int> peer;                               // neighbouring ranks, ascending
    std::vector<int64_t> send_off, recv_off;             // [n_peers+1] node offsets of the peers' segments
    int32_t *send_idx = nullptr, *recv_idx = nullptr;    // device: library node ids, all peers concatenated
    double *send_buf[kSets] = {nullptr, nullptr, nullptr}, *recv_buf[kSets] = {nullptr, nullptr, nullptr};   // device: [nodes][5]
    int32_t *tiles_boundary = nullptr, *tiles_interior = nullptr, *tiles_all = nullptr;   // (all = boundary then interior: one launch per stage)
    int32_t n_boundary = 0, n_interior = 0;
    Stream comm_stream;
    Event packed[kSets], arrived[kSets];
    Event reduced, gathered, joined;   // the in-process all-reduce of the time step; graph capture joins
    double *gmin = nullptr;                              // device [world]: [0] = the group's minimum time step (in-process groups)
    // in-process groups: every rank reads the others' minima IN PLACE (k_min_over_peers), so a rank's minimum of sweep k must not
    // be overwritten by its reduction of sweep k + 1 while a rank that is no halo neighbour — nothing on the device orders the two —
    // may still be reading it: the minima alternate between two words by sweep parity (a reader two sweeps behind cannot exist:
    // the writer's gather of sweep k + 1 waits for the reader's reduction event of sweep k + 1, which lies behind its read of sweep k)
    double *min_par = nullptr;                           // device [2]: this rank's minimum of even / odd sweeps
    int min_parity = 0;                                  // ... and which of them the NEXT sweep writes
    const double **peer_scalars[2] = {nullptr, nullptr}; // device [world] per parity: where every rank of the group keeps that minimum
    // the sweep as a captured graph per buffer rotation (one host call per sweep instead of ~25): RCCL ranks
    GraphExec sweep_graph[6];   // [rotation (+ 3 x parity of the minima: in-process groups)]
    int64_t graph_iters[6][MGCFD_NUM_LOOPS] = {{0}};
    bool graph_failed = false;
    int64_t sweeps_replayed = 0;          // ... launched from one of them so far (mgcfd_rank_graph_status)
    // in-process groups, direct mode: a rank's message is stored by ONE launch straight into its peers' ghost slots
    // (k_halo_push) — no message buffers, no second stream, no unpack; a stage's boundary tiles wait for the peers'
    // previous-stage events instead
    std::vector<int32_t> recv_idx_host;                  // recv_idx on the host (a peer builds its push targets from it)
    int32_t *push_target = nullptr;                      // device [total_send]: slot k's node in the numbering of the peer it goes to
    Event bdone[3];                                      // [stage] this rank's boundary tiles and push of that stage are enqueued up to here
    bool direct = false;
    // ranks in different PROCESSES, direct mode (mgcfd_rank_ipc_*): the peers' state buffers and flag words opened through HIP IPC
    bool ipc = false;
    unsigned long long *flags = nullptr;                 // device [kMaxIpcRanks][4]: word [r][slot] is raised by rank r (slot = stage; 3 = the time-step all-reduce)
    double *gmins = nullptr;                             // device [2][kMaxIpcRanks]: every rank's time-step minimum of this sweep (parity) / the last
    bool ipc_all = false;                                // every rank of the job is attached: the time-step all-reduce goes through the flags too
    unsigned long long sweep_seq = 0;                    // all-reduces published so far
    double *all_mins[kMaxIpcRanks] = {};                 // opened (own: gmins): rank r's gmins
    unsigned long long *all_flag[kMaxIpcRanks] = {};     // opened: rank r's flag word [this rank][3]
    unsigned *ticket = nullptr;                          // device: workgroups of the running push that are done
    int *ipc_timeouts = nullptr;                         // device: waits that gave up (a peer that never arrived)
    bool ipc_unacknowledged = false;                     // a synchronising call has found ipc_timeouts != 0 and nobody has asked mgcfd_rank_ipc_status since
    unsigned long long seq = 0;                          // messages pushed so far (all ranks push in lockstep)
    double *peer_state[kMaxPushPeers][3] = {};           // opened: peer k's three state buffers, as the peer numbers them
    int64_t peer_stride[kMaxPushPeers] = {};
    int peer_rot_delta[kMaxPushPeers] = {};              // (peer's rotation - ours) mod 3 when the buffers were exchanged
    unsigned long long *peer_flag[kMaxPushPeers] = {};   // opened: the words of peer k's flag array this rank raises
    std::vector<IpcMapping> ipc_opened;                  // every mapping opened (closed again in mgcfd_rank_ipc_detach, or with the exchange)
    int32_t *node_send_ptr = nullptr, *node_send_target = nullptr;   // device: the message per NODE (StagePush: a stage that sends it itself)
    int8_t *node_send_peer = nullptr;
    bool group_prepared() const { return min_par || peer_scalars[0] || direct; }   // the other ranks of a group hold addresses into this exchange
    int64_t total_send() const { return send_off.empty() ? 0 : send_off.back(); }
    int64_t total_recv() const { return recv_off.empty() ? 0 : recv_off.back(); }
};

// The column families of the surface loads (DESIGN.md "Adding a loads column family"): the pressure six, the friction six
// beside them, the heat rate Q and the wall area A behind the twelve.  The public calls name a kind (the partitioned form
// sums the pressure six only); everything below them takes it.
enum class LoadsKind { Pressure, Friction, Heat };
constexpr int kLoadsKinds = 3, kLoadsMaxWidth = 14;
constexpr size_t loads_width(LoadsKind kind) { constexpr size_t w[kLoadsKinds] = {6, 12, kLoadsMaxWidth}; return w[static_cast<int>(kind)]; }

// Where a loads launch stores its row: a device address, or the kind's history at the row of the cycle whose RMS was
// appended last.
struct LoadsDest {
    double *out = nullptr;               // nullptr: the history row
    static LoadsDest at(double *p) { return LoadsDest{p}; }
    static LoadsDest history() { return LoadsDest{}; }
};

// Surface loads of a level split over ranks (mgcfd_rank_set_wall_slots; INTEGRATION.md "Surface loads", the partitioned form)
struct RankLoads {
    std::vector<int64_t> slot_host;      // position of this rank's k-th solid-wall edge in the whole level's solid-wall slice
    int64_t total = 0;                   // the whole level's solid-wall edge count
    DeviceOwner mem;                     // every device array named below
    int32_t *slot = nullptr;             // device [n_wall_rec]
    Event terms;                         // this rank's terms of the evaluation under way are stored up to here
    bool checked = false;                // the host checks over all ranks have passed with these slots
    // the gathering rank (rank 0):
    int64_t row = 0;                     // total rounded up to 256
    double *table = nullptr;             // device [6][row]: every rank's terms in the whole level's order, pad lanes +0.0
    double *partial = nullptr;           // [6][row / 256]
    unsigned *ticket = nullptr;
    Event read;                          // the reduce that read the table last is enqueued up to here
    // one rank per process over RCCL: the terms travel as a message
    std::vector<int64_t> counts;         // every rank's edge count, agreed once
    double *compact = nullptr;           // this rank's terms [6][own count]; rank 0: the other ranks' messages, one after another
    std::vector<int32_t *> peer_slot;    // rank 0: device copies of the other ranks' slots
};

// The wall nodes of a level and what the viscous surface loads and the surface distribution keep on the device for them
// (mgcfd_surface_loads_viscous, mgcfd_wall_distribution; INTEGRATION.md "Viscous surface loads"): made by the first such call
// for the level, gone with the level.
struct WallPlan {
    std::vector<int64_t> original;       // the wall nodes' original ids, ascending
    DeviceOwner mem;                     // every device array named below
    WallNodes wn;
    int32_t *wall_of_rec = nullptr;      // [n_wall_rec] the wall node of every solid-wall record
    double *sw = nullptr;                // [12][wn.n] the wall nodes' stresses of the last k_wall_stress launch
    double *partial = nullptr;           // [14][ceil(n_wall_rec / 256)]: the widest kind's sums, a narrower kind uses the front
    unsigned *ticket = nullptr;
    double *dist = nullptr;              // [wn.n][MGCFD_WALL_COLUMNS] the distribution's result
    // the heat table (mgcfd_wall_heat), made by the first such call for the level
    double *heat = nullptr;              // [wn.n][MGCFD_WALL_HEAT_COLUMNS] the heat table's result
};

struct DeviceLevel {
    mgcfd_level_desc info{};             // sizes only (pointers nulled)
    std::vector<mgcfd_edge> edges;       // final edge weights, original order
    LevelPlan plan;                      // host copy (permutations for get/set)
    DevicePlan dp;
    // SoA state, stride = dp.stride: q = the reference's `variables`
    double *q = nullptr, *old_variables = nullptr, *fluxes = nullptr, *residuals = nullptr;   // [5][stride]
    double *q_alt = nullptr;             // [5][stride] second state buffer for the fused RK stages
    // The three state buffers change roles after every fused sweep (no copy<double>(old, variables)):
    // variables = state[rot], q_alt = state[rot+1], old_variables = state[rot+2] (mod 3).
    double *state[3] = {nullptr, nullptr, nullptr};
    int rot = 0;
    void apply_rot() { q = state[rot % 3]; q_alt = state[(rot + 1) % 3]; old_variables = state[(rot + 2) % 3]; }
    // The end of a fused sweep: variables = b1 (the last stage's result: stage_out, where a sweep keeps it, needs no update),
    // q_alt = b2, old_variables = start.  ahead: the last stage looked ahead (min_ahead).
    void finish_sweep(bool ahead) { rot = (rot + 1) % 3; apply_rot(); min_ahead = ahead; }
    double *tile_sumsq = nullptr;        // [n_tiles] per-tile sums of squares of the residuals, written by a last stage on request
    bool want_sumsq = false;             // the next fused sweep's last stage also fills tile_sumsq (cycle driver, level 0)
    bool have_sumsq = false;             // ... and did
    int64_t row_bytes = 0;               // bytes of the incidence rows (ids + weights)
    bool min_ahead = false;              // the launch that produced the CURRENT variables looked ahead: partial_min holds the
                                         // first half of compute_step_factor for them (global time step), or sf_alt holds
                                         // their step factors (a local time step: mesh_name = fvcorr, or mgcfd_set_time_step)
    double *sf_alt = nullptr;            // [stride] a local time step's look-ahead target; swapped with step_factors when consumed
    int sf_par = 0;                      // parity of those swaps (part of the graph keys)
    double *sfb[2] = {nullptr, nullptr};
    void apply_sf() { step_factors = sfb[sf_par & 1]; sf_alt = sfb[(sf_par & 1) ^ 1]; }
    double *smooth_buf[2] = {nullptr, nullptr};   // [5][stride] each: the residual smoothing's iterates, alternating (allocated when it is first switched on)
    double *jst_buf = nullptr;           // [7][stride]: the JST dissipation's L [5], nu and r (allocated when it is first switched on for this level)
    double *time_n = nullptr, *time_n1 = nullptr;   // [5][stride] each: dual time stepping's time levels Wn and Wn1 (held while it is on)
    const double *flux_in = nullptr;     // the state the last flux launch read: W of the dual-time source
    // the viscous terms (mgcfd_set_viscous), held while they are on for this level: the node stresses S [12][stride], the step
    // limit's g = cbrt(vol)^2 / vol [stride] and the no-slip wall's nodes (the distinct b ends of the solid-wall edges, renumbered)
    double *visc_s = nullptr, *visc_g = nullptr;
    int32_t *visc_wall = nullptr;
    int64_t n_visc_wall = 0;
    double *wall_area = nullptr;         // [n_visc_wall] while the heat-flux wall is in effect on the level (mgcfd_set_wall_temperature)
    // ... and, while a non-default viscosity model is set as well (mgcfd_set_viscosity_model): the eddy viscosity [stride] and
    // d2 = cbrt(vol) * cbrt(vol) [stride]
    double *visc_mut = nullptr, *visc_d2 = nullptr;
    int eddy_mode = 0;                   // the model's eddy mode while visc_mut is held (MGCFD_ARR_EDDY_VISCOSITY: who may write it)
    // the wall distance (mgcfd_compute_wall_distance), held until mgcfd_release_wall_distance: d [stride], the nearest wall
    // node's index in the wall list [stride] and that list's original ids on the host; the level's coordinates as given at
    // creation stay on the host (original numbering, empty where the level came without) and visit the device per computation
    std::vector<double> coords;
    double *wall_d = nullptr;
    int32_t *wall_near = nullptr;
    std::vector<int64_t> wall_ids;
    double *visc_l2 = nullptr;           // [stride] while the wall damping is in effect on the level: l2 (k_wall_length)
    // the Spalart-Allmaras model, held while it is in effect on the level: nu_tilde [stride] and, on level 0, its value at the
    // sweep's start, the spare buffer a stage's pass 2 writes (swapped with sa_nt behind it) and sa_gradient [5][stride]
    double *sa_nt = nullptr, *sa_old = nullptr, *sa_spare = nullptr, *sa_grad = nullptr;
    // the unsteady model (mgcfd_set_sa_unsteady), level 0 only: nu_tilde at the two last physical time levels [stride] each, held
    // while the model, dual time stepping and time_accurate are all in effect; the longest internal edge per node and the model
    // length d~ [stride] each, held while the model is in effect and the length is not the wall distance
    double *sa_ntn = nullptr, *sa_ntn1 = nullptr, *sa_delta = nullptr, *sa_len = nullptr;
    // the corrected face gradient (mgcfd_set_face_gradient), held while it is in effect on the level: G, me, kap [14][stride] and
    // the coordinates in the solver's numbering [3][stride]
    double *fg_g = nullptr, *fg_x = nullptr;
    // the upwind flux (mgcfd_set_upwind): Gl [15][stride] and psi [5][stride] in one allocation, made when a MUSCL level first
    // covers this level; the coordinates are fg_x, held while the corrected face gradient OR a MUSCL level is in effect here
    double *up_buf = nullptr;
    // the flow statistics (mgcfd_set_statistics), level 0 only, held while a mode is on: the means [6][stride] and the co-moments
    // [7][stride]; in mode 2 on a level with solid walls also the wall table [n_wall][8] and the distribution table [n_wall][7] its
    // samples are formed in
    double *stat_mean = nullptr, *stat_mom = nullptr, *stat_wall = nullptr, *stat_dist = nullptr;
    bool stat_made_wp = false;           // the wall plan below was first made for the wall statistics: it goes with them
    double *fas_p = nullptr, *fas_w0 = nullptr;     // [5][stride] each, levels >= 1 while FAS multigrid is on: the forcing P and the start state W0
    int32_t *new_of_old_dev = nullptr;   // [nel] level 0 while ordered_rms(): its RMS is summed in original numbering (settle_rms_order)
    double *step_factors = nullptr, *volumes = nullptr, *cbrt_vol = nullptr;                  // [stride]
    double *min_dt = nullptr;            // global-min time step scalar (after the reduction)
    double *partial_min = nullptr;       // one partial minimum per step-factor workgroup
    double *sumsq = nullptr, *partials = nullptr;
    int n_partials = 0;
    bool fluxes_zero = true;             // fluxes[] is logically zero (the flux launch need not read it)
    bool fluxes_stale = false;           // ... but its memory has not been zeroed (lazy zero after a fused time_step)
    bool residuals_stale = false;        // residuals[] = variables - old_variables of the last sweep (validation.cpp:77-89), not written
                                         // yet: a single-level run's sweeps overwrite it unread; settle_residuals writes it on demand
    bool sweep_flux0_done = false;       // mgcfd_sweep_flux0 ran since mgcfd_sweep_begin
    int stage_next = 0;                  // mgcfd_sweep_stage: the stage expected next (0 = a sweep may start)
    double *stage_out = nullptr;         // ... and the buffer the last one wrote (MGCFD_ARR_STAGE)
    int64_t n_owned = 0;                 // < nel on a partitioned level: original ids >= n_owned are ghosts
    std::vector<std::pair<int32_t *, int64_t>> halo_plans;   // device id lists of the halo messages
    std::unique_ptr<HaloExchange> hx;    // the C++-side exchange of a partitioned level (mgcfd_rank_set_halo)
    bool has_transfer = false;           // plan to the next-coarser level present
    // surface loads (mgcfd_surface_loads): one record per solid-wall edge, the per-workgroup sums, the arrival ticket
    WallRecord *wall_rec = nullptr;
    int64_t n_wall_rec = 0;
    double *loads_partial = nullptr;
    unsigned *loads_ticket = nullptr;
    std::unique_ptr<RankLoads> rl;       // a partitioned level whose ranks add their loads up
    std::unique_ptr<WallPlan> wp;        // the viscous surface loads' and the surface distribution's plan (first call)
    DeviceOwner mem;                     // the one block behind every array listed at creation (LevelStaging), the three state
                                         // buffers, and what an option or a halo plan uploaded later
    int64_t iters[MGCFD_NUM_LOOPS] = {0};
    double times[MGCFD_NUM_LOOPS] = {0};
    double flux_time = 0.0;
    int64_t flux_launches = 0;
    // MGCFD_OPT_TIMING = 4 (per-loop times by attribution): how often each loop ran on this level and how often under events
    int64_t att_sweeps = 0, att_sweeps_sampled = 0;      // smoothing sweeps (flux, compute_step, time_step, indirect_rw run together)
    int64_t att_calls[MGCFD_NUM_LOOPS] = {0}, att_calls_sampled[MGCFD_NUM_LOOPS] = {0};   // restrict (booked on the coarse level) and prolong
};

// Where a sweep's first stage (or time_step) takes the global time step's minimum from.
// None: the step factors are final (local time step, or not a first stage); Partials: the workgroups' partial minima (partial_min);
// Scalar: the reduced — on a rank: all-reduced — scalar (min_dt); List: a list of rank minima (StageArgs::min_list)
enum class ApplyMin { None, Partials, Scalar, List };
// What one fused Runge-Kutta stage does beside flux + time_step (mgcfd_solver::op_fused_stage); a caller names what it means.
struct StageArgs {
    ApplyMin apply_min = ApplyMin::None;
    const double *min_list = nullptr; int n_min = 0;        // ApplyMin::List
    bool with_residual = false;              // last stage: residuals = variables - old ...
    bool lazy_residual = false;              // ... left unwritten (settle_residuals writes it on demand)
    bool sumsq = false;                      // ... and its squares per tile into tile_sumsq
    const double *old = nullptr;             // where the sweep's start state is read from (default: old_variables)
    bool look_ahead = false;                 // the stage leaves the next sweep's step-factor work behind (partial minima in partial_min, or fvcorr's factors in sf_alt)
    const double *vin_flux = nullptr;        // the stage applies the first stage's time_step on these fluxes to its input (role 5)
    const int32_t *tile_list = nullptr; int32_t n_list = 0; // a launch over part of the level's tiles (a partitioned level)
    bool count_iters = true;                 // (a stage launched in two parts counts once)
    const StagePush *push = nullptr;         // the stage sends its own halo message
};

// The state buffers of stage j of a fused sweep: the stages run variables -> q_alt -> (the former old_variables buffer) -> q_alt
// from the sweep's start state, which stays in `variables` until finish_sweep rotates the three.
struct StageBuffers { double *start, *in, *out; };
static StageBuffers stage_buffers(const DeviceLevel &lv, int j)
{
    double *const start = lv.q, *const b1 = lv.q_alt, *const b2 = lv.old_variables;
    return {start, j == 0 ? start : (j == 1 ? b1 : b2), j == 1 ? b2 : b1};
}

} // namespace mgcfd

using namespace mgcfd;

struct mgcfd_mesh { HostMesh mesh; };

// what a solver knows about the ranks around it
struct mgcfd_comm {
    int rank = 0, world = 1;
    void *rccl = nullptr;                         // ncclComm_t (one rank per process)
    struct mgcfd_group *group = nullptr;          // or: the in-process group this solver is rank `rank` of
};
struct mgcfd_group {
    std::vector<struct mgcfd_solver *> ranks;     // (a rank destroyed before its group leaves a null entry)
    bool peer_ok = true;                          // every device of the group can address every other one's memory (direct mode stores into it)
};

struct mgcfd_solver {
    int device = 0;
    int mesh_variant = 0;
    // Members that own device resources free them after ~mgcfd_solver's body has synchronised, in reverse order of
    // declaration: the stream is declared first, so everything that ran on it goes before it does.
    Stream own_stream;
    hipStream_t stream = nullptr;
    DeviceOwner mem;                         // err, the RMS and loads rings, loads_dev
    std::vector<DeviceLevel> L;
    std::optional<mgcfd_comm> comm;          // set while the solver is a rank of something (mgcfd_rank_attach_*, mgcfd_group_create)
    FarField ff{};
    double ff17[17] = {0};
    unsigned long long *err = nullptr;       // device: packed (cell << 8 | code), ~0 = clean
    int opt_exact = 1, opt_timing = 0, opt_indirect_rw = 0, opt_check = 1, opt_variant = -1, opt_fuse = 1, opt_graph = 0, opt_stage_wg4 = 1;
    // (MGCFD_LAZY_RESIDUAL=0: every sweep's last stage writes residuals[] — for A/B measurements)
    int opt_rank_split = 1;
    bool opt_lazy_residual = !(std::getenv("MGCFD_LAZY_RESIDUAL") && std::atoi(std::getenv("MGCFD_LAZY_RESIDUAL")) == 0);
    // check_for_invalid_variables: every checked launch carries its sequence number since the host last read the
    // error word, so the EARLIEST failing time_step wins, as in the reference (kernel_device.hpp: err_key)
    int check_seq = 0;
    int64_t invalid_cell = -1; int invalid_cycle = -1;                     // where the last reported invalid state was found
    int next_check() { if (!opt_check) return 0; if (check_seq < (1 << 22)) check_seq++; return check_seq; }
    int force_check = -1;                    // >= 0: the sequence number the next fused stage carries (a stage launched in two parts)
    int timing_stride = 8;                  // OPT_TIMING == 2: bracket the flux launches of every Nth sweep; == 4: every Nth sweep / transfer of a level runs unfused under events
    double att_total = 0.0;                 // OPT_TIMING == 4: GPU seconds of the cycle batches (one event pair around each)
    bool probe_first_stage_only = false;    // (a sampled sweep of OPT_TIMING == 4 runs the indirect_rw probe behind its first stage only)
    int64_t sweep_counter = 0;
    bool in_timed_group = false;
    struct SweepGraph { GraphExec exec; int64_t iters[MGCFD_NUM_LOOPS] = {0}; bool ahead_after = false; int rot_after = 0; int sf_par_after = 0; bool sumsq_after = false, res_stale_after = false; };
    std::map<uint64_t, SweepGraph> sweep_graphs;   // captured smoothing sweeps, keyed by (level, options)
    struct CycleGraph { GraphExec exec; std::vector<std::vector<int64_t>> iters; std::vector<bool> ahead_after, res_stale_after; std::vector<int> rot_after, sf_par_after; };
    std::map<uint64_t, CycleGraph> cycle_graphs;   // captured whole multigrid cycles, keyed by options
    static constexpr int kRmsRing = 4096;
    double *rms_ring = nullptr;                    // level-0 sum of squares of the cycles run since the last read-back
    int *rms_count = nullptr;
    // surface loads: per kind a [kRmsRing][loads_width(kind)] history filled beside rms_ring (row = the cycle's RMS slot;
    // made by ensure_loads_ring, so a call of one kind never reads rows another kind wrote), the reference point and a
    // synchronous call's result on the device; the cycle appends rows of loads_kind to that kind's history while
    // loads_in_cycle is set
    double *loads_ring[kLoadsKinds] = {nullptr, nullptr, nullptr};
    double *loads_dev = nullptr;                                              // ref [3] | out [kLoadsMaxWidth]
    double loads_ref_host[3] = {0.0, 0.0, 0.0};
    bool loads_in_cycle = false;
    LoadsKind loads_kind = LoadsKind::Pressure;
    bool partitioned = false;                      // made by mgcfd_create_partitioned* (loads: the group and rank forms, over all ranks)
    double p_inf = 0.0;                            // far-field pressure, derive()'s expression on ff_variable
    double fs_mach = kDefaultMach, fs_alpha_deg = kDefaultAlphaDeg;      // what ff17 was computed from (mgcfd_set_free_stream)
    // The time step (mgcfd_set_time_step): which formula compute_step_factor runs and its CFL number.  REFERENCE is what the
    // reference's main() picks by mesh name (src/euler3d_cpu_double.cpp:388-395); every caller asks the two predicates.
    int dt_mode = MGCFD_DT_REFERENCE;
    double cfl = 0.5;                                                    // the reference's literal (cfd_loops.cpp:56,118)
    bool global_dt() const { return dt_mode == MGCFD_DT_GLOBAL || (dt_mode == MGCFD_DT_REFERENCE && mesh_variant != MGCFD_MESH_FVCORR); }   // one step for the level: a minimum to reduce
    bool legacy_dt() const { return dt_mode == MGCFD_DT_LOCAL_LEGACY || (dt_mode == MGCFD_DT_REFERENCE && mesh_variant == MGCFD_MESH_FVCORR); }   // compute_step_factor_legacy's formula
    // Implicit residual smoothing (mgcfd_set_residual_smoothing): irs_iters Jacobi iterations with coefficient irs_eps stand in
    // for every time_step; 0 = off.  While it is on a stage is one standalone flux launch + irs_iters smoothing launches: no
    // fused stage, no look-ahead, no graph (the launches leave fluxes[] to be zeroed lazily, a host-side flag).
    double irs_eps = 0.0;
    int irs_iters = 0;
    bool smoothing() const { return irs_iters > 0; }
    // Dual time stepping (mgcfd_set_dual_time): dual_dt > 0 = on.  Every stage's update takes F - src for F (the BDF source of
    // the physical step over W, Wn, Wn1) and the pseudo step is clamped to dual_clamp * dual_dt / vol.  While it is on a stage is
    // one standalone flux launch + the dual time_step (or the source launch + the smoothing launches): no fused stage, no
    // look-ahead, no graph.  dual_levels: time levels held (0: none yet, the next mgcfd_dual_time_begin_step stores one and
    // BDF1 runs; 2: both, BDF2 runs unless dual_order is 1).
    double dual_dt = 0.0, dual_clamp = 0.0;
    int dual_order = 2, dual_levels = 0, dual_invalid_step = -1;
    bool dual_time() const { return dual_dt > 0.0; }
    DualSource dual_source(const DeviceLevel &lv) const
    {
        DualSource d;
        d.w = lv.flux_in ? lv.flux_in : lv.q; d.wn = lv.time_n; d.wn1 = lv.time_n1; d.volumes = lv.volumes;
        d.dt = dual_dt; d.order = (dual_order == 2 && dual_levels == 2) ? 2 : 1;
        return d;
    }
    // JST dissipation (mgcfd_set_jst): on levels 0 .. jst_levels-1 every flux launch is followed by the sensor and the
    // dissipation launch, which add the correction C into fluxes[].  Such a level runs a stage as standalone flux launch + the
    // two + the update the other settings select: no fused stage, no look-ahead, no graph.  Other levels run as ever.
    double jst_kappa2 = 0.0, jst_kappa4 = 0.0;
    int jst_levels = 0;
    bool jst_on(int l) const { return l < jst_levels; }
    // Upwind fluxes (mgcfd_set_upwind; INTEGRATION.md "Upwind fluxes"): on levels 0 .. up_levels-1 the internal edges take Roe's
    // flux in place of the reference's — the flux launch runs the wall and far-field faces alone, then pass 2 adds U — and on
    // levels 0 .. up_muscl-1 pass 1 first forms the limited gradient pass 2 reconstructs with.  Such a level runs unfused stages
    // outside graphs, as a JST level does.
    int up_levels = 0, up_muscl = 0, up_limiter = MGCFD_LIMITER_NONE;
    double up_k = 0.0, up_fix = 0.0;
    bool upwind_on(int l) const { return l < up_levels; }
    bool muscl_on(int l) const { return l < up_muscl; }
    UpwindStep upwind_step(const DeviceLevel &lv) const
    {
        UpwindStep a;
        a.w = lv.q; a.x = lv.fg_x; a.volumes = lv.volumes; a.fluxes = lv.fluxes;
        a.gl = lv.up_buf; a.psi = lv.up_buf ? lv.up_buf + 15 * lv.dp.stride : nullptr;
        a.limiter = up_limiter; a.k3 = (up_k * up_k) * up_k; a.entropy_fix = up_fix;
        return a;
    }
    // Laminar viscous terms (mgcfd_set_viscous): on levels 0 .. visc_levels-1 every flux launch (behind the JST pair, where on)
    // is followed by the stress and the viscous-flux launch, which add V into fluxes[], the final step factors take the
    // viscous limit, and with visc_wall every launch that writes such a level's variables is followed by the no-slip launch.
    // Such a level runs unfused stages outside graphs, as a JST level does.
    double visc_mu = 0.0, visc_prandtl = 0.0, visc_cfl = 0.0;
    int visc_wall = 0, visc_levels = 0;
    bool viscous_on(int l) const { return l < visc_levels; }
    ViscousStep viscous_step(DeviceLevel &lv) const
    {
        ViscousStep a;
        a.w = lv.q; a.s = lv.visc_s; a.volumes = lv.volumes; a.fluxes = lv.fluxes;
        a.mu = visc_mu; a.kappa = (visc_mu * 1.4) / ((1.4 - 1.0) * visc_prandtl);
        a.model = viscosity_model(lv);
        return a;
    }
    // The viscosity model (mgcfd_set_viscosity_model): the law of mu(T) and the eddy viscosity, applied per node by the stress
    // launch, the wall-stress launch and the step limit on the levels the viscous terms cover.  Kept while the terms are off.
    int vm_law = MGCFD_VISCOSITY_CONSTANT, vm_eddy = MGCFD_EDDY_NONE;
    double vm_t_ref = 0.0, vm_s = MGCFD_SUTHERLAND_S, vm_cs = MGCFD_SMAGORINSKY_CS, vm_prandtl_t = MGCFD_PRANDTL_TURBULENT;
    bool variable_viscosity() const { return vm_law != MGCFD_VISCOSITY_CONSTANT || vm_eddy != MGCFD_EDDY_NONE; }
    ViscosityModel viscosity_model(const DeviceLevel &lv) const
    {
        ViscosityModel m;
        if (!variable_viscosity()) return m;
        m.law = vm_law;
        m.eddy = vm_eddy == MGCFD_EDDY_SPALART_ALLMARAS ? MGCFD_EDDY_FIELD : vm_eddy;   // (the model's kernels write mut; every consumer reads it)
        m.t_ref = vm_t_ref; m.s = vm_s; m.one_plus_s = 1.0 + vm_s;
        m.c2 = vm_cs * vm_cs; m.cp = 1.4 / (1.4 - 1.0);
        m.prandtl = visc_prandtl; m.prandtl_t = vm_prandtl_t;
        m.mut = lv.visc_mut; m.d2 = lv.visc_d2;
        if (lv.visc_l2) { m.d2 = lv.visc_l2; m.damped = 1; }       // (held exactly while the wall damping is in effect here)
        return m;
    }
    // The wall damping of the Smagorinsky model (mgcfd_set_wall_damping): kept like the viscosity model; in effect on the levels
    // the viscous terms cover while the eddy mode is Smagorinsky.
    int wd_on = 0;
    double wd_kappa = MGCFD_WALL_KAPPA;
    bool damping_in_effect() const { return wd_on && vm_eddy == MGCFD_EDDY_SMAGORINSKY && visc_levels > 0; }
    // The Spalart-Allmaras model (eddy mode MGCFD_EDDY_SPALART_ALLMARAS; INTEGRATION.md "Spalart-Allmaras model"): in effect on
    // the levels the viscous terms cover; transport on level 0, a restricted nt and a frozen mut on the others.
    double sa_ratio = MGCFD_SA_RATIO;
    bool sa_on(int l) const { return vm_eddy == MGCFD_EDDY_SPALART_ALLMARAS && viscous_on(l); }
    bool sa_in_effect() const { return vm_eddy == MGCFD_EDDY_SPALART_ALLMARAS && visc_levels > 0; }
    // The unsteady model (mgcfd_set_sa_unsteady; INTEGRATION.md "Unsteady Spalart-Allmaras"): kept like the viscosity model.
    int sa_time_accurate = 0, sa_length = MGCFD_SA_LENGTH_WALL;
    double sa_cdes = MGCFD_SA_CDES;
    bool sa_timed() const { return sa_time_accurate && dual_time() && sa_on(0); }
    bool sa_model_length() const { return sa_length != MGCFD_SA_LENGTH_WALL && sa_on(0); }
    SaShield sa_shield(const DeviceLevel &lv) const
    {
        SaShield a;
        a.d = lv.wall_d; a.delta = lv.sa_delta; a.c_des = sa_cdes; a.length = lv.sa_len;
        return a;
    }
    SaTime sa_time(const DeviceLevel &lv) const
    {
        SaTime t;
        t.ntn = lv.sa_ntn; t.ntn1 = lv.sa_ntn1; t.dt = dual_dt;
        t.order = (dual_order == 2 && dual_levels == 2) ? 2 : 1;
        t.cj = (t.order == 2 ? 1.5 : 1.0) / dual_dt;
        return t;
    }
    // pass 1 of level 0: under delayed DES the instantiation that writes d~ too
    void sa_gradient(DeviceLevel &lv)
    {
        if (lv.sa_len && sa_length == MGCFD_SA_LENGTH_DDES) { const SaShield sh = sa_shield(lv); launch_sa_gradient(stream, lv.dp, sa_step(lv), &sh); }
        else launch_sa_gradient(stream, lv.dp, sa_step(lv));
    }
    // pass 2 of level 0 with the arguments `a`: with the physical-time source where the time levels are held
    void sa_launch_transport(DeviceLevel &lv, const SaStep &a)
    {
        if (lv.sa_ntn) { const SaTime t = sa_time(lv); launch_sa_transport(stream, lv.dp, a, lv.fg_x, &t); }
        else launch_sa_transport(stream, lv.dp, a, lv.fg_x);
    }
    SaStep sa_step(const DeviceLevel &lv, int j = 0) const
    {
        const double cb1 = 0.1355, cb2 = 0.622, sigma = 2.0 / 3.0, kappa = 0.41, cv1 = 7.1;
        SaStep a;
        a.w = lv.q; a.nt = lv.sa_nt; a.grad = lv.sa_grad; a.mut = lv.visc_mut; a.volumes = lv.volumes;
        a.mu = visc_mu; a.model = viscosity_model(lv);
        a.cv1_3 = (cv1 * cv1) * cv1;
        a.nt_old = lv.sa_old; a.nt_out = lv.sa_spare; a.g = lv.visc_g; a.step_factors = lv.step_factors;
        a.d = lv.sa_len ? lv.sa_len : lv.wall_d;                     // (sa_len: the model length d~, level 0 alone)
        a.cw1 = cb1 / (kappa * kappa) + (1.0 + cb2) / sigma; a.c6 = 64.0; a.inv_sigma = 1.0 / sigma; a.ks = (1.0 + cb2) / sigma;
        a.cfl_v = visc_cfl; a.rk_div = double(MGCFD_RK + 1 - j);
        return a;
    }
    // nt at the sweep's start, beside every copy of variables into old_variables
    void sa_copy_old(int l)
    {
        if (l != 0 || !sa_on(l)) return;
        DeviceLevel &lv = level(l);
        HIP_CHECK(hipMemcpyAsync(lv.sa_old, lv.sa_nt, sizeof(double) * lv.dp.stride, hipMemcpyDeviceToDevice, stream));
    }
    // pass 2 of stage j, before the update of the five variables: into the spare buffer, which becomes nt
    void sa_transport(int l, int j)
    {
        if (l != 0 || !sa_on(l)) return;
        DeviceLevel &lv = level(l);
        sa_launch_transport(lv, sa_step(lv, j));                       // (fg_x: held exactly while the corrected face gradient is in effect here)
        std::swap(lv.sa_nt, lv.sa_spare);
    }
    // behind a restriction into level `coarse`: nt averaged over the children, mut from it and the restricted state
    void sa_restrict(int coarse)
    {
        if (!sa_on(coarse)) return;
        DeviceLevel &F = level(coarse - 1), &C = level(coarse);
        launch_sa_restrict(stream, C.info.nel, C.dp.stride, F.dp.child_ptr, F.dp.child, F.sa_nt, C.sa_nt, sa_step(C));
    }
    // nt = (ratio * mu) / rho_inf, +0.0 on the wall, and mut from it (d given); mut from nt as it stands (d == nullptr)
    void sa_form(DeviceLevel &lv, bool initialise)
    {
        launch_sa_init(stream, lv.info.nel, lv.dp.stride, (sa_ratio * visc_mu) / ff.var[0], initialise ? lv.wall_d : nullptr, lv.sa_nt, sa_step(lv));
    }
    // sf = min(sf, (k0 * rho) * g) on final step factors, before dual time stepping's clamp; under a non-default viscosity
    // model the limit from mu_i and mut_i per node
    void viscous_clamp(int l)
    {
        DeviceLevel &lv = level(l);
        if (variable_viscosity()) {
            ViscousClamp a;
            a.q = lv.q; a.g = lv.visc_g; a.step_factors = lv.step_factors;
            a.mu = visc_mu; a.cfl_v = visc_cfl; a.model = viscosity_model(lv);
            launch_viscous_clamp_variable(stream, lv.info.nel, lv.dp.stride, a);
            return;
        }
        const double kv = std::max(4.0 / 3.0, 1.4 / visc_prandtl);
        launch_viscous_clamp(stream, lv.info.nel, visc_cfl / (kv * visc_mu), lv.q, lv.visc_g, lv.step_factors);
    }
    // The face gradient of the diffusion terms (mgcfd_set_face_gradient; INTEGRATION.md "Corrected face gradients"): kept like the
    // viscosity model; in effect on the levels the viscous terms cover.  Corrected: the node-gradient launch behind the stress
    // launch and the correction launch behind the viscous-flux launch, wherever the two run.
    // The flow statistics (mgcfd_set_statistics; INTEGRATION.md "Flow statistics"): the mode, the samples taken and the sum of their
    // weights.  The accumulators are level 0's (stat_mean, stat_mom, stat_wall).
    int stat_mode = MGCFD_STATISTICS_OFF;
    int64_t stat_samples = 0;
    double stat_wsum = 0.0;
    int fg_mode = MGCFD_FACE_GRADIENT_AVERAGED;
    bool fg_on(int l) const { return fg_mode == MGCFD_FACE_GRADIENT_CORRECTED && viscous_on(l); }
    FaceGradientStep face_gradient_step(const DeviceLevel &lv) const
    {
        FaceGradientStep a;
        a.w = lv.q; a.g = lv.fg_g; a.x = lv.fg_x; a.volumes = lv.volumes; a.fluxes = lv.fluxes;
        a.mu = visc_mu; a.kappa = (visc_mu * 1.4) / ((1.4 - 1.0) * visc_prandtl);
        a.model = viscosity_model(lv);
        return a;
    }
    // Wall thermal conditions (mgcfd_set_wall_temperature; INTEGRATION.md "Wall thermal conditions"): kept like the viscosity
    // model; in effect on the levels the viscous terms cover while their wall is the no-slip one.  wt_ew = Tw / (GAMMA - 1.0).
    int wt_mode = MGCFD_WALL_ADIABATIC;
    double wt_value = 0.0, wt_ew = 0.0;
    bool wall_thermal(int mode) const { return wt_mode == mode && visc_wall && visc_levels > 0; }
    // the no-slip wall behind a launch that wrote q (and q2: FAS's copy of it); residuals where that launch wrote them; the
    // isothermal wall's launch in its place while that mode is in effect
    void viscous_wall(int l, double *q, double *q2 = nullptr, const double *old = nullptr, double *residuals = nullptr)
    {
        if (!viscous_on(l) || !visc_wall) return;
        DeviceLevel &lv = level(l);
        if (wt_mode == MGCFD_WALL_ISOTHERMAL) launch_viscous_wall_isothermal(stream, lv.n_visc_wall, lv.dp.stride, lv.visc_wall, wt_ew, q, q2, old, residuals);
        else launch_viscous_wall(stream, lv.n_visc_wall, lv.dp.stride, lv.visc_wall, q, q2, old, residuals);
    }
    // the heat-flux wall's addition into fluxes[][4], directly behind the viscous-flux launch
    void wall_heat_flux(int l)
    {
        DeviceLevel &lv = level(l);
        if (!wall_thermal(MGCFD_WALL_HEAT_FLUX) || !lv.wall_area) return;
        launch_wall_heat_flux(stream, lv.n_visc_wall, lv.dp.stride, lv.visc_wall, lv.wall_area, wt_value, lv.fluxes);
    }
    // FAS multigrid (mgcfd_set_fas): the V-cycle's transfers become the FAS legs (op_fas_restrict, op_fas_prolong) and every stage
    // of a level >= 1 takes R + P for its total residual R.  Such a level runs unfused stages (standalone flux launch + the
    // forced update): no fused stage, no look-ahead; no graph on any level.  Level 0 sweeps as ever.
    bool fas = false;
    // (a run of cycles from level cycle_top > 0, mgcfd_run_cycles_from: that level plays level 0's part and is unforced)
    bool fas_forced(int l) const { return fas && l > cycle_top; }
    // The cycle (mgcfd_set_cycle): its shape and the sweeps per level before the down leg and after the up leg.  Empty vectors
    // are the defaults — pre 1, post 1 on the levels 0 < l < n-1, 0 on level 0 — and the setter stores the defaults as empty
    // vectors, so that default_cycle() is the one question every caller asks.  A non-default cycle runs its launches directly.
    int cycle_shape = MGCFD_CYCLE_V;
    std::vector<int> cycle_pre, cycle_post;
    int cycle_top = 0;                             // the level mgcfd_run_cycles_from is cycling from, 0 otherwise
    bool default_cycle() const { return cycle_shape == MGCFD_CYCLE_V && cycle_pre.empty() && cycle_post.empty(); }
    int pre_sweeps(int l) const { return cycle_pre.empty() ? 1 : cycle_pre[static_cast<size_t>(l)]; }
    int post_sweeps(int l) const { return cycle_post.empty() ? (l == 0 ? 0 : 1) : cycle_post[static_cast<size_t>(l)]; }
    // the level-0 RMS of a cycle is summed in the order fixed on the original numbering (mgcfd.h) while any of them is on
    bool ordered_rms() const { return dual_time() || jst_on(0) || fas || viscous_on(0) || upwind_on(0); }
    // What the options above allow — every one of them that is on for a level replaces its fused flux + time_step stages by
    // standalone launches, which leave host-side flags behind (fluxes_stale) that a graph replay would not set.  The callers
    // add what is not physics: opt_fuse, the two-phase flux variant, the indirect_rw probe, timing and the level's flux flags.
    //   fused stages on level l: FAS forces the levels >= 1 only (level 0 sweeps as ever) ...
    bool options_allow_fused(int l) const { return !smoothing() && !dual_time() && !jst_on(l) && !viscous_on(l) && !fas_forced(l) && !upwind_on(l); }
    //   ... but no sweep is graphed on any level while it is on; JST and viscous levels count one by one
    bool options_allow_sweep_graph(int l) const { return options_allow_fused(l) && !fas && default_cycle(); }
    //   a whole cycle as one graph: every level's sweep must be (JST and the viscous terms run on levels 0 .. n-1: level 0 decides)
    bool options_allow_cycle_graph() const { return options_allow_sweep_graph(0) && cycle_top == 0; }
    JstStep jst_step(DeviceLevel &lv) const
    {
        JstStep a;
        a.w = lv.q; a.lap = lv.jst_buf; a.nu = lv.jst_buf + 5 * lv.dp.stride; a.r = lv.jst_buf + 6 * lv.dp.stride;
        a.fluxes = lv.fluxes; a.kappa2 = jst_kappa2; a.kappa4 = jst_kappa4;
        return a;
    }
    // ff17 -> the kernels' argument (ff) and the loads' p_inf.  Launches already captured keep the old values: drop_graphs.
    void set_far_field(const double *in17)
    {
        std::memcpy(ff17, in17, sizeof(double) * 17);
        std::memcpy(ff.var, ff17, sizeof(double) * 5);
        std::memcpy(ff.fc_mx, ff17 + 5, sizeof(double) * 3);
        std::memcpy(ff.fc_my, ff17 + 8, sizeof(double) * 3);
        std::memcpy(ff.fc_mz, ff17 + 11, sizeof(double) * 3);
        std::memcpy(ff.fc_de, ff17 + 14, sizeof(double) * 3);
        // derive() (cfd_loops.h:121-148) on the far field, as k_surface_loads evaluates it per node
        const double *f = ff17;
        const double vx = f[1] / f[0], vy = f[2] / f[0], vz = f[3] / f[0];
        const double speed_sqd = vx * vx + vy * vy + vz * vz;
        p_inf = (1.4 - 1.0) * (f[4] - 0.5 * f[0] * speed_sqd);
    }
    // Every captured launch carries the far field (and p_inf) it was captured with as kernel arguments: after a change of
    // free stream the sweep graphs, the cycle graphs and a rank's sweep graphs go, and the next run captures again.
    // Call with the stream idle.
    void drop_graphs()
    {
        sweep_graphs.clear();
        cycle_graphs.clear();
        for (DeviceLevel &lv : L)
            if (lv.hx) for (GraphExec &ge : lv.hx->sweep_graph) ge.reset();
    }
    std::vector<EventPair> pending;
    std::vector<Event> free_events;

    ~mgcfd_solver();
    void use_device() const { HIP_CHECK(hipSetDevice(device)); }
    const Launchers &k() const                                  // the kernels of this solver's numeric flavour
    {
        // (one table per flavour from the one list of kernels.hpp, every entry set by its member's name)
#define MGCFD_EXACT_ENTRY(member, launcher, params) t.member = exact::launcher;
#define MGCFD_FAST_ENTRY(member, launcher, params) t.member = fast::launcher;
        static constexpr Launchers kExact = [] { Launchers t{}; MGCFD_FLAVOURED_LAUNCHERS(MGCFD_EXACT_ENTRY) return t; }();
        static constexpr Launchers kFast = [] { Launchers t{}; MGCFD_FLAVOURED_LAUNCHERS(MGCFD_FAST_ENTRY) return t; }();
#undef MGCFD_EXACT_ENTRY
#undef MGCFD_FAST_ENTRY
        return opt_exact ? kExact : kFast;
    }
    DeviceLevel &level(int l)
    {
        if (l < 0 || l >= static_cast<int>(L.size())) throw std::invalid_argument("level out of range");
        return L[static_cast<size_t>(l)];
    }

    // ---- timing --------------------------------------------------------------------------
    Event get_event()
    {
        if (pending.size() >= 8192) fold_events();
        if (free_events.empty()) return make_event();
        Event e = std::move(free_events.back());
        free_events.pop_back();
        return e;
    }
    void fold_events()
    {
        if (pending.empty()) return;
        HIP_CHECK(hipStreamSynchronize(stream));
        for (auto &p : pending) {
            float ms = 0.f;
            HIP_CHECK(hipEventElapsedTime(&ms, p.start.get(), p.stop.get()));
            DeviceLevel &lv = L[static_cast<size_t>(p.level)];
            lv.times[p.loop] += double(ms) * 1e-3;
            if (p.is_flux_internal) { lv.flux_time += double(ms) * 1e-3; lv.flux_launches += p.launches; }
            free_events.push_back(std::move(p.start));
            free_events.push_back(std::move(p.stop));
        }
        pending.clear();
    }
    struct Timed {
        mgcfd_solver *s; EventPair p; bool on;
        // launches > 1: one pair brackets that many back-to-back launches of the flux kernel, so
        // only the first pays the dispatch latency an event pair adds (the others' dispatch
        // overlaps the predecessor) and the mean agrees with rocprofv3's kernel duration
        Timed(mgcfd_solver *s_, int level, int loop, bool flux_internal = false, int launches = 1)
            : s(s_), on(!s_->in_timed_group && (s_->opt_timing == 1 || (s_->opt_timing == 2 && flux_internal)))
        {
            if (!on) return;
            p = EventPair{s->get_event(), s->get_event(), level, loop, flux_internal, launches};
            if (launches > 1) s->in_timed_group = true;
            HIP_CHECK(hipEventRecord(p.start.get(), s->stream));
        }
        ~Timed()
        {
            if (!on) return;
            (void)hipEventRecord(p.stop.get(), s->stream);
            if (p.launches > 1) s->in_timed_group = false;
            s->pending.push_back(std::move(p));
        }
    };

    // What every mgcfd_bench_* hook measures: the mean GPU seconds of `launches` back-to-back calls of `launch` between two
    // events on the stream.  The hook checks its arguments and does its warm-up launches first, and sets the flags its
    // launches leave behind afterwards.
    template <typename F>
    double timed_launches(int launches, F &&launch)
    {
        Event a = get_event(), b = get_event();
        HIP_CHECK(hipEventRecord(a.get(), stream));
        for (int k = 0; k < launches; k++) launch();
        HIP_CHECK(hipEventRecord(b.get(), stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        float ms = 0.f;
        HIP_CHECK(hipEventElapsedTime(&ms, a.get(), b.get()));
        free_events.push_back(std::move(a));
        free_events.push_back(std::move(b));
        return launches > 0 ? double(ms) * 1e-3 / launches : 0.0;
    }

    // ---- operations ----------------------------------------------------------------------
    void op_copy_old(int l)
    {
        DeviceLevel &lv = level(l);
        settle_residuals(lv);
        HIP_CHECK(hipMemcpyAsync(lv.old_variables, lv.q, sizeof(double) * 5 * lv.dp.stride, hipMemcpyDeviceToDevice, stream));
        sa_copy_old(l);
    }
    // first half of compute_step_factor; reduce_to_scalar also folds the workgroups' partial
    // minima into the one fp64 scalar the kernel-granular API / the all-reduce hook work on
    void op_step_factor_local(int l, bool fuse_copy_old, bool reduce_to_scalar)
    {
        DeviceLevel &lv = level(l);
        lv.min_ahead = false;                       // partial_min is rewritten (same values if it was ahead)
        if (fuse_copy_old) settle_residuals(lv);
        double *old = fuse_copy_old ? lv.old_variables : nullptr;
        if (old) sa_copy_old(l);
        k().step_factor_local(stream, lv.info.nel, lv.dp.stride, lv.q, lv.cbrt_vol, cfl, lv.step_factors, lv.partial_min, old);
        if (reduce_to_scalar) launch_min_reduce(stream, lv.info.nel, lv.partial_min, lv.min_dt);
    }
    void op_step_factor_apply(int l)
    {
        DeviceLevel &lv = level(l);
        k().step_factor_apply(stream, lv.info.nel, lv.min_dt, lv.volumes, lv.step_factors);
    }
    // Write the residual of the last sweep if its last stage left it out (single-level runs: the next sweep would only
    // overwrite it).  Both operands are still in place — `variables` and the sweep's start state, which the buffer rotation
    // made old_variables — and the subtraction is the one the stage would have done, so the bits are the same.  Called by
    // everything that reads residuals[] and by everything that is about to change either operand.
    void settle_residuals(DeviceLevel &lv)
    {
        if (!lv.residuals_stale) return;
        lv.residuals_stale = false;
        k().residual(stream, lv.dp.stride, lv.old_variables, lv.q, lv.residuals);
    }
    // materialise a logically-zero flux array before anything reads its memory
    void settle_fluxes(DeviceLevel &lv)
    {
        if (!lv.fluxes_stale) return;
        HIP_CHECK(hipMemsetAsync(lv.fluxes, 0, sizeof(double) * 5 * lv.dp.stride, stream));
        lv.fluxes_stale = false;
    }
    // fused = true: also copy old_variables <- variables, and leave the "/ volume" half of the
    // global time step to the first time_step of the sweep (returns true in that case)
    bool op_step_factor(int l, bool fused = false, bool copy_old = true)
    {
        DeviceLevel &lv = level(l);
        Timed t(this, l, MGCFD_LOOP_COMPUTE_STEP);
        bool apply_pending = false;
        if (!global_dt()) {
            double *old = (fused && copy_old) ? lv.old_variables : nullptr;
            if (old) { settle_residuals(lv); sa_copy_old(l); }
            if (legacy_dt()) k().step_factor_legacy(stream, lv.info.nel, lv.dp.stride, lv.q, lv.volumes, cfl, lv.step_factors, old);
            else k().step_factor_nodal(stream, lv.info.nel, lv.dp.stride, lv.q, lv.cbrt_vol, lv.volumes, cfl, lv.step_factors, old);
        } else {
            // (dual time stepping clamps final step factors: nothing is left to the first time_step then)
            // (... nor on a FAS-forced level, whose time_step takes final factors)
            // (... nor on a viscous level, whose limit works on final factors)
            const bool finish = !fused || dual_time() || fas_forced(l) || viscous_on(l);
            op_step_factor_local(l, fused && copy_old, finish);
            if (finish) op_step_factor_apply(l);
            else apply_pending = true;
        }
        if (viscous_on(l)) viscous_clamp(l);
        if (dual_time()) clamp_step_factors(l);
        lv.iters[MGCFD_LOOP_COMPUTE_STEP] += lv.info.nel;
        return apply_pending;
    }
    // dual time stepping: sf = min(sf, (clamp * dt) / vol) on final step factors, before stage 0
    void clamp_step_factors(int l)
    {
        DeviceLevel &lv = level(l);
        launch_dual_clamp(stream, lv.info.nel, dual_clamp * dual_dt, lv.volumes, lv.step_factors);
    }
    // The parts of a level's plan that only a non-default option reaches are uploaded when an option first asks for them
    // (at creation: nothing but the 32-bit neighbour codes of levels whose indirect_rw probe runs the L1-gather form).  Called
    // at the end of creation and from mgcfd_set_option — never from a launch path, so never inside a stream capture.
    void upload_optional_plans(DeviceLevel &lv)
    {
        LevelPlan &P = lv.plan;
        const int v = opt_variant;
        auto take = [&lv](auto &vec) { auto *p = lv.mem.upload(vec); vec.clear(); vec.shrink_to_fit(); return p; };
        // the half-row plan: MGCFD_OPT_EXACT = 0 (the automatic variant takes the order-free kernel), or bit 6
        if (lv.dp.free_rows && !lv.dp.hr_code && (!opt_exact || (v >= 0 && (v & 64)))) {
            lv.dp.hr_row0 = lv.mem.upload(P.hr_row0);
            lv.dp.hr_code = take(P.hr_code);
            lv.dp.hr_w = take(P.hr_w);
            if (lv.dp.free_wide) lv.dp.free_halo = take(P.free_halo);
        }
        // the two-phase design point (bit 2)
        if (!lv.dp.fe_ab && v >= 0 && (v & 4)) {
            lv.dp.fe_ab = take(P.fe_ab);
            lv.dp.fe_w = take(P.fe_w);
            lv.dp.row_edge = take(P.row_edge);
        }
        // 32-bit neighbour codes: the L1-gather form of the indirect_rw probe (bit 3, or a level the tile form cannot run on)
        if (!lv.dp.nbr && ((v >= 0 && (v & 8)) || !lv.dp.lds_complete || lv.dp.has_tail)) lv.dp.nbr = take(P.nbr);
    }
    void upload_optional_plans()
    {
        use_device();
        for (DeviceLevel &lv : L) upload_optional_plans(lv);
    }
    // MGCFD_OPT_FLUX_VARIANT = -1 (auto): the edge-length factor is recomputed from the weights (8 of 34 bytes per entry
    // less to stream, one sqrt more per entry).  The fused stages run equally fast either way while a level's rows fit the
    // Infinity Cache (bench level: 20.15 against 20.2 us) and 13-17 % faster without the stream beyond it (1.5-2.4 M
    // nodes); the standalone flux launch gains at every size (bench level: 16.0-16.15 against 16.8-16.9 us).
    // With MGCFD_OPT_EXACT = 0 auto also takes the order-free kernel (bit 6) wherever it is the faster one: for every standalone
    // flux launch of a level that has the half-row plan (bench level 14.8 against 15.4 us, mixed-element level 16.4 against 17.5,
    // tetrahedral level 12.9 against 24.0), and for the fused stages of levels with long rows or halos beyond the shared table
    // (tetrahedral level: 45 against 78 us per sweep; on lattice-like levels the role-specialised node-gather stages stay ahead).
    int variant_for(const DeviceLevel &lv, bool fused = false) const
    {
        if (opt_variant >= 0) return opt_variant;
        // (round 4: the order-free stages are role-specialised where a level is on the kernel's fast path — halos within the
        //  smaller LDS image, at most five half rows per lane — and lead there too: bench level 47.1 against 51.1 us per sweep,
        //  the 4-level V-cycle 0.256 against 0.271 ms, profiles/r4_fast_mode.txt)
        const bool free_fast_path = !lv.dp.free_wide && lv.dp.halo_max <= kFreeCap4Halo && lv.dp.hr_max_rows <= kHalfMaxRows;
        if (!opt_exact && lv.dp.free_rows && (!fused || lv.dp.free_wide || lv.dp.has_tail || free_fast_path)) return 1 | 64;
        return 1;
    }
    // MGCFD_OPT_STAGE_WG4: the bit-identical stages of a level at four workgroups per CU (80-byte records, rows one at a time)
    // where its halos fit the records' slots AND its tiles outnumber what three per CU hold at once.  The bench level (1,175
    // tiles) then runs in 1.15 rounds instead of 1.53: stages 18.3 / 17.4 / 18.9 -> 17.1 / 16.2 / 17.8 us, sweep 53.0 -> 50.5 us;
    // a level of one round either way only pays the single-row loop (the V-cycle's 48^3 level, 432 tiles: +1.7 % per cycle).
    mutable int n_cus = 0;
    bool stage_wg4_for(const DeviceLevel &lv) const
    {
        if (!opt_exact || !opt_stage_wg4 || !stage_wg4_fits(lv.dp)) return false;
        if (n_cus == 0) {
            use_device();
            HIP_CHECK(hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, device));
        }
        return lv.dp.n_tiles > 3 * n_cus;
    }
    // classes: bit0 internal, bit1 solid wall (-1), bit2 far field (-2)
    void op_flux(int l, int classes)
    {
        DeviceLevel &lv = level(l);
        Timed t(this, l, MGCFD_LOOP_FLUX, (classes & 1) != 0);
        // a partial launch leaves other nodes' memory as it is; on an upwind level pass 2 adds into memory whatever the classes
        if (classes != 7 || upwind_on(l)) settle_fluxes(lv);
        const int accumulate = lv.fluxes_zero ? 0 : 1;     // 0.0 + x: same bits either way
        const int variant = variant_for(lv);
        if ((variant & 4) && !lv.dp.edge_flux)              // two-phase design point: edge-flux scratch on first use
            lv.dp.edge_flux = lv.mem.alloc<double>(static_cast<size_t>(lv.dp.n_edges_pad) * 5 + 8);
        if (upwind_on(l)) {
            // upwind level: B from the wall and far-field faces alone, then F = B + U (pass 1 on a MUSCL level, pass 2)
            if (classes & 6) k().flux(stream, lv.dp, lv.q, ff, lv.fluxes, classes & 6, accumulate, variant, nullptr, nullptr);
            if (classes & 1) {
                const UpwindStep a = upwind_step(lv);
                if (muscl_on(l)) launch_upwind_gradient(stream, lv.dp, a);
                launch_upwind_flux(stream, lv.dp, a, muscl_on(l));
            }
        } else {
            k().flux(stream, lv.dp, lv.q, ff, lv.fluxes, classes, accumulate, variant, nullptr, nullptr);
        }
        if ((classes & 1) && jst_on(l)) {
            // JST: L, nu, r of the state the fluxes were computed from, then fluxes += C (both passes keep row order in either flavour)
            const JstStep a = jst_step(lv);
            k().jst_sensor(stream, lv.dp, a);
            k().jst_dissipation(stream, lv.dp, a);
        }
        if ((classes & 1) && viscous_on(l)) {
            // the Spalart-Allmaras model's pass 1 first: the stress launch reads the mut it writes
            if (l == 0 && sa_on(l)) sa_gradient(lv);
            // viscous terms: S of the same state, then fluxes[1..4] += V, behind C (both passes keep row order in either flavour)
            const ViscousStep a = viscous_step(lv);
            k().viscous_stress(stream, lv.dp, a);
            // the corrected face gradient: G, me, kap of the same state directly behind the stress launch (mut as it left it) ...
            if (fg_on(l)) launch_face_gradient_nodes(stream, lv.dp, face_gradient_step(lv));
            k().viscous_flux(stream, lv.dp, a);
            // ... and fluxes[1..4] += Vc, Wk, Hc directly behind F = F + V
            if (fg_on(l)) launch_face_gradient_correction(stream, lv.dp, face_gradient_step(lv));
            wall_heat_flux(l);
        }
        if (dual_time()) lv.flux_in = lv.q;
        lv.fluxes_zero = false;
        lv.fluxes_stale = false;
        if (classes & 1) lv.iters[MGCFD_LOOP_FLUX] += lv.info.n_internal;
    }
    // One whole Runge-Kutta stage in one launch: fluxes of all edge classes from `in`, then
    // time_step into `out` (in != out).  fluxes[] stays logically zero, as after time_step.
    void op_fused_stage(int l, int j, const double *in, double *out, const StageArgs &a = StageArgs{})
    {
        DeviceLevel &lv = level(l);
        const FusedStep fs = fused_step(l, j, out, a);
        Timed t(this, l, MGCFD_LOOP_FLUX, true);
        // (kVariantStageWg4 is never set with MGCFD_OPT_EXACT = 0: stage_wg4_for)
        k().flux(stream, lv.dp, in, ff, lv.fluxes, 7, 0, variant_for(lv, true) | (stage_wg4_for(lv) ? kVariantStageWg4 : 0), &fs, a.push);
        if (a.count_iters) {
            lv.iters[MGCFD_LOOP_FLUX] += lv.info.n_internal;
            lv.iters[MGCFD_LOOP_TIME_STEP] += lv.info.nel;
        }
    }
    // the kernel's arguments of one fused stage (what op_fused_stage launches; tools/exp/sweep_flow.patch takes three of them for one launch)
    FusedStep fused_step(int l, int j, double *out, const StageArgs &a)
    {
        DeviceLevel &lv = level(l);
        settle_residuals(lv);                       // (a sweep that supersedes the residual has dropped the flag: smooth_once)
        FusedStep fs;
        fs.tile_list = a.tile_list;
        fs.n_list = a.n_list;
        // the C++ partitioned sweeps (tile lists): ghosts numbered last are left to the halo messages
        if (a.tile_list && lv.plan.ghosts_last && lv.n_owned < lv.info.nel) fs.nel_active = lv.n_owned;
        fs.rk_div = double(MGCFD_RK + 1 - j);
        fs.step_factors = lv.step_factors;
        fs.old_variables = a.old ? a.old : lv.old_variables;
        fs.q_out = out;
        fs.next_partial_min = (a.look_ahead && global_dt()) ? lv.partial_min : nullptr;
        fs.next_legacy_sf = (a.look_ahead && !global_dt()) ? lv.sf_alt : nullptr;
        fs.next_nodal = legacy_dt() ? 0 : 1;
        fs.cfl = cfl;
        fs.cbrt_vol = lv.cbrt_vol;
        if (out == lv.q) lv.min_ahead = false;      // (a caller that looks ahead sets it after its last stage)
        fs.partial_min = a.apply_min == ApplyMin::Partials ? lv.partial_min : (a.apply_min == ApplyMin::Scalar ? lv.min_dt : (a.apply_min == ApplyMin::List ? a.min_list : nullptr));
        fs.n_partial = a.apply_min == ApplyMin::Scalar ? 1 : (a.apply_min == ApplyMin::List ? a.n_min : static_cast<int>((lv.info.nel + 255) / 256));
        fs.volumes = lv.volumes;
        fs.residuals = (a.with_residual && !a.lazy_residual) ? lv.residuals : nullptr;
        fs.sumsq_partial = (a.with_residual && a.sumsq) ? lv.tile_sumsq : nullptr;
        fs.vin_flux = a.vin_flux;                   // role 5: the input is the first stage's time_step of (old, vin_flux)
        fs.vin_div = double(MGCFD_RK + 1);
        fs.old_of_new = lv.dp.old_of_new;
        fs.err = err;
        if (a.vin_flux) fs.check_vin = next_check();     // the absorbed first stage's check_for_invalid_variables comes first
        fs.check = force_check >= 0 ? force_check : next_check();
        return fs;
    }
    void op_indirect_rw(int l)
    {
        DeviceLevel &lv = level(l);
        settle_fluxes(lv);
        Timed t(this, l, MGCFD_LOOP_INDIRECT_RW);
        k().indirect_rw(stream, lv.dp, lv.q, lv.fluxes, variant_for(lv));
        lv.fluxes_zero = false;
        lv.iters[MGCFD_LOOP_INDIRECT_RW] += lv.info.n_internal;
    }
    void op_zero_fluxes(int l)
    {
        DeviceLevel &lv = level(l);
        HIP_CHECK(hipMemsetAsync(lv.fluxes, 0, sizeof(double) * 5 * lv.dp.stride, stream));
        lv.fluxes_zero = true;
        lv.fluxes_stale = false;
    }
    // old / out: default old_variables / variables (in place, as the reference); a sweep that keeps its
    // start state in `variables` passes both
    void op_time_step(int l, int j, ApplyMin apply_min = ApplyMin::None, bool with_residual = false, bool lazy_zero = false,
                      const double *old = nullptr, double *out = nullptr)
    {
        if (j < 0 || j >= MGCFD_RK) throw std::invalid_argument("RK stage out of range");
        DeviceLevel &lv = level(l);
        settle_fluxes(lv);
        settle_residuals(lv);
        if (!old) old = lv.old_variables;
        if (!out) out = lv.q;
        if (out == lv.q) lv.min_ahead = false;
        double *const res = with_residual ? lv.residuals : nullptr;
        sa_transport(l, j);                          // (reads the stage's input W, which an in-place update overwrites)
        bool stale = true;                          // fluxes[] is not written unless k_time_step zeroes it: logically zero, as after a lazy time_step
        Timed t(this, l, MGCFD_LOOP_TIME_STEP);
        if (smoothing()) {
            // the smoothing works on final step factors: finish compute_step_factor first (the same division k_time_step would do)
            // (booked where k_time_step's own division is booked: under time_step)
            if (apply_min == ApplyMin::Partials) launch_min_reduce(stream, lv.info.nel, lv.partial_min, lv.min_dt);
            if (apply_min != ApplyMin::None) op_step_factor_apply(l);
            // dual time stepping: F' = F - src into fluxes[] first, in a node-wise launch of its own — the first iteration forms
            // D = sf * F' for halo nodes too, which would read three more states per staged node inside k_smooth_tile
            if (dual_time()) k().dual_source(stream, lv.info.nel, lv.dp.stride, lv.fluxes, dual_source(lv));
            // FAS: the forcing is the last addition, F' = (F - src) + P, node-wise as the source
            if (fas_forced(l)) launch_fas_add_forcing(stream, lv.dp.stride, lv.fluxes, lv.fas_p);
            SmoothStep a;
            a.fluxes = lv.fluxes; a.step_factors = lv.step_factors; a.eps = irs_eps;
            for (int m = 0; m < irs_iters; m++) {
                a.prev = m == 0 ? nullptr : lv.smooth_buf[(m - 1) & 1];
                a.next = m == irs_iters - 1 ? nullptr : lv.smooth_buf[m & 1];
                if (!a.next) {
                    a.rk_div = double(MGCFD_RK + 1 - j); a.old_variables = old; a.q_out = out;
                    a.residuals = res;
                    a.old_of_new = lv.dp.old_of_new; a.err = err; a.check = next_check();
                }
                k().smooth(stream, lv.dp, a);       // (never zeroes fluxes[]: with one iteration other tiles still read them)
            }
        } else if (fas_forced(l) || dual_time()) {
            // the update with F - src, F + P or (F - src) + P for F, in the one launch; the step factors are final and, under
            // dual time, clamped (op_step_factor)
            if (apply_min != ApplyMin::None)
                throw std::invalid_argument(fas_forced(l) ? "FAS multigrid: the step factors must be final before time_step"
                                                          : "dual time: the step factors must be final before time_step");
            DualSource d;
            if (dual_time()) d = dual_source(lv); else d.order = 0;
            k().time_step_src(stream, lv.info.nel, lv.dp.stride, j, lv.step_factors, lv.fluxes, fas_forced(l) ? lv.fas_p : nullptr, old, out,
                              lv.dp.old_of_new, err, next_check(), res, d);
        } else {
            const double *pm = apply_min == ApplyMin::Partials ? lv.partial_min : (apply_min == ApplyMin::Scalar ? lv.min_dt : nullptr);
            const int n_pm = apply_min == ApplyMin::Scalar ? 1 : static_cast<int>((lv.info.nel + 255) / 256);
            const int check = next_check();
            k().time_step(stream, lv.info.nel, lv.dp.stride, j, lv.step_factors, lv.fluxes, old, out, lv.dp.old_of_new, err, check, pm, n_pm, lv.volumes, res, lazy_zero ? 0 : 1);
            stale = lazy_zero;
        }
        viscous_wall(l, out, nullptr, old, res);
        lv.fluxes_stale = stale;
        lv.fluxes_zero = true;
        lv.iters[MGCFD_LOOP_TIME_STEP] += lv.info.nel;
    }
    void op_residual(int l)
    {
        DeviceLevel &lv = level(l);
        lv.residuals_stale = false;
        k().residual(stream, lv.dp.stride, lv.old_variables, lv.q, lv.residuals);
    }
    void op_sumsq(int l)
    {
        DeviceLevel &lv = level(l);
        settle_residuals(lv);
        k().sumsq(stream, lv.info.nel, lv.dp.stride, lv.residuals, lv.partials, lv.n_partials, lv.sumsq, lv.dp.old_of_new, lv.n_owned);
    }
    // ... of level 0 in the order the options of ordered_rms() fix on the original numbering (mgcfd.h): per-workgroup sums of 256
    // original nodes into tile_sumsq (no fused stage fills it while one of them is on), then their sum, appended to `ring` if given
    // (level > 0: the RMS of mgcfd_run_cycles_from, which uploads that level's numbering on first use)
    void op_sumsq_ordered(double *ring = nullptr, int *count = nullptr, int cap = 0, int l = 0)
    {
        DeviceLevel &l0 = level(l);
        if (!l0.new_of_old_dev) throw std::logic_error("the ordered RMS sum without the level's numbering on the device");
        settle_residuals(l0);
        launch_sumsq_original(stream, l0.info.nel, l0.dp.stride, l0.residuals, l0.new_of_old_dev, l0.tile_sumsq);
        launch_sum_partials_append(stream, static_cast<int>((l0.info.nel + 255) / 256), l0.tile_sumsq, l0.sumsq, ring, count, cap);
    }
    // rms (may be null): per-tile sums of squares of the fine level that the launch adds up on the side (cycle_once)
    void op_restrict(int fine, const SumTask *rms = nullptr)
    {
        DeviceLevel &F = level(fine);
        DeviceLevel &C = level(fine + 1);
        if (!F.has_transfer) throw std::invalid_argument("level has no multigrid map");
        settle_residuals(C);
        // Timer / iteration attribution quirk: the reference bumps `level` before the call,
        // so restriction is booked to the COARSE level.
        // the coarse sweep that follows starts with compute_step_factor on the restricted state: the
        // kernel leaves its first half (per-workgroup minima) in partial_min (global time step only)
        // (not on a partitioned level: its ghosts are stale until the halo exchange that follows)
        // (nor onto a viscous level: its sweeps are unfused and the no-slip launch below changes the state)
        const bool ahead = global_dt() && C.n_owned == C.info.nel && !viscous_on(fine + 1);
        double *pm = ahead ? C.partial_min : nullptr;
        Timed t(this, fine + 1, MGCFD_LOOP_RESTRICT);
        const SumTask task = rms ? *rms : SumTask{};
        k().restrict_(stream, C.info.nel, C.dp.stride, F.dp.stride, F.dp.child_ptr, F.dp.child, F.dp.child4, F.q, C.q, C.cbrt_vol, cfl, pm, task);
        viscous_wall(fine + 1, C.q);
        sa_restrict(fine + 1);
        C.min_ahead = ahead;
        C.iters[MGCFD_LOOP_RESTRICT] += 2 * F.info.mgc + C.info.nel;   // mg_loops.cpp:61,117,172
    }
    void op_prolong(int fine)
    {
        DeviceLevel &F = level(fine);
        DeviceLevel &C = level(fine + 1);
        if (!F.has_transfer) throw std::invalid_argument("level has no multigrid map");
        settle_residuals(C);
        settle_residuals(F);
        const bool ahead = global_dt() && F.n_owned == F.info.nel && !viscous_on(fine);   // as in op_restrict
        double *pm = ahead ? F.partial_min : nullptr;
        Timed t(this, fine, MGCFD_LOOP_PROLONG);
        k().prolong(stream, F.dp, C.dp.stride, C.residuals, F.residuals, F.q, F.cbrt_vol, cfl, pm);
        viscous_wall(fine, F.q);
        F.min_ahead = ahead;
        F.iters[MGCFD_LOOP_PROLONG] += F.info.n_internal + F.info.nel;  // mg_loops.cpp:728,842
    }
    // ---- FAS multigrid: the two legs of the cycle (mgcfd.h) ----
    // R_l(variables[l]) into fluxes[l], from zero fluxes: the fluxes of all three classes (+ C on a JST level: op_flux), then
    // - src while dual time is on.  Serves step 1 and step 4 of the down leg; counted and timed as flux launches.
    void op_total_residual(int l)
    {
        DeviceLevel &lv = level(l);
        if (!lv.fluxes_zero) throw std::invalid_argument("FAS multigrid: the total residual needs zero fluxes (as after time_step)");
        op_flux(l, 7);
        if (dual_time()) {
            Timed t(this, l, MGCFD_LOOP_FLUX);
            k().dual_source(stream, lv.info.nel, lv.dp.stride, lv.fluxes, dual_source(lv));
        }
    }
    // down-leg steps 1-4: T = R (+ P) of the fine level; the state restricted as mg_restrict does it, W0 its copy, Q the
    // children's summed T, in one launch; then P = Q - R(W0) on the coarse level.  Both levels' fluxes are logically zero after.
    void op_fas_restrict(int fine)
    {
        if (!fas) throw std::invalid_argument("FAS multigrid is off: switch it on first (mgcfd_set_fas)");
        DeviceLevel &F = level(fine);
        DeviceLevel &C = level(fine + 1);
        if (!F.has_transfer) throw std::invalid_argument("level has no multigrid map");
        if (!C.fluxes_zero) throw std::invalid_argument("FAS multigrid: the coarse level needs zero fluxes (as after time_step)");
        op_total_residual(fine);
        settle_residuals(C);
        {
            Timed t(this, fine + 1, MGCFD_LOOP_RESTRICT);       // (booked on the coarse level, as op_restrict)
            k().restrict_fas(stream, C.info.nel, C.dp.stride, F.dp.stride, F.dp.child_ptr, F.dp.child, F.dp.child4, F.q, F.fluxes,
                             fas_forced(fine) ? F.fas_p : nullptr, C.q, C.fas_w0, C.fas_p);
            viscous_wall(fine + 1, C.q, C.fas_w0);
            sa_restrict(fine + 1);
        }
        F.fluxes_zero = true; F.fluxes_stale = true;            // (T is used up)
        C.min_ahead = false;
        C.iters[MGCFD_LOOP_RESTRICT] += 2 * F.info.mgc + C.info.nel;
        op_total_residual(fine + 1);                            // R(W0): variables[fine + 1] is W0 now
        {
            Timed t(this, fine + 1, MGCFD_LOOP_FLUX);
            launch_fas_forcing(stream, C.info.nel, C.dp.stride, F.dp.child_ptr, C.fluxes, C.fas_p);
        }
        C.fluxes_zero = true; C.fluxes_stale = true;
    }
    // up-leg steps 1-2: variables[fine] += 0.0 - wavg(W0 - variables[fine + 1]); no residuals array is touched
    void op_fas_prolong(int fine)
    {
        if (!fas) throw std::invalid_argument("FAS multigrid is off: switch it on first (mgcfd_set_fas)");
        DeviceLevel &F = level(fine);
        DeviceLevel &C = level(fine + 1);
        if (!F.has_transfer) throw std::invalid_argument("level has no multigrid map");
        settle_residuals(F);                                    // (an unwritten residual's operand is about to change)
        // (the look-ahead only where the sweep that follows takes it: level 0's fused stages under a global time step)
        const bool ahead = global_dt() && !fas_forced(fine) && !viscous_on(fine) && F.n_owned == F.info.nel;
        double *pm = ahead ? F.partial_min : nullptr;
        Timed t(this, fine, MGCFD_LOOP_PROLONG);
        k().prolong_fas(stream, F.dp, C.dp.stride, C.fas_w0, C.q, F.q, F.cbrt_vol, cfl, pm);
        viscous_wall(fine, F.q);
        F.min_ahead = ahead;
        F.iters[MGCFD_LOOP_PROLONG] += F.info.n_internal + F.info.nel;
    }
    // mgcfd_prolong_state: variables[fine] = 0.0 - (0.0 - wavg(variables[fine + 1])).  Neither level's residuals are touched and
    // the fine state is only written, so the look-ahead minima are those of the state the launch writes, where the sweep that
    // follows takes them (as op_fas_prolong).
    void op_prolong_state(int fine)
    {
        DeviceLevel &F = level(fine);
        DeviceLevel &C = level(fine + 1);
        if (!F.has_transfer) throw std::invalid_argument("level has no multigrid map");
        if (partitioned || comm) throw std::invalid_argument("mgcfd_prolong_state: not on a partitioned solver or a rank (split levels are out of scope)");
        settle_residuals(F);                                    // (an unwritten residual's operand is about to change)
        const bool ahead = global_dt() && !fas_forced(fine) && !viscous_on(fine) && F.n_owned == F.info.nel;
        double *pm = ahead ? F.partial_min : nullptr;
        Timed t(this, fine, MGCFD_LOOP_PROLONG);
        k().prolong_state(stream, F.dp, C.dp.stride, C.q, F.q, F.cbrt_vol, cfl, pm);
        viscous_wall(fine, F.q);
        F.min_ahead = ahead;
        F.iters[MGCFD_LOOP_PROLONG] += F.info.n_internal + F.info.nel;
    }
    // Synchronises.  seq (may be null): the sequence number of the checked launch that found it.
    int read_error(int64_t *bad_cell, int *seq = nullptr)
    {
        unsigned long long h = 0;
        HIP_CHECK(hipMemcpyAsync(&h, err, sizeof(h), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        check_seq = 0;                              // (nothing is in flight: later launches count from 1 again)
        if (h == ~0ULL) return MGCFD_OK;
        invalid_cell = static_cast<int64_t>((h >> 8) & 0xFFFFFFFFULL);
        invalid_cycle = -1;
        if (bad_cell) *bad_cell = invalid_cell;
        if (seq) *seq = static_cast<int>(h >> 40);
        HIP_CHECK(hipMemsetAsync(err, 0xFF, sizeof(unsigned long long), stream));
        switch (h & 0xFF) {
            case 1: return MGCFD_ERR_NAN;
            case 2: return MGCFD_ERR_NEG_DENSITY;
            default: return MGCFD_ERR_NEG_ENERGY;
        }
    }
};

// Ranks in different processes, direct stores (mgcfd_rank_ipc_*): a wait for a neighbour's message that gave up (k_flags_wait,
// about two seconds) let the stages behind it run on stale ghosts.  Every call that synchronises looks at the counter and
// FAILS while it is not zero; mgcfd_rank_ipc_status reads it and thereby acknowledges.  Call with the stream idle.
static void fail_on_ipc_timeouts(mgcfd_solver *s)
{
    for (DeviceLevel &lv : s->L) {
        if (!lv.hx || !lv.hx->ipc || !lv.hx->ipc_timeouts) continue;
        int n = 0;
        HIP_CHECK(hipMemcpy(&n, lv.hx->ipc_timeouts, sizeof(int), hipMemcpyDeviceToHost));
        if (n != 0) {
            lv.hx->ipc_unacknowledged = true;
            throw HipError(std::to_string(n) + " wait(s) for a neighbouring rank's message gave up: the state of this rank was computed from stale ghosts "
                           "(mgcfd_rank_ipc_status acknowledges; mgcfd_rank_ipc_detach returns to the buffered exchange)");
        }
    }
}

// (does not call into RCCL: a communicator goes with mgcfd_rank_detach)
mgcfd_solver::~mgcfd_solver()
{
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    for (DeviceLevel &lv : L) if (lv.hx) (void)hipStreamSynchronize(lv.hx->comm_stream.get());
    if (comm && comm->group) comm->group->ranks[static_cast<size_t>(comm->rank)] = nullptr;
}

// ------------------------------------------------------------------------------------------
// construction
// ------------------------------------------------------------------------------------------
// mgcfd_device_warm_up: the runtime's and the device context's start-up on a thread of its own (once per process)
static std::mutex g_warm_mutex;
static std::shared_future<void> g_warm;
static bool warm_up_under_way()
{
    std::shared_future<void> f;
    { std::lock_guard<std::mutex> lk(g_warm_mutex); f = g_warm; }
    return f.valid() && f.wait_for(std::chrono::seconds(0)) != std::future_status::ready;
}
static void wait_for_warm_up()
{
    std::shared_future<void> f;
    { std::lock_guard<std::mutex> lk(g_warm_mutex); f = g_warm; }
    if (f.valid()) f.wait();
}

static std::unique_ptr<mgcfd_solver> build_solver(const mgcfd_level_desc *levels, int nlevels, int mesh_variant, int device,
                                                  const int64_t *n_owned = nullptr, const int64_t *const *order_keys = nullptr)
{
    if (!levels || nlevels <= 0) throw std::invalid_argument("no levels given");
    if (mesh_variant != MGCFD_MESH_FVCORR && mesh_variant != MGCFD_MESH_M6_WING &&
        mesh_variant != MGCFD_MESH_LA_CASCADE && mesh_variant != MGCFD_MESH_ROTOR_37)
        throw std::invalid_argument("unknown mesh variant");
    // The device is looked at before any host work, unless a warm-up of it is still under way on its own thread
    // (mgcfd_device_warm_up): then the gather plans, which need no device, are built beside it and the device's turn
    // comes before the uploads.
    auto device_ready = [&]() {
        wait_for_warm_up();
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
            throw HipError("no HIP device available: libmgcfd_hip.so has no CPU fallback");
        if (device < 0 || device >= ndev) throw std::invalid_argument("device index out of range");
    };
    const bool device_later = warm_up_under_way();
    if (!device_later) device_ready();

    auto s = std::make_unique<mgcfd_solver>();
    s->device = device;
    s->mesh_variant = mesh_variant;
    {
        double ff17[17];
        far_field_constants(ff17);
        s->set_far_field(ff17);
    }
    s->partitioned = n_owned != nullptr;

    s->L.resize(static_cast<size_t>(nlevels));
    const bool timing = std::getenv("MGCFD_PLAN_TIMING") != nullptr;      // where the host time of a solver's creation goes (stderr)
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!timing) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[mgcfd create] %-34s %7.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    PlanOptions popt;
    if (const char *o = std::getenv("MGCFD_ORDERING")) popt.ordering = std::atoi(o);   // diagnostic override
    if (const char *o = std::getenv("MGCFD_TILE_ORDER")) popt.tile_order = std::atoi(o);   // (A/B: 0 as clustered, 1 costliest first, 2 default)
    if (const char *o = std::getenv("MGCFD_TILE_CURVE")) popt.tile_curve = std::atoi(o);   // (A/B: 0 as clustered, 1 Morton — default —, 2 Hilbert)
    // host-side plans first (coarse permutations are needed by the fine level's transfer plan).  The levels' plans are
    // independent of each other: one host thread per level (level 0 of the M6-like hierarchy takes 1 s, all four 2.2 s in a row).
    auto run_per_level = [&](int count, auto &&body) {
        std::vector<std::exception_ptr> errors(static_cast<size_t>(std::max(count, 0)));
        std::vector<std::thread> workers;
        auto guarded_body = [&](int l) { try { body(l); } catch (...) { errors[static_cast<size_t>(l)] = std::current_exception(); } };
        for (int l = 1; l < count; l++) workers.emplace_back(guarded_body, l);
        if (count > 0) guarded_body(0);
        for (std::thread &w : workers) w.join();
        for (const std::exception_ptr &e : errors) if (e) std::rethrow_exception(e);      // (the lowest level's error first)
    };
    run_per_level(nlevels, [&](int l) {
        PlanOptions popt_l = popt;                           // (a thread's own copy: n_owned differs per level)
        PlanOptions &popt = popt_l;
        const mgcfd_level_desc &d = levels[l];
        DeviceLevel &lv = s->L[static_cast<size_t>(l)];
        if (!d.volumes || !d.edges) throw std::invalid_argument("level is missing volumes/edges");
        if (d.internal_start < 0 || d.internal_start + d.n_internal > d.n_edges || d.boundary_start < 0 ||
            d.boundary_start + d.n_boundary > d.n_edges || d.wall_start < 0 || d.wall_start + d.n_wall > d.n_edges)
            throw std::invalid_argument("edge class ranges exceed n_edges");
        lv.edges.assign(d.edges, d.edges + d.n_edges);
        adjust_and_dampen(d, mesh_variant, lv.edges);
        lv.n_owned = d.nel;
        popt.n_owned = -1;
        if (n_owned && n_owned[l] >= 0 && n_owned[l] < d.nel) {
            lv.n_owned = n_owned[l];
            popt.n_owned = n_owned[l];
        }
        popt.long_rows = !std::getenv("MGCFD_NO_LONG_ROWS");      // (diagnostic: per-node rows only, overflow entries gathered in the loop)
        build_level_plan(d, lv.edges, popt, lv.plan);
        if (std::getenv("MGCFD_VERBOSE"))
            std::fprintf(stderr, "[mgcfd] level %d: %ld nodes, %d tiles, halo mean %.0f max %d (cap %d), overflow refs %ld, ELL padding %.1f%%\n",
                         l, (long)d.nel, lv.plan.n_tiles, lv.plan.halo_mean, lv.plan.halo_max, kTileCap - kTile,
                         (long)lv.plan.halo_overflow_refs, 100.0 * lv.plan.pad_fraction);
        if (std::getenv("MGCFD_VERBOSE"))
            std::fprintf(stderr, "[mgcfd] level %d: half rows %s: %ld evaluations (%.2f per node), %ld in another node's lane, %ld padding slots (%.1f%%)\n", l, lv.plan.half ? "yes" : "no",
                         (long)lv.plan.hr_entries, double(lv.plan.hr_entries) / double(d.nel), (long)lv.plan.hr_foreign, (long)lv.plan.hr_padding,
                         lv.plan.hr_entries ? 100.0 * double(lv.plan.hr_padding) / double(lv.plan.hr_entries) : 0.0);
        if (std::getenv("MGCFD_VERBOSE")) {
            // how many staged halo nodes belong to a tile of ANOTHER XCD's range (their state cannot meet its owner's in an L2)
            const int64_t nt = lv.plan.n_tiles, q8 = nt >> 3, r8 = nt & 7;
            auto xcd_of = [&](int64_t t) { return t < r8 * (q8 + 1) ? t / (q8 + 1) : r8 + (t - r8 * (q8 + 1)) / std::max<int64_t>(q8, 1); };
            int64_t total = 0, foreign = 0, near_ = 0;
            for (int64_t t = 0; t < nt; t++)
                for (int32_t k = lv.plan.tile_halo_ptr[static_cast<size_t>(t)]; k < lv.plan.tile_halo_ptr[static_cast<size_t>(t) + 1]; k++) {
                    const int64_t o = lv.plan.tile_halo[static_cast<size_t>(k)] / kTile;
                    total++;
                    if (xcd_of(o) != xcd_of(t)) foreign++;
                    else if (std::llabs(o - t) <= 48) near_++;
                }
            std::fprintf(stderr, "[mgcfd] level %d: staged halo nodes %ld: %.1f%% owned by a tile of another XCD's range, %.1f%% by a tile within 48 of the reader in its own range\n",
                         l, (long)total, total ? 100.0 * foreign / total : 0.0, total ? 100.0 * near_ / total : 0.0);
        }
        if (std::getenv("MGCFD_VERBOSE") && lv.plan.has_tail) {
            int64_t rows_full = 0, rows_cut = 0;
            for (size_t q = 0; q < lv.plan.rows_int.size(); q++) { rows_full += lv.plan.rows_int[q]; rows_cut += lv.plan.rows_main[q]; }
            std::fprintf(stderr, "[mgcfd] level %d: long rows: %ld entries left to the workgroups (%.1f per tile), per-node loop %.1f -> %.1f rows per slice\n",
                         l, (long)lv.plan.tail_total, double(lv.plan.tail_total) / lv.plan.n_tiles,
                         double(rows_full) / double(lv.plan.rows_int.size()), double(rows_cut) / double(lv.plan.rows_int.size()));
        }
    });
    lap("level plans (a thread per level)");
    // (a transfer plan writes its own fine level's plan and only READS the coarse level's permutation)
    run_per_level(nlevels - 1, [&](int l) {
        const mgcfd_level_desc &d = levels[l];
        if (!d.mg_map) throw std::invalid_argument("multigrid map missing between levels");
        build_transfer_plan(d, s->L[static_cast<size_t>(l)].edges, levels[l + 1].coords, levels[l + 1].nel,
                            s->L[static_cast<size_t>(l) + 1].plan.new_of_old, s->L[static_cast<size_t>(l)].plan,
                            order_keys ? order_keys[l] : nullptr, s->L[static_cast<size_t>(l)].n_owned);
        s->L[static_cast<size_t>(l)].has_transfer = true;
    });
    lap("transfer plans");
    // What the device gets, level by level, listed and repacked with no call into the runtime (LevelStaging): a host thread
    // per level.  What only a non-default option reaches — the order-free kernel's half-row plan, the
    // two-phase arrays, the 32-bit neighbour codes — stays on the host until an option asks for it (upload_optional_plans):
    // 60 % of the bytes.
    std::vector<LevelStaging> staging(static_cast<size_t>(nlevels));
    run_per_level(nlevels, [&](int l) {
        LevelStaging &st = staging[static_cast<size_t>(l)];
        const mgcfd_level_desc &d = levels[l];
        DeviceLevel &lv = s->L[static_cast<size_t>(l)];
        lv.info = d;
        lv.info.volumes = nullptr; lv.info.coords = nullptr; lv.info.edges = nullptr; lv.info.mg_map = nullptr;
        const int64_t nel = d.nel;
        if (d.coords) lv.coords.assign(d.coords, d.coords + 3 * nel);       // (the wall distance's, should it be asked for)
        const LevelPlan &P = lv.plan;
        const int64_t stride = int64_t(P.n_slices) * kSlice;
        std::vector<double> vol(static_cast<size_t>(stride), 1.0), cb(static_cast<size_t>(stride), 1.0);
        for (int64_t n = 0; n < nel; n++) {
            const double v = d.volumes[P.old_of_new[static_cast<size_t>(n)]];
            vol[static_cast<size_t>(n)] = v;
            cb[static_cast<size_t>(n)] = std::cbrt(v);        // cfd_loops.cpp:116, static => host libm once
            // a ghost never holds the minimum of compute_step_factor (its owner counts it): a launch that looks ahead
            // sees a ghost at the sweep's START state, which must not enter the next sweep's minimum
            if (P.old_of_new[static_cast<size_t>(n)] >= lv.n_owned) cb[static_cast<size_t>(n)] = std::numeric_limits<double>::infinity();
        }
        st.upload(lv.volumes, std::move(vol));
        st.upload(lv.cbrt_vol, std::move(cb));
        st.alloc(lv.fluxes, sizeof(double) * (static_cast<size_t>(stride) * 5));
        st.alloc(lv.residuals, sizeof(double) * (static_cast<size_t>(stride) * 5));
        st.alloc(lv.step_factors, sizeof(double) * (static_cast<size_t>(stride)));
        st.alloc(lv.sf_alt, sizeof(double) * (static_cast<size_t>(stride)));
        st.alloc(lv.min_dt, sizeof(double) * (1));
        // (+inf: a tile that is never launched — the ghost-only tiles of a partitioned level — holds no minimum)
        st.upload(lv.partial_min, std::vector<double>(static_cast<size_t>((nel + 255) / 256), std::numeric_limits<double>::infinity()));
        st.alloc(lv.tile_sumsq, sizeof(double) * (static_cast<size_t>((nel + 255) / 256)));
        st.alloc(lv.sumsq, sizeof(double) * (1));
        lv.n_partials = static_cast<int>(std::min<int64_t>(1024, (nel * 5 + 255) / 256));
        st.alloc(lv.partials, sizeof(double) * (static_cast<size_t>(lv.n_partials)));
        lv.dp.nel = nel;
        lv.dp.stride = stride;
        lv.dp.n_slices = P.n_slices;
        st.upload(lv.dp.slice_row0, P.slice_row0);
        st.upload(lv.dp.rows_int, P.rows_int);
        st.upload(lv.dp.rows_bnd, P.rows_bnd);
        {
            // edge weights as [row][component][lane] so each component load of a wave is one
            // contiguous 512-byte run
            std::vector<double> ws(P.w.size() * 4 + 2 * 4 * kSlice, 0.0);   // + two rows of padding (k_flux_tile's prologue)
            for (size_t e = 0; e < P.w.size(); e++) {
                const size_t row = e / kSlice, lane = e % kSlice;
                ws[(row * 4 + 0) * kSlice + lane] = P.w[e].x;
                ws[(row * 4 + 1) * kSlice + lane] = P.w[e].y;
                ws[(row * 4 + 2) * kSlice + lane] = P.w[e].z;
                ws[(row * 4 + 3) * kSlice + lane] = P.w[e].k;
            }
            st.upload(lv.dp.w, std::move(ws));
        }
        st.upload(lv.dp.old_of_new, P.old_of_new);
        lv.dp.n_tiles = P.n_tiles;
        lv.plan.nbr16.resize(P.nbr16.size() + 2 * kSlice, static_cast<uint16_t>(kT16Pad));   // two rows of padding
        st.upload(lv.dp.nbr16, P.nbr16);
        {
            std::vector<int32_t> fixed(static_cast<size_t>(P.n_tiles) * kHaloStride, -1);
            for (int32_t t = 0; t < P.n_tiles; t++)
                std::copy(P.tile_halo.begin() + P.tile_halo_ptr[static_cast<size_t>(t)],
                          P.tile_halo.begin() + P.tile_halo_ptr[static_cast<size_t>(t) + 1],
                          fixed.begin() + static_cast<size_t>(t) * kHaloStride);
            st.upload(lv.dp.tile_halo, std::move(fixed));
        }
        st.upload(lv.dp.tile_ovf_ptr, P.tile_ovf_ptr);
        st.upload(lv.dp.tile_ovf, P.tile_ovf);
        lv.row_bytes = int64_t(P.slice_row0.back()) * kSlice * 34;
        lv.dp.pad_row = P.slice_row0.back();
        lv.dp.n_edges = d.n_internal;
        lv.dp.n_edges_pad = (d.n_internal + 255) / 256 * 256;
        lv.plan.row_edge.resize(P.row_edge.size() + 2 * kSlice, -1);                     // two rows of padding
        lv.dp.has_tail = P.has_tail ? 1 : 0;
        if (lv.dp.has_tail) {
            st.upload(lv.dp.tail.rows_main, P.rows_main);
            st.upload(lv.dp.tail.tile_ptr, P.tail_tile_ptr);
            st.upload(lv.dp.tail.rec, P.tail_rec);
            lv.plan.tail_begin.resize(static_cast<size_t>(lv.dp.stride), 0);         // (threads past nel read these too)
            lv.plan.tail_count.resize(static_cast<size_t>(lv.dp.stride), 0);
            st.upload(lv.dp.tail.begin, P.tail_begin);
            st.upload(lv.dp.tail.count, P.tail_count);
            st.alloc(lv.dp.tail.flux, sizeof(double) * static_cast<size_t>(6 * P.tail_total));
        }
        lv.dp.vin_ok = (P.halo_overflow_refs == 0 && P.halo_max <= kTile) ? 1 : 0;
        lv.dp.lds_complete = P.halo_overflow_refs == 0 ? 1 : 0;
        lv.dp.halo_max = P.halo_max;
        lv.dp.half = (P.half && !std::getenv("MGCFD_NO_HALF_ROWS")) ? 1 : 0;
        lv.dp.free_rows = (P.free_rows && !std::getenv("MGCFD_NO_HALF_ROWS")) ? 1 : 0;
        lv.dp.hr_max_rows = P.hr_max_rows;
        lv.dp.free_wide = (lv.dp.free_rows && P.free_wide) ? 1 : 0;
        if (!lv.dp.free_wide) { lv.plan.free_halo.clear(); lv.plan.free_halo.shrink_to_fit(); }
        if (lv.dp.free_rows) {
            lv.dp.hr_pad_row = P.hr_row0.back();
            lv.plan.hr_code.resize(P.hr_code.size() + 2 * kSlice, kHalfPad);      // two half rows of padding
            lv.plan.hr_w.resize(P.hr_w.size() + 2 * 3 * kSlice, 0.0);
        } else {
            lv.plan.hr_code.clear(); lv.plan.hr_code.shrink_to_fit();
            lv.plan.hr_w.clear(); lv.plan.hr_w.shrink_to_fit();
        }
        if (lv.has_transfer) {
            st.upload(lv.dp.child_ptr, P.child_ptr);
            st.upload(lv.dp.child, P.child);
            {
                const size_t nc = P.child_ptr.size() - 1;
                std::vector<int32_t> c4(nc * 4, -1);
                for (size_t c = 0; c < nc; c++)
                    for (int32_t k = P.child_ptr[c]; k < P.child_ptr[c + 1] && k < P.child_ptr[c] + 4; k++)
                        c4[c * 4 + static_cast<size_t>(k - P.child_ptr[c])] = P.child[static_cast<size_t>(k)];
                st.upload(lv.dp.child4, std::move(c4));
            }
            {
                // prolongation entries as [row][component][lane]: every load of a wave is one contiguous run
                const size_t rows_n = P.pro.size() / kSlice;
                std::vector<double> pw((rows_n + 4) * 2 * kSlice, 0.0);      // + four rows of padding (k_prolong_tile reads ahead)
                std::vector<int32_t> pp(rows_n * kSlice);
                for (size_t e = 0; e < P.pro.size(); e++) {
                    const size_t row = e / kSlice, lane = e % kSlice;
                    pw[(row * 2 + 0) * kSlice + lane] = P.pro[e].w_own;
                    pw[(row * 2 + 1) * kSlice + lane] = P.pro[e].w_other;
                    pp[row * kSlice + lane] = P.pro[e].p_other;
                }
                st.upload(lv.dp.pro_w, std::move(pw));
                st.upload(lv.dp.pro_p, std::move(pp));
            }
            lv.dp.pro_tiled = P.pro_tiled ? 1 : 0;
            if (P.pro_tiled) {
                st.upload(lv.dp.pro_tile_n, P.pro_tile_n);
                st.upload(lv.dp.pro_tile_ids, P.pro_tile_ids);
                lv.plan.pro_s16.resize(P.pro_s16.size() + 4 * kSlice, 0);          // four rows of padding
                st.upload(lv.dp.pro_s16, P.pro_s16);
                st.upload(lv.dp.pro_own16, P.pro_own16);
            }
            st.upload(lv.dp.pro_parent, P.pro_parent);
            st.upload(lv.dp.pro_wsum, P.pro_wsum);
            // the per-entry host copies are not needed again
            lv.plan.pro.clear(); lv.plan.pro.shrink_to_fit();
        }
        lv.plan.w.clear(); lv.plan.w.shrink_to_fit();
        // the solid-wall edges (neighbour code -1) as compact records for the surface loads; no host copy is kept
        lv.n_wall_rec = d.n_boundary;
        if (d.n_boundary > 0) {
            std::vector<WallRecord> rec(static_cast<size_t>(d.n_boundary));
            for (int64_t k = 0; k < d.n_boundary; k++) {
                const mgcfd_edge &e = lv.edges[static_cast<size_t>(d.boundary_start + k)];
                if (e.b < 0 || e.b >= nel) throw std::invalid_argument("solid-wall edge with a node out of range");
                WallRecord &r = rec[static_cast<size_t>(k)];
                r.x = e.x; r.y = e.y; r.z = e.z;
                r.cx = d.coords ? d.coords[e.b * 3 + 0] : 0.0;
                r.cy = d.coords ? d.coords[e.b * 3 + 1] : 0.0;
                r.cz = d.coords ? d.coords[e.b * 3 + 2] : 0.0;
                r.node = P.new_of_old[static_cast<size_t>(e.b)];
                r.pad = 0;
            }
            st.upload(lv.wall_rec, std::move(rec));
            st.alloc(lv.loads_partial, sizeof(double) * 6 * static_cast<size_t>((d.n_boundary + 255) / 256));
            st.upload(lv.loads_ticket, std::vector<unsigned>(1, 0u));
        }
    });
    lap("device layouts repacked (a thread per level)");
    if (device_later) device_ready();
    s->use_device();
    s->own_stream = make_stream();
    s->stream = s->own_stream.get();
    s->err = s->mem.alloc<unsigned long long>(1);
    HIP_CHECK(hipMemset(s->err, 0xFF, sizeof(unsigned long long)));
    lap("device (behind its warm-up), stream");
    // the copies out of pageable memory are host work too: a thread per level again, every thread selects the device
    // for itself; the state's initialisation goes to the one stream
    run_per_level(nlevels, [&](int l) {
        s->use_device();
        DeviceLevel &lv = s->L[static_cast<size_t>(l)];
        LevelStaging &st = staging[static_cast<size_t>(l)];
        const int64_t stride = lv.dp.stride;
        char *const block = static_cast<char *>(lv.mem.alloc_bytes(st.total));
        for (const LevelStaging::Item &it : st.items) {
            it.place(block);
            if (it.bytes) HIP_CHECK(hipMemcpy(block + it.offset, it.src, it.bytes, hipMemcpyHostToDevice));
        }
        st = LevelStaging();
        // (the three state buffers keep allocations of their own: a partitioned level exports them to its peers'
        // processes, and an inter-process handle names a whole allocation)
        lv.q = lv.mem.alloc<double>(static_cast<size_t>(stride) * kNumStateFields);
        lv.q_alt = lv.mem.alloc<double>(static_cast<size_t>(stride) * 5);
        lv.old_variables = lv.mem.alloc<double>(static_cast<size_t>(stride) * 5);
        lv.state[0] = lv.q; lv.state[1] = lv.q_alt; lv.state[2] = lv.old_variables;
        lv.sfb[0] = lv.step_factors; lv.sfb[1] = lv.sf_alt;
        lv.plan.nbr16.clear(); lv.plan.nbr16.shrink_to_fit();
        s->upload_optional_plans(lv);
        // initial state: far field everywhere, fluxes/residuals/old/step factors zero
        HIP_CHECK(hipMemsetAsync(lv.old_variables, 0, sizeof(double) * 5 * stride, s->stream));
        HIP_CHECK(hipMemsetAsync(lv.fluxes, 0, sizeof(double) * 5 * stride, s->stream));
        HIP_CHECK(hipMemsetAsync(lv.residuals, 0, sizeof(double) * 5 * stride, s->stream));
        HIP_CHECK(hipMemsetAsync(lv.step_factors, 0, sizeof(double) * stride, s->stream));
        HIP_CHECK(hipMemsetAsync(lv.sf_alt, 0, sizeof(double) * stride, s->stream));
        launch_init_variables(s->stream, stride, s->ff, lv.q);
        launch_init_variables(s->stream, stride, s->ff, lv.q_alt);     // valid numbers in the padded tail
    });
    s->use_device();
    HIP_CHECK(hipStreamSynchronize(s->stream));
    HIP_CHECK(hipGetLastError());
    lap("one block per level, copies (a thread per level)");
    return s;
}

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
template <typename F> static int guarded(F &&f)
{
    try {
        f();
        return MGCFD_OK;
    } catch (const HipError &e) {
        g_last_error = e.what();
        return MGCFD_ERR_HIP;
    } catch (const std::invalid_argument &e) {
        g_last_error = e.what();
        return MGCFD_ERR_ARG;
    } catch (const std::exception &e) {
        g_last_error = e.what();
        return MGCFD_ERR_IO;
    }
}

#define REQUIRE(p) do { if (!(p)) { g_last_error = "null argument: " #p; return MGCFD_ERR_ARG; } } while (0)

extern "C" {

const char *mgcfd_last_error(void) { return g_last_error.c_str(); }
int mgcfd_abi_version(void) { return 1; }
int mgcfd_live_device_resources(int64_t out[3])
{
    REQUIRE(out);
    out[0] = g_live.allocations; out[1] = g_live.bytes; out[2] = g_live.handles;
    return MGCFD_OK;
}
int mgcfd_device_warm_up(int device)
{
    std::lock_guard<std::mutex> lk(g_warm_mutex);
    if (!g_warm.valid())
        g_warm = std::async(std::launch::async, [device] { if (hipSetDevice(device) == hipSuccess) (void)hipFree(nullptr); }).share();
    return MGCFD_OK;
}

// ---- file boundary ----
int mgcfd_mesh_load(const char *input_dat, const char *directory, int duplicate, mgcfd_mesh **out)
{
    REQUIRE(input_dat); REQUIRE(out);
    return guarded([&] {
        auto m = std::make_unique<mgcfd_mesh>();
        m->mesh = load_mesh(input_dat, directory ? directory : "", duplicate);
        *out = m.release();
    });
}
int mgcfd_mesh_load_ex(const char *input_dat, const char *directory, int duplicate, int flags, mgcfd_mesh **out)
{
    REQUIRE(input_dat); REQUIRE(out);
    return guarded([&] {
        auto m = std::make_unique<mgcfd_mesh>();
        m->mesh = load_mesh(input_dat, directory ? directory : "", duplicate, (flags & MGCFD_MESH_LEGACY_ORDERING) != 0);
        *out = m.release();
    });
}
void mgcfd_mesh_free(mgcfd_mesh *m) { delete m; }
int mgcfd_mesh_num_levels(const mgcfd_mesh *m) { return m ? static_cast<int>(m->mesh.levels.size()) : 0; }
int mgcfd_mesh_variant(const mgcfd_mesh *m) { return m ? m->mesh.mesh_variant : -1; }
int mgcfd_mesh_size(const mgcfd_mesh *m) { return m ? m->mesh.size : 0; }
int mgcfd_mesh_level(const mgcfd_mesh *m, int level, mgcfd_level_desc *out)
{
    REQUIRE(m); REQUIRE(out);
    if (level < 0 || level >= static_cast<int>(m->mesh.levels.size())) { g_last_error = "level out of range"; return MGCFD_ERR_ARG; }
    *out = m->mesh.levels[static_cast<size_t>(level)].desc();
    return MGCFD_OK;
}
int mgcfd_write_array(const char *path, const double *data, int64_t nel, int ncols)
{
    REQUIRE(path); REQUIRE(data);
    return guarded([&] { write_array(path, data, nel, ncols); });
}
int mgcfd_identify_differences(const double *t, const double *m, int64_t nel, int mesh_variant, int64_t *first_bad)
{
    REQUIRE(t); REQUIRE(m);
    const int64_t k = identify_differences(t, m, nel, mesh_variant);
    if (first_bad) *first_bad = k;
    if (k >= 0) { g_last_error = "Unacceptable error detected at flat index " + std::to_string(k); return MGCFD_ERR_VALIDATION; }
    return MGCFD_OK;
}

// Host only: the gather plans mgcfd_create[_partitioned[_mg]] would build for these levels, audited (preprocess.cpp:
// audit_level_plan).  No device is touched.
int mgcfd_plan_audit(const mgcfd_level_desc *levels, int nlevels, int mesh_variant, const int64_t *n_owned,
                     const int64_t *const *order_keys, char *report, int64_t report_cap)
{
    REQUIRE(levels);
    std::string rep;
    const int rc = guarded([&] {
        if (nlevels <= 0) throw std::invalid_argument("no levels given");
        std::vector<LevelPlan> plans(static_cast<size_t>(nlevels));
        std::vector<std::vector<mgcfd_edge>> edges(static_cast<size_t>(nlevels));
        for (int l = 0; l < nlevels; l++) {
            const mgcfd_level_desc &d = levels[l];
            if (!d.volumes || !d.edges) throw std::invalid_argument("level is missing volumes/edges");
            edges[static_cast<size_t>(l)].assign(d.edges, d.edges + d.n_edges);
            adjust_and_dampen(d, mesh_variant, edges[static_cast<size_t>(l)]);
            PlanOptions popt;
            if (const char *o = std::getenv("MGCFD_TILE_ORDER")) popt.tile_order = std::atoi(o);
            if (const char *o = std::getenv("MGCFD_TILE_CURVE")) popt.tile_curve = std::atoi(o);
            if (n_owned && n_owned[l] >= 0 && n_owned[l] < d.nel) popt.n_owned = n_owned[l];
            build_level_plan(d, edges[static_cast<size_t>(l)], popt, plans[static_cast<size_t>(l)]);
        }
        for (int l = 0; l + 1 < nlevels; l++) {
            if (!levels[l].mg_map) throw std::invalid_argument("multigrid map missing between levels");
            build_transfer_plan(levels[l], edges[static_cast<size_t>(l)], levels[l + 1].coords, levels[l + 1].nel,
                                plans[static_cast<size_t>(l) + 1].new_of_old, plans[static_cast<size_t>(l)],
                                order_keys ? order_keys[l] : nullptr, (n_owned && n_owned[l] >= 0) ? n_owned[l] : -1);
        }
        for (int l = 0; l < nlevels; l++) {
            const std::string r = audit_level_plan(levels[l], plans[static_cast<size_t>(l)], l + 1 < nlevels ? levels[l + 1].nel : -1);
            if (!r.empty()) rep += "level " + std::to_string(l) + ":\n" + r;
            if (std::getenv("MGCFD_PLAN_DIGEST")) {          // (diagnostic: the report then always holds text)
                char buf[64];
                std::snprintf(buf, sizeof(buf), "digest level %d: %016llx\n", l, (unsigned long long)plan_digest(plans[static_cast<size_t>(l)]));
                rep += buf;
            }
        }
    });
    if (rc != MGCFD_OK) return rc;
    if (report && report_cap > 0) { std::snprintf(report, static_cast<size_t>(report_cap), "%s", rep.c_str()); }
    if (!rep.empty()) { g_last_error = "plan audit: " + rep; return MGCFD_ERR_ARG; }
    return MGCFD_OK;
}

// ---- life cycle ----
int mgcfd_create(const mgcfd_level_desc *levels, int nlevels, int mesh_variant, int device, mgcfd_solver **out)
{
    REQUIRE(out);
    return guarded([&] { *out = build_solver(levels, nlevels, mesh_variant, device).release(); });
}
int mgcfd_create_partitioned(const mgcfd_level_desc *levels, int nlevels, int mesh_variant, int device,
                             const int64_t *n_owned, mgcfd_solver **out)
{
    REQUIRE(out); REQUIRE(n_owned);
    return guarded([&] { *out = build_solver(levels, nlevels, mesh_variant, device, n_owned).release(); });
}
int mgcfd_create_partitioned_mg(const mgcfd_level_desc *levels, int nlevels, int mesh_variant, int device,
                                const int64_t *n_owned, const int64_t *const *order_keys, mgcfd_solver **out)
{
    REQUIRE(out); REQUIRE(n_owned);
    return guarded([&] { *out = build_solver(levels, nlevels, mesh_variant, device, n_owned, order_keys).release(); });
}
int mgcfd_create_from_mesh(const mgcfd_mesh *m, int device, mgcfd_solver **out)
{
    REQUIRE(m); REQUIRE(out);
    return guarded([&] {
        std::vector<mgcfd_level_desc> d;
        for (auto &l : m->mesh.levels) d.push_back(l.desc());
        *out = build_solver(d.data(), static_cast<int>(d.size()), m->mesh.mesh_variant, device).release();
    });
}
void mgcfd_destroy(mgcfd_solver *s) { delete s; }

int mgcfd_set_option(mgcfd_solver *s, int option, int value)
{
    REQUIRE(s);
    return guarded([&] {
        switch (option) {
            case MGCFD_OPT_EXACT: s->opt_exact = value != 0; s->upload_optional_plans(); break;
            case MGCFD_OPT_TIMING:
                if (value < 0 || value > 4) throw std::invalid_argument("MGCFD_OPT_TIMING is 0 ... 4");
                s->use_device(); s->fold_events(); s->opt_timing = value == 3 ? 2 : value; s->timing_stride = value == 3 ? 1 : (value == 4 ? 32 : 8);
                if (const char *e = std::getenv("MGCFD_TIMING_STRIDE")) if (std::atoi(e) > 0 && value != 3) s->timing_stride = std::atoi(e);
                break;
            case MGCFD_OPT_INDIRECT_RW: s->opt_indirect_rw = value != 0; break;
            case MGCFD_OPT_CHECK_INVALID: s->opt_check = value != 0; break;
            case MGCFD_OPT_FLUX_VARIANT:
                // (the layouts of bits 1, 4 and 5 are gone: refused by name, never run as another kernel; the option keeps its value)
                if (value >= 0 && (value & 2)) throw std::invalid_argument("MGCFD_OPT_FLUX_VARIANT bit 1 (2): the edge-once layout was removed");
                if (value >= 0 && (value & 16)) throw std::invalid_argument("MGCFD_OPT_FLUX_VARIANT bit 4 (16): the indexed-weights layout was removed");
                if (value >= 0 && (value & 32)) throw std::invalid_argument("MGCFD_OPT_FLUX_VARIANT bit 5 (32): the ordered half-row layout was removed");
                s->opt_variant = value; s->upload_optional_plans(); break;
            case MGCFD_OPT_FUSE_UPDATE: s->opt_fuse = value != 0; break;
            case MGCFD_OPT_GRAPH: s->opt_graph = value != 0; break;
            case MGCFD_OPT_RANK_SPLIT: s->opt_rank_split = value < 0 ? 0 : (value > 2 ? 2 : value); break;
            case MGCFD_OPT_STAGE_WG4: s->opt_stage_wg4 = value != 0; break;
            default: throw std::invalid_argument("unknown option");
        }
    });
}
int mgcfd_level_has_half_rows(const mgcfd_solver *s, int level, int *yes)
{
    REQUIRE(s); REQUIRE(yes);
    if (level < 0 || level >= static_cast<int>(s->L.size())) { g_last_error = "level out of range"; return MGCFD_ERR_ARG; }
    *yes = s->L[static_cast<size_t>(level)].dp.half;
    return MGCFD_OK;
}
int mgcfd_level_has_order_free(const mgcfd_solver *s, int level, int *yes)
{
    REQUIRE(s); REQUIRE(yes);
    if (level < 0 || level >= static_cast<int>(s->L.size())) { g_last_error = "level out of range"; return MGCFD_ERR_ARG; }
    *yes = s->L[static_cast<size_t>(level)].dp.free_rows;
    return MGCFD_OK;
}
int mgcfd_level_stage_wg4(const mgcfd_solver *s, int level, int *yes)
{
    REQUIRE(s); REQUIRE(yes);
    if (level < 0 || level >= static_cast<int>(s->L.size())) { g_last_error = "level out of range"; return MGCFD_ERR_ARG; }
    *yes = s->stage_wg4_for(s->L[static_cast<size_t>(level)]) ? 1 : 0;
    return MGCFD_OK;
}
int mgcfd_level_tiling(const mgcfd_solver *s, int level, int64_t out[10])
{
    REQUIRE(s); REQUIRE(out);
    if (level < 0 || level >= static_cast<int>(s->L.size())) { g_last_error = "level out of range"; return MGCFD_ERR_ARG; }
    const LevelPlan &P = s->L[static_cast<size_t>(level)].plan;
    out[0] = P.n_tiles;
    out[1] = P.halo_total;
    out[2] = P.halo_max;
    out[3] = kTileCap - kTile;
    out[4] = P.halo_overflow_refs;
    out[5] = P.n_internal_entries;
    out[6] = P.pad_entries;
    out[7] = P.ordered_by_boxes ? 1 : 0;
    out[8] = P.has_tail ? P.tail_total : 0;
    out[9] = 0;
    for (int32_t r : P.rows_main) out[9] += r;
    return MGCFD_OK;
}
int mgcfd_get_option(const mgcfd_solver *s, int option, int *value)
{
    REQUIRE(s); REQUIRE(value);
    switch (option) {
        case MGCFD_OPT_EXACT: *value = s->opt_exact; break;
        case MGCFD_OPT_TIMING: *value = s->opt_timing; break;
        case MGCFD_OPT_INDIRECT_RW: *value = s->opt_indirect_rw; break;
        case MGCFD_OPT_CHECK_INVALID: *value = s->opt_check; break;
        case MGCFD_OPT_FLUX_VARIANT: *value = s->opt_variant; break;
        case MGCFD_OPT_FUSE_UPDATE: *value = s->opt_fuse; break;
        case MGCFD_OPT_GRAPH: *value = s->opt_graph; break;
        case MGCFD_OPT_RANK_SPLIT: *value = s->opt_rank_split; break;
        case MGCFD_OPT_STAGE_WG4: *value = s->opt_stage_wg4; break;
        default: g_last_error = "unknown option"; return MGCFD_ERR_ARG;
    }
    return MGCFD_OK;
}
int mgcfd_set_stream(mgcfd_solver *s, void *hip_stream)
{
    REQUIRE(s);
    return guarded([&] {
        s->use_device();
        s->fold_events();
        HIP_CHECK(hipStreamSynchronize(s->stream));
        s->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->own_stream.get();
    });
}
int mgcfd_synchronize(mgcfd_solver *s)
{
    REQUIRE(s);
    return guarded([&] { s->use_device(); HIP_CHECK(hipStreamSynchronize(s->stream)); HIP_CHECK(hipGetLastError()); fail_on_ipc_timeouts(s); });
}
int mgcfd_num_levels(const mgcfd_solver *s) { return s ? static_cast<int>(s->L.size()) : 0; }
int64_t mgcfd_level_nel(const mgcfd_solver *s, int l)
{ return (s && l >= 0 && l < static_cast<int>(s->L.size())) ? s->L[static_cast<size_t>(l)].info.nel : -1; }
int64_t mgcfd_level_num_internal_edges(const mgcfd_solver *s, int l)
{ return (s && l >= 0 && l < static_cast<int>(s->L.size())) ? s->L[static_cast<size_t>(l)].info.n_internal : -1; }
int mgcfd_get_far_field(const mgcfd_solver *s, double *out17)
{
    REQUIRE(s); REQUIRE(out17);
    std::memcpy(out17, s->ff17, sizeof(double) * 17);
    return MGCFD_OK;
}
int mgcfd_free_stream_constants(double mach, double alpha_deg, double out17[17])
{
    REQUIRE(out17);
    if (!std::isfinite(mach) || !std::isfinite(alpha_deg)) { g_last_error = "free stream: Mach number and angle of attack must be finite"; return MGCFD_ERR_ARG; }
    if (!(mach > 0.0)) { g_last_error = "free stream: the Mach number must be positive"; return MGCFD_ERR_ARG; }
    if (!(std::fabs(alpha_deg) < 90.0)) { g_last_error = "free stream: the angle of attack must lie inside (-90, 90) degrees"; return MGCFD_ERR_ARG; }
    free_stream_constants(mach, alpha_deg, out17);
    return MGCFD_OK;
}
int mgcfd_get_free_stream(const mgcfd_solver *s, double *mach, double *alpha_deg)
{
    REQUIRE(s);
    if (mach) *mach = s->fs_mach;
    if (alpha_deg) *alpha_deg = s->fs_alpha_deg;
    return MGCFD_OK;
}
static void synchronize_with_group(mgcfd_solver *s);
// A kernel-granular sweep that has begun (mgcfd_sweep_flux0, mgcfd_sweep_stage 0 or 1) holds half a sweep of the OLD free
// stream in its buffers and flags: the setter refuses until its last stage has run.
static void require_no_sweep_under_way(const mgcfd_solver *s, const char *what = "free stream")
{
    for (size_t l = 0; l < s->L.size(); l++)
        if (s->L[l].stage_next != 0 || s->L[l].sweep_flux0_done)
            throw std::invalid_argument(std::string(what) + ": a sweep is under way on level " + std::to_string(l) + " (mgcfd_sweep_flux0 / mgcfd_sweep_stage): finish it first");
}
// How every setter of a run-time option starts: no kernel-granular sweep under way (`what` names the option in the refusal), the
// solver idle — its stream, and as a rank its message stream and the streams a group's graph forks to — its timings folded
// and its captured graphs gone (captured launches carry the options they were captured with as kernel arguments).
static void quiesce(mgcfd_solver *s, const char *what)
{
    require_no_sweep_under_way(s, what);
    s->use_device();
    s->fold_events();
    HIP_CHECK(hipStreamSynchronize(s->stream));
    synchronize_with_group(s);
    s->drop_graphs();
}
// ... and how it ends where the option changes the kind of sweep a level runs: partial_min / sf_alt hold work done ahead
// for the other kind
static void drop_look_ahead(mgcfd_solver *s)
{
    for (DeviceLevel &lv : s->L) lv.min_ahead = false;
}
// Level 0's numbering for the ordered RMS sum (mgcfd_solver::ordered_rms, op_sumsq_ordered) is held exactly while an option that
// orders the sum is on: every setter of such an option calls this once its new state is stored.
static void settle_rms_order(mgcfd_solver *s)
{
    DeviceLevel &l0 = s->L[0];
    if (!s->ordered_rms()) l0.mem.release(l0.new_of_old_dev);
    else if (!l0.new_of_old_dev) l0.new_of_old_dev = l0.mem.upload(l0.plan.new_of_old);
}
// The solver is idle and its graphs are gone: the new far field, and with `reinitialise` the state mgcfd_create leaves.
static void apply_free_stream(mgcfd_solver *s, const double ff17[17], double mach, double alpha_deg, int reinitialise)
{
    s->use_device();
    s->set_far_field(ff17);
    s->fs_mach = mach;
    s->fs_alpha_deg = alpha_deg;
    if (!reinitialise) return;                  // warm start: the state stays
    for (DeviceLevel &lv : s->L) {
        s->settle_residuals(lv);                // (residuals[] keeps what the last sweep left: its operands are about to change)
        launch_init_variables(s->stream, lv.dp.stride, s->ff, lv.q);
        launch_init_variables(s->stream, lv.dp.stride, s->ff, lv.q_alt);     // valid numbers in the padded tail
        lv.min_ahead = false;
        lv.have_sumsq = false;
        lv.stage_out = nullptr;                 // (MGCFD_ARR_STAGE named a stage of the state that has just gone)
        if (lv.fas_p) HIP_CHECK(hipMemsetAsync(lv.fas_p, 0, sizeof(double) * 5 * lv.dp.stride, s->stream));   // (the forcing belonged to the old state)
        s->viscous_wall(static_cast<int>(&lv - s->L.data()), lv.q);
        if (s->sa_on(static_cast<int>(&lv - s->L.data()))) s->sa_form(lv, true);
        if (lv.sa_ntn) launch_dual_shift(s->stream, lv.dp.stride, lv.sa_nt, lv.sa_ntn, lv.sa_ntn1, 1);     // (both time levels: the new nt)
    }
    HIP_CHECK(hipMemsetAsync(s->err, 0xFF, sizeof(unsigned long long), s->stream));
    s->check_seq = 0;
    s->invalid_cell = -1; s->invalid_cycle = -1;
    HIP_CHECK(hipStreamSynchronize(s->stream));
    HIP_CHECK(hipGetLastError());
}
int mgcfd_set_free_stream(mgcfd_solver *s, double mach, double alpha_deg, int reinitialise)
{
    REQUIRE(s);
    double ff17[17];
    const int rc = mgcfd_free_stream_constants(mach, alpha_deg, ff17);
    if (rc != MGCFD_OK) return rc;
    return guarded([&] {
        quiesce(s, "free stream");
        apply_free_stream(s, ff17, mach, alpha_deg, reinitialise);
    });
}

// ---- the time step: mode and CFL number ----
static void check_time_step(int mode, double cfl)
{
    if (mode != MGCFD_DT_REFERENCE && mode != MGCFD_DT_GLOBAL && mode != MGCFD_DT_LOCAL && mode != MGCFD_DT_LOCAL_LEGACY)
        throw std::invalid_argument("time step: unknown mode " + std::to_string(mode));
    if (!std::isfinite(cfl) || !(cfl > 0.0)) throw std::invalid_argument("time step: the CFL number must be finite and positive");
}
// The solver is idle and its graphs are gone (captured launches carry the CFL number and the look-ahead they were captured
// with): the new policy, and nothing computed ahead under the old one survives.
static void apply_time_step(mgcfd_solver *s, int mode, double cfl)
{
    s->dt_mode = mode;
    s->cfl = cfl;
    drop_look_ahead(s);
}
int mgcfd_set_time_step(mgcfd_solver *s, int mode, double cfl)
{
    REQUIRE(s);
    return guarded([&] {
        check_time_step(mode, cfl);
        quiesce(s, "time step");
        apply_time_step(s, mode, cfl);
    });
}
int mgcfd_get_time_step(const mgcfd_solver *s, int *mode, double *cfl)
{
    REQUIRE(s);
    if (mode) *mode = s->dt_mode;
    if (cfl) *cfl = s->cfl;
    return MGCFD_OK;
}

// ---- implicit residual smoothing: coefficient and Jacobi iterations ----
int mgcfd_set_residual_smoothing(mgcfd_solver *s, double eps, int iterations)
{
    REQUIRE(s);
    return guarded([&] {
        if (iterations < 0 || iterations > MGCFD_MAX_SMOOTHING_ITERATIONS)
            throw std::invalid_argument("residual smoothing: iterations must be 0 ... " + std::to_string(MGCFD_MAX_SMOOTHING_ITERATIONS));
        if (iterations > 0 && (!std::isfinite(eps) || !(eps > 0.0))) throw std::invalid_argument("residual smoothing: eps must be finite and positive");
        if (iterations > 0 && (s->partitioned || s->comm))
            throw std::invalid_argument("residual smoothing: not on a partitioned solver or a rank (a level split over ranks would need a ghost exchange per iteration)");
        quiesce(s, "residual smoothing");
        if (iterations > 0)
            for (DeviceLevel &lv : s->L)
                for (double *&b : lv.smooth_buf)
                    if (!b) b = lv.mem.alloc<double>(static_cast<size_t>(5 * lv.dp.stride));
        s->irs_iters = iterations;
        s->irs_eps = iterations > 0 ? eps : 0.0;
    });
}
int mgcfd_get_residual_smoothing(const mgcfd_solver *s, double *eps, int *iterations)
{
    REQUIRE(s);
    if (eps) *eps = s->irs_eps;
    if (iterations) *iterations = s->irs_iters;
    return MGCFD_OK;
}

// ---- JST dissipation: the two coefficients and the levels it runs on ----
int mgcfd_set_jst(mgcfd_solver *s, double kappa2, double kappa4, int levels)
{
    REQUIRE(s);
    return guarded([&] {
        if (levels < 0) throw std::invalid_argument("JST dissipation: levels must be 0 (off) or more");
        if (!std::isfinite(kappa2) || kappa2 < 0.0 || !std::isfinite(kappa4) || kappa4 < 0.0)
            throw std::invalid_argument("JST dissipation: kappa2 and kappa4 must be finite and not negative");
        if (levels > 0 && !(kappa2 > 0.0) && !(kappa4 > 0.0)) throw std::invalid_argument("JST dissipation: one of kappa2 and kappa4 must be positive");
        if (levels > 0 && (s->partitioned || s->comm))
            throw std::invalid_argument("JST dissipation: not on a partitioned solver or a rank (a level split over ranks would need L, nu and r exchanged per stage)");
        if (levels > 0 && s->up_levels > 0)
            throw std::invalid_argument("JST dissipation: not on a level the upwind flux is on (mgcfd_set_upwind: Roe's flux carries its own dissipation)");
        quiesce(s, "JST dissipation");
        const int n = std::min(levels, static_cast<int>(s->L.size()));
        for (int l = 0; l < n; l++) {
            DeviceLevel &lv = s->L[static_cast<size_t>(l)];
            if (!lv.jst_buf) lv.jst_buf = lv.mem.alloc<double>(static_cast<size_t>(7 * lv.dp.stride));
        }
        s->jst_levels = n;
        s->jst_kappa2 = n > 0 ? kappa2 : 0.0;
        s->jst_kappa4 = n > 0 ? kappa4 : 0.0;
        settle_rms_order(s);
        drop_look_ahead(s);
    });
}
int mgcfd_get_jst(const mgcfd_solver *s, double *kappa2, double *kappa4, int *levels)
{
    REQUIRE(s);
    if (kappa2) *kappa2 = s->jst_kappa2;
    if (kappa4) *kappa4 = s->jst_kappa4;
    if (levels) *levels = s->jst_levels;
    return MGCFD_OK;
}

// ---- wall distance: the nearest-wall-node field of a level, the wall-limited Smagorinsky length scale ----
// The level's wall distance where it does not hold one yet (allocations, uploads and a synchronisation: never inside a capture
// or a cycle).  The coordinates, permuted to the solver's numbering, and the wall nodes' live on the device for the launch only.
static void compute_level_wall_distance(mgcfd_solver *s, DeviceLevel &lv)
{
    if (lv.wall_d) return;
    if (lv.coords.empty()) throw std::invalid_argument("wall distance: the level was created without coordinates");
    const int64_t nel = lv.info.nel, stride = lv.dp.stride;
    if (stride % kTile != 0 || stride < nel) throw std::logic_error("wall distance: the level's stride is not a whole number of tiles");
    // the wall nodes: the distinct b ends of the solid-wall edges in ascending original id (WallRows::original)
    std::vector<int64_t> ids;
    ids.reserve(static_cast<size_t>(lv.info.n_boundary));
    for (int64_t k = 0; k < lv.info.n_boundary; k++) {
        const int64_t b = lv.edges[static_cast<size_t>(lv.info.boundary_start + k)].b;
        if (b < 0 || b >= nel) throw std::invalid_argument("wall distance: a solid-wall edge names a node out of range");
        ids.push_back(b);
    }
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const size_t m = ids.size(), st = static_cast<size_t>(stride);
    std::vector<double> x(3 * st, 0.0), wx(3 * m);
    for (int64_t n = 0; n < nel; n++) {
        const size_t o = static_cast<size_t>(lv.plan.old_of_new[static_cast<size_t>(n)]);
        for (size_t c = 0; c < 3; c++) x[c * st + static_cast<size_t>(n)] = lv.coords[3 * o + c];
    }
    for (size_t j = 0; j < m; j++)
        for (size_t c = 0; c < 3; c++) wx[c * m + j] = lv.coords[3 * static_cast<size_t>(ids[j]) + c];
    DeviceOwner visiting, kept;                      // (the coordinates go when this returns, d and nearest stay with the level)
    WallDistance a;
    a.x = visiting.upload(x); a.wx = visiting.upload(wx); a.m = static_cast<int32_t>(m);
    a.d = kept.alloc<double>(st); a.nearest = kept.alloc<int32_t>(st);
    launch_wall_distance(s->stream, nel, stride, a);
    HIP_CHECK(hipStreamSynchronize(s->stream));
    HIP_CHECK(hipGetLastError());
    lv.mem.absorb(std::move(kept));
    lv.wall_d = a.d; lv.wall_near = a.nearest; lv.wall_ids = std::move(ids);
}
// A setter about to store (visc_levels, eddy, on) asks first: MGCFD_ERR_ARG with nothing changed where the damping would take
// effect on a level that neither holds the distance nor came with coordinates.
static void require_damping_possible(const mgcfd_solver *s, int visc_levels, int eddy, int on)
{
    if (!on || eddy != MGCFD_EDDY_SMAGORINSKY) return;
    for (int l = 0; l < visc_levels && l < static_cast<int>(s->L.size()); l++)
        if (!s->L[static_cast<size_t>(l)].wall_d && s->L[static_cast<size_t>(l)].coords.empty())
            throw std::invalid_argument("wall damping: level " + std::to_string(l) + " was created without coordinates (the damping would take effect there)");
}
// ... and likewise for the Spalart-Allmaras model, which needs the distance on every level it takes effect on and has no BDF
// source under dual time stepping.
static void require_sa_possible(const mgcfd_solver *s, int visc_levels, int eddy)
{
    if (eddy != MGCFD_EDDY_SPALART_ALLMARAS) return;
    if (s->dual_time() && !s->sa_time_accurate)
        throw std::invalid_argument("Spalart-Allmaras model: not while dual time stepping is on (nu_tilde has no BDF source; mgcfd_set_sa_unsteady with time_accurate gives it one)");
    for (int l = 0; l < visc_levels && l < static_cast<int>(s->L.size()); l++)
        if (!s->L[static_cast<size_t>(l)].wall_d && s->L[static_cast<size_t>(l)].coords.empty())
            throw std::invalid_argument("Spalart-Allmaras model: level " + std::to_string(l) + " was created without coordinates (the model needs the wall distance there)");
}
// nt of a level — and on level 0, where the transport runs, its two companions and sa_gradient — is held exactly while the
// model is in effect on it; a level that comes
// into the model (or every level, `all`: the eddy mode has just changed) starts from the free-stream value.  Called once the
// new state is stored and mut is settled.
static void settle_sa(mgcfd_solver *s, bool all)
{
    for (int l = 0; l < static_cast<int>(s->L.size()); l++) {
        DeviceLevel &lv = s->L[static_cast<size_t>(l)];
        if (!s->sa_on(l)) {
            lv.mem.release(lv.sa_nt); lv.mem.release(lv.sa_old); lv.mem.release(lv.sa_spare); lv.mem.release(lv.sa_grad);
            continue;
        }
        compute_level_wall_distance(s, lv);
        const size_t stride = static_cast<size_t>(lv.dp.stride);
        const bool fresh = !lv.sa_nt;
        if (fresh) {
            lv.sa_nt = lv.mem.alloc<double>(stride);
            if (l == 0) {                            // (transport runs on level 0 only: the others hold nt alone)
                lv.sa_old = lv.mem.alloc<double>(stride); lv.sa_spare = lv.mem.alloc<double>(stride);
                lv.sa_grad = lv.mem.alloc<double>(5 * stride);
                HIP_CHECK(hipMemsetAsync(lv.sa_spare, 0, sizeof(double) * stride, s->stream));
                HIP_CHECK(hipMemsetAsync(lv.sa_grad, 0, sizeof(double) * 5 * stride, s->stream));
            }
        }
        if (fresh || all) {
            s->sa_form(lv, true);
            if (l == 0) HIP_CHECK(hipMemcpyAsync(lv.sa_old, lv.sa_nt, sizeof(double) * stride, hipMemcpyDeviceToDevice, s->stream));
        }
    }
    HIP_CHECK(hipStreamSynchronize(s->stream));
}

// The unsteady model's arrays on level 0 (mgcfd_set_sa_unsteady): the two time levels of nt are held exactly while the model,
// dual time stepping and time_accurate are all in effect, and start as nt; delta and d~ exactly while the model is in effect and
// the length is not the wall distance.  Every setter that can complete or end either combination calls this once its new state
// is stored and nt is settled; `length_changed`: the length or c_des has changed, so d~ is formed again.
static void settle_sa_unsteady(mgcfd_solver *s, bool length_changed = false)
{
    DeviceLevel &lv = s->L[0];
    const size_t stride = static_cast<size_t>(lv.dp.stride);
    if (!s->sa_timed()) { lv.mem.release(lv.sa_ntn); lv.mem.release(lv.sa_ntn1); }
    else if (!lv.sa_ntn) {
        lv.sa_ntn = lv.mem.alloc<double>(stride); lv.sa_ntn1 = lv.mem.alloc<double>(stride);
        launch_dual_shift(s->stream, lv.dp.stride, lv.sa_nt, lv.sa_ntn, lv.sa_ntn1, 1);
    }
    if (!s->sa_model_length()) { lv.mem.release(lv.sa_delta); lv.mem.release(lv.sa_len); }
    else {
        const bool fresh = !lv.sa_len;
        if (fresh) {
            // delta: the longest internal edge at the node from the coordinates as given (a node without internal edges: +inf)
            std::vector<double> delta(stride, std::numeric_limits<double>::infinity()), longest(static_cast<size_t>(lv.info.nel), -1.0);
            for (int64_t k = 0; k < lv.info.n_internal; k++) {
                const auto &e = lv.edges[static_cast<size_t>(lv.info.internal_start + k)];
                const size_t a = static_cast<size_t>(e.a), b = static_cast<size_t>(e.b);
                const double dx = lv.coords[3 * b] - lv.coords[3 * a], dy = lv.coords[3 * b + 1] - lv.coords[3 * a + 1], dz = lv.coords[3 * b + 2] - lv.coords[3 * a + 2];
                const double len = std::sqrt((dx * dx + dy * dy) + dz * dz);
                if (len > longest[a]) longest[a] = len;
                if (len > longest[b]) longest[b] = len;
            }
            for (int64_t n = 0; n < lv.info.nel; n++) {
                const double v = longest[static_cast<size_t>(lv.plan.old_of_new[static_cast<size_t>(n)])];
                if (v >= 0.0) delta[static_cast<size_t>(n)] = v;
            }
            lv.sa_delta = lv.mem.upload(delta);
            lv.sa_len = lv.mem.alloc<double>(stride);
        }
        if (fresh || length_changed) launch_sa_length(s->stream, lv.info.nel, lv.dp.stride, s->sa_shield(lv));
    }
    HIP_CHECK(hipStreamSynchronize(s->stream));
}

// l2 of a level is held exactly while the wall damping is in effect on it, and formed again by every setter that could have
// changed cs, kappa or the levels: called once the new state is stored and d2 is settled.
static void settle_wall_damping(mgcfd_solver *s)
{
    for (int l = 0; l < static_cast<int>(s->L.size()); l++) {
        DeviceLevel &lv = s->L[static_cast<size_t>(l)];
        if (!s->damping_in_effect() || !s->viscous_on(l)) { lv.mem.release(lv.visc_l2); continue; }
        compute_level_wall_distance(s, lv);
        if (!lv.visc_l2) lv.visc_l2 = lv.mem.alloc<double>(static_cast<size_t>(lv.dp.stride));
        WallLength a;
        a.d2 = lv.visc_d2; a.d = lv.wall_d; a.c2 = s->vm_cs * s->vm_cs; a.kappa = s->wd_kappa; a.l2 = lv.visc_l2;
        launch_wall_length(s->stream, lv.dp.stride, a);
    }
    HIP_CHECK(hipStreamSynchronize(s->stream));
}

// The eddy viscosity and d2 of a level are held exactly while the viscous terms cover it and a non-default viscosity model is
// set: both setters call this once their new state is stored.  A new array holds +0.0; `zero` clears the ones that stay (the
// eddy mode has changed: the values belonged to the old one).  The wall damping's l2 follows (settle_wall_damping).
static void settle_viscosity_arrays(mgcfd_solver *s, bool zero)
{
    for (int l = 0; l < static_cast<int>(s->L.size()); l++) {
        DeviceLevel &lv = s->L[static_cast<size_t>(l)];
        if (!s->viscous_on(l) || !s->variable_viscosity()) {
            lv.mem.release(lv.visc_mut); lv.mem.release(lv.visc_d2);
            lv.eddy_mode = 0;
            continue;
        }
        lv.eddy_mode = s->vm_eddy;
        const size_t stride = static_cast<size_t>(lv.dp.stride);
        if (lv.visc_mut) {
            if (zero) HIP_CHECK(hipMemsetAsync(lv.visc_mut, 0, sizeof(double) * stride, s->stream));
            continue;
        }
        lv.visc_mut = lv.mem.alloc<double>(stride);
        HIP_CHECK(hipMemsetAsync(lv.visc_mut, 0, sizeof(double) * stride, s->stream));
        // d2 = cbrt(vol) * cbrt(vol) from the host libm's cube roots the step factor uses (pad lanes: 1.0)
        std::vector<double> cb(stride), d2(stride, 1.0);
        HIP_CHECK(hipMemcpyAsync(cb.data(), lv.cbrt_vol, sizeof(double) * stride, hipMemcpyDeviceToHost, s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
        for (int64_t k = 0; k < lv.info.nel; k++) d2[static_cast<size_t>(k)] = cb[static_cast<size_t>(k)] * cb[static_cast<size_t>(k)];
        lv.visc_d2 = lv.mem.upload(d2);
    }
    HIP_CHECK(hipStreamSynchronize(s->stream));
    settle_wall_damping(s);
}

// The wall areas of a level are held exactly while the heat-flux wall is in effect on it (mgcfd_set_wall_temperature): both
// setters call this once their new state is stored and the level's wall nodes are settled.
static void settle_wall_areas(mgcfd_solver *s)
{
    for (int l = 0; l < static_cast<int>(s->L.size()); l++) {
        DeviceLevel &lv = s->L[static_cast<size_t>(l)];
        if (!s->wall_thermal(MGCFD_WALL_HEAT_FLUX) || !s->viscous_on(l)) { lv.mem.release(lv.wall_area); continue; }
        if (lv.wall_area) continue;
        std::vector<int32_t> nodes(static_cast<size_t>(lv.n_visc_wall));
        if (!nodes.empty()) HIP_CHECK(hipMemcpy(nodes.data(), lv.visc_wall, sizeof(int32_t) * nodes.size(), hipMemcpyDeviceToHost));
        lv.wall_area = lv.mem.upload(wall_areas(lv.info, lv.edges, lv.plan.new_of_old, nodes));
    }
}

// A setter about to store (visc_levels, mode) asks first: MGCFD_ERR_ARG with nothing changed where the corrected face gradient
// would take effect on a level created without coordinates.
static void require_face_gradient_possible(const mgcfd_solver *s, int visc_levels, int mode)
{
    if (mode != MGCFD_FACE_GRADIENT_CORRECTED) return;
    for (int l = 0; l < visc_levels && l < static_cast<int>(s->L.size()); l++)
        if (s->L[static_cast<size_t>(l)].coords.empty())
            throw std::invalid_argument("face gradient: level " + std::to_string(l) + " was created without coordinates (the corrected gradient would take effect there)");
}
// G of a level is held exactly while the corrected face gradient is in effect on it, its coordinates while that or a MUSCL level
// of the upwind flux is: the three setters call this once their new state is stored.  A new G holds +0.0.
static void settle_face_gradient(mgcfd_solver *s)
{
    for (int l = 0; l < static_cast<int>(s->L.size()); l++) {
        DeviceLevel &lv = s->L[static_cast<size_t>(l)];
        // (the coordinates serve the upwind flux's MUSCL levels too: held while either is in effect here)
        if (!s->fg_on(l) && !s->muscl_on(l)) lv.mem.release(lv.fg_x);
        else if (!lv.fg_x) lv.fg_x = lv.mem.upload(permuted_coordinates(lv.coords, lv.plan.old_of_new, lv.info.nel, lv.dp.stride));
        if (!s->fg_on(l)) { lv.mem.release(lv.fg_g); continue; }
        if (lv.fg_g) continue;
        const size_t stride = static_cast<size_t>(lv.dp.stride);
        lv.fg_g = lv.mem.alloc<double>(14 * stride);
        HIP_CHECK(hipMemsetAsync(lv.fg_g, 0, sizeof(double) * 14 * stride, s->stream));
    }
    HIP_CHECK(hipStreamSynchronize(s->stream));
}

// ---- laminar viscous terms: viscosity, Prandtl number, wall condition, step limit and the levels they run on ----
int mgcfd_set_viscous(mgcfd_solver *s, double mu, double prandtl, int wall, double cfl_v, int levels)
{
    REQUIRE(s);
    return guarded([&] {
        if (levels < 0) throw std::invalid_argument("viscous terms: levels must be 0 (off) or more");
        if (levels > 0) {
            if (!std::isfinite(mu) || !(mu > 0.0) || !std::isfinite(prandtl) || !(prandtl > 0.0) || !std::isfinite(cfl_v) || !(cfl_v > 0.0))
                throw std::invalid_argument("viscous terms: mu, prandtl and cfl_v must be finite and positive");
            if (wall != 0 && wall != 1) throw std::invalid_argument("viscous terms: wall must be 0 (slip) or 1 (no-slip, adiabatic)");
            if (s->partitioned || s->comm)
                throw std::invalid_argument("viscous terms: not on a partitioned solver or a rank (a level split over ranks would need the node stresses exchanged per stage)");
        }
        require_damping_possible(s, levels, s->vm_eddy, s->wd_on);
        require_sa_possible(s, levels, s->vm_eddy);
        require_face_gradient_possible(s, levels, s->fg_mode);
        quiesce(s, "viscous terms");
        const int n = std::min(levels, static_cast<int>(s->L.size()));
        for (int l = 0; l < static_cast<int>(s->L.size()); l++) {
            DeviceLevel &lv = s->L[static_cast<size_t>(l)];
            if (l >= n) {
                lv.mem.release(lv.visc_s); lv.mem.release(lv.visc_g); lv.mem.release(lv.visc_wall);
                lv.n_visc_wall = 0;
                continue;
            }
            if (lv.visc_s) continue;
            const size_t stride = static_cast<size_t>(lv.dp.stride);
            lv.visc_s = lv.mem.alloc<double>(12 * stride);
            HIP_CHECK(hipMemsetAsync(lv.visc_s, 0, sizeof(double) * 12 * stride, s->stream));
            // g = (cbrt(vol) * cbrt(vol)) / vol from the volumes and the host libm's cube roots the step factor uses
            std::vector<double> vol(stride), cb(stride), g(stride, 1.0);
            HIP_CHECK(hipMemcpyAsync(vol.data(), lv.volumes, sizeof(double) * stride, hipMemcpyDeviceToHost, s->stream));
            HIP_CHECK(hipMemcpyAsync(cb.data(), lv.cbrt_vol, sizeof(double) * stride, hipMemcpyDeviceToHost, s->stream));
            HIP_CHECK(hipStreamSynchronize(s->stream));
            for (int64_t k = 0; k < lv.info.nel; k++) g[static_cast<size_t>(k)] = (cb[static_cast<size_t>(k)] * cb[static_cast<size_t>(k)]) / vol[static_cast<size_t>(k)];
            lv.visc_g = lv.mem.upload(g);
            // the wall nodes: the distinct b ends of the solid-wall edges, in the library's numbering, ascending
            std::vector<int32_t> nodes;
            nodes.reserve(static_cast<size_t>(lv.info.n_boundary));
            for (int64_t k = 0; k < lv.info.n_boundary; k++)
                nodes.push_back(lv.plan.new_of_old[static_cast<size_t>(lv.edges[static_cast<size_t>(lv.info.boundary_start + k)].b)]);
            std::sort(nodes.begin(), nodes.end());
            nodes.erase(std::unique(nodes.begin(), nodes.end()), nodes.end());
            lv.n_visc_wall = static_cast<int64_t>(nodes.size());
            lv.visc_wall = lv.mem.upload(nodes);
        }
        s->visc_levels = n;
        s->visc_mu = n > 0 ? mu : 0.0;
        s->visc_prandtl = n > 0 ? prandtl : 0.0;
        s->visc_cfl = n > 0 ? cfl_v : 0.0;
        s->visc_wall = n > 0 ? wall : 0;
        settle_wall_areas(s);
        settle_viscosity_arrays(s, false);
        settle_face_gradient(s);
        settle_rms_order(s);
        drop_look_ahead(s);
        // the no-slip condition holds from the start
        for (int l = 0; l < n; l++) {
            DeviceLevel &lv = s->L[static_cast<size_t>(l)];
            if (s->visc_wall) s->settle_residuals(lv);          // (an unwritten residual's operand is about to change)
            s->viscous_wall(l, lv.q);
        }
        settle_sa(s, false);                                    // (behind the wall rule: mut of a new level is formed from the state it leaves)
        settle_sa_unsteady(s);
        HIP_CHECK(hipStreamSynchronize(s->stream));
        HIP_CHECK(hipGetLastError());
    });
}
int mgcfd_get_viscous(const mgcfd_solver *s, double *mu, double *prandtl, int *wall, double *cfl_v, int *levels)
{
    REQUIRE(s);
    if (mu) *mu = s->visc_mu;
    if (prandtl) *prandtl = s->visc_prandtl;
    if (wall) *wall = s->visc_wall;
    if (cfl_v) *cfl_v = s->visc_cfl;
    if (levels) *levels = s->visc_levels;
    return MGCFD_OK;
}
// ---- wall thermal conditions: adiabatic, isothermal and heat-flux no-slip walls (INTEGRATION.md "Wall thermal conditions") ----
// what every call of the section refuses: a rank holds part of the wall only
static void wall_heat_require_whole(const mgcfd_solver *s)
{
    if (s->partitioned || s->comm)
        throw std::invalid_argument("wall thermal conditions: not on a partitioned solver, a group member or a rank (a rank holds part of the wall only)");
}
int mgcfd_set_wall_temperature(mgcfd_solver *s, int mode, double value)
{
    REQUIRE(s);
    return guarded([&] {
        if (mode != MGCFD_WALL_ADIABATIC && mode != MGCFD_WALL_ISOTHERMAL && mode != MGCFD_WALL_HEAT_FLUX)
            throw std::invalid_argument("wall temperature: mode must be MGCFD_WALL_ADIABATIC, MGCFD_WALL_ISOTHERMAL or MGCFD_WALL_HEAT_FLUX");
        if (mode == MGCFD_WALL_ISOTHERMAL && (!std::isfinite(value) || !(value > 0.0)))
            throw std::invalid_argument("wall temperature: the wall temperature must be finite and positive");
        if (mode == MGCFD_WALL_HEAT_FLUX && !std::isfinite(value)) throw std::invalid_argument("wall temperature: the wall heat flux must be finite");
        wall_heat_require_whole(s);
        quiesce(s, "wall temperature");
        s->wt_mode = mode;
        s->wt_value = mode == MGCFD_WALL_ADIABATIC ? 0.0 : value;
        s->wt_ew = mode == MGCFD_WALL_ISOTHERMAL ? value / (1.4 - 1.0) : 0.0;
        settle_wall_areas(s);
        // the isothermal wall holds from the start (going back to adiabatic leaves the state as it stands)
        if (s->wall_thermal(MGCFD_WALL_ISOTHERMAL))
            for (int l = 0; l < s->visc_levels; l++) {
                DeviceLevel &lv = s->L[static_cast<size_t>(l)];
                s->settle_residuals(lv);                            // (an unwritten residual's operand is about to change)
                s->viscous_wall(l, lv.q);
            }
        HIP_CHECK(hipStreamSynchronize(s->stream));
        HIP_CHECK(hipGetLastError());
    });
}
// ---- the face gradient of the diffusion terms: averaged or corrected (INTEGRATION.md "Corrected face gradients") ----
int mgcfd_set_face_gradient(mgcfd_solver *s, int mode)
{
    REQUIRE(s);
    return guarded([&] {
        if (mode != MGCFD_FACE_GRADIENT_AVERAGED && mode != MGCFD_FACE_GRADIENT_CORRECTED)
            throw std::invalid_argument("face gradient: mode must be MGCFD_FACE_GRADIENT_AVERAGED or MGCFD_FACE_GRADIENT_CORRECTED");
        if (mode == MGCFD_FACE_GRADIENT_CORRECTED && (s->partitioned || s->comm))
            throw std::invalid_argument("face gradient: not on a partitioned solver, a group member or a rank (the viscous terms do not run there)");
        require_face_gradient_possible(s, s->visc_levels, mode);
        quiesce(s, "face gradient");
        s->fg_mode = mode;
        settle_face_gradient(s);
        HIP_CHECK(hipGetLastError());
    });
}
int mgcfd_get_face_gradient(const mgcfd_solver *s, int *mode)
{
    REQUIRE(s);
    if (mode) *mode = s->fg_mode;
    return MGCFD_OK;
}
// Diagnostic: kind 0 the node-gradient launch, 1 the correction launch (fluxes keeps accumulating: numbers, not a state).
int mgcfd_bench_face_gradient(mgcfd_solver *s, int level, int kind, int launches, double *avg_seconds)
{
    REQUIRE(s); REQUIRE(avg_seconds);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        if (!s->fg_on(level)) throw std::invalid_argument("the corrected face gradient is not in effect on this level (mgcfd_set_face_gradient, mgcfd_set_viscous)");
        if (kind < 0 || kind > 1) throw std::invalid_argument("face gradient launch kind: 0 node gradients, 1 correction");
        s->settle_fluxes(lv);
        const FaceGradientStep a = s->face_gradient_step(lv);
        launch_face_gradient_nodes(s->stream, lv.dp, a);    // (every array holds a stage's numbers)
        *avg_seconds = s->timed_launches(launches, [&] {
            if (kind == 0) launch_face_gradient_nodes(s->stream, lv.dp, a);
            else launch_face_gradient_correction(s->stream, lv.dp, a);
        });
        lv.fluxes_zero = false; lv.fluxes_stale = false;
    });
}
// ---- upwind fluxes: Roe's flux on the internal edges, limited MUSCL reconstruction (INTEGRATION.md "Upwind fluxes") ----
int mgcfd_set_upwind(mgcfd_solver *s, int levels, int muscl_levels, int limiter, double k, double entropy_fix)
{
    REQUIRE(s);
    return guarded([&] {
        if (levels < 0 || muscl_levels < 0) throw std::invalid_argument("upwind flux: levels and muscl_levels must be 0 (off) or more");
        if (muscl_levels > levels) throw std::invalid_argument("upwind flux: muscl_levels must not exceed levels (a level reconstructs for Roe's flux only)");
        if (limiter != MGCFD_LIMITER_NONE && limiter != MGCFD_LIMITER_BARTH_JESPERSEN && limiter != MGCFD_LIMITER_VENKATAKRISHNAN)
            throw std::invalid_argument("upwind flux: unknown limiter " + std::to_string(limiter));
        if (!std::isfinite(k) || !(k > 0.0)) throw std::invalid_argument("upwind flux: Venkatakrishnan's k must be finite and positive");
        if (!std::isfinite(entropy_fix) || entropy_fix < 0.0 || entropy_fix > 1.0)
            throw std::invalid_argument("upwind flux: entropy_fix must lie in 0 .. 1 (0: none)");
        const int n = std::min(levels, static_cast<int>(s->L.size())), nm = std::min(muscl_levels, n);
        if (n > 0 && (s->partitioned || s->comm))
            throw std::invalid_argument("upwind flux: not on a partitioned solver, a group member or a rank (a level split over ranks would need Gl exchanged per stage)");
        if (n > 0 && s->jst_levels > 0)
            throw std::invalid_argument("upwind flux: not on a level the JST dissipation is on (mgcfd_set_jst: Roe's flux carries its own dissipation)");
        for (int l = 0; l < nm; l++)
            if (s->L[static_cast<size_t>(l)].coords.empty())
                throw std::invalid_argument("upwind flux: level " + std::to_string(l) + " was created without coordinates (a MUSCL level reconstructs along the edge)");
        quiesce(s, "upwind flux");
        if (nm > 0) {
            // the reconstructing flux kernel declares more LDS than every device grants: ask before the first launch
            int lds = 0;
            HIP_CHECK(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, s->device));
            if (lds < kUpwindMusclLds)
                throw std::invalid_argument("upwind flux: a MUSCL level needs " + std::to_string(kUpwindMusclLds) + " bytes of LDS per workgroup; the device grants " + std::to_string(lds));
        }
        for (int l = 0; l < nm; l++) {
            DeviceLevel &lv = s->L[static_cast<size_t>(l)];
            if (lv.up_buf) continue;
            const size_t stride = static_cast<size_t>(lv.dp.stride);
            lv.up_buf = lv.mem.alloc<double>(20 * stride);
            HIP_CHECK(hipMemsetAsync(lv.up_buf, 0, sizeof(double) * 20 * stride, s->stream));
        }
        s->up_levels = n;
        s->up_muscl = nm;
        s->up_limiter = n > 0 ? limiter : MGCFD_LIMITER_NONE;
        s->up_k = n > 0 ? k : 0.0;
        s->up_fix = n > 0 ? entropy_fix : 0.0;
        settle_face_gradient(s);                            // (the coordinates of the MUSCL levels; synchronises)
        settle_rms_order(s);
        drop_look_ahead(s);
        HIP_CHECK(hipGetLastError());
    });
}
int mgcfd_get_upwind(const mgcfd_solver *s, int *levels, int *muscl_levels, int *limiter, double *k, double *entropy_fix)
{
    REQUIRE(s);
    if (levels) *levels = s->up_levels;
    if (muscl_levels) *muscl_levels = s->up_muscl;
    if (limiter) *limiter = s->up_limiter;
    if (k) *k = s->up_k;
    if (entropy_fix) *entropy_fix = s->up_fix;
    return MGCFD_OK;
}
// Diagnostic: kind 0 the gradient launch (a MUSCL level), 1 the flux launch of the level's instantiation (fluxes keeps
// accumulating: numbers, not a state).
int mgcfd_bench_upwind(mgcfd_solver *s, int level, int kind, int launches, double *avg_seconds)
{
    REQUIRE(s); REQUIRE(avg_seconds);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        if (!s->upwind_on(level)) throw std::invalid_argument("the upwind flux is off on this level: switch it on first (mgcfd_set_upwind)");
        if (kind < 0 || kind > 1) throw std::invalid_argument("upwind launch kind: 0 gradient, 1 flux");
        if (kind == 0 && !s->muscl_on(level)) throw std::invalid_argument("upwind launch kind 0: the level does not reconstruct (mgcfd_set_upwind's muscl_levels)");
        s->settle_fluxes(lv);
        const UpwindStep a = s->upwind_step(lv);
        const bool muscl = s->muscl_on(level);
        if (muscl) launch_upwind_gradient(s->stream, lv.dp, a);    // (every array holds a stage's numbers)
        *avg_seconds = s->timed_launches(launches, [&] {
            if (kind == 0) launch_upwind_gradient(s->stream, lv.dp, a);
            else launch_upwind_flux(s->stream, lv.dp, a, muscl);
        });
        lv.fluxes_zero = false; lv.fluxes_stale = false;
    });
}
int mgcfd_get_wall_temperature(const mgcfd_solver *s, int *mode, double *value)
{
    REQUIRE(s);
    if (mode) *mode = s->wt_mode;
    if (value) *value = s->wt_value;
    return MGCFD_OK;
}
int mgcfd_free_stream_temperature(const double ff17[17], double *t_static, double *t_total)
{
    REQUIRE(ff17);
    return guarded([&] {
        // derive()'s pressure on ff_variable; M*M = speed_sqd / (GAMMA * T)
        const double rho = ff17[0];
        const double vx = ff17[1] / rho, vy = ff17[2] / rho, vz = ff17[3] / rho;
        const double speed_sqd = vx * vx + vy * vy + vz * vz;
        const double p = (1.4 - 1.0) * (ff17[4] - 0.5 * rho * speed_sqd);
        const double t = p / rho;
        if (!std::isfinite(t) || !(t > 0.0)) throw std::invalid_argument("free-stream temperature: the far field's p / rho is not finite and positive");
        const double m2 = speed_sqd / (1.4 * t);
        if (t_static) *t_static = t;
        if (t_total) *t_total = t * (1.0 + 0.2 * m2);
    });
}
// ---- viscosity model: Sutherland's law, a caller's eddy-viscosity field, Smagorinsky ----
int mgcfd_set_viscosity_model(mgcfd_solver *s, int law, double t_ref, double s_ratio, int eddy, double cs, double prandtl_t)
{
    REQUIRE(s);
    return guarded([&] {
        auto positive = [](double x) { return std::isfinite(x) && x > 0.0; };
        if (law != MGCFD_VISCOSITY_CONSTANT && law != MGCFD_VISCOSITY_SUTHERLAND)
            throw std::invalid_argument("viscosity model: law must be MGCFD_VISCOSITY_CONSTANT or MGCFD_VISCOSITY_SUTHERLAND");
        if (eddy != MGCFD_EDDY_NONE && eddy != MGCFD_EDDY_FIELD && eddy != MGCFD_EDDY_SMAGORINSKY && eddy != MGCFD_EDDY_SPALART_ALLMARAS)
            throw std::invalid_argument("viscosity model: eddy must be MGCFD_EDDY_NONE, MGCFD_EDDY_FIELD, MGCFD_EDDY_SMAGORINSKY or MGCFD_EDDY_SPALART_ALLMARAS");
        if (!std::isfinite(t_ref) || t_ref < 0.0) throw std::invalid_argument("viscosity model: t_ref must be finite and positive, or 0 for the far field's p / rho");
        if (law == MGCFD_VISCOSITY_SUTHERLAND && !positive(s_ratio)) throw std::invalid_argument("viscosity model: Sutherland's s must be finite and positive");
        if (eddy == MGCFD_EDDY_SMAGORINSKY && !positive(cs)) throw std::invalid_argument("viscosity model: the Smagorinsky constant cs must be finite and positive");
        if (eddy != MGCFD_EDDY_NONE && !positive(prandtl_t)) throw std::invalid_argument("viscosity model: the turbulent Prandtl number must be finite and positive");
        const bool variable = law != MGCFD_VISCOSITY_CONSTANT || eddy != MGCFD_EDDY_NONE;
        const double t_taken = t_ref == 0.0 ? s->p_inf / s->ff.var[0] : t_ref;
        if (!positive(t_taken)) throw std::invalid_argument("viscosity model: the far field's p / rho is not finite and positive");
        if (variable && (s->partitioned || s->comm))
            throw std::invalid_argument("viscosity model: not on a partitioned solver, a group member or a rank (the viscous terms do not run there)");
        require_damping_possible(s, s->visc_levels, eddy, s->wd_on);
        require_sa_possible(s, s->visc_levels, eddy);
        quiesce(s, "viscosity model");
        const bool eddy_changed = eddy != s->vm_eddy;
        s->vm_law = law; s->vm_eddy = eddy;
        s->vm_t_ref = t_taken;
        // (a value the model does not use is kept as given where it could be used, the default otherwise)
        s->vm_s = positive(s_ratio) ? s_ratio : MGCFD_SUTHERLAND_S;
        s->vm_cs = positive(cs) ? cs : MGCFD_SMAGORINSKY_CS;
        s->vm_prandtl_t = positive(prandtl_t) ? prandtl_t : MGCFD_PRANDTL_TURBULENT;
        settle_viscosity_arrays(s, eddy_changed);
        settle_sa(s, eddy_changed);
        settle_sa_unsteady(s);
        HIP_CHECK(hipGetLastError());
    });
}
int mgcfd_get_viscosity_model(const mgcfd_solver *s, int *law, double *t_ref, double *s_ratio, int *eddy, double *cs, double *prandtl_t)
{
    REQUIRE(s);
    if (law) *law = s->vm_law;
    if (t_ref) *t_ref = s->vm_t_ref;
    if (s_ratio) *s_ratio = s->vm_s;
    if (eddy) *eddy = s->vm_eddy;
    if (cs) *cs = s->vm_cs;
    if (prandtl_t) *prandtl_t = s->vm_prandtl_t;
    return MGCFD_OK;
}
int mgcfd_viscosity_from_reynolds(const double ff17[17], double reynolds, double ref_length, double *mu)
{
    REQUIRE(ff17); REQUIRE(mu);
    return guarded([&] {
        if (!std::isfinite(reynolds) || !(reynolds > 0.0) || !std::isfinite(ref_length) || !(ref_length > 0.0))
            throw std::invalid_argument("viscosity from Reynolds number: reynolds and ref_length must be finite and positive");
        const double rho = ff17[0];
        const double vx = ff17[1] / rho, vy = ff17[2] / rho, vz = ff17[3] / rho;
        const double speed = std::sqrt(vx * vx + vy * vy + vz * vz);
        const double m = rho * speed * ref_length / reynolds;
        if (!std::isfinite(m) || !(m > 0.0)) throw std::invalid_argument("viscosity from Reynolds number: the far field is at rest or not finite");
        *mu = m;
    });
}

// ---- FAS multigrid: the switch ----
int mgcfd_set_fas(mgcfd_solver *s, int on)
{
    REQUIRE(s);
    return guarded([&] {
        if (on && s->L.size() < 2) throw std::invalid_argument("FAS multigrid: a one-level solver has no coarse level to force");
        if (on && (s->partitioned || s->comm))
            throw std::invalid_argument("FAS multigrid: not on a partitioned solver or a rank (a level split over ranks would need T, P and D exchanged)");
        quiesce(s, "FAS multigrid");
        for (size_t l = 1; l < s->L.size(); l++) {
            DeviceLevel &lv = s->L[l];
            const size_t n = static_cast<size_t>(5 * lv.dp.stride);
            if (on) {
                if (!lv.fas_p) lv.fas_p = lv.mem.alloc<double>(n);
                HIP_CHECK(hipMemsetAsync(lv.fas_p, 0, sizeof(double) * n, s->stream));
                if (!lv.fas_w0) { lv.fas_w0 = lv.mem.alloc<double>(n); HIP_CHECK(hipMemsetAsync(lv.fas_w0, 0, sizeof(double) * n, s->stream)); }
            } else {
                lv.mem.release(lv.fas_p);
                lv.mem.release(lv.fas_w0);
            }
        }
        HIP_CHECK(hipStreamSynchronize(s->stream));
        s->fas = on != 0;
        settle_rms_order(s);
        drop_look_ahead(s);
    });
}
int mgcfd_get_fas(const mgcfd_solver *s, int *on)
{
    REQUIRE(s);
    if (on) *on = s->fas ? 1 : 0;
    return MGCFD_OK;
}

// ---- kernel-granular operations ----
#define OP(body) REQUIRE(s); return guarded([&] { s->use_device(); body; HIP_CHECK(hipGetLastError()); })   /* (a launch that failed must not come back as MGCFD_OK) */
int mgcfd_copy_old_variables(mgcfd_solver *s, int level) { OP(s->op_copy_old(level)); }
int mgcfd_compute_step_factor(mgcfd_solver *s, int level) { OP(s->op_step_factor(level)); }
int mgcfd_compute_flux_edge(mgcfd_solver *s, int level) { OP(s->op_flux(level, 1)); }
int mgcfd_compute_boundary_flux_edge(mgcfd_solver *s, int level) { OP(s->op_flux(level, 2)); }
int mgcfd_compute_wall_flux_edge(mgcfd_solver *s, int level) { OP(s->op_flux(level, 4)); }
int mgcfd_compute_fluxes(mgcfd_solver *s, int level) { OP(s->op_flux(level, 7)); }
int mgcfd_time_step(mgcfd_solver *s, int level, int j) { OP(s->op_time_step(level, j)); }
int mgcfd_zero_fluxes(mgcfd_solver *s, int level) { OP(s->op_zero_fluxes(level)); }
int mgcfd_indirect_rw(mgcfd_solver *s, int level) { OP(s->op_indirect_rw(level)); }
int mgcfd_residual(mgcfd_solver *s, int level) { OP(s->op_residual(level)); }
int mgcfd_restrict(mgcfd_solver *s, int fine_level) { OP(s->op_restrict(fine_level)); }
int mgcfd_prolong(mgcfd_solver *s, int fine_level) { OP(s->op_prolong(fine_level)); }
int mgcfd_fas_restrict(mgcfd_solver *s, int fine_level) { OP(s->op_fas_restrict(fine_level)); }
int mgcfd_fas_prolong(mgcfd_solver *s, int fine_level) { OP(s->op_fas_prolong(fine_level)); }
int mgcfd_prolong_state(mgcfd_solver *s, int fine_level) { OP({ s->level(fine_level + 1); s->op_prolong_state(fine_level); }); }
int mgcfd_step_factor_local(mgcfd_solver *s, int level)
{
    OP({
        if (!s->global_dt()) throw std::invalid_argument("a local time step (mesh_name = fvcorr, or a local mode of mgcfd_set_time_step): nothing to reduce");
        s->op_step_factor_local(level, false, true);
        s->level(level).iters[MGCFD_LOOP_COMPUTE_STEP] += s->level(level).info.nel;
    });
}
int mgcfd_step_factor_min_devptr(mgcfd_solver *s, int level, void **devptr)
{ REQUIRE(devptr); OP(*devptr = s->level(level).min_dt); }
int mgcfd_step_factor_apply(mgcfd_solver *s, int level) { OP({ s->op_step_factor_apply(level); if (s->viscous_on(level)) s->viscous_clamp(level); if (s->dual_time()) s->clamp_step_factors(level); }); }
int mgcfd_residual_sumsq(mgcfd_solver *s, int level, void **devptr)
{ REQUIRE(devptr); OP({ s->op_sumsq(level); *devptr = s->level(level).sumsq; }); }

int mgcfd_calc_rms(mgcfd_solver *s, int level, double *rms)
{
    REQUIRE(s); REQUIRE(rms);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        if (s->ordered_rms() && level == 0) s->op_sumsq_ordered();     // (as the cycle driver runs it)
        else s->op_sumsq(level);
        double sum = 0.0;
        HIP_CHECK(hipMemcpyAsync(&sum, lv.sumsq, sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
        *rms = std::sqrt(sum / double(lv.n_owned));          // (a partitioned level: its owned nodes; ghosts are counted by their owners)
    });
}
int mgcfd_invalid_state_location(const mgcfd_solver *s, int64_t *cell, int *cycle)
{
    REQUIRE(s);
    if (cell) *cell = s->invalid_cell;
    if (cycle) *cycle = s->invalid_cycle;
    return MGCFD_OK;
}
int mgcfd_check_for_invalid_variables(mgcfd_solver *s, int level, int64_t *bad_cell)
{
    REQUIRE(s);
    int code = MGCFD_OK;
    int rc = guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        launch_check_invalid(s->stream, lv.info.nel, lv.dp.stride, lv.q, lv.dp.old_of_new, s->err);
        code = s->read_error(bad_cell);
    });
    if (rc != MGCFD_OK) return rc;
    if (code != MGCFD_OK) g_last_error = "invalid variables detected";
    return code;
}

int mgcfd_pending_invalid_state(mgcfd_solver *s, int64_t *bad_cell)
{
    REQUIRE(s);
    int code = MGCFD_OK;
    int rc = guarded([&] { s->use_device(); code = s->read_error(bad_cell); });
    if (rc != MGCFD_OK) return rc;
    if (code != MGCFD_OK) g_last_error = "invalid variables detected";
    return code;
}

// Every workgroup of a sweep's first stage takes the minimum over ALL per-workgroup partial minima: fine for a
// thousand tiles (11 MB of L2 reads at the M6 size), quadratic beyond — large levels reduce them once.
static ApplyMin first_stage_min(mgcfd_solver *s, DeviceLevel &lv)
{
    if (lv.plan.n_tiles <= 2048) return ApplyMin::Partials;
    launch_min_reduce(s->stream, lv.info.nel, lv.partial_min, lv.min_dt);
    return ApplyMin::Scalar;
}

// One smoothing sweep = the per-level body of the reference's cycle loop
// (src/euler3d_cpu_double.cpp:383-508): copy, step factor, RK x (fluxes, time_step), residual.
// Same operations, fewer passes over memory: the copy rides on the step-factor kernel, the
// "/ volume" half of the global time step on the first time_step, the residual on the last, and
// the three edge classes share one flux launch.
static void smooth_once(mgcfd_solver *s, int level)
{
    DeviceLevel &lv = s->level(level);
    if (s->opt_fuse && s->options_allow_fused(level) && !(s->variant_for(lv) & 4) && !s->opt_indirect_rw && s->opt_timing != 1 && lv.fluxes_zero) {
        // Fused stages: flux + time_step in one launch each.  No copy<double>(old_variables, variables)
        // (:383): the sweep's start state stays where it is and BECOMES old_variables; the stages run
        // variables -> q_alt -> (the former old_variables buffer) -> q_alt, and the three buffers
        // change roles at the end (DeviceLevel::rot).
        const bool global_dt = s->global_dt();
        bool apply_pending = global_dt;
        lv.residuals_stale = false;                // (an unwritten residual of the previous sweep: this sweep's replaces it)
        if (lv.min_ahead) {
            // the launch that produced `variables` already did compute_step_factor's work on them
            // (:388-395): the per-workgroup minima are in partial_min, or (fvcorr) the factors in sf_alt
            if (!global_dt) { lv.sf_par ^= 1; lv.apply_sf(); }
            lv.iters[MGCFD_LOOP_COMPUTE_STEP] += lv.info.nel;
        } else {
            apply_pending = s->op_step_factor(level, true, false);
        }
        // single level: the next sweep starts from this sweep's result, let the last stage look ahead
        const bool look_ahead = s->L.size() == 1 && lv.n_owned == lv.info.nel;   // (a partitioned level's ghosts are stale)
        const bool sumsq = lv.want_sumsq && lv.n_owned == lv.info.nel;
        // residual (:508) = the last stage's result - the sweep's start state.  On a single-level run nothing reads it before
        // the next sweep overwrites it, so the stage leaves the 40 B per node unwritten (its squares still go into the
        // RMS partials) and settle_residuals writes it if anybody asks: both operands stay where they are.
        const bool lazy_res = s->L.size() == 1 && s->opt_lazy_residual;
        const ApplyMin apply = apply_pending ? first_stage_min(s, lv) : ApplyMin::None;
        mgcfd_solver::Timed group(s, level, MGCFD_LOOP_FLUX, true, s->opt_timing == 2 ? MGCFD_RK : 1);
        for (int j = 0; j < MGCFD_RK; j++) {
            const StageBuffers b = stage_buffers(lv, j);
            StageArgs a;
            a.old = b.start;
            if (j == 0) a.apply_min = apply;
            if (j == MGCFD_RK - 1) { a.with_residual = true; a.lazy_residual = lazy_res; a.sumsq = sumsq; a.look_ahead = look_ahead; }
            s->op_fused_stage(level, j, b.in, b.out, a);
        }
        lv.have_sumsq = sumsq;
        lv.finish_sweep(look_ahead);
        lv.residuals_stale = lazy_res;
        return;
    }
    const ApplyMin apply0 = s->op_step_factor(level, true) ? first_stage_min(s, lv) : ApplyMin::None;   // :383 + :388-395
    for (int j = 0; j < MGCFD_RK; j++) {                           // :397-506
        s->op_flux(level, 7);
        // the indirect_rw probe reads fluxes[] right after, so zero for real when it is on
        s->op_time_step(level, j, j == 0 ? apply0 : ApplyMin::None, j == MGCFD_RK - 1, !s->opt_indirect_rw);   // + :508 on the last stage
        if (s->opt_indirect_rw && (j == 0 || !s->probe_first_stage_only)) { s->op_indirect_rw(level); s->op_zero_fluxes(level); }
    }
}

// One smoothing sweep.  With MGCFD_OPT_GRAPH the three (or four) launches of a fused sweep are captured once
// per (level, options, buffer rotation, look-ahead state) into a hipGraph and replayed — one host call per
// sweep; by default they are launched directly, which is faster here.  Sweeps that are being
// timed per kernel (OPT_TIMING) always run eagerly.
static void run_sweep(mgcfd_solver *s, int level)
{
    DeviceLevel &lv = s->level(level);
    const int64_t n = s->sweep_counter++;
    bool timed = s->opt_timing == 1 || (s->opt_timing == 2 && (n % s->timing_stride) == 0);     // (stride 1 when MGCFD_OPT_TIMING was set to 3)
    if (s->opt_timing == 4) {
        // Per-loop times by ATTRIBUTION (src/Monitoring/timer.cpp:58-195 wants a time per loop; bracketing every loop means
        // un-fusing every stage: 0.80 ms per cycle against 0.29).  Every Nth sweep of a level runs one launch per loop under
        // events — flux, compute_step, time_step and the indirect_rw probe as the reference's -DTIME build brackets them —
        // all others run fused and un-bracketed; mgcfd_get_loop_times apportions the batches' measured GPU time to the
        // loops by the sampled sweeps' ratios.  Same results either way (the fused stages are the same operations).
        const bool sampled = (lv.att_sweeps % s->timing_stride) == 0;
        // (the indirect_rw probe — not part of the solution — runs in every fourth sampled sweep only; LoopNumIters books it per
        //  stage, as the reference's loop structure has it, and its time is extrapolated at the measured rate)
        const bool probe = sampled && s->opt_indirect_rw && (lv.att_sweeps_sampled % 4) == 0;
        lv.att_sweeps++;
        if (sampled) lv.att_sweeps_sampled++;
        if (probe) lv.att_calls_sampled[MGCFD_LOOP_INDIRECT_RW]++;
        const int keep_t = s->opt_timing, keep_p = s->opt_indirect_rw;
        s->opt_timing = sampled ? 1 : 0;
        // (... and there behind the first Runge-Kutta stage only: the three stages' probes move the same bytes)
        if (keep_p) lv.iters[MGCFD_LOOP_INDIRECT_RW] += int64_t(probe ? MGCFD_RK - 1 : MGCFD_RK) * lv.info.n_internal;
        if (!probe) s->opt_indirect_rw = 0;
        s->probe_first_stage_only = true;
        try { smooth_once(s, level); } catch (...) { s->opt_timing = keep_t; s->opt_indirect_rw = keep_p; s->probe_first_stage_only = false; throw; }
        s->opt_timing = keep_t; s->opt_indirect_rw = keep_p; s->probe_first_stage_only = false;
        return;
    }
    // (only the fused launches are replayed: the unfused ones — the two-phase flux variant — leave host-side flags
    //  behind, fluxes_stale, that a replay would not set)
    const bool graphable = s->opt_graph && s->opt_fuse && s->options_allow_sweep_graph(level) && !(s->variant_for(lv) & 4) && !s->opt_indirect_rw && !timed && lv.fluxes_zero && !lv.fluxes_stale;
    if (!graphable) {
        const int keep = s->opt_timing;
        if (!timed) s->opt_timing = 0;
        smooth_once(s, level);
        s->opt_timing = keep;
        return;
    }
    const uint64_t key = (uint64_t(level) << 32) | (uint64_t(lv.want_sumsq) << 28) | (uint64_t(lv.sf_par) << 27) | (uint64_t(lv.rot) << 25) | (uint64_t(lv.min_ahead) << 24) | (uint64_t(s->opt_exact) << 16) | (uint64_t(s->opt_stage_wg4) << 17) | (uint64_t(s->opt_check) << 8) | uint64_t(s->opt_variant & 0xFF);
    auto it = s->sweep_graphs.find(key);
    if (it == s->sweep_graphs.end()) {
        mgcfd_solver::SweepGraph g;
        int64_t before[MGCFD_NUM_LOOPS];
        std::memcpy(before, lv.iters, sizeof(before));
        const int keep = s->opt_timing;
        s->opt_timing = 0;
        hipGraph_t graph = nullptr;
        HIP_CHECK(hipStreamBeginCapture(s->stream, hipStreamCaptureModeRelaxed));
        try {
            smooth_once(s, level);
        } catch (...) {
            (void)hipStreamEndCapture(s->stream, &graph);
            if (graph) (void)hipGraphDestroy(graph);
            s->opt_timing = keep;
            throw;
        }
        s->opt_timing = keep;
        HIP_CHECK(hipStreamEndCapture(s->stream, &graph));
        g.exec = instantiate(graph);
        for (int k = 0; k < MGCFD_NUM_LOOPS; k++) { g.iters[k] = lv.iters[k] - before[k]; lv.iters[k] = before[k]; }
        g.ahead_after = lv.min_ahead;
        g.rot_after = lv.rot;
        g.sf_par_after = lv.sf_par;
        g.sumsq_after = lv.have_sumsq;
        g.res_stale_after = lv.residuals_stale;
        it = s->sweep_graphs.emplace(key, std::move(g)).first;
    }
    HIP_CHECK(hipGraphLaunch(it->second.exec.get(), s->stream));
    lv.min_ahead = it->second.ahead_after;
    lv.rot = it->second.rot_after;
    lv.apply_rot();
    lv.sf_par = it->second.sf_par_after;
    lv.apply_sf();
    lv.have_sumsq = it->second.sumsq_after;
    lv.residuals_stale = it->second.res_stale_after;
    for (int k = 0; k < MGCFD_NUM_LOOPS; k++) lv.iters[k] += it->second.iters[k];
}

// The split sweep is made of fused stages, which residual smoothing replaces: refused while it is on.
static void require_no_smoothing(const mgcfd_solver *s, const char *who)
{
    if (s->smoothing()) throw std::invalid_argument(std::string(who) + ": not while residual smoothing is on (mgcfd_set_residual_smoothing; use mgcfd_smooth or the kernel-granular calls)");
    if (s->dual_time()) throw std::invalid_argument(std::string(who) + ": not while dual time stepping is on (mgcfd_set_dual_time; use mgcfd_smooth or the kernel-granular calls)");
    if (s->jst_on(0)) throw std::invalid_argument(std::string(who) + ": not while the JST dissipation is on (mgcfd_set_jst; use mgcfd_smooth or the kernel-granular calls)");
    if (s->upwind_on(0)) throw std::invalid_argument(std::string(who) + ": not while the upwind flux is on (mgcfd_set_upwind; use mgcfd_smooth or the kernel-granular calls)");
    if (s->viscous_on(0)) throw std::invalid_argument(std::string(who) + ": not while the viscous terms are on (mgcfd_set_viscous; use mgcfd_smooth or the kernel-granular calls)");
    if (s->fas) throw std::invalid_argument(std::string(who) + ": not while FAS multigrid is on (mgcfd_set_fas; use mgcfd_smooth or the kernel-granular calls)");
}
// The same sweep split around the one collective a multi-GPU run needs (see mgcfd.h).
static int sweep_begin_impl(mgcfd_solver *s, int level, bool scalar)
{
    OP({
        require_no_smoothing(s, "mgcfd_sweep_begin");
        DeviceLevel &lv = s->level(level);
        if (!lv.fluxes_zero) throw std::invalid_argument("sweep_begin needs zero fluxes (as after time_step)");
        lv.sweep_flux0_done = false;
        // As in smooth_once: no copy (the start state stays in `variables` and becomes old_variables
        // when sweep_end rotates the buffers), and no step-factor kernel when the launch that produced
        // `variables` already left the minima behind.
        const bool global_dt = s->global_dt();
        if (lv.min_ahead) {
            if (!global_dt) { lv.sf_par ^= 1; lv.apply_sf(); }
            lv.iters[MGCFD_LOOP_COMPUTE_STEP] += lv.info.nel;
        } else {
            s->op_step_factor(level, true, false);
        }
        if (global_dt && scalar) launch_min_reduce(s->stream, lv.info.nel, lv.partial_min, lv.min_dt);
    });
}
int mgcfd_sweep_flux0(mgcfd_solver *s, int level)
{
    OP({
        require_no_smoothing(s, "mgcfd_sweep_flux0");
        DeviceLevel &lv = s->level(level);
        if (!lv.fluxes_zero) throw std::invalid_argument("sweep_flux0 must follow sweep_begin");
        s->op_flux(level, 7);                      // stage-0 fluxes: independent of the time step
        lv.sweep_flux0_done = true;
    });
}
static int sweep_end_impl(mgcfd_solver *s, int level, bool scalar)
{
    OP({
        require_no_smoothing(s, "mgcfd_sweep_end");
        DeviceLevel &lv = s->level(level);
        const bool global_dt = s->global_dt();
        const ApplyMin apply = global_dt ? (scalar ? ApplyMin::Scalar : ApplyMin::Partials) : ApplyMin::None;
        const bool look_ahead = s->L.size() == 1 && lv.n_owned == lv.info.nel;
        auto stage = [&](int j, StageArgs a) {
            const StageBuffers b = stage_buffers(lv, j);
            a.old = b.start;
            s->op_fused_stage(level, j, a.vin_flux ? b.start : b.in, b.out, a);
        };
        StageArgs first;
        first.apply_min = apply;
        if (lv.sweep_flux0_done && global_dt && lv.dp.vin_ok) {
            // the second stage applies the first stage's time_step (on the fluxes of sweep_flux0) to its own
            // input while it stages it: no separate time_step launch, the first stage's result never touches memory
            first.vin_flux = lv.fluxes;
            stage(1, first);
            lv.iters[MGCFD_LOOP_TIME_STEP] += lv.info.nel;      // the first stage's time_step
            lv.fluxes_zero = true;                               // ... which leaves fluxes[] logically zero
            lv.fluxes_stale = true;
            lv.sweep_flux0_done = false;
        } else {
            if (lv.sweep_flux0_done) {
                s->op_time_step(level, 0, apply, false, true, lv.q, lv.q_alt);   // time_step on the fluxes of sweep_flux0
                lv.sweep_flux0_done = false;
            } else {
                s->settle_fluxes(lv);
                stage(0, first);
            }
            stage(1, StageArgs{});
        }
        StageArgs last;
        last.with_residual = true;
        last.look_ahead = look_ahead;
        stage(2, last);
        lv.finish_sweep(look_ahead);
    });
}

int mgcfd_sweep_stage(mgcfd_solver *s, int level, int j, int partials)
{
    OP({
        require_no_smoothing(s, "mgcfd_sweep_stage");
        DeviceLevel &lv = s->level(level);
        if (j != lv.stage_next) throw std::invalid_argument("mgcfd_sweep_stage: stages must run in order 0, 1, 2 after mgcfd_sweep_begin");
        const bool global_dt = s->global_dt();
        const StageBuffers b = stage_buffers(lv, j);
        StageArgs a;
        a.old = b.start;
        if (j == 0) {
            if (!lv.fluxes_zero) throw std::invalid_argument("mgcfd_sweep_stage needs zero fluxes (as after time_step)");
            s->settle_fluxes(lv);
            if (global_dt) a.apply_min = partials ? ApplyMin::Partials : ApplyMin::Scalar;
        }
        // (no look-ahead: on a partitioned level the ghosts of the new state are stale until the exchange)
        a.with_residual = j == MGCFD_RK - 1;
        s->op_fused_stage(level, j, b.in, b.out, a);
        lv.stage_out = b.out;
        lv.stage_next = (j + 1) % MGCFD_RK;
        if (j == MGCFD_RK - 1) lv.finish_sweep(false);
    });
}
int mgcfd_sweep_begin(mgcfd_solver *s, int level) { return sweep_begin_impl(s, level, true); }
int mgcfd_sweep_end(mgcfd_solver *s, int level) { return sweep_end_impl(s, level, true); }
int mgcfd_sweep_begin_partials(mgcfd_solver *s, int level) { return sweep_begin_impl(s, level, false); }
int mgcfd_sweep_end_partials(mgcfd_solver *s, int level) { return sweep_end_impl(s, level, false); }
int mgcfd_step_factor_partials_devptr(mgcfd_solver *s, int level, void **devptr, int *count)
{
    REQUIRE(devptr); REQUIRE(count);
    OP({ DeviceLevel &lv = s->level(level); *devptr = lv.partial_min; *count = static_cast<int>((lv.info.nel + 255) / 256); });
}

int mgcfd_smooth(mgcfd_solver *s, int level, int sweeps)
{
    OP({
        s->level(level);
        for (int k = 0; k < sweeps; k++) run_sweep(s, level);
    });
}

// ---- surface loads (no reference counterpart: the sum of compute_boundary_flux_edge's momentum term) ----
// The destination's fields of a task that sums rows of `kind` on solver s.
static void loads_store_to(mgcfd_solver *s, LoadsKind kind, LoadsDest to, LoadsTask &t)
{
    if (to.out) { t.out = to.out; return; }
    t.ring = s->loads_ring[static_cast<int>(kind)]; t.count = s->rms_count; t.cap = mgcfd_solver::kRmsRing;
}

// The wall plan of a level (allocations and uploads: never inside a capture or a cycle).
static WallPlan &wall_plan(mgcfd_solver *s, DeviceLevel &lv)
{
    if (lv.wp) return *lv.wp;
    const WallRows R = build_wall_rows(lv.info, lv.edges, lv.plan.new_of_old);
    auto wp = std::make_unique<WallPlan>();
    wp->original = R.original;
    wp->wn.n = static_cast<int64_t>(R.node.size());
    wp->wn.node = wp->mem.upload(R.node);
    wp->wn.int_ptr = wp->mem.upload(R.int_ptr);
    wp->wn.int_nbr = wp->mem.upload(R.int_nbr);
    wp->wn.int_n = wp->mem.upload(R.int_n);
    wp->wn.wall_ptr = wp->mem.upload(R.wall_ptr);
    wp->wn.wall_edge = wp->mem.upload(R.wall_edge);
    wp->wall_of_rec = wp->mem.upload(R.wall_of_rec);
    wp->sw = wp->mem.alloc<double>(12 * R.node.size());
    wp->partial = wp->mem.alloc<double>(kLoadsMaxWidth * static_cast<size_t>((lv.n_wall_rec + 255) / 256));
    wp->ticket = wp->mem.upload(std::vector<unsigned>(1, 0u));
    wp->dist = wp->mem.alloc<double>(MGCFD_WALL_COLUMNS * R.node.size());
    lv.wp = std::move(wp);
    return *lv.wp;
}

// The wall nodes' stresses of level l's current `variables` into the plan's table (the level is viscous and has a plan).
static void launch_wall_stress(mgcfd_solver *s, int l)
{
    DeviceLevel &lv = s->level(l);
    WallStress a;
    a.wn = lv.wp->wn; a.volumes = lv.volumes; a.sw = lv.wp->sw;
    a.mu = s->visc_mu; a.kappa = (s->visc_mu * 1.4) / ((1.4 - 1.0) * s->visc_prandtl);
    a.model = s->viscosity_model(lv);
    launch_wall_stress(s->stream, lv.dp.stride, lv.q, a);
}

// Level l's loads of `kind` of its current `variables`, stored at `to`.  Always the non-contracting kernels, whatever
// MGCFD_OPT_EXACT says.  The pressure six sum over the level's own partial sums; the wider kinds need the level's wall plan
// (loads_plan) and run the stress launch first where the viscous terms are on for the level (stress = false: the loads
// launch alone, for the diagnostics that time it).
static void launch_loads(mgcfd_solver *s, int l, LoadsKind kind, LoadsDest to, bool stress = true)
{
    DeviceLevel &lv = s->level(l);
    LoadsTaskViscous t;
    t.base.rec = lv.wall_rec; t.base.n = lv.n_wall_rec; t.base.p_inf = s->p_inf; t.base.ref = s->loads_dev;
    loads_store_to(s, kind, to, t.base);
    if (kind == LoadsKind::Pressure) {
        t.base.partial = lv.loads_partial; t.base.ticket = lv.loads_ticket;
        launch_surface_loads(s->stream, lv.dp.stride, lv.q, t.base);
        return;
    }
    const bool viscous = s->viscous_on(l);
    if (viscous && stress) launch_wall_stress(s, l);
    t.base.partial = lv.wp->partial; t.base.ticket = lv.wp->ticket;
    t.wall_of_rec = lv.wp->wall_of_rec; t.sw = viscous ? lv.wp->sw : nullptr; t.nw = lv.wp->wn.n;
    launch_surface_loads_viscous(s->stream, lv.dp.stride, lv.q, t, static_cast<int>(loads_width(kind)));
}
// What a level keeps for the launches of `kind` (allocations and uploads: never inside a capture or a cycle).
static void loads_plan(mgcfd_solver *s, DeviceLevel &lv, LoadsKind kind)
{
    if (kind != LoadsKind::Pressure) wall_plan(s, lv);
}
// The wall plan with the heat table (allocations: never inside a capture or a cycle).
static WallPlan &wall_plan_heat(mgcfd_solver *s, DeviceLevel &lv)
{
    WallPlan &wp = wall_plan(s, lv);
    if (!wp.heat) wp.heat = wp.mem.alloc<double>(MGCFD_WALL_HEAT_COLUMNS * static_cast<size_t>(wp.wn.n));
    return wp;
}

// Loads need the whole level on one solver: refuse a partitioned solver or a rank.
static void loads_require_whole(const mgcfd_solver *s);

// the reference point to the device (and the room for a synchronous call's result)
static void loads_upload_ref(mgcfd_solver *s, const double *ref_point);

// The rings a run of cycles or sweeps appends to, made by whoever first asks for them — with the solver's device selected,
// and never inside a capture.
static void ensure_rms_ring(mgcfd_solver *s)
{
    if (s->rms_ring) return;
    s->rms_ring = s->mem.alloc<double>(mgcfd_solver::kRmsRing);
    s->rms_count = s->mem.alloc<int>(1);
}
static void ensure_loads_ring(mgcfd_solver *s, LoadsKind kind)
{
    double *&ring = s->loads_ring[static_cast<int>(kind)];
    if (!ring) ring = s->mem.alloc<double>(static_cast<size_t>(mgcfd_solver::kRmsRing) * loads_width(kind));
}

static void loads_prepare(mgcfd_solver *s, const double *ref_point)
{
    loads_require_whole(s);
    loads_upload_ref(s, ref_point);
}

static void loads_upload_ref(mgcfd_solver *s, const double *ref_point)
{
    if (!s->loads_dev) s->loads_dev = s->mem.alloc<double>(3 + kLoadsMaxWidth);
    for (int k = 0; k < 3; k++) s->loads_ref_host[k] = ref_point ? ref_point[k] : 0.0;
    HIP_CHECK(hipMemcpyAsync(s->loads_dev, s->loads_ref_host, sizeof(double) * 3, hipMemcpyHostToDevice, s->stream));
}

// The tail of every synchronous loads call: `launch(to)` stores the row of `kind` at `to` on s's stream (whatever it takes:
// the single solver launches, a group waits for its ranks' terms and reduces, a rank reduces and shares), then the row to
// the caller.  wall = false, the level has no solid wall: exact zeros, nothing launched.
static void loads_now(mgcfd_solver *s, LoadsKind kind, bool wall, double *out, const std::function<void(LoadsDest)> &launch)
{
    double got[kLoadsMaxWidth] = {};
    const size_t bytes = sizeof(double) * loads_width(kind);
    if (wall) {
        launch(LoadsDest::at(s->loads_dev + 3));
        HIP_CHECK(hipMemcpyAsync(got, s->loads_dev + 3, bytes, hipMemcpyDeviceToHost, s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
        HIP_CHECK(hipGetLastError());
    }
    std::memcpy(out, got, bytes);
}

// The read-back of every loads history, [..][loads_width(kind)] at `out`: rows [first, first + n) from the first n rows of
// s's history of `kind` on s's stream (the caller synchronises before it reads them; wall = false: exact zeros, nothing
// was launched), rows [first + n, end) NaN: what did not complete.
static void loads_rows(mgcfd_solver *s, LoadsKind kind, bool wall, double *out, size_t first, size_t n, size_t end)
{
    const size_t width = loads_width(kind);
    if (n > 0 && wall)
        HIP_CHECK(hipMemcpyAsync(out + first * width, s->loads_ring[static_cast<int>(kind)], sizeof(double) * width * n, hipMemcpyDeviceToHost, s->stream));
    else std::fill(out + first * width, out + (first + n) * width, 0.0);
    if (end > first + n) std::fill(out + (first + n) * width, out + end * width, std::numeric_limits<double>::quiet_NaN());
}

// ---- cycle driver: src/euler3d_cpu_double.cpp:371-694 ----
// One multigrid cycle: the reference's state machine (sweeps on levels 0,1,..,n-1,n-2,..,1 with restrictions on the way
// up and prolongations on the way down, src/euler3d_cpu_double.cpp:371-694) generalised to the configured shape and sweep
// counts (mgcfd_set_cycle) and to a start level (mgcfd_run_cycles_from); the sum of squares of the level it starts from is
// appended to the rms ring.
static void cycle_once(mgcfd_solver *s, bool capturing)
{
    const int n = static_cast<int>(s->L.size());
    auto sweep = [&](int l) { if (capturing) smooth_once(s, l); else run_sweep(s, l); };
    SumTask rms_task;
    bool rms_pending = false;
    // (MGCFD_OPT_TIMING = 4: every Nth restriction / prolongation of a level pair is bracketed with events, see run_sweep)
    auto transfer = [&](bool restriction, int fine, const SumTask *task) {
        const int keep = s->opt_timing;
        if (keep == 4) {
            DeviceLevel &book = s->L[static_cast<size_t>(restriction ? fine + 1 : fine)];     // (the reference books restrict on the coarse level)
            const int loop = restriction ? MGCFD_LOOP_RESTRICT : MGCFD_LOOP_PROLONG;
            const bool sampled = (book.att_calls[loop] % s->timing_stride) == 0;
            book.att_calls[loop]++;
            if (sampled) book.att_calls_sampled[loop]++;
            s->opt_timing = sampled ? 1 : 0;
        }
        try {
            if (s->fas) { if (restriction) s->op_fas_restrict(fine); else s->op_fas_prolong(fine); }      // the FAS legs (mgcfd.h)
            else if (restriction) s->op_restrict(fine, task); else s->op_prolong(fine);
        } catch (...) { s->opt_timing = keep; throw; }
        s->opt_timing = keep;
    };
    // visit(l, kind) of mgcfd.h.  With the default configuration from level 0 this is the reference's cycle launch for launch:
    // sweeps on levels 0, 1, .., n-1, n-2, .., 1.  The step-factor look-ahead needs no care of its own here: a level's
    // min_ahead is set by the launch that wrote its CURRENT variables and cleared by every other writer, whatever the order.
    const int top = s->cycle_top;
    std::function<void(int, int)> visit = [&](int l, int kind) {
        DeviceLevel &lt = s->L[static_cast<size_t>(l)];
        for (int k = s->pre_sweeps(l); k > 0; k--) {
            const bool measured = l == top && k == 1;                          // the cycle's RMS: after the last of these
            // (FAS keeps level 0's fused stages but fixes the order of the RMS sum: their per-tile sums are not asked for)
            if (measured) { lt.want_sumsq = top == 0 && !s->ordered_rms(); lt.have_sumsq = false; }
            sweep(l);                                                          // :383-508
            if (!measured) continue;
            lt.want_sumsq = false;                                             // :509-512
            if (top > 0) {
                // a cycle from a coarser level: always the fixed order on that level's original numbering
                s->op_sumsq_ordered(s->rms_ring, s->rms_count, mgcfd_solver::kRmsRing, top);
            } else if (lt.have_sumsq && n > 1) {
                // the last stage left per-tile sums of squares: the restriction that follows adds them up and appends
                rms_task = SumTask{lt.tile_sumsq, static_cast<int>((lt.info.nel + 255) / 256), lt.sumsq, s->rms_ring, s->rms_count,
                                   mgcfd_solver::kRmsRing};
                rms_pending = true;
            } else if (lt.have_sumsq) {
                // ... single level: one small launch does
                launch_sum_partials_append(s->stream, static_cast<int>((lt.info.nel + 255) / 256), lt.tile_sumsq, lt.sumsq,
                                                  s->rms_ring, s->rms_count, mgcfd_solver::kRmsRing);
            } else if (s->ordered_rms()) {
                s->op_sumsq_ordered(s->rms_ring, s->rms_count, mgcfd_solver::kRmsRing);
            } else {
                s->op_sumsq(0);
                launch_append_scalar(s->stream, lt.sumsq, s->rms_ring, s->rms_count, mgcfd_solver::kRmsRing);
            }
        }
        if (l == n - 1) return;
        transfer(true, l, rms_pending ? &rms_task : nullptr);                  // :527-559
        rms_pending = false;
        visit(l + 1, kind);
        if (l + 1 < n - 1) {                                                   // (the coarsest level is visited once per down leg)
            if (kind == MGCFD_CYCLE_W) visit(l + 1, MGCFD_CYCLE_W);
            else if (kind == MGCFD_CYCLE_F) visit(l + 1, MGCFD_CYCLE_V);
        }
        transfer(false, l, nullptr);                                           // :560-688
        for (int k = s->post_sweeps(l); k > 0; k--) sweep(l);
    };
    visit(top, s->cycle_shape);
    // (the state the cycle leaves: after the last prolongation and level 0's post-sweeps)
    if (s->loads_in_cycle) launch_loads(s, 0, s->loads_kind, LoadsDest::history());
}

// loads_out != nullptr (mgcfd_run_cycles_loads*): also the level-0 surface loads of `kind` at the end of every cycle,
// [cycles][loads_width(kind)]; the kinds wider than the pressure six are launched directly (no cycle graph)
static int run_cycles_impl(mgcfd_solver *s, int cycles, double *rms_out, const double *ref_point, double *loads_out, LoadsKind kind = LoadsKind::Pressure)
{
    REQUIRE(s);
    int code = MGCFD_OK, failed_cycle = -1, seq_before = 0, seq_per_cycle = 0;
    const bool friction = loads_out && kind != LoadsKind::Pressure;
    int rc = guarded([&] {
        s->use_device();
        ensure_rms_ring(s);
        struct LoadsOff { mgcfd_solver *s; ~LoadsOff() { s->loads_in_cycle = false; s->loads_kind = LoadsKind::Pressure; } } loads_off{s};
        if (loads_out) {
            loads_prepare(s, ref_point);
            ensure_loads_ring(s, kind);
            s->loads_in_cycle = s->L[0].n_wall_rec > 0;        // (no solid wall: zeros, nothing launched)
            s->loads_kind = kind;
            if (s->loads_in_cycle) loads_plan(s, s->L[0], kind);
        }
        const size_t nl = s->L.size();
        std::vector<double> sums;
        sums.reserve(static_cast<size_t>(cycles > 0 ? cycles : 0));
        seq_before = s->check_seq;                  // checked launches of earlier calls nobody has read back yet
        for (int done = 0; done < cycles;) {
            const int chunk = std::min(cycles - done, mgcfd_solver::kRmsRing);
            HIP_CHECK(hipMemsetAsync(s->rms_count, 0, sizeof(int), s->stream));
            Event att0, att1;
            if (s->opt_timing == 4) { att0 = s->get_event(); att1 = s->get_event(); HIP_CHECK(hipEventRecord(att0.get(), s->stream)); }
            bool graphable = s->opt_graph && !friction && s->opt_fuse && s->options_allow_cycle_graph() && !s->opt_indirect_rw && s->opt_timing == 0;
            for (auto &lv : s->L) graphable = graphable && lv.fluxes_zero && !lv.fluxes_stale && !(s->variant_for(lv) & 4);
            graphable = graphable && nl <= 8;               // the graph key holds 8 levels' buffer rotations
            if (graphable) {
                // the whole cycle — every sweep and transfer of every level — as ONE graph replay.
                // The launch sequence depends on which levels enter with their step-factor minima
                // already computed (min_ahead), so that is part of the key and looked up per cycle.
                for (int c = 0; c < chunk; c++) {
                    uint64_t key = (uint64_t(s->opt_exact) << 16) | (uint64_t(s->opt_stage_wg4) << 17) | (uint64_t(s->opt_check) << 8) | uint64_t(s->opt_variant & 0xFF);
                    key |= uint64_t(s->loads_in_cycle) << 18;      // (the cycle that appends its surface loads)
                    for (size_t l = 0; l < nl && l < 8; l++) key |= (uint64_t(s->L[l].min_ahead) << (24 + l)) | (uint64_t(s->L[l].rot) << (32 + 2 * l)) | (uint64_t(s->L[l].sf_par) << (48 + l));
                    auto it = s->cycle_graphs.find(key);
                    if (it == s->cycle_graphs.end()) {
                        mgcfd_solver::CycleGraph g;
                        std::vector<std::vector<int64_t>> before(nl);
                        std::vector<bool> ahead_before, stale_before;
                        std::vector<int> rot_before, sf_before;
                        for (size_t l = 0; l < nl; l++) {
                            before[l].assign(s->L[l].iters, s->L[l].iters + MGCFD_NUM_LOOPS);
                            ahead_before.push_back(s->L[l].min_ahead);
                            stale_before.push_back(s->L[l].residuals_stale);
                            rot_before.push_back(s->L[l].rot);
                            sf_before.push_back(s->L[l].sf_par);
                        }
                        hipGraph_t graph = nullptr;
                        HIP_CHECK(hipStreamBeginCapture(s->stream, hipStreamCaptureModeRelaxed));
                        try {
                            cycle_once(s, true);
                        } catch (...) {
                            (void)hipStreamEndCapture(s->stream, &graph);
                            if (graph) (void)hipGraphDestroy(graph);
                            throw;
                        }
                        HIP_CHECK(hipStreamEndCapture(s->stream, &graph));
                        g.exec = instantiate(graph);
                        g.iters.resize(nl);
                        for (size_t l = 0; l < nl; l++) {
                            for (int k = 0; k < MGCFD_NUM_LOOPS; k++) {
                                g.iters[l].push_back(s->L[l].iters[k] - before[l][static_cast<size_t>(k)]);
                                s->L[l].iters[k] = before[l][static_cast<size_t>(k)];
                            }
                            g.ahead_after.push_back(s->L[l].min_ahead);
                            g.rot_after.push_back(s->L[l].rot);
                            g.sf_par_after.push_back(s->L[l].sf_par);
                            g.res_stale_after.push_back(s->L[l].residuals_stale);
                            s->L[l].residuals_stale = stale_before[l];
                            s->L[l].min_ahead = ahead_before[l];          // nothing ran yet: capture only recorded
                            s->L[l].rot = rot_before[l];
                            s->L[l].apply_rot();
                            s->L[l].sf_par = sf_before[l];
                            s->L[l].apply_sf();
                        }
                        it = s->cycle_graphs.emplace(key, std::move(g)).first;
                    }
                    HIP_CHECK(hipGraphLaunch(it->second.exec.get(), s->stream));
                    for (size_t l = 0; l < nl; l++) {
                        for (int k = 0; k < MGCFD_NUM_LOOPS; k++) s->L[l].iters[k] += it->second.iters[l][static_cast<size_t>(k)];
                        s->L[l].min_ahead = it->second.ahead_after[l];
                        s->L[l].residuals_stale = it->second.res_stale_after[l];   // (a single level's cycle leaves its residual unwritten)
                        s->L[l].rot = it->second.rot_after[l];
                        s->L[l].apply_rot();
                        s->L[l].sf_par = it->second.sf_par_after[l];
                        s->L[l].apply_sf();
                    }
                }
            } else {
                for (int c = 0; c < chunk; c++) {
                    cycle_once(s, false);
                    if (c == 0) seq_per_cycle = s->check_seq - seq_before;
                }
            }
            if (att1) HIP_CHECK(hipEventRecord(att1.get(), s->stream));
            const size_t at = sums.size();
            sums.resize(at + static_cast<size_t>(chunk));
            HIP_CHECK(hipMemcpyAsync(sums.data() + at, s->rms_ring, sizeof(double) * chunk, hipMemcpyDeviceToHost, s->stream));
            if (loads_out) loads_rows(s, kind, s->loads_in_cycle, loads_out, at, static_cast<size_t>(chunk), at + static_cast<size_t>(chunk));
            int seq = 0;
            code = s->read_error(nullptr, &seq);                           // synchronises
            if (att1) {
                float ms = 0.f;
                HIP_CHECK(hipEventElapsedTime(&ms, att0.get(), att1.get()));
                s->att_total += double(ms) * 1e-3;
                s->free_events.push_back(std::move(att0)); s->free_events.push_back(std::move(att1));
            }
            if (code != MGCFD_OK) {
                // the reference exits inside the failing time_step: stop here, and say in which cycle it was when
                // the launches were numbered one by one (a replayed graph repeats its numbers)
                if (seq_per_cycle > 0 && seq > seq_before)
                    failed_cycle = done + std::min(chunk - 1, (seq - 1 - seq_before) / seq_per_cycle);
                done += chunk;
                break;
            }
            done += chunk;
            seq_before = 0;
        }
        if (rms_out) {
            const double nan = std::numeric_limits<double>::quiet_NaN();
            for (int c = 0; c < cycles; c++)
                rms_out[c] = (c < static_cast<int>(sums.size()) && (failed_cycle < 0 || c < failed_cycle))
                                 ? std::sqrt(sums[static_cast<size_t>(c)] / double(s->L[static_cast<size_t>(s->cycle_top)].n_owned)) : nan;
        }
        if (loads_out && cycles > 0) {
            // NaN from the failing cycle on (the rows read back before it stay)
            const size_t valid = failed_cycle < 0 ? sums.size() : std::min(sums.size(), static_cast<size_t>(failed_cycle));
            loads_rows(s, kind, s->loads_in_cycle, loads_out, valid, 0, static_cast<size_t>(cycles));
        }
        HIP_CHECK(hipGetLastError());
    });
    if (rc != MGCFD_OK) return rc;
    if (code != MGCFD_OK) {
        s->invalid_cycle = failed_cycle;
        g_last_error = std::string("check_for_invalid_variables: ") +
                       (code == MGCFD_ERR_NAN ? "NaN/Inf" : code == MGCFD_ERR_NEG_DENSITY ? "negative density" : "negative density*energy") +
                       " at cell " + std::to_string(s->invalid_cell) +
                       (failed_cycle >= 0 ? " in cycle " + std::to_string(failed_cycle + 1) : std::string(" during the cycles"));
    }
    return code;
}

int mgcfd_run_cycles(mgcfd_solver *s, int cycles, double *rms_out) { return run_cycles_impl(s, cycles, rms_out, nullptr, nullptr); }

// ---- the cycle: shape, sweeps per level, cycles from a coarser level, full multigrid ----
int mgcfd_set_cycle(mgcfd_solver *s, int shape, const int *pre, const int *post)
{
    REQUIRE(s);
    return guarded([&] {
        const int n = static_cast<int>(s->L.size());
        if (shape != MGCFD_CYCLE_V && shape != MGCFD_CYCLE_W && shape != MGCFD_CYCLE_F)
            throw std::invalid_argument("cycle: unknown shape " + std::to_string(shape));
        std::vector<int> p(static_cast<size_t>(n), 1), q(static_cast<size_t>(n), 1);
        q[0] = 0;
        bool is_default = shape == MGCFD_CYCLE_V;
        for (int l = 0; l < n; l++) {
            if (pre) p[static_cast<size_t>(l)] = pre[l];
            if (post && l < n - 1) q[static_cast<size_t>(l)] = post[l];            // (post[n-1] is ignored)
            if (p[static_cast<size_t>(l)] < 1 || p[static_cast<size_t>(l)] > MGCFD_MAX_CYCLE_SWEEPS)
                throw std::invalid_argument("cycle: pre[" + std::to_string(l) + "] must lie in 1.." + std::to_string(MGCFD_MAX_CYCLE_SWEEPS));
            if (q[static_cast<size_t>(l)] < 0 || q[static_cast<size_t>(l)] > MGCFD_MAX_CYCLE_SWEEPS)
                throw std::invalid_argument("cycle: post[" + std::to_string(l) + "] must lie in 0.." + std::to_string(MGCFD_MAX_CYCLE_SWEEPS));
            is_default = is_default && p[static_cast<size_t>(l)] == 1 && (l == n - 1 || q[static_cast<size_t>(l)] == (l == 0 ? 0 : 1));
        }
        if (!is_default && (s->partitioned || s->comm))
            throw std::invalid_argument("cycle: only the default cycle on a partitioned solver or a rank (split levels are out of scope)");
        quiesce(s, "cycle");
        s->cycle_shape = shape;
        if (is_default) { s->cycle_pre.clear(); s->cycle_post.clear(); }
        else { s->cycle_pre = std::move(p); s->cycle_post = std::move(q); }
    });
}
int mgcfd_get_cycle(const mgcfd_solver *s, int *shape, int *pre, int *post)
{
    REQUIRE(s);
    if (shape) *shape = s->cycle_shape;
    const int n = static_cast<int>(s->L.size());
    for (int l = 0; l < n; l++) {
        if (pre) pre[l] = s->pre_sweeps(l);
        if (post) post[l] = s->post_sweeps(l);                 // (the coarsest level's entry is ignored and stays its default)
    }
    return MGCFD_OK;
}
// The groups and ranks run the reference's cycle from their own drivers: a solver with another one is refused there.
static void require_default_cycle(const mgcfd_solver *s, const char *who)
{
    if (!s->default_cycle()) throw std::invalid_argument(std::string(who) + ": not with a non-default cycle (mgcfd_set_cycle)");
}

int mgcfd_run_cycles_from(mgcfd_solver *s, int top, int cycles, double *rms_out)
{
    REQUIRE(s);
    if (top == 0) return mgcfd_run_cycles(s, cycles, rms_out);
    int rc = guarded([&] {
        DeviceLevel &lv = s->level(top);
        if (s->dual_time()) throw std::invalid_argument("mgcfd_run_cycles_from: a coarser start level while dual time is on is out of scope");
        if (cycles > MGCFD_MAX_ADVANCE_CYCLES)
            throw std::invalid_argument("mgcfd_run_cycles_from: at most " + std::to_string(MGCFD_MAX_ADVANCE_CYCLES) + " cycles per call");
        if (s->partitioned || s->comm) throw std::invalid_argument("mgcfd_run_cycles_from: not on a partitioned solver or a rank (split levels are out of scope)");
        require_no_sweep_under_way(s, "mgcfd_run_cycles_from");
        s->use_device();
        if (!lv.new_of_old_dev) lv.new_of_old_dev = lv.mem.upload(lv.plan.new_of_old);      // (goes with the solver)
    });
    if (rc != MGCFD_OK) return rc;
    s->cycle_top = top;
    rc = run_cycles_impl(s, cycles, rms_out, nullptr, nullptr);
    s->cycle_top = 0;
    s->L[static_cast<size_t>(top)].min_ahead = false;      // (work done ahead for an unforced sweep of this level: the next one may be forced)
    return rc;
}

int mgcfd_full_multigrid(mgcfd_solver *s, const int *cycles, double *rms_out)
{
    REQUIRE(s); REQUIRE(cycles);
    const int n = static_cast<int>(s->L.size());
    // everything mgcfd_run_cycles_from and mgcfd_prolong_state would refuse, before the restrictions change a coarse state
    int rc0 = guarded([&] {
        if (n > 1 && s->dual_time()) throw std::invalid_argument("mgcfd_full_multigrid: not while dual time is on (out of scope)");
        if (s->partitioned || s->comm) throw std::invalid_argument("mgcfd_full_multigrid: not on a partitioned solver or a rank (split levels are out of scope)");
        for (int l = 1; l < n; l++)
            if (cycles[l] < 0 || cycles[l] > MGCFD_MAX_ADVANCE_CYCLES)
                throw std::invalid_argument("mgcfd_full_multigrid: cycles[" + std::to_string(l) + "] must lie in 0.." + std::to_string(MGCFD_MAX_ADVANCE_CYCLES));
        require_no_sweep_under_way(s, "mgcfd_full_multigrid");
    });
    if (rc0 != MGCFD_OK) return rc0;
    for (int l = 0; l + 1 < n; l++) {
        const int rc = mgcfd_restrict(s, l);
        if (rc != MGCFD_OK) return rc;
    }
    size_t at = 0;
    for (int top = n - 1; top >= 1; top--) {
        int rc = mgcfd_run_cycles_from(s, top, cycles[top], rms_out ? rms_out + at : nullptr);
        at += static_cast<size_t>(cycles[top]);
        if (rc == MGCFD_OK) rc = mgcfd_prolong_state(s, top - 1);
        if (rc != MGCFD_OK) return rc;
    }
    return MGCFD_OK;
}

// ---- state access ----
static double *array_ptr(DeviceLevel &lv, int which, int *ncols)
{
    *ncols = 5;
    switch (which) {
        case MGCFD_ARR_VARIABLES: return lv.q;
        case MGCFD_ARR_OLD_VARIABLES: return lv.old_variables;
        case MGCFD_ARR_FLUXES: return lv.fluxes;
        case MGCFD_ARR_RESIDUALS: return lv.residuals;
        case MGCFD_ARR_STEP_FACTORS: *ncols = 1; return lv.step_factors;
        case MGCFD_ARR_VOLUMES: *ncols = 1; return lv.volumes;
        case MGCFD_ARR_TIME_N: case MGCFD_ARR_TIME_N1:
            if (!lv.time_n) throw std::invalid_argument("MGCFD_ARR_TIME_N / _TIME_N1: dual time stepping is off (mgcfd_set_dual_time)");
            return which == MGCFD_ARR_TIME_N ? lv.time_n : lv.time_n1;
        case MGCFD_ARR_JST_LAPLACIAN: case MGCFD_ARR_JST_SENSOR: case MGCFD_ARR_JST_RADIUS:
            if (!lv.jst_buf) throw std::invalid_argument("MGCFD_ARR_JST_*: the JST dissipation has not been on for this level (mgcfd_set_jst)");
            if (which == MGCFD_ARR_JST_LAPLACIAN) return lv.jst_buf;
            *ncols = 1;
            return lv.jst_buf + (which == MGCFD_ARR_JST_SENSOR ? 5 : 6) * lv.dp.stride;
        case MGCFD_ARR_FAS_FORCING: case MGCFD_ARR_FAS_START:
            if (!lv.fas_p) throw std::invalid_argument("MGCFD_ARR_FAS_*: levels >= 1 while FAS multigrid is on (mgcfd_set_fas)");
            return which == MGCFD_ARR_FAS_FORCING ? lv.fas_p : lv.fas_w0;
        case MGCFD_ARR_VISCOUS_STRESS:
            if (!lv.visc_s) throw std::invalid_argument("MGCFD_ARR_VISCOUS_STRESS: the viscous terms are off on this level (mgcfd_set_viscous)");
            *ncols = 12;
            return lv.visc_s;
        case MGCFD_ARR_EDDY_VISCOSITY:
            if (!lv.visc_mut || !lv.eddy_mode) throw std::invalid_argument("MGCFD_ARR_EDDY_VISCOSITY: no eddy viscosity on this level (mgcfd_set_viscosity_model with an eddy mode, on a level mgcfd_set_viscous covers)");
            *ncols = 1;
            return lv.visc_mut;
        case MGCFD_ARR_WALL_DISTANCE:
            if (!lv.wall_d) throw std::invalid_argument("MGCFD_ARR_WALL_DISTANCE: the level does not hold the wall distance (mgcfd_compute_wall_distance)");
            *ncols = 1;
            return lv.wall_d;
        case MGCFD_ARR_SA_NU_TILDE:
            if (!lv.sa_nt) throw std::invalid_argument("MGCFD_ARR_SA_NU_TILDE: the Spalart-Allmaras model is not in effect on this level (mgcfd_set_viscosity_model with MGCFD_EDDY_SPALART_ALLMARAS, on a level mgcfd_set_viscous covers)");
            *ncols = 1;
            return lv.sa_nt;
        case MGCFD_ARR_SA_GRADIENT:
            if (!lv.sa_grad) throw std::invalid_argument("MGCFD_ARR_SA_GRADIENT: level 0 while the Spalart-Allmaras model is in effect");
            *ncols = 5;
            return lv.sa_grad;
        case MGCFD_ARR_SA_TIME_N: case MGCFD_ARR_SA_TIME_N1:
            if (!lv.sa_ntn) throw std::invalid_argument("MGCFD_ARR_SA_TIME_N / _SA_TIME_N1: level 0 while the Spalart-Allmaras model, dual time stepping and mgcfd_set_sa_unsteady's time_accurate are all in effect");
            *ncols = 1;
            return which == MGCFD_ARR_SA_TIME_N ? lv.sa_ntn : lv.sa_ntn1;
        case MGCFD_ARR_SA_LENGTH:
            if (!lv.sa_len) throw std::invalid_argument("MGCFD_ARR_SA_LENGTH: level 0 while the Spalart-Allmaras model is in effect with a DES or DDES length (mgcfd_set_sa_unsteady)");
            *ncols = 1;
            return lv.sa_len;
        case MGCFD_ARR_VISCOUS_GRADIENT:
            if (!lv.fg_g) throw std::invalid_argument("MGCFD_ARR_VISCOUS_GRADIENT: the corrected face gradient is not in effect on this level (mgcfd_set_face_gradient, on a level mgcfd_set_viscous covers)");
            *ncols = 12;
            return lv.fg_g;
        case MGCFD_ARR_STATISTICS_MEAN: case MGCFD_ARR_STATISTICS_MOMENTS:
            if (!lv.stat_mean) throw std::invalid_argument("MGCFD_ARR_STATISTICS_MEAN / _MOMENTS: level 0 while the flow statistics are on (mgcfd_set_statistics)");
            *ncols = which == MGCFD_ARR_STATISTICS_MEAN ? 6 : 7;
            return which == MGCFD_ARR_STATISTICS_MEAN ? lv.stat_mean : lv.stat_mom;
        case MGCFD_ARR_UPWIND_GRADIENT: case MGCFD_ARR_UPWIND_LIMITER:
            if (!lv.up_buf) throw std::invalid_argument("MGCFD_ARR_UPWIND_*: no MUSCL level of the upwind flux has covered this level (mgcfd_set_upwind)");
            *ncols = which == MGCFD_ARR_UPWIND_GRADIENT ? 15 : 5;
            return which == MGCFD_ARR_UPWIND_GRADIENT ? lv.up_buf : lv.up_buf + 15 * lv.dp.stride;
        case MGCFD_ARR_STAGE:
            if (!lv.stage_out) throw std::invalid_argument("MGCFD_ARR_STAGE: no mgcfd_sweep_stage has run on this level");
            return lv.stage_out;
        default: throw std::invalid_argument("unknown array id");
    }
}
int mgcfd_get_array(mgcfd_solver *s, int level, int which, double *out)
{
    REQUIRE(s); REQUIRE(out);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        int nc = 0;
        double *src = (s->settle_residuals(lv), array_ptr(lv, which, &nc));
        if (which == MGCFD_ARR_FLUXES) s->settle_fluxes(lv);
        const int64_t stride = lv.dp.stride;
        std::vector<double> tmp(static_cast<size_t>(stride) * nc);
        HIP_CHECK(hipMemcpyAsync(tmp.data(), src, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
        fail_on_ipc_timeouts(s);                             // (an array computed from stale ghosts is not handed out as if it were good)
        for (int64_t n = 0; n < lv.info.nel; n++) {          // device: [field][new id]  ->  caller: [old id][field]
            const int64_t o = lv.plan.old_of_new[static_cast<size_t>(n)];
            for (int c = 0; c < nc; c++) out[o * nc + c] = tmp[static_cast<size_t>(c * stride + n)];
        }
    });
}
int mgcfd_set_array(mgcfd_solver *s, int level, int which, const double *in)
{
    REQUIRE(s); REQUIRE(in);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        int nc = 0;
        double *dst = (s->settle_residuals(lv), array_ptr(lv, which, &nc));
        if (which == MGCFD_ARR_VOLUMES) throw std::invalid_argument("volumes are fixed at creation");
        if (which == MGCFD_ARR_JST_LAPLACIAN || which == MGCFD_ARR_JST_SENSOR || which == MGCFD_ARR_JST_RADIUS)
            throw std::invalid_argument("MGCFD_ARR_JST_*: read-only (every flux launch of a JST level overwrites them)");
        if (which == MGCFD_ARR_FAS_FORCING || which == MGCFD_ARR_FAS_START)
            throw std::invalid_argument("MGCFD_ARR_FAS_*: read-only (every FAS restriction overwrites them)");
        if (which == MGCFD_ARR_VISCOUS_STRESS)
            throw std::invalid_argument("MGCFD_ARR_VISCOUS_STRESS: read-only (every flux launch of a viscous level overwrites it)");
        if (which == MGCFD_ARR_EDDY_VISCOSITY && lv.eddy_mode == MGCFD_EDDY_SMAGORINSKY)
            throw std::invalid_argument("MGCFD_ARR_EDDY_VISCOSITY: read-only under Smagorinsky (every flux launch of a viscous level overwrites it)");
        if (which == MGCFD_ARR_WALL_DISTANCE) throw std::invalid_argument("MGCFD_ARR_WALL_DISTANCE: read-only (geometry, from mgcfd_compute_wall_distance)");
        if (which == MGCFD_ARR_EDDY_VISCOSITY && lv.eddy_mode == MGCFD_EDDY_SPALART_ALLMARAS)
            throw std::invalid_argument("MGCFD_ARR_EDDY_VISCOSITY: read-only under the Spalart-Allmaras model (formed from MGCFD_ARR_SA_NU_TILDE)");
        if (which == MGCFD_ARR_SA_GRADIENT) throw std::invalid_argument("MGCFD_ARR_SA_GRADIENT: read-only (every flux launch of level 0 overwrites it)");
        if (which == MGCFD_ARR_VISCOUS_GRADIENT) throw std::invalid_argument("MGCFD_ARR_VISCOUS_GRADIENT: read-only (every flux launch of the level overwrites it)");
        if (which == MGCFD_ARR_SA_LENGTH) throw std::invalid_argument("MGCFD_ARR_SA_LENGTH: read-only (formed from the wall distance, the mesh and, under delayed DES, every pass 1)");
        if (which == MGCFD_ARR_UPWIND_GRADIENT || which == MGCFD_ARR_UPWIND_LIMITER)
            throw std::invalid_argument("MGCFD_ARR_UPWIND_*: read-only (every flux launch of a MUSCL level overwrites them)");
        const int64_t stride = lv.dp.stride;
        // keep the padded tail of every field as it is on the device (valid numbers)
        std::vector<double> tmp(static_cast<size_t>(stride) * nc);
        HIP_CHECK(hipMemcpyAsync(tmp.data(), dst, tmp.size() * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
        for (int64_t n = 0; n < lv.info.nel; n++) {
            const int64_t o = lv.plan.old_of_new[static_cast<size_t>(n)];
            for (int c = 0; c < nc; c++) tmp[static_cast<size_t>(c * stride + n)] = in[o * nc + c];
        }
        HIP_CHECK(hipMemcpyAsync(dst, tmp.data(), tmp.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
        if (which == MGCFD_ARR_FLUXES) { lv.fluxes_zero = false; lv.fluxes_stale = false; }
        if (which == MGCFD_ARR_VARIABLES) lv.min_ahead = false;
        // a restart: a time level written is a time level held
        if (which == MGCFD_ARR_TIME_N || which == MGCFD_ARR_SA_TIME_N) s->dual_levels = std::max(s->dual_levels, 1);
        if (which == MGCFD_ARR_TIME_N1 || which == MGCFD_ARR_SA_TIME_N1) s->dual_levels = 2;
        // a restart: mut of the new nt and the level's state, as the enabling call forms it
        if (which == MGCFD_ARR_SA_NU_TILDE) { s->sa_form(lv, false); HIP_CHECK(hipStreamSynchronize(s->stream)); }
    });
}
int mgcfd_array_devptr(mgcfd_solver *s, int level, int which, void **devptr, int64_t *count)
{
    REQUIRE(s); REQUIRE(devptr); REQUIRE(count);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        int nc = 0;
        double *p = (s->settle_residuals(lv), array_ptr(lv, which, &nc));
        if (which == MGCFD_ARR_FLUXES) s->settle_fluxes(lv);
        *devptr = p;
        *count = int64_t(nc) * lv.dp.stride;
    });
}
int mgcfd_array_written(mgcfd_solver *s, int level, int which)
{
    REQUIRE(s);
    return guarded([&] {
        DeviceLevel &lv = s->level(level);
        int nc = 0;
        (void)(s->settle_residuals(lv), array_ptr(lv, which, &nc));
        if (which == MGCFD_ARR_VOLUMES) throw std::invalid_argument("volumes are fixed at creation");
        if (which == MGCFD_ARR_EDDY_VISCOSITY && lv.eddy_mode == MGCFD_EDDY_SMAGORINSKY)
            throw std::invalid_argument("MGCFD_ARR_EDDY_VISCOSITY: read-only under Smagorinsky (every flux launch of a viscous level overwrites it)");
        if (which == MGCFD_ARR_WALL_DISTANCE) throw std::invalid_argument("MGCFD_ARR_WALL_DISTANCE: read-only (geometry, from mgcfd_compute_wall_distance)");
        if (which == MGCFD_ARR_EDDY_VISCOSITY && lv.eddy_mode == MGCFD_EDDY_SPALART_ALLMARAS)
            throw std::invalid_argument("MGCFD_ARR_EDDY_VISCOSITY: read-only under the Spalart-Allmaras model (formed from MGCFD_ARR_SA_NU_TILDE)");
        if (which == MGCFD_ARR_SA_GRADIENT) throw std::invalid_argument("MGCFD_ARR_SA_GRADIENT: read-only (every flux launch of level 0 overwrites it)");
        if (which == MGCFD_ARR_VISCOUS_GRADIENT) throw std::invalid_argument("MGCFD_ARR_VISCOUS_GRADIENT: read-only (every flux launch of the level overwrites it)");
        if (which == MGCFD_ARR_SA_LENGTH) throw std::invalid_argument("MGCFD_ARR_SA_LENGTH: read-only (formed from the wall distance, the mesh and, under delayed DES, every pass 1)");
        if (which == MGCFD_ARR_UPWIND_GRADIENT || which == MGCFD_ARR_UPWIND_LIMITER)
            throw std::invalid_argument("MGCFD_ARR_UPWIND_*: read-only (every flux launch of a MUSCL level overwrites them)");
        if (which == MGCFD_ARR_FLUXES) { lv.fluxes_zero = false; lv.fluxes_stale = false; }
        if (which == MGCFD_ARR_VARIABLES) lv.min_ahead = false;
        if (which == MGCFD_ARR_SA_NU_TILDE) { s->use_device(); s->sa_form(lv, false); }
        if (which == MGCFD_ARR_SA_TIME_N) s->dual_levels = std::max(s->dual_levels, 1);
        if (which == MGCFD_ARR_SA_TIME_N1) s->dual_levels = 2;
    });
}
// One level per rank: take a restricted `variables` array computed by the rank that holds the finer level.
int mgcfd_accept_restricted(mgcfd_solver *s, int fine_level, const void *dev_src)
{
    REQUIRE(s); REQUIRE(dev_src);
    return guarded([&] {
        s->use_device();
        DeviceLevel &fine = s->level(fine_level);
        DeviceLevel &coarse = s->level(fine_level + 1);
        if (!fine.dp.child_ptr) throw std::invalid_argument("level has no coarser level");
        launch_accept_restricted(s->stream, coarse.info.nel, coarse.dp.stride, fine.dp.child_ptr,
                                        static_cast<const double *>(dev_src), coarse.q);
        s->viscous_wall(fine_level + 1, coarse.q);
        coarse.min_ahead = false;
    });
}
int mgcfd_get_edges(mgcfd_solver *s, int level, mgcfd_edge *out)
{
    REQUIRE(s); REQUIRE(out);
    return guarded([&] {
        DeviceLevel &lv = s->level(level);
        std::memcpy(out, lv.edges.data(), lv.edges.size() * sizeof(mgcfd_edge));
    });
}

// ---- halo exchange of a partitioned level ----
int mgcfd_halo_plan(mgcfd_solver *s, int level, int64_t n, const int64_t *node_ids, int *plan)
{
    REQUIRE(s); REQUIRE(plan);
    if (n > 0) REQUIRE(node_ids);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        std::vector<int32_t> ids(static_cast<size_t>(n));
        for (int64_t k = 0; k < n; k++) {
            if (node_ids[k] < 0 || node_ids[k] >= lv.info.nel) throw std::invalid_argument("halo node id out of range");
            ids[static_cast<size_t>(k)] = lv.plan.new_of_old[static_cast<size_t>(node_ids[k])];
        }
        lv.halo_plans.emplace_back(lv.mem.upload(ids), n);
        *plan = static_cast<int>(lv.halo_plans.size()) - 1;
    });
}
static void halo_move(mgcfd_solver *s, int level, int plan, int which, void *dev_buf, bool pack)
{
    s->use_device();
    DeviceLevel &lv = s->level(level);
    if (plan < 0 || plan >= static_cast<int>(lv.halo_plans.size())) throw std::invalid_argument("unknown halo plan");
    int nc = 0;
    double *field = (s->settle_residuals(lv), array_ptr(lv, which, &nc));
    if (nc != 5) throw std::invalid_argument("halo messages carry 5-component node arrays");
    if (which == MGCFD_ARR_FLUXES) { if (pack) s->settle_fluxes(lv); else { lv.fluxes_zero = false; lv.fluxes_stale = false; } }
    if (which == MGCFD_ARR_VARIABLES && !pack) lv.min_ahead = false;
    const auto &hp = lv.halo_plans[static_cast<size_t>(plan)];
    if (hp.second > 0 && !dev_buf) throw std::invalid_argument("null message buffer");
    if (pack) launch_halo_pack(s->stream, hp.second, lv.dp.stride, hp.first, field, static_cast<double *>(dev_buf));
    else launch_halo_unpack(s->stream, hp.second, lv.dp.stride, hp.first, static_cast<const double *>(dev_buf), field);
}
int mgcfd_halo_pack(mgcfd_solver *s, int level, int plan, int which, void *dev_buf)
{ REQUIRE(s); return guarded([&] { halo_move(s, level, plan, which, dev_buf, true); }); }
int mgcfd_halo_unpack(mgcfd_solver *s, int level, int plan, int which, const void *dev_buf)
{ REQUIRE(s); return guarded([&] { halo_move(s, level, plan, which, const_cast<void *>(dev_buf), false); }); }

// ---- monitoring ----
int mgcfd_get_loop_iters(const mgcfd_solver *s, int level, int64_t out[MGCFD_NUM_LOOPS])
{
    REQUIRE(s); REQUIRE(out);
    if (level < 0 || level >= static_cast<int>(s->L.size())) { g_last_error = "level out of range"; return MGCFD_ERR_ARG; }
    std::memcpy(out, s->L[static_cast<size_t>(level)].iters, sizeof(int64_t) * MGCFD_NUM_LOOPS);
    return MGCFD_OK;
}
int mgcfd_get_loop_times(mgcfd_solver *s, int level, double out[MGCFD_NUM_LOOPS])
{
    REQUIRE(s); REQUIRE(out);
    return guarded([&] {
        s->use_device();
        s->fold_events();
        std::memcpy(out, s->level(level).times, sizeof(double) * MGCFD_NUM_LOOPS);
        if (s->opt_timing != 4 || s->att_total <= 0.0) return;
        // attribution (see run_sweep): what the un-bracketed launches of every level and loop would have taken at the sampled
        // rate, scaled so that everything adds up to the GPU time the cycle batches really took
        auto estimate = [&](const DeviceLevel &lv, int k) {
            if (k == MGCFD_LOOP_RESTRICT || k == MGCFD_LOOP_PROLONG)
                return lv.att_calls_sampled[k] > 0 ? lv.times[k] / double(lv.att_calls_sampled[k]) * double(lv.att_calls[k] - lv.att_calls_sampled[k]) : 0.0;
            if (k == MGCFD_LOOP_INDIRECT_RW) return 0.0;        // (the probe does not run in the fused sweeps: none of their time is its)
            return lv.att_sweeps_sampled > 0 ? lv.times[k] / double(lv.att_sweeps_sampled) * double(lv.att_sweeps - lv.att_sweeps_sampled) : 0.0;
        };
        double measured = 0.0, estimated = 0.0;
        for (const DeviceLevel &lv : s->L)
            for (int k = 0; k < MGCFD_NUM_LOOPS; k++) { measured += lv.times[k]; estimated += estimate(lv, k); }
        const double rest = std::max(0.0, s->att_total - measured);
        const double scale = estimated > 0.0 ? rest / estimated : 0.0;
        const DeviceLevel &lv = s->level(level);
        for (int k = 0; k < MGCFD_NUM_LOOPS; k++) out[k] = lv.times[k] + scale * estimate(lv, k);
        // indirect_rw: the measured probes' rate applied to every sweep LoopNumIters books (a rate column: iterations / time
        // stays the probe's measured rate; this time is NOT part of the batches' total)
        if (lv.att_calls_sampled[MGCFD_LOOP_INDIRECT_RW] > 0)
            out[MGCFD_LOOP_INDIRECT_RW] = lv.times[MGCFD_LOOP_INDIRECT_RW] / double(lv.att_calls_sampled[MGCFD_LOOP_INDIRECT_RW]) * double(MGCFD_RK) * double(lv.att_sweeps);
    });
}
int mgcfd_reset_monitoring(mgcfd_solver *s)
{
    REQUIRE(s);
    return guarded([&] {
        s->use_device();
        s->fold_events();
        for (auto &lv : s->L) {
            std::memset(lv.iters, 0, sizeof(lv.iters));
            std::memset(lv.times, 0, sizeof(lv.times));
            lv.flux_time = 0.0;
            lv.flux_launches = 0;
            lv.att_sweeps = lv.att_sweeps_sampled = 0;
            std::memset(lv.att_calls, 0, sizeof(lv.att_calls));
            std::memset(lv.att_calls_sampled, 0, sizeof(lv.att_calls_sampled));
        }
        s->att_total = 0.0;
    });
}
int mgcfd_get_flux_kernel_time(mgcfd_solver *s, int level, double *avg_seconds, int64_t *launches)
{
    REQUIRE(s); REQUIRE(avg_seconds); REQUIRE(launches);
    return guarded([&] {
        s->use_device();
        s->fold_events();
        DeviceLevel &lv = s->level(level);
        *launches = lv.flux_launches;
        *avg_seconds = lv.flux_launches ? lv.flux_time / double(lv.flux_launches) : 0.0;
    });
}

// Diagnostic: time `launches` back-to-back flux launches (all classes, from zero) between two
// hipEvents on the solver's stream; the state is left as after one compute_fluxes call.
int mgcfd_bench_flux(mgcfd_solver *s, int level, int launches, double *avg_seconds)
{
    REQUIRE(s); REQUIRE(avg_seconds);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        const int variant = s->variant_for(lv);
        if ((variant & 4) && !lv.dp.edge_flux)
            lv.dp.edge_flux = lv.mem.alloc<double>(static_cast<size_t>(lv.dp.n_edges_pad) * 5 + 8);
        auto go = [&] {
            s->k().flux(s->stream, lv.dp, lv.q, s->ff, lv.fluxes, 7, 0, variant, nullptr, nullptr);
        };
        go();
        *avg_seconds = s->timed_launches(launches, go);
        lv.fluxes_zero = false;
    });
}

// ... and for one kind of residual-smoothing launch: 0 the first iteration (D formed on load), 1 a middle one, 2 the last
// (the update, written to the second state buffer: the state stays; no check, no residual).  After one flux launch, so
// that fluxes[] holds a stage's numbers.
int mgcfd_bench_residual_smoothing(mgcfd_solver *s, int level, int kind, int launches, double *avg_seconds)
{
    REQUIRE(s); REQUIRE(avg_seconds);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        if (!s->smoothing()) throw std::invalid_argument("residual smoothing is off: switch it on first (mgcfd_set_residual_smoothing)");
        if (kind < 0 || kind > 2) throw std::invalid_argument("residual smoothing launch kind: 0 first, 1 middle, 2 last");
        s->k().flux(s->stream, lv.dp, lv.q, s->ff, lv.fluxes, 7, 0, s->variant_for(lv) & ~4, nullptr, nullptr);
        SmoothStep st;
        st.fluxes = lv.fluxes; st.step_factors = lv.step_factors; st.eps = s->irs_eps;
        st.next = lv.smooth_buf[0];
        s->k().smooth(s->stream, lv.dp, st);                       // smooth_buf[0] holds an iterate
        if (kind >= 1) st.prev = lv.smooth_buf[0];
        st.next = kind == 1 ? lv.smooth_buf[1] : (kind == 0 ? lv.smooth_buf[0] : nullptr);
        if (kind == 2) { st.rk_div = double(MGCFD_RK + 1); st.old_variables = lv.q; st.q_out = lv.q_alt; st.old_of_new = lv.dp.old_of_new; st.err = s->err; }
        *avg_seconds = s->timed_launches(launches, [&] { s->k().smooth(s->stream, lv.dp, st); });
        lv.fluxes_zero = false;
        lv.fluxes_stale = false;
    });
}

// ... and for one of the JST dissipation's launches: 0 the sensor, 1 the dissipation (which adds into fluxes[], accumulating
// over the launches: the state stays).  After one flux launch with both passes, so that every array holds a stage's numbers.
int mgcfd_bench_jst(mgcfd_solver *s, int level, int kind, int launches, double *avg_seconds)
{
    REQUIRE(s); REQUIRE(avg_seconds);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        if (!s->jst_on(level)) throw std::invalid_argument("the JST dissipation is off on this level: switch it on first (mgcfd_set_jst)");
        if (kind < 0 || kind > 1) throw std::invalid_argument("JST launch kind: 0 sensor, 1 dissipation");
        s->k().flux(s->stream, lv.dp, lv.q, s->ff, lv.fluxes, 7, 0, s->variant_for(lv) & ~4, nullptr, nullptr);
        const JstStep st = s->jst_step(lv);
        s->k().jst_sensor(s->stream, lv.dp, st);
        s->k().jst_dissipation(s->stream, lv.dp, st);
        *avg_seconds = s->timed_launches(launches, [&] {
            if (kind == 0) s->k().jst_sensor(s->stream, lv.dp, st);
            else s->k().jst_dissipation(s->stream, lv.dp, st);
        });
        lv.fluxes_zero = false;
        lv.fluxes_stale = false;
    });
}

// ... and for one of the viscous terms' launches: 0 the stress launch, 1 the viscous-flux launch (which adds into fluxes[], accumulating
// over the launches: the state stays).  After one flux launch with both passes, so that every array holds a stage's numbers.
int mgcfd_bench_viscous(mgcfd_solver *s, int level, int kind, int launches, double *avg_seconds)
{
    REQUIRE(s); REQUIRE(avg_seconds);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        if (!s->viscous_on(level)) throw std::invalid_argument("the viscous terms are off on this level: switch them on first (mgcfd_set_viscous)");
        if (kind < 0 || kind > 2) throw std::invalid_argument("viscous launch kind: 0 stress, 1 viscous flux, 2 the step limit");
        s->k().flux(s->stream, lv.dp, lv.q, s->ff, lv.fluxes, 7, 0, s->variant_for(lv) & ~4, nullptr, nullptr);
        const ViscousStep st = s->viscous_step(lv);
        s->k().viscous_stress(s->stream, lv.dp, st);
        s->k().viscous_flux(s->stream, lv.dp, st);
        *avg_seconds = s->timed_launches(launches, [&] {
            if (kind == 0) s->k().viscous_stress(s->stream, lv.dp, st);
            else if (kind == 1) s->k().viscous_flux(s->stream, lv.dp, st);
            else s->viscous_clamp(level);            // (a minimum: the step factors stay what the first launch left)
        });
        lv.fluxes_zero = false;
        lv.fluxes_stale = false;
    });
}

// ... and for one of FAS multigrid's launches between levels `fine_level` and `fine_level + 1`, behind one mgcfd_fas_restrict
// (so that W0 equals the coarse state and the correction the prolongation interpolates is zero): kind 0 k_restrict_fas, 1 the
// forcing launch, 2 k_time_step_src<0, true> on the coarse level (into the second state buffer, unchecked: the state stays), 3 the FAS
// prolongation; and the launches they stand beside: 4 k_restrict, 5 k_time_step on the coarse level (likewise), 6 the
// reference's prolongation (which moves the fine state launch after launch: re-initialise afterwards).
int mgcfd_bench_fas(mgcfd_solver *s, int fine_level, int kind, int launches, double *avg_seconds)
{
    REQUIRE(s); REQUIRE(avg_seconds);
    return guarded([&] {
        s->use_device();
        if (kind < 0 || kind > 6) throw std::invalid_argument("FAS launch kind: 0 ... 6");
        s->op_fas_restrict(fine_level);             // (throws while FAS is off)
        DeviceLevel &F = s->level(fine_level);
        DeviceLevel &C = s->level(fine_level + 1);
        s->settle_residuals(F);
        DualSource none;
        none.order = 0;
        *avg_seconds = s->timed_launches(launches, [&] {
            switch (kind) {
                case 0: s->k().restrict_fas(s->stream, C.info.nel, C.dp.stride, F.dp.stride, F.dp.child_ptr, F.dp.child, F.dp.child4, F.q, F.fluxes,
                                            fine_level >= 1 ? F.fas_p : nullptr, C.q, C.fas_w0, C.fas_p); break;
                case 1: launch_fas_forcing(s->stream, C.info.nel, C.dp.stride, F.dp.child_ptr, C.fluxes, C.fas_p); break;
                case 2: s->k().time_step_src(s->stream, C.info.nel, C.dp.stride, 0, C.step_factors, C.fluxes, C.fas_p, C.q, C.q_alt, C.dp.old_of_new,
                                             s->err, 0, nullptr, none); break;
                case 3: s->k().prolong_fas(s->stream, F.dp, C.dp.stride, C.fas_w0, C.q, F.q, F.cbrt_vol, s->cfl, nullptr); break;
                case 4: s->k().restrict_(s->stream, C.info.nel, C.dp.stride, F.dp.stride, F.dp.child_ptr, F.dp.child, F.dp.child4, F.q, C.q, C.cbrt_vol,
                                         s->cfl, nullptr, SumTask{}); break;
                case 5: s->k().time_step(s->stream, C.info.nel, C.dp.stride, 0, C.step_factors, C.fluxes, C.q, C.q_alt, C.dp.old_of_new, s->err, 0,
                                         nullptr, 0, C.volumes, nullptr, 0); break;
                default: s->k().prolong(s->stream, F.dp, C.dp.stride, C.residuals, F.residuals, F.q, F.cbrt_vol, s->cfl, nullptr); break;
            }
        });
        F.min_ahead = false;
        C.min_ahead = false;
    });
}

// The same for the indirect_rw probe (fluxes += ..., accumulating over the launches): the data-movement ceiling of the
// flux kernel on this level's tiles.
int mgcfd_bench_indirect_rw(mgcfd_solver *s, int level, int launches, double *avg_seconds)
{
    REQUIRE(s); REQUIRE(avg_seconds);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        s->settle_fluxes(lv);
        const int variant = s->variant_for(lv);
        auto go = [&] {
            s->k().indirect_rw(s->stream, lv.dp, lv.q, lv.fluxes, variant);
        };
        go();
        *avg_seconds = s->timed_launches(launches, go);
        lv.fluxes_zero = false;
    });
}

// The practical ceiling of that launch's data movement: a tile-shaped stream of exactly the bytes SURVEY.md §8d prices
// (40 B per internal edge + 40 B per node read from a scratch buffer of that size, 40 B per node written into `fluxes`), one
// workgroup per tile of the level, nothing dependent and nothing computed (kernels_plain.hip: k_stream_tiles).
int mgcfd_bench_stream_ceiling(mgcfd_solver *s, int level, int launches, double *avg_seconds)
{
    REQUIRE(s); REQUIRE(avg_seconds);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        s->settle_fluxes(lv);
        const int64_t rd_total = (5 * int64_t(lv.info.n_internal) + 5 * lv.dp.nel + 1) & ~int64_t(1), wr_total = 5 * lv.dp.nel;
        DeviceOwner scratch;
        double *src = scratch.alloc<double>(static_cast<size_t>(rd_total) + 512);
        HIP_CHECK(hipMemsetAsync(src, 0, (static_cast<size_t>(rd_total) + 512) * sizeof(double), s->stream));
        auto go = [&] { launch_stream_tiles(s->stream, lv.dp.n_tiles, src, lv.fluxes, rd_total, wr_total); };
        go();
        *avg_seconds = s->timed_launches(launches, go);
        lv.fluxes_zero = false;
    });
}

// 1/x and sqrt(x) as the `fast` build's order-free flux kernel computes them (kernels.hip: fast_rcp, fast_sqrt, fast_sqrt_pos),
// element by element; whatever MGCFD_OPT_EXACT says, the `fast` build's code runs.
int mgcfd_diag_fast_math(mgcfd_solver *s, int kind, int64_t n, const double *in, double *out)
{
    REQUIRE(s);
    if (kind < 0 || kind > 2 || n < 0 || (n > 0 && (!in || !out))) { g_last_error = "mgcfd_diag_fast_math: kind 0, 1 or 2, n >= 0 and both arrays"; return MGCFD_ERR_ARG; }
    return guarded([&] {
        if (n == 0) return;
        s->use_device();
        DeviceOwner scratch;
        double *d_in = scratch.alloc<double>(static_cast<size_t>(n)), *d_out = scratch.alloc<double>(static_cast<size_t>(n));
        HIP_CHECK(hipMemcpyAsync(d_in, in, static_cast<size_t>(n) * sizeof(double), hipMemcpyHostToDevice, s->stream));
        fast::launch_diag_fast_math(s->stream, kind, n, d_in, d_out);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(out, d_out, static_cast<size_t>(n) * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
    });
}

} // extern "C"

// ==========================================================================================================
// Multi-GPU in the C++ host (include/mgcfd.h "Multi-GPU in the C++ host").
//
// One level partitioned over ranks: mgcfd_rank_set_halo gives a solver its neighbours and the node lists of the
// messages; mgcfd_rank_sweeps then runs whole smoothing sweeps — the per-level body of the reference's cycle loop,
// src/euler3d_cpu_double.cpp:383-508 — with the coupling a partitioned level needs: one all-reduce(MIN) of the time
// step per sweep (src/Kernels/cfd_loops.cpp:137-150) and one halo message per neighbour after every Runge-Kutta stage.
// Per stage: the tiles next to ghost nodes first, ONE pack launch for all peers, the message on its way (RCCL:
// ncclSend/ncclRecv grouped on a second stream; in-process groups: hipMemcpyPeerAsync), the interior tiles meanwhile,
// then ONE unpack launch before the next stage's boundary tiles.  Same arithmetic as mgcfd_sweep_stage, bit for bit.
// ==========================================================================================================
namespace {

// ---- RCCL, loaded at run time (only a multi-process run needs it; a process that already holds torch's copy gets that one)
struct Rccl {
    struct Id { char b[128]; };                   // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128), passed by value
    void *lib = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, Id, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*Recv)(void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    int (*CommCount)(void *, int *) = nullptr;    // (optional: what the communicator itself says about its size and this rank)
    int (*CommUserRank)(void *, int *) = nullptr;
    static constexpr int kDouble = 8, kInt32 = 2, kMin = 3, kSum = 0;     // ncclDouble, ncclInt32, ncclMin, ncclSum (rccl.h)
};
Rccl g_rccl;

void rccl_load()
{
    if (g_rccl.lib) return;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *h = nullptr;
    for (const char *n : names) { h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
    if (!h) throw std::runtime_error(std::string("cannot load librccl: ") + dlerror());
    auto sym = [&](const char *n) { void *p = dlsym(h, n); if (!p) throw std::runtime_error(std::string("librccl lacks ") + n); return p; };
    g_rccl.GetUniqueId = reinterpret_cast<decltype(g_rccl.GetUniqueId)>(sym("ncclGetUniqueId"));
    g_rccl.CommInitRank = reinterpret_cast<decltype(g_rccl.CommInitRank)>(sym("ncclCommInitRank"));
    g_rccl.CommDestroy = reinterpret_cast<decltype(g_rccl.CommDestroy)>(sym("ncclCommDestroy"));
    g_rccl.GroupStart = reinterpret_cast<decltype(g_rccl.GroupStart)>(sym("ncclGroupStart"));
    g_rccl.GroupEnd = reinterpret_cast<decltype(g_rccl.GroupEnd)>(sym("ncclGroupEnd"));
    g_rccl.Send = reinterpret_cast<decltype(g_rccl.Send)>(sym("ncclSend"));
    g_rccl.Recv = reinterpret_cast<decltype(g_rccl.Recv)>(sym("ncclRecv"));
    g_rccl.AllReduce = reinterpret_cast<decltype(g_rccl.AllReduce)>(sym("ncclAllReduce"));
    g_rccl.GetErrorString = reinterpret_cast<decltype(g_rccl.GetErrorString)>(sym("ncclGetErrorString"));
    g_rccl.CommCount = reinterpret_cast<decltype(g_rccl.CommCount)>(dlsym(h, "ncclCommCount"));
    g_rccl.CommUserRank = reinterpret_cast<decltype(g_rccl.CommUserRank)>(dlsym(h, "ncclCommUserRank"));
    g_rccl.lib = h;
}
#define RCCL_CHECK(x) do { const int rc_ = (x); if (rc_ != 0) throw std::runtime_error(std::string("RCCL: ") + #x + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc_) : "error")); } while (0)

} // namespace


static mgcfd_comm &comm_of(mgcfd_solver *s)
{
    if (!s->comm) throw std::invalid_argument("the solver is not a rank of anything: call mgcfd_rank_attach_rccl or mgcfd_group_create first");
    return *s->comm;
}

// mgcfd_set_free_stream: whatever else may still touch this solver's memory or replay launches captured for it is idle too —
// the rank's message stream, and in an in-process group the other ranks' streams (their pushes land in this rank's ghosts,
// and a group's sweep graph, kept by rank 0, holds every rank's launches: it goes as well)
static void synchronize_with_group(mgcfd_solver *s)
{
    for (DeviceLevel &lv : s->L) if (lv.hx) HIP_CHECK(hipStreamSynchronize(lv.hx->comm_stream.get()));
    if (!s->comm || !s->comm->group) return;
    mgcfd_group *const g = s->comm->group;
    for (mgcfd_solver *r : g->ranks) {
        if (r == s) continue;
        r->use_device();
        HIP_CHECK(hipStreamSynchronize(r->stream));
        for (DeviceLevel &lv : r->L) if (lv.hx) HIP_CHECK(hipStreamSynchronize(lv.hx->comm_stream.get()));
    }
    mgcfd_solver *r0 = g->ranks[0];
    if (r0 != s) { r0->use_device(); r0->drop_graphs(); }
    s->use_device();
}

// The ranks of a group sweep ONE flow: their far fields must be the same 17 doubles, bit for bit (mgcfd_group_set_free_stream
// sets all of them; a rank set on its own is the caller's to bring back in line).
static void group_require_same_free_stream(const mgcfd_group *g)
{
    for (size_t r = 1; r < g->ranks.size(); r++)
        if (std::memcmp(g->ranks[r]->ff17, g->ranks[0]->ff17, sizeof(double) * 17) != 0)
            throw std::invalid_argument("the free stream of rank " + std::to_string(r) + " differs from rank 0's (Mach " + std::to_string(g->ranks[r]->fs_mach) +
                                        ", alpha " + std::to_string(g->ranks[r]->fs_alpha_deg) + " against Mach " + std::to_string(g->ranks[0]->fs_mach) + ", alpha " +
                                        std::to_string(g->ranks[0]->fs_alpha_deg) + "): mgcfd_group_set_free_stream sets every rank");
}

// ... and one time-step policy: the same mode and the same CFL number, bit for bit (mgcfd_group_set_time_step).
static void group_require_same_time_step(const mgcfd_group *g)
{
    const mgcfd_solver *r0 = g->ranks[0];
    for (size_t r = 1; r < g->ranks.size(); r++)
        if (g->ranks[r]->dt_mode != r0->dt_mode || std::memcmp(&g->ranks[r]->cfl, &r0->cfl, sizeof(double)) != 0)
            throw std::invalid_argument("the time step of rank " + std::to_string(r) + " differs from rank 0's (mode " + std::to_string(g->ranks[r]->dt_mode) +
                                        ", CFL " + std::to_string(g->ranks[r]->cfl) + " against mode " + std::to_string(r0->dt_mode) + ", CFL " +
                                        std::to_string(r0->cfl) + "): mgcfd_group_set_time_step sets every rank");
}

static void build_halo(mgcfd_solver *s, int level, int n_peers, const int *peers, const int64_t *send_counts, const int64_t *const *send_ids,
                       const int64_t *recv_counts, const int64_t *const *recv_ids, int world)
{
    s->use_device();
    DeviceLevel &lv = s->level(level);
    // other ranks hold device addresses into an exchange they have attached to or a group has prepared
    if (lv.hx && lv.hx->ipc)
        throw std::invalid_argument("the level's halo exchange is attached to other processes: mgcfd_rank_ipc_detach on every rank before mgcfd_rank_set_halo replaces it");
    if (lv.hx && lv.hx->group_prepared())
        throw std::invalid_argument("the level's halo exchange is in use by its group, whose ranks hold addresses into it: it cannot be replaced (create the solvers and the group anew)");
    auto hx = std::make_unique<HaloExchange>();
    std::vector<int32_t> sidx, ridx;
    hx->send_off.push_back(0); hx->recv_off.push_back(0);
    for (int k = 0; k < n_peers; k++) {
        if (k > 0 && peers[k] <= peers[k - 1]) throw std::invalid_argument("peers must be ascending");
        hx->peer.push_back(peers[k]);
        for (int64_t i = 0; i < send_counts[k]; i++) {
            const int64_t id = send_ids[k][i];
            if (id < 0 || id >= lv.n_owned) throw std::invalid_argument("a node sent to a peer must be owned");
            sidx.push_back(lv.plan.new_of_old[static_cast<size_t>(id)]);
        }
        for (int64_t i = 0; i < recv_counts[k]; i++) {
            const int64_t id = recv_ids[k][i];
            if (id < lv.n_owned || id >= lv.info.nel) throw std::invalid_argument("a node received from a peer must be a ghost");
            ridx.push_back(lv.plan.new_of_old[static_cast<size_t>(id)]);
        }
        hx->send_off.push_back(static_cast<int64_t>(sidx.size()));
        hx->recv_off.push_back(static_cast<int64_t>(ridx.size()));
    }
    hx->send_idx = hx->mem.upload(sidx);
    hx->recv_idx = hx->mem.upload(ridx);
    hx->recv_idx_host = ridx;
    for (int j = 0; j < 3; j++) hx->bdone[j] = make_event(hipEventDisableTiming);
    for (int b = 0; b < HaloExchange::kSets; b++) {
        hx->send_buf[b] = hx->mem.alloc<double>(sidx.size() * 5);
        hx->recv_buf[b] = hx->mem.alloc<double>(ridx.size() * 5);
        hx->packed[b] = make_event(hipEventDisableTiming);
        hx->arrived[b] = make_event(hipEventDisableTiming);
    }
    hx->reduced = make_event(hipEventDisableTiming);
    hx->gathered = make_event(hipEventDisableTiming);
    hx->joined = make_event(hipEventDisableTiming);
    hx->comm_stream = make_stream();
    hx->gmin = hx->mem.alloc<double>(static_cast<size_t>(std::max(world, 1)));
    // tiles next to ghosts: a tile that holds a ghost node, or an owned node with an edge to one
    std::vector<char> boundary(static_cast<size_t>(lv.plan.n_tiles), 0);
    auto tile_of = [&](int64_t original) { return lv.plan.new_of_old[static_cast<size_t>(original)] / kTile; };
    for (int64_t g = lv.n_owned; g < lv.info.nel; g++) boundary[static_cast<size_t>(tile_of(g))] = 1;
    for (int64_t e = lv.info.internal_start; e < lv.info.internal_start + lv.info.n_internal; e++) {
        const mgcfd_edge &E = lv.edges[static_cast<size_t>(e)];
        if (E.a >= lv.n_owned || E.b >= lv.n_owned) { boundary[static_cast<size_t>(tile_of(E.a))] = 1; boundary[static_cast<size_t>(tile_of(E.b))] = 1; }
    }
    std::vector<int32_t> tb, ti;
    for (int32_t t = 0; t < lv.plan.n_tiles; t++) {
        if (lv.plan.ghosts_last && int64_t(t) * kTile >= lv.n_owned) break;      // ghost-only tiles are never launched
        (boundary[static_cast<size_t>(t)] ? tb : ti).push_back(t);
    }
    hx->n_boundary = static_cast<int32_t>(tb.size());
    hx->n_interior = static_cast<int32_t>(ti.size());
    hx->tiles_boundary = hx->mem.upload(tb);
    hx->tiles_interior = hx->mem.upload(ti);
    {
        std::vector<int32_t> all(tb);
        all.insert(all.end(), ti.begin(), ti.end());
        hx->tiles_all = hx->mem.upload(all);
    }
    if (lv.hx) {
        // the old exchange goes: nothing of this rank may still run on it
        HIP_CHECK(hipStreamSynchronize(s->stream));
        HIP_CHECK(hipStreamSynchronize(lv.hx->comm_stream.get()));
    }
    lv.hx = std::move(hx);
}

// the message of the state `field` (the buffer a stage just wrote, or `variables`) in buffer set b: pack, start the transfer
static void halo_start(mgcfd_solver *s, int level, const double *field, int b)
{
    DeviceLevel &lv = s->level(level);
    HaloExchange &hx = *lv.hx;
    mgcfd_comm &c = comm_of(s);
    if (hx.total_send() > 0)
        launch_halo_pack(s->stream, hx.total_send(), lv.dp.stride, hx.send_idx, field, hx.send_buf[b]);
    HIP_CHECK(hipEventRecord(hx.packed[b].get(), s->stream));
    if (c.rccl) {
        HIP_CHECK(hipStreamWaitEvent(hx.comm_stream.get(), hx.packed[b].get(), 0));
        RCCL_CHECK(g_rccl.GroupStart());
        for (size_t k = 0; k < hx.peer.size(); k++) {
            const int64_t ns = hx.send_off[k + 1] - hx.send_off[k], nr = hx.recv_off[k + 1] - hx.recv_off[k];
            if (ns > 0) RCCL_CHECK(g_rccl.Send(hx.send_buf[b] + hx.send_off[k] * 5, static_cast<size_t>(ns) * 5, Rccl::kDouble, hx.peer[k], c.rccl, hx.comm_stream.get()));
            if (nr > 0) RCCL_CHECK(g_rccl.Recv(hx.recv_buf[b] + hx.recv_off[k] * 5, static_cast<size_t>(nr) * 5, Rccl::kDouble, hx.peer[k], c.rccl, hx.comm_stream.get()));
        }
        RCCL_CHECK(g_rccl.GroupEnd());
        HIP_CHECK(hipEventRecord(hx.arrived[b].get(), hx.comm_stream.get()));
    }
    // (in-process group: the copies are issued by group_deliver once every rank has packed)
}

// in-process group: every rank's segments copied into its peers' receive buffers (device to device, over xGMI between
// devices), each destination's copies on its own comm stream behind the sources' pack events
static void deliver_to(mgcfd_group *g, mgcfd_solver *dst, int level, int b, bool behind_own_pack);
static void group_deliver(mgcfd_group *g, int level, int b, bool behind_own_pack = false)
{
    for (mgcfd_solver *dst : g->ranks) deliver_to(g, dst, level, b, behind_own_pack);
}
// the segments the other ranks packed for `dst` into its receive buffer (its comm stream behind the sources' pack events)
static void deliver_to(mgcfd_group *g, mgcfd_solver *dst, int level, int b, bool behind_own_pack)
{
    {
        dst->use_device();
        DeviceLevel &ld = dst->level(level);
        HaloExchange &hd = *ld.hx;
        const int me = comm_of(dst).rank;
        bool any = false;
        // (an exchange outside the sweeps' three-set rotation: the destination's receive buffer is free only behind its own
        //  stream's last unpack, which lies before its pack of this exchange)
        if (behind_own_pack) HIP_CHECK(hipStreamWaitEvent(hd.comm_stream.get(), hd.packed[b].get(), 0));
        for (size_t k = 0; k < hd.peer.size(); k++) {
            mgcfd_solver *src = g->ranks[static_cast<size_t>(hd.peer[k])];
            HaloExchange &hs = *src->level(level).hx;
            const auto it = std::find(hs.peer.begin(), hs.peer.end(), me);
            if (it == hs.peer.end()) throw std::logic_error("halo lists of two ranks do not match");
            const size_t ks = static_cast<size_t>(it - hs.peer.begin());
            const int64_t n = hd.recv_off[k + 1] - hd.recv_off[k];
            if (n != hs.send_off[ks + 1] - hs.send_off[ks]) throw std::logic_error("halo message lengths of two ranks do not match");
            if (n == 0) continue;
            HIP_CHECK(hipStreamWaitEvent(hd.comm_stream.get(), hs.packed[b].get(), 0));
            // (unified addressing + peer access: a plain device-to-device copy crosses xGMI; unlike hipMemcpyPeerAsync it can be captured)
            HIP_CHECK(hipMemcpyAsync(hd.recv_buf[b] + hd.recv_off[k] * 5, hs.send_buf[b] + hs.send_off[ks] * 5,
                                     sizeof(double) * 5 * static_cast<size_t>(n), hipMemcpyDeviceToDevice, hd.comm_stream.get()));
            any = true;
        }
        if (!any) HIP_CHECK(hipStreamWaitEvent(hd.comm_stream.get(), hd.packed[b].get(), 0));     // (keeps the comm stream behind the rank's own stream)
        HIP_CHECK(hipEventRecord(hd.arrived[b].get(), hd.comm_stream.get()));
    }
}

// wait for the message of buffer set b and write it into the ghosts of `field`
static void halo_finish(mgcfd_solver *s, int level, double *field, int b)
{
    DeviceLevel &lv = s->level(level);
    HaloExchange &hx = *lv.hx;
    HIP_CHECK(hipStreamWaitEvent(s->stream, hx.arrived[b].get(), 0));
    if (hx.total_recv() > 0)
        launch_halo_unpack(s->stream, hx.total_recv(), lv.dp.stride, hx.recv_idx, hx.recv_buf[b], field);
}

// (MGCFD_PART_LOOK_AHEAD=0: the last stage of a partitioned sweep does not compute the next sweep's step-factor minima —
//  every sweep then starts with its own k_step_factor_local launch; for A/B measurements)
static bool part_look_ahead()
{
    static const bool on = !(std::getenv("MGCFD_PART_LOOK_AHEAD") && std::atoi(std::getenv("MGCFD_PART_LOOK_AHEAD")) == 0);
    return on;
}

// Does the last stage of a partitioned sweep look ahead?  Under a global time step only — which is what `apply_min` says:
// every caller passes None exactly under a local time step (rank_sweep_once and the group sweeps pass global_dt ? Scalar or
// List : None; rank_sweep_once_ipc sets it under `if (global_dt)`).
static bool part_looks_ahead(ApplyMin apply_min) { return apply_min != ApplyMin::None && part_look_ahead(); }
// How a partitioned sweep's first stage gets the global time step (None: local time step).
struct PartMin { ApplyMin apply = ApplyMin::None; const double *list = nullptr; int n = 0; };
// The arguments of stage j of a partitioned sweep, launched over `tiles`: the time step on the first stage, the residual
// and the look-ahead on the last — there every tile leaves its own minimum over its OWNED nodes (cbrt_vol is +inf on ghosts).
static StageArgs part_stage_args(const DeviceLevel &lv, int j, const PartMin &pm, const int32_t *tiles, int32_t n_tiles)
{
    StageArgs a;
    a.old = lv.q;
    a.tile_list = tiles; a.n_list = n_tiles;
    if (j == 0) { a.apply_min = pm.apply; a.min_list = pm.list; a.n_min = pm.n; }
    if (j == MGCFD_RK - 1) { a.with_residual = true; a.look_ahead = part_looks_ahead(pm.apply); }
    return a;
}
// Before the first launch of a partitioned stage (its input's ghosts are there, or being waited for on the stream)
static void part_stage_begin(mgcfd_solver *s, DeviceLevel &lv, int j)
{
    if (j == 0 && !lv.fluxes_zero) throw std::invalid_argument("a partitioned sweep needs zero fluxes (as after time_step)");
    if (j == 0) s->settle_fluxes(lv);
    s->force_check = s->next_check();                       // all launches of the stage are one time_step for check_for_invalid_variables
}
// ... and behind its last
static void part_stage_end(mgcfd_solver *s, DeviceLevel &lv, int j, const PartMin &pm)
{
    s->force_check = -1;
    if (j == MGCFD_RK - 1) lv.finish_sweep(part_looks_ahead(pm.apply));
}

// One stage of a partitioned sweep on one rank, part 1: the ghosts of the stage's input arrive (the previous stage's
// message), the boundary tiles run, their results are packed and sent.  Part 2 (stage_interior) runs the other tiles
// while the message travels.
static void stage_boundary(mgcfd_solver *s, int level, int j, const PartMin &pm)
{
    DeviceLevel &lv = s->level(level);
    HaloExchange &hx = *lv.hx;
    const StageBuffers b = stage_buffers(lv, j);
    if (j > 0) halo_finish(s, level, b.in, j - 1);
    part_stage_begin(s, lv, j);
    s->op_fused_stage(level, j, b.in, b.out, part_stage_args(lv, j, pm, hx.tiles_boundary, hx.n_boundary));
    lv.stage_out = b.out;
    halo_start(s, level, b.out, j);
}
static void stage_interior(mgcfd_solver *s, int level, int j, const PartMin &pm)
{
    DeviceLevel &lv = s->level(level);
    HaloExchange &hx = *lv.hx;
    const StageBuffers b = stage_buffers(lv, j);
    StageArgs a = part_stage_args(lv, j, pm, hx.tiles_interior, hx.n_interior);
    a.count_iters = false;                                  // (stage_boundary has counted the stage)
    s->op_fused_stage(level, j, b.in, b.out, a);
    part_stage_end(s, lv, j, pm);
}

static void sweep_first_half(mgcfd_solver *s, int level, double *min_out = nullptr)
{
    DeviceLevel &lv = s->level(level);
    if (!lv.hx) throw std::invalid_argument("the level has no halo lists: call mgcfd_rank_set_halo first");
    if (lv.stage_next != 0) throw std::invalid_argument("a sweep is under way (mgcfd_sweep_stage)");
    const bool global_dt = s->global_dt();
    if (global_dt && lv.min_ahead) lv.iters[MGCFD_LOOP_COMPUTE_STEP] += lv.info.nel;      // the previous sweep's last stage looked ahead
    else s->op_step_factor(level, true, false);             // first half of compute_step_factor (a ghost's factor is its owner's business)
    if (global_dt) launch_min_reduce(s->stream, lv.info.nel, lv.partial_min, min_out ? min_out : lv.min_dt);
}

// one sweep of an RCCL rank, as issued (and as captured): every exchange it starts it also finishes
static void rank_sweep_once(mgcfd_solver *s, int level)
{
    mgcfd_comm &c = comm_of(s);
    DeviceLevel &lv = s->level(level);
    const bool global_dt = s->global_dt();
    sweep_first_half(s, level);
    if (global_dt) RCCL_CHECK(g_rccl.AllReduce(lv.min_dt, lv.min_dt, 1, Rccl::kDouble, Rccl::kMin, c.rccl, s->stream));
    PartMin pm;
    if (global_dt) pm.apply = ApplyMin::Scalar;
    for (int j = 0; j < MGCFD_RK; j++) {
        stage_boundary(s, level, j, pm);
        stage_interior(s, level, j, pm);
    }
    halo_finish(s, level, lv.q, MGCFD_RK - 1);              // the ghosts of `variables` are current when the sweep ends
}

// ---- in-process groups, direct mode -------------------------------------------------------------------------------------
// Every rank of a group can store into every other rank's memory (one process: unified addressing, peer access over xGMI),
// so a message needs no buffers: behind its boundary tiles a rank runs ONE k_halo_push that writes the nodes its peers need
// straight into their ghost slots of the buffer the stage writes, and records bdone[stage].  A peer's next stage waits
// for that event before its boundary tiles (the only ones that read ghosts) start.  Ghost slots are written by pushes
// only (the stage launches are told nel = n_owned: the plan numbers ghosts last), so a push may land while the
// receiver's own kernels of that stage still run.  Why nothing is overwritten while somebody may still read it: rank A's
// push of stage j goes into the buffer B's stage j writes, whose ghost slots B last read in the stage before (as that
// stage's input) — and A's boundary tiles of stage j start only behind B's bdone of that earlier stage.
// Per stage and rank: [P event waits] boundary launch, push launch, event record, interior launch — against
// unpack, boundary, pack, record, wait, P copies, record, interior, wait of the buffered form.
// (MGCFD_GROUP_DIRECT=0 keeps the buffered form.)
static bool group_direct_wanted()
{
    // (not together with group graphs, MGCFD_GROUP_GRAPH=1: the capture code joins the buffered form's streams)
    const bool on = !(std::getenv("MGCFD_GROUP_DIRECT") && std::atoi(std::getenv("MGCFD_GROUP_DIRECT")) == 0) &&
                           !(std::getenv("MGCFD_GROUP_GRAPH") && std::atoi(std::getenv("MGCFD_GROUP_GRAPH")) != 0);
    return on;
}

// every rank's two words for its time-step minimum (HaloExchange::min_par) and, on every rank, where all of them lie
static void group_ensure_min_words(mgcfd_group *g, int level)
{
    for (mgcfd_solver *s : g->ranks) {
        HaloExchange &hx = *s->level(level).hx;
        if (hx.min_par) continue;
        s->use_device();
        hx.min_par = hx.mem.alloc<double>(2);
    }
    for (mgcfd_solver *s : g->ranks) {
        HaloExchange &hx = *s->level(level).hx;
        if (hx.peer_scalars[1]) continue;
        s->use_device();
        for (int par = 0; par < 2; par++) {
            std::vector<const double *> ptrs;
            for (mgcfd_solver *src : g->ranks) ptrs.push_back(src->level(level).hx->min_par + par);
            hx.mem.release(hx.peer_scalars[par]);           // (of an earlier call that threw before the second list)
            hx.peer_scalars[par] = hx.mem.upload(ptrs);
        }
    }
}

// build the push targets of every rank (once; allocations and uploads never happen inside a sweep)
static void group_prepare_direct(mgcfd_group *g, int level)
{
    bool possible = group_direct_wanted() && g->peer_ok;   // (a kernel must never store into memory its device cannot address)
    for (mgcfd_solver *s : g->ranks) {
        DeviceLevel &lv = s->level(level);
        if (!lv.hx) throw std::invalid_argument("a rank has no halo lists");
        if (lv.hx->direct) return;                          // (done before)
        if (static_cast<int>(lv.hx->peer.size()) > kMaxPushPeers) possible = false;
        if (lv.n_owned < lv.info.nel && !lv.plan.ghosts_last) possible = false;     // (a plan that mixes ghosts into the tiles: its stages write them)
    }
    if (!possible) return;
    for (mgcfd_solver *src : g->ranks) {
        src->use_device();
        HaloExchange &hs = *src->level(level).hx;
        const int me = comm_of(src).rank;
        std::vector<int32_t> target(static_cast<size_t>(hs.total_send()), 0);
        for (size_t k = 0; k < hs.peer.size(); k++) {
            mgcfd_solver *dst = g->ranks[static_cast<size_t>(hs.peer[k])];
            HaloExchange &hd = *dst->level(level).hx;
            const auto it = std::find(hd.peer.begin(), hd.peer.end(), me);
            if (it == hd.peer.end()) throw std::logic_error("halo lists of two ranks do not match");
            const size_t kd = static_cast<size_t>(it - hd.peer.begin());
            const int64_t n = hs.send_off[k + 1] - hs.send_off[k];
            if (n != hd.recv_off[kd + 1] - hd.recv_off[kd]) throw std::logic_error("halo message lengths of two ranks do not match");
            for (int64_t i = 0; i < n; i++)
                target[static_cast<size_t>(hs.send_off[k] + i)] = hd.recv_idx_host[static_cast<size_t>(hd.recv_off[kd] + i)];
        }
        hs.mem.release(hs.push_target);                     // (of an earlier call that threw at a later rank)
        hs.push_target = hs.mem.upload(target);
    }
    for (mgcfd_solver *s : g->ranks) s->level(level).hx->direct = true;
}

// where a rank's push goes: the buffer `peer_field(peer's level)` of every peer, the peers' segments of the message
template <typename PeerField>
static PushPeers make_push_peers(mgcfd_group *g, mgcfd_solver *s, int level, PeerField &&peer_field)
{
    HaloExchange &hx = *s->level(level).hx;
    PushPeers pp;
    pp.n = static_cast<int>(hx.peer.size());
    for (int k = 0; k < pp.n; k++) {
        DeviceLevel &pl = g->ranks[static_cast<size_t>(hx.peer[static_cast<size_t>(k)])]->level(level);
        pp.base[k] = peer_field(pl);
        pp.stride[k] = pl.dp.stride;
        pp.first[k] = hx.send_off[static_cast<size_t>(k)];
    }
    pp.first[pp.n] = hx.total_send();
    return pp;
}

// the nodes the peers need of `field` (this rank's buffer) into the peers' buffers, then the event
static void push_and_record(mgcfd_solver *s, int level, const double *field, const PushPeers &pp, int ev)
{
    DeviceLevel &lv = s->level(level);
    HaloExchange &hx = *lv.hx;
    if (hx.total_send() > 0) launch_halo_push(s->stream, hx.total_send(), lv.dp.stride, hx.send_idx, hx.push_target, field, pp);
    HIP_CHECK(hipEventRecord(hx.bdone[ev].get(), s->stream));
}

static void wait_for_peers(mgcfd_group *g, mgcfd_solver *s, int level, int ev)
{
    HaloExchange &hx = *s->level(level).hx;
    for (int p : hx.peer) HIP_CHECK(hipStreamWaitEvent(s->stream, g->ranks[static_cast<size_t>(p)]->level(level).hx->bdone[ev].get(), 0));
}

// the time step of an in-process group's sweep: the first stage takes the minimum over the group's minima (hx.gmin)
static PartMin group_min(bool global_dt, const HaloExchange &hx) { return {global_dt ? ApplyMin::List : ApplyMin::None, hx.gmin, 1}; }

// part 1 of a stage in direct mode (part 2 is stage_interior as it is); `to` = where the push goes (nullptr: the peers'
// buffers as they are named now — one host thread drives the group, nobody has rotated since the stage began)
static void stage_boundary_direct(mgcfd_group *g, mgcfd_solver *s, int level, int j, const PartMin &pm, const PushPeers *to = nullptr)
{
    DeviceLevel &lv = s->level(level);
    HaloExchange &hx = *lv.hx;
    const StageBuffers b = stage_buffers(lv, j);
    wait_for_peers(g, s, level, (j + 2) % 3);               // the ghosts of `in`: the peers' pushes of the stage before (stage 0: of the last sweep, or of the exchange)
    part_stage_begin(s, lv, j);
    s->op_fused_stage(level, j, b.in, b.out, part_stage_args(lv, j, pm, hx.tiles_boundary, hx.n_boundary));
    lv.stage_out = b.out;
    push_and_record(s, level, b.out, to ? *to : make_push_peers(g, s, level, [&](DeviceLevel &pl) { return stage_buffers(pl, j).out; }), j);
}

// ---- a host thread per rank ---------------------------------------------------------------------------------------------
// One thread issuing every rank's calls costs the host N x ~67 us per sweep (launches 3.5 us, event records and waits 4-5 us
// each on ROCm) — more than the kernels of a rank take.  In direct mode every rank's calls touch only its own stream, its
// own events and its own solver, so each rank gets a thread of its own.  What the threads must agree on is the ORDER of
// event records and waits (a wait refers to the event's most recent record at the time of the call): a barrier after the
// first half of compute_step_factor and after every stage puts each record ahead of the waits for it.
namespace {
struct SpinBarrier {
    explicit SpinBarrier(int n) : n_(n) {}
    void wait()
    {
        const unsigned gen = gen_.load(std::memory_order_acquire);
        if (count_.fetch_add(1, std::memory_order_acq_rel) + 1 == n_) {
            count_.store(0, std::memory_order_relaxed);
            gen_.fetch_add(1, std::memory_order_release);
        } else {
            for (int spins = 0; gen_.load(std::memory_order_acquire) == gen; spins++)
                if (spins > 4000) std::this_thread::yield();
        }
    }
    std::atomic<int> count_{0};
    std::atomic<unsigned> gen_{0};
    const int n_;
};
}

// `sweeps` sweeps of every rank, a thread per rank (the calling thread takes rank 0).  with_rms: after every sweep each rank
// appends the sum of its owned nodes' squared residuals to its ring (mgcfd_solver::rms_ring) for one read-back at the end.
static void group_sweeps_threaded(mgcfd_group *g, int level, int sweeps, bool with_rms)
{
    const int n = static_cast<int>(g->ranks.size());
    SpinBarrier bar(n);
    std::atomic<bool> failed{false};
    std::mutex mu;
    std::exception_ptr first_error;
    const bool global_dt = g->ranks[0]->global_dt();
    auto run = [&](int r) {
        mgcfd_solver *s = g->ranks[static_cast<size_t>(r)];
        // (a rank that failed keeps arriving at the barriers, doing nothing, so that the others are not left waiting)
        auto step = [&](auto &&body) {
            if (failed.load(std::memory_order_acquire)) return;
            try { body(); }
            catch (...) { std::lock_guard<std::mutex> lock(mu); if (!first_error) first_error = std::current_exception(); failed.store(true, std::memory_order_release); }
        };
        step([&] { s->use_device(); });
        DeviceLevel &lv = s->level(level);
        HaloExchange &hx = *lv.hx;
        for (int k = 0; k < sweeps; k++) {
            const int par = hx.min_parity;
            step([&] {
                sweep_first_half(s, level, hx.min_par + par);
                if (global_dt) HIP_CHECK(hipEventRecord(hx.reduced.get(), s->stream));
            });
            hx.min_parity = par ^ 1;
            bar.wait();
            PushPeers to[MGCFD_RK];
            step([&] {
                if (global_dt) {
                    for (mgcfd_solver *src : g->ranks) if (src != s) HIP_CHECK(hipStreamWaitEvent(s->stream, src->level(level).hx->reduced.get(), 0));
                    launch_min_over_peers(s->stream, hx.peer_scalars[par], n, hx.gmin);
                }
                // the peers' buffers of this sweep's three stages, read while nobody rotates (a rank rotates in its last stage's
                // second part, two barriers from here; its previous rotation lies before the barrier just passed)
                for (int j = 0; j < MGCFD_RK; j++) to[j] = make_push_peers(g, s, level, [&](DeviceLevel &pl) { return stage_buffers(pl, j).out; });
            });
            for (int j = 0; j < MGCFD_RK; j++) {
                step([&] {
                    stage_boundary_direct(g, s, level, j, group_min(global_dt, hx), &to[j]);
                    stage_interior(s, level, j, group_min(global_dt, hx));
                });
                bar.wait();
            }
            if (with_rms) step([&] {
                exact::launch_sumsq(s->stream, lv.info.nel, lv.dp.stride, lv.residuals, lv.partials, lv.n_partials, lv.sumsq, lv.dp.old_of_new, lv.n_owned);
                launch_append_scalar(s->stream, lv.sumsq, s->rms_ring, s->rms_count, mgcfd_solver::kRmsRing);
            });
        }
        step([&] { wait_for_peers(g, s, level, 2); HIP_CHECK(hipGetLastError()); });
    };
    std::vector<std::thread> threads;
    for (int r = 1; r < n; r++) threads.emplace_back(run, r);
    run(0);
    for (std::thread &t : threads) t.join();
    if (first_error) std::rethrow_exception(first_error);
}


// one sweep of every rank of an in-process group
static void group_sweep_once(mgcfd_group *g, int level)
{
    const int n = static_cast<int>(g->ranks.size());
    const bool global_dt = g->ranks[0]->global_dt();
    const int par = g->ranks[0]->level(level).hx->min_parity;       // (the ranks of a group sweep in step)
    for (mgcfd_solver *s : g->ranks) { s->use_device(); HaloExchange &hx = *s->level(level).hx; sweep_first_half(s, level, hx.min_par + par); hx.min_parity = par ^ 1; }
    if (global_dt) {
        // all-reduce(MIN) of one fp64 over the group: behind every rank's reduction event each rank reads the others'
        // scalars itself (k_min_over_peers: 8-byte loads over xGMI) — no message, no second stream
        for (mgcfd_solver *src : g->ranks) { src->use_device(); HIP_CHECK(hipEventRecord(src->level(level).hx->reduced.get(), src->stream)); }
        for (mgcfd_solver *dst : g->ranks) {
            dst->use_device();
            HaloExchange &hd = *dst->level(level).hx;
            for (mgcfd_solver *src : g->ranks) if (src != dst) HIP_CHECK(hipStreamWaitEvent(dst->stream, src->level(level).hx->reduced.get(), 0));
            launch_min_over_peers(dst->stream, hd.peer_scalars[par], n, hd.gmin);
        }
    }
    const bool direct = g->ranks[0]->level(level).hx->direct;
    for (int j = 0; j < MGCFD_RK; j++) {
        for (mgcfd_solver *s : g->ranks) {
            s->use_device();
            if (direct) stage_boundary_direct(g, s, level, j, group_min(global_dt, *s->level(level).hx));
            else stage_boundary(s, level, j, group_min(global_dt, *s->level(level).hx));
        }
        // (set 0 is also the set of the transfers' exchanges, outside the sweeps' rotation: a destination's copies of stage 0 wait
        //  for its OWN pack of this stage, which lies behind its unpack of such an exchange — with the local time step nothing
        //  else orders a peer's stage-0 message behind that unpack; round 3's advisor finding)
        if (!direct) group_deliver(g, level, j, j == 0);
        for (mgcfd_solver *s : g->ranks) { s->use_device(); stage_interior(s, level, j, group_min(global_dt, *s->level(level).hx)); }
    }
    // (direct mode: the last stage's pushes went into the buffer that is `variables` now; whoever reads ghosts next waits for bdone[2])
    if (!direct) for (mgcfd_solver *s : g->ranks) { s->use_device(); halo_finish(s, level, s->level(level).q, MGCFD_RK - 1); }
}

// The sweep as a hipGraph: the ~25 host calls a rank's sweep takes (launches, event records and waits, copies or RCCL
// calls) cost more host time than the kernels take on the GPU; captured once per buffer rotation (the launch arguments
// repeat with period 3) a sweep is ONE host call.  `body` issues the sweep; `streams` beyond the first are forked
// from and joined to the capturing stream.  Returns false (and leaves everything eager) when capture is not possible.
template <typename Body>
static bool capture_sweep(hipStream_t origin, const std::vector<std::pair<hipStream_t, hipEvent_t>> &others, hipEvent_t fork, Body &&body,
                          GraphExec &exec)
{
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(origin, hipStreamCaptureModeRelaxed) != hipSuccess) { (void)hipGetLastError(); return false; }
    bool ok = true;
    try {
        HIP_CHECK(hipEventRecord(fork, origin));
        for (auto &o : others) HIP_CHECK(hipStreamWaitEvent(o.first, fork, 0));
        body();
        for (auto &o : others) { HIP_CHECK(hipEventRecord(o.second, o.first)); HIP_CHECK(hipStreamWaitEvent(origin, o.second, 0)); }
    } catch (...) {
        ok = false;
    }
    if (hipStreamEndCapture(origin, &graph) != hipSuccess || !graph) { (void)hipGetLastError(); ok = false; }
    hipGraphExec_t made = nullptr;
    if (ok && hipGraphInstantiate(&made, graph, nullptr, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); made = nullptr; ok = false; }
    if (graph) (void)hipGraphDestroy(graph);
    exec = adopt_graph_exec(made);
    return ok;
}


// ---- ranks in different processes, direct mode (HIP IPC) -------------------------------------------------------------------
// What the in-process groups do with events, done between processes: every rank publishes IPC handles of its three state
// buffers and of a small array of flag words (mgcfd_rank_ipc_export), opens its neighbours' (mgcfd_rank_ipc_attach), and from
// then on a stage is: k_flags_wait (the neighbours' messages of the stage before have arrived) -> boundary tiles -> ONE
// k_halo_push_flags (stores into the neighbours' ghost slots, then raises their flags) -> interior tiles.  No message
// buffers, no second stream, no RCCL call per stage; the all-reduce of the global time step stays on RCCL.
// Opt-in (bench.py --exchange ipc): it could be rehearsed with two processes on ONE GPU only (tests/test_gpu_configs.py).
namespace {
struct IpcExportHeader {
    hipIpcMemHandle_t state[3], flags, gmins;
    int64_t stride, n_recv;
    int32_t rot, rank, n_peers, reserved;
    int32_t peers[kMaxPushPeers];
    int64_t recv_off[kMaxPushPeers + 1];
};
}

static void ipc_wait(mgcfd_solver *s, HaloExchange &hx, int slot)
{
    FlagRows rows;
    rows.n = static_cast<int>(hx.peer.size());
    for (int k = 0; k < rows.n; k++) rows.row[k] = hx.peer[static_cast<size_t>(k)];       // (a rank's row is its rank)
    launch_flags_wait(s->stream, hx.flags, rows, slot, hx.seq, hx.ipc_timeouts);
}

// all-reduce(MIN) of lv.min_dt over every rank through the flags: the minima end up in hx.gmins[parity][0..world)
static const double *ipc_allreduce_min(mgcfd_solver *s, DeviceLevel &lv)
{
    HaloExchange &hx = *lv.hx;
    const mgcfd_comm &c = comm_of(s);
    MinPublish mp;
    mp.world = c.world; mp.me = c.rank;
    mp.parity = static_cast<int>(hx.sweep_seq & 1ull);
    hx.sweep_seq++;
    mp.value = hx.sweep_seq;
    FlagRows rows;
    for (int r = 0; r < c.world; r++) {
        mp.mins[r] = hx.all_mins[r];
        mp.flag[r] = hx.all_flag[r];
        if (r != c.rank) rows.row[rows.n++] = r;
    }
    launch_min_publish(s->stream, lv.min_dt, mp);
    launch_flags_wait(s->stream, hx.flags, rows, 3, hx.sweep_seq, hx.ipc_timeouts);
    return hx.gmins + mp.parity * kMaxIpcRanks;
}

// this rank's nodes of `field` into the peers' buffers state[(rot + which) % 3] (which: 0 variables, 1 q_alt, 2 old_variables,
// by the PEER's numbering of its buffers), flag word `slot`
static void ipc_push(mgcfd_solver *s, DeviceLevel &lv, const double *field, int which, int slot)
{
    HaloExchange &hx = *lv.hx;
    PushPeers pp;
    PushFlags pf;
    pp.n = pf.n = static_cast<int>(hx.peer.size());
    for (int k = 0; k < pp.n; k++) {
        pp.base[k] = hx.peer_state[k][(lv.rot + hx.peer_rot_delta[k] + which) % 3];
        pp.stride[k] = hx.peer_stride[k];
        pp.first[k] = hx.send_off[static_cast<size_t>(k)];
        pf.flag[k] = hx.peer_flag[k] + slot;
    }
    pp.first[pp.n] = hx.total_send();
    hx.seq++;
    pf.value = hx.seq;
    launch_halo_push_flags(s->stream, hx.total_send(), lv.dp.stride, hx.send_idx, hx.push_target, field, pp, pf, hx.ticket);
}

static void rank_sweep_once_ipc(mgcfd_solver *s, int level)
{
    mgcfd_comm &c = comm_of(s);
    DeviceLevel &lv = s->level(level);
    HaloExchange &hx = *lv.hx;
    const bool global_dt = s->global_dt();
    if (global_dt && !c.rccl && !hx.ipc_all) throw std::invalid_argument("a global time step needs the all-reduce: attach every rank (mgcfd_rank_ipc_attach with all exports) or RCCL");
    sweep_first_half(s, level);
    // the time step: over the flags when every rank is attached (the ranks' minima side by side, the first stage takes their
    // minimum), else RCCL's all-reduce into the scalar
    PartMin pm;
    if (global_dt) {
        if (hx.ipc_all) pm = PartMin{ApplyMin::List, ipc_allreduce_min(s, lv), c.world};
        else { RCCL_CHECK(g_rccl.AllReduce(lv.min_dt, lv.min_dt, 1, Rccl::kDouble, Rccl::kMin, c.rccl, s->stream)); pm.apply = ApplyMin::Scalar; }
    }
    for (int j = 0; j < MGCFD_RK; j++) {
        const StageBuffers b = stage_buffers(lv, j);
        const int which = j == 1 ? 2 : 1;                   // (before the rotation: stage 1 writes old_variables' buffer, stages 0 and 2 q_alt's)
        ipc_wait(s, hx, (j + 2) % 3);                       // the ghosts of `in`: the peers' pushes of the stage before (stage 0: of the last sweep, or of the exchange)
        part_stage_begin(s, lv, j);
        lv.stage_out = b.out;
        if (s->opt_rank_split == 2 && hx.n_boundary > 0) {
            // MGCFD_OPT_RANK_SPLIT = 2: ONE launch per stage that sends its own message — the boundary tiles first, their
            // epilogue stores into the neighbours, the last of them raises the flags, the interior tiles run on meanwhile
            StagePush sp;
            sp.send_ptr = hx.node_send_ptr; sp.send_peer = hx.node_send_peer; sp.send_target = hx.node_send_target;
            sp.ticket = hx.ticket; sp.n_boundary = hx.n_boundary;
            sp.peers.n = sp.flags.n = static_cast<int>(hx.peer.size());
            for (int k = 0; k < sp.peers.n; k++) {
                sp.peers.base[k] = hx.peer_state[k][(lv.rot + hx.peer_rot_delta[k] + which) % 3];
                sp.peers.stride[k] = hx.peer_stride[k];
                sp.flags.flag[k] = hx.peer_flag[k] + j;
            }
            hx.seq++;
            sp.flags.value = hx.seq;
            StageArgs a = part_stage_args(lv, j, pm, hx.tiles_all, hx.n_boundary + hx.n_interior);
            a.push = &sp;
            s->op_fused_stage(level, j, b.in, b.out, a);
            part_stage_end(s, lv, j, pm);
        } else if (s->opt_rank_split) {
            s->op_fused_stage(level, j, b.in, b.out, part_stage_args(lv, j, pm, hx.tiles_boundary, hx.n_boundary));
            ipc_push(s, lv, b.out, which, j);
            stage_interior(s, level, j, pm);
        } else {
            // MGCFD_OPT_RANK_SPLIT = 0: every tile of the rank in one launch, the message behind it
            s->op_fused_stage(level, j, b.in, b.out, part_stage_args(lv, j, pm, hx.tiles_all, hx.n_boundary + hx.n_interior));
            ipc_push(s, lv, b.out, which, j);
            part_stage_end(s, lv, j, pm);
        }
    }
}

extern "C" {

int mgcfd_rccl_unique_id(void *out128)
{
    REQUIRE(out128);
    return guarded([&] { rccl_load(); RCCL_CHECK(g_rccl.GetUniqueId(out128)); });
}

int mgcfd_rank_attach_rccl(mgcfd_solver *s, int rank, int world, const void *id128)
{
    REQUIRE(s); REQUIRE(id128);
    return guarded([&] {
        if (rank < 0 || rank >= world) throw std::invalid_argument("rank out of range");
        require_no_smoothing(s, "mgcfd_rank_attach_rccl");
        require_default_cycle(s, "mgcfd_rank_attach_rccl");
        s->use_device();
        rccl_load();
        Rccl::Id id;
        std::memcpy(id.b, id128, sizeof(id.b));
        mgcfd_comm c;
        c.rank = rank; c.world = world;
        RCCL_CHECK(g_rccl.CommInitRank(&c.rccl, world, id, rank));
        s->comm = c;
    });
}

// a rank of `world` processes without an RCCL communicator: enough for a level with a local time step (mesh_name = fvcorr),
// whose sweeps need no all-reduce, once the neighbours' buffers are attached (mgcfd_rank_ipc_attach)
int mgcfd_rank_attach_plain(mgcfd_solver *s, int rank, int world)
{
    REQUIRE(s);
    return guarded([&] {
        if (rank < 0 || rank >= world) throw std::invalid_argument("rank out of range");
        require_no_smoothing(s, "mgcfd_rank_attach_plain");
        require_default_cycle(s, "mgcfd_rank_attach_plain");
        mgcfd_comm c;
        c.rank = rank; c.world = world;
        s->comm = c;
    });
}

int mgcfd_rank_ipc_export_size(mgcfd_solver *s, int level, int64_t *bytes)
{
    REQUIRE(s); REQUIRE(bytes);
    return guarded([&] {
        DeviceLevel &lv = s->level(level);
        if (!lv.hx) throw std::invalid_argument("the level has no halo lists: call mgcfd_rank_set_halo first");
        *bytes = static_cast<int64_t>(sizeof(IpcExportHeader) + sizeof(int32_t) * lv.hx->recv_idx_host.size());
    });
}

int mgcfd_rank_ipc_export(mgcfd_solver *s, int level, void *out)
{
    REQUIRE(s); REQUIRE(out);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        if (!lv.hx) throw std::invalid_argument("the level has no halo lists: call mgcfd_rank_set_halo first");
        HaloExchange &hx = *lv.hx;
        if (static_cast<int>(hx.peer.size()) > kMaxPushPeers) throw std::invalid_argument("more neighbouring ranks than a push addresses (8)");
        if (lv.n_owned < lv.info.nel && !lv.plan.ghosts_last) throw std::invalid_argument("the level's plan mixes ghosts into the tiles");
        if (!hx.flags) {
            // the words other devices write and this one polls; made under an owner of their own, so that a failure leaves
            // the exchange without any of them
            DeviceOwner made;
            auto *flags = static_cast<unsigned long long *>(made.alloc_fine_grained(sizeof(unsigned long long) * kMaxIpcRanks * 4));
            HIP_CHECK(hipMemset(flags, 0, sizeof(unsigned long long) * kMaxIpcRanks * 4));
            auto *gmins = static_cast<double *>(made.alloc_fine_grained(sizeof(double) * 2 * kMaxIpcRanks));
            const std::vector<double> inf(2 * kMaxIpcRanks, std::numeric_limits<double>::infinity());
            HIP_CHECK(hipMemcpy(gmins, inf.data(), sizeof(double) * inf.size(), hipMemcpyHostToDevice));
            auto *ticket = made.alloc<unsigned>(1);
            HIP_CHECK(hipMemset(ticket, 0, sizeof(unsigned)));
            auto *timeouts = made.alloc<int>(1);
            HIP_CHECK(hipMemset(timeouts, 0, sizeof(int)));
            hx.mem.absorb(std::move(made));
            hx.flags = flags; hx.gmins = gmins; hx.ticket = ticket; hx.ipc_timeouts = timeouts;
        }
        IpcExportHeader h{};
        for (int k = 0; k < 3; k++) HIP_CHECK(hipIpcGetMemHandle(&h.state[k], lv.state[k]));
        HIP_CHECK(hipIpcGetMemHandle(&h.flags, hx.flags));
        HIP_CHECK(hipIpcGetMemHandle(&h.gmins, hx.gmins));
        if (comm_of(s).world > kMaxIpcRanks) throw std::invalid_argument("more ranks than flag rows (16)");
        h.stride = lv.dp.stride;
        h.n_recv = static_cast<int64_t>(hx.recv_idx_host.size());
        h.rot = lv.rot % 3;
        h.rank = comm_of(s).rank;
        h.n_peers = static_cast<int32_t>(hx.peer.size());
        for (size_t k = 0; k < hx.peer.size(); k++) h.peers[k] = hx.peer[k];
        for (size_t k = 0; k <= hx.peer.size(); k++) h.recv_off[k] = hx.recv_off[k];
        std::memcpy(out, &h, sizeof(h));
        std::memcpy(static_cast<char *>(out) + sizeof(h), hx.recv_idx_host.data(), sizeof(int32_t) * hx.recv_idx_host.size());
    });
}

// exports: what other ranks exported, in any order — at least every neighbouring rank's (mgcfd_rank_set_halo's peers); with
// EVERY other rank's the all-reduce of a global time step goes through the flags as well and no RCCL call is left in a sweep
int mgcfd_rank_ipc_attach(mgcfd_solver *s, int level, int n_exports, const void *const *exports)
{
    REQUIRE(s);
    if (n_exports > 0) REQUIRE(exports);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        if (!lv.hx || !lv.hx->flags) throw std::invalid_argument("export this rank's buffers first (mgcfd_rank_ipc_export)");
        HaloExchange &hx = *lv.hx;
        const mgcfd_comm &c = comm_of(s);
        const int me = c.rank;
        std::vector<int32_t> target(static_cast<size_t>(hx.total_send()), 0);
        std::vector<char> peer_seen(hx.peer.size(), 0), rank_seen(static_cast<size_t>(c.world), 0);
        auto open = [&](const hipIpcMemHandle_t &h) {
            hx.ipc_opened.push_back(open_ipc_mapping(h));
            return hx.ipc_opened.back().get();
        };
        for (int e = 0; e < n_exports; e++) {
            IpcExportHeader h;
            std::memcpy(&h, exports[e], sizeof(h));
            if (h.rank == me) continue;
            if (h.rank < 0 || h.rank >= c.world || rank_seen[static_cast<size_t>(h.rank)]) throw std::invalid_argument("an export of an unknown rank, or of one rank twice");
            rank_seen[static_cast<size_t>(h.rank)] = 1;
            unsigned long long *their_flags = static_cast<unsigned long long *>(open(h.flags));
            hx.all_flag[h.rank] = their_flags + me * 4 + 3;
            hx.all_mins[h.rank] = static_cast<double *>(open(h.gmins));
            const auto it = std::find(hx.peer.begin(), hx.peer.end(), h.rank);
            if (it == hx.peer.end()) continue;              // (not a neighbour: only the all-reduce talks to it)
            const size_t k = static_cast<size_t>(it - hx.peer.begin());
            peer_seen[k] = 1;
            int kd = -1;
            for (int q = 0; q < h.n_peers; q++) if (h.peers[q] == me) kd = q;
            if (kd < 0) throw std::logic_error("halo lists of two ranks do not match");
            const int64_t n = hx.send_off[k + 1] - hx.send_off[k];
            if (n != h.recv_off[kd + 1] - h.recv_off[kd]) throw std::logic_error("halo message lengths of two ranks do not match");
            const int32_t *ridx = reinterpret_cast<const int32_t *>(static_cast<const char *>(exports[e]) + sizeof(h));
            for (int64_t i = 0; i < n; i++) target[static_cast<size_t>(hx.send_off[k] + i)] = ridx[h.recv_off[kd] + i];
            for (int b = 0; b < 3; b++) hx.peer_state[k][b] = static_cast<double *>(open(h.state[b]));
            hx.peer_flag[k] = their_flags + me * 4;
            hx.peer_stride[k] = h.stride;
            hx.peer_rot_delta[k] = ((h.rot - lv.rot % 3) % 3 + 3) % 3;
        }
        for (char seen : peer_seen) if (!seen) throw std::invalid_argument("the export of a neighbouring rank is missing");
        hx.all_mins[me] = hx.gmins;
        hx.all_flag[me] = hx.flags + me * 4 + 3;            // (never raised: a rank does not wait for itself)
        int others = 0;
        for (char seen : rank_seen) others += seen;
        hx.ipc_all = others == c.world - 1;
        hx.mem.release(hx.push_target);
        hx.push_target = hx.mem.upload(target);
        {   // the same message per node (library numbering): what a stage that sends its own message walks (StagePush)
            std::vector<int32_t> sidx(static_cast<size_t>(hx.total_send()));
            HIP_CHECK(hipMemcpy(sidx.data(), hx.send_idx, sizeof(int32_t) * sidx.size(), hipMemcpyDeviceToHost));
            std::vector<int32_t> ptr(static_cast<size_t>(lv.dp.stride) + 2, 0), tgt(sidx.size());
            std::vector<int8_t> peer(sidx.size());
            for (int32_t n : sidx) ptr[static_cast<size_t>(n) + 1]++;
            for (size_t n = 1; n < ptr.size(); n++) ptr[n] += ptr[n - 1];
            std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
            for (size_t k = 0; k < hx.peer.size(); k++)
                for (int64_t m = hx.send_off[k]; m < hx.send_off[k + 1]; m++) {
                    const int32_t at = fill[static_cast<size_t>(sidx[static_cast<size_t>(m)])]++;
                    peer[static_cast<size_t>(at)] = static_cast<int8_t>(k);
                    tgt[static_cast<size_t>(at)] = target[static_cast<size_t>(m)];
                }
            hx.mem.release(hx.node_send_ptr);
            hx.mem.release(hx.node_send_target);
            hx.mem.release(hx.node_send_peer);
            hx.node_send_ptr = hx.mem.upload(ptr);
            if (tgt.empty()) { tgt.push_back(0); peer.push_back(0); }
            hx.node_send_target = hx.mem.upload(tgt);
            hx.node_send_peer = hx.mem.upload(peer);
        }
        hx.ipc = true;
    });
}

// back to the buffered form (RCCL send / receive): the neighbours' mappings are closed.  Synchronises.
int mgcfd_rank_ipc_detach(mgcfd_solver *s, int level)
{
    REQUIRE(s);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        if (!lv.hx || !lv.hx->ipc) return;
        HaloExchange &hx = *lv.hx;
        HIP_CHECK(hipStreamSynchronize(s->stream));
        hx.ipc_opened.clear();
        hx.ipc = false;
        hx.ipc_all = false;
        hx.ipc_unacknowledged = false;
        if (hx.ipc_timeouts) HIP_CHECK(hipMemset(hx.ipc_timeouts, 0, sizeof(int)));
    });
}

// how many waits for a neighbour's message gave up since the last call (0: every message arrived).  Synchronises.
int mgcfd_rank_ipc_status(mgcfd_solver *s, int level, int *timed_out)
{
    REQUIRE(s); REQUIRE(timed_out);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        *timed_out = 0;
        if (!lv.hx || !lv.hx->ipc) return;
        HIP_CHECK(hipMemcpyAsync(timed_out, lv.hx->ipc_timeouts, sizeof(int), hipMemcpyDeviceToHost, s->stream));
        HIP_CHECK(hipMemsetAsync(lv.hx->ipc_timeouts, 0, sizeof(int), s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
        lv.hx->ipc_unacknowledged = false;
    });
}

int mgcfd_rank_detach(mgcfd_solver *s)
{
    REQUIRE(s);
    return guarded([&] {
        if (!s->comm) return;
        if (s->comm->rccl) { s->use_device(); (void)hipStreamSynchronize(s->stream); (void)g_rccl.CommDestroy(s->comm->rccl); }
        s->comm.reset();
    });
}

int mgcfd_rank_set_halo(mgcfd_solver *s, int level, int n_peers, const int *peers, const int64_t *send_counts, const int64_t *const *send_ids,
                        const int64_t *recv_counts, const int64_t *const *recv_ids)
{
    REQUIRE(s);
    if (n_peers > 0) { REQUIRE(peers); REQUIRE(send_counts); REQUIRE(send_ids); REQUIRE(recv_counts); REQUIRE(recv_ids); }
    return guarded([&] { build_halo(s, level, n_peers, peers, send_counts, send_ids, recv_counts, recv_ids, comm_of(s).world); });
}

// what a replayed sweep leaves behind on the host side (the captured launches carry their arguments; the flags and
// counters the eager path updates as it goes are advanced here)
static void after_replayed_sweep(mgcfd_solver *s, int level, const int64_t *iters_delta)
{
    DeviceLevel &lv = s->level(level);
    lv.finish_sweep(s->global_dt() && part_look_ahead());    // (as stage_interior leaves it)
    lv.stage_out = lv.q;                            // (the replayed stages did not name it)
    for (int k = 0; k < MGCFD_NUM_LOOPS; k++) lv.iters[k] += iters_delta[k];
}

// (MGCFD_SWEEP_GRAPH=0 switches every captured partitioned sweep off, whatever the solvers' MGCFD_OPT_GRAPH says)
static bool sweep_graphs_enabled()
{
    static const bool on = !(std::getenv("MGCFD_SWEEP_GRAPH") && std::atoi(std::getenv("MGCFD_SWEEP_GRAPH")) == 0);
    return on;
}

// Bring the ghosts of `variables` up to date (after mgcfd_set_array, before the first sweep).  In an in-process group
// call mgcfd_group_exchange instead.
int mgcfd_rank_exchange(mgcfd_solver *s, int level)
{
    OP({
        DeviceLevel &lv = s->level(level);
        if (!lv.hx) throw std::invalid_argument("the level has no halo lists");
        if (lv.hx->ipc) {
            // direct mode between processes: behind whatever the peers still read of the last sweep, this rank's owned
            // `variables` into their ghost slots; the rank's own stream goes on behind the messages INTO it
            s->settle_residuals(lv);
            ipc_wait(s, *lv.hx, 2);
            ipc_push(s, lv, lv.q, 0, 2);
            ipc_wait(s, *lv.hx, 2);
            lv.min_ahead = false;
            return;
        }
        if (!comm_of(s).rccl) throw std::invalid_argument("in-process ranks exchange through mgcfd_group_exchange");
        halo_start(s, level, lv.q, 0);
        halo_finish(s, level, lv.q, 0);
        lv.min_ahead = false;
    });
}

int mgcfd_rank_sweeps(mgcfd_solver *s, int level, int sweeps)
{
    OP({
        mgcfd_comm &c = comm_of(s);
        DeviceLevel &lv = s->level(level);
        if (!lv.hx) throw std::invalid_argument("the level has no halo lists: call mgcfd_rank_set_halo first");
        HaloExchange &hx = *lv.hx;
        s->settle_fluxes(lv);                               // (outside any capture: a lazy zero is not part of a sweep)
        if (hx.ipc) {
            if (hx.ipc_unacknowledged) throw HipError("a wait for a neighbouring rank's message gave up earlier and nobody has asked mgcfd_rank_ipc_status since: no further sweeps on stale ghosts");
            for (int k = 0; k < sweeps; k++) rank_sweep_once_ipc(s, level);
            ipc_wait(s, hx, 2);                             // (the ghosts of `variables` are complete in this rank's stream order)
            return;
        }
        if (!c.rccl) throw std::invalid_argument("in-process ranks sweep through mgcfd_group_sweeps");
        for (int k = 0; k < sweeps; k++) {
            const int rot = lv.rot % 3;
            // MGCFD_OPT_GRAPH = 1: the sweep replayed from a hipGraph (measured with the one rank a one-GPU box offers: 76 us
            // per sweep against 129 us issued call by call; ncclSend/ncclRecv inside a capture could not be rehearsed
            // there, hence opt-in)
            // (global time step: a sweep is captured / replayed only from a looked-ahead state — the steady state; the first
            //  sweep after an exchange, which still runs k_step_factor_local, goes out eagerly)
            const bool steady = !s->global_dt() || lv.min_ahead || !part_look_ahead();
            if (s->opt_graph && sweep_graphs_enabled() && !hx.graph_failed && s->opt_timing == 0 && steady) {
                if (!hx.sweep_graph[rot]) {
                    const bool ahead_before = lv.min_ahead;
                    int64_t before[MGCFD_NUM_LOOPS];
                    std::memcpy(before, lv.iters, sizeof(before));
                    const int rot_before = lv.rot;
                    const bool ok = capture_sweep(s->stream, {}, hx.joined.get(), [&] { rank_sweep_once(s, level); }, hx.sweep_graph[rot]);
                    s->force_check = -1;
                    if (!ok) {                              // nothing ran: put the host state back and go on eagerly
                        hx.graph_failed = true;
                        lv.rot = rot_before; lv.apply_rot();
                        lv.min_ahead = ahead_before;
                        std::memcpy(lv.iters, before, sizeof(before));
                        rank_sweep_once(s, level);
                        continue;
                    }
                    for (int q = 0; q < MGCFD_NUM_LOOPS; q++) { hx.graph_iters[rot][q] = lv.iters[q] - before[q]; lv.iters[q] = before[q]; }
                    lv.rot = rot_before; lv.apply_rot();    // (the capture advanced the host state without running anything)
                    lv.min_ahead = ahead_before;
                }
                HIP_CHECK(hipGraphLaunch(hx.sweep_graph[rot].get(), s->stream));
                hx.sweeps_replayed++;
                after_replayed_sweep(s, level, hx.graph_iters[rot]);
            } else {
                rank_sweep_once(s, level);
            }
        }
    });
}

// calc_rms over a partitioned level (src/Kernels/validation.cpp:91-105): the sum of squared residuals over the OWNED nodes
// of every rank (all-reduce SUM of one fp64); rms = sqrt(sum / nodes of the whole level).  Synchronises.
int mgcfd_rank_residual_sumsq(mgcfd_solver *s, int level, double *sum_all_ranks)
{
    REQUIRE(sum_all_ranks);
    OP({
        mgcfd_comm &c = comm_of(s);
        if (!c.rccl) throw std::invalid_argument("in-process ranks: mgcfd_group_rms");
        DeviceLevel &lv = s->level(level);
        if (!lv.hx) throw std::invalid_argument("the level has no halo lists");
        exact::launch_sumsq(s->stream, lv.info.nel, lv.dp.stride, lv.residuals, lv.partials, lv.n_partials, lv.sumsq, lv.dp.old_of_new, lv.n_owned);
        RCCL_CHECK(g_rccl.AllReduce(lv.sumsq, lv.hx->gmin, 1, Rccl::kDouble, Rccl::kSum, c.rccl, s->stream));
        HIP_CHECK(hipMemcpyAsync(sum_all_ranks, lv.hx->gmin, sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
    });
}

// ---- in-process groups: the ranks are solvers of this process (one per device — or several on one device in tests) ----
int mgcfd_group_create(int n, mgcfd_solver *const *solvers, mgcfd_group **out)
{
    REQUIRE(solvers); REQUIRE(out);
    return guarded([&] {
        if (n < 1) throw std::invalid_argument("a group needs at least one rank");
        auto g = std::make_unique<mgcfd_group>();
        for (int r = 0; r < n; r++) {
            if (!solvers[r]) throw std::invalid_argument("null solver");
            require_no_smoothing(solvers[r], "mgcfd_group_create");
            require_default_cycle(solvers[r], "mgcfd_group_create");
            g->ranks.push_back(solvers[r]);
        }
        // peer access between the devices of the group (xGMI): a copy between two devices then goes direct
        for (int a = 0; a < n; a++)
            for (int b = 0; b < n; b++) {
                if (solvers[a]->device == solvers[b]->device) continue;
                int can = 0;
                HIP_CHECK(hipDeviceCanAccessPeer(&can, solvers[a]->device, solvers[b]->device));
                if (can) { solvers[a]->use_device(); const hipError_t e = hipDeviceEnablePeerAccess(solvers[b]->device, 0); if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIP_CHECK(e); (void)hipGetLastError(); }
                else g->peer_ok = false;
            }
        // the group's all-reduce reads the other ranks' scalars in place and its messages are stores into the peers' memory:
        // a kernel must never touch memory its device cannot address, so such a set of devices is refused here
        if (!g->peer_ok) throw std::invalid_argument("the devices of an in-process group must have peer access to each other (use one rank per process over RCCL instead)");
        for (int r = 0; r < n; r++) {
            mgcfd_comm c;
            c.rank = r; c.world = n; c.group = g.get();
            solvers[r]->comm = c;
        }
        *out = g.release();
    });
}

void mgcfd_group_destroy(mgcfd_group *g)
{
    if (!g) return;
    for (mgcfd_solver *s : g->ranks) if (s && s->comm && s->comm->group == g) s->comm.reset();
    delete g;
}

int mgcfd_group_set_free_stream(mgcfd_group *g, double mach, double alpha_deg, int reinitialise)
{
    REQUIRE(g);
    double ff17[17];
    const int rc = mgcfd_free_stream_constants(mach, alpha_deg, ff17);      // (a bad argument changes no rank)
    if (rc != MGCFD_OK) return rc;
    return guarded([&] {
        for (mgcfd_solver *s : g->ranks) require_no_sweep_under_way(s);     // (... nor does a sweep under way on any of them)
        // one pass that leaves every rank idle and without graphs (rank 0 keeps the group's sweep graph), then one that sets them
        for (mgcfd_solver *s : g->ranks) {
            s->use_device();
            s->fold_events();
            HIP_CHECK(hipStreamSynchronize(s->stream));
            for (DeviceLevel &lv : s->L) if (lv.hx) HIP_CHECK(hipStreamSynchronize(lv.hx->comm_stream.get()));
            s->drop_graphs();
        }
        for (mgcfd_solver *s : g->ranks) apply_free_stream(s, ff17, mach, alpha_deg, reinitialise);
    });
}

int mgcfd_group_set_time_step(mgcfd_group *g, int mode, double cfl)
{
    REQUIRE(g);
    return guarded([&] {
        check_time_step(mode, cfl);                                         // (a bad argument changes no rank)
        for (mgcfd_solver *s : g->ranks) require_no_sweep_under_way(s, "time step");
        for (mgcfd_solver *s : g->ranks) {                                  // as mgcfd_group_set_free_stream: all idle and without graphs, then set
            s->use_device();
            s->fold_events();
            HIP_CHECK(hipStreamSynchronize(s->stream));
            for (DeviceLevel &lv : s->L) if (lv.hx) HIP_CHECK(hipStreamSynchronize(lv.hx->comm_stream.get()));
            s->drop_graphs();
        }
        for (mgcfd_solver *s : g->ranks) apply_time_step(s, mode, cfl);
    });
}

int mgcfd_group_exchange(mgcfd_group *g, int level)
{
    REQUIRE(g);
    return guarded([&] {
        for (mgcfd_solver *s : g->ranks) if (!s->level(level).hx) throw std::invalid_argument("a rank has no halo lists");
        group_prepare_direct(g, level);
        if (g->ranks[0]->level(level).hx->direct) {
            // every rank's owned `variables` into its peers' ghost slots; a peer's stream continues behind the pushes into it
            for (mgcfd_solver *s : g->ranks) {
                s->use_device();
                DeviceLevel &lv = s->level(level);
                s->settle_residuals(lv);
                wait_for_peers(g, s, level, 2);             // (nobody still reads the ghosts a peer is about to overwrite: their last sweep's last stage is behind this)
                push_and_record(s, level, lv.q, make_push_peers(g, s, level, [](DeviceLevel &pl) { return pl.q; }), 2);
                lv.min_ahead = false;
            }
            for (mgcfd_solver *s : g->ranks) { s->use_device(); wait_for_peers(g, s, level, 2); }
            return;
        }
        for (mgcfd_solver *s : g->ranks) { s->use_device(); DeviceLevel &lv = s->level(level); halo_start(s, level, lv.q, 0); }
        group_deliver(g, level, 0);
        for (mgcfd_solver *s : g->ranks) { s->use_device(); DeviceLevel &lv = s->level(level); halo_finish(s, level, lv.q, 0); lv.min_ahead = false; }
    });
}

// rms_out (may be null): the RMS after each of the `sweeps` sweeps, read back once at the end (direct mode only)
static int group_sweeps_impl(mgcfd_group *g, int level, int sweeps, double *rms_out)
{
    REQUIRE(g);
    return guarded([&] {
        if (rms_out && sweeps > mgcfd_solver::kRmsRing) throw std::invalid_argument("at most 4096 sweeps per call with the RMS of each");
        group_require_same_free_stream(g);
        group_require_same_time_step(g);
        mgcfd_solver *s0 = g->ranks[0];
        for (mgcfd_solver *s : g->ranks) {
            s->use_device();
            DeviceLevel &lv = s->level(level);
            if (!lv.hx) throw std::invalid_argument("a rank has no halo lists: call mgcfd_rank_set_halo first");
            s->settle_fluxes(lv);
        }
        group_ensure_min_words(g, level);               // (allocations and uploads: never inside a capture)
        group_prepare_direct(g, level);
        HaloExchange &h0 = *s0->level(level).hx;
        bool timing = false;
        for (mgcfd_solver *s : g->ranks) timing = timing || s->opt_timing != 0;
        // direct mode: a host thread per rank (MGCFD_GROUP_THREADS=0: one thread issues everything, for A/B)
        const bool threads_wanted = !(std::getenv("MGCFD_GROUP_THREADS") && std::atoi(std::getenv("MGCFD_GROUP_THREADS")) == 0);
        if (rms_out && !h0.direct) {
            // the buffered form: the RMS read back after every sweep (as mgcfd_group_rms does it)
            for (int k = 0; k < sweeps; k++) {
                group_sweep_once(g, level);
                double sum = 0.0;
                int64_t nodes = 0;
                for (mgcfd_solver *s : g->ranks) {
                    s->use_device();
                    DeviceLevel &lv = s->level(level);
                    exact::launch_sumsq(s->stream, lv.info.nel, lv.dp.stride, lv.residuals, lv.partials, lv.n_partials, lv.sumsq, lv.dp.old_of_new, lv.n_owned);
                    double part = 0.0;
                    HIP_CHECK(hipMemcpyAsync(&part, lv.sumsq, sizeof(double), hipMemcpyDeviceToHost, s->stream));
                    HIP_CHECK(hipStreamSynchronize(s->stream));
                    sum += part;
                    nodes += lv.n_owned;
                }
                rms_out[k] = std::sqrt(sum / double(nodes));
            }
            return;
        }
        // (the threads are started per call — ~50 us — so a call of one or two sweeps is issued by the caller's thread alone)
        const bool threaded = threads_wanted && g->ranks.size() > 1 && sweeps >= 4;
        if (h0.direct && (rms_out || threaded)) {
            if (rms_out)
                for (mgcfd_solver *s : g->ranks) {
                    s->use_device();
                    ensure_rms_ring(s);
                    HIP_CHECK(hipMemsetAsync(s->rms_count, 0, sizeof(int), s->stream));
                }
            if (threaded) group_sweeps_threaded(g, level, sweeps, rms_out != nullptr);
            else {
                for (int k = 0; k < sweeps; k++) {
                    group_sweep_once(g, level);
                    if (rms_out)
                        for (mgcfd_solver *s : g->ranks) {
                            s->use_device();
                            DeviceLevel &lv = s->level(level);
                            exact::launch_sumsq(s->stream, lv.info.nel, lv.dp.stride, lv.residuals, lv.partials, lv.n_partials, lv.sumsq, lv.dp.old_of_new, lv.n_owned);
                            launch_append_scalar(s->stream, lv.sumsq, s->rms_ring, s->rms_count, mgcfd_solver::kRmsRing);
                        }
                }
                for (mgcfd_solver *s : g->ranks) { s->use_device(); wait_for_peers(g, s, level, 2); }
            }
            if (rms_out) {
                // one read-back: the ranks' sums of every sweep, added in rank order as mgcfd_group_rms adds them
                std::vector<double> sums(static_cast<size_t>(sweeps), 0.0), part(static_cast<size_t>(sweeps));
                int64_t nodes = 0;
                for (mgcfd_solver *s : g->ranks) {
                    s->use_device();
                    HIP_CHECK(hipMemcpyAsync(part.data(), s->rms_ring, sizeof(double) * static_cast<size_t>(sweeps), hipMemcpyDeviceToHost, s->stream));
                    HIP_CHECK(hipStreamSynchronize(s->stream));
                    for (int k = 0; k < sweeps; k++) sums[static_cast<size_t>(k)] += part[static_cast<size_t>(k)];
                    nodes += s->level(level).n_owned;
                }
                for (int k = 0; k < sweeps; k++) rms_out[k] = std::sqrt(sums[static_cast<size_t>(k)] / double(nodes));
            }
            return;
        }
        // One graph over all ranks' streams replays SLOWER than the eager calls on ROCm 7.2 (2 ranks: 301 against 262 us per
        // sweep; launching a graph of ~40 nodes on 4 streams costs the host 150 us), so groups capture only on request
        // (MGCFD_GROUP_GRAPH=1); a single rank's two-stream sweep does gain (mgcfd_rank_sweeps: 76 against 129 us).
        static const bool group_graphs = std::getenv("MGCFD_GROUP_GRAPH") && std::atoi(std::getenv("MGCFD_GROUP_GRAPH")) != 0;
        const bool graphs = group_graphs && sweep_graphs_enabled() && !timing;
        if (graphs) {
            // a replayed graph is launched on rank 0's stream: it must start behind whatever the other ranks' streams hold
            for (mgcfd_solver *s : g->ranks) {
                if (s == s0) continue;
                s->use_device();
                HIP_CHECK(hipEventRecord(s->level(level).hx->joined.get(), s->stream));
                HIP_CHECK(hipStreamWaitEvent(s0->stream, s->level(level).hx->joined.get(), 0));
            }
        }
        bool replayed = false;
        for (int k = 0; k < sweeps; k++) {
            const int rot = s0->level(level).rot % 3 + 3 * h0.min_parity;     // (the captured launches name the minima's word of this parity)
            const bool steady = !s0->global_dt() || s0->level(level).min_ahead || !part_look_ahead();   // (as in mgcfd_rank_sweeps)
            if (graphs && !h0.graph_failed && steady) {
                if (!h0.sweep_graph[rot]) {
                    const bool ahead_before = s0->level(level).min_ahead;
                    // every rank's sweep in ONE graph: the other ranks' streams fork from rank 0's and join it at the end
                    std::vector<std::vector<int64_t>> before;
                    std::vector<int> rot_before;
                    std::vector<std::pair<hipStream_t, hipEvent_t>> others;
                    for (mgcfd_solver *s : g->ranks) {
                        DeviceLevel &lv = s->level(level);
                        before.emplace_back(lv.iters, lv.iters + MGCFD_NUM_LOOPS);
                        rot_before.push_back(lv.rot);
                        if (s != s0) others.emplace_back(s->stream, lv.hx->joined.get());
                    }
                    s0->use_device();
                    const bool ok = capture_sweep(s0->stream, others, h0.joined.get(), [&] { group_sweep_once(g, level); }, h0.sweep_graph[rot]);
                    for (size_t r = 0; r < g->ranks.size(); r++) {
                        mgcfd_solver *s = g->ranks[r];
                        DeviceLevel &lv = s->level(level);
                        s->force_check = -1;
                        for (int q = 0; q < MGCFD_NUM_LOOPS; q++) { lv.hx->graph_iters[rot][q] = lv.iters[q] - before[r][static_cast<size_t>(q)]; lv.iters[q] = before[r][static_cast<size_t>(q)]; }
                        lv.rot = rot_before[r]; lv.apply_rot();
                        lv.hx->min_parity = rot / 3;        // (the capture advanced the host state without running anything)
                        lv.min_ahead = ahead_before;
                    }
                    if (!ok) { h0.graph_failed = true; group_sweep_once(g, level); continue; }
                }
                s0->use_device();
                HIP_CHECK(hipGraphLaunch(h0.sweep_graph[rot].get(), s0->stream));
                replayed = true;
                for (mgcfd_solver *s : g->ranks) { after_replayed_sweep(s, level, s->level(level).hx->graph_iters[rot]); s->level(level).hx->min_parity ^= 1; }
            } else {
                group_sweep_once(g, level);
            }
        }
        // direct mode: the last stage's pushes land in the peers' `variables`; a rank's stream goes on only behind the pushes into it
        if (h0.direct) for (mgcfd_solver *s : g->ranks) { s->use_device(); wait_for_peers(g, s, level, 2); }
        if (replayed) {
            // ... and what the other ranks' streams are given next must wait for the graphs
            s0->use_device();
            HIP_CHECK(hipEventRecord(h0.joined.get(), s0->stream));
            for (mgcfd_solver *s : g->ranks) if (s != s0) { s->use_device(); HIP_CHECK(hipStreamWaitEvent(s->stream, h0.joined.get(), 0)); }
        }
    });
}

int mgcfd_group_sweeps(mgcfd_group *g, int level, int sweeps) { return group_sweeps_impl(g, level, sweeps, nullptr); }
int mgcfd_group_sweeps_rms(mgcfd_group *g, int level, int sweeps, double *rms_of_each)
{
    REQUIRE(rms_of_each);
    return group_sweeps_impl(g, level, sweeps, rms_of_each);
}

// calc_rms over the whole level: sqrt(sum over the ranks' owned nodes of residual^2 / owned nodes of all ranks).  Synchronises.
int mgcfd_group_rms(mgcfd_group *g, int level, double *rms)
{
    REQUIRE(g); REQUIRE(rms);
    return guarded([&] {
        double sum = 0.0;
        int64_t nodes = 0;
        for (mgcfd_solver *s : g->ranks) {
            s->use_device();
            DeviceLevel &lv = s->level(level);
            exact::launch_sumsq(s->stream, lv.info.nel, lv.dp.stride, lv.residuals, lv.partials, lv.n_partials, lv.sumsq, lv.dp.old_of_new, lv.n_owned);
            double part = 0.0;
            HIP_CHECK(hipMemcpyAsync(&part, lv.sumsq, sizeof(double), hipMemcpyDeviceToHost, s->stream));
            HIP_CHECK(hipStreamSynchronize(s->stream));
            sum += part;
            nodes += lv.n_owned;
        }
        *rms = std::sqrt(sum / double(nodes));
    });
}

int mgcfd_group_synchronize(mgcfd_group *g)
{
    REQUIRE(g);
    return guarded([&] { for (mgcfd_solver *s : g->ranks) { s->use_device(); HIP_CHECK(hipStreamSynchronize(s->stream)); HIP_CHECK(hipGetLastError()); } });
}

// ---- V-cycles on a PARTITIONED hierarchy, the whole state machine inside the library --------------------------------------
// mgcfd_create_partitioned_mg + mgcfd_rank_set_halo on EVERY level.  The cycle is the reference's
// (src/euler3d_cpu_double.cpp:371-694: sweeps on levels 0 .. n-1, n-2 .. 1 with mg_restrict on the way up and
// prolong_residuals_interpolate_proper on the way down) with ghost values moved where the next loop reads them:
//   `variables` of a level   after every time_step (inside the partitioned sweep: one message per Runge-Kutta stage),
//                            after mg_restrict filled it (coarse ghosts: mg_loops.cpp:30-202 writes owned coarse nodes only) and
//                            after the prolongation corrected it (fine ghosts: the next sweep's fluxes read them);
//   `residuals` of the coarse level before the prolongation (mg_loops.cpp:678-864 reads the parents of a node's neighbours).
// A coarse node is averaged where it is owned, over its children in GLOBAL-id order (order_keys), so every level equals the
// unpartitioned hierarchy's bit for bit on owned nodes.  The transfers' exchanges are the buffered form (pack, copies or RCCL
// send / receive, unpack) outside the sweeps' three-set rotation, hence with explicit waits for the buffers.

static void group_prepare_level(mgcfd_group *g, int level)
{
    for (mgcfd_solver *s : g->ranks) {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        if (!lv.hx) throw std::invalid_argument("a rank has no halo lists on level " + std::to_string(level) + ": call mgcfd_rank_set_halo for every level");
        s->settle_fluxes(lv);
    }
    group_ensure_min_words(g, level);                       // (allocations and uploads: never inside a sweep)
    group_prepare_direct(g, level);
}

static double *array_ptr(DeviceLevel &lv, int which, int *ncols);

// the ghosts of array `which` of `level` <- their owners, on every rank of the group
static void group_exchange_array(mgcfd_group *g, int level, int which)
{
    const int b = 0;
    for (mgcfd_solver *s : g->ranks) {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        HaloExchange &hx = *lv.hx;
        s->settle_residuals(lv);
        // this rank's send buffer is free behind the copies the peers made out of it (their `arrived` of the last use of the
        // set); and in direct mode nobody's last push into this rank's ghosts may still be on its way when the unpack writes them
        for (int p : hx.peer) HIP_CHECK(hipStreamWaitEvent(s->stream, g->ranks[static_cast<size_t>(p)]->level(level).hx->arrived[b].get(), 0));
        if (hx.direct) wait_for_peers(g, s, level, 2);
        int nc = 0;
        halo_start(s, level, array_ptr(lv, which, &nc), b);
    }
    group_deliver(g, level, b, true);
    for (mgcfd_solver *s : g->ranks) {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        int nc = 0;
        halo_finish(s, level, array_ptr(lv, which, &nc), b);
        if (which == MGCFD_ARR_VARIABLES) lv.min_ahead = false;
    }
}

// ---- surface loads of a partitioned level -------------------------------------------------------------------------------
// mgcfd_surface_loads needs every solid-wall edge of the level in ONE order to be the bitwise function of the state it is.  A
// level split over ranks keeps that order: rank r's k-th solid-wall edge is edge slot[k] of the whole level's solid-wall slice
// (mgcfd_rank_set_wall_slots), every rank stores its edges' six terms at those slots of a table on rank 0 (k_loads_terms: in a
// group straight into rank 0's memory, as the direct halo push stores into the peers' ghosts; over RCCL as a message that
// rank 0 places by slot, k_loads_scatter), and rank 0 reduces the table by the trees of k_surface_loads (k_loads_reduce).
// Terms travel by stores and copies only — an arithmetic reduction of "term + zeros" would turn -0.0 into +0.0.
static RankLoads &rank_loads_of(mgcfd_solver *s, int level, int rank)
{
    DeviceLevel &lv = s->level(level);
    if (!lv.rl)
        throw std::invalid_argument("surface loads: rank " + std::to_string(rank) + " has no wall slots on level " + std::to_string(level) +
                                    " (mgcfd_rank_set_wall_slots)");
    return *lv.rl;
}

// the gathering rank's table (pad lanes zero, and they stay zero: slots lie below `total`), partial sums and ticket
static void loads_gather_alloc(RankLoads &r0)
{
    if (r0.table || r0.total == 0) return;
    r0.row = (r0.total + 255) / 256 * 256;
    DeviceOwner made;                                   // (all three or none: r0.table says whether this has been done)
    double *table = made.alloc<double>(static_cast<size_t>(6 * r0.row));
    HIP_CHECK(hipMemset(table, 0, sizeof(double) * static_cast<size_t>(6 * r0.row)));
    double *partial = made.alloc<double>(static_cast<size_t>(6 * (r0.row / 256)));
    unsigned *ticket = made.alloc<unsigned>(1);
    HIP_CHECK(hipMemset(ticket, 0, sizeof(unsigned)));
    r0.mem.absorb(std::move(made));
    r0.table = table; r0.partial = partial; r0.ticket = ticket;
}

static LoadsTerms loads_terms_of(mgcfd_solver *s, DeviceLevel &lv, const int32_t *slot, double *table, int64_t row)
{
    LoadsTerms t;
    t.rec = lv.wall_rec; t.n = lv.n_wall_rec; t.p_inf = s->p_inf; t.ref = s->loads_dev;
    t.slot = slot; t.table = table; t.row = row;
    return t;
}

// rank 0's reduce of its table on its stream, stored at `to` (the terms tables hold the pressure six)
static void loads_reduce(mgcfd_solver *s0, RankLoads &r0, LoadsDest to)
{
    LoadsTask t;
    t.n = r0.total; t.partial = r0.partial; t.ticket = r0.ticket;
    loads_store_to(s0, LoadsKind::Pressure, to, t);
    launch_loads_reduce(s0->stream, r0.table, r0.row, t);
}

// In-process groups.  Before the first launch, once per set of slots: every rank of the level has slots, all name the same
// total, and together they name every edge of the whole level exactly once.  Then the reference point to every rank, rank
// 0's table and the events — nothing of this happens inside a cycle.
static void group_loads_prepare(mgcfd_group *g, int level, const double *ref_point)
{
    const int n = static_cast<int>(g->ranks.size());
    bool checked = true;
    for (int r = 0; r < n; r++) checked = rank_loads_of(g->ranks[static_cast<size_t>(r)], level, r).checked && checked;
    RankLoads &r0 = *g->ranks[0]->level(level).rl;
    if (!checked) {
        std::vector<int> named_by(static_cast<size_t>(r0.total), -1);
        int64_t named = 0;
        for (int r = 0; r < n; r++) {
            const RankLoads &rl = *g->ranks[static_cast<size_t>(r)]->level(level).rl;
            const std::string who = "surface loads: the wall slots of rank " + std::to_string(r) + " on level " + std::to_string(level);
            if (rl.total != r0.total)
                throw std::invalid_argument(who + " give the whole level " + std::to_string(rl.total) + " solid-wall edges, rank 0's " + std::to_string(r0.total));
            for (int64_t k : rl.slot_host) {
                int &by = named_by[static_cast<size_t>(k)];
                if (by >= 0) throw std::invalid_argument(who + " name slot " + std::to_string(k) + ", which rank " + std::to_string(by) + " names too");
                by = r;
                named++;
            }
        }
        if (named != r0.total)
            throw std::invalid_argument("surface loads: the wall slots of ranks 0 .. " + std::to_string(n - 1) + " on level " + std::to_string(level) + " name " +
                                        std::to_string(named) + " of the level's " + std::to_string(r0.total) + " solid-wall edges");
        for (mgcfd_solver *s : g->ranks) s->level(level).rl->checked = true;
    }
    for (mgcfd_solver *s : g->ranks) {
        s->use_device();
        loads_upload_ref(s, ref_point);
        RankLoads &rl = *s->level(level).rl;
        if (!rl.terms) rl.terms = make_event(hipEventDisableTiming);
    }
    g->ranks[0]->use_device();
    loads_gather_alloc(r0);
    if (!r0.read) r0.read = make_event(hipEventDisableTiming);
}

// One rank's part of an evaluation (on its device): its terms into rank 0's table, behind the reduce that read the table
// last, then its event.  A rank without a solid-wall edge launches nothing and records the event all the same.
static void group_loads_terms(mgcfd_group *g, mgcfd_solver *s, int level)
{
    mgcfd_solver *s0 = g->ranks[0];
    RankLoads &r0 = *s0->level(level).rl;
    if (r0.total == 0) return;
    DeviceLevel &lv = s->level(level);
    if (s != s0) HIP_CHECK(hipStreamWaitEvent(s->stream, r0.read.get(), 0));      // (rank 0's own stream is behind its reduce anyway)
    launch_loads_terms(s->stream, lv.dp.stride, lv.q, loads_terms_of(s, lv, lv.rl->slot, r0.table, r0.row));
    HIP_CHECK(hipEventRecord(lv.rl->terms.get(), s->stream));
}

// ... and rank 0's (on its device, every rank's terms event of this evaluation recorded): the reduce behind all of them
static void group_loads_reduce(mgcfd_group *g, int level, LoadsDest to)
{
    mgcfd_solver *s0 = g->ranks[0];
    RankLoads &r0 = *s0->level(level).rl;
    if (r0.total == 0) return;
    for (mgcfd_solver *s : g->ranks) if (s != s0) HIP_CHECK(hipStreamWaitEvent(s0->stream, s->level(level).rl->terms.get(), 0));
    loads_reduce(s0, r0, to);
    HIP_CHECK(hipEventRecord(r0.read.get(), s0->stream));
}

static void group_loads_once(mgcfd_group *g, int level, LoadsDest to)
{
    for (mgcfd_solver *s : g->ranks) { s->use_device(); group_loads_terms(g, s, level); }
    g->ranks[0]->use_device();
    group_loads_reduce(g, level, to);
}

static void append_level0_sumsq(mgcfd_solver *s)
{
    DeviceLevel &lv = s->level(0);
    exact::launch_sumsq(s->stream, lv.info.nel, lv.dp.stride, lv.residuals, lv.partials, lv.n_partials, lv.sumsq, lv.dp.old_of_new, lv.n_owned);
    launch_append_scalar(s->stream, lv.sumsq, s->rms_ring, s->rms_count, mgcfd_solver::kRmsRing);
}

// one V-cycle of every rank of an in-process group (one host thread issues it)
// with_loads: the level-0 loads of the state the cycle leaves into the row of the cycle's RMS (rank 0's history)
static void group_cycle_once(mgcfd_group *g, bool with_rms, bool with_loads)
{
    const int n = static_cast<int>(g->ranks[0]->L.size());
    for (int l = 0; l < n; l++) {
        group_sweep_once(g, l);                                                    // :383-508
        if (l == 0 && with_rms) for (mgcfd_solver *s : g->ranks) { s->use_device(); append_level0_sumsq(s); }   // :509-512
        if (l + 1 < n) {
            for (mgcfd_solver *s : g->ranks) {
                s->use_device();
                if (s->level(l).hx->direct) wait_for_peers(g, s, l, 2);            // (the children this rank holds as ghosts: the peers' last pushes)
                s->op_restrict(l);                                                 // :527-559
            }
            group_exchange_array(g, l + 1, MGCFD_ARR_VARIABLES);
        }
    }
    for (int l = n - 2; l >= 0; l--) {
        group_exchange_array(g, l + 1, MGCFD_ARR_RESIDUALS);
        for (mgcfd_solver *s : g->ranks) { s->use_device(); s->op_prolong(l); }    // :560-688
        group_exchange_array(g, l, MGCFD_ARR_VARIABLES);
        if (l > 0) group_sweep_once(g, l);
    }
    if (with_loads) group_loads_once(g, 0, LoadsDest::history());
}

// The same cycle with a host thread per rank (direct mode; what mgcfd_group_cycles runs for groups of several ranks:
// one thread issuing every rank's ~100 calls per cycle makes the host the bottleneck N times over).  As in
// group_sweeps_threaded the threads agree on the ORDER of event records and waits through barriers: one after the first
// half of compute_step_factor and after every stage of a sweep, two per transfer exchange (all packed | all delivered).
static void group_cycles_threaded(mgcfd_group *g, int cycles, bool with_rms, bool with_loads)
{
    const int n = static_cast<int>(g->ranks.size());
    const int nl = static_cast<int>(g->ranks[0]->L.size());
    SpinBarrier bar(n);
    std::atomic<bool> failed{false};
    std::mutex mu;
    std::exception_ptr first_error;
    const bool global_dt = g->ranks[0]->global_dt();
    auto run = [&](int r) {
        mgcfd_solver *s = g->ranks[static_cast<size_t>(r)];
        // (a rank that failed keeps arriving at the barriers, doing nothing, so that the others are not left waiting)
        auto step = [&](auto &&body) {
            if (failed.load(std::memory_order_acquire)) return;
            try { body(); }
            catch (...) { std::lock_guard<std::mutex> lock(mu); if (!first_error) first_error = std::current_exception(); failed.store(true, std::memory_order_release); }
        };
        step([&] { s->use_device(); });
        auto sweep = [&](int level) {                   // (group_sweeps_threaded's body)
            DeviceLevel &lv = s->level(level);
            HaloExchange &hx = *lv.hx;
            const int par = hx.min_parity;
            step([&] {
                sweep_first_half(s, level, hx.min_par + par);
                if (global_dt) HIP_CHECK(hipEventRecord(hx.reduced.get(), s->stream));
            });
            hx.min_parity = par ^ 1;
            bar.wait();
            PushPeers to[MGCFD_RK];
            step([&] {
                if (global_dt) {
                    for (mgcfd_solver *src : g->ranks) if (src != s) HIP_CHECK(hipStreamWaitEvent(s->stream, src->level(level).hx->reduced.get(), 0));
                    launch_min_over_peers(s->stream, hx.peer_scalars[par], n, hx.gmin);
                }
                for (int j = 0; j < MGCFD_RK; j++) to[j] = make_push_peers(g, s, level, [&](DeviceLevel &pl) { return stage_buffers(pl, j).out; });
            });
            for (int j = 0; j < MGCFD_RK; j++) {
                step([&] {
                    stage_boundary_direct(g, s, level, j, group_min(global_dt, hx), &to[j]);
                    stage_interior(s, level, j, group_min(global_dt, hx));
                });
                bar.wait();
            }
        };
        auto exchange = [&](int level, int which) {
            const int b = 0;
            DeviceLevel &lv = s->level(level);
            HaloExchange &hx = *lv.hx;
            step([&] {
                s->settle_residuals(lv);
                for (int p : hx.peer) HIP_CHECK(hipStreamWaitEvent(s->stream, g->ranks[static_cast<size_t>(p)]->level(level).hx->arrived[b].get(), 0));
                wait_for_peers(g, s, level, 2);
                int nc = 0;
                halo_start(s, level, array_ptr(lv, which, &nc), b);
            });
            bar.wait();                                 // every rank's pack event is recorded
            step([&] {
                deliver_to(g, s, level, b, true);
                int nc = 0;
                halo_finish(s, level, array_ptr(lv, which, &nc), b);
                if (which == MGCFD_ARR_VARIABLES) lv.min_ahead = false;
            });
            bar.wait();                                 // ... and every rank's arrival event, before anybody's next wait for it
        };
        for (int c = 0; c < cycles; c++) {
            for (int l = 0; l < nl; l++) {
                sweep(l);
                if (l == 0 && with_rms) step([&] { append_level0_sumsq(s); });
                if (l + 1 < nl) {
                    step([&] { wait_for_peers(g, s, l, 2); s->op_restrict(l); });
                    exchange(l + 1, MGCFD_ARR_VARIABLES);
                }
            }
            for (int l = nl - 2; l >= 0; l--) {
                exchange(l + 1, MGCFD_ARR_RESIDUALS);
                step([&] { s->op_prolong(l); });
                exchange(l, MGCFD_ARR_VARIABLES);
                if (l > 0) sweep(l);
            }
            if (with_loads) {
                step([&] { group_loads_terms(g, s, 0); });
                bar.wait();                             // every rank's terms event is recorded
                // (rank 0's record of `read` lies ahead of the barriers of the next cycle's first sweep, the other ranks' waits for it behind them)
                if (r == 0) step([&] { group_loads_reduce(g, 0, LoadsDest::history()); });
            }
        }
        step([&] { for (int l = 0; l < nl; l++) wait_for_peers(g, s, l, 2); HIP_CHECK(hipGetLastError()); });
    };
    std::vector<std::thread> threads;
    for (int r = 1; r < n; r++) threads.emplace_back(run, r);
    run(0);
    for (std::thread &t : threads) t.join();
    if (first_error) std::rethrow_exception(first_error);
}

// what the checks inside the launches of every rank found (the reference exits at the first bad cell of the first failing time_step)
static int group_read_errors(mgcfd_group *g)
{
    int code = MGCFD_OK;
    for (mgcfd_solver *s : g->ranks) {
        s->use_device();
        const int c = s->read_error(nullptr);
        if (c != MGCFD_OK && code == MGCFD_OK) code = c;
    }
    return code;
}

// loads_out != nullptr (mgcfd_group_cycles_loads): also the level-0 surface loads of the state every cycle leaves, [cycles][6]
static int group_cycles_impl(mgcfd_group *g, int cycles, double *rms_out, const double *ref_point, double *loads_out)
{
    REQUIRE(g);
    int code = MGCFD_OK;
    const LoadsKind kind = LoadsKind::Pressure;                 // (what the terms tables hold)
    if (loads_out) loads_rows(nullptr, kind, false, loads_out, 0, 0, static_cast<size_t>(std::max(cycles, 0)));    // NaN until the run is through
    const bool with_rms = rms_out || loads_out;                 // (a cycle's loads go into the row of its RMS)
    const int rc = guarded([&] {
        if (cycles > mgcfd_solver::kRmsRing) throw std::invalid_argument("at most 4096 cycles per call");
        group_require_same_free_stream(g);
        group_require_same_time_step(g);
        const int n = static_cast<int>(g->ranks[0]->L.size());
        for (mgcfd_solver *s : g->ranks) if (static_cast<int>(s->L.size()) != n) throw std::invalid_argument("the ranks of a group hold the same number of levels");
        for (int l = 0; l < n; l++) group_prepare_level(g, l);
        if (loads_out) {
            group_loads_prepare(g, 0, ref_point);
            mgcfd_solver *s0 = g->ranks[0];
            s0->use_device();
            ensure_loads_ring(s0, kind);
        }
        const bool with_loads = loads_out != nullptr;
        for (mgcfd_solver *s : g->ranks) {
            s->use_device();
            ensure_rms_ring(s);
            HIP_CHECK(hipMemsetAsync(s->rms_count, 0, sizeof(int), s->stream));
        }
        // A host thread per rank where every level runs the direct form and every rank has a device of its own: one thread
        // issuing N ranks' ~100 calls per cycle costs N x 0.76 ms (tools/hostcost_cycles.py).  Ranks that SHARE a device (the
        // one-GPU rehearsal) are issued by the caller's thread: there the threads only contend for the one device's queues
        // (8 ranks: 12.2 ms per cycle against 6.0).  MGCFD_GROUP_THREADS=0 / 1 forces either form.
        bool all_direct = g->ranks.size() > 1;
        for (int l = 0; l < n; l++) all_direct = all_direct && g->ranks[0]->level(l).hx->direct;
        if (const char *e = std::getenv("MGCFD_GROUP_THREADS")) all_direct = all_direct && std::atoi(e) != 0;
        else {
            std::vector<int> devs;
            for (mgcfd_solver *s : g->ranks) devs.push_back(s->device);
            std::sort(devs.begin(), devs.end());
            all_direct = all_direct && std::adjacent_find(devs.begin(), devs.end()) == devs.end();
        }
        if (all_direct) group_cycles_threaded(g, cycles, with_rms, with_loads);
        else for (int c = 0; c < cycles; c++) group_cycle_once(g, with_rms, with_loads);
        // every rank's stream behind the last pushes into it, then the read-backs
        for (mgcfd_solver *s : g->ranks) { s->use_device(); for (int l = 0; l < n; l++) if (s->level(l).hx->direct) wait_for_peers(g, s, l, 2); }
        if (rms_out) {
            std::vector<double> sums(static_cast<size_t>(cycles), 0.0), part(static_cast<size_t>(std::max(cycles, 1)));
            int64_t nodes = 0;
            for (mgcfd_solver *s : g->ranks) {                  // (added in rank order, as mgcfd_group_rms adds them)
                s->use_device();
                HIP_CHECK(hipMemcpyAsync(part.data(), s->rms_ring, sizeof(double) * static_cast<size_t>(cycles), hipMemcpyDeviceToHost, s->stream));
                HIP_CHECK(hipStreamSynchronize(s->stream));
                for (int k = 0; k < cycles; k++) sums[static_cast<size_t>(k)] += part[static_cast<size_t>(k)];
                nodes += s->level(0).n_owned;
            }
            for (int k = 0; k < cycles; k++) rms_out[k] = std::sqrt(sums[static_cast<size_t>(k)] / double(nodes));
        }
        if (loads_out && cycles > 0) {
            mgcfd_solver *s0 = g->ranks[0];
            s0->use_device();
            loads_rows(s0, kind, s0->level(0).rl->total > 0, loads_out, 0, static_cast<size_t>(cycles), static_cast<size_t>(cycles));
            HIP_CHECK(hipStreamSynchronize(s0->stream));
        }
        code = group_read_errors(g);
        for (mgcfd_solver *s : g->ranks) { s->use_device(); HIP_CHECK(hipGetLastError()); }
    });
    if (rc != MGCFD_OK) return rc;
    if (code != MGCFD_OK) g_last_error = "check_for_invalid_variables: a rank of the group found an invalid state during the cycles";
    return code;
}

int mgcfd_group_cycles(mgcfd_group *g, int cycles, double *rms_out) { return group_cycles_impl(g, cycles, rms_out, nullptr, nullptr); }
int mgcfd_group_cycles_loads(mgcfd_group *g, int cycles, const double ref_point[3], double *rms_out, double *loads_out)
{
    REQUIRE(loads_out);
    return group_cycles_impl(g, cycles, rms_out, ref_point, loads_out);
}

int mgcfd_group_surface_loads(mgcfd_group *g, int level, const double ref_point[3], double out6[6])
{
    REQUIRE(g); REQUIRE(out6);
    return guarded([&] {
        group_require_same_free_stream(g);
        group_require_same_time_step(g);
        group_loads_prepare(g, level, ref_point);
        mgcfd_solver *s0 = g->ranks[0];
        loads_now(s0, LoadsKind::Pressure, s0->level(level).rl->total > 0, out6, [&](LoadsDest to) { group_loads_once(g, level, to); });
    });
}

// ---- the same for one rank per process over RCCL ----
static void rank_exchange_array(mgcfd_solver *s, int level, int which)
{
    DeviceLevel &lv = s->level(level);
    s->settle_residuals(lv);
    int nc = 0;
    double *field = array_ptr(lv, which, &nc);
    halo_start(s, level, field, 0);                         // (set 0 is free: a sweep finishes every exchange it starts, and so does this)
    halo_finish(s, level, field, 0);
    if (which == MGCFD_ARR_VARIABLES) lv.min_ahead = false;
}

// Surface loads, one rank per process.  NOTE: rehearsed with ONE rank only (what a one-GPU box offers): with more, the
// agreement below and the messages are as written, never run.
// Once per set of slots, outside the cycles: the message lengths (every rank's edge count and the total it names, by one
// all-reduce(SUM) of a vector that is zero but for the rank's own entries — counts, not terms), the other ranks' slots to
// rank 0, which checks them before any launch stores by them, and the verdict to everybody.
static void rank_loads_prepare(mgcfd_solver *s, int level, const double *ref_point)
{
    mgcfd_comm &c = comm_of(s);
    if (!c.rccl) throw std::invalid_argument("in-process ranks: mgcfd_group_surface_loads / mgcfd_group_cycles_loads");
    DeviceLevel &lv = s->level(level);
    RankLoads &rl = rank_loads_of(s, level, c.rank);
    loads_upload_ref(s, ref_point);
    if (rl.checked) return;
    const size_t w = static_cast<size_t>(c.world), me = static_cast<size_t>(c.rank);
    auto all_sum = [&](std::vector<double> &v) {
        DeviceOwner scratch;
        double *d = scratch.upload(v);
        RCCL_CHECK(g_rccl.AllReduce(d, d, v.size(), Rccl::kDouble, Rccl::kSum, c.rccl, s->stream));
        HIP_CHECK(hipMemcpyAsync(v.data(), d, sizeof(double) * v.size(), hipMemcpyDeviceToHost, s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
    };
    std::vector<double> v(2 * w, 0.0);
    v[me] = double(lv.n_wall_rec); v[w + me] = double(rl.total);
    all_sum(v);
    rl.counts.assign(w, 0);
    int64_t sum = 0;
    for (size_t r = 0; r < w; r++) {
        rl.counts[r] = static_cast<int64_t>(v[r]);
        sum += rl.counts[r];
        if (static_cast<int64_t>(v[w + r]) != rl.total)
            throw std::invalid_argument("surface loads: the wall slots of rank " + std::to_string(r) + " on level " + std::to_string(level) + " give the whole level " +
                                        std::to_string(static_cast<int64_t>(v[w + r])) + " solid-wall edges, rank " + std::to_string(me) + "'s " + std::to_string(rl.total));
    }
    if (sum != rl.total)
        throw std::invalid_argument("surface loads: the wall slots of the ranks on level " + std::to_string(level) + " name " + std::to_string(sum) +
                                    " of the level's " + std::to_string(rl.total) + " solid-wall edges");
    if (w > 1 && rl.total > 0) {
        if (me == 0) { for (int32_t *&p : rl.peer_slot) rl.mem.release(p); rl.peer_slot.assign(w, nullptr); }
        RCCL_CHECK(g_rccl.GroupStart());
        if (me == 0) {
            for (size_t r = 1; r < w; r++) {
                if (rl.counts[r] == 0) continue;
                rl.peer_slot[r] = rl.mem.alloc<int32_t>(static_cast<size_t>(rl.counts[r]));
                RCCL_CHECK(g_rccl.Recv(rl.peer_slot[r], static_cast<size_t>(rl.counts[r]), Rccl::kInt32, static_cast<int>(r), c.rccl, s->stream));
            }
        } else if (lv.n_wall_rec > 0) {
            RCCL_CHECK(g_rccl.Send(rl.slot, static_cast<size_t>(lv.n_wall_rec), Rccl::kInt32, 0, c.rccl, s->stream));
        }
        RCCL_CHECK(g_rccl.GroupEnd());
        std::vector<double> bad(1, 0.0);
        if (me == 0) {
            std::vector<char> seen(static_cast<size_t>(rl.total), 0);
            for (int64_t k : rl.slot_host) seen[static_cast<size_t>(k)] = 1;
            for (size_t r = 1; r < w; r++) {
                std::vector<int32_t> got(static_cast<size_t>(rl.counts[r]));
                if (!got.empty()) HIP_CHECK(hipMemcpyAsync(got.data(), rl.peer_slot[r], sizeof(int32_t) * got.size(), hipMemcpyDeviceToHost, s->stream));
                HIP_CHECK(hipStreamSynchronize(s->stream));
                for (int32_t k : got) {
                    if (k < 0 || k >= rl.total || seen[static_cast<size_t>(k)]) { bad[0] = 1.0; break; }
                    seen[static_cast<size_t>(k)] = 1;
                }
            }
        }
        all_sum(bad);
        if (bad[0] != 0.0)
            throw std::invalid_argument("surface loads: the wall slots of the ranks on level " + std::to_string(level) + " name a slot twice or outside the level's " +
                                        std::to_string(rl.total) + " solid-wall edges");
    }
    if (me == 0) loads_gather_alloc(rl);
    if (w > 1 && !rl.compact) {
        const int64_t n = me == 0 ? rl.total - rl.counts[0] : lv.n_wall_rec;
        rl.compact = rl.mem.alloc<double>(static_cast<size_t>(6 * n));
    }
    rl.checked = true;
}

// one evaluation on this rank's stream: the other ranks send their compact terms, rank 0 places them by slot and reduces
static void rank_loads_once(mgcfd_solver *s, int level, LoadsDest to)
{
    mgcfd_comm &c = comm_of(s);
    DeviceLevel &lv = s->level(level);
    RankLoads &rl = *lv.rl;
    if (rl.total == 0) return;
    if (c.rank != 0) {
        if (lv.n_wall_rec == 0) return;
        launch_loads_terms(s->stream, lv.dp.stride, lv.q, loads_terms_of(s, lv, nullptr, rl.compact, lv.n_wall_rec));
        RCCL_CHECK(g_rccl.GroupStart());
        RCCL_CHECK(g_rccl.Send(rl.compact, static_cast<size_t>(6 * lv.n_wall_rec), Rccl::kDouble, 0, c.rccl, s->stream));
        RCCL_CHECK(g_rccl.GroupEnd());
        return;
    }
    launch_loads_terms(s->stream, lv.dp.stride, lv.q, loads_terms_of(s, lv, rl.slot, rl.table, rl.row));
    if (c.world > 1) {
        RCCL_CHECK(g_rccl.GroupStart());
        int64_t off = 0;
        for (size_t r = 1; r < rl.counts.size(); r++) {
            if (rl.counts[r] == 0) continue;
            RCCL_CHECK(g_rccl.Recv(rl.compact + 6 * off, static_cast<size_t>(6 * rl.counts[r]), Rccl::kDouble, static_cast<int>(r), c.rccl, s->stream));
            off += rl.counts[r];
        }
        RCCL_CHECK(g_rccl.GroupEnd());
        off = 0;
        for (size_t r = 1; r < rl.counts.size(); r++) {
            launch_loads_scatter(s->stream, rl.counts[r], rl.compact + 6 * off, rl.counts[r], rl.peer_slot[r], rl.table, rl.row);
            off += rl.counts[r];
        }
    }
    loads_reduce(s, rl, to);
}

// rank 0's `n` results at `buf` to the same place on every other rank
static void rank_loads_share(mgcfd_solver *s, double *buf, size_t n)
{
    mgcfd_comm &c = comm_of(s);
    if (c.world == 1 || n == 0) return;
    RCCL_CHECK(g_rccl.GroupStart());
    if (c.rank == 0) { for (int r = 1; r < c.world; r++) RCCL_CHECK(g_rccl.Send(buf, n, Rccl::kDouble, r, c.rccl, s->stream)); }
    else RCCL_CHECK(g_rccl.Recv(buf, n, Rccl::kDouble, 0, c.rccl, s->stream));
    RCCL_CHECK(g_rccl.GroupEnd());
}

static void rank_cycle_once(mgcfd_solver *s, bool with_rms, bool with_loads)
{
    const int n = static_cast<int>(s->L.size());
    for (int l = 0; l < n; l++) {
        rank_sweep_once(s, l);
        if (l == 0 && with_rms) append_level0_sumsq(s);
        if (l + 1 < n) { s->op_restrict(l); rank_exchange_array(s, l + 1, MGCFD_ARR_VARIABLES); }
    }
    for (int l = n - 2; l >= 0; l--) {
        rank_exchange_array(s, l + 1, MGCFD_ARR_RESIDUALS);
        s->op_prolong(l);
        rank_exchange_array(s, l, MGCFD_ARR_VARIABLES);
        if (l > 0) rank_sweep_once(s, l);
    }
    if (with_loads) rank_loads_once(s, 0, LoadsDest::history());
}

// loads_out != nullptr (mgcfd_rank_cycles_loads): also the level-0 surface loads of the state every cycle leaves, [cycles][6]
static int rank_cycles_impl(mgcfd_solver *s, int cycles, double *rms_out, const double *ref_point, double *loads_out)
{
    REQUIRE(s);
    int code = MGCFD_OK;
    const LoadsKind kind = LoadsKind::Pressure;                 // (what the terms tables hold)
    if (loads_out) loads_rows(nullptr, kind, false, loads_out, 0, 0, static_cast<size_t>(std::max(cycles, 0)));    // NaN until the run is through
    const bool with_rms = rms_out || loads_out;                 // (a cycle's loads go into the row of its RMS)
    const int rc = guarded([&] {
        s->use_device();
        mgcfd_comm &c = comm_of(s);
        if (!c.rccl) throw std::invalid_argument("in-process ranks cycle through mgcfd_group_cycles");
        if (cycles > mgcfd_solver::kRmsRing) throw std::invalid_argument("at most 4096 cycles per call");
        for (DeviceLevel &lv : s->L) {
            if (!lv.hx) throw std::invalid_argument("a level has no halo lists: call mgcfd_rank_set_halo for every level");
            if (lv.hx->ipc) throw std::invalid_argument("mgcfd_rank_cycles runs the buffered exchange: mgcfd_rank_ipc_detach first");
            s->settle_fluxes(lv);
        }
        ensure_rms_ring(s);
        HIP_CHECK(hipMemsetAsync(s->rms_count, 0, sizeof(int), s->stream));
        if (loads_out) {
            rank_loads_prepare(s, 0, ref_point);
            ensure_loads_ring(s, kind);
        }
        for (int k = 0; k < cycles; k++) rank_cycle_once(s, with_rms, loads_out != nullptr);
        if (loads_out && cycles > 0) {
            const bool wall = s->level(0).rl->total > 0;
            if (wall) rank_loads_share(s, s->loads_ring[static_cast<int>(kind)], static_cast<size_t>(cycles) * loads_width(kind));
            loads_rows(s, kind, wall, loads_out, 0, static_cast<size_t>(cycles), static_cast<size_t>(cycles));
            HIP_CHECK(hipStreamSynchronize(s->stream));
        }
        if (rms_out && cycles > 0) {
            // calc_rms of the whole level (validation.cpp:91-105): the ranks' sums of every cycle added by ONE all-reduce
            RCCL_CHECK(g_rccl.AllReduce(s->rms_ring, s->rms_ring, static_cast<size_t>(cycles), Rccl::kDouble, Rccl::kSum, c.rccl, s->stream));
            double nodes_local = double(s->level(0).n_owned);
            DeviceLevel &l0 = s->level(0);
            HIP_CHECK(hipMemcpyAsync(l0.sumsq, &nodes_local, sizeof(double), hipMemcpyHostToDevice, s->stream));
            RCCL_CHECK(g_rccl.AllReduce(l0.sumsq, l0.hx->gmin, 1, Rccl::kDouble, Rccl::kSum, c.rccl, s->stream));
            double nodes = 0.0;
            std::vector<double> sums(static_cast<size_t>(cycles));
            HIP_CHECK(hipMemcpyAsync(sums.data(), s->rms_ring, sizeof(double) * static_cast<size_t>(cycles), hipMemcpyDeviceToHost, s->stream));
            HIP_CHECK(hipMemcpyAsync(&nodes, l0.hx->gmin, sizeof(double), hipMemcpyDeviceToHost, s->stream));
            HIP_CHECK(hipStreamSynchronize(s->stream));
            for (int k = 0; k < cycles; k++) rms_out[k] = std::sqrt(sums[static_cast<size_t>(k)] / nodes);
        }
        code = s->read_error(nullptr);                      // synchronises
        HIP_CHECK(hipGetLastError());
    });
    if (rc != MGCFD_OK) return rc;
    if (code != MGCFD_OK) g_last_error = "check_for_invalid_variables: invalid state during the cycles";
    return code;
}

int mgcfd_rank_cycles(mgcfd_solver *s, int cycles, double *rms_out) { return rank_cycles_impl(s, cycles, rms_out, nullptr, nullptr); }
int mgcfd_rank_cycles_loads(mgcfd_solver *s, int cycles, const double ref_point[3], double *rms_out, double *loads_out)
{
    REQUIRE(loads_out);
    return rank_cycles_impl(s, cycles, rms_out, ref_point, loads_out);
}

int mgcfd_rank_surface_loads(mgcfd_solver *s, int level, const double ref_point[3], double out6[6])
{
    REQUIRE(s); REQUIRE(out6);
    return guarded([&] {
        s->use_device();
        rank_loads_prepare(s, level, ref_point);
        loads_now(s, LoadsKind::Pressure, s->level(level).rl->total > 0, out6, [&](LoadsDest to) {      // (no solid wall: nothing sent either)
            rank_loads_once(s, level, to);
            rank_loads_share(s, to.out, loads_width(LoadsKind::Pressure));
        });
    });
}

// A partitioned solver's solid-wall edges in the whole level's order: slot[k] = position of its k-th one in the whole
// level's solid-wall slice, n_total = that slice's length, n = how many slots are given (the level's local n_boundary).
int mgcfd_rank_set_wall_slots(mgcfd_solver *s, int level, int64_t n_total, int64_t n, const int64_t *slot)
{
    REQUIRE(s);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        const std::string who = "surface loads: wall slots of level " + std::to_string(level) + ": ";
        if (!s->partitioned) throw std::invalid_argument(who + "the solver holds whole levels (mgcfd_surface_loads needs no slots)");
        if (n_total < 0 || n_total > int64_t(1) << 30) throw std::invalid_argument(who + "the whole level's count must lie in [0, 2^30]");
        if (n != lv.n_wall_rec)
            throw std::invalid_argument(who + std::to_string(n) + " slots given, the level holds " + std::to_string(lv.n_wall_rec) + " solid-wall edges here");
        if (lv.n_wall_rec > 0 && !slot) throw std::invalid_argument(who + "null slot list");
        auto rl = std::make_unique<RankLoads>();
        rl->total = n_total;
        std::vector<int32_t> slot32;
        for (int64_t k = 0; k < lv.n_wall_rec; k++) {
            if (slot[k] < 0 || slot[k] >= n_total || (k > 0 && slot[k] <= slot[k - 1]))
                throw std::invalid_argument(who + "the slots must be strictly ascending in [0, n_total) (local edge lists keep the whole level's order)");
            rl->slot_host.push_back(slot[k]);
            slot32.push_back(static_cast<int32_t>(slot[k]));
        }
        if (!slot32.empty()) rl->slot = rl->mem.upload(slot32);
        HIP_CHECK(hipStreamSynchronize(s->stream));          // (nothing in flight still reads what the old slots' arrays held)
        lv.rl = std::move(rl);
    });
}

// What a solver is a rank of, AS THE LIBRARY SEES IT: out[0] this rank, out[1] the number of ranks, out[2] the transport
// (0 none, 1 RCCL communicator, 2 in-process group, 3 plain attachment: messages through HIP IPC only), out[3] the size the
// RCCL communicator itself reports (ncclCommCount; -1 when there is none).
int mgcfd_rank_info(const mgcfd_solver *s, int out[4])
{
    REQUIRE(s); REQUIRE(out);
    out[0] = 0; out[1] = 1; out[2] = 0; out[3] = -1;
    if (!s->comm) return MGCFD_OK;
    const mgcfd_comm &c = *s->comm;
    out[0] = c.rank; out[1] = c.world; out[2] = c.rccl ? 1 : (c.group ? 2 : 3);
    if (c.rccl && g_rccl.CommCount) { int n = -1; if (g_rccl.CommCount(c.rccl, &n) == 0) out[3] = n; }
    return MGCFD_OK;
}

int mgcfd_rank_graph_status(const mgcfd_solver *s, int level, int64_t out[3])
{
    REQUIRE(s); REQUIRE(out);
    if (level < 0 || level >= static_cast<int>(s->L.size()) || !s->L[static_cast<size_t>(level)].hx) { g_last_error = "the level has no halo lists"; return MGCFD_ERR_ARG; }
    const HaloExchange &hx = *s->L[static_cast<size_t>(level)].hx;
    out[0] = 0;
    for (const GraphExec &ge : hx.sweep_graph) if (ge) out[0]++;
    out[1] = hx.graph_failed ? 1 : 0;
    out[2] = hx.sweeps_replayed;
    return MGCFD_OK;
}

// how a level's tiles split for the overlapped exchange: out[0] boundary tiles, out[1] interior tiles, out[2] nodes sent, out[3] nodes received
int mgcfd_rank_halo_info(const mgcfd_solver *s, int level, int64_t out[4])
{
    REQUIRE(s); REQUIRE(out);
    if (level < 0 || level >= static_cast<int>(s->L.size()) || !s->L[static_cast<size_t>(level)].hx) { g_last_error = "the level has no halo lists"; return MGCFD_ERR_ARG; }
    const HaloExchange &hx = *s->L[static_cast<size_t>(level)].hx;
    out[0] = hx.n_boundary; out[1] = hx.n_interior; out[2] = hx.total_send(); out[3] = hx.total_recv();
    return MGCFD_OK;
}

} // extern "C"

// ------------------------------------------------------------------------------------------
// Surface loads on the solid walls ("Surface loads")
// ------------------------------------------------------------------------------------------
static void loads_require_whole(const mgcfd_solver *s)
{
    if (s->partitioned)
        throw std::invalid_argument("surface loads: the solver holds a partitioned level (mgcfd_create_partitioned*); the loads over all "
                                    "ranks come from mgcfd_group_surface_loads / mgcfd_group_cycles_loads or mgcfd_rank_surface_loads / mgcfd_rank_cycles_loads");
    if (s->comm)
        throw std::invalid_argument("surface loads: the solver is attached as a rank; the loads of a partitioned level come from the group and rank calls");
}

// the wall nodes' table after `fill` has launched what writes it: ids and rows to the host, synchronously
template <typename Fill>
static void wall_table(mgcfd_solver *s, int level, int64_t *node_ids, double *out, int columns, Fill fill)
{
    s->use_device();
    DeviceLevel &lv = s->level(level);
    loads_require_whole(s);
    WallPlan &wp = wall_plan(s, lv);
    if (node_ids) std::copy(wp.original.begin(), wp.original.end(), node_ids);
    if (wp.wn.n == 0) return;
    const double *table = fill(lv, wp);
    HIP_CHECK(hipMemcpyAsync(out, table, sizeof(double) * static_cast<size_t>(columns) * static_cast<size_t>(wp.wn.n), hipMemcpyDeviceToHost, s->stream));
    HIP_CHECK(hipStreamSynchronize(s->stream));
    HIP_CHECK(hipGetLastError());
}

// mgcfd_surface_loads*: level `level`'s loads of `kind` in its current state, synchronously
static int surface_loads_impl(mgcfd_solver *s, int level, const double *ref_point, double *out, LoadsKind kind)
{
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        loads_prepare(s, ref_point);
        loads_now(s, kind, lv.n_wall_rec > 0, out, [&](LoadsDest to) { loads_plan(s, lv, kind); launch_loads(s, level, kind, to); });
    });
}

extern "C" {

int mgcfd_surface_loads(mgcfd_solver *s, int level, const double ref_point[3], double out6[6])
{
    REQUIRE(s); REQUIRE(out6);
    return surface_loads_impl(s, level, ref_point, out6, LoadsKind::Pressure);
}

int mgcfd_run_cycles_loads(mgcfd_solver *s, int cycles, const double ref_point[3], double *rms_out, double *loads_out)
{
    REQUIRE(s); REQUIRE(loads_out);
    return run_cycles_impl(s, cycles, rms_out, ref_point, loads_out);
}

// ---- viscous surface loads: the friction six beside the pressure six, the surface distribution ----
int mgcfd_surface_loads_viscous(mgcfd_solver *s, int level, const double ref_point[3], double out12[12])
{
    REQUIRE(s); REQUIRE(out12);
    return surface_loads_impl(s, level, ref_point, out12, LoadsKind::Friction);
}

int mgcfd_run_cycles_loads_viscous(mgcfd_solver *s, int cycles, const double ref_point[3], double *rms_out, double *loads_out)
{
    REQUIRE(s); REQUIRE(loads_out);
    return run_cycles_impl(s, cycles, rms_out, ref_point, loads_out, LoadsKind::Friction);
}

int mgcfd_wall_node_count(mgcfd_solver *s, int level, int64_t *n)
{
    REQUIRE(s); REQUIRE(n);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        loads_require_whole(s);
        *n = wall_plan(s, lv).wn.n;
    });
}

int mgcfd_wall_distribution(mgcfd_solver *s, int level, int64_t *node_ids, double *out)
{
    REQUIRE(s); REQUIRE(out);
    return guarded([&] {
        wall_table(s, level, node_ids, out, MGCFD_WALL_COLUMNS, [&](DeviceLevel &lv, WallPlan &wp) {
            const bool viscous = s->viscous_on(level);
            if (viscous) launch_wall_stress(s, level);
            WallDistribution a;
            a.wn = wp.wn; a.rec = lv.wall_rec; a.p_inf = s->p_inf; a.sw = viscous ? wp.sw : nullptr; a.out = wp.dist;
            launch_wall_distribution(s->stream, lv.dp.stride, lv.q, a);
            return wp.dist;
        });
    });
}

int mgcfd_wall_stress(mgcfd_solver *s, int level, int64_t *node_ids, double *out)
{
    REQUIRE(s); REQUIRE(out);
    return guarded([&] {
        if ((void)s->level(level), !s->viscous_on(level)) throw std::invalid_argument("mgcfd_wall_stress: the viscous terms are off on this level (mgcfd_set_viscous)");
        wall_table(s, level, node_ids, out, 12, [&](DeviceLevel &, WallPlan &wp) { launch_wall_stress(s, level); return wp.sw; });
        // the device table is [12][n]: rows of twelve for the caller
        const size_t n = static_cast<size_t>(s->level(level).wp->wn.n);
        const std::vector<double> cols(out, out + 12 * n);
        for (size_t k = 0; k < n; k++)
            for (size_t f = 0; f < 12; f++) out[k * 12 + f] = cols[f * n + k];
    });
}

// Diagnostic: mean GPU time of `launches` back-to-back launches of k_wall_stress (kind 0), k_surface_loads_viscous (1) or
// k_surface_loads (2) on the level's current state, as mgcfd_bench_viscous times its launches.
int mgcfd_bench_friction_loads(mgcfd_solver *s, int level, int kind, int launches, double *avg_seconds)
{
    REQUIRE(s); REQUIRE(avg_seconds);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        if (!s->viscous_on(level)) throw std::invalid_argument("the viscous terms are off on this level: switch them on first (mgcfd_set_viscous)");
        if (kind < 0 || kind > 2) throw std::invalid_argument("friction loads launch kind: 0 wall stress, 1 pressure and friction loads, 2 pressure loads");
        if (lv.n_wall_rec == 0) throw std::invalid_argument("the level has no solid-wall edge");
        loads_prepare(s, nullptr);
        loads_plan(s, lv, LoadsKind::Friction);
        const LoadsDest to = LoadsDest::at(s->loads_dev + 3);
        launch_loads(s, level, LoadsKind::Friction, to);
        *avg_seconds = s->timed_launches(launches, [&] {
            if (kind == 0) launch_wall_stress(s, level);
            else if (kind == 1) launch_loads(s, level, LoadsKind::Friction, to, false);
            else launch_loads(s, level, LoadsKind::Pressure, to);
        });
    });
}

// ---- heat loads: Q and A behind the twelve, the heat table (INTEGRATION.md "Wall thermal conditions") ----
int mgcfd_surface_loads_heat(mgcfd_solver *s, int level, const double ref_point[3], double out14[14])
{
    REQUIRE(s); REQUIRE(out14);
    return surface_loads_impl(s, level, ref_point, out14, LoadsKind::Heat);
}

int mgcfd_run_cycles_loads_heat(mgcfd_solver *s, int cycles, const double ref_point[3], double *rms_out, double *loads_out)
{
    REQUIRE(s); REQUIRE(loads_out);
    return run_cycles_impl(s, cycles, rms_out, ref_point, loads_out, LoadsKind::Heat);
}

int mgcfd_wall_heat(mgcfd_solver *s, int level, int64_t *node_ids, double *out)
{
    REQUIRE(s); REQUIRE(out);
    return guarded([&] {
        wall_table(s, level, node_ids, out, MGCFD_WALL_HEAT_COLUMNS, [&](DeviceLevel &lv, WallPlan &) {
            WallPlan &wp = wall_plan_heat(s, lv);
            const bool viscous = s->viscous_on(level);
            if (viscous) launch_wall_stress(s, level);
            WallDistribution a;
            a.wn = wp.wn; a.rec = lv.wall_rec; a.p_inf = s->p_inf; a.sw = viscous ? wp.sw : nullptr; a.out = wp.heat;
            launch_wall_heat(s->stream, lv.dp.stride, lv.q, a);
            return wp.heat;
        });
    });
}

// Diagnostic: mean GPU time of `launches` back-to-back launches of the isothermal wall launch (kind 0), the adiabatic one (1) —
// both on the level's second state buffer, so the state stays — the heat-flux launch (2: it adds into fluxes[], accumulating),
// the fourteen-column loads (3) or k_wall_heat (4), as mgcfd_bench_viscous times its launches.
int mgcfd_bench_wall_heat(mgcfd_solver *s, int level, int kind, int launches, double *avg_seconds)
{
    REQUIRE(s); REQUIRE(avg_seconds);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        loads_require_whole(s);
        if (!s->viscous_on(level) || !s->visc_wall) throw std::invalid_argument("the viscous terms with a no-slip wall are off on this level: switch them on first (mgcfd_set_viscous)");
        if (kind < 0 || kind > 4) throw std::invalid_argument("wall heat launch kind: 0 isothermal wall, 1 adiabatic wall, 2 heat-flux wall, 3 fourteen-column loads, 4 heat table");
        if (lv.n_wall_rec == 0) throw std::invalid_argument("the level has no solid-wall edge");
        require_no_sweep_under_way(s, "wall heat");
        loads_upload_ref(s, nullptr);
        WallPlan &wp = wall_plan_heat(s, lv);
        const LoadsDest to = LoadsDest::at(s->loads_dev + 3);
        const double ew = s->wt_mode == MGCFD_WALL_ISOTHERMAL ? s->wt_ew : 1.0 / (1.4 - 1.0);
        const double qw = s->wt_mode == MGCFD_WALL_HEAT_FLUX ? s->wt_value : 1.0;
        DeviceOwner local;
        const double *area = lv.wall_area;
        if (kind == 2 && !area) {
            std::vector<int32_t> nodes(static_cast<size_t>(lv.n_visc_wall));
            HIP_CHECK(hipMemcpy(nodes.data(), lv.visc_wall, sizeof(int32_t) * nodes.size(), hipMemcpyDeviceToHost));
            area = local.upload(wall_areas(lv.info, lv.edges, lv.plan.new_of_old, nodes));
        }
        if (kind == 2) s->settle_fluxes(lv);
        launch_loads(s, level, LoadsKind::Heat, to);
        WallDistribution a;
        a.wn = wp.wn; a.rec = lv.wall_rec; a.p_inf = s->p_inf; a.sw = wp.sw; a.out = wp.heat;
        *avg_seconds = s->timed_launches(launches, [&] {
            if (kind == 0) launch_viscous_wall_isothermal(s->stream, lv.n_visc_wall, lv.dp.stride, lv.visc_wall, ew, lv.q_alt, nullptr, nullptr, nullptr);
            else if (kind == 1) launch_viscous_wall(s->stream, lv.n_visc_wall, lv.dp.stride, lv.visc_wall, lv.q_alt, nullptr, nullptr, nullptr);
            else if (kind == 2) launch_wall_heat_flux(s->stream, lv.n_visc_wall, lv.dp.stride, lv.visc_wall, area, qw, lv.fluxes);
            else if (kind == 3) launch_loads(s, level, LoadsKind::Heat, to, false);
            else launch_wall_heat(s->stream, lv.dp.stride, lv.q, a);
        });
        if (kind == 2) { lv.fluxes_zero = false; lv.fluxes_stale = false; }
        HIP_CHECK(hipStreamSynchronize(s->stream));         // (before the local area goes)
    });
}

// ---- wall distance, wall spacing, wall damping (INTEGRATION.md "Wall distance") ----
// what every call below that computes or frees refuses: a rank holds part of the wall only
static void wall_distance_require_whole(const mgcfd_solver *s)
{
    if (s->partitioned || s->comm)
        throw std::invalid_argument("wall distance: not on a partitioned solver, a group member or a rank (a rank holds part of the wall only)");
}
int mgcfd_compute_wall_distance(mgcfd_solver *s, int levels)
{
    REQUIRE(s);
    return guarded([&] {
        if (levels < 1 || levels > static_cast<int>(s->L.size())) throw std::invalid_argument("wall distance: levels must be 1 .. mgcfd_num_levels");
        wall_distance_require_whole(s);
        for (int l = 0; l < levels; l++)
            if (!s->L[static_cast<size_t>(l)].wall_d && s->L[static_cast<size_t>(l)].coords.empty())
                throw std::invalid_argument("wall distance: level " + std::to_string(l) + " was created without coordinates");
        require_no_sweep_under_way(s, "wall distance");
        s->use_device();
        for (int l = 0; l < levels; l++) compute_level_wall_distance(s, s->L[static_cast<size_t>(l)]);
    });
}
int mgcfd_get_wall_distance(const mgcfd_solver *s, int *levels)
{
    REQUIRE(s);
    int n = 0;
    while (n < static_cast<int>(s->L.size()) && s->L[static_cast<size_t>(n)].wall_d) n++;
    if (levels) *levels = n;
    return MGCFD_OK;
}
int mgcfd_release_wall_distance(mgcfd_solver *s)
{
    REQUIRE(s);
    return guarded([&] {
        wall_distance_require_whole(s);
        if (s->damping_in_effect()) throw std::invalid_argument("wall distance: the wall damping is in effect (mgcfd_set_wall_damping): switch it off first");
        if (s->sa_in_effect()) throw std::invalid_argument("wall distance: the Spalart-Allmaras model is in effect (mgcfd_set_viscosity_model): switch it off first");
        require_no_sweep_under_way(s, "wall distance");
        s->use_device();
        HIP_CHECK(hipStreamSynchronize(s->stream));
        for (DeviceLevel &lv : s->L) {
            lv.mem.release(lv.wall_d); lv.mem.release(lv.wall_near);
            lv.wall_ids.clear(); lv.wall_ids.shrink_to_fit();
        }
    });
}
int mgcfd_wall_nearest(mgcfd_solver *s, int level, int64_t *nearest)
{
    REQUIRE(s); REQUIRE(nearest);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        if (!lv.wall_d) throw std::invalid_argument("mgcfd_wall_nearest: the level does not hold the wall distance (mgcfd_compute_wall_distance)");
        std::vector<int32_t> near(static_cast<size_t>(lv.dp.stride));
        HIP_CHECK(hipMemcpyAsync(near.data(), lv.wall_near, sizeof(int32_t) * near.size(), hipMemcpyDeviceToHost, s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
        for (int64_t n = 0; n < lv.info.nel; n++) {
            const int32_t j = near[static_cast<size_t>(n)];
            nearest[lv.plan.old_of_new[static_cast<size_t>(n)]] = j < 0 ? -1 : lv.wall_ids[static_cast<size_t>(j)];
        }
    });
}
int mgcfd_wall_spacing(mgcfd_solver *s, int level, int64_t *node_ids, double *h)
{
    REQUIRE(s); REQUIRE(h);
    return guarded([&] {
        if (!s->level(level).wall_d) throw std::invalid_argument("mgcfd_wall_spacing: the level does not hold the wall distance (mgcfd_compute_wall_distance)");
        // (the plan's distribution table is free between calls: its first column block takes h)
        wall_table(s, level, node_ids, h, 1, [&](DeviceLevel &lv, WallPlan &wp) {
            WallSpacing a;
            a.wn = wp.wn; a.d = lv.wall_d; a.h = wp.dist;
            launch_wall_spacing(s->stream, a);
            return wp.dist;
        });
    });
}
int mgcfd_set_wall_damping(mgcfd_solver *s, int on, double kappa)
{
    REQUIRE(s);
    return guarded([&] {
        if (on != 0 && on != 1) throw std::invalid_argument("wall damping: on must be 0 or 1");
        if (!std::isfinite(kappa) || !(kappa > 0.0)) throw std::invalid_argument("wall damping: kappa must be finite and positive");
        if (on) wall_distance_require_whole(s);
        require_damping_possible(s, s->visc_levels, s->vm_eddy, on);
        quiesce(s, "wall damping");
        s->wd_on = on; s->wd_kappa = kappa;
        settle_wall_damping(s);
        HIP_CHECK(hipGetLastError());
    });
}
int mgcfd_get_wall_damping(const mgcfd_solver *s, int *on, double *kappa)
{
    REQUIRE(s);
    if (on) *on = s->wd_on;
    if (kappa) *kappa = s->wd_kappa;
    return MGCFD_OK;
}
// ---- Spalart-Allmaras model: the free-stream ratio and the launches' times (INTEGRATION.md "Spalart-Allmaras model") ----
int mgcfd_set_sa_free_stream(mgcfd_solver *s, double ratio, int reinitialise)
{
    REQUIRE(s);
    return guarded([&] {
        if (!std::isfinite(ratio) || !(ratio > 0.0)) throw std::invalid_argument("Spalart-Allmaras model: the free-stream ratio must be finite and positive");
        quiesce(s, "Spalart-Allmaras free stream");
        s->sa_ratio = ratio;
        if (!reinitialise) return;
        for (int l = 0; l < static_cast<int>(s->L.size()); l++)
            if (s->sa_on(l)) s->sa_form(s->L[static_cast<size_t>(l)], true);
        HIP_CHECK(hipStreamSynchronize(s->stream));
        HIP_CHECK(hipGetLastError());
    });
}
int mgcfd_get_sa_free_stream(const mgcfd_solver *s, double *ratio)
{
    REQUIRE(s);
    if (ratio) *ratio = s->sa_ratio;
    return MGCFD_OK;
}
// ---- the unsteady model: nt under dual time stepping, the DES97 and delayed-DES lengths (INTEGRATION.md "Unsteady Spalart-Allmaras") ----
int mgcfd_set_sa_unsteady(mgcfd_solver *s, int time_accurate, int length, double c_des)
{
    REQUIRE(s);
    return guarded([&] {
        if (time_accurate != 0 && time_accurate != 1) throw std::invalid_argument("unsteady Spalart-Allmaras: time_accurate must be 0 or 1");
        if (length != MGCFD_SA_LENGTH_WALL && length != MGCFD_SA_LENGTH_DES && length != MGCFD_SA_LENGTH_DDES)
            throw std::invalid_argument("unsteady Spalart-Allmaras: length must be MGCFD_SA_LENGTH_WALL, MGCFD_SA_LENGTH_DES or MGCFD_SA_LENGTH_DDES");
        if (!std::isfinite(c_des) || !(c_des > 0.0)) throw std::invalid_argument("unsteady Spalart-Allmaras: c_des must be finite and positive");
        if (s->partitioned || s->comm)
            throw std::invalid_argument("unsteady Spalart-Allmaras: not on a partitioned solver, a group member or a rank (the model does not run there)");
        if (!time_accurate && s->dual_time() && s->sa_in_effect())
            throw std::invalid_argument("unsteady Spalart-Allmaras: time_accurate cannot go off while dual time stepping is on and the model is in effect (nu_tilde would have no BDF source)");
        quiesce(s, "unsteady Spalart-Allmaras");
        const bool length_changed = length != s->sa_length || c_des != s->sa_cdes;
        s->sa_time_accurate = time_accurate; s->sa_length = length; s->sa_cdes = c_des;
        settle_sa_unsteady(s, length_changed);
        HIP_CHECK(hipGetLastError());
    });
}
int mgcfd_get_sa_unsteady(const mgcfd_solver *s, int *time_accurate, int *length, double *c_des)
{
    REQUIRE(s);
    if (time_accurate) *time_accurate = s->sa_time_accurate;
    if (length) *length = s->sa_length;
    if (c_des) *c_des = s->sa_cdes;
    return MGCFD_OK;
}
int mgcfd_bench_sa(mgcfd_solver *s, int level, int kind, int launches, double *avg_seconds)
{
    REQUIRE(s); REQUIRE(avg_seconds);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        if (!s->sa_on(level)) throw std::invalid_argument("the Spalart-Allmaras model is not in effect on this level (mgcfd_set_viscosity_model, mgcfd_set_viscous)");
        if (kind < 0 || kind > 2) throw std::invalid_argument("Spalart-Allmaras launch kind: 0 gradient, 1 transport, 2 restrict");
        if ((kind == 2) != (level > 0)) throw std::invalid_argument("Spalart-Allmaras launch kind: the gradient and the transport run on level 0, the restriction into a level >= 1");
        if (kind == 2) { *avg_seconds = s->timed_launches(launches, [&] { s->sa_restrict(level); }); return; }
        const SaStep a = s->sa_step(lv);
        s->sa_gradient(lv);                                 // (every array holds a stage's numbers; the transport writes the spare buffer: nt stays)
        *avg_seconds = s->timed_launches(launches, [&] {    // (the instantiations the settings select)
            if (kind == 0) s->sa_gradient(lv);
            else s->sa_launch_transport(lv, a);
        });
    });
}
int mgcfd_bench_wall_distance(mgcfd_solver *s, int level, int launches, double *avg_seconds)
{
    REQUIRE(s); REQUIRE(avg_seconds);
    return guarded([&] {
        s->use_device();
        DeviceLevel &lv = s->level(level);
        if (!lv.wall_d) throw std::invalid_argument("mgcfd_bench_wall_distance: the level does not hold the wall distance (mgcfd_compute_wall_distance)");
        const size_t st = static_cast<size_t>(lv.dp.stride), m = lv.wall_ids.size();
        std::vector<double> x(3 * st, 0.0), wx(3 * m);
        for (int64_t n = 0; n < lv.info.nel; n++)
            for (size_t c = 0; c < 3; c++) x[c * st + static_cast<size_t>(n)] = lv.coords[3 * static_cast<size_t>(lv.plan.old_of_new[static_cast<size_t>(n)]) + c];
        for (size_t j = 0; j < m; j++)
            for (size_t c = 0; c < 3; c++) wx[c * m + j] = lv.coords[3 * static_cast<size_t>(lv.wall_ids[j]) + c];
        DeviceOwner visiting;
        WallDistance a;
        a.x = visiting.upload(x); a.wx = visiting.upload(wx); a.m = static_cast<int32_t>(m);
        a.d = lv.wall_d; a.nearest = lv.wall_near;             // (the launches write what the arrays hold)
        *avg_seconds = s->timed_launches(launches, [&] { launch_wall_distance(s->stream, lv.info.nel, lv.dp.stride, a); });
        HIP_CHECK(hipStreamSynchronize(s->stream));
    });
}

int mgcfd_load_coefficients(const double ff17[17], const double loads6[6], double ref_area, double ref_length, double out6[6])
{
    REQUIRE(ff17); REQUIRE(loads6); REQUIRE(out6);
    if (!(ref_area > 0.0) || !(ref_length > 0.0) || !std::isfinite(ref_area) || !std::isfinite(ref_length)) {
        g_last_error = "mgcfd_load_coefficients: the reference area and length must be positive and finite";
        return MGCFD_ERR_ARG;
    }
    const double rho = ff17[0];
    const double vx = ff17[1] / rho, vy = ff17[2] / rho, vz = ff17[3] / rho;
    const double q = 0.5 * rho * (vx * vx + vy * vy + vz * vz);
    if (!(q > 0.0) || !std::isfinite(q)) {
        g_last_error = "mgcfd_load_coefficients: the far field has no positive dynamic pressure";
        return MGCFD_ERR_ARG;
    }
    const double alpha = std::atan2(vy, vx);              // the angle of attack lies in the x-y plane (cfd_loops.h:85-104)
    const double ca = std::cos(alpha), sa = std::sin(alpha);
    const double qs = q * ref_area, qsc = qs * ref_length;
    out6[0] = (loads6[0] * ca + loads6[1] * sa) / qs;     // CD
    out6[1] = (-loads6[0] * sa + loads6[1] * ca) / qs;    // CL
    out6[2] = loads6[2] / qs;                             // CS
    for (int k = 0; k < 3; k++) out6[3 + k] = loads6[3 + k] / qsc;
    return MGCFD_OK;
}

// ---- dual time stepping: the physical step, its time levels, the driver loop ----
static void require_dual_time(const mgcfd_solver *s, const char *who)
{
    if (!s->dual_time()) throw std::invalid_argument(std::string(who) + ": dual time stepping is off (mgcfd_set_dual_time)");
}
int mgcfd_set_dual_time(mgcfd_solver *s, double dt, double clamp)
{
    REQUIRE(s);
    return guarded([&] {
        if (!std::isfinite(dt) || dt < 0.0) throw std::invalid_argument("dual time: the physical step must be finite and positive (0 switches it off)");
        const bool on = dt > 0.0;
        if (on && (!std::isfinite(clamp) || !(clamp > 0.0))) throw std::invalid_argument("dual time: the clamp must be finite and positive");
        if (on && (s->partitioned || s->comm))
            throw std::invalid_argument("dual time: not on a partitioned solver or a rank (levels split over ranks are out of scope)");
        if (on && s->vm_eddy == MGCFD_EDDY_SPALART_ALLMARAS && !s->sa_time_accurate)
            throw std::invalid_argument("dual time: not while the Spalart-Allmaras model is selected (nu_tilde has no BDF source; mgcfd_set_sa_unsteady with time_accurate gives it one)");
        quiesce(s, "dual time");
        if (on && !s->dual_time()) {
            // switched on: both levels start as the current state (sweeps before the first begin_step see BDF1 against it)
            for (DeviceLevel &lv : s->L) {
                lv.flux_in = nullptr;               // (no flux launch has run under dual time yet: W is `variables`)
                if (!lv.time_n) lv.time_n = lv.mem.alloc<double>(static_cast<size_t>(5 * lv.dp.stride));
                if (!lv.time_n1) lv.time_n1 = lv.mem.alloc<double>(static_cast<size_t>(5 * lv.dp.stride));
            }
            for (DeviceLevel &lv : s->L) launch_dual_shift(s->stream, 5 * lv.dp.stride, lv.q, lv.time_n, lv.time_n1, 1);
            HIP_CHECK(hipStreamSynchronize(s->stream));
            HIP_CHECK(hipGetLastError());
            s->dual_levels = 0;
            s->dual_invalid_step = -1;
        }
        if (!on) {
            for (DeviceLevel &lv : s->L) { lv.mem.release(lv.time_n); lv.mem.release(lv.time_n1); lv.flux_in = nullptr; }
            s->dual_levels = 0;
        }
        s->dual_dt = dt;
        s->dual_clamp = on ? clamp : 0.0;
        settle_sa_unsteady(s);
        settle_rms_order(s);
        drop_look_ahead(s);
    });
}
int mgcfd_get_dual_time(const mgcfd_solver *s, double *dt, double *clamp, int *order, int *levels, int *invalid_step)
{
    REQUIRE(s);
    if (dt) *dt = s->dual_dt;
    if (clamp) *clamp = s->dual_clamp;
    if (order) *order = s->dual_order;
    if (levels) *levels = s->dual_levels;
    if (invalid_step) *invalid_step = s->dual_invalid_step;
    return MGCFD_OK;
}
int mgcfd_dual_time_set_order(mgcfd_solver *s, int order)
{
    REQUIRE(s);
    return guarded([&] {
        require_dual_time(s, "mgcfd_dual_time_set_order");
        if (order != 1 && order != 2) throw std::invalid_argument("dual time: the order is 1 (BDF1) or 2 (BDF2)");
        require_no_sweep_under_way(s, "dual time");
        s->dual_order = order;
    });
}
int mgcfd_dual_time_reset(mgcfd_solver *s)
{
    REQUIRE(s);
    return guarded([&] {
        require_dual_time(s, "mgcfd_dual_time_reset");
        require_no_sweep_under_way(s, "dual time");
        s->dual_levels = 0;
        DeviceLevel &l0 = s->L[0];
        if (l0.sa_ntn) { s->use_device(); launch_dual_shift(s->stream, l0.dp.stride, l0.sa_nt, l0.sa_ntn, l0.sa_ntn1, 1); }   // (nt's time levels: nt)
    });
}
// Wn1 <- Wn, Wn <- variables on every level (the first step: both <- variables); asynchronous on the solver's stream
static void dual_begin_step(mgcfd_solver *s)
{
    require_dual_time(s, "mgcfd_dual_time_begin_step");
    require_no_sweep_under_way(s, "dual time");
    for (DeviceLevel &lv : s->L)
        launch_dual_shift(s->stream, 5 * lv.dp.stride, lv.q, lv.time_n, lv.time_n1, s->dual_levels == 0 ? 1 : 0);
    DeviceLevel &l0 = s->L[0];
    if (l0.sa_ntn) {
        launch_dual_shift(s->stream, l0.dp.stride, l0.sa_nt, l0.sa_ntn, l0.sa_ntn1, s->dual_levels == 0 ? 1 : 0);   // (nt beside the state)
        // mut as a write of nt forms it, on every covered level: the step limit of the step's first sweep reads the array as it
        // stands, and so a physical step is a function of variables, Wn, Wn1, nt, ntn and ntn1 alone (a restart continues in bits)
        for (int l = 0; l < static_cast<int>(s->L.size()); l++)
            if (s->sa_on(l)) s->sa_form(s->L[static_cast<size_t>(l)], false);
    }
    s->dual_levels = s->dual_levels == 0 ? 1 : 2;
}
int mgcfd_dual_time_begin_step(mgcfd_solver *s) { OP(dual_begin_step(s)); }

// ---- flow statistics: time means and Reynolds stresses of level 0 (INTEGRATION.md "Flow statistics") ----
static void statistics_require_whole(const mgcfd_solver *s)
{
    if (s->partitioned || s->comm)
        throw std::invalid_argument("flow statistics: not on a partitioned solver, a group member or a rank (levels split over ranks are out of scope)");
}
static void statistics_require_on(const mgcfd_solver *s, const char *who)
{
    statistics_require_whole(s);
    if (s->stat_mode == MGCFD_STATISTICS_OFF) throw std::invalid_argument(std::string(who) + ": the flow statistics are off (mgcfd_set_statistics)");
    require_no_sweep_under_way(s, "flow statistics");
}
static void statistics_require_wall(const mgcfd_solver *s, const char *who)
{
    statistics_require_on(s, who);
    if (s->stat_mode != MGCFD_STATISTICS_VOLUME_AND_WALL)
        throw std::invalid_argument(std::string(who) + ": the wall statistics are off (mgcfd_set_statistics with MGCFD_STATISTICS_VOLUME_AND_WALL)");
}
// the wall table and the distribution table its samples are formed in: held exactly in mode 2 on a level with solid walls; zeroed
static void statistics_settle_wall(mgcfd_solver *s)
{
    DeviceLevel &lv = s->L[0];
    if (s->stat_mode != MGCFD_STATISTICS_VOLUME_AND_WALL || lv.n_wall_rec == 0) {
        lv.mem.release(lv.stat_wall); lv.mem.release(lv.stat_dist);
        if (lv.stat_made_wp) { lv.wp.reset(); lv.stat_made_wp = false; }   // (the next call that needs the plan makes it again)
        return;
    }
    if (!lv.wp) lv.stat_made_wp = true;
    const size_t n = static_cast<size_t>(wall_plan(s, lv).wn.n);
    if (!lv.stat_wall) lv.stat_wall = lv.mem.alloc<double>(MGCFD_WALL_STATISTICS_COLUMNS * n);
    if (!lv.stat_dist) lv.stat_dist = lv.mem.alloc<double>(MGCFD_WALL_COLUMNS * n);
    HIP_CHECK(hipMemsetAsync(lv.stat_wall, 0, sizeof(double) * MGCFD_WALL_STATISTICS_COLUMNS * n, s->stream));
}
static void statistics_zero_volume(mgcfd_solver *s)
{
    DeviceLevel &lv = s->L[0];
    const size_t stride = static_cast<size_t>(lv.dp.stride);
    HIP_CHECK(hipMemsetAsync(lv.stat_mean, 0, sizeof(double) * 6 * stride, s->stream));
    HIP_CHECK(hipMemsetAsync(lv.stat_mom, 0, sizeof(double) * 7 * stride, s->stream));
}
// the launches of one sample with the factors a and w: the volume accumulation, and in mode 2 on a level with solid walls the
// wall-stress and wall-distribution launches into the solver's own table and the wall accumulation
static void statistics_launch_volume(mgcfd_solver *s, double a, double w)
{
    DeviceLevel &lv = s->L[0];
    const double *mut = (lv.visc_mut && lv.eddy_mode) ? lv.visc_mut : nullptr;
    launch_statistics_sample(s->stream, lv.info.nel, lv.dp.stride, lv.q, mut, lv.stat_mean, lv.stat_mom, a, w);
}
static void statistics_launch_wall(mgcfd_solver *s, double a, double w, bool form = true)
{
    DeviceLevel &lv = s->L[0];
    if (!lv.stat_wall) return;
    if (form) {
        const bool viscous = s->viscous_on(0);
        if (viscous) launch_wall_stress(s, 0);
        WallDistribution d;
        d.wn = lv.wp->wn; d.rec = lv.wall_rec; d.p_inf = s->p_inf; d.sw = viscous ? lv.wp->sw : nullptr; d.out = lv.stat_dist;
        launch_wall_distribution(s->stream, lv.dp.stride, lv.q, d);
    }
    launch_statistics_wall(s->stream, lv.wp->wn.n, lv.stat_dist, lv.stat_wall, a, w);
}
// one sample of level 0's current state with weight w (checked by the caller); asynchronous on the solver's stream
static void statistics_sample(mgcfd_solver *s, double w)
{
    s->use_device();
    const double wsum_new = s->stat_wsum + w;
    const double a = w / wsum_new;
    statistics_launch_volume(s, a, w);
    statistics_launch_wall(s, a, w);
    HIP_CHECK(hipGetLastError());
    s->stat_wsum = wsum_new;
    s->stat_samples++;
}
int mgcfd_set_statistics(mgcfd_solver *s, int mode)
{
    REQUIRE(s);
    return guarded([&] {
        if (mode != MGCFD_STATISTICS_OFF && mode != MGCFD_STATISTICS_VOLUME && mode != MGCFD_STATISTICS_VOLUME_AND_WALL)
            throw std::invalid_argument("flow statistics: the mode is MGCFD_STATISTICS_OFF, MGCFD_STATISTICS_VOLUME or MGCFD_STATISTICS_VOLUME_AND_WALL");
        statistics_require_whole(s);
        quiesce(s, "flow statistics");
        DeviceLevel &lv = s->L[0];
        const int was = s->stat_mode;
        s->stat_mode = mode;
        if (mode == MGCFD_STATISTICS_OFF) {
            lv.mem.release(lv.stat_mean); lv.mem.release(lv.stat_mom);
            s->stat_samples = 0; s->stat_wsum = 0.0;
        } else if (was == MGCFD_STATISTICS_OFF) {
            const size_t stride = static_cast<size_t>(lv.dp.stride);
            lv.stat_mean = lv.mem.alloc<double>(6 * stride);
            lv.stat_mom = lv.mem.alloc<double>(7 * stride);
            statistics_zero_volume(s);
            s->stat_samples = 0; s->stat_wsum = 0.0;
        }
        statistics_settle_wall(s);
        HIP_CHECK(hipStreamSynchronize(s->stream));
        HIP_CHECK(hipGetLastError());
    });
}
int mgcfd_get_statistics(const mgcfd_solver *s, int *mode, int64_t *samples, double *wsum)
{
    REQUIRE(s);
    if (mode) *mode = s->stat_mode;
    if (samples) *samples = s->stat_samples;
    if (wsum) *wsum = s->stat_wsum;
    return MGCFD_OK;
}
int mgcfd_statistics_reset(mgcfd_solver *s)
{
    REQUIRE(s);
    return guarded([&] {
        statistics_require_on(s, "mgcfd_statistics_reset");
        s->use_device();
        statistics_zero_volume(s);
        DeviceLevel &lv = s->L[0];
        if (lv.stat_wall)
            HIP_CHECK(hipMemsetAsync(lv.stat_wall, 0, sizeof(double) * MGCFD_WALL_STATISTICS_COLUMNS * static_cast<size_t>(lv.wp->wn.n), s->stream));
        s->stat_samples = 0; s->stat_wsum = 0.0;
    });
}
int mgcfd_statistics_sample(mgcfd_solver *s, double weight)
{
    REQUIRE(s);
    return guarded([&] {
        statistics_require_on(s, "mgcfd_statistics_sample");
        if (!std::isfinite(weight) || !(weight > 0.0)) throw std::invalid_argument("mgcfd_statistics_sample: the weight must be finite and positive");
        statistics_sample(s, weight);
    });
}
int mgcfd_statistics_restore(mgcfd_solver *s, int64_t samples, double wsum)
{
    REQUIRE(s);
    return guarded([&] {
        statistics_require_on(s, "mgcfd_statistics_restore");
        if (samples < 0) throw std::invalid_argument("mgcfd_statistics_restore: samples must be >= 0");
        if (!std::isfinite(wsum) || wsum < 0.0) throw std::invalid_argument("mgcfd_statistics_restore: wsum must be finite and >= 0");
        if ((samples == 0) != (wsum == 0.0)) throw std::invalid_argument("mgcfd_statistics_restore: samples and wsum are zero together or not at all");
        s->stat_samples = samples;
        s->stat_wsum = wsum == 0.0 ? 0.0 : wsum;           // (+0.0)
    });
}
int mgcfd_wall_statistics(mgcfd_solver *s, int64_t *node_ids, double *out)
{
    REQUIRE(s); REQUIRE(out);
    return guarded([&] {
        statistics_require_wall(s, "mgcfd_wall_statistics");
        wall_table(s, 0, node_ids, out, MGCFD_WALL_STATISTICS_COLUMNS, [&](DeviceLevel &lv, WallPlan &) { return lv.stat_wall; });
    });
}
int mgcfd_set_wall_statistics(mgcfd_solver *s, const double *in)
{
    REQUIRE(s); REQUIRE(in);
    return guarded([&] {
        statistics_require_wall(s, "mgcfd_set_wall_statistics");
        s->use_device();
        DeviceLevel &lv = s->L[0];
        if (!lv.stat_wall) return;                          // (no solid wall: n = 0)
        HIP_CHECK(hipMemcpyAsync(lv.stat_wall, in, sizeof(double) * MGCFD_WALL_STATISTICS_COLUMNS * static_cast<size_t>(lv.wp->wn.n), hipMemcpyHostToDevice, s->stream));
        HIP_CHECK(hipStreamSynchronize(s->stream));
    });
}
int mgcfd_statistics_derive(double wsum, const double *moments7, int64_t n, double *out8)
{
    REQUIRE(moments7); REQUIRE(out8);
    if (!std::isfinite(wsum) || !(wsum > 0.0) || n < 0) {
        g_last_error = "mgcfd_statistics_derive: wsum must be finite and positive, n >= 0";
        return MGCFD_ERR_ARG;
    }
    for (int64_t i = 0; i < n; i++) {
        const double *c = moments7 + 7 * i;
        double *o = out8 + 8 * i;
        for (int k = 0; k < 6; k++) o[k] = c[k] / wsum;
        o[6] = std::sqrt(c[6] / wsum);
        o[7] = 0.5 * ((o[0] + o[1]) + o[2]);
    }
    return MGCFD_OK;
}
int mgcfd_bench_statistics(mgcfd_solver *s, int kind, int launches, double *avg_seconds)
{
    REQUIRE(s); REQUIRE(avg_seconds);
    return guarded([&] {
        statistics_require_on(s, "mgcfd_bench_statistics");
        if (kind < 0 || kind > 1) throw std::invalid_argument("flow statistics launch kind: 0 volume sample, 1 wall accumulation");
        s->use_device();
        if (kind == 1) {
            statistics_require_wall(s, "mgcfd_bench_statistics");
            if (!s->L[0].stat_wall) throw std::invalid_argument("the level has no solid-wall edge");
            statistics_launch_wall(s, 0.0, 0.0);            // (the distribution table holds the current state's rows)
        }
        *avg_seconds = s->timed_launches(launches, [&] {
            if (kind == 0) statistics_launch_volume(s, 0.0, 0.0);
            else statistics_launch_wall(s, 0.0, 0.0, false);
        });
    });
}
// loads_out != nullptr: also the level-0 loads of `kind` of the state every physical step leaves, [steps][loads_width(kind)].
// Every step's launches store into the next row of the kind's history on the device; the rows held there are read back when it
// is full and at the end.
static int advance_impl(mgcfd_solver *s, int steps, int cycles_per_step, double *rms_out, double *loads_out, const double *ref_point, LoadsKind kind)
{
    REQUIRE(s);
    const size_t width = loads_width(kind);
    bool wall = false;                          // the loads are asked for and level 0 has a solid wall
    int held = 0;                               // history rows not yet read back, the last of them row `step`
    auto read_rows = [&](int step) {
        if (held == 0) return int(MGCFD_OK);
        return guarded([&] {
            loads_rows(s, kind, true, loads_out, size_t(step + 1 - held), size_t(held), size_t(step + 1));
            HIP_CHECK(hipStreamSynchronize(s->stream));
            held = 0;
        });
    };
    int rc = guarded([&] {
        require_dual_time(s, "mgcfd_advance");
        if (steps < 0 || cycles_per_step < 1) throw std::invalid_argument("mgcfd_advance (dual time): steps >= 0 and cycles_per_step >= 1");
        if (int64_t(steps) * cycles_per_step > MGCFD_MAX_ADVANCE_CYCLES)
            throw std::invalid_argument("mgcfd_advance (dual time): at most " + std::to_string(MGCFD_MAX_ADVANCE_CYCLES) + " cycles per call (steps * cycles_per_step)");
        if (loads_out) {
            loads_require_whole(s);
            s->use_device();
            loads_upload_ref(s, ref_point);
            ensure_loads_ring(s, kind);
            wall = s->L[0].n_wall_rec > 0;
            if (wall) loads_plan(s, s->L[0], kind);
            else loads_rows(s, kind, false, loads_out, 0, size_t(steps), size_t(steps));     // (no solid wall: zeros, nothing launched)
        }
        s->dual_invalid_step = -1;
    });
    if (rc != MGCFD_OK) return rc;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int step = 0; step < steps; step++) {
        double *rms = rms_out ? rms_out + size_t(step) * size_t(cycles_per_step) : nullptr;
        rc = mgcfd_dual_time_begin_step(s);
        if (rc == MGCFD_OK) rc = run_cycles_impl(s, cycles_per_step, rms, nullptr, nullptr);
        // the flow statistics: one sample of the completed step with weight dt, behind the loads launch
        const auto sample = [&] { if (s->stat_mode != MGCFD_STATISTICS_OFF) statistics_sample(s, s->dual_dt); };
        if (rc == MGCFD_OK && wall) {
            rc = guarded([&] {
                s->use_device();
                launch_loads(s, 0, kind, LoadsDest::at(s->loads_ring[static_cast<int>(kind)] + size_t(held) * width));
                sample();
            });
            if (rc == MGCFD_OK) held++;
            if (rc == MGCFD_OK && (held == mgcfd_solver::kRmsRing || step + 1 == steps)) rc = read_rows(step);
        }
        else if (rc == MGCFD_OK) rc = guarded(sample);
        if (rc == MGCFD_OK) continue;
        (void)read_rows(step - 1);                                 // (the steps that completed keep their rows)
        // as mgcfd_run_cycles: what did not complete is NaN (the failing step's RMS entries are already), later steps do not run
        if (rc >= MGCFD_ERR_NAN && rc <= MGCFD_ERR_NEG_ENERGY) s->dual_invalid_step = step;
        for (int k = step + 1; rms_out && k < steps; k++)
            for (int c = 0; c < cycles_per_step; c++) rms_out[size_t(k) * size_t(cycles_per_step) + size_t(c)] = nan;
        if (loads_out) loads_rows(s, kind, wall, loads_out, size_t(step), 0, size_t(steps));
        return rc;
    }
    return MGCFD_OK;
}
int mgcfd_advance(mgcfd_solver *s, int steps, int cycles_per_step, double *rms_out, double *loads_out, const double ref_point[3])
{
    return advance_impl(s, steps, cycles_per_step, rms_out, loads_out, ref_point, LoadsKind::Pressure);
}
int mgcfd_advance_loads_viscous(mgcfd_solver *s, int steps, int cycles_per_step, double *rms_out, double *loads_out, const double ref_point[3])
{
    REQUIRE(loads_out);
    return advance_impl(s, steps, cycles_per_step, rms_out, loads_out, ref_point, LoadsKind::Friction);
}
int mgcfd_advance_loads_heat(mgcfd_solver *s, int steps, int cycles_per_step, double *rms_out, double *loads_out, const double ref_point[3])
{
    REQUIRE(loads_out);
    return advance_impl(s, steps, cycles_per_step, rms_out, loads_out, ref_point, LoadsKind::Heat);
}

} // extern "C"
