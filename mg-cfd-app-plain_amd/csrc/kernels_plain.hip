// kernels_plain.hip — the kernels that exist once, with their launchers (kernels.hpp: the prototypes in namespace mgcfd):
// copies, packing and signalling, reductions in a stated order, the surface loads, the wall fields, the step-factor limits.
// Compiled ONCE, with -ffp-contract=off: nothing here is ever contracted, whichever flavour the solver runs, so what these
// kernels produce is a bitwise function of their input.  The kernels of the two-flavour launchers are in kernels.hip; what
// the two files share is in kernel_device.hpp.
#include "kernel_device.hpp"

namespace mgcfd {

// ------------------------------------------------------------------------------------------
// initialize_variables (cfd_loops.h:44-55).  Runs over the padded length so the tail of every
// field holds valid numbers.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_init_variables(int64_t stride, FarField ff, double *__restrict__ q)
{
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (i >= stride) return;
    store_conserved(q, stride, i, ff.var[0], ff.var[1], ff.var[2], ff.var[3], ff.var[4]);
}

// partial minima -> one scalar (only needed where the scalar itself is the interface: the
// kernel-granular API and the multi-GPU all-reduce hook)
__global__ void __launch_bounds__(kBlock)
k_min_reduce(const double *__restrict__ partial_min, int n_partial, double *__restrict__ out)
{
    const double m = block_min_of_partials(partial_min, n_partial);
    if (threadIdx.x == 0) out[0] = m;
}

// ------------------------------------------------------------------------------------------
// FAS multigrid (no reference counterpart; INTEGRATION.md "FAS multigrid"): on a level >= 1 every stage's update takes
// F' = R + P for R, the level's total residual (fluxes, + the JST correction, - the dual-time source), P the forcing of the
// cycle's down leg.  The forcing is the last addition; one IEEE operation per line of the definition (include/mgcfd.h).
// The update itself is k_time_step_src<SRC, true> (kernels.hip).
// ------------------------------------------------------------------------------------------
// ... and with residual smoothing on: fluxes = F' for every node of the level before the Jacobi iterations, as k_dual_source
// (which runs first where dual time is on); n = 5 * stride, padding included (P's padding is zero).
__global__ void __launch_bounds__(kBlock)
k_fas_add_forcing(int64_t n, double *__restrict__ fluxes, const double *__restrict__ forcing)
{
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (i >= n) return;
    fluxes[i] = fluxes[i] + forcing[i];
}

// The forcing of the coarse level: P = Q - R(W0) where the coarse node has children (Q, the children's summed residuals, is
// what k_restrict_fas left in P), +0.0 where it has none.
__global__ void __launch_bounds__(kBlock)
k_fas_forcing(int64_t nel_coarse, int64_t stride_coarse, const int32_t *__restrict__ child_ptr,
              const double *__restrict__ fluxes, double *__restrict__ forcing)
{
    const int64_t c = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (c >= nel_coarse) return;
    const bool has_children = child_ptr[c + 1] > child_ptr[c];
#pragma unroll
    for (int v = 0; v < 5; v++) {
        const int64_t at = v * stride_coarse + c;
        forcing[at] = has_children ? forcing[at] - fluxes[at] : 0.0;
    }
}

// The pseudo step's clamp (the source is explicit in pseudo-time): sf = min(sf, (clamp * dt) / vol); cdt = clamp * dt.
__global__ void __launch_bounds__(kBlock)
k_dual_clamp(int64_t nel, double cdt, const double *__restrict__ volumes, double *__restrict__ step_factors)
{
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (i >= nel) return;
    const double sf = step_factors[i], cap = cdt / volumes[i];
    step_factors[i] = cap < sf ? cap : sf;              // (a NaN factor stays NaN, as the invalid-state check expects)
}

// The time levels advance: Wn1 <- Wn (first: <- variables), Wn <- variables; n = 5 * stride, padding included.
__global__ void __launch_bounds__(kBlock)
k_dual_shift(int64_t n, const double *__restrict__ q, double *__restrict__ wn, double *__restrict__ wn1, int first)
{
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (i >= n) return;
    const double now = q[i];
    wn1[i] = first ? now : wn[i];
    wn[i] = now;
}

// The viscous limit on final step factors: sf = min(sf, (k0 * rho) * g), k0 = cfl_v / (kv * mu), g = cbrt(vol)^2 / vol from the host.
__global__ void __launch_bounds__(kBlock)
k_viscous_clamp(int64_t nel, double k0, const double *__restrict__ rho, const double *__restrict__ g, double *__restrict__ step_factors)
{
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (i >= nel) return;
    const double sf = step_factors[i], cap = (k0 * rho[i]) * g[i];
    step_factors[i] = cap < sf ? cap : sf;              // (a NaN factor stays NaN, as the invalid-state check expects)
}

// The limit under a variable viscosity (mgcfd_set_viscosity_model): sf = min(sf, ((cfl_v * rho) * g) / d), d = max((4/3) (mu_i +
// mut_i), GAMMA (mu_i / prandtl + mut_i / prandtl_t)) with mu_i by the law from the level's state and mut_i as the array holds it.
__global__ void __launch_bounds__(kBlock)
k_viscous_clamp_variable(int64_t nel, int64_t stride, ViscousClamp a)
{
#pragma clang fp contract(off)
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (i >= nel) return;
    const double rho = a.q[i];
    const Derived dv = derive(rho, a.q[stride + i], a.q[2 * stride + i], a.q[3 * stride + i], a.q[4 * stride + i]);
    const double mu_i = viscosity_of(a.model, a.mu, dv.p / rho);
    const double mut = a.model.eddy != 0 ? a.model.mut[i] : 0.0;
    const double da = (4.0 / 3.0) * (mu_i + mut), db = kGamma * (mu_i / a.model.prandtl + mut / a.model.prandtl_t);
    const double d = da < db ? db : da;
    const double sf = a.step_factors[i], cap = ((a.cfl_v * rho) * a.g[i]) / d;
    a.step_factors[i] = cap < sf ? cap : sf;            // (a NaN factor stays NaN, as the invalid-state check expects)
}

// The no-slip wall: momentum +0.0 at the n listed nodes of q (and of q2, where given: FAS's copy of a restricted state);
// where the launch before wrote residuals, the residual of the clamped state, +0.0 - old.
__global__ void __launch_bounds__(kBlock)
k_viscous_wall(int64_t n, int64_t stride, const int32_t *__restrict__ nodes, double *__restrict__ q, double *__restrict__ q2,
               const double *__restrict__ old_variables, double *__restrict__ residuals)
{
    const int64_t k = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (k >= n) return;
    const int64_t i = nodes[k];
#pragma unroll
    for (int v = 1; v <= 3; v++) {
        q[v * stride + i] = 0.0;
        if (q2) q2[v * stride + i] = 0.0;
        if (residuals) residuals[v * stride + i] = 0.0 - old_variables[v * stride + i];
    }
}

// check_for_invalid_variables as a standalone sweep
__global__ void __launch_bounds__(kBlock)
k_check_invalid(int64_t nel, int64_t stride, const double *__restrict__ q, const int32_t *__restrict__ old_of_new,
                unsigned long long *__restrict__ err)
{
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (i >= nel) return;
    const double v0 = q[i], v1 = q[stride + i], v2 = q[2 * stride + i], v3 = q[3 * stride + i], v4 = q[4 * stride + i];
    const bool finite = isfinite(v0) && isfinite(v1) && isfinite(v2) && isfinite(v3) && isfinite(v4);
    int code = 0;
    if (!finite) code = 1;
    else if (v0 < 0.0) code = 2;
    else if (v4 < 0.0) code = 3;
    if (code) atomicMin(err, err_key(1, old_of_new[i], code));
}

// The level-0 sum of squares under dual time stepping, in an order that is a function of the ORIGINAL node numbering alone
// (include/mgcfd.h states it, tests/dual_time_emulator.py repeats it in numpy): a workgroup takes 256 consecutive original
// nodes, a lane its node's five squares added one after another from +0.0 (a lane past the last node: +0.0), a wave the
// pairwise tree of wave_sum (lane i with lane i ^ 32, then ^ 16, ... ^ 1), lane 0 of the workgroup the four waves' sums one
// after another.  k_sum_partials adds the workgroups' sums up.  Never contracted, as everything in this file.
__global__ void __launch_bounds__(kBlock)
k_sumsq_original(int64_t nel, int64_t stride, const double *__restrict__ x, const int32_t *__restrict__ new_of_old,
                 double *__restrict__ partial)
{
    __shared__ double s[kBlock / 64];
    const int64_t o = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    double acc = 0.0;
    if (o < nel) {
        const int64_t i = new_of_old[o];
        for (int f = 0; f < 5; f++) { const double v = x[f * stride + i]; acc += v * v; }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < kBlock / 64; w++) t += s[w];
        partial[blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(kBlock)
k_sum_partials(SumTask task)
{
    block_sum_partials(task);
}

// ------------------------------------------------------------------------------------------
// Halo exchange of a partitioned level: pack n nodes' 5 values into a contiguous [n][5] message
// (what an RCCL send/recv moves) and unpack a received message into the ghost nodes.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_halo_pack(int64_t n, int64_t stride, const int32_t *__restrict__ idx, const double *__restrict__ field, double *__restrict__ msg)
{
    const int64_t k = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (k >= n) return;
    const int64_t i = idx[k];
    for (int f = 0; f < 5; f++) msg[k * 5 + f] = field[f * stride + i];
}

__global__ void __launch_bounds__(kBlock)
k_halo_unpack(int64_t n, int64_t stride, const int32_t *__restrict__ idx, const double *__restrict__ msg, double *__restrict__ field)
{
    const int64_t k = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (k >= n) return;
    const int64_t i = idx[k];
    for (int f = 0; f < 5; f++) field[f * stride + i] = msg[k * 5 + f];
}

// The message of a partitioned level stored straight into the neighbours' ghost slots: slot k of the message is node idx[k]
// here and node target[k] in the numbering of the peer whose segment k lies in.  One launch replaces pack, the copies (or
// send/receive) and the peers' unpack launches; the stores cross xGMI (peer access) or stay on the device.
__global__ void __launch_bounds__(kBlock)
k_halo_push(int64_t n, int64_t stride, const int32_t *__restrict__ idx, const int32_t *__restrict__ target,
            const double *__restrict__ field, PushPeers peers)
{
    const int64_t k = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (k >= n) return;
    double *dst = peers.base[0];
    int64_t ps = peers.stride[0];
#pragma unroll
    for (int p = 1; p < kMaxPushPeers; p++)                          // (selects, no indexed access to the argument block)
        if (p < peers.n && k >= peers.first[p]) { dst = peers.base[p]; ps = peers.stride[p]; }
    const int64_t i = idx[k], g = target[k];
    for (int f = 0; f < 5; f++) dst[f * ps + g] = field[f * stride + i];
}

// The same between PROCESSES (the peers' buffers opened through HIP IPC): the push also tells every peer that the message is
// complete, by a sequence number in a word of the peer's memory.  Every wave drains its stores, the workgroup counts itself
// off (device-scope ticket), and the workgroup that counts last raises the flags behind a system-scope release — so a peer
// that reads the number finds the whole message.  The receiver does not poll inside a compute kernel: k_flags_wait is a
// launch of its own in front of the boundary tiles (one wave; it gives up after about two seconds and says so), and the
// boundary launch behind it starts with the acquire every launch starts with.
__global__ void __launch_bounds__(kBlock)
k_halo_push_flags(int64_t n, int64_t stride, const int32_t *__restrict__ idx, const int32_t *__restrict__ target,
                  const double *__restrict__ field, PushPeers peers, PushFlags flags, unsigned *__restrict__ ticket)
{
    const int64_t k = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (k < n) {
        double *dst = peers.base[0];
        int64_t ps = peers.stride[0];
#pragma unroll
        for (int p = 1; p < kMaxPushPeers; p++)
            if (p < peers.n && k >= peers.first[p]) { dst = peers.base[p]; ps = peers.stride[p]; }
        const int64_t i = idx[k], g = target[k];
        for (int f = 0; f < 5; f++) dst[f * ps + g] = field[f * stride + i];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // this wave's stores have been acknowledged
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence_system();
        const unsigned done = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (done == gridDim.x - 1) {
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // (the next push starts from zero again)
            __threadfence_system();
#pragma unroll
            for (int p = 0; p < kMaxPushPeers; p++)
                if (p < flags.n) __hip_atomic_store(flags.flag[p], flags.value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// wait until the flag words [row][slot] of the given source ranks have reached `value` (see above); *timed_out counts the waits that gave up
__global__ void k_flags_wait(const unsigned long long *__restrict__ flags, FlagRows rows, int slot, unsigned long long value,
                             int *__restrict__ timed_out)
{
    const int p = threadIdx.x;
    int row = rows.row[0];
#pragma unroll
    for (int q = 1; q < kMaxIpcRanks; q++) if (q == p) row = rows.row[q];         // (selects, no indexed access to the argument block)
    if (p >= rows.n) return;
    const unsigned long long *w = flags + row * 4 + slot;
    const unsigned long long t0 = wall_clock64();                       // (100 MHz)
    while (__hip_atomic_load(w, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < value) {
        __builtin_amdgcn_s_sleep(64);
        if (wall_clock64() - t0 > 200000000ull) { atomicAdd(timed_out, 1); break; }
    }
}

// this rank's time-step minimum into every rank's array, then their flags (one lane per destination rank)
__global__ void k_min_publish(const double *__restrict__ my_min, MinPublish mp)
{
    const int p = threadIdx.x;
    double *dst = mp.mins[0];
    unsigned long long *flag = mp.flag[0];
#pragma unroll
    for (int q = 1; q < kMaxIpcRanks; q++) if (q == p) { dst = mp.mins[q]; flag = mp.flag[q]; }
    if (p >= mp.world) return;
    const double v = *my_min;
    __hip_atomic_store(dst + mp.parity * kMaxIpcRanks + mp.me, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (p == mp.me) return;
    __threadfence_system();
    __hip_atomic_store(flag, mp.value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One multigrid level per rank: the restricted variables arrive from the rank that holds the finer level as a whole
// [5][stride] array.  mg_restrict leaves a coarse node WITHOUT children at its old value (mg_loops.cpp:63-78,174-189),
// and only the rank that sweeps the coarse level has that value: take the message for nodes with children only.
__global__ void __launch_bounds__(kBlock)
k_accept_restricted(int64_t nel_coarse, int64_t stride_coarse, const int32_t *__restrict__ child_ptr,
                    const double *__restrict__ src, double *__restrict__ coarse_q)
{
    const int64_t c = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (c >= nel_coarse || child_ptr[c + 1] == child_ptr[c]) return;
    for (int f = 0; f < 5; f++) coarse_q[f * stride_coarse + c] = src[f * stride_coarse + c];
}

// In-process groups (several solvers of one process, peer access between their devices): the all-reduce(MIN) of the
// time step is every rank reading the others' scalars directly (8-byte loads over xGMI) behind their events.
__global__ void k_min_over_peers(const double *const *__restrict__ scalars, int n, double *__restrict__ out)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double m = scalars[0][0];
        for (int r = 1; r < n; r++) m = fmin(m, scalars[r][0]);
        out[0] = m;
    }
}

// rms history: append a device scalar to a ring (lets a whole multigrid cycle live in one hipGraph)
__global__ void k_append_scalar(const double *__restrict__ src, double *__restrict__ ring, int *__restrict__ count, int cap)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const int k = *count;
        if (k < cap) ring[k] = src[0];
        *count = k + 1;
    }
}

// ------------------------------------------------------------------------------------------
// Surface loads: the pressure force and moment on the solid walls, sum over the solid-wall edges (neighbour code -1) of
// the term compute_boundary_flux_edge adds to the momentum residual (flux_boundary_kernel.elemfunc.c), with the far-field
// pressure taken off: f = (p_b - p_inf) * (x, y, z), m = (c_b - ref) x f.  Summation order fixed: chunks
// of 256 edges reduced by the stride-halving tree v[t] += v[t + s], s = 128 .. 1 (stage A, one workgroup per chunk), then
// the same over the list of partial sums until one value is left (stage B, the workgroup that arrives last).  Never
// contracted to FMA, whichever flavour the solver runs, so the loads are a bitwise function of the state.
// ------------------------------------------------------------------------------------------
// The tree over the 256 lanes' six values; lane 0 holds the sums.  s = 128, 64 through LDS, s < 64 by shuffles within
// wave 0 (lane t adds lane t + s: the same operand pairs).
// NC columns: six for the pressure loads, twelve with the friction loads beside them (k_surface_loads_viscous).
template <int NC>
__device__ __forceinline__ void loads_tree(double (&v)[NC], double (&sh)[NC][kBlock])
{
#pragma clang fp contract(off)
    const int t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < NC; c++) sh[c][t] = v[c];
    __syncthreads();
    if (t < 128) {
#pragma unroll
        for (int c = 0; c < NC; c++) v[c] += sh[c][t + 128];
    }
    __syncthreads();
    if (t < 128) {
#pragma unroll
        for (int c = 0; c < NC; c++) sh[c][t] = v[c];
    }
    __syncthreads();
    if (t < 64) {
#pragma unroll
        for (int c = 0; c < NC; c++) v[c] += sh[c][t + 64];
        for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
            for (int c = 0; c < NC; c++) v[c] += __shfl_down(v[c], s, 64);
        }
    }
    __syncthreads();                                                   // (sh is free again)
}

template <int NC>
__device__ __forceinline__ void loads_store(const LoadsTask &task, const double (&v)[NC])
{
    if (task.out) {
#pragma unroll
        for (int c = 0; c < NC; c++) task.out[c] = v[c];
    }
    if (task.ring) {
        const int k = *task.count - 1;                                 // the row of the cycle whose RMS was appended last
        if (k >= 0 && k < task.cap) {
#pragma unroll
            for (int c = 0; c < NC; c++) task.ring[int64_t(k) * NC + c] = v[c];
        }
    }
}

__global__ void __launch_bounds__(kBlock)
k_surface_loads(int64_t stride, const double *__restrict__ q, LoadsTask task)
{
#pragma clang fp contract(off)
    __shared__ double sh[6][kBlock];
    __shared__ int last;
    const int t = threadIdx.x;
    const int64_t e = int64_t(blockIdx.x) * kBlock + t;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (e < task.n) {
        const WallRecord r = task.rec[e];
        const int64_t b = r.node;
        const double rho = q[b], mx = q[stride + b], my = q[2 * stride + b], mz = q[3 * stride + b], en = q[4 * stride + b];
        // derive()'s pressure, written out here so that the pragma above covers it (cfd_loops.h:121-148)
        const double vx = mx / rho, vy = my / rho, vz = mz / rho;
        const double speed_sqd = vx * vx + vy * vy + vz * vz;
        const double p = (kGamma - 1.0) * (en - 0.5 * rho * speed_sqd);
        const double dp = p - task.p_inf;
        const double fx = dp * r.x, fy = dp * r.y, fz = dp * r.z;
        const double rx = r.cx - task.ref[0], ry = r.cy - task.ref[1], rz = r.cz - task.ref[2];
        v[0] = fx; v[1] = fy; v[2] = fz;
        v[3] = ry * fz - rz * fy;
        v[4] = rz * fx - rx * fz;
        v[5] = rx * fy - ry * fx;
    }
    loads_tree(v, sh);                                                 // stage A
    const int nb = int(gridDim.x);
    if (nb == 1) {
        if (t == 0) loads_store(task, v);
        return;
    }
    if (t == 0) {
#pragma unroll
        for (int c = 0; c < 6; c++) task.partial[int64_t(c) * nb + blockIdx.x] = v[c];
        const unsigned done = __hip_atomic_fetch_add(task.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last = done == unsigned(nb - 1);
        if (last) __hip_atomic_store(task.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a graph replay starts from zero)
    }
    __syncthreads();
    if (!last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");                  // every lane sees the other workgroups' partials
    // stage B: the list of partials reduced by the same tree, chunk by chunk, in place (chunk k's sum lands in slot k,
    // which chunk k has already read or an earlier chunk has), until one value is left
    for (int n = nb; n > 1;) {
        const int m = (n + kBlock - 1) / kBlock;
        for (int k = 0; k < m; k++) {
            const int i = k * kBlock + t;
#pragma unroll
            for (int c = 0; c < 6; c++) v[c] = i < n ? task.partial[int64_t(c) * nb + i] : 0.0;
            loads_tree(v, sh);
            if (t == 0) {
#pragma unroll
                for (int c = 0; c < 6; c++) task.partial[int64_t(c) * nb + k] = v[c];
            }
            __syncthreads();
        }
        n = m;
    }
    if (t == 0) loads_store(task, v);
}

// The same loads of a level split over ranks ("Surface loads": the partitioned form), in two launches.
// k_loads_terms, on every rank: one lane per solid-wall edge the rank holds, the six terms by the expressions of
// k_surface_loads, stored at the edge's slot of the terms table [6][row] — the whole level's order, on the gathering
// rank's device (plain stores over xGMI, as k_halo_push's) — or, slot == nullptr, at the lane's own index of a compact
// buffer that travels as a message and is placed by k_loads_scatter.  Terms move by stores and copies only.
__global__ void __launch_bounds__(kBlock)
k_loads_terms(int64_t stride, const double *__restrict__ q, LoadsTerms task)
{
#pragma clang fp contract(off)
    const int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= task.n) return;
    const WallRecord r = task.rec[e];
    const int64_t b = r.node;
    const double rho = q[b], mx = q[stride + b], my = q[2 * stride + b], mz = q[3 * stride + b], en = q[4 * stride + b];
    const double vx = mx / rho, vy = my / rho, vz = mz / rho;
    const double speed_sqd = vx * vx + vy * vy + vz * vz;
    const double p = (kGamma - 1.0) * (en - 0.5 * rho * speed_sqd);
    const double dp = p - task.p_inf;
    const double fx = dp * r.x, fy = dp * r.y, fz = dp * r.z;
    const double rx = r.cx - task.ref[0], ry = r.cy - task.ref[1], rz = r.cz - task.ref[2];
    const int64_t at = task.slot ? int64_t(task.slot[e]) : e;
    double *dst = task.table + at;
    dst[0] = fx; dst[task.row] = fy; dst[2 * task.row] = fz;
    dst[3 * task.row] = ry * fz - rz * fy;
    dst[4 * task.row] = rz * fx - rx * fz;
    dst[5 * task.row] = rx * fy - ry * fx;
}

// a rank's compact terms [6][src_row] into the table, by slot (the gathering rank, behind the message's arrival)
__global__ void __launch_bounds__(kBlock)
k_loads_scatter(int64_t n, const double *__restrict__ src, int64_t src_row, const int32_t *__restrict__ slot,
                double *__restrict__ table, int64_t row)
{
    const int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (k >= n) return;
    const int64_t at = slot[k];
#pragma unroll
    for (int c = 0; c < 6; c++) table[c * row + at] = src[c * src_row + k];
}

// k_loads_reduce, on the gathering rank: k_surface_loads with the term evaluation replaced by a coalesced read of the
// table — workgroup k takes lanes [256 k, 256 k + 256) of every row (pad lanes hold +0.0, what k_surface_loads gives a lane
// past the last edge), the same trees, the same ticket.  task.n = the whole level's edge count, task.rec unused.
__global__ void __launch_bounds__(kBlock)
k_loads_reduce(const double *__restrict__ table, int64_t row, LoadsTask task)
{
#pragma clang fp contract(off)
    __shared__ double sh[6][kBlock];
    __shared__ int last;
    const int t = threadIdx.x;
    const int64_t e = int64_t(blockIdx.x) * kBlock + t;
    double v[6];
#pragma unroll
    for (int c = 0; c < 6; c++) v[c] = table[c * row + e];
    loads_tree(v, sh);                                                 // stage A
    const int nb = int(gridDim.x);
    if (nb == 1) {
        if (t == 0) loads_store(task, v);
        return;
    }
    if (t == 0) {
#pragma unroll
        for (int c = 0; c < 6; c++) task.partial[int64_t(c) * nb + blockIdx.x] = v[c];
        const unsigned done = __hip_atomic_fetch_add(task.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last = done == unsigned(nb - 1);
        if (last) __hip_atomic_store(task.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (the next call starts from zero)
    }
    __syncthreads();
    if (!last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    for (int n = nb; n > 1;) {                                          // stage B, as in k_surface_loads
        const int m = (n + kBlock - 1) / kBlock;
        for (int k = 0; k < m; k++) {
            const int i = k * kBlock + t;
#pragma unroll
            for (int c = 0; c < 6; c++) v[c] = i < n ? task.partial[int64_t(c) * nb + i] : 0.0;
            loads_tree(v, sh);
            if (t == 0) {
#pragma unroll
                for (int c = 0; c < 6; c++) task.partial[int64_t(c) * nb + k] = v[c];
            }
            __syncthreads();
        }
        n = m;
    }
    if (t == 0) loads_store(task, v);
}

// ------------------------------------------------------------------------------------------
// Viscous surface loads (INTEGRATION.md "Viscous surface loads"): the friction the no-slip or slip wall of a viscous level
// feeds into its nodes' momentum, g = -(tau . w) per solid-wall edge with tau the node's stresses, summed beside the
// pressure terms through the same trees.  The stresses come from k_wall_stress: pass 1 of the viscous terms (the
// expressions of k_viscous_stress_tile, in the same order) for the wall nodes alone, one lane per wall node over a CSR
// row of its internal incidences, so that the cost follows the wall and not the level and S stays as the last flux launch
// left it.  Never contracted to FMA.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_wall_stress(int64_t stride, const double *__restrict__ q, WallStress a)
{
#pragma clang fp contract(off)
    const int64_t k = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (k >= a.wn.n) return;
    const int64_t i = a.wn.node[k];
    const int32_t e0 = a.wn.int_ptr[k], e1 = a.wn.int_ptr[k + 1];
    const Primitive me = primitive_of(q, stride, i);
    const double vol = a.volumes[i];
    double ux = 0.0, uy = 0.0, uz = 0.0, vx = 0.0, vy = 0.0, vz = 0.0, wx = 0.0, wy = 0.0, wz = 0.0, tx = 0.0, ty = 0.0, tz = 0.0;
    for (int32_t e = e0; e < e1; e++) {
        const Primitive ot = primitive_of(q, stride, a.wn.int_nbr[e]);
        const double nx = a.wn.int_n[3 * int64_t(e)], ny = a.wn.int_n[3 * int64_t(e) + 1], nz = a.wn.int_n[3 * int64_t(e) + 2];
        const double du = ot.u - me.u, dv = ot.v - me.v, dw = ot.w - me.w, dT = ot.T - me.T;
        ux += du * nx; uy += du * ny; uz += du * nz;
        vx += dv * nx; vy += dv * ny; vz += dv * nz;
        wx += dw * nx; wy += dw * ny; wz += dw * nz;
        tx += dT * nx; ty += dT * ny; tz += dT * nz;
    }
    const double gux = (0.5 * ux) / vol, guy = (0.5 * uy) / vol, guz = (0.5 * uz) / vol;
    const double gvx = (0.5 * vx) / vol, gvy = (0.5 * vy) / vol, gvz = (0.5 * vz) / vol;
    const double gwx = (0.5 * wx) / vol, gwy = (0.5 * wy) / vol, gwz = (0.5 * wz) / vol;
    const double gtx = (0.5 * tx) / vol, gty = (0.5 * ty) / vol, gtz = (0.5 * tz) / vol;
    const double div = (gux + gvy) + gwz;
    const double tt = (2.0 / 3.0) * div;
    double mu_e = a.mu, kap = a.kappa;
    if (a.model.variable()) {                          // the stress launch's model, eddy 2 formed here and stored nowhere
        const ViscosityModel &m = a.model;
        const double mu_i = viscosity_of(m, a.mu, me.T);
        double mut = 0.0;
        if (m.eddy == 1) mut = m.mut[i];
        else if (m.eddy == 2) mut = smagorinsky_of(m, m.d2[i], q[i], gux, guy, guz, gvx, gvy, gvz, gwx, gwy, gwz);
        mu_e = mu_i + mut;
        kap = m.cp * (mu_i / m.prandtl + mut / m.prandtl_t);
    }
    double out[12];
    out[0] = me.u; out[1] = me.v; out[2] = me.w;
    out[3] = mu_e * (2.0 * gux - tt); out[4] = mu_e * (2.0 * gvy - tt); out[5] = mu_e * (2.0 * gwz - tt);
    out[6] = mu_e * (guy + gvx); out[7] = mu_e * (guz + gwx); out[8] = mu_e * (gvz + gwy);
    out[9] = kap * gtx; out[10] = kap * gty; out[11] = kap * gtz;
#pragma unroll
    for (int f = 0; f < 12; f++) a.sw[f * a.wn.n + k] = out[f];
}

// ------------------------------------------------------------------------------------------
// Wall distance (INTEGRATION.md "Wall distance"): every node's distance to the nearest wall NODE of its level, an exact
// all-pairs minimum — no search radius, no tree.  One lane per node in the solver's numbering, one tile per workgroup; the
// node's coordinates and the running (best, near) stay in registers.  The wall nodes' coordinates pass through LDS in
// chunks of kWallChunk, one field per array: every lane of a wave reads the same address, which the LDS serves as a
// broadcast, at full rate for 8- and 16-byte reads (the walk is unrolled by four so that the loads of a field pair up).
// r2 = (dx dx + dy dy) + dz dz, one IEEE operation each; the strict < over ascending list positions, within and across
// chunks, gives a tie to the lowest wall id.  Slots behind the list's end hold NaN: a NaN r2 is never taken, so the walk
// runs to a multiple of four without a bound per point.  Never contracted to FMA.
// ------------------------------------------------------------------------------------------
constexpr int kWallChunk = 256;
static_assert(kWallChunk == kBlock, "k_wall_distance: every thread stages one wall node of a chunk");

__global__ void __launch_bounds__(kBlock)
k_wall_distance(uint32_t n_tiles, int64_t stride, int64_t nel, WallDistance a)
{
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double sx[kWallChunk], sy[kWallChunk], sz[kWallChunk];
    const unsigned t = xcd_contiguous_block(blockIdx.x, n_tiles);
    const int tid = threadIdx.x;
    const int64_t i = int64_t(t) * kBlock + tid;                  // < stride = 256 * n_tiles
    const double x = a.x[i], y = a.x[stride + i], z = a.x[2 * stride + i];
    double best = __builtin_inf();
    int32_t near = -1;
    for (int32_t c0 = 0; c0 < a.m; c0 += kWallChunk) {
        const int32_t j = c0 + tid;
        const bool in = j < a.m;
        const double wx = in ? a.wx[j] : __builtin_nan(""), wy = in ? a.wx[int64_t(a.m) + j] : __builtin_nan(""),
                     wz = in ? a.wx[2 * int64_t(a.m) + j] : __builtin_nan("");
        __syncthreads();                                          // (the chunk before has been walked by every wave)
        sx[tid] = wx; sy[tid] = wy; sz[tid] = wz;
        __syncthreads();
        const int32_t left = a.m - c0;
        const int32_t n4 = ((left < kWallChunk ? left : kWallChunk) + 3) & ~3;
        for (int32_t k = 0; k < n4; k += 4) {
            double r2[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const double dx = x - sx[k + u], dy = y - sy[k + u], dz = z - sz[k + u];
                r2[u] = (dx * dx + dy * dy) + dz * dz;
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (r2[u] < best) { best = r2[u]; near = c0 + k + u; }
        }
    }
    const bool present = i < nel;
    a.d[i] = present ? sqrt(best) : __builtin_inf();
    a.nearest[i] = present ? near : -1;
}

// The wall spacing: for wall node k the smallest d_n > 0.0 over the other ends n of its internal incidences in row order,
// +0.0 where there is none.
__global__ void __launch_bounds__(kBlock)
k_wall_spacing(WallSpacing a)
{
    const int64_t k = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (k >= a.wn.n) return;
    const int32_t e0 = a.wn.int_ptr[k], e1 = a.wn.int_ptr[k + 1];
    double h = 0.0;
    bool found = false;
    for (int32_t e = e0; e < e1; e++) {
        const double dn = a.d[a.wn.int_nbr[e]];
        if (dn > 0.0 && (!found || dn < h)) { h = dn; found = true; }
    }
    a.h[k] = h;
}

// The wall-limited length scale of the Smagorinsky model: l2_i = min(c2 d2_i, (kappa d_i)^2), the whole padded length (a pad
// lane's d is +inf: c2 * 1.0).
__global__ void __launch_bounds__(kBlock)
k_wall_length(int64_t stride, WallLength a)
{
#pragma clang fp contract(off)
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (i >= stride) return;
    const double c = a.c2 * a.d2[i];
    const double kd = a.kappa * a.d[i];
    const double w2 = kd * kd;
    a.l2[i] = w2 < c ? w2 : c;
}

// k_surface_loads with the friction six beside the pressure six: one lane per solid-wall edge, twelve terms, the trees
// of k_surface_loads over twelve columns (24 KB of LDS), the same ticket and stage B.  The pressure terms are
// k_surface_loads' expressions; task.sw == nullptr (a level the viscous terms are not on for) leaves the friction +0.0.
// NC = 12, or 14 with the heat loads' two columns behind them (mgcfd_surface_loads_heat): h = -(q . w) from the node's heat flux
// in Sw and the face area s = |w|, the same trees over fourteen columns (28 KB of LDS).  task.sw == nullptr leaves h +0.0 too.
template <int NC>
__global__ void __launch_bounds__(kBlock)
k_surface_loads_viscous(int64_t stride, const double *__restrict__ q, LoadsTaskViscous task)
{
#pragma clang fp contract(off)
    static_assert(NC == 12 || NC == 14, "twelve columns, or fourteen with the heat loads");
    __shared__ double sh[NC][kBlock];
    __shared__ int last;
    const LoadsTask &base = task.base;
    const int t = threadIdx.x;
    const int64_t e = int64_t(blockIdx.x) * kBlock + t;
    double v[NC] = {};
    if (e < base.n) {
        const WallRecord r = base.rec[e];
        const int64_t b = r.node;
        const double rho = q[b], mx = q[stride + b], my = q[2 * stride + b], mz = q[3 * stride + b], en = q[4 * stride + b];
        const double vx = mx / rho, vy = my / rho, vz = mz / rho;
        const double speed_sqd = vx * vx + vy * vy + vz * vz;
        const double p = (kGamma - 1.0) * (en - 0.5 * rho * speed_sqd);
        const double dp = p - base.p_inf;
        const double fx = dp * r.x, fy = dp * r.y, fz = dp * r.z;
        const double rx = r.cx - base.ref[0], ry = r.cy - base.ref[1], rz = r.cz - base.ref[2];
        v[0] = fx; v[1] = fy; v[2] = fz;
        v[3] = ry * fz - rz * fy;
        v[4] = rz * fx - rx * fz;
        v[5] = rx * fy - ry * fx;
        if (task.sw) {
            const double *s = task.sw + task.wall_of_rec[e];
            const double txx = s[3 * task.nw], tyy = s[4 * task.nw], tzz = s[5 * task.nw];
            const double txy = s[6 * task.nw], txz = s[7 * task.nw], tyz = s[8 * task.nw];
            const double gx = -((txx * r.x + txy * r.y) + txz * r.z);
            const double gy = -((txy * r.x + tyy * r.y) + tyz * r.z);
            const double gz = -((txz * r.x + tyz * r.y) + tzz * r.z);
            v[6] = gx; v[7] = gy; v[8] = gz;
            v[9] = ry * gz - rz * gy;
            v[10] = rz * gx - rx * gz;
            v[11] = rx * gy - ry * gx;
            if constexpr (NC == 14) {
                const double qx = s[9 * task.nw], qy = s[10 * task.nw], qz = s[11 * task.nw];
                v[12] = -((qx * r.x + qy * r.y) + qz * r.z);
            }
        }
        if constexpr (NC == 14) v[13] = sqrt((r.x * r.x + r.y * r.y) + r.z * r.z);
    }
    loads_tree(v, sh);                                                 // stage A
    const int nb = int(gridDim.x);
    if (nb == 1) {
        if (t == 0) loads_store(base, v);
        return;
    }
    if (t == 0) {
#pragma unroll
        for (int c = 0; c < NC; c++) base.partial[int64_t(c) * nb + blockIdx.x] = v[c];
        const unsigned done = __hip_atomic_fetch_add(base.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last = done == unsigned(nb - 1);
        if (last) __hip_atomic_store(base.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (the next call starts from zero)
    }
    __syncthreads();
    if (!last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    for (int n = nb; n > 1;) {                                          // stage B, as in k_surface_loads
        const int m = (n + kBlock - 1) / kBlock;
        for (int k = 0; k < m; k++) {
            const int i = k * kBlock + t;
#pragma unroll
            for (int c = 0; c < NC; c++) v[c] = i < n ? base.partial[int64_t(c) * nb + i] : 0.0;
            loads_tree(v, sh);
            if (t == 0) {
#pragma unroll
                for (int c = 0; c < NC; c++) base.partial[int64_t(c) * nb + k] = v[c];
            }
            __syncthreads();
        }
        n = m;
    }
    if (t == 0) loads_store(base, v);
}

// The surface distribution: one lane per wall node over its solid-wall edges in record order.  a = the sum of their
// weights from +0.0, dp = p - p_inf by k_surface_loads' expressions, t = -(tau . a) associated as the edge terms are.
__global__ void __launch_bounds__(kBlock)
k_wall_distribution(int64_t stride, const double *__restrict__ q, WallDistribution a)
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
    double tx = 0.0, ty = 0.0, tz = 0.0;
    if (a.sw) {
        const double *s = a.sw + k;
        const double txx = s[3 * a.wn.n], tyy = s[4 * a.wn.n], tzz = s[5 * a.wn.n];
        const double txy = s[6 * a.wn.n], txz = s[7 * a.wn.n], tyz = s[8 * a.wn.n];
        tx = -((txx * ax + txy * ay) + txz * az);
        ty = -((txy * ax + tyy * ay) + tyz * az);
        tz = -((txz * ax + tyz * ay) + tzz * az);
    }
    double *o = a.out + 7 * k;
    o[0] = ax; o[1] = ay; o[2] = az; o[3] = p - a.p_inf; o[4] = tx; o[5] = ty; o[6] = tz;
}

// The practical ceiling of the flux launch's data movement (bench.py: roofline.practical_ceiling_us): a tile-shaped STREAM of
// exactly the algorithmic bytes — workgroup t reads its share of `rd_total` doubles (contiguous, 16 bytes per lane and load,
// eight loads in flight) and writes its share of `wr_total` (write-through, as the flux launch stores) — with the order-free
// kernel's LDS footprint (four workgroups per CU), nothing dependent, nothing computed.  What the chip gives 1,175 workgroups
// that only move the bytes SURVEY.md §8d prices, launch included.
__global__ void __launch_bounds__(kBlock)
k_stream_tiles(const double2 *__restrict__ src, double *__restrict__ dst, int64_t rd_total2, int64_t wr_total, int rd2_per_thread, int wr_per_thread)
{
    __shared__ double lds[40960 / 8 - 64];
    const int64_t r0 = int64_t(blockIdx.x) * rd2_per_thread * kBlock + threadIdx.x;
    double acc = 0.0;
    for (int k = 0; k < rd2_per_thread; k += 8) {
        double2 v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int64_t j = r0 + int64_t(k + u) * kBlock;
            v[u] = src[(k + u < rd2_per_thread && j < rd_total2) ? j : int64_t(threadIdx.x)];
        }
#pragma unroll
        for (int u = 0; u < 8; u++) acc += v[u].x + v[u].y;
    }
    if (acc == 1.2345e300) { lds[threadIdx.x] = acc; __syncthreads(); acc = lds[(threadIdx.x + 1) & 255]; }   // (keeps the footprint)
    const int64_t w0 = int64_t(blockIdx.x) * wr_per_thread * kBlock + threadIdx.x;
    for (int k = 0; k < wr_per_thread; k++) {
        const int64_t j = w0 + int64_t(k) * kBlock;
        if (j < wr_total) MGCFD_ST_FLUX(dst + j, acc + double(k));
    }
}

// ==========================================================================================
// launchers
// ==========================================================================================
void launch_init_variables(hipStream_t st, int64_t stride, const FarField &ff, double *q)
{ hipLaunchKernelGGL(k_init_variables, dim3(grid_for(stride)), dim3(kBlock), 0, st, stride, ff, q); }

void launch_min_reduce(hipStream_t st, int64_t nel, const double *partial_min, double *out)
{ hipLaunchKernelGGL(k_min_reduce, dim3(1), dim3(kBlock), 0, st, partial_min, int(grid_for(nel)), out); }

void launch_stream_tiles(hipStream_t st, int n_tiles, const double *src, double *dst, int64_t rd_total, int64_t wr_total)
{
    const int64_t rd2 = rd_total / 2;
    const int rd2_per_thread = int((rd2 + int64_t(n_tiles) * kBlock - 1) / (int64_t(n_tiles) * kBlock));
    const int wr_per_thread = int((wr_total + int64_t(n_tiles) * kBlock - 1) / (int64_t(n_tiles) * kBlock));
    hipLaunchKernelGGL(k_stream_tiles, dim3(n_tiles), dim3(kBlock), 0, st, reinterpret_cast<const double2 *>(src), dst, rd2, wr_total, rd2_per_thread, wr_per_thread);
}

void launch_dual_clamp(hipStream_t st, int64_t nel, double cdt, const double *volumes, double *sf)
{ hipLaunchKernelGGL(k_dual_clamp, dim3(grid_for(nel)), dim3(kBlock), 0, st, nel, cdt, volumes, sf); }

void launch_dual_shift(hipStream_t st, int64_t n, const double *q, double *wn, double *wn1, int first)
{ hipLaunchKernelGGL(k_dual_shift, dim3(grid_for(n)), dim3(kBlock), 0, st, n, q, wn, wn1, first); }

void launch_viscous_clamp(hipStream_t st, int64_t nel, double k0, const double *rho, const double *g, double *sf)
{ hipLaunchKernelGGL(k_viscous_clamp, dim3(grid_for(nel)), dim3(kBlock), 0, st, nel, k0, rho, g, sf); }
void launch_viscous_clamp_variable(hipStream_t st, int64_t nel, int64_t stride, const ViscousClamp &a)
{ hipLaunchKernelGGL(k_viscous_clamp_variable, dim3(grid_for(nel)), dim3(kBlock), 0, st, nel, stride, a); }
void launch_viscous_wall(hipStream_t st, int64_t n, int64_t stride, const int32_t *nodes, double *q, double *q2,
                         const double *old_variables, double *residuals)
{ if (n > 0) hipLaunchKernelGGL(k_viscous_wall, dim3(grid_for(n)), dim3(kBlock), 0, st, n, stride, nodes, q, q2, old_variables, residuals); }

void launch_check_invalid(hipStream_t st, int64_t nel, int64_t stride, const double *q, const int32_t *old_of_new,
                          unsigned long long *err)
{ hipLaunchKernelGGL(k_check_invalid, dim3(grid_for(nel)), dim3(kBlock), 0, st, nel, stride, q, old_of_new, err); }

void launch_halo_pack(hipStream_t st, int64_t n, int64_t stride, const int32_t *idx, const double *field, double *msg)
{ if (n > 0) hipLaunchKernelGGL(k_halo_pack, dim3(grid_for(n)), dim3(kBlock), 0, st, n, stride, idx, field, msg); }

void launch_halo_push(hipStream_t st, int64_t n, int64_t stride, const int32_t *idx, const int32_t *target, const double *field, const PushPeers &peers)
{ if (n > 0) hipLaunchKernelGGL(k_halo_push, dim3(grid_for(n)), dim3(kBlock), 0, st, n, stride, idx, target, field, peers); }

void launch_halo_push_flags(hipStream_t st, int64_t n, int64_t stride, const int32_t *idx, const int32_t *target, const double *field,
                            const PushPeers &peers, const PushFlags &flags, unsigned *ticket)
{ if (n > 0) hipLaunchKernelGGL(k_halo_push_flags, dim3(grid_for(n)), dim3(kBlock), 0, st, n, stride, idx, target, field, peers, flags, ticket); }

void launch_flags_wait(hipStream_t st, const unsigned long long *flags, const FlagRows &rows, int slot, unsigned long long value, int *timed_out)
{ if (rows.n > 0) hipLaunchKernelGGL(k_flags_wait, dim3(1), dim3(64), 0, st, flags, rows, slot, value, timed_out); }

void launch_min_publish(hipStream_t st, const double *my_min, const MinPublish &mp)
{ hipLaunchKernelGGL(k_min_publish, dim3(1), dim3(64), 0, st, my_min, mp); }

void launch_halo_unpack(hipStream_t st, int64_t n, int64_t stride, const int32_t *idx, const double *msg, double *field)
{ if (n > 0) hipLaunchKernelGGL(k_halo_unpack, dim3(grid_for(n)), dim3(kBlock), 0, st, n, stride, idx, msg, field); }

void launch_accept_restricted(hipStream_t st, int64_t nel_coarse, int64_t stride_coarse, const int32_t *child_ptr, const double *src, double *coarse_q)
{ hipLaunchKernelGGL(k_accept_restricted, dim3(grid_for(nel_coarse)), dim3(kBlock), 0, st, nel_coarse, stride_coarse, child_ptr, src, coarse_q); }

void launch_min_over_peers(hipStream_t st, const double *const *scalars, int n, double *out)
{ hipLaunchKernelGGL(k_min_over_peers, dim3(1), dim3(64), 0, st, scalars, n, out); }

void launch_sum_partials_append(hipStream_t st, int n, const double *partial, double *out, double *ring, int *count, int cap)
{ hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(kBlock), 0, st, SumTask{partial, n, out, ring, count, cap}); }

// partial must hold grid_for(nel) doubles
void launch_sumsq_original(hipStream_t st, int64_t nel, int64_t stride, const double *x, const int32_t *new_of_old, double *partial)
{ hipLaunchKernelGGL(k_sumsq_original, dim3(grid_for(nel)), dim3(kBlock), 0, st, nel, stride, x, new_of_old, partial); }

void launch_append_scalar(hipStream_t st, const double *src, double *ring, int *count, int cap)
{ hipLaunchKernelGGL(k_append_scalar, dim3(1), dim3(64), 0, st, src, ring, count, cap); }

void launch_surface_loads(hipStream_t st, int64_t stride, const double *q, const LoadsTask &task)
{
    if (task.n <= 0) return;                                           // (the caller writes the zeros)
    hipLaunchKernelGGL(k_surface_loads, dim3(unsigned((task.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, stride, q, task);
}

void launch_wall_stress(hipStream_t st, int64_t stride, const double *q, const WallStress &a)
{ if (a.wn.n > 0) hipLaunchKernelGGL(k_wall_stress, dim3(grid_for(a.wn.n)), dim3(kBlock), 0, st, stride, q, a); }
// (the grid is the level's tiles: stride = 256 * n_tiles)
void launch_wall_distance(hipStream_t st, int64_t nel, int64_t stride, const WallDistance &a)
{ hipLaunchKernelGGL(k_wall_distance, dim3(unsigned(stride / kBlock)), dim3(kBlock), 0, st, uint32_t(stride / kBlock), stride, nel, a); }
void launch_wall_spacing(hipStream_t st, const WallSpacing &a)
{ if (a.wn.n > 0) hipLaunchKernelGGL(k_wall_spacing, dim3(grid_for(a.wn.n)), dim3(kBlock), 0, st, a); }
void launch_wall_length(hipStream_t st, int64_t stride, const WallLength &a)
{ hipLaunchKernelGGL(k_wall_length, dim3(grid_for(stride)), dim3(kBlock), 0, st, stride, a); }

// columns: 12, or 14 with the heat loads' two columns behind them (task.base.partial [14][..], rows of 14)
void launch_surface_loads_viscous(hipStream_t st, int64_t stride, const double *q, const LoadsTaskViscous &task, int columns)
{
    if (task.base.n <= 0) return;
    const dim3 grid(unsigned((task.base.n + kBlock - 1) / kBlock));
    if (columns == 14) hipLaunchKernelGGL(k_surface_loads_viscous<14>, grid, dim3(kBlock), 0, st, stride, q, task);
    else hipLaunchKernelGGL(k_surface_loads_viscous<12>, grid, dim3(kBlock), 0, st, stride, q, task);
}

void launch_wall_distribution(hipStream_t st, int64_t stride, const double *q, const WallDistribution &a)
{ if (a.wn.n > 0) hipLaunchKernelGGL(k_wall_distribution, dim3(grid_for(a.wn.n)), dim3(kBlock), 0, st, stride, q, a); }

void launch_loads_terms(hipStream_t st, int64_t stride, const double *q, const LoadsTerms &task)
{
    if (task.n <= 0) return;                                           // (a rank without a solid-wall edge stores nothing)
    hipLaunchKernelGGL(k_loads_terms, dim3(grid_for(task.n)), dim3(kBlock), 0, st, stride, q, task);
}

void launch_loads_scatter(hipStream_t st, int64_t n, const double *src, int64_t src_row, const int32_t *slot, double *table, int64_t row)
{ if (n > 0) hipLaunchKernelGGL(k_loads_scatter, dim3(grid_for(n)), dim3(kBlock), 0, st, n, src, src_row, slot, table, row); }

// `row` is a multiple of 256 and the table holds 6 rows of it: one workgroup per 256 lanes
void launch_loads_reduce(hipStream_t st, const double *table, int64_t row, const LoadsTask &task)
{
    if (task.n <= 0) return;                                           // (the caller writes the zeros)
    hipLaunchKernelGGL(k_loads_reduce, dim3(unsigned(row / kBlock)), dim3(kBlock), 0, st, table, row, task);
}

void launch_fas_forcing(hipStream_t st, int64_t nel_coarse, int64_t stride_coarse, const int32_t *child_ptr, const double *fluxes,
                        double *forcing)
{ hipLaunchKernelGGL(k_fas_forcing, dim3(grid_for(nel_coarse)), dim3(kBlock), 0, st, nel_coarse, stride_coarse, child_ptr, fluxes, forcing); }

void launch_fas_add_forcing(hipStream_t st, int64_t stride, double *fluxes, const double *forcing)
{ hipLaunchKernelGGL(k_fas_add_forcing, dim3(grid_for(stride * 5)), dim3(kBlock), 0, st, stride * 5, fluxes, forcing); }

} // namespace mgcfd
