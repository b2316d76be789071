// kernel_device.hpp — what the kernel translation units share: kernels.hip (compiled once per numeric flavour) and
// kernels_plain.hip (compiled once, never contracted).  Everything that does arithmetic here has internal linkage (the
// anonymous namespace below), so each translation unit gets the copy compiled under its own -ffp-contract flag.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_plan.hpp"

// Cache policy of the standalone flux launch's stores: write-through (`sc1`: the line leaves the XCD's L2 at once and is not
// kept).  Nothing in the launch reads `fluxes`, an XCD's L2 keeps nothing across a kernel boundary (profiles/r4_l2_across_launches.txt)
// and a launch otherwise ends with the write-back of everything it left dirty: 14.7 -> 14.1 us order-free, 16.1 -> 15.8 us
// bit-identical (profiles/r4_flux_levers.txt).  Experiment switches (tools/exp_flags.py builds libraries with -DMGCFD_EXP_*;
// the shipped build defines none of them; an experiment library rebuilds kernels.hip alone, so the two switches below reach
// its kernels and not kernels_plain.hip's).
#if defined(MGCFD_EXP_FLUX_ST_NT)
#define MGCFD_ST_FLUX(p, v) __builtin_nontemporal_store((v), (p))
#elif defined(MGCFD_EXP_FLUX_ST_PLAIN)
#define MGCFD_ST_FLUX(p, v) (*(p) = (v))
#else
#define MGCFD_ST_FLUX(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#endif
// ... and of every store of a node's new state (the fused stages, time_step, the transfers): write-through as well
// (sweep 55.0 -> 54.4 us, V-cycle 0.293 -> 0.287 ms; non-temporal stores: 57.1 us / 0.295 ms, profiles/r4_flux_levers.txt)
#if defined(MGCFD_EXP_STAGE_ST_PLAIN)
#define MGCFD_ST_STAGE(p, v) (*(p) = (v))
#elif defined(MGCFD_EXP_STAGE_ST_NT)
#define MGCFD_ST_STAGE(p, v) __builtin_nontemporal_store((v), (p))
#else
#define MGCFD_ST_STAGE(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#endif

namespace mgcfd {
namespace {

constexpr double kGamma = 1.4;                // src/Base/const.h:9
constexpr int kBlock = 256;
// doubles per LDS field of the node-gather tile kernels (k_smooth_tile and every kernel on its walk): one field per array
constexpr int kSmoothRow = 560;
static_assert(kSmoothRow >= kTileCap, "every staged slot has a place");

// ---- per-node derived state -------------------------------------------------------------
// cfd_loops.h:121-148.  Same expressions, same association as the reference.
struct Derived { double vx, vy, vz, p, speed, c, speed_sqd; };

__device__ __forceinline__ Derived derive(double rho, double mx, double my, double mz, double en)
{
    Derived d;
    d.vx = mx / rho;
    d.vy = my / rho;
    d.vz = mz / rho;
    d.speed_sqd = d.vx * d.vx + d.vy * d.vy + d.vz * d.vz;
    d.p = (kGamma - 1.0) * (en - 0.5 * rho * d.speed_sqd);
    d.speed = sqrt(d.speed_sqd);
    d.c = sqrt(kGamma * d.p / rho);
    return d;
}

// What the flux needs of one node: the 5 conserved variables plus what the reference derives
// from them for every incident edge.
struct NodeQ { double rho, mx, my, mz, en, vx, vy, vz, p, speed, c; };

__device__ __forceinline__ NodeQ make_nodeq(double rho, double mx, double my, double mz, double en)
{
    const Derived d = derive(rho, mx, my, mz, en);
    NodeQ r;
    r.rho = rho; r.mx = mx; r.my = my; r.mz = mz; r.en = en;
    r.vx = d.vx; r.vy = d.vy; r.vz = d.vz; r.p = d.p; r.speed = d.speed; r.c = d.c;
    return r;
}

__device__ __forceinline__ NodeQ load_and_derive(const double *__restrict__ q, int64_t stride, int64_t i)
{
    return make_nodeq(q[i], q[stride + i], q[2 * stride + i], q[3 * stride + i], q[4 * stride + i]);
}

__device__ __forceinline__ void store_conserved(double *__restrict__ q, int64_t stride, int64_t i, double rho,
                                                double mx, double my, double mz, double en)
{
    MGCFD_ST_STAGE(q + i, rho);
    MGCFD_ST_STAGE(q + stride + i, mx);
    MGCFD_ST_STAGE(q + 2 * stride + i, my);
    MGCFD_ST_STAGE(q + 3 * stride + i, mz);
    MGCFD_ST_STAGE(q + 4 * stride + i, en);
}

// Minimum over the 64 lanes of a wave, in every lane; call it with all 64 lanes active (a disabled lane would
// be read as 0 by the DPP moves).  Cross-lane moves by DPP inside each row of 16
// lanes (no trip through the LDS crossbar as __shfl_xor takes, which would also queue behind the
// record stores of the tile kernels), then the four row minima are read as scalars.
template <int ctrl>
__device__ __forceinline__ double dpp_move(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_mov_dpp(static_cast<int>(b), ctrl, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp(static_cast<int>(b >> 32), ctrl, 0xF, 0xF, true);
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo));
}

__device__ __forceinline__ double read_lane(double v, int lane)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane(static_cast<int>(b), lane);
    const int hi = __builtin_amdgcn_readlane(static_cast<int>(b >> 32), lane);
    return __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<unsigned>(lo));
}

__device__ __forceinline__ double wave_min(double v)
{
    v = fmin(v, dpp_move<0xB1>(v));      // quad_perm [1,0,3,2]: lane ^ 1
    v = fmin(v, dpp_move<0x4E>(v));      // quad_perm [2,3,0,1]: lane ^ 2  -> quads uniform
    v = fmin(v, dpp_move<0x141>(v));     // row_half_mirror: i <-> 7-i     -> groups of 8 uniform
    v = fmin(v, dpp_move<0x140>(v));     // row_mirror: i <-> 15-i         -> rows of 16 uniform
    return fmin(fmin(read_lane(v, 0), read_lane(v, 16)), fmin(read_lane(v, 32), read_lane(v, 48)));
}

__device__ __forceinline__ double wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// check_for_invalid_variables (validation.cpp:107-138) runs after every time_step and stops at the first bad cell
// in original order.  Here a bad cell leaves (launch sequence number, original id, code) in one word and the
// smallest wins: the earliest checked launch since the host last looked, then the smallest original id.
// `check` = that sequence number (>= 1, < 2^23; 0 switches the check off).
__device__ __forceinline__ unsigned long long err_key(int check, int32_t original_id, int code)
{
    return (static_cast<unsigned long long>(check) << 40) | (static_cast<unsigned long long>(uint32_t(original_id)) << 8) | unsigned(code);
}

// XCD-aware block order: hardware deals consecutive workgroups round-robin over the 8 XCDs
// (each with a private L2).  Give every XCD one CONTIGUOUS range of tiles instead, so that a
// tile's halo — owned by neighbouring tiles — is usually already in the same L2.  Pure speed:
// any placement is correct.
__device__ __forceinline__ unsigned xcd_contiguous_block(unsigned b, unsigned nb)
{
    const unsigned q = nb >> 3, r = nb & 7u, x = b & 7u, k = b >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + k;
}

// minimum of the partial minima, by every thread of a workgroup (result in all lanes)
__device__ __forceinline__ double block_min_of_partials(const double *__restrict__ partial_min, int n_partial)
{
    __shared__ double s_red[kBlock / 64];
    double m = __longlong_as_double(0x7FF0000000000000LL);
    for (int k = threadIdx.x; k < n_partial; k += kBlock) m = fmin(m, partial_min[k]);
    m = wave_min(m);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    double r = s_red[0];
    for (int w = 1; w < kBlock / 64; w++) r = fmin(r, s_red[w]);
    return r;
}

// One workgroup's minimum of v -> out[blockIdx.x]; every thread of the workgroup must call it.
__device__ __forceinline__ void block_min_to(double v, double *__restrict__ out)
{
    __shared__ double s_m[kBlock / 64];
    v = wave_min(v);
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = s_m[0];
        for (int w = 1; w < kBlock / 64; w++) m = fmin(m, s_m[w]);
        out[blockIdx.x] = m;
    }
}

// The primitive variables the viscous terms difference: velocity and T = p / rho (k_viscous_stress_tile, k_wall_stress).
struct Primitive { double u, v, w, T; };

__device__ __forceinline__ Primitive primitive_of(const double *__restrict__ q, int64_t stride, int64_t n)
{
    const double rho = q[n];
    const Derived d = derive(rho, q[stride + n], q[2 * stride + n], q[3 * stride + n], q[4 * stride + n]);
    Primitive r;
    r.u = d.vx; r.v = d.vy; r.w = d.vz; r.T = d.p / rho;
    return r;
}

// The viscosity model (mgcfd_set_viscosity_model; INTEGRATION.md "Variable viscosity"): a node's viscosity by the law and its
// eddy viscosity under Smagorinsky, one IEEE operation each in the definition's order; the stress launch, the wall-stress
// launch and the variable step limit share them.
__device__ __forceinline__ double viscosity_of(const ViscosityModel &m, double mu, double T)
{
    if (m.law == 0) return mu;
    const double r = T / m.t_ref;
    return ((mu * (r * sqrt(r))) * m.one_plus_s) / (r + m.s);
}
// (d2: the node's entry of m.d2 — d2_i, or under wall damping l2_i as k_wall_length left it, which stands for c2 * d2_i)
__device__ __forceinline__ double smagorinsky_of(const ViscosityModel &m, double d2, double rho, double gux, double guy, double guz,
                                                 double gvx, double gvy, double gvz, double gwx, double gwy, double gwz)
{
    const double sxy = 0.5 * (guy + gvx), sxz = 0.5 * (guz + gwx), syz = 0.5 * (gvz + gwy);
    const double ss = ((gux * gux + gvy * gvy) + gwz * gwz) + 2.0 * ((sxy * sxy + sxz * sxz) + syz * syz);
    const double l2 = m.damped ? d2 : m.c2 * d2;
    return (l2 * rho) * sqrt(2.0 * ss);
}

// One workgroup adds up n partial sums (always in this order) and may append the total to the rms history.
__device__ __forceinline__ void block_sum_partials(const SumTask &task)
{
    __shared__ double s[kBlock / 64];
    double acc = 0.0;
    for (int k = threadIdx.x; k < task.n; k += kBlock) acc += task.partial[k];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < kBlock / 64; w++) t += s[w];
        task.out[0] = t;
        if (task.ring) {
            const int c = *task.count;
            if (c < task.cap) task.ring[c] = t;
            *task.count = c + 1;
        }
    }
}

// workgroups of kBlock lanes for n items (host)
static inline unsigned grid_for(int64_t n) { return static_cast<unsigned>((n + kBlock - 1) / kBlock); }

} // namespace

// block_sum_partials as a launch of its own.  Defined once, in kernels_plain.hip, and launched by both flavours of
// launch_sumsq as well: it only adds, so there is nothing for -ffp-contract to contract and one copy serves all three.
__global__ void __launch_bounds__(kBlock) k_sum_partials(SumTask task);

} // namespace mgcfd

