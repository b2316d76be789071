// kernels.hip — hand-written HIP kernels for gfx950 (MI355X) for the MG-CFD hot path: the kernels of the launchers that
// exist in two numeric flavours (kernels.hpp: MGCFD_FLAVOURED_LAUNCHERS, and launch_diag_fast_math).  Every other kernel
// is in kernels_plain.hip; what the two files share is in kernel_device.hpp.
//
// Compiled TWICE into two namespaces:
//   -DMGCFD_KERNEL_NS=exact -ffp-contract=off   every fp64 op rounds as in the reference built
//                                               with -ffp-contract=off; together with the
//                                               reference-order gathers this is bit-identical
//   -DMGCFD_KERNEL_NS=fast  -ffp-contract=fast  same code, FMA contraction allowed
//
// Design: there is no dense contraction here, so no MFMA; every loop is a
// node-centred sweep with one lane per node, over structure-of-arrays state
// (field f of node i at q[f*stride + i]) so that per-node accesses coalesce perfectly.
//   * flux_tile     replaces the reference's edge loop + scatter-add
//                   (src/Kernels/flux_loops.cpp:133-136, flux_kernel.elemfunc.c) by a per-node
//                   GATHER: a 256-thread workgroup owns a compact cluster of 256 nodes, stages
//                   their state and their halo's state into an LDS tile (each node fetched once
//                   per tile instead of once per incident edge), and every lane then walks its
//                   incidence rows (sliced ELLPACK, 26-34 B per entry, coalesced) and sums the
//                   edge fluxes in the reference's order — no atomics, no colouring,
//                   deterministic, bit-identical.
//   * The division / square-root work (8 div + 5 sqrt per edge in the reference) is done once
//     per STAGED node while the tile is filled (3 div + 2 sqrt); values are identical because
//     the reference recomputes the very same per-node expressions for every incident edge.
#include <algorithm>
#include <cstdlib>
#include <stdexcept>
#include <type_traits>

#include "kernel_device.hpp"

#ifndef MGCFD_KERNEL_NS
#error "compile with -DMGCFD_KERNEL_NS=exact|fast"
#endif

namespace mgcfd {
namespace MGCFD_KERNEL_NS {

// Diagnostic build only (-DMGCFD_PHASES): thread 0 of every workgroup adds the wall-clock ticks between the phase
// boundaries (PH_MARK) of the flux kernel it runs to its own slot.  The shipped build defines the marks away.
#ifdef MGCFD_PHASES
__device__ unsigned long long g_phase[4096 * 8];
__device__ unsigned long long g_phase_abs[4096 * 8];     // the LAST launch: [0] when every workgroup began, [1 + k] when it passed mark k (100 MHz ticks), [7] XCC_ID << 32 | HW_ID
#define PH_MARK(k) do { if (threadIdx.x == 0) { unsigned long long now_ = wall_clock64(); g_phase[(blockIdx.x & 4095) * 8 + (k)] += now_ - ph_last_; ph_last_ = now_; g_phase_abs[(blockIdx.x & 4095) * 8 + 1 + (k)] = now_; } } while (0)
#define PH_BEGIN() unsigned long long ph_last_ = wall_clock64(); if (threadIdx.x == 0) { g_phase[(blockIdx.x & 4095) * 8 + 7] += 1ull; g_phase_abs[(blockIdx.x & 4095) * 8] = ph_last_; \
        g_phase_abs[(blockIdx.x & 4095) * 8 + 7] = (static_cast<unsigned long long>(__builtin_amdgcn_s_getreg(20 | (0 << 6) | (31 << 11))) << 32) | __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11)); }
#else
#define PH_MARK(k) do { } while (0)
#define PH_BEGIN() do { } while (0)
#endif

// (the cache policy of the stores, MGCFD_ST_FLUX and MGCFD_ST_STAGE: kernel_device.hpp; of the flux kernels' state loads:)
#if defined(MGCFD_EXP_STATE_LD_NT)
#define MGCFD_LD_STATE(p) __builtin_nontemporal_load(p)
#else
#define MGCFD_LD_STATE(p) (*(p))
#endif

namespace {

// LDS tile records: 12 doubles (96 B) per staged node, read back with 16-byte LDS loads.
constexpr int kLdsRecD2 = 6;               // double2 per record

// Within a record the three pairs of 16-byte quads are swapped when bit 3 of the slot is set: with a
// 24-dword record stride a fixed quad of slots s and s+8 would otherwise sit on the same 4 banks and
// a 16-lane ds_read_b128 group could reach only 8 of the 16 quad positions of the 256-B bank row
// (MI355X_MICROARCH.md, LDS); the swap makes all 16 reachable.
__device__ __forceinline__ void lds_store_record(double2 *tile, uint32_t slot, const NodeQ &n)
{
    double2 *rec = tile + slot * kLdsRecD2;
    const uint32_t b = (slot >> 3) & 1u;
    rec[0 ^ b] = make_double2(n.rho, n.mx);
    rec[1 ^ b] = make_double2(n.my, n.mz);
    rec[2 ^ b] = make_double2(n.en, n.vx);
    rec[3 ^ b] = make_double2(n.vy, n.vz);
    rec[4 ^ b] = make_double2(n.p, n.speed);
    rec[5 ^ b] = make_double2(n.c, 0.0);
}

__device__ __forceinline__ NodeQ lds_load_record(const double2 *tile, uint32_t slot)
{
    const uint32_t b = (slot >> 3) & 1u;
    const double2 *even = tile + slot * kLdsRecD2 + b;      // logical quads 0, 2, 4 (+0, +2, +4)
    const double2 *odd = tile + slot * kLdsRecD2 - b;       // logical quads 1, 3, 5 (+1, +3, +5)
    const double2 a = even[0], bq = odd[1], c = even[2], d = odd[3], e = even[4];
    const double f = odd[5].x;
    NodeQ r;
    r.rho = a.x; r.mx = a.y; r.my = bq.x; r.mz = bq.y; r.en = c.x; r.vx = c.y;
    r.vy = d.x; r.vz = d.y; r.p = e.x; r.speed = e.y; r.c = f;
    return r;
}

// The records of the four-workgroups-per-CU stages (FluxTileLds4): 10 doubles (80 B), the pressure left out and recomputed
// where a record is read, by derive's expression on the same stored doubles (the same bits under -ffp-contract=off).  The
// stride of 5 quads is odd, so 16 consecutive slots already cover all 16 quad positions of the 256-B bank row: no swizzle.
constexpr int kLdsRec80D2 = 5;

__device__ __forceinline__ void lds_put_record80(double2 *tile, uint32_t slot, const NodeQ &n)
{
    double2 *rec = tile + slot * kLdsRec80D2;
    rec[0] = make_double2(n.rho, n.mx);
    rec[1] = make_double2(n.my, n.mz);
    rec[2] = make_double2(n.en, n.vx);
    rec[3] = make_double2(n.vy, n.vz);
    rec[4] = make_double2(n.speed, n.c);
}

__device__ __forceinline__ NodeQ lds_get_record80(const double2 *tile, uint32_t slot)
{
    const double2 *rec = tile + slot * kLdsRec80D2;
    const double2 a = rec[0], b = rec[1], c = rec[2], d = rec[3], e = rec[4];
    NodeQ r;
    r.rho = a.x; r.mx = a.y; r.my = b.x; r.mz = b.y; r.en = c.x; r.vx = c.y;
    r.vy = d.x; r.vz = d.y; r.speed = e.x; r.c = e.y;
    r.p = (kGamma - 1.0) * (r.en - 0.5 * r.rho * (r.vx * r.vx + r.vy * r.vy + r.vz * r.vz));      // derive(), cfd_loops.h:121-148
    return r;
}

template <bool SLIM>
__device__ __forceinline__ void lds_put_rec(double2 *tile, uint32_t slot, const NodeQ &n)
{
    if (SLIM) lds_put_record80(tile, slot, n);
    else lds_store_record(tile, slot, n);
}

template <bool SLIM>
__device__ __forceinline__ NodeQ lds_get_rec(const double2 *tile, uint32_t slot)
{
    return SLIM ? lds_get_record80(tile, slot) : lds_load_record(tile, slot);
}

// The nine distinct flux-contribution components (cfd_loops.h:57-83); the momentum tensor is
// symmetric in storage: fmy.x = fmx.y, fmz.x = fmx.z, fmz.y = fmy.z.
struct FluxC { double xx, xy, xz, yy, yz, zz, ex, ey, ez; };

__device__ __forceinline__ FluxC flux_contribution(const NodeQ &q)
{
    FluxC f;
    f.xx = q.vx * q.mx + q.p;
    f.xy = q.vx * q.my;
    f.xz = q.vx * q.mz;
    f.yy = q.vy * q.my + q.p;
    f.yz = q.vy * q.mz;
    f.zz = q.vz * q.mz + q.p;
    const double de_p = q.en + q.p;
    f.ex = q.vx * de_p;
    f.ey = q.vy * de_p;
    f.ez = q.vz * de_p;
    return f;
}

} // namespace

// ------------------------------------------------------------------------------------------
// compute_step_factor, first half (cfd_loops.cpp:98-125): sf = cfl * (cbrt(vol) / (|v| + c)) and
// the minimum over the level (cfl: the reference's literal 0.5, an argument here — the same IEEE
// multiplication).  cbrt(vol) is static and precomputed on the host with the same libm the
// reference would call.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_step_factor_local(int64_t nel, int64_t stride, const double *__restrict__ q, const double *__restrict__ cbrt_vol,
                    double cfl, double *__restrict__ step_factors, double *__restrict__ partial_min,
                    double *__restrict__ old_variables /* nullptr, or: fused copy<double>(old, variables) */)
{
    __shared__ double s_min[kBlock / 64];
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    double sf = __longlong_as_double(0x7FF0000000000000LL);          // +inf
    if (i < nel) {
        const double rho = q[i], mx = q[stride + i], my = q[2 * stride + i], mz = q[3 * stride + i], en = q[4 * stride + i];
        if (old_variables) {
            old_variables[i] = rho; old_variables[stride + i] = mx; old_variables[2 * stride + i] = my;
            old_variables[3 * stride + i] = mz; old_variables[4 * stride + i] = en;
        }
        const Derived d = derive(rho, mx, my, mz, en);
        const double dt = cbrt_vol[i] / (d.speed + d.c);
        sf = cfl * dt;
        step_factors[i] = sf;
    }
    // One partial minimum per workgroup; the consumer reduces them (min is order independent,
    // and one atomic word would serialise ~1200 updates).
    sf = wave_min(sf);
    if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = sf;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = s_min[0];
        for (int w = 1; w < kBlock / 64; w++) m = fmin(m, s_min[w]);
        partial_min[blockIdx.x] = m;
    }
}

// first half of compute_step_factor for one node, as k_step_factor_local computes it
__device__ __forceinline__ double local_step_factor(double rho, double mx, double my, double mz, double en, double cbrt_vol, double cfl)
{
    const Derived d = derive(rho, mx, my, mz, en);
    const double dt = cbrt_vol / (d.speed + d.c);
    return cfl * dt;
}

// MGCFD_DT_LOCAL: a node's own step, sf = (cfl * dt) / vol with the dt of compute_step_factor (cfd_loops.cpp:116).
// A ghost of a partitioned level (cbrt_vol = +inf: its owner computes its step) gets 0: it holds no rows, so its sum of
// fluxes is zero and time_step leaves it where it is, which inf * 0 would not.
__device__ __forceinline__ double nodal_step_factor(const Derived &d, double cbrt_vol, double vol, double cfl)
{
    const double dt = cbrt_vol / (d.speed + d.c);
    return cbrt_vol < __longlong_as_double(0x7FF0000000000000LL) ? (cfl * dt) / vol : 0.0;
}

// second half (cfd_loops.cpp:146-156): step_factors[i] = min_dt / volumes[i]
__global__ void __launch_bounds__(kBlock)
k_step_factor_apply(int64_t nel, const double *__restrict__ min_dt_scalar,
                    const double *__restrict__ volumes, double *__restrict__ step_factors)
{
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (i >= nel) return;
    step_factors[i] = min_dt_scalar[0] / volumes[i];
}

// compute_step_factor_legacy (cfd_loops.cpp:37-61): what mesh_name = fvcorr runs, MGCFD_DT_LOCAL_LEGACY on any mesh
// (cfl: the reference's literal 0.5)
__global__ void __launch_bounds__(kBlock)
k_step_factor_legacy(int64_t nel, int64_t stride, const double *__restrict__ q, const double *__restrict__ volumes,
                     double cfl, double *__restrict__ step_factors, double *__restrict__ old_variables /* nullptr or fused copy */)
{
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (i >= nel) return;
    const double rho = q[i], mx = q[stride + i], my = q[2 * stride + i], mz = q[3 * stride + i], en = q[4 * stride + i];
    if (old_variables) {
        old_variables[i] = rho; old_variables[stride + i] = mx; old_variables[2 * stride + i] = my;
        old_variables[3 * stride + i] = mz; old_variables[4 * stride + i] = en;
    }
    const Derived d = derive(rho, mx, my, mz, en);
    step_factors[i] = cfl / (sqrt(volumes[i]) * (d.speed + d.c));
}

// MGCFD_DT_LOCAL: step_factors[i] = (cfl * cbrt(vol_i) / (|v_i| + c_i)) / vol_i, no minimum over the level
__global__ void __launch_bounds__(kBlock)
k_step_factor_nodal(int64_t nel, int64_t stride, const double *__restrict__ q, const double *__restrict__ cbrt_vol,
                    const double *__restrict__ volumes, double cfl, double *__restrict__ step_factors,
                    double *__restrict__ old_variables /* nullptr or fused copy */)
{
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (i >= nel) return;
    const double rho = q[i], mx = q[stride + i], my = q[2 * stride + i], mz = q[3 * stride + i], en = q[4 * stride + i];
    if (old_variables) {
        old_variables[i] = rho; old_variables[stride + i] = mx; old_variables[2 * stride + i] = my;
        old_variables[3 * stride + i] = mz; old_variables[4 * stride + i] = en;
    }
    const Derived d = derive(rho, mx, my, mz, en);
    step_factors[i] = nodal_step_factor(d, cbrt_vol[i], volumes[i], cfl);
}

// ------------------------------------------------------------------------------------------
// flux_tile: compute_flux_edge + compute_boundary_flux_edge + compute_wall_flux_edge
// (flux_loops.cpp:10-153) as one node-centred gather served from an LDS tile.
//
// One 256-thread workgroup = one tile = 256 consecutive nodes forming a compact cluster of
// the mesh graph (preprocess.cpp: cluster_order).  Phase 1: every staged node — the 256 own
// nodes (coalesced loads) and the tile's halo, the few hundred outside nodes its edges touch
// (gathered by id) — has its 5 conserved variables read from HBM ONCE, its velocity, pressure,
// |v| and speed of sound derived (cfd_loops.h:121-148) and the 11 values written to LDS as one
// 96-byte record.  Phase 2: every lane walks the incidence rows of its node (sliced ELLPACK:
// row r of a wave = the r-th incident edge of its 64 nodes, stored contiguously: a 16-bit
// tile-local neighbour slot, the 3 signed, halved edge-weight components and optionally the
// precomputed length factor = 26 or 34 B per entry),
// reads the neighbour's record from LDS and adds the edge flux.  Rows are in ORIGINAL edge
// order, internal edges first, then solid-wall faces, then far-field faces — exactly the order
// in which the reference's serial loops add into fluxes[node] — so the per-node sequential sum
// reproduces the reference's floating-point result bit for bit (exact build).
//
// `classes` selects the edge classes (bit0 internal, bit1 solid wall "-1", bit2 far field
// "-2"); ACC starts from the value already in `fluxes` (the reference's "+=" when the array is
// not known to be zero).  Halo nodes beyond the LDS capacity (ragged clusters
// only) are listed in a per-tile overflow table and read straight from HBM.
// ------------------------------------------------------------------------------------------
struct EdgeRow { uint32_t code; double fx, fy, fz, k; };

// Edge weights are stored [row][4 components][64 lanes]: fx, fy, fz (signed, halved) and
// k = -|e|*smoothing*0.5.  LOADK = false skips the k stream (8 of 34 bytes per entry) and
// recomputes it from fx,fy,fz — bit-identical either way, a bandwidth-for-arithmetic trade.
template <bool LOADK>
__device__ __forceinline__ EdgeRow load_row(const uint16_t *__restrict__ nbr, const double *__restrict__ w,
                                            int64_t row, int lane)
{
    EdgeRow e;
    const double *wr = w + (row << 8) + lane;
#ifdef MGCFD_EXP_ROW_LD_NT          // (experiment: the rows are read once — streamed past the L2 so that the state stays in it)
    e.code = __builtin_nontemporal_load(nbr + (row << 6) + lane);
    e.fx = __builtin_nontemporal_load(wr); e.fy = __builtin_nontemporal_load(wr + 64); e.fz = __builtin_nontemporal_load(wr + 128);
    e.k = LOADK ? __builtin_nontemporal_load(wr + 192) : 0.0;
#elif defined(MGCFD_EXP_ROW_LD_SC1)  // (experiment: agent-scope loads of the weights — past the XCD's L2, from the memory-side cache)
    e.code = nbr[(row << 6) + lane];
    e.fx = __hip_atomic_load(wr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    e.fy = __hip_atomic_load(wr + 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    e.fz = __hip_atomic_load(wr + 128, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    e.k = LOADK ? __hip_atomic_load(wr + 192, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
#else
    e.code = nbr[(row << 6) + lane];
    e.fx = wr[0]; e.fy = wr[64]; e.fz = wr[128];
    e.k = LOADK ? wr[192] : 0.0;
#endif
    return e;
}

struct Flux5 { double d, mx, my, mz, en; };

// One edge's contribution to THIS node's flux (flux_kernel.elemfunc.c:130-189 seen from this
// node: "me" - "other"; the b-side sign is folded into fx,fy,fz by the plan, x - f*y == x + (-f)*y).
template <bool LOADK>
__device__ __forceinline__ Flux5 edge_flux(const NodeQ &me, const FluxC &fm, const NodeQ &ot, const EdgeRow &e)
{
    const FluxC fo = flux_contribution(ot);
    const bool me_is_b = (e.code & kT16RoleB) != 0;
    const double fx = e.fx, fy = e.fy, fz = e.fz;
    double k = e.k;
    if (!LOADK) {
        // The plan stores f = -+0.5*e, so sqrt(f.f) = |e|/2 exactly and -(|e|/2 * s) is the
        // reference's -|e|*s*0.5 bit for bit (power-of-two scalings commute with rounding).
        const double half_ewt = sqrt(fx * fx + fy * fy + fz * fz);           // flux_kernel.elemfunc.c:27
        k = -(half_ewt * double(0.2f));                                       // :130, smoothing_coefficient = double(0.2f)
    }
    // factor = k * (speed_a + speed_b + c_a + c_b), left-associated (:130-131); only the order
    // of the two sound speeds depends on which end this node is.
    const double c_a = me_is_b ? ot.c : me.c;
    const double c_b = me_is_b ? me.c : ot.c;
    const double factor = k * (((me.speed + ot.speed) + c_a) + c_b);
    Flux5 f;
    f.d = factor * (me.rho - ot.rho) + fx * (me.mx + ot.mx) + fy * (me.my + ot.my) + fz * (me.mz + ot.mz);
    f.en = factor * (me.en - ot.en) + fx * (fm.ex + fo.ex) + fy * (fm.ey + fo.ey) + fz * (fm.ez + fo.ez);
    f.mx = factor * (me.mx - ot.mx) + fx * (fm.xx + fo.xx) + fy * (fm.xy + fo.xy) + fz * (fm.xz + fo.xz);
    f.my = factor * (me.my - ot.my) + fx * (fm.xy + fo.xy) + fy * (fm.yy + fo.yy) + fz * (fm.yz + fo.yz);
    f.mz = factor * (me.mz - ot.mz) + fx * (fm.xz + fo.xz) + fy * (fm.yz + fo.yz) + fz * (fm.zz + fo.zz);
    return f;
}

// What a node does with its complete flux: store it, or (FUSE) apply time_step to it
// (cfd_loops.cpp:241-268) — same operations as k_time_step — and write the new state to fs.q_out.
template <bool FUSE>
__device__ __forceinline__ void finish_node(int64_t i, int64_t nel, int64_t stride, double a0, double a1, double a2,
                                            double a3, double a4, double *__restrict__ fluxes, const FusedStep &fs,
                                            double min_dt, unsigned t)
{
    if (!FUSE) {
        if (i < nel) {
#ifdef MGCFD_ABL_FREE_ST_AOS           /* diagnostic: the node's fluxes written as one 40-byte record (layout wrong) */
            *reinterpret_cast<double2 *>(fluxes + 5 * i) = make_double2(a0, a1);
            *reinterpret_cast<double2 *>(fluxes + 5 * i + 2) = make_double2(a2, a3);
            fluxes[5 * i + 4] = a4;
#else
            MGCFD_ST_FLUX(fluxes + i, a0); MGCFD_ST_FLUX(fluxes + stride + i, a1); MGCFD_ST_FLUX(fluxes + 2 * stride + i, a2);
            MGCFD_ST_FLUX(fluxes + 3 * stride + i, a3); MGCFD_ST_FLUX(fluxes + 4 * stride + i, a4);
#endif
        }
        return;
    }
    // ---- fused time_step: same operations as k_time_step on the flux just summed ----
    // (operands fetched here, not under the row loop: the loop already sits at the register budget
    //  of 3 waves per SIMD and hoisting these twelve registers makes it spill)
    double sf_next = __longlong_as_double(0x7FF0000000000000LL);          // +inf: lanes past nel
    double ss = 0.0;                                                      // this node's share of the residual sum of squares
    if (i < nel) {
        const double r0 = fs.old_variables[i], r1 = fs.old_variables[stride + i], r2 = fs.old_variables[2 * stride + i],
                     r3 = fs.old_variables[3 * stride + i], r4 = fs.old_variables[4 * stride + i];
        double sf;
        if (fs.partial_min) {                       // first stage: finish compute_step_factor (cfd_loops.cpp:137-156)
            sf = min_dt / fs.volumes[i];
            fs.step_factors[i] = sf;
        } else {
            sf = fs.step_factors[i];
        }
        const double factor = sf / fs.rk_div;
        const double rho = r0 + factor * a0, mx = r1 + factor * a1, my = r2 + factor * a2, mz = r3 + factor * a3,
                     en = r4 + factor * a4;
        // q_out may be the array old_variables points at (last stage, in place): this thread has read
        // its node's old values above and nobody else reads them
        store_conserved(fs.q_out, stride, i, rho, mx, my, mz, en);
        if (fs.residuals || fs.sumsq_partial) {
            const double d0 = rho - r0, d1 = mx - r1, d2 = my - r2, d3 = mz - r3, d4 = en - r4;
            if (fs.residuals) {                      // (null: the caller writes it on demand, solver.cpp settle_residuals)
                MGCFD_ST_STAGE(fs.residuals + i, d0); MGCFD_ST_STAGE(fs.residuals + stride + i, d1); MGCFD_ST_STAGE(fs.residuals + 2 * stride + i, d2);
                MGCFD_ST_STAGE(fs.residuals + 3 * stride + i, d3); MGCFD_ST_STAGE(fs.residuals + 4 * stride + i, d4);
            }
            if (fs.sumsq_partial) ss = (((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3) + d4 * d4;
        }
        if (fs.check) {
            const bool finite = isfinite(rho) && isfinite(mx) && isfinite(my) && isfinite(mz) && isfinite(en);
            int code = 0;
            if (!finite) code = 1;
            else if (rho < 0.0) code = 2;
            else if (en < 0.0) code = 3;
            if (code) atomicMin(fs.err, err_key(fs.check, fs.old_of_new[i], code));
        }
        // look-ahead: the next sweep's compute_step_factor starts from the state just produced
        if (fs.next_partial_min) {
            const Derived d = derive(rho, mx, my, mz, en);
            const double dt = fs.cbrt_vol[i] / (d.speed + d.c);          // k_step_factor_local
            sf_next = fs.cfl * dt;
        } else if (fs.next_legacy_sf) {
            const Derived d = derive(rho, mx, my, mz, en);
            if (fs.next_nodal) fs.next_legacy_sf[i] = nodal_step_factor(d, fs.cbrt_vol[i], fs.volumes[i], fs.cfl);   // k_step_factor_nodal
            else fs.next_legacy_sf[i] = fs.cfl / (sqrt(fs.volumes[i]) * (d.speed + d.c));   // k_step_factor_legacy
        }
    }
    if (fs.next_partial_min || fs.sumsq_partial) {  // uniform: every thread of the workgroup takes part
        __shared__ double s_next[2][kBlock / 64];
        sf_next = wave_min(sf_next);
        ss = wave_sum(ss);
        if ((threadIdx.x & 63) == 0) { s_next[0][threadIdx.x >> 6] = sf_next; s_next[1][threadIdx.x >> 6] = ss; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double m = s_next[0][0], sum = s_next[1][0];
            for (int wv = 1; wv < kBlock / 64; wv++) { m = fmin(m, s_next[0][wv]); sum += s_next[1][wv]; }
            if (fs.next_partial_min) fs.next_partial_min[t] = m;
            if (fs.sumsq_partial) fs.sumsq_partial[t] = sum;
        }
    }
}

// The boundary rows of a node (after its internal rows): solid-wall faces, then far-field faces.
__device__ __forceinline__ void boundary_rows(const NodeQ &me, const FluxC &fm, const FarField &ff,
                                              const uint16_t *__restrict__ nbr16, const double *__restrict__ w,
                                              int64_t first_row, int32_t n_bnd, int lane, int classes, double &a0,
                                              double &a1, double &a2, double &a3, double &a4)
{
    for (int32_t r = 0; r < n_bnd; r++) {
        const EdgeRow e = load_row<false>(nbr16, w, first_row + r, lane);
        const double fx = e.fx, fy = e.fy, fz = e.fz;
        if (e.code == kT16Wall && (classes & 2)) {
            // flux_boundary_kernel.elemfunc.c:37-64: pressure force only
            a0 += 0.0;
            a1 += fx * me.p;
            a2 += fy * me.p;
            a3 += fz * me.p;
            a4 += 0.0;
        } else if (e.code == kT16Far && (classes & 4)) {
            // flux_wall_kernel.elemfunc.c:51-88: average with the far-field state
            a0 += fx * (ff.var[1] + me.mx) + fy * (ff.var[2] + me.my) + fz * (ff.var[3] + me.mz);
            a4 += fx * (ff.fc_de[0] + fm.ex) + fy * (ff.fc_de[1] + fm.ey) + fz * (ff.fc_de[2] + fm.ez);
            a1 += fx * (ff.fc_mx[0] + fm.xx) + fy * (ff.fc_mx[1] + fm.xy) + fz * (ff.fc_mx[2] + fm.xz);
            a2 += fx * (ff.fc_my[0] + fm.xy) + fy * (ff.fc_my[1] + fm.yy) + fz * (ff.fc_my[2] + fm.yz);
            a3 += fx * (ff.fc_mz[0] + fm.xz) + fy * (ff.fc_mz[1] + fm.yz) + fz * (ff.fc_mz[2] + fm.zz);
        }
    }
}

// ROLE (fused stages only): 0 = may finish compute_step_factor (first stage), 2 = may write the residual, its
// squares and the look-ahead (last stage), 1 = neither: the paths a stage cannot take are compiled out.
// 3 = a last stage that also leaves the next sweep's partial minima, 4 = ... fvcorr's next step factors instead,
// 5 = a middle stage that applies the first stage's time_step while it stages its input (FusedStep::vin_flux); stage_role()
// beside launch_flux reads the role off a stage's arguments.
// TAIL: the level has long rows (TailPlan): the per-node loop stops at the tile's row limit and the workgroup
// evaluates the remaining entries together (see below).
// LOADK: the length factor k is streamed with the row's weights; false: recomputed from them.
// The workgroup's LDS: the staged records, the first stage's partial minima per wave, the last stage's per-wave sums
// (559 records x 96 B + 32 + 64 B = 53,760 B = 42 of the 1,280-byte granules LDS is handed out in: three workgroups per CU).
struct FluxTileLds {
    double2 tile[kTileCap * kLdsRecD2];
    double s_pm[kBlock / 64];
    double s_next[2][kBlock / 64];
};
// SLIM: the 80-byte records (lds_put_record80) of at most kTileCap4 staged nodes, 40,896 B: four workgroups per CU.  Levels
// whose every tile halo fits kTileCap4 - kTile slots (the launcher checks halo_max; no overflow table, no second halo id).
struct FluxTileLds4 {
    double2 tile[kTileCap4 * kLdsRec80D2];
    double s_pm[kBlock / 64];
    double s_next[2][kBlock / 64];
};
static_assert(sizeof(FluxTileLds4) <= 160 * 1024 / 4, "four workgroups per CU");
static_assert(kTileCap4 - kTile < kBlock, "one halo id per thread");

// The kernel's body as a function of the workgroup's position in the launch (`block`): k_flux_tile calls it with blockIdx.x
// (tools/exp/sweep_flow.patch: a dataflow sweep calls it with the tile a workgroup has claimed).
// SLIM (with FluxTileLds4): 80-byte records and the rows walked one at a time, for four workgroups per CU.
template <bool LOADK, bool FUSE, bool ACC, int ROLE, bool TAIL, bool PUSH, bool SLIM = false, typename Lds = FluxTileLds>
__device__ __forceinline__ void
flux_tile_body(Lds &lds, const unsigned block,
               const double *__restrict__ q, const int32_t *__restrict__ tile_halo, uint32_t n_tiles, int32_t pad_row,
               int64_t stride, int64_t nel, const int32_t *__restrict__ slice_row0,
               const int32_t *__restrict__ rows_int, const int32_t *__restrict__ rows_bnd,
               const uint16_t *__restrict__ nbr16, const double *__restrict__ w,
               const int32_t *__restrict__ tile_ovf_ptr, const int32_t *__restrict__ tile_ovf, const FarField &ff,
               double *__restrict__ fluxes, int classes, const FusedStep &fs, const TailPlan &tp,
               const StagePush &push /* PUSH instantiations only: the stage sends its own message (device_plan.hpp) */,
               const bool block_is_tile = false /* `block` IS the tile (tools/exp/sweep_flow.patch) */)
{
    static_assert(!PUSH || FUSE, "only a fused stage sends its message");
    PH_BEGIN();
    static_assert(!SLIM || (!TAIL && !PUSH && ROLE != 5), "80-byte records: the stages without long rows, message or absorbed stage");
    double2 *const tile = lds.tile;

    // FUSE: this launch is a whole Runge-Kutta stage — the node's complete flux never leaves
    // registers; time_step (cfd_loops.cpp:241-268) is applied to it at the end and the new state
    // goes to fs.q_out (a different buffer: neighbours still read the stage's input from q).
    double min_dt = 0.0;
    // First stage: the minimum over the step-factor partials.  Their loads go out with the prologue's (last, they
    // are not on its dependent chain), the reduction happens after the records are staged and shares the staging
    // barrier, so none of it adds to the prologue's latency chain.
    constexpr int kPartPre = 6;                                           // partials per thread held in registers (1,536 tiles)
    double *const s_pm = lds.s_pm;
    double pmv[kPartPre];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    unsigned t = block_is_tile ? block : xcd_contiguous_block(block, n_tiles);   // n_tiles == gridDim.x, without the hidden-argument load
    if (PUSH) {
        // boundary tiles in dispatch order first (their message leaves while the rest of the launch runs), the interior
        // tiles behind them in XCD-contiguous ranges
        const unsigned nb = unsigned(push.n_boundary);
        t = block < nb ? block : nb + xcd_contiguous_block(block - nb, n_tiles - nb);
    }
    if (FUSE && fs.tile_list) t = unsigned(fs.tile_list[t]);           // a launch over part of the level (uniform branch)
    const int64_t base = int64_t(t) * kTile;
    const int64_t i = base + tid;
    const int32_t slice = __builtin_amdgcn_readfirstlane(static_cast<int32_t>(i >> 6));

    // Issue order of the prologue's loads (they return in order, and a wait after a conditional load
    // is conservative, so none of them sits under a branch): the halo ids first — they head the only
    // dependent chain (ids -> halo state; fixed-stride table, the address needs only the tile number)
    // — then the own node's state, the first two rows' ids and weights, and the halo state by id.
    const int32_t *hrow = tile_halo + int64_t(t) * kHaloStride;
    const int32_t hid = hrow[tid];                                     // -1: no halo node for this thread
    const int32_t hid2 = (!SLIM && ROLE != 5 && tid < kHaloStride - kBlock) ? hrow[kBlock + tid] : -1;   // halo larger than the workgroup (rare)
    const int32_t row0 = slice_row0[slice];
    const int32_t n_int = (classes & 1) ? (TAIL ? tp.rows_main : rows_int)[slice] : 0;
    const int32_t n_bnd = rows_bnd[slice];
    const bool has_halo = hid >= 0;
    const int64_t hnode = has_halo ? int64_t(hid) : i;
    double o0, o1, o2, o3, o4, g0, g1, g2, g3, g4;
    EdgeRow e0, e1;
    if (FUSE && ROLE == 5) {
        // The input state of this stage does not exist in memory: it is the first stage's time_step,
        // old + (min_dt/volume/vin_div) * flux, applied here to every staged node (own and halo) from the
        // first stage's fluxes — the split sweep of a multi-rank run saves its separate time_step launch.
#pragma unroll
        for (int u = 0; u < kPartPre; u++) {
            const int k = threadIdx.x + u * kBlock;
            pmv[u] = fs.partial_min[k < fs.n_partial ? k : fs.n_partial - 1];
        }
        const double *od = fs.old_variables, *fl = fs.vin_flux;
        const double b0 = od[i], b1 = od[stride + i], b2 = od[2 * stride + i], b3 = od[3 * stride + i], b4 = od[4 * stride + i];
        const double f0 = fl[i], f1 = fl[stride + i], f2 = fl[2 * stride + i], f3 = fl[3 * stride + i], f4 = fl[4 * stride + i];
        const double vo = fs.volumes[i];
        const double c0 = od[hnode], c1 = od[stride + hnode], c2 = od[2 * stride + hnode], c3 = od[3 * stride + hnode],
                     c4 = od[4 * stride + hnode];
        const double h0 = fl[hnode], h1 = fl[stride + hnode], h2 = fl[2 * stride + hnode], h3 = fl[3 * stride + hnode],
                     h4 = fl[4 * stride + hnode];
        const double vh = fs.volumes[hnode];
        e0 = load_row<LOADK>(nbr16, w, n_int > 0 ? row0 : pad_row, lane);
        e1 = load_row<LOADK>(nbr16, w, n_int > 1 ? row0 + 1 : pad_row, lane);
        double pm = pmv[0];
#pragma unroll
        for (int u = 1; u < kPartPre; u++) pm = fmin(pm, pmv[u]);
        for (int k = threadIdx.x + kPartPre * kBlock; k < fs.n_partial; k += kBlock) pm = fmin(pm, fs.partial_min[k]);
        pm = wave_min(pm);
        if (lane == 0) s_pm[tid >> 6] = pm;
        __syncthreads();
        min_dt = s_pm[0];
        for (int wv = 1; wv < kBlock / 64; wv++) min_dt = fmin(min_dt, s_pm[wv]);
        const double fo = (min_dt / vo) / fs.vin_div, fh = (min_dt / vh) / fs.vin_div;      // k_time_step: factor = sf / rk_div
        o0 = b0 + fo * f0; o1 = b1 + fo * f1; o2 = b2 + fo * f2; o3 = b3 + fo * f3; o4 = b4 + fo * f4;
        g0 = c0 + fh * h0; g1 = c1 + fh * h1; g2 = c2 + fh * h2; g3 = c3 + fh * h3; g4 = c4 + fh * h4;
        if (fs.check_vin && i < nel) {                                  // the first stage's check_for_invalid_variables (its own, earlier, sequence number)
            const bool finite = isfinite(o0) && isfinite(o1) && isfinite(o2) && isfinite(o3) && isfinite(o4);
            int code = 0;
            if (!finite) code = 1;
            else if (o0 < 0.0) code = 2;
            else if (o4 < 0.0) code = 3;
            if (code) atomicMin(fs.err, err_key(fs.check_vin, fs.old_of_new[i], code));
        }
    } else {
        o0 = q[i]; o1 = q[stride + i]; o2 = q[2 * stride + i]; o3 = q[3 * stride + i]; o4 = q[4 * stride + i];
        g0 = q[hnode]; g1 = q[stride + hnode]; g2 = q[2 * stride + hnode]; g3 = q[3 * stride + hnode]; g4 = q[4 * stride + hnode];
        // (a row the slice does not have is read from pad_row, a row of padding after the last one: the
        //  load itself is never conditional, so the compiler can count the loads in flight exactly)
        e0 = load_row<LOADK>(nbr16, w, n_int > 0 ? row0 : pad_row, lane);
        if (!SLIM) e1 = load_row<LOADK>(nbr16, w, n_int > 1 ? row0 + 1 : pad_row, lane);
    }
    // (the step-factor partials: wanted only at the staging barrier, so requested after everything on the critical chain)
    if (FUSE && ROLE == 0) {                         // (role 0 is launched only with fs.partial_min set)
#pragma unroll
        for (int u = 0; u < kPartPre; u++) {
            const int k = threadIdx.x + u * kBlock;
            pmv[u] = fs.partial_min[k < fs.n_partial ? k : fs.n_partial - 1];     // clamped: a repeat does not change a minimum
        }
    }
    const NodeQ me = make_nodeq(o0, o1, o2, o3, o4);
    lds_put_rec<SLIM>(tile, uint32_t(tid), me);
    // Unconditional: a thread without a halo node re-reads its own node and parks the copy in its
    // (unused) halo slot.  A branch here lets the compiler sink the gather loads below the own
    // record's derivation and serialise the two.  (SLIM: the last threads have no halo slot — their halo
    // id is -1 on the levels that run it — and write the copy over their own record, the same bits.)
    const uint32_t hslot = (SLIM && tid >= kTileCap4 - kTile) ? uint32_t(tid) : uint32_t(kTile + tid);
    lds_put_rec<SLIM>(tile, hslot, make_nodeq(g0, g1, g2, g3, g4));
    if (hid2 >= 0) lds_store_record(tile, uint32_t(kTile + kBlock + tid), load_and_derive(q, stride, hid2));

    const FluxC fm_pre = flux_contribution(me);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
    if (ACC) {
        a0 = fluxes[i]; a1 = fluxes[stride + i]; a2 = fluxes[2 * stride + i];
        a3 = fluxes[3 * stride + i]; a4 = fluxes[4 * stride + i];
    }
    const int32_t ovf0 = tile_ovf_ptr[t];
    if (FUSE && ROLE == 0) {                         // (role 0 is launched only with fs.partial_min set)
        double pm = pmv[0];
#pragma unroll
        for (int u = 1; u < kPartPre; u++) pm = fmin(pm, pmv[u]);
        for (int k = threadIdx.x + kPartPre * kBlock; k < fs.n_partial; k += kBlock) pm = fmin(pm, fs.partial_min[k]);
        pm = wave_min(pm);
        if (lane == 0) s_pm[tid >> 6] = pm;
    }
    PH_MARK(0);
    __syncthreads();
    PH_MARK(1);
    // (the four per-wave minima stay in LDS until the epilogue: nothing of them occupies a register across the row loop)

    // ---- phase 2: incidence rows two at a time (independent arithmetic, ordered accumulation),
    //      ids/weights fetched two rows ahead ----
    // The row pair's work (rows e0, e1 -> a0..a4, strictly in row order = the reference's summation order).
    // ELL padding carries zero weights, so on a sum that started at +0.0 its +-0.0 contribution changes no
    // bit (x + y = -0.0 only if both are); a sum read from memory (ACC) may be -0.0 and skips padding.
    // With long rows (TAIL) an entry the plan moved to the workgroup's list is blanked in nbr16 only (its weights stay,
    // other kernels read them), so there too a padding code skips the add.
    // Halo nodes beyond the LDS tile (ragged clusters) are read from HBM.
#define MGCFD_ROW_PAIR()                                                                                     \
    do {                                                                                                     \
            const uint32_t s0 = e0.code & kT16SlotMask, s1 = e1.code & kT16SlotMask;                         \
            const bool v0 = s0 != kT16Pad, v1 = s1 != kT16Pad;                                               \
            const bool o0 = v0 && s0 >= uint32_t(kTileCap), o1 = v1 && s1 >= uint32_t(kTileCap);             \
            NodeQ n0, n1;                                                                                    \
            if (!TAIL && __builtin_expect(__any(o0 || o1), 0)) {      /* (long rows: such entries are on the list) */ \
                n0 = o0 ? load_and_derive(q, stride, tile_ovf[ovf0 + int32_t(s0) - kTileCap])                \
                        : lds_load_record(tile, v0 ? s0 : uint32_t(tid));                                    \
                n1 = o1 ? load_and_derive(q, stride, tile_ovf[ovf0 + int32_t(s1) - kTileCap])                \
                        : lds_load_record(tile, v1 ? s1 : uint32_t(tid));                                    \
            } else {                                                                                         \
                n0 = lds_load_record(tile, v0 ? s0 : uint32_t(tid));                                         \
                n1 = lds_load_record(tile, v1 ? s1 : uint32_t(tid));                                         \
            }                                                                                                \
            Flux5 f0, f1;                                                                                    \
            f0 = edge_flux<LOADK>(me, fm_pre, n0, e0);                                                       \
            f1 = edge_flux<LOADK>(me, fm_pre, n1, e1);                                                       \
            if (ACC || TAIL) {                                                                               \
                a0 = v0 ? a0 + f0.d : a0;   a1 = v0 ? a1 + f0.mx : a1;   a2 = v0 ? a2 + f0.my : a2;          \
                a3 = v0 ? a3 + f0.mz : a3;  a4 = v0 ? a4 + f0.en : a4;                                       \
                a0 = v1 ? a0 + f1.d : a0;   a1 = v1 ? a1 + f1.mx : a1;   a2 = v1 ? a2 + f1.my : a2;          \
                a3 = v1 ? a3 + f1.mz : a3;  a4 = v1 ? a4 + f1.en : a4;                                       \
            } else {                                                                                         \
                a0 += f0.d; a1 += f0.mx; a2 += f0.my; a3 += f0.mz; a4 += f0.en;                              \
                a0 += f1.d; a1 += f1.mx; a2 += f1.my; a3 += f1.mz; a4 += f1.en;                              \
            }                                                                                                \
    } while (0)
    // long rows: what the workgroup's list pass needs first is requested here and arrives while the rows are walked
    int32_t tl_b = 0, tl_e = 0, tl_nb = 0, tl_nc = 0;
    double2 tl_r0 = make_double2(0.0, 0.0), tl_r1 = tl_r0, tl_r2 = tl_r0;
    if (TAIL && (classes & 1)) {
        tl_b = tp.tile_ptr[t]; tl_e = tp.tile_ptr[t + 1];
        tl_nb = tp.begin[i]; tl_nc = tp.count[i];
        const int32_t e_first = tl_b + tid;
        if (e_first < tl_e) { tl_r0 = tp.rec[3 * int64_t(e_first)]; tl_r1 = tp.rec[3 * int64_t(e_first) + 1]; tl_r2 = tp.rec[3 * int64_t(e_first) + 2]; }
    }
    double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0, r4 = 0.0, sfv = 0.0;       // fused stages: the time_step operands
    // SLIM: one row at a time, the next row's ids and weights fetched one row ahead (two rows of records and
    // weights in registers do not fit the 128 registers of four waves per SIMD).  Same rows in the same order, the same
    // adds; no overflow table (every halo node has its slot).
#define MGCFD_ROW_ONE()                                                                                      \
    do {                                                                                                     \
            const uint32_t s0 = e0.code & kT16SlotMask;                                                      \
            const bool v0 = s0 != kT16Pad;                                                                   \
            const NodeQ n0 = lds_get_record80(tile, v0 ? s0 : uint32_t(tid));                              \
            const Flux5 f0 = edge_flux<LOADK>(me, fm_pre, n0, e0);                                           \
            if (ACC) {                                                                                       \
                a0 = v0 ? a0 + f0.d : a0;   a1 = v0 ? a1 + f0.mx : a1;   a2 = v0 ? a2 + f0.my : a2;          \
                a3 = v0 ? a3 + f0.mz : a3;  a4 = v0 ? a4 + f0.en : a4;                                       \
            } else {                                                                                         \
                a0 += f0.d; a1 += f0.mx; a2 += f0.my; a3 += f0.mz; a4 += f0.en;                              \
            }                                                                                                \
    } while (0)
    if (SLIM) {
        int32_t r = 0;
        for (; r + 1 < n_int; r++) {
            const EdgeRow e1n = load_row<LOADK>(nbr16, w, row0 + r + 1, lane);
            MGCFD_ROW_ONE();
            e0 = e1n;
        }
        // the last row: the time_step operands arrive while it is summed (as after the last pair below)
        if (FUSE) {
            if (ROLE == 0) {
                r0 = me.rho; r1 = me.mx; r2 = me.my; r3 = me.mz; r4 = me.en;
            } else {
                r0 = fs.old_variables[i]; r1 = fs.old_variables[stride + i]; r2 = fs.old_variables[2 * stride + i];
                r3 = fs.old_variables[3 * stride + i]; r4 = fs.old_variables[4 * stride + i];
            }
            sfv = (ROLE == 0 ? fs.volumes : fs.step_factors)[i];
        }
        if (r < n_int) MGCFD_ROW_ONE();
    } else
    {
        // every pair but the last, each prefetching the pair after it
        int32_t r = 0;
        for (; r + 2 < n_int; r += 2) {
            const EdgeRow e2 = load_row<LOADK>(nbr16, w, row0 + r + 2, lane);
            const EdgeRow e3 = load_row<LOADK>(nbr16, w, r + 3 < n_int ? row0 + r + 3 : pad_row, lane);
            MGCFD_ROW_PAIR();
            e0 = e2; e1 = e3;
        }
        // The last pair has nothing left to prefetch: in the fused stages the registers its prefetch would
        // have used take the time_step operands instead, which arrive while the pair is being summed.
        if (FUSE) {
            if (ROLE == 0) {
                // the first stage's input IS the sweep's start state (the launcher checks q == old_variables): the node's own
                // record, live in registers for every edge anyway, holds the five values
                r0 = me.rho; r1 = me.mx; r2 = me.my; r3 = me.mz; r4 = me.en;
            } else {
                r0 = fs.old_variables[i]; r1 = fs.old_variables[stride + i]; r2 = fs.old_variables[2 * stride + i];
                r3 = fs.old_variables[3 * stride + i]; r4 = fs.old_variables[4 * stride + i];
            }
            sfv = ((ROLE == 0 || ROLE == 5) ? fs.volumes : fs.step_factors)[i];
        }
        if (r < n_int) MGCFD_ROW_PAIR();
    }
#undef MGCFD_ROW_PAIR
#undef MGCFD_ROW_ONE
    PH_MARK(2);

    if (TAIL && (classes & 1) && tl_e > tl_b) {                            // (uniform)
        // Long rows.  The entries beyond the tile's row limit, one per thread whatever node they belong to: the same
        // edge_flux from the same operands (the owner's record is read back from LDS); then every owner adds its own
        // entries in row order — the accumulation order is untouched, only the evaluation is spread over the
        // workgroup instead of waiting for the highest-degree lanes.  The results of the last round of 256 entries
        // (usually the only one) are handed over through LDS, where the records are dead by then; earlier rounds
        // go through a global scratch.
        const int32_t last0 = tl_b + ((tl_e - tl_b - 1) / kBlock) * kBlock;   // first entry of the last round
        int32_t e = tl_b + tid;
        double2 r0 = tl_r0, r1 = tl_r1, r2 = tl_r2;
        Flux5 fl;
        fl.d = 0.0; fl.mx = 0.0; fl.my = 0.0; fl.mz = 0.0; fl.en = 0.0;
        while (e < tl_e) {
            const double2 c0 = r0, c1 = r1, c2 = r2;
            const int32_t en = e + kBlock;
            if (en < tl_e) { r0 = tp.rec[3 * int64_t(en)]; r1 = tp.rec[3 * int64_t(en) + 1]; r2 = tp.rec[3 * int64_t(en) + 2]; }   // next round's entry
            const uint32_t word = static_cast<uint32_t>(__double_as_longlong(c2.x));
            const uint32_t own = word & 0xFFFFu;
            if (own != kT16Pad) {
                EdgeRow er;
                er.code = word >> 16;
                er.fx = c0.x; er.fy = c0.y; er.fz = c1.x; er.k = LOADK ? c1.y : 0.0;
                const uint32_t s = er.code & kT16SlotMask;
                const NodeQ mo = lds_load_record(tile, own);
                const NodeQ ot = s >= uint32_t(kTileCap) ? load_and_derive(q, stride, tile_ovf[ovf0 + int32_t(s) - kTileCap])
                                                         : lds_load_record(tile, s);
                const Flux5 f = edge_flux<LOADK>(mo, flux_contribution(mo), ot, er);
                if (e >= last0) {
                    fl = f;
                } else {
                    double2 *out = tp.flux + 3 * int64_t(e);
                    out[0] = make_double2(f.d, f.mx); out[1] = make_double2(f.my, f.mz); out[2] = make_double2(f.en, 0.0);
                }
            }
            e = en;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // this wave's scratch stores have left
        __syncthreads();                                                  // ... and nobody reads a record any more
        tile[3 * tid] = make_double2(fl.d, fl.mx); tile[3 * tid + 1] = make_double2(fl.my, fl.mz); tile[3 * tid + 2] = make_double2(fl.en, 0.0);
        __syncthreads();
        // (a tile's scratch range is whole 128-byte lines that only this workgroup touches, and it reads them
        //  only now: no stale copy can sit in this CU's L1)
        // ordered adds: first the node's entries of the earlier rounds (global), then those of the last round (LDS)
        const int32_t n_glob = min(tl_nc, max(0, last0 - tl_nb));
#define MGCFD_ADD_ENTRIES(in, count)                                                                              \
        do {                                                                                                      \
            int32_t k_ = 0;                                                                                       \
            for (; k_ + 3 <= (count); k_ += 3) {           /* the records fetched three entries ahead of the sums */ \
                const double2 u0 = in[0], u1 = in[1], u2 = in[2], v0 = in[3], v1 = in[4], v2 = in[5],              \
                              w0 = in[6], w1 = in[7], w2 = in[8];                                                 \
                in += 9;                                                                                          \
                a0 += u0.x; a1 += u0.y; a2 += u1.x; a3 += u1.y; a4 += u2.x;                                       \
                a0 += v0.x; a1 += v0.y; a2 += v1.x; a3 += v1.y; a4 += v2.x;                                       \
                a0 += w0.x; a1 += w0.y; a2 += w1.x; a3 += w1.y; a4 += w2.x;                                       \
            }                                                                                                     \
            for (; k_ < (count); k_++) {                                                                          \
                const double2 u0 = in[0], u1 = in[1], u2 = in[2];                                                 \
                in += 3;                                                                                          \
                a0 += u0.x; a1 += u0.y; a2 += u1.x; a3 += u1.y; a4 += u2.x;                                       \
            }                                                                                                     \
        } while (0)
        if (n_glob > 0) {
            const double2 *in = tp.flux + 3 * int64_t(tl_nb);
            MGCFD_ADD_ENTRIES(in, n_glob);
        }
        {
            const double2 *in = tile + 3 * (tl_nb + n_glob - last0);
            const int32_t n_lds = tl_nc - n_glob;
            MGCFD_ADD_ENTRIES(in, n_lds);
        }
#undef MGCFD_ADD_ENTRIES
    }

    if ((classes & 6) && n_bnd > 0) {
        // The reference runs ALL solid-wall faces, then ALL far-field faces; the plan lists a
        // node's faces in exactly that order, so one walk over the rows keeps the per-node order.
        const int32_t first_bnd = rows_int[slice];
        const FluxC fm = fm_pre;
        for (int32_t r = 0; r < n_bnd; r++) {
            const EdgeRow e = load_row<false>(nbr16, w, int64_t(row0) + first_bnd + r, lane);
            const double fx = e.fx, fy = e.fy, fz = e.fz;
            if (e.code == kT16Wall && (classes & 2)) {
                // flux_boundary_kernel.elemfunc.c:37-64: pressure force only
                a0 += 0.0;
                a1 += fx * me.p;
                a2 += fy * me.p;
                a3 += fz * me.p;
                a4 += 0.0;
            } else if (e.code == kT16Far && (classes & 4)) {
                // flux_wall_kernel.elemfunc.c:51-88: average with the far-field state
                a0 += fx * (ff.var[1] + me.mx) + fy * (ff.var[2] + me.my) + fz * (ff.var[3] + me.mz);
                a4 += fx * (ff.fc_de[0] + fm.ex) + fy * (ff.fc_de[1] + fm.ey) + fz * (ff.fc_de[2] + fm.ez);
                a1 += fx * (ff.fc_mx[0] + fm.xx) + fy * (ff.fc_mx[1] + fm.xy) + fz * (ff.fc_mx[2] + fm.xz);
                a2 += fx * (ff.fc_my[0] + fm.xy) + fy * (ff.fc_my[1] + fm.yy) + fz * (ff.fc_my[2] + fm.yz);
                a3 += fx * (ff.fc_mz[0] + fm.xz) + fy * (ff.fc_mz[1] + fm.yz) + fz * (ff.fc_mz[2] + fm.zz);
            }
        }
    }

    if (!FUSE) {
        if (i < nel) {
            MGCFD_ST_FLUX(fluxes + i, a0); MGCFD_ST_FLUX(fluxes + stride + i, a1); MGCFD_ST_FLUX(fluxes + 2 * stride + i, a2);
            MGCFD_ST_FLUX(fluxes + 3 * stride + i, a3); MGCFD_ST_FLUX(fluxes + 4 * stride + i, a4);
        }
        PH_MARK(3);
        return;
    }
    // ---- fused time_step: same operations as k_time_step on the flux just summed ----
    double sf_next = __longlong_as_double(0x7FF0000000000000LL);          // +inf: lanes past nel
    double ss = 0.0;                                                      // this node's share of the residual sum of squares
    if (i < nel) {
        double sf = sfv;                            // (operands: requested before the last row pair)
        if (ROLE == 0 || ROLE == 5) {               // first stage (or the stage that absorbed it): finish compute_step_factor (cfd_loops.cpp:137-156)
            min_dt = s_pm[0];
            for (int wv = 1; wv < kBlock / 64; wv++) min_dt = fmin(min_dt, s_pm[wv]);
            sf = min_dt / sfv;                      // sfv holds the volume
            fs.step_factors[i] = sf;
        }
        const double factor = sf / fs.rk_div;
        const double rho = r0 + factor * a0, mx = r1 + factor * a1, my = r2 + factor * a2, mz = r3 + factor * a3,
                     en = r4 + factor * a4;
        // q_out may be the array old_variables points at (last stage, in place): this thread has read
        // its node's old values above and nobody else reads them
        store_conserved(fs.q_out, stride, i, rho, mx, my, mz, en);
        if (ROLE >= 2 && ROLE <= 4) {               // last stage: residual (validation.cpp:77-89)
            const double d0 = rho - r0, d1 = mx - r1, d2 = my - r2, d3 = mz - r3, d4 = en - r4;
            if (fs.residuals) {                      // (null: the caller writes it on demand, solver.cpp settle_residuals)
                MGCFD_ST_STAGE(fs.residuals + i, d0); MGCFD_ST_STAGE(fs.residuals + stride + i, d1); MGCFD_ST_STAGE(fs.residuals + 2 * stride + i, d2);
                MGCFD_ST_STAGE(fs.residuals + 3 * stride + i, d3); MGCFD_ST_STAGE(fs.residuals + 4 * stride + i, d4);
            }
            if (fs.sumsq_partial) ss = (((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3) + d4 * d4;
        }
        if (fs.check) {
            const bool finite = isfinite(rho) && isfinite(mx) && isfinite(my) && isfinite(mz) && isfinite(en);
            int code = 0;
            if (!finite) code = 1;
            else if (rho < 0.0) code = 2;
            else if (en < 0.0) code = 3;
            if (code) atomicMin(fs.err, err_key(fs.check, fs.old_of_new[i], code));
        }
        // look-ahead: the next sweep's compute_step_factor starts from the state just produced
        if (ROLE == 3) {
            const Derived d = derive(rho, mx, my, mz, en);
            const double dt = fs.cbrt_vol[i] / (d.speed + d.c);          // k_step_factor_local
            sf_next = fs.cfl * dt;
        } else if (ROLE == 4) {
            const Derived d = derive(rho, mx, my, mz, en);
            if (fs.next_nodal) fs.next_legacy_sf[i] = nodal_step_factor(d, fs.cbrt_vol[i], fs.volumes[i], fs.cfl);   // k_step_factor_nodal
            else fs.next_legacy_sf[i] = fs.cfl / (sqrt(fs.volumes[i]) * (d.speed + d.c));   // k_step_factor_legacy
        }
        if (PUSH && block < unsigned(push.n_boundary)) {
            // this node into the ghost slots of the neighbours that hold it
            for (int32_t e = push.send_ptr[i]; e < push.send_ptr[i + 1]; e++) {
                const int k = push.send_peer[e];
                const int64_t g = push.send_target[e];
                double *dst = push.peers.base[0];
                int64_t ps = push.peers.stride[0];
#pragma unroll
                for (int p = 1; p < kMaxPushPeers; p++) if (p == k) { dst = push.peers.base[p]; ps = push.peers.stride[p]; }
                dst[g] = rho; dst[ps + g] = mx; dst[2 * ps + g] = my; dst[3 * ps + g] = mz; dst[4 * ps + g] = en;
            }
        }
    }
    if (PUSH && block < unsigned(push.n_boundary)) {              // (uniform per workgroup)
        // as k_halo_push_flags: the stores acknowledged, the workgroup counted off, the last boundary tile raises the flags
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            __threadfence_system();
            const unsigned done = __hip_atomic_fetch_add(push.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            if (done == unsigned(push.n_boundary) - 1u) {
                __hip_atomic_store(push.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __threadfence_system();
#pragma unroll
                for (int p = 0; p < kMaxPushPeers; p++)
                    if (p < push.flags.n) __hip_atomic_store(push.flags.flag[p], push.flags.value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
    }
    if (ROLE == 3 || (ROLE >= 2 && ROLE <= 4 && fs.sumsq_partial)) {  // uniform: every thread of the workgroup takes part
        double (*const s_next)[kBlock / 64] = lds.s_next;
        if (ROLE == 3) sf_next = wave_min(sf_next);
        if (fs.sumsq_partial) ss = wave_sum(ss);
        if ((threadIdx.x & 63) == 0) { s_next[0][threadIdx.x >> 6] = sf_next; s_next[1][threadIdx.x >> 6] = ss; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double m = s_next[0][0], sum = s_next[1][0];
            for (int wv = 1; wv < kBlock / 64; wv++) { m = fmin(m, s_next[0][wv]); sum += s_next[1][wv]; }
            if (ROLE == 3) fs.next_partial_min[t] = m;
            if (fs.sumsq_partial) fs.sumsq_partial[t] = sum;
        }
    }
    PH_MARK(3);
}

template <int MINW, bool LOADK, bool FUSE, bool ACC, int ROLE, bool TAIL, bool PUSH = false, bool SLIM = false>
__global__ void __launch_bounds__(kBlock, MINW)
k_flux_tile(// the first 16 dwords of the arguments are preloaded into SGPRs at wave launch (Makefile:
            // -amdgpu-kernarg-preload-count): what the first loads of the prologue need comes first
            const double *__restrict__ q, const int32_t *__restrict__ tile_halo, uint32_t n_tiles, int32_t pad_row,
            int64_t stride, int64_t nel, const int32_t *__restrict__ slice_row0,
            const int32_t *__restrict__ rows_int, const int32_t *__restrict__ rows_bnd,
            const uint16_t *__restrict__ nbr16, const double *__restrict__ w,
            const int32_t *__restrict__ tile_ovf_ptr, const int32_t *__restrict__ tile_ovf, FarField ff,
            double *__restrict__ fluxes, int classes, FusedStep fs, TailPlan tp,
            StagePush push)
{
    __shared__ std::conditional_t<SLIM, FluxTileLds4, FluxTileLds> lds;
    flux_tile_body<LOADK, FUSE, ACC, ROLE, TAIL, PUSH, SLIM>(lds, blockIdx.x, q, tile_halo, n_tiles, pad_row, stride, nel, slice_row0, rows_int, rows_bnd, nbr16, w,
                                                       tile_ovf_ptr, tile_ovf, ff, fluxes, classes, fs, tp, push);
}

// One entry of the half-row plan (preprocess.hpp: hr_code, hr_w): the code word and the evaluator's three weights; k is recomputed.
__device__ __forceinline__ EdgeRow load_half_row(const uint32_t *__restrict__ code, const double *__restrict__ w3, int64_t row, int lane)
{
    EdgeRow e;
    e.code = code[(row << 6) + lane];
    const double *wr = w3 + row * (3 * kSlice) + lane;
    e.fx = wr[0]; e.fy = wr[64]; e.fz = wr[128];
    e.k = 0.0;
    return e;
}

#ifdef MGCFD_ORDER_FREE
// ------------------------------------------------------------------------------------------
// flux_free (the `fast` namespace only: MGCFD_OPT_EXACT = 0, MGCFD_OPT_FLUX_VARIANT bit 6): compute_flux_edge +
// boundary + far-field faces with ORDER-FREE accumulation.
//
// Every byte-saving layout of the bit-identical kernels that was tried (EXPERIMENTS.md; since removed) lost what it
// saved to the hand-over that keeps the reference's summation ORDER: a second pass over LDS and two more barriers.
// north_star's bound is 1e-10, not bits, so this kernel drops the order and nothing else: a tile streams ONE 28-byte
// entry per internal edge that touches it (the half-row plan, preprocess.hpp: the evaluator of an edge inside the tile
// is one of its end points, a cut edge is evaluated by the tile of each end), the evaluating lane adds +F to its own
// node's sum in registers and — for an edge inside the tile — adds -F to the other end's sum in LDS with ds_add_f64
// (the reference's expressions for the other end evaluate to exactly -F, flux_kernel.elemfunc.c:142-189).  One barrier,
// every node adds its LDS sum to its register sum, the boundary faces follow, store.  No second pass, no ordered adds;
// the result differs from the reference's by the rounding of a differently associated sum (<= 1e-12 relative per
// launch, tests/test_gpu_order_free.py) and is not reproducible bit for bit from run to run (LDS atomics commute, their
// rounding does not).
//
// Records are 64 bytes (rho, m, E, p, |v| + c, 1/rho): with contraction allowed |v| + c may be kept as one number, and
// the velocity is three multiplications away from 1/rho — one division and two square roots per staged node instead of
// three and two, four 16-byte LDS reads per neighbour instead of six.  Quad q of slot s sits at position q ^ ((s >> 2) & 3)
// of its record, so a 16-lane ds_read_b128 group reaches all 16 quad positions of the 256-byte bank row.
// ------------------------------------------------------------------------------------------
struct NodeF { double rho, vx, vy, vz, en, p, sc; };
constexpr int kFreeRecD2 = 3;                  // double2 per record (+ one double in the array beside)

// 1/x and sqrt(x) from the hardware's estimates and Newton steps in FMAs (~1e-16 relative; the IEEE sequences hipcc emits
// under -fno-fast-math cost 15 and 20 instructions, and fp64 instructions issue at a quarter of the fp32 rate: the kernel's
// phases are bound by them, profiles/r3_free_phases.txt)
__device__ __forceinline__ double fast_rcp(double x)
{
    double y = __builtin_amdgcn_rcp(x);
    double e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    e = fma(-x, y, 1.0);
    return fma(y, e, y);
}

// sqrt(x) for x > 0 (no special cases: x = 0 gives NaN)
__device__ __forceinline__ double fast_sqrt_pos(double x)
{
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;                  // g -> sqrt(x), h -> 0.5 / sqrt(x) (Goldschmidt)
    double r = fma(-h, g, 0.5);
    g = fma(g, r, g); h = fma(h, r, h);
    r = fma(-h, g, 0.5);
    g = fma(g, r, g); h = fma(h, r, h);
    const double d = fma(-g, g, x);
    return fma(d, h, g);
}

__device__ __forceinline__ double fast_sqrt(double x)
{
    const double g = fast_sqrt_pos(x);
    // (x = 0: the estimate is infinite; +inf: the estimate is 0 and the product NaN; negative or NaN: NaN, as sqrt gives)
    return (x > 0.0 && x < __builtin_inf()) ? g : ((x == 0.0 || x == __builtin_inf()) ? x : __builtin_nan(""));
}

// What a staged node keeps (round 4): the VELOCITY instead of the momentum.  The evaluating end needs both of its neighbour
// — m for the dissipation's differences, v for the convective terms — and rho * v is three multiplications where m / rho was
// a reciprocal (five instructions) and three.
__device__ __forceinline__ NodeF make_nodef(double rho, double mx, double my, double mz, double en)
{
    NodeF n;
    const double inv = fast_rcp(rho);
    n.rho = rho; n.en = en;
    n.vx = mx * inv; n.vy = my * inv; n.vz = mz * inv;
    const double speed_sqd = n.vx * n.vx + n.vy * n.vy + n.vz * n.vz;
    n.p = (kGamma - 1.0) * (en - 0.5 * rho * speed_sqd);
    n.sc = fast_sqrt(speed_sqd) + fast_sqrt(kGamma * n.p * inv);
    return n;
}

// LDS image of a staged node: 48 bytes (rho, v, E, p) in an array of records + |v| + c in an array of its own.
// 56 bytes per node: with the tile's 10 KB of sums, 546 nodes fit the 40 KB a
// workgroup may take when FOUR share a CU.  A 12-dword record stride spreads a 16-lane ds_read_b128 group over all 16 quad
// positions of the 256-byte bank row by itself.
__device__ __forceinline__ void lds_store_nodef(double2 *rec, double *scs, uint32_t slot, const NodeF &n)
{
    double2 *r = rec + slot * kFreeRecD2;
    r[0] = make_double2(n.rho, n.vx);
    r[1] = make_double2(n.vy, n.vz);
    r[2] = make_double2(n.en, n.p);
    scs[slot] = n.sc;
}

__device__ __forceinline__ NodeF lds_load_nodef(const double2 *rec, const double *scs, uint32_t slot)
{
    const double2 *r = rec + slot * kFreeRecD2;
    const double2 a = r[0], c = r[1], d = r[2];
    NodeF n;
    n.rho = a.x; n.vx = a.y; n.vy = c.x; n.vz = c.y; n.en = d.x; n.p = d.y; n.sc = scs[slot];
    return n;
}

// what the evaluating end keeps beside its record: momentum and total enthalpy per volume
struct OwnF { double mx, my, mz, H; };
__device__ __forceinline__ OwnF make_ownf(const NodeF &n)
{
    OwnF o;
    o.mx = n.rho * n.vx; o.my = n.rho * n.vy; o.mz = n.rho * n.vz; o.H = n.en + n.p;
    return o;
}

// MINUS the flux of flux_kernel.elemfunc.c:130-161 seen from end `a` (the plan folded the b-side sign into the weights f),
// regrouped: with d_x = f . m_x = rho_x (f . v_x) the contracted flux contributions are f . Phi_x = v_x d_x + p_x f for the
// momenta and H_x (f . v_x) for the energy (cfd_loops.h:57-83), so nothing of the 3 x 3 tensors is formed.  The NEGATED
// flux is what the other end of an edge inside the tile adds to its sum (ds_add_f64 has no operand negation; the evaluating
// end subtracts, which costs nothing).  The weights of a real entry are never all zero; a padding entry's are, and it meets
// its own record as "neighbour": the length is then ~1e-150 times a difference that is exactly zero.
__device__ __forceinline__ Flux5 edge_flux_neg_f(const NodeF &a, const OwnF &oa, const NodeF &b, double fx, double fy, double fz)
{
    const double half_ewt = fast_sqrt_pos(fmax(fx * fx + fy * fy + fz * fz, 1e-300));       // :27, the plan stores f = -+0.5 e
    const double factor = (half_ewt * double(0.2f)) * (a.sc + b.sc);                          // MINUS the factor of :130-131
    const double fva = fx * a.vx + fy * a.vy + fz * a.vz;
    const double fvb = fx * b.vx + fy * b.vy + fz * b.vz;
    const double da = a.rho * fva, db = b.rho * fvb;
    const double bmx = b.rho * b.vx, bmy = b.rho * b.vy, bmz = b.rho * b.vz;
    const double ps = a.p + b.p;
    Flux5 g;
    g.d = factor * (a.rho - b.rho) - (da + db);
    g.mx = factor * (oa.mx - bmx) - a.vx * da - b.vx * db - ps * fx;
    g.my = factor * (oa.my - bmy) - a.vy * da - b.vy * db - ps * fy;
    g.mz = factor * (oa.mz - bmz) - a.vz * da - b.vz * db - ps * fz;
    g.en = factor * (a.en - b.en) - oa.H * fva - (b.en + b.p) * fvb;
    return g;
}

__device__ __forceinline__ FluxC flux_contribution_f(const NodeF &q, const OwnF &o)
{
    FluxC f;
    f.xx = q.vx * o.mx + q.p;
    f.xy = q.vx * o.my;
    f.xz = q.vx * o.mz;
    f.yy = q.vy * o.my + q.p;
    f.yz = q.vy * o.mz;
    f.zz = q.vz * o.mz + q.p;
    f.ex = q.vx * o.H;
    f.ey = q.vy * o.H;
    f.ez = q.vz * o.H;
    return f;
}

__device__ __forceinline__ void lds_add(double *p, double v) { unsafeAtomicAdd(p, v); }    // ds_add_f64

// CAP: nodes a tile may stage.  kFreeCap4 (halos of at most 290 nodes) lets four workgroups share a CU, kTileCap three.
constexpr int kFreeCap4 = 546;
static_assert(kFreeCap4 - kTile == kFreeCap4Halo, "preprocess.hpp: kFreeCap4Halo");
// LONG: some slice of the level holds more half rows than the prologue requests (the loop behind the unrolled pairs exists)
// WIDE: some tile's halo exceeds the shared table's 303 ids: the halo comes from the kernel's own table, two ids per thread
//       (tile_halo then points at it, stride kFreeHaloStride; CAP = kTile + kFreeHaloStride)
// ROLE (fused stages, round 4): -1 = the generic epilogue (finish_node: every optional path behind a run-time test, the
// step-factor partials reduced before anything else is requested); 0 ... 3 = k_flux_tile's role specialisation — 0 the first
// stage (finishes compute_step_factor: the partials are requested with the prologue and reduced under the staging barrier; the
// sweep's start state IS this stage's input, nothing of it is loaded twice), 1 a middle stage, 2 the last stage (residual or
// its squares), 3 the last stage that also leaves the next sweep's step-factor minima — with the time_step operands requested
// right behind the staging barrier, so that they arrive while the half rows are evaluated.
template <bool FUSE, bool ACC, int CAP, bool LONG, bool WIDE = false, int ROLE = -1>
__global__ void __launch_bounds__(kBlock, CAP <= kFreeCap4 ? 4 : 3)
k_flux_free(// (the first 16 dwords are preloaded into SGPRs: what the prologue's first loads need)
            const double *__restrict__ q, const int32_t *__restrict__ tile_halo, uint32_t n_tiles, int32_t hr_pad_row,
            int64_t stride, int64_t nel, const int32_t *__restrict__ hr_row0, const uint32_t *__restrict__ hr_code,
            const double *__restrict__ hr_w, const int32_t *__restrict__ slice_row0,
            const int32_t *__restrict__ rows_int, const int32_t *__restrict__ rows_bnd,
            const uint16_t *__restrict__ nbr16, const double *__restrict__ w, FarField ff, double *__restrict__ fluxes,
            int classes, FusedStep fs)
{
    __shared__ double2 tile[CAP * kFreeRecD2];
    __shared__ double scs[CAP];
    __shared__ double acc[5 * kTile];               // the sums neighbours leave for this tile's own nodes, [field][node]

    PH_BEGIN();
    constexpr bool SPEC = FUSE && ROLE >= 0;
    static_assert(ROLE < 0 || FUSE, "roles belong to the fused stages");
    double min_dt = 0.0;
    if (FUSE && !SPEC && fs.partial_min) min_dt = block_min_of_partials(fs.partial_min, fs.n_partial);
    constexpr int kPartPre = 6;                     // step-factor partials per thread held in registers (1,536 tiles)
    __shared__ double s_pm[kBlock / 64];
    double pmv[kPartPre];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const unsigned t = xcd_contiguous_block(blockIdx.x, n_tiles);
    const int64_t i = int64_t(t) * kTile + tid;
    const int32_t slice = __builtin_amdgcn_readfirstlane(static_cast<int32_t>(i >> 6));

    // load issue order as in k_flux_tile: halo ids, own state, the first two half rows, then the halo state by id;
    // nothing under a branch
    const int32_t *hrow = tile_halo + int64_t(t) * (WIDE ? kFreeHaloStride : kHaloStride);
    const int32_t hid = hrow[tid];
    const int32_t hid2 = (WIDE || tid < kHaloStride - kBlock) ? hrow[kBlock + tid] : -1;
    const int32_t h0 = hr_row0[slice];
    const int32_t n_h = (classes & 1) ? hr_row0[slice + 1] - h0 : 0;
    const int32_t n_bnd = rows_bnd[slice];
#ifdef MGCFD_ABL_FREE_OWN_AOS          /* diagnostic: the own node read as one 40-byte record, lanes 40 bytes apart (results wrong) */
    const double2 oa_ = *reinterpret_cast<const double2 *>(q + 5 * i), ob_ = *reinterpret_cast<const double2 *>(q + 5 * i + 2);
    const double o0 = oa_.x, o1 = oa_.y, o2 = ob_.x, o3 = ob_.y, o4 = q[5 * i + 4];
#else
    const double o0 = MGCFD_LD_STATE(q + i), o1 = MGCFD_LD_STATE(q + stride + i), o2 = MGCFD_LD_STATE(q + 2 * stride + i),
                 o3 = MGCFD_LD_STATE(q + 3 * stride + i), o4 = MGCFD_LD_STATE(q + 4 * stride + i);
#endif
    // EVERY half row of the lane is requested here (the plan gives a lane at most kHalfMaxRows): the row loop then waits for
    // nothing, and a workgroup has all of its tile's bytes in flight at once — what hides the memory latency is the other
    // workgroups of the CU, not a prefetch distance
    EdgeRow er[kHalfMaxRows];
    // (round 4: the halo state is requested behind the first TWO half rows and ahead of the others, so the records can be
    //  staged while the last three half rows are still on their way: 14.7 -> 14.1 us; 0, 1, 3 and 5 rows first: 14.3, 14.2,
    //  14.5, 14.7 us, profiles/r4_flux_levers.txt)
#ifdef MGCFD_EXP_FREE_ORDER
    constexpr int kRowsFirst = MGCFD_EXP_FREE_ORDER;
#else
    constexpr int kRowsFirst = 2;
#endif
#pragma unroll
    for (int j = 0; j < kRowsFirst; j++) er[j] = load_half_row(hr_code, hr_w, j < n_h ? h0 + j : hr_pad_row, lane);
    const int64_t hnode = hid >= 0 ? int64_t(hid) : i;
#if defined(MGCFD_ABL_FREE_HALO) && MGCFD_ABL_FREE_HALO == 1      /* diagnostic: the halo node read as ONE 40-byte record (results wrong) */
    const double2 ga_ = *reinterpret_cast<const double2 *>(q + 5 * hnode), gb_ = *reinterpret_cast<const double2 *>(q + 5 * hnode + 2);
    const double g0 = ga_.x, g1 = ga_.y, g2 = gb_.x, g3 = gb_.y, g4 = q[5 * hnode + 4];
#elif defined(MGCFD_ABL_FREE_HALO) && MGCFD_ABL_FREE_HALO == 2    /* diagnostic: ... as a 64-byte aligned record (results wrong) */
    const double2 ga_ = *reinterpret_cast<const double2 *>(q + 8 * (hnode >> 1)), gb_ = *reinterpret_cast<const double2 *>(q + 8 * (hnode >> 1) + 2);
    const double g0 = ga_.x, g1 = ga_.y, g2 = gb_.x, g3 = gb_.y, g4 = q[8 * (hnode >> 1) + 4];
#elif defined(MGCFD_ABL_FREE_HALO) && MGCFD_ABL_FREE_HALO == 3    /* diagnostic: no gather, the own node again (results wrong) */
    const double g0 = q[i], g1 = q[stride + i], g2 = q[2 * stride + i], g3 = q[3 * stride + i], g4 = q[4 * stride + i];
#elif defined(MGCFD_ABL_FREE_HALO) && MGCFD_ABL_FREE_HALO == 4    /* diagnostic: nothing loaded for the halo at all (results wrong) */
    const double g0 = o0 + double(hnode), g1 = o1, g2 = o2, g3 = o3, g4 = o4;
#else
    const double g0 = MGCFD_LD_STATE(q + hnode), g1 = MGCFD_LD_STATE(q + stride + hnode), g2 = MGCFD_LD_STATE(q + 2 * stride + hnode),
                 g3 = MGCFD_LD_STATE(q + 3 * stride + hnode), g4 = MGCFD_LD_STATE(q + 4 * stride + hnode);
#endif
#pragma unroll
    for (int j = kRowsFirst; j < kHalfMaxRows; j++) er[j] = load_half_row(hr_code, hr_w, j < n_h ? h0 + j : hr_pad_row, lane);
    // (WIDE: the second halo node of every thread as unconditionally as the first)
    const int64_t hnode2 = (WIDE && hid2 >= 0) ? int64_t(hid2) : i;
    double u0 = 0.0, u1 = 0.0, u2 = 0.0, u3 = 0.0, u4 = 0.0;
    if (WIDE) { u0 = q[hnode2]; u1 = q[stride + hnode2]; u2 = q[2 * stride + hnode2]; u3 = q[3 * stride + hnode2]; u4 = q[4 * stride + hnode2]; }

    if (SPEC && ROLE == 0) {                        // (requested last: wanted only at the staging barrier)
#pragma unroll
        for (int u = 0; u < kPartPre; u++) {
            const int k = threadIdx.x + u * kBlock;
            pmv[u] = fs.partial_min[k < fs.n_partial ? k : fs.n_partial - 1];     // clamped: a repeat does not change a minimum
        }
    }
#pragma unroll
    for (int f = 0; f < 5; f++) acc[f * kTile + tid] = 0.0;
    const NodeF me = make_nodef(o0, o1, o2, o3, o4);
    lds_store_nodef(tile, scs, uint32_t(tid), me);
    lds_store_nodef(tile, scs, uint32_t(kTile + tid), make_nodef(g0, g1, g2, g3, g4));          // unconditional, see k_flux_tile
    if (WIDE) lds_store_nodef(tile, scs, uint32_t(kTile + kBlock + tid), make_nodef(u0, u1, u2, u3, u4));
    else if (hid2 >= 0) {
        const int64_t h = hid2;
        lds_store_nodef(tile, scs, uint32_t(kTile + kBlock + tid), make_nodef(q[h], q[stride + h], q[2 * stride + h], q[3 * stride + h], q[4 * stride + h]));
    }
    const OwnF mo = make_ownf(me);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
    if (ACC) {
        a0 = fluxes[i]; a1 = fluxes[stride + i]; a2 = fluxes[2 * stride + i];
        a3 = fluxes[3 * stride + i]; a4 = fluxes[4 * stride + i];
    }
    if (SPEC && ROLE == 0) {
        double pm = pmv[0];
#pragma unroll
        for (int u = 1; u < kPartPre; u++) pm = fmin(pm, pmv[u]);
        for (int k = threadIdx.x + kPartPre * kBlock; k < fs.n_partial; k += kBlock) pm = fmin(pm, fs.partial_min[k]);
        pm = wave_min(pm);
        if (lane == 0) s_pm[tid >> 6] = pm;
    }
    PH_MARK(0);
    __syncthreads();
    PH_MARK(1);
    // role-specialised stages: the time_step operands go out behind the first pair of half rows (whose registers they take)
    // and arrive under the others
    double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0, r4 = 0.0, sfv = 0.0;
    auto request_operands = [&](int part) {        // part 0 behind the first pair, part 1 behind the second (the register budget of four waves per SIMD)
        if (ROLE == 0) {
            // the first stage's input IS the sweep's start state (the launcher checks q == old_variables): rho and E are in the
            // node's record, the momenta are rho v again (this kernel's results are not the reference's bits anyway)
            if (part == 0) { r0 = me.rho; r1 = mo.mx; r2 = mo.my; r3 = mo.mz; r4 = me.en; sfv = fs.volumes[i]; }
        } else if (part == 0) {
            r0 = fs.old_variables[i]; r1 = fs.old_variables[stride + i]; r2 = fs.old_variables[2 * stride + i];
            r3 = fs.old_variables[3 * stride + i];
        } else {
            r4 = fs.old_variables[4 * stride + i];
            sfv = fs.step_factors[i];
        }
    };
    if (SPEC && n_h <= 0) request_operands(0);      // (uniform over the wave: a slice without half rows)
    if (SPEC && n_h <= 2) request_operands(1);

    // ---- this lane's half rows, two at a time (independent arithmetic; a half row the slice does not have was read from the
    //      padding row: zero weights, nothing added) ----
    auto eval = [&](const EdgeRow &e0, bool may_be_foreign) {
        const uint32_t s = e0.code & kT16SlotMask;
        const bool v = s != kT16Pad;
        const NodeF ot = lds_load_nodef(tile, scs, v ? s : uint32_t(tid));
        Flux5 G;                                    // MINUS the edge's flux as its evaluating end sees it
        bool mine = true;
        if (may_be_foreign) {
            // an evaluation another node owns (the plan found no room in that node's lane): its record comes from LDS too,
            // and its share goes to its LDS sum
            const bool foreign = (e0.code & kHalfForeign) != 0;
            const uint32_t own = (e0.code >> 16) & 0xFFu;
            const NodeF m0 = foreign ? lds_load_nodef(tile, scs, own) : me;
            G = edge_flux_neg_f(m0, make_ownf(m0), ot, e0.fx, e0.fy, e0.fz);
            if (foreign && v) {
                lds_add(&acc[own], -G.d); lds_add(&acc[kTile + own], -G.mx); lds_add(&acc[2 * kTile + own], -G.my);
                lds_add(&acc[3 * kTile + own], -G.mz); lds_add(&acc[4 * kTile + own], -G.en);
            }
            mine = !foreign;
        } else {
            G = edge_flux_neg_f(me, mo, ot, e0.fx, e0.fy, e0.fz);
        }
        // (padding: G = 0)
        if (mine) { a0 -= G.d; a1 -= G.mx; a2 -= G.my; a3 -= G.mz; a4 -= G.en; }
        if (v && (e0.code & kHalfMirror)) {
            // the other end lies in this tile and does not evaluate the edge itself: it gets -F
            lds_add(&acc[s], G.d); lds_add(&acc[kTile + s], G.mx); lds_add(&acc[2 * kTile + s], G.my);
            lds_add(&acc[3 * kTile + s], G.mz); lds_add(&acc[4 * kTile + s], G.en);
        }
    };
#pragma unroll
    for (int j = 0; j < kHalfMaxRows; j += 2) {
        if (j >= n_h) break;                        // (uniform over the wave)
        const bool two = j + 1 < kHalfMaxRows;      // (compile time)
        const bool any_foreign = ((er[j].code | (two ? er[j + 1 < kHalfMaxRows ? j + 1 : j].code : 0u)) & kHalfForeign) != 0;
        if (__builtin_expect(__any(any_foreign), 0)) {
            eval(er[j], true);
            if (two) eval(er[j + 1 < kHalfMaxRows ? j + 1 : j], true);
        } else {
            eval(er[j], false);
            if (two) eval(er[j + 1 < kHalfMaxRows ? j + 1 : j], false);
        }
        if (SPEC && j == 0) request_operands(0);
        if (SPEC && j == 2) request_operands(1);
    }
    // a slice with more half rows than the prologue requests (tetrahedral regions, hubs: the plan spreads a high-degree node's
    // evaluations over the tile's lanes, preprocess.hpp kFreeMaxRows): the rest one at a time, two in flight
    if (LONG && n_h > kHalfMaxRows) {               // (uniform over the wave)
        EdgeRow x0 = load_half_row(hr_code, hr_w, h0 + kHalfMaxRows, lane);
        EdgeRow x1 = load_half_row(hr_code, hr_w, kHalfMaxRows + 1 < n_h ? h0 + kHalfMaxRows + 1 : hr_pad_row, lane);
        for (int32_t j = kHalfMaxRows; j < n_h; j++) {
            const EdgeRow x2 = load_half_row(hr_code, hr_w, j + 2 < n_h ? h0 + j + 2 : hr_pad_row, lane);
            if (__any((x0.code & kHalfForeign) != 0)) eval(x0, true);
            else eval(x0, false);
            x0 = x1; x1 = x2;
        }
    }
    PH_MARK(2);
    __syncthreads();
    PH_MARK(3);
    a0 += acc[tid]; a1 += acc[kTile + tid]; a2 += acc[2 * kTile + tid]; a3 += acc[3 * kTile + tid]; a4 += acc[4 * kTile + tid];

    if ((classes & 6) && n_bnd > 0) {
        const int32_t row0 = slice_row0[slice];
        const int64_t first_bnd = int64_t(row0) + rows_int[slice];
        const FluxC fm = flux_contribution_f(me, mo);
        for (int32_t r = 0; r < n_bnd; r++) {
            const EdgeRow e = load_row<false>(nbr16, w, first_bnd + r, lane);
            const double fx = e.fx, fy = e.fy, fz = e.fz;
            if (e.code == kT16Wall && (classes & 2)) {
                // flux_boundary_kernel.elemfunc.c:37-64: pressure force only
                a1 += fx * me.p;
                a2 += fy * me.p;
                a3 += fz * me.p;
            } else if (e.code == kT16Far && (classes & 4)) {
                // flux_wall_kernel.elemfunc.c:51-88: average with the far-field state
                a0 += fx * (ff.var[1] + mo.mx) + fy * (ff.var[2] + mo.my) + fz * (ff.var[3] + mo.mz);
                a4 += fx * (ff.fc_de[0] + fm.ex) + fy * (ff.fc_de[1] + fm.ey) + fz * (ff.fc_de[2] + fm.ez);
                a1 += fx * (ff.fc_mx[0] + fm.xx) + fy * (ff.fc_mx[1] + fm.xy) + fz * (ff.fc_mx[2] + fm.xz);
                a2 += fx * (ff.fc_my[0] + fm.xy) + fy * (ff.fc_my[1] + fm.yy) + fz * (ff.fc_my[2] + fm.yz);
                a3 += fx * (ff.fc_mz[0] + fm.xz) + fy * (ff.fc_mz[1] + fm.yz) + fz * (ff.fc_mz[2] + fm.zz);
            }
        }
    }
    if (!SPEC) {
        finish_node<FUSE>(i, nel, stride, a0, a1, a2, a3, a4, fluxes, fs, min_dt, t);
        PH_MARK(4);
        return;
    }
    // ---- fused time_step, role-specialised (k_flux_tile's epilogue: the same operations as k_time_step, cfd_loops.cpp:241-268) ----
    double sf_next = __longlong_as_double(0x7FF0000000000000LL);          // +inf: lanes past nel
    double ss = 0.0;                                                      // this node's share of the residual sum of squares
    if (i < nel) {
        double sf = sfv;
        if (ROLE == 0) {                            // finish compute_step_factor (cfd_loops.cpp:137-156)
            min_dt = s_pm[0];
            for (int wv = 1; wv < kBlock / 64; wv++) min_dt = fmin(min_dt, s_pm[wv]);
            sf = min_dt / sfv;                      // sfv holds the volume
            MGCFD_ST_STAGE(fs.step_factors + i, sf);
        }
        const double factor = sf / fs.rk_div;
        const double rho = r0 + factor * a0, mx = r1 + factor * a1, my = r2 + factor * a2, mz = r3 + factor * a3,
                     en = r4 + factor * a4;
        store_conserved(fs.q_out, stride, i, rho, mx, my, mz, en);
        if (ROLE >= 2) {                            // last stage: residual (validation.cpp:77-89)
            const double d0 = rho - r0, d1 = mx - r1, d2 = my - r2, d3 = mz - r3, d4 = en - r4;
            if (fs.residuals) {                      // (null: the caller writes it on demand, solver.cpp settle_residuals)
                MGCFD_ST_STAGE(fs.residuals + i, d0); MGCFD_ST_STAGE(fs.residuals + stride + i, d1); MGCFD_ST_STAGE(fs.residuals + 2 * stride + i, d2);
                MGCFD_ST_STAGE(fs.residuals + 3 * stride + i, d3); MGCFD_ST_STAGE(fs.residuals + 4 * stride + i, d4);
            }
            if (fs.sumsq_partial) ss = (((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3) + d4 * d4;
        }
        if (fs.check) {
            const bool finite = isfinite(rho) && isfinite(mx) && isfinite(my) && isfinite(mz) && isfinite(en);
            int code = 0;
            if (!finite) code = 1;
            else if (rho < 0.0) code = 2;
            else if (en < 0.0) code = 3;
            if (code) atomicMin(fs.err, err_key(fs.check, fs.old_of_new[i], code));
        }
        if (ROLE == 3) {                            // look-ahead: the next sweep's compute_step_factor starts from the state just produced
            const Derived d = derive(rho, mx, my, mz, en);
            const double dt = fs.cbrt_vol[i] / (d.speed + d.c);          // k_step_factor_local
            sf_next = fs.cfl * dt;
        }
    }
    if (ROLE == 3 || (ROLE == 2 && fs.sumsq_partial)) {                // uniform: every thread of the workgroup takes part
        __shared__ double s_next[2][kBlock / 64];
        if (ROLE == 3) sf_next = wave_min(sf_next);
        if (fs.sumsq_partial) ss = wave_sum(ss);
        if ((threadIdx.x & 63) == 0) { s_next[0][threadIdx.x >> 6] = sf_next; s_next[1][threadIdx.x >> 6] = ss; }
        __syncthreads();
        if (threadIdx.x == 0) {
            double m = s_next[0][0], sum = s_next[1][0];
            for (int wv = 1; wv < kBlock / 64; wv++) { m = fmin(m, s_next[0][wv]); sum += s_next[1][wv]; }
            if (ROLE == 3) fs.next_partial_min[t] = m;
            if (fs.sumsq_partial) fs.sumsq_partial[t] = sum;
        }
    }
    PH_MARK(4);
}

// Diagnostic (mgcfd_diag_fast_math): one of the approximations above per element, as this build compiles it for the flux kernel.
// kind 0: fast_rcp, 1: fast_sqrt, 2: fast_sqrt_pos.
__global__ void __launch_bounds__(kBlock)
k_diag_fast_math(int kind, int64_t n, const double *__restrict__ in, double *__restrict__ out)
{
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    const double x = in[i];
    out[i] = kind == 0 ? fast_rcp(x) : (kind == 1 ? fast_sqrt(x) : fast_sqrt_pos(x));
}
#endif // MGCFD_ORDER_FREE

// ------------------------------------------------------------------------------------------
// Two-phase ("fission") design point, MGCFD_OPT_FLUX_VARIANT bit 2 — the GPU form of the
// reference's FLUX_FISSION build (flux_kernel.elemfunc.c:193-204 + update_edges,
// cfd_loops.cpp:159-213): phase 1 evaluates every internal edge once, edge-parallel, and writes its
// five fluxes to memory; phase 2 is a node-centred sum of each node's incident edges in row order
// (+F at the a end, -F at the b end) followed by the boundary rows.  Bit-identical to the other
// variants; kept to put a number on the scatter-strategy choice.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_fission_edge_flux(int64_t n_edges, int64_t n_edges_pad, int64_t stride, const double *__restrict__ q,
                    const int32_t *__restrict__ fe_ab, const double *__restrict__ fe_w, double *__restrict__ eflux)
{
    const int64_t e = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (e >= n_edges) return;
    const int64_t a = fe_ab[e], b = fe_ab[n_edges + e];
    EdgeRow er;
    er.code = 0;                                                     // a-side form
    er.fx = fe_w[e]; er.fy = fe_w[n_edges + e]; er.fz = fe_w[2 * n_edges + e]; er.k = fe_w[3 * n_edges + e];
    const NodeQ A = load_and_derive(q, stride, a), B = load_and_derive(q, stride, b);
    const Flux5 f = edge_flux<true>(A, flux_contribution(A), B, er);
    eflux[e] = f.d; eflux[n_edges_pad + e] = f.mx; eflux[2 * n_edges_pad + e] = f.my;
    eflux[3 * n_edges_pad + e] = f.mz; eflux[4 * n_edges_pad + e] = f.en;
}

template <bool ACC>
__global__ void __launch_bounds__(kBlock)
k_fission_node_sum(int64_t nel, int64_t stride, int64_t n_edges_pad, const double *__restrict__ q,
                   const int32_t *__restrict__ slice_row0, const int32_t *__restrict__ rows_int,
                   const int32_t *__restrict__ rows_bnd, const int32_t *__restrict__ row_edge,
                   const uint16_t *__restrict__ nbr16, const double *__restrict__ w,
                   const double *__restrict__ eflux, FarField ff, double *__restrict__ fluxes, int classes)
{
    const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
    const int64_t i = blk * int64_t(kBlock) + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t slice = __builtin_amdgcn_readfirstlane(static_cast<int32_t>(i >> 6));
    const int32_t row0 = slice_row0[slice];
    const int32_t n_int = rows_int[slice];
    const int32_t n_bnd = rows_bnd[slice];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
    if (ACC) {
        a0 = fluxes[i]; a1 = fluxes[stride + i]; a2 = fluxes[2 * stride + i];
        a3 = fluxes[3 * stride + i]; a4 = fluxes[4 * stride + i];
    }
    if (classes & 1) {
        const int32_t *re = row_edge + (int64_t(row0) << 6) + lane;
        for (int32_t r = 0; r < n_int; r++) {
            const int32_t code = re[int64_t(r) << 6];
            if (code == -1) continue;                                // ELL padding
            const int64_t e = code & 0x7FFFFFFF;
            const double f0 = eflux[e], f1 = eflux[n_edges_pad + e], f2 = eflux[2 * n_edges_pad + e],
                         f3 = eflux[3 * n_edges_pad + e], f4 = eflux[4 * n_edges_pad + e];
            if (code < 0) { a0 -= f0; a1 -= f1; a2 -= f2; a3 -= f3; a4 -= f4; }      // this node is the b end
            else { a0 += f0; a1 += f1; a2 += f2; a3 += f3; a4 += f4; }
        }
    }
    if ((classes & 6) && n_bnd > 0) {
        const NodeQ me = load_and_derive(q, stride, i);
        boundary_rows(me, flux_contribution(me), ff, nbr16, w, int64_t(row0) + n_int, n_bnd, lane, classes, a0, a1, a2, a3, a4);
    }
    if (i < nel) {
        fluxes[i] = a0; fluxes[stride + i] = a1; fluxes[2 * stride + i] = a2;
        fluxes[3 * stride + i] = a3; fluxes[4 * stride + i] = a4;
    }
}

// ------------------------------------------------------------------------------------------
// indirect_rw (indirect_rw_kernel.elemfunc.c:4-94) in gather form: the reference's "same data
// movement, minimal arithmetic" probe.  a-side gets q_b + (ex, ez, 0, 0, ey); b-side gets q_a.
// The plan stores -0.5*e (a side), so e = -2*w exactly.  Neighbour state straight from HBM/L2.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_indirect_rw(int64_t nel, int64_t stride, const double *__restrict__ q, const int32_t *__restrict__ slice_row0,
              const int32_t *__restrict__ rows_int, const int32_t *__restrict__ nbr,
              const double *__restrict__ w, double *__restrict__ fluxes)
{
    const unsigned blk = xcd_contiguous_block(blockIdx.x, gridDim.x);
    const int64_t i = blk * int64_t(kBlock) + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t slice = __builtin_amdgcn_readfirstlane(static_cast<int32_t>(i >> 6));
    const int32_t row0 = slice_row0[slice];
    const int32_t n_int = rows_int[slice];
    double a0 = fluxes[i], a1 = fluxes[stride + i], a2 = fluxes[2 * stride + i],
           a3 = fluxes[3 * stride + i], a4 = fluxes[4 * stride + i];
    for (int32_t r = 0; r < n_int; r++) {
        const int64_t row = int64_t(row0) + r;
        const int32_t code = nbr[(row << 6) + lane];
        if (code < 0) continue;
        const int64_t j = code & kIdMask;
        const double o0 = q[j], o1 = q[stride + j], o2 = q[2 * stride + j], o3 = q[3 * stride + j], o4 = q[4 * stride + j];
        if (code & kRoleB) {
            a0 += o0; a1 += o1; a2 += o2; a3 += o3; a4 += o4;
        } else {
            const double *wr = w + (row << 8) + lane;
            a0 += o0 + (-2.0 * wr[0]);
            a1 += o1 + (-2.0 * wr[128]);
            a2 += o2;
            a3 += o3;
            a4 += o4 + (-2.0 * wr[64]);
        }
    }
    if (i < nel) {
        fluxes[i] = a0; fluxes[stride + i] = a1; fluxes[2 * stride + i] = a2;
        fluxes[3 * stride + i] = a3; fluxes[4 * stride + i] = a4;
    }
}

// ------------------------------------------------------------------------------------------
// indirect_rw through the LDS tiles: the probe the reference keeps to bound compute_flux_edge from above
// (indirect_rw_loop.cpp:8-10, "same data movement, minimal arithmetic").  Here "same data movement" means the flux
// kernel's own: the same prologue (halo ids, own and halo state into 96-byte LDS records — the derived fields filled
// with copies, nothing is derived), the same incidence rows two at a time with the same prefetch, every byte the
// flux kernel loads is loaded (weights of both roles and the length factor included; an empty asm consumes what the
// probe's arithmetic does not use), the same stores.  Arithmetic: indirect_rw_kernel.elemfunc.c:41-55 in gather form.
// Levels whose tiles leave halo nodes outside LDS or have long rows use k_indirect_rw above.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void keep_alive(double x) { asm volatile("" ::"v"(x)); }

template <bool LOADK>
__global__ void __launch_bounds__(kBlock, 3)
k_indirect_rw_tile(const double *__restrict__ q, const int32_t *__restrict__ tile_halo, uint32_t n_tiles, int32_t pad_row,
                   int64_t stride, int64_t nel, const int32_t *__restrict__ slice_row0, const int32_t *__restrict__ rows_int,
                   const uint16_t *__restrict__ nbr16, const double *__restrict__ w, double *__restrict__ fluxes)
{
    __shared__ double2 tile[kTileCap * kLdsRecD2];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const unsigned t = xcd_contiguous_block(blockIdx.x, n_tiles);
    const int64_t i = int64_t(t) * kTile + tid;
    const int32_t slice = __builtin_amdgcn_readfirstlane(static_cast<int32_t>(i >> 6));
    const int32_t *hrow = tile_halo + int64_t(t) * kHaloStride;
    const int32_t hid = hrow[tid];
    const int32_t hid2 = tid < kHaloStride - kBlock ? hrow[kBlock + tid] : -1;
    const int32_t row0 = slice_row0[slice];
    const int32_t n_int = rows_int[slice];
#if defined(MGCFD_ABL_NO_HALO)      /* diagnostic: the halo state not gathered: the dependent ids -> state chain is gone (results wrong) */
    const int64_t hnode = hid >= 0 ? i : i;
#elif defined(MGCFD_ABL_HALO_COALESCED)   /* diagnostic: the chain ids -> state kept, but the gather made contiguous (results wrong) */
    const int64_t hnode = hid >= 0 ? ((int64_t(__builtin_amdgcn_readfirstlane(hid)) & ~int64_t(255)) + tid) : i;
#else
    const int64_t hnode = hid >= 0 ? int64_t(hid) : i;
#endif
    const double o0 = q[i], o1 = q[stride + i], o2 = q[2 * stride + i], o3 = q[3 * stride + i], o4 = q[4 * stride + i];
    const double g0 = q[hnode], g1 = q[stride + hnode], g2 = q[2 * stride + hnode], g3 = q[3 * stride + hnode], g4 = q[4 * stride + hnode];
    EdgeRow e0 = load_row<LOADK>(nbr16, w, n_int > 0 ? row0 : pad_row, lane);
    EdgeRow e1 = load_row<LOADK>(nbr16, w, n_int > 1 ? row0 + 1 : pad_row, lane);
    auto record = [](double r, double mx, double my, double mz, double en) {
        NodeQ n;
        n.rho = r; n.mx = mx; n.my = my; n.mz = mz; n.en = en;
        n.vx = r; n.vy = mx; n.vz = my; n.p = mz; n.speed = en; n.c = r;      // (copies: the record keeps its 96 bytes)
        return n;
    };
    lds_store_record(tile, uint32_t(tid), record(o0, o1, o2, o3, o4));
    lds_store_record(tile, uint32_t(kTile + tid), record(g0, g1, g2, g3, g4));
    if (hid2 >= 0) {
        const int64_t h = hid2;
        lds_store_record(tile, uint32_t(kTile + kBlock + tid), record(q[h], q[stride + h], q[2 * stride + h], q[3 * stride + h], q[4 * stride + h]));
    }
    // fluxes += ... (indirect_rw_kernel.elemfunc.c:84-94)
    double a0 = fluxes[i], a1 = fluxes[stride + i], a2 = fluxes[2 * stride + i], a3 = fluxes[3 * stride + i], a4 = fluxes[4 * stride + i];
    __syncthreads();
    auto entry = [&](const EdgeRow &e) {
        const uint32_t s = e.code & kT16SlotMask;
        const bool v = s != kT16Pad;
#if defined(MGCFD_ABL_LDS_OWN)      /* diagnostic: every lane reads its own record: no bank conflicts (results wrong) */
        const NodeQ n = lds_load_record(tile, uint32_t(tid));
#else
        const NodeQ n = lds_load_record(tile, v ? s : uint32_t(tid));
#endif
        keep_alive(n.vx); keep_alive(n.vy); keep_alive(n.vz); keep_alive(n.p); keep_alive(n.speed); keep_alive(n.c);
        keep_alive(e.fx); keep_alive(e.fy); keep_alive(e.fz);
        if (LOADK) keep_alive(e.k);
        if (!v) return;
        if (e.code & kT16RoleB) {                                  // this node is the edge's b end: += q_a (:50-54)
            a0 += n.rho; a1 += n.mx; a2 += n.my; a3 += n.mz; a4 += n.en;
        } else {                                                    // a end: += q_b + (ex, ez, 0, 0, ey) (:41-45); the plan stores -0.5*e
            a0 += n.rho + (-2.0 * e.fx);
            a1 += n.mx + (-2.0 * e.fz);
            a2 += n.my;
            a3 += n.mz;
            a4 += n.en + (-2.0 * e.fy);
        }
    };
    int32_t r = 0;
    for (; r + 2 < n_int; r += 2) {
        const EdgeRow e2 = load_row<LOADK>(nbr16, w, row0 + r + 2, lane);
        const EdgeRow e3 = load_row<LOADK>(nbr16, w, r + 3 < n_int ? row0 + r + 3 : pad_row, lane);
        entry(e0); entry(e1);
        e0 = e2; e1 = e3;
    }
    if (r < n_int) { entry(e0); entry(e1); }
    if (i < nel) {
        fluxes[i] = a0; fluxes[stride + i] = a1; fluxes[2 * stride + i] = a2;
        fluxes[3 * stride + i] = a3; fluxes[4 * stride + i] = a4;
    }
}

// ------------------------------------------------------------------------------------------
// The end of a node-wise update (k_time_step, k_time_step_src): the new state stored, and on request
//   * residuals != nullptr: last stage — residuals = variables - old_variables (validation.cpp:77-89);
//   * check: raise the check_for_invalid_variables flag (validation.cpp:107-138),
//     err = (smallest offending ORIGINAL cell id << 8) | code.
// q and residuals are not declared restrict: an update in place passes the array it read as q.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void finish_update(double *q, double *residuals, int64_t stride, int64_t i, const double (&r)[5],
                                              double rho, double mx, double my, double mz, double en,
                                              const int32_t *__restrict__ old_of_new, unsigned long long *__restrict__ err, int check)
{
    store_conserved(q, stride, i, rho, mx, my, mz, en);
    if (residuals) {
        residuals[i] = rho - r[0]; residuals[stride + i] = mx - r[1]; residuals[2 * stride + i] = my - r[2];
        residuals[3 * stride + i] = mz - r[3]; residuals[4 * stride + i] = en - r[4];
    }
    if (check) {
        const bool finite = isfinite(rho) && isfinite(mx) && isfinite(my) && isfinite(mz) && isfinite(en);
        int code = 0;
        if (!finite) code = 1;
        else if (rho < 0.0) code = 2;
        else if (en < 0.0) code = 3;
        if (code) atomicMin(err, err_key(check, old_of_new[i], code));
    }
}

// ------------------------------------------------------------------------------------------
// time_step (cfd_loops.cpp:241-268): variables = old + sf/(RK+1-j) * fluxes ; fluxes = 0.
// Fused options (same operations, fewer passes over memory):
//   * partial_min != nullptr: this is the first stage after compute_step_factor's first half —
//     finish it here: min over the workgroups' partial minima, then
//     step_factors[i] = min_dt / volumes[i] (cfd_loops.cpp:137-156);
//   * zero_fluxes == 0: leave fluxes[] stale; the caller treats the array as logically zero and
//     the next flux launch overwrites it (saves the 40 B/node of zero stores);
//   * residuals and check: finish_update.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_time_step(int64_t nel, int64_t stride, double rk_div, double *__restrict__ step_factors,
            double *__restrict__ fluxes, const double *__restrict__ old_variables, double *__restrict__ q,
            const int32_t *__restrict__ old_of_new, unsigned long long *__restrict__ err, int check,
            const double *__restrict__ partial_min, int n_partial, const double *__restrict__ volumes,
            double *__restrict__ residuals, int zero_fluxes)
{
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    double min_dt = 0.0;
    if (partial_min) min_dt = block_min_of_partials(partial_min, n_partial);   // all threads take part
    if (i >= nel) return;
    double sf;
    if (partial_min) {
        sf = min_dt / volumes[i];
        step_factors[i] = sf;
    } else {
        sf = step_factors[i];
    }
    const double factor = sf / rk_div;
    const double r[5] = {old_variables[i], old_variables[stride + i], old_variables[2 * stride + i],
                         old_variables[3 * stride + i], old_variables[4 * stride + i]};
    const double rho = r[0] + factor * fluxes[i];
    const double mx = r[1] + factor * fluxes[stride + i];
    const double my = r[2] + factor * fluxes[2 * stride + i];
    const double mz = r[3] + factor * fluxes[3 * stride + i];
    const double en = r[4] + factor * fluxes[4 * stride + i];
    if (zero_fluxes) {
        fluxes[i] = 0.0; fluxes[stride + i] = 0.0; fluxes[2 * stride + i] = 0.0;
        fluxes[3 * stride + i] = 0.0; fluxes[4 * stride + i] = 0.0;
    }
    finish_update(q, residuals, stride, i, r, rho, mx, my, mz, en, old_of_new, err, check);
}

// ------------------------------------------------------------------------------------------
// Dual time stepping (no reference counterpart; INTEGRATION.md "Dual time stepping"): the physical-time derivative as a
// source in every stage's update, BDF2 (BDF1 on the first physical step) over the state W the stage's fluxes were computed
// from and the two stored time levels Wn, Wn1.  The differences are formed first, so a state equal to both levels gives
// src = +0.0 exactly; one IEEE operation per line of the definition (include/mgcfd.h), never contracted in the exact build.
// ------------------------------------------------------------------------------------------
template <bool BDF2>
__device__ __forceinline__ double dual_source(double w, double wn, double wn1, double vol, double dt)
{
    const double a = w - wn;
    if (!BDF2) return vol * (a / dt);
    const double b = wn - wn1;
    return vol * ((3.0 * a - b) / (2.0 * dt));
}

// time_step with F' in place of F, in the one launch (SRC: 0 no source, 1 BDF1, 2 BDF2; FORCED: FAS multigrid's forcing P, below):
//   F' = F - src          dual time stepping;
//   F' = F + P            a FAS-forced level;
//   F' = (F - src) + P    both: the forcing is the last addition.
// W, Wn, Wn1 (BDF2) and the volume are read beside what k_time_step reads (128 B per node more; BDF1: 88), P likewise (40 B),
// F' exists in registers only, fluxes[] is never written and stays logically zero (the lazy zero of k_time_step), the residual
// and check_for_invalid_variables ride along as there.  The step factors are final (the sweep clamped them: k_dual_clamp).
// In place: W and q are the same array, every lane reads its node before it writes it, so neither pointer is declared restrict.
template <int SRC, bool FORCED>
__global__ void __launch_bounds__(kBlock)
k_time_step_src(int64_t nel, int64_t stride, double rk_div, const double *__restrict__ step_factors,
                const double *__restrict__ fluxes, const double *__restrict__ forcing, const double *old_variables, double *q,
                const int32_t *__restrict__ old_of_new, unsigned long long *__restrict__ err, int check,
                double *residuals, DualSource d)
{
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (i >= nel) return;
    const double factor = step_factors[i] / rk_div;
    const double vol = SRC ? d.volumes[i] : 0.0;
    double fp[5], r[5];
#pragma unroll
    for (int v = 0; v < 5; v++) {
        const int64_t at = v * stride + i;
        double f = fluxes[at];
        if (SRC) f = f - dual_source<SRC == 2>(d.w[at], d.wn[at], SRC == 2 ? d.wn1[at] : 0.0, vol, d.dt);
        if (FORCED) f = f + forcing[at];
        fp[v] = f;
        r[v] = old_variables[at];
    }
    const double rho = r[0] + factor * fp[0];
    const double mx = r[1] + factor * fp[1];
    const double my = r[2] + factor * fp[2];
    const double mz = r[3] + factor * fp[3];
    const double en = r[4] + factor * fp[4];
    finish_update(q, residuals, stride, i, r, rho, mx, my, mz, en, old_of_new, err, check);
}

// ... and with residual smoothing on: fluxes = F - src for every node of the level, before the Jacobi iterations, whose
// first launch forms D = sf * F' for own and halo nodes alike from fluxes[] (k_smooth_tile stays as it is).
template <bool BDF2>
__global__ void __launch_bounds__(kBlock)
k_dual_source(int64_t nel, int64_t stride, double *__restrict__ fluxes, DualSource d)
{
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (i >= nel) return;
    const double vol = d.volumes[i];
#pragma unroll
    for (int v = 0; v < 5; v++) {
        const int64_t at = v * stride + i;
        const double wn1 = BDF2 ? d.wn1[at] : 0.0;
        fluxes[at] = fluxes[at] - dual_source<BDF2>(d.w[at], d.wn[at], wn1, vol, d.dt);
    }
}

// ------------------------------------------------------------------------------------------
// Implicit residual smoothing (no reference counterpart; INTEGRATION.md "Implicit residual smoothing"): one Jacobi
// iteration of (1 + eps*n_i) Db_i - eps * sum_j Db_j = D_i over the internal edges, D_i = step_factor_i * fluxes_i.
//   Db^m_i = (D_i + eps * S_i) / (1 + eps * n_i),   S_i = the sum of Db^(m-1) at the other ends of node i's internal edges,
// started at +0.0 and added one edge at a time in the level's original edge order — the incidence rows' order, so the
// per-node walk is the one k_flux_tile does: a workgroup stages the Db^(m-1) records of its 256 nodes and of their halo in
// LDS, every lane walks its internal rows through nbr16 (a halo node beyond the table: from the overflow list in memory),
// then — long rows — its entries of the workgroup's list, which follow the loop rows in row order (preprocess.cpp).
//   FIRST: Db^0 = D is formed from fluxes and step_factors while it is staged (own and halo nodes alike).
//   LAST:  time_step with Db^M in place of step_factor * fluxes: variables = old + Db^M / (RK+1-j), the residual on
//          request and check_for_invalid_variables, as k_time_step carries them.  fluxes[] is left as it is (the
//          solver treats it as logically zero, as after a lazy time_step): with FIRST && LAST other tiles still read it.
// LDS: five fields of 560 doubles (22,400 B; one field per instruction, a slot's doubles 8 B apart: lanes that read
// consecutive slots hit consecutive bank pairs — the 40-byte record of the state arrays would put two lanes in five on
// the same pair).  44-56 registers, no scratch; seven workgroups per CU by LDS (the launch bound asks for six at least):
// nothing here waits on arithmetic, so the loads in flight are what matters.
// ------------------------------------------------------------------------------------------
template <bool FIRST, bool LAST, bool TAIL>
__global__ void __launch_bounds__(kBlock, 6)
k_smooth_tile(const int32_t *__restrict__ tile_halo, uint32_t n_tiles, int64_t stride, int64_t nel,
              const int32_t *__restrict__ slice_row0, const int32_t *__restrict__ rows_int, const uint16_t *__restrict__ nbr16,
              const int32_t *__restrict__ tile_ovf_ptr, const int32_t *__restrict__ tile_ovf, TailPlan tp, SmoothStep a)
{
    __shared__ double rec[5][kSmoothRow];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const unsigned t = xcd_contiguous_block(blockIdx.x, n_tiles);
    const int64_t i = int64_t(t) * kTile + tid;
    const int32_t slice = __builtin_amdgcn_readfirstlane(static_cast<int32_t>(i >> 6));
    const int32_t *hrow = tile_halo + int64_t(t) * kHaloStride;
    const int32_t hid = hrow[tid];
    const int32_t hid2 = tid < kHaloStride - kBlock ? hrow[kBlock + tid] : -1;
    const int32_t row0 = slice_row0[slice];
    const int32_t n_int = (TAIL ? tp.rows_main : rows_int)[slice];
    const int32_t ovf0 = tile_ovf_ptr[t];
    const int64_t hnode = hid >= 0 ? int64_t(hid) : i;                 // (no halo node: a copy of the own one in the unused slot)
    // Db^(m-1) of node n: the previous iteration's record, or (FIRST) D = step_factor * fluxes, one multiplication
    auto previous = [&](int64_t n, double &v0, double &v1, double &v2, double &v3, double &v4) {
        if (FIRST) {
            const double sf = a.step_factors[n];
            v0 = sf * a.fluxes[n]; v1 = sf * a.fluxes[stride + n]; v2 = sf * a.fluxes[2 * stride + n];
            v3 = sf * a.fluxes[3 * stride + n]; v4 = sf * a.fluxes[4 * stride + n];
        } else {
            v0 = a.prev[n]; v1 = a.prev[stride + n]; v2 = a.prev[2 * stride + n]; v3 = a.prev[3 * stride + n]; v4 = a.prev[4 * stride + n];
        }
    };
    auto stage = [&](uint32_t slot, int64_t n) {
        double v0, v1, v2, v3, v4;
        previous(n, v0, v1, v2, v3, v4);
        rec[0][slot] = v0; rec[1][slot] = v1; rec[2][slot] = v2; rec[3][slot] = v3; rec[4][slot] = v4;
    };
    uint32_t c = nbr16[(int64_t(n_int > 0 ? row0 : 0) << 6) + lane];   // (row 0 exists on every level; unused when n_int == 0)
    stage(uint32_t(tid), i);
    stage(uint32_t(kTile + tid), hnode);
    if (hid2 >= 0) stage(uint32_t(kTile + kBlock + tid), hid2);
    // the right-hand side D of the own node (FIRST: what was just staged)
    const double sfi = a.step_factors[i];
    const double d0 = sfi * a.fluxes[i], d1 = sfi * a.fluxes[stride + i], d2 = sfi * a.fluxes[2 * stride + i],
                 d3 = sfi * a.fluxes[3 * stride + i], d4 = sfi * a.fluxes[4 * stride + i];
    double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0, r4 = 0.0;
    if (LAST) {
        r0 = a.old_variables[i]; r1 = a.old_variables[stride + i]; r2 = a.old_variables[2 * stride + i];
        r3 = a.old_variables[3 * stride + i]; r4 = a.old_variables[4 * stride + i];
    }
    int32_t tl_b = 0, tl_n = 0;
    if (TAIL) { tl_b = tp.begin[i]; tl_n = tp.count[i]; }
    __syncthreads();

    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
    int32_t n_edges = 0;                                               // n_i: internal edges with this node as an end point
    auto add = [&](uint32_t code) {
        const uint32_t s = code & kT16SlotMask;
        if (s == kT16Pad) return;
        double v0, v1, v2, v3, v4;
        if (s >= uint32_t(kTileCap)) previous(tile_ovf[ovf0 + int32_t(s) - kTileCap], v0, v1, v2, v3, v4);
        else { v0 = rec[0][s]; v1 = rec[1][s]; v2 = rec[2][s]; v3 = rec[3][s]; v4 = rec[4][s]; }
        s0 += v0; s1 += v1; s2 += v2; s3 += v3; s4 += v4;
        n_edges++;
    };
    for (int32_t r = 0; r < n_int; r++) {                             // the codes one row ahead of the sums
        const uint32_t cn = r + 1 < n_int ? nbr16[(int64_t(row0 + r + 1) << 6) + lane] : kT16Pad;
        add(c);
        c = cn;
    }
    if (TAIL) {
        for (int32_t k = 0; k < tl_n; k++) {
            const unsigned long long word = static_cast<unsigned long long>(__double_as_longlong(tp.rec[3 * int64_t(tl_b + k) + 2].x));
            add(static_cast<uint32_t>(word >> 16) & 0xFFFFu);
        }
    }
    if (i >= nel) return;
    const double den = 1.0 + a.eps * double(n_edges);
    const double b0 = (d0 + a.eps * s0) / den, b1 = (d1 + a.eps * s1) / den, b2 = (d2 + a.eps * s2) / den,
                 b3 = (d3 + a.eps * s3) / den, b4 = (d4 + a.eps * s4) / den;
    if (!LAST) {
        a.next[i] = b0; a.next[stride + i] = b1; a.next[2 * stride + i] = b2; a.next[3 * stride + i] = b3; a.next[4 * stride + i] = b4;
        return;
    }
    const double rho = r0 + b0 / a.rk_div, mx = r1 + b1 / a.rk_div, my = r2 + b2 / a.rk_div, mz = r3 + b3 / a.rk_div,
                 en = r4 + b4 / a.rk_div;
    store_conserved(a.q_out, stride, i, rho, mx, my, mz, en);
    if (a.residuals) {
        a.residuals[i] = rho - r0; a.residuals[stride + i] = mx - r1; a.residuals[2 * stride + i] = my - r2;
        a.residuals[3 * stride + i] = mz - r3; a.residuals[4 * stride + i] = en - r4;
    }
    if (a.check) {
        const bool finite = isfinite(rho) && isfinite(mx) && isfinite(my) && isfinite(mz) && isfinite(en);
        int code = 0;
        if (!finite) code = 1;
        else if (rho < 0.0) code = 2;
        else if (en < 0.0) code = 3;
        if (code) atomicMin(a.err, err_key(a.check, a.old_of_new[i], code));
    }
}

// ------------------------------------------------------------------------------------------
// JST dissipation (no reference counterpart; INTEGRATION.md "JST dissipation"): the pressure-switched blend of second and
// fourth differences as a CORRECTION C added to the stage's fluxes F, which already hold the reference's first-difference term
// k_e (r_i + r_j) (W_i - W_j) on every internal edge.  Two node-centred gathers over the internal incidence rows in row order,
// the walk k_smooth_tile does (halo table, nbr16, overflow list, long-row lists), sums started at +0.0, one addition per edge:
//   k_jst_sensor_tile       L_i = sum (W_j - W_i),  nu_i = |sum (p_j - p_i)| / sum (p_j + p_i)  (no internal edge: 0.0),
//                           r_i = |v_i| + c_i;  p and r are derive()'s expressions.
//   k_jst_dissipation_tile  C_i = sum fac ((e2 - 1) (W_i - W_j) - e4 (L_i - L_j)),  fac = k_e (r_i + r_j),
//                           e2 = min(kappa2 max(nu_i, nu_j), 1),  e4 = max(kappa4 - e2, 0);  fluxes_i = fluxes_i + C_i.
// LDS, one field per array as in k_smooth_tile (a slot's doubles 8 B apart): the sensor stages W and the pressure derived
// once per slot (six fields of 560 doubles, 26,880 B); the dissipation stages W, L, nu and r (twelve fields, 53,760 B, under
// the 64 KB of static LDS; two workgroups per CU by LDS).  A halo node beyond the table is read — and for the sensor derived —
// from memory.  Pad lanes of the last tile write zeros to L, nu and r so that whoever stages them reads numbers.
// ------------------------------------------------------------------------------------------
template <bool TAIL>
__global__ void __launch_bounds__(kBlock, 4)
k_jst_sensor_tile(const int32_t *__restrict__ tile_halo, uint32_t n_tiles, int64_t stride, int64_t nel,
                  const int32_t *__restrict__ slice_row0, const int32_t *__restrict__ rows_int, const uint16_t *__restrict__ nbr16,
                  const int32_t *__restrict__ tile_ovf_ptr, const int32_t *__restrict__ tile_ovf, TailPlan tp, JstStep a)
{
    __shared__ double rec[6][kSmoothRow];                              // W [5] and p
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const unsigned t = xcd_contiguous_block(blockIdx.x, n_tiles);
    const int64_t i = int64_t(t) * kTile + tid;
    const int32_t slice = __builtin_amdgcn_readfirstlane(static_cast<int32_t>(i >> 6));
    const int32_t *hrow = tile_halo + int64_t(t) * kHaloStride;
    const int32_t hid = hrow[tid];
    const int32_t hid2 = tid < kHaloStride - kBlock ? hrow[kBlock + tid] : -1;
    const int32_t row0 = slice_row0[slice];
    const int32_t n_int = (TAIL ? tp.rows_main : rows_int)[slice];
    const int32_t ovf0 = tile_ovf_ptr[t];
    const int64_t hnode = hid >= 0 ? int64_t(hid) : i;                 // (no halo node: a copy of the own one in the unused slot)
    auto stage = [&](uint32_t slot, int64_t n) {
        const double rho = a.w[n], mx = a.w[stride + n], my = a.w[2 * stride + n], mz = a.w[3 * stride + n], en = a.w[4 * stride + n];
        const Derived d = derive(rho, mx, my, mz, en);
        rec[0][slot] = rho; rec[1][slot] = mx; rec[2][slot] = my; rec[3][slot] = mz; rec[4][slot] = en; rec[5][slot] = d.p;
    };
    uint32_t c = nbr16[(int64_t(n_int > 0 ? row0 : 0) << 6) + lane];   // (row 0 exists on every level; unused when n_int == 0)
    const double w0 = a.w[i], w1 = a.w[stride + i], w2 = a.w[2 * stride + i], w3 = a.w[3 * stride + i], w4 = a.w[4 * stride + i];
    const Derived me = derive(w0, w1, w2, w3, w4);
    rec[0][tid] = w0; rec[1][tid] = w1; rec[2][tid] = w2; rec[3][tid] = w3; rec[4][tid] = w4; rec[5][tid] = me.p;
    stage(uint32_t(kTile + tid), hnode);
    if (hid2 >= 0) stage(uint32_t(kTile + kBlock + tid), hid2);
    int32_t tl_b = 0, tl_n = 0;
    if (TAIL) { tl_b = tp.begin[i]; tl_n = tp.count[i]; }
    __syncthreads();

    double l0 = 0.0, l1 = 0.0, l2 = 0.0, l3 = 0.0, l4 = 0.0, pm = 0.0, pp = 0.0;
    int32_t n_edges = 0;
    auto add = [&](uint32_t code) {
        const uint32_t s = code & kT16SlotMask;
        if (s == kT16Pad) return;
        double v0, v1, v2, v3, v4, p;
        if (s >= uint32_t(kTileCap)) {
            const int64_t n = tile_ovf[ovf0 + int32_t(s) - kTileCap];
            v0 = a.w[n]; v1 = a.w[stride + n]; v2 = a.w[2 * stride + n]; v3 = a.w[3 * stride + n]; v4 = a.w[4 * stride + n];
            p = derive(v0, v1, v2, v3, v4).p;
        } else { v0 = rec[0][s]; v1 = rec[1][s]; v2 = rec[2][s]; v3 = rec[3][s]; v4 = rec[4][s]; p = rec[5][s]; }
        l0 += v0 - w0; l1 += v1 - w1; l2 += v2 - w2; l3 += v3 - w3; l4 += v4 - w4;
        pm += p - me.p;
        pp += p + me.p;
        n_edges++;
    };
    for (int32_t r = 0; r < n_int; r++) {                             // the codes one row ahead of the sums
        const uint32_t cn = r + 1 < n_int ? nbr16[(int64_t(row0 + r + 1) << 6) + lane] : kT16Pad;
        add(c);
        c = cn;
    }
    if (TAIL) {
        for (int32_t k = 0; k < tl_n; k++) {
            const unsigned long long word = static_cast<unsigned long long>(__double_as_longlong(tp.rec[3 * int64_t(tl_b + k) + 2].x));
            add(static_cast<uint32_t>(word >> 16) & 0xFFFFu);
        }
    }
    const bool present = i < nel;
    a.lap[i] = present ? l0 : 0.0; a.lap[stride + i] = present ? l1 : 0.0; a.lap[2 * stride + i] = present ? l2 : 0.0;
    a.lap[3 * stride + i] = present ? l3 : 0.0; a.lap[4 * stride + i] = present ? l4 : 0.0;
    a.nu[i] = (present && n_edges > 0) ? fabs(pm) / pp : 0.0;
    a.r[i] = present ? me.speed + me.c : 0.0;
}

template <bool TAIL>
__global__ void __launch_bounds__(kBlock, 2)
k_jst_dissipation_tile(const int32_t *__restrict__ tile_halo, uint32_t n_tiles, int64_t stride, int64_t nel,
                       const int32_t *__restrict__ slice_row0, const int32_t *__restrict__ rows_int, const uint16_t *__restrict__ nbr16,
                       const double *__restrict__ w, const int32_t *__restrict__ tile_ovf_ptr, const int32_t *__restrict__ tile_ovf,
                       TailPlan tp, JstStep a)
{
    __shared__ double rec[12][kSmoothRow];                             // W [5], L [5], nu, r
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const unsigned t = xcd_contiguous_block(blockIdx.x, n_tiles);
    const int64_t i = int64_t(t) * kTile + tid;
    const int32_t slice = __builtin_amdgcn_readfirstlane(static_cast<int32_t>(i >> 6));
    const int32_t *hrow = tile_halo + int64_t(t) * kHaloStride;
    const int32_t hid = hrow[tid];
    const int32_t hid2 = tid < kHaloStride - kBlock ? hrow[kBlock + tid] : -1;
    const int32_t row0 = slice_row0[slice];
    const int32_t n_int = (TAIL ? tp.rows_main : rows_int)[slice];
    const int32_t ovf0 = tile_ovf_ptr[t];
    const int64_t hnode = hid >= 0 ? int64_t(hid) : i;                 // (no halo node: a copy of the own one in the unused slot)
    struct Node { double w[5], l[5], nu, r; };
    auto load = [&](int64_t n) {
        Node q;
        for (int v = 0; v < 5; v++) { q.w[v] = a.w[v * stride + n]; q.l[v] = a.lap[v * stride + n]; }
        q.nu = a.nu[n]; q.r = a.r[n];
        return q;
    };
    auto stage = [&](uint32_t slot, const Node &q) {
        for (int v = 0; v < 5; v++) { rec[v][slot] = q.w[v]; rec[5 + v][slot] = q.l[v]; }
        rec[10][slot] = q.nu; rec[11][slot] = q.r;
    };
    const int64_t first_row = n_int > 0 ? row0 : 0;                    // (row 0 exists on every level; unused when n_int == 0)
    uint32_t c = nbr16[(first_row << 6) + lane];
    double ke = w[(first_row << 8) + 192 + lane];
    const Node me = load(i);
    stage(uint32_t(tid), me);
    stage(uint32_t(kTile + tid), load(hnode));
    if (hid2 >= 0) stage(uint32_t(kTile + kBlock + tid), load(hid2));
    int32_t tl_b = 0, tl_n = 0;
    if (TAIL) { tl_b = tp.begin[i]; tl_n = tp.count[i]; }
    __syncthreads();

    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0, c4 = 0.0;
    auto add = [&](uint32_t code, double k_e) {
        const uint32_t s = code & kT16SlotMask;
        if (s == kT16Pad) return;
        Node ot;
        if (s >= uint32_t(kTileCap)) ot = load(tile_ovf[ovf0 + int32_t(s) - kTileCap]);
        else {
            for (int v = 0; v < 5; v++) { ot.w[v] = rec[v][s]; ot.l[v] = rec[5 + v][s]; }
            ot.nu = rec[10][s]; ot.r = rec[11][s];
        }
        const double fac = k_e * (me.r + ot.r);
        const double nu = me.nu > ot.nu ? me.nu : ot.nu;
        double e2 = a.kappa2 * nu;
        e2 = e2 < 1.0 ? e2 : 1.0;
        double e4 = a.kappa4 - e2;
        e4 = e4 > 0.0 ? e4 : 0.0;
        const double e2m = e2 - 1.0;
        c0 += fac * (e2m * (me.w[0] - ot.w[0]) - e4 * (me.l[0] - ot.l[0]));
        c1 += fac * (e2m * (me.w[1] - ot.w[1]) - e4 * (me.l[1] - ot.l[1]));
        c2 += fac * (e2m * (me.w[2] - ot.w[2]) - e4 * (me.l[2] - ot.l[2]));
        c3 += fac * (e2m * (me.w[3] - ot.w[3]) - e4 * (me.l[3] - ot.l[3]));
        c4 += fac * (e2m * (me.w[4] - ot.w[4]) - e4 * (me.l[4] - ot.l[4]));
    };
    for (int32_t r = 0; r < n_int; r++) {                             // code and weight one row ahead of the sums
        const bool more = r + 1 < n_int;
        const uint32_t cn = more ? nbr16[(int64_t(row0 + r + 1) << 6) + lane] : kT16Pad;
        const double kn = more ? w[(int64_t(row0 + r + 1) << 8) + 192 + lane] : 0.0;
        add(c, ke);
        c = cn;
        ke = kn;
    }
    if (TAIL) {
        for (int32_t k = 0; k < tl_n; k++) {
            const double2 fzk = tp.rec[3 * int64_t(tl_b + k) + 1];
            const unsigned long long word = static_cast<unsigned long long>(__double_as_longlong(tp.rec[3 * int64_t(tl_b + k) + 2].x));
            add(static_cast<uint32_t>(word >> 16) & 0xFFFFu, fzk.y);
        }
    }
    if (i >= nel) return;
    a.fluxes[i] = a.fluxes[i] + c0; a.fluxes[stride + i] = a.fluxes[stride + i] + c1; a.fluxes[2 * stride + i] = a.fluxes[2 * stride + i] + c2;
    a.fluxes[3 * stride + i] = a.fluxes[3 * stride + i] + c3; a.fluxes[4 * stride + i] = a.fluxes[4 * stride + i] + c4;
}

// ------------------------------------------------------------------------------------------
// Laminar viscous terms (no reference counterpart; INTEGRATION.md "Laminar viscous terms"): the Navier-Stokes stresses and
// the heat flux as a CORRECTION V added to the stage's fluxes F (+ C), components 1..4.  Two node-centred gathers over the
// internal incidence rows in row order, the walk k_jst_dissipation_tile does (halo table, nbr16, overflow list, long-row
// lists; code and weights one row ahead of the sums), sums started at +0.0, one addition per edge.  The rows hold the edge
// weights as the flux kernel wants them, f = -0.5 e at the a end and +0.5 e at the b end: the normal seen from this node
// is n = -2.0 * f, exactly.
//   k_viscous_stress_tile   A[phi][d] = sum (phi_j - phi_i) n_d for phi in (u, v, w, T = p / rho);  G = (0.5 A) / vol;
//                           S_i = (u, v, w, txx, tyy, tzz, txy, txz, tyz, qx, qy, qz): Stokes' stresses at constant mu and
//                           q = kappa grad T, finished per node so that pass 2 stages twelve doubles and not seventeen.
//                           Under a viscosity model (mgcfd_set_viscosity_model) mu and kappa are per-node factors formed here,
//                           where the gradients already are: the kernel's VAR instantiation.
//   k_viscous_flux_tile     V_i[1..3] = sum tau_bar . n,  V_i[4] = sum (tau_bar . v_bar + q_bar) . n,  bars = 0.5 (S_i + S_j);
//                           fluxes_i[1..4] = fluxes_i[1..4] + V_i[1..4].
// LDS, one field per array as in k_smooth_tile (a slot's doubles 8 B apart): the stress launch stages u, v, w, T derived
// once per slot (four fields of 560 doubles, 17,920 B); the flux launch stages S (twelve fields, 53,760 B, the JST
// dissipation launch's footprint; two workgroups per CU by LDS).  A halo node beyond the table is read — and for the stress
// launch derived — from memory.  Pad lanes of the last tile write zeros to S so that whoever stages them reads numbers.
// ------------------------------------------------------------------------------------------
// VAR: the variable instantiation — after the row walk mu_i by the law, mut_i read (eddy 1) or formed and written (eddy 2; pad
// lanes of the last tile write +0.0), me_i = mu_i + mut_i on the stresses and kap_i on the heat flux.  VAR = false is the
// constant-viscosity kernel, which reads nothing of a.model.
template <bool TAIL, bool VAR>
__global__ void __launch_bounds__(kBlock, 4)
k_viscous_stress_tile(const int32_t *__restrict__ tile_halo, uint32_t n_tiles, int64_t stride, int64_t nel,
                      const int32_t *__restrict__ slice_row0, const int32_t *__restrict__ rows_int, const uint16_t *__restrict__ nbr16,
                      const double *__restrict__ w, const int32_t *__restrict__ tile_ovf_ptr, const int32_t *__restrict__ tile_ovf,
                      TailPlan tp, ViscousStep a)
{
    __shared__ double rec[4][kSmoothRow];                              // u, v, w, T
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const unsigned t = xcd_contiguous_block(blockIdx.x, n_tiles);
    const int64_t i = int64_t(t) * kTile + tid;
    const int32_t slice = __builtin_amdgcn_readfirstlane(static_cast<int32_t>(i >> 6));
    const int32_t *hrow = tile_halo + int64_t(t) * kHaloStride;
    const int32_t hid = hrow[tid];
    const int32_t hid2 = tid < kHaloStride - kBlock ? hrow[kBlock + tid] : -1;
    const int32_t row0 = slice_row0[slice];
    const int32_t n_int = (TAIL ? tp.rows_main : rows_int)[slice];
    const int32_t ovf0 = tile_ovf_ptr[t];
    const int64_t hnode = hid >= 0 ? int64_t(hid) : i;                 // (no halo node: a copy of the own one in the unused slot)
    auto stage = [&](uint32_t slot, const Primitive &q) { rec[0][slot] = q.u; rec[1][slot] = q.v; rec[2][slot] = q.w; rec[3][slot] = q.T; };
    const int64_t first_row = n_int > 0 ? row0 : 0;                    // (row 0 exists on every level; unused when n_int == 0)
    uint32_t c = nbr16[(first_row << 6) + lane];
    double fx = w[(first_row << 8) + lane], fy = w[(first_row << 8) + 64 + lane], fz = w[(first_row << 8) + 128 + lane];
    const Primitive me = primitive_of(a.w, stride, i);
    stage(uint32_t(tid), me);
    stage(uint32_t(kTile + tid), primitive_of(a.w, stride, hnode));
    if (hid2 >= 0) stage(uint32_t(kTile + kBlock + tid), primitive_of(a.w, stride, hid2));
    int32_t tl_b = 0, tl_n = 0;
    if (TAIL) { tl_b = tp.begin[i]; tl_n = tp.count[i]; }
    const double vol = a.volumes[i];
    __syncthreads();

    double ux = 0.0, uy = 0.0, uz = 0.0, vx = 0.0, vy = 0.0, vz = 0.0, wx = 0.0, wy = 0.0, wz = 0.0, tx = 0.0, ty = 0.0, tz = 0.0;
    auto add = [&](uint32_t code, double hx, double hy, double hz) {
        const uint32_t s = code & kT16SlotMask;
        if (s == kT16Pad) return;
        Primitive ot;
        if (s >= uint32_t(kTileCap)) ot = primitive_of(a.w, stride, tile_ovf[ovf0 + int32_t(s) - kTileCap]);
        else { ot.u = rec[0][s]; ot.v = rec[1][s]; ot.w = rec[2][s]; ot.T = rec[3][s]; }
        const double nx = -2.0 * hx, ny = -2.0 * hy, nz = -2.0 * hz;   // the rows hold -+0.5 e
        const double du = ot.u - me.u, dv = ot.v - me.v, dw = ot.w - me.w, dT = ot.T - me.T;
        ux += du * nx; uy += du * ny; uz += du * nz;
        vx += dv * nx; vy += dv * ny; vz += dv * nz;
        wx += dw * nx; wy += dw * ny; wz += dw * nz;
        tx += dT * nx; ty += dT * ny; tz += dT * nz;
    };
    for (int32_t r = 0; r < n_int; r++) {                             // code and weights one row ahead of the sums
        const bool more = r + 1 < n_int;
        const int64_t nr = int64_t(row0 + r + 1);
        const uint32_t cn = more ? nbr16[(nr << 6) + lane] : kT16Pad;
        const double fxn = more ? w[(nr << 8) + lane] : 0.0, fyn = more ? w[(nr << 8) + 64 + lane] : 0.0, fzn = more ? w[(nr << 8) + 128 + lane] : 0.0;
        add(c, fx, fy, fz);
        c = cn; fx = fxn; fy = fyn; fz = fzn;
    }
    if (TAIL) {
        for (int32_t k = 0; k < tl_n; k++) {
            const double2 fxy = tp.rec[3 * int64_t(tl_b + k)], fzk = tp.rec[3 * int64_t(tl_b + k) + 1];
            const unsigned long long word = static_cast<unsigned long long>(__double_as_longlong(tp.rec[3 * int64_t(tl_b + k) + 2].x));
            add(static_cast<uint32_t>(word >> 16) & 0xFFFFu, fxy.x, fxy.y, fzk.x);
        }
    }
    const double gux = (0.5 * ux) / vol, guy = (0.5 * uy) / vol, guz = (0.5 * uz) / vol;
    const double gvx = (0.5 * vx) / vol, gvy = (0.5 * vy) / vol, gvz = (0.5 * vz) / vol;
    const double gwx = (0.5 * wx) / vol, gwy = (0.5 * wy) / vol, gwz = (0.5 * wz) / vol;
    const double gtx = (0.5 * tx) / vol, gty = (0.5 * ty) / vol, gtz = (0.5 * tz) / vol;
    const double div = (gux + gvy) + gwz;
    const double tt = (2.0 / 3.0) * div;
    const bool present = i < nel;
    double mu_e = a.mu, kap = a.kappa;
    if (VAR) {
        const ViscosityModel &m = a.model;
        const double mu_i = viscosity_of(m, a.mu, me.T);
        double mut = 0.0;
        if (m.eddy == 1) mut = m.mut[i];
        else if (m.eddy == 2) {
            mut = smagorinsky_of(m, m.d2[i], a.w[i], gux, guy, guz, gvx, gvy, gvz, gwx, gwy, gwz);
            m.mut[i] = present ? mut : 0.0;
        }
        mu_e = mu_i + mut;
        kap = m.cp * (mu_i / m.prandtl + mut / m.prandtl_t);
    }
    double out[12];
    out[0] = me.u; out[1] = me.v; out[2] = me.w;
    out[3] = mu_e * (2.0 * gux - tt); out[4] = mu_e * (2.0 * gvy - tt); out[5] = mu_e * (2.0 * gwz - tt);
    out[6] = mu_e * (guy + gvx); out[7] = mu_e * (guz + gwx); out[8] = mu_e * (gvz + gwy);
    out[9] = kap * gtx; out[10] = kap * gty; out[11] = kap * gtz;
#pragma unroll
    for (int f = 0; f < 12; f++) a.s[f * stride + i] = present ? out[f] : 0.0;
}

template <bool TAIL>
__global__ void __launch_bounds__(kBlock, 2)
k_viscous_flux_tile(const int32_t *__restrict__ tile_halo, uint32_t n_tiles, int64_t stride, int64_t nel,
                    const int32_t *__restrict__ slice_row0, const int32_t *__restrict__ rows_int, const uint16_t *__restrict__ nbr16,
                    const double *__restrict__ w, const int32_t *__restrict__ tile_ovf_ptr, const int32_t *__restrict__ tile_ovf,
                    TailPlan tp, ViscousStep a)
{
    __shared__ double rec[12][kSmoothRow];                             // S
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const unsigned t = xcd_contiguous_block(blockIdx.x, n_tiles);
    const int64_t i = int64_t(t) * kTile + tid;
    const int32_t slice = __builtin_amdgcn_readfirstlane(static_cast<int32_t>(i >> 6));
    const int32_t *hrow = tile_halo + int64_t(t) * kHaloStride;
    const int32_t hid = hrow[tid];
    const int32_t hid2 = tid < kHaloStride - kBlock ? hrow[kBlock + tid] : -1;
    const int32_t row0 = slice_row0[slice];
    const int32_t n_int = (TAIL ? tp.rows_main : rows_int)[slice];
    const int32_t ovf0 = tile_ovf_ptr[t];
    const int64_t hnode = hid >= 0 ? int64_t(hid) : i;                 // (no halo node: a copy of the own one in the unused slot)
    struct Node { double s[12]; };
    auto load = [&](int64_t n) {
        Node q;
#pragma unroll
        for (int f = 0; f < 12; f++) q.s[f] = a.s[f * stride + n];
        return q;
    };
    auto stage = [&](uint32_t slot, const Node &q) {
#pragma unroll
        for (int f = 0; f < 12; f++) rec[f][slot] = q.s[f];
    };
    const int64_t first_row = n_int > 0 ? row0 : 0;                    // (row 0 exists on every level; unused when n_int == 0)
    uint32_t c = nbr16[(first_row << 6) + lane];
    double fx = w[(first_row << 8) + lane], fy = w[(first_row << 8) + 64 + lane], fz = w[(first_row << 8) + 128 + lane];
    const Node me = load(i);
    stage(uint32_t(tid), me);
    stage(uint32_t(kTile + tid), load(hnode));
    if (hid2 >= 0) stage(uint32_t(kTile + kBlock + tid), load(hid2));
    int32_t tl_b = 0, tl_n = 0;
    if (TAIL) { tl_b = tp.begin[i]; tl_n = tp.count[i]; }
    __syncthreads();

    double v1 = 0.0, v2 = 0.0, v3 = 0.0, v4 = 0.0;
    auto add = [&](uint32_t code, double hx, double hy, double hz) {
        const uint32_t s = code & kT16SlotMask;
        if (s == kT16Pad) return;
        Node ot;
        if (s >= uint32_t(kTileCap)) ot = load(tile_ovf[ovf0 + int32_t(s) - kTileCap]);
        else {
#pragma unroll
            for (int f = 0; f < 12; f++) ot.s[f] = rec[f][s];
        }
        const double nx = -2.0 * hx, ny = -2.0 * hy, nz = -2.0 * hz;   // the rows hold -+0.5 e
        double b[12];
#pragma unroll
        for (int f = 0; f < 12; f++) b[f] = 0.5 * (me.s[f] + ot.s[f]);
        const double u = b[0], v = b[1], ww = b[2], txx = b[3], tyy = b[4], tzz = b[5], txy = b[6], txz = b[7], tyz = b[8];
        const double ex = ((u * txx + v * txy) + ww * txz) + b[9];
        const double ey = ((u * txy + v * tyy) + ww * tyz) + b[10];
        const double ez = ((u * txz + v * tyz) + ww * tzz) + b[11];
        v1 += (txx * nx + txy * ny) + txz * nz;
        v2 += (txy * nx + tyy * ny) + tyz * nz;
        v3 += (txz * nx + tyz * ny) + tzz * nz;
        v4 += (ex * nx + ey * ny) + ez * nz;
    };
    for (int32_t r = 0; r < n_int; r++) {                             // code and weights one row ahead of the sums
        const bool more = r + 1 < n_int;
        const int64_t nr = int64_t(row0 + r + 1);
        const uint32_t cn = more ? nbr16[(nr << 6) + lane] : kT16Pad;
        const double fxn = more ? w[(nr << 8) + lane] : 0.0, fyn = more ? w[(nr << 8) + 64 + lane] : 0.0, fzn = more ? w[(nr << 8) + 128 + lane] : 0.0;
        add(c, fx, fy, fz);
        c = cn; fx = fxn; fy = fyn; fz = fzn;
    }
    if (TAIL) {
        for (int32_t k = 0; k < tl_n; k++) {
            const double2 fxy = tp.rec[3 * int64_t(tl_b + k)], fzk = tp.rec[3 * int64_t(tl_b + k) + 1];
            const unsigned long long word = static_cast<unsigned long long>(__double_as_longlong(tp.rec[3 * int64_t(tl_b + k) + 2].x));
            add(static_cast<uint32_t>(word >> 16) & 0xFFFFu, fxy.x, fxy.y, fzk.x);
        }
    }
    if (i >= nel) return;
    a.fluxes[stride + i] = a.fluxes[stride + i] + v1; a.fluxes[2 * stride + i] = a.fluxes[2 * stride + i] + v2;
    a.fluxes[3 * stride + i] = a.fluxes[3 * stride + i] + v3; a.fluxes[4 * stride + i] = a.fluxes[4 * stride + i] + v4;
}

// residual (validation.cpp:77-89), flat over the 5 padded fields
__global__ void __launch_bounds__(kBlock)
k_residual(int64_t n, const double *__restrict__ old_variables, const double *__restrict__ variables,
           double *__restrict__ residuals)
{
    const int64_t k = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (k < n) residuals[k] = variables[k] - old_variables[k];
}

// sum of squares for calc_rms (validation.cpp:91-105) over the nel real entries of 5 fields.
// Tree order differs from the reference's serial sum; the value is only ever printed with %.3e.
__global__ void __launch_bounds__(kBlock)
k_sumsq(int64_t nel, int64_t stride, const double *__restrict__ x, double *__restrict__ partial,
        const int32_t *__restrict__ old_of_new, int64_t n_owned)
{
    __shared__ double s[kBlock / 64];
    double acc = 0.0;
    for (int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x; i < nel; i += int64_t(gridDim.x) * kBlock) {
        if (old_of_new && old_of_new[i] >= n_owned) continue;        // ghost of a partitioned level: counted by its owner
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

// ------------------------------------------------------------------------------------------
// mg_restrict (mg_loops.cpp:30-202) as a coarse-centred gather: coarse = (sum of children in
// ascending fine id) * (1/count); coarse nodes without children keep their value.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_restrict(int64_t nel_coarse, int64_t stride_coarse, int64_t stride_fine, const int32_t *__restrict__ child_ptr,
           const int32_t *__restrict__ child, const int4 *__restrict__ child4, const double *__restrict__ fine_q,
           double *__restrict__ coarse_q, const double *__restrict__ cbrt_vol, double cfl,
           double *__restrict__ partial_min /* nullptr, or: look ahead, see below */,
           SumTask rms /* .partial != nullptr: the last workgroup also adds up the fine level's per-tile sums of squares
                          (calc_rms of the sweep just finished) — the launch that would do only that is saved */)
{
    // (coarse tiles next to each other read children next to each other: one XCD's L2 per contiguous range of them)
    const int64_t c = xcd_contiguous_block(blockIdx.x, gridDim.x) * int64_t(kBlock) + threadIdx.x;
    double sf = __longlong_as_double(0x7FF0000000000000LL);          // +inf
    if (c < nel_coarse) {
        // The first four children come from a fixed-stride table (-1 padded): their ids need no
        // pointer look-up and their 20 loads are all in flight together; the sum keeps the reference's
        // order (ascending original fine id, mg_loops.cpp:119-142).
        const int4 k4 = child4[c];
        const int32_t b = child_ptr[c], e = child_ptr[c + 1];
        const int32_t n = e - b;
        const int64_t j0 = k4.x < 0 ? 0 : k4.x, j1 = k4.y < 0 ? 0 : k4.y, j2 = k4.z < 0 ? 0 : k4.z, j3 = k4.w < 0 ? 0 : k4.w;
        const int64_t sfn = stride_fine;
        const double a0 = fine_q[j0], a1 = fine_q[sfn + j0], a2 = fine_q[2 * sfn + j0], a3 = fine_q[3 * sfn + j0], a4 = fine_q[4 * sfn + j0];
        const double b0 = fine_q[j1], b1 = fine_q[sfn + j1], b2 = fine_q[2 * sfn + j1], b3 = fine_q[3 * sfn + j1], b4 = fine_q[4 * sfn + j1];
        const double c0 = fine_q[j2], c1 = fine_q[sfn + j2], c2 = fine_q[2 * sfn + j2], c3 = fine_q[3 * sfn + j2], c4 = fine_q[4 * sfn + j2];
        const double d0 = fine_q[j3], d1 = fine_q[sfn + j3], d2 = fine_q[2 * sfn + j3], d3 = fine_q[3 * sfn + j3], d4 = fine_q[4 * sfn + j3];
        double n0, n1, n2, n3, n4;
        if (n == 0) {
            // no children: the coarse node keeps its value (mg_loops.cpp:63-78,174-189)
            if (partial_min) {
                n0 = coarse_q[c]; n1 = coarse_q[stride_coarse + c]; n2 = coarse_q[2 * stride_coarse + c];
                n3 = coarse_q[3 * stride_coarse + c]; n4 = coarse_q[4 * stride_coarse + c];
            }
        } else {
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
            s0 += a0; s1 += a1; s2 += a2; s3 += a3; s4 += a4;
            if (n > 1) { s0 += b0; s1 += b1; s2 += b2; s3 += b3; s4 += b4; }
            if (n > 2) { s0 += c0; s1 += c1; s2 += c2; s3 += c3; s4 += c4; }
            if (n > 3) { s0 += d0; s1 += d1; s2 += d2; s3 += d3; s4 += d4; }
            for (int32_t k = b + 4; k < e; k++) {                     // fifth child onwards (rare)
                const int64_t j = child[k];
                s0 += fine_q[j]; s1 += fine_q[sfn + j]; s2 += fine_q[2 * sfn + j];
                s3 += fine_q[3 * sfn + j]; s4 += fine_q[4 * sfn + j];
            }
            const double average = 1.0 / double(n);
            n0 = s0 * average; n1 = s1 * average; n2 = s2 * average; n3 = s3 * average; n4 = s4 * average;
            store_conserved(coarse_q, stride_coarse, c, n0, n1, n2, n3, n4);
        }
        // The sweep that follows on the coarse level starts with compute_step_factor on exactly these
        // values: leave its first half (the per-workgroup minima) behind.
        if (partial_min) sf = local_step_factor(n0, n1, n2, n3, n4, cbrt_vol[c], cfl);
    }
    if (partial_min) block_min_to(sf, partial_min);
    // (the workgroup dispatched FIRST adds them up: its extra microsecond ends long before the launch's last workgroups do)
    if (rms.partial && blockIdx.x == 0) block_sum_partials(rms);                  // (uniform per workgroup)
}

// ------------------------------------------------------------------------------------------
// The FAS restriction: k_restrict's gather carrying ten values per child — the state, averaged exactly as there (same
// operations in the same order: same bits), and the fine level's total residual T = R (+ P on a fine level >= 1), summed
// from +0.0 in the same child order and not averaged.  One launch writes the coarse state, its copy W0 (all nodes: a node
// without children keeps its value there too) and the residual sum Q (+0.0 without children).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
k_restrict_fas(int64_t nel_coarse, int64_t stride_coarse, int64_t stride_fine, const int32_t *__restrict__ child_ptr,
               const int32_t *__restrict__ child, const int4 *__restrict__ child4, const double *__restrict__ fine_q,
               const double *__restrict__ fine_r, const double *__restrict__ fine_p /* nullptr on level 0: no forcing there */,
               double *__restrict__ coarse_q, double *__restrict__ w0, double *__restrict__ qsum)
{
    const int64_t c = xcd_contiguous_block(blockIdx.x, gridDim.x) * int64_t(kBlock) + threadIdx.x;
    if (c >= nel_coarse) return;
    const int4 k4 = child4[c];
    const int32_t b = child_ptr[c], e = child_ptr[c + 1];
    const int32_t n = e - b;
    const int64_t sfn = stride_fine, sc = stride_coarse;
    // the first four children unconditionally (-1 padded table: a missing one reads node 0 and is not added)
    const int64_t j4[4] = {k4.x < 0 ? 0 : k4.x, k4.y < 0 ? 0 : k4.y, k4.z < 0 ? 0 : k4.z, k4.w < 0 ? 0 : k4.w};
    double a[4][5], t[4][5];
#pragma unroll
    for (int k = 0; k < 4; k++) {
#pragma unroll
        for (int v = 0; v < 5; v++) {
            a[k][v] = fine_q[v * sfn + j4[k]];
            t[k][v] = fine_r[v * sfn + j4[k]];
            if (fine_p) t[k][v] = t[k][v] + fine_p[v * sfn + j4[k]];
        }
    }
    if (n == 0) {
#pragma unroll
        for (int v = 0; v < 5; v++) { w0[v * sc + c] = coarse_q[v * sc + c]; qsum[v * sc + c] = 0.0; }
        return;
    }
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, g[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (n > k) {
#pragma unroll
            for (int v = 0; v < 5; v++) { s[v] += a[k][v]; g[v] += t[k][v]; }
        }
    }
    for (int32_t k = b + 4; k < e; k++) {                             // fifth child onwards
        const int64_t j = child[k];
#pragma unroll
        for (int v = 0; v < 5; v++) {
            double tv = fine_r[v * sfn + j];
            if (fine_p) tv = tv + fine_p[v * sfn + j];
            s[v] += fine_q[v * sfn + j];
            g[v] += tv;
        }
    }
    const double average = 1.0 / double(n);
    const double n0 = s[0] * average, n1 = s[1] * average, n2 = s[2] * average, n3 = s[3] * average, n4 = s[4] * average;
    store_conserved(coarse_q, sc, c, n0, n1, n2, n3, n4);
    store_conserved(w0, sc, c, n0, n1, n2, n3, n4);
#pragma unroll
    for (int v = 0; v < 5; v++) qsum[v * sc + c] = g[v];
}

// ------------------------------------------------------------------------------------------
// prolong_residuals_interpolate_proper (mg_loops.cpp:678-864) as a fine-node gather over the
// same sliced-ELL rows as the flux (one entry per incident internal edge, reference order):
//   wavg = sum_e (w_own*R[p_own] + w_other*R[p_other]) / w_sum   (or R[parent] if coincident)
//   variables += residuals - wavg
// ------------------------------------------------------------------------------------------
// FAS (the up leg of a FAS cycle): what is interpolated is D = W0 - W, the coarse level's start state minus its current one,
// formed as the coarse value is loaded (`coarse_residuals` is W0, `coarse_q` is W), and the fine residual's place is taken by
// +0.0: variables += 0.0 - wavg(D).  Same entries, order, weights and quirks.
// STATE (mgcfd_prolong_state): what is interpolated is the coarse STATE itself (`coarse_residuals` is variables[fine + 1]) and
// the fine node's own state and residual are not read at all: variables = 0.0 - (0.0 - wavg), which only turns a -0.0 into +0.0.
enum { kProResiduals = 0, kProFas = 1, kProState = 2 };
template <int MODE>
__device__ __forceinline__ double pro_coarse(const double *__restrict__ coarse_residuals, const double *__restrict__ coarse_q, int64_t at)
{
    return MODE == kProFas ? coarse_residuals[at] - coarse_q[at] : coarse_residuals[at];
}
// the fine node's new value: q + (f - wavg), or in the STATE mode 0.0 - (0.0 - wavg)
template <int MODE>
__device__ __forceinline__ double pro_result(double q, double f, double wavg)
{
    return MODE == kProState ? 0.0 - (0.0 - wavg) : q + (f - wavg);
}

template <int MODE>
__global__ void __launch_bounds__(kBlock)
k_prolong(int64_t nel, int64_t stride, int64_t stride_coarse, const int32_t *__restrict__ slice_row0,
          const int32_t *__restrict__ rows_int, const double *__restrict__ pro_w, const int32_t *__restrict__ pro_p,
          const int32_t *__restrict__ pro_parent, const double *__restrict__ pro_wsum,
          const double *__restrict__ coarse_residuals, const double *__restrict__ fine_residuals /* the reference's mode only */,
          double *__restrict__ fine_q, const double *__restrict__ cbrt_vol, double cfl,
          double *__restrict__ partial_min /* nullptr, or: look ahead as in k_restrict */, const double *__restrict__ coarse_q /* FAS only */)
{
    constexpr bool STATE = MODE == kProState, NO_F = MODE != kProResiduals;       // (only the reference's prolongation reads fine residuals)
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int32_t slice = __builtin_amdgcn_readfirstlane(static_cast<int32_t>(i >> 6));
    if ((int64_t(slice) << 6) >= nel) {                              // a wave past the last node
        if (partial_min) block_min_to(__longlong_as_double(0x7FF0000000000000LL), partial_min);
        return;
    }
    const bool active = i < nel;
    const int64_t ii = active ? i : nel - 1;
    const int32_t row0 = slice_row0[slice];
    const int32_t n_int = rows_int[slice];
    const int32_t parent = pro_parent[ii];
    const int64_t sc = stride_coarse;
    // this node's own state and residual: needed at the end, requested now
    const double q0 = STATE ? 0.0 : fine_q[ii], q1 = STATE ? 0.0 : fine_q[stride + ii], q2 = STATE ? 0.0 : fine_q[2 * stride + ii],
                 q3 = STATE ? 0.0 : fine_q[3 * stride + ii], q4 = STATE ? 0.0 : fine_q[4 * stride + ii];
    const double f0 = NO_F ? 0.0 : fine_residuals[ii], f1 = NO_F ? 0.0 : fine_residuals[stride + ii], f2 = NO_F ? 0.0 : fine_residuals[2 * stride + ii],
                 f3 = NO_F ? 0.0 : fine_residuals[3 * stride + ii], f4 = NO_F ? 0.0 : fine_residuals[4 * stride + ii];
    const double ws = pro_wsum[ii];
    // The node's own parent appears in every entry (and, through the reference's b1-for-a1 quirk,
    // as BOTH terms of every entry in which this node is the edge's 'b' end): fetch it once.
    const int64_t own = parent < 0 ? int64_t(~parent) : int64_t(parent);
    const double o0 = pro_coarse<MODE>(coarse_residuals, coarse_q, own), o1 = pro_coarse<MODE>(coarse_residuals, coarse_q, sc + own), o2 = pro_coarse<MODE>(coarse_residuals, coarse_q, 2 * sc + own),
                 o3 = pro_coarse<MODE>(coarse_residuals, coarse_q, 3 * sc + own), o4 = pro_coarse<MODE>(coarse_residuals, coarse_q, 4 * sc + own);
    double r0, r1, r2, r3, r4;
    if (parent < 0) {
        r0 = o0; r1 = o1; r2 = o2; r3 = o3; r4 = o4;
    } else {
        r0 = r1 = r2 = r3 = r4 = 0.0;
        // entries stored [row][w_own | w_other][64 lanes] and [row][64 lanes] (the other end's parent)
        const double *wr = pro_w + (int64_t(row0) << 7) + lane;
        const int32_t *pr = pro_p + (int64_t(row0) << 6) + lane;
        for (int32_t r = 0; r < n_int; r++, wr += 128, pr += 64) {
            const double w_own = wr[0], w_other = wr[64];
            const int32_t p_other = pr[0];
            if (w_own == 0.0 && w_other == 0.0) continue;            // ELL padding
            r0 += w_own * o0; r1 += w_own * o1; r2 += w_own * o2; r3 += w_own * o3; r4 += w_own * o4;
            double x0 = o0, x1 = o1, x2 = o2, x3 = o3, x4 = o4;
            if (p_other != parent) {                                   // the other end's parent: gather
                const int64_t px = p_other;
                x0 = pro_coarse<MODE>(coarse_residuals, coarse_q, px); x1 = pro_coarse<MODE>(coarse_residuals, coarse_q, sc + px); x2 = pro_coarse<MODE>(coarse_residuals, coarse_q, 2 * sc + px);
                x3 = pro_coarse<MODE>(coarse_residuals, coarse_q, 3 * sc + px); x4 = pro_coarse<MODE>(coarse_residuals, coarse_q, 4 * sc + px);
            }
            r0 += w_other * x0; r1 += w_other * x1; r2 += w_other * x2; r3 += w_other * x3; r4 += w_other * x4;
        }
    }
    double sf = __longlong_as_double(0x7FF0000000000000LL);          // +inf
    if (active) {
        const double n0 = pro_result<MODE>(q0, f0, r0 / ws);
        const double n1 = pro_result<MODE>(q1, f1, r1 / ws);
        const double n2 = pro_result<MODE>(q2, f2, r2 / ws);
        const double n3 = pro_result<MODE>(q3, f3, r3 / ws);
        const double n4 = pro_result<MODE>(q4, f4, r4 / ws);
        store_conserved(fine_q, stride, i, n0, n1, n2, n3, n4);
        if (partial_min) sf = local_step_factor(n0, n1, n2, n3, n4, cbrt_vol[i], cfl);
    }
    if (partial_min) block_min_to(sf, partial_min);
}

// ------------------------------------------------------------------------------------------
// The same prolongation with the coarse residuals served from LDS: one workgroup = one fine tile;
// the distinct coarse nodes the tile refers to (own parents and the other ends' parents, a few
// hundred) are read from HBM once, 40 bytes each, and every entry then finds them in LDS instead
// of gathering five scattered doubles through L1.  Same entries, same order, same arithmetic.
// ------------------------------------------------------------------------------------------
template <int MODE>
__global__ void __launch_bounds__(kBlock)
k_prolong_tile(int64_t nel, int64_t stride, int64_t stride_coarse, const int32_t *__restrict__ slice_row0,
               const int32_t *__restrict__ rows_int, const double *__restrict__ pro_w,
               const uint16_t *__restrict__ pro_s16, const uint16_t *__restrict__ pro_own16,
               const int32_t *__restrict__ pro_tile_n, const int32_t *__restrict__ pro_tile_ids,
               const int32_t *__restrict__ pro_parent, const double *__restrict__ pro_wsum,
               const double *__restrict__ coarse_residuals, const double *__restrict__ fine_residuals /* the reference's mode only */,
               double *__restrict__ fine_q, const double *__restrict__ cbrt_vol, double cfl, double *__restrict__ partial_min,
               const double *__restrict__ coarse_q /* FAS only */)
{
    constexpr bool STATE = MODE == kProState, NO_F = MODE != kProResiduals;       // (only the reference's prolongation reads fine residuals)
    __shared__ double cr[kProCap * 5];
    const unsigned t = xcd_contiguous_block(blockIdx.x, gridDim.x);   // neighbouring tiles (they share coarse parents) on one XCD's L2
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int64_t i = int64_t(t) * kTile + tid;
    const bool active = i < nel;
    const int64_t ii = active ? i : nel - 1;
    const int32_t slice = __builtin_amdgcn_readfirstlane(static_cast<int32_t>(i >> 6));
    const int64_t sc = stride_coarse;

    // The tile's coarse residuals are staged behind a dependent chain (ids -> residuals by id): the id of this thread's first staged
    // node goes out FIRST (a fixed-stride table, -1 padded: the address needs only the tile number), everything that depends on
    // nothing — the node's own state, residual, weights — behind it, and the gather last, so that the chain's two round trips are
    // not followed by a third (round 4: the staging loop used to stand in front of every other load).
    const int32_t *ids = pro_tile_ids + int64_t(t) * kProCap;
    const int32_t c_first = ids[tid];
    const int32_t n_ids = pro_tile_n[t];
    const bool wave_live = (int64_t(slice) << 6) < nel;
    const int32_t row0 = wave_live ? slice_row0[slice] : 0;
    const int32_t n_int = wave_live ? rows_int[slice] : 0;
    const int32_t parent = pro_parent[ii];
    const uint32_t own_slot = pro_own16[ii];
    const double q0 = STATE ? 0.0 : fine_q[ii], q1 = STATE ? 0.0 : fine_q[stride + ii], q2 = STATE ? 0.0 : fine_q[2 * stride + ii],
                 q3 = STATE ? 0.0 : fine_q[3 * stride + ii], q4 = STATE ? 0.0 : fine_q[4 * stride + ii];
    const double f0 = NO_F ? 0.0 : fine_residuals[ii], f1 = NO_F ? 0.0 : fine_residuals[stride + ii], f2 = NO_F ? 0.0 : fine_residuals[2 * stride + ii],
                 f3 = NO_F ? 0.0 : fine_residuals[3 * stride + ii], f4 = NO_F ? 0.0 : fine_residuals[4 * stride + ii];
    const double ws = pro_wsum[ii];
    // the first row pair's entries go out before the staging barrier too (they do not depend on the staged residuals)
    const double *wr = pro_w + (int64_t(row0) << 7) + lane;
    const uint16_t *sr = pro_s16 + (int64_t(row0) << 6) + lane;
    double wa0 = wr[0], wb0 = wr[64], wa1 = wr[128], wb1 = wr[192];
    uint32_t sl0 = sr[0], sl1 = sr[64];
    {
        // (a thread without a staged node of its own gathers node 0 and stores nothing: the load is never conditional)
        const int64_t c = c_first >= 0 ? c_first : 0;
        const double d0 = pro_coarse<MODE>(coarse_residuals, coarse_q, c), d1 = pro_coarse<MODE>(coarse_residuals, coarse_q, sc + c), d2 = pro_coarse<MODE>(coarse_residuals, coarse_q, 2 * sc + c),
                     d3 = pro_coarse<MODE>(coarse_residuals, coarse_q, 3 * sc + c), d4 = pro_coarse<MODE>(coarse_residuals, coarse_q, 4 * sc + c);
        if (tid < n_ids) { double *d = cr + tid * 5; d[0] = d0; d[1] = d1; d[2] = d2; d[3] = d3; d[4] = d4; }
        for (int32_t k = tid + kBlock; k < n_ids; k += kBlock) {        // (a tile that refers to more than 256 coarse nodes: rare)
            const int64_t c2 = ids[k];
            double *d = cr + k * 5;
            d[0] = pro_coarse<MODE>(coarse_residuals, coarse_q, c2); d[1] = pro_coarse<MODE>(coarse_residuals, coarse_q, sc + c2); d[2] = pro_coarse<MODE>(coarse_residuals, coarse_q, 2 * sc + c2);
            d[3] = pro_coarse<MODE>(coarse_residuals, coarse_q, 3 * sc + c2); d[4] = pro_coarse<MODE>(coarse_residuals, coarse_q, 4 * sc + c2);
        }
    }
    __syncthreads();

    const double *od = cr + own_slot * 5;
    const double o0 = od[0], o1 = od[1], o2 = od[2], o3 = od[3], o4 = od[4];
    double r0, r1, r2, r3, r4;
    if (parent < 0) {
        r0 = o0; r1 = o1; r2 = o2; r3 = o3; r4 = o4;
    } else {
        r0 = r1 = r2 = r3 = r4 = 0.0;
        // entries two rows ahead of their use (the arrays end in padding rows, so the reads past a
        // slice's last row are in bounds and nothing is conditional)
#define MGCFD_PRO_PAIR(R)                                                                                      \
        do {                                                                                                   \
            const bool v0 = wa0 != 0.0 || wb0 != 0.0;                                                          \
            const bool v1 = ((R) + 1 < n_int) && (wa1 != 0.0 || wb1 != 0.0);                                   \
            const double *xd0 = cr + (v0 ? sl0 : own_slot) * 5, *xd1 = cr + (v1 ? sl1 : own_slot) * 5;         \
            const double x00 = xd0[0], x01 = xd0[1], x02 = xd0[2], x03 = xd0[3], x04 = xd0[4];                 \
            const double x10 = xd1[0], x11 = xd1[1], x12 = xd1[2], x13 = xd1[3], x14 = xd1[4];                 \
            if (v0) {                                                                                          \
                r0 += wa0 * o0; r1 += wa0 * o1; r2 += wa0 * o2; r3 += wa0 * o3; r4 += wa0 * o4;                \
                r0 += wb0 * x00; r1 += wb0 * x01; r2 += wb0 * x02; r3 += wb0 * x03; r4 += wb0 * x04;           \
            }                                                                                                  \
            if (v1) {                                                                                          \
                r0 += wa1 * o0; r1 += wa1 * o1; r2 += wa1 * o2; r3 += wa1 * o3; r4 += wa1 * o4;                \
                r0 += wb1 * x10; r1 += wb1 * x11; r2 += wb1 * x12; r3 += wb1 * x13; r4 += wb1 * x14;           \
            }                                                                                                  \
        } while (0)
        // every pair but the last prefetches the pair after it (ELL padding carries zero weights)
        int32_t r = 0;
        for (; r + 2 < n_int; r += 2, wr += 256, sr += 128) {
            const double wa2 = wr[256], wb2 = wr[320], wa3 = wr[384], wb3 = wr[448];
            const uint32_t sl2 = sr[128], sl3 = sr[192];
            MGCFD_PRO_PAIR(r);
            wa0 = wa2; wb0 = wb2; wa1 = wa3; wb1 = wb3; sl0 = sl2; sl1 = sl3;
        }
        if (r < n_int) MGCFD_PRO_PAIR(r);
#undef MGCFD_PRO_PAIR
    }
    double sf = __longlong_as_double(0x7FF0000000000000LL);          // +inf
    if (active) {
        const double n0 = pro_result<MODE>(q0, f0, r0 / ws);
        const double n1 = pro_result<MODE>(q1, f1, r1 / ws);
        const double n2 = pro_result<MODE>(q2, f2, r2 / ws);
        const double n3 = pro_result<MODE>(q3, f3, r3 / ws);
        const double n4 = pro_result<MODE>(q4, f4, r4 / ws);
        store_conserved(fine_q, stride, i, n0, n1, n2, n3, n4);
        if (partial_min) sf = local_step_factor(n0, n1, n2, n3, n4, cbrt_vol[i], cfl);
    }
    if (partial_min) block_min_to(sf, partial_min);
}

// ==========================================================================================
// launchers
// ==========================================================================================
// partial_min must hold grid_for(nel) doubles
void launch_step_factor_local(hipStream_t st, int64_t nel, int64_t stride, const double *q, const double *cbrt_vol,
                              double cfl, double *sf, double *partial_min, double *old_variables)
{ hipLaunchKernelGGL(k_step_factor_local, dim3(grid_for(nel)), dim3(kBlock), 0, st, nel, stride, q, cbrt_vol, cfl, sf, partial_min, old_variables); }

void launch_step_factor_apply(hipStream_t st, int64_t nel, const double *min_dt_scalar,
                              const double *volumes, double *sf)
{ hipLaunchKernelGGL(k_step_factor_apply, dim3(grid_for(nel)), dim3(kBlock), 0, st, nel, min_dt_scalar, volumes, sf); }

void launch_step_factor_legacy(hipStream_t st, int64_t nel, int64_t stride, const double *q, const double *volumes, double cfl,
                               double *sf, double *old_variables)
{ hipLaunchKernelGGL(k_step_factor_legacy, dim3(grid_for(nel)), dim3(kBlock), 0, st, nel, stride, q, volumes, cfl, sf, old_variables); }

void launch_step_factor_nodal(hipStream_t st, int64_t nel, int64_t stride, const double *q, const double *cbrt_vol,
                              const double *volumes, double cfl, double *sf, double *old_variables)
{ hipLaunchKernelGGL(k_step_factor_nodal, dim3(grid_for(nel)), dim3(kBlock), 0, st, nel, stride, q, cbrt_vol, volumes, cfl, sf, old_variables); }

// ---- the flux launch: which kernel, which instantiation ------------------------------------------------------------------
// A run-time value as a compile-time constant: f(std::integral_constant<int, V>) for the V of the list that equals v.
template <int... Vs, typename F>
static void with_constant(int v, F &&f)
{ if (!((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...)) throw std::logic_error("no kernel is built for this value"); }
template <typename F>
static void with_bool(bool b, F &&f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
// The three kinds of flux launch as f(FUSE, ACC): a fused stage, '+=' into fluxes[], '='.
template <typename F>
static void with_kind(bool fused, bool accumulate, F &&f)
{
    if (fused) f(std::true_type{}, std::false_type{});
    else if (accumulate) f(std::false_type{}, std::true_type{});
    else f(std::false_type{}, std::false_type{});
}

// What every flux kernel is launched with.
struct FluxLaunch {
    hipStream_t st; const DevicePlan &p; const double *q; const FarField &ff; double *fluxes; int classes; const FusedStep &fs;
    dim3 grid; int64_t nel_arg;         // the launch's workgroups; the nodes it treats as present (FusedStep::nel_active)
};

template <bool LOADK, bool FUSE, bool ACC, int ROLE, bool TAIL, bool PUSH = false, bool SLIM = false>
static void launch_tile(const FluxLaunch &a, const StagePush &push = StagePush{})
{
    const DevicePlan &p = a.p;
    // 3 tiles of 52.4 KiB LDS fit a CU (preprocess.hpp: kTileCap) => at least 3 waves per SIMD wanted (168 registers).  The two long-row instantiations that
    // do not fit them — the kernel-granular '+=' launch and the split sweep's absorbed first stage, both off the sweep path —
    // are built for 2 waves per SIMD instead of spilling 20-36 bytes per lane.  (SLIM: four workgroups of 40,896 B per CU.)
    constexpr int MINW = SLIM ? 4 : ((TAIL && (ACC || ROLE == 5)) ? 2 : 3);
    hipLaunchKernelGGL((k_flux_tile<MINW, LOADK, FUSE, ACC, ROLE, TAIL, PUSH, SLIM>), a.grid, dim3(kBlock), 0, a.st, a.q, p.tile_halo,
                       uint32_t(a.grid.x), p.pad_row, p.stride, a.nel_arg, p.slice_row0, p.rows_int, p.rows_bnd,
                       p.nbr16, p.w, p.tile_ovf_ptr, p.tile_ovf, a.ff, a.fluxes, a.classes, a.fs, p.tail, push);
}

#ifdef MGCFD_ORDER_FREE
// (WIDE: a level with halos beyond the shared table: the kernel's own table of kFreeHaloStride ids per tile, 768 LDS images)
template <bool FUSE, bool ACC, int CAP, bool LONG, bool WIDE = false, int ROLE = -1>
static void launch_free(const FluxLaunch &a)
{
    const DevicePlan &p = a.p;
    hipLaunchKernelGGL((k_flux_free<FUSE, ACC, CAP, LONG, WIDE, ROLE>), a.grid, dim3(kBlock), 0, a.st, a.q, WIDE ? p.free_halo : p.tile_halo, uint32_t(p.n_tiles),
                       p.hr_pad_row, p.stride, p.nel, p.hr_row0, p.hr_code, p.hr_w, p.slice_row0,
                       p.rows_int, p.rows_bnd, p.nbr16, p.w, a.ff, a.fluxes, a.classes, a.fs);
}

// The order-free kernel's role-specialised instantiations know roles 0-3 only; everything else runs its generic epilogue (-1).
static int free_stage_role(const FusedStep &fs, int role)
{
    if (fs.next_legacy_sf) return -1;                   // fvcorr's look-ahead, whatever else the stage does: the generic epilogue
    if (role == 1 && fs.sumsq_partial) return 2;        // sums of squares without residuals[] (a lazy residual): a last stage all the same
    return role;
}

void launch_diag_fast_math(hipStream_t st, int kind, int64_t n, const double *in, double *out)
{ if (n > 0) hipLaunchKernelGGL(k_diag_fast_math, dim3(grid_for(n)), dim3(kBlock), 0, st, kind, n, in, out); }
#endif

// The role of a fused stage (k_flux_tile's ROLE), read off its arguments; a launch that is no stage runs as role 1.
static inline int stage_role(const FusedStep &fs)
{
    if (fs.vin_flux) return 5;
    if (fs.partial_min) return 0;
    if (fs.next_partial_min) return 3;
    if (fs.next_legacy_sf) return 4;
    return fs.residuals ? 2 : 1;
}

// (role 0 takes the sweep's start state from its own record instead of loading old_variables)
static void check_first_stage_input(int role, const double *q, const FusedStep &fs)
{ if (role == 0 && q != fs.old_variables) throw std::logic_error("a first stage whose input is not the sweep's start state"); }

void launch_flux(hipStream_t st, const DevicePlan &p, const double *q, const FarField &ff, double *fluxes,
                 int classes, int accumulate, int variant, const FusedStep *fused, const StagePush *push)
{
    FusedStep fs{};
    if (fused) fs = *fused;
    const bool part = fused && fs.tile_list;                        // part of the level's tiles (node gather only)
    if (part && fs.n_list <= 0) return;
    const FluxLaunch a{st, p, q, ff, fluxes, classes, fs, dim3(part ? fs.n_list : p.n_tiles), (fused && fs.nel_active > 0) ? fs.nel_active : p.nel};
    // fused stages: the role decides which optional paths exist in the launched kernel
    const int role = fused ? stage_role(fs) : 1;
    // levels with long rows (tetrahedral meshes, hubs) run the instantiation that hands them to the workgroup
    const bool tail = p.has_tail && (classes & 1);
    const bool loadk = (variant & 1) == 0;      // odd variants recompute k = -|e|*s*0.5 from the weights
    // a stage that sends its own message (StagePush): fused stages over a tile list, roles 0-4, k streamed or recomputed
    if (push && fused && part && !fs.vin_flux) {
        check_first_stage_input(role, q, fs);
        with_bool(loadk, [&](auto K) { with_bool(tail, [&](auto T) { with_constant<0, 1, 2, 3, 4>(role, [&](auto R) {
            launch_tile<decltype(K)::value, true, false, decltype(R)::value, decltype(T)::value, true>(a, *push);
        }); }); });
        return;
    }
    check_first_stage_input(role, q, fs);
    // variant bit 2: the two-phase design point (never for the fused stages: they keep the flux in registers)
    if ((variant & 4) && !fused && p.edge_flux) {
        if (classes & 1)
            hipLaunchKernelGGL(k_fission_edge_flux, dim3(grid_for(p.n_edges)), dim3(kBlock), 0, st, p.n_edges, p.n_edges_pad, p.stride, q,
                               p.fe_ab, p.fe_w, p.edge_flux);
        with_bool(accumulate != 0, [&](auto A) {
            hipLaunchKernelGGL(k_fission_node_sum<decltype(A)::value>, a.grid, dim3(kBlock), 0, st, p.nel, p.stride, p.n_edges_pad, q, p.slice_row0,
                               p.rows_int, p.rows_bnd, p.row_edge, p.nbr16, p.w, p.edge_flux, ff, fluxes, classes);
        });
        return;
    }
#ifdef MGCFD_ORDER_FREE
    // variant bit 6 (64), this namespace only: order-free accumulation over the half-row plan (k_flux_free)
    // (not for a launch that must leave the ghost slots alone — fs.nel_active, a partitioned level in direct mode: this kernel
    //  writes every node of the level)
    if ((variant & 64) && p.free_rows && (classes & 1) && !(fused && fs.vin_flux) && !part && !(fused && fs.nel_active > 0)) {
        // (four workgroups per CU where every tile's halo fits the smaller LDS image, three otherwise; MGCFD_FREE_WG3=1: always three, for A/B)
        static const bool wg3 = std::getenv("MGCFD_FREE_WG3") && std::atoi(std::getenv("MGCFD_FREE_WG3")) != 0;
        static const bool no_roles = std::getenv("MGCFD_FREE_NO_ROLES") && std::atoi(std::getenv("MGCFD_FREE_NO_ROLES")) != 0;   // (A/B)
        const bool cap4 = p.halo_max <= kFreeCap4 - kTile && !wg3;
        // fused stages of levels on the fast path (halos within the smaller LDS image, at most five half rows per lane): the
        // role-specialised instantiations; fvcorr's look-ahead and every other configuration: the generic epilogue
        // (a first stage with another input than the sweep's start state has been refused above)
        const int role_f = fused ? free_stage_role(fs, role) : -1;
        if (role_f >= 0 && !p.free_wide && cap4 && p.hr_max_rows <= kHalfMaxRows && !no_roles) {
            with_constant<0, 1, 2, 3>(role_f, [&](auto R) { launch_free<true, false, kFreeCap4, false, false, decltype(R)::value>(a); });
            return;
        }
        with_kind(fused, accumulate, [&](auto F, auto A) {
            constexpr bool FUSE = decltype(F)::value, ACC = decltype(A)::value;
            if (p.free_wide) launch_free<FUSE, ACC, kTile + kFreeHaloStride, true, true>(a);
            else with_bool(p.hr_max_rows > kHalfMaxRows, [&](auto L) {
                if (cap4) launch_free<FUSE, ACC, kFreeCap4, decltype(L)::value>(a); else launch_free<FUSE, ACC, kTileCap, decltype(L)::value>(a);
            });
        });
        return;
    }
#endif
#ifndef MGCFD_ORDER_FREE
    // kVariantStageWg4 (the bit-identical stages, solver.cpp): four workgroups per CU with 80-byte records where every tile
    // halo fits kTileCap4 - kTile slots — roles 0-4 of levels without long rows, k recomputed or streamed
    if (fused && (variant & kVariantStageWg4) && stage_wg4_fits(p) && role != 5) {
        with_bool(loadk, [&](auto K) { with_constant<0, 1, 2, 3, 4>(role, [&](auto R) {
            launch_tile<decltype(K)::value, true, false, decltype(R)::value, false, false, true>(a);
        }); });
        return;
    }
#endif
    // the node gather; a launch that is no stage has no role (1)
    with_bool(loadk, [&](auto K) { with_bool(tail, [&](auto T) {
        constexpr bool LOADK = decltype(K)::value, TAIL = decltype(T)::value;
        if (fused) with_constant<0, 1, 2, 3, 4, 5>(role, [&](auto R) { launch_tile<LOADK, true, false, decltype(R)::value, TAIL>(a); });
        else if (accumulate) launch_tile<LOADK, false, true, 1, TAIL>(a);
        else launch_tile<LOADK, false, false, 1, TAIL>(a);
    }); });
}

void launch_indirect_rw(hipStream_t st, const DevicePlan &p, const double *q, double *fluxes, int variant)
{
    // through the flux kernel's LDS tiles where the level allows it (no halo node left outside LDS, no long rows);
    // variant bit 3 (8) forces the plain L1 gather
    if (p.lds_complete && !p.has_tail && !(variant & 8)) {
        with_bool((variant & 1) == 0, [&](auto K) {
            hipLaunchKernelGGL((k_indirect_rw_tile<decltype(K)::value>), dim3(p.n_tiles), dim3(kBlock), 0, st, q, p.tile_halo, uint32_t(p.n_tiles),
                               p.pad_row, p.stride, p.nel, p.slice_row0, p.rows_int, p.nbr16, p.w, fluxes);
        });
        return;
    }
    hipLaunchKernelGGL(k_indirect_rw, dim3(p.n_tiles), dim3(kBlock), 0, st, p.nel, p.stride, q,
                       p.slice_row0, p.rows_int, p.nbr, p.w, fluxes);
}

void launch_time_step(hipStream_t st, int64_t nel, int64_t stride, int j, double *sf, double *fluxes,
                      const double *old_variables, double *q, const int32_t *old_of_new, unsigned long long *err, int check,
                      const double *partial_min, int n_partial, const double *volumes, double *residuals, int zero_fluxes)
{
    const double rk_div = double(3 + 1 - j);    // double(RK+1-j), cfd_loops.cpp:243
    hipLaunchKernelGGL(k_time_step, dim3(grid_for(nel)), dim3(kBlock), 0, st, nel, stride, rk_div, sf, fluxes,
                       old_variables, q, old_of_new, err, check, partial_min, n_partial, volumes, residuals,
                       zero_fluxes);
}

// time_step with a source term: final step factors, fluxes[] left as it is (logically zero afterwards).  F - src where d.order
// is 1 or 2 (0: dual time off, d otherwise unused), + P where forcing is given (a FAS-forced level); one of the two at least.
void launch_time_step_src(hipStream_t st, int64_t nel, int64_t stride, int j, const double *sf, const double *fluxes,
                          const double *forcing, const double *old_variables, double *q, const int32_t *old_of_new,
                          unsigned long long *err, int check, double *residuals, const DualSource &d)
{
    const double rk_div = double(3 + 1 - j);
    with_constant<1, 2, 3, 4, 5>(d.order + (forcing ? 3 : 0), [&](auto c) {
        constexpr int kind = decltype(c)::value;            // SRC + 3 * FORCED
        hipLaunchKernelGGL((k_time_step_src<kind % 3, (kind >= 3)>), dim3(grid_for(nel)), dim3(kBlock), 0, st, nel, stride, rk_div, sf, fluxes,
                           forcing, old_variables, q, old_of_new, err, check, residuals, d);
    });
}

void launch_dual_source(hipStream_t st, int64_t nel, int64_t stride, double *fluxes, const DualSource &d)
{
    with_bool(d.order == 2, [&](auto bdf2) {
        hipLaunchKernelGGL((k_dual_source<decltype(bdf2)::value>), dim3(grid_for(nel)), dim3(kBlock), 0, st, nel, stride, fluxes, d);
    });
}

// one iteration of the residual smoothing: the first forms D on load (a.prev == nullptr), the last applies the update (a.next == nullptr)
void launch_smooth(hipStream_t st, const DevicePlan &p, const SmoothStep &a)
{
    with_bool(a.prev == nullptr, [&](auto first) {
        with_bool(a.next == nullptr, [&](auto last) {
            with_bool(p.has_tail != 0, [&](auto tail) {
                hipLaunchKernelGGL((k_smooth_tile<decltype(first)::value, decltype(last)::value, decltype(tail)::value>), dim3(p.n_tiles), dim3(kBlock), 0, st,
                                   p.tile_halo, uint32_t(p.n_tiles), p.stride, p.nel, p.slice_row0, p.rows_int, p.nbr16, p.tile_ovf_ptr, p.tile_ovf, p.tail, a);
            });
        });
    });
}

// the two launches of the JST dissipation: L, nu, r from W; then fluxes += C
void launch_jst_sensor(hipStream_t st, const DevicePlan &p, const JstStep &a)
{
    with_bool(p.has_tail != 0, [&](auto tail) {
        hipLaunchKernelGGL((k_jst_sensor_tile<decltype(tail)::value>), dim3(p.n_tiles), dim3(kBlock), 0, st,
                           p.tile_halo, uint32_t(p.n_tiles), p.stride, p.nel, p.slice_row0, p.rows_int, p.nbr16, p.tile_ovf_ptr, p.tile_ovf, p.tail, a);
    });
}
void launch_jst_dissipation(hipStream_t st, const DevicePlan &p, const JstStep &a)
{
    with_bool(p.has_tail != 0, [&](auto tail) {
        hipLaunchKernelGGL((k_jst_dissipation_tile<decltype(tail)::value>), dim3(p.n_tiles), dim3(kBlock), 0, st,
                           p.tile_halo, uint32_t(p.n_tiles), p.stride, p.nel, p.slice_row0, p.rows_int, p.nbr16, p.w, p.tile_ovf_ptr, p.tile_ovf, p.tail, a);
    });
}

// the two launches of the viscous terms: S from W; then fluxes[1..4] += V
void launch_viscous_stress(hipStream_t st, const DevicePlan &p, const ViscousStep &a)
{
    // (constant viscosity: the instantiation without the model)
    with_bool(p.has_tail != 0, [&](auto tail) { with_bool(a.model.variable(), [&](auto var) {
        hipLaunchKernelGGL((k_viscous_stress_tile<decltype(tail)::value, decltype(var)::value>), dim3(p.n_tiles), dim3(kBlock), 0, st,
                           p.tile_halo, uint32_t(p.n_tiles), p.stride, p.nel, p.slice_row0, p.rows_int, p.nbr16, p.w, p.tile_ovf_ptr, p.tile_ovf, p.tail, a);
    }); });
}
void launch_viscous_flux(hipStream_t st, const DevicePlan &p, const ViscousStep &a)
{
    with_bool(p.has_tail != 0, [&](auto tail) {
        hipLaunchKernelGGL((k_viscous_flux_tile<decltype(tail)::value>), dim3(p.n_tiles), dim3(kBlock), 0, st,
                           p.tile_halo, uint32_t(p.n_tiles), p.stride, p.nel, p.slice_row0, p.rows_int, p.nbr16, p.w, p.tile_ovf_ptr, p.tile_ovf, p.tail, a);
    });
}

void launch_residual(hipStream_t st, int64_t stride, const double *old_variables, const double *q, double *residuals)
{ hipLaunchKernelGGL(k_residual, dim3(grid_for(stride * 5)), dim3(kBlock), 0, st, stride * 5, old_variables, q, residuals); }

void launch_sumsq(hipStream_t st, int64_t nel, int64_t stride, const double *x, double *partial, int n_partial, double *out,
                  const int32_t *old_of_new, int64_t n_owned)
{
    hipLaunchKernelGGL(k_sumsq, dim3(n_partial), dim3(kBlock), 0, st, nel, stride, x, partial,
                       n_owned < nel ? old_of_new : nullptr, n_owned);
    // (kernels_plain.hip's one definition, whichever flavour this is: additions only — kernel_device.hpp)
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(kBlock), 0, st, SumTask{partial, n_partial, out, nullptr, nullptr, 0});
}

void launch_restrict(hipStream_t st, int64_t nel_coarse, int64_t stride_coarse, int64_t stride_fine,
                     const int32_t *child_ptr, const int32_t *child, const int32_t *child4, const double *fine_q,
                     double *coarse_q, const double *cbrt_vol, double cfl, double *partial_min, const SumTask &rms)
{
    hipLaunchKernelGGL(k_restrict, dim3(grid_for(nel_coarse)), dim3(kBlock), 0, st, nel_coarse, stride_coarse,
                       stride_fine, child_ptr, child, reinterpret_cast<const int4 *>(child4), fine_q, coarse_q, cbrt_vol,
                       cfl, partial_min, rms);
}

// kProResiduals: coarse_a = the coarse residuals, fine_residuals given; kProFas: coarse_a = W0, coarse_q = W, no fine residuals;
// kProState: coarse_a = the coarse state, neither
template <int MODE>
static void launch_prolong_kind(hipStream_t st, const DevicePlan &p, int64_t stride_coarse, const double *coarse_a, const double *coarse_q,
                                const double *fine_residuals, double *fine_q, const double *cbrt_vol, double cfl, double *partial_min)
{
    // grid_for(nel) workgroups: the same partition k_step_factor_local's partial minima use
    if (p.pro_tiled) {
        hipLaunchKernelGGL(k_prolong_tile<MODE>, dim3(grid_for(p.nel)), dim3(kBlock), 0, st, p.nel, p.stride, stride_coarse,
                           p.slice_row0, p.rows_int, p.pro_w, p.pro_s16, p.pro_own16, p.pro_tile_n, p.pro_tile_ids,
                           p.pro_parent, p.pro_wsum, coarse_a, fine_residuals, fine_q, cbrt_vol, cfl, partial_min, coarse_q);
        return;
    }
    hipLaunchKernelGGL(k_prolong<MODE>, dim3(grid_for(p.nel)), dim3(kBlock), 0, st, p.nel, p.stride, stride_coarse,
                       p.slice_row0, p.rows_int, p.pro_w, p.pro_p, p.pro_parent, p.pro_wsum, coarse_a, fine_residuals, fine_q,
                       cbrt_vol, cfl, partial_min, coarse_q);
}
void launch_prolong(hipStream_t st, const DevicePlan &p, int64_t stride_coarse, const double *coarse_residuals,
                    const double *fine_residuals, double *fine_q, const double *cbrt_vol, double cfl, double *partial_min)
{ launch_prolong_kind<kProResiduals>(st, p, stride_coarse, coarse_residuals, nullptr, fine_residuals, fine_q, cbrt_vol, cfl, partial_min); }

// the up leg of a FAS cycle: variables[fine] += 0.0 - wavg(W0 - W) of the coarse level
void launch_prolong_fas(hipStream_t st, const DevicePlan &p, int64_t stride_coarse, const double *coarse_w0, const double *coarse_q,
                        double *fine_q, const double *cbrt_vol, double cfl, double *partial_min)
{ launch_prolong_kind<kProFas>(st, p, stride_coarse, coarse_w0, coarse_q, nullptr, fine_q, cbrt_vol, cfl, partial_min); }

// mgcfd_prolong_state: variables[fine] = 0.0 - (0.0 - wavg(variables[fine + 1])); the fine level is only written
void launch_prolong_state(hipStream_t st, const DevicePlan &p, int64_t stride_coarse, const double *coarse_q, double *fine_q,
                          const double *cbrt_vol, double cfl, double *partial_min)
{ launch_prolong_kind<kProState>(st, p, stride_coarse, coarse_q, nullptr, nullptr, fine_q, cbrt_vol, cfl, partial_min); }

void launch_restrict_fas(hipStream_t st, int64_t nel_coarse, int64_t stride_coarse, int64_t stride_fine, const int32_t *child_ptr,
                         const int32_t *child, const int32_t *child4, const double *fine_q, const double *fine_r, const double *fine_p,
                         double *coarse_q, double *w0, double *qsum)
{
    hipLaunchKernelGGL(k_restrict_fas, dim3(grid_for(nel_coarse)), dim3(kBlock), 0, st, nel_coarse, stride_coarse, stride_fine,
                       child_ptr, child, reinterpret_cast<const int4 *>(child4), fine_q, fine_r, fine_p, coarse_q, w0, qsum);
}

} // namespace MGCFD_KERNEL_NS
} // namespace mgcfd

#if defined(MGCFD_PHASES) && defined(MGCFD_PHASE_EXPORT)
extern "C" void mgcfd_debug_phases(unsigned long long *out, int reset)
{
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(mgcfd::MGCFD_KERNEL_NS::g_phase), sizeof(unsigned long long) * 4096 * 8);
    if (reset) { static unsigned long long z[4096 * 8]; (void)hipMemcpyToSymbol(HIP_SYMBOL(mgcfd::MGCFD_KERNEL_NS::g_phase), z, sizeof(z)); }
}
extern "C" void mgcfd_debug_phase_abs(unsigned long long *out)
{
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(mgcfd::MGCFD_KERNEL_NS::g_phase_abs), sizeof(unsigned long long) * 4096 * 8);
}
#endif
