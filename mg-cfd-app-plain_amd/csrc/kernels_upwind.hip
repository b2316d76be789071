// kernels_upwind.hip — the kernels of the upwind flux with their launchers (kernels_upwind.hpp: the prototypes in namespace
// mgcfd).  Compiled ONCE, with -ffp-contract=off, as kernels_plain.hip is: nothing here is ever contracted, whichever flavour the
// solver runs, so what these kernels produce is a bitwise function of their input.
#include "kernel_device.hpp"
#include "kernels_upwind.hpp"

namespace mgcfd {

// ------------------------------------------------------------------------------------------
// The upwind flux (no reference counterpart; INTEGRATION.md "Upwind fluxes"): Roe's flux-difference splitting on the states
// q = (rho, u, v, w, p) of an internal edge's two ends, on MUSCL levels reconstructed along the edge with the limited Green-Gauss
// gradient.  Node-centred gathers over the internal incidence rows in row order, the walk k_jst_dissipation_tile does (halo
// table, nbr16, overflow list, long-row lists; code and weights one row ahead of the sums; n = -2.0 * f), sums started at +0.0,
// one addition per edge; every line of the definition is one IEEE operation.
//   k_upwind_gradient_tile      pass 1: G, the extrema of q over the node and its neighbours, then (a second walk over the same
//                               ends) psi, and Gl = psi * G.  Stages q [5] and x [3] (35,840 B); p is derived once per slot.
//   k_upwind_flux_tile<MUSCL>   pass 2: qL, qR per edge end, the positivity fallback, the canonical orientation, Roe's flux;
//                               fluxes += U.  First order: stages q [5] (22,400 B).  MUSCL: q, x and Gl, 23 fields of 560
//                               doubles, 103,040 B, one workgroup per CU (as k_face_gradient_correction_tile runs at 94,080 B).
// A halo node beyond the table is read — and derived — from memory.  Pad lanes of the last tile write +0.0 to Gl and psi.
// ------------------------------------------------------------------------------------------
namespace {

// q of node n: velocities by division, p by derive()'s expression
__device__ __forceinline__ void primitive5_of(const double *__restrict__ w, int64_t stride, int64_t n, double *q)
{
    const double rho = w[n];
    const Derived d = derive(rho, w[stride + n], w[2 * stride + n], w[3 * stride + n], w[4 * stride + n]);
    q[0] = rho; q[1] = d.vx; q[2] = d.vy; q[3] = d.vz; q[4] = d.p;
}

// the Euler flux of q through the unit normal nh, with un and the total enthalpy H
__device__ __forceinline__ void normal_flux(const double *q, double hx, double hy, double hz, double *f, double &un, double &H)
{
    const double rho = q[0], u = q[1], v = q[2], w = q[3], p = q[4];
    un = (u * hx + v * hy) + w * hz;
    const double E = p / (kGamma - 1.0) + (0.5 * rho) * ((u * u + v * v) + w * w);
    const double ru = rho * un;
    f[0] = ru;
    f[1] = ru * u + p * hx;
    f[2] = ru * v + p * hy;
    f[3] = ru * w + p * hz;
    f[4] = (E + p) * un;
    H = (E + p) / rho;
}

// Phi(qa, qb, m): Roe's flux through m, in the definition's order of operations
__device__ __forceinline__ void roe_flux(const double *qa, const double *qb, double mx, double my, double mz, double fix, double *phi)
{
    const double area = sqrt((mx * mx + my * my) + mz * mz);
    if (area == 0.0) {
#pragma unroll
        for (int k = 0; k < 5; k++) phi[k] = 0.0;
        return;
    }
    const double hx = mx / area, hy = my / area, hz = mz / area;
    double fa[5], fb[5], una, unb, Ha, Hb;
    normal_flux(qa, hx, hy, hz, fa, una, Ha);
    normal_flux(qb, hx, hy, hz, fb, unb, Hb);
    const double ra = sqrt(qa[0]), rb = sqrt(qb[0]);
    const double den = ra + rb;
    const double ut = (ra * qa[1] + rb * qb[1]) / den, vt = (ra * qa[2] + rb * qb[2]) / den, wt = (ra * qa[3] + rb * qb[3]) / den;
    const double Ht = (ra * Ha + rb * Hb) / den;
    const double q2 = (ut * ut + vt * vt) + wt * wt;
    const double c2 = (kGamma - 1.0) * (Ht - 0.5 * q2);
    const double ct = sqrt(c2);                                        // (c2 <= 0: NaN or zero divisors below; the invalid-state check sees it)
    const double unt = (ut * hx + vt * hy) + wt * hz;
    const double rt = ra * rb;
    const double drho = qb[0] - qa[0], du = qb[1] - qa[1], dv = qb[2] - qa[2], dw = qb[3] - qa[3], dp = qb[4] - qa[4];
    const double dun = (du * hx + dv * hy) + dw * hz;
    double l1 = fabs(unt - ct), l2 = fabs(unt), l3 = fabs(unt + ct);
    const double d = fix * (l2 + ct);
    const double dd = d * d, d2 = 2.0 * d;
    if (l1 < d) l1 = (l1 * l1 + dd) / d2;
    if (l3 < d) l3 = (l3 * l3 + dd) / d2;
    if (l2 < d) l2 = (l2 * l2 + dd) / d2;
    const double rc = rt * ct, t2c = 2.0 * c2;
    const double a1 = (dp - rc * dun) / t2c, a2 = drho - dp / c2, a3 = (dp + rc * dun) / t2c;
    const double k1 = l1 * a1, k2 = l2 * a2, ks = l2 * rt, k3 = l3 * a3;
    double D[5];
    D[0] = (k1 + k2) + k3;
    D[1] = ((k1 * (ut - ct * hx) + k2 * ut) + ks * (du - dun * hx)) + k3 * (ut + ct * hx);
    D[2] = ((k1 * (vt - ct * hy) + k2 * vt) + ks * (dv - dun * hy)) + k3 * (vt + ct * hy);
    D[3] = ((k1 * (wt - ct * hz) + k2 * wt) + ks * (dw - dun * hz)) + k3 * (wt + ct * hz);
    D[4] = ((k1 * (Ht - ct * unt) + k2 * (0.5 * q2)) + ks * (((ut * du + vt * dv) + wt * dw) - unt * dun)) + k3 * (Ht + ct * unt);
#pragma unroll
    for (int k = 0; k < 5; k++) phi[k] = area * (0.5 * (fa[k] + fb[k]) - 0.5 * D[k]);
}

} // namespace

template <bool TAIL>
__global__ void __launch_bounds__(kBlock, 2)
k_upwind_gradient_tile(const int32_t *__restrict__ tile_halo, uint32_t n_tiles, int64_t stride, int64_t nel,
                       const int32_t *__restrict__ slice_row0, const int32_t *__restrict__ rows_int, const uint16_t *__restrict__ nbr16,
                       const double *__restrict__ w, const int32_t *__restrict__ tile_ovf_ptr, const int32_t *__restrict__ tile_ovf,
                       TailPlan tp, UpwindStep a)
{
#pragma clang fp contract(off)
    __shared__ double rec[8][kSmoothRow];                              // rho, u, v, w, p | x, y, z
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
    struct Node { double f[8]; };
    auto load = [&](int64_t n) {
        Node q;
        primitive5_of(a.w, stride, n, q.f);
#pragma unroll
        for (int f = 0; f < 3; f++) q.f[5 + f] = a.x[f * stride + n];
        return q;
    };
    auto stage = [&](uint32_t slot, const Node &q) {
#pragma unroll
        for (int f = 0; f < 8; f++) rec[f][slot] = q.f[f];
    };
    auto fetch = [&](uint32_t s) {
        if (s >= uint32_t(kTileCap)) return load(tile_ovf[ovf0 + int32_t(s) - kTileCap]);
        Node ot;
#pragma unroll
        for (int f = 0; f < 8; f++) ot.f[f] = rec[f][s];
        return ot;
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
    const double vol = a.volumes[i];
    __syncthreads();

    // the first walk: the Green-Gauss sums and the extrema
    double s[15], qmax[5], qmin[5];
#pragma unroll
    for (int f = 0; f < 15; f++) s[f] = 0.0;
#pragma unroll
    for (int v = 0; v < 5; v++) { qmax[v] = me.f[v]; qmin[v] = me.f[v]; }
    auto add = [&](uint32_t code, double hx, double hy, double hz) {
        const uint32_t sl = code & kT16SlotMask;
        if (sl == kT16Pad) return;
        const Node ot = fetch(sl);
        const double nx = -2.0 * hx, ny = -2.0 * hy, nz = -2.0 * hz;   // the rows hold -+0.5 e
#pragma unroll
        for (int v = 0; v < 5; v++) {
            const double dq = ot.f[v] - me.f[v];
            s[3 * v] += dq * nx; s[3 * v + 1] += dq * ny; s[3 * v + 2] += dq * nz;
            if (ot.f[v] > qmax[v]) qmax[v] = ot.f[v];
            if (ot.f[v] < qmin[v]) qmin[v] = ot.f[v];
        }
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
    double G[15], psi[5];
#pragma unroll
    for (int f = 0; f < 15; f++) G[f] = (0.5 * s[f]) / vol;
#pragma unroll
    for (int v = 0; v < 5; v++) psi[v] = 1.0;

    // the second walk over the same ends: the limiter
    if (a.limiter != 0) {
        const bool venkat = a.limiter == 2;
        const double e2 = a.k3 * vol;
        auto limit = [&](uint32_t code) {
            const uint32_t sl = code & kT16SlotMask;
            if (sl == kT16Pad) return;
            double ox, oy, oz;
            if (sl >= uint32_t(kTileCap)) {
                const int64_t n = tile_ovf[ovf0 + int32_t(sl) - kTileCap];
                ox = a.x[n]; oy = a.x[stride + n]; oz = a.x[2 * stride + n];
            } else { ox = rec[5][sl]; oy = rec[6][sl]; oz = rec[7][sl]; }
            const double dx = ox - me.f[5], dy = oy - me.f[6], dz = oz - me.f[7];
#pragma unroll
            for (int v = 0; v < 5; v++) {
                const double d2 = 0.5 * ((G[3 * v] * dx + G[3 * v + 1] * dy) + G[3 * v + 2] * dz);
                double pe = 1.0;
                if (d2 > 0.0 || d2 < 0.0) {
                    const double d1 = (d2 > 0.0 ? qmax[v] : qmin[v]) - me.f[v];
                    if (venkat) {
                        const double d11 = d1 * d1, d22 = (2.0 * d2) * d2;
                        pe = ((d11 + e2) * d2 + d22 * d1) / (d2 * (((d11 + d22) + d1 * d2) + e2));
                    } else {
                        const double r = d1 / d2;
                        pe = r < 1.0 ? r : 1.0;
                    }
                }
                if (pe < psi[v]) psi[v] = pe;
            }
        };
        for (int32_t r = 0; r < n_int; r++) limit(nbr16[(int64_t(row0 + r) << 6) + lane]);
        if (TAIL) {
            for (int32_t k = 0; k < tl_n; k++) {
                const unsigned long long word = static_cast<unsigned long long>(__double_as_longlong(tp.rec[3 * int64_t(tl_b + k) + 2].x));
                limit(static_cast<uint32_t>(word >> 16) & 0xFFFFu);
            }
        }
    }
    const bool present = i < nel;
#pragma unroll
    for (int v = 0; v < 5; v++) {
#pragma unroll
        for (int d = 0; d < 3; d++) a.gl[(3 * v + d) * stride + i] = present ? psi[v] * G[3 * v + d] : 0.0;
        a.psi[v * stride + i] = present ? psi[v] : 0.0;
    }
}

template <bool MUSCL, bool TAIL>
__global__ void __launch_bounds__(kBlock, MUSCL ? 1 : 2)
k_upwind_flux_tile(const int32_t *__restrict__ tile_halo, uint32_t n_tiles, int64_t stride, int64_t nel,
                   const int32_t *__restrict__ slice_row0, const int32_t *__restrict__ rows_int, const uint16_t *__restrict__ nbr16,
                   const double *__restrict__ w, const int32_t *__restrict__ tile_ovf_ptr, const int32_t *__restrict__ tile_ovf,
                   TailPlan tp, UpwindStep a)
{
#pragma clang fp contract(off)
    constexpr int kFields = MUSCL ? 23 : 5;                            // rho u v w p | x y z | Gl [15]
    static_assert(23 * kSmoothRow * 8 == kUpwindMusclLds, "the host asks the device for what the kernel declares");
    __shared__ double rec[kFields][kSmoothRow];
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
    struct Node { double f[kFields]; };
    auto load = [&](int64_t n) {
        Node q;
        primitive5_of(a.w, stride, n, q.f);
        if constexpr (MUSCL) {
#pragma unroll
            for (int f = 0; f < 3; f++) q.f[5 + f] = a.x[f * stride + n];
#pragma unroll
            for (int f = 0; f < 15; f++) q.f[8 + f] = a.gl[f * stride + n];
        }
        return q;
    };
    auto stage = [&](uint32_t slot, const Node &q) {
#pragma unroll
        for (int f = 0; f < kFields; f++) rec[f][slot] = q.f[f];
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

    double u[5];
#pragma unroll
    for (int k = 0; k < 5; k++) u[k] = 0.0;
    auto add = [&](uint32_t code, double hx, double hy, double hz) {
        const uint32_t s = code & kT16SlotMask;
        if (s == kT16Pad) return;
        Node ot;
        if (s >= uint32_t(kTileCap)) ot = load(tile_ovf[ovf0 + int32_t(s) - kTileCap]);
        else {
#pragma unroll
            for (int f = 0; f < kFields; f++) ot.f[f] = rec[f][s];
        }
        const double nx = -2.0 * hx, ny = -2.0 * hy, nz = -2.0 * hz;   // the rows hold -+0.5 e
        double qL[5], qR[5];
#pragma unroll
        for (int v = 0; v < 5; v++) { qL[v] = me.f[v]; qR[v] = ot.f[v]; }
        if constexpr (MUSCL) {
            const double dx = ot.f[5] - me.f[5], dy = ot.f[6] - me.f[6], dz = ot.f[7] - me.f[7];
            double rL[5], rR[5];
#pragma unroll
            for (int v = 0; v < 5; v++) {
                const int g = 8 + 3 * v;
                rL[v] = me.f[v] + 0.5 * ((me.f[g] * dx + me.f[g + 1] * dy) + me.f[g + 2] * dz);
                rR[v] = ot.f[v] - 0.5 * ((ot.f[g] * dx + ot.f[g + 1] * dy) + ot.f[g + 2] * dz);
            }
            // the positivity fallback: the whole edge first order
            if (rL[0] > 0.0 && rL[4] > 0.0 && rR[0] > 0.0 && rR[4] > 0.0) {
#pragma unroll
                for (int v = 0; v < 5; v++) { qL[v] = rL[v]; qR[v] = rR[v]; }
            }
        }
        // the canonical orientation: both ends of the edge evaluate Phi on the same bits
        const bool pos = nx != 0.0 ? nx > 0.0 : (ny != 0.0 ? ny > 0.0 : nz > 0.0);
        double phi[5];
        if (pos) roe_flux(qL, qR, nx, ny, nz, a.entropy_fix, phi);
        else roe_flux(qR, qL, -nx, -ny, -nz, a.entropy_fix, phi);
#pragma unroll
        for (int k = 0; k < 5; k++) u[k] = pos ? u[k] - phi[k] : u[k] + phi[k];   // (fluxes hold minus the outflow, as the reference's)
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
#pragma unroll
    for (int k = 0; k < 5; k++) a.fluxes[k * stride + i] = a.fluxes[k * stride + i] + u[k];
}

// ==========================================================================================
// launchers
// ==========================================================================================
#define MGCFD_UPWIND_LAUNCH(kernel)                                                                                             \
    hipLaunchKernelGGL((kernel), dim3(p.n_tiles), dim3(kBlock), 0, st, p.tile_halo, uint32_t(p.n_tiles), p.stride, p.nel,       \
                       p.slice_row0, p.rows_int, p.nbr16, p.w, p.tile_ovf_ptr, p.tile_ovf, p.tail, a)

void launch_upwind_gradient(hipStream_t st, const DevicePlan &p, const UpwindStep &a)
{
    if (p.has_tail) MGCFD_UPWIND_LAUNCH(k_upwind_gradient_tile<true>);
    else MGCFD_UPWIND_LAUNCH(k_upwind_gradient_tile<false>);
}
void launch_upwind_flux(hipStream_t st, const DevicePlan &p, const UpwindStep &a, bool muscl)
{
    if (muscl) {
        if (p.has_tail) MGCFD_UPWIND_LAUNCH((k_upwind_flux_tile<true, true>));
        else MGCFD_UPWIND_LAUNCH((k_upwind_flux_tile<true, false>));
    } else {
        if (p.has_tail) MGCFD_UPWIND_LAUNCH((k_upwind_flux_tile<false, true>));
        else MGCFD_UPWIND_LAUNCH((k_upwind_flux_tile<false, false>));
    }
}
#undef MGCFD_UPWIND_LAUNCH

} // namespace mgcfd
