// kernels_face_gradient.hip — the kernels of the corrected face gradient with their launchers (kernels_face_gradient.hpp: the
// prototypes in namespace mgcfd).  Compiled ONCE, with -ffp-contract=off, as kernels_plain.hip is: nothing here is ever
// contracted, whichever flavour the solver runs, so what these kernels produce is a bitwise function of their input.
#include "kernel_device.hpp"
#include "kernels_face_gradient.hpp"

namespace mgcfd {

// ------------------------------------------------------------------------------------------
// The corrected face gradient (no reference counterpart; INTEGRATION.md "Corrected face gradients"): the along-edge component
// of the averaged node gradient replaced by the two-point difference, as a CORRECTION added to the stage's fluxes behind
// F = F + V.  Two node-centred gathers over the internal incidence rows in row order, the walk k_jst_dissipation_tile does
// (halo table, nbr16, overflow list, long-row lists; code and weights one row ahead of the sums; n = -2.0 * f), sums started
// at +0.0, one addition per edge; every line of the definition is one IEEE operation.
//   k_face_gradient_nodes_tile        G of (u, v, w, T) as the stress launch forms it, and the node's me and kap (the constants
//                                     without a viscosity model; by the law and the eddy viscosity as it stands behind the
//                                     stress launch otherwise) into g [14][stride].  Stages u, v, w, T (17,920 B).
//   k_face_gradient_correction_tile   per edge t, L from the coordinates, c_phi, the stresses and heat flux of the correction;
//                                     Vc, Wk, Hc per node; fluxes[1..3] += Vc, fluxes[4] = (fluxes[4] + Wk) + Hc.  Stages
//                                     u, v, w, T, g and x: 21 fields of 560 doubles, 94,080 B, one workgroup per CU.
// A halo node beyond the table is read — and derived — from memory.  Pad lanes of the last tile write +0.0 to g.
// ------------------------------------------------------------------------------------------
template <bool TAIL>
__global__ void __launch_bounds__(kBlock, 4)
k_face_gradient_nodes_tile(const int32_t *__restrict__ tile_halo, uint32_t n_tiles, int64_t stride, int64_t nel,
                           const int32_t *__restrict__ slice_row0, const int32_t *__restrict__ rows_int, const uint16_t *__restrict__ nbr16,
                           const double *__restrict__ w, const int32_t *__restrict__ tile_ovf_ptr, const int32_t *__restrict__ tile_ovf,
                           TailPlan tp, FaceGradientStep a)
{
#pragma clang fp contract(off)
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

    double s[12];
#pragma unroll
    for (int f = 0; f < 12; f++) s[f] = 0.0;
    auto add = [&](uint32_t code, double hx, double hy, double hz) {
        const uint32_t sl = code & kT16SlotMask;
        if (sl == kT16Pad) return;
        Primitive ot;
        if (sl >= uint32_t(kTileCap)) ot = primitive_of(a.w, stride, tile_ovf[ovf0 + int32_t(sl) - kTileCap]);
        else { ot.u = rec[0][sl]; ot.v = rec[1][sl]; ot.w = rec[2][sl]; ot.T = rec[3][sl]; }
        const double nx = -2.0 * hx, ny = -2.0 * hy, nz = -2.0 * hz;   // the rows hold -+0.5 e
        const double du = ot.u - me.u, dv = ot.v - me.v, dw = ot.w - me.w, dT = ot.T - me.T;
        s[0] += du * nx; s[1] += du * ny; s[2] += du * nz;
        s[3] += dv * nx; s[4] += dv * ny; s[5] += dv * nz;
        s[6] += dw * nx; s[7] += dw * ny; s[8] += dw * nz;
        s[9] += dT * nx; s[10] += dT * ny; s[11] += dT * nz;
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
    const bool present = i < nel;
    double mu_e = a.mu, kap = a.kappa;
    const ViscosityModel &m = a.model;
    if (m.variable()) {                                                // the stress launch's expressions, mut as that launch left it
        const double mu_i = viscosity_of(m, a.mu, me.T);
        const double mut = m.eddy != 0 ? m.mut[i] : 0.0;
        mu_e = mu_i + mut;
        kap = m.cp * (mu_i / m.prandtl + mut / m.prandtl_t);
    }
#pragma unroll
    for (int f = 0; f < 12; f++) a.g[f * stride + i] = present ? (0.5 * s[f]) / vol : 0.0;
    a.g[12 * stride + i] = present ? mu_e : 0.0;
    a.g[13 * stride + i] = present ? kap : 0.0;
}

constexpr int kFaceFields = 21;                                        // u v w T | G [12] | me kap | x y z

template <bool TAIL>
__global__ void __launch_bounds__(kBlock, 1)
k_face_gradient_correction_tile(const int32_t *__restrict__ tile_halo, uint32_t n_tiles, int64_t stride, int64_t nel,
                                const int32_t *__restrict__ slice_row0, const int32_t *__restrict__ rows_int, const uint16_t *__restrict__ nbr16,
                                const double *__restrict__ w, const int32_t *__restrict__ tile_ovf_ptr, const int32_t *__restrict__ tile_ovf,
                                TailPlan tp, FaceGradientStep a)
{
#pragma clang fp contract(off)
    __shared__ double rec[kFaceFields][kSmoothRow];
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
    struct Node { double f[kFaceFields]; };
    auto load = [&](int64_t n) {
        const Primitive p = primitive_of(a.w, stride, n);
        Node q;
        q.f[0] = p.u; q.f[1] = p.v; q.f[2] = p.w; q.f[3] = p.T;
#pragma unroll
        for (int f = 0; f < 14; f++) q.f[4 + f] = a.g[f * stride + n];
#pragma unroll
        for (int f = 0; f < 3; f++) q.f[18 + f] = a.x[f * stride + n];
        return q;
    };
    auto stage = [&](uint32_t slot, const Node &q) {
#pragma unroll
        for (int f = 0; f < kFaceFields; f++) rec[f][slot] = q.f[f];
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

    double v1 = 0.0, v2 = 0.0, v3 = 0.0, wk = 0.0, hc = 0.0;
    auto add = [&](uint32_t code, double hx, double hy, double hz) {
        const uint32_t s = code & kT16SlotMask;
        if (s == kT16Pad) return;
        Node ot;
        if (s >= uint32_t(kTileCap)) ot = load(tile_ovf[ovf0 + int32_t(s) - kTileCap]);
        else {
#pragma unroll
            for (int f = 0; f < kFaceFields; f++) ot.f[f] = rec[f][s];
        }
        const double dxx = ot.f[18] - me.f[18], dxy = ot.f[19] - me.f[19], dxz = ot.f[20] - me.f[20];
        const double len = sqrt((dxx * dxx + dxy * dxy) + dxz * dxz);
        if (len == 0.0) return;                                        // coincident nodes: the edge contributes nothing
        const double tx = dxx / len, ty = dxy / len, tz = dxz / len;
        const double nx = -2.0 * hx, ny = -2.0 * hy, nz = -2.0 * hz;   // the rows hold -+0.5 e
        double cc[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double gx = 0.5 * (me.f[4 + 3 * k] + ot.f[4 + 3 * k]), gy = 0.5 * (me.f[5 + 3 * k] + ot.f[5 + 3 * k]), gz = 0.5 * (me.f[6 + 3 * k] + ot.f[6 + 3 * k]);
            cc[k] = (ot.f[k] - me.f[k]) / len - ((gx * tx + gy * ty) + gz * tz);
        }
        const double cu = cc[0], cv = cc[1], cw = cc[2], cT = cc[3];
        const double mf = 0.5 * (me.f[16] + ot.f[16]), kf = 0.5 * (me.f[17] + ot.f[17]);
        const double dv = (cu * tx + cv * ty) + cw * tz;
        const double tt = (2.0 / 3.0) * dv;
        const double txx = mf * (2.0 * (cu * tx) - tt), tyy = mf * (2.0 * (cv * ty) - tt), tzz = mf * (2.0 * (cw * tz) - tt);
        const double txy = mf * (cu * ty + cv * tx), txz = mf * (cu * tz + cw * tx), tyz = mf * (cv * tz + cw * ty);
        const double qx = kf * (cT * tx), qy = kf * (cT * ty), qz = kf * (cT * tz);
        const double ub = 0.5 * (me.f[0] + ot.f[0]), vb = 0.5 * (me.f[1] + ot.f[1]), wb = 0.5 * (me.f[2] + ot.f[2]);
        v1 += (txx * nx + txy * ny) + txz * nz;
        v2 += (txy * nx + tyy * ny) + tyz * nz;
        v3 += (txz * nx + tyz * ny) + tzz * nz;
        const double wx = (ub * txx + vb * txy) + wb * txz, wy = (ub * txy + vb * tyy) + wb * tyz, wz = (ub * txz + vb * tyz) + wb * tzz;
        wk += (wx * nx + wy * ny) + wz * nz;
        hc += (qx * nx + qy * ny) + qz * nz;
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
    a.fluxes[3 * stride + i] = a.fluxes[3 * stride + i] + v3; a.fluxes[4 * stride + i] = (a.fluxes[4 * stride + i] + wk) + hc;
}

// ==========================================================================================
// launchers
// ==========================================================================================
void launch_face_gradient_nodes(hipStream_t st, const DevicePlan &p, const FaceGradientStep &a)
{
    if (p.has_tail)
        hipLaunchKernelGGL((k_face_gradient_nodes_tile<true>), dim3(p.n_tiles), dim3(kBlock), 0, st,
                           p.tile_halo, uint32_t(p.n_tiles), p.stride, p.nel, p.slice_row0, p.rows_int, p.nbr16, p.w, p.tile_ovf_ptr, p.tile_ovf, p.tail, a);
    else
        hipLaunchKernelGGL((k_face_gradient_nodes_tile<false>), dim3(p.n_tiles), dim3(kBlock), 0, st,
                           p.tile_halo, uint32_t(p.n_tiles), p.stride, p.nel, p.slice_row0, p.rows_int, p.nbr16, p.w, p.tile_ovf_ptr, p.tile_ovf, p.tail, a);
}
void launch_face_gradient_correction(hipStream_t st, const DevicePlan &p, const FaceGradientStep &a)
{
    if (p.has_tail)
        hipLaunchKernelGGL((k_face_gradient_correction_tile<true>), dim3(p.n_tiles), dim3(kBlock), 0, st,
                           p.tile_halo, uint32_t(p.n_tiles), p.stride, p.nel, p.slice_row0, p.rows_int, p.nbr16, p.w, p.tile_ovf_ptr, p.tile_ovf, p.tail, a);
    else
        hipLaunchKernelGGL((k_face_gradient_correction_tile<false>), dim3(p.n_tiles), dim3(kBlock), 0, st,
                           p.tile_halo, uint32_t(p.n_tiles), p.stride, p.nel, p.slice_row0, p.rows_int, p.nbr16, p.w, p.tile_ovf_ptr, p.tile_ovf, p.tail, a);
}

} // namespace mgcfd
