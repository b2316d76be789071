// kernels_sa.hip — the kernels of the Spalart-Allmaras model with their launchers (kernels_sa.hpp: the prototypes in namespace
// mgcfd).  Compiled ONCE, with -ffp-contract=off, as kernels_plain.hip is: nothing here is ever contracted, whichever flavour the
// solver runs, so what these kernels produce is a bitwise function of their input.
#include <type_traits>

#include "kernel_device.hpp"
#include "kernels_sa.hpp"

namespace mgcfd {

// ------------------------------------------------------------------------------------------
// The Spalart-Allmaras model (no reference counterpart; INTEGRATION.md "Spalart-Allmaras model"): nu_tilde, a sixth
// transported quantity beside the state, in the noft2 form with the 2012 limiter of S~.  Two node-centred gathers over the
// internal incidence rows in row order, the walk k_jst_dissipation_tile does (halo table, nbr16, overflow list, long-row
// lists; code and weights one row ahead of the sums; n = -2.0 * f), sums started at +0.0, one addition per edge; every
// line of the definition is one IEEE operation.
//   k_sa_gradient_tile   G of (u, v, w, nt) as the stress launch forms G; om = |curl v|; mut = (rho nt) fv1 -> eddy_viscosity;
//                        sa_gradient = (G[nt], om, nu).  Stages u, v, w, nt (four fields of 560 doubles, 17,920 B).
//   k_sa_transport_tile  Qc (upwind convection), Qd (diffusion on averaged node gradients) per edge; source, point-implicit
//                        destruction and the step per node; nt_out = max(nt_old + dn, +0.0), +0.0 on the wall (d == 0).
//                        Stages u, v, w, nt, nu, G[nt] (eight fields, 35,840 B).
// A halo node beyond the table is read — and derived — from memory.  Pad lanes of the last tile write +0.0.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ double sa_root6(double t)
{
    const double s = sqrt(t);
    double y = __longlong_as_double(__double_as_longlong(s) / 3 + 0x2A9F7893782DA1CELL);
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const double y3 = (y * y) * y;
        y = y * ((y3 + (s + s)) / ((y3 + y3) + s));
    }
    return y;
}
__device__ __forceinline__ double sa_fv1(double chi, double cv1_3)
{
    const double chi3 = (chi * chi) * chi;
    return chi3 / (chi3 + cv1_3);
}

// tanh of z in [0, 20] by a fixed algorithm (INTEGRATION.md "Unsteady Spalart-Allmaras"): exp(z / 512) by its Taylor polynomial
// of degree 8, squared ten times to exp(2 z), then (p - 1) / (p + 1).  No exp on the device.
__device__ __forceinline__ double sa_tanh_fixed(double z)
{
    const double q = z * (1.0 / 512.0);
    double p = 1.0 / 40320.0;
    p = 1.0 / 5040.0 + q * p;
    p = 1.0 / 720.0 + q * p;
    p = 1.0 / 120.0 + q * p;
    p = 1.0 / 24.0 + q * p;
    p = 1.0 / 6.0 + q * p;
    p = 1.0 / 2.0 + q * p;
    p = 1.0 / 1.0 + q * p;
    p = 1.0 + q * p;
#pragma unroll
    for (int k = 0; k < 10; k++) p = p * p;
    return (p - 1.0) / (p + 1.0);
}
// The DES97 length: d~ = min(d, c_des * delta), +0.0 on the wall, lim where d = +inf.
__device__ __forceinline__ double sa_length_des(double d, double lim)
{
    if (d == 0.0) return 0.0;
    return d <= lim ? d : lim;
}

// SHIELD: under delayed DES (mgcfd_set_sa_unsteady with MGCFD_SA_LENGTH_DDES) the three diagonal sums are taken too and the
// shielded length d~ is written per node: STEP = SaStepShielded.  STEP = SaStep is the plain kernel.
template <bool TAIL, bool SHIELD>
__global__ void __launch_bounds__(kBlock, (SHIELD ? 5 : 4))
k_sa_gradient_tile(const int32_t *__restrict__ tile_halo, uint32_t n_tiles, int64_t stride, int64_t nel,
                   const int32_t *__restrict__ slice_row0, const int32_t *__restrict__ rows_int, const uint16_t *__restrict__ nbr16,
                   const double *__restrict__ w, const int32_t *__restrict__ tile_ovf_ptr, const int32_t *__restrict__ tile_ovf,
                   TailPlan tp, std::conditional_t<SHIELD, SaStepShielded, SaStep> a)
{
#pragma clang fp contract(off)
    __shared__ double rec[4][kSmoothRow];                              // u, v, w, nt
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
    struct Node { double u, v, w, nt; };
    auto load = [&](int64_t n) {
        const double rho = a.w[n];
        Node q;
        q.u = a.w[stride + n] / rho; q.v = a.w[2 * stride + n] / rho; q.w = a.w[3 * stride + n] / rho; q.nt = a.nt[n];
        return q;
    };
    auto stage = [&](uint32_t slot, const Node &q) { rec[0][slot] = q.u; rec[1][slot] = q.v; rec[2][slot] = q.w; rec[3][slot] = q.nt; };
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

    double uy = 0.0, uz = 0.0, vx = 0.0, vz = 0.0, wx = 0.0, wy = 0.0, tx = 0.0, ty = 0.0, tz = 0.0;   // (the curl takes the six off-diagonal sums)
    double ux = 0.0, vy = 0.0, wz = 0.0;                               // (SHIELD: the diagonal too)
    auto add = [&](uint32_t code, double hx, double hy, double hz) {
        const uint32_t s = code & kT16SlotMask;
        if (s == kT16Pad) return;
        Node ot;
        if (s >= uint32_t(kTileCap)) ot = load(tile_ovf[ovf0 + int32_t(s) - kTileCap]);
        else { ot.u = rec[0][s]; ot.v = rec[1][s]; ot.w = rec[2][s]; ot.nt = rec[3][s]; }
        const double nx = -2.0 * hx, ny = -2.0 * hy, nz = -2.0 * hz;   // the rows hold -+0.5 e
        const double du = ot.u - me.u, dv = ot.v - me.v, dw = ot.w - me.w, dn = ot.nt - me.nt;
        uy += du * ny; uz += du * nz;
        vx += dv * nx; vz += dv * nz;
        wx += dw * nx; wy += dw * ny;
        tx += dn * nx; ty += dn * ny; tz += dn * nz;
        if constexpr (SHIELD) { ux += du * nx; vy += dv * ny; wz += dw * nz; }
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
    const double guy = (0.5 * uy) / vol, guz = (0.5 * uz) / vol;
    const double gvx = (0.5 * vx) / vol, gvz = (0.5 * vz) / vol;
    const double gwx = (0.5 * wx) / vol, gwy = (0.5 * wy) / vol;
    const double gtx = (0.5 * tx) / vol, gty = (0.5 * ty) / vol, gtz = (0.5 * tz) / vol;
    const double ox = gwy - gvz, oy = guz - gwx, oz = gvx - guy;
    const double om = sqrt((ox * ox + oy * oy) + oz * oz);
    const double rho = a.w[i];
    const Derived dv = derive(rho, a.w[stride + i], a.w[2 * stride + i], a.w[3 * stride + i], a.w[4 * stride + i]);
    const double mu_i = viscosity_of(a.model, a.mu, dv.p / rho);
    const double nu = mu_i / rho;
    const double chi = me.nt / nu;
    const double mut = (rho * me.nt) * sa_fv1(chi, a.cv1_3);
    if constexpr (SHIELD) {
        constexpr double kappa = 0.41;
        const double fv1 = sa_fv1(chi, a.cv1_3);
        const double gux = (0.5 * ux) / vol, gvy = (0.5 * vy) / vol, gwz = (0.5 * wz) / vol;
        const double su = (gux * gux + guy * guy) + guz * guz;
        const double sv = (gvx * gvx + gvy * gvy) + gvz * gvz;
        const double sw = (gwx * gwx + gwy * gwy) + gwz * gwz;
        const double sq = sqrt((su + sv) + sw);
        const double d_i = a.sh.d[i];
        const double lim = a.sh.c_des * a.sh.delta[i];
        const double kd = kappa * d_i;
        const double kd2 = kd * kd;
        const double rd = (me.nt * fv1 + nu) / (sq * kd2);
        const double e = 8.0 * rd;
        double z = (e * e) * e;
        z = z < 20.0 ? z : 20.0;                                       // (inf and NaN give 20.0)
        const double fd = 1.0 - sa_tanh_fixed(z);
        double len;
        if (d_i == 0.0) len = 0.0;
        else if (d_i == __builtin_huge_val()) len = lim;
        else if (d_i <= lim) len = d_i;
        else len = d_i - fd * (d_i - lim);
        a.sh.length[i] = present ? len : 0.0;
    }
    a.grad[i] = present ? gtx : 0.0; a.grad[stride + i] = present ? gty : 0.0; a.grad[2 * stride + i] = present ? gtz : 0.0;
    a.grad[3 * stride + i] = present ? om : 0.0; a.grad[4 * stride + i] = present ? nu : 0.0;
    a.mut[i] = present ? mut : 0.0;
}

template <class STEP> struct sa_timed : std::false_type {};
template <> struct sa_timed<SaStepTimed> : std::true_type {};
template <> struct sa_timed<SaStepCorrectedTimed> : std::true_type {};

// TIMED (STEP = SaStepTimed, SaStepCorrectedTimed): the physical-time source of nt under dual time stepping; the own node's two time
// levels are read from memory behind the sums, nothing more is staged.
// CORR: under the corrected face gradient (mgcfd_set_face_gradient) the coordinates are staged too (eleven fields, 49,280 B) and
// Qdc, the along-edge correction of the diffusion, is summed beside Qd: STEP = SaStepCorrected.  STEP = SaStep is the averaged kernel.
template <bool TAIL, class STEP>
__global__ void __launch_bounds__(kBlock, (std::is_base_of<SaStepCorrected, STEP>::value ? 3 : 4))
k_sa_transport_tile(const int32_t *__restrict__ tile_halo, uint32_t n_tiles, int64_t stride, int64_t nel,
                    const int32_t *__restrict__ slice_row0, const int32_t *__restrict__ rows_int, const uint16_t *__restrict__ nbr16,
                    const double *__restrict__ w, const int32_t *__restrict__ tile_ovf_ptr, const int32_t *__restrict__ tile_ovf,
                    TailPlan tp, STEP a)
{
#pragma clang fp contract(off)
    constexpr bool CORR = std::is_base_of<SaStepCorrected, STEP>::value;
    constexpr bool TIMED = sa_timed<STEP>::value;
    constexpr int NF = CORR ? 11 : 8;
    __shared__ double rec[NF][kSmoothRow];                             // u, v, w, nt, nu, G[nt][x], G[nt][y], G[nt][z] (CORR: x, y, z)
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
    struct Node { double f[NF]; };
    auto load = [&](int64_t n) {
        const double rho = a.w[n];
        Node q;
        q.f[0] = a.w[stride + n] / rho; q.f[1] = a.w[2 * stride + n] / rho; q.f[2] = a.w[3 * stride + n] / rho; q.f[3] = a.nt[n];
        q.f[4] = a.grad[4 * stride + n]; q.f[5] = a.grad[n]; q.f[6] = a.grad[stride + n]; q.f[7] = a.grad[2 * stride + n];
        if constexpr (CORR) { q.f[8] = a.x[n]; q.f[9] = a.x[stride + n]; q.f[10] = a.x[2 * stride + n]; }
        return q;
    };
    auto stage = [&](uint32_t slot, const Node &q) {
#pragma unroll
        for (int f = 0; f < NF; f++) rec[f][slot] = q.f[f];
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

    const double nt_i = me.f[3], nu_i = me.f[4];
    double qc = 0.0, qd = 0.0, qdc = 0.0;
    auto add = [&](uint32_t code, double hx, double hy, double hz) {
        const uint32_t s = code & kT16SlotMask;
        if (s == kT16Pad) return;
        Node ot;
        if (s >= uint32_t(kTileCap)) ot = load(tile_ovf[ovf0 + int32_t(s) - kTileCap]);
        else {
#pragma unroll
            for (int f = 0; f < NF; f++) ot.f[f] = rec[f][s];
        }
        const double nx = -2.0 * hx, ny = -2.0 * hy, nz = -2.0 * hz;   // the rows hold -+0.5 e
        const double ub = 0.5 * (me.f[0] + ot.f[0]), vb = 0.5 * (me.f[1] + ot.f[1]), wb = 0.5 * (me.f[2] + ot.f[2]);
        const double phi = (ub * nx + vb * ny) + wb * nz;
        const double pm = phi < 0.0 ? phi : 0.0;
        qc += pm * (nt_i - ot.f[3]);
        const double nb = 0.5 * ((nu_i + nt_i) + (ot.f[4] + ot.f[3]));
        const double gxb = 0.5 * (me.f[5] + ot.f[5]), gyb = 0.5 * (me.f[6] + ot.f[6]), gzb = 0.5 * (me.f[7] + ot.f[7]);
        qd += nb * ((gxb * nx + gyb * ny) + gzb * nz);
        if constexpr (CORR) {
            const double dxx = ot.f[8] - me.f[8], dxy = ot.f[9] - me.f[9], dxz = ot.f[10] - me.f[10];
            const double len = sqrt((dxx * dxx + dxy * dxy) + dxz * dxz);
            if (len == 0.0) return;                                    // coincident nodes: nothing to Qdc
            const double tx = dxx / len, ty = dxy / len, tz = dxz / len;
            const double cnt = (ot.f[3] - nt_i) / len - ((gxb * tx + gyb * ty) + gzb * tz);
            const double tn = (tx * nx + ty * ny) + tz * nz;
            qdc += nb * (cnt * tn);
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
    if (i >= nel) { a.nt_out[i] = 0.0; return; }
    const double d_i = a.d[i];
    if (d_i == 0.0) { a.nt_out[i] = 0.0; return; }                     // a wall node: Dirichlet
    constexpr double cb1 = 0.1355, cb2 = 0.622, kappa = 0.41, cw2 = 0.3, cv2 = 0.7, cv3 = 0.9, rlim = 10.0;
    const double om = a.grad[3 * stride + i], vol = a.volumes[i];
    const double chi = nt_i / nu_i;
    const double fv1 = sa_fv1(chi, a.cv1_3);
    const double kd = kappa * d_i;
    const double kd2 = kd * kd;
    const double fv2 = 1.0 - chi / (1.0 + chi * fv1);
    const double sb = (nt_i * fv2) / kd2;
    double st;
    if (sb >= -(cv2 * om)) st = om + sb;
    else st = om + (om * ((cv2 * cv2) * om + cv3 * sb)) / ((cv3 - 2.0 * cv2) * om - sb);
    const double den = st * kd2;
    const double r = (den > 0.0 && nt_i < rlim * den) ? nt_i / den : rlim;
    const double r2 = r * r;
    const double r6 = (r2 * r2) * r2;
    const double g = r + cw2 * (r6 - r);
    const double g2 = g * g;
    const double g6 = (g2 * g2) * g2;
    const double fw = g * sa_root6((1.0 + a.c6) / (g6 + a.c6));
    const double nd = nt_i / d_i;
    const double gg = (me.f[5] * me.f[5] + me.f[6] * me.f[6]) + me.f[7] * me.f[7];
    const double src = ((cb1 * st) * nt_i - (a.cw1 * fw) * (nd * nd)) + (cb2 * a.inv_sigma) * gg;
    const double q = (qc + a.inv_sigma * (CORR ? qd + qdc : qd)) + vol * src;
    double jac = ((2.0 * a.cw1) * fw) * (nt_i / (d_i * d_i)) - cb1 * st;
    jac = jac > 0.0 ? jac : 0.0;
    const double cap = (a.cfl_v * a.g[i]) / (a.ks * (nu_i + nt_i));
    const double sf = a.step_factors[i];
    const double sft = cap < sf ? cap : sf;
    const double fac = sft / a.rk_div;
    double dn;
    if constexpr (TIMED) {
        const double ntn = a.t.ntn[i];
        const double ta = nt_i - ntn;
        double ts;
        if (a.t.order == 2) { const double tb = ntn - a.t.ntn1[i]; ts = (3.0 * ta - tb) / (2.0 * a.t.dt); }
        else ts = ta / a.t.dt;
        const double qt = q - vol * ts;
        dn = (fac * qt) / (1.0 + (fac * vol) * (jac + a.t.cj));
    } else dn = (fac * q) / (1.0 + (fac * vol) * jac);
    const double x = a.nt_old[i] + dn;
    a.nt_out[i] = x < 0.0 ? 0.0 : x;                                   // (a NaN stays NaN)
}

// The model on a covered coarse level: nt_I = (sum of the children's nt in ascending fine id) * (1 / count), as k_restrict
// averages a component (a coarse node without children keeps its value), and mut_I = (rho_I nt_I) fv1 from the restricted
// coarse state; one lane per coarse node.
__global__ void __launch_bounds__(kBlock)
k_sa_restrict(int64_t nel_coarse, int64_t stride_coarse, const int32_t *__restrict__ child_ptr, const int32_t *__restrict__ child,
              const double *__restrict__ fine_nt, double *__restrict__ coarse_nt, SaStep a)
{
#pragma clang fp contract(off)
    const int64_t c = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (c >= nel_coarse) return;
    const int32_t b = child_ptr[c], e = child_ptr[c + 1];
    double nt = coarse_nt[c];
    if (e > b) {
        double s = 0.0;
        for (int32_t k = b; k < e; k++) s += fine_nt[child[k]];
        nt = s * (1.0 / double(e - b));
        coarse_nt[c] = nt;
    }
    const double rho = a.w[c];
    const Derived dv = derive(rho, a.w[stride_coarse + c], a.w[2 * stride_coarse + c], a.w[3 * stride_coarse + c], a.w[4 * stride_coarse + c]);
    const double nu = viscosity_of(a.model, a.mu, dv.p / rho) / rho;
    a.mut[c] = (rho * nt) * sa_fv1(nt / nu, a.cv1_3);
}

// nt = nt0 (the host's (ratio * mu) / rho_inf) per node, +0.0 on the wall (d == 0.0), and mut from it with mu_i by the law
// from the level's state.  The whole level; pad lanes +0.0.
__global__ void __launch_bounds__(kBlock)
k_sa_init(int64_t nel, int64_t stride, double nt0, const double *__restrict__ d, double *__restrict__ nt, SaStep a)
{
#pragma clang fp contract(off)
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (i >= stride) return;
    if (i >= nel) { if (d) nt[i] = 0.0; a.mut[i] = 0.0; return; }
    const double rho = a.w[i];
    const Derived dv = derive(rho, a.w[stride + i], a.w[2 * stride + i], a.w[3 * stride + i], a.w[4 * stride + i]);
    const double mu_i = viscosity_of(a.model, a.mu, dv.p / rho);
    const double v = d ? (d[i] == 0.0 ? 0.0 : nt0) : nt[i];          // (d == nullptr: mut of nt as it stands)
    if (d) nt[i] = v;
    a.mut[i] = (rho * v) * sa_fv1(v / (mu_i / rho), a.cv1_3);
}

// d~ of DES97 per node, which is also delayed DES's length until the first pass 1 writes it; pad lanes +0.0.
__global__ void __launch_bounds__(kBlock)
k_sa_length(int64_t nel, int64_t stride, SaShield a)
{
#pragma clang fp contract(off)
    const int64_t i = blockIdx.x * int64_t(kBlock) + threadIdx.x;
    if (i >= stride) return;
    a.length[i] = i < nel ? sa_length_des(a.d[i], a.c_des * a.delta[i]) : 0.0;
}

// ==========================================================================================
// launchers
// ==========================================================================================
void launch_sa_gradient(hipStream_t st, const DevicePlan &p, const SaStep &a, const SaShield *shield)
{
    auto go = [&](auto tail, auto sh, const auto &step) {
        hipLaunchKernelGGL((k_sa_gradient_tile<decltype(tail)::value, decltype(sh)::value>), dim3(p.n_tiles), dim3(kBlock), 0, st,
                           p.tile_halo, uint32_t(p.n_tiles), p.stride, p.nel, p.slice_row0, p.rows_int, p.nbr16, p.w, p.tile_ovf_ptr, p.tile_ovf, p.tail, step);
    };
    if (shield) {                                                      // (delayed DES: d~ beside sa_gradient)
        SaStepShielded c;
        static_cast<SaStep &>(c) = a; c.sh = *shield;
        if (p.has_tail) go(std::true_type{}, std::true_type{}, c); else go(std::false_type{}, std::true_type{}, c);
    } else { if (p.has_tail) go(std::true_type{}, std::false_type{}, a); else go(std::false_type{}, std::false_type{}, a); }
}
void launch_sa_transport(hipStream_t st, const DevicePlan &p, const SaStep &a, const double *x, const SaTime *time)
{
    auto go = [&](const auto &step) {
        auto launch = [&](auto tail) {
            hipLaunchKernelGGL((k_sa_transport_tile<decltype(tail)::value, std::decay_t<decltype(step)>>), dim3(p.n_tiles), dim3(kBlock), 0, st,
                               p.tile_halo, uint32_t(p.n_tiles), p.stride, p.nel, p.slice_row0, p.rows_int, p.nbr16, p.w, p.tile_ovf_ptr, p.tile_ovf, p.tail, step);
        };
        if (p.has_tail) launch(std::true_type{}); else launch(std::false_type{});
    };
    if (x && time) {                                                   // (the corrected face gradient: Qdc beside Qd; the physical-time source)
        SaStepCorrectedTimed c;
        static_cast<SaStep &>(c) = a; c.x = x; c.t = *time;
        go(c);
    } else if (x) {
        SaStepCorrected c;
        static_cast<SaStep &>(c) = a; c.x = x;
        go(c);
    } else if (time) {
        SaStepTimed c;
        static_cast<SaStep &>(c) = a; c.t = *time;
        go(c);
    } else go(a);
}
void launch_sa_length(hipStream_t st, int64_t nel, int64_t stride, const SaShield &a)
{ hipLaunchKernelGGL(k_sa_length, dim3(grid_for(stride)), dim3(kBlock), 0, st, nel, stride, a); }
void launch_sa_restrict(hipStream_t st, int64_t nel_coarse, int64_t stride_coarse, const int32_t *child_ptr, const int32_t *child,
                        const double *fine_nt, double *coarse_nt, const SaStep &a)
{ hipLaunchKernelGGL(k_sa_restrict, dim3(grid_for(nel_coarse)), dim3(kBlock), 0, st, nel_coarse, stride_coarse, child_ptr, child, fine_nt, coarse_nt, a); }
void launch_sa_init(hipStream_t st, int64_t nel, int64_t stride, double nt0, const double *d, double *nt, const SaStep &a)
{ hipLaunchKernelGGL(k_sa_init, dim3(grid_for(stride)), dim3(kBlock), 0, st, nel, stride, nt0, d, nt, a); }

} // namespace mgcfd
