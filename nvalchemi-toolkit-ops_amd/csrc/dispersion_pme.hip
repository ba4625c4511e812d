// dispersion_pme.hip -- the r^-6 dispersion lattice sum on a mesh (LJ-PME): the k-space operator and the gather.  gfx950, wave64.
// Driver: nvalchemiops/interactions/vdw/pme.py.  The reference package has no counterpart; written from the definitions.
//
// With beta = alpha, b = |k| / (2 beta), f(b) = (1 - 2 b^2) exp(-b^2) + 2 sqrt(pi) b^3 erfc(b) (the f of dispersion_ewald.hip) and W_i(g) the
// order-p B-spline weight of atom i at mesh point g:
//     rho = sum_i c_i W_i,   phi = IFFT_unscaled[D FFT(rho)],   D(m) = -(pi^1.5 beta^3 / (6 V)) f(b_m) / sf^2(m)   over the FULL spectrum
//     E_i = c_i W_i.phi + (beta^6 / 12) c_i^2
// f(0) = 1: the m = 0 element of D IS the k = 0 term of the explicit sum, so nothing is skipped and nothing is added afterwards.  The spread
// is mi_spline_spread (pme.hip) and the transforms are mi_fft_lds or the plans; this file holds what is specific to the r^-6 kernel.
//
//   convolve  grid (DP_VIR_BLOCKS, n_systems), one launch for all systems.  A thread owns a spectrum point of its system: k from
//             2 pi cell^-1 and the Miller indices, then exp, erfc and the sinc product ONCE in fp64, whatever the dtype; the M meshes of the
//             system (1 forward; 2 in the adjoint, the second being the g-weighted one) are multiplied by the same D in a loop.  In place or
//             into a second buffer: a point is read and written by its owner only.  When asked, the same pass sums the six virial words of
//             mesh 0 in fp64,
//               W[a][b] = sum_m h_m |rho_m|^2 (D_m delta_ab + v_m k_a k_b),  v_m = (pi^1.5 beta^3 / (6 V)) 1.5 (exp(-b^2) - sqrt(pi) b erfc(b)) / (beta^2 sf^2)
//             (v = D f'/f / (2 beta |k|) with f' = -6 b exp(-b^2) + 6 sqrt(pi) b^2 erfc(b), written without the division by f and finite at
//             k = 0; h_m the Hermitian weight of the half spectrum), thread sums in stride order, wave butterflies, four wave words added in
//             index order: one block partial per (system, block), no atomics, bit-reproducible.
//   gather    DP_LANES = 8 lanes per atom, lane t owns the x-plane t of the p^3 stencil (t < p) and reads phi -- in the adjoint also phi^g --
//             once per point.  The stencil start, the fractional offset and the 1-D weights and derivatives are fp64 for float32 calls too
//             (the spread of a float32 call runs in fp64 and rounds once, so both sides see the same W): one pass of the B-spline recursion
//             per axis yields all p weights and derivatives, everything unrolled on the order, in registers.  Per (x, y) row the lane forms
//             sum_z phi w_z and sum_z phi w_z' first, so the p^2 inner trips cost two fp64 FMAs per mesh value.  Lane sums by xor butterflies
//             inside the 8-lane group; lane 0 maps the fractional gradient to Cartesian (cit^T) and writes, all in fp64:
//               forward            E_i = c_i s + (beta^6 / 12) c_i^2,  forces_i = -2 c_i grad,  dE/dc_i = 2 s + (beta^6 / 6) c_i
//               weights g, phi^g   forces_i = -(g_i c_i grad + c_i grad^g),  dL/dc_i = g_i s + s^g + g_i (beta^6 / 6) c_i
//             with s = W_i.phi, grad = grad W_i.phi.  c_i = 0 gives exact zeros in energies and forces.  Outputs whose pointer is NULL are
//             not computed.  No LDS, no atomics, no private scratch (DESIGN 3.37 has the register table).
#include "common.h"
#include "pme_kspace.h"

namespace {

#include "pair_row.h"  // mi_block_fold

#define DP_VIR_BLOCKS 128  // blocks per system of the convolve grid = block partials per system of the virial
#define DP_VIR_WORDS 6     // {xx, yy, zz, xy, xz, yz}, the layout of mi_ewald_dispersion_recip_virial
#define DP_LANES 8         // lanes per atom of the gather (orders 4..6: lanes p..7 only take part in the butterflies)
#define DP_SQRT_PI 1.7724538509055159
#define DP_PI_15 5.5683279968317078  // pi^1.5

template <class T> struct DpCplx { T re, im; };

template <class T, bool VIRIAL>
__global__ __launch_bounds__(256) void dp_convolve_kernel(const DpCplx<T>* __restrict__ spec, const T* __restrict__ recip, const T* __restrict__ alpha,
                                                          const T* __restrict__ volume, int B, int M, int nx, int ny, int nz, int order,
                                                          DpCplx<T>* __restrict__ out, double* __restrict__ partial) {
  const int b = blockIdx.y;
  const int nzr = nz / 2 + 1;
  const size_t per = (size_t)nx * ny * nzr;
  double R[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) R[q] = (double)recip[9 * (size_t)b + q];
  const double be = (double)alpha[b];
  const double pref = DP_PI_15 * be * be * be / (6.0 * (double)volume[b]);
  const double inv_2be = 0.5 / be, vscale = 1.5 * pref / (be * be);
  double acc[DP_VIR_WORDS] = {0, 0, 0, 0, 0, 0};
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < per; r += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(r % nzr), j = (int)((r / nzr) % ny), i = (int)(r / ((size_t)nzr * ny));
    const int mx = miller_of(i, nx), my = miller_of(j, ny), mz = k;
    // k_c = sum_d m_d (2 pi cell^-1)[c][d], as pme_convolve_kernel forms it
    double kv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) kv[c] = (double)mx * R[3 * c] + (double)my * R[3 * c + 1] + (double)mz * R[3 * c + 2];
    const double k2 = kv[0] * kv[0] + kv[1] * kv[1] + kv[2] * kv[2];
    const double bb = sqrt(k2) * inv_2be, b2 = bb * bb, eb = exp(-b2), ec = erfc(bb);
    const double f = (1.0 - 2.0 * b2) * eb + 2.0 * DP_SQRT_PI * (b2 * bb) * ec;
    const double inv_sf2 = 1.0 / sf_sq_of<double>(mx, my, mz, nx, ny, nz, order);
    const double D = -pref * f * inv_sf2;
    for (int m = 0; m < M; ++m) {
      const size_t at = ((size_t)m * B + b) * per + r;
      const DpCplx<T> v = spec[at];
      if (VIRIAL && m == 0) {
        const double h = (k == 0 || 2 * k == nz) ? 1.0 : 2.0;
        const double s2 = h * ((double)v.re * (double)v.re + (double)v.im * (double)v.im);
        const double d = D * s2, o = vscale * (eb - DP_SQRT_PI * bb * ec) * inv_sf2 * s2;
        acc[0] += d + o * (kv[0] * kv[0]); acc[1] += d + o * (kv[1] * kv[1]); acc[2] += d + o * (kv[2] * kv[2]);
        acc[3] += o * (kv[0] * kv[1]); acc[4] += o * (kv[0] * kv[2]); acc[5] += o * (kv[1] * kv[2]);
      }
      out[at] = DpCplx<T>{(T)(D * (double)v.re), (T)(D * (double)v.im)};
    }
  }
  if (VIRIAL) {
    __shared__ double part[256 / MI_WAVE][DP_VIR_WORDS];
    mi_block_fold<DP_VIR_WORDS>(acc, part, partial + ((size_t)b * gridDim.x + blockIdx.x) * DP_VIR_WORDS, DP_VIR_WORDS);
  }
}

// w[j] = M_p(x + j), d[j] = M_p'(x + j), j = 0..p-1, for x in [0, 1): one pass of M_q(u) = [u M_{q-1}(u) + (q - u) M_{q-1}(u - 1)] / (q - 1)
// up to q = p - 1, whose level gives the derivative M_p'(u) = M_{p-1}(u) - M_{p-1}(u - 1), then the last step.  Static indices only.
template <int ORDER> __device__ __forceinline__ void dp_spline(double x, double (&w)[ORDER], double (&d)[ORDER]) {
#pragma unroll
  for (int j = 1; j < ORDER; ++j) w[j] = 0.0;
  w[0] = 1.0;
#pragma unroll
  for (int q = 2; q < ORDER; ++q) {
    const double inv = 1.0 / (double)(q - 1);
#pragma unroll
    for (int j = q - 1; j >= 1; --j) w[j] = ((x + (double)j) * w[j] + ((double)(q - j) - x) * w[j - 1]) * inv;
    w[0] = x * w[0] * inv;
  }
  d[0] = w[0];
#pragma unroll
  for (int j = 1; j < ORDER; ++j) d[j] = w[j] - w[j - 1];
  const double inv = 1.0 / (double)(ORDER - 1);
#pragma unroll
  for (int j = ORDER - 1; j >= 1; --j) w[j] = ((x + (double)j) * w[j] + ((double)(ORDER - j) - x) * w[j - 1]) * inv;
  w[0] = x * w[0] * inv;
}

__device__ __forceinline__ int dp_wrap(int i, int n) { return ((i % n) + n) % n; }

// One axis of an atom's stencil, as make_stencil of pme.hip lays it out, in fp64: mesh coordinate mc, base = floor(mc), theta = mc - base,
// off0 = floor(theta - (p - 2) / 2); stencil point t sits at mesh index base + off0 + t and has the spline argument p - 1 + x - t with
// x = theta - (p - 2) / 2 - off0 in [0, 1) (exact), i.e. the weight w[p - 1 - t] of dp_spline.  Returns the mesh index of point 0.
template <int ORDER> __device__ __forceinline__ int dp_axis(double mc, double& x) {
  const double base = floor(mc);
  const double t = (mc - base) - 0.5 * (double)(ORDER - 2), off = floor(t);
  x = t - off;
  return (int)base + (int)off;
}

template <class T, int ORDER, bool ADJ>
__global__ __launch_bounds__(256) void dp_gather_kernel(const T* __restrict__ pos, const T* __restrict__ coef, const double* __restrict__ weights,
                                                        const int* __restrict__ batch_idx, const T* __restrict__ cit, const T* __restrict__ phi,
                                                        const T* __restrict__ phi_g, const T* __restrict__ alpha, int N, int nx, int ny, int nz,
                                                        double* __restrict__ energies, T* __restrict__ forces, double* __restrict__ cgrads) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i0 = t / DP_LANES, tx = t - i0 * DP_LANES;
  const int i = i0 < N ? i0 : N - 1;  // surplus groups of the last block recompute the last atom and do not store
  const int s = batch_idx ? batch_idx[i] : 0;
  double c[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) c[q] = (double)cit[9 * (size_t)s + q];
  const double p[3] = {(double)pos[3 * (size_t)i], (double)pos[3 * (size_t)i + 1], (double)pos[3 * (size_t)i + 2]};
  double frac[3];
  mat3_colvec(c, p, frac);
  double xs[3];
  const int g0x = dp_axis<ORDER>(frac[0] * (double)nx, xs[0]);
  const int g0y = dp_axis<ORDER>(frac[1] * (double)ny, xs[1]);
  const int g0z = dp_axis<ORDER>(frac[2] * (double)nz, xs[2]);
  double wy[ORDER], dy[ORDER], wz[ORDER], dz[ORDER];
  dp_spline<ORDER>(xs[1], wy, dy);
  dp_spline<ORDER>(xs[2], wz, dz);
  int gy[ORDER], gz[ORDER];  // mesh indices of the stencil points: point k has weight index ORDER - 1 - k
#pragma unroll
  for (int k = 0; k < ORDER; ++k) { gy[k] = dp_wrap(g0y + k, ny); gz[k] = dp_wrap(g0z + k, nz); }
  double sP = 0, gP[3] = {0, 0, 0}, sG = 0, gG[3] = {0, 0, 0};
  if (tx < ORDER) {
    double wxs[ORDER], dxs[ORDER];
    dp_spline<ORDER>(xs[0], wxs, dxs);
    double wx = 0, dx = 0;  // the lane's own x-plane: a select chain, never a dynamic index into the register arrays
#pragma unroll
    for (int k = 0; k < ORDER; ++k)
      if (k == ORDER - 1 - tx) { wx = wxs[k]; dx = dxs[k]; }
    const size_t m0 = ((size_t)s * nx + dp_wrap(g0x + tx, nx)) * ny;
#pragma unroll
    for (int ty = 0; ty < ORDER; ++ty) {
      const size_t row = (m0 + gy[ty]) * nz;
      double a0 = 0, a1 = 0, b0 = 0, b1 = 0;  // sum_z phi w_z, sum_z phi w_z' (and of phi^g)
#pragma unroll
      for (int tz = 0; tz < ORDER; ++tz) {
        const double a = (double)phi[row + gz[tz]];
        a0 = fma(a, wz[ORDER - 1 - tz], a0);
        a1 = fma(a, dz[ORDER - 1 - tz], a1);
        if (ADJ) {
          const double g = (double)phi_g[row + gz[tz]];
          b0 = fma(g, wz[ORDER - 1 - tz], b0);
          b1 = fma(g, dz[ORDER - 1 - tz], b1);
        }
      }
      const double wyv = wy[ORDER - 1 - ty], dyv = dy[ORDER - 1 - ty];
      const double ww = wx * wyv, dw = dx * wyv, wd = wx * dyv;
      sP = fma(ww, a0, sP); gP[0] = fma(dw, a0, gP[0]); gP[1] = fma(wd, a0, gP[1]); gP[2] = fma(ww, a1, gP[2]);
      if (ADJ) { sG = fma(ww, b0, sG); gG[0] = fma(dw, b0, gG[0]); gG[1] = fma(wd, b0, gG[1]); gG[2] = fma(ww, b1, gG[2]); }
    }
  }
#pragma unroll
  for (int o = DP_LANES / 2; o > 0; o >>= 1) {
    sP += __shfl_xor(sP, o, DP_LANES);
#pragma unroll
    for (int a = 0; a < 3; ++a) gP[a] += __shfl_xor(gP[a], o, DP_LANES);
    if (ADJ) {
      sG += __shfl_xor(sG, o, DP_LANES);
#pragma unroll
      for (int a = 0; a < 3; ++a) gG[a] += __shfl_xor(gG[a], o, DP_LANES);
    }
  }
  if (tx != 0 || i0 >= N) return;
  // d / d(mesh coordinate) -> d / d(fractional coordinate): times the mesh dimension
  const double dims[3] = {(double)nx, (double)ny, (double)nz};
  const double ci = (double)coef[i], be = (double)alpha[s];
  const double be3 = be * be * be, self = be3 * be3 * (1.0 / 12.0);
  const double gw = ADJ ? weights[i] : 2.0;  // forward: each atom is source and probe
  double sX = gw * sP, gX[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) gX[a] = gw * gP[a] * dims[a];
  if (ADJ) {
    sX += sG;
#pragma unroll
    for (int a = 0; a < 3; ++a) gX[a] += gG[a] * dims[a];
  }
  if (energies) energies[i] = ci * sP + self * (ci * ci);
  if (cgrads) cgrads[i] = sX + (ADJ ? gw : 1.0) * (2.0 * self) * ci;
  if (forces) {
#pragma unroll
    for (int bq = 0; bq < 3; ++bq)  // fractional -> Cartesian: v_cart[b] = sum_a cit[a][b] v_frac[a]
      forces[3 * (size_t)i + bq] = (T)(-ci * (c[bq] * gX[0] + c[3 + bq] * gX[1] + c[6 + bq] * gX[2]));
  }
}

}  // namespace

extern "C" int mi_pme_dispersion_virial_blocks(void) { return DP_VIR_BLOCKS; }

extern "C" int mi_pme_dispersion_convolve(const void* spec, const void* recip_cell, const void* alpha, const void* volume, int n_systems,
                                          int n_meshes, int nx, int ny, int nz, int order, int dtype, void* out, double* virial_partial,
                                          void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(order >= 4 && order <= 6, "spline order must be 4..6");
  MI_REQUIRE(n_systems >= 1 && n_systems <= 65535, "n_systems must be in [1, 65535]");
  MI_REQUIRE(n_meshes >= 1 && n_meshes <= 2, "n_meshes must be 1 (forward) or 2 (adjoint)");
  MI_REQUIRE(nx >= order && ny >= order && nz >= order, "every mesh dimension must be at least the spline order");
  MI_REQUIRE(spec && recip_cell && alpha && volume && out, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(DP_VIR_BLOCKS, n_systems);
  mi_timing_begin("pme_dispersion_convolve", stream);
#define DP_CONVOLVE(T_, V_)                                                                                                                  \
  dp_convolve_kernel<T_, V_><<<grid, 256, 0, st>>>((const DpCplx<T_>*)spec, (const T_*)recip_cell, (const T_*)alpha, (const T_*)volume, n_systems, \
                                                   n_meshes, nx, ny, nz, order, (DpCplx<T_>*)out, virial_partial)
  if (dtype == MI_F32) { if (virial_partial) DP_CONVOLVE(float, true); else DP_CONVOLVE(float, false); }
  else { if (virial_partial) DP_CONVOLVE(double, true); else DP_CONVOLVE(double, false); }
#undef DP_CONVOLVE
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_pme_dispersion_gather(const void* positions, const void* coefficients, const double* weights, const int32_t* batch_idx,
                                        const void* cell_inv_t, const void* phi, const void* phi_g, const void* alpha, int n_atoms, int n_systems,
                                        int nx, int ny, int nz, int order, int dtype, double* energies, void* forces, double* coefficient_grads,
                                        void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(order >= 4 && order <= 6, "spline order must be 4..6");
  MI_REQUIRE(n_systems >= 1 && nx >= order && ny >= order && nz >= order, "every mesh dimension must be at least the spline order");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE((weights == nullptr) == (phi_g == nullptr), "weights and phi_g come together (the adjoint) or not at all");
  if (n_atoms <= 0) return MI_OK;
  MI_REQUIRE(positions && coefficients && cell_inv_t && phi && alpha, "null pointer");
  MI_REQUIRE((long long)n_atoms * DP_LANES <= 2147483647LL - 256, "too many atoms for one launch");
  hipStream_t st = (hipStream_t)stream;
  const int blocks = mi_blocks((long long)n_atoms * DP_LANES, 256);
  mi_timing_begin("pme_dispersion_gather", stream);
#define DP_GATHER(T_, O_, A_)                                                                                                                 \
  dp_gather_kernel<T_, O_, A_><<<blocks, 256, 0, st>>>((const T_*)positions, (const T_*)coefficients, weights, batch_idx, (const T_*)cell_inv_t, \
                                                       (const T_*)phi, (const T_*)phi_g, (const T_*)alpha, n_atoms, nx, ny, nz, energies,    \
                                                       (T_*)forces, coefficient_grads)
#define DP_GATHER_O(T_, A_)                                                       \
  do {                                                                            \
    if (order == 4) DP_GATHER(T_, 4, A_); else if (order == 5) DP_GATHER(T_, 5, A_); else DP_GATHER(T_, 6, A_); \
  } while (0)
  if (dtype == MI_F32) { if (weights) DP_GATHER_O(float, true); else DP_GATHER_O(float, false); }
  else { if (weights) DP_GATHER_O(double, true); else DP_GATHER_O(double, false); }
#undef DP_GATHER_O
#undef DP_GATHER
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}
