// multipole.hip -- real spherical harmonics and Gaussian-type multipole basis functions up to L = 2.  gfx950, float64.
//
// Counterpart of the reference's math/spherical_harmonics.py and math/gto.py host wrappers (`eval_*_pytorch`); its Warp device functions
// (@wp.func, callable only from other Warp kernels) have no counterpart here.  Written from the closed forms:
//
//   real orthonormal harmonics of the direction r^ = r / |r|, in the order
//     [Y00, Y1-1 (y), Y10 (z), Y1+1 (x), Y2-2 (xy), Y2-1 (yz), Y20 (3 z^2 - r^2), Y2+1 (xz), Y2+2 (x^2 - y^2)]
//     Y00 = 1 / (2 sqrt(pi));  Y1m = sqrt(3 / (4 pi)) {y, z, x} / r;
//     Y2{-2,-1,+1} = (1/2) sqrt(15 / pi) {xy, yz, xz} / r^2;  Y20 = (1/4) sqrt(5 / pi) (3 z^2 - r^2) / r^2;  Y2+2 = (1/4) sqrt(15 / pi) (x^2 - y^2) / r^2
//   1 / r is rsqrt(r^2 + 1e-30) and 1 / r^2 is 1 / (r^2 + 1e-30): every L > 0 value is 0 at the origin, Y00 is a constant.
//   Gradients are the analytic derivatives of Y_lm(r / |r|) with respect to r (singular at the origin; regularised by the same epsilon only).
//   GTO density  sqrt(4 pi) / (2 pi sigma^2)^(3/2) Y_lm(r^) exp(-r^2 / (2 sigma^2))
//   Fourier side exp(-k^2 sigma^2 / 2) times: 1 (L = 0, real part), (1/2) sqrt(4 pi) Y_1m(k^) (L = 1, IMAGINARY part),
//                -(1/4) sqrt(4 pi) Y_2m(k^) (L = 2, real part); the other part is zero.
// One thread per point; the outputs are row-major [n, 1 | 4 | 9] (gradients [n, 1 | 4 | 9, 3]).
#include "common.h"

namespace {

constexpr double MP_EPS = 1e-30;
constexpr double MP_Y00 = 0.28209479177387814;     // 1 / (2 sqrt(pi))
constexpr double MP_Y1 = 0.4886025119029199;       // sqrt(3 / (4 pi))
constexpr double MP_Y2A = 1.0925484305920792;      // (1/2) sqrt(15 / pi): xy, yz, xz
constexpr double MP_Y20 = 0.31539156525252005;     // (1/4) sqrt(5 / pi)
constexpr double MP_Y22 = 0.5462742152960396;      // (1/4) sqrt(15 / pi)
constexpr double MP_SQRT_4PI = 3.5449077018110318;  // sqrt(4 pi)
constexpr double MP_TWO_PI = 6.283185307179586;

__host__ __device__ constexpr int mp_components(int l_max) { return (l_max + 1) * (l_max + 1); }

// y[0 .. (l_max + 1)^2) of the direction of (x, y, z)
__device__ __forceinline__ void sph_harm(double x, double y, double z, int l_max, double* __restrict__ out) {
  out[0] = MP_Y00;
  if (l_max < 1) return;
  const double r2 = x * x + y * y + z * z;
  const double rinv = 1.0 / sqrt(r2 + MP_EPS);
  out[1] = MP_Y1 * y * rinv;
  out[2] = MP_Y1 * z * rinv;
  out[3] = MP_Y1 * x * rinv;
  if (l_max < 2) return;
  const double r2inv = 1.0 / (r2 + MP_EPS);
  out[4] = MP_Y2A * x * y * r2inv;
  out[5] = MP_Y2A * y * z * r2inv;
  out[6] = MP_Y20 * (3.0 * z * z - r2) * r2inv;
  out[7] = MP_Y2A * x * z * r2inv;
  out[8] = MP_Y22 * (x * x - y * y) * r2inv;
}

__global__ __launch_bounds__(256) void sph_harm_kernel(const double* __restrict__ pos, int n, int l_max, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double y[9];
  sph_harm(pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2], l_max, y);
  const int nc = mp_components(l_max);
  double* o = out + (size_t)i * nc;
#pragma unroll
  for (int c = 0; c < 9; ++c)
    if (c < nc) o[c] = y[c];
}

// d/dr of f(r) = p(r) / r^n for a homogeneous polynomial p of degree n: grad p / r^n - n p r / r^(n + 2)
__global__ __launch_bounds__(256) void sph_harm_grad_kernel(const double* __restrict__ pos, int n, int l_max, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = pos[3 * (size_t)i], y = pos[3 * (size_t)i + 1], z = pos[3 * (size_t)i + 2];
  const int nc = mp_components(l_max);
  double* o = out + (size_t)i * nc * 3;
  o[0] = 0.0; o[1] = 0.0; o[2] = 0.0;
  if (l_max < 1) return;
  const double r2 = x * x + y * y + z * z;
  const double r2inv = 1.0 / (r2 + MP_EPS);
  const double rinv = 1.0 / sqrt(r2 + MP_EPS);
  const double rinv3 = rinv * r2inv;
  const double r[3] = {x, y, z};
  const double p1[3] = {y, z, x};       // Y1-1, Y10, Y1+1
  const int axis1[3] = {1, 2, 0};
#pragma unroll
  for (int m = 0; m < 3; ++m)
#pragma unroll
    for (int a = 0; a < 3; ++a) o[3 * (1 + m) + a] = MP_Y1 * ((a == axis1[m] ? rinv : 0.0) - p1[m] * r[a] * rinv3);
  if (l_max < 2) return;
  const double r4inv = r2inv * r2inv;
  // polynomial p and its gradient for the five L = 2 functions (Y20 is written as 3 z^2 / r^2 - 1)
  const double coef[5] = {MP_Y2A, MP_Y2A, MP_Y20, MP_Y2A, MP_Y22};
  const double p2[5] = {x * y, y * z, 3.0 * z * z, x * z, x * x - y * y};
  const double g2[5][3] = {{y, x, 0.0}, {0.0, z, y}, {0.0, 0.0, 6.0 * z}, {z, 0.0, x}, {2.0 * x, -2.0 * y, 0.0}};
#pragma unroll
  for (int m = 0; m < 5; ++m)
#pragma unroll
    for (int a = 0; a < 3; ++a) o[3 * (4 + m) + a] = coef[m] * (g2[m][a] * r2inv - 2.0 * p2[m] * r[a] * r4inv);
}

__global__ __launch_bounds__(256) void gto_density_kernel(const double* __restrict__ pos, int n, double sigma, int l_max, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = pos[3 * (size_t)i], y = pos[3 * (size_t)i + 1], z = pos[3 * (size_t)i + 2];
  double yl[9];
  sph_harm(x, y, z, l_max, yl);
  const double s2 = sigma * sigma;
  const double norm = MP_SQRT_4PI / (MP_TWO_PI * s2 * sqrt(MP_TWO_PI * s2));
  const double radial = norm * exp(-(x * x + y * y + z * z) / (2.0 * s2));
  const int nc = mp_components(l_max);
  double* o = out + (size_t)i * nc;
#pragma unroll
  for (int c = 0; c < 9; ++c)
    if (c < nc) o[c] = yl[c] * radial;
}

__global__ __launch_bounds__(256) void gto_fourier_kernel(const double* __restrict__ kvec, int n, double sigma, int l_max, double* __restrict__ re,
                                                          double* __restrict__ im) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = kvec[3 * (size_t)i], y = kvec[3 * (size_t)i + 1], z = kvec[3 * (size_t)i + 2];
  double yl[9];
  sph_harm(x, y, z, l_max, yl);
  const double g = exp(-0.5 * (x * x + y * y + z * z) * sigma * sigma);
  const int nc = mp_components(l_max);
  double* r = re + (size_t)i * nc;
  double* m = im + (size_t)i * nc;
#pragma unroll
  for (int c = 0; c < 9; ++c)
    if (c < nc) {
      r[c] = c == 0 ? g : (c < 4 ? 0.0 : -0.25 * MP_SQRT_4PI * yl[c] * g);
      m[c] = (c >= 1 && c < 4) ? 0.5 * MP_SQRT_4PI * yl[c] * g : 0.0;
    }
}

}  // namespace

extern "C" {

int mi_sph_harm(const double* positions, int n, int l_max, double* out, void* stream) {
  MI_REQUIRE(l_max >= 0 && l_max <= 2, "L_max must be 0, 1 or 2");
  if (n <= 0) return MI_OK;
  MI_REQUIRE(positions && out, "null pointer");
  mi_timing_begin("sph_harm", stream);
  sph_harm_kernel<<<mi_blocks(n, 256), 256, 0, (hipStream_t)stream>>>(positions, n, l_max, out);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_sph_harm_grad(const double* positions, int n, int l_max, double* out, void* stream) {
  MI_REQUIRE(l_max >= 0 && l_max <= 2, "L_max must be 0, 1 or 2");
  if (n <= 0) return MI_OK;
  MI_REQUIRE(positions && out, "null pointer");
  mi_timing_begin("sph_harm_grad", stream);
  sph_harm_grad_kernel<<<mi_blocks(n, 256), 256, 0, (hipStream_t)stream>>>(positions, n, l_max, out);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_gto_density(const double* positions, int n, double sigma, int l_max, double* out, void* stream) {
  MI_REQUIRE(l_max >= 0 && l_max <= 2, "L_max must be 0, 1 or 2");
  MI_REQUIRE(sigma > 0.0, "sigma must be positive");
  if (n <= 0) return MI_OK;
  MI_REQUIRE(positions && out, "null pointer");
  mi_timing_begin("gto_density", stream);
  gto_density_kernel<<<mi_blocks(n, 256), 256, 0, (hipStream_t)stream>>>(positions, n, sigma, l_max, out);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_gto_fourier(const double* k_vectors, int n, double sigma, int l_max, double* out_real, double* out_imag, void* stream) {
  MI_REQUIRE(l_max >= 0 && l_max <= 2, "L_max must be 0, 1 or 2");
  MI_REQUIRE(sigma > 0.0, "sigma must be positive");
  if (n <= 0) return MI_OK;
  MI_REQUIRE(k_vectors && out_real && out_imag, "null pointer");
  mi_timing_begin("gto_fourier", stream);
  gto_fourier_kernel<<<mi_blocks(n, 256), 256, 0, (hipStream_t)stream>>>(k_vectors, n, sigma, l_max, out_real, out_imag);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

}  // extern "C"
