// pme_kspace.h -- the per-mesh-point helpers the k-space passes of pme.hip and dispersion_pme.hip share: the Miller index of a natural-order
// slot and the squared B-spline structure factor.  Include after common.h.
#pragma once

template <class T> __device__ __forceinline__ T sinc_pi(T x) {
  if (fabs(x) < T(1e-6)) return T(1);
  const T px = T(3.14159265358979323846) * x;
  return sin(px) / px;
}
__device__ __forceinline__ int miller_of(int i, int n) { return i < (n + 1) / 2 ? i : i - n; }  // fftfreq(n, 1/n)

template <class T> __device__ __forceinline__ T sf_sq_of(int mx, int my, int mz, int nx, int ny, int nz, int expo) {
  // pme_kernels.py:208-225: (sinc sinc sinc)^expo, clamped at 1e-10, squared.  The reference caps the exponent at
  // min(order, 4); the caller passes that for orders <= 4 and the mathematically right `order` for the
  // true order-5/6 splines of this build.
  const T sp = sinc_pi((T)mx / (T)nx) * sinc_pi((T)my / (T)ny) * sinc_pi((T)mz / (T)nz);
  T sf = sp;
  for (int t = 1; t < expo; ++t) sf = sf * sp;
  if (sf < T(1e-10)) sf = T(1e-10);
  return sf * sf;
}
