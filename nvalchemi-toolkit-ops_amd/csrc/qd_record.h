// qd_record.h -- the per-atom record of the kernels that see charges, dipoles and quadrupoles at once (quadrupole.hip, pair_scale.hip), its
// pack kernel and the symmetric 3 x 3 product.  Included inside the anonymous namespace of the translation unit, after common.h.
//
// One 16-word record {x, y, z, q, mu(3), Q(6 unique words of 1/2 (Q + Q^T)), 3 words of padding} per atom, 64 / 128 bytes: a pair loop gathers
// one line (two in fp64) per neighbour and never a second array.
#pragma once

template <class T> struct QdRec {  // 64 / 128 bytes: one line
  T x, y, z, q, mx, my, mz, xx, xy, xz, yy, yz, zz, pad[3];
};

// o = Q v for the six words {xx, xy, xz, yy, yz, zz} of a symmetric Q
__device__ __forceinline__ void qd_matvec(const double s[6], double vx, double vy, double vz, double& ox, double& oy, double& oz) {
  ox = s[0] * vx + s[1] * vy + s[2] * vz;
  oy = s[1] * vx + s[3] * vy + s[4] * vz;
  oz = s[2] * vx + s[4] * vy + s[5] * vz;
}

// OPTIONAL: mu and quad may be NULL (no dipoles, no quadrupoles: zero words)
template <class T, bool OPTIONAL>
__device__ __forceinline__ void qd_pack_atom(const T* __restrict__ pos, const T* __restrict__ q, const T* __restrict__ mu,
                                             const T* __restrict__ quad, int i, QdRec<T>* __restrict__ rec) {
  const size_t n = (size_t)i;
  QdRec<T> r;
  r.x = pos[3 * n]; r.y = pos[3 * n + 1]; r.z = pos[3 * n + 2]; r.q = q[i];
  if (OPTIONAL && !mu) { r.mx = r.my = r.mz = T(0); }
  else { r.mx = mu[3 * n]; r.my = mu[3 * n + 1]; r.mz = mu[3 * n + 2]; }
  if (OPTIONAL && !quad) { r.xx = r.yy = r.zz = r.xy = r.xz = r.yz = T(0); }
  else {
    const T* m = quad + 9 * n;
    r.xx = m[0]; r.yy = m[4]; r.zz = m[8];
    r.xy = T(0.5) * (m[1] + m[3]); r.xz = T(0.5) * (m[2] + m[6]); r.yz = T(0.5) * (m[5] + m[7]);
  }
  r.pad[0] = r.pad[1] = r.pad[2] = T(0);
  rec[i] = r;
}

template <class T>
__global__ void qd_pack_kernel(const T* __restrict__ pos, const T* __restrict__ q, const T* __restrict__ mu, const T* __restrict__ quad, int N,
                               QdRec<T>* __restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  qd_pack_atom<T, false>(pos, q, mu, quad, i, rec);
}

// the same record where the dipoles, the quadrupoles or both are absent (NULL)
template <class T>
__global__ void qd_pack_optional_kernel(const T* __restrict__ pos, const T* __restrict__ q, const T* __restrict__ mu, const T* __restrict__ quad,
                                        int N, QdRec<T>* __restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  qd_pack_atom<T, true>(pos, q, mu, quad, i, rec);
}
