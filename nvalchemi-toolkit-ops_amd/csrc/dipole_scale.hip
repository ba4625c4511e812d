// dipole_scale.hip -- scaled, Thole-damped bonded pairs of point dipoles: what the direct-field and mutual scale factors of a polarisable
// force field add to the unscaled charge-dipole and dipole-dipole energy, and the same pairs as a second small stored operator beside the
// 44-byte one of induced.hip.  gfx950, wave64.
//
// Every stored entry e = (i, j, S) of a FULL list carries two scales, s^d_e on the charge-dipole term and s^m_e on the dipole-dipole term
// (both symmetric).  With R, r, B1 = 1 / r^3, B2 = 3 / r^5, B3 = 15 / r^7 of pair_scale.hip, c_i = mu_i . R, d = mu_i . mu_j,
// A_q = q_j c_i - q_i c_j and the damping factors of dp_pair_kernel's Thole kind (dipole.hip), E = a_T r^3 / sqrt(a_i a_j),
//     l3 = 1 - e^-E,   l5 = 1 - (1 + E) e^-E,   l7 = 1 - (1 + E + 3/5 E^2) e^-E,      G1 = l3 B1, G2 = l5 B2, G3 = l7 B3
// (l = 1 without a Thole width, when either end has a <= 0 or NaN, and for E >= 50, which leaves before the exp):
//     U        = (s^d - 1) G1 A_q + (s^m - 1) (G1 d - G2 c_i c_j),                 E_i = 1/2 sum_{row i} U
//     dU/dR    = (s^d - 1) [-G2 A_q R + G1 (q_j mu_i - q_i mu_j)] + (s^m - 1) [(G3 c_i c_j - G2 d) R - G2 (c_j mu_i + c_i mu_j)]
//     dU/dq_i  = -(s^d - 1) G1 c_j
//     dU/dmu_i = (s^d - 1) G1 q_j R + (s^m - 1) (G1 mu_j - G2 c_j R)                                              (no mu_i in it)
//     E dU/dE  = (s^d - 1) B1 E e^-E A_q + (s^m - 1) (B1 E e^-E d - B2 E^2 e^-E c_i c_j),     dL/da_i = -1 / (2 a_i) sum_row w E dU/dE
// G_{n+1} = -(1/r) dG_n/dr as for the B_n, which is what the R derivative uses.  An entry with s^d = s^m = 1 leaves before any arithmetic.
//
// Execution shape: that of pair_scale.hip.  One group of DS_GROUP = 8 lanes owns a row (8 rows per wave64, 32 per 256-thread block), the
// lanes stride the row's entries, three butterfly steps sum the group and its lane 0 alone writes.  The group walk is a second copy of the
// one in pair_scale.hip and not a shared header: that file's instantiations keep their code as it is.  The per-atom record is the 8-word
// {x, y, z, q, mu, a} (32 / 64 bytes: one gather of one or two 32-byte sectors per neighbour, against four scattered reads from the caller's
// arrays), packed by a block-parallel pre-pass.  Pair vector and r^2 in the positions dtype (minimum image: reduced in fp64, rounded once),
// everything else fp64.  No atomics, fixed summation orders, plain vector stores: every output is bit-reproducible.  The kernel is its own
// adjoint: with per-atom weights g an entry weighs (g_i + g_j) / 2.
//
// Stored operator.  ds_tensor_kernel (once per geometry) writes, for every slot of a bonded MATRIX list, the neighbour index and
// {c1 = (s^m - 1) G1, c2 = (s^m - 1) G2, R_x, R_y, R_z} in the six-stream layout of induced.hip; padding, skipped entries, s^m = 1 and a
// non-polarisable end hold zeros and the row's own index.  ds_apply_kernel forms y_i = y_in,i + sum_row (c1 x_j - c2 (R . x_j) R) with the same
// 8 lanes per row, in fp64, without a transcendental; its output is the y_in of mi_induced_apply.
#include "common.h"

namespace {

#include "pair_row.h"

#define DS_GROUP 8  // lanes per row
#define DS_ROWS (256 / DS_GROUP)
#define DS_VIR_WORDS 9
#define DS_TENSOR_WORDS 5
#define DS_THOLE_EXIT 50.0

template <class T> struct DsRec {  // 32 / 64 bytes
  T x, y, z, q, mx, my, mz, a;
};

template <class T>
__global__ void ds_pack_kernel(const T* __restrict__ pos, const T* __restrict__ q, const T* __restrict__ mu, const T* __restrict__ polar, int N,
                               DsRec<T>* __restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  DsRec<T> r;
  r.x = pos[3 * (size_t)i]; r.y = pos[3 * (size_t)i + 1]; r.z = pos[3 * (size_t)i + 2]; r.q = q[i];
  r.mx = mu[3 * (size_t)i]; r.my = mu[3 * (size_t)i + 1]; r.mz = mu[3 * (size_t)i + 2];
  r.a = polar ? polar[i] : T(0);
  rec[i] = r;
}

template <class V> __device__ __forceinline__ V ds_group_sum(V v) {
#pragma unroll
  for (int o = DS_GROUP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, MI_WAVE);
  return v;
}

// the cell of system s and its inverse in fp64, and the minimum image of (ex, ey, ez)
struct DsImage {
  double cd[9], ci[9];
  template <class T> __device__ __forceinline__ void load(const T* __restrict__ cell, int s) {
#pragma unroll
    for (int k = 0; k < 9; ++k) cd[k] = (double)cell[9 * (size_t)s + k];
    inverse3(cd, ci);
  }
  __device__ __forceinline__ void reduce(double& ex, double& ey, double& ez) const {
    const double n0 = rint(ex * ci[0] + ey * ci[3] + ez * ci[6]);
    const double n1 = rint(ex * ci[1] + ey * ci[4] + ez * ci[7]);
    const double n2 = rint(ex * ci[2] + ey * ci[5] + ez * ci[8]);
    ex -= n0 * cd[0] + n1 * cd[3] + n2 * cd[6];
    ey -= n0 * cd[1] + n1 * cd[4] + n2 * cd[7];
    ez -= n0 * cd[2] + n1 * cd[5] + n2 * cd[8];
  }
};

// FV: forces or virial are wanted (l7 and B3 are compiled in only then).  MIN: minimum image.  THOLE: a width was given (the exp lives here).
template <class T, bool CSR, bool FV, bool MIN, bool THOLE>
__global__ __launch_bounds__(256, 2) void ds_pair_kernel(const DsRec<T>* __restrict__ rec, const T* __restrict__ cell,
                                                         const int* __restrict__ batch_idx, const double* __restrict__ g, int N,
                                                         const int* __restrict__ idx, const double* __restrict__ sdir,
                                                         const double* __restrict__ smut, const int* __restrict__ ush,
                                                         const int* __restrict__ nptr, int M, int mask_value, int flags, double width,
                                                         double* __restrict__ energies, T* __restrict__ forces, double* __restrict__ cgrad,
                                                         double* __restrict__ dgrad, double* __restrict__ pgrad, double* __restrict__ trow) {
  const int gl = threadIdx.x & (DS_GROUP - 1);
  const long long row = (long long)blockIdx.x * DS_ROWS + threadIdx.x / DS_GROUP;
  const bool live = row < N;
  const int i = live ? (int)row : 0;
  const bool wf = FV && (flags & MI_DP_FORCES) != 0, wv = FV && (flags & MI_DP_VIRIAL) != 0;
  const bool wc = (flags & MI_DP_CHARGE_GRAD) != 0, wd = (flags & MI_DP_DIPOLE_GRAD) != 0;
  const bool wp = (flags & MI_DP_POLAR_GRAD) != 0;
  long long beg = 0, end = 0;
  if (live) pair_row_range<CSR>(nptr, i, M, beg, end);
  double eacc = 0.0, cgi = 0.0, pacc = 0.0, fx = 0.0, fy = 0.0, fz = 0.0, dx_ = 0.0, dy_ = 0.0, dz_ = 0.0;
  double t[DS_VIR_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double ai = 0.0;
  if (__any(end > beg)) {  // wave-uniform: a wave without an entry goes straight to its zeros
    const bool shifted = !MIN && ush != nullptr;
    const int s = (live && batch_idx) ? batch_idx[i] : 0;
    T cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    DsImage im = {};
    if (shifted) pair_row_cell(cell, s, cm);
    if constexpr (MIN) im.load(cell, s);
    DsRec<T> ri = {};
    if (live) ri = rec[i];
    const double qi = (double)ri.q, mix = (double)ri.mx, miy = (double)ri.my, miz = (double)ri.mz;
    ai = (double)ri.a;
    const double gi = (g && live) ? g[i] : 1.0;
    for (long long e = beg + gl; e < end; e += DS_GROUP) {
      const int j = idx[e];
      if (pair_is_padding<CSR>(j, mask_value, N)) continue;
      const double sd1 = sdir ? sdir[e] - 1.0 : 0.0, sm1 = smut ? smut[e] - 1.0 : 0.0;
      if (sd1 == 0.0 && sm1 == 0.0) continue;  // an unscaled pair: exactly nothing
      const DsRec<T> rj = rec[j];
      T sx, sy, sz;
      if constexpr (MIN) {
        double ex = (double)rj.x - (double)ri.x, ey = (double)rj.y - (double)ri.y, ez = (double)rj.z - (double)ri.z;
        im.reduce(ex, ey, ez);
        sx = (T)ex; sy = (T)ey; sz = (T)ez;  // rounded once to the positions dtype
      } else {
        sx = rj.x - ri.x; sy = rj.y - ri.y; sz = rj.z - ri.z;
        if (shifted) {
          T sh[3];
          pair_separation(ush, e, cm, sh);
          sx += sh[0]; sy += sh[1]; sz += sh[2];
        }
      }
      const T r2t = sx * sx + sy * sy + sz * sz;
      const double dist = (double)sqrt(r2t);  // the distance is a quantity of the positions dtype
      if (!(dist > 1e-8)) continue;           // (NaN distances leave here too)
      const double rinv = 1.0 / dist, rinv2 = rinv * rinv;
      const double b1 = rinv * rinv2, b2 = 3.0 * b1 * rinv2;
      double g1 = b1, g2 = b2, l7 = 1.0, x1 = 0.0, x2 = 0.0;  // x1 = B1 E e^-E, x2 = B2 E^2 e^-E
      if constexpr (THOLE) {
        const double aj = (double)rj.a;
        if (ai > 0.0 && aj > 0.0) {
          const double big = width * (dist * dist * dist) / sqrt(ai * aj);
          if (big < DS_THOLE_EXIT) {
            const double ex = exp(-big);
            g1 = (1.0 - ex) * b1;
            g2 = (1.0 - (1.0 + big) * ex) * b2;
            l7 = 1.0 - (1.0 + big + 0.6 * big * big) * ex;
            x1 = big * ex * b1; x2 = big * big * ex * b2;
          }
        }
      }
      const double rx = (double)sx, ry = (double)sy, rz = (double)sz;
      const double qj = (double)rj.q, mjx = (double)rj.mx, mjy = (double)rj.my, mjz = (double)rj.mz;
      const double ci = mix * rx + miy * ry + miz * rz, cj = mjx * rx + mjy * ry + mjz * rz;
      const double aq = qj * ci - qi * cj, d = mix * mjx + miy * mjy + miz * mjz;
      const double cc = ci * cj;
      eacc += 0.5 * (sd1 * g1 * aq + sm1 * (g1 * d - g2 * cc));
      const double w = g ? 0.5 * (gi + g[j]) : 1.0;
      const double wd1 = w * sd1, wm1 = w * sm1;
      if (wc) cgi -= wd1 * g1 * cj;
      if (wd) {
        const double u = wd1 * g1 * qj - wm1 * g2 * cj, v = wm1 * g1;
        dx_ += u * rx + v * mjx; dy_ += u * ry + v * mjy; dz_ += u * rz + v * mjz;
      }
      if constexpr (THOLE) {
        if (wp) pacc += wd1 * x1 * aq + wm1 * (x1 * d - x2 * cc);
      }
      if constexpr (FV) {
        if (wf || wv) {
          const double g3 = l7 * 5.0 * b2 * rinv2;
          const double cr = wm1 * (g3 * cc - g2 * d) - wd1 * g2 * aq;
          const double cmi = wd1 * g1 * qj - wm1 * g2 * cj, cmj = -(wd1 * g1 * qi + wm1 * g2 * ci);
          const double ux = cr * rx + cmi * mix + cmj * mjx, uy = cr * ry + cmi * miy + cmj * mjy, uz = cr * rz + cmi * miz + cmj * mjz;
          fx += ux; fy += uy; fz += uz;
          if (wv) {
            t[0] -= 0.5 * ux * rx; t[1] -= 0.5 * ux * ry; t[2] -= 0.5 * ux * rz;
            t[3] -= 0.5 * uy * rx; t[4] -= 0.5 * uy * ry; t[5] -= 0.5 * uy * rz;
            t[6] -= 0.5 * uz * rx; t[7] -= 0.5 * uz * ry; t[8] -= 0.5 * uz * rz;
          }
        }
      }
    }
    // every lane of the wave is back here: the butterflies stay inside the groups
    if (energies) eacc = ds_group_sum(eacc);
    if (wf) { fx = ds_group_sum(fx); fy = ds_group_sum(fy); fz = ds_group_sum(fz); }
    if (wc) cgi = ds_group_sum(cgi);
    if (wd) { dx_ = ds_group_sum(dx_); dy_ = ds_group_sum(dy_); dz_ = ds_group_sum(dz_); }
    if (THOLE && wp) pacc = ds_group_sum(pacc);
    if (wv) {
#pragma unroll
      for (int k = 0; k < DS_VIR_WORDS; ++k) t[k] = ds_group_sum(t[k]);
    }
  }
  if (!live || gl != 0) return;
  const size_t n = (size_t)i;
  if (energies) energies[n] = eacc;
  if (wf) { forces[3 * n] = (T)fx; forces[3 * n + 1] = (T)fy; forces[3 * n + 2] = (T)fz; }
  if (wc) cgrad[n] = cgi;
  if (wd) { dgrad[3 * n] = dx_; dgrad[3 * n + 1] = dy_; dgrad[3 * n + 2] = dz_; }
  if (wp) pgrad[n] = (THOLE && ai > 0.0) ? -0.5 * pacc / ai : 0.0;
  if (wv) {
    double* o = trow + DS_VIR_WORDS * n;
#pragma unroll
    for (int k = 0; k < DS_VIR_WORDS; ++k) o[k] = t[k];
  }
}

// per-system fold of the per-row virials: partial[s][x][0..9) with plain stores; the caller sums the MI_FOLD_BLOCKS rows.  No atomics.
__global__ __launch_bounds__(256) void ds_fold_kernel(const double* __restrict__ trow, const int* __restrict__ batch_idx, int N,
                                                      double* __restrict__ partial) {
  mi_system_fold<DS_VIR_WORDS, MI_FOLD_BLOCKS>(batch_idx, N, DS_VIR_WORDS, partial, [&](long long r, double* a) {
#pragma unroll
    for (int k = 0; k < DS_VIR_WORDS; ++k) a[k] += trow[DS_VIR_WORDS * r + k];
  });
}

// the stored bonded operator of a matrix list [N, M]: group lanes stride the row's slots and every slot is written
template <class T, bool MIN, bool THOLE>
__global__ __launch_bounds__(256) void ds_tensor_kernel(const T* __restrict__ pos, const T* __restrict__ polar, const T* __restrict__ cell,
                                                        const int* __restrict__ batch_idx, int N, const int* __restrict__ idx,
                                                        const double* __restrict__ smut, int M, int mask_value, long long slots, double width,
                                                        double* __restrict__ ten, int* __restrict__ nbr) {
  const int gl = threadIdx.x & (DS_GROUP - 1);
  const long long row = (long long)blockIdx.x * DS_ROWS + threadIdx.x / DS_GROUP;
  if (row >= N) return;
  const int i = (int)row;
  const T pix = pos[3 * (size_t)i], piy = pos[3 * (size_t)i + 1], piz = pos[3 * (size_t)i + 2];
  const T ai = polar[i];
  const bool pol_i = ai > T(0);  // (NaN: not polarisable)
  DsImage im = {};
  if constexpr (MIN) im.load(cell, batch_idx ? batch_idx[i] : 0);
  const long long beg = (long long)i * M, end = beg + M;
  for (long long e = beg + gl; e < end; e += DS_GROUP) {
    const int j = idx[e];
    double c1 = 0.0, c2 = 0.0, rx = 0.0, ry = 0.0, rz = 0.0;
    int jj = i;  // padding and skipped entries: zero coefficients on the row's own index
    T aj = T(0);
    double sm1 = 0.0;
    if (pol_i && !pair_is_padding<false>(j, mask_value, N) && (sm1 = smut[e] - 1.0) != 0.0 && (aj = polar[j]) > T(0)) {
      T sx, sy, sz;
      if constexpr (MIN) {
        double ex = (double)pos[3 * (size_t)j] - (double)pix, ey = (double)pos[3 * (size_t)j + 1] - (double)piy,
               ez = (double)pos[3 * (size_t)j + 2] - (double)piz;
        im.reduce(ex, ey, ez);
        sx = (T)ex; sy = (T)ey; sz = (T)ez;
      } else {
        sx = pos[3 * (size_t)j] - pix; sy = pos[3 * (size_t)j + 1] - piy; sz = pos[3 * (size_t)j + 2] - piz;
      }
      const T r2t = sx * sx + sy * sy + sz * sz;
      const double dist = (double)sqrt(r2t);
      if (dist > 1e-8) {  // (NaN fails)
        const double rinv = 1.0 / dist, rinv2 = rinv * rinv;
        const double b1 = rinv * rinv2, b2 = 3.0 * b1 * rinv2;
        double l3 = 1.0, l5 = 1.0;
        if constexpr (THOLE) {
          const double big = width * (dist * dist * dist) / sqrt((double)ai * (double)aj);
          if (big < DS_THOLE_EXIT) {
            const double ex = exp(-big);
            l3 = 1.0 - ex; l5 = 1.0 - (1.0 + big) * ex;
          }
        }
        c1 = sm1 * (l3 * b1); c2 = sm1 * (l5 * b2);
        rx = (double)sx; ry = (double)sy; rz = (double)sz;
        jj = j;
      }
    }
    ten[e] = c1; ten[slots + e] = c2; ten[2 * slots + e] = rx; ten[3 * slots + e] = ry; ten[4 * slots + e] = rz;
    nbr[e] = jj;
  }
}

// y_i = y_in,i + sum_{row i} (c1 x_j - c2 (R . x_j) R): 8 lanes per row, lane sums and butterfly in a fixed order
__global__ __launch_bounds__(256) void ds_apply_kernel(const double* __restrict__ ten, const int* __restrict__ nbr, const double* __restrict__ x,
                                                       const double* __restrict__ y_in, int N, int M, long long slots,
                                                       double* __restrict__ y) {
  const int gl = threadIdx.x & (DS_GROUP - 1);
  const long long row = (long long)blockIdx.x * DS_ROWS + threadIdx.x / DS_GROUP;
  const bool live = row < N;
  const long long beg = live ? row * M : 0, end = live ? beg + M : 0;
  const double *s1 = ten, *s2 = ten + slots, *sx = ten + 2 * slots, *sy = ten + 3 * slots, *sz = ten + 4 * slots;
  double ax = 0.0, ay = 0.0, az = 0.0;
  for (long long e = beg + gl; e < end; e += DS_GROUP) {
    const int j = nbr[e];
    const double vx = x[3 * (size_t)j], vy = x[3 * (size_t)j + 1], vz = x[3 * (size_t)j + 2];
    const double c1 = s1[e], rx = sx[e], ry = sy[e], rz = sz[e];
    const double w = -s2[e] * fma(rz, vz, fma(ry, vy, rx * vx));
    ax = fma(w, rx, fma(c1, vx, ax));
    ay = fma(w, ry, fma(c1, vy, ay));
    az = fma(w, rz, fma(c1, vz, az));
  }
  ax = ds_group_sum(ax); ay = ds_group_sum(ay); az = ds_group_sum(az);
  if (!live || gl != 0) return;
  const size_t n = 3 * (size_t)row;
  y[n] = (y_in ? y_in[n] : 0.0) + ax;
  y[n + 1] = (y_in ? y_in[n + 1] : 0.0) + ay;
  y[n + 2] = (y_in ? y_in[n + 2] : 0.0) + az;
}

size_t ds_rec_bytes(int n_atoms, int dtype) {
  return mi_align((dtype == MI_F32 ? sizeof(DsRec<float>) : sizeof(DsRec<double>)) * (size_t)(n_atoms > 0 ? n_atoms : 0));
}

template <class T, bool CSR, bool FV, bool MIN>
void ds_launch_thole(bool thole, int blocks, hipStream_t st, const DsRec<T>* rec, const T* cell, const int* bi, const double* g, int N,
                     const int* idx, const double* sdir, const double* smut, const int* ush, const int* nptr, int M, int mask_value, int flags,
                     double width, double* energies, T* forces, double* cgrad, double* dgrad, double* pgrad, double* trow) {
#define DS_GO(TH_)                                                                                                                           \
  ds_pair_kernel<T, CSR, FV, MIN, TH_><<<blocks, 256, 0, st>>>(rec, cell, bi, g, N, idx, sdir, smut, ush, nptr, M, mask_value, flags, width, \
                                                                energies, forces, cgrad, dgrad, pgrad, trow)
  if (thole) DS_GO(true); else DS_GO(false);
#undef DS_GO
}

template <class T, bool CSR, class... A> void ds_launch(bool fv, bool min_image, A... a) {
  if (fv) { if (min_image) ds_launch_thole<T, CSR, true, true>(a...); else ds_launch_thole<T, CSR, true, false>(a...); }
  else { if (min_image) ds_launch_thole<T, CSR, false, true>(a...); else ds_launch_thole<T, CSR, false, false>(a...); }
}

}  // namespace

extern "C" int mi_dipole_scale_blocks(void) { return MI_FOLD_BLOCKS; }
extern "C" size_t mi_dipole_scale_scratch_bytes(int n_atoms, int dtype) {
  return ds_rec_bytes(n_atoms, dtype) + mi_align(sizeof(double) * DS_VIR_WORDS * (size_t)(n_atoms > 0 ? n_atoms : 0));
}

extern "C" int mi_dipole_scale(const void* positions, const void* charges, const void* dipoles, const void* polarizability, const void* cell,
                               const int32_t* batch_idx, const double* weights, const double* direct_scales, const double* mutual_scales,
                               double thole_a, int n_atoms, int n_systems, int dtype, const int32_t* idx_j, const int32_t* unit_shifts,
                               const int32_t* neighbor_ptr, int max_neighbors, int mask_value, int minimum_image, int flags, double* energies,
                               void* forces, double* charge_grads, double* dipole_grads, double* polarizability_grads, double* virial_partial,
                               void* scratch, size_t scratch_bytes, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1 && n_systems <= 65535, "n_systems must be in [1, 65535]");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(!(flags & ~(MI_DP_FORCES | MI_DP_CHARGE_GRAD | MI_DP_DIPOLE_GRAD | MI_DP_VIRIAL | MI_DP_POLAR_GRAD)), "unknown flag");
  MI_REQUIRE(cell || !unit_shifts, "unit_shifts need a cell");
  MI_REQUIRE(cell || !minimum_image, "minimum_image needs a cell");
  MI_REQUIRE(!(minimum_image && unit_shifts), "minimum_image takes a list without unit_shifts");
  MI_REQUIRE(thole_a >= 0.0 && thole_a < INFINITY, "thole_a must be 0 (undamped) or positive and finite");
  MI_REQUIRE(!(thole_a > 0.0) || polarizability, "a Thole width needs the polarizability");
  MI_REQUIRE(direct_scales || mutual_scales, "direct_scales and mutual_scales are both NULL");
  const bool virial = (flags & MI_DP_VIRIAL) != 0;
  MI_REQUIRE(!virial || ((unit_shifts || minimum_image) && virial_partial), "the virial needs unit_shifts or minimum_image, and virial_partial");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && charges && dipoles && idx_j, "null pointer");
  MI_REQUIRE(energies || flags, "nothing to compute");
  MI_REQUIRE(!(flags & MI_DP_FORCES) || forces, "forces output");
  MI_REQUIRE(!(flags & MI_DP_CHARGE_GRAD) || charge_grads, "charge gradient output");
  MI_REQUIRE(!(flags & MI_DP_DIPOLE_GRAD) || dipole_grads, "dipole gradient output");
  MI_REQUIRE(!(flags & MI_DP_POLAR_GRAD) || polarizability_grads, "polarizability gradient output");
  MI_REQUIRE(scratch && scratch_bytes >= mi_dipole_scale_scratch_bytes(n_atoms, dtype), "scratch smaller than mi_dipole_scale_scratch_bytes()");
  hipStream_t st = (hipStream_t)stream;
  double* trow = reinterpret_cast<double*>((char*)scratch + ds_rec_bytes(n_atoms, dtype));
  const int blocks = mi_blocks(n_atoms, DS_ROWS);
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;  // one system: every atom belongs to system 0 and the batch index is not read
  const bool fv = (flags & (MI_DP_FORCES | MI_DP_VIRIAL)) != 0, mi = minimum_image != 0, thole = thole_a > 0.0;
#define MI_DS(T_)                                                                                                                            \
  do {                                                                                                                                       \
    ds_pack_kernel<T_><<<mi_blocks(n_atoms, 256), 256, 0, st>>>((const T_*)positions, (const T_*)charges, (const T_*)dipoles,                \
                                                                (const T_*)polarizability, n_atoms, (DsRec<T_>*)scratch);                    \
    if (neighbor_ptr)                                                                                                                        \
      ds_launch<T_, true>(fv, mi, thole, blocks, st, (const DsRec<T_>*)scratch, (const T_*)cell, bi, weights, n_atoms, idx_j, direct_scales, \
                          mutual_scales, unit_shifts, neighbor_ptr, max_neighbors, mask_value, flags, thole_a, energies, (T_*)forces,        \
                          charge_grads, dipole_grads, polarizability_grads, trow);                                                           \
    else                                                                                                                                     \
      ds_launch<T_, false>(fv, mi, thole, blocks, st, (const DsRec<T_>*)scratch, (const T_*)cell, bi, weights, n_atoms, idx_j,               \
                           direct_scales, mutual_scales, unit_shifts, neighbor_ptr, max_neighbors, mask_value, flags, thole_a, energies,     \
                           (T_*)forces, charge_grads, dipole_grads, polarizability_grads, trow);                                             \
  } while (0)
  mi_timing_begin("dipole_scale", stream);
  if (dtype == MI_F32) MI_DS(float); else MI_DS(double);
  mi_timing_end(stream);
#undef MI_DS
  MI_LAUNCH_CHECK();
  if (virial) {
    ds_fold_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>(trow, bi, n_atoms, virial_partial);
    MI_LAUNCH_CHECK();
  }
  return MI_OK;
}

extern "C" int mi_scaled_dipole_tensor_words(void) { return DS_TENSOR_WORDS; }

extern "C" int mi_scaled_dipole_tensors(const void* positions, const void* polarizability, const void* cell, const int32_t* batch_idx,
                                        const double* mutual_scales, double thole_a, int n_atoms, int n_systems, int dtype,
                                        const int32_t* idx_j, int max_neighbors, int mask_value, long long n_slots, double* tensors,
                                        int32_t* neighbors, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_slots == (long long)n_atoms * max_neighbors, "n_slots must be n_atoms * max_neighbors");
  MI_REQUIRE(!cell || n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(thole_a >= 0.0 && thole_a < INFINITY, "thole_a must be 0 (undamped) or positive and finite");
  if (n_atoms == 0 || n_slots == 0) return MI_OK;
  MI_REQUIRE(positions && polarizability && mutual_scales && idx_j && tensors && neighbors, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int blocks = mi_blocks(n_atoms, DS_ROWS);
  const int32_t* bi = (cell && n_systems > 1) ? batch_idx : nullptr;
  const bool thole = thole_a > 0.0;
#define MI_DT(T_, MIN_, TH_)                                                                                                                 \
  ds_tensor_kernel<T_, MIN_, TH_><<<blocks, 256, 0, st>>>((const T_*)positions, (const T_*)polarizability, (const T_*)cell, bi, n_atoms,     \
                                                          idx_j, mutual_scales, max_neighbors, mask_value, n_slots, thole_a, tensors,        \
                                                          neighbors)
#define MI_DT_KIND(T_)                                                                                                                       \
  do {                                                                                                                                       \
    if (cell) { if (thole) MI_DT(T_, true, true); else MI_DT(T_, true, false); }                                                             \
    else { if (thole) MI_DT(T_, false, true); else MI_DT(T_, false, false); }                                                                \
  } while (0)
  mi_timing_begin("scaled_dipole_tensors", stream);
  if (dtype == MI_F32) MI_DT_KIND(float); else MI_DT_KIND(double);
  mi_timing_end(stream);
#undef MI_DT_KIND
#undef MI_DT
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_scaled_dipole_apply(const double* tensors, const int32_t* neighbors, const double* x, const double* y_in, int n_atoms,
                                      int max_neighbors, long long n_slots, double* y, void* stream) {
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_slots == (long long)n_atoms * max_neighbors, "n_slots must be n_atoms * max_neighbors");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(x && y, "null pointer");
  MI_REQUIRE(n_slots == 0 || (tensors && neighbors), "null pointer");
  MI_REQUIRE(x != y && y_in != y, "x, y_in and y must not overlap");
  mi_timing_begin("scaled_dipole_apply", stream);
  ds_apply_kernel<<<mi_blocks(n_atoms, DS_ROWS), 256, 0, (hipStream_t)stream>>>(tensors, neighbors, x, y_in, n_atoms, max_neighbors, n_slots, y);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}
