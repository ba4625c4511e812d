// dipole.hip -- point-dipole Ewald sum: what point dipoles add to the periodic energy of point charges.  gfx950, wave64.
//
// Atom i carries a charge q_i and a dipole mu_i (fixed in the laboratory frame).  The periodic energy is the charge-charge Ewald / PME energy
// plus the term of this file, split as the charge sum is (Gaussian units, tin-foil boundary):
//
//   real space, over the stored entries (i, j, S) of a FULL list, R = r_j - r_i + S . cell, r = |R|:
//     B0 = erfc(a r) / r,   B_n = [(2n - 1) B_{n-1} + (2 a^2)^n / (a sqrt(pi)) exp(-a^2 r^2)] / r^2        (one erfc, one exp per entry)
//     c_i = mu_i . R, c_j = mu_j . R, d = mu_i . mu_j, A = q_j c_i - q_i c_j + d
//     U        = B1 A - B2 c_i c_j                                   = (q_i + mu_i . grad_i)(q_j + mu_j . grad_j) B0 minus q_i q_j B0
//     dU/dR    = (-B2 A + B3 c_i c_j) R + (B1 q_j - B2 c_j) mu_i - (B1 q_i + B2 c_i) mu_j
//     dU/dq_i  = -B1 c_j            dU/dmu_i = B1 (q_j R + mu_j) - B2 c_j R
//     E_i = 1/2 sum_row U,  forces_i = sum_row dU/dR,  W[a][b] = -1/2 sum_entries (dU/dR)_a R_b      (nine components: dU/dR is not along R)
//
//   reciprocal space, over a half-space k set, G_k = (8 pi / V) exp(-k^2 / 4 a^2) / k^2 (k^2 < 1e-10: 0):
//     S_q = sum_j q_j e^{i k.r_j},  M = sum_j mu_j e^{i k.r_j},  S = S_q + i k.M
//     E_i = 1/2 sum_k G_k { Re[conj((q_i + i k.mu_i) e^{i k.r_i}) S] - q_i Re[e^{-i k.r_i} S_q] } - 2 a^3 / (3 sqrt(pi)) |mu_i|^2
//
// Execution shape.  Real space: a pack kernel writes one record {x, y, z, q, mu_x, mu_y, mu_z, -} per atom (32 / 64 bytes: one gather per
// neighbour, never a second array); one wave64 per row, lanes stride the row, the row owner sums in fp64 and alone writes.  Reciprocal
// space: one block per (system, k) walks the system's atoms in a fixed stride and tree-reduces the UNSCALED table {S_q, M_x, M_y, M_z}
// (8 doubles); one wave per atom gathers over k; one block per system folds the virial.  Pair vector and r^2 in the positions dtype, phases
// and everything else fp64.  No floating-point atomics, plain vector stores, fixed summation orders: every output is bit-reproducible.
//
// Every kernel is its own adjoint: with per-atom weights g (NULL: all ones) an entry weighs w = (g_i + g_j) / 2, the table is summed with
// g_j on every atom, and the owner sums become the derivatives of L = sum_i g_i E_i (the contract of mi_gaussian_charges).
//
// The real-space pair kernel has two more radial kinds beside the Ewald one (below): Thole damping (mi_thole_dipole) and the bare 1 / r
// interaction of clusters and cut-off sums (mi_coulomb_dipole: the alpha -> 0 limit, B1 = 1 / r^3, B_{n+1} = (2n + 1) B_n / r^2).
#include "common.h"

namespace {

#include "pair_row.h"  // the row walk of dp_pair_kernel, the pack kernel and the fixed-order folds

#define DP_VIR_WORDS 9
#define DP_SF_WORDS 8  // {Re S_q, Im S_q, Re M_x, Im M_x, Re M_y, Im M_y, Re M_z, Im M_z}

template <class T> struct DpRec {  // 32 / 64 bytes: two vector loads of one line
  T x, y, z, q, mx, my, mz, pad;
  __device__ __forceinline__ void set_tail(const T* __restrict__ mu, size_t i) { mx = mu[3 * i]; my = mu[3 * i + 1]; mz = mu[3 * i + 2]; pad = T(0); }
};

// the record of the Thole kind: the polarisability rides in the word the Ewald kind leaves empty
template <class T>
__global__ void dp_thole_pack_kernel(const T* __restrict__ pos, const T* __restrict__ q, const T* __restrict__ mu, const T* __restrict__ polar,
                                     int N, DpRec<T>* __restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  DpRec<T> r;
  r.x = pos[3 * (size_t)i]; r.y = pos[3 * (size_t)i + 1]; r.z = pos[3 * (size_t)i + 2]; r.q = q[i];
  r.set_tail(mu, (size_t)i);
  r.pad = polar[i];
  rec[i] = r;
}

__device__ __forceinline__ double dp_volume(const double* cm) {
  return fabs(cm[0] * (cm[4] * cm[8] - cm[5] * cm[7]) - cm[1] * (cm[3] * cm[8] - cm[5] * cm[6]) + cm[2] * (cm[3] * cm[7] - cm[4] * cm[6]));
}

// The radial kind of dp_pair_kernel: what stands for B1, B2, B3 in the pair expressions above.  The kind's own launch arguments travel as one
// struct in the place of the Ewald kernel's alpha pointer, so the Ewald instantiation keeps its argument block.
//   DpEwald: B_n of the header, alpha per system.
//   DpThole: the correction that ADDS exponential Thole smearing (the AMOEBA form) to undamped point dipoles.  With a_i, a_j the
//     polarisabilities (the record's last word), a_T the Thole width and E = a_T r^3 / sqrt(a_i a_j):
//       D1 = -e^-E / r^3,  D2 = -3 (1 + E) e^-E / r^5,  D3 = -15 (1 + E + 3/5 E^2) e^-E / r^7             (D_{n+1} = -(1/r) dD_n/dr, as for B_n)
//     An entry with a_i <= 0 or a_j <= 0 (or NaN) is not damped, and one with E >= 50 leaves before the exp (its D_n are below 4e-19 of the
//     undamped terms): both contribute exactly 0.  dL/da_i = -1 / (2 a_i) sum_row w E X,  X = dU/dE at fixed R = -D1 A - (3 E e^-E / r^5) c_i c_j.
//   DpBare: the undamped 1/r interaction of a cluster or a cut-off sum, the alpha -> 0 limit of the B_n: B1 = 1 / r^3, B2 = 3 / r^5,
//     B3 = 15 / r^7 (B_{n+1} = (2n + 1) B_n / r^2).  No erfc, no exp, no launch argument of its own (the word it carries is not read).
template <class T> struct DpEwald {
  static constexpr bool thole = false, bare = false;
  const T* alpha;
};
template <class T> struct DpBare {
  static constexpr bool thole = false, bare = true;
  int unused;
};
template <class T> struct DpThole {
  static constexpr bool thole = true, bare = false;
  double width;
  double* __restrict__ pgrad;
};
#define DP_THOLE_EXIT 50.0

template <class T, bool CSR, class Radial>
__global__ __launch_bounds__(256) void dp_pair_kernel(const DpRec<T>* __restrict__ rec, const T* __restrict__ cell, const Radial rad,
                                                      const int* __restrict__ batch_idx, const double* __restrict__ g, int N,
                                                      const int* __restrict__ idx, const int* __restrict__ ush, const int* __restrict__ nptr, int M,
                                                      int mask_value, int flags, double* __restrict__ energies, T* __restrict__ forces,
                                                      double* __restrict__ cgrad, double* __restrict__ dgrad, double* __restrict__ trow) {
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const int i = pair_row_index();
  if (i >= N) return;
  const int s = batch_idx ? batch_idx[i] : 0;
  const bool shifted = ush != nullptr;
  T cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (shifted) pair_row_cell(cell, s, cm);
  double al = 0.0, ta = 0.0, inv_a_sqrt_pi = 0.0;
  if constexpr (!Radial::thole && !Radial::bare) {
    al = (double)rad.alpha[s];
    ta = 2.0 * al * al; inv_a_sqrt_pi = 1.0 / (al * 1.7724538509055159);
  }
  const DpRec<T> ri = rec[i];
  const double qi = (double)ri.q, mix = (double)ri.mx, miy = (double)ri.my, miz = (double)ri.mz;
  const double gi = g ? g[i] : 1.0;
  const bool wf = (flags & MI_DP_FORCES) != 0, wc = (flags & MI_DP_CHARGE_GRAD) != 0, wd = (flags & MI_DP_DIPOLE_GRAD) != 0;
  const bool wv = (flags & MI_DP_VIRIAL) != 0;
  long long beg, end;
  pair_row_range<CSR>(nptr, i, M, beg, end);
  double eacc = 0.0, cgi = 0.0, fx = 0.0, fy = 0.0, fz = 0.0, dx_ = 0.0, dy_ = 0.0, dz_ = 0.0;
  double t[DP_VIR_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double pacc = 0.0;  // DpThole: sum_row w E X
  const bool wp = Radial::thole && (flags & MI_DP_POLAR_GRAD) != 0;
  const double ai = (double)ri.pad;
  if constexpr (Radial::thole) {
    if (!(ai > 0.0)) end = beg;  // row of an atom that is not polarisable: zeros
  }
  for (long long e = beg + lane; e < end; e += MI_WAVE) {
    const int j = idx[e];
    if (pair_is_padding<CSR>(j, mask_value, N)) continue;
    const DpRec<T> rj = rec[j];
    T sx = rj.x - ri.x, sy = rj.y - ri.y, sz = rj.z - ri.z;
    if (shifted) {
      T sh[3];
      pair_separation(ush, e, cm, sh);
      sx += sh[0]; sy += sh[1]; sz += sh[2];
    }
    const T r2t = sx * sx + sy * sy + sz * sz;
    const double dist = (double)sqrt(r2t);  // the distance is a quantity of the positions dtype
    if (!(dist > 1e-8)) continue;           // (NaN distances leave here too)
    double rinv2, pre, b1, b2;
    double b3 = 0.0, xa = 0.0, xe = 0.0;  // DpThole: D3 and the two coefficients of E X = xa A - xe c_i c_j
    if constexpr (Radial::bare) {
      const double rinv = 1.0 / dist;
      rinv2 = rinv * rinv; pre = 0.0;
      b1 = rinv * rinv2;
      b2 = 3.0 * b1 * rinv2;
    } else if constexpr (!Radial::thole) {
      const double rinv = 1.0 / dist, ar = al * dist;
      rinv2 = rinv * rinv;
      pre = exp(-(ar * ar)) * inv_a_sqrt_pi;
      const double b0 = erfc(ar) * rinv;
      b1 = (b0 + ta * pre) * rinv2;
      b2 = (3.0 * b1 + ta * ta * pre) * rinv2;
    } else {
      const double aj = (double)rj.pad;
      if (!(aj > 0.0)) continue;
      const double big = rad.width * (dist * dist * dist) / sqrt(ai * aj);
      if (!(big < DP_THOLE_EXIT)) continue;
      const double rinv = 1.0 / dist, ex = exp(-big);
      rinv2 = rinv * rinv; pre = 0.0;
      const double d3 = ex * rinv * rinv2, d5 = 3.0 * d3 * rinv2;
      b1 = -d3;
      b2 = -(1.0 + big) * d5;
      b3 = -5.0 * (1.0 + big + 0.6 * big * big) * d5 * rinv2;
      xa = big * d3; xe = big * big * d5;
    }
    const double rx = (double)sx, ry = (double)sy, rz = (double)sz;
    const double qj = (double)rj.q, mjx = (double)rj.mx, mjy = (double)rj.my, mjz = (double)rj.mz;
    const double ci = mix * rx + miy * ry + miz * rz, cj = mjx * rx + mjy * ry + mjz * rz;
    const double a = qj * ci - qi * cj + (mix * mjx + miy * mjy + miz * mjz);
    const double cc = ci * cj;
    eacc += 0.5 * (b1 * a - b2 * cc);
    const double w = g ? 0.5 * (gi + g[j]) : 1.0;
    if (wc) cgi -= w * b1 * cj;
    if (wd) {
      const double u = w * (b1 * qj - b2 * cj), v = w * b1;
      dx_ += u * rx + v * mjx; dy_ += u * ry + v * mjy; dz_ += u * rz + v * mjz;
    }
    if (wp) pacc += w * (xa * a - xe * cc);
    if (wf || wv) {
      if constexpr (Radial::bare) b3 = 5.0 * b2 * rinv2;
      else if constexpr (!Radial::thole) b3 = (5.0 * b2 + ta * ta * ta * pre) * rinv2;
      const double cr = w * (b3 * cc - b2 * a), cmi = w * (b1 * qj - b2 * cj), cmj = -w * (b1 * qi + b2 * ci);
      const double ux = cr * rx + cmi * mix + cmj * mjx, uy = cr * ry + cmi * miy + cmj * mjy, uz = cr * rz + cmi * miz + cmj * mjz;
      fx += ux; fy += uy; fz += uz;
      if (wv) {
        t[0] -= 0.5 * ux * rx; t[1] -= 0.5 * ux * ry; t[2] -= 0.5 * ux * rz;
        t[3] -= 0.5 * uy * rx; t[4] -= 0.5 * uy * ry; t[5] -= 0.5 * uy * rz;
        t[6] -= 0.5 * uz * rx; t[7] -= 0.5 * uz * ry; t[8] -= 0.5 * uz * rz;
      }
    }
  }
  if (energies) { eacc = wave_sum(eacc); if (lane == 0) energies[i] = eacc; }
  if (wf) {
    fx = wave_sum(fx); fy = wave_sum(fy); fz = wave_sum(fz);
    if (lane == 0) { forces[3 * (size_t)i] = (T)fx; forces[3 * (size_t)i + 1] = (T)fy; forces[3 * (size_t)i + 2] = (T)fz; }
  }
  if (wc) { cgi = wave_sum(cgi); if (lane == 0) cgrad[i] = cgi; }
  if (wd) {
    dx_ = wave_sum(dx_); dy_ = wave_sum(dy_); dz_ = wave_sum(dz_);
    if (lane == 0) { dgrad[3 * (size_t)i] = dx_; dgrad[3 * (size_t)i + 1] = dy_; dgrad[3 * (size_t)i + 2] = dz_; }
  }
  if constexpr (Radial::thole) {
    if (wp) { pacc = wave_sum(pacc); if (lane == 0) rad.pgrad[i] = ai > 0.0 ? -0.5 * pacc / ai : 0.0; }
  }
  if (wv) {
#pragma unroll
    for (int k = 0; k < DP_VIR_WORDS; ++k) t[k] = wave_sum(t[k]);
    if (lane == 0) {
      double* o = trow + DP_VIR_WORDS * (size_t)i;
#pragma unroll
      for (int k = 0; k < DP_VIR_WORDS; ++k) o[k] = t[k];
    }
  }
}

// per-system fold of the per-row virials: partial[s][x][0..9) with plain stores; the caller sums the MI_FOLD_BLOCKS rows.  No atomics.
__global__ __launch_bounds__(256) void dp_fold_kernel(const double* __restrict__ trow, const int* __restrict__ batch_idx, int N,
                                                      double* __restrict__ partial) {
  mi_system_fold<DP_VIR_WORDS, MI_FOLD_BLOCKS>(batch_idx, N, DP_VIR_WORDS, partial, [&](long long r, double* a) {
#pragma unroll
    for (int k = 0; k < DP_VIR_WORDS; ++k) a[k] += trow[DP_VIR_WORDS * r + k];
  });
}

// table[b][k] = {S_q, M_x, M_y, M_z} = sum_j g_j {q_j, mu_j} exp(i k.r_j), unscaled (the consumers apply G_k).  Block (k, b): thread t takes
// the atoms a0 + t, a0 + t + 256, ... of system b; wave butterflies, then the four wave partials in a fixed order.
template <class T>
__global__ __launch_bounds__(256) void dp_sf_kernel(const T* __restrict__ pos, const T* __restrict__ q, const T* __restrict__ mu,
                                                    const double* __restrict__ g, const T* __restrict__ kvec, const int* __restrict__ system_ptr,
                                                    int n_atoms, int K, double* __restrict__ table) {
  const int b = blockIdx.y, k = blockIdx.x;
  const int a0 = system_ptr ? system_ptr[b] : 0, a1 = system_ptr ? system_ptr[b + 1] : n_atoms;
  const T* kv = kvec + 3 * ((size_t)b * K + k);
  const double kx = kv[0], ky = kv[1], kz = kv[2];
  double a[DP_SF_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int j = a0 + (int)threadIdx.x; j < a1; j += 256) {
    const double ph = kx * (double)pos[3 * (size_t)j] + ky * (double)pos[3 * (size_t)j + 1] + kz * (double)pos[3 * (size_t)j + 2];
    double sn, cs;
    sincos(ph, &sn, &cs);
    if (g) { const double gj = g[j]; sn *= gj; cs *= gj; }
    const double qj = q[j], mx = mu[3 * (size_t)j], my = mu[3 * (size_t)j + 1], mz = mu[3 * (size_t)j + 2];
    a[0] += qj * cs; a[1] += qj * sn; a[2] += mx * cs; a[3] += mx * sn; a[4] += my * cs; a[5] += my * sn; a[6] += mz * cs; a[7] += mz * sn;
  }
  __shared__ double part[256 / MI_WAVE][DP_SF_WORDS];
  mi_block_fold<DP_SF_WORDS>(a, part, table + DP_SF_WORDS * ((size_t)b * K + k), DP_SF_WORDS);
}

// One wave per atom, lanes stride k.  With X = table (no weights) or X = g_i table + table_g (adjoint; f = 1/2 then, 1 otherwise), D = i k.M^X,
// e^{i k.r_i} = c + i s, p = k.mu_i and  v_q = Re[conj(X_q) e], u_q = Re[conj(X_q) i e], v_d / u_d the same of D, u_s = u_q + u_d, v_s = v_q + v_d:
//   E_i       = 1/2 sum_k G (q_i v_d + p u_s) - 2 a^3 / (3 sqrt(pi)) |mu_i|^2
//   forces_i  = -f sum_k G (q_i u_d - p v_s) k          charge_grads_i = f sum_k G v_d
//   dipole_grads_i = f sum_k G u_s k - g_i 4 a^3 / (3 sqrt(pi)) mu_i
// D enters through v_d / u_d directly, so nothing is formed as a difference of the charge sums: zero dipoles give exact zeros.
template <class T>
__global__ __launch_bounds__(256) void dp_recip_gather_kernel(const T* __restrict__ pos, const T* __restrict__ q, const T* __restrict__ mu,
                                                              const T* __restrict__ kvec, const T* __restrict__ cell, const T* __restrict__ alpha,
                                                              const int* __restrict__ batch_idx, const double* __restrict__ table,
                                                              const double* __restrict__ table_g, const double* __restrict__ g, int n_atoms, int K,
                                                              double* __restrict__ energies, T* __restrict__ forces, double* __restrict__ cgrad,
                                                              double* __restrict__ dgrad) {
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x / MI_WAVE) + threadIdx.x / MI_WAVE);
  if (i >= n_atoms) return;
  const int b = batch_idx ? batch_idx[i] : 0;
  double cm[9];
  for (int c = 0; c < 9; ++c) cm[c] = (double)cell[9 * (size_t)b + c];
  const double al = (double)alpha[b], c4 = 0.25 / (al * al), pref = 8.0 * M_PI / dp_volume(cm);
  const double x = pos[3 * (size_t)i], y = pos[3 * (size_t)i + 1], z = pos[3 * (size_t)i + 2];
  const double qi = q[i], mx = mu[3 * (size_t)i], my = mu[3 * (size_t)i + 1], mz = mu[3 * (size_t)i + 2];
  const bool adj = table_g != nullptr;
  const double gi = g ? g[i] : 1.0;
  const T* kv = kvec + 3 * (size_t)b * K;
  const double* tb = table + DP_SF_WORDS * (size_t)b * K;
  const double* tg = adj ? table_g + DP_SF_WORDS * (size_t)b * K : nullptr;
  double e = 0, fx = 0, fy = 0, fz = 0, cg = 0, dx_ = 0, dy_ = 0, dz_ = 0;
  for (int k = lane; k < K; k += MI_WAVE) {
    const double kx = kv[3 * k], ky = kv[3 * k + 1], kz = kv[3 * k + 2];
    const double k2 = kx * kx + ky * ky + kz * kz;
    if (k2 < 1e-10) continue;
    const double green = pref * exp(-k2 * c4) / k2;
    double w[DP_SF_WORDS];
#pragma unroll
    for (int c = 0; c < DP_SF_WORDS; ++c) w[c] = tb[DP_SF_WORDS * (size_t)k + c];
    if (adj) {
#pragma unroll
      for (int c = 0; c < DP_SF_WORDS; ++c) w[c] = gi * w[c] + tg[DP_SF_WORDS * (size_t)k + c];
    }
    const double mr = kx * w[2] + ky * w[4] + kz * w[6], mi = kx * w[3] + ky * w[5] + kz * w[7];  // k.M = mr + i mi, D = -mi + i mr
    double sn, cs;
    sincos(kx * x + ky * y + kz * z, &sn, &cs);
    const double vq = w[0] * cs + w[1] * sn, uq = w[1] * cs - w[0] * sn;
    const double vd = mr * sn - mi * cs, ud = mr * cs + mi * sn;
    const double us = uq + ud, vs = vq + vd;
    const double p = kx * mx + ky * my + kz * mz;
    e += green * (qi * vd + p * us);
    const double fr = green * (qi * ud - p * vs), du = green * us;
    fx += fr * kx; fy += fr * ky; fz += fr * kz;
    cg += green * vd;
    dx_ += du * kx; dy_ += du * ky; dz_ += du * kz;
  }
  e = wave_sum(e); fx = wave_sum(fx); fy = wave_sum(fy); fz = wave_sum(fz); cg = wave_sum(cg);
  dx_ = wave_sum(dx_); dy_ = wave_sum(dy_); dz_ = wave_sum(dz_);
  if (lane != 0) return;
  const double f = adj ? 0.5 : 1.0, selfc = 2.0 * al * al * al / (3.0 * 1.7724538509055159);
  if (energies) energies[i] = 0.5 * e - selfc * (mx * mx + my * my + mz * mz);
  if (forces) { forces[3 * (size_t)i] = (T)(-f * fx); forces[3 * (size_t)i + 1] = (T)(-f * fy); forces[3 * (size_t)i + 2] = (T)(-f * fz); }
  if (cgrad) cgrad[i] = f * cg;
  if (dgrad) {
    const double sg = 2.0 * selfc * gi;
    dgrad[3 * (size_t)i] = f * dx_ - sg * mx; dgrad[3 * (size_t)i + 1] = f * dy_ - sg * my; dgrad[3 * (size_t)i + 2] = f * dz_ - sg * mz;
  }
}

// virial of the reciprocal sum from the unscaled table.  With e_k = 1/2 G (|S|^2 - |S_q|^2) = 1/2 G (|D|^2 + 2 Re[conj(S_q) D]) and the k set
// following the cell (k -> (I + eps)^-T k, so d(k.mu)/d eps_ab = -k_a mu_b at fixed mu):
//   W[a][b] = sum_k e_k (delta_ab - 2 (1/k^2 + 1/(4 a^2)) k_a k_b) + G k_a (Im S Re M_b - Re S Im M_b)            (nine words, row-major)
// One block per system strides k and folds in a fixed order.
template <class T>
__global__ __launch_bounds__(256) void dp_recip_virial_kernel(const double* __restrict__ table, const T* __restrict__ kvec, const T* __restrict__ cell,
                                                              const T* __restrict__ alpha, int K, double* __restrict__ virial) {
  const int b = blockIdx.x;
  double cm[9];
  for (int c = 0; c < 9; ++c) cm[c] = (double)cell[9 * (size_t)b + c];
  const double al = (double)alpha[b], c4 = 0.25 / (al * al), pref = 8.0 * M_PI / dp_volume(cm);
  double a[DP_VIR_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = threadIdx.x; k < K; k += 256) {
    const T* kv = kvec + 3 * ((size_t)b * K + k);
    const double kk[3] = {(double)kv[0], (double)kv[1], (double)kv[2]};
    const double k2 = kk[0] * kk[0] + kk[1] * kk[1] + kk[2] * kk[2];
    if (k2 < 1e-10) continue;
    const double green = pref * exp(-k2 * c4) / k2;
    const double* w = table + DP_SF_WORDS * ((size_t)b * K + k);
    const double mre[3] = {w[2], w[4], w[6]}, mim[3] = {w[3], w[5], w[7]};
    const double mr = kk[0] * mre[0] + kk[1] * mre[1] + kk[2] * mre[2], mi = kk[0] * mim[0] + kk[1] * mim[1] + kk[2] * mim[2];
    const double sr = w[0] - mi, si = w[1] + mr;
    const double ek = 0.5 * green * (mr * mr + mi * mi + 2.0 * (w[1] * mr - w[0] * mi));
    const double c = -2.0 * ek * (1.0 / k2 + c4);
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int r = 0; r < 3; ++r) a[3 * p + r] += (p == r ? ek : 0.0) + c * kk[p] * kk[r] + green * kk[p] * (si * mre[r] - sr * mim[r]);
  }
  __shared__ double part[256 / MI_WAVE][DP_VIR_WORDS];
  mi_block_fold<DP_VIR_WORDS>(a, part, virial + DP_VIR_WORDS * (size_t)b, DP_VIR_WORDS);
}

size_t dp_rec_bytes(int n_atoms, int dtype) { return mi_align((dtype == MI_F32 ? sizeof(DpRec<float>) : sizeof(DpRec<double>)) * (size_t)(n_atoms > 0 ? n_atoms : 0)); }

}  // namespace

extern "C" int mi_ewald_dipole_blocks(void) { return MI_FOLD_BLOCKS; }
extern "C" size_t mi_ewald_dipole_real_scratch_bytes(int n_atoms, int dtype) {
  return dp_rec_bytes(n_atoms, dtype) + mi_align(sizeof(double) * DP_VIR_WORDS * (size_t)(n_atoms > 0 ? n_atoms : 0));
}

extern "C" int mi_ewald_dipole_real(const void* positions, const void* charges, const void* dipoles, const void* cell, const void* alpha,
                                    const int32_t* batch_idx, const double* weights, int n_atoms, int n_systems, int dtype, const int32_t* idx_j,
                                    const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors, int mask_value, int flags,
                                    double* energies, void* forces, double* charge_grads, double* dipole_grads, double* virial_partial,
                                    void* scratch, size_t scratch_bytes, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1 && n_systems <= 65535, "n_systems must be in [1, 65535]");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  const bool virial = (flags & MI_DP_VIRIAL) != 0;
  MI_REQUIRE(!virial || (unit_shifts && virial_partial), "the virial needs unit_shifts and virial_partial");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && charges && dipoles && cell && alpha && idx_j, "null pointer");
  MI_REQUIRE(energies || flags, "nothing to compute");
  MI_REQUIRE(!(flags & MI_DP_FORCES) || forces, "forces output");
  MI_REQUIRE(!(flags & MI_DP_CHARGE_GRAD) || charge_grads, "charge gradient output");
  MI_REQUIRE(!(flags & MI_DP_DIPOLE_GRAD) || dipole_grads, "dipole gradient output");
  MI_REQUIRE(scratch && scratch_bytes >= mi_ewald_dipole_real_scratch_bytes(n_atoms, dtype), "scratch smaller than mi_ewald_dipole_real_scratch_bytes()");
  hipStream_t st = (hipStream_t)stream;
  double* trow = reinterpret_cast<double*>((char*)scratch + dp_rec_bytes(n_atoms, dtype));
  const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;  // one system: every atom belongs to system 0 and the batch index is not read
#define MI_DP(T_, CSR_)                                                                                                                          \
  do {                                                                                                                                           \
    pair_pack_kernel<<<mi_blocks(n_atoms, 256), 256, 0, st>>>((const T_*)positions, (const T_*)charges, (const T_*)dipoles, n_atoms,             \
                                                              (DpRec<T_>*)scratch);                                                              \
    dp_pair_kernel<T_, CSR_, DpEwald<T_>><<<blocks, 256, 0, st>>>((const DpRec<T_>*)scratch, (const T_*)cell, DpEwald<T_>{(const T_*)alpha}, bi,  \
                                                                  weights, n_atoms, idx_j, unit_shifts, neighbor_ptr, max_neighbors, mask_value, \
                                                                  flags, energies, (T_*)forces, charge_grads, dipole_grads, trow);               \
  } while (0)
  mi_timing_begin("ewald_dipole_real", stream);
  if (dtype == MI_F32) { if (neighbor_ptr) MI_DP(float, true); else MI_DP(float, false); }
  else { if (neighbor_ptr) MI_DP(double, true); else MI_DP(double, false); }
  mi_timing_end(stream);
#undef MI_DP
  MI_LAUNCH_CHECK();
  if (virial) {
    dp_fold_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>(trow, bi, n_atoms, virial_partial);
    MI_LAUNCH_CHECK();
  }
  return MI_OK;
}

extern "C" int mi_thole_dipole_blocks(void) { return MI_FOLD_BLOCKS; }
extern "C" size_t mi_thole_dipole_scratch_bytes(int n_atoms, int dtype) { return mi_ewald_dipole_real_scratch_bytes(n_atoms, dtype); }

extern "C" int mi_thole_dipole(const void* positions, const void* charges, const void* dipoles, const void* cell, const void* polarizability,
                               double thole_a, const int32_t* batch_idx, const double* weights, int n_atoms, int n_systems, int dtype,
                               const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors, int mask_value,
                               int flags, double* energies, void* forces, double* charge_grads, double* dipole_grads,
                               double* polarizability_grads, double* virial_partial, void* scratch, size_t scratch_bytes, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1 && n_systems <= 65535, "n_systems must be in [1, 65535]");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(thole_a > 0.0 && thole_a < INFINITY, "thole_a must be positive and finite");
  MI_REQUIRE(cell || !unit_shifts, "unit_shifts need a cell");
  const bool virial = (flags & MI_DP_VIRIAL) != 0;
  MI_REQUIRE(!virial || (unit_shifts && virial_partial), "the virial needs unit_shifts and virial_partial");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && charges && dipoles && polarizability && idx_j, "null pointer");
  MI_REQUIRE(energies || flags, "nothing to compute");
  MI_REQUIRE(!(flags & MI_DP_FORCES) || forces, "forces output");
  MI_REQUIRE(!(flags & MI_DP_CHARGE_GRAD) || charge_grads, "charge gradient output");
  MI_REQUIRE(!(flags & MI_DP_DIPOLE_GRAD) || dipole_grads, "dipole gradient output");
  MI_REQUIRE(!(flags & MI_DP_POLAR_GRAD) || polarizability_grads, "polarizability gradient output");
  MI_REQUIRE(scratch && scratch_bytes >= mi_thole_dipole_scratch_bytes(n_atoms, dtype), "scratch smaller than mi_thole_dipole_scratch_bytes()");
  hipStream_t st = (hipStream_t)stream;
  double* trow = reinterpret_cast<double*>((char*)scratch + dp_rec_bytes(n_atoms, dtype));
  const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;
#define MI_TH(T_, CSR_)                                                                                                                          \
  do {                                                                                                                                           \
    dp_thole_pack_kernel<<<mi_blocks(n_atoms, 256), 256, 0, st>>>((const T_*)positions, (const T_*)charges, (const T_*)dipoles,                  \
                                                                  (const T_*)polarizability, n_atoms, (DpRec<T_>*)scratch);                      \
    dp_pair_kernel<T_, CSR_, DpThole<T_>><<<blocks, 256, 0, st>>>((const DpRec<T_>*)scratch, (const T_*)cell,                                    \
                                                                  DpThole<T_>{thole_a, polarizability_grads}, bi, weights, n_atoms, idx_j,       \
                                                                  unit_shifts, neighbor_ptr, max_neighbors, mask_value, flags, energies,         \
                                                                  (T_*)forces, charge_grads, dipole_grads, trow);                                \
  } while (0)
  mi_timing_begin("thole_dipole", stream);
  if (dtype == MI_F32) { if (neighbor_ptr) MI_TH(float, true); else MI_TH(float, false); }
  else { if (neighbor_ptr) MI_TH(double, true); else MI_TH(double, false); }
  mi_timing_end(stream);
#undef MI_TH
  MI_LAUNCH_CHECK();
  if (virial) {
    dp_fold_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>(trow, bi, n_atoms, virial_partial);
    MI_LAUNCH_CHECK();
  }
  return MI_OK;
}

extern "C" int mi_coulomb_dipole_blocks(void) { return MI_FOLD_BLOCKS; }
extern "C" size_t mi_coulomb_dipole_scratch_bytes(int n_atoms, int dtype) { return mi_ewald_dipole_real_scratch_bytes(n_atoms, dtype); }

extern "C" int mi_coulomb_dipole(const void* positions, const void* charges, const void* dipoles, const void* cell, const int32_t* batch_idx,
                                 const double* weights, int n_atoms, int n_systems, int dtype, const int32_t* idx_j, const int32_t* unit_shifts,
                                 const int32_t* neighbor_ptr, int max_neighbors, int mask_value, int flags, double* energies, void* forces,
                                 double* charge_grads, double* dipole_grads, double* virial_partial, void* scratch, size_t scratch_bytes,
                                 void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1 && n_systems <= 65535, "n_systems must be in [1, 65535]");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(!(flags & ~(MI_DP_FORCES | MI_DP_CHARGE_GRAD | MI_DP_DIPOLE_GRAD | MI_DP_VIRIAL)), "unknown flag");
  MI_REQUIRE(cell || !unit_shifts, "unit_shifts need a cell");
  const bool virial = (flags & MI_DP_VIRIAL) != 0;
  MI_REQUIRE(!virial || (unit_shifts && virial_partial), "the virial needs unit_shifts and virial_partial");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && charges && dipoles && idx_j, "null pointer");
  MI_REQUIRE(energies || flags, "nothing to compute");
  MI_REQUIRE(!(flags & MI_DP_FORCES) || forces, "forces output");
  MI_REQUIRE(!(flags & MI_DP_CHARGE_GRAD) || charge_grads, "charge gradient output");
  MI_REQUIRE(!(flags & MI_DP_DIPOLE_GRAD) || dipole_grads, "dipole gradient output");
  MI_REQUIRE(scratch && scratch_bytes >= mi_coulomb_dipole_scratch_bytes(n_atoms, dtype), "scratch smaller than mi_coulomb_dipole_scratch_bytes()");
  hipStream_t st = (hipStream_t)stream;
  double* trow = reinterpret_cast<double*>((char*)scratch + dp_rec_bytes(n_atoms, dtype));
  const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;
#define MI_CD(T_, CSR_)                                                                                                                          \
  do {                                                                                                                                           \
    pair_pack_kernel<<<mi_blocks(n_atoms, 256), 256, 0, st>>>((const T_*)positions, (const T_*)charges, (const T_*)dipoles, n_atoms,             \
                                                              (DpRec<T_>*)scratch);                                                              \
    dp_pair_kernel<T_, CSR_, DpBare<T_>><<<blocks, 256, 0, st>>>((const DpRec<T_>*)scratch, (const T_*)cell, DpBare<T_>{0}, bi, weights,         \
                                                                 n_atoms, idx_j, unit_shifts, neighbor_ptr, max_neighbors, mask_value, flags,    \
                                                                 energies, (T_*)forces, charge_grads, dipole_grads, trow);                       \
  } while (0)
  mi_timing_begin("coulomb_dipole", stream);
  if (dtype == MI_F32) { if (neighbor_ptr) MI_CD(float, true); else MI_CD(float, false); }
  else { if (neighbor_ptr) MI_CD(double, true); else MI_CD(double, false); }
  mi_timing_end(stream);
#undef MI_CD
  MI_LAUNCH_CHECK();
  if (virial) {
    dp_fold_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>(trow, bi, n_atoms, virial_partial);
    MI_LAUNCH_CHECK();
  }
  return MI_OK;
}

extern "C" int mi_ewald_dipole_structure_factors(const void* positions, const void* charges, const void* dipoles, const double* weights,
                                                 const void* k_vectors, const int32_t* system_ptr, int n_atoms, int n_systems, int n_k, int dtype,
                                                 double* table, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0 && n_k >= 0, "n_atoms and n_k must not be negative");
  MI_REQUIRE(n_systems >= 1 && n_systems <= 65535, "n_systems must be in [1, 65535]");
  MI_REQUIRE(n_systems == 1 || system_ptr, "system_ptr is required for batches");
  if (n_k == 0) return MI_OK;
  MI_REQUIRE(table && k_vectors && (n_atoms == 0 || (positions && charges && dipoles)), "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int32_t* sp = n_systems > 1 ? system_ptr : nullptr;
  mi_timing_begin("ewald_dipole_structure_factors", stream);
  if (dtype == MI_F32)
    dp_sf_kernel<float><<<dim3(n_k, n_systems), 256, 0, st>>>((const float*)positions, (const float*)charges, (const float*)dipoles, weights,
                                                              (const float*)k_vectors, sp, n_atoms, n_k, table);
  else
    dp_sf_kernel<double><<<dim3(n_k, n_systems), 256, 0, st>>>((const double*)positions, (const double*)charges, (const double*)dipoles, weights,
                                                               (const double*)k_vectors, sp, n_atoms, n_k, table);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_ewald_dipole_recip_gather(const void* positions, const void* charges, const void* dipoles, const void* k_vectors, const void* cell,
                                            const void* alpha, const int32_t* batch_idx, const double* table, const double* table_g,
                                            const double* weights, int n_atoms, int n_systems, int n_k, int dtype, double* energies, void* forces,
                                            double* charge_grads, double* dipole_grads, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0 && n_k >= 0, "n_atoms and n_k must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE((table_g != nullptr) == (weights != nullptr), "table_g and weights come together");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && charges && dipoles && cell && alpha && (n_k == 0 || (k_vectors && table)), "null pointer");
  MI_REQUIRE(energies || forces || charge_grads || dipole_grads, "nothing to compute");
  hipStream_t st = (hipStream_t)stream;
  const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;
  mi_timing_begin("ewald_dipole_recip_gather", stream);
  if (dtype == MI_F32)
    dp_recip_gather_kernel<float><<<blocks, 256, 0, st>>>((const float*)positions, (const float*)charges, (const float*)dipoles,
                                                          (const float*)k_vectors, (const float*)cell, (const float*)alpha, bi, table, table_g, weights,
                                                          n_atoms, n_k, energies, (float*)forces, charge_grads, dipole_grads);
  else
    dp_recip_gather_kernel<double><<<blocks, 256, 0, st>>>((const double*)positions, (const double*)charges, (const double*)dipoles,
                                                           (const double*)k_vectors, (const double*)cell, (const double*)alpha, bi, table, table_g,
                                                           weights, n_atoms, n_k, energies, (double*)forces, charge_grads, dipole_grads);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_ewald_dipole_recip_virial(const double* table, const void* k_vectors, const void* cell, const void* alpha, int n_systems, int n_k,
                                            int dtype, double* virial, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_systems >= 1 && n_k >= 0, "n_systems must be at least 1, n_k not negative");
  MI_REQUIRE(virial && cell && alpha && (n_k == 0 || (table && k_vectors)), "null pointer");
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("ewald_dipole_recip_virial", stream);
  if (dtype == MI_F32)
    dp_recip_virial_kernel<float><<<n_systems, 256, 0, st>>>(table, (const float*)k_vectors, (const float*)cell, (const float*)alpha, n_k, virial);
  else
    dp_recip_virial_kernel<double><<<n_systems, 256, 0, st>>>(table, (const double*)k_vectors, (const double*)cell, (const double*)alpha, n_k, virial);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}
