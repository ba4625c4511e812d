// quadrupole.hip -- point-quadrupole Ewald sum: what point quadrupoles add to the periodic energy of point charges and point dipoles.
// gfx950, wave64.
//
// Atom i carries q_i, mu_i and a symmetric Cartesian quadrupole Q_i (the second Taylor coefficient 1/2 sum q d d of its charge distribution; a
// traceless Stone / AMOEBA quadrupole Theta enters as Q = Theta / 3), all fixed in the laboratory frame.  With the multipole operator
// L_i = q_i + mu_i . grad_i + Q_i : grad_i grad_i the periodic energy is 1/2 sum' L_i L_j psi(r_ij); this file returns the part of it in which
// at least one quadrupole appears (charge-quadrupole, dipole-quadrupole, quadrupole-quadrupole), split as the charge and dipole sums are
// (Gaussian units, tin-foil boundary).  The nine stored words of Q_i need not be symmetric or traceless: 1/2 (Q + Q^T) is what is used.
//
//   real space, over the stored entries (i, j, S) of a FULL list, R = r_j - r_i + S . cell, r = |R|, B_n of dipole.hip continued to B4 (B5 for
//   forces and virial; still one erfc and one exp per entry):
//     c_i = mu_i . R, t_i = tr Q_i, a_i = Q_i R, s_i = R . a_i  (c_j, t_j, a_j, s_j alike),  m_ij = mu_i . a_j, m_ji = mu_j . a_i,
//     p = a_i . a_j, d = Q_i : Q_j
//     C1 = -(q_i t_j + q_j t_i)
//     C2 = q_i s_j + q_j s_i + 2 (m_ji - m_ij) + t_i c_j - t_j c_i + t_i t_j + 2 d
//     C3 = c_i s_j - c_j s_i - t_i s_j - t_j s_i - 4 p
//     C4 = s_i s_j
//     U        = B1 C1 + B2 C2 + B3 C3 + B4 C4
//     dU/dR    = -(B2 C1 + B3 C2 + B4 C3 + B5 C4) R + 2 A1 a_i + 2 (B2 q_i + B3 (c_i - t_i) + B4 s_i) a_j + (B3 s_j - B2 t_j) mu_i
//                + (B2 t_i - B3 s_i) mu_j + 2 B2 (Q_i mu_j - Q_j mu_i) - 4 B3 (Q_i a_j + Q_j a_i)
//     dU/dq_i  = B2 s_j - B1 t_j            dU/dmu_i = (B3 s_j - B2 t_j) R - 2 B2 a_j                     (no mu in it: U is linear in mu)
//     dU/dQ_i  = A0 I + A1 R R^T + B2 (mu_j R^T + R mu_j^T) - 2 B3 (R a_j^T + a_j R^T) + 2 B2 Q_j                          (symmetric)
//                A0 = -B1 q_j + B2 (c_j + t_j) - B3 s_j,  A1 = B2 q_j - B3 (c_j + t_j) + B4 s_j
//     E_i = 1/2 sum_row U,  forces_i = sum_row dU/dR,  W[a][b] = -1/2 sum_entries (dU/dR)_a R_b      (nine components: dU/dR is not along R)
//
//   reciprocal space, over a half-space k set, G_k as in dipole.hip; tau_j = k . Q_j . k:
//     S_q, M as in dipole.hip, S' = S_q + i k.M,  T = sum_j tau_j e^{i k.r_j},  V = sum_j (Q_j k) e^{i k.r_j}  (T = k . V; V for the virial only)
//     energy per k: 1/2 G_k (|T|^2 - 2 Re[conj(S') T]); atom i owns the part that carries its own factor (q_i + i k.mu_i - tau_i) e^{i k.r_i}:
//     E_i = 1/2 sum_k G_k { tau_i Re[e^{-i k.r_i} (T - S')] - Re[conj((q_i + i k.mu_i) e^{i k.r_i}) T] }
//           + 4 a^3 / (3 sqrt(pi)) q_i t_i - 4 a^5 / (5 sqrt(pi)) (2 Q_i : Q_i + t_i^2)
//   Everything is assembled from products with T or tau_i, never as |S|^2 - |S'|^2: zero quadrupoles give exact zeros.
//
// Execution shape: that of dipole.hip.  A pack kernel writes one 16-word record {x, y, z, q, mu(3), Q(6 unique words), 3 words of padding}
// per atom (64 / 128 bytes: one gather per neighbour); one wave64 per row, lanes stride the row, the row owner sums in fp64 and alone writes.
// One block per (system, k) tree-reduces the UNSCALED table {S_q, M_x, M_y, M_z, T} (10 doubles) and, when a virial is wanted, V (6 doubles);
// one wave per atom gathers over k; one block per system folds the virial.  Pair vector and r^2 in the positions dtype, everything else fp64.
// No floating-point atomics, plain vector stores, fixed summation orders: every output is bit-reproducible.
//
// Every kernel is its own adjoint under the contract of dipole.hip: with per-atom weights g (NULL: all ones) an entry weighs
// w = (g_i + g_j) / 2, the table is summed with g_j on every atom, and the owner sums become the derivatives of L = sum_i g_i E_i.
//
// The real-space pair kernel has a second radial kind, the bare 1 / r interaction of clusters and cut-off sums (mi_coulomb_quadrupole: the
// alpha -> 0 limit, B1 = 1 / r^3, B_{n+1} = (2n + 1) B_n / r^2, with C1 ... C4, dU/dR, dU/dq, dU/dmu and dU/dQ exactly as above).
#include "common.h"

namespace {

#include "pair_row.h"
#include "qd_record.h"  // QdRec, qd_matvec, qd_pack_kernel (shared with pair_scale.hip)

#define QD_VIR_WORDS 9
#define QD_SF_WORDS 10  // {Re, Im} of S_q, M_x, M_y, M_z, T
#define QD_V_WORDS 6    // {Re, Im} of V_x, V_y, V_z
#define QD_SQRT_PI 1.7724538509055159

// the six unique words of 1/2 (Q + Q^T) of atom i, in fp64: {xx, xy, xz, yy, yz, zz}
template <class T> __device__ __forceinline__ void qd_sym(const T* __restrict__ quad, size_t i, double s[6]) {
  const T* m = quad + 9 * i;
  s[0] = (double)m[0]; s[3] = (double)m[4]; s[5] = (double)m[8];
  s[1] = 0.5 * ((double)m[1] + (double)m[3]); s[2] = 0.5 * ((double)m[2] + (double)m[6]); s[4] = 0.5 * ((double)m[5] + (double)m[7]);
}
__device__ __forceinline__ double qd_volume(const double* cm) {
  return fabs(cm[0] * (cm[4] * cm[8] - cm[5] * cm[7]) - cm[1] * (cm[3] * cm[8] - cm[5] * cm[6]) + cm[2] * (cm[3] * cm[7] - cm[4] * cm[6]));
}

// FV: forces or virial are wanted (B5 and the four extra matrix-vector products are compiled in only then).  The fp64 variant without FV is
// asked for three waves per SIMD: it fits 167 VGPRs without scratch (174 when not asked).  The same request spills in the fp32 variant and
// in any FV variant, so those keep two waves: no instantiation may use scratch.
// BARE: the undamped 1/r interaction of a cluster or a cut-off sum, the alpha -> 0 limit: B1 = 1 / r^3, B_{n+1} = (2n + 1) B_n / r^2; no erfc,
// no exp, alpha is not read (NULL).
template <class T, bool CSR, bool FV, bool BARE = false>
__global__ __launch_bounds__(256, (FV || sizeof(T) == 4) ? 2 : 3) void qd_pair_kernel(const QdRec<T>* __restrict__ rec, const T* __restrict__ cell, const T* __restrict__ alpha,
                                                      const int* __restrict__ batch_idx, const double* __restrict__ g, int N,
                                                      const int* __restrict__ idx, const int* __restrict__ ush, const int* __restrict__ nptr, int M,
                                                      int mask_value, int flags, double* __restrict__ energies, T* __restrict__ forces,
                                                      double* __restrict__ cgrad, double* __restrict__ dgrad, double* __restrict__ qgrad,
                                                      double* __restrict__ trow) {
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const int i = pair_row_index();
  if (i >= N) return;
  const int s = batch_idx ? batch_idx[i] : 0;
  const bool shifted = ush != nullptr;
  T cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (shifted) pair_row_cell(cell, s, cm);
  double al = 0.0;
  if constexpr (!BARE) al = (double)alpha[s];
  const double ta = 2.0 * al * al, inv_a_sqrt_pi = BARE ? 0.0 : 1.0 / (al * QD_SQRT_PI);
  const QdRec<T> ri = rec[i];
  const double qi = (double)ri.q, mix = (double)ri.mx, miy = (double)ri.my, miz = (double)ri.mz;
  const double Qi[6] = {(double)ri.xx, (double)ri.xy, (double)ri.xz, (double)ri.yy, (double)ri.yz, (double)ri.zz};
  const double ti = Qi[0] + Qi[3] + Qi[5];
  const double gi = g ? g[i] : 1.0;
  const bool wf = FV && (flags & MI_QD_FORCES) != 0, wv = FV && (flags & MI_QD_VIRIAL) != 0;
  const bool wc = (flags & MI_QD_CHARGE_GRAD) != 0, wd = (flags & MI_QD_DIPOLE_GRAD) != 0, wq = (flags & MI_QD_QUADRUPOLE_GRAD) != 0;
  long long beg, end;
  pair_row_range<CSR>(nptr, i, M, beg, end);
  double eacc = 0.0, cgi = 0.0, fx = 0.0, fy = 0.0, fz = 0.0, dx_ = 0.0, dy_ = 0.0, dz_ = 0.0;
  double qg[6] = {0, 0, 0, 0, 0, 0};
  double t[QD_VIR_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (long long e = beg + lane; e < end; e += MI_WAVE) {
    const int j = idx[e];
    if (pair_is_padding<CSR>(j, mask_value, N)) continue;
    const QdRec<T> rj = rec[j];
    T sx = rj.x - ri.x, sy = rj.y - ri.y, sz = rj.z - ri.z;
    if (shifted) {
      T sh[3];
      pair_separation(ush, e, cm, sh);
      sx += sh[0]; sy += sh[1]; sz += sh[2];
    }
    const T r2t = sx * sx + sy * sy + sz * sz;
    const double dist = (double)sqrt(r2t);  // the distance is a quantity of the positions dtype
    if (!(dist > 1e-8)) continue;           // (NaN distances leave here too)
    const double rinv = 1.0 / dist, ar = al * dist, rinv2 = rinv * rinv;
    const double ta2 = ta * ta;
    double pre = 0.0, b1, b2, b3, b4;
    if constexpr (BARE) {
      b1 = rinv * rinv2;
      b2 = 3.0 * b1 * rinv2;
      b3 = 5.0 * b2 * rinv2;
      b4 = 7.0 * b3 * rinv2;
    } else {
      pre = exp(-(ar * ar)) * inv_a_sqrt_pi;
      const double b0 = erfc(ar) * rinv;
      b1 = (b0 + ta * pre) * rinv2;
      b2 = (3.0 * b1 + ta2 * pre) * rinv2;
      b3 = (5.0 * b2 + ta2 * ta * pre) * rinv2;
      b4 = (7.0 * b3 + ta2 * ta2 * pre) * rinv2;
    }
    const double rx = (double)sx, ry = (double)sy, rz = (double)sz;
    const double qj = (double)rj.q, mjx = (double)rj.mx, mjy = (double)rj.my, mjz = (double)rj.mz;
    const double Qj[6] = {(double)rj.xx, (double)rj.xy, (double)rj.xz, (double)rj.yy, (double)rj.yz, (double)rj.zz};
    const double tj = Qj[0] + Qj[3] + Qj[5];
    double aix, aiy, aiz, ajx, ajy, ajz;
    qd_matvec(Qi, rx, ry, rz, aix, aiy, aiz);
    qd_matvec(Qj, rx, ry, rz, ajx, ajy, ajz);
    const double si = rx * aix + ry * aiy + rz * aiz, sj = rx * ajx + ry * ajy + rz * ajz;
    const double ci = mix * rx + miy * ry + miz * rz, cj = mjx * rx + mjy * ry + mjz * rz;
    const double mij = mix * ajx + miy * ajy + miz * ajz, mji = mjx * aix + mjy * aiy + mjz * aiz;
    const double p = aix * ajx + aiy * ajy + aiz * ajz;
    const double d = Qi[0] * Qj[0] + Qi[3] * Qj[3] + Qi[5] * Qj[5] + 2.0 * (Qi[1] * Qj[1] + Qi[2] * Qj[2] + Qi[4] * Qj[4]);
    const double c1 = -(qi * tj + qj * ti);
    const double c2 = qi * sj + qj * si + 2.0 * (mji - mij) + ti * cj - tj * ci + ti * tj + 2.0 * d;
    const double c3 = ci * sj - cj * si - ti * sj - tj * si - 4.0 * p;
    const double c4 = si * sj;
    eacc += 0.5 * (b1 * c1 + b2 * c2 + b3 * c3 + b4 * c4);
    const double w = g ? 0.5 * (gi + g[j]) : 1.0;
    const double a1 = b2 * qj - b3 * (cj + tj) + b4 * sj;
    if (wc) cgi += w * (b2 * sj - b1 * tj);
    if (wd) {
      const double u = w * (b3 * sj - b2 * tj), v = -2.0 * w * b2;
      dx_ += u * rx + v * ajx; dy_ += u * ry + v * ajy; dz_ += u * rz + v * ajz;
    }
    if (wq) {
      const double a0 = -b1 * qj + b2 * (cj + tj) - b3 * sj;
      const double tb2 = 2.0 * b2, tb3 = 2.0 * b3;
      qg[0] += w * (a0 + a1 * rx * rx + tb2 * (mjx * rx + Qj[0]) - 2.0 * tb3 * rx * ajx);
      qg[3] += w * (a0 + a1 * ry * ry + tb2 * (mjy * ry + Qj[3]) - 2.0 * tb3 * ry * ajy);
      qg[5] += w * (a0 + a1 * rz * rz + tb2 * (mjz * rz + Qj[5]) - 2.0 * tb3 * rz * ajz);
      qg[1] += w * (a1 * rx * ry + b2 * (mjx * ry + mjy * rx + 2.0 * Qj[1]) - tb3 * (rx * ajy + ry * ajx));
      qg[2] += w * (a1 * rx * rz + b2 * (mjx * rz + mjz * rx + 2.0 * Qj[2]) - tb3 * (rx * ajz + rz * ajx));
      qg[4] += w * (a1 * ry * rz + b2 * (mjy * rz + mjz * ry + 2.0 * Qj[4]) - tb3 * (ry * ajz + rz * ajy));
    }
    if constexpr (FV) {
      if (wf || wv) {
        const double b5 = BARE ? 9.0 * b4 * rinv2 : (9.0 * b4 + ta2 * ta2 * ta * pre) * rinv2;
        const double cr = -w * (b2 * c1 + b3 * c2 + b4 * c3 + b5 * c4);
        const double cai = 2.0 * w * a1, caj = 2.0 * w * (b2 * qi + b3 * (ci - ti) + b4 * si);
        const double cmi = w * (b3 * sj - b2 * tj), cmj = w * (b2 * ti - b3 * si);
        const double cq = 2.0 * w * b2, cp = -4.0 * w * b3;
        double ax, ay, az, bx, by, bz;
        // Q_i mu_j - Q_j mu_i
        qd_matvec(Qi, mjx, mjy, mjz, ax, ay, az);
        qd_matvec(Qj, mix, miy, miz, bx, by, bz);
        const double dqx = ax - bx, dqy = ay - by, dqz = az - bz;
        // Q_i a_j + Q_j a_i
        qd_matvec(Qi, ajx, ajy, ajz, ax, ay, az);
        qd_matvec(Qj, aix, aiy, aiz, bx, by, bz);
        const double ux = cr * rx + cai * aix + caj * ajx + cmi * mix + cmj * mjx + cq * dqx + cp * (ax + bx);
        const double uy = cr * ry + cai * aiy + caj * ajy + cmi * miy + cmj * mjy + cq * dqy + cp * (ay + by);
        const double uz = cr * rz + cai * aiz + caj * ajz + cmi * miz + cmj * mjz + cq * dqz + cp * (az + bz);
        fx += ux; fy += uy; fz += uz;
        if (wv) {
          t[0] -= 0.5 * ux * rx; t[1] -= 0.5 * ux * ry; t[2] -= 0.5 * ux * rz;
          t[3] -= 0.5 * uy * rx; t[4] -= 0.5 * uy * ry; t[5] -= 0.5 * uy * rz;
          t[6] -= 0.5 * uz * rx; t[7] -= 0.5 * uz * ry; t[8] -= 0.5 * uz * rz;
        }
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
  if (wq) {
#pragma unroll
    for (int k = 0; k < 6; ++k) qg[k] = wave_sum(qg[k]);
    if (lane == 0) {
      double* o = qgrad + 9 * (size_t)i;
      o[0] = qg[0]; o[1] = qg[1]; o[2] = qg[2]; o[3] = qg[1]; o[4] = qg[3]; o[5] = qg[4]; o[6] = qg[2]; o[7] = qg[4]; o[8] = qg[5];
    }
  }
  if (wv) {
#pragma unroll
    for (int k = 0; k < QD_VIR_WORDS; ++k) t[k] = wave_sum(t[k]);
    if (lane == 0) {
      double* o = trow + QD_VIR_WORDS * (size_t)i;
#pragma unroll
      for (int k = 0; k < QD_VIR_WORDS; ++k) o[k] = t[k];
    }
  }
}

// per-system fold of the per-row virials: partial[s][x][0..9) with plain stores; the caller sums the MI_FOLD_BLOCKS rows.  No atomics.
__global__ __launch_bounds__(256) void qd_fold_kernel(const double* __restrict__ trow, const int* __restrict__ batch_idx, int N,
                                                      double* __restrict__ partial) {
  mi_system_fold<QD_VIR_WORDS, MI_FOLD_BLOCKS>(batch_idx, N, QD_VIR_WORDS, partial, [&](long long r, double* a) {
#pragma unroll
    for (int k = 0; k < QD_VIR_WORDS; ++k) a[k] += trow[QD_VIR_WORDS * r + k];
  });
}

// table[b][k] = {S_q, M_x, M_y, M_z, T} and, when table_v is given, table_v[b][k] = V = sum_j g_j (Q_j k) exp(i k.r_j); unscaled (the
// consumers apply G_k).  Block (k, b): thread t takes the atoms a0 + t, a0 + t + 256, ... of system b; wave butterflies, then the four wave
// partials in a fixed order.
template <class T>
__global__ __launch_bounds__(256) void qd_sf_kernel(const T* __restrict__ pos, const T* __restrict__ q, const T* __restrict__ mu,
                                                    const T* __restrict__ quad, const double* __restrict__ g, const T* __restrict__ kvec,
                                                    const int* __restrict__ system_ptr, int n_atoms, int K, double* __restrict__ table,
                                                    double* __restrict__ table_v) {
  const int b = blockIdx.y, k = blockIdx.x;
  const int a0 = system_ptr ? system_ptr[b] : 0, a1 = system_ptr ? system_ptr[b + 1] : n_atoms;
  const T* kv = kvec + 3 * ((size_t)b * K + k);
  const double kx = kv[0], ky = kv[1], kz = kv[2];
  constexpr int W = QD_SF_WORDS + QD_V_WORDS;
  double a[W];
#pragma unroll
  for (int c = 0; c < W; ++c) a[c] = 0.0;
  for (int j = a0 + (int)threadIdx.x; j < a1; j += 256) {
    const double ph = kx * (double)pos[3 * (size_t)j] + ky * (double)pos[3 * (size_t)j + 1] + kz * (double)pos[3 * (size_t)j + 2];
    double sn, cs;
    sincos(ph, &sn, &cs);
    if (g) { const double gj = g[j]; sn *= gj; cs *= gj; }
    const double qj = q[j], mx = mu[3 * (size_t)j], my = mu[3 * (size_t)j + 1], mz = mu[3 * (size_t)j + 2];
    double Q[6], vx, vy, vz;
    qd_sym(quad, (size_t)j, Q);
    qd_matvec(Q, kx, ky, kz, vx, vy, vz);
    const double tau = kx * vx + ky * vy + kz * vz;
    a[0] += qj * cs; a[1] += qj * sn; a[2] += mx * cs; a[3] += mx * sn; a[4] += my * cs; a[5] += my * sn; a[6] += mz * cs; a[7] += mz * sn;
    a[8] += tau * cs; a[9] += tau * sn;
    a[10] += vx * cs; a[11] += vx * sn; a[12] += vy * cs; a[13] += vy * sn; a[14] += vz * cs; a[15] += vz * sn;
  }
  __shared__ double part[256 / MI_WAVE][W];
  const int lane = threadIdx.x & (MI_WAVE - 1), wave = threadIdx.x / MI_WAVE;
#pragma unroll
  for (int c = 0; c < W; ++c) { const double v = wave_sum(a[c]); if (lane == 0) part[wave][c] = v; }
  __syncthreads();
  const int c = threadIdx.x;
  if (c < W) {
    const double v = part[0][c] + part[1][c] + part[2][c] + part[3][c];
    if (c < QD_SF_WORDS) table[QD_SF_WORDS * ((size_t)b * K + k) + c] = v;
    else if (table_v) table_v[QD_V_WORDS * ((size_t)b * K + k) + (c - QD_SF_WORDS)] = v;
  }
}

// One wave per atom, lanes stride k.  With X = table (no weights) or X = g_i table + table_g (adjoint; f = 1/2 then, 1 otherwise),
// e^{i k.r_i} = c + i s, p = k.mu_i, tau = k.Q_i.k, and for a table entry Y: v_Y = Re[conj(Y) e], u_Y = Re[conj(Y) i e];  S' = X_q + i k.M^X:
//   E_i       = 1/2 sum_k G (tau (v_T - v_S') - q_i v_T - p u_T) + c3 q_i t_i - c5 (2 Q_i:Q_i + t_i^2),   c3 = 4 a^3 / (3 sqrt(pi)), c5 = 4 a^5 / (5 sqrt(pi))
//   forces_i  = -f sum_k G (tau (u_T - u_S') - q_i u_T + p v_T) k
//   charge_grads_i = -f sum_k G v_T + g_i c3 t_i               dipole_grads_i = -f sum_k G u_T k
//   quadrupole_grads_i = f sum_k G (v_T - v_S') k k^T + g_i (c3 q_i I - c5 (4 Q_i + 2 t_i I))
template <class T>
__global__ __launch_bounds__(256) void qd_recip_gather_kernel(const T* __restrict__ pos, const T* __restrict__ q, const T* __restrict__ mu,
                                                              const T* __restrict__ quad, const T* __restrict__ kvec, const T* __restrict__ cell,
                                                              const T* __restrict__ alpha, const int* __restrict__ batch_idx,
                                                              const double* __restrict__ table, const double* __restrict__ table_g,
                                                              const double* __restrict__ g, int n_atoms, int K, double* __restrict__ energies,
                                                              T* __restrict__ forces, double* __restrict__ cgrad, double* __restrict__ dgrad,
                                                              double* __restrict__ qgrad) {
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x / MI_WAVE) + threadIdx.x / MI_WAVE);
  if (i >= n_atoms) return;
  const int b = batch_idx ? batch_idx[i] : 0;
  double cm[9];
  for (int c = 0; c < 9; ++c) cm[c] = (double)cell[9 * (size_t)b + c];
  const double al = (double)alpha[b], c4 = 0.25 / (al * al), pref = 8.0 * M_PI / qd_volume(cm);
  const double x = pos[3 * (size_t)i], y = pos[3 * (size_t)i + 1], z = pos[3 * (size_t)i + 2];
  const double qi = q[i], mx = mu[3 * (size_t)i], my = mu[3 * (size_t)i + 1], mz = mu[3 * (size_t)i + 2];
  double Q[6];
  qd_sym(quad, (size_t)i, Q);
  const bool adj = table_g != nullptr;
  const double gi = g ? g[i] : 1.0;
  const T* kv = kvec + 3 * (size_t)b * K;
  const double* tb = table + QD_SF_WORDS * (size_t)b * K;
  const double* tg = adj ? table_g + QD_SF_WORDS * (size_t)b * K : nullptr;
  double e = 0, fx = 0, fy = 0, fz = 0, cg = 0, dx_ = 0, dy_ = 0, dz_ = 0;
  double qg[6] = {0, 0, 0, 0, 0, 0};
  for (int k = lane; k < K; k += MI_WAVE) {
    const double kx = kv[3 * k], ky = kv[3 * k + 1], kz = kv[3 * k + 2];
    const double k2 = kx * kx + ky * ky + kz * kz;
    if (k2 < 1e-10) continue;
    const double green = pref * exp(-k2 * c4) / k2;
    double w[QD_SF_WORDS];
#pragma unroll
    for (int c = 0; c < QD_SF_WORDS; ++c) w[c] = tb[QD_SF_WORDS * (size_t)k + c];
    if (adj) {
#pragma unroll
      for (int c = 0; c < QD_SF_WORDS; ++c) w[c] = gi * w[c] + tg[QD_SF_WORDS * (size_t)k + c];
    }
    const double mr = kx * w[2] + ky * w[4] + kz * w[6], mi = kx * w[3] + ky * w[5] + kz * w[7];  // k.M = mr + i mi, i k.M = -mi + i mr
    double sn, cs;
    sincos(kx * x + ky * y + kz * z, &sn, &cs);
    const double vs = (w[0] * cs + w[1] * sn) + (mr * sn - mi * cs), us = (w[1] * cs - w[0] * sn) + (mr * cs + mi * sn);
    const double vt = w[8] * cs + w[9] * sn, ut = w[9] * cs - w[8] * sn;
    const double p = kx * mx + ky * my + kz * mz;
    double vx, vy, vz;
    qd_matvec(Q, kx, ky, kz, vx, vy, vz);
    const double tau = kx * vx + ky * vy + kz * vz;
    e += green * (tau * (vt - vs) - qi * vt - p * ut);
    const double fr = green * (tau * (ut - us) - qi * ut + p * vt), du = green * ut, dq = green * (vt - vs);
    fx += fr * kx; fy += fr * ky; fz += fr * kz;
    cg += green * vt;
    dx_ += du * kx; dy_ += du * ky; dz_ += du * kz;
    qg[0] += dq * kx * kx; qg[1] += dq * kx * ky; qg[2] += dq * kx * kz; qg[3] += dq * ky * ky; qg[4] += dq * ky * kz; qg[5] += dq * kz * kz;
  }
  e = wave_sum(e); fx = wave_sum(fx); fy = wave_sum(fy); fz = wave_sum(fz); cg = wave_sum(cg);
  dx_ = wave_sum(dx_); dy_ = wave_sum(dy_); dz_ = wave_sum(dz_);
#pragma unroll
  for (int c = 0; c < 6; ++c) qg[c] = wave_sum(qg[c]);
  if (lane != 0) return;
  const double f = adj ? 0.5 : 1.0, a3 = al * al * al;
  const double c3 = 4.0 * a3 / (3.0 * QD_SQRT_PI), c5 = 4.0 * a3 * al * al / (5.0 * QD_SQRT_PI);
  const double ti = Q[0] + Q[3] + Q[5];
  const double qq = Q[0] * Q[0] + Q[3] * Q[3] + Q[5] * Q[5] + 2.0 * (Q[1] * Q[1] + Q[2] * Q[2] + Q[4] * Q[4]);
  if (energies) energies[i] = 0.5 * e + (c3 * qi * ti - c5 * (2.0 * qq + ti * ti));
  if (forces) { forces[3 * (size_t)i] = (T)(-f * fx); forces[3 * (size_t)i + 1] = (T)(-f * fy); forces[3 * (size_t)i + 2] = (T)(-f * fz); }
  if (cgrad) cgrad[i] = -f * cg + gi * c3 * ti;
  if (dgrad) { dgrad[3 * (size_t)i] = -f * dx_; dgrad[3 * (size_t)i + 1] = -f * dy_; dgrad[3 * (size_t)i + 2] = -f * dz_; }
  if (qgrad) {
    const double dg = gi * (c3 * qi - 2.0 * c5 * ti), od = -4.0 * gi * c5;
    double o[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) o[c] = f * qg[c] + od * Q[c];
    o[0] += dg; o[3] += dg; o[5] += dg;
    double* out = qgrad + 9 * (size_t)i;
    out[0] = o[0]; out[1] = o[1]; out[2] = o[2]; out[3] = o[1]; out[4] = o[3]; out[5] = o[4]; out[6] = o[2]; out[7] = o[4]; out[8] = o[5];
  }
}

// virial of the reciprocal sum from the unscaled tables.  With e_k = 1/2 G (|T|^2 - 2 Re[conj(S') T]) and the k set following the cell
// (k -> (I + eps)^-T k, so d(k.mu)/d eps_ab = -k_a mu_b and d(k.Q.k)/d eps_ab = -2 k_a (Q k)_b at fixed mu, Q):
//   W[a][b] = sum_k e_k (delta_ab - 2 (1/k^2 + 1/(4 a^2)) k_a k_b) + G k_a (2 Re[conj(T - S') V_b] - (Im T Re M_b - Re T Im M_b))
// (nine words, row-major).  One block per system strides k and folds in a fixed order.
template <class T>
__global__ __launch_bounds__(256) void qd_recip_virial_kernel(const double* __restrict__ table, const double* __restrict__ table_v,
                                                              const T* __restrict__ kvec, const T* __restrict__ cell, const T* __restrict__ alpha,
                                                              int K, double* __restrict__ virial) {
  const int b = blockIdx.x;
  double cm[9];
  for (int c = 0; c < 9; ++c) cm[c] = (double)cell[9 * (size_t)b + c];
  const double al = (double)alpha[b], c4 = 0.25 / (al * al), pref = 8.0 * M_PI / qd_volume(cm);
  double a[QD_VIR_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = threadIdx.x; k < K; k += 256) {
    const T* kv = kvec + 3 * ((size_t)b * K + k);
    const double kk[3] = {(double)kv[0], (double)kv[1], (double)kv[2]};
    const double k2 = kk[0] * kk[0] + kk[1] * kk[1] + kk[2] * kk[2];
    if (k2 < 1e-10) continue;
    const double green = pref * exp(-k2 * c4) / k2;
    const double* w = table + QD_SF_WORDS * ((size_t)b * K + k);
    const double* v = table_v + QD_V_WORDS * ((size_t)b * K + k);
    const double mre[3] = {w[2], w[4], w[6]}, mim[3] = {w[3], w[5], w[7]};
    const double vre[3] = {v[0], v[2], v[4]}, vim[3] = {v[1], v[3], v[5]};
    const double mr = kk[0] * mre[0] + kk[1] * mre[1] + kk[2] * mre[2], mi = kk[0] * mim[0] + kk[1] * mim[1] + kk[2] * mim[2];
    const double sr = w[0] - mi, si = w[1] + mr, tr = w[8], ti = w[9];
    const double ek = 0.5 * green * (tr * tr + ti * ti - 2.0 * (sr * tr + si * ti));
    const double c = -2.0 * ek * (1.0 / k2 + c4);
    const double dr = tr - sr, di = ti - si;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int r = 0; r < 3; ++r)
        a[3 * p + r] += (p == r ? ek : 0.0) + c * kk[p] * kk[r]
                        + green * kk[p] * (2.0 * (dr * vre[r] + di * vim[r]) - (ti * mre[r] - tr * mim[r]));
  }
  __shared__ double part[256 / MI_WAVE][QD_VIR_WORDS];
  mi_block_fold<QD_VIR_WORDS>(a, part, virial + QD_VIR_WORDS * (size_t)b, QD_VIR_WORDS);
}

size_t qd_rec_bytes(int n_atoms, int dtype) { return mi_align((dtype == MI_F32 ? sizeof(QdRec<float>) : sizeof(QdRec<double>)) * (size_t)(n_atoms > 0 ? n_atoms : 0)); }

}  // namespace

extern "C" int mi_ewald_quadrupole_blocks(void) { return MI_FOLD_BLOCKS; }
extern "C" size_t mi_ewald_quadrupole_real_scratch_bytes(int n_atoms, int dtype) {
  return qd_rec_bytes(n_atoms, dtype) + mi_align(sizeof(double) * QD_VIR_WORDS * (size_t)(n_atoms > 0 ? n_atoms : 0));
}

extern "C" int mi_ewald_quadrupole_real(const void* positions, const void* charges, const void* dipoles, const void* quadrupoles, const void* cell,
                                        const void* alpha, const int32_t* batch_idx, const double* weights, int n_atoms, int n_systems, int dtype,
                                        const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors,
                                        int mask_value, int flags, double* energies, void* forces, double* charge_grads, double* dipole_grads,
                                        double* quadrupole_grads, double* virial_partial, void* scratch, size_t scratch_bytes, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1 && n_systems <= 65535, "n_systems must be in [1, 65535]");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  const bool virial = (flags & MI_QD_VIRIAL) != 0;
  MI_REQUIRE(!virial || (unit_shifts && virial_partial), "the virial needs unit_shifts and virial_partial");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && charges && dipoles && quadrupoles && cell && alpha && idx_j, "null pointer");
  MI_REQUIRE(energies || flags, "nothing to compute");
  MI_REQUIRE(!(flags & MI_QD_FORCES) || forces, "forces output");
  MI_REQUIRE(!(flags & MI_QD_CHARGE_GRAD) || charge_grads, "charge gradient output");
  MI_REQUIRE(!(flags & MI_QD_DIPOLE_GRAD) || dipole_grads, "dipole gradient output");
  MI_REQUIRE(!(flags & MI_QD_QUADRUPOLE_GRAD) || quadrupole_grads, "quadrupole gradient output");
  MI_REQUIRE(scratch && scratch_bytes >= mi_ewald_quadrupole_real_scratch_bytes(n_atoms, dtype),
             "scratch smaller than mi_ewald_quadrupole_real_scratch_bytes()");
  hipStream_t st = (hipStream_t)stream;
  double* trow = reinterpret_cast<double*>((char*)scratch + qd_rec_bytes(n_atoms, dtype));
  const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;  // one system: every atom belongs to system 0 and the batch index is not read
  const bool fv = (flags & (MI_QD_FORCES | MI_QD_VIRIAL)) != 0;
#define MI_QD_ARGS(T_)                                                                                                                        \
  (const QdRec<T_>*)scratch, (const T_*)cell, (const T_*)alpha, bi, weights, n_atoms, idx_j, unit_shifts, neighbor_ptr, max_neighbors,       \
      mask_value, flags, energies, (T_*)forces, charge_grads, dipole_grads, quadrupole_grads, trow
#define MI_QD(T_, CSR_)                                                                                                                       \
  do {                                                                                                                                        \
    qd_pack_kernel<T_><<<mi_blocks(n_atoms, 256), 256, 0, st>>>((const T_*)positions, (const T_*)charges, (const T_*)dipoles,                 \
                                                                (const T_*)quadrupoles, n_atoms, (QdRec<T_>*)scratch);                        \
    if (fv) qd_pair_kernel<T_, CSR_, true><<<blocks, 256, 0, st>>>(MI_QD_ARGS(T_));                                                           \
    else qd_pair_kernel<T_, CSR_, false><<<blocks, 256, 0, st>>>(MI_QD_ARGS(T_));                                                             \
  } while (0)
  mi_timing_begin("ewald_quadrupole_real", stream);
  if (dtype == MI_F32) { if (neighbor_ptr) MI_QD(float, true); else MI_QD(float, false); }
  else { if (neighbor_ptr) MI_QD(double, true); else MI_QD(double, false); }
  mi_timing_end(stream);
#undef MI_QD
#undef MI_QD_ARGS
  MI_LAUNCH_CHECK();
  if (virial) {
    qd_fold_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>(trow, bi, n_atoms, virial_partial);
    MI_LAUNCH_CHECK();
  }
  return MI_OK;
}

extern "C" int mi_coulomb_quadrupole_blocks(void) { return MI_FOLD_BLOCKS; }
extern "C" size_t mi_coulomb_quadrupole_scratch_bytes(int n_atoms, int dtype) { return mi_ewald_quadrupole_real_scratch_bytes(n_atoms, dtype); }

extern "C" int mi_coulomb_quadrupole(const void* positions, const void* charges, const void* dipoles, const void* quadrupoles, const void* cell,
                                     const int32_t* batch_idx, const double* weights, int n_atoms, int n_systems, int dtype, const int32_t* idx_j,
                                     const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors, int mask_value, int flags,
                                     double* energies, void* forces, double* charge_grads, double* dipole_grads, double* quadrupole_grads,
                                     double* virial_partial, void* scratch, size_t scratch_bytes, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1 && n_systems <= 65535, "n_systems must be in [1, 65535]");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(!(flags & ~(MI_QD_FORCES | MI_QD_CHARGE_GRAD | MI_QD_DIPOLE_GRAD | MI_QD_VIRIAL | MI_QD_QUADRUPOLE_GRAD)), "unknown flag");
  MI_REQUIRE(cell || !unit_shifts, "unit_shifts need a cell");
  const bool virial = (flags & MI_QD_VIRIAL) != 0;
  MI_REQUIRE(!virial || (unit_shifts && virial_partial), "the virial needs unit_shifts and virial_partial");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && charges && dipoles && quadrupoles && idx_j, "null pointer");
  MI_REQUIRE(energies || flags, "nothing to compute");
  MI_REQUIRE(!(flags & MI_QD_FORCES) || forces, "forces output");
  MI_REQUIRE(!(flags & MI_QD_CHARGE_GRAD) || charge_grads, "charge gradient output");
  MI_REQUIRE(!(flags & MI_QD_DIPOLE_GRAD) || dipole_grads, "dipole gradient output");
  MI_REQUIRE(!(flags & MI_QD_QUADRUPOLE_GRAD) || quadrupole_grads, "quadrupole gradient output");
  MI_REQUIRE(scratch && scratch_bytes >= mi_coulomb_quadrupole_scratch_bytes(n_atoms, dtype),
             "scratch smaller than mi_coulomb_quadrupole_scratch_bytes()");
  hipStream_t st = (hipStream_t)stream;
  double* trow = reinterpret_cast<double*>((char*)scratch + qd_rec_bytes(n_atoms, dtype));
  const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;
  const bool fv = (flags & (MI_QD_FORCES | MI_QD_VIRIAL)) != 0;
#define MI_CQ_ARGS(T_)                                                                                                                        \
  (const QdRec<T_>*)scratch, (const T_*)cell, (const T_*)nullptr, bi, weights, n_atoms, idx_j, unit_shifts, neighbor_ptr, max_neighbors,     \
      mask_value, flags, energies, (T_*)forces, charge_grads, dipole_grads, quadrupole_grads, trow
#define MI_CQ(T_, CSR_)                                                                                                                       \
  do {                                                                                                                                        \
    qd_pack_kernel<T_><<<mi_blocks(n_atoms, 256), 256, 0, st>>>((const T_*)positions, (const T_*)charges, (const T_*)dipoles,                 \
                                                                (const T_*)quadrupoles, n_atoms, (QdRec<T_>*)scratch);                        \
    if (fv) qd_pair_kernel<T_, CSR_, true, true><<<blocks, 256, 0, st>>>(MI_CQ_ARGS(T_));                                                     \
    else qd_pair_kernel<T_, CSR_, false, true><<<blocks, 256, 0, st>>>(MI_CQ_ARGS(T_));                                                       \
  } while (0)
  mi_timing_begin("coulomb_quadrupole", stream);
  if (dtype == MI_F32) { if (neighbor_ptr) MI_CQ(float, true); else MI_CQ(float, false); }
  else { if (neighbor_ptr) MI_CQ(double, true); else MI_CQ(double, false); }
  mi_timing_end(stream);
#undef MI_CQ
#undef MI_CQ_ARGS
  MI_LAUNCH_CHECK();
  if (virial) {
    qd_fold_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>(trow, bi, n_atoms, virial_partial);
    MI_LAUNCH_CHECK();
  }
  return MI_OK;
}

extern "C" int mi_ewald_quadrupole_structure_factors(const void* positions, const void* charges, const void* dipoles, const void* quadrupoles,
                                                     const double* weights, const void* k_vectors, const int32_t* system_ptr, int n_atoms,
                                                     int n_systems, int n_k, int dtype, double* table, double* table_v, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0 && n_k >= 0, "n_atoms and n_k must not be negative");
  MI_REQUIRE(n_systems >= 1 && n_systems <= 65535, "n_systems must be in [1, 65535]");
  MI_REQUIRE(n_systems == 1 || system_ptr, "system_ptr is required for batches");
  if (n_k == 0) return MI_OK;
  MI_REQUIRE(table && k_vectors && (n_atoms == 0 || (positions && charges && dipoles && quadrupoles)), "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int32_t* sp = n_systems > 1 ? system_ptr : nullptr;
  mi_timing_begin("ewald_quadrupole_structure_factors", stream);
  if (dtype == MI_F32)
    qd_sf_kernel<float><<<dim3(n_k, n_systems), 256, 0, st>>>((const float*)positions, (const float*)charges, (const float*)dipoles,
                                                              (const float*)quadrupoles, weights, (const float*)k_vectors, sp, n_atoms, n_k, table,
                                                              table_v);
  else
    qd_sf_kernel<double><<<dim3(n_k, n_systems), 256, 0, st>>>((const double*)positions, (const double*)charges, (const double*)dipoles,
                                                               (const double*)quadrupoles, weights, (const double*)k_vectors, sp, n_atoms, n_k,
                                                               table, table_v);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_ewald_quadrupole_recip_gather(const void* positions, const void* charges, const void* dipoles, const void* quadrupoles,
                                                const void* k_vectors, const void* cell, const void* alpha, const int32_t* batch_idx,
                                                const double* table, const double* table_g, const double* weights, int n_atoms, int n_systems,
                                                int n_k, int dtype, double* energies, void* forces, double* charge_grads, double* dipole_grads,
                                                double* quadrupole_grads, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0 && n_k >= 0, "n_atoms and n_k must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE((table_g != nullptr) == (weights != nullptr), "table_g and weights come together");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && charges && dipoles && quadrupoles && cell && alpha && (n_k == 0 || (k_vectors && table)), "null pointer");
  MI_REQUIRE(energies || forces || charge_grads || dipole_grads || quadrupole_grads, "nothing to compute");
  hipStream_t st = (hipStream_t)stream;
  const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;
  mi_timing_begin("ewald_quadrupole_recip_gather", stream);
  if (dtype == MI_F32)
    qd_recip_gather_kernel<float><<<blocks, 256, 0, st>>>((const float*)positions, (const float*)charges, (const float*)dipoles,
                                                          (const float*)quadrupoles, (const float*)k_vectors, (const float*)cell,
                                                          (const float*)alpha, bi, table, table_g, weights, n_atoms, n_k, energies, (float*)forces,
                                                          charge_grads, dipole_grads, quadrupole_grads);
  else
    qd_recip_gather_kernel<double><<<blocks, 256, 0, st>>>((const double*)positions, (const double*)charges, (const double*)dipoles,
                                                           (const double*)quadrupoles, (const double*)k_vectors, (const double*)cell,
                                                           (const double*)alpha, bi, table, table_g, weights, n_atoms, n_k, energies,
                                                           (double*)forces, charge_grads, dipole_grads, quadrupole_grads);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_ewald_quadrupole_recip_virial(const double* table, const double* table_v, const void* k_vectors, const void* cell,
                                                const void* alpha, int n_systems, int n_k, int dtype, double* virial, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_systems >= 1 && n_k >= 0, "n_systems must be at least 1, n_k not negative");
  MI_REQUIRE(virial && cell && alpha && (n_k == 0 || (table && table_v && k_vectors)), "null pointer");
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("ewald_quadrupole_recip_virial", stream);
  if (dtype == MI_F32)
    qd_recip_virial_kernel<float><<<n_systems, 256, 0, st>>>(table, table_v, (const float*)k_vectors, (const float*)cell, (const float*)alpha, n_k,
                                                             virial);
  else
    qd_recip_virial_kernel<double><<<n_systems, 256, 0, st>>>(table, table_v, (const double*)k_vectors, (const double*)cell, (const double*)alpha,
                                                              n_k, virial);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}
