// pair_scale.hip -- scaled bonded pairs of point multipoles: what the 1-2 ... 1-5 scale factors of a force field add to the unscaled
// electrostatic energy of charges, dipoles and quadrupoles.  gfx950, wave64.
//
// Every stored entry e = (i, j, S) of a FULL list carries a scale s_e (s_ij = s_ji).  The unscaled operators of this library (Ewald, mesh,
// cluster) count the pair with weight 1; this file returns the rest,
//
//     E_i = 1/2 sum_{row i} (s_e - 1) U_ij,     U_ij = L_i L_j (1 / r),     L = q + mu . grad + Q : grad grad,
//
// the COMPLETE bare pair energy, all six terms qq, q mu, mu mu, q Q, mu Q, Q Q.  With R = r_j - r_i (+ S . cell, or reduced to its minimum
// image), r = |R|, B0 = 1 / r, B1 = 1 / r^3, B_{n+1} = (2n + 1) B_n / r^2, and c, t, a, s, m, p, d, C1 ... C4, A0, A1 of quadrupole.hip,
// A = q_j c_i - q_i c_j + mu_i . mu_j of dipole.hip:
//
//     U        = B0 q_i q_j + B1 A - B2 c_i c_j + B1 C1 + B2 C2 + B3 C3 + B4 C4
//     dU/dR    = (-B1 q_i q_j - B2 A + B3 c_i c_j - B2 C1 - B3 C2 - B4 C3 - B5 C4) R + 2 A1 a_i + 2 (B2 q_i + B3 (c_i - t_i) + B4 s_i) a_j
//                + (B1 q_j - B2 c_j + B3 s_j - B2 t_j) mu_i + (-B1 q_i - B2 c_i + B2 t_i - B3 s_i) mu_j
//                + 2 B2 (Q_i mu_j - Q_j mu_i) - 4 B3 (Q_i a_j + Q_j a_i)
//     dU/dq_i  = B0 q_j - B1 c_j + B2 s_j - B1 t_j
//     dU/dmu_i = (B1 q_j - B2 c_j + B3 s_j - B2 t_j) R + B1 mu_j - 2 B2 a_j                                       (no mu_i in it)
//     dU/dQ_i  = A0 I + A1 R R^T + B2 (mu_j R^T + R mu_j^T) - 2 B3 (R a_j^T + a_j R^T) + 2 B2 Q_j                   (symmetric)
//
// i.e. the sums of the expressions of dp_pair_kernel and qd_pair_kernel in their bare kind, plus the charge-charge part.  s_e = 0 is an
// exclusion; an entry with s_e = 1 leaves before any arithmetic and contributes exactly 0.  Entries with r <= 1e-8 are skipped.
//
// Execution shape.  Bonded rows are short (water 2 entries, organic molecules 10 - 25), so a wave per row would idle 60 - 97 % of its lanes:
// one GROUP of PS_GROUP = 8 lanes owns a row (8 rows per wave64, 32 per 256-thread block), the lanes of the group stride the row's
// entries, the group sums by three butterfly steps (__shfl_xor 4, 2, 1) and lane 0 of the group alone writes.  A wave whose rows are all
// empty or past N writes its zeros and leaves after the range test.  The record is QdRec of quadrupole.hip (one 64 / 128-byte gather per
// neighbour); s_e is read from a float64 stream laid out like idx.  Pair vector and r^2 in the positions dtype -- under minimum_image the
// difference is reduced in fp64 (rint of the fractional components, as frames.hip does) and rounded once to the positions dtype --
// everything else fp64.  No atomics, fixed summation orders: every output is bit-reproducible.  Per-row virials go through the per-system
// fold of pair_row.h.
//
// The kernel is its own adjoint under the contract of dipole.hip: with per-atom weights g an entry weighs (g_i + g_j) / 2 . (s_e - 1).
#include "common.h"

namespace {

#include "pair_row.h"
#include "qd_record.h"

#ifndef PS_GROUP
#define PS_GROUP 8  // lanes per row; a power of two that divides the wave (-DPS_GROUP=16 builds the variant DESIGN 3.32 timed)
#endif
#define PS_ROWS (256 / PS_GROUP)
#define PS_VIR_WORDS 9

template <class V> __device__ __forceinline__ V ps_group_sum(V v) {
#pragma unroll
  for (int o = PS_GROUP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, MI_WAVE);
  return v;
}

// FV: forces or virial are wanted (B5 and the four extra matrix-vector products are compiled in only then).  MIN: minimum image (the cell and
// its inverse ride in fp64 registers per lane: the rows of a wave may belong to different systems).
template <class T, bool CSR, bool FV, bool MIN>
__global__ __launch_bounds__(256, 2) void ps_pair_kernel(const QdRec<T>* __restrict__ rec, const T* __restrict__ cell,
                                                         const int* __restrict__ batch_idx, const double* __restrict__ g, int N,
                                                         const int* __restrict__ idx, const double* __restrict__ scl,
                                                         const int* __restrict__ ush, const int* __restrict__ nptr, int M, int mask_value,
                                                         int flags, double* __restrict__ energies, T* __restrict__ forces,
                                                         double* __restrict__ cgrad, double* __restrict__ dgrad, double* __restrict__ qgrad,
                                                         double* __restrict__ trow) {
  const int gl = threadIdx.x & (PS_GROUP - 1);
  const long long row = (long long)blockIdx.x * PS_ROWS + threadIdx.x / PS_GROUP;
  const bool live = row < N;
  const int i = live ? (int)row : 0;
  const bool wf = FV && (flags & MI_QD_FORCES) != 0, wv = FV && (flags & MI_QD_VIRIAL) != 0;
  const bool wc = (flags & MI_QD_CHARGE_GRAD) != 0, wd = (flags & MI_QD_DIPOLE_GRAD) != 0, wq = (flags & MI_QD_QUADRUPOLE_GRAD) != 0;
  long long beg = 0, end = 0;
  if (live) pair_row_range<CSR>(nptr, i, M, beg, end);
  double eacc = 0.0, cgi = 0.0, fx = 0.0, fy = 0.0, fz = 0.0, dx_ = 0.0, dy_ = 0.0, dz_ = 0.0;
  double qg[6] = {0, 0, 0, 0, 0, 0};
  double t[PS_VIR_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (__any(end > beg)) {  // wave-uniform: a wave without an entry goes straight to its zeros
    const bool shifted = !MIN && ush != nullptr;
    const int s = (live && batch_idx) ? batch_idx[i] : 0;
    T cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double cd[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, ci9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (shifted) pair_row_cell(cell, s, cm);
    if constexpr (MIN) {
#pragma unroll
      for (int k = 0; k < 9; ++k) cd[k] = (double)cell[9 * (size_t)s + k];
      inverse3(cd, ci9);
    }
    QdRec<T> ri = {};
    if (live) ri = rec[i];
    const double qi = (double)ri.q, mix = (double)ri.mx, miy = (double)ri.my, miz = (double)ri.mz;
    const double Qi[6] = {(double)ri.xx, (double)ri.xy, (double)ri.xz, (double)ri.yy, (double)ri.yz, (double)ri.zz};
    const double ti = Qi[0] + Qi[3] + Qi[5];
    const double gi = (g && live) ? g[i] : 1.0;
    for (long long e = beg + gl; e < end; e += PS_GROUP) {
      const int j = idx[e];
      const double se = scl[e];
      if (pair_is_padding<CSR>(j, mask_value, N)) continue;
      if (se == 1.0) continue;  // an unscaled pair: exactly nothing
      const QdRec<T> rj = rec[j];
      T sx, sy, sz;
      if constexpr (MIN) {
        double ex = (double)rj.x - (double)ri.x, ey = (double)rj.y - (double)ri.y, ez = (double)rj.z - (double)ri.z;
        const double n0 = rint(ex * ci9[0] + ey * ci9[3] + ez * ci9[6]);
        const double n1 = rint(ex * ci9[1] + ey * ci9[4] + ez * ci9[7]);
        const double n2 = rint(ex * ci9[2] + ey * ci9[5] + ez * ci9[8]);
        ex -= n0 * cd[0] + n1 * cd[3] + n2 * cd[6];
        ey -= n0 * cd[1] + n1 * cd[4] + n2 * cd[7];
        ez -= n0 * cd[2] + n1 * cd[5] + n2 * cd[8];
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
      const double b0 = 1.0 / dist, rinv2 = b0 * b0;
      const double b1 = b0 * rinv2, b2 = 3.0 * b1 * rinv2, b3 = 5.0 * b2 * rinv2, b4 = 7.0 * b3 * rinv2;
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
      const double a = qj * ci - qi * cj + (mix * mjx + miy * mjy + miz * mjz);
      const double cc = ci * cj;
      const double c1 = -(qi * tj + qj * ti);
      const double c2 = qi * sj + qj * si + 2.0 * (mji - mij) + ti * cj - tj * ci + ti * tj + 2.0 * d;
      const double c3 = ci * sj - cj * si - ti * sj - tj * si - 4.0 * p;
      const double c4 = si * sj;
      const double sm1 = se - 1.0;
      eacc += 0.5 * sm1 * (b0 * qi * qj + (b1 * a - b2 * cc) + (b1 * c1 + b2 * c2 + b3 * c3 + b4 * c4));
      const double w = g ? 0.5 * (gi + g[j]) * sm1 : sm1;
      const double a1 = b2 * qj - b3 * (cj + tj) + b4 * sj;
      const double um = (b1 * qj - b2 * cj) + (b3 * sj - b2 * tj);  // the coefficient of R in dU/dmu_i and of mu_i in dU/dR
      if (wc) cgi += w * (b0 * qj - b1 * cj + (b2 * sj - b1 * tj));
      if (wd) {
        const double u = w * um, vm = w * b1, va = -2.0 * w * b2;
        dx_ += u * rx + vm * mjx + va * ajx; dy_ += u * ry + vm * mjy + va * ajy; dz_ += u * rz + vm * mjz + va * ajz;
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
          const double b5 = 9.0 * b4 * rinv2;
          const double cr = w * (-b1 * qi * qj + (b3 * cc - b2 * a) - (b2 * c1 + b3 * c2 + b4 * c3 + b5 * c4));
          const double cai = 2.0 * w * a1, caj = 2.0 * w * (b2 * qi + b3 * (ci - ti) + b4 * si);
          const double cmi = w * um, cmj = w * (-(b1 * qi + b2 * ci) + (b2 * ti - b3 * si));
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
    // every lane of the wave is back here: the butterflies stay inside the groups
    if (energies) eacc = ps_group_sum(eacc);
    if (wf) { fx = ps_group_sum(fx); fy = ps_group_sum(fy); fz = ps_group_sum(fz); }
    if (wc) cgi = ps_group_sum(cgi);
    if (wd) { dx_ = ps_group_sum(dx_); dy_ = ps_group_sum(dy_); dz_ = ps_group_sum(dz_); }
    if (wq) {
#pragma unroll
      for (int k = 0; k < 6; ++k) qg[k] = ps_group_sum(qg[k]);
    }
    if (wv) {
#pragma unroll
      for (int k = 0; k < PS_VIR_WORDS; ++k) t[k] = ps_group_sum(t[k]);
    }
  }
  if (!live || gl != 0) return;
  const size_t n = (size_t)i;
  if (energies) energies[n] = eacc;
  if (wf) { forces[3 * n] = (T)fx; forces[3 * n + 1] = (T)fy; forces[3 * n + 2] = (T)fz; }
  if (wc) cgrad[n] = cgi;
  if (wd) { dgrad[3 * n] = dx_; dgrad[3 * n + 1] = dy_; dgrad[3 * n + 2] = dz_; }
  if (wq) {
    double* o = qgrad + 9 * n;
    o[0] = qg[0]; o[1] = qg[1]; o[2] = qg[2]; o[3] = qg[1]; o[4] = qg[3]; o[5] = qg[4]; o[6] = qg[2]; o[7] = qg[4]; o[8] = qg[5];
  }
  if (wv) {
    double* o = trow + PS_VIR_WORDS * n;
#pragma unroll
    for (int k = 0; k < PS_VIR_WORDS; ++k) o[k] = t[k];
  }
}

// per-system fold of the per-row virials: partial[s][x][0..9) with plain stores; the caller sums the MI_FOLD_BLOCKS rows.  No atomics.
__global__ __launch_bounds__(256) void ps_fold_kernel(const double* __restrict__ trow, const int* __restrict__ batch_idx, int N,
                                                      double* __restrict__ partial) {
  mi_system_fold<PS_VIR_WORDS, MI_FOLD_BLOCKS>(batch_idx, N, PS_VIR_WORDS, partial, [&](long long r, double* a) {
#pragma unroll
    for (int k = 0; k < PS_VIR_WORDS; ++k) a[k] += trow[PS_VIR_WORDS * r + k];
  });
}

size_t ps_rec_bytes(int n_atoms, int dtype) {
  return mi_align((dtype == MI_F32 ? sizeof(QdRec<float>) : sizeof(QdRec<double>)) * (size_t)(n_atoms > 0 ? n_atoms : 0));
}

template <class T, bool CSR>
void ps_launch(bool fv, bool min_image, int blocks, hipStream_t st, const QdRec<T>* rec, const T* cell, const int* bi, const double* g, int N,
               const int* idx, const double* scl, const int* ush, const int* nptr, int M, int mask_value, int flags, double* energies, T* forces,
               double* cgrad, double* dgrad, double* qgrad, double* trow) {
#define PS_GO(FV_, MIN_)                                                                                                                     \
  ps_pair_kernel<T, CSR, FV_, MIN_><<<blocks, 256, 0, st>>>(rec, cell, bi, g, N, idx, scl, ush, nptr, M, mask_value, flags, energies, forces, \
                                                             cgrad, dgrad, qgrad, trow)
  if (fv) { if (min_image) PS_GO(true, true); else PS_GO(true, false); }
  else { if (min_image) PS_GO(false, true); else PS_GO(false, false); }
#undef PS_GO
}

}  // namespace

extern "C" int mi_pair_scale_blocks(void) { return MI_FOLD_BLOCKS; }
extern "C" size_t mi_pair_scale_scratch_bytes(int n_atoms, int dtype) {
  return ps_rec_bytes(n_atoms, dtype) + mi_align(sizeof(double) * PS_VIR_WORDS * (size_t)(n_atoms > 0 ? n_atoms : 0));
}

extern "C" int mi_pair_scale(const void* positions, const void* charges, const void* dipoles, const void* quadrupoles, const void* cell,
                             const int32_t* batch_idx, const double* weights, const double* pair_scales, int n_atoms, int n_systems, int dtype,
                             const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors, int mask_value,
                             int minimum_image, int flags, double* energies, void* forces, double* charge_grads, double* dipole_grads,
                             double* quadrupole_grads, double* virial_partial, void* scratch, size_t scratch_bytes, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1 && n_systems <= 65535, "n_systems must be in [1, 65535]");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(!(flags & ~(MI_QD_FORCES | MI_QD_CHARGE_GRAD | MI_QD_DIPOLE_GRAD | MI_QD_VIRIAL | MI_QD_QUADRUPOLE_GRAD)), "unknown flag");
  MI_REQUIRE(cell || !unit_shifts, "unit_shifts need a cell");
  MI_REQUIRE(cell || !minimum_image, "minimum_image needs a cell");
  MI_REQUIRE(!(minimum_image && unit_shifts), "minimum_image takes a list without unit_shifts");
  const bool virial = (flags & MI_QD_VIRIAL) != 0;
  MI_REQUIRE(!virial || ((unit_shifts || minimum_image) && virial_partial), "the virial needs unit_shifts or minimum_image, and virial_partial");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && charges && idx_j && pair_scales, "null pointer");
  MI_REQUIRE(energies || flags, "nothing to compute");
  MI_REQUIRE(!(flags & MI_QD_FORCES) || forces, "forces output");
  MI_REQUIRE(!(flags & MI_QD_CHARGE_GRAD) || charge_grads, "charge gradient output");
  MI_REQUIRE(!(flags & MI_QD_DIPOLE_GRAD) || dipole_grads, "dipole gradient output");
  MI_REQUIRE(!(flags & MI_QD_QUADRUPOLE_GRAD) || quadrupole_grads, "quadrupole gradient output");
  MI_REQUIRE(scratch && scratch_bytes >= mi_pair_scale_scratch_bytes(n_atoms, dtype), "scratch smaller than mi_pair_scale_scratch_bytes()");
  hipStream_t st = (hipStream_t)stream;
  double* trow = reinterpret_cast<double*>((char*)scratch + ps_rec_bytes(n_atoms, dtype));
  const int blocks = mi_blocks(n_atoms, PS_ROWS);
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;  // one system: every atom belongs to system 0 and the batch index is not read
  const bool fv = (flags & (MI_QD_FORCES | MI_QD_VIRIAL)) != 0, mi = minimum_image != 0, full = dipoles && quadrupoles;
#define MI_PS(T_)                                                                                                                             \
  do {                                                                                                                                        \
    if (full)                                                                                                                                 \
      qd_pack_kernel<T_><<<mi_blocks(n_atoms, 256), 256, 0, st>>>((const T_*)positions, (const T_*)charges, (const T_*)dipoles,               \
                                                                  (const T_*)quadrupoles, n_atoms, (QdRec<T_>*)scratch);                      \
    else                                                                                                                                      \
      qd_pack_optional_kernel<T_><<<mi_blocks(n_atoms, 256), 256, 0, st>>>((const T_*)positions, (const T_*)charges, (const T_*)dipoles,      \
                                                                           (const T_*)quadrupoles, n_atoms, (QdRec<T_>*)scratch);             \
    if (neighbor_ptr)                                                                                                                         \
      ps_launch<T_, true>(fv, mi, blocks, st, (const QdRec<T_>*)scratch, (const T_*)cell, bi, weights, n_atoms, idx_j, pair_scales,           \
                          unit_shifts, neighbor_ptr, max_neighbors, mask_value, flags, energies, (T_*)forces, charge_grads, dipole_grads,     \
                          quadrupole_grads, trow);                                                                                            \
    else                                                                                                                                      \
      ps_launch<T_, false>(fv, mi, blocks, st, (const QdRec<T_>*)scratch, (const T_*)cell, bi, weights, n_atoms, idx_j, pair_scales,          \
                           unit_shifts, neighbor_ptr, max_neighbors, mask_value, flags, energies, (T_*)forces, charge_grads, dipole_grads,    \
                           quadrupole_grads, trow);                                                                                           \
  } while (0)
  mi_timing_begin("pair_scale", stream);
  if (dtype == MI_F32) MI_PS(float); else MI_PS(double);
  mi_timing_end(stream);
#undef MI_PS
  MI_LAUNCH_CHECK();
  if (virial) {
    ps_fold_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>(trow, bi, n_atoms, virial_partial);
    MI_LAUNCH_CHECK();
  }
  return MI_OK;
}
