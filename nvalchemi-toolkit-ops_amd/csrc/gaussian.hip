// gaussian.hip -- short-ranged correction that turns point-charge electrostatics into Gaussian-smeared-charge electrostatics.  gfx950, wave64.
//
// Atom i carries a Gaussian charge cloud of width sigma_i (sigma_i <= 0: a point charge).  Two clouds interact as q_i q_j erf(r / g_ij) / r,
// g_ij = sqrt(2 (s_i + s_j)), s = max(sigma, 0)^2, so the periodic Gaussian-charge energy is the point-charge Ewald / PME energy plus
//     E_i = -1/2 sum_{entries (i, j, S) of row i} q_i q_j erfc(r / g_ij) / r          r = r_j - r_i + S . cell
// over a FULL (symmetric) neighbour list -- this file -- plus a self term and a neutralising-background term (O(N), elementwise on the host
// side: nvalchemiops/interactions/electrostatics/gaussian.py).  The reference package has no counterpart.
//
// Execution shape: one wave64 per atom, lanes stride the row / CSR range (as ewald_real_kernel does).  A pack kernel writes one record
// {x, y, z, q | max(sigma, 0)} per atom so the pair loop gathers one record per neighbour.  The pair vector and the squared distance are
// formed in the positions dtype; everything after that is fp64 (the device library's erfc and exp), forces included, with one cast at the
// store.  An entry leaves before any transcendental or square root when r / g_ij >= 6, tested as r^2 >= 72 (s_i + s_j): erfc(6) = 2.2e-17,
// below fp64 resolution of the sums it would join; the same test drops pairs of two point charges (g_ij = 0).  On a 9 A electrostatics list
// with sigma ~ 0.5 A most entries leave there.
//
// The row owner alone writes: the list is full, so every owner sum counts twice (entry and mirror) -- no atomics, plain vector stores,
// fixed summation order, deterministic.  A half or truncated list is NOT detected (stated requirement, as for the D3 kernels).
//
// The same kernel is forward and adjoint.  With a weight array g[N] (NULL: all ones) every entry is weighted by w = (g_i + g_j) / 2, which
// makes the owner sums the derivatives of L = sum_i g_i E_i:
//     fm   = 1/2 q_i q_j (erfc(x) / r^3 + 2 / (sqrt(pi) g_ij) exp(-x^2) / r^2),  x = r / g_ij
//     -dL/dr_i     = +2 sum_row w fm r                      (g = NULL: the forces; sign opposite to the point-charge real-space force)
//     dL/dq_i      = -sum_row w q_j erfc(x) / r
//     dL/dsigma_i  = -(4 / sqrt(pi)) q_i sigma_i sum_row w q_j exp(-x^2) / g_ij^3     (self-image entries (i, i, S) included correctly)
//     per system   : MI_GC_VIRIAL     W[a][b]      = -sum_entries w fm r_a r_b   (-dE/d(strain); six components)
//                    MI_GC_CELL_GRAD  dL/dcell[a][b] = sum_entries w fm S_a r_b  (nine components)
// The per-system sums are written per row and folded in a fixed order by gc_fold_kernel (mi_system_fold of pair_row.h, which also holds the
// row walk of gc_pair_kernel and the pack kernel).
#include "common.h"

namespace {

#include "pair_row.h"

#define GC_ROW_WORDS 9  // doubles per row of the per-row tensor buffer (6 used by the virial, 9 by the cell gradient)

template <class T> struct GcRec {  // 32 / 64 bytes: two vector loads of one line
  T x, y, z, q, sg, pad0, pad1, pad2;
  __device__ __forceinline__ void set_tail(const T* __restrict__ sigma, size_t i) {
    const T s = sigma[i];
    sg = s > T(0) ? s : T(0);  // (NaN -> 0 as well)
    pad0 = pad1 = pad2 = T(0);
  }
};

template <class T, bool CSR>
__global__ __launch_bounds__(256) void gc_pair_kernel(const GcRec<T>* __restrict__ rec, const T* __restrict__ cell, const int* __restrict__ batch_idx,
                                                      const double* __restrict__ g, int N, const int* __restrict__ idx, const int* __restrict__ ush,
                                                      const int* __restrict__ nptr, int M, int mask_value, int flags, double* __restrict__ energies,
                                                      T* __restrict__ forces, double* __restrict__ cgrad, double* __restrict__ sgrad,
                                                      double* __restrict__ trow) {
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const int i = pair_row_index();
  if (i >= N) return;
  const bool shifted = ush != nullptr && cell != nullptr;
  T cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (shifted) pair_row_cell(cell, batch_idx ? batch_idx[i] : 0, cm);
  const GcRec<T> ri = rec[i];
  const double qi = (double)ri.q, sgi = (double)ri.sg, si = sgi * sgi;
  const double gi = g ? g[i] : 1.0;
  const bool wf = (flags & MI_GC_FORCES) != 0, wc = (flags & MI_GC_CHARGE_GRAD) != 0, ws = (flags & MI_GC_SIGMA_GRAD) != 0;
  const bool wv = (flags & MI_GC_VIRIAL) != 0, wg = (flags & MI_GC_CELL_GRAD) != 0 && !wv;
  const double two_over_sqrt_pi = 2.0 / 1.7724538509055159;
  long long beg, end;
  pair_row_range<CSR>(nptr, i, M, beg, end);
  double eacc = 0.0, cgi = 0.0, sgacc = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
  double t[GC_ROW_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (long long e = beg + lane; e < end; e += MI_WAVE) {
    const int j = idx[e];
    if (pair_is_padding<CSR>(j, mask_value, N)) continue;
    const GcRec<T> rj = rec[j];
    T sx = rj.x - ri.x, sy = rj.y - ri.y, sz = rj.z - ri.z;
    int3 S = {0, 0, 0};
    if (shifted) {
      T sh[3];
      S = pair_separation(ush, e, cm, sh);
      sx += sh[0]; sy += sh[1]; sz += sh[2];
    }
    const T r2t = sx * sx + sy * sy + sz * sz;
    const double sgj = (double)rj.sg;
    const double ss = si + sgj * sgj;
    // x = r / g_ij >= 6  <=>  r^2 >= 36 g_ij^2 = 72 (s_i + s_j); two point charges (ss == 0) leave here too.  (NaN distances fall through to
    // the r > 1e-8 test below, which they fail.)
    if ((double)r2t >= 72.0 * ss) continue;
    const double dist = (double)sqrt(r2t);  // the distance is a quantity of the positions dtype
    if (!(dist > 1e-8)) continue;
    const double rinv = 1.0 / dist, ginv = 1.0 / sqrt(2.0 * ss);
    const double x = dist * ginv;
    const double ex = exp(-(x * x));
    const double ec = erfc(x);
    const double qj = (double)rj.q;
    const double w = g ? 0.5 * (gi + g[j]) : 1.0;
    const double pot = ec * rinv;
    eacc -= 0.5 * qi * qj * pot;
    if (wc) cgi -= w * qj * pot;
    if (ws) sgacc += w * qj * ex * (ginv * ginv * ginv);
    if (wf || wv || wg) {
      const double rinv2 = rinv * rinv;
      const double fm = w * (0.5 * qi * qj) * (pot * rinv2 + two_over_sqrt_pi * ginv * ex * rinv2);
      const double dx = (double)sx, dy = (double)sy, dz = (double)sz;
      fx += fm * dx; fy += fm * dy; fz += fm * dz;
      if (wv) {
        t[0] -= fm * (dx * dx); t[1] -= fm * (dy * dy); t[2] -= fm * (dz * dz);
        t[3] -= fm * (dx * dy); t[4] -= fm * (dx * dz); t[5] -= fm * (dy * dz);
      }
      if (wg) {
        const double a0 = fm * (double)S.x, a1 = fm * (double)S.y, a2 = fm * (double)S.z;
        t[0] += a0 * dx; t[1] += a0 * dy; t[2] += a0 * dz;
        t[3] += a1 * dx; t[4] += a1 * dy; t[5] += a1 * dz;
        t[6] += a2 * dx; t[7] += a2 * dy; t[8] += a2 * dz;
      }
    }
  }
  if (energies) { eacc = wave_sum(eacc); if (lane == 0) energies[i] = eacc; }
  if (wf) {
    fx = wave_sum(fx); fy = wave_sum(fy); fz = wave_sum(fz);
    if (lane == 0) { forces[3 * (size_t)i] = (T)(2.0 * fx); forces[3 * (size_t)i + 1] = (T)(2.0 * fy); forces[3 * (size_t)i + 2] = (T)(2.0 * fz); }
  }
  if (wc) { cgi = wave_sum(cgi); if (lane == 0) cgrad[i] = cgi; }
  if (ws) { sgacc = wave_sum(sgacc); if (lane == 0) sgrad[i] = -(2.0 * two_over_sqrt_pi) * qi * sgi * sgacc; }
  if (wv || wg) {
    const int words = wv ? 6 : 9;
#pragma unroll
    for (int k = 0; k < GC_ROW_WORDS; ++k) if (k < words) t[k] = wave_sum(t[k]);  // (words is wave-uniform)
    if (lane == 0) {
      double* o = trow + GC_ROW_WORDS * (size_t)i;
#pragma unroll
      for (int k = 0; k < GC_ROW_WORDS; ++k) if (k < words) o[k] = t[k];
    }
  }
}

// per-system fold of the per-row tensors: partial[s][x][0..words) with plain stores; the caller sums the MI_FOLD_BLOCKS rows.  No atomics.
__global__ __launch_bounds__(256) void gc_fold_kernel(const double* __restrict__ trow, const int* __restrict__ batch_idx, int N, int words,
                                                      double* __restrict__ partial) {
  mi_system_fold<GC_ROW_WORDS, MI_FOLD_BLOCKS>(batch_idx, N, words, partial, [&](long long r, double* a) {
#pragma unroll
    for (int k = 0; k < GC_ROW_WORDS; ++k) if (k < words) a[k] += trow[GC_ROW_WORDS * r + k];
  });
}

// per-system sums of the O(N) background term, in the same fixed order: partial[s][x][0..2] = block partials of {q, q s, g q s} over the atoms
// of system s (s = max(sigma, 0)^2, g = 1 without weights).  Plain stores, no atomics: the background term is as reproducible as the pair sum.
template <class T>
__global__ __launch_bounds__(256) void gc_system_sums_kernel(const T* __restrict__ q, const T* __restrict__ sigma, const double* __restrict__ g,
                                                             const int* __restrict__ batch_idx, int N, double* __restrict__ partial) {
  mi_system_fold<3, MI_FOLD_BLOCKS>(batch_idx, N, 3, partial, [&](long long r, double* a) {
    const double qr = (double)q[r], sg = (double)sigma[r];
    const double qs = sg > 0.0 ? qr * (sg * sg) : 0.0;
    a[0] += qr; a[1] += qs; a[2] += g ? g[r] * qs : qs;
  });
}

size_t gc_rec_bytes(int n_atoms, int dtype) { return mi_align((dtype == MI_F32 ? sizeof(GcRec<float>) : sizeof(GcRec<double>)) * (size_t)(n_atoms > 0 ? n_atoms : 0)); }

}  // namespace

extern "C" int mi_gaussian_charges_blocks(void) { return MI_FOLD_BLOCKS; }
extern "C" int mi_gaussian_charges_row_words(void) { return GC_ROW_WORDS; }
extern "C" size_t mi_gaussian_charges_scratch_bytes(int n_atoms, int dtype) {
  return gc_rec_bytes(n_atoms, dtype) + mi_align(sizeof(double) * GC_ROW_WORDS * (size_t)(n_atoms > 0 ? n_atoms : 0));
}

extern "C" int mi_gaussian_charges_system_sums(const void* charges, const void* sigma, const double* weights, const int32_t* batch_idx, int n_atoms,
                                               int n_systems, int dtype, double* partial, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(partial && (n_atoms == 0 || (charges && sigma)), "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;
  if (dtype == MI_F32)
    gc_system_sums_kernel<float><<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>((const float*)charges, (const float*)sigma, weights, bi, n_atoms, partial);
  else
    gc_system_sums_kernel<double><<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>((const double*)charges, (const double*)sigma, weights, bi, n_atoms, partial);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_gaussian_charges(const void* positions, const void* charges, const void* sigma, const void* cell, const int32_t* batch_idx,
                                   const double* weights, int n_atoms, int n_systems, int dtype, const int32_t* idx_j, const int32_t* unit_shifts,
                                   const int32_t* neighbor_ptr, int max_neighbors, int mask_value, int flags, double* energies, void* forces,
                                   double* charge_grads, double* sigma_grads, double* system_partial, void* scratch, size_t scratch_bytes,
                                   void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  const bool tensor = (flags & (MI_GC_VIRIAL | MI_GC_CELL_GRAD)) != 0;
  MI_REQUIRE((flags & (MI_GC_VIRIAL | MI_GC_CELL_GRAD)) != (MI_GC_VIRIAL | MI_GC_CELL_GRAD), "virial and cell gradient are separate modes");
  MI_REQUIRE(!tensor || (cell && system_partial), "virial / cell gradient need cell and system_partial");
  MI_REQUIRE(!unit_shifts || cell, "unit_shifts without a cell");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && charges && sigma && idx_j, "null pointer");
  MI_REQUIRE(energies || flags, "nothing to compute");
  MI_REQUIRE(!(flags & MI_GC_FORCES) || forces, "forces output");
  MI_REQUIRE(!(flags & MI_GC_CHARGE_GRAD) || charge_grads, "charge gradient output");
  MI_REQUIRE(!(flags & MI_GC_SIGMA_GRAD) || sigma_grads, "sigma gradient output");
  MI_REQUIRE(scratch && scratch_bytes >= mi_gaussian_charges_scratch_bytes(n_atoms, dtype), "scratch smaller than mi_gaussian_charges_scratch_bytes()");
  hipStream_t st = (hipStream_t)stream;
  double* trow = reinterpret_cast<double*>((char*)scratch + gc_rec_bytes(n_atoms, dtype));
  const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
  // one system: every atom belongs to system 0 and the batch index is not read
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;
#define MI_GC(T_, CSR_)                                                                                                                        \
  do {                                                                                                                                         \
    pair_pack_kernel<<<mi_blocks(n_atoms, 256), 256, 0, st>>>((const T_*)positions, (const T_*)charges, (const T_*)sigma, n_atoms, (GcRec<T_>*)scratch); \
    gc_pair_kernel<T_, CSR_><<<blocks, 256, 0, st>>>((const GcRec<T_>*)scratch, (const T_*)cell, bi, weights, n_atoms, idx_j, unit_shifts,     \
                                                     neighbor_ptr, max_neighbors, mask_value, flags, energies, (T_*)forces, charge_grads,      \
                                                     sigma_grads, trow);                                                                       \
  } while (0)
  mi_timing_begin("gaussian_charges", stream);
  if (dtype == MI_F32) { if (neighbor_ptr) MI_GC(float, true); else MI_GC(float, false); }
  else { if (neighbor_ptr) MI_GC(double, true); else MI_GC(double, false); }
  mi_timing_end(stream);
#undef MI_GC
  MI_LAUNCH_CHECK();
  if (tensor) {
    gc_fold_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>(trow, bi, n_atoms, (flags & MI_GC_VIRIAL) ? 6 : 9, system_partial);
    MI_LAUNCH_CHECK();
  }
  return MI_OK;
}
