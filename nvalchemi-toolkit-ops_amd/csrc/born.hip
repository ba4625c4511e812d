// born.hip -- generalized Born implicit solvent: Hawkins-Cramer-Truhlar pairwise descreening, the Onufriev-Bashford-Case rescaling of the
// Born radii, the Still pair function and an ACE-type surface term.  gfx950, wave64.  The reference package has no counterpart.
//
// With rho_i = R_i - offset, S_j = screening_j rho_j and r = |r_j - r_i + S . cell| over the stored entries (i, j, S) of a FULL (symmetric)
// neighbour list -- the list IS the sum, for a cluster (no cell) and for a periodic box (the listed images) alike:
//     I(r; rho, S) = (1/4pi) int |x|^-4 d^3x over the part of the sphere of radius S at distance r that lies outside the sphere rho about 0
//                  = 0                                                                             if r + S <= rho   (engulfed)
//                  = 1/2 [1/L - 1/U + (r/4)(1/U^2 - 1/L^2) + ln(L/U)/(2r) + (S^2/(4r))(1/L^2 - 1/U^2)]   L = max(rho, |r - S|), U = r + S
//                    + (1/rho - 1/L)                                                               if rho < S - r    (i buried in j)
//     dI/dr        = 1/8 (1 + S^2/r^2)(1/U^2 - 1/L^2) + ln(U/L)/(4 r^2)          (dI/dU = 0 identically; dI/dL dL/dr cancels the buried term)
//     Psi_i = rho_i sum_row I(r; rho_i, S_j),    1/B_i = 1/rho_i - tanh(a Psi - b Psi^2 + c Psi^3) / R_i
//     E_i   = C [q_i^2 / B_i + sum_row q_i q_j / f],   f^2 = r^2 + B_i B_j exp(-r^2 / (4 B_i B_j)),   C = -1/2 k (1/eps_in - 1/eps_out)
//             + 4 pi gamma_sa (R_i + probe)^2 (R_i / B_i)^6
//
// Three passes, one wave64 per row each, lanes stride the row's entries (pair_row.h), the row owner alone writes -- the list is full, so the
// owner sees every pair it belongs to and counts entry and mirror together: no atomics, plain vector stores, fixed summation order.
//   1. gb_radii_kernel   I per entry: one log, three Newton reciprocals; engulfed spheres leave before any of them.  Lane 0 finishes Psi, tanh,
//                        B_i and chi_i = rho_i dB_i/dPsi_i = rho_i B_i^2 (1 - tanh^2)(a - 2 b Psi + 3 c Psi^2) / R_i in the same kernel.
//   2. gb_energy_kernel  per entry one exp, one Newton reciprocal, one Newton rsqrt.  With per-atom weights g (NULL: ones) an entry carries
//                        w = (g_i + g_j) / 2, self and surface terms g_i: the sums are derivatives of L = sum_i g_i E_i.  With u = w q_j / f^3:
//                          dL/dq_i = 2 C (sum_row w q_j / f + g_i q_i / B_i)
//                          direct force  -dL/dr_i |_B = -2 C q_i sum_row u (1 - e/4) r_vec,               e = exp(-D), D = r^2 / (4 B_i B_j)
//                          dL/dB_i = -C q_i sum_row u B_j e (1 + D) - g_i (C q_i^2 / B_i^2 + 6 E_surf / B_i)       (complete: both ends of a pair)
//                          virial partial  -dL/d(strain)_ab |_B = C q_i sum_row u (1 - e/4) r_a r_b
//                        The CHAIN instantiations write the direct force, the virial partial and g_i = dL/dB_i chi_i for pass 3; the energy-only
//                        instantiation has none of that code.
//   3. gb_chain_kernel   the path through the Born radii: per entry both dI(r; rho_i, S_j)/dr and dI(r; rho_j, S_i)/dr (I is not symmetric),
//                        force += (g_i dI_ij + g_j dI_ji) r_vec / r, virial partial -= 1/2 (same) r_a r_b / r; adds the direct parts of pass 2
//                        and stores the force in the positions dtype.
// One record {x, y, z, q, R, screening} per atom (pack kernel) serves the three passes; B_j and g_j are float64 arrays gathered beside it.
// The pair vector and r^2 are formed in the positions dtype, everything after that is fp64 (the arithmetic model of gaussian.hip).
#include "common.h"

namespace {

#include "pair_row.h"

#define GB_ROW_WORDS 6  // doubles per row of the per-row virial buffer {xx, yy, zz, xy, xz, yz}

// 32 / 64 bytes: two vector loads of one line.  Six words are used; the two padding words keep the record a power of two, so a gather never
// straddles a cache line and stays 16-byte vector loads (a 24 / 48-byte record would do both).  They cannot carry B_i or g_i instead: those are
// float64 whatever T is, and the pass that computes them would store into records that other waves of the same pass are gathering.  rho and S are not stored
// either: in float32 they would be rounded once more, and R - offset and screening * rho in fp64 cost two instructions per entry.
template <class T> struct GbRec {
  T x, y, z, q, rad, scr, pad0, pad1;
};

struct GbParams {
  double offset, a, b, c;  // rho = R - offset; tanh(a Psi - b Psi^2 + c Psi^3)
  double pref;             // C = -1/2 k (1/eps_in - 1/eps_out)
  double surf, probe;      // 4 pi gamma_sa (0: no surface term), probe radius
};

template <class T>
__global__ void gb_pack_kernel(const T* __restrict__ pos, const T* __restrict__ q, const T* __restrict__ rad, const T* __restrict__ scr, int N,
                               GbRec<T>* __restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  GbRec<T> r;
  r.x = pos[3 * (size_t)i]; r.y = pos[3 * (size_t)i + 1]; r.z = pos[3 * (size_t)i + 2];
  r.q = q[i]; r.rad = rad[i]; r.scr = scr[i]; r.pad0 = r.pad1 = T(0);
  rec[i] = r;
}

// 1/sqrt(x) in fp64 from the hardware seed (v_rsq_f64) + two Newton steps
__device__ __forceinline__ double gb_rsqrt(double x) {
  double y = __builtin_amdgcn_rsq(x);
  const double h = 0.5 * x;
  y = fma(y, fma(-h * y, y, 0.5), y);
  y = fma(y, fma(-h * y, y, 0.5), y);
  return y;
}

// dI(r; rho, S)/dr; ir = 1/r.  Zero for an engulfed sphere, before the log.
__device__ __forceinline__ double gb_descreen_dr(double r, double ir, double rho, double S) {
  const double U = r + S;
  if (U <= rho) return 0.0;
  const double d = fabs(r - S);
  const double L = d > rho ? d : rho;
  const double iL = MiNewton::rcp(L), iU = MiNewton::rcp(U), ir2 = ir * ir;
  return 0.125 * (1.0 + S * S * ir2) * (iU * iU - iL * iL) + 0.25 * ir2 * log(U * iL);
}

// entry e of the row: its record rj and the pair vector (sx, sy, sz), r2t in the positions dtype; `continue`s past padding and r <= 1e-8
#define GB_PAIR_VECTOR()                                    \
  const int j = idx[e];                                     \
  if (pair_is_padding<CSR>(j, mask_value, N)) continue;     \
  const GbRec<T> rj = rec[j];                               \
  T sx = rj.x - ri.x, sy = rj.y - ri.y, sz = rj.z - ri.z;   \
  if (shifted) {                                            \
    T sh[3];                                                \
    pair_separation(ush, e, cm, sh);                        \
    sx += sh[0]; sy += sh[1]; sz += sh[2];                  \
  }                                                         \
  const T r2t = sx * sx + sy * sy + sz * sz;                \
  if (!(r2t > T(1e-16))) continue /* r <= 1e-8, NaN */

// ---- pass 1: Born radii ---------------------------------------------------------------------------------------------------------------------
template <class T, bool CSR>
__global__ __launch_bounds__(256) void gb_radii_kernel(const GbRec<T>* __restrict__ rec, const T* __restrict__ cell, const int* __restrict__ batch_idx,
                                                       int N, const int* __restrict__ idx, const int* __restrict__ ush,
                                                       const int* __restrict__ nptr, int M, int mask_value, GbParams p,
                                                       double* __restrict__ born, double* __restrict__ chi) {
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const int i = pair_row_index();
  if (i >= N) return;
  const bool shifted = ush != nullptr && cell != nullptr;
  T cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (shifted) pair_row_cell(cell, batch_idx ? batch_idx[i] : 0, cm);
  const GbRec<T> ri = rec[i];
  const double Ri = (double)ri.rad, rho = Ri - p.offset, irho = 1.0 / rho;
  long long beg, end;
  pair_row_range<CSR>(nptr, i, M, beg, end);
  double acc = 0.0;
  for (long long e = beg + lane; e < end; e += MI_WAVE) {
    GB_PAIR_VECTOR();
    const double r = sqrt((double)r2t);
    const double S = (double)rj.scr * ((double)rj.rad - p.offset);
    const double U = r + S;
    if (U <= rho) continue;  // sphere j inside atom i: exactly zero, no transcendental
    const double d = fabs(r - S);
    const double L = d > rho ? d : rho;
    const double iL = MiNewton::rcp(L), iU = MiNewton::rcp(U), ir = MiNewton::rcp(r);
    const double iL2 = iL * iL, iU2 = iU * iU;
    double I = 0.5 * (iL - iU + 0.25 * r * (iU2 - iL2) + 0.5 * ir * log(L * iU) + 0.25 * S * S * ir * (iL2 - iU2));
    if (rho < S - r) I += irho - iL;  // atom i buried in sphere j: the whole shell rho .. S - r
    acc += I;
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    const double psi = rho * acc;
    const double th = tanh(psi * (p.a + psi * (-p.b + p.c * psi)));
    const double B = 1.0 / (irho - th / Ri);
    born[i] = B;
    if (chi) chi[i] = rho * B * B * (1.0 - th * th) * (p.a + psi * (-2.0 * p.b + 3.0 * p.c * psi)) / Ri;
  }
}

// ---- pass 2: energies, dE/dq, and with CHAIN the direct force, the virial partial and dE/dB ---------------------------------------------------
template <class T, bool CSR, bool CHAIN, bool VIRIAL>
__global__ __launch_bounds__(256) void gb_energy_kernel(const GbRec<T>* __restrict__ rec, const double* __restrict__ born, const double* __restrict__ chi,
                                                        const T* __restrict__ cell, const int* __restrict__ batch_idx, const double* __restrict__ g,
                                                        int N, const int* __restrict__ idx, const int* __restrict__ ush,
                                                        const int* __restrict__ nptr, int M, int mask_value, GbParams p,
                                                        double* __restrict__ energies, double* __restrict__ cgrad, double* __restrict__ fdir,
                                                        double* __restrict__ gchain, double* __restrict__ trow) {
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const int i = pair_row_index();
  if (i >= N) return;
  const bool shifted = ush != nullptr && cell != nullptr;
  T cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (shifted) pair_row_cell(cell, batch_idx ? batch_idx[i] : 0, cm);
  const GbRec<T> ri = rec[i];
  const double qi = (double)ri.q, Bi = born[i];
  const double gi = g ? g[i] : 1.0;
  const bool wc = cgrad != nullptr;
  long long beg, end;
  pair_row_range<CSR>(nptr, i, M, beg, end);
  double se = 0.0, sc = 0.0, sb = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
  double t[GB_ROW_WORDS] = {0, 0, 0, 0, 0, 0};
  for (long long e = beg + lane; e < end; e += MI_WAVE) {
    GB_PAIR_VECTOR();
    const double r2 = (double)r2t, qj = (double)rj.q, Bj = born[j];
    const double P = Bi * Bj;
    const double D = 0.25 * r2 * MiNewton::rcp(P);
    const double ex = exp(-D);
    const double fi = gb_rsqrt(fma(P, ex, r2));  // 1 / f
    const double w = g ? 0.5 * (gi + g[j]) : 1.0;
    se += qj * fi;
    if (wc) sc += w * qj * fi;
    if (CHAIN) {
      const double u = w * qj * (fi * fi * fi);
      const double ur = u * (1.0 - 0.25 * ex);
      const double dx = (double)sx, dy = (double)sy, dz = (double)sz;
      fx += ur * dx; fy += ur * dy; fz += ur * dz;
      sb += u * Bj * ex * (1.0 + D);
      if (VIRIAL) {
        t[0] += ur * (dx * dx); t[1] += ur * (dy * dy); t[2] += ur * (dz * dz);
        t[3] += ur * (dx * dy); t[4] += ur * (dx * dz); t[5] += ur * (dy * dz);
      }
    }
  }
  const double iB = 1.0 / Bi, Ri = (double)ri.rad;
  double esurf = 0.0;
  if (p.surf != 0.0) {
    const double rb = Ri * iB, rb3 = rb * rb * rb, rp = Ri + p.probe;
    esurf = p.surf * rp * rp * rb3 * rb3;
  }
  const double cq = p.pref * qi;
  if (energies) { se = wave_sum(se); if (lane == 0) energies[i] = cq * (qi * iB + se) + esurf; }
  if (wc) { sc = wave_sum(sc); if (lane == 0) cgrad[i] = 2.0 * p.pref * (sc + gi * qi * iB); }
  if (CHAIN) {
    fx = wave_sum(fx); fy = wave_sum(fy); fz = wave_sum(fz); sb = wave_sum(sb);
    if (VIRIAL) {
#pragma unroll
      for (int k = 0; k < GB_ROW_WORDS; ++k) t[k] = wave_sum(t[k]);
    }
    if (lane == 0) {
      fdir[3 * (size_t)i] = -2.0 * cq * fx; fdir[3 * (size_t)i + 1] = -2.0 * cq * fy; fdir[3 * (size_t)i + 2] = -2.0 * cq * fz;
      const double dB = -cq * sb - gi * (cq * qi * iB * iB + 6.0 * esurf * iB);
      gchain[i] = dB * chi[i];
      if (VIRIAL) {
        double* o = trow + GB_ROW_WORDS * (size_t)i;
#pragma unroll
        for (int k = 0; k < GB_ROW_WORDS; ++k) o[k] = cq * t[k];
      }
    }
  }
}

// ---- pass 3: the chain through the Born radii -------------------------------------------------------------------------------------------------
template <class T, bool CSR, bool VIRIAL>
__global__ __launch_bounds__(256) void gb_chain_kernel(const GbRec<T>* __restrict__ rec, const double* __restrict__ gchain, const double* __restrict__ fdir,
                                                       const T* __restrict__ cell, const int* __restrict__ batch_idx, int N, const int* __restrict__ idx,
                                                       const int* __restrict__ ush, const int* __restrict__ nptr, int M, int mask_value, GbParams p,
                                                       T* __restrict__ forces, double* __restrict__ trow) {
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const int i = pair_row_index();
  if (i >= N) return;
  const bool shifted = ush != nullptr && cell != nullptr;
  T cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (shifted) pair_row_cell(cell, batch_idx ? batch_idx[i] : 0, cm);
  const GbRec<T> ri = rec[i];
  const double rho_i = (double)ri.rad - p.offset, S_i = (double)ri.scr * rho_i, g_i = gchain[i];
  long long beg, end;
  pair_row_range<CSR>(nptr, i, M, beg, end);
  double fx = 0.0, fy = 0.0, fz = 0.0;
  double t[GB_ROW_WORDS] = {0, 0, 0, 0, 0, 0};
  for (long long e = beg + lane; e < end; e += MI_WAVE) {
    GB_PAIR_VECTOR();
    const double r = sqrt((double)r2t), ir = MiNewton::rcp(r);
    const double rho_j = (double)rj.rad - p.offset, S_j = (double)rj.scr * rho_j;
    const double s = (g_i * gb_descreen_dr(r, ir, rho_i, S_j) + gchain[j] * gb_descreen_dr(r, ir, rho_j, S_i)) * ir;
    const double dx = (double)sx, dy = (double)sy, dz = (double)sz;
    fx += s * dx; fy += s * dy; fz += s * dz;
    if (VIRIAL) {
      t[0] += s * (dx * dx); t[1] += s * (dy * dy); t[2] += s * (dz * dz);
      t[3] += s * (dx * dy); t[4] += s * (dx * dz); t[5] += s * (dy * dz);
    }
  }
  fx = wave_sum(fx); fy = wave_sum(fy); fz = wave_sum(fz);
  if (VIRIAL) {
#pragma unroll
    for (int k = 0; k < GB_ROW_WORDS; ++k) t[k] = wave_sum(t[k]);
  }
  if (lane == 0) {
    if (forces) {
      forces[3 * (size_t)i] = (T)(fdir[3 * (size_t)i] + fx);
      forces[3 * (size_t)i + 1] = (T)(fdir[3 * (size_t)i + 1] + fy);
      forces[3 * (size_t)i + 2] = (T)(fdir[3 * (size_t)i + 2] + fz);
    }
    if (VIRIAL) {
      double* o = trow + GB_ROW_WORDS * (size_t)i;
#pragma unroll
      for (int k = 0; k < GB_ROW_WORDS; ++k) o[k] -= 0.5 * t[k];
    }
  }
}
#undef GB_PAIR_VECTOR

// per-system fold of the per-row virials: partial[s][x][0..6) with plain stores; the caller sums the MI_FOLD_BLOCKS rows.  No atomics.
__global__ __launch_bounds__(256) void gb_fold_kernel(const double* __restrict__ trow, const int* __restrict__ batch_idx, int N,
                                                      double* __restrict__ partial) {
  mi_system_fold<GB_ROW_WORDS, MI_FOLD_BLOCKS>(batch_idx, N, GB_ROW_WORDS, partial, [&](long long r, double* a) {
#pragma unroll
    for (int k = 0; k < GB_ROW_WORDS; ++k) a[k] += trow[GB_ROW_WORDS * r + k];
  });
}

// scratch: records | chi [N] | g [N] | direct force [N][3] | per-row virial [N][6]
struct GbScratch {
  void* rec;
  double *chi, *gchain, *fdir, *trow;
};
size_t gb_rec_bytes(size_t n, int dtype) { return mi_align((dtype == MI_F32 ? sizeof(GbRec<float>) : sizeof(GbRec<double>)) * n); }
size_t gb_scratch_bytes(int n_atoms, int dtype) {
  const size_t n = (size_t)(n_atoms > 0 ? n_atoms : 0);
  return gb_rec_bytes(n, dtype) + 2 * mi_align(sizeof(double) * n) + mi_align(3 * sizeof(double) * n) + mi_align(GB_ROW_WORDS * sizeof(double) * n);
}
GbScratch gb_scratch(void* base, int n_atoms, int dtype) {
  const size_t n = (size_t)n_atoms, col = mi_align(sizeof(double) * n);
  char* b = (char*)base;
  GbScratch s;
  s.rec = b;
  s.chi = (double*)(b += gb_rec_bytes(n, dtype));
  s.gchain = (double*)(b += col);
  s.fdir = (double*)(b += col);
  s.trow = (double*)(b += mi_align(3 * sizeof(double) * n));
  return s;
}

GbParams gb_params(const double* v) { return GbParams{v[0], v[1], v[2], v[3], v[4], v[5], v[6]}; }

int gb_check_list(int n_atoms, int n_systems, int dtype, const void* cell, const int32_t* batch_idx, const int32_t* idx_j, const int32_t* unit_shifts,
                  const int32_t* neighbor_ptr, int max_neighbors, const double* params, const void* scratch, size_t scratch_bytes) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(!unit_shifts || cell, "unit_shifts without a cell");
  MI_REQUIRE(params, "null pointer");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(idx_j || (!neighbor_ptr && max_neighbors == 0), "null pointer");
  MI_REQUIRE(scratch && scratch_bytes >= gb_scratch_bytes(n_atoms, dtype), "scratch smaller than mi_born_scratch_bytes()");
  return MI_OK;
}

}  // namespace

extern "C" int mi_born_blocks(void) { return MI_FOLD_BLOCKS; }
extern "C" int mi_born_row_words(void) { return GB_ROW_WORDS; }
extern "C" size_t mi_born_scratch_bytes(int n_atoms, int dtype) { return gb_scratch_bytes(n_atoms, dtype); }

#define MI_GB_DISPATCH(RUN)                                                                    \
  do {                                                                                         \
    if (dtype == MI_F32) { if (neighbor_ptr) RUN(float, true); else RUN(float, false); }       \
    else { if (neighbor_ptr) RUN(double, true); else RUN(double, false); }                     \
  } while (0)

extern "C" int mi_born_radii(const void* positions, const void* charges, const void* radii, const void* screening, const void* cell,
                             const int32_t* batch_idx, int n_atoms, int n_systems, int dtype, const int32_t* idx_j, const int32_t* unit_shifts,
                             const int32_t* neighbor_ptr, int max_neighbors, int mask_value, const double* params, int flags, double* born_radii,
                             void* scratch, size_t scratch_bytes, void* stream) {
  const int rc = gb_check_list(n_atoms, n_systems, dtype, cell, batch_idx, idx_j, unit_shifts, neighbor_ptr, max_neighbors, params, scratch, scratch_bytes);
  if (rc != MI_OK || n_atoms == 0) return rc;
  MI_REQUIRE(positions && charges && radii && screening && born_radii, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const GbScratch s = gb_scratch(scratch, n_atoms, dtype);
  const GbParams p = gb_params(params);
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;
  double* chi = (flags & (MI_GB_FORCES | MI_GB_VIRIAL)) ? s.chi : nullptr;
  const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
#define MI_GB_RADII(T_, CSR_)                                                                                                                   \
  do {                                                                                                                                          \
    gb_pack_kernel<<<mi_blocks(n_atoms, 256), 256, 0, st>>>((const T_*)positions, (const T_*)charges, (const T_*)radii, (const T_*)screening,   \
                                                            n_atoms, (GbRec<T_>*)s.rec);                                                        \
    gb_radii_kernel<T_, CSR_><<<blocks, 256, 0, st>>>((const GbRec<T_>*)s.rec, (const T_*)cell, bi, n_atoms, idx_j, unit_shifts, neighbor_ptr,  \
                                                      max_neighbors, mask_value, p, born_radii, chi);                                           \
  } while (0)
  mi_timing_begin("born_radii", stream);
  MI_GB_DISPATCH(MI_GB_RADII);
  mi_timing_end(stream);
#undef MI_GB_RADII
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_born_energy(const void* cell, const int32_t* batch_idx, const double* weights, int n_atoms, int n_systems, int dtype,
                              const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors, int mask_value,
                              const double* params, int flags, const double* born_radii, double* energies, double* charge_grads, void* scratch,
                              size_t scratch_bytes, void* stream) {
  const int rc = gb_check_list(n_atoms, n_systems, dtype, cell, batch_idx, idx_j, unit_shifts, neighbor_ptr, max_neighbors, params, scratch, scratch_bytes);
  if (rc != MI_OK || n_atoms == 0) return rc;
  MI_REQUIRE(born_radii, "null pointer");
  MI_REQUIRE(energies || flags, "nothing to compute");
  MI_REQUIRE(!(flags & MI_GB_CHARGE_GRAD) || charge_grads, "charge gradient output");
  hipStream_t st = (hipStream_t)stream;
  const GbScratch s = gb_scratch(scratch, n_atoms, dtype);
  const GbParams p = gb_params(params);
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;
  double* cg = (flags & MI_GB_CHARGE_GRAD) ? charge_grads : nullptr;
  const int mode = (flags & MI_GB_VIRIAL) ? 2 : (flags & MI_GB_FORCES) ? 1 : 0;
  const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
#define MI_GB_ENERGY_ARGS(T_) (const GbRec<T_>*)s.rec, born_radii, s.chi, (const T_*)cell, bi, weights, n_atoms, idx_j, unit_shifts, neighbor_ptr, \
                              max_neighbors, mask_value, p, energies, cg, s.fdir, s.gchain, s.trow
#define MI_GB_ENERGY(T_, CSR_)                                                                                   \
  do {                                                                                                           \
    if (mode == 2) gb_energy_kernel<T_, CSR_, true, true><<<blocks, 256, 0, st>>>(MI_GB_ENERGY_ARGS(T_));        \
    else if (mode == 1) gb_energy_kernel<T_, CSR_, true, false><<<blocks, 256, 0, st>>>(MI_GB_ENERGY_ARGS(T_));  \
    else gb_energy_kernel<T_, CSR_, false, false><<<blocks, 256, 0, st>>>(MI_GB_ENERGY_ARGS(T_));                \
  } while (0)
  mi_timing_begin("born_energy", stream);
  MI_GB_DISPATCH(MI_GB_ENERGY);
  mi_timing_end(stream);
#undef MI_GB_ENERGY
#undef MI_GB_ENERGY_ARGS
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_born_chain(const void* cell, const int32_t* batch_idx, int n_atoms, int n_systems, int dtype, const int32_t* idx_j,
                             const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors, int mask_value, const double* params,
                             int flags, void* forces, double* system_partial, void* scratch, size_t scratch_bytes, void* stream) {
  const int rc = gb_check_list(n_atoms, n_systems, dtype, cell, batch_idx, idx_j, unit_shifts, neighbor_ptr, max_neighbors, params, scratch, scratch_bytes);
  if (rc != MI_OK) return rc;
  const bool wf = (flags & MI_GB_FORCES) != 0, wv = (flags & MI_GB_VIRIAL) != 0;
  MI_REQUIRE(wf || wv, "nothing to compute");
  MI_REQUIRE(!wf || forces || n_atoms == 0, "forces output");
  MI_REQUIRE(!wv || (cell && system_partial), "virial needs cell and system_partial");
  if (n_atoms == 0) return MI_OK;
  hipStream_t st = (hipStream_t)stream;
  const GbScratch s = gb_scratch(scratch, n_atoms, dtype);
  const GbParams p = gb_params(params);
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;
  const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
#define MI_GB_CHAIN_ARGS(T_) (const GbRec<T_>*)s.rec, s.gchain, s.fdir, (const T_*)cell, bi, n_atoms, idx_j, unit_shifts, neighbor_ptr, max_neighbors, \
                             mask_value, p, (T_*)(wf ? forces : nullptr), s.trow
#define MI_GB_CHAIN(T_, CSR_)                                                                        \
  do {                                                                                               \
    if (wv) gb_chain_kernel<T_, CSR_, true><<<blocks, 256, 0, st>>>(MI_GB_CHAIN_ARGS(T_));           \
    else gb_chain_kernel<T_, CSR_, false><<<blocks, 256, 0, st>>>(MI_GB_CHAIN_ARGS(T_));             \
  } while (0)
  mi_timing_begin("born_chain", stream);
  MI_GB_DISPATCH(MI_GB_CHAIN);
  mi_timing_end(stream);
#undef MI_GB_CHAIN
#undef MI_GB_CHAIN_ARGS
  MI_LAUNCH_CHECK();
  if (wv) {
    gb_fold_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>(s.trow, bi, n_atoms, system_partial);
    MI_LAUNCH_CHECK();
  }
  return MI_OK;
}
