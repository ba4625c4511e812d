// vdw.hip -- van der Waals pair potentials between reduced sites: Halgren's buffered 14-7 (AMOEBA) and Lennard-Jones.  gfx950, wave64.
// Driver: nvalchemiops/interactions/vdw/pair.py.  The reference package has no counterpart; written from the definitions.
//
// Over the stored entries (i, j, S) of a FULL (symmetric) list, with d = site_j - site_i + S . cell, r = |d|, rho = r / R_ij:
//     E_i = 1/2 sum_{entries of row i} s_e T(r) U_ij(r)
//     MI_VDW_BUFFERED_14_7   U = eps_ij ((1 + delta) / (rho + delta))^7 ((1 + gamma) / (rho^7 + gamma) - 2)
//     MI_VDW_LENNARD_JONES   U = eps_ij (rho^-12 - 2 rho^-6)
// R is the minimum-energy distance (R_min, not sigma) of both kinds: U(R_ij) = -eps_ij.  T is Tinker's quintic switch between taper_on and
// cutoff, T = 1 - 10 t^3 + 15 t^4 - 6 t^5, t = (r - taper_on) / (cutoff - taper_on); s_e the caller's per-entry scale (NULL: 1).  Entries with
// r^2 >= cutoff^2 leave before the square root; r <= 1e-8 contributes nothing.
//
// Three kernels.
//   pack     one thread per atom writes the 8-word record {site x, y, z, R, R^2, R^3, eps, sqrt(eps)} in the positions dtype (32 / 64 bytes: one
//            gather per neighbour).  The site of a reduced atom, site = r_i - (1 - kappa) (r_i - r_p) with r_i - r_p the minimum image -- kept at the atom's
//            OWN image, so the list's shifts, which belong to the atom's stored position, hold for its site -- is formed in
//            fp64 and rounded once.  An atom with R <= 0, eps <= 0 or NaN has no site: its parameter words are 0 and the pair loop tests eps alone.
//   pair     one wave64 per row, lanes stride the row (pair_row.h).  Pair vector and r^2 in the positions dtype, everything after that fp64;
//            rho^7 and rho^-6 by multiplication, one square root (two with the geometric radius rule), no other library call.  The row owner
//            alone writes -- the list is full, so owner sums stand for both ends -- no atomics, fixed order, bit-reproducible.  The kind is a
//            template parameter; the combining rules are wave-uniform branches on two integers.
//   gather   (only with reduced sites) one thread per atom: forces[a] = kappa_a F_a + sum_{children c of a, index order} (1 - kappa_c) F_c from
//            the fp64 site forces the pair kernel left in scratch, cast once at the store.
//
// The pair kernel is its own adjoint.  With weights g[N] (NULL: ones) every entry carries w = (g_i + g_j) / 2 and the owner sums are the
// derivatives of L = sum_i g_i E_i.  With P = T U, P' = T' U + T dU/drho / R_ij:
//     site force   F_i          = sum_row w s P' d / r                                   (= -dL/dsite_i)
//     dL/dR_i      = sum_row w s T dU/drho (-rho / R_ij) dR_ij/dR_i
//     dL/deps_i    = sum_row w s T (U / eps_ij) deps_ij/deps_i
//     virial       W[a][b]      = -1/2 sum_entries w s P' d_a d_b / r                    (-dE/d(strain); sites strain with the atoms)
//   14-7: A = ((1 + delta) / (rho + delta))^7, b = (1 + gamma) / (rho^7 + gamma):  U / eps = A (b - 2),
//         dU/drho / eps = -7 A ((b - 2) / (rho + delta) + b rho^6 / (rho^7 + gamma))
//   LJ:   dU/drho / eps = -12 (rho^-12 - rho^-6) / rho
//   radius rules    arithmetic (R_i + R_j) / 2: 1/2;  geometric sqrt(R_i R_j): R_ij / (2 R_i);
//                   cubic-mean (R_i^3 + R_j^3) / (R_i^2 + R_j^2): (3 R_i^2 - 2 R_i R_ij) / (R_i^2 + R_j^2)
//   epsilon rules   geometric sqrt(eps_i eps_j): sqrt(eps_j) / (2 sqrt(eps_i));
//                   hhg 4 eps_i eps_j / (sqrt(eps_i) + sqrt(eps_j))^2: 4 sqrt(eps_j)^3 / (sqrt(eps_i) + sqrt(eps_j))^3
#include "common.h"

namespace {

#include "pair_row.h"

#define VDW_ROW_WORDS 6  // doubles per row of the per-row virial buffer {xx, yy, zz, xy, xz, yz}

template <class T> struct VdwRec { T x, y, z, R, R2, R3, eps, seps; };  // 32 / 64 bytes

struct VdwModel {
  double cut2, ron, tinv;       // cutoff^2; taper_on and 1 / (cutoff - taper_on), or cutoff and 0 without a taper
  double delta, dp1, gamma, gp1;  // 14-7 buffers: delta, 1 + delta, gamma, 1 + gamma
  int rrule, erule;
};

// a reduced atom: parent names another atom of [0, N)
__device__ __forceinline__ bool vdw_reduced(const int* __restrict__ parent, int i, int N) {
  if (!parent) return false;
  const int p = parent[i];
  return (unsigned)p < (unsigned)N && p != i;
}

template <class T>
__global__ __launch_bounds__(256) void vdw_pack_kernel(const T* __restrict__ pos, const T* __restrict__ radii, const T* __restrict__ eps,
                                                       const int* __restrict__ parent, const T* __restrict__ reduction, const T* __restrict__ cell,
                                                       const int* __restrict__ batch_idx, int N, VdwRec<T>* __restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  double x = (double)pos[3 * (size_t)i], y = (double)pos[3 * (size_t)i + 1], z = (double)pos[3 * (size_t)i + 2];
  if (vdw_reduced(parent, i, N)) {
    const size_t p = (size_t)parent[i];
    const double k = (double)reduction[i];
    const double px = (double)pos[3 * p], py = (double)pos[3 * p + 1], pz = (double)pos[3 * p + 2];
    double dx = x - px, dy = y - py, dz = z - pz;
    if (cell) {  // minimum image of r_i - r_p, as the frame vectors of frames.hip
      double m[9], inv[9];
      const size_t s = batch_idx ? (size_t)batch_idx[i] : 0;
#pragma unroll
      for (int c = 0; c < 9; ++c) m[c] = (double)cell[9 * s + c];
      inverse3(m, inv);
      const double n0 = rint(dx * inv[0] + dy * inv[3] + dz * inv[6]);
      const double n1 = rint(dx * inv[1] + dy * inv[4] + dz * inv[7]);
      const double n2 = rint(dx * inv[2] + dy * inv[5] + dz * inv[8]);
      dx -= n0 * m[0] + n1 * m[3] + n2 * m[6];
      dy -= n0 * m[1] + n1 * m[4] + n2 * m[7];
      dz -= n0 * m[2] + n1 * m[5] + n2 * m[8];
    }
    x -= (1.0 - k) * dx; y -= (1.0 - k) * dy; z -= (1.0 - k) * dz;
  }
  const double R = (double)radii[i], e = (double)eps[i];
  const bool site = R > 0.0 && e > 0.0;  // (NaN fails both)
  VdwRec<T> r;
  r.x = (T)x; r.y = (T)y; r.z = (T)z;
  r.R = site ? (T)R : T(0); r.R2 = site ? (T)(R * R) : T(0); r.R3 = site ? (T)(R * R * R) : T(0);
  r.eps = site ? (T)e : T(0); r.seps = site ? (T)sqrt(e) : T(0);
  rec[i] = r;
}

template <class T, int KIND, bool CSR>
__global__ __launch_bounds__(256) void vdw_pair_kernel(const VdwRec<T>* __restrict__ rec, const T* __restrict__ cell, const int* __restrict__ batch_idx,
                                                       const double* __restrict__ g, const float* __restrict__ ps32, const double* __restrict__ ps64,
                                                       int N, const int* __restrict__ idx, const int* __restrict__ ush, const int* __restrict__ nptr,
                                                       int M, int mask_value, int flags, VdwModel P, double* __restrict__ energies,
                                                       T* __restrict__ forces, double* __restrict__ fsite, double* __restrict__ rgrad,
                                                       double* __restrict__ egrad, double* __restrict__ trow) {
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const int i = pair_row_index();
  if (i >= N) return;
  const bool shifted = ush != nullptr && cell != nullptr;
  T cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (shifted) pair_row_cell(cell, batch_idx ? batch_idx[i] : 0, cm);
  const VdwRec<T> ri = rec[i];
  // float32 records: R^2 and R^3 rounded to float32 would cost the cubic-mean rule as much as one ulp of r^2 does, so the
  // powers are taken from R in fp64; the float64 record's words are used as packed
  const bool wide = sizeof(T) == sizeof(double);
  const double Ri = (double)ri.R, Ri2 = wide ? (double)ri.R2 : Ri * Ri, Ri3 = wide ? (double)ri.R3 : Ri * Ri * Ri, si = (double)ri.seps;
  const double gi = g ? g[i] : 1.0;
  const bool wf = (flags & MI_VDW_FORCES) != 0, wr = (flags & MI_VDW_RADIUS_GRAD) != 0, we = (flags & MI_VDW_EPSILON_GRAD) != 0;
  const bool wv = (flags & MI_VDW_VIRIAL) != 0;
  long long beg, end;
  pair_row_range<CSR>(nptr, i, M, beg, end);
  if (ri.eps == T(0)) end = beg;  // no site: the row is skipped, every output of the atom is exactly 0
  double eacc = 0.0, racc = 0.0, gacc = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
  double t[VDW_ROW_WORDS] = {0, 0, 0, 0, 0, 0};
  for (long long e = beg + lane; e < end; e += MI_WAVE) {
    const int j = idx[e];
    if (pair_is_padding<CSR>(j, mask_value, N)) continue;
    const VdwRec<T> rj = rec[j];
    if (rj.eps == T(0)) continue;
    T sx = rj.x - ri.x, sy = rj.y - ri.y, sz = rj.z - ri.z;
    if (shifted) {
      T sh[3];
      pair_separation(ush, e, cm, sh);
      sx += sh[0]; sy += sh[1]; sz += sh[2];
    }
    const T r2t = sx * sx + sy * sy + sz * sz;
    const double r2 = (double)r2t;
    if (!(r2 < P.cut2)) continue;  // beyond the cutoff (and NaN distances): before the square root
    const double r = sqrt(r2);
    if (!(r > 1e-8)) continue;
    // combining rules: R_ij, dR_ij/dR_i, eps_ij, deps_ij/deps_i
    const double Rj = (double)rj.R, sj = (double)rj.seps;
    double Rij, dRi, eij, dei;
    if (P.rrule == MI_VDW_RADIUS_ARITHMETIC) { Rij = 0.5 * (Ri + Rj); dRi = 0.5; }
    else if (P.rrule == MI_VDW_RADIUS_GEOMETRIC) { Rij = sqrt(Ri * Rj); dRi = 0.5 * Rij / Ri; }
    else {
      const double Rj2 = wide ? (double)rj.R2 : Rj * Rj, Rj3 = wide ? (double)rj.R3 : Rj2 * Rj;
      const double Dinv = 1.0 / (Ri2 + Rj2);
      Rij = (Ri3 + Rj3) * Dinv; dRi = (3.0 * Ri2 - 2.0 * Ri * Rij) * Dinv;
    }
    if (P.erule == MI_VDW_EPSILON_GEOMETRIC) { eij = si * sj; dei = 0.5 * sj / si; }
    else { const double q = 1.0 / (si + sj), h = 2.0 * si * sj * q, c = sj * q; eij = h * h; dei = 4.0 * c * c * c; }
    const double Rinv = 1.0 / Rij, rinv = 1.0 / r;
    const double rho = r * Rinv;
    double u, du;  // U / eps_ij and dU/drho / eps_ij
    if (KIND == MI_VDW_BUFFERED_14_7) {
      const double rho2 = rho * rho, rho3 = rho2 * rho, rho6 = rho3 * rho3, rho7 = rho6 * rho;
      const double ainv = 1.0 / (rho + P.delta), binv = 1.0 / (rho7 + P.gamma);
      const double a = P.dp1 * ainv, a2 = a * a, a4 = a2 * a2, a7 = a4 * a2 * a;
      const double b = P.gp1 * binv;
      u = a7 * (b - 2.0);
      du = -7.0 * a7 * ((b - 2.0) * ainv + b * binv * rho6);
    } else {
      const double q = Rij * rinv, q2 = q * q, q6 = q2 * q2 * q2, q12 = q6 * q6;
      u = q12 - 2.0 * q6;
      du = -12.0 * (q12 - q6) * q;
    }
    double tt = 1.0, dt = 0.0;
    if (r > P.ron) {
      const double x = (r - P.ron) * P.tinv, y = 1.0 - x;
      tt = 1.0 - x * x * x * (10.0 - 15.0 * x + 6.0 * x * x);
      dt = -30.0 * (x * x) * (y * y) * P.tinv;
    }
    const double s = ps32 ? (double)ps32[e] : (ps64 ? ps64[e] : 1.0);
    const double w = g ? 0.5 * (gi + g[j]) : 1.0;
    eacc += 0.5 * (s * eij) * (tt * u);
    const double ws = w * s;
    if (wr) racc -= ws * eij * tt * du * (rho * Rinv) * dRi;
    if (we) gacc += ws * tt * u * dei;
    if (wf || wv) {
      const double fm = ws * eij * (dt * u + tt * du * Rinv) * rinv;
      const double dx = (double)sx, dy = (double)sy, dz = (double)sz;
      fx += fm * dx; fy += fm * dy; fz += fm * dz;
      if (wv) {
        const double hm = 0.5 * fm;
        t[0] -= hm * (dx * dx); t[1] -= hm * (dy * dy); t[2] -= hm * (dz * dz);
        t[3] -= hm * (dx * dy); t[4] -= hm * (dx * dz); t[5] -= hm * (dy * dz);
      }
    }
  }
  if (energies) { eacc = wave_sum(eacc); if (lane == 0) energies[i] = eacc; }
  if (wf) {
    fx = wave_sum(fx); fy = wave_sum(fy); fz = wave_sum(fz);
    if (lane == 0) {
      if (fsite) { fsite[3 * (size_t)i] = fx; fsite[3 * (size_t)i + 1] = fy; fsite[3 * (size_t)i + 2] = fz; }
      else { forces[3 * (size_t)i] = (T)fx; forces[3 * (size_t)i + 1] = (T)fy; forces[3 * (size_t)i + 2] = (T)fz; }
    }
  }
  if (wr) { racc = wave_sum(racc); if (lane == 0) rgrad[i] = racc; }
  if (we) { gacc = wave_sum(gacc); if (lane == 0) egrad[i] = gacc; }
  if (wv) {
#pragma unroll
    for (int k = 0; k < VDW_ROW_WORDS; ++k) t[k] = wave_sum(t[k]);
    if (lane == 0) {
      double* o = trow + VDW_ROW_WORDS * (size_t)i;
#pragma unroll
      for (int k = 0; k < VDW_ROW_WORDS; ++k) o[k] = t[k];
    }
  }
}

// forces on ATOMS from the site forces: atom a keeps kappa_a of its own site's force and receives (1 - kappa_c) of each child's, children in
// index order (the inverse CSR of ReducedSites).  One thread per atom, plain stores.
template <class T>
__global__ __launch_bounds__(256) void vdw_gather_kernel(const double* __restrict__ fsite, const int* __restrict__ parent, const T* __restrict__ reduction,
                                                         const int* __restrict__ cptr, const int* __restrict__ cidx, long long n_children, int N,
                                                         T* __restrict__ forces) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= N) return;
  const double ka = vdw_reduced(parent, a, N) ? (double)reduction[a] : 1.0;
  double fx = ka * fsite[3 * (size_t)a], fy = ka * fsite[3 * (size_t)a + 1], fz = ka * fsite[3 * (size_t)a + 2];
  long long beg = cptr[a], end = cptr[a + 1];
  if (beg < 0) beg = 0;
  if (end > n_children) end = n_children;
  for (long long e = beg; e < end; ++e) {
    const int c = cidx[e];
    if ((unsigned)c >= (unsigned)N) continue;
    const double kc = 1.0 - (double)reduction[c];
    fx += kc * fsite[3 * (size_t)c]; fy += kc * fsite[3 * (size_t)c + 1]; fz += kc * fsite[3 * (size_t)c + 2];
  }
  forces[3 * (size_t)a] = (T)fx; forces[3 * (size_t)a + 1] = (T)fy; forces[3 * (size_t)a + 2] = (T)fz;
}

// per-system fold of the per-row virial words: partial[s][x][0..6) with plain stores; the caller sums the MI_FOLD_BLOCKS rows.  No atomics.
__global__ __launch_bounds__(256) void vdw_fold_kernel(const double* __restrict__ trow, const int* __restrict__ batch_idx, int N,
                                                       double* __restrict__ partial) {
  mi_system_fold<VDW_ROW_WORDS, MI_FOLD_BLOCKS>(batch_idx, N, VDW_ROW_WORDS, partial, [&](long long r, double* a) {
#pragma unroll
    for (int k = 0; k < VDW_ROW_WORDS; ++k) a[k] += trow[VDW_ROW_WORDS * r + k];
  });
}

size_t vdw_count(int n_atoms) { return (size_t)(n_atoms > 0 ? n_atoms : 0); }
size_t vdw_rec_bytes(int n_atoms, int dtype) { return mi_align((dtype == MI_F32 ? sizeof(VdwRec<float>) : sizeof(VdwRec<double>)) * vdw_count(n_atoms)); }
size_t vdw_row_bytes(int n_atoms) { return mi_align(sizeof(double) * VDW_ROW_WORDS * vdw_count(n_atoms)); }

}  // namespace

extern "C" int mi_vdw_blocks(void) { return MI_FOLD_BLOCKS; }
extern "C" int mi_vdw_row_words(void) { return VDW_ROW_WORDS; }
extern "C" size_t mi_vdw_scratch_bytes(int n_atoms, int dtype, int with_sites) {
  return vdw_rec_bytes(n_atoms, dtype) + vdw_row_bytes(n_atoms) + (with_sites ? mi_align(sizeof(double) * 3 * vdw_count(n_atoms)) : 0);
}

extern "C" int mi_vdw(const void* positions, const void* radii, const void* epsilons, const void* cell, const int32_t* batch_idx,
                      const double* weights, const int32_t* parent, const void* reduction, const int32_t* child_ptr, const int32_t* child_idx,
                      long long n_children, const void* pair_scales, int pair_scales_dtype, int n_atoms, int n_systems, int dtype, int kind,
                      int radius_rule, int epsilon_rule, double delta, double gamma, double cutoff, double taper_on, const int32_t* idx_j,
                      const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors, int mask_value, int flags, double* energies,
                      void* forces, double* radius_grads, double* epsilon_grads, double* system_partial, void* scratch, size_t scratch_bytes,
                      void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(kind == MI_VDW_BUFFERED_14_7 || kind == MI_VDW_LENNARD_JONES, "kind");
  MI_REQUIRE(radius_rule >= MI_VDW_RADIUS_ARITHMETIC && radius_rule <= MI_VDW_RADIUS_CUBIC_MEAN, "radius_rule");
  MI_REQUIRE(epsilon_rule == MI_VDW_EPSILON_GEOMETRIC || epsilon_rule == MI_VDW_EPSILON_HHG, "epsilon_rule");
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(cutoff > 0.0, "cutoff must be positive");
  MI_REQUIRE(taper_on < 0.0 || (taper_on > 0.0 && taper_on < cutoff), "taper_on must lie inside (0, cutoff), or be negative for none");
  MI_REQUIRE(kind != MI_VDW_BUFFERED_14_7 || (delta > 0.0 && gamma > 0.0), "delta and gamma must be positive");
  MI_REQUIRE(!(flags & MI_VDW_VIRIAL) || (cell && system_partial), "virial needs cell and system_partial");
  MI_REQUIRE(!unit_shifts || cell, "unit_shifts without a cell");
  MI_REQUIRE(!pair_scales || pair_scales_dtype == MI_F32 || pair_scales_dtype == MI_F64, "pair_scales_dtype");
  const bool sites = parent != nullptr;
  MI_REQUIRE(!sites || (reduction && child_ptr && (child_idx || n_children == 0) && n_children >= 0), "reduced sites need parent, reduction and the child CSR");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && radii && epsilons && idx_j, "null pointer");
  MI_REQUIRE(energies || flags, "nothing to compute");
  MI_REQUIRE(!(flags & MI_VDW_FORCES) || forces, "forces output");
  MI_REQUIRE(!(flags & MI_VDW_RADIUS_GRAD) || radius_grads, "radius gradient output");
  MI_REQUIRE(!(flags & MI_VDW_EPSILON_GRAD) || epsilon_grads, "epsilon gradient output");
  MI_REQUIRE(scratch && scratch_bytes >= mi_vdw_scratch_bytes(n_atoms, dtype, sites ? 1 : 0), "scratch smaller than mi_vdw_scratch_bytes()");
  hipStream_t st = (hipStream_t)stream;
  double* trow = reinterpret_cast<double*>((char*)scratch + vdw_rec_bytes(n_atoms, dtype));
  double* fsite = sites ? reinterpret_cast<double*>((char*)trow + vdw_row_bytes(n_atoms)) : nullptr;
  VdwModel P;
  P.cut2 = cutoff * cutoff;
  P.ron = taper_on > 0.0 ? taper_on : cutoff;
  P.tinv = taper_on > 0.0 ? 1.0 / (cutoff - taper_on) : 0.0;
  P.delta = delta; P.dp1 = 1.0 + delta; P.gamma = gamma; P.gp1 = 1.0 + gamma;
  P.rrule = radius_rule; P.erule = epsilon_rule;
  const float* ps32 = pair_scales && pair_scales_dtype == MI_F32 ? (const float*)pair_scales : nullptr;
  const double* ps64 = pair_scales && pair_scales_dtype == MI_F64 ? (const double*)pair_scales : nullptr;
  const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
  // one system: every atom belongs to system 0 and the batch index is not read
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;
#define MI_VDW_RUN(T_, KIND_, CSR_)                                                                                                            \
  do {                                                                                                                                         \
    vdw_pack_kernel<T_><<<mi_blocks(n_atoms, 256), 256, 0, st>>>((const T_*)positions, (const T_*)radii, (const T_*)epsilons, parent,          \
                                                                 (const T_*)reduction, (const T_*)cell, bi, n_atoms, (VdwRec<T_>*)scratch);    \
    vdw_pair_kernel<T_, KIND_, CSR_><<<blocks, 256, 0, st>>>((const VdwRec<T_>*)scratch, (const T_*)cell, bi, weights, ps32, ps64, n_atoms,    \
                                                             idx_j, unit_shifts, neighbor_ptr, max_neighbors, mask_value, flags, P, energies,  \
                                                             (T_*)forces, fsite, radius_grads, epsilon_grads, trow);                           \
    if (sites && (flags & MI_VDW_FORCES))                                                                                                      \
      vdw_gather_kernel<T_><<<mi_blocks(n_atoms, 256), 256, 0, st>>>(fsite, parent, (const T_*)reduction, child_ptr, child_idx, n_children,    \
                                                                     n_atoms, (T_*)forces);                                                    \
  } while (0)
#define MI_VDW_KIND(T_, CSR_)                                                                  \
  do {                                                                                         \
    if (kind == MI_VDW_BUFFERED_14_7) MI_VDW_RUN(T_, MI_VDW_BUFFERED_14_7, CSR_);              \
    else MI_VDW_RUN(T_, MI_VDW_LENNARD_JONES, CSR_);                                           \
  } while (0)
  mi_timing_begin(kind == MI_VDW_BUFFERED_14_7 ? "vdw_buffered_14_7" : "vdw_lennard_jones", stream);
  if (dtype == MI_F32) { if (neighbor_ptr) MI_VDW_KIND(float, true); else MI_VDW_KIND(float, false); }
  else { if (neighbor_ptr) MI_VDW_KIND(double, true); else MI_VDW_KIND(double, false); }
  mi_timing_end(stream);
#undef MI_VDW_KIND
#undef MI_VDW_RUN
  MI_LAUNCH_CHECK();
  if (flags & MI_VDW_VIRIAL) {
    vdw_fold_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>(trow, bi, n_atoms, system_partial);
    MI_LAUNCH_CHECK();
  }
  return MI_OK;
}
