// dispersion_ewald.hip -- explicit-k Ewald sum of the r^-6 dispersion energy E = -1/2 sum'_{i,j,n} c_i c_j / |r_j - r_i + n|^6.  gfx950, wave64.
// Driver: nvalchemiops/interactions/vdw/ewald.py.  The reference package has no counterpart; written from the definitions.
//
// With beta = alpha, a = beta r, g(a) = exp(-a^2) (1 + a^2 + a^4 / 2), b = |k| / (2 beta), S(k) = sum_j c_j e^{i k.r_j}:
//     real space   E_i = -1/2 sum_{entries of row i} c_i c_j (g(beta r) - T_c(r)) / r^6                          (FULL list; r <= 1e-8 skipped)
//     reciprocal   E_i = c_i sum_{k in half space} w_k Re[e^{-i k.r_i} S(k)] + w_0 c_i S(0) + (beta^6 / 12) c_i^2
//                  w_k = -(pi^1.5 beta^3 / (3 V)) f(b),  f(b) = (1 - 2 b^2) exp(-b^2) + 2 sqrt(pi) b^3 erfc(b),  w_0 = -(pi^1.5 beta^3 / (6 V))
// T_c is the part a truncated Lennard-Jones sum has already counted: Tinker's quintic switch as vdw.hip forms it (1 below the taper, 0 from
// the cutoff on), identically 0 in the plain kind.
//
// Real space: pair_row.h's walk -- one wave64 per row, lanes stride the entries, the row owner sums in fp64 and writes alone.
//   pack   pair_pack_kernel writes {x, y, z, c} in the positions dtype: one 16 / 32-byte gather per neighbour.
//   pair   pair vector and r^2 in the positions dtype, the rest fp64; one exp and one division per entry, r^-6 = (1 / r^2)^3.  COUNTED is a
//          template parameter.  In it g - T_c = (g - 1) + (1 - T_c): 1 - T_c = t^3 (10 - 15 t + 6 t^2) has no cancellation, and
//          1 - g = exp(-a^2) sum_{n >= 3} a^(2n) / n! is summed as that series (positive terms, n <= 20) for a^2 < 1 and formed as the
//          difference above it, where it is right to 2 ulp.  One square root, only inside the taper window.
//   With P = (g - T_c) / r^6 and weights g (NULL: ones), w = (g_i + g_j) / 2, the owner sums are the derivatives of L = sum_i g_i E_i:
//     forces_i = sum_row w (-c_i c_j) P' d / r,   dL/dc_i = -sum_row w c_j P,   W[a][b] = 1/2 sum_entries w c_i c_j P' d_a d_b / r
//     P' / r = ((g' - T_c') / r - 6 (g - T_c) / r^2) / r^6,   g' / r = -beta^2 a^4 exp(-a^2)
//
// Reciprocal space: the table word is one complex number and the per-k factor one scalar, so the split is the opposite of dipole.hip's
// block-per-k / wave-per-atom (which pays a cross-lane reduction per k and per atom): a thread owns a k-vector (structure factors) or an
// atom (gather) and keeps its sums in registers; the other index comes through LDS by broadcast reads.  No reduction, no atomics.
//   structure factors   block (k tile, atom tile, system) stages {x, y, z, g_j c_j} of its atoms in LDS; thread = one k walks the tile and
//                       writes one partial per (atom tile, k).  The fold adds a system's tiles in index order and writes the table
//                       {Re S, Im S} and the gather records {k_x, k_y, k_z, w_k Re S, w_k Im S}: erfc and exp once per k.  Slot K of every
//                       system is k = 0 (S(0) = sum_j c_j, weight w_0), so the k = 0 term needs no pass of its own.
//   gather              block stages a tile of records in LDS; thread = one atom: with X = S (f = 2) or X = g_i S + S^g (adjoint, f = 1),
//                       e^{i k.r_i} = cs + i sn, v = Re X cs + Im X sn, u = Im X cs - Re X sn:
//                         E_i = c_i sum v + (beta^6 / 12) c_i^2,  forces_i = -f c_i sum u k,  dL/dc_i = f sum v + g_i (beta^6 / 6) c_i
//   virial              one block per system over the table: W[a][b] = sum_k |S|^2 (w_k delta_ab + v_k k_a k_b),
//                       v_k = -(pi^1.5 beta^3 / (3 V)) f'(b) / (2 beta |k|) = (pi^1.5 beta^3 / (3 V)) 1.5 (exp(-b^2) - sqrt(pi) b erfc(b)) / beta^2
//                       (f' = 6 b (sqrt(pi) b erfc(b) - exp(-b^2)), d|k|/d eps_ab = -k_a k_b / |k|, 1/V carries w_k delta_ab; the self term has none).
// Phases are fp64.  Atoms of one system are contiguous (system_ptr / a monotonic batch_idx), as for the other reciprocal sums.
#include "common.h"

namespace {

#include "pair_row.h"

#define DE_ROW_WORDS 6    // doubles per row of the per-row virial buffer {xx, yy, zz, xy, xz, yz}
#define DE_ATOM_TILE 256  // atoms a structure-factor block stages
#define DE_K_TILE 256     // k-vectors per block: one per thread (structure factors), records a gather block stages
#define DE_REC_WORDS 5    // {k_x, k_y, k_z, w Re S, w Im S}
#define DE_SQRT_PI 1.7724538509055159
#define DE_PI_15 5.5683279968317078  // pi^1.5

template <class T> struct DeRec {
  T x, y, z, q;  // q: the dispersion coefficient c
  __device__ __forceinline__ void set_tail(const T*, size_t) {}
};

struct DeCounted { double rc2, ron2, ron, tinv; };  // cutoff^2, taper^2, taper, 1 / (cutoff - taper); without a taper: taper = cutoff, tinv = 0

// sum_{n >= 3}^{20} a2^n / n!, Horner from the inside: every term positive
__device__ __forceinline__ double de_series(double a2) {
  double s = 1.0;
#pragma unroll
  for (int n = 20; n >= 4; --n) s = fma(s, a2 * (1.0 / n), 1.0);
  return a2 * a2 * a2 * (1.0 / 6.0) * s;
}

template <class T, bool COUNTED, bool CSR>
__global__ __launch_bounds__(256) void de_pair_kernel(const DeRec<T>* __restrict__ rec, const T* __restrict__ cell, const T* __restrict__ alpha,
                                                      const int* __restrict__ batch_idx, const double* __restrict__ g, int N,
                                                      const int* __restrict__ idx, const int* __restrict__ ush, const int* __restrict__ nptr, int M,
                                                      int mask_value, int flags, DeCounted P, double* __restrict__ energies, T* __restrict__ forces,
                                                      double* __restrict__ cgrad, double* __restrict__ trow) {
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const int i = pair_row_index();
  if (i >= N) return;
  const int s = batch_idx ? batch_idx[i] : 0;
  const bool shifted = ush != nullptr;
  T cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (shifted) pair_row_cell(cell, s, cm);
  const DeRec<T> ri = rec[i];
  const double ci = (double)ri.q, gi = g ? g[i] : 1.0;
  const double be = (double)alpha[s], be2 = be * be;
  const bool wf = (flags & MI_DE_FORCES) != 0, wc = (flags & MI_DE_COEFFICIENT_GRAD) != 0, wv = (flags & MI_DE_VIRIAL) != 0;
  long long beg, end;
  pair_row_range<CSR>(nptr, i, M, beg, end);
  double eacc = 0.0, cacc = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
  double t[DE_ROW_WORDS] = {0, 0, 0, 0, 0, 0};
  for (long long e = beg + lane; e < end; e += MI_WAVE) {
    const int j = idx[e];
    if (pair_is_padding<CSR>(j, mask_value, N)) continue;
    const DeRec<T> rj = rec[j];
    if (rj.q == T(0)) continue;  // contributes exact zeros to every sum of the row
    T sx = rj.x - ri.x, sy = rj.y - ri.y, sz = rj.z - ri.z;
    if (shifted) {
      T sh[3];
      pair_separation(ush, e, cm, sh);
      sx += sh[0]; sy += sh[1]; sz += sh[2];
    }
    const T r2t = sx * sx + sy * sy + sz * sz;
    const double r2 = (double)r2t;
    if (!(r2 > 1e-16)) continue;  // r <= 1e-8 (and NaN distances)
    const double a2 = be2 * r2, ex = exp(-a2);
    const double ri2 = 1.0 / r2, ri6 = ri2 * ri2 * ri2;
    double ker = ex * (1.0 + a2 + 0.5 * (a2 * a2));  // g - T_c
    double dker = -be2 * (a2 * a2) * ex;             // (g' - T_c') / r
    if (COUNTED) {
      if (r2 < P.rc2) {
        ker = a2 < 1.0 ? -ex * de_series(a2) : ker - 1.0;
        if (r2 > P.ron2) {
          const double r = sqrt(r2), x = (r - P.ron) * P.tinv, y = 1.0 - x;
          ker += x * x * x * (10.0 - 15.0 * x + 6.0 * (x * x));
          dker += 30.0 * (x * x) * (y * y) * P.tinv * (r * ri2);
        }
      }
    }
    const double cj = (double)rj.q;
    const double w = g ? 0.5 * (gi + g[j]) : 1.0;
    const double p = ker * ri6;
    eacc -= 0.5 * (ci * cj) * p;
    if (wc) cacc -= w * cj * p;
    if (wf || wv) {
      const double fm = -w * (ci * cj) * ri6 * (dker - 6.0 * ker * ri2);
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
    if (lane == 0) { forces[3 * (size_t)i] = (T)fx; forces[3 * (size_t)i + 1] = (T)fy; forces[3 * (size_t)i + 2] = (T)fz; }
  }
  if (wc) { cacc = wave_sum(cacc); if (lane == 0) cgrad[i] = cacc; }
  if (wv) {
#pragma unroll
    for (int k = 0; k < DE_ROW_WORDS; ++k) t[k] = wave_sum(t[k]);
    if (lane == 0) {
      double* o = trow + DE_ROW_WORDS * (size_t)i;
#pragma unroll
      for (int k = 0; k < DE_ROW_WORDS; ++k) o[k] = t[k];
    }
  }
}

// per-system fold of the per-row virial words: partial[s][x][0..6) with plain stores; the caller sums the MI_FOLD_BLOCKS rows.  No atomics.
__global__ __launch_bounds__(256) void de_fold_kernel(const double* __restrict__ trow, const int* __restrict__ batch_idx, int N,
                                                      double* __restrict__ partial) {
  mi_system_fold<DE_ROW_WORDS, MI_FOLD_BLOCKS>(batch_idx, N, DE_ROW_WORDS, partial, [&](long long r, double* a) {
#pragma unroll
    for (int k = 0; k < DE_ROW_WORDS; ++k) a[k] += trow[DE_ROW_WORDS * r + k];
  });
}

// ---- reciprocal space -------------------------------------------------------------------------------------------------------------------------
// atom tiles are global: tile t holds the atoms [t * DE_ATOM_TILE, (t + 1) * DE_ATOM_TILE); the part of tile t inside system b has the
// partial slot t + b (unique: the first tile of system b + 1 is not below the last of system b), (n_tiles + n_systems) slots in all
__device__ __forceinline__ void de_system_range(const int* __restrict__ sptr, int b, int n_atoms, int& a0, int& a1) {
  a0 = sptr ? sptr[b] : 0;
  a1 = sptr ? sptr[b + 1] : n_atoms;
  if (a0 < 0) a0 = 0;
  if (a1 > n_atoms) a1 = n_atoms;
}

template <class T> __device__ __forceinline__ double de_volume(const T* __restrict__ c) {
  const double m[9] = {(double)c[0], (double)c[1], (double)c[2], (double)c[3], (double)c[4], (double)c[5], (double)c[6], (double)c[7], (double)c[8]};
  return fabs(m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]));
}

// w_k, and v_k of the virial, of one slot: `zero` is the k = 0 slot; a caller's k-vector with |k|^2 < 1e-10 weighs nothing
__device__ __forceinline__ void de_weight(bool zero, double k2, double be, double vol, double& w, double& v) {
  const double pref = DE_PI_15 * be * be * be / (3.0 * vol);
  w = zero ? -0.5 * pref : 0.0;
  v = 0.0;
  if (zero || k2 < 1e-10) return;
  const double b = 0.5 * sqrt(k2) / be, b2 = b * b, eb = exp(-b2), ec = erfc(b);
  w = -pref * ((1.0 - 2.0 * b2) * eb + 2.0 * DE_SQRT_PI * (b2 * b) * ec);
  v = pref * 1.5 * (eb - DE_SQRT_PI * b * ec) / (be * be);
}

template <class T>
__global__ __launch_bounds__(DE_K_TILE) void de_sf_kernel(const T* __restrict__ pos, const T* __restrict__ c, const double* __restrict__ g,
                                                          const T* __restrict__ kvec, const int* __restrict__ sptr, int n_atoms, int K,
                                                          double* __restrict__ partial) {
  const int b = blockIdx.z, tile = blockIdx.y;
  int a0, a1;
  de_system_range(sptr, b, n_atoms, a0, a1);
  const int lo = max(a0, tile * DE_ATOM_TILE), hi = min(a1, (tile + 1) * DE_ATOM_TILE);
  if (lo >= hi) return;  // block-uniform: the tile has no atom of this system, its slot is never read
  __shared__ double4 at[DE_ATOM_TILE];
  const int count = hi - lo;
  for (int t = threadIdx.x; t < count; t += DE_K_TILE) {
    const size_t j = (size_t)(lo + t);
    const double cj = (double)c[j];
    at[t] = make_double4((double)pos[3 * j], (double)pos[3 * j + 1], (double)pos[3 * j + 2], g ? g[j] * cj : cj);
  }
  __syncthreads();
  const int k = blockIdx.x * DE_K_TILE + threadIdx.x;  // slot K: k = 0
  if (k > K) return;
  double kx = 0.0, ky = 0.0, kz = 0.0;
  if (k < K) {
    const T* kv = kvec + 3 * ((size_t)b * K + k);
    kx = (double)kv[0]; ky = (double)kv[1]; kz = (double)kv[2];
  }
  double sr = 0.0, si = 0.0;
  for (int t = 0; t < count; ++t) {
    const double4 a = at[t];  // every lane reads the same record: an LDS broadcast
    double sn, cs;
    sincos(kx * a.x + ky * a.y + kz * a.z, &sn, &cs);
    sr = fma(a.w, cs, sr); si = fma(a.w, sn, si);
  }
  double* o = partial + 2 * ((size_t)(tile + b) * (K + 1) + k);
  o[0] = sr; o[1] = si;
}

// table[b][k] = sum over the atom tiles of system b, in index order; records (NULL: not wanted) = {k, w_k S}
template <class T>
__global__ __launch_bounds__(256) void de_sf_fold_kernel(const double* __restrict__ partial, const T* __restrict__ kvec, const T* __restrict__ cell,
                                                         const T* __restrict__ alpha, const int* __restrict__ sptr, int n_atoms, int K,
                                                         double* __restrict__ table, double* __restrict__ records) {
  const int b = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x;
  if (k > K) return;
  int a0, a1;
  de_system_range(sptr, b, n_atoms, a0, a1);
  double sr = 0.0, si = 0.0;
  if (a1 > a0) {
    for (int tile = a0 / DE_ATOM_TILE; tile <= (a1 - 1) / DE_ATOM_TILE; ++tile) {
      const double* p = partial + 2 * ((size_t)(tile + b) * (K + 1) + k);
      sr += p[0]; si += p[1];
    }
  }
  const size_t slot = (size_t)b * (K + 1) + k;
  table[2 * slot] = sr; table[2 * slot + 1] = si;
  if (!records) return;
  double kx = 0.0, ky = 0.0, kz = 0.0;
  if (k < K) {
    const T* kv = kvec + 3 * ((size_t)b * K + k);
    kx = (double)kv[0]; ky = (double)kv[1]; kz = (double)kv[2];
  }
  double w, v;
  de_weight(k == K, kx * kx + ky * ky + kz * kz, (double)alpha[b], de_volume(cell + 9 * (size_t)b), w, v);
  double* r = records + DE_REC_WORDS * slot;
  r[0] = kx; r[1] = ky; r[2] = kz; r[3] = w * sr; r[4] = w * si;
}

template <class T, bool ADJ>
__global__ __launch_bounds__(256) void de_gather_kernel(const T* __restrict__ pos, const T* __restrict__ c, const T* __restrict__ alpha,
                                                        const int* __restrict__ batch_idx, const double* __restrict__ records,
                                                        const double* __restrict__ records_g, const double* __restrict__ g, int n_atoms,
                                                        int n_systems, int K, double* __restrict__ energies, T* __restrict__ forces,
                                                        double* __restrict__ cgrad) {
  const int first = blockIdx.x * 256, i = first + (int)threadIdx.x;
  const bool live = i < n_atoms;
  const int last = min(n_atoms, first + 256) - 1;
  // the systems of this block's atoms (contiguous per system): block-uniform loop bounds, clamped to the record table
  int b0 = batch_idx ? batch_idx[first] : 0, b1 = batch_idx ? batch_idx[last] : 0;
  b0 = min(max(b0, 0), n_systems - 1); b1 = min(max(b1, 0), n_systems - 1);
  const int mine = live ? (batch_idx ? batch_idx[i] : 0) : -1;
  const size_t a = (size_t)(live ? i : 0);
  const double x = (double)pos[3 * a], y = (double)pos[3 * a + 1], z = (double)pos[3 * a + 2];
  const double ci = (double)c[a], gi = ADJ ? g[a] : 1.0;
  __shared__ double kr[DE_K_TILE][ADJ ? 7 : 5];
  double vs = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
  for (int b = b0; b <= b1; ++b) {
    for (int k0 = 0; k0 <= K; k0 += DE_K_TILE) {
      const int count = min(DE_K_TILE, K + 1 - k0);
      __syncthreads();
      if ((int)threadIdx.x < count) {
        const size_t slot = (size_t)b * (K + 1) + k0 + threadIdx.x;
#pragma unroll
        for (int w = 0; w < DE_REC_WORDS; ++w) kr[threadIdx.x][w] = records[DE_REC_WORDS * slot + w];
        if (ADJ) { kr[threadIdx.x][5] = records_g[DE_REC_WORDS * slot + 3]; kr[threadIdx.x][6] = records_g[DE_REC_WORDS * slot + 4]; }
      }
      __syncthreads();
      if (b != mine) continue;
      for (int t = 0; t < count; ++t) {
        const double kx = kr[t][0], ky = kr[t][1], kz = kr[t][2];
        double xr = kr[t][3], xi = kr[t][4];
        if (ADJ) { xr = fma(gi, xr, kr[t][5]); xi = fma(gi, xi, kr[t][6]); }
        double sn, cs;
        sincos(kx * x + ky * y + kz * z, &sn, &cs);
        const double u = xi * cs - xr * sn;
        vs += xr * cs + xi * sn;
        fx = fma(u, kx, fx); fy = fma(u, ky, fy); fz = fma(u, kz, fz);
      }
    }
  }
  if (!live) return;
  const double be = (double)alpha[min(max(mine, 0), n_systems - 1)], be3 = be * be * be, self = be3 * be3 * (1.0 / 12.0);
  const double f = ADJ ? 1.0 : 2.0;
  if (energies) energies[i] = ci * vs + self * (ci * ci);
  if (forces) {
    const double m = -f * ci;
    forces[3 * a] = (T)(m * fx); forces[3 * a + 1] = (T)(m * fy); forces[3 * a + 2] = (T)(m * fz);
  }
  if (cgrad) cgrad[i] = f * vs + gi * (2.0 * self) * ci;
}

template <class T>
__global__ __launch_bounds__(256) void de_recip_virial_kernel(const double* __restrict__ table, const T* __restrict__ kvec, const T* __restrict__ cell,
                                                              const T* __restrict__ alpha, int K, double* __restrict__ virial) {
  const int b = blockIdx.x;
  const double be = (double)alpha[b], vol = de_volume(cell + 9 * (size_t)b);
  double a[DE_ROW_WORDS] = {0, 0, 0, 0, 0, 0};
  for (int k = threadIdx.x; k <= K; k += 256) {
    double kx = 0.0, ky = 0.0, kz = 0.0;
    if (k < K) {
      const T* kv = kvec + 3 * ((size_t)b * K + k);
      kx = (double)kv[0]; ky = (double)kv[1]; kz = (double)kv[2];
    }
    double w, v;
    de_weight(k == K, kx * kx + ky * ky + kz * kz, be, vol, w, v);
    const double* s = table + 2 * ((size_t)b * (K + 1) + k);
    const double s2 = s[0] * s[0] + s[1] * s[1];
    const double d = w * s2, o = v * s2;
    a[0] += d + o * (kx * kx); a[1] += d + o * (ky * ky); a[2] += d + o * (kz * kz);
    a[3] += o * (kx * ky); a[4] += o * (kx * kz); a[5] += o * (ky * kz);
  }
  __shared__ double part[256 / MI_WAVE][DE_ROW_WORDS];
  mi_block_fold<DE_ROW_WORDS>(a, part, virial + DE_ROW_WORDS * (size_t)b, DE_ROW_WORDS);
}

size_t de_count(int n) { return (size_t)(n > 0 ? n : 0); }
size_t de_rec_bytes(int n_atoms, int dtype) { return mi_align((dtype == MI_F32 ? sizeof(DeRec<float>) : sizeof(DeRec<double>)) * de_count(n_atoms)); }
int de_tiles(int n_atoms) { return mi_blocks(n_atoms > 0 ? n_atoms : 0, DE_ATOM_TILE); }

}  // namespace

extern "C" int mi_ewald_dispersion_blocks(void) { return MI_FOLD_BLOCKS; }
extern "C" int mi_ewald_dispersion_row_words(void) { return DE_ROW_WORDS; }
extern "C" int mi_ewald_dispersion_atom_tile(void) { return DE_ATOM_TILE; }
extern "C" int mi_ewald_dispersion_k_tile(void) { return DE_K_TILE; }
extern "C" int mi_ewald_dispersion_record_words(void) { return DE_REC_WORDS; }
extern "C" size_t mi_ewald_dispersion_real_scratch_bytes(int n_atoms, int dtype) {
  return de_rec_bytes(n_atoms, dtype) + mi_align(sizeof(double) * DE_ROW_WORDS * de_count(n_atoms));
}
extern "C" size_t mi_ewald_dispersion_sf_scratch_bytes(int n_atoms, int n_systems, int n_k) {
  return mi_align(sizeof(double) * 2 * (de_count(n_k) + 1) * ((size_t)de_tiles(n_atoms) + de_count(n_systems)));
}

extern "C" int mi_ewald_dispersion_real(const void* positions, const void* coefficients, const void* cell, const void* alpha,
                                        const int32_t* batch_idx, const double* weights, int n_atoms, int n_systems, int dtype,
                                        double counted_cutoff, double counted_taper, const int32_t* idx_j, const int32_t* unit_shifts,
                                        const int32_t* neighbor_ptr, int max_neighbors, int mask_value, int flags, double* energies, void* forces,
                                        double* coefficient_grads, double* virial_partial, void* scratch, size_t scratch_bytes, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1 && n_systems <= 65535, "n_systems must be in [1, 65535]");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(!(flags & ~(MI_DE_FORCES | MI_DE_COEFFICIENT_GRAD | MI_DE_VIRIAL)), "unknown flag");
  const bool counted = counted_cutoff > 0.0;
  MI_REQUIRE(counted || !(counted_taper > 0.0), "counted_taper without counted_cutoff");
  MI_REQUIRE(!counted || !(counted_taper > 0.0) || counted_taper < counted_cutoff, "counted_taper must lie inside (0, counted_cutoff), or be negative for none");
  const bool virial = (flags & MI_DE_VIRIAL) != 0;
  MI_REQUIRE(!virial || (unit_shifts && virial_partial), "the virial needs unit_shifts and virial_partial");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && coefficients && cell && alpha && idx_j, "null pointer");
  MI_REQUIRE(energies || flags, "nothing to compute");
  MI_REQUIRE(!(flags & MI_DE_FORCES) || forces, "forces output");
  MI_REQUIRE(!(flags & MI_DE_COEFFICIENT_GRAD) || coefficient_grads, "coefficient gradient output");
  MI_REQUIRE(scratch && scratch_bytes >= mi_ewald_dispersion_real_scratch_bytes(n_atoms, dtype),
             "scratch smaller than mi_ewald_dispersion_real_scratch_bytes()");
  hipStream_t st = (hipStream_t)stream;
  double* trow = reinterpret_cast<double*>((char*)scratch + de_rec_bytes(n_atoms, dtype));
  DeCounted P = {0.0, 0.0, 0.0, 0.0};
  if (counted) {
    const bool taper = counted_taper > 0.0;
    P.rc2 = counted_cutoff * counted_cutoff;
    P.ron = taper ? counted_taper : counted_cutoff;
    P.ron2 = P.ron * P.ron;
    P.tinv = taper ? 1.0 / (counted_cutoff - counted_taper) : 0.0;
  }
  const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;  // one system: every atom belongs to system 0 and the batch index is not read
#define MI_DE_RUN(T_, COUNTED_, CSR_)                                                                                                          \
  do {                                                                                                                                         \
    pair_pack_kernel<<<mi_blocks(n_atoms, 256), 256, 0, st>>>((const T_*)positions, (const T_*)coefficients, (const T_*)nullptr, n_atoms,      \
                                                              (DeRec<T_>*)scratch);                                                            \
    de_pair_kernel<T_, COUNTED_, CSR_><<<blocks, 256, 0, st>>>((const DeRec<T_>*)scratch, (const T_*)cell, (const T_*)alpha, bi, weights,      \
                                                               n_atoms, idx_j, unit_shifts, neighbor_ptr, max_neighbors, mask_value, flags, P, \
                                                               energies, (T_*)forces, coefficient_grads, trow);                                \
  } while (0)
#define MI_DE_KIND(T_, CSR_)                                                           \
  do {                                                                                 \
    if (counted) MI_DE_RUN(T_, true, CSR_); else MI_DE_RUN(T_, false, CSR_);           \
  } while (0)
  mi_timing_begin(counted ? "ewald_dispersion_real_counted" : "ewald_dispersion_real", stream);
  if (dtype == MI_F32) { if (neighbor_ptr) MI_DE_KIND(float, true); else MI_DE_KIND(float, false); }
  else { if (neighbor_ptr) MI_DE_KIND(double, true); else MI_DE_KIND(double, false); }
  mi_timing_end(stream);
#undef MI_DE_KIND
#undef MI_DE_RUN
  MI_LAUNCH_CHECK();
  if (virial) {
    de_fold_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>(trow, bi, n_atoms, virial_partial);
    MI_LAUNCH_CHECK();
  }
  return MI_OK;
}

extern "C" int mi_ewald_dispersion_structure_factors(const void* positions, const void* coefficients, const double* weights, const void* k_vectors,
                                                     const void* cell, const void* alpha, const int32_t* system_ptr, int n_atoms, int n_systems,
                                                     int n_k, int dtype, double* table, double* records, void* scratch, size_t scratch_bytes,
                                                     void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0 && n_k >= 0, "n_atoms and n_k must not be negative");
  MI_REQUIRE(n_systems >= 1 && n_systems <= 65535, "n_systems must be in [1, 65535]");
  MI_REQUIRE(n_systems == 1 || system_ptr, "system_ptr is required for batches");
  MI_REQUIRE(table && (n_k == 0 || k_vectors) && (n_atoms == 0 || (positions && coefficients)), "null pointer");
  MI_REQUIRE(!records || (cell && alpha), "the records need cell and alpha");
  MI_REQUIRE(n_atoms == 0 || (scratch && scratch_bytes >= mi_ewald_dispersion_sf_scratch_bytes(n_atoms, n_systems, n_k)),
             "scratch smaller than mi_ewald_dispersion_sf_scratch_bytes()");
  const int tiles = de_tiles(n_atoms);
  MI_REQUIRE(tiles <= 65535, "too many atoms for the explicit-k sum (more than 65535 atom tiles)");
  hipStream_t st = (hipStream_t)stream;
  const int32_t* sp = n_systems > 1 ? system_ptr : nullptr;
  const int kblocks = mi_blocks((long long)n_k + 1, DE_K_TILE);
  double* partial = (double*)scratch;
#define MI_DE_SF(T_)                                                                                                                             \
  do {                                                                                                                                           \
    if (tiles > 0)                                                                                                                               \
      de_sf_kernel<T_><<<dim3(kblocks, tiles, n_systems), DE_K_TILE, 0, st>>>((const T_*)positions, (const T_*)coefficients, weights,           \
                                                                              (const T_*)k_vectors, sp, n_atoms, n_k, partial);                  \
    de_sf_fold_kernel<T_><<<dim3(mi_blocks((long long)n_k + 1, 256), n_systems), 256, 0, st>>>(partial, (const T_*)k_vectors, (const T_*)cell,   \
                                                                                               (const T_*)alpha, sp, n_atoms, n_k, table, records); \
  } while (0)
  mi_timing_begin("ewald_dispersion_structure_factors", stream);
  if (dtype == MI_F32) MI_DE_SF(float); else MI_DE_SF(double);
  mi_timing_end(stream);
#undef MI_DE_SF
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_ewald_dispersion_recip_gather(const void* positions, const void* coefficients, const void* alpha, const int32_t* batch_idx,
                                                const double* records, const double* records_g, const double* weights, int n_atoms,
                                                int n_systems, int n_k, int dtype, double* energies, void* forces, double* coefficient_grads,
                                                void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0 && n_k >= 0, "n_atoms and n_k must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE((records_g != nullptr) == (weights != nullptr), "records_g and weights come together");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && coefficients && alpha && records, "null pointer");
  MI_REQUIRE(energies || forces || coefficient_grads, "nothing to compute");
  hipStream_t st = (hipStream_t)stream;
  const int blocks = mi_blocks(n_atoms, 256);
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;
#define MI_DE_GATHER(T_)                                                                                                                       \
  do {                                                                                                                                         \
    if (weights)                                                                                                                               \
      de_gather_kernel<T_, true><<<blocks, 256, 0, st>>>((const T_*)positions, (const T_*)coefficients, (const T_*)alpha, bi, records,         \
                                                         records_g, weights, n_atoms, n_systems, n_k, energies, (T_*)forces,                   \
                                                         coefficient_grads);                                                                   \
    else                                                                                                                                       \
      de_gather_kernel<T_, false><<<blocks, 256, 0, st>>>((const T_*)positions, (const T_*)coefficients, (const T_*)alpha, bi, records,        \
                                                          nullptr, nullptr, n_atoms, n_systems, n_k, energies, (T_*)forces,                    \
                                                          coefficient_grads);                                                                  \
  } while (0)
  mi_timing_begin("ewald_dispersion_recip_gather", stream);
  if (dtype == MI_F32) MI_DE_GATHER(float); else MI_DE_GATHER(double);
  mi_timing_end(stream);
#undef MI_DE_GATHER
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_ewald_dispersion_recip_virial(const double* table, const void* k_vectors, const void* cell, const void* alpha, int n_systems,
                                                int n_k, int dtype, double* virial, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_systems >= 1 && n_k >= 0, "n_systems must be at least 1, n_k not negative");
  MI_REQUIRE(virial && cell && alpha && table && (n_k == 0 || k_vectors), "null pointer");
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("ewald_dispersion_recip_virial", stream);
  if (dtype == MI_F32)
    de_recip_virial_kernel<float><<<n_systems, 256, 0, st>>>(table, (const float*)k_vectors, (const float*)cell, (const float*)alpha, n_k, virial);
  else
    de_recip_virial_kernel<double><<<n_systems, 256, 0, st>>>(table, (const double*)k_vectors, (const double*)cell, (const double*)alpha, n_k, virial);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}
