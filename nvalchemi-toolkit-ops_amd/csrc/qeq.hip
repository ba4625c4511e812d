// qeq.hip -- charge equilibration: the pair operator of Gaussian-charge electrostatics as a stored sparse matrix, and the vector kernels of a
// batched projected conjugate-gradient solve on it.  gfx950, wave64.
//
// Charge equilibration minimises, per system s, E(q) = sum chi_i q_i + 1/2 sum J_i q_i^2 + E_el(q) subject to sum_{i in s} q_i = Q_s, with E_el
// the Gaussian-charge electrostatic energy of this package (point-charge Ewald / PME + gaussian_charge_correction, or erf(r/g)/r pairs without
// a cell).  E_el is a quadratic form, and the geometry does not change during a solve, so the real-space part of its Hessian is a constant
// sparse matrix over the caller's FULL neighbour list:
//     c_e = [erfc_AS(a_s r) - erfc(r / g_ij)] / r      with a cell  (erfc_AS: the Abramowitz-Stegun polynomial ewald.hip uses, pair_row.h;
//                                                                   erfc: the device library's, as in gaussian.hip)
//     c_e = [1 - erfc(r / g_ij)] / r                   without one
//     d_i = J_i + [sigma_i > 0] / (sqrt(pi) sigma_i)   hardness + Gaussian self term
// r = |r_j - r_i + S . cell| in the positions dtype (as gc_pair_kernel forms it), everything after that fp64.  The rules of the two public pair
// sums hold term by term: an entry with r <= 1e-8 contributes nothing; the erfc(r / g_ij) term is dropped for r / g_ij >= 6 (tested as
// r^2 >= 72 (s_i + s_j) before any transcendental) and for two point charges (g_ij = 0).  So (A x)_i = sum_row c_e x_j is exactly what
// ewald_real_space + gaussian_charge_correction return as dE/dq (pair terms), self-image entries (i, i, S != 0) included.
//
// Layout of the stored operator: two streams in the caller's list layout ([N, M] or CSR), coefficients[e] (fp64, 8 bytes) and neighbors[e]
// (int32, 4 bytes): 12 bytes per slot, read with two coalesced loads per trip.  Padding and skipped entries hold c_e = 0 and the row's own
// index, so the product kernel gathers x[neighbors[e]] without a padding branch and without leaving [0, N).
//
// Kernels: qeq_coef_kernel (once per geometry), qeq_apply_kernel (y = y_in + d x + A x: one wave64 per row, nothing but two stream loads, one
// 8-byte gather and one FMA per slot), qeq_fold_kernel (per-system block partials of sum y and x.y in a fixed order: mi_system_fold of
// pair_row.h) and the two vector kernels of a CG iteration.  Every reduction is a wave reduction in a fixed order, every store a plain
// vector store, there are no atomics: these kernels are bit-reproducible (a periodic solve as a whole is not: the reciprocal-space calls the
// driver makes between them add with atomics in arrival order).
//
// The fold and CG kernels run on a grid (MI_FOLD_BLOCKS, n_systems), so n_systems <= 65535 (checked), and every block scans batch_idx once:
// O(N n_systems) index reads per launch, as every mi_system_fold.  Fine for a few large systems; thousands of small ones would want per-system
// atom ranges (batch_idx sorted), which are not built.
#include "common.h"

namespace {

#include "pair_row.h"  // the row walk of qeq_coef_kernel, the fixed-order fold, erfc_as_poly with the Newton reciprocal as ewald.hip runs it

#define QEQ_STATE_WORDS 8   // doubles of solver state per system: {r.r, b.b, done, iterations, alpha, beta, 0, 0}

template <class T, bool CSR>
__global__ __launch_bounds__(256) void qeq_coef_kernel(const T* __restrict__ pos, const T* __restrict__ sigma, const double* __restrict__ hardness,
                                                       const T* __restrict__ cell, const T* __restrict__ alpha, const int* __restrict__ batch_idx,
                                                       int N, const int* __restrict__ idx, const int* __restrict__ ush, const int* __restrict__ nptr,
                                                       int M, int mask_value, double* __restrict__ coef, int* __restrict__ nbr,
                                                       double* __restrict__ diag) {
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const int i = pair_row_index();
  if (i >= N) return;
  const bool periodic = cell != nullptr;
  const bool shifted = periodic && ush != nullptr;
  T cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  double al = 0.0;
  if (periodic) {
    const int s = batch_idx ? batch_idx[i] : 0;
    pair_row_cell(cell, s, cm);
    al = (double)alpha[s];
  }
  const T pix = pos[3 * (size_t)i], piy = pos[3 * (size_t)i + 1], piz = pos[3 * (size_t)i + 2];
  const T sgt = sigma[i];
  const double sgi = sgt > T(0) ? (double)sgt : 0.0, si = sgi * sgi;  // (NaN -> point charge, as GcRec::set_tail)
  if (lane == 0) diag[i] = hardness[i] + (sgi > 0.0 ? 1.0 / (1.7724538509055159 * sgi) : 0.0);
  long long beg, end;
  pair_row_range<CSR>(nptr, i, M, beg, end);
  for (long long e = beg + lane; e < end; e += MI_WAVE) {
    const int j = idx[e];
    double c = 0.0;
    int jj = i;  // padding and skipped entries: coefficient 0 on the row's own index
    if (!pair_is_padding<CSR>(j, mask_value, N)) {
      T sx = pos[3 * (size_t)j] - pix, sy = pos[3 * (size_t)j + 1] - piy, sz = pos[3 * (size_t)j + 2] - piz;
      if (shifted) {
        T sh[3];
        pair_separation(ush, e, cm, sh);
        sx += sh[0]; sy += sh[1]; sz += sh[2];
      }
      const T r2t = sx * sx + sy * sy + sz * sz;
      const double dist = (double)sqrt(r2t);  // the distance is a quantity of the positions dtype
      if (dist > 1e-8) {  // (NaN fails)
        const double rinv = 1.0 / dist;
        double lr = 1.0;  // long-ranged factor: erfc_AS(a r) with a cell, 1 without
        if (periodic) {
          const double ar = al * dist;
          lr = erfc_as_poly<MiNewton>(ar, exp(-(ar * ar)));
        }
        const T sgj = sigma[j];
        const double sj = sgj > T(0) ? (double)sgj : 0.0;
        const double ss = si + sj * sj;
        double ec = 0.0;
        if ((double)r2t < 72.0 * ss) ec = erfc(dist * (1.0 / sqrt(2.0 * ss)));  // x = r / g_ij < 6; two point charges (ss == 0) never enter
        c = (lr - ec) * rinv;
        jj = j;
      }
    }
    coef[e] = c;
    nbr[e] = jj;
  }
}

// y_i = y_in,i + d_i x_i + sum_{row i} c_e x[nbr_e]: one wave per row, rows longer than 64 take several trips (four in flight).  The lane sums
// and the wave reduction run in a fixed order.
template <bool CSR>
__global__ __launch_bounds__(256) void qeq_apply_kernel(const double* __restrict__ coef, const int* __restrict__ nbr, const double* __restrict__ diag,
                                                        const double* __restrict__ x, const double* y_in /* may be y */, int N,
                                                        const int* __restrict__ nptr, int M, double* y) {
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const int i = pair_row_index();
  if (i >= N) return;
  long long beg, end;
  pair_row_range<CSR>(nptr, i, M, beg, end);
  double acc = 0.0;
  long long e = beg + lane;
  for (; e + 3 * MI_WAVE < end; e += 4 * MI_WAVE) {
    const int j0 = nbr[e], j1 = nbr[e + MI_WAVE], j2 = nbr[e + 2 * MI_WAVE], j3 = nbr[e + 3 * MI_WAVE];
    const double c0 = coef[e], c1 = coef[e + MI_WAVE], c2 = coef[e + 2 * MI_WAVE], c3 = coef[e + 3 * MI_WAVE];
    const double x0 = x[j0], x1 = x[j1], x2 = x[j2], x3 = x[j3];
    acc = fma(c0, x0, acc); acc = fma(c1, x1, acc); acc = fma(c2, x2, acc); acc = fma(c3, x3, acc);
  }
  for (; e < end; e += MI_WAVE) acc = fma(coef[e], x[nbr[e]], acc);
  acc = wave_sum(acc);
  if (lane == 0) y[i] = (y_in ? y_in[i] : 0.0) + fma(diag[i], x[i], acc);
}

// block (b, s) sums {y, x y} over the atoms of system s in the fixed order of mi_system_fold: partial[s][b][0..1], plain stores
__global__ __launch_bounds__(256) void qeq_fold_kernel(const double* __restrict__ y, const double* __restrict__ x, const int* __restrict__ batch_idx,
                                                       int N, double* __restrict__ partial) {
  mi_system_fold<2, MI_FOLD_BLOCKS>(batch_idx, N, 2, partial, [&](long long r, double* a) {
    const double yr = y[r];
    a[0] += yr; a[1] = fma(x[r], yr, a[1]);
  });
}

// the MI_FOLD_BLOCKS block partials of word k of system s, summed by the calling wave: every lane of every wave of every block gets the
// same bits (a butterfly of commutative additions), so all blocks of a system derive identical scalars without talking to each other
__device__ __forceinline__ double qeq_total(const double* __restrict__ partial, int s, int words, int k) {
  static_assert(MI_FOLD_BLOCKS == MI_WAVE, "one wave folds the block partials of a system with one wave_sum");
  return wave_sum(partial[((size_t)s * MI_FOLD_BLOCKS + (threadIdx.x & (MI_WAVE - 1))) * words + k]);
}

// First half of a CG iteration.  From the partials {sum y, p.y} of y = H p:  w = y - mean_s(y) (the projection),  alpha_s = r.r / p.w
// (p sums to zero, so p.w = p.y), q += alpha p, r -= alpha w, and the block partials of the new r.r.  A system that is done, or whose p.w is
// not positive (p = 0: nothing left to do), takes alpha = 0 and is left untouched.  mode 1 is the set-up of a solve: r = -(y - mean_s(y))
// for y = chi + H q0, q untouched, the other state words carried over.  State is read from state_in and written to state_out by block 0 of
// each system (ping-pong: no block reads what another writes).
__global__ __launch_bounds__(256) void qeq_cg_update_kernel(const double* __restrict__ y, const double* __restrict__ partial_y,
                                                            const double* __restrict__ counts, const int* __restrict__ batch_idx, int N, int mode,
                                                            double* __restrict__ q, double* __restrict__ r, const double* __restrict__ p,
                                                            const double* __restrict__ state_in, double* __restrict__ state_out,
                                                            double* __restrict__ partial_rr) {
  const int s = blockIdx.y;
  const double sum_y = qeq_total(partial_y, s, 2, 0), py = qeq_total(partial_y, s, 2, 1);
  const double* st = state_in + QEQ_STATE_WORDS * (size_t)s;
  const double cnt = counts[s];
  const double mean = cnt > 0.0 ? sum_y / cnt : 0.0;
  const bool init = mode == 1;
  bool done = !init && st[2] != 0.0;
  double alpha = 0.0;
  if (init) alpha = 1.0;
  else if (!done) {
    if (py > 0.0 && py < INFINITY) alpha = st[0] / py;
    else done = true;
  }
  double acc = 0.0;
  for (long long a = (long long)blockIdx.x * 256 + threadIdx.x; a < N; a += (long long)MI_FOLD_BLOCKS * 256) {
    if (batch_idx && batch_idx[a] != s) continue;
    double ra = init ? 0.0 : r[a];
    if (alpha != 0.0) {
      ra = fma(-alpha, y[a] - mean, ra);
      r[a] = ra;
      if (!init) q[a] = fma(alpha, p[a], q[a]);
    }
    acc = fma(ra, ra, acc);
  }
  __shared__ double part[256 / MI_WAVE];
  const int lane = threadIdx.x & (MI_WAVE - 1), wave = threadIdx.x / MI_WAVE;
  acc = wave_sum(acc);
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    partial_rr[(size_t)s * MI_FOLD_BLOCKS + blockIdx.x] = part[0] + part[1] + part[2] + part[3];
    if (blockIdx.x == 0) {
      double* so = state_out + QEQ_STATE_WORDS * (size_t)s;
      so[0] = st[0]; so[1] = st[1]; so[2] = done ? 1.0 : 0.0; so[3] = st[3]; so[4] = alpha; so[5] = st[5]; so[6] = 0.0; so[7] = 0.0;
    }
  }
}

// Second half: from the partials of the new r.r,  beta_s = r.r_new / r.r_old,  p = r + beta p,  iterations += 1,
// done = r.r_new <= tolerance^2 b.b.  A done system is frozen.  mode 1 starts a solve (b = r: b.b = r.r, p = r, iterations = 0; b = 0 is
// done at once, which also covers one-atom and empty systems); mode 2 restarts from a new r and keeps b.b (warm start).
__global__ __launch_bounds__(256) void qeq_cg_direction_kernel(const double* __restrict__ partial_rr, const int* __restrict__ batch_idx, int N, int mode,
                                                               double tol2, const double* __restrict__ r, double* __restrict__ p,
                                                               const double* __restrict__ state_in, double* __restrict__ state_out) {
  const int s = blockIdx.y;
  const double rr_new = qeq_total(partial_rr, s, 1, 0);
  const double* st = state_in + QEQ_STATE_WORDS * (size_t)s;
  const bool was_done = mode == 0 && st[2] != 0.0;
  double bb = mode == 1 ? rr_new : st[1];
  double beta = 0.0, iters = mode == 0 ? st[3] : 0.0;
  if (mode == 0 && !was_done) { beta = rr_new / st[0]; iters += 1.0; }
  const bool done = was_done || !(bb > 0.0) || rr_new <= tol2 * bb;
  if (!was_done) {
    for (long long a = (long long)blockIdx.x * 256 + threadIdx.x; a < N; a += (long long)MI_FOLD_BLOCKS * 256) {
      if (batch_idx && batch_idx[a] != s) continue;
      p[a] = mode == 0 ? fma(beta, p[a], r[a]) : r[a];
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double* so = state_out + QEQ_STATE_WORDS * (size_t)s;
    so[0] = rr_new; so[1] = bb; so[2] = done ? 1.0 : 0.0; so[3] = iters; so[4] = st[4]; so[5] = beta; so[6] = 0.0; so[7] = 0.0;
  }
}

}  // namespace

extern "C" int mi_qeq_blocks(void) { return MI_FOLD_BLOCKS; }
extern "C" int mi_qeq_state_words(void) { return QEQ_STATE_WORDS; }

extern "C" int mi_qeq_pair_coefficients(const void* positions, const void* sigma, const double* hardness, const void* cell, const void* alpha,
                                        const int32_t* batch_idx, int n_atoms, int n_systems, int dtype, const int32_t* idx_j,
                                        const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors, int mask_value,
                                        double* coefficients, int32_t* neighbors, double* diagonal, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(!cell || n_systems == 1 || batch_idx, "batch_idx is required for more than one cell");
  MI_REQUIRE(!unit_shifts || cell, "unit_shifts without a cell");
  MI_REQUIRE(!cell || alpha, "a cell needs alpha");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && sigma && hardness && diagonal, "null pointer");
  MI_REQUIRE(neighbor_ptr || max_neighbors == 0 || (idx_j && coefficients && neighbors), "null pointer");  // (a CSR list may be empty)
  hipStream_t st = (hipStream_t)stream;
  const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;
#define MI_QC(T_, CSR_)                                                                                                                          \
  qeq_coef_kernel<T_, CSR_><<<blocks, 256, 0, st>>>((const T_*)positions, (const T_*)sigma, hardness, (const T_*)cell, (const T_*)alpha, bi, n_atoms, \
                                                    idx_j, unit_shifts, neighbor_ptr, max_neighbors, mask_value, coefficients, neighbors, diagonal)
  mi_timing_begin("qeq_pair_coefficients", stream);
  if (dtype == MI_F32) { if (neighbor_ptr) MI_QC(float, true); else MI_QC(float, false); }
  else { if (neighbor_ptr) MI_QC(double, true); else MI_QC(double, false); }
  mi_timing_end(stream);
#undef MI_QC
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_qeq_apply(const double* coefficients, const int32_t* neighbors, const double* diagonal, const double* x, const double* y_in,
                            const int32_t* batch_idx, int n_atoms, int n_systems, const int32_t* neighbor_ptr, int max_neighbors, double* y,
                            double* partial, void* stream) {
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(!partial || n_systems <= 65535, "n_systems must not exceed 65535 (one grid row per system)");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(!partial || n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(n_atoms == 0 || (diagonal && x && y), "null pointer");
  MI_REQUIRE(n_atoms == 0 || neighbor_ptr || max_neighbors == 0 || (coefficients && neighbors), "null pointer");  // (a CSR list may be empty)
  MI_REQUIRE(n_atoms == 0 || (x != y), "x and y must not overlap");
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("qeq_apply", stream);
  if (n_atoms > 0) {
    const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
    if (neighbor_ptr) qeq_apply_kernel<true><<<blocks, 256, 0, st>>>(coefficients, neighbors, diagonal, x, y_in, n_atoms, neighbor_ptr, 0, y);
    else qeq_apply_kernel<false><<<blocks, 256, 0, st>>>(coefficients, neighbors, diagonal, x, y_in, n_atoms, nullptr, max_neighbors, y);
  }
  if (partial) qeq_fold_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>(y, x, n_systems > 1 ? batch_idx : nullptr, n_atoms, partial);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_qeq_cg_update(const double* y, const double* partial_y, const double* counts, const int32_t* batch_idx, int n_atoms, int n_systems,
                                int mode, double* q, double* r, const double* p, const double* state_in, double* state_out, double* partial_rr,
                                void* stream) {
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(n_systems <= 65535, "n_systems must not exceed 65535 (one grid row per system)");
  MI_REQUIRE(mode == 0 || mode == 1, "mode");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(partial_y && counts && state_in && state_out && partial_rr, "null pointer");
  MI_REQUIRE(state_in != state_out, "state_in and state_out must differ");
  MI_REQUIRE(n_atoms == 0 || (y && r && (mode == 1 || (q && p))), "null pointer");
  mi_timing_begin("qeq_cg_update", stream);
  qeq_cg_update_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, (hipStream_t)stream>>>(y, partial_y, counts, n_systems > 1 ? batch_idx : nullptr,
                                                                                         n_atoms, mode, q, r, p, state_in, state_out, partial_rr);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_qeq_cg_direction(const double* partial_rr, const int32_t* batch_idx, int n_atoms, int n_systems, int mode, double tolerance,
                                   const double* r, double* p, const double* state_in, double* state_out, void* stream) {
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(n_systems <= 65535, "n_systems must not exceed 65535 (one grid row per system)");
  MI_REQUIRE(mode >= 0 && mode <= 2, "mode");
  MI_REQUIRE(tolerance >= 0.0, "tolerance must not be negative");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(partial_rr && state_in && state_out, "null pointer");
  MI_REQUIRE(state_in != state_out, "state_in and state_out must differ");
  MI_REQUIRE(n_atoms == 0 || (r && p), "null pointer");
  mi_timing_begin("qeq_cg_direction", stream);
  qeq_cg_direction_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, (hipStream_t)stream>>>(partial_rr, n_systems > 1 ? batch_idx : nullptr, n_atoms,
                                                                                            mode, tolerance * tolerance, r, p, state_in, state_out);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}
