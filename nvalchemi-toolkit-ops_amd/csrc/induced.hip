// induced.hip -- induced point dipoles: the real-space dipole-dipole operator of the point-dipole Ewald sum as a stored sparse operator of
// 3 x 3 blocks, its product, and the vector kernels of a batched Jacobi-preconditioned conjugate-gradient solve on it.  gfx950, wave64.
//
// The induced dipoles minimise, per system, U(mu) = sum_i |mu_i|^2 / (2 a_i) + E_dip(q, mu) - sum_i mu_i . F_i with E_dip the energy of
// dipole.hip / pme.hip: H mu = b, H = diag(1 / a) + T, b = -dE_dip/dmu at mu = 0 plus F.  The geometry does not change during a solve, so the
// real-space part of T is a constant operator over the caller's FULL neighbour list.  On a stored entry (i, j, S), R = r_j - r_i + S . cell:
//     T_e = B1 I - B2 R R^T,   B0 = erfc(a r) / r,  B1 = (B0 + 2 a^2 pre) / r^2,  B2 = (3 B1 + 4 a^4 pre) / r^2,  pre = exp(-a^2 r^2) / (a sqrt(pi))
// formed exactly as dp_pair_kernel forms them: libm erfc and exp, pair vector and distance in the positions dtype, everything after that fp64,
// entries with r <= 1e-8 skipped, self-image entries (i, i, S != 0) kept.  So sum_row T_e x_j is what mi_ewald_dipole_real returns as dE/dmu
// for zero charges.  An atom with a_i <= 0 (or NaN) is not polarisable: its row of H is the identity row, and every entry that has it at
// either end is stored as zero, so H stays symmetric.
//
// Layout of the stored operator: 44 bytes per slot of the caller's list layout ([N, M] or CSR with n_slots entries) in six streams, each
// read with one coalesced load per trip: tensors[0..5)[n_slots] = {B1, B2, R_x, R_y, R_z} (fp64) and neighbors[n_slots] (int32).  Padding and
// skipped entries hold zero coefficients and the row's own index, so the product gathers without a padding branch and never leaves [0, N).
// (One 48-byte record per slot read with three 16-byte loads was measured 31 % slower than the six streams: DESIGN 3.22.)
// The solver's vectors are dense [N, 3] doubles: padding them to [N, 4] for one aligned 32-byte gather per slot was measured and bought nothing
// (DESIGN 3.22), so it is not built.
//
// Kernels: ind_tensor_kernel (once per geometry: the only transcendentals of a solve), ind_apply_kernel (y = y_in + x / a + T x: one wave64
// per row, four trips in flight, nothing but stream loads, one gather and nine FMAs per slot), ind_dot_kernel (per-system block partials of
// x . y: mi_system_fold of pair_row.h) and the two vector kernels of a CG iteration.  Every reduction runs in a fixed order, every store is a
// plain vector store, there are no atomics: these kernels are bit-reproducible.
//
// mi_cluster_induced_pair_tensors stores the operator of a cluster without a cell in the same layout: B1 = 1 / r^3, B2 = 3 / r^5 (the alpha -> 0
// limit), optionally Thole-damped; product and CG kernels do not know the difference.
//
// The fold and CG kernels run on a grid (MI_FOLD_BLOCKS, n_systems), so n_systems <= 65535 (checked), and every block scans batch_idx once:
// O(N n_systems) index reads per launch, as every mi_system_fold.
#include "common.h"

namespace {

#include "pair_row.h"  // the row walk of ind_tensor_kernel and the fixed-order fold

#define IND_STATE_WORDS 8  // doubles of solver state per system: {r.z, b.b, done, iterations, alpha, beta, breakdown, r.r}
#define IND_TENSOR_WORDS 5 // streams of the stored operator: {B1, B2, R_x, R_y, R_z}
#define IND_DEPTH 4        // trips of a row in flight in ind_apply_kernel

// THOLE: the stored coefficients are B1 + D1 and B2 + D2 with the D_n of dp_pair_kernel's Thole kind (dipole.hip), E = thole_a r^3 / sqrt(a_i a_j)
// and the same early exit at E >= 50, so sum_row T_e x_j is dE/dmu of mi_ewald_dipole_real + mi_thole_dipole for zero charges.
// BARE: the undamped 1/r operator of a cluster, B1 = 1 / r^3 and B2 = 3 / r^5 (the alpha -> 0 limit; no erfc, no exp): cell, alpha, batch_idx and
// ush are not read (NULL).  With THOLE the D_n are added as above, so sum_row T_e x_j is dE/dmu of mi_coulomb_dipole (+ mi_thole_dipole).
template <class T, bool CSR, bool THOLE, bool BARE = false>
__global__ __launch_bounds__(256) void ind_tensor_kernel(const T* __restrict__ pos, const T* __restrict__ polar, const T* __restrict__ cell,
                                                         const T* __restrict__ alpha, const int* __restrict__ batch_idx, int N,
                                                         const int* __restrict__ idx, const int* __restrict__ ush, const int* __restrict__ nptr,
                                                         int M, int mask_value, long long slots, double* __restrict__ ten, int* __restrict__ nbr,
                                                         double* __restrict__ diag, double* __restrict__ precond, double thole_a) {
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const int i = pair_row_index();
  if (i >= N) return;
  const int s = batch_idx ? batch_idx[i] : 0;
  const bool shifted = ush != nullptr;
  T cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (shifted) pair_row_cell(cell, s, cm);
  const double al = BARE ? 0.0 : (double)alpha[s];
  const double ta = 2.0 * al * al, inv_a_sqrt_pi = 1.0 / (al * 1.7724538509055159);  // (BARE: not used)
  const T pix = pos[3 * (size_t)i], piy = pos[3 * (size_t)i + 1], piz = pos[3 * (size_t)i + 2];
  const T ai = polar[i];
  const bool pol_i = ai > T(0);  // (NaN: not polarisable)
  if (lane == 0) {
    diag[i] = pol_i ? 1.0 / (double)ai : 1.0;
    precond[i] = pol_i ? (double)ai : 1.0;
  }
  long long beg, end;
  pair_row_range<CSR>(nptr, i, M, beg, end);
  for (long long e = beg + lane; e < end; e += MI_WAVE) {
    const int j = idx[e];
    double b1 = 0.0, b2 = 0.0, rx = 0.0, ry = 0.0, rz = 0.0;
    int jj = i;  // padding and skipped entries: zero coefficients on the row's own index
    T aj = T(0);
    if (pol_i && !pair_is_padding<CSR>(j, mask_value, N) && (aj = polar[j]) > T(0)) {
      T sx = pos[3 * (size_t)j] - pix, sy = pos[3 * (size_t)j + 1] - piy, sz = pos[3 * (size_t)j + 2] - piz;
      if (shifted) {
        T sh[3];
        pair_separation(ush, e, cm, sh);
        sx += sh[0]; sy += sh[1]; sz += sh[2];
      }
      const T r2t = sx * sx + sy * sy + sz * sz;
      const double dist = (double)sqrt(r2t);  // the distance is a quantity of the positions dtype
      if (dist > 1e-8) {                      // (NaN fails)
        const double rinv = 1.0 / dist, rinv2 = rinv * rinv, ar = al * dist;
        if constexpr (BARE) {
          b1 = rinv * rinv2;
          b2 = 3.0 * b1 * rinv2;
        } else {
          const double pre = exp(-(ar * ar)) * inv_a_sqrt_pi;
          const double b0 = erfc(ar) * rinv;
          b1 = (b0 + ta * pre) * rinv2;
          b2 = (3.0 * b1 + ta * ta * pre) * rinv2;
        }
        if constexpr (THOLE) {
          const double big = thole_a * (dist * dist * dist) / sqrt((double)ai * (double)aj);
          if (big < 50.0) {
            const double d3 = exp(-big) * rinv * rinv2;
            b1 -= d3;
            b2 -= 3.0 * (1.0 + big) * d3 * rinv2;
          }
        }
        rx = (double)sx; ry = (double)sy; rz = (double)sz;
        jj = j;
      }
    }
    ten[e] = b1; ten[slots + e] = b2; ten[2 * slots + e] = rx; ten[3 * slots + e] = ry; ten[4 * slots + e] = rz;
    nbr[e] = jj;
  }
}

__device__ __forceinline__ void ind_load(const double* __restrict__ x, int j, double& vx, double& vy, double& vz) {
  vx = x[3 * (size_t)j]; vy = x[3 * (size_t)j + 1]; vz = x[3 * (size_t)j + 2];
}

// one slot of the product: acc += B1 x_j - B2 (R . x_j) R
__device__ __forceinline__ void ind_term(double b1, double b2, double rx, double ry, double rz, double vx, double vy, double vz, double& ax,
                                         double& ay, double& az) {
  const double w = -b2 * fma(rz, vz, fma(ry, vy, rx * vx));
  ax = fma(w, rx, fma(b1, vx, ax));
  ay = fma(w, ry, fma(b1, vy, ay));
  az = fma(w, rz, fma(b1, vz, az));
}

// y_i = y_in,i + x_i / a_i + sum_{row i} T_e x[nbr_e]: one wave per row, rows longer than 64 take several trips (IND_DEPTH in flight).  The
// lane sums and the wave reduction run in a fixed order.
template <bool CSR>
__global__ __launch_bounds__(256) void ind_apply_kernel(const double* __restrict__ ten, const int* __restrict__ nbr, const double* __restrict__ diag,
                                                        const double* __restrict__ x, const double* __restrict__ y_in, int N,
                                                        const int* __restrict__ nptr, int M, long long slots, double* __restrict__ y) {
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const int i = pair_row_index();
  if (i >= N) return;
  long long beg, end;
  pair_row_range<CSR>(nptr, i, M, beg, end);
  const double *s1 = ten, *s2 = ten + slots, *sx = ten + 2 * slots, *sy = ten + 3 * slots, *sz = ten + 4 * slots;
  double ax = 0.0, ay = 0.0, az = 0.0;
  long long e = beg + lane;
  for (; e + (IND_DEPTH - 1) * MI_WAVE < end; e += IND_DEPTH * MI_WAVE) {
    int j[IND_DEPTH];
    double b1[IND_DEPTH], b2[IND_DEPTH], rx[IND_DEPTH], ry[IND_DEPTH], rz[IND_DEPTH], vx[IND_DEPTH], vy[IND_DEPTH], vz[IND_DEPTH];
#pragma unroll
    for (int k = 0; k < IND_DEPTH; ++k) j[k] = nbr[e + k * MI_WAVE];
#pragma unroll
    for (int k = 0; k < IND_DEPTH; ++k) {
      const long long ek = e + k * MI_WAVE;
      b1[k] = s1[ek]; b2[k] = s2[ek]; rx[k] = sx[ek]; ry[k] = sy[ek]; rz[k] = sz[ek];
    }
#pragma unroll
    for (int k = 0; k < IND_DEPTH; ++k) ind_load(x, j[k], vx[k], vy[k], vz[k]);
#pragma unroll
    for (int k = 0; k < IND_DEPTH; ++k) ind_term(b1[k], b2[k], rx[k], ry[k], rz[k], vx[k], vy[k], vz[k], ax, ay, az);
  }
  for (; e < end; e += MI_WAVE) {
    double vx, vy, vz;
    ind_load(x, nbr[e], vx, vy, vz);
    ind_term(s1[e], s2[e], sx[e], sy[e], sz[e], vx, vy, vz, ax, ay, az);
  }
  ax = wave_sum(ax); ay = wave_sum(ay); az = wave_sum(az);
  if (lane == 0) {
    const double d = diag[i];
    double xi, yi, zi;
    ind_load(x, i, xi, yi, zi);
    double* o = y + 3 * (size_t)i;
    o[0] = (y_in ? y_in[3 * (size_t)i] : 0.0) + fma(d, xi, ax);
    o[1] = (y_in ? y_in[3 * (size_t)i + 1] : 0.0) + fma(d, yi, ay);
    o[2] = (y_in ? y_in[3 * (size_t)i + 2] : 0.0) + fma(d, zi, az);
  }
}

// block (b, s) sums x . y over the atoms of system s in the fixed order of mi_system_fold: partial[s][b], plain stores
__global__ __launch_bounds__(256) void ind_dot_kernel(const double* __restrict__ x, const double* __restrict__ y, const int* __restrict__ batch_idx,
                                                      int N, double* __restrict__ partial) {
  mi_system_fold<1, MI_FOLD_BLOCKS>(batch_idx, N, 1, partial, [&](long long r, double* a) {
    const double *xr = x + 3 * r, *yr = y + 3 * r;
    a[0] = fma(xr[2], yr[2], fma(xr[1], yr[1], fma(xr[0], yr[0], a[0])));
  });
}

// the MI_FOLD_BLOCKS block partials of word k of system s, summed by the calling wave: every lane of every wave of every block gets the
// same bits (a butterfly of commutative additions), so all blocks of a system derive identical scalars without talking to each other
__device__ __forceinline__ double ind_total(const double* __restrict__ partial, int s, int words, int k) {
  static_assert(MI_FOLD_BLOCKS == MI_WAVE, "one wave folds the block partials of a system with one wave_sum");
  return wave_sum(partial[((size_t)s * MI_FOLD_BLOCKS + (threadIdx.x & (MI_WAVE - 1))) * words + k]);
}

// First half of a CG iteration.  From the partials {p.y} of y = H p:  alpha_s = r.z / p.y,  x += alpha p,  r -= alpha y, and the block
// partials {r.r, r.z} of the new r with z = d r (the Jacobi preconditioner, never stored).  A done system is left untouched.  A system that
// is not done and whose p.y is not positive and finite has met a direction of non-positive curvature -- the operator is not positive
// definite -- and is frozen WITH the breakdown word of its state raised.  mode 1 is the set-up of a solve: r = -y for y = H x0 - b, x and p
// not used, partial_y not read.  State is read from state_in and written to state_out by block 0 of each system (ping-pong).
__global__ __launch_bounds__(256) void ind_cg_update_kernel(const double* __restrict__ y, const double* __restrict__ partial_y,
                                                            const double* __restrict__ precond, const int* __restrict__ batch_idx, int N,
                                                            int mode, double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
                                                            const double* __restrict__ state_in, double* __restrict__ state_out,
                                                            double* __restrict__ partial_rr) {
  const int s = blockIdx.y;
  const bool init = mode == 1;
  const double py = init ? 0.0 : ind_total(partial_y, s, 1, 0);
  const double* st = state_in + IND_STATE_WORDS * (size_t)s;
  bool done = !init && st[2] != 0.0;
  double broke = init ? 0.0 : st[6];
  double alpha = 0.0;
  if (init) alpha = 1.0;
  else if (!done) {
    if (py > 0.0 && py < INFINITY) alpha = st[0] / py;
    else { done = true; broke = 1.0; }
  }
  double acc_rr = 0.0, acc_rz = 0.0;
  for (long long a = (long long)blockIdx.x * 256 + threadIdx.x; a < N; a += (long long)MI_FOLD_BLOCKS * 256) {
    if (batch_idx && batch_idx[a] != s) continue;
    double sq = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t w = 3 * (size_t)a + c;
      double ra = init ? 0.0 : r[w];
      if (alpha != 0.0) {
        ra = fma(-alpha, y[w], ra);
        r[w] = ra;
        if (!init) x[w] = fma(alpha, p[w], x[w]);
      }
      sq = fma(ra, ra, sq);
    }
    acc_rr += sq;
    acc_rz = fma(precond[a], sq, acc_rz);
  }
  __shared__ double part[256 / MI_WAVE][2];
  const int lane = threadIdx.x & (MI_WAVE - 1), wave = threadIdx.x / MI_WAVE;
  acc_rr = wave_sum(acc_rr); acc_rz = wave_sum(acc_rz);
  if (lane == 0) { part[wave][0] = acc_rr; part[wave][1] = acc_rz; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = partial_rr + 2 * ((size_t)s * MI_FOLD_BLOCKS + blockIdx.x);
    o[0] = part[0][0] + part[1][0] + part[2][0] + part[3][0];
    o[1] = part[0][1] + part[1][1] + part[2][1] + part[3][1];
    if (blockIdx.x == 0) {
      double* so = state_out + IND_STATE_WORDS * (size_t)s;
      so[0] = st[0]; so[1] = st[1]; so[2] = done ? 1.0 : 0.0; so[3] = st[3]; so[4] = alpha; so[5] = st[5]; so[6] = broke; so[7] = st[7];
    }
  }
}

// Second half: from the partials {r.r, r.z} of the new r,  beta_s = r.z_new / r.z_old,  p = d r + beta p,  iterations += 1,
// done = r.r_new <= tolerance^2 b.b.  A done system is frozen.  mode 1 starts a solve (b = r: b.b = r.r, p = d r, iterations = 0; b = 0 is
// done at once); mode 2 restarts from a new r and keeps b.b (the start of the iteration proper, cold or warm).
__global__ __launch_bounds__(256) void ind_cg_direction_kernel(const double* __restrict__ partial_rr, const double* __restrict__ precond,
                                                               const int* __restrict__ batch_idx, int N, int mode, double tol2,
                                                               const double* __restrict__ r, double* __restrict__ p,
                                                               const double* __restrict__ state_in, double* __restrict__ state_out) {
  const int s = blockIdx.y;
  const double rr_new = ind_total(partial_rr, s, 2, 0), rz_new = ind_total(partial_rr, s, 2, 1);
  const double* st = state_in + IND_STATE_WORDS * (size_t)s;
  const bool was_done = mode == 0 && st[2] != 0.0;
  const double bb = mode == 1 ? rr_new : st[1];
  double beta = 0.0, iters = mode == 0 ? st[3] : 0.0;
  if (mode == 0 && !was_done) { beta = rz_new / st[0]; iters += 1.0; }
  const bool done = was_done || !(bb > 0.0) || rr_new <= tol2 * bb;
  if (!was_done) {
    for (long long a = (long long)blockIdx.x * 256 + threadIdx.x; a < N; a += (long long)MI_FOLD_BLOCKS * 256) {
      if (batch_idx && batch_idx[a] != s) continue;
      const double d = precond[a];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const size_t w = 3 * (size_t)a + c;
        p[w] = mode == 0 ? fma(beta, p[w], d * r[w]) : d * r[w];
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double* so = state_out + IND_STATE_WORDS * (size_t)s;
    so[0] = rz_new; so[1] = bb; so[2] = done ? 1.0 : 0.0; so[3] = iters; so[4] = st[4]; so[5] = beta; so[6] = mode == 0 ? st[6] : 0.0;
    so[7] = rr_new;
  }
}

}  // namespace

extern "C" int mi_induced_blocks(void) { return MI_FOLD_BLOCKS; }
extern "C" int mi_induced_state_words(void) { return IND_STATE_WORDS; }
extern "C" int mi_induced_tensor_words(void) { return IND_TENSOR_WORDS; }
extern "C" int mi_induced_unroll_depth(void) { return IND_DEPTH; }

namespace {

int ind_pair_tensors(const void* positions, const void* polarizability, const void* cell, const void* alpha, const int32_t* batch_idx, int n_atoms,
                     int n_systems, int dtype, const int32_t* idx_j, const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors,
                     int mask_value, long long n_slots, double* tensors, int32_t* neighbors, double* diagonal, double* preconditioner,
                     bool thole, double thole_a, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_slots >= 0, "n_slots must not be negative");
  MI_REQUIRE(neighbor_ptr || n_slots == (long long)n_atoms * max_neighbors, "n_slots must be n_atoms * max_neighbors for a matrix");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(!thole || (thole_a > 0.0 && thole_a < INFINITY), "thole_a must be positive and finite");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && polarizability && cell && alpha && diagonal && preconditioner, "null pointer");
  MI_REQUIRE(n_slots == 0 || (idx_j && tensors && neighbors), "null pointer");  // (a list may be empty)
  hipStream_t st = (hipStream_t)stream;
  const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;
#define MI_IT(T_, CSR_, THOLE_)                                                                                                                  \
  ind_tensor_kernel<T_, CSR_, THOLE_><<<blocks, 256, 0, st>>>((const T_*)positions, (const T_*)polarizability, (const T_*)cell,                  \
                                                              (const T_*)alpha, bi, n_atoms, idx_j, unit_shifts, neighbor_ptr, max_neighbors,    \
                                                              mask_value, n_slots, tensors, neighbors, diagonal, preconditioner, thole_a)
#define MI_IT_LAYOUT(T_)                                                                                                                         \
  do {                                                                                                                                           \
    if (thole) { if (neighbor_ptr) MI_IT(T_, true, true); else MI_IT(T_, false, true); }                                                         \
    else { if (neighbor_ptr) MI_IT(T_, true, false); else MI_IT(T_, false, false); }                                                             \
  } while (0)
  mi_timing_begin(thole ? "thole_induced_pair_tensors" : "induced_pair_tensors", stream);
  if (dtype == MI_F32) MI_IT_LAYOUT(float); else MI_IT_LAYOUT(double);
  mi_timing_end(stream);
#undef MI_IT_LAYOUT
#undef MI_IT
  MI_LAUNCH_CHECK();
  return MI_OK;
}

}  // namespace

extern "C" int mi_induced_pair_tensors(const void* positions, const void* polarizability, const void* cell, const void* alpha,
                                       const int32_t* batch_idx, int n_atoms, int n_systems, int dtype, const int32_t* idx_j,
                                       const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors, int mask_value,
                                       long long n_slots, double* tensors, int32_t* neighbors, double* diagonal, double* preconditioner,
                                       void* stream) {
  return ind_pair_tensors(positions, polarizability, cell, alpha, batch_idx, n_atoms, n_systems, dtype, idx_j, unit_shifts, neighbor_ptr,
                          max_neighbors, mask_value, n_slots, tensors, neighbors, diagonal, preconditioner, false, 0.0, stream);
}

extern "C" int mi_thole_induced_pair_tensors(const void* positions, const void* polarizability, const void* cell, const void* alpha,
                                             const int32_t* batch_idx, int n_atoms, int n_systems, int dtype, const int32_t* idx_j,
                                             const int32_t* unit_shifts, const int32_t* neighbor_ptr, int max_neighbors, int mask_value,
                                             long long n_slots, double* tensors, int32_t* neighbors, double* diagonal, double* preconditioner,
                                             double thole_a, void* stream) {
  return ind_pair_tensors(positions, polarizability, cell, alpha, batch_idx, n_atoms, n_systems, dtype, idx_j, unit_shifts, neighbor_ptr,
                          max_neighbors, mask_value, n_slots, tensors, neighbors, diagonal, preconditioner, true, thole_a, stream);
}

extern "C" int mi_cluster_induced_pair_tensors(const void* positions, const void* polarizability, int n_atoms, int dtype, const int32_t* idx_j,
                                               const int32_t* neighbor_ptr, int max_neighbors, int mask_value, long long n_slots,
                                               double* tensors, int32_t* neighbors, double* diagonal, double* preconditioner, double thole_a,
                                               void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_slots >= 0, "n_slots must not be negative");
  MI_REQUIRE(neighbor_ptr || n_slots == (long long)n_atoms * max_neighbors, "n_slots must be n_atoms * max_neighbors for a matrix");
  MI_REQUIRE(thole_a >= 0.0 && thole_a < INFINITY, "thole_a must be 0 (undamped) or positive and finite");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && polarizability && diagonal && preconditioner, "null pointer");
  MI_REQUIRE(n_slots == 0 || (idx_j && tensors && neighbors), "null pointer");  // (a list may be empty)
  hipStream_t st = (hipStream_t)stream;
  const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
  const bool thole = thole_a > 0.0;
#define MI_CT(T_, CSR_, THOLE_)                                                                                                                  \
  ind_tensor_kernel<T_, CSR_, THOLE_, true><<<blocks, 256, 0, st>>>((const T_*)positions, (const T_*)polarizability, (const T_*)nullptr,         \
                                                                    (const T_*)nullptr, nullptr, n_atoms, idx_j, nullptr, neighbor_ptr,          \
                                                                    max_neighbors, mask_value, n_slots, tensors, neighbors, diagonal,            \
                                                                    preconditioner, thole_a)
#define MI_CT_LAYOUT(T_)                                                                                                                         \
  do {                                                                                                                                           \
    if (thole) { if (neighbor_ptr) MI_CT(T_, true, true); else MI_CT(T_, false, true); }                                                         \
    else { if (neighbor_ptr) MI_CT(T_, true, false); else MI_CT(T_, false, false); }                                                             \
  } while (0)
  mi_timing_begin("cluster_induced_pair_tensors", stream);
  if (dtype == MI_F32) MI_CT_LAYOUT(float); else MI_CT_LAYOUT(double);
  mi_timing_end(stream);
#undef MI_CT_LAYOUT
#undef MI_CT
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_induced_apply(const double* tensors, const int32_t* neighbors, const double* diagonal, const double* x, const double* y_in,
                                const int32_t* batch_idx, int n_atoms, int n_systems, const int32_t* neighbor_ptr, int max_neighbors,
                                long long n_slots, double* y, double* partial, void* stream) {
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(!partial || n_systems <= 65535, "n_systems must not exceed 65535 (one grid row per system)");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_slots >= 0, "n_slots must not be negative");
  MI_REQUIRE(neighbor_ptr || n_slots == (long long)n_atoms * max_neighbors, "n_slots must be n_atoms * max_neighbors for a matrix");
  MI_REQUIRE(!partial || n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(n_atoms == 0 || (diagonal && x && y), "null pointer");
  MI_REQUIRE(n_atoms == 0 || n_slots == 0 || (tensors && neighbors), "null pointer");  // (a list may be empty)
  MI_REQUIRE(n_atoms == 0 || (x != y && y_in != y), "x, y_in and y must not overlap");
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("induced_apply", stream);
  if (n_atoms > 0) {
    const int blocks = mi_blocks(n_atoms, 256 / MI_WAVE);
    if (neighbor_ptr) ind_apply_kernel<true><<<blocks, 256, 0, st>>>(tensors, neighbors, diagonal, x, y_in, n_atoms, neighbor_ptr, 0, n_slots, y);
    else ind_apply_kernel<false><<<blocks, 256, 0, st>>>(tensors, neighbors, diagonal, x, y_in, n_atoms, nullptr, max_neighbors, n_slots, y);
  }
  if (partial)
    ind_dot_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>(x, y, n_systems > 1 ? batch_idx : nullptr, n_atoms, partial);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_induced_dot(const double* x, const double* y, const int32_t* batch_idx, int n_atoms, int n_systems, double* partial,
                              void* stream) {
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(n_systems <= 65535, "n_systems must not exceed 65535 (one grid row per system)");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(partial && (n_atoms == 0 || (x && y)), "null pointer");
  mi_timing_begin("induced_dot", stream);
  ind_dot_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, (hipStream_t)stream>>>(x, y, n_systems > 1 ? batch_idx : nullptr, n_atoms,
                                                                                   partial);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_induced_cg_update(const double* y, const double* partial_y, const double* preconditioner, const int32_t* batch_idx, int n_atoms,
                                    int n_systems, int mode, double* x, double* r, const double* p, const double* state_in,
                                    double* state_out, double* partial_rr, void* stream) {
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(n_systems <= 65535, "n_systems must not exceed 65535 (one grid row per system)");
  MI_REQUIRE(mode == 0 || mode == 1, "mode");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE((mode == 1 || partial_y) && state_in && state_out && partial_rr, "null pointer");
  MI_REQUIRE(state_in != state_out, "state_in and state_out must differ");
  MI_REQUIRE(n_atoms == 0 || (y && r && preconditioner && (mode == 1 || (x && p))), "null pointer");
  MI_REQUIRE(n_atoms == 0 || (y != r && y != x), "y must not overlap x or r");
  mi_timing_begin("induced_cg_update", stream);
  ind_cg_update_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, (hipStream_t)stream>>>(y, partial_y, preconditioner,
                                                                                         n_systems > 1 ? batch_idx : nullptr, n_atoms,
                                                                                         mode, x, r, p, state_in, state_out, partial_rr);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

extern "C" int mi_induced_cg_direction(const double* partial_rr, const double* preconditioner, const int32_t* batch_idx, int n_atoms, int n_systems,
                                       int mode, double tolerance, const double* r, double* p, const double* state_in,
                                       double* state_out, void* stream) {
  MI_REQUIRE(n_atoms >= 0, "n_atoms must not be negative");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(n_systems <= 65535, "n_systems must not exceed 65535 (one grid row per system)");
  MI_REQUIRE(mode >= 0 && mode <= 2, "mode");
  MI_REQUIRE(tolerance >= 0.0, "tolerance must not be negative");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(partial_rr && state_in && state_out, "null pointer");
  MI_REQUIRE(state_in != state_out, "state_in and state_out must differ");
  MI_REQUIRE(n_atoms == 0 || (r && p && preconditioner), "null pointer");
  MI_REQUIRE(n_atoms == 0 || r != p, "r and p must not overlap");
  mi_timing_begin("induced_cg_direction", stream);
  ind_cg_direction_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, (hipStream_t)stream>>>(partial_rr, preconditioner,
                                                                                            n_systems > 1 ? batch_idx : nullptr, n_atoms,
                                                                                            mode, tolerance * tolerance, r, p,
                                                                                            state_in, state_out);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}
