// pair_row.h -- the two pieces of device scaffolding that the pair-sum kernels share: the wave-per-row walk over a full neighbour list
// (gaussian.hip, dipole.hip, qeq.hip) and the per-system fixed-order fold (those three, d4.hip / d4_atm.h and the virial fold of ewald.hip).
// Included inside the anonymous namespace of the translation unit, after common.h; __device__ __forceinline__ pieces and one __global__
// template (the pack kernel), nothing here launches a kernel.
//
// Row walk.  One wave64 per row i of the list ([N, M] matrix or CSR), lanes stride the row's entries.  The helpers are the parts every such
// kernel wrote out alike -- the wave's row, the row's range, the padding test, the cell of the row's system, the lattice translation
// S . cell of an entry in the positions dtype -- and NOT a loop taking a callback: each kernel keeps its own visible loop, its own early
// exits and its own accumulators.
//
// Fold.  Grid (MI_FOLD_BLOCKS, n_systems), 256 threads: block (x, s) takes the rows x*256 + t + k*MI_FOLD_BLOCKS*256 of system s
// (batch_idx == NULL: every row), each thread adds its rows in that order, wave butterflies, four wave partials through LDS, added as
// 0 + 1 + 2 + 3, and writes partial[s][x][0..words) with plain stores; the caller sums the MI_FOLD_BLOCKS rows.  No atomics: bit-reproducible.
// Every block scans batch_idx once, O(N n_systems) index reads per launch, L2-resident for the batches this is used with.
#pragma once

#define MI_FOLD_BLOCKS 64  // block partials per system, of every fold kernel (mi_*_blocks() return it)

// ---- math shared by ewald.hip and qeq.hip -------------------------------------------------------------------------------------------------
// 1/x in fp64 from the hardware seed (v_rcp_f64, ~26 bits) + two Newton steps: <= 1 ulp
struct MiNewton {
  static __device__ __forceinline__ double rcp(double x) {
    double y = __builtin_amdgcn_rcp(x);
    y = fma(fma(-x, y, 1.0), y, y);
    y = fma(fma(-x, y, 1.0), y, y);
    return y;
  }
};
// erfc(x) e^{x^2} by Abramowitz & Stegun 7.1.26, times e_neg_x2 = exp(-x^2); x >= 0 (alpha * distance).  Constants verbatim from
// math/math.py:73-78.  Math::rcp is the caller's reciprocal (ewald.hip swaps in the IEEE divide under EW_IEEE_DIV).
template <class Math> __device__ __forceinline__ double erfc_as_poly(double x, double e_neg_x2) {
  const double p = 0.3275911, a1 = 0.254829592, a2 = -0.284496736, a3 = 1.421413741, a4 = -1.453152027, a5 = 1.061405429;
  const double t = Math::rcp(1.0 + p * x);
  const double t2 = t * t, t3 = t2 * t, t4 = t3 * t, t5 = t4 * t;
  const double poly = a1 * t + a2 * t2 + a3 * t3 + a4 * t4 + a5 * t5;
  return poly * e_neg_x2;
}

// ---- the per-system fixed-order fold --------------------------------------------------------------------------------------------------------
// wave sums of a[0..W) -> part[wave][0..W) -> the first `words` threads add the four wave partials in a fixed order into out[0..words)
template <int W> __device__ __forceinline__ void mi_block_fold(double* a, double (*part)[W], double* __restrict__ out, int words) {
  const int lane = threadIdx.x & (MI_WAVE - 1), wave = threadIdx.x / MI_WAVE;
#pragma unroll
  for (int k = 0; k < W; ++k) { const double v = wave_sum(a[k]); if (lane == 0) part[wave][k] = v; }
  __syncthreads();
  if ((int)threadIdx.x < words) out[threadIdx.x] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

// block (x, s) of a (BLOCKS, n_systems) grid: load(r, a) accumulates row r into a[0..W) for the rows of system s in the stride above, then
// partial[s][x][0..words) (row pitch W) = the block's sums
template <int W, int BLOCKS, class Load>
__device__ __forceinline__ void mi_system_fold(const int* __restrict__ batch_idx, int N, int words, double* __restrict__ partial, Load load) {
  const int s = blockIdx.y;
  double a[W];
#pragma unroll
  for (int k = 0; k < W; ++k) a[k] = 0.0;
  for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < N; r += (long long)BLOCKS * 256) {
    if (batch_idx && batch_idx[r] != s) continue;
    load(r, a);
  }
  __shared__ double part[256 / MI_WAVE][W];
  mi_block_fold<W>(a, part, partial + ((size_t)s * BLOCKS + blockIdx.x) * W, words);
}

// ---- the wave-per-row walk ------------------------------------------------------------------------------------------------------------------
// the row of this wave (wave-uniform, in a scalar register)
__device__ __forceinline__ int pair_row_index() {
  return __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x / MI_WAVE) + threadIdx.x / MI_WAVE);
}
// entries [beg, end) of row i: neighbor_ptr of a CSR list, or the row's M slots of a matrix
template <bool CSR> __device__ __forceinline__ void pair_row_range(const int* __restrict__ nptr, int i, int M, long long& beg, long long& end) {
  if (CSR) { beg = nptr[i]; end = nptr[i + 1]; } else { beg = (long long)i * M; end = beg + M; }
}
// padding: mask_value (matrix only), or any index outside [0, N)
template <bool CSR> __device__ __forceinline__ bool pair_is_padding(int j, int mask_value, int N) {
  return (!CSR && j == mask_value) || (unsigned)j >= (unsigned)N;
}
// cm = the cell of system s, row-major
template <class T> __device__ __forceinline__ void pair_row_cell(const T* __restrict__ cell, int s, T cm[9]) {
  for (int k = 0; k < 9; ++k) cm[k] = cell[9 * (size_t)s + k];
}
// sh = S . cm, the lattice translation of entry e of a shifted list in the positions dtype (rowvec_mat3's summation order); returns the integer
// shift S.  The kernel adds sh to r_j - r_i under its own `if (shifted)`: with the branch inside a helper the compiler fuses another product
// of sx sx + sy sy + sz sz into the FMA, and every distance moves in the last bit.
template <class T> __device__ __forceinline__ int3 pair_separation(const int* __restrict__ ush, long long e, const T* cm, T sh[3]) {
  const int3 S = {ush[3 * e], ush[3 * e + 1], ush[3 * e + 2]};
  const T fs[3] = {(T)S.x, (T)S.y, (T)S.z};
  rowvec_mat3(fs, cm, sh);
  return S;
}

// one record per atom so the pair loop gathers one record per neighbour: Rec = {x, y, z, q, tail...} with Rec::set_tail(tail, i) filling the
// kernel's own words (and its padding) from the third per-atom array
template <class Rec, class T>
__global__ void pair_pack_kernel(const T* __restrict__ pos, const T* __restrict__ q, const T* __restrict__ tail, int N, Rec* __restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  Rec r;
  r.x = pos[3 * (size_t)i]; r.y = pos[3 * (size_t)i + 1]; r.z = pos[3 * (size_t)i + 2]; r.q = q[i];
  r.set_tail(tail, (size_t)i);
  rec[i] = r;
}
