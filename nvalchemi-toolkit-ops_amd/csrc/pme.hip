// pme.hip -- reciprocal-space mesh kernels of particle-mesh Ewald.  gfx950.
//
// B-spline charge spreading / gathering (reference: spline.py:127-488 functions, :497-676 and :763-959 kernels),
// Green function + sinc structure factor (interactions/electrostatics/pme_kernels.py:93-331), self/background
// corrections (:340-657) and the elementwise spectrum algebra of _pme_reciprocal_space_impl (pme.py:1418-1419,
// 1455-1477), and -- since round 4 -- the FFTs themselves for power-of-two meshes: the fused mesh solve at the end of this file
// (mi_pme_solve: plane / column transforms in LDS, bodies in fft_lds.h) replaces rfftn -> spectrum algebra -> irfftn (pme.py:1398-1461);
// other meshes go through the hipFFT plans of fft.cpp (the reference leans on torch.fft for all of it).
//
// MI355X-first choices:
//   * spread: MESH-TILE OWNERSHIP, no global atomics on the mesh.  Atoms are binned by the 8^3 mesh tile their stencil starts in
//     (counting sort by tile key with atomic counters, binsort.h: 3 small kernels); one block owns one tile, accumulates the in-tile part of the stencils of the atoms of the <= 8 bins
//     that can reach it in a 4 KB LDS tile (native LDS fp64 adds) and writes the finished tile with plain coalesced stores --
//     every mesh point is written exactly once, the mesh needs no zero-fill.  (Device-scope fp64 atomics to a mesh shared by
//     8 XCDs ran at ~25 G/s: 0.49 ms for the 12.5 M contributions of the headline box.)  The order^2-threads-per-atom atomic
//     kernel remains for meshes that are not multiples of the tile edge (the reference launches N*order^3 threads that
//     each redo the fractional-coordinate transform and all three 1-D weights).
//   * convolve: ONE pass over the half-spectrum produces conv = spec/sf^2*G and the three field spectra -i k_d conv;
//     k, k^2, G and sf^2 are evaluated in registers (no k-vector / Green / structure-factor arrays in HBM).
//   * gather-finish: potential + 3 field components gathered in one kernel with the self/background corrections and the
//     force factor applied in the epilogue (reference: 2 gathers of N*order^3 atomics + 2 elementwise kernels + torch ops).
//   * orders 1-4 use the reference's piecewise polynomials verbatim; orders 5-6 (which the reference evaluates as 0,
//     SURVEY F2) use the cardinal B-spline recursion.
#include <atomic>

#include "binsort.h"
#include "common.h"
#include "fft_lds.h"

namespace {

#define MI_MAX_ORDER 6

// ---- cardinal B-spline M_n(u) on [0,n) ---------------------------------------------------------------
template <class T> __device__ __forceinline__ T bspline_ref(T u, int order) {
  // spline.py:127-194, same polynomial forms and half-open intervals
  const T zero = 0, one = 1, two = 2, three = 3, four = 4, six = 6;
  if (order == 4) {
    if (u >= zero && u < one) return u * u * u / six;
    if (u >= one && u < two) { const T u2 = u * u, u3 = u2 * u; return (T(-3) * u3 + T(12) * u2 - T(12) * u + four) / six; }
    if (u >= two && u < three) { const T u2 = u * u, u3 = u2 * u; return (three * u3 - T(24) * u2 + T(60) * u - T(44)) / six; }
    if (u >= three && u < four) { const T v = four - u; return v * v * v / six; }
    return zero;
  }
  if (order == 3) {
    if (u >= zero && u < one) return u * u / two;
    if (u >= one && u < two) return T(0.75) - (u - T(1.5)) * (u - T(1.5));
    if (u >= two && u < three) { const T v = three - u; return v * v / two; }
    return zero;
  }
  if (order == 2) {
    if (u >= zero && u < one) return u;
    if (u >= one && u < two) return two - u;
    return zero;
  }
  if (order == 1) return (u >= zero && u < one) ? one : zero;
  return zero;
}
// stable bottom-up recursion for orders 5 and 6: value of M_n at u
template <class T> __device__ __forceinline__ T bspline_high(T u, int n) {
  if (!(u >= T(0) && u < T(n))) return T(0);
  T m[MI_MAX_ORDER + 1];
#pragma unroll
  for (int k = 0; k <= MI_MAX_ORDER; ++k) { const T x = u - T(k); m[k] = (x >= T(0) && x < T(1)) ? T(1) : T(0); }  // M_1(u-k)
#pragma unroll
  for (int p = 2; p <= MI_MAX_ORDER; ++p) {
    if (p > n) break;
    const T inv = T(1) / T(p - 1);
#pragma unroll
    for (int k = 0; k <= MI_MAX_ORDER - 2; ++k) {
      if (k > n - p) break;
      const T x = u - T(k);
      m[k] = (x * m[k] + (T(p) - x) * m[k + 1]) * inv;  // M_p(u-k) from M_{p-1}(u-k), M_{p-1}(u-k-1)
    }
  }
  return m[0];
}
template <class T> __device__ __forceinline__ T bspline_weight(T u, int order) {
  return order <= 4 ? bspline_ref(u, order) : bspline_high(u, order);
}

// d M_n / du: the reference's piecewise forms for n <= 4 (spline.py:197-254), M_{n-1}(u) - M_{n-1}(u-1) for n = 5, 6
template <class T> __device__ __forceinline__ T bspline_deriv(T u, int order) {
  const T zero = 0, one = 1, two = 2, three = 3, four = 4, six = 6;
  if (order == 4) {
    if (u >= zero && u < one) return u * u / two;
    if (u >= one && u < two) return (T(-9) * u * u + T(24) * u - T(12)) / six;
    if (u >= two && u < three) return (T(9) * u * u - T(48) * u + T(60)) / six;
    if (u >= three && u < four) { const T v = four - u; return -three * v * v / six; }
    return zero;
  }
  if (order == 3) {
    if (u >= zero && u < one) return u;
    if (u >= one && u < two) return -two * (u - T(1.5));
    if (u >= two && u < three) return -(three - u);
    return zero;
  }
  if (order == 2) {
    if (u >= zero && u < one) return one;
    if (u >= one && u < two) return -one;
    return zero;
  }
  if (order >= 5) return bspline_high(u, order - 1) - bspline_high(u - one, order - 1);
  return zero;
}

// d^2 M_n / du^2: derivative of the piecewise forms above, interval by interval (what differentiating `bspline_deriv` once more gives;
// order 3 is piecewise constant, order 2 zero), M_{n-2}(u) - 2 M_{n-2}(u-1) + M_{n-2}(u-2) for n = 5, 6
template <class T> __device__ __forceinline__ T bspline_deriv2(T u, int order) {
  const T zero = 0, one = 1, two = 2, three = 3, four = 4;
  if (order == 4) {
    if (u >= zero && u < one) return u;
    if (u >= one && u < two) return T(-3) * u + four;
    if (u >= two && u < three) return three * u - T(8);
    if (u >= three && u < four) return four - u;
    return zero;
  }
  if (order == 3) {
    if (u >= zero && u < one) return one;
    if (u >= one && u < two) return -two;
    if (u >= two && u < three) return one;
    return zero;
  }
  if (order >= 5) return bspline_high(u, order - 2) - two * bspline_high(u - one, order - 2) + bspline_high(u - two, order - 2);
  return zero;
}

template <class T> struct Stencil { int base[3]; T theta[3]; int off0[3]; };

// compute_fractional_coords + bspline_grid_offset (spline.py:258-347)
template <class T>
__device__ __forceinline__ Stencil<T> make_stencil(const T* __restrict__ pos3, const T* __restrict__ cit, int nx, int ny, int nz, int order) {
  Stencil<T> s;
  const T p[3] = {pos3[0], pos3[1], pos3[2]};
  T frac[3];
  mat3_colvec(cit, p, frac);
  const int dims[3] = {nx, ny, nz};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const T mc = frac[d] * (T)dims[d];
    s.base[d] = (int)floor(mc);
    s.theta[d] = mc - (T)s.base[d];
    s.off0[d] = (int)floor(s.theta[d] - (T)(order - 2) * T(0.5));
  }
  return s;
}
// 1-D weight of stencil point t (0..order-1) along dimension d; returns 0 outside [0,order) like bspline_weight_3d (:351-408)
template <class T> __device__ __forceinline__ T weight_1d(const Stencil<T>& s, int d, int t, int order) {
  const T u = (T)order * T(0.5) + s.theta[d] - (T)(t + s.off0[d]);
  if (u < T(0) || u >= (T)order) return T(0);
  return bspline_weight(u, order);
}
__device__ __forceinline__ int wrap_idx(int i, int n) { return ((i % n) + n) % n; }

// ---- spread -------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void spline_spread_kernel(const T* __restrict__ pos, const T* __restrict__ values, const int* __restrict__ batch_idx,
                                                            const T* __restrict__ cit, int N, int nx, int ny, int nz, int order, int batched,
                                                            T* __restrict__ mesh) {
  const int tpa = order * order;
  const int apb = blockDim.x / tpa;  // atoms per block
  const int la = threadIdx.x / tpa, col = threadIdx.x - la * tpa;
  const int i = blockIdx.x * apb + la;
  if (la >= apb || i >= N) return;
  const int s = batch_idx ? batch_idx[i] : 0;
  const Stencil<T> st = make_stencil(pos + 3 * (size_t)i, cit + 9 * (size_t)s, nx, ny, nz, order);
  const int tx = col / order, ty = col - tx * order;
  const T wx = weight_1d(st, 0, tx, order), wy = weight_1d(st, 1, ty, order);
  const T val = values[i];
  const int gx = wrap_idx(st.base[0] + tx + st.off0[0], nx), gy = wrap_idx(st.base[1] + ty + st.off0[1], ny);
  T* row = mesh + (((size_t)s * nx + gx) * ny + gy) * nz;
  const T thr = batched ? T(1e-8) : T(0);  // spline.py:548 (w > 0) vs :820 (w > 1e-8)
  for (int tz = 0; tz < order; ++tz) {
    const T wz = weight_1d(st, 2, tz, order);
    const T w = wx * wy * wz;
    if (w > thr) atomicAdd(row + wrap_idx(st.base[2] + tz + st.off0[2], nz), val * w);
  }
}

// ---- tiled spread ----------------------------------------------------------------------------------------------------------
#define MI_SPREAD_TILE_MIN_ATOMS 12000
#define MI_SPREAD_TILE_MIN_TILES 128
#define SP_T 8  // largest mesh tile edge (points).  Per axis the edge is the largest divisor of the mesh dimension that is <= SP_T; a
                // stencil of `order` points starting in tile t reaches at most t and t+1 when order <= edge + 1
struct SpTile { int ex, ey, ez; };
static int sp_edge(int n) { for (int e = SP_T; e > 1; --e) if (n % e == 0) return e; return 1; }
static SpTile sp_tile(int nx, int ny, int nz) { return SpTile{sp_edge(nx), sp_edge(ny), sp_edge(nz)}; }

struct SpLayout { size_t keys_in, vals_out, bin_start, lo3, theta, bins, boxes, total; long long nbins; };
// `order` / `elem_bytes`: what the box scratch -- the last and by far the largest field -- is sized for.  The defaults (largest order, fp64)
// give the size every run fits in (mi_spline_spread_workspace_bytes); an actual (order, dtype) gives the exact size
// (mi_spline_spread_workspace_bytes_for): (e + order - 1)^3 values of the mesh dtype per tile instead of (e + 5)^3 doubles -- a 256^3 fp32
// order-4 mesh needs 178 MB of boxes instead of 576.  All other offsets do not depend on either.
static SpLayout sp_layout(int N, int B, int nx, int ny, int nz, int order = MI_MAX_ORDER, size_t elem_bytes = sizeof(double), int box_channels = 1) {
  SpLayout L;
  size_t o = 0;
  auto take = [&](size_t b) { size_t at = o; o += mi_align(b); return at; };
  const SpTile e = sp_tile(nx, ny, nz);
  L.nbins = (long long)B * (nx / e.ex) * (ny / e.ey) * (nz / e.ez);
  L.keys_in = take(sizeof(int) * (size_t)N);
  L.vals_out = take(sizeof(int) * ((size_t)N + 4));                // [0]: order header (see spread_key_kernel), [4..]: atom ids grouped by tile
  L.bin_start = take(sizeof(int) * (size_t)(L.nbins + 2));
  L.lo3 = take(sizeof(int) * 4 * (size_t)N);                       // first stencil index per axis (wrapped) + system, per atom
  L.theta = take(sizeof(double) * 3 * (size_t)N);                  // fractional offset inside the mesh cell per axis, [3][N] (sized for fp64)
  L.bins = take(sizeof(int) * bs_scratch_ints(L.nbins + 1));  // counting-sort counters (binsort.h)
  // per-tile accumulation boxes of the two-phase spread: (e + order - 1)^3 points per tile
  if (order < 1 || order > MI_MAX_ORDER) order = MI_MAX_ORDER;
  // (box_channels: the channels of one block of the multi-channel spread, spread_box_channels_kernel)
  L.boxes = take(elem_bytes * (size_t)box_channels * (size_t)L.nbins * (e.ex + order - 1) * (e.ey + order - 1) * (e.ez + order - 1));
  L.total = o;
  return L;
}
// `order` <= 0: can ANY order run tiled on this mesh (sizing the workspace)?  Otherwise: can this order?
static bool sp_tiled_ok(int nx, int ny, int nz, int B, int order) {
  const SpTile e = sp_tile(nx, ny, nz);
  const int need = order > 0 ? order - 1 : 1;  // edge >= order - 1; an edge of 1 would be one block per mesh point
  const int emin = e.ex < e.ey ? (e.ex < e.ez ? e.ex : e.ez) : (e.ey < e.ez ? e.ey : e.ez);
  return nx >= MI_MAX_ORDER && ny >= MI_MAX_ORDER && nz >= MI_MAX_ORDER && emin >= (need > 2 ? need : 2) && nx <= 65535 && B <= 65535 &&  // (grid.y / grid.z of the reduce kernel)
         (long long)B * (nx / e.ex) * (ny / e.ey) * (nz / e.ez) < (1ll << 30);
}

template <class T>
__global__ void spread_key_kernel(const T* __restrict__ pos, const int* __restrict__ batch_idx, const T* __restrict__ cit, int N, int nx, int ny,
                                  int nz, int order, SpTile e, int* __restrict__ keys, int* __restrict__ count, int4* __restrict__ lo3,
                                  T* __restrict__ theta, int* __restrict__ incoherent) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < N;
  int key = 0;
  if (in) {
    const int s = batch_idx ? batch_idx[i] : 0;
    const Stencil<T> st = make_stencil(pos + 3 * (size_t)i, cit + 9 * (size_t)s, nx, ny, nz, order);
    const int lx = wrap_idx(st.base[0] + st.off0[0], nx), ly = wrap_idx(st.base[1] + st.off0[1], ny), lz = wrap_idx(st.base[2] + st.off0[2], nz);
    key = ((s * (nx / e.ex) + lx / e.ex) * (ny / e.ey) + ly / e.ey) * (nz / e.ez) + lz / e.ez;
    keys[i] = key;
    // the box kernel evaluates the 1-D weights of its own atoms from exactly these numbers (round 4; this kernel used to store 144 B of weights
    // per atom): stencil start and fractional offsets come from ONE evaluation, so tile and weights cannot disagree at a mesh-cell boundary
    lo3[i] = make_int4(lx, ly, lz, s);
    theta[i] = st.theta[0]; theta[(size_t)N + i] = st.theta[1]; theta[2 * (size_t)N + i] = st.theta[2];
  }
  bs_wave_add<false>(count, key, in);  // the tile's atom counter (binsort.h): one atomic per distinct tile per wave
  // Is the caller's atom order spatially coherent?  Count the consecutive atoms (i, i + 1) that share neither a tile nor a neighbouring
  // one: a lattice- or molecule-ordered system has a few per cent of them, a randomly ordered one nearly all.  The gather epilogue walks
  // the atoms tile by tile instead of in index order when more than a quarter of the pairs are like that (pme_gather_finish_kernel).
  const int nbx = nx / e.ex, nby = ny / e.ey, nbz = nz / e.ez;
  int kk = key;
  const int tz_ = kk % nbz; kk /= nbz;
  const int ty_ = kk % nby; kk /= nby;
  const int tx_ = kk % nbx; const int ts_ = kk / nbx;
  const int nx_ = __shfl_down(tx_, 1, MI_WAVE), ny_ = __shfl_down(ty_, 1, MI_WAVE), nz_ = __shfl_down(tz_, 1, MI_WAVE), ns_ = __shfl_down(ts_, 1, MI_WAVE);
  auto far = [](int a, int b, int n) { int d = a > b ? a - b : b - a; d = d < n - d ? d : n - d; return d > 1; };
  const bool pair = in && i + 1 < N && (threadIdx.x & (MI_WAVE - 1)) != MI_WAVE - 1;
  const bool bad = pair && (ns_ != ts_ || far(tx_, nx_, nbx) || far(ty_, ny_, nby) || far(tz_, nz_, nbz));
  const unsigned long long m = __ballot(bad);
  if (m && (threadIdx.x & (MI_WAVE - 1)) == 0) atomicAdd(incoherent, (int)__popcll(m));
}
// ---- two-phase tile spread (round 4) -------------------------------------------------------------------------------------------------
// Rounds 1 - 3 ran a tile-owned kernel: a block per mesh tile collected from the atoms of up to 8 source tiles (a stencil starting in tile t
// reaches t and t+1 per axis) and threw seven eighths of the visited points away -- 20 M thread-visits for 2.5 M useful columns on the
// headline mesh, each behind three dependent loads (0.092 ms, latency-bound).  Here a tile's block handles ITS atoms once, accumulating whole stencils into an LDS box of
// (e + order - 1)^3 points (tile + forward halo, no wrap inside the box), and writes the box to scratch; a second kernel owns the mesh
// points and adds the <= 8 boxes that cover each: plain coalesced loads, a fixed summation order across tiles, no global atomics.
#define SPB_CHUNK 32  // atoms of the tile staged per pass: their 1-D weights (3 x order each) are evaluated once, by 3 threads per atom, into LDS
template <class T, int ORDER>
__global__ __launch_bounds__(256) void spread_box_kernel(const T* __restrict__ values, const int* __restrict__ atom_of, const int* __restrict__ bin_start,
                                                         const int4* __restrict__ lo3, const T* __restrict__ theta_all, int N, int nx, int ny, int nz,
                                                         int batched, SpTile e, T* __restrict__ boxes, int* __restrict__ order_hdr,
                                                         const int* __restrict__ incoherent) {
  constexpr int order = ORDER, H = ORDER - 1;
  __shared__ T box[(SP_T + H) * (SP_T + H) * (SP_T + H)];
  __shared__ T wl[SPB_CHUNK][3][ORDER];
  __shared__ int lo_s[SPB_CHUNK][3];
  __shared__ T val_s[SPB_CHUNK];
  if (blockIdx.x == 0 && threadIdx.x == 0) order_hdr[0] = *incoherent;  // header of the tile-grouped atom list (read by the gather epilogue)
  const int nbx = nx / e.ex, nby = ny / e.ey, nbz = nz / e.ez;
  const int bxn = e.ex + H, byn = e.ey + H, bzn = e.ez + H, box_n = bxn * byn * bzn;
  int b = blockIdx.x;
  const int bz = b % nbz; b /= nbz;
  const int by = b % nby; b /= nby;
  const int bx = b % nbx;
  const int org[3] = {bx * e.ex, by * e.ey, bz * e.ez};
  for (int k = threadIdx.x; k < box_n; k += blockDim.x) box[k] = T(0);
  const int tpa = order * order;
  const T thr = batched ? T(1e-8) : T(0);  // spline.py:548 (w > 0) vs :820 (w > 1e-8)
  const int beg = bin_start[blockIdx.x], end = bin_start[blockIdx.x + 1];
  for (int c0 = beg; c0 < end; c0 += SPB_CHUNK) {
    const int nc = end - c0 < SPB_CHUNK ? end - c0 : SPB_CHUNK;
    __syncthreads();  // box zeroed / previous chunk consumed
    if (threadIdx.x < 3 * nc) {
      // one thread per (atom, axis): the `order` 1-D weights of that axis from the key kernel's fractional offset (weight_1d's expression:
      // bspline_grid_offset + bspline_weight_3d, spline.py:300-408) and the stencil start in box coordinates
      const int a = threadIdx.x / 3, d = threadIdx.x - 3 * a;
      const int i = atom_of[c0 + a];
      const int4 lo = lo3[i];
      const T theta = theta_all[(size_t)d * N + i];
      const int off0 = (int)floor(theta - (T)(order - 2) * T(0.5));
      lo_s[a][d] = (d == 0 ? lo.x : (d == 1 ? lo.y : lo.z)) - org[d];  // inside [0, e): the bin key IS the tile of the stencil's first point
#pragma unroll
      for (int t = 0; t < order; ++t) {
        const T u = (T)order * T(0.5) + theta - (T)(t + off0);
        wl[a][d][t] = (u < T(0) || u >= (T)order) ? T(0) : bspline_weight(u, order);
      }
      if (d == 0) val_s[a] = values[i];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nc * tpa; t += blockDim.x) {
      const int a = t / tpa, col = t - a * tpa;
      const int tx = col / order, ty = col - tx * order;
      const T wxy = wl[a][0][tx] * wl[a][1][ty];
      const T val = val_s[a];
      T* row = box + ((lo_s[a][0] + tx) * byn + lo_s[a][1] + ty) * bzn + lo_s[a][2];  // box coordinates need no wrap
#pragma unroll
      for (int tz = 0; tz < order; ++tz) {
        const T w = wxy * wl[a][2][tz];
        if (w > thr) atomicAdd(row + tz, val * w);
      }
    }
  }
  __syncthreads();
  T* out = boxes + (size_t)blockIdx.x * box_n;
  for (int k = threadIdx.x; k < box_n; k += blockDim.x) out[k] = box[k];
}
// thread per mesh point: its own tile's box plus, per axis, the previous tile's box where the point lies inside that tile's forward halo
template <class T>
__global__ __launch_bounds__(256) void spread_box_reduce_kernel(const T* __restrict__ boxes, int nx, int ny, int nz, int B, int order, SpTile e,
                                                               T* __restrict__ mesh) {
  // grid = (ceil(ny nz / 256), nx, B): one 32-bit division per thread for (y, z); x and the system are block-uniform.  (A flat 64-bit index
  // cost five 64-bit divisions per mesh point -- most of this kernel's instructions.)
  const unsigned yz = blockIdx.x * blockDim.x + threadIdx.x;
  if (yz >= (unsigned)ny * (unsigned)nz) return;
  const int y = (int)(yz / (unsigned)nz), z = (int)(yz - (unsigned)y * (unsigned)nz), x = (int)blockIdx.y, s = (int)blockIdx.z;
  const size_t g = ((size_t)s * nx + x) * ((size_t)ny * nz) + yz;
  const int H = order - 1;
  const int nbx = nx / e.ex, nby = ny / e.ey, nbz = nz / e.ez;
  const int bxn = e.ex + H, byn = e.ey + H, bzn = e.ez + H;
  const size_t box_n = (size_t)bxn * byn * bzn;
  const int tx = x / e.ex, ty = y / e.ey, tz = z / e.ez;
  const int lx = x - tx * e.ex, ly = y - ty * e.ey, lz = z - tz * e.ez;
  T acc = T(0);
  for (int dx = 0; dx < 2; ++dx) {
    if (dx && lx >= H) break;
    const int sx = dx ? (tx == 0 ? nbx - 1 : tx - 1) : tx, px = lx + dx * e.ex;
    for (int dy = 0; dy < 2; ++dy) {
      if (dy && ly >= H) break;
      const int sy = dy ? (ty == 0 ? nby - 1 : ty - 1) : ty, py = ly + dy * e.ey;
      for (int dz = 0; dz < 2; ++dz) {
        if (dz && lz >= H) break;
        const int sz = dz ? (tz == 0 ? nbz - 1 : tz - 1) : tz, pz = lz + dz * e.ez;
        const size_t tile = (((size_t)s * nbx + sx) * nby + sy) * nbz + sz;
        acc += boxes[tile * box_n + ((size_t)px * byn + py) * bzn + pz];
      }
    }
  }
  mesh[g] = acc;
}

// ---- multi-channel spread (values[N, C] -> mesh[B, C, nx, ny, nz]) ------------------------------------------------------------------
// The channels of a multipole spread share the stencil, the tile and the 3 x order 1-D weights of every atom; only the per-atom value
// differs.  Atomic path: the scalar kernel's thread mapping, weights once, a loop over the channels around the atomic add.
template <class T>
__global__ __launch_bounds__(256) void spline_spread_channels_kernel(const T* __restrict__ pos, const T* __restrict__ values,
                                                                     const int* __restrict__ batch_idx, const T* __restrict__ cit, int N, int C,
                                                                     int nx, int ny, int nz, int order, int batched, T* __restrict__ mesh) {
  const int tpa = order * order;
  const int apb = blockDim.x / tpa;  // atoms per block
  const int la = threadIdx.x / tpa, col = threadIdx.x - la * tpa;
  const int i = blockIdx.x * apb + la;
  if (la >= apb || i >= N) return;
  const int s = batch_idx ? batch_idx[i] : 0;
  const Stencil<T> st = make_stencil(pos + 3 * (size_t)i, cit + 9 * (size_t)s, nx, ny, nz, order);
  const int tx = col / order, ty = col - tx * order;
  const T wx = weight_1d(st, 0, tx, order), wy = weight_1d(st, 1, ty, order);
  const int gx = wrap_idx(st.base[0] + tx + st.off0[0], nx), gy = wrap_idx(st.base[1] + ty + st.off0[1], ny);
  const size_t plane = (size_t)nx * ny * nz;
  T* row = mesh + (size_t)s * C * plane + ((size_t)gx * ny + gy) * nz;
  const T* vals = values + (size_t)i * C;
  const T thr = batched ? T(1e-8) : T(0);  // the scalar kernel's thresholds (spline.py:548 / :820), not :1107's
  for (int tz = 0; tz < order; ++tz) {
    const T wz = weight_1d(st, 2, tz, order);
    const T w = wx * wy * wz;
    if (w > thr) {
      T* p = row + wrap_idx(st.base[2] + tz + st.off0[2], nz);
      for (int c = 0; c < C; ++c) atomicAdd(p + (size_t)c * plane, vals[c] * w);
    }
  }
}

// Tile path: key kernel and counting sort run once per call; the box kernel below accumulates a BLOCK of channels into LDS boxes from one
// staging of the chunk's weights, and the reduce writes that block's mesh planes.  The channel block is what keeps three thread blocks on
// a CU: the boxes of one block of channels take at most SPC_LDS_BYTES of the CU's 160 KiB (fp64, order 6: 2 x 17.6 KB; fp32, order 4: 9 x
// 5.3 KB).  The host runs box + reduce once per channel block, so the box scratch is sized for one block, not for C channels.
#define SPC_LDS_BYTES 49152
#define SPC_MAX_BLOCK 9
constexpr int spc_block_max(int order, size_t elem_bytes) {
  const size_t box = (size_t)(SP_T + order - 1) * (SP_T + order - 1) * (SP_T + order - 1) * elem_bytes;
  const int m = (int)(SPC_LDS_BYTES / box);
  return m < 1 ? 1 : (m > SPC_MAX_BLOCK ? SPC_MAX_BLOCK : m);
}
struct SpcPlan { int nblk, cb; };  // number of channel blocks and channels per block (the last block may hold fewer)
static SpcPlan spc_plan(int C, int order, size_t elem_bytes) {
  const int m = spc_block_max(order, elem_bytes);
  const int nblk = (C + m - 1) / m;
  return SpcPlan{nblk, (C + nblk - 1) / nblk};  // 9 channels at a limit of 4: three blocks of 3, not 4 + 4 + 1
}
static bool spc_tiled_ok(int nx, int ny, int nz, int B, int order, int C, size_t elem_bytes) {
  return sp_tiled_ok(nx, ny, nz, B, order) && (long long)B * spc_plan(C, order, elem_bytes).cb <= 65535;  // grid.z of the reduce
}

template <class T, int ORDER>
__global__ __launch_bounds__(256) void spread_box_channels_kernel(const T* __restrict__ values, int C, int c0, int cb,
                                                                  const int* __restrict__ atom_of, const int* __restrict__ bin_start,
                                                                  const int4* __restrict__ lo3, const T* __restrict__ theta_all, int N, int nx, int ny,
                                                                  int nz, int batched, SpTile e, T* __restrict__ boxes) {
  constexpr int order = ORDER, H = ORDER - 1, CBM = spc_block_max(ORDER, sizeof(T));
  __shared__ T box[CBM * (SP_T + H) * (SP_T + H) * (SP_T + H)];  // [cb][box_n]
  __shared__ T wl[SPB_CHUNK][3][ORDER];
  __shared__ int lo_s[SPB_CHUNK][3];
  __shared__ T val_s[SPB_CHUNK][CBM];
  const int nbx = nx / e.ex, nby = ny / e.ey, nbz = nz / e.ez;
  const int bxn = e.ex + H, byn = e.ey + H, bzn = e.ez + H, box_n = bxn * byn * bzn;
  int b = blockIdx.x;
  const int bz = b % nbz; b /= nbz;
  const int by = b % nby; b /= nby;
  const int bx = b % nbx;
  const int org[3] = {bx * e.ex, by * e.ey, bz * e.ez};
  for (int k = threadIdx.x; k < cb * box_n; k += blockDim.x) box[k] = T(0);
  const int tpa = order * order;
  const T thr = batched ? T(1e-8) : T(0);
  const int beg = bin_start[blockIdx.x], end = bin_start[blockIdx.x + 1];
  for (int a0 = beg; a0 < end; a0 += SPB_CHUNK) {
    const int nc = end - a0 < SPB_CHUNK ? end - a0 : SPB_CHUNK;
    __syncthreads();  // boxes zeroed / previous chunk consumed
    if (threadIdx.x < 3 * nc) {  // one thread per (atom, axis), as in spread_box_kernel
      const int a = threadIdx.x / 3, d = threadIdx.x - 3 * a;
      const int i = atom_of[a0 + a];
      const int4 lo = lo3[i];
      const T theta = theta_all[(size_t)d * N + i];
      const int off0 = (int)floor(theta - (T)(order - 2) * T(0.5));
      lo_s[a][d] = (d == 0 ? lo.x : (d == 1 ? lo.y : lo.z)) - org[d];
#pragma unroll
      for (int t = 0; t < order; ++t) {
        const T u = (T)order * T(0.5) + theta - (T)(t + off0);
        wl[a][d][t] = (u < T(0) || u >= (T)order) ? T(0) : bspline_weight(u, order);
      }
    }
    for (int k = threadIdx.x; k < nc * cb; k += blockDim.x) {
      const int a = k / cb, c = k - a * cb;
      val_s[a][c] = values[(size_t)atom_of[a0 + a] * C + c0 + c];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < nc * tpa; t += blockDim.x) {
      const int a = t / tpa, col = t - a * tpa;
      const int tx = col / order, ty = col - tx * order;
      const T wxy = wl[a][0][tx] * wl[a][1][ty];
      T* row = box + ((lo_s[a][0] + tx) * byn + lo_s[a][1] + ty) * bzn + lo_s[a][2];  // box coordinates need no wrap
#pragma unroll
      for (int tz = 0; tz < order; ++tz) {
        const T w = wxy * wl[a][2][tz];
        if (w > thr)
          for (int c = 0; c < cb; ++c) atomicAdd(row + c * box_n + tz, val_s[a][c] * w);
      }
    }
  }
  __syncthreads();
  T* out = boxes + (size_t)blockIdx.x * cb * box_n;  // [tile][cb][box_n]
  for (int k = threadIdx.x; k < cb * box_n; k += blockDim.x) out[k] = box[k];
}
// spread_box_reduce_kernel for one block of channels: grid.z = system * cb + channel of the block
template <class T>
__global__ __launch_bounds__(256) void spread_box_reduce_channels_kernel(const T* __restrict__ boxes, int nx, int ny, int nz, int C, int c0, int cb,
                                                                        int order, SpTile e, T* __restrict__ mesh) {
  const unsigned yz = blockIdx.x * blockDim.x + threadIdx.x;
  if (yz >= (unsigned)ny * (unsigned)nz) return;
  const int y = (int)(yz / (unsigned)nz), z = (int)(yz - (unsigned)y * (unsigned)nz), x = (int)blockIdx.y;
  const int s = (int)blockIdx.z / cb, c = (int)blockIdx.z - s * cb;
  const size_t g = (((size_t)s * C + c0 + c) * nx + x) * ((size_t)ny * nz) + yz;
  const int H = order - 1;
  const int nbx = nx / e.ex, nby = ny / e.ey, nbz = nz / e.ez;
  const int bxn = e.ex + H, byn = e.ey + H, bzn = e.ez + H;
  const size_t box_n = (size_t)bxn * byn * bzn;
  const int tx = x / e.ex, ty = y / e.ey, tz = z / e.ez;
  const int lx = x - tx * e.ex, ly = y - ty * e.ey, lz = z - tz * e.ez;
  T acc = T(0);
  for (int dx = 0; dx < 2; ++dx) {
    if (dx && lx >= H) break;
    const int sx = dx ? (tx == 0 ? nbx - 1 : tx - 1) : tx, px = lx + dx * e.ex;
    for (int dy = 0; dy < 2; ++dy) {
      if (dy && ly >= H) break;
      const int sy = dy ? (ty == 0 ? nby - 1 : ty - 1) : ty, py = ly + dy * e.ey;
      for (int dz = 0; dz < 2; ++dz) {
        if (dz && lz >= H) break;
        const int sz = dz ? (tz == 0 ? nbz - 1 : tz - 1) : tz, pz = lz + dz * e.ez;
        const size_t tile = (((size_t)s * nbx + sx) * nby + sy) * nbz + sz;
        acc += boxes[(tile * cb + c) * box_n + ((size_t)px * byn + py) * bzn + pz];
      }
    }
  }
  mesh[g] = acc;
}

// ---- per-system cell geometry in one launch: cell^-T (fractional-coordinate transform), 2 pi cell^-1 (reciprocal rows), |det|
// (replaces torch.linalg.inv_ex + det + the elementwise glue of `_pme_reciprocal_space_impl`, pme.py:1382-1395: ~30 launches)
template <class T>
__global__ void cell_geometry_kernel(const T* __restrict__ cell, int B, T* __restrict__ cit, T* __restrict__ recip, T* __restrict__ vol) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= B) return;
  const T* a = cell + 9 * (size_t)s;
  T inv[9];
  inverse3(a, inv);
  const T det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      cit[9 * (size_t)s + 3 * r + c] = inv[3 * c + r];
      recip[9 * (size_t)s + 3 * r + c] = (T)(2.0 * M_PI) * inv[3 * r + c];
    }
  vol[s] = det < T(0) ? -det : det;
}

// geometry of every system AND the per-system total charge in one launch (threads < B: geometry; all threads: wave-reduced charge
// sums, one atomic per wave and system) -- replaces mi_cell_geometry + a zero-fill + mi_segment_sum in the fused PME step
template <class T>
__global__ __launch_bounds__(256) void pme_prepare_kernel(const T* __restrict__ cell, const T* __restrict__ charges, const int* __restrict__ batch_idx,
                                                          int N, int B, T* __restrict__ cit, T* __restrict__ recip, T* __restrict__ vol,
                                                          T* __restrict__ qtot /*zeroed*/) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < B) {
    const T* a = cell + 9 * (size_t)t;
    T inv[9];
    inverse3(a, inv);
    const T det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        cit[9 * (size_t)t + 3 * r + c] = inv[3 * c + r];
        recip[9 * (size_t)t + 3 * r + c] = (T)(2.0 * M_PI) * inv[3 * r + c];
      }
    vol[t] = det < T(0) ? -det : det;
  }
  // total charge per system.  Each thread takes atoms t, t + stride, ... (a contiguous run of atoms per wave trip); a wave whose 64 atoms
  // share a system adds its sum to a running (system, sum) pair and touches global memory once per system change, and the waves of a
  // block whose pairs agree at the end are combined in LDS first -- the single-system headline box issued 1563 same-address fp64 atomics
  // (one per wave) before, 20 us of serialisation on the PME branch; now <= 128.
  const int lane = threadIdx.x & (MI_WAVE - 1), wave = threadIdx.x / MI_WAVE;
  const long long stride = (long long)gridDim.x * blockDim.x;
  int cur = -1;
  T acc = T(0);
  for (long long a = t; a - lane < N; a += stride) {  // (wave-uniform trip count)
    const bool in = a < N;
    const int s = in ? (batch_idx ? batch_idx[a] : 0) : -1;
    T x = in ? charges[a] : T(0);
    const int s0 = __shfl(s, 0, MI_WAVE);
    if (__all(!in || s == s0)) {
      x = wave_sum(x);
      if (s0 != cur) { if (lane == 0 && cur >= 0) atomicAdd(&qtot[cur], acc); cur = s0; acc = T(0); }
      acc += x;
    } else if (in) {
      atomicAdd(&qtot[s], x);
    }
  }
  __shared__ int cur_sh[4];
  __shared__ T acc_sh[4];
  if (lane == 0) { cur_sh[wave] = cur; acc_sh[wave] = acc; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < (int)(blockDim.x / MI_WAVE); ++w) {
      if (cur_sh[w] < 0) continue;
      T v = acc_sh[w];
      for (int u = w + 1; u < (int)(blockDim.x / MI_WAVE); ++u) if (cur_sh[u] == cur_sh[w]) { v += acc_sh[u]; cur_sh[u] = -1; }
      atomicAdd(&qtot[cur_sh[w]], v);
    }
  }
}

// ---- gathers (one thread per atom, z innermost) -----------------------------------------------------------
// CH = 1: scalar mesh [B,nx,ny,nz] -> out[N];  CH = 3: interleaved mesh [B,nx,ny,nz,3] times charge -> out[N,3]
template <class T, int CH>
__global__ void spline_gather_kernel(const T* __restrict__ pos, const T* __restrict__ charges, const T* __restrict__ mesh,
                                     const int* __restrict__ batch_idx, const T* __restrict__ cit, int N, int nx, int ny, int nz, int order,
                                     T* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int s = batch_idx ? batch_idx[i] : 0;
  const Stencil<T> st = make_stencil(pos + 3 * (size_t)i, cit + 9 * (size_t)s, nx, ny, nz, order);
  T wz[MI_MAX_ORDER];
  int gz[MI_MAX_ORDER];
  for (int t = 0; t < order; ++t) { wz[t] = weight_1d(st, 2, t, order); gz[t] = wrap_idx(st.base[2] + t + st.off0[2], nz); }
  const T q = CH == 3 ? charges[i] : T(1);
  T acc[CH];
  for (int c = 0; c < CH; ++c) acc[c] = T(0);
  for (int tx = 0; tx < order; ++tx) {
    const T wx = weight_1d(st, 0, tx, order);
    const int gx = wrap_idx(st.base[0] + tx + st.off0[0], nx);
    for (int ty = 0; ty < order; ++ty) {
      const T wxy = wx * weight_1d(st, 1, ty, order);
      const int gy = wrap_idx(st.base[1] + ty + st.off0[1], ny);
      const T* row = mesh + ((((size_t)s * nx + gx) * ny + gy) * nz) * CH;
      for (int tz = 0; tz < order; ++tz) {
        const T w = wxy * wz[tz];
        if (w > T(1e-8)) {  // spline.py:608,670,885,953
          if (CH == 1) acc[0] += row[gz[tz]] * w;
          else for (int c = 0; c < CH; ++c) acc[c] += (q * row[(size_t)gz[tz] * CH + c]) * w;
        }
      }
    }
  }
  for (int c = 0; c < CH; ++c) out[(size_t)i * CH + c] = acc[c];
}

// gradient of the scalar gather w.r.t. the fractional coordinate (x mesh dims): building block of the spread/gather adjoints
template <class T, int ORDER>
__global__ __launch_bounds__(128) void spline_gather_grad_kernel(const T* __restrict__ pos, const T* __restrict__ mesh, const int* __restrict__ batch_idx,
                                          const T* __restrict__ cit, int N, int nx, int ny, int nz, T* __restrict__ out) {
  // ORDER is a template parameter: every stencil loop unrolls and the 1-D weight tables stay in registers (with a run-time order they
  // were indexed dynamically and lived in scratch: 160 / 368 B per thread)
  constexpr int order = ORDER;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int s = batch_idx ? batch_idx[i] : 0;
  const Stencil<T> st = make_stencil(pos + 3 * (size_t)i, cit + 9 * (size_t)s, nx, ny, nz, order);
  T w1[3][ORDER], d1[3][ORDER];
  int gi[3][ORDER];
  const int dims[3] = {nx, ny, nz};
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int t = 0; t < order; ++t) {
      const T u = (T)order * T(0.5) + st.theta[d] - (T)(t + st.off0[d]);
      const bool in = !(u < T(0) || u >= (T)order);
      w1[d][t] = in ? bspline_weight(u, order) : T(0);
      d1[d][t] = in ? bspline_deriv(u, order) * (T)dims[d] : T(0);  // du/dtheta = +1, dtheta/dfrac = dims
      gi[d][t] = wrap_idx(st.base[d] + t + st.off0[d], dims[d]);
    }
  T gx = 0, gy = 0, gz = 0;
  const T* m0 = mesh + (size_t)s * nx * ny * nz;
#pragma unroll
  for (int tx = 0; tx < order; ++tx)
#pragma unroll
    for (int ty = 0; ty < order; ++ty) {
      const T* row = m0 + ((size_t)gi[0][tx] * ny + gi[1][ty]) * nz;
      const T wxy = w1[0][tx] * w1[1][ty], dxy = d1[0][tx] * w1[1][ty], xdy = w1[0][tx] * d1[1][ty];
#pragma unroll
      for (int tz = 0; tz < order; ++tz) {
        const T v = row[gi[2][tz]];
        gx += v * dxy * w1[2][tz];
        gy += v * xdy * w1[2][tz];
        gz += v * wxy * d1[2][tz];
      }
    }
  out[3 * (size_t)i] = gx; out[3 * (size_t)i + 1] = gy; out[3 * (size_t)i + 2] = gz;
}

// ---- multi-channel gathers (mesh[B, C, nx, ny, nz] -> out[N, C]) -------------------------------------------------------------------
// One thread per atom: stencil, wrapped z indices and z weights once, SGC_BLOCK channel accumulators, a loop over channel blocks for larger
// C.  The body is spline_gather_kernel<T, 1>'s, statement for statement (run-time order, the same loop nest, wxy = wx * wy, w = wxy * wz,
// the w > 1e-8 test, acc += mesh * w), with the channel loop around the accumulation only: a channel must equal the scalar gather of its
// plane bit for bit, and the compiler contracts / packs the fp32 stencil arithmetic differently once the loops are unrolled over a
// compile-time order (tests/test_spline_channels_gpu.py asserts the equality for every order, dtype and channel count).
#define SGC_BLOCK 5
template <class T, bool FULL>
__device__ __forceinline__ void gather_channel_block(const Stencil<T>& st, const T* __restrict__ wz, const int* __restrict__ gz, const T* __restrict__ m0,
                                                     size_t plane, int nc, int nx, int ny, int nz, int order, T* __restrict__ out) {
  T acc[SGC_BLOCK];
#pragma unroll
  for (int c = 0; c < SGC_BLOCK; ++c) acc[c] = T(0);
  for (int tx = 0; tx < order; ++tx) {
    const T wx = weight_1d(st, 0, tx, order);
    const int gx = wrap_idx(st.base[0] + tx + st.off0[0], nx);
    for (int ty = 0; ty < order; ++ty) {
      const T wxy = wx * weight_1d(st, 1, ty, order);
      const int gy = wrap_idx(st.base[1] + ty + st.off0[1], ny);
      const T* row = m0 + ((size_t)gx * ny + gy) * nz;
      for (int tz = 0; tz < order; ++tz) {
        const T w = wxy * wz[tz];
        if (w > T(1e-8)) {
#pragma unroll
          for (int c = 0; c < SGC_BLOCK; ++c)
            if (FULL || c < nc) acc[c] += row[(size_t)c * plane + gz[tz]] * w;
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < SGC_BLOCK; ++c)
    if (FULL || c < nc) out[c] = acc[c];
}
template <class T>
__global__ __launch_bounds__(128) void spline_gather_channels_kernel(const T* __restrict__ pos, const T* __restrict__ mesh,
                                                                     const int* __restrict__ batch_idx, const T* __restrict__ cit, int N, int C, int nx,
                                                                     int ny, int nz, int order, T* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int s = batch_idx ? batch_idx[i] : 0;
  const Stencil<T> st = make_stencil(pos + 3 * (size_t)i, cit + 9 * (size_t)s, nx, ny, nz, order);
  T wz[MI_MAX_ORDER];
  int gz[MI_MAX_ORDER];
  for (int t = 0; t < order; ++t) { wz[t] = weight_1d(st, 2, t, order); gz[t] = wrap_idx(st.base[2] + t + st.off0[2], nz); }
  const size_t plane = (size_t)nx * ny * nz;
  const T* m0 = mesh + (size_t)s * C * plane;
  T* o = out + (size_t)i * C;
  int c0 = 0;
  for (; c0 + SGC_BLOCK <= C; c0 += SGC_BLOCK) gather_channel_block<T, true>(st, wz, gz, m0 + (size_t)c0 * plane, plane, SGC_BLOCK, nx, ny, nz, order, o + c0);
  if (c0 < C) gather_channel_block<T, false>(st, wz, gz, m0 + (size_t)c0 * plane, plane, C - c0, nx, ny, nz, order, o + c0);
}

// out[i][a] = sum_c coef[i][c] sum_g mesh[c][g] dW_i(g) / dfrac_a: spline_gather_grad_kernel on the per-atom combination of the channel
// planes.  Weights and derivative weights (times the mesh dimension) once per atom; the channels enter only through v = sum_c coef_c mesh_c.
template <class T, int ORDER>
__global__ __launch_bounds__(128) void spline_gather_channels_frac_grad_kernel(const T* __restrict__ pos, const T* __restrict__ mesh,
                                                                               const T* __restrict__ coef, const int* __restrict__ batch_idx,
                                                                               const T* __restrict__ cit, int N, int C, int nx, int ny, int nz,
                                                                               T* __restrict__ out) {
  constexpr int order = ORDER;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int s = batch_idx ? batch_idx[i] : 0;
  const Stencil<T> st = make_stencil(pos + 3 * (size_t)i, cit + 9 * (size_t)s, nx, ny, nz, order);
  T w1[2][ORDER], d1[2][ORDER];  // y and z tables; the x pair is evaluated inside the (rolled) outer loop
  int gi[2][ORDER];
  const int dims[3] = {nx, ny, nz};
#pragma unroll
  for (int d = 1; d < 3; ++d)
#pragma unroll
    for (int t = 0; t < order; ++t) {
      const T u = (T)order * T(0.5) + st.theta[d] - (T)(t + st.off0[d]);
      const bool in = !(u < T(0) || u >= (T)order);
      w1[d - 1][t] = in ? bspline_weight(u, order) : T(0);
      d1[d - 1][t] = in ? bspline_deriv(u, order) * (T)dims[d] : T(0);
      gi[d - 1][t] = wrap_idx(st.base[d] + t + st.off0[d], dims[d]);
    }
  const size_t plane = (size_t)nx * ny * nz;
  const T* m0 = mesh + (size_t)s * C * plane;
  const T* cf = coef + (size_t)i * C;
  T gx = 0, gy = 0, gz = 0;
  for (int c0 = 0; c0 < C; c0 += SGC_BLOCK) {
    const int nc = C - c0 < SGC_BLOCK ? C - c0 : SGC_BLOCK;
    T k[SGC_BLOCK];
#pragma unroll
    for (int c = 0; c < SGC_BLOCK; ++c) k[c] = c < nc ? cf[c0 + c] : T(0);
    const T* mb = m0 + (size_t)c0 * plane;
#pragma unroll 1
    for (int tx = 0; tx < order; ++tx) {
      const T u = (T)order * T(0.5) + st.theta[0] - (T)(tx + st.off0[0]);
      const bool in = !(u < T(0) || u >= (T)order);
      const T wx = in ? bspline_weight(u, order) : T(0), dx = in ? bspline_deriv(u, order) * (T)nx : T(0);
      const int ix = wrap_idx(st.base[0] + tx + st.off0[0], nx);
#pragma unroll
      for (int ty = 0; ty < order; ++ty) {
        const T* row = mb + ((size_t)ix * ny + gi[0][ty]) * nz;
        const T wxy = wx * w1[0][ty], dxy = dx * w1[0][ty], xdy = wx * d1[0][ty];
#pragma unroll
        for (int tz = 0; tz < order; ++tz) {
          T v = T(0);
#pragma unroll
          for (int c = 0; c < SGC_BLOCK; ++c)
            if (c < nc) v += k[c] * row[(size_t)c * plane + gi[1][tz]];
          gx += v * dxy * w1[1][tz];
          gy += v * xdy * w1[1][tz];
          gz += v * wxy * d1[1][tz];
        }
      }
    }
  }
  out[3 * (size_t)i] = gx; out[3 * (size_t)i + 1] = gy; out[3 * (size_t)i + 2] = gz;
}

// Second-order building blocks of the adjoint of `spline_gather_gradient` (F_i = -q_i sum_a G_i[a] cit[a][.], G = the kernel above):
//   hess_dot   out_i[b] = sum_g mesh[g] sum_a v_i[a] d^2 W_i(g) / dfrac_a dfrac_b      (dL/dfrac_i for L = sum_i v_i . G_i)
//   spread_grad mesh[g] += sum_i sum_a v_i[a] d W_i(g) / dfrac_a                        (dL/dmesh)
// One thread per atom; `spread_grad` uses atomics (training path, not the step the bench times).
template <class T, int ORDER> struct Stencil2 { T w[3][ORDER], d[3][ORDER], dd[3][ORDER]; int gi[3][ORDER]; };
template <class T, int ORDER>
__device__ __forceinline__ void stencil_derivs(const Stencil<T>& st, int nx, int ny, int nz, bool second, Stencil2<T, ORDER>& o) {
  constexpr int order = ORDER;
  const int dims[3] = {nx, ny, nz};
#pragma unroll
  for (int d = 0; d < 3; ++d)
#pragma unroll
    for (int t = 0; t < order; ++t) {
      const T u = (T)order * T(0.5) + st.theta[d] - (T)(t + st.off0[d]);
      const bool in = !(u < T(0) || u >= (T)order);
      const T n = (T)dims[d];
      o.w[d][t] = in ? bspline_weight(u, order) : T(0);
      o.d[d][t] = in ? bspline_deriv(u, order) * n : T(0);
      o.dd[d][t] = (in && second) ? bspline_deriv2(u, order) * n * n : T(0);
      o.gi[d][t] = wrap_idx(st.base[d] + t + st.off0[d], dims[d]);
    }
}
template <class T, int ORDER>
__global__ __launch_bounds__(128) void spline_gather_hess_dot_kernel(const T* __restrict__ pos, const T* __restrict__ mesh, const int* __restrict__ batch_idx,
                                              const T* __restrict__ cit, const T* __restrict__ vec, int N, int nx, int ny, int nz,
                                              T* __restrict__ out) {
  constexpr int order = ORDER;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int s = batch_idx ? batch_idx[i] : 0;
  const Stencil<T> st = make_stencil(pos + 3 * (size_t)i, cit + 9 * (size_t)s, nx, ny, nz, order);
  Stencil2<T, ORDER> k;
  stencil_derivs<T, ORDER>(st, nx, ny, nz, true, k);
  const T vx = vec[3 * (size_t)i], vy = vec[3 * (size_t)i + 1], vz = vec[3 * (size_t)i + 2];
  T ox = 0, oy = 0, oz = 0;
  const T* m0 = mesh + (size_t)s * nx * ny * nz;
#pragma unroll
  for (int tx = 0; tx < order; ++tx)
#pragma unroll
    for (int ty = 0; ty < order; ++ty) {
      const T* row = m0 + ((size_t)k.gi[0][tx] * ny + k.gi[1][ty]) * nz;
      const T wx = k.w[0][tx], dx = k.d[0][tx], ddx = k.dd[0][tx], wy = k.w[1][ty], dy = k.d[1][ty], ddy = k.dd[1][ty];
#pragma unroll
      for (int tz = 0; tz < order; ++tz) {
        const T m = row[k.gi[2][tz]];
        const T wz = k.w[2][tz], dz = k.d[2][tz], ddz = k.dd[2][tz];
        // Hessian of wx wy wz in (x, y, z)
        const T hxx = ddx * wy * wz, hyy = wx * ddy * wz, hzz = wx * wy * ddz, hxy = dx * dy * wz, hxz = dx * wy * dz, hyz = wx * dy * dz;
        ox += m * (vx * hxx + vy * hxy + vz * hxz);
        oy += m * (vx * hxy + vy * hyy + vz * hyz);
        oz += m * (vx * hxz + vy * hyz + vz * hzz);
      }
    }
  out[3 * (size_t)i] = ox; out[3 * (size_t)i + 1] = oy; out[3 * (size_t)i + 2] = oz;
}
template <class T, int ORDER>
__global__ __launch_bounds__(128) void spline_spread_grad_kernel(const T* __restrict__ pos, const T* __restrict__ vec, const int* __restrict__ batch_idx,
                                          const T* __restrict__ cit, int N, int nx, int ny, int nz, T* __restrict__ mesh) {
  constexpr int order = ORDER;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int s = batch_idx ? batch_idx[i] : 0;
  const Stencil<T> st = make_stencil(pos + 3 * (size_t)i, cit + 9 * (size_t)s, nx, ny, nz, order);
  Stencil2<T, ORDER> k;
  stencil_derivs<T, ORDER>(st, nx, ny, nz, false, k);
  const T vx = vec[3 * (size_t)i], vy = vec[3 * (size_t)i + 1], vz = vec[3 * (size_t)i + 2];
  T* m0 = mesh + (size_t)s * nx * ny * nz;
#pragma unroll
  for (int tx = 0; tx < order; ++tx)
#pragma unroll
    for (int ty = 0; ty < order; ++ty) {
      T* row = m0 + ((size_t)k.gi[0][tx] * ny + k.gi[1][ty]) * nz;
      const T a = vx * k.d[0][tx] * k.w[1][ty] + vy * k.w[0][tx] * k.d[1][ty], b = vz * k.w[0][tx] * k.w[1][ty];
#pragma unroll
      for (int tz = 0; tz < order; ++tz) {
        const T val = a * k.w[2][tz] + b * k.d[2][tz];
        if (val != T(0)) atomicAdd(row + k.gi[2][tz], val);
      }
    }
}

// PME epilogue: potential (+ field) gather from PLANAR meshes [B,C,nx,ny,nz] (C = 1 or 4), corrections, force factor.
// EIGHT LANES PER ATOM: lane l of an atom's group takes the x-plane tx = l of the stencil (order <= 6 planes; idle lanes add zeros) and
// its order^2 points on the 1 or 4 meshes; the four partial sums meet in three shuffle steps.  Measured neutral on the 100k-atom box
// (0.131 vs 0.133 ms with one thread per atom: the kernel is bound by the ~1.7 GB of cache lines the stencils pull from L2 / MALL, not by
// per-thread latency); kept because small systems get 8x the threads.
#define PG_LANES 8
#ifndef PME_XCD_SLABS
#define PME_XCD_SLABS 1
#endif
template <class T, int ORDER>
__global__ __launch_bounds__(256) void pme_gather_finish_kernel(const T* __restrict__ pos, const T* __restrict__ charges, const int* __restrict__ batch_idx,
                                         const T* __restrict__ cit, const T* __restrict__ meshes, const T* __restrict__ alpha,
                                         const T* __restrict__ volume, const T* __restrict__ qtot, int N, int nx, int ny, int nz,
                                         int with_field, T* __restrict__ energies, T* __restrict__ forces, T* __restrict__ cgrads,
                                         const double* __restrict__ add_e, const T* __restrict__ add_f, const double* __restrict__ add_cg,
                                         const int* __restrict__ atom_order, T wscale) {
  // wscale: 1, or 0 for the reference's all-zero weights of orders 5 / 6 (MI_SPLINE_REFERENCE_ORDERS): phi = field = 0, corrections only
  constexpr int order = ORDER;  // compile-time spline order: the weight evaluations and the stencil loops unroll
  // XCD-aware block -> atom-range mapping: workgroups are dispatched round-robin over the 8 XCDs (each with its own L2), so with the identity
  // mapping every XCD walks the whole system and each L2 pulls all four meshes (PMC: 0.40 GB of fetches for 0.07 GB of mesh on the headline
  // box).  Block b runs on XCD b mod 8: give XCD x the x-th eighth of the atom range, so that -- for tile-grouped (atom_order) or spatially ordered atoms
  // -- each L2 only sees its slab of the meshes.  Any atom order stays correct; PME_XCD_SLABS=0 restores the identity mapping (A/B).
  int vb = blockIdx.x;
  if (PME_XCD_SLABS && gridDim.x >= 64) {
    const int per = gridDim.x / 8, full = per * 8;  // the last gridDim.x % 8 blocks keep their place
    if (vb < full) vb = (vb & 7) * per + (vb >> 3);
  }
  const int t = vb * blockDim.x + threadIdx.x;
  const int i0 = t / PG_LANES, tx = t - i0 * PG_LANES;
  const int ic = i0 < N ? i0 : N - 1;  // surplus groups of the last block recompute the last atom and do not store
  // atom_order = {header, 3 unused, ids grouped by mesh tile} left by the tile-owned spread of the same call.  When the caller's atom order
  // is not spatially coherent (header: consecutive atoms in far-apart tiles, > N/4 of them) the atoms are taken tile by tile, so that
  // neighbouring groups of lanes read neighbouring stencils (randomly ordered 100k box: 0.59 -> 0.15 ms); a coherent order is kept
  // (it is slightly better than the arrival order inside a tile: 0.116 vs 0.130 ms).  Results go to atom i either way.
  const bool by_tile = atom_order != nullptr && 4ll * atom_order[0] > (long long)N;
  const int i = by_tile ? atom_order[4 + ic] : ic;
  const int s = batch_idx ? batch_idx[i] : 0;
  const Stencil<T> st = make_stencil(pos + 3 * (size_t)i, cit + 9 * (size_t)s, nx, ny, nz, order);
  T wz[ORDER];
  int gz[ORDER];
#pragma unroll
  for (int k = 0; k < order; ++k) { wz[k] = weight_1d(st, 2, k, order); gz[k] = wrap_idx(st.base[2] + k + st.off0[2], nz); }
  const T q = charges[i];
  const size_t plane = (size_t)nx * ny * nz;
  const int C = with_field ? 4 : 1;
  const T* m0 = meshes + (size_t)s * C * plane;
  T phi = 0, ex = 0, ey = 0, ez = 0;
  if (tx < order) {
    const T wx = weight_1d(st, 0, tx, order) * wscale;
    const int gx = wrap_idx(st.base[0] + tx + st.off0[0], nx);
#pragma unroll
    for (int ty = 0; ty < order; ++ty) {
      const T wxy = wx * weight_1d(st, 1, ty, order);
      const int gy = wrap_idx(st.base[1] + ty + st.off0[1], ny);
      const size_t row = ((size_t)gx * ny + gy) * nz;
#pragma unroll
      for (int tz = 0; tz < order; ++tz) {
        const T w = wxy * wz[tz];
        if (w > T(1e-8)) {
          const size_t g = row + gz[tz];
          phi += m0[g] * w;
          if (with_field) {
            ex += (q * m0[plane + g]) * w;
            ey += (q * m0[2 * plane + g]) * w;
            ez += (q * m0[3 * plane + g]) * w;
          }
        }
      }
    }
  }
#pragma unroll
  for (int o = PG_LANES / 2; o > 0; o >>= 1) {
    phi += __shfl_xor(phi, o, PG_LANES);
    if (with_field) { ex += __shfl_xor(ex, o, PG_LANES); ey += __shfl_xor(ey, o, PG_LANES); ez += __shfl_xor(ez, o, PG_LANES); }
  }
  if (tx != 0 || i0 >= N) return;
  // `_pme_energy_corrections[_with_charge_grad]_kernel` (pme_kernels.py:340-657)
  const T pi = T(3.14159265358979323846), two = 2;
  const T a = alpha[s], vol = volume[s], qt = qtot[s];
  // add_*: the real-space part of particle_mesh_ewald (pme.py:1975-1990 adds real + reciprocal with torch; real-space energies and
  // charge gradients arrive in float64 and are cast to the output dtype first, as `.to(dtype)` does there)
  const T er = q * phi - q * q * a / sqrt(pi) - q * pi * qt / (two * a * a * vol);
  energies[i] = add_e ? (T)add_e[i] + er : er;
  if (cgrads) { const T cr = two * phi - two * a * q / sqrt(pi) - pi * qt / (a * a * vol); cgrads[i] = add_cg ? (T)add_cg[i] + cr : cr; }
  if (with_field && forces) {  // forces = 2 * gather_vec3 (pme.py:1477)
    const T fx = two * ex, fy = two * ey, fz = two * ez;
    if (add_f) {
      forces[3 * (size_t)i] = add_f[3 * (size_t)i] + fx; forces[3 * (size_t)i + 1] = add_f[3 * (size_t)i + 1] + fy;
      forces[3 * (size_t)i + 2] = add_f[3 * (size_t)i + 2] + fz;
    } else { forces[3 * (size_t)i] = fx; forces[3 * (size_t)i + 1] = fy; forces[3 * (size_t)i + 2] = fz; }
  }
}

// ---- tile-staged gather epilogue (round 4) ----------------------------------------------------------------------------------------------------
// The kernel above reads order^3 x (1 | 4) mesh values per atom straight from L2 / MALL: 50 M scattered 8-byte loads on the headline mesh,
// latency-bound (0.11 ms) with 5 of 8 lanes busy at order 5.  The spread of the same step has already grouped the atoms by mesh tile and left
// each atom's stencil start and fractional offsets in its workspace; a stencil that starts in tile t lies inside t's box (tile + forward halo).
// So: a block per tile stages the box of one mesh channel at a time in LDS with coalesced loads (periodic wrap applied while staging), its
// atoms take their order^3 values from LDS -- one (x, y) column per lane, 25 of 32 lanes per atom at order 5, fixed shuffle tree: the sums
// do not depend on any arrival order -- and one thread per atom finishes exactly as above (corrections, x2 force, real-space parts added).
#define PGB_CHUNK 32  // atoms of the tile per pass (tiles hold ~24 atoms at liquid density; denser tiles take more passes and re-stage the boxes)
template <class T, int ORDER>
__global__ __launch_bounds__(256) void pme_gather_box_kernel(const T* __restrict__ charges, const T* __restrict__ meshes, const T* __restrict__ alpha,
                                                            const T* __restrict__ volume, const T* __restrict__ qtot, const int* __restrict__ atom_of,
                                                            const int* __restrict__ bin_start, const int4* __restrict__ lo3,
                                                            const T* __restrict__ theta_all, int N, int nx, int ny, int nz, int with_field, SpTile e,
                                                            T* __restrict__ energies, T* __restrict__ forces, T* __restrict__ cgrads,
                                                            const double* __restrict__ add_e, const T* __restrict__ add_f,
                                                            const double* __restrict__ add_cg, T wscale) {
  constexpr int order = ORDER, H = ORDER - 1;
  constexpr int GL = ORDER * ORDER <= 16 ? 16 : (ORDER * ORDER <= 32 ? 32 : 64);  // lanes per atom: the (x, y) columns, rounded up to a power of two
  __shared__ T box[(SP_T + H) * (SP_T + H) * (SP_T + H)];
  __shared__ T wl[PGB_CHUNK][3][ORDER];
  __shared__ int lo_s[PGB_CHUNK][3];
  __shared__ T res[PGB_CHUNK][4];
  __shared__ T qs[PGB_CHUNK];  // the pass's charges (and atom indices): the gather loop used to load them per atom and field channel through two dependent
  __shared__ int ai[PGB_CHUNK];  // global loads, in front of its FMAs (0.097 -> 0.087 ms on the headline mesh)
  const int nbx = nx / e.ex, nby = ny / e.ey, nbz = nz / e.ez;
  const int bxn = e.ex + H, byn = e.ey + H, bzn = e.ez + H, box_n = bxn * byn * bzn;
  int b = blockIdx.x;
  const int bz = b % nbz; b /= nbz;
  const int by = b % nby; b /= nby;
  const int bx = b % nbx;
  const int s = b / nbx;
  const int org[3] = {bx * e.ex, by * e.ey, bz * e.ez};
  const size_t plane = (size_t)nx * ny * nz;
  const int C = with_field ? 4 : 1;
  const T* m0 = meshes + (size_t)s * C * plane;
  const int beg = bin_start[blockIdx.x], end = bin_start[blockIdx.x + 1];
  const int grp = threadIdx.x / GL, gl = threadIdx.x - grp * GL, ngrp = 256 / GL;
  const int gtx = gl / order, gty = gl - gtx * order;
  const unsigned mz = 0xFFFFFFFFu / (unsigned)bzn + 1u, my = 0xFFFFFFFFu / (unsigned)byn + 1u;
  for (int c0 = beg; c0 < end; c0 += PGB_CHUNK) {
    const int nc = end - c0 < PGB_CHUNK ? end - c0 : PGB_CHUNK;
    __syncthreads();  // previous pass consumed
    // the box of channel ch + 1 is fetched into registers while channel ch is being gathered from LDS (staging latency off the critical path)
    constexpr int NPT = ((SP_T + H) * (SP_T + H) * (SP_T + H) + 255) / 256;
    T pre[NPT];
    auto fetch = [&](int ch) {
      const T* mc = m0 + (size_t)ch * plane;
#pragma unroll
      for (int u = 0; u < NPT; ++u) {
        const int k = threadIdx.x + u * 256;
        if (k < box_n) {
          // k = (px * byn + py) * bzn + pz by two multiply-high's (k < 4096, edges <= 13: exact) instead of two runtime divisions per point
          // and channel (0.087 -> 0.084 ms)
          const int pxy = (int)__umulhi((unsigned)k, mz), pz = k - pxy * bzn, px = (int)__umulhi((unsigned)pxy, my), py = pxy - px * byn;
          int gx = org[0] + px, gy = org[1] + py, gz = org[2] + pz;  // forward halo: at most one wrap
          gx -= gx >= nx ? nx : 0; gy -= gy >= ny ? ny : 0; gz -= gz >= nz ? nz : 0;
          pre[u] = mc[((size_t)gx * ny + gy) * nz + gz];
        }
      }
    };
    if (threadIdx.x < 3 * nc) {  // 1-D weights of this pass's atoms, exactly as the spread's box kernel forms them (weight_1d's expression)
      const int a = threadIdx.x / 3, d = threadIdx.x - 3 * a;
      const int i = atom_of[c0 + a];
      const int4 lo = lo3[i];
      const T theta = theta_all[(size_t)d * N + i];
      const int off0 = (int)floor(theta - (T)(order - 2) * T(0.5));
      lo_s[a][d] = (d == 0 ? lo.x : (d == 1 ? lo.y : lo.z)) - org[d];
      if (d == 0) {
        qs[a] = charges[i];
        ai[a] = i;
      }
#pragma unroll
      for (int t = 0; t < order; ++t) {
        const T u = (T)order * T(0.5) + theta - (T)(t + off0);
        wl[a][d][t] = ((u < T(0) || u >= (T)order) ? T(0) : bspline_weight(u, order)) * (d == 0 ? wscale : T(1));
      }
    }
    fetch(0);
    for (int ch = 0; ch < C; ++ch) {
      __syncthreads();  // weights ready / previous channel's box consumed
#pragma unroll
      for (int u = 0; u < NPT; ++u) { const int k = threadIdx.x + u * 256; if (k < box_n) box[k] = pre[u]; }
      if (ch + 1 < C) fetch(ch + 1);
      __syncthreads();
      for (int a = grp; a < nc; a += ngrp) {
        T part = T(0);
        if (gl < order * order) {
          const T wxy = wl[a][0][gtx] * wl[a][1][gty];
          const T* row = box + ((lo_s[a][0] + gtx) * byn + lo_s[a][1] + gty) * bzn + lo_s[a][2];
          const T q = ch ? qs[a] : T(1);  // field channels: (q * mesh) * w as in gather_vec3
#pragma unroll
          for (int tz = 0; tz < order; ++tz) {
            const T w = wxy * wl[a][2][tz];
            if (w > T(1e-8)) part += (ch ? q * row[tz] : row[tz]) * w;
          }
        }
#pragma unroll
        for (int o = GL / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, GL);
        if (gl == 0) res[a][ch] = part;
      }
    }
    __syncthreads();
    if (threadIdx.x < nc) {
      // `_pme_energy_corrections[_with_charge_grad]_kernel` (pme_kernels.py:340-657) and the real-space parts, as in pme_gather_finish_kernel
      const int i = ai[threadIdx.x];
      const T q = qs[threadIdx.x], phi = res[threadIdx.x][0];
      const T pi = T(3.14159265358979323846), two = 2;
      const T al = alpha[s], vol = volume[s], qt = qtot[s];
      const T er = q * phi - q * q * al / sqrt(pi) - q * pi * qt / (two * al * al * vol);
      energies[i] = add_e ? (T)add_e[i] + er : er;
      if (cgrads) { const T cr = two * phi - two * al * q / sqrt(pi) - pi * qt / (al * al * vol); cgrads[i] = add_cg ? (T)add_cg[i] + cr : cr; }
      if (with_field && forces) {  // forces = 2 * gather_vec3 (pme.py:1477)
        const T fx = two * res[threadIdx.x][1], fy = two * res[threadIdx.x][2], fz = two * res[threadIdx.x][3];
        if (add_f) {
          forces[3 * (size_t)i] = add_f[3 * (size_t)i] + fx; forces[3 * (size_t)i + 1] = add_f[3 * (size_t)i + 1] + fy;
          forces[3 * (size_t)i + 2] = add_f[3 * (size_t)i + 2] + fz;
        } else { forces[3 * (size_t)i] = fx; forces[3 * (size_t)i + 1] = fy; forces[3 * (size_t)i + 2] = fz; }
      }
    }
  }
}

// ---- k-space --------------------------------------------------------------------------------------------
template <class T> __device__ __forceinline__ T sinc_pi(T x) {
  if (fabs(x) < T(1e-6)) return T(1);
  const T px = T(3.14159265358979323846) * x;
  return sin(px) / px;
}
__device__ __forceinline__ int miller_of(int i, int n) { return i < (n + 1) / 2 ? i : i - n; }  // fftfreq(n, 1/n)

template <class T> __device__ __forceinline__ T green_of(T k2, T alpha, T volume, bool origin) {
  // pme_kernels.py:194-206: 2 pi exp(-k^2 / 4 a^2) / (k^2 V), 0 for k^2 < 1e-10 and at index (0,0,0)
  if (origin || k2 < T(1e-10)) return T(0);
  const T ef = exp(-(T(1) / (T(4) * alpha * alpha)) * k2) / k2;
  return T(6.283185307179586) * ef / volume;
}
template <class T> __device__ __forceinline__ T sf_sq_of(int mx, int my, int mz, int nx, int ny, int nz, int expo) {
  // pme_kernels.py:208-225: (sinc sinc sinc)^expo, clamped at 1e-10, squared.  The reference caps the exponent at
  // min(order, 4); the caller passes that for orders <= 4 and the mathematically right `order` for the
  // true order-5/6 splines of this build.
  const T sp = sinc_pi((T)mx / (T)nx) * sinc_pi((T)my / (T)ny) * sinc_pi((T)mz / (T)nz);
  T sf = sp;
  for (int t = 1; t < expo; ++t) sf = sf * sp;
  if (sf < T(1e-10)) sf = T(1e-10);
  return sf * sf;
}

template <class T>
__global__ void pme_green_sf_kernel(const T* __restrict__ k2, const T* __restrict__ alpha, const T* __restrict__ volume, int B, int nx, int ny,
                                    int nz, int order, T* __restrict__ G, T* __restrict__ sf2) {
  const int nzr = nz / 2 + 1;
  const size_t per = (size_t)nx * ny * nzr;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= per * B) return;
  const int b = (int)(g / per);
  const size_t r = g - (size_t)b * per;
  const int k = (int)(r % nzr), j = (int)((r / nzr) % ny), i = (int)(r / ((size_t)nzr * ny));
  G[g] = green_of(k2[g], alpha[b], volume[b], i == 0 && j == 0 && k == 0);
  if (b == 0) sf2[r] = sf_sq_of<T>(miller_of(i, nx), miller_of(j, ny), k, nx, ny, nz, order);
}

template <class T> struct Cplx { T re, im; };

template <class T>
__global__ void pme_convolve_kernel(const Cplx<T>* __restrict__ spec, const T* __restrict__ recip, const T* __restrict__ alpha,
                                    const T* __restrict__ volume, int B, int nx, int ny, int nz, int order, int with_field,
                                    const T* __restrict__ kvec_in, const T* __restrict__ k2_in, int k_batched, Cplx<T>* __restrict__ out) {
  const int nzr = nz / 2 + 1;
  const size_t per = (size_t)nx * ny * nzr;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= per * B) return;
  const int b = (int)(g / per);
  const size_t r = g - (size_t)b * per;
  const int k = (int)(r % nzr), j = (int)((r / nzr) % ny), i = (int)(r / ((size_t)nzr * ny));
  const int mx = miller_of(i, nx), my = miller_of(j, ny), mz = k;
  // k_c = sum_d m_d * (2 pi cell^-1)[c][d]   (k_vectors.py:270-282)
  const T* R = recip + 9 * (size_t)b;
  const T m[3] = {(T)mx, (T)my, (T)mz};
  T kv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) kv[c] = m[0] * R[3 * c] + m[1] * R[3 * c + 1] + m[2] * R[3 * c + 2];
  T k2 = kv[0] * kv[0] + kv[1] * kv[1] + kv[2] * kv[2];
  if (!(k2 > T(1e-12))) k2 = T(1e-12);
  // caller-supplied k arrays (pme_reciprocal_space(k_vectors=, k_squared=), pme.py:1386-1392): read instead of evaluated, wave-uniform tests
  const size_t kidx = (k_batched ? (size_t)b * per : 0) + r;
  if (k2_in) k2 = k2_in[kidx];
  if (kvec_in && with_field) { kv[0] = kvec_in[3 * kidx]; kv[1] = kvec_in[3 * kidx + 1]; kv[2] = kvec_in[3 * kidx + 2]; }
  const T G = green_of(k2, alpha[b], volume[b], i == 0 && j == 0 && k == 0);
  const T sf2 = sf_sq_of<T>(mx, my, mz, nx, ny, nz, order);
  const Cplx<T> v = spec[g];
  // conv = (spec / sf2) * G   (pme.py:1418-1419)
  const T cr = (v.re / sf2) * G, ci = (v.im / sf2) * G;
  const int C = with_field ? 4 : 1;
  Cplx<T>* o = out + (size_t)b * C * per + r;
  o[0] = Cplx<T>{cr, ci};
  if (with_field) {
#pragma unroll
    for (int d = 0; d < 3; ++d) o[(size_t)(d + 1) * per] = Cplx<T>{kv[d] * ci, -(kv[d] * cr)};  // (-i k_d) * conv
  }
}

// ---- adjoint of the k-space pass (round 4: fused forward under autograd) ------------------------------------------------------------
// Upstream weights arrive as meshes: A_E = spread(g_E q) for a loss on the energies and, with `nchan` = 4, A_d = spread(2 g_F,d q) for a loss
// on the explicit forces F = 2 q gather(E_d), E_d = F^H (-i k_d D) F rho.  With W_hat = A_E_hat + sum_d (i k_d) A_d_hat the whole loss is
// L = sum_k h_k Re(conj(W_hat_k) D_k rho_hat_k), D_k = G(k^2; alpha, V) / sf2_k, h_k the Hermitian weights of the half spectrum (1 on the planes
// kz = 0 and -- even nz -- kz = nz/2, else 2).  One pass over the spectra produces
//   conv_out = D W_hat                     its unscaled inverse transform is dL/d(charge mesh): the operator is self-adjoint
//   per system and block, 20 sums (double; the caller folds the blocks: no same-address atomics):
//     [0]  h Re(.) G / sf2                               -> dL/dV = -[0] / V
//     [1]  h Re(.) G k^2 / (2 alpha^3) / sf2               =  dL/dalpha
//     [2 + 3c + d]  h Re(.) dG/dk^2 2 k_c m_d / sf2       =  dL/d(2 pi cell^-1)[c][d] through k^2   (k_c = sum_d m_d recip[c][d])
//     [11 + 3c + d] h D Im(conj(A_c_hat) rho_hat) m_d      =  dL/d(2 pi cell^-1)[c][d] through the explicit k_c of the field (nchan = 4 only)
// Spectra: `spec` [B][...], `aspec` channel-major [nchan][B][...].  Reference: the Warp tape + torch autograd over pme_kernels.py:121-331 and
// pme.py:1398-1457; this is the closed form of those adjoints.
#define PME_BWD_BLOCKS 256
#define PME_BWD_SUMS 20
template <class T>
__global__ __launch_bounds__(256) void pme_convolve_bwd_kernel(const Cplx<T>* __restrict__ spec, const Cplx<T>* __restrict__ aspec, int nchan,
                                                              const T* __restrict__ recip, const T* __restrict__ alpha,
                                                              const T* __restrict__ volume, int B, int nx, int ny, int nz, int order,
                                                              Cplx<T>* __restrict__ conv_out, double* __restrict__ partial) {
  const int b = blockIdx.y;
  const int nzr = nz / 2 + 1;
  const size_t per = (size_t)nx * ny * nzr;
  const T* R = recip + 9 * (size_t)b;
  const T al = alpha[b], vol = volume[b];
  double acc[PME_BWD_SUMS];
#pragma unroll
  for (int q = 0; q < PME_BWD_SUMS; ++q) acc[q] = 0.0;
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < per; r += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(r % nzr), j = (int)((r / nzr) % ny), i = (int)(r / ((size_t)nzr * ny));
    const int mx = miller_of(i, nx), my = miller_of(j, ny), mz = k;
    const T m[3] = {(T)mx, (T)my, (T)mz};
    T kv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) kv[c] = m[0] * R[3 * c] + m[1] * R[3 * c + 1] + m[2] * R[3 * c + 2];
    const T k2 = kv[0] * kv[0] + kv[1] * kv[1] + kv[2] * kv[2];
    // clamped / masked in the forward pass (origin, k^2 <= 1e-12, G = 0 below 1e-10): no contribution and no dependence on the parameters
    const bool live = !(i == 0 && j == 0 && k == 0) && (k2 > T(1e-12)) && !(k2 < T(1e-10));
    const T G = live ? green_of(k2, al, vol, false) : T(0);
    const T sf2 = sf_sq_of<T>(mx, my, mz, nx, ny, nz, order);
    const Cplx<T> v = spec[(size_t)b * per + r];
    const Cplx<T> ae = aspec[(size_t)b * per + r];
    double wre = (double)ae.re, wim = (double)ae.im;  // W_hat
    double imd[3] = {0.0, 0.0, 0.0};                  // Im(conj(A_d_hat) rho_hat)
    if (nchan == 4) {
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const Cplx<T> ad = aspec[((size_t)(d + 1) * B + b) * per + r];
        wre -= (double)kv[d] * (double)ad.im;  // (i k_d)(re + i im) = -k_d im + i k_d re
        wim += (double)kv[d] * (double)ad.re;
        imd[d] = (double)ad.re * (double)v.im - (double)ad.im * (double)v.re;
      }
    }
    const double dk = (double)G / (double)sf2;
    if (conv_out) conv_out[(size_t)b * per + r] = Cplx<T>{(T)(dk * wre), (T)(dk * wim)};
    if (!live) continue;
    const double h = (k == 0 || (2 * k == nz)) ? 1.0 : 2.0;
    const double w = h * (wre * (double)v.re + wim * (double)v.im) * dk;  // h Re(conj(W) rho) G / sf2
    acc[0] += w;
    acc[1] += w * (double)k2 / (2.0 * (double)al * (double)al * (double)al);
    const double dg = w * (-1.0 / (4.0 * (double)al * (double)al) - 1.0 / (double)k2) * 2.0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        acc[2 + 3 * c + d] += dg * (double)kv[c] * (double)m[d];
        acc[11 + 3 * c + d] += h * dk * imd[c] * (double)m[d];
      }
  }
  __shared__ double part[4][PME_BWD_SUMS];
  const int lane = threadIdx.x & (MI_WAVE - 1), wave = threadIdx.x / MI_WAVE;
#pragma unroll
  for (int q = 0; q < PME_BWD_SUMS; ++q) { const double t = wave_sum(acc[q]); if (lane == 0) part[wave][q] = t; }
  __syncthreads();
  if (threadIdx.x < PME_BWD_SUMS)
    partial[((size_t)b * gridDim.x + blockIdx.x) * PME_BWD_SUMS + threadIdx.x] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

// ---- virial of the mesh sum (forward only) ---------------------------------------------------------------------------------------------
// The mesh energy is E = sum_m h_m G(k_m) |rho_hat_m|^2 / sf2_m over the half spectrum (h as above).  Under x -> (I + eps) x the spread and
// the gather see fractional coordinates only, so rho_hat and sf2 do not move; k_m = 2 pi cell^-1 m follows the cell and V grows by det(I+eps):
//   W[a][b] = -dE/deps[a][b] = sum_m E_m (delta_ab - 2 (1/k^2 + 1/(4 alpha^2)) k_a k_b)
// Six sums {xx, yy, zz, xy, xz, yz}, laid out like mi_pme_convolve_bwd's: partial[b][block][6], every entry written, the caller folds.
// k from `recip` (as pme_convolve_kernel evaluates it) or from the caller's arrays (kvec_in / k2_in, shared or per system).
#define PME_VIR_BLOCKS 256
template <class T>
__global__ __launch_bounds__(256) void pme_virial_kernel(const Cplx<T>* __restrict__ spec, const T* __restrict__ recip, const T* __restrict__ alpha,
                                                         const T* __restrict__ volume, int nx, int ny, int nz, int order,
                                                         const T* __restrict__ kvec_in, const T* __restrict__ k2_in, int k_batched,
                                                         const T* __restrict__ qtot, double* __restrict__ partial) {
  const int b = blockIdx.y;
  const int nzr = nz / 2 + 1;
  const size_t per = (size_t)nx * ny * nzr;
  const T* R = recip + 9 * (size_t)b;
  const T al = alpha[b], vol = volume[b];
  const double c4 = 1.0 / (4.0 * (double)al * (double)al);
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < per; r += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(r % nzr), j = (int)((r / nzr) % ny), i = (int)(r / ((size_t)nzr * ny));
    const int mx = miller_of(i, nx), my = miller_of(j, ny), mz = k;
    const T m[3] = {(T)mx, (T)my, (T)mz};
    T kv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) kv[c] = m[0] * R[3 * c] + m[1] * R[3 * c + 1] + m[2] * R[3 * c + 2];
    T k2 = kv[0] * kv[0] + kv[1] * kv[1] + kv[2] * kv[2];
    if (!(k2 > T(1e-12))) k2 = T(1e-12);
    const size_t kidx = (k_batched ? (size_t)b * per : 0) + r;
    if (k2_in) k2 = k2_in[kidx];
    if (kvec_in) { kv[0] = kvec_in[3 * kidx]; kv[1] = kvec_in[3 * kidx + 1]; kv[2] = kvec_in[3 * kidx + 2]; }
    const T G = green_of(k2, al, vol, i == 0 && j == 0 && k == 0);
    if (G == T(0)) continue;  // origin and masked modes: no energy, no virial
    const T sf2 = sf_sq_of<T>(mx, my, mz, nx, ny, nz, order);
    const Cplx<T> v = spec[(size_t)b * per + r];
    const double h = (k == 0 || (2 * k == nz)) ? 1.0 : 2.0;
    const double e = h * ((double)v.re * (double)v.re + (double)v.im * (double)v.im) * ((double)G / (double)sf2);
    const double c = -2.0 * e * (1.0 / (double)k2 + c4);
    const double kx = kv[0], ky = kv[1], kz = kv[2];
    acc[0] += e + c * kx * kx; acc[1] += e + c * ky * ky; acc[2] += e + c * kz * kz;
    acc[3] += c * kx * ky; acc[4] += c * kx * kz; acc[5] += c * ky * kz;
  }
  __shared__ double part[4][6];
  const int lane = threadIdx.x & (MI_WAVE - 1), wave = threadIdx.x / MI_WAVE;
#pragma unroll
  for (int q = 0; q < 6; ++q) { const double t = wave_sum(acc[q]); if (lane == 0) part[wave][q] = t; }
  __syncthreads();
  if (threadIdx.x < 6) {
    double v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    // background term -pi Q^2 / (2 alpha^2 V): it scales as 1/V, so it adds E_bg to the diagonal (block 0 of each system)
    if (qtot && blockIdx.x == 0 && threadIdx.x < 3) { const double Q = (double)qtot[b]; v -= M_PI * Q * Q / (2.0 * (double)al * (double)al * (double)vol); }
    partial[((size_t)b * gridDim.x + blockIdx.x) * 6 + threadIdx.x] = v;
  }
}

template <class T>
__global__ void pme_corrections_kernel(const T* __restrict__ raw, const T* __restrict__ q, const int* __restrict__ batch_idx,
                                       const T* __restrict__ vol, const T* __restrict__ alpha, const T* __restrict__ qtot, int N,
                                       T* __restrict__ E, T* __restrict__ dEdq) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int s = batch_idx ? batch_idx[i] : 0;
  const T pi = T(3.14159265358979323846), two = 2;
  const T c = q[i], a = alpha[s];
  E[i] = c * raw[i] - c * c * a / sqrt(pi) - c * pi * qtot[s] / (two * a * a * vol[s]);
  if (dEdq) dEdq[i] = two * raw[i] - two * a * c / sqrt(pi) - pi * qtot[s] / (a * a * vol[s]);
}

template <class T>
__global__ void segment_sum_kernel(const T* __restrict__ v, const int* __restrict__ batch_idx, int N, T* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const bool in = i < N;
  const int s = in ? (batch_idx ? batch_idx[i] : 0) : -1;
  const int s0 = __shfl(s, 0, MI_WAVE);
  T x = in ? v[i] : T(0);
  if (__all(!in || s == s0)) {
    x = wave_sum(x);
    if (lane == 0 && s0 >= 0) atomicAdd(&out[s0], x);
  } else if (in) {
    atomicAdd(&out[s], x);
  }
}

template <class T>
int spread_tiled(const T* pos, const T* values, const int* batch_idx, const T* cit, int N, int B, int nx, int ny, int nz, int order,
                        int batched, T* mesh, char* ws, hipStream_t st) {
  const SpLayout L = sp_layout(N, B, nx, ny, nz);
  const SpTile e = sp_tile(nx, ny, nz);
  int* keys_in = reinterpret_cast<int*>(ws + L.keys_in);
  int* order_hdr = reinterpret_cast<int*>(ws + L.vals_out);
  int* vals_out = order_hdr + 4;
  int* bin_start = reinterpret_cast<int*>(ws + L.bin_start);
  int4* lo3 = reinterpret_cast<int4*>(ws + L.lo3);
  T* theta = reinterpret_cast<T*>(ws + L.theta);
  const BsScratch bins = bs_carve(reinterpret_cast<int*>(ws + L.bins), L.nbins + 1);  // + 1: the end sentinel bin_start[nbins] = N
  MI_HIP_CHECK(bs_clear(bins, st));
  int* incoherent = bins.fill + L.nbins;  // the sentinel's fill slot: cleared with the counters, touched by no key
  spread_key_kernel<T><<<mi_blocks(N, 256), 256, 0, st>>>(pos, batch_idx, cit, N, nx, ny, nz, order, e, keys_in, bins.count, lo3, theta, incoherent);
  MI_LAUNCH_CHECK();
  // order inside a tile's atom list is arrival order: the tile kernel adds the contributions with LDS atomics, whose order is
  // not fixed either (fp64/fp32 sums of <= a few hundred terms per mesh point; parity tests hold at 1e-10)
  MI_HIP_CHECK(bs_sort(bins, keys_in, N, nullptr, vals_out, bin_start, st));
  // two-phase spread: per-tile LDS boxes, then every mesh point adds the boxes that cover it
  T* boxes = reinterpret_cast<T*>(ws + L.boxes);
  switch (order) {
#define MI_SPB(O_) case O_: spread_box_kernel<T, O_><<<(int)L.nbins, 256, 0, st>>>(values, vals_out, bin_start, lo3, theta, N, nx, ny, nz, batched, e, boxes, order_hdr, incoherent); break
    MI_SPB(1); MI_SPB(2); MI_SPB(3); MI_SPB(4); MI_SPB(5);
    default: spread_box_kernel<T, 6><<<(int)L.nbins, 256, 0, st>>>(values, vals_out, bin_start, lo3, theta, N, nx, ny, nz, batched, e, boxes, order_hdr, incoherent); break;
#undef MI_SPB
  }
  MI_LAUNCH_CHECK();
  spread_box_reduce_kernel<T><<<dim3((unsigned)mi_blocks((long long)ny * nz, 256), (unsigned)nx, (unsigned)B), 256, 0, st>>>(boxes, nx, ny, nz, B, order, e, mesh);
  MI_LAUNCH_CHECK();
  return MI_OK;
}


// ---- fused mesh solve: the whole k-space step of a power-of-two mesh in four kernels (bodies: fft_lds.h) ----------------------------------
#define MI_LDS_MAX 163840
template <class T> __global__ void pme_solve_tables_kernel(void* base, mifft::Geom g) { mifft::tables_body<T>(base, g, threadIdx.x, blockDim.x); }
// GEN: the mixed-radix form of the bodies (meshes with factors 3 and 5); false = power-of-two meshes, shift / mask index arithmetic only
template <class T, bool GEN, bool NAT = false>
__global__ __launch_bounds__(1024) void pme_solve_fwd_kernel(const T* __restrict__ mesh, mifft::Cx<T>* __restrict__ spec, mifft::Geom g, mifft::Tables<T> tb) {
  extern __shared__ __align__(16) unsigned char solve_smem[];
  const size_t plane = blockIdx.x;  // (system, x)
  mifft::fwd_plane_body<T, GEN, NAT>(mesh + plane * g.ny * g.nz, spec + plane * g.ny * g.P, (mifft::Cx<T>*)solve_smem, g, tb, threadIdx.x, blockDim.x);
}
template <class T, bool GEN, bool PLAIN = false>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2))) void pme_solve_fwd_cols_kernel(mifft::Cx<T>* __restrict__ spec, mifft::Geom g, mifft::Tables<T> tb, const T* __restrict__ recip,
                                                                const T* __restrict__ alpha, const T* __restrict__ volume, int sf_expo,
                                                                mifft::Cx<T>* __restrict__ spec_nat /*NULL or [B][nx][ny][P]*/) {
  extern __shared__ __align__(16) unsigned char solve_smem[];
  const int b = blockIdx.y;
  const size_t per = (size_t)g.nx * g.ny * g.P;
  if (PLAIN)  // a transform on its own (mi_fft_lds_r2c): recip / alpha / volume are null and never read
    mifft::fwd_cols_body<T, GEN, true>(spec + b * per, (mifft::Cx<T>*)solve_smem, g, tb, nullptr, T(1), T(1), 1, blockIdx.x * MI_SOLVE_COLS, threadIdx.x, blockDim.x,
                                       spec_nat + b * per);
  else
    mifft::fwd_cols_body<T, GEN>(spec + b * per, (mifft::Cx<T>*)solve_smem, g, tb, recip + 9 * b, alpha[b], volume[b], sf_expo, blockIdx.x * MI_SOLVE_COLS,
                                 threadIdx.x, blockDim.x, spec_nat ? spec_nat + b * per : nullptr);
}
// grid.x = 8-padded column tiles x channels.  The channels of one tile read the same conv lines: consecutive block ids go round the 8 XCDs,
// so the id is unpacked as (xcd, channel, tile group) -- the n_channels blocks of a tile follow each other on ONE XCD and share its L2.
template <class T, bool GEN, bool PLAIN = false>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2))) void pme_solve_inv_cols_kernel(const mifft::Cx<T>* __restrict__ conv_spec, mifft::Cx<T>* __restrict__ conv, mifft::Geom g,
                                                                mifft::Tables<T> tb, const T* __restrict__ recip, int n_channels, int col_blocks) {
  extern __shared__ __align__(16) unsigned char solve_smem[];
  const int b = blockIdx.y;
  const int xcd = blockIdx.x & 7, i = blockIdx.x >> 3;
  const int ch = i % n_channels, tile = (i / n_channels) * 8 + xcd;
  if (tile >= col_blocks) return;
  const size_t per = (size_t)g.nx * g.ny * g.P;
  if (PLAIN)  // a transform on its own (mi_fft_lds_c2r): conv_spec is a half spectrum in natural order, one channel, recip is null
    mifft::inv_cols_body<T, GEN, true>(conv_spec + b * per, conv + (size_t)b * per, (mifft::Cx<T>*)solve_smem, g, tb, nullptr, 0, tile * MI_SOLVE_COLS, threadIdx.x,
                                       blockDim.x);
  else
    mifft::inv_cols_body<T, GEN>(conv_spec + b * per, conv + ((size_t)b * n_channels + ch) * per, (mifft::Cx<T>*)solve_smem, g, tb, recip + 9 * b, ch,
                                 tile * MI_SOLVE_COLS, threadIdx.x, blockDim.x);
}
// persistent: one block per CU walks its planes, so that the stores of one plane are still draining while the loads of the next are issued
// (with one 133 KB plane per CU in LDS nothing else overlaps the two)
template <class T, bool GEN, bool NAT = false>
__global__ __launch_bounds__(1024) void pme_solve_inv_kernel(const mifft::Cx<T>* __restrict__ conv, T* __restrict__ real, mifft::Geom g, mifft::Tables<T> tb,
                                                             int n_planes) {
  extern __shared__ __align__(16) unsigned char solve_smem[];
  for (size_t plane = blockIdx.x; plane < (size_t)n_planes; plane += gridDim.x) {  // (system, channel, x)
    mifft::inv_plane_body<T, GEN, NAT>(conv + plane * g.ny * g.P, real + plane * g.ny * g.nz, (mifft::Cx<T>*)solve_smem, g, tb, threadIdx.x, blockDim.x);
    __syncthreads();
  }
}
// per-device facts (a process may drive several GPUs: HIP function attributes and CU counts are per device -- ADVICE r4): indexed by the
// current device, published with release / acquire so two host threads cannot see a half-written entry
#define MI_SOLVE_MAX_DEVICES 64
static int solve_device() {
  int dev = 0;
  return (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < MI_SOLVE_MAX_DEVICES) ? dev : -1;
}
static int solve_cus() {
  static std::atomic<int> cus[MI_SOLVE_MAX_DEVICES];
  const int dev = solve_device();
  if (dev < 0) return 256;
  int n = cus[dev].load(std::memory_order_acquire);
  if (!n) {
    int v = 0;
    n = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
    cus[dev].store(n, std::memory_order_release);
  }
  return n;
}
template <class T> static bool solve_fits(const mifft::Geom& g) {
  return mifft::plane_lds_bytes<T>(g) <= MI_LDS_MAX && mifft::fwd_cols_lds_bytes<T>(g) <= MI_LDS_MAX;
}
static int solve_plane_threads(const mifft::Geom& g) {
  const long long items = (long long)g.ny * g.M / 8;  // radix-8 butterflies of one row stage
  return items >= 1024 ? 1024 : items >= 512 ? 512 : 256;
}
template <class T, bool GEN>
static int solve_launch_as(const void* mesh, const void* recip_cell, const void* alpha, const void* volume, const mifft::Geom& g, int expo, int nch,
                        void* spec, void* conv, void* tab, bool tab_ready, void* real_out, void* spec_nat, int pt, int col_blocks, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t pl = mifft::plane_lds_bytes<T>(g), fl = mifft::fwd_cols_lds_bytes<T>(g), il = mifft::inv_cols_lds_bytes<T>(g);
  // more than 64 KB of dynamic LDS has to be asked for once per kernel AND device (setting it again is harmless: a race between two
  // threads costs a repeated call, never a launch without the opt-in)
  static std::atomic<bool> raised_on[MI_SOLVE_MAX_DEVICES];  // (one per instantiation of this function)
  const int dev_ix = solve_device();
  if (dev_ix < 0 || !raised_on[dev_ix].load(std::memory_order_acquire)) {
    MI_HIP_CHECK(hipFuncSetAttribute((const void*)pme_solve_fwd_kernel<T, GEN>, hipFuncAttributeMaxDynamicSharedMemorySize, MI_LDS_MAX));
    MI_HIP_CHECK(hipFuncSetAttribute((const void*)pme_solve_fwd_cols_kernel<T, GEN>, hipFuncAttributeMaxDynamicSharedMemorySize, MI_LDS_MAX));
    MI_HIP_CHECK(hipFuncSetAttribute((const void*)pme_solve_inv_cols_kernel<T, GEN>, hipFuncAttributeMaxDynamicSharedMemorySize, MI_LDS_MAX));
    MI_HIP_CHECK(hipFuncSetAttribute((const void*)pme_solve_inv_kernel<T, GEN>, hipFuncAttributeMaxDynamicSharedMemorySize, MI_LDS_MAX));
    if (dev_ix >= 0) raised_on[dev_ix].store(true, std::memory_order_release);
  }
  // unit roots / sinc / Miller index per FFT slot: a few KB, recomputed by one small launch per call into the caller's scratch -- the
  // library keeps NO device memory of its own here (a per-shape cache allocated with hipMalloc was tried first) --
  // unless the caller hands in a block it filled once with mi_fft_lds_tables (round 6: the Python host keeps one per mesh shape)
  if (!tab_ready) pme_solve_tables_kernel<T><<<1, 256, 0, st>>>(tab, g);
  const mifft::Tables<T> tb = mifft::tables_at<T>(tab, g);
  mi_timing_begin("pme_solve_fwd", stream);
  pme_solve_fwd_kernel<T, GEN><<<g.B * g.nx, pt, pl, st>>>((const T*)mesh, (mifft::Cx<T>*)spec, g, tb);
  mi_timing_end(stream);
  mi_timing_begin("pme_solve_cols", stream);
  pme_solve_fwd_cols_kernel<T, GEN><<<dim3(col_blocks, g.B), 128, fl, st>>>((mifft::Cx<T>*)spec, g, tb, (const T*)recip_cell, (const T*)alpha, (const T*)volume, expo,
                                                                      (mifft::Cx<T>*)spec_nat);
  pme_solve_inv_cols_kernel<T, GEN><<<dim3((col_blocks + 7) / 8 * 8 * nch, g.B), 128, il, st>>>((const mifft::Cx<T>*)spec, (mifft::Cx<T>*)conv, g, tb,
                                                                                          (const T*)recip_cell, nch, col_blocks);
  mi_timing_end(stream);
  mi_timing_begin("pme_solve_inv", stream);
  const int n_planes = g.B * nch * g.nx;
  // persistent only where one plane fills the CU's LDS; small planes run several blocks per CU and overlap by themselves
  const int inv_grid = (2 * pl <= MI_LDS_MAX || n_planes < solve_cus()) ? n_planes : solve_cus();
  pme_solve_inv_kernel<T, GEN><<<inv_grid, pt, pl, st>>>((const mifft::Cx<T>*)conv, (T*)real_out, g, tb, n_planes);
  mi_timing_end(stream);
  return MI_OK;
}
// The same kernels as transforms on their own (round 6): real [B][nx][ny][nz] <-> half spectrum [B][nx][ny][nz/2+1] in natural order, unscaled
// both ways -- the layout and scaling of mi_fft_plan_exec, so that the autograd node's backward (and every other caller of a plan) runs
// without hipFFT wherever the mesh solve itself is supported.  `work` = one half spectrum in slot order, `tab` = the per-shape tables.
template <class T, bool GEN>
static int fft_lds_launch_as(bool inverse, const void* in, void* out, const mifft::Geom& g, void* work, void* tab, bool tab_ready, int pt, int col_blocks, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t pl = mifft::plane_lds_bytes_nat<T>(g), fl = mifft::fwd_cols_lds_bytes<T>(g), il = mifft::inv_cols_lds_bytes<T>(g);
  static std::atomic<bool> raised_on[MI_SOLVE_MAX_DEVICES];
  const int dev_ix = solve_device();
  if (dev_ix < 0 || !raised_on[dev_ix].load(std::memory_order_acquire)) {
    MI_HIP_CHECK(hipFuncSetAttribute((const void*)pme_solve_fwd_kernel<T, GEN, true>, hipFuncAttributeMaxDynamicSharedMemorySize, MI_LDS_MAX));
    MI_HIP_CHECK(hipFuncSetAttribute((const void*)pme_solve_fwd_cols_kernel<T, GEN, true>, hipFuncAttributeMaxDynamicSharedMemorySize, MI_LDS_MAX));
    MI_HIP_CHECK(hipFuncSetAttribute((const void*)pme_solve_inv_cols_kernel<T, GEN, true>, hipFuncAttributeMaxDynamicSharedMemorySize, MI_LDS_MAX));
    MI_HIP_CHECK(hipFuncSetAttribute((const void*)pme_solve_inv_kernel<T, GEN, true>, hipFuncAttributeMaxDynamicSharedMemorySize, MI_LDS_MAX));
    if (dev_ix >= 0) raised_on[dev_ix].store(true, std::memory_order_release);
  }
  if (!tab_ready) pme_solve_tables_kernel<T><<<1, 256, 0, st>>>(tab, g);
  const mifft::Tables<T> tb = mifft::tables_at<T>(tab, g);
  if (!inverse) {
    mi_timing_begin("fft_lds_r2c", stream);
    pme_solve_fwd_kernel<T, GEN, true><<<g.B * g.nx, pt, pl, st>>>((const T*)in, (mifft::Cx<T>*)work, g, tb);
    pme_solve_fwd_cols_kernel<T, GEN, true><<<dim3(col_blocks, g.B), 128, fl, st>>>((mifft::Cx<T>*)work, g, tb, nullptr, nullptr, nullptr, 1, (mifft::Cx<T>*)out);
    mi_timing_end(stream);
  } else {
    mi_timing_begin("fft_lds_c2r", stream);
    pme_solve_inv_cols_kernel<T, GEN, true><<<dim3((col_blocks + 7) / 8 * 8, g.B), 128, il, st>>>((const mifft::Cx<T>*)in, (mifft::Cx<T>*)work, g, tb, nullptr, 1, col_blocks);
    const int n_planes = g.B * g.nx;
    const int inv_grid = (2 * pl <= MI_LDS_MAX || n_planes < solve_cus()) ? n_planes : solve_cus();
    pme_solve_inv_kernel<T, GEN, true><<<inv_grid, pt, pl, st>>>((const mifft::Cx<T>*)work, (T*)out, g, tb, n_planes);
    mi_timing_end(stream);
  }
  return MI_OK;
}
template <class T>
static int solve_launch(const void* mesh, const void* recip_cell, const void* alpha, const void* volume, const mifft::Geom& g, int expo, int nch,
                        void* spec, void* conv, void* tab, bool tab_ready, void* real_out, void* spec_nat, int pt, int col_blocks, void* stream) {
  // power-of-two meshes run the kernels compiled without the mixed-radix paths (the code of rounds 4 - 5); everything else the general ones
  if (g.p2) return solve_launch_as<T, false>(mesh, recip_cell, alpha, volume, g, expo, nch, spec, conv, tab, tab_ready, real_out, spec_nat, pt, col_blocks, stream);
  return solve_launch_as<T, true>(mesh, recip_cell, alpha, volume, g, expo, nch, spec, conv, tab, tab_ready, real_out, spec_nat, pt, col_blocks, stream);
}
}  // namespace

#define MI_DISPATCH_T(dtype, CALL)                     \
  do {                                                 \
    if ((dtype) == MI_F32) { using T_ = float; CALL; } \
    else { using T_ = double; CALL; }                  \
  } while (0)

// spline order as a compile-time constant O_ (1..6; the callers have validated the range)
#define MI_DISPATCH_ORDER(order, CALL)                   \
  do {                                                   \
    switch (order) {                                     \
      case 1: { constexpr int O_ = 1; CALL; } break;     \
      case 2: { constexpr int O_ = 2; CALL; } break;     \
      case 3: { constexpr int O_ = 3; CALL; } break;     \
      case 4: { constexpr int O_ = 4; CALL; } break;     \
      case 5: { constexpr int O_ = 5; CALL; } break;     \
      default: { constexpr int O_ = 6; CALL; } break;    \
    }                                                    \
  } while (0)

namespace {
// multi-channel tile spread: key + counting sort ONCE, then box + reduce per block of channels (mesh [B, C, nx, ny, nz])
template <class T>
int spread_channels_tiled(const T* pos, const T* values, const int* batch_idx, const T* cit, int N, int B, int C, int nx, int ny, int nz, int order,
                          int batched, T* mesh, char* ws, hipStream_t st) {
  const SpcPlan plan = spc_plan(C, order, sizeof(T));
  const SpLayout L = sp_layout(N, B, nx, ny, nz, order, sizeof(T), plan.cb);
  const SpTile e = sp_tile(nx, ny, nz);
  int* keys_in = reinterpret_cast<int*>(ws + L.keys_in);
  int* vals_out = reinterpret_cast<int*>(ws + L.vals_out) + 4;
  int* bin_start = reinterpret_cast<int*>(ws + L.bin_start);
  int4* lo3 = reinterpret_cast<int4*>(ws + L.lo3);
  T* theta = reinterpret_cast<T*>(ws + L.theta);
  const BsScratch bins = bs_carve(reinterpret_cast<int*>(ws + L.bins), L.nbins + 1);
  MI_HIP_CHECK(bs_clear(bins, st));
  int* incoherent = bins.fill + L.nbins;
  spread_key_kernel<T><<<mi_blocks(N, 256), 256, 0, st>>>(pos, batch_idx, cit, N, nx, ny, nz, order, e, keys_in, bins.count, lo3, theta, incoherent);
  MI_LAUNCH_CHECK();
  MI_HIP_CHECK(bs_sort(bins, keys_in, N, nullptr, vals_out, bin_start, st));
  T* boxes = reinterpret_cast<T*>(ws + L.boxes);
  for (int c0 = 0; c0 < C; c0 += plan.cb) {
    const int cb = C - c0 < plan.cb ? C - c0 : plan.cb;
    MI_DISPATCH_ORDER(order, (spread_box_channels_kernel<T, O_><<<(int)L.nbins, 256, 0, st>>>(values, C, c0, cb, vals_out, bin_start, lo3, theta, N, nx, ny,
                                                                                             nz, batched, e, boxes)));
    MI_LAUNCH_CHECK();
    spread_box_reduce_channels_kernel<T><<<dim3((unsigned)mi_blocks((long long)ny * nz, 256), (unsigned)nx, (unsigned)(B * cb)), 256, 0, st>>>(
        boxes, nx, ny, nz, C, c0, cb, order, e, mesh);
    MI_LAUNCH_CHECK();
  }
  return MI_OK;
}
}  // namespace

// `order` arguments of the C ABI: low byte = spline order; MI_SPLINE_REFERENCE_ORDERS + order >= 5 selects the reference's evaluation of
// those orders -- identically ZERO weights (spline.py:150-193 implements orders 1-4 only) and the structure-factor exponent capped at 4
// (pme_kernels.py:213-225).  Without the flag orders 5 and 6 are the true cardinal B-splines.
struct OrderArg { int order; bool ref_zero; int sf_exponent; };
static inline OrderArg decode_order(int arg) {
  OrderArg o;
  o.order = arg & 0xff;
  const bool ref = (arg & MI_SPLINE_REFERENCE_ORDERS) != 0;
  o.ref_zero = ref && o.order >= 5;
  o.sf_exponent = ref && o.order > 4 ? 4 : o.order;
  return o;
}
static inline size_t dtype_bytes(int dtype) { return dtype == MI_F32 ? 4 : 8; }

extern "C" {

int mi_cell_geometry(const void* cell, int n_systems, int dtype, void* cell_inv_t, void* reciprocal_cell, void* volume, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_systems >= 1 && cell && cell_inv_t && reciprocal_cell && volume, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  MI_DISPATCH_T(dtype, (cell_geometry_kernel<T_><<<mi_blocks(n_systems, 64), 64, 0, st>>>((const T_*)cell, n_systems, (T_*)cell_inv_t,
                                                                                         (T_*)reciprocal_cell, (T_*)volume)));
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_pme_prepare(const void* cell, const void* charges, const int32_t* batch_idx, int n_atoms, int n_systems, int dtype, void* cell_inv_t,
                   void* reciprocal_cell, void* volume, void* total_charge, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_systems >= 1 && cell && cell_inv_t && reciprocal_cell && volume && total_charge, "null pointer");
  MI_REQUIRE(n_atoms == 0 || charges, "charges");
  hipStream_t st = (hipStream_t)stream;
  MI_HIP_CHECK(hipMemsetAsync(total_charge, 0, (dtype == MI_F32 ? 4 : 8) * (size_t)n_systems, st));
  const int threads = n_atoms > n_systems ? n_atoms : n_systems;
  int prep_blocks = mi_blocks(threads, 256);
  if (prep_blocks > 128 && n_systems <= 128 * 256) prep_blocks = 128;  // (every system still gets its geometry thread: t < B covered by 128 x 256 threads)
  MI_DISPATCH_T(dtype, (pme_prepare_kernel<T_><<<prep_blocks, 256, 0, st>>>((const T_*)cell, (const T_*)charges, batch_idx, n_atoms, n_systems,
                                                                                         (T_*)cell_inv_t, (T_*)reciprocal_cell, (T_*)volume,
                                                                                         (T_*)total_charge)));
  MI_LAUNCH_CHECK();
  return MI_OK;
}

/* 1 when mi_spline_spread runs tile-owned for this mesh / order (every mesh point is then WRITTEN: the mesh needs no zero-fill) */
int mi_spline_spread_is_tiled(int n_systems, int nx, int ny, int nz, int order) {
  if (decode_order(order).ref_zero) return 0;  // reference-mode orders 5 / 6: the mesh is just zero-filled, no tile list
  order &= 0xff;
  return (nx > 0 && ny > 0 && nz > 0 && n_systems >= 1 && order >= 1 && order <= MI_MAX_ORDER && sp_tiled_ok(nx, ny, nz, n_systems, order)) ? 1 : 0;
}

/* Host policy, measured on MI355X (profiles/r04_ab_spread_path.log): the tile pipeline (5 launches, every mesh point written once) beats the
 * atomic kernel + per-atom gather (zero-fill + 1 launch) from about 12k atoms on, provided the mesh has enough tiles to occupy the CUs. */
int mi_spline_spread_prefers_tiles(int n_atoms, int n_systems, int nx, int ny, int nz, int order) {
  if (!mi_spline_spread_is_tiled(n_systems, nx, ny, nz, order)) return 0;
  const SpTile e = sp_tile(nx, ny, nz);
  const long long tiles = (long long)n_systems * (nx / e.ex) * (ny / e.ey) * (nz / e.ez);
  return (n_atoms >= MI_SPREAD_TILE_MIN_ATOMS && tiles >= MI_SPREAD_TILE_MIN_TILES) ? 1 : 0;
}

long long mi_spline_spread_order_offset(int n_atoms, int n_systems, int nx, int ny, int nz, int order) {
  if (decode_order(order).ref_zero) return -1;
  order &= 0xff;
  if (n_atoms <= 0 || n_systems < 1 || nx <= 0 || ny <= 0 || nz <= 0 || order < 1 || order > MI_MAX_ORDER) return -1;
  if (!sp_tiled_ok(nx, ny, nz, n_systems, order)) return -1;  // the atomic kernel does not sort
  return (long long)sp_layout(n_atoms, n_systems, nx, ny, nz).vals_out;
}

size_t mi_spline_spread_workspace_bytes(int n_atoms, int n_systems, int nx, int ny, int nz) {
  if (n_atoms < 0 || n_systems < 1 || nx <= 0 || ny <= 0 || nz <= 0) return 0;
  if (!sp_tiled_ok(nx, ny, nz, n_systems, 0)) return 256;  // the atomic kernel needs no scratch
  return sp_layout(n_atoms, n_systems, nx, ny, nz).total;
}

size_t mi_spline_spread_workspace_bytes_for(int n_atoms, int n_systems, int nx, int ny, int nz, int order, int dtype) {
  if (n_atoms < 0 || n_systems < 1 || nx <= 0 || ny <= 0 || nz <= 0 || (dtype != MI_F32 && dtype != MI_F64)) return 0;
  const OrderArg oa = decode_order(order);
  if (oa.order < 1 || oa.order > MI_MAX_ORDER) return 0;
  if (oa.ref_zero || !sp_tiled_ok(nx, ny, nz, n_systems, oa.order)) return 256;
  return sp_layout(n_atoms, n_systems, nx, ny, nz, oa.order, dtype_bytes(dtype)).total;
}

int mi_spline_spread(const void* positions, const void* values, const int32_t* batch_idx, const void* cell_inv_t, int n_atoms, int n_systems,
                     int nx, int ny, int nz, int order, int batched, int dtype, void* mesh, void* workspace, size_t workspace_bytes,
                     void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  const OrderArg oa = decode_order(order);
  order = oa.order;
  MI_REQUIRE(order >= 1 && order <= MI_MAX_ORDER, "spline order must be 1..6");
  MI_REQUIRE(nx > 0 && ny > 0 && nz > 0 && n_systems >= 1, "mesh dimensions");
  if (n_atoms <= 0) return MI_OK;
  MI_REQUIRE(positions && values && cell_inv_t && mesh, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (oa.ref_zero) {  // all weights are zero: nothing is spread
    MI_HIP_CHECK(hipMemsetAsync(mesh, 0, (size_t)n_systems * nx * ny * nz * dtype_bytes(dtype), st));
    return MI_OK;
  }
  mi_timing_begin("spline_spread", stream);
  int rc = MI_OK;
  if (workspace && sp_tiled_ok(nx, ny, nz, n_systems, order) && workspace_bytes >= sp_layout(n_atoms, n_systems, nx, ny, nz, order, dtype_bytes(dtype)).total) {
    if (dtype == MI_F32)
      rc = spread_tiled<float>((const float*)positions, (const float*)values, batch_idx, (const float*)cell_inv_t, n_atoms, n_systems, nx, ny, nz,
                               order, batched, (float*)mesh, (char*)workspace, st);
    else
      rc = spread_tiled<double>((const double*)positions, (const double*)values, batch_idx, (const double*)cell_inv_t, n_atoms, n_systems, nx, ny,
                                nz, order, batched, (double*)mesh, (char*)workspace, st);
  } else {
    const int apb = 256 / (order * order);
    MI_DISPATCH_T(dtype, (spline_spread_kernel<T_><<<mi_blocks(n_atoms, apb), 256, 0, st>>>((const T_*)positions, (const T_*)values, batch_idx,
                                                                                            (const T_*)cell_inv_t, n_atoms, nx, ny, nz, order,
                                                                                            batched, (T_*)mesh)));
  }
  mi_timing_end(stream);
  if (rc != MI_OK) return rc;
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_spline_gather(const void* positions, const void* mesh, const int32_t* batch_idx, const void* cell_inv_t, int n_atoms, int n_systems, int nx,
                     int ny, int nz, int order, int dtype, void* out, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  const OrderArg oa = decode_order(order);
  order = oa.order;
  MI_REQUIRE(order >= 1 && order <= MI_MAX_ORDER, "spline order must be 1..6");
  (void)n_systems;
  if (n_atoms <= 0) return MI_OK;
  MI_REQUIRE(positions && mesh && cell_inv_t && out, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (oa.ref_zero) { MI_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)n_atoms * dtype_bytes(dtype), st)); return MI_OK; }
  mi_timing_begin("spline_gather", stream);
  MI_DISPATCH_T(dtype, (spline_gather_kernel<T_, 1><<<mi_blocks(n_atoms, 128), 128, 0, st>>>((const T_*)positions, nullptr, (const T_*)mesh, batch_idx,
                                                                                             (const T_*)cell_inv_t, n_atoms, nx, ny, nz, order,
                                                                                             (T_*)out)));
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

/* ---- multi-channel spread / gather (values[N, C] <-> mesh[B, C, nx, ny, nz]) ---- */
size_t mi_spline_spread_channels_workspace_bytes_for(int n_atoms, int n_systems, int nx, int ny, int nz, int order, int n_channels, int dtype) {
  if (n_atoms < 0 || n_systems < 1 || nx <= 0 || ny <= 0 || nz <= 0 || n_channels < 1 || (dtype != MI_F32 && dtype != MI_F64)) return 0;
  const OrderArg oa = decode_order(order);
  if (oa.order < 1 || oa.order > MI_MAX_ORDER) return 0;
  if (oa.ref_zero || !spc_tiled_ok(nx, ny, nz, n_systems, oa.order, n_channels, dtype_bytes(dtype))) return 256;  // the atomic kernel needs no scratch
  return sp_layout(n_atoms, n_systems, nx, ny, nz, oa.order, dtype_bytes(dtype), spc_plan(n_channels, oa.order, dtype_bytes(dtype)).cb).total;
}

int mi_spline_spread_channels(const void* positions, const void* values, const int32_t* batch_idx, const void* cell_inv_t, int n_atoms,
                              int n_systems, int n_channels, int nx, int ny, int nz, int order, int batched, int dtype, void* mesh, void* workspace,
                              size_t workspace_bytes, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  const OrderArg oa = decode_order(order);
  order = oa.order;
  MI_REQUIRE(order >= 1 && order <= MI_MAX_ORDER, "spline order must be 1..6");
  MI_REQUIRE(nx > 0 && ny > 0 && nz > 0 && n_systems >= 1, "mesh dimensions");
  MI_REQUIRE(n_channels >= 1, "n_channels must be >= 1");
  if (n_atoms <= 0) return MI_OK;
  MI_REQUIRE(positions && values && cell_inv_t && mesh, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const size_t mesh_bytes = (size_t)n_systems * n_channels * nx * ny * nz * dtype_bytes(dtype);
  if (oa.ref_zero) {  // all weights are zero: nothing is spread
    MI_HIP_CHECK(hipMemsetAsync(mesh, 0, mesh_bytes, st));
    return MI_OK;
  }
  mi_timing_begin("spline_spread_channels", stream);
  int rc = MI_OK;
  if (workspace && spc_tiled_ok(nx, ny, nz, n_systems, order, n_channels, dtype_bytes(dtype)) &&
      workspace_bytes >= sp_layout(n_atoms, n_systems, nx, ny, nz, order, dtype_bytes(dtype), spc_plan(n_channels, order, dtype_bytes(dtype)).cb).total) {
    MI_DISPATCH_T(dtype, rc = spread_channels_tiled<T_>((const T_*)positions, (const T_*)values, batch_idx, (const T_*)cell_inv_t, n_atoms, n_systems,
                                                        n_channels, nx, ny, nz, order, batched, (T_*)mesh, (char*)workspace, st));
  } else {
    // the atomic kernel adds into a zeroed mesh; the call clears it itself, so the caller's mesh may be uninitialised on either path
    hipError_t he = hipMemsetAsync(mesh, 0, mesh_bytes, st);
    if (he != hipSuccess) { mi_timing_end(stream); MI_HIP_CHECK(he); }
    const int apb = 256 / (order * order);
    MI_DISPATCH_T(dtype, (spline_spread_channels_kernel<T_><<<mi_blocks(n_atoms, apb), 256, 0, st>>>(
                             (const T_*)positions, (const T_*)values, batch_idx, (const T_*)cell_inv_t, n_atoms, n_channels, nx, ny, nz, order, batched,
                             (T_*)mesh)));
  }
  mi_timing_end(stream);
  if (rc != MI_OK) return rc;
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_spline_gather_channels(const void* positions, const void* mesh, const int32_t* batch_idx, const void* cell_inv_t, int n_atoms, int n_systems,
                              int n_channels, int nx, int ny, int nz, int order, int dtype, void* out, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  const OrderArg oa = decode_order(order);
  order = oa.order;
  MI_REQUIRE(order >= 1 && order <= MI_MAX_ORDER, "spline order must be 1..6");
  MI_REQUIRE(nx > 0 && ny > 0 && nz > 0 && n_systems >= 1, "mesh dimensions");
  MI_REQUIRE(n_channels >= 1, "n_channels must be >= 1");
  if (n_atoms <= 0) return MI_OK;
  MI_REQUIRE(positions && mesh && cell_inv_t && out, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (oa.ref_zero) { MI_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)n_atoms * n_channels * dtype_bytes(dtype), st)); return MI_OK; }
  mi_timing_begin("spline_gather_channels", stream);
  MI_DISPATCH_T(dtype, (spline_gather_channels_kernel<T_><<<mi_blocks(n_atoms, 128), 128, 0, st>>>((const T_*)positions, (const T_*)mesh, batch_idx,
                                                                                                   (const T_*)cell_inv_t, n_atoms, n_channels, nx, ny, nz,
                                                                                                   order, (T_*)out)));
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_spline_gather_channels_frac_grad(const void* positions, const void* mesh, const void* coef, const int32_t* batch_idx, const void* cell_inv_t,
                                        int n_atoms, int n_systems, int n_channels, int nx, int ny, int nz, int order, int dtype, void* out,
                                        void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  const OrderArg oa = decode_order(order);
  order = oa.order;
  MI_REQUIRE(order >= 1 && order <= MI_MAX_ORDER, "spline order must be 1..6");
  MI_REQUIRE(nx > 0 && ny > 0 && nz > 0 && n_systems >= 1, "mesh dimensions");
  MI_REQUIRE(n_channels >= 1, "n_channels must be >= 1");
  if (n_atoms <= 0) return MI_OK;
  MI_REQUIRE(positions && mesh && coef && cell_inv_t && out, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (oa.ref_zero) { MI_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)n_atoms * 3 * dtype_bytes(dtype), st)); return MI_OK; }
  mi_timing_begin("spline_gather_channels_frac_grad", stream);
  MI_DISPATCH_ORDER(order, MI_DISPATCH_T(dtype, (spline_gather_channels_frac_grad_kernel<T_, O_><<<mi_blocks(n_atoms, 128), 128, 0, st>>>(
                                                    (const T_*)positions, (const T_*)mesh, (const T_*)coef, batch_idx, (const T_*)cell_inv_t, n_atoms,
                                                    n_channels, nx, ny, nz, (T_*)out))));
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_spline_gather_grad(const void* positions, const void* mesh, const int32_t* batch_idx, const void* cell_inv_t, int n_atoms, int n_systems,
                          int nx, int ny, int nz, int order, int dtype, void* out, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  const OrderArg oa = decode_order(order);
  order = oa.order;
  MI_REQUIRE(order >= 1 && order <= MI_MAX_ORDER, "spline order must be 1..6");
  (void)n_systems;
  if (n_atoms <= 0) return MI_OK;
  MI_REQUIRE(positions && mesh && cell_inv_t && out, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (oa.ref_zero) { MI_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)n_atoms * 3 * dtype_bytes(dtype), st)); return MI_OK; }
  mi_timing_begin("spline_gather_grad", stream);
  MI_DISPATCH_ORDER(order, MI_DISPATCH_T(dtype, (spline_gather_grad_kernel<T_, O_><<<mi_blocks(n_atoms, 128), 128, 0, st>>>(
                                                    (const T_*)positions, (const T_*)mesh, batch_idx, (const T_*)cell_inv_t, n_atoms, nx, ny, nz, (T_*)out))));
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_spline_gather_hess_dot(const void* positions, const void* mesh, const int32_t* batch_idx, const void* cell_inv_t, const void* vec,
                              int n_atoms, int n_systems, int nx, int ny, int nz, int order, int dtype, void* out, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  const OrderArg oa = decode_order(order);
  order = oa.order;
  MI_REQUIRE(order >= 1 && order <= MI_MAX_ORDER, "spline order must be 1..6");
  (void)n_systems;
  if (n_atoms <= 0) return MI_OK;
  MI_REQUIRE(positions && mesh && cell_inv_t && vec && out, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (oa.ref_zero) { MI_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)n_atoms * 3 * dtype_bytes(dtype), st)); return MI_OK; }
  mi_timing_begin("spline_gather_hess_dot", stream);
  MI_DISPATCH_ORDER(order, MI_DISPATCH_T(dtype, (spline_gather_hess_dot_kernel<T_, O_><<<mi_blocks(n_atoms, 128), 128, 0, st>>>(
                                                    (const T_*)positions, (const T_*)mesh, batch_idx, (const T_*)cell_inv_t, (const T_*)vec, n_atoms, nx, ny, nz, (T_*)out))));
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_spline_spread_grad(const void* positions, const void* vec, const int32_t* batch_idx, const void* cell_inv_t, int n_atoms, int n_systems,
                          int nx, int ny, int nz, int order, int dtype, void* mesh, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  const OrderArg oa = decode_order(order);
  order = oa.order;
  MI_REQUIRE(order >= 1 && order <= MI_MAX_ORDER, "spline order must be 1..6");
  MI_REQUIRE(n_systems >= 1 && mesh, "mesh");
  hipStream_t st = (hipStream_t)stream;
  MI_HIP_CHECK(hipMemsetAsync(mesh, 0, (size_t)n_systems * nx * ny * nz * (dtype == MI_F32 ? 4 : 8), st));
  if (n_atoms <= 0 || oa.ref_zero) return MI_OK;
  MI_REQUIRE(positions && vec && cell_inv_t, "null pointer");
  mi_timing_begin("spline_spread_grad", stream);
  MI_DISPATCH_ORDER(order, MI_DISPATCH_T(dtype, (spline_spread_grad_kernel<T_, O_><<<mi_blocks(n_atoms, 128), 128, 0, st>>>(
                                                    (const T_*)positions, (const T_*)vec, batch_idx, (const T_*)cell_inv_t, n_atoms, nx, ny, nz, (T_*)mesh))));
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_spline_gather_vec3(const void* positions, const void* charges, const void* mesh_vec3, const int32_t* batch_idx, const void* cell_inv_t,
                          int n_atoms, int n_systems, int nx, int ny, int nz, int order, int dtype, void* out, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  const OrderArg oa = decode_order(order);
  order = oa.order;
  MI_REQUIRE(order >= 1 && order <= MI_MAX_ORDER, "spline order must be 1..6");
  (void)n_systems;
  if (n_atoms <= 0) return MI_OK;
  MI_REQUIRE(positions && charges && mesh_vec3 && cell_inv_t && out, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (oa.ref_zero) { MI_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)n_atoms * 3 * dtype_bytes(dtype), st)); return MI_OK; }
  MI_DISPATCH_T(dtype, (spline_gather_kernel<T_, 3><<<mi_blocks(n_atoms, 128), 128, 0, st>>>((const T_*)positions, (const T_*)charges,
                                                                                             (const T_*)mesh_vec3, batch_idx, (const T_*)cell_inv_t,
                                                                                             n_atoms, nx, ny, nz, order, (T_*)out)));
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_pme_green_sf(const void* k_squared, const void* alpha, const void* volume, int n_systems, int nx, int ny, int nz, int order, int dtype,
                    void* green, void* sf_sq, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(k_squared && alpha && volume && green && sf_sq && n_systems >= 1, "null pointer");
  order = decode_order(order).sf_exponent;
  const size_t tot = (size_t)nx * ny * (nz / 2 + 1) * n_systems;
  hipStream_t st = (hipStream_t)stream;
  MI_DISPATCH_T(dtype, (pme_green_sf_kernel<T_><<<mi_blocks((long long)tot, 256), 256, 0, st>>>((const T_*)k_squared, (const T_*)alpha,
                                                                                                (const T_*)volume, n_systems, nx, ny, nz, order,
                                                                                                (T_*)green, (T_*)sf_sq)));
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_pme_convolve(const void* spec, const void* recip_cell, const void* alpha, const void* volume, int n_systems, int nx, int ny, int nz, int order,
                    int with_field, int dtype, const void* k_vectors, const void* k_squared, int k_batched, void* out, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(spec && recip_cell && alpha && volume && out && n_systems >= 1, "null pointer");
  order = decode_order(order).sf_exponent;
  const size_t tot = (size_t)nx * ny * (nz / 2 + 1) * n_systems;
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("pme_convolve", stream);
  MI_DISPATCH_T(dtype, (pme_convolve_kernel<T_><<<mi_blocks((long long)tot, 256), 256, 0, st>>>((const Cplx<T_>*)spec, (const T_*)recip_cell,
                                                                                                (const T_*)alpha, (const T_*)volume, n_systems, nx,
                                                                                                ny, nz, order, with_field, (const T_*)k_vectors,
                                                                                                (const T_*)k_squared, k_batched, (Cplx<T_>*)out)));
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_pme_convolve_bwd(const void* spec, const void* weight_spec, int n_channels, const void* recip_cell, const void* alpha, const void* volume,
                        int n_systems, int nx, int ny, int nz, int order, int dtype, void* conv_out,
                        double* partial /*[n_systems][mi_pme_convolve_bwd_blocks()][20]*/, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_channels == 1 || n_channels == 4, "n_channels must be 1 (energy weights) or 4 (energy + three force-component weights)");
  MI_REQUIRE(spec && weight_spec && recip_cell && alpha && volume && partial && n_systems >= 1, "null pointer");
  order = decode_order(order).sf_exponent;
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("pme_convolve_bwd", stream);
  MI_DISPATCH_T(dtype, (pme_convolve_bwd_kernel<T_><<<dim3(PME_BWD_BLOCKS, n_systems), 256, 0, st>>>(
                           (const Cplx<T_>*)spec, (const Cplx<T_>*)weight_spec, n_channels, (const T_*)recip_cell, (const T_*)alpha, (const T_*)volume,
                           n_systems, nx, ny, nz, order, (Cplx<T_>*)conv_out, partial)));
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}
int mi_pme_convolve_bwd_blocks(void) { return PME_BWD_BLOCKS; }

int mi_pme_virial(const void* spec, const void* recip_cell, const void* alpha, const void* volume, int n_systems, int nx, int ny, int nz, int order,
                  int dtype, const void* k_vectors, const void* k_squared, int k_batched, const void* total_charge,
                  double* partial /*[n_systems][mi_pme_virial_blocks()][6]*/, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(spec && recip_cell && alpha && volume && partial && n_systems >= 1 && nx > 0 && ny > 0 && nz > 0, "null pointer");
  MI_REQUIRE((k_vectors == nullptr) == (k_squared == nullptr), "k_vectors and k_squared are given together or not at all");
  order = decode_order(order).sf_exponent;
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("pme_virial", stream);
  MI_DISPATCH_T(dtype, (pme_virial_kernel<T_><<<dim3(PME_VIR_BLOCKS, n_systems), 256, 0, st>>>(
                           (const Cplx<T_>*)spec, (const T_*)recip_cell, (const T_*)alpha, (const T_*)volume, nx, ny, nz, order,
                           (const T_*)k_vectors, (const T_*)k_squared, k_batched, (const T_*)total_charge, partial)));
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}
int mi_pme_virial_blocks(void) { return PME_VIR_BLOCKS; }

/* ---- fused mesh solve ------------------------------------------------------------------------------------------------------------------ */
int mi_pme_solve_supported(int n_systems, int nx, int ny, int nz, int dtype) {
  if (n_systems < 1 || !(dtype == MI_F32 || dtype == MI_F64) || !mifft::geom_ok(nx, ny, nz)) return 0;
  const mifft::Geom g = mifft::make_geom(n_systems, nx, ny, nz);
  if ((long long)n_systems * 4 * nx > 0x7fffffffll || n_systems > 65535) return 0;
  return (dtype == MI_F32 ? solve_fits<float>(g) : solve_fits<double>(g)) ? 1 : 0;
}
/* Host policy, measured.  Round 4 kept hipFFT's batched plans for batches of small meshes (128 x 32^3: 0.66 vs 0.85 ms with a build whose
 * persistent inverse plane kernel walked the small planes one after the other, profiles/r04_ab_solve_size.log).  With the round-5 build the
 * fused solve is at parity there and ahead elsewhere (profiles/r05_ab_solve_size.log: 128 x 32^3 0.674 vs 0.659 ms with forces, 0.402 vs
 * 0.407 energies only; 16 x 32^3 0.152 vs 0.149; 8 x 64^3 0.326 vs 0.335; 128^3 0.343 vs 0.371; 2 x 128^3 0.582 vs 0.650), and it is the
 * path that does not depend on rocFFT: every mesh the solve supports takes it. */
int mi_pme_solve_preferred(int n_systems, int nx, int ny, int nz, int dtype) {
  return mi_pme_solve_supported(n_systems, nx, ny, nz, dtype);
}
int mi_fft_lds_supported(int batch, int nx, int ny, int nz, int dtype) {
  if (!mi_pme_solve_supported(batch, nx, ny, nz, dtype)) return 0;
  const mifft::Geom g = mifft::make_geom(batch, nx, ny, nz);  // (the plane kernels of the transforms carry two small index tables more)
  return (dtype == MI_F32 ? mifft::plane_lds_bytes_nat<float>(g) : mifft::plane_lds_bytes_nat<double>(g)) <= MI_LDS_MAX ? 1 : 0;
}
size_t mi_fft_lds_scratch_bytes(int batch, int nx, int ny, int nz, int dtype) {
  if (!mi_fft_lds_supported(batch, nx, ny, nz, dtype)) return 0;
  const size_t per = (size_t)batch * nx * ny * (nz / 2 + 1) * (dtype == MI_F32 ? 8 : 16);
  const mifft::Geom g = mifft::make_geom(batch, nx, ny, nz);
  return mi_align(per) + mi_align(dtype == MI_F32 ? mifft::tables_bytes<float>(g) : mifft::tables_bytes<double>(g));
}
size_t mi_fft_lds_tables_bytes(int nx, int ny, int nz, int dtype) {
  if (nx < 1 || ny < 1 || nz < 2 || (dtype != MI_F32 && dtype != MI_F64) || !mifft::geom_ok(nx, ny, nz)) return 0;
  const mifft::Geom g = mifft::make_geom(1, nx, ny, nz);
  return mi_align(dtype == MI_F32 ? mifft::tables_bytes<float>(g) : mifft::tables_bytes<double>(g));
}
int mi_fft_lds_tables(int nx, int ny, int nz, int dtype, void* tables, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(tables && mifft::geom_ok(nx, ny, nz), "tables pointer / mesh not supported by the in-LDS transforms");
  const mifft::Geom g = mifft::make_geom(1, nx, ny, nz);
  MI_DISPATCH_T(dtype, (pme_solve_tables_kernel<T_><<<1, 256, 0, (hipStream_t)stream>>>(tables, g)));
  MI_LAUNCH_CHECK();
  return MI_OK;
}
int mi_fft_lds(const void* in, void* out, int batch, int nx, int ny, int nz, int dtype, int inverse, void* scratch, size_t scratch_bytes,
               const void* tables, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(in && out && scratch, "null pointer");
  MI_REQUIRE(mi_fft_lds_supported(batch, nx, ny, nz, dtype), "mesh not supported by the in-LDS transforms (see mi_fft_lds_supported)");
  MI_REQUIRE(scratch_bytes >= mi_fft_lds_scratch_bytes(batch, nx, ny, nz, dtype), "scratch too small (mi_fft_lds_scratch_bytes)");
  const mifft::Geom g = mifft::make_geom(batch, nx, ny, nz);
  const size_t per = (size_t)batch * nx * ny * g.P * (dtype == MI_F32 ? 8 : 16);
  void* work = scratch;
  void* tab = tables ? const_cast<void*>(tables) : (void*)((char*)scratch + mi_align(per));
  const bool ready = tables != nullptr;
  const int pt = solve_plane_threads(g);
  const int col_blocks = (g.ny * g.P + MI_SOLVE_COLS - 1) / MI_SOLVE_COLS;
  int rc = MI_OK;
  MI_DISPATCH_T(dtype, (rc = g.p2 ? fft_lds_launch_as<T_, false>(inverse != 0, in, out, g, work, tab, ready, pt, col_blocks, stream)
                                  : fft_lds_launch_as<T_, true>(inverse != 0, in, out, g, work, tab, ready, pt, col_blocks, stream)));
  if (rc != MI_OK) return rc;
  MI_LAUNCH_CHECK();
  return MI_OK;
}
size_t mi_pme_solve_scratch_bytes(int n_systems, int nx, int ny, int nz, int n_channels, int dtype) {
  const size_t per = (size_t)n_systems * nx * ny * (nz / 2 + 1) * (dtype == MI_F32 ? 8 : 16);
  const mifft::Geom g = mifft::make_geom(n_systems, nx, ny, nz);
  return mi_align(per) + mi_align(per * (size_t)n_channels) + mi_align(dtype == MI_F32 ? mifft::tables_bytes<float>(g) : mifft::tables_bytes<double>(g));
}
int mi_pme_solve(const void* mesh, const void* recip_cell, const void* alpha, const void* volume, int n_systems, int nx, int ny, int nz, int order,
                 int with_field, int dtype, void* scratch, size_t scratch_bytes, void* real_out, void* stream) {
  return mi_pme_solve_keep(mesh, recip_cell, alpha, volume, n_systems, nx, ny, nz, order, with_field, dtype, scratch, scratch_bytes, real_out, nullptr, stream);
}
int mi_pme_solve_keep(const void* mesh, const void* recip_cell, const void* alpha, const void* volume, int n_systems, int nx, int ny, int nz, int order,
                      int with_field, int dtype, void* scratch, size_t scratch_bytes, void* real_out, void* spectrum_out, void* stream) {
  return mi_pme_solve_tabled(mesh, recip_cell, alpha, volume, n_systems, nx, ny, nz, order, with_field, dtype, scratch, scratch_bytes, real_out, spectrum_out,
                             nullptr, stream);
}
int mi_pme_solve_tabled(const void* mesh, const void* recip_cell, const void* alpha, const void* volume, int n_systems, int nx, int ny, int nz, int order,
                        int with_field, int dtype, void* scratch, size_t scratch_bytes, void* real_out, void* spectrum_out, const void* tables, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(mesh && recip_cell && alpha && volume && scratch && real_out, "null pointer");
  MI_REQUIRE(mi_pme_solve_supported(n_systems, nx, ny, nz, dtype), "mesh not supported by the fused solve (see mi_pme_solve_supported)");
  const int nch = with_field ? 4 : 1;
  MI_REQUIRE(scratch_bytes >= mi_pme_solve_scratch_bytes(n_systems, nx, ny, nz, nch, dtype), "scratch too small (mi_pme_solve_scratch_bytes)");
  const int expo = decode_order(order).sf_exponent;
  const mifft::Geom g = mifft::make_geom(n_systems, nx, ny, nz);
  const size_t per = (size_t)n_systems * nx * ny * g.P * (dtype == MI_F32 ? 8 : 16);
  void* spec = scratch;
  void* conv = (char*)scratch + mi_align(per);
  void* tab = tables ? const_cast<void*>(tables) : (void*)((char*)conv + mi_align(per * (size_t)nch));
  const int pt = solve_plane_threads(g);
  const int col_blocks = (g.ny * g.P + MI_SOLVE_COLS - 1) / MI_SOLVE_COLS;
  int rc = MI_OK;
  MI_DISPATCH_T(dtype, (rc = solve_launch<T_>(mesh, recip_cell, alpha, volume, g, expo, nch, spec, conv, tab, tables != nullptr, real_out, spectrum_out, pt, col_blocks,
                                              stream)));
  if (rc != MI_OK) return rc;
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_pme_gather_finish(const void* positions, const void* charges, const int32_t* batch_idx, const void* cell_inv_t, const void* meshes,
                         const void* alpha, const void* volume, const void* total_charge, int n_atoms, int n_systems, int nx, int ny, int nz,
                         int order, int with_field, int dtype, void* energies, void* forces, void* charge_grads, const double* add_energies,
                         const void* add_forces, const double* add_charge_grads, const void* spread_workspace, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  const OrderArg oa = decode_order(order);
  order = oa.order;
  MI_REQUIRE(order >= 1 && order <= MI_MAX_ORDER, "spline order must be 1..6");
  if (n_atoms <= 0) return MI_OK;
  MI_REQUIRE(positions && charges && cell_inv_t && meshes && alpha && volume && total_charge && energies && n_systems >= 1, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("pme_gather_finish", stream);
  // the workspace of the tile-owned mi_spline_spread of the SAME step (same positions, mesh, order): atoms grouped by mesh tile, stencil
  // starts and fractional offsets -- the tile-staged kernel; without it the per-atom kernel
  static const bool allow_box = []() { const char* v = getenv("NVALCHEMIOPS_GATHER"); return !(v && v[0] == 'a'); }();  // "atom": A/B
  if (spread_workspace && allow_box && !oa.ref_zero && sp_tiled_ok(nx, ny, nz, n_systems, order)) {
    const SpLayout L = sp_layout(n_atoms, n_systems, nx, ny, nz);
    const SpTile e = sp_tile(nx, ny, nz);
    const char* ws = static_cast<const char*>(spread_workspace);
    const int* atom_of = reinterpret_cast<const int*>(ws + L.vals_out) + 4;
    const int* bin_start = reinterpret_cast<const int*>(ws + L.bin_start);
    const int4* lo3 = reinterpret_cast<const int4*>(ws + L.lo3);
    MI_DISPATCH_ORDER(order, MI_DISPATCH_T(dtype, (pme_gather_box_kernel<T_, O_><<<(int)L.nbins, 256, 0, st>>>(
                             (const T_*)charges, (const T_*)meshes, (const T_*)alpha, (const T_*)volume, (const T_*)total_charge, atom_of, bin_start, lo3,
                             reinterpret_cast<const T_*>(ws + L.theta), n_atoms, nx, ny, nz, with_field, e, (T_*)energies, (T_*)forces,
                             (T_*)charge_grads, add_energies, (const T_*)add_forces, add_charge_grads, T_(1)))));
  } else {
    const int32_t* atom_order = nullptr;
    if (spread_workspace && sp_tiled_ok(nx, ny, nz, n_systems, order))
      atom_order = reinterpret_cast<const int32_t*>(static_cast<const char*>(spread_workspace) + sp_layout(n_atoms, n_systems, nx, ny, nz).vals_out);
    MI_DISPATCH_ORDER(order, MI_DISPATCH_T(dtype, (pme_gather_finish_kernel<T_, O_><<<mi_blocks((long long)n_atoms * PG_LANES, 256), 256, 0, st>>>(
                             (const T_*)positions, (const T_*)charges, batch_idx, (const T_*)cell_inv_t, (const T_*)meshes, (const T_*)alpha,
                             (const T_*)volume, (const T_*)total_charge, n_atoms, nx, ny, nz, with_field, (T_*)energies, (T_*)forces,
                             (T_*)charge_grads, add_energies, (const T_*)add_forces, add_charge_grads, atom_order, oa.ref_zero ? T_(0) : T_(1)))));
  }
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_pme_corrections(const void* raw, const void* charges, const int32_t* batch_idx, const void* volume, const void* alpha,
                       const void* total_charge, int n_atoms, int dtype, void* energies, void* charge_grads, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  if (n_atoms <= 0) return MI_OK;
  MI_REQUIRE(raw && charges && volume && alpha && total_charge && energies, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  MI_DISPATCH_T(dtype, (pme_corrections_kernel<T_><<<mi_blocks(n_atoms, 256), 256, 0, st>>>((const T_*)raw, (const T_*)charges, batch_idx,
                                                                                            (const T_*)volume, (const T_*)alpha,
                                                                                            (const T_*)total_charge, n_atoms, (T_*)energies,
                                                                                            (T_*)charge_grads)));
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_segment_sum(const void* values, const int32_t* batch_idx, int n_atoms, int dtype, void* out, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  if (n_atoms <= 0) return MI_OK;
  MI_REQUIRE(values && out, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  MI_DISPATCH_T(dtype, (segment_sum_kernel<T_><<<mi_blocks(n_atoms, 256), 256, 0, st>>>((const T_*)values, batch_idx, n_atoms, (T_*)out)));
  MI_LAUNCH_CHECK();
  return MI_OK;
}

}  // extern "C"

// ==== particle-mesh Ewald for point dipoles (driver: nvalchemiops/interactions/electrostatics/pme_dipole.py) ================================
// Smooth PME with analytic spline derivatives (Toukmaji, Sagui, Board, Darden): with W_i(g) the B-spline weight of atom i at mesh point g,
//   rho_q = sum_i q_i W_i,  rho_mu = sum_i mu_i . grad W_i,  phi_X = the mesh solve of rho_X (mi_pme_solve* / mi_pme_convolve: linear, so the
//   meshes are further "systems" of one batched call),  phi_t = phi_q + phi_mu,  c = 2 alpha^3 / (3 sqrt(pi)):
//   E_i = q_i W_i.phi_mu + mu_i.grad W_i.phi_t - c |mu_i|^2,   dE/dq_i = 2 W_i.phi_mu,   dE/dmu_i = 2 grad W_i.phi_t - 2 c mu_i,
//   F_i = -2 [q_i grad W_i.phi_mu + (mu_i.grad) grad W_i.phi_t]
// grad is Cartesian: d W / d r_b = sum_a cit[a][b] n_a d W / d m_a, so the dipole enters as mu_frac = cit mu and the gather turns its
// fractional sums into Cartesian ones with cit once, at the end.
namespace {

// M_p(u), M_p'(u) and M_p''(u) from ONE pass of the B-spline recursion: at level p - 2 it holds a_k = M_{p-2}(u - k), k = 0..2, and
//   M_p'' = a_0 - 2 a_1 + a_2,   M_p' = b_0 - b_1 with b_k = M_{p-1}(u - k),   M_p = [u b_0 + (p - u) b_1] / (p - 1).
// Order 4 goes through the recursion as well: the expanded cubics of `bspline_ref` cancel terms of size 48 into a value below 0.67, which in
// float32 costs the dipole outputs a factor 3 in error against orders 5 and 6 (measured: 2.6e-6 vs 8e-7 of scale).
template <class T, int ORDER> __device__ __forceinline__ void dipole_spline(T u, T& w, T& d, T& dd) {
  w = d = dd = T(0);
  if (!(u >= T(0) && u < T(ORDER))) return;
  T m[ORDER];
#pragma unroll
  for (int k = 0; k < ORDER; ++k) { const T x = u - T(k); m[k] = (x >= T(0) && x < T(1)) ? T(1) : T(0); }
#pragma unroll
  for (int p = 2; p <= ORDER - 2; ++p) {
    const T inv = T(1) / T(p - 1);
#pragma unroll
    for (int k = 0; k <= ORDER - p; ++k) { const T x = u - T(k); m[k] = (x * m[k] + (T(p) - x) * m[k + 1]) * inv; }
  }
  dd = m[0] - T(2) * m[1] + m[2];
  const T inv = T(1) / T(ORDER - 2), x1 = u - T(1);
  const T b0 = (u * m[0] + (T(ORDER - 1) - u) * m[1]) * inv, b1 = (x1 * m[1] + (T(ORDER - 1) - x1) * m[2]) * inv;
  d = b0 - b1;
  w = (u * b0 + (T(ORDER) - u) * b1) / T(ORDER - 1);
}

// 1-D weights and first derivatives (times the mesh dimension) of one atom, evaluated ONCE by 3 x ORDER threads of its group, in LDS
template <class T, int ORDER> struct DipoleStencil { T w[3][ORDER], d[3][ORDER]; int gi[3][ORDER]; };

// Spread: order^2 threads per atom (one (tx, ty) column each, z innermost), like spline_spread_kernel; one pass writes rho_q and rho_mu -- and
// with per-atom weights g the two weighted meshes of the adjoint -- by atomic adds into meshes [2 | 4][B][nx][ny][nz] the entry point zeroed.
template <class T, int ORDER>
__global__ __launch_bounds__(256) void pme_dipole_spread_kernel(const T* __restrict__ pos, const T* __restrict__ charges, const T* __restrict__ dipoles,
                                                                const double* __restrict__ weights, const int* __restrict__ batch_idx,
                                                                const T* __restrict__ cit, int N, int B, int nx, int ny, int nz,
                                                                T* __restrict__ meshes) {
  constexpr int tpa = ORDER * ORDER, apb = 256 / tpa;
  __shared__ DipoleStencil<T, ORDER> sten[apb];
  const int la = threadIdx.x / tpa, col = threadIdx.x - la * tpa;
  const int i = blockIdx.x * apb + la;
  const bool active = la < apb && i < N;
  const int s = active && batch_idx ? batch_idx[i] : 0;
  if (active && col < 3 * ORDER) {
    const Stencil<T> st = make_stencil(pos + 3 * (size_t)i, cit + 9 * (size_t)s, nx, ny, nz, ORDER);
    const int d = col / ORDER, t = col - d * ORDER;
    const int n = d == 0 ? nx : (d == 1 ? ny : nz);
    const T u = (T)ORDER * T(0.5) + st.theta[d] - (T)(t + st.off0[d]);
    T w1, d1, dd1;
    dipole_spline<T, ORDER>(u, w1, d1, dd1);
    sten[la].w[d][t] = w1;
    sten[la].d[d][t] = d1 * (T)n;
    sten[la].gi[d][t] = wrap_idx(st.base[d] + t + st.off0[d], n);
  }
  __syncthreads();
  if (!active) return;
  const DipoleStencil<T, ORDER>& k = sten[la];
  const T* c = cit + 9 * (size_t)s;
  const T mu[3] = {dipoles[3 * (size_t)i], dipoles[3 * (size_t)i + 1], dipoles[3 * (size_t)i + 2]};
  T mf[3];
  mat3_colvec(c, mu, mf);  // mu_frac = cit mu
  const T q = charges[i];
  const int tx = col / ORDER, ty = col - tx * ORDER;
  const T wxy = k.w[0][tx] * k.w[1][ty];
  const T dxy = mf[0] * (k.d[0][tx] * k.w[1][ty]) + mf[1] * (k.w[0][tx] * k.d[1][ty]);  // the x and y terms of mu . grad W, without their w_z
  const T dz = mf[2] * wxy;
  const size_t mesh = (size_t)B * nx * ny * nz;
  T* row = meshes + (((size_t)s * nx + k.gi[0][tx]) * ny + k.gi[1][ty]) * nz;
  const bool weighted = weights != nullptr;
  const T g = weighted ? (T)weights[i] : T(0);
#pragma unroll
  for (int tz = 0; tz < ORDER; ++tz) {
    const T vq = q * (wxy * k.w[2][tz]);
    const T vm = dxy * k.w[2][tz] + dz * k.d[2][tz];
    T* p = row + k.gi[2][tz];
    if (vq != T(0)) atomicAdd(p, vq);
    if (vm != T(0)) atomicAdd(p + mesh, vm);
    if (weighted) {
      if (g * vq != T(0)) atomicAdd(p + 2 * mesh, g * vq);
      if (g * vm != T(0)) atomicAdd(p + 3 * mesh, g * vm);
    }
  }
}

// Gather: PG_LANES lanes per atom, one x-plane of the stencil each, shuffle fold -- the shape of pme_gather_finish_kernel.  One read of each
// of the two meshes A and B [B][nx][ny][nz] per stencil point; thirteen sums in fractional coordinates:
//   sA = W.A,  gA = grad W.A,  gB = grad W.B,  hB = (mu_frac . grad) grad W.B   (the six Hessian words contracted with mu_frac on the fly)
// and with D_i = {dq: sA, dmu: cit^T gB, dr: q cit^T gA + cit^T hB} the outputs are s_i D_i, s_i = 2 (the forward call: each atom is source
// and probe), g_i (weights) or 1 (accumulate: the second launch of the adjoint, added to what the first one wrote).  No atomics.
template <class T, int ORDER>
__global__ __launch_bounds__(256) void pme_dipole_gather_kernel(const T* __restrict__ pos, const T* __restrict__ charges, const T* __restrict__ dipoles,
                                                                const double* __restrict__ weights, const int* __restrict__ batch_idx,
                                                                const T* __restrict__ cit, const T* __restrict__ mesh_a, const T* __restrict__ mesh_b,
                                                                const T* __restrict__ alpha, int N, int nx, int ny, int nz, int accumulate,
                                                                double* __restrict__ energies, T* __restrict__ forces, double* __restrict__ cgrads,
                                                                double* __restrict__ dgrads) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i0 = t / PG_LANES, tx = t - i0 * PG_LANES;
  const int i = i0 < N ? i0 : N - 1;  // surplus groups of the last block recompute the last atom and do not store
  const int s = batch_idx ? batch_idx[i] : 0;
  const T* c = cit + 9 * (size_t)s;
  const Stencil<T> st = make_stencil(pos + 3 * (size_t)i, c, nx, ny, nz, ORDER);
  const int dims[3] = {nx, ny, nz};
  T w[2][ORDER], d[2][ORDER], dd[2][ORDER];  // the y and z axes; the lane's own x-plane below
  int gi[2][ORDER];
#pragma unroll
  for (int a = 1; a < 3; ++a)
#pragma unroll
    for (int k = 0; k < ORDER; ++k) {
      const T u = (T)ORDER * T(0.5) + st.theta[a] - (T)(k + st.off0[a]);
      const T n = (T)dims[a];
      T w1, d1, dd1;
      dipole_spline<T, ORDER>(u, w1, d1, dd1);
      w[a - 1][k] = w1;
      d[a - 1][k] = d1 * n;
      dd[a - 1][k] = dd1 * n * n;
      gi[a - 1][k] = wrap_idx(st.base[a] + k + st.off0[a], dims[a]);
    }
  const T mu[3] = {dipoles[3 * (size_t)i], dipoles[3 * (size_t)i + 1], dipoles[3 * (size_t)i + 2]};
  T mf[3];
  mat3_colvec(c, mu, mf);
  T sA = 0, gA[3] = {0, 0, 0}, gB[3] = {0, 0, 0}, hB[3] = {0, 0, 0};
  if (tx < ORDER) {
    const T u = (T)ORDER * T(0.5) + st.theta[0] - (T)(tx + st.off0[0]);
    T wx, dx, ddx;
    dipole_spline<T, ORDER>(u, wx, dx, ddx);
    dx *= (T)nx;
    ddx *= (T)nx * (T)nx;
    const size_t m0 = ((size_t)s * nx + wrap_idx(st.base[0] + tx + st.off0[0], nx)) * ny;
#pragma unroll
    for (int ty = 0; ty < ORDER; ++ty) {
      const size_t row = (m0 + gi[0][ty]) * nz;
      const T wy = w[0][ty], dy = d[0][ty], ddy = dd[0][ty];
#pragma unroll
      for (int tz = 0; tz < ORDER; ++tz) {
        const T a = mesh_a[row + gi[1][tz]], b = mesh_b[row + gi[1][tz]];
        const T wz = w[1][tz], dz = d[1][tz], ddz = dd[1][tz];
        const T W = wx * wy * wz, Gx = dx * wy * wz, Gy = wx * dy * wz, Gz = wx * wy * dz;
        const T hxx = ddx * wy * wz, hyy = wx * ddy * wz, hzz = wx * wy * ddz, hxy = dx * dy * wz, hxz = dx * wy * dz, hyz = wx * dy * dz;
        sA += a * W;
        gA[0] += a * Gx; gA[1] += a * Gy; gA[2] += a * Gz;
        gB[0] += b * Gx; gB[1] += b * Gy; gB[2] += b * Gz;
        hB[0] += b * (mf[0] * hxx + mf[1] * hxy + mf[2] * hxz);
        hB[1] += b * (mf[0] * hxy + mf[1] * hyy + mf[2] * hyz);
        hB[2] += b * (mf[0] * hxz + mf[1] * hyz + mf[2] * hzz);
      }
    }
  }
#pragma unroll
  for (int o = PG_LANES / 2; o > 0; o >>= 1) {
    sA += __shfl_xor(sA, o, PG_LANES);
#pragma unroll
    for (int a = 0; a < 3; ++a) { gA[a] += __shfl_xor(gA[a], o, PG_LANES); gB[a] += __shfl_xor(gB[a], o, PG_LANES); hB[a] += __shfl_xor(hB[a], o, PG_LANES); }
  }
  if (tx != 0 || i0 >= N) return;
  // fractional -> Cartesian: v_cart[b] = sum_a cit[a][b] v_frac[a], in double
  const double q = (double)charges[i];
  double cA[3], cB[3], cH[3];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    cA[b] = (double)c[b] * (double)gA[0] + (double)c[3 + b] * (double)gA[1] + (double)c[6 + b] * (double)gA[2];
    cB[b] = (double)c[b] * (double)gB[0] + (double)c[3 + b] * (double)gB[1] + (double)c[6 + b] * (double)gB[2];
    cH[b] = (double)c[b] * (double)hB[0] + (double)c[3 + b] * (double)hB[1] + (double)c[6 + b] * (double)hB[2];
  }
  const double al = (double)alpha[s];
  const double self = 2.0 * al * al * al / (3.0 * 1.7724538509055160273);  // 2 alpha^3 / (3 sqrt(pi))
  const double m[3] = {(double)mu[0], (double)mu[1], (double)mu[2]};
  const double gw = weights ? weights[i] : 1.0;
  const double sc = accumulate ? 1.0 : (weights ? gw : 2.0);
  if (energies) energies[i] = q * (double)sA + (m[0] * cB[0] + m[1] * cB[1] + m[2] * cB[2]) - self * (m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
  if (cgrads) { const double v = sc * (double)sA; cgrads[i] = accumulate ? cgrads[i] + v : v; }
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const size_t o = 3 * (size_t)i + b;
    if (dgrads) { const double v = sc * cB[b]; dgrads[o] = accumulate ? dgrads[o] + v : v - 2.0 * self * gw * m[b]; }
    if (forces) { const double v = -sc * (q * cA[b] + cH[b]); forces[o] = accumulate ? (T)((double)forces[o] + v) : (T)v; }
  }
}

// k-space virial of the cross spectrum: pme_virial_kernel over the two spectra rho_hat_q, rho_hat_mu [B][nx][ny][nzr],
//   W[a][b] = sum_m E_m (delta_ab - 2 (1/k^2 + 1/(4 alpha^2)) k_a k_b),  E_m = h_m G_m (2 Re[conj(rho_hat_q) rho_hat_mu] + |rho_hat_mu|^2) / sf2_m
// (the cross form: never the difference of two quadratic forms).  Nine sums, row-major, per system and block; the caller adds the term of
// the dipoles' fractional components, sum_i (dE/dmu_i without the self term)_a mu_i,b, which is what makes the virial non-symmetric.
template <class T>
__global__ __launch_bounds__(256) void pme_dipole_virial_kernel(const Cplx<T>* __restrict__ spec_q, const Cplx<T>* __restrict__ spec_mu,
                                                                const T* __restrict__ recip, const T* __restrict__ alpha, const T* __restrict__ volume,
                                                                int nx, int ny, int nz, int order, double* __restrict__ partial) {
  const int b = blockIdx.y;
  const int nzr = nz / 2 + 1;
  const size_t per = (size_t)nx * ny * nzr;
  const T* R = recip + 9 * (size_t)b;
  const T al = alpha[b], vol = volume[b];
  const double c4 = 1.0 / (4.0 * (double)al * (double)al);
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x; r < per; r += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(r % nzr), j = (int)((r / nzr) % ny), i = (int)(r / ((size_t)nzr * ny));
    const int mx = miller_of(i, nx), my = miller_of(j, ny), mz = k;
    const T m[3] = {(T)mx, (T)my, (T)mz};
    T kv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) kv[c] = m[0] * R[3 * c] + m[1] * R[3 * c + 1] + m[2] * R[3 * c + 2];
    T k2 = kv[0] * kv[0] + kv[1] * kv[1] + kv[2] * kv[2];
    if (!(k2 > T(1e-12))) k2 = T(1e-12);
    const T G = green_of(k2, al, vol, i == 0 && j == 0 && k == 0);
    if (G == T(0)) continue;
    const T sf2 = sf_sq_of<T>(mx, my, mz, nx, ny, nz, order);
    const Cplx<T> vq = spec_q[(size_t)b * per + r], vm = spec_mu[(size_t)b * per + r];
    const double h = (k == 0 || (2 * k == nz)) ? 1.0 : 2.0;
    const double cross = 2.0 * ((double)vq.re * (double)vm.re + (double)vq.im * (double)vm.im) + (double)vm.re * (double)vm.re + (double)vm.im * (double)vm.im;
    const double e = h * cross * ((double)G / (double)sf2);
    const double c = -2.0 * e * (1.0 / (double)k2 + c4);
    const double kx = kv[0], ky = kv[1], kz = kv[2];
    acc[0] += e + c * kx * kx; acc[1] += e + c * ky * ky; acc[2] += e + c * kz * kz;
    acc[3] += c * kx * ky; acc[4] += c * kx * kz; acc[5] += c * ky * kz;
  }
  __shared__ double part[4][6];
  const int lane = threadIdx.x & (MI_WAVE - 1), wave = threadIdx.x / MI_WAVE;
#pragma unroll
  for (int q = 0; q < 6; ++q) { const double t = wave_sum(acc[q]); if (lane == 0) part[wave][q] = t; }
  __syncthreads();
  if (threadIdx.x < 9) {
    const int a = threadIdx.x / 3, bb = threadIdx.x - 3 * a;
    const int q = a == bb ? a : (a + bb + 2);  // {xx, yy, zz, xy, xz, yz} -> row-major 3 x 3 (this part is symmetric)
    partial[((size_t)b * gridDim.x + blockIdx.x) * 9 + threadIdx.x] = part[0][q] + part[1][q] + part[2][q] + part[3][q];
  }
}

}  // namespace

extern "C" {

int mi_pme_dipole_spread(const void* positions, const void* charges, const void* dipoles, const double* weights, const int32_t* batch_idx,
                         const void* cell_inv_t, int n_atoms, int n_systems, int nx, int ny, int nz, int order, int dtype, void* meshes, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(order >= 4 && order <= MI_MAX_ORDER, "spline order must be 4..6 (the dipole terms need two continuous derivatives of the spline)");
  MI_REQUIRE(n_systems >= 1 && nx >= order && ny >= order && nz >= order, "every mesh dimension must be at least the spline order");
  MI_REQUIRE(n_atoms >= 0 && meshes && cell_inv_t, "null pointer");
  MI_REQUIRE(n_atoms == 0 || (positions && charges && dipoles), "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const size_t mesh_bytes = (size_t)n_systems * nx * ny * nz * dtype_bytes(dtype);
  mi_timing_begin("pme_dipole_spread", stream);
  MI_HIP_CHECK(hipMemsetAsync(meshes, 0, (weights ? 4 : 2) * mesh_bytes, st));
  if (n_atoms > 0) {
    const int apb = 256 / (order * order);
    MI_DISPATCH_ORDER(order, MI_DISPATCH_T(dtype, (pme_dipole_spread_kernel<T_, (O_ < 4 ? 4 : O_)><<<mi_blocks(n_atoms, apb), 256, 0, st>>>(
                                 (const T_*)positions, (const T_*)charges, (const T_*)dipoles, weights, batch_idx, (const T_*)cell_inv_t, n_atoms,
                                 n_systems, nx, ny, nz, (T_*)meshes))));
  }
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_pme_dipole_gather(const void* positions, const void* charges, const void* dipoles, const double* weights, const int32_t* batch_idx,
                         const void* cell_inv_t, const void* mesh_a, const void* mesh_b, const void* alpha, int n_atoms, int n_systems, int nx, int ny,
                         int nz, int order, int dtype, int accumulate, double* energies, void* forces, double* charge_grads, double* dipole_grads,
                         void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(order >= 4 && order <= MI_MAX_ORDER, "spline order must be 4..6 (the dipole terms need two continuous derivatives of the spline)");
  MI_REQUIRE(n_systems >= 1 && nx >= order && ny >= order && nz >= order, "every mesh dimension must be at least the spline order");
  MI_REQUIRE(!(accumulate && weights), "accumulate (the second launch of the adjoint) takes no weights");
  if (n_atoms <= 0) return MI_OK;
  MI_REQUIRE(positions && charges && dipoles && cell_inv_t && mesh_a && mesh_b && alpha, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("pme_dipole_gather", stream);
  MI_DISPATCH_ORDER(order, MI_DISPATCH_T(dtype, (pme_dipole_gather_kernel<T_, (O_ < 4 ? 4 : O_)><<<mi_blocks((long long)n_atoms * PG_LANES, 256), 256, 0, st>>>(
                               (const T_*)positions, (const T_*)charges, (const T_*)dipoles, weights, batch_idx, (const T_*)cell_inv_t, (const T_*)mesh_a,
                               (const T_*)mesh_b, (const T_*)alpha, n_atoms, nx, ny, nz, accumulate, energies, (T_*)forces, charge_grads, dipole_grads))));
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_pme_dipole_virial(const void* spec_q, const void* spec_mu, const void* recip_cell, const void* alpha, const void* volume, int n_systems, int nx,
                         int ny, int nz, int order, int dtype, double* partial /*[n_systems][mi_pme_dipole_virial_blocks()][9]*/, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(order >= 4 && order <= MI_MAX_ORDER, "spline order must be 4..6 (the dipole terms need two continuous derivatives of the spline)");
  MI_REQUIRE(spec_q && spec_mu && recip_cell && alpha && volume && partial && n_systems >= 1 && n_systems <= 65535 && nx > 0 && ny > 0 && nz > 0,
             "null pointer");
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("pme_dipole_virial", stream);
  MI_DISPATCH_T(dtype, (pme_dipole_virial_kernel<T_><<<dim3(PME_VIR_BLOCKS, n_systems), 256, 0, st>>>(
                           (const Cplx<T_>*)spec_q, (const Cplx<T_>*)spec_mu, (const T_*)recip_cell, (const T_*)alpha, (const T_*)volume, nx, ny, nz, order,
                           partial)));
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}
int mi_pme_dipole_virial_blocks(void) { return PME_VIR_BLOCKS; }

}  // extern "C"

// ==== particle-mesh Ewald for point quadrupoles (driver: nvalchemiops/interactions/electrostatics/pme_quadrupole.py) ========================
// The section above continued by one multipole order.  With l_i = q_i + mu_i . grad and Theta_i = Q_i : grad grad (Q_i symmetric):
//   rho_l = sum_i l_i W_i,  rho_T = sum_i Theta_i W_i,  phi_T = solve(rho_T),  phi_L = solve(rho_l) + phi_T,
//   c3 = 4 alpha^3 / (3 sqrt(pi)),  c5 = 4 alpha^5 / (5 sqrt(pi)):
//   E_i = l_i W_i.phi_T + Theta_i W_i.phi_L + c3 q_i tr Q_i - c5 (2 Q_i:Q_i + (tr Q_i)^2)
//   dE/dq_i = 2 W_i.phi_T + c3 tr Q_i,   dE/dmu_i = 2 grad W_i.phi_T,   dE/dQ_i = 2 grad grad W_i.phi_L + c3 q_i I - c5 (4 Q_i + 2 tr Q_i I)
//   F_i = -2 [q_i grad W_i.phi_T + (mu_i.grad) grad W_i.phi_T + (Q_i:grad grad) grad W_i.phi_L]
// In mesh coordinates Q : grad grad W = sum_aa' Qf[a][a'] d2 W / dm_a dm_a' with Qf = cit Q cit^T; the factors n_a of d / dm_a live in the 1-D
// tables (M' n, M'' n^2, M''' n^3), and Qf travels as six words {xx, yy, zz, 2 xy, 2 xz, 2 yz}.
namespace {

// `dipole_spline` with M_p''' as well, from the same single pass of the recursion: at level p - 3 it holds c_k = M_{p-3}(u - k), k = 0..3, and
//   M_p''' = c_0 - 3 c_1 + 3 c_2 - c_3.   ORDER is 5 or 6 (at order 4 level p - 3 is the indicator function: M_4''' is not continuous).
template <class T, int ORDER> __device__ __forceinline__ void quadrupole_spline(T u, T& w, T& d, T& dd, T& ddd) {
  static_assert(ORDER >= 5, "the third derivative needs order 5 or 6");
  w = d = dd = ddd = T(0);
  if (!(u >= T(0) && u < T(ORDER))) return;
  T m[ORDER];
#pragma unroll
  for (int k = 0; k < ORDER; ++k) { const T x = u - T(k); m[k] = (x >= T(0) && x < T(1)) ? T(1) : T(0); }
#pragma unroll
  for (int p = 2; p <= ORDER - 3; ++p) {
    const T inv = T(1) / T(p - 1);
#pragma unroll
    for (int k = 0; k <= ORDER - p; ++k) { const T x = u - T(k); m[k] = (x * m[k] + (T(p) - x) * m[k + 1]) * inv; }
  }
  ddd = m[0] - T(3) * m[1] + T(3) * m[2] - m[3];
  {
    const T inv = T(1) / T(ORDER - 3);
#pragma unroll
    for (int k = 0; k <= 2; ++k) { const T x = u - T(k); m[k] = (x * m[k] + (T(ORDER - 2) - x) * m[k + 1]) * inv; }
  }
  dd = m[0] - T(2) * m[1] + m[2];
  const T inv = T(1) / T(ORDER - 2), x1 = u - T(1);
  const T b0 = (u * m[0] + (T(ORDER - 1) - u) * m[1]) * inv, b1 = (x1 * m[1] + (T(ORDER - 1) - x1) * m[2]) * inv;
  d = b0 - b1;
  w = (u * b0 + (T(ORDER) - u) * b1) / T(ORDER - 1);
}

// Qf = cit Qs cit^T of Qs = 1/2 (Q + Q^T), as six words {xx, yy, zz, 2 xy, 2 xz, 2 yz}: Q : grad grad W = sum_w qf[w] H[w] over the six
// distinct second derivatives of W in mesh coordinates
template <class T> __device__ __forceinline__ void quadrupole_frac(const T* __restrict__ c, const T* __restrict__ Q9, T qf[6]) {
  T qs[3][3], cq[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) qs[a][b] = T(0.5) * (Q9[3 * a + b] + Q9[3 * b + a]);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) cq[a][b] = c[3 * a] * qs[0][b] + c[3 * a + 1] * qs[1][b] + c[3 * a + 2] * qs[2][b];
  auto f = [&](int a, int b) { return cq[a][0] * c[3 * b] + cq[a][1] * c[3 * b + 1] + cq[a][2] * c[3 * b + 2]; };
  qf[0] = f(0, 0); qf[1] = f(1, 1); qf[2] = f(2, 2);
  qf[3] = T(2) * f(0, 1); qf[4] = T(2) * f(0, 2); qf[5] = T(2) * f(1, 2);
}

// 1-D values, first and second derivatives (times n, n^2) of one atom, evaluated ONCE by 3 x ORDER threads of its group, in LDS
template <class T, int ORDER> struct QuadrupoleStencil { T w[3][ORDER], d[3][ORDER], dd[3][ORDER]; int gi[3][ORDER]; };

// Spread: pme_dipole_spread_kernel with a second-derivative table.  One pass adds l_i W_i into meshes[0] and Theta_i W_i into meshes[1] -- and
// with per-atom weights g their weighted twins into meshes[2], meshes[3] -- by atomic adds into [2 | 4][B][nx][ny][nz] the entry point zeroed.
// A value that is exactly zero is not added: zero quadrupoles leave meshes[1] exactly zero.
template <class T, int ORDER>
__global__ __launch_bounds__(256) void pme_quadrupole_spread_kernel(const T* __restrict__ pos, const T* __restrict__ charges, const T* __restrict__ dipoles,
                                                                    const T* __restrict__ quadrupoles, const double* __restrict__ weights,
                                                                    const int* __restrict__ batch_idx, const T* __restrict__ cit, int N, int B, int nx,
                                                                    int ny, int nz, T* __restrict__ meshes) {
  constexpr int tpa = ORDER * ORDER, apb = 256 / tpa;
  __shared__ QuadrupoleStencil<T, ORDER> sten[apb];
  const int la = threadIdx.x / tpa, col = threadIdx.x - la * tpa;
  const int i = blockIdx.x * apb + la;
  const bool active = la < apb && i < N;
  const int s = active && batch_idx ? batch_idx[i] : 0;
  if (active && col < 3 * ORDER) {
    const Stencil<T> st = make_stencil(pos + 3 * (size_t)i, cit + 9 * (size_t)s, nx, ny, nz, ORDER);
    const int d = col / ORDER, t = col - d * ORDER;
    const int n = d == 0 ? nx : (d == 1 ? ny : nz);
    const T u = (T)ORDER * T(0.5) + st.theta[d] - (T)(t + st.off0[d]);
    T w1, d1, dd1, ddd1;
    quadrupole_spline<T, ORDER>(u, w1, d1, dd1, ddd1);
    sten[la].w[d][t] = w1;
    sten[la].d[d][t] = d1 * (T)n;
    sten[la].dd[d][t] = dd1 * (T)n * (T)n;
    sten[la].gi[d][t] = wrap_idx(st.base[d] + t + st.off0[d], n);
  }
  __syncthreads();
  if (!active) return;
  const QuadrupoleStencil<T, ORDER>& k = sten[la];
  const T* c = cit + 9 * (size_t)s;
  const T mu[3] = {dipoles[3 * (size_t)i], dipoles[3 * (size_t)i + 1], dipoles[3 * (size_t)i + 2]};
  T mf[3], qf[6];
  mat3_colvec(c, mu, mf);  // mu_frac = cit mu
  quadrupole_frac(c, quadrupoles + 9 * (size_t)i, qf);
  const T q = charges[i];
  const int tx = col / ORDER, ty = col - tx * ORDER;
  const T wx = k.w[0][tx], dx = k.d[0][tx], ddx = k.dd[0][tx], wy = k.w[1][ty], dy = k.d[1][ty], ddy = k.dd[1][ty];
  // per column: the coefficients of w_z, w_z' and w_z'' of the two densities
  const T l0 = q * (wx * wy) + mf[0] * (dx * wy) + mf[1] * (wx * dy), l1 = mf[2] * (wx * wy);
  const T t0 = qf[0] * (ddx * wy) + qf[1] * (wx * ddy) + qf[3] * (dx * dy), t1 = qf[4] * (dx * wy) + qf[5] * (wx * dy), t2 = qf[2] * (wx * wy);
  const size_t mesh = (size_t)B * nx * ny * nz;
  T* row = meshes + (((size_t)s * nx + k.gi[0][tx]) * ny + k.gi[1][ty]) * nz;
  const bool weighted = weights != nullptr;
  const T g = weighted ? (T)weights[i] : T(0);
#pragma unroll
  for (int tz = 0; tz < ORDER; ++tz) {
    const T vl = l0 * k.w[2][tz] + l1 * k.d[2][tz];
    const T vt = t0 * k.w[2][tz] + t1 * k.d[2][tz] + t2 * k.dd[2][tz];
    T* p = row + k.gi[2][tz];
    if (vl != T(0)) atomicAdd(p, vl);
    if (vt != T(0)) atomicAdd(p + mesh, vt);
    if (weighted) {
      if (g * vl != T(0)) atomicAdd(p + 2 * mesh, g * vl);
      if (g * vt != T(0)) atomicAdd(p + 3 * mesh, g * vt);
    }
  }
}

// Gather: PG_LANES lanes per atom, one x-plane of the stencil each, shuffle fold, no atomics -- the shape of pme_dipole_gather_kernel.  One read
// of each of the two meshes A and B per stencil point.  The sums are taken axis by axis: the z-contractions of a mesh row with w_z .. w_z''',
// then those with the y table, and once per lane with the lane's x values, which gives every mixed derivative up to the order needed:
//   sA = W.A,  gA = grad W.A,  hA = (mu_frac . grad) grad W.A (FV only),  HB = the six Hessian words of B,  tB = (Qf : grad grad) grad W.B (FV only)
// With D_i = {dq: sA, dmu: cit^T gA, dQ: cit^T HB cit, dr: cit^T (q gA + hA + tB)} the outputs are s_i D_i, s_i = 2 (the forward call), g_i
// (weights) or 1 (accumulate: the second launch of the adjoint, added to what the first one wrote); the self terms ride with the first launch.
// FV (forces wanted) is a compile-time split: the third-derivative tables and the Hessian of A exist only where the forces are asked for.
template <class T, int ORDER, bool FV>
__global__ __launch_bounds__(256) void pme_quadrupole_gather_kernel(const T* __restrict__ pos, const T* __restrict__ charges, const T* __restrict__ dipoles,
                                                                    const T* __restrict__ quadrupoles, const double* __restrict__ weights,
                                                                    const int* __restrict__ batch_idx, const T* __restrict__ cit,
                                                                    const T* __restrict__ mesh_a, const T* __restrict__ mesh_b, const T* __restrict__ alpha,
                                                                    int N, int nx, int ny, int nz, int accumulate, double* __restrict__ energies,
                                                                    T* __restrict__ forces, double* __restrict__ cgrads, double* __restrict__ dgrads,
                                                                    double* __restrict__ qgrads) {
  constexpr int D = FV ? 4 : 3;  // derivative orders held per axis
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int i0 = t / PG_LANES, tx = t - i0 * PG_LANES;
  const int i = i0 < N ? i0 : N - 1;  // surplus groups of the last block recompute the last atom and do not store
  const int s = batch_idx ? batch_idx[i] : 0;
  const T* c = cit + 9 * (size_t)s;
  // The stencil and the 1-D tables are formed in double from the caller's values and rounded once: a float32 call spreads in double
  // (`_spread`), so its meshes hold the weights of the unrounded mesh coordinate.  Tables from a float32 coordinate (off by up to 1e-6 of
  // a mesh spacing) are those of a slightly displaced atom, on which its own density then pulls: a force of float32-rounding size that
  // does not shrink with the net force.  In a float64 call every operation below is what it was.
  double p3[3], c9[9];
#pragma unroll
  for (int k = 0; k < 3; ++k) p3[k] = (double)pos[3 * (size_t)i + k];
#pragma unroll
  for (int k = 0; k < 9; ++k) c9[k] = (double)c[k];
  const Stencil<double> st = make_stencil<double>(p3, c9, nx, ny, nz, ORDER);
  const int dims[3] = {nx, ny, nz};
  T tab[2][D][ORDER];  // the y and z axes: M, M' n, M'' n^2 (, M''' n^3); the lane's own x-plane below
  int gi[2][ORDER];
#pragma unroll
  for (int a = 1; a < 3; ++a)
#pragma unroll
    for (int k = 0; k < ORDER; ++k) {
      const double u = (double)ORDER * 0.5 + st.theta[a] - (double)(k + st.off0[a]);
      const double n = (double)dims[a];
      double v[4];
      quadrupole_spline<double, ORDER>(u, v[0], v[1], v[2], v[3]);
      double f = 1.0;
#pragma unroll
      for (int o = 0; o < D; ++o) { tab[a - 1][o][k] = (T)(v[o] * f); f *= n; }
      gi[a - 1][k] = wrap_idx(st.base[a] + k + st.off0[a], dims[a]);
    }
  const T mu[3] = {dipoles[3 * (size_t)i], dipoles[3 * (size_t)i + 1], dipoles[3 * (size_t)i + 2]};
  T mf[3], qf[6];
  mat3_colvec(c, mu, mf);
  quadrupole_frac(c, quadrupoles + 9 * (size_t)i, qf);
  T sA = 0, gA[3] = {0, 0, 0}, hA[3] = {0, 0, 0}, HB[6] = {0, 0, 0, 0, 0, 0}, tB[3] = {0, 0, 0};
  if (tx < ORDER) {
    const double u = (double)ORDER * 0.5 + st.theta[0] - (double)(tx + st.off0[0]);
    double Xd[4];
    quadrupole_spline<double, ORDER>(u, Xd[0], Xd[1], Xd[2], Xd[3]);
    Xd[1] *= (double)nx;
    Xd[2] *= (double)nx * (double)nx;
    Xd[3] *= (double)nx * (double)nx * (double)nx;
    const T X[4] = {(T)Xd[0], (T)Xd[1], (T)Xd[2], (T)Xd[3]};
    const size_t m0 = ((size_t)s * nx + wrap_idx(st.base[0] + tx + st.off0[0], nx)) * ny;
    // P[j][k] = sum over the lane's plane of (d/dm_y)^j (d/dm_z)^k of the weights times the mesh, j + k < D (A: j + k < D - 1)
    T PA[D - 1][D - 1], PB[D][D];
#pragma unroll
    for (int j = 0; j < D; ++j)
#pragma unroll
      for (int k = 0; k < D; ++k) { PB[j][k] = T(0); if (j < D - 1 && k < D - 1) PA[j][k] = T(0); }
#pragma unroll
    for (int ty = 0; ty < ORDER; ++ty) {
      const size_t row = (m0 + gi[0][ty]) * nz;
      T za[D - 1], zb[D];
#pragma unroll
      for (int k = 0; k < D; ++k) { zb[k] = T(0); if (k < D - 1) za[k] = T(0); }
#pragma unroll
      for (int tz = 0; tz < ORDER; ++tz) {
        const T a = mesh_a[row + gi[1][tz]], b = mesh_b[row + gi[1][tz]];
#pragma unroll
        for (int k = 0; k < D; ++k) { zb[k] += b * tab[1][k][tz]; if (k < D - 1) za[k] += a * tab[1][k][tz]; }
      }
#pragma unroll
      for (int j = 0; j < D; ++j)
#pragma unroll
        for (int k = 0; k + j < D; ++k) {
          PB[j][k] += tab[0][j][ty] * zb[k];
          if (j + k < D - 1) PA[j][k] += tab[0][j][ty] * za[k];
        }
    }
    sA = X[0] * PA[0][0];
    gA[0] = X[1] * PA[0][0]; gA[1] = X[0] * PA[1][0]; gA[2] = X[0] * PA[0][1];
    HB[0] = X[2] * PB[0][0]; HB[1] = X[0] * PB[2][0]; HB[2] = X[0] * PB[0][2];
    HB[3] = X[1] * PB[1][0]; HB[4] = X[1] * PB[0][1]; HB[5] = X[0] * PB[1][1];
    if constexpr (FV) {
      const T axx = X[2] * PA[0][0], ayy = X[0] * PA[2][0], azz = X[0] * PA[0][2], axy = X[1] * PA[1][0], axz = X[1] * PA[0][1], ayz = X[0] * PA[1][1];
      hA[0] = mf[0] * axx + mf[1] * axy + mf[2] * axz;
      hA[1] = mf[0] * axy + mf[1] * ayy + mf[2] * ayz;
      hA[2] = mf[0] * axz + mf[1] * ayz + mf[2] * azz;
      const T xxx = X[3] * PB[0][0], xxy = X[2] * PB[1][0], xxz = X[2] * PB[0][1], xyy = X[1] * PB[2][0], xyz = X[1] * PB[1][1], xzz = X[1] * PB[0][2];
      const T yyy = X[0] * PB[3][0], yyz = X[0] * PB[2][1], yzz = X[0] * PB[1][2], zzz = X[0] * PB[0][3];
      tB[0] = qf[0] * xxx + qf[1] * xyy + qf[2] * xzz + qf[3] * xxy + qf[4] * xxz + qf[5] * xyz;
      tB[1] = qf[0] * xxy + qf[1] * yyy + qf[2] * yzz + qf[3] * xyy + qf[4] * xyz + qf[5] * yyz;
      tB[2] = qf[0] * xxz + qf[1] * yyz + qf[2] * zzz + qf[3] * xyz + qf[4] * xzz + qf[5] * yzz;
    }
  }
#pragma unroll
  for (int o = PG_LANES / 2; o > 0; o >>= 1) {
    sA += __shfl_xor(sA, o, PG_LANES);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      gA[a] += __shfl_xor(gA[a], o, PG_LANES);
      if constexpr (FV) { hA[a] += __shfl_xor(hA[a], o, PG_LANES); tB[a] += __shfl_xor(tB[a], o, PG_LANES); }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) HB[a] += __shfl_xor(HB[a], o, PG_LANES);
  }
  if (tx != 0 || i0 >= N) return;
  // fractional -> Cartesian, in double: v_cart[b] = sum_a cit[a][b] v_frac[a],  H_cart[b][b'] = sum_aa' cit[a][b] cit[a'][b'] H_frac[a][a']
  double cd[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) cd[k] = (double)c[k];
  const double q = (double)charges[i];
  double cA[3], cF[3];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    cA[b] = cd[b] * (double)gA[0] + cd[3 + b] * (double)gA[1] + cd[6 + b] * (double)gA[2];
    cF[b] = cd[b] * ((double)hA[0] + (double)tB[0]) + cd[3 + b] * ((double)hA[1] + (double)tB[1]) + cd[6 + b] * ((double)hA[2] + (double)tB[2]);
  }
  const double hf[3][3] = {{(double)HB[0], (double)HB[3], (double)HB[4]}, {(double)HB[3], (double)HB[1], (double)HB[5]}, {(double)HB[4], (double)HB[5], (double)HB[2]}};
  double hc[3][3], half[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) half[a][b] = hf[a][0] * cd[b] + hf[a][1] * cd[3 + b] + hf[a][2] * cd[6 + b];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = a; b < 3; ++b) hc[a][b] = hc[b][a] = cd[a] * half[0][b] + cd[3 + a] * half[1][b] + cd[6 + a] * half[2][b];  // symmetric to the bit
  double Q[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) Q[a][b] = 0.5 * ((double)quadrupoles[9 * (size_t)i + 3 * a + b] + (double)quadrupoles[9 * (size_t)i + 3 * b + a]);
  const double al = (double)alpha[s], al3 = al * al * al;
  const double c3 = 4.0 * al3 / (3.0 * 1.7724538509055160273), c5 = 4.0 * al3 * al * al / (5.0 * 1.7724538509055160273);
  const double tr = Q[0][0] + Q[1][1] + Q[2][2];
  const double m[3] = {(double)mu[0], (double)mu[1], (double)mu[2]};
  const double gw = weights ? weights[i] : 1.0;
  const double sc = accumulate ? 1.0 : (weights ? gw : 2.0);
  if (energies) {
    double qq = 0.0, qh = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) { qq += Q[a][b] * Q[a][b]; qh += Q[a][b] * hc[a][b]; }
    energies[i] = q * (double)sA + (m[0] * cA[0] + m[1] * cA[1] + m[2] * cA[2]) + qh + c3 * q * tr - c5 * (2.0 * qq + tr * tr);
  }
  if (cgrads) { const double v = sc * (double)sA; cgrads[i] = accumulate ? cgrads[i] + v : v + gw * c3 * tr; }
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    const size_t o = 3 * (size_t)i + b;
    if (dgrads) { const double v = sc * cA[b]; dgrads[o] = accumulate ? dgrads[o] + v : v; }
    if constexpr (FV) { const double v = -sc * (q * cA[b] + cF[b]); forces[o] = accumulate ? (T)((double)forces[o] + v) : (T)v; }
  }
  if (qgrads) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const size_t o = 9 * (size_t)i + 3 * a + b;
        const double v = sc * hc[a][b];
        qgrads[o] = accumulate ? qgrads[o] + v : v + gw * ((a == b ? c3 * q - 2.0 * c5 * tr : 0.0) - 4.0 * c5 * Q[a][b]);
      }
  }
}

}  // namespace

extern "C" {

int mi_pme_quadrupole_spread(const void* positions, const void* charges, const void* dipoles, const void* quadrupoles, const double* weights,
                             const int32_t* batch_idx, const void* cell_inv_t, int n_atoms, int n_systems, int nx, int ny, int nz, int order, int dtype,
                             void* meshes, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(order >= 5 && order <= MI_MAX_ORDER, "spline order must be 5 or 6 (the quadrupole terms need three continuous derivatives of the spline)");
  MI_REQUIRE(n_systems >= 1 && nx >= order && ny >= order && nz >= order, "every mesh dimension must be at least the spline order");
  MI_REQUIRE(n_atoms >= 0 && meshes && cell_inv_t, "null pointer");
  MI_REQUIRE(n_atoms == 0 || (positions && charges && dipoles && quadrupoles), "null pointer");
  hipStream_t st = (hipStream_t)stream;
  const size_t mesh_bytes = (size_t)n_systems * nx * ny * nz * dtype_bytes(dtype);
  mi_timing_begin("pme_quadrupole_spread", stream);
  MI_HIP_CHECK(hipMemsetAsync(meshes, 0, (weights ? 4 : 2) * mesh_bytes, st));
  if (n_atoms > 0) {
    const int apb = 256 / (order * order);
    MI_DISPATCH_ORDER(order, MI_DISPATCH_T(dtype, (pme_quadrupole_spread_kernel<T_, (O_ < 5 ? 5 : O_)><<<mi_blocks(n_atoms, apb), 256, 0, st>>>(
                                 (const T_*)positions, (const T_*)charges, (const T_*)dipoles, (const T_*)quadrupoles, weights, batch_idx,
                                 (const T_*)cell_inv_t, n_atoms, n_systems, nx, ny, nz, (T_*)meshes))));
  }
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

#define MI_PME_QUADRUPOLE_GATHER(FV_)                                                                                                                  \
  MI_DISPATCH_ORDER(order, MI_DISPATCH_T(dtype, (pme_quadrupole_gather_kernel<T_, (O_ < 5 ? 5 : O_), FV_><<<mi_blocks((long long)n_atoms * PG_LANES, 256), 256, 0, st>>>( \
                               (const T_*)positions, (const T_*)charges, (const T_*)dipoles, (const T_*)quadrupoles, weights, batch_idx,                \
                               (const T_*)cell_inv_t, (const T_*)mesh_a, (const T_*)mesh_b, (const T_*)alpha, n_atoms, nx, ny, nz, accumulate, energies, \
                               (T_*)forces, charge_grads, dipole_grads, quadrupole_grads))))

int mi_pme_quadrupole_gather(const void* positions, const void* charges, const void* dipoles, const void* quadrupoles, const double* weights,
                             const int32_t* batch_idx, const void* cell_inv_t, const void* mesh_a, const void* mesh_b, const void* alpha, int n_atoms,
                             int n_systems, int nx, int ny, int nz, int order, int dtype, int accumulate, double* energies, void* forces,
                             double* charge_grads, double* dipole_grads, double* quadrupole_grads, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(order >= 5 && order <= MI_MAX_ORDER, "spline order must be 5 or 6 (the quadrupole terms need three continuous derivatives of the spline)");
  MI_REQUIRE(n_systems >= 1 && nx >= order && ny >= order && nz >= order, "every mesh dimension must be at least the spline order");
  MI_REQUIRE(!(accumulate && weights), "accumulate (the second launch of the adjoint) takes no weights");
  if (n_atoms <= 0) return MI_OK;
  MI_REQUIRE(positions && charges && dipoles && quadrupoles && cell_inv_t && mesh_a && mesh_b && alpha, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("pme_quadrupole_gather", stream);
  if (forces) MI_PME_QUADRUPOLE_GATHER(true);
  else MI_PME_QUADRUPOLE_GATHER(false);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}
#undef MI_PME_QUADRUPOLE_GATHER

// The k-space virial is the cross form of the dipole section with (rho_l, rho_T) in the places of (rho_q, rho_mu):
//   E_m = h_m G_m (2 Re[conj(rho_l) rho_T] + |rho_T|^2) / sf2_m -- the same kernel.  The caller adds the two terms of the multipoles' fractional
// components, sum_i (dE/dmu_i)_a mu_i,b + 2 sum_i (G_i Q_i)_ab with G_i = dE/dQ_i without its self terms.
int mi_pme_quadrupole_virial(const void* spec_l, const void* spec_t, const void* recip_cell, const void* alpha, const void* volume, int n_systems,
                             int nx, int ny, int nz, int order, int dtype, double* partial /*[n_systems][mi_pme_quadrupole_virial_blocks()][9]*/,
                             void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(order >= 5 && order <= MI_MAX_ORDER, "spline order must be 5 or 6 (the quadrupole terms need three continuous derivatives of the spline)");
  MI_REQUIRE(spec_l && spec_t && recip_cell && alpha && volume && partial && n_systems >= 1 && n_systems <= 65535 && nx > 0 && ny > 0 && nz > 0,
             "null pointer");
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("pme_quadrupole_virial", stream);
  MI_DISPATCH_T(dtype, (pme_dipole_virial_kernel<T_><<<dim3(PME_VIR_BLOCKS, n_systems), 256, 0, st>>>(
                           (const Cplx<T_>*)spec_l, (const Cplx<T_>*)spec_t, (const T_*)recip_cell, (const T_*)alpha, (const T_*)volume, nx, ny, nz, order,
                           partial)));
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}
int mi_pme_quadrupole_virial_blocks(void) { return PME_VIR_BLOCKS; }

}  // extern "C"
