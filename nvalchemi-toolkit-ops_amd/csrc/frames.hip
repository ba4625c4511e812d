// frames.hip -- local-frame multipoles: the rotation of per-atom local dipoles and quadrupoles into the laboratory frame and its adjoint, the
// torque forces on the frame-defining atoms.  gfx950.  Driver: nvalchemiops/interactions/electrostatics/frames.py.  The reference package has no
// counterpart; the frames are Tinker / OpenMM's axis types, written from their definition:
//
//   d_a = r_a - r_i (minimum image when a cell is given) for the frame atoms a = z, x, y of atom i;  n(v) = v / |v|
//   kind         u (e_z = n(u))                 v (the x-like vector)
//   Z_ONLY       d_z                            lab x if |e_z . x^| < 0.866, else lab y (a constant: no gradient)
//   Z_THEN_X     d_z                            d_x
//   BISECTOR     n(d_z) + n(d_x)                d_x
//   Z_BISECT     d_z                            n(n(d_x) + n(d_y))
//   THREE_FOLD   n(d_z) + n(d_x) + n(d_y)       d_x
//   w = v - (v . e_z) e_z,  e_x = n(w),  e_y = e_z x e_x,  R = [e_x e_y e_z] (columns);  NONE: R = I
//   Z_THEN_X with a y atom: sigma = sign(d_y . (d_z x d_x)) mirrors the local y axis (mu_y, Q_xy, Q_yz change sign; a constant for the gradient)
//   mu = R mu_loc,  Q = R Q_loc R^T with Q_loc = 1/2 (Q + Q^T) of what is given
//
// Adjoint of L(mu, Q) with g_mu = dL/dmu, S = 1/2 (g_Q + g_Q^T):  G = dL/dR = g_mu mu_loc^T + 2 S R Q_loc, columns (g_ex, g_ey, g_ez), then
//   g_ez += e_x x g_ey;  g_ex += g_ey x e_z;  g_w = (g_ex - e_x (e_x . g_ex)) / |w|;  g_v = g_w - e_z (e_z . g_w);
//   g_ez -= (v . e_z) g_w + (e_z . g_w) v;  g_u = (g_ez - e_z (e_z . g_ez)) / |u|
// and through u, v of the kind with P(d) g = (g - n(d) (n(d) . g)) / |d|, the adjoint of n(d).  dL/dr_a = dL/dd_a, dL/dr_i = -sum_a dL/dd_a.
//
// Three kernels, one thread per atom, 256 threads per block, every one fp64 whatever the positions dtype, outputs rounded once, no atomics:
//   fr_rotate_kernel   gathers up to three neighbour positions, builds R, writes mu and Q
//   fr_adjoint_kernel  writes the record {-sum_a dL/dd_a, dL/dd_z, dL/dd_x, dL/dd_y} of the atom (zeros for slots its kind does not use), on
//                      request R^T g_mu, R^T S R and the nine virial words -sum_a (dL/dd_a)[p] d_a[q] (row-major)
//   fr_gather_kernel   sums the atom's own slot 0 and the slots the inverse CSR lists for it, in the stored order
// and the per-system fold of the virial rows is pair_row.h's.
#include "common.h"

namespace {

#include "pair_row.h"  // the fixed-order per-system fold

constexpr int FR_THREADS = 256;
constexpr int FR_NONE = 0, FR_Z_ONLY = 1, FR_Z_THEN_X = 2, FR_BISECTOR = 3, FR_Z_BISECT = 4, FR_THREE_FOLD = 5;
constexpr double FR_Z_ONLY_SWITCH = 0.866;
constexpr int FR_VIR_WORDS = 9;
constexpr int FR_REC_WORDS = 12;  // four 3-vectors: self, z, x, y

struct V3 { double x, y, z; };
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 unit(V3 a) { return (1.0 / sqrt(dot(a, a))) * a; }
// the adjoint of n(d) = d / |d| applied to g
__device__ __forceinline__ V3 unit_adjoint(V3 d, V3 g) {
  const double inv = 1.0 / sqrt(dot(d, d));
  const V3 n = inv * d;
  return inv * (g - dot(n, g) * n);
}
template <class T> __device__ __forceinline__ V3 load3(const T* __restrict__ p, size_t i) {
  return {(double)p[3 * i], (double)p[3 * i + 1], (double)p[3 * i + 2]};
}
__device__ __forceinline__ void store3(double* __restrict__ p, V3 a) { p[0] = a.x; p[1] = a.y; p[2] = a.z; }

// the cell of the atom's system and its inverse, fp64 (row vectors: fractional = d . cell^-1)
struct Cell { double m[9], inv[9]; };
template <class T> __device__ __forceinline__ void load_cell(const T* __restrict__ cell, int s, Cell& c) {
#pragma unroll
  for (int k = 0; k < 9; ++k) c.m[k] = (double)cell[9 * (size_t)s + k];
  inverse3(c.m, c.inv);
}
// d_a = r_a - r_i, the minimum image with a cell; zero for a slot that names no atom of [0, N)
template <class T> __device__ __forceinline__ V3 frame_vector(const T* __restrict__ pos, int i, int a, int N, bool periodic, const Cell& c) {
  if ((unsigned)a >= (unsigned)N) return {0.0, 0.0, 0.0};
  V3 d = load3(pos, (size_t)a) - load3(pos, (size_t)i);
  if (periodic) {
    const double n0 = rint(d.x * c.inv[0] + d.y * c.inv[3] + d.z * c.inv[6]);
    const double n1 = rint(d.x * c.inv[1] + d.y * c.inv[4] + d.z * c.inv[7]);
    const double n2 = rint(d.x * c.inv[2] + d.y * c.inv[5] + d.z * c.inv[8]);
    d.x -= n0 * c.m[0] + n1 * c.m[3] + n2 * c.m[6];
    d.y -= n0 * c.m[1] + n1 * c.m[4] + n2 * c.m[7];
    d.z -= n0 * c.m[2] + n1 * c.m[5] + n2 * c.m[8];
  }
  return d;
}

// what both kernels need of atom i's frame
struct Frame {
  int kind;
  V3 dz, dx, dy;   // frame vectors (zero for an unused slot)
  V3 v;            // the x-like vector before orthogonalising
  V3 ex, ey, ez;   // the columns of R
  double inv_u, inv_w;  // 1 / |u|, 1 / |w|
  double sigma;    // +1, or -1 for a mirrored local y axis
};

template <class T>
__device__ __forceinline__ void frame_build(const T* __restrict__ pos, const int* __restrict__ atoms, const int* __restrict__ kinds,
                                            const T* __restrict__ cell, const int* __restrict__ batch_idx, int nsys, int i, int N, Frame& f) {
  f.kind = kinds[i];
  f.sigma = 1.0;
  f.inv_u = f.inv_w = 0.0;
  f.dz = f.dx = f.dy = f.v = {0.0, 0.0, 0.0};
  f.ex = {1.0, 0.0, 0.0}; f.ey = {0.0, 1.0, 0.0}; f.ez = {0.0, 0.0, 1.0};
  if (f.kind < FR_Z_ONLY || f.kind > FR_THREE_FOLD) { f.kind = FR_NONE; return; }
  Cell c;
  const bool periodic = cell != nullptr;
  if (periodic) {
    const int s = batch_idx ? batch_idx[i] : 0;
    load_cell(cell, (unsigned)s < (unsigned)nsys ? s : 0, c);
  }
  f.dz = frame_vector(pos, i, atoms[3 * (size_t)i], N, periodic, c);
  f.dx = frame_vector(pos, i, atoms[3 * (size_t)i + 1], N, periodic, c);
  f.dy = frame_vector(pos, i, atoms[3 * (size_t)i + 2], N, periodic, c);
  V3 u = f.dz;
  if (f.kind == FR_BISECTOR) u = unit(f.dz) + unit(f.dx);
  if (f.kind == FR_THREE_FOLD) u = unit(f.dz) + unit(f.dx) + unit(f.dy);
  f.inv_u = 1.0 / sqrt(dot(u, u));
  f.ez = f.inv_u * u;
  f.v = f.dx;
  if (f.kind == FR_Z_ONLY) f.v = fabs(f.ez.x) < FR_Z_ONLY_SWITCH ? V3{1.0, 0.0, 0.0} : V3{0.0, 1.0, 0.0};
  if (f.kind == FR_Z_BISECT) f.v = unit(unit(f.dx) + unit(f.dy));
  const V3 w = f.v - dot(f.v, f.ez) * f.ez;
  f.inv_w = 1.0 / sqrt(dot(w, w));
  f.ex = f.inv_w * w;
  f.ey = cross(f.ez, f.ex);
  if (f.kind == FR_Z_THEN_X && (unsigned)atoms[3 * (size_t)i + 2] < (unsigned)N && dot(f.dy, cross(f.dz, f.dx)) < 0.0) f.sigma = -1.0;
}

// the local multipoles as the rotation uses them: the mirrored y components, 1/2 (Q + Q^T) as {xx, yy, zz, xy, xz, yz}
template <class T>
__device__ __forceinline__ void load_local(const T* __restrict__ mu_loc, const T* __restrict__ q_loc, int i, double sigma, V3& m, double q[6]) {
  m = {0.0, 0.0, 0.0};
  if (mu_loc) { m = load3(mu_loc, (size_t)i); m.y *= sigma; }
#pragma unroll
  for (int k = 0; k < 6; ++k) q[k] = 0.0;
  if (q_loc) {
    const T* p = q_loc + 9 * (size_t)i;
    q[0] = (double)p[0]; q[1] = (double)p[4]; q[2] = (double)p[8];
    q[3] = sigma * 0.5 * ((double)p[1] + (double)p[3]);
    q[4] = 0.5 * ((double)p[2] + (double)p[6]);
    q[5] = sigma * 0.5 * ((double)p[5] + (double)p[7]);
  }
}

template <class T>
__global__ __launch_bounds__(FR_THREADS) void fr_rotate_kernel(const T* __restrict__ pos, const T* __restrict__ mu_loc, const T* __restrict__ q_loc,
                                                               const int* __restrict__ atoms, const int* __restrict__ kinds,
                                                               const T* __restrict__ cell, const int* __restrict__ batch_idx, int nsys, int N,
                                                               T* __restrict__ mu, T* __restrict__ quad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  Frame f;
  frame_build(pos, atoms, kinds, cell, batch_idx, nsys, i, N, f);
  V3 m;
  double q[6];
  load_local(mu_loc, q_loc, i, f.sigma, m, q);
  if (mu) {
    const V3 r = m.x * f.ex + m.y * f.ey + m.z * f.ez;
    T* o = mu + 3 * (size_t)i;
    o[0] = (T)r.x; o[1] = (T)r.y; o[2] = (T)r.z;
  }
  if (quad) {
    // t_k = R Q_loc[:, k]; Q = sum_k t_k (column k of R)^T, symmetric
    const V3 t0 = q[0] * f.ex + q[3] * f.ey + q[4] * f.ez;
    const V3 t1 = q[3] * f.ex + q[1] * f.ey + q[5] * f.ez;
    const V3 t2 = q[4] * f.ex + q[5] * f.ey + q[2] * f.ez;
    const V3 r0 = f.ex.x * t0 + f.ey.x * t1 + f.ez.x * t2;  // column 0 of Q
    const V3 r1 = f.ex.y * t0 + f.ey.y * t1 + f.ez.y * t2;
    const V3 r2 = f.ex.z * t0 + f.ey.z * t1 + f.ez.z * t2;
    T* o = quad + 9 * (size_t)i;
    const double xy = 0.5 * (r1.x + r0.y), xz = 0.5 * (r2.x + r0.z), yz = 0.5 * (r2.y + r1.z);
    o[0] = (T)r0.x; o[1] = (T)xy; o[2] = (T)xz;
    o[3] = (T)xy; o[4] = (T)r1.y; o[5] = (T)yz;
    o[6] = (T)xz; o[7] = (T)yz; o[8] = (T)r2.z;
  }
}

template <class T>
__global__ __launch_bounds__(FR_THREADS) void fr_adjoint_kernel(const T* __restrict__ pos, const T* __restrict__ mu_loc, const T* __restrict__ q_loc,
                                                                const int* __restrict__ atoms, const int* __restrict__ kinds,
                                                                const T* __restrict__ cell, const int* __restrict__ batch_idx,
                                                                const T* __restrict__ g_mu, const T* __restrict__ g_quad, int nsys, int N,
                                                                double* __restrict__ rec, double* __restrict__ mu_grads,
                                                                double* __restrict__ quad_grads, double* __restrict__ vrow) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  Frame f;
  frame_build(pos, atoms, kinds, cell, batch_idx, nsys, i, N, f);
  V3 m;
  double q[6];
  load_local(mu_loc, q_loc, i, f.sigma, m, q);
  const V3 gm = (g_mu && mu_loc) ? load3(g_mu, (size_t)i) : V3{0.0, 0.0, 0.0};
  // S = 1/2 (g_Q + g_Q^T) by rows; sr_k = S (column k of R)
  V3 s0 = {0.0, 0.0, 0.0}, s1 = s0, s2 = s0;
  if (g_quad && q_loc) {
    const T* p = g_quad + 9 * (size_t)i;
    const double xy = 0.5 * ((double)p[1] + (double)p[3]), xz = 0.5 * ((double)p[2] + (double)p[6]), yz = 0.5 * ((double)p[5] + (double)p[7]);
    s0 = {(double)p[0], xy, xz}; s1 = {xy, (double)p[4], yz}; s2 = {xz, yz, (double)p[8]};
  }
  const V3 srx = {dot(s0, f.ex), dot(s1, f.ex), dot(s2, f.ex)};
  const V3 sry = {dot(s0, f.ey), dot(s1, f.ey), dot(s2, f.ey)};
  const V3 srz = {dot(s0, f.ez), dot(s1, f.ez), dot(s2, f.ez)};
  if (mu_grads) {
    double* o = mu_grads + 3 * (size_t)i;
    o[0] = dot(f.ex, gm); o[1] = f.sigma * dot(f.ey, gm); o[2] = dot(f.ez, gm);
  }
  if (quad_grads) {
    double* o = quad_grads + 9 * (size_t)i;
    const double xy = f.sigma * dot(f.ex, sry), xz = dot(f.ex, srz), yz = f.sigma * dot(f.ey, srz);
    o[0] = dot(f.ex, srx); o[1] = xy; o[2] = xz;
    o[3] = xy; o[4] = dot(f.ey, sry); o[5] = yz;
    o[6] = xz; o[7] = yz; o[8] = dot(f.ez, srz);
  }
  V3 gz = {0.0, 0.0, 0.0}, gx = gz, gy = gz;
  if (f.kind != FR_NONE) {
    // G = g_mu mu_loc^T + 2 (S R) Q_loc by columns
    V3 g_ex = m.x * gm + 2.0 * (q[0] * srx + q[3] * sry + q[4] * srz);
    const V3 g_ey = m.y * gm + 2.0 * (q[3] * srx + q[1] * sry + q[5] * srz);
    V3 g_ez = m.z * gm + 2.0 * (q[4] * srx + q[5] * sry + q[2] * srz);
    g_ez = g_ez + cross(f.ex, g_ey);
    g_ex = g_ex + cross(g_ey, f.ez);
    const V3 g_w = f.inv_w * (g_ex - dot(f.ex, g_ex) * f.ex);
    const double wz = dot(f.ez, g_w);
    const V3 g_v = g_w - wz * f.ez;
    g_ez = g_ez - (dot(f.v, f.ez) * g_w + wz * f.v);
    const V3 g_u = f.inv_u * (g_ez - dot(f.ez, g_ez) * f.ez);
    if (f.kind == FR_Z_ONLY) {
      gz = g_u;
    } else if (f.kind == FR_Z_THEN_X) {
      gz = g_u; gx = g_v;
    } else if (f.kind == FR_BISECTOR) {
      gz = unit_adjoint(f.dz, g_u);
      gx = g_v + unit_adjoint(f.dx, g_u);
    } else if (f.kind == FR_Z_BISECT) {
      gz = g_u;
      const V3 g_s = unit_adjoint(unit(f.dx) + unit(f.dy), g_v);
      gx = unit_adjoint(f.dx, g_s);
      gy = unit_adjoint(f.dy, g_s);
    } else {  // FR_THREE_FOLD
      gz = unit_adjoint(f.dz, g_u);
      gx = g_v + unit_adjoint(f.dx, g_u);
      gy = unit_adjoint(f.dy, g_u);
    }
  }
  double* r = rec + FR_REC_WORDS * (size_t)i;
  store3(r, -1.0 * (gz + gx + gy));
  store3(r + 3, gz);
  store3(r + 6, gx);
  store3(r + 9, gy);
  if (vrow) {
    double* o = vrow + FR_VIR_WORDS * (size_t)i;
    store3(o, -1.0 * (gz.x * f.dz + gx.x * f.dx + gy.x * f.dy));
    store3(o + 3, -1.0 * (gz.y * f.dz + gx.y * f.dx + gy.y * f.dy));
    store3(o + 6, -1.0 * (gz.z * f.dz + gx.z * f.dx + gy.z * f.dy));
  }
}

// out[i] = sign (rec[i][0] + sum over the inverse row of i of rec[entry]), entry = 4 atom + 1 + slot, in the stored order
template <class TO>
__global__ __launch_bounds__(FR_THREADS) void fr_gather_kernel(const double* __restrict__ rec, const int* __restrict__ iptr,
                                                               const int* __restrict__ islots, int N, long long E, double sign,
                                                               TO* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  V3 a = load3(rec, 4 * (size_t)i);
  long long beg = iptr[i], end = iptr[i + 1];
  if (beg < 0) beg = 0;
  if (end > E) end = E;
  for (long long e = beg; e < end; ++e) {
    const int code = islots[e];
    if ((unsigned)code < 4u * (unsigned)N) a = a + load3(rec, (size_t)code);
  }
  TO* o = out + 3 * (size_t)i;
  o[0] = (TO)(sign * a.x); o[1] = (TO)(sign * a.y); o[2] = (TO)(sign * a.z);
}

// per-system fold of the per-atom virial rows: partial[s][x][0..9) with plain stores; the caller sums the MI_FOLD_BLOCKS rows.  No atomics.
__global__ __launch_bounds__(256) void fr_fold_kernel(const double* __restrict__ vrow, const int* __restrict__ batch_idx, int N,
                                                      double* __restrict__ partial) {
  mi_system_fold<FR_VIR_WORDS, MI_FOLD_BLOCKS>(batch_idx, N, FR_VIR_WORDS, partial, [&](long long r, double* a) {
#pragma unroll
    for (int k = 0; k < FR_VIR_WORDS; ++k) a[k] += vrow[FR_VIR_WORDS * r + k];
  });
}

}  // namespace

extern "C" {

int mi_frame_blocks(void) { return MI_FOLD_BLOCKS; }
int mi_frame_block_threads(void) { return FR_THREADS; }

int mi_frame_rotate(const void* positions, const void* local_dipoles, const void* local_quadrupoles, const int32_t* frame_atoms,
                    const int32_t* frame_kinds, const void* cell, const int32_t* batch_idx, int n_atoms, int n_systems, int dtype, void* dipoles,
                    void* quadrupoles, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  MI_REQUIRE(n_atoms >= 0 && n_atoms <= (1 << 29), "n_atoms must be in [0, 2^29]");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && frame_atoms && frame_kinds, "null pointer");
  MI_REQUIRE((local_dipoles != nullptr) == (dipoles != nullptr), "dipoles is written exactly when local_dipoles is given");
  MI_REQUIRE((local_quadrupoles != nullptr) == (quadrupoles != nullptr), "quadrupoles is written exactly when local_quadrupoles is given");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(n_systems == 1 || (batch_idx && cell), "more than one system needs cell and batch_idx");
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("frame_rotate", stream);
  if (dtype == MI_F32)
    fr_rotate_kernel<float><<<mi_blocks(n_atoms, FR_THREADS), FR_THREADS, 0, st>>>(
        (const float*)positions, (const float*)local_dipoles, (const float*)local_quadrupoles, frame_atoms, frame_kinds, (const float*)cell,
        cell ? batch_idx : nullptr, n_systems, n_atoms, (float*)dipoles, (float*)quadrupoles);
  else
    fr_rotate_kernel<double><<<mi_blocks(n_atoms, FR_THREADS), FR_THREADS, 0, st>>>(
        (const double*)positions, (const double*)local_dipoles, (const double*)local_quadrupoles, frame_atoms, frame_kinds, (const double*)cell,
        cell ? batch_idx : nullptr, n_systems, n_atoms, (double*)dipoles, (double*)quadrupoles);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_frame_adjoint(const void* positions, const void* local_dipoles, const void* local_quadrupoles, const int32_t* frame_atoms,
                     const int32_t* frame_kinds, const void* cell, const int32_t* batch_idx, const void* dipole_grads,
                     const void* quadrupole_grads, int n_atoms, int n_systems, int dtype, double* records, double* local_dipole_grads,
                     double* local_quadrupole_grads, double* virial_rows, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  MI_REQUIRE(n_atoms >= 0 && n_atoms <= (1 << 29), "n_atoms must be in [0, 2^29]");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && frame_atoms && frame_kinds && records, "null pointer");
  MI_REQUIRE(!local_dipole_grads || (local_dipoles && dipole_grads), "local_dipole_grads needs local_dipoles and dipole_grads");
  MI_REQUIRE(!local_quadrupole_grads || (local_quadrupoles && quadrupole_grads), "local_quadrupole_grads needs local_quadrupoles and quadrupole_grads");
  MI_REQUIRE(!virial_rows || cell, "the virial needs a cell");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(n_systems == 1 || (batch_idx && cell), "more than one system needs cell and batch_idx");
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("frame_adjoint", stream);
  if (dtype == MI_F32)
    fr_adjoint_kernel<float><<<mi_blocks(n_atoms, FR_THREADS), FR_THREADS, 0, st>>>(
        (const float*)positions, (const float*)local_dipoles, (const float*)local_quadrupoles, frame_atoms, frame_kinds, (const float*)cell,
        cell ? batch_idx : nullptr, (const float*)dipole_grads, (const float*)quadrupole_grads, n_systems, n_atoms, records, local_dipole_grads,
        local_quadrupole_grads, virial_rows);
  else
    fr_adjoint_kernel<double><<<mi_blocks(n_atoms, FR_THREADS), FR_THREADS, 0, st>>>(
        (const double*)positions, (const double*)local_dipoles, (const double*)local_quadrupoles, frame_atoms, frame_kinds, (const double*)cell,
        cell ? batch_idx : nullptr, (const double*)dipole_grads, (const double*)quadrupole_grads, n_systems, n_atoms, records, local_dipole_grads,
        local_quadrupole_grads, virial_rows);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

int mi_frame_gather(const double* records, const int32_t* inverse_ptr, const int32_t* inverse_slots, long long n_entries,
                    const double* virial_rows, const int32_t* batch_idx, int n_atoms, int n_systems, int dtype, double sign, void* out,
                    double* virial_partial, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  MI_REQUIRE(n_atoms >= 0 && n_atoms <= (1 << 29), "n_atoms must be in [0, 2^29]");
  MI_REQUIRE(n_entries >= 0, "n_entries must not be negative");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(records && inverse_ptr && out, "null pointer");
  MI_REQUIRE(n_entries == 0 || inverse_slots, "null pointer");
  MI_REQUIRE((virial_rows != nullptr) == (virial_partial != nullptr), "virial_rows and virial_partial go together");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(n_systems == 1 || batch_idx, "more than one system needs batch_idx");
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("frame_gather", stream);
  if (dtype == MI_F32)
    fr_gather_kernel<float><<<mi_blocks(n_atoms, FR_THREADS), FR_THREADS, 0, st>>>(records, inverse_ptr, inverse_slots, n_atoms, n_entries, sign,
                                                                                     (float*)out);
  else
    fr_gather_kernel<double><<<mi_blocks(n_atoms, FR_THREADS), FR_THREADS, 0, st>>>(records, inverse_ptr, inverse_slots, n_atoms, n_entries, sign,
                                                                                      (double*)out);
  if (virial_rows)
    fr_fold_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>(virial_rows, n_systems > 1 ? batch_idx : nullptr, n_atoms, virial_partial);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

}  // extern "C"
