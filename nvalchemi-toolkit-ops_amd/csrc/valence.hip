// valence.hip -- the bonded (valence) terms of an AMOEBA-class or fixed-charge force field: bond stretch, angle bend, stretch-bend, out-of-plane
// bend and Fourier torsion.  gfx950.  Driver: nvalchemiops/interactions/valence.  The reference package has no counterpart; the definitions are
// Tinker's, written from their formulas (angles in radians, no 1/2 in front of any force constant):
//
//   kind           atoms (A)          difference vectors                      E_t
//   BOND           a b      (2)       d = r_a - r_b                           k D^2 (1 + c3 D + c4 D^2),                   D = |d| - r0
//   ANGLE          a b c    (3)       u = r_a - r_b, v = r_c - r_b            k D^2 (1 + c3 D + c4 D^2 + c5 D^3 + c6 D^4), D = theta - theta0
//   STRETCH_BEND   a b c    (3)       u, v                                    (k1 (|u| - r1) + k2 (|v| - r2)) (theta - theta0)
//   OUT_OF_PLANE   a b c d  (4)       u, v, w = r_d - r_b                     k X^2 (1 + c3 X + ... + c6 X^4),  X = asin(|V| / sqrt(cc |w|^2)),
//                                                                             V = w . (u x v);  cc = |u x v|^2 (W-D-C) or |(u - w) x (v - w)|^2 (Allinger)
//   TORSION        a b c d  (4)       b1 = r_b - r_a, b2 = r_c - r_b,         sum_{n=1..F} V_n (1 + cos(n phi - gamma_n)),
//                                     b3 = r_d - r_c                          phi = atan2(|b2| b1 . n, m . n), m = b1 x b2, n = b2 x b3 (trans = pi)
//
// Every kind is a function of its A - 1 difference vectors (minimum images when a cell is given), so each computes dE/d(vector) once; the
// atom gradients are the fixed linear map of the table above applied to them and the virial is -sum_v dE/dv (x) v.
//   theta = atan2(|u x v|, u . v);  dtheta/du = u x (u x v) / (|u|^2 |u x v|),  dtheta/dv = (u x v) x v / (|v|^2 |u x v|)
//   dphi/db1 = |b2| m / |m|^2,  dphi/db3 = |b2| n / |n|^2,  dphi/db2 = -(b1 . b2) m / (|m|^2 |b2|) - (b2 . b3) n / (|n|^2 |b2|)
//   cos n phi, sin n phi by the angle-addition recurrence from (cos phi, sin phi) = (m . n, |b2| b1 . n) / (|m| |n|); the phases enter as
//   sincos(gamma_n), a call on the parameter and none on n phi
//   s = sin X = |V| / sqrt(cc ww):  ds = sign(V) dV / sqrt(cc ww) - s/2 (dcc / cc + dww / ww),  dX = ds / cos X
//
// Three kernels, 256 threads per block, fp64 arithmetic whatever the positions dtype, outputs rounded once, no atomics:
//   va_term_kernel    one thread per term: gathers the A positions, writes the term energy, the gradient record (A 3-vectors, as planes
//                     [A][3][T] so that a wave stores 64 consecutive words per plane), the [P] parameter gradients and on request the nine
//                     virial words and the system of the term.  Templated on (kind, positions dtype, flag set): a pass nobody asked for costs no
//                     registers.  A term that names an atom outside [0, N) writes zeros everywhere.
//   va_gather_kernel  one thread per atom: sums the slots slot_idx[slot_ptr[i] .. slot_ptr[i + 1]) (slot = t A + p) in the stored order into
//                     the force and the energy share E_t / A
//   va_fold_kernel    pair_row.h's fixed-order per-system fold of the virial words
// With weights g (the adjoint of L = sum_i g_i E_i) every derivative of term t is scaled by w_t = (1 / A) sum_{a in t} g_a.
#include "common.h"

namespace {

#include "pair_row.h"  // the fixed-order per-system fold

constexpr int VA_THREADS = 256;
constexpr int VA_VIR_WORDS = 9;
constexpr int VA_MAX_FOLDS = 6;

__host__ __device__ constexpr int va_arity(int kind) { return kind == MI_VALENCE_BOND ? 2 : (kind == MI_VALENCE_ANGLE || kind == MI_VALENCE_STRETCH_BEND) ? 3 : 4; }

struct V3 { double x, y, z; };
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
template <class T> __device__ __forceinline__ V3 load3(const T* __restrict__ p, size_t i) {
  return {(double)p[3 * i], (double)p[3 * i + 1], (double)p[3 * i + 2]};
}

// what a launch passes to the term kernel
struct VaArgs {
  const void* pos; const int* atoms; const void* par; const void* cell; const int* batch; const double* weights;
  int P, N, T, nsys, plane;
  double c3, c4, c5, c6;
  size_t plane_stride, term_stride;  // word (p, c) of term t of the record sits at (3 p + c) * plane_stride + t * term_stride
  double* et; double* rec; double* pgrads; double* vir; int* tsys;
};

// the cell of the term's system and its inverse, fp64 (row vectors: fractional = d . cell^-1)
struct Cell { double m[9], inv[9]; };
__device__ __forceinline__ V3 min_image(V3 d, bool periodic, const Cell& c) {
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

// E = k D^2 (1 + c3 D + c4 D^2 + c5 D^3 + c6 D^4): shape = E / k and dshape = d(E / k)/dD, powers by multiplication
__device__ __forceinline__ void anharmonic(double D, double c3, double c4, double c5, double c6, double& shape, double& dshape) {
  const double D2 = D * D, D3 = D2 * D, D4 = D2 * D2;
  shape = D2 * (1.0 + c3 * D + c4 * D2 + c5 * D3 + c6 * D4);
  dshape = D * (2.0 + 3.0 * c3 * D + 4.0 * c4 * D2 + 5.0 * c5 * D3 + 6.0 * c6 * D4);
}

// theta = angle(u, v) from one atan2, with its gradients
__device__ __forceinline__ double angle_of(V3 u, V3 v, V3& dtu, V3& dtv) {
  const V3 n = cross(u, v);
  const double nn = sqrt(dot(n, n));
  dtu = (1.0 / (dot(u, u) * nn)) * cross(u, n);
  dtv = (1.0 / (dot(v, v) * nn)) * cross(n, v);
  return atan2(nn, dot(u, v));
}

// Each term function takes the A - 1 difference vectors d[], the parameter row p (positions dtype) and returns E_t; with GRAD it fills the
// gradients g[] w.r.t. the vectors, with PG it writes w dE/dparameter to pg[0..P).
template <bool GRAD, bool PG, class T>
__device__ __forceinline__ double term_bond(const V3* d, const T* __restrict__ p, const VaArgs& a, double w, V3* g, double* __restrict__ pg) {
  const double k = (double)p[0], r0 = (double)p[1];
  const double r = sqrt(dot(d[0], d[0]));
  double shape, dshape;
  anharmonic(r - r0, a.c3, a.c4, 0.0, 0.0, shape, dshape);
  if (GRAD) g[0] = (w * k * dshape / r) * d[0];
  if (PG) { pg[0] = w * shape; pg[1] = -w * k * dshape; }
  return k * shape;
}

template <bool GRAD, bool PG, class T>
__device__ __forceinline__ double term_angle(const V3* d, const T* __restrict__ p, const VaArgs& a, double w, V3* g, double* __restrict__ pg) {
  const double k = (double)p[0], t0 = (double)p[1];
  V3 dtu, dtv;
  const double theta = angle_of(d[0], d[1], dtu, dtv);
  double shape, dshape;
  anharmonic(theta - t0, a.c3, a.c4, a.c5, a.c6, shape, dshape);
  if (GRAD) { g[0] = (w * k * dshape) * dtu; g[1] = (w * k * dshape) * dtv; }
  if (PG) { pg[0] = w * shape; pg[1] = -w * k * dshape; }
  return k * shape;
}

template <bool GRAD, bool PG, class T>
__device__ __forceinline__ double term_stretch_bend(const V3* d, const T* __restrict__ p, const VaArgs& a, double w, V3* g, double* __restrict__ pg) {
  const double k1 = (double)p[0], k2 = (double)p[1], r1 = (double)p[2], r2 = (double)p[3], t0 = (double)p[4];
  V3 dtu, dtv;
  const double theta = angle_of(d[0], d[1], dtu, dtv);
  const double ru = sqrt(dot(d[0], d[0])), rv = sqrt(dot(d[1], d[1]));
  const double D1 = ru - r1, D2 = rv - r2, Dt = theta - t0;
  const double S = k1 * D1 + k2 * D2;
  if (GRAD) {
    g[0] = w * ((k1 * Dt / ru) * d[0] + S * dtu);
    g[1] = w * ((k2 * Dt / rv) * d[1] + S * dtv);
  }
  if (PG) { pg[0] = w * D1 * Dt; pg[1] = w * D2 * Dt; pg[2] = -w * k1 * Dt; pg[3] = -w * k2 * Dt; pg[4] = -w * S; }
  return S * Dt;
}

template <bool GRAD, bool PG, class T>
__device__ __forceinline__ double term_out_of_plane(const V3* d, const T* __restrict__ p, const VaArgs& a, double w, V3* g, double* __restrict__ pg) {
  const double k = (double)p[0];
  const V3 u = d[0], v = d[1], ww = d[2];
  const V3 uv = cross(u, v);
  const double V = dot(ww, uv);
  const bool allinger = a.plane == MI_VALENCE_PLANE_ALLINGER;
  // cc = |x|^2 |y|^2 - (x . y)^2 of the two in-plane vectors: (u, v), or (u - w, v - w)
  const V3 x = allinger ? u - ww : u, y = allinger ? v - ww : v;
  const double xx = dot(x, x), yy = dot(y, y), xy = dot(x, y);
  const double cc = xx * yy - xy * xy, w2 = dot(ww, ww);
  const double inv_root = 1.0 / sqrt(cc * w2);
  const double s = fmin(fabs(V) * inv_root, 1.0);
  const double chi = asin(s);
  double shape, dshape;
  anharmonic(chi, a.c3, a.c4, a.c5, a.c6, shape, dshape);
  if (GRAD) {
    if (V == 0.0) {
      g[0] = g[1] = g[2] = {0.0, 0.0, 0.0};
    } else {
      const double dEds = w * k * dshape / sqrt(fmax(1.0 - s * s, 0.0));  // dE/dX / cos X
      const double fV = dEds * (V > 0.0 ? inv_root : -inv_root), fc = -dEds * s / cc, fw = -dEds * s / w2;  // dE/dV, dE/dcc * 2, dE/dww * 2
      const V3 gx = fc * (yy * x - xy * y), gy = fc * (xx * y - xy * x);  // 1/2 dcc/dx = yy x - xy y
      g[0] = fV * cross(v, ww) + gx;
      g[1] = fV * cross(ww, u) + gy;
      g[2] = fV * uv + fw * ww;
      if (allinger) g[2] = g[2] - (gx + gy);
    }
  }
  if (PG) pg[0] = w * shape;
  return k * shape;
}

template <bool GRAD, bool PG, class T>
__device__ __forceinline__ double term_torsion(const V3* d, const T* __restrict__ p, const VaArgs& a, double w, V3* g, double* __restrict__ pg) {
  const V3 b1 = d[0], b2 = d[1], b3 = d[2];
  const V3 m = cross(b1, b2), n = cross(b2, b3);
  const double mm = dot(m, m), nn = dot(n, n), b22 = dot(b2, b2), lb2 = sqrt(b22);
  const double inv_mn = 1.0 / sqrt(mm * nn);
  const double c1 = dot(m, n) * inv_mn, s1 = lb2 * dot(b1, n) * inv_mn;
  const int F = a.P / 2;
  double e = 0.0, dEdphi = 0.0, cn = 1.0, sn = 0.0;
#pragma unroll
  for (int f = 0; f < VA_MAX_FOLDS; ++f) {
    if (f < F) {
      const double c = cn * c1 - sn * s1;  // cos (f + 1) phi, sin (f + 1) phi
      sn = sn * c1 + cn * s1;
      cn = c;
      const double Vn = (double)p[f];
      double sg, cg;
      sincos((double)p[F + f], &sg, &cg);
      const double cosd = cn * cg + sn * sg, sind = sn * cg - cn * sg;  // cos, sin of (n phi - gamma)
      e += Vn * (1.0 + cosd);
      dEdphi -= (double)(f + 1) * Vn * sind;
      if (PG) { pg[f] = w * (1.0 + cosd); pg[F + f] = w * Vn * sind; }
    }
  }
  if (GRAD) {
    const double q = w * dEdphi;
    g[0] = (q * lb2 / mm) * m;
    g[2] = (q * lb2 / nn) * n;
    g[1] = (-q * dot(b1, b2) / (mm * lb2)) * m + (-q * dot(b2, b3) / (nn * lb2)) * n;
  }
  return e;
}

template <int KIND, class T, int FLAGS>
__global__ __launch_bounds__(VA_THREADS) void va_term_kernel(VaArgs a) {
  constexpr int A = va_arity(KIND);
  constexpr bool FORCES = FLAGS & MI_VALENCE_FORCES, PG = FLAGS & MI_VALENCE_PARAMETER_GRAD, VIRIAL = FLAGS & MI_VALENCE_VIRIAL;
  constexpr bool GRAD = FORCES || VIRIAL;
  const int t = blockIdx.x * VA_THREADS + threadIdx.x;
  if (t >= a.T) return;
  const T* pos = (const T*)a.pos;
  int idx[A];
  bool ok = true;
#pragma unroll
  for (int p = 0; p < A; ++p) {
    idx[p] = a.atoms[A * (size_t)t + p];
    ok = ok && (unsigned)idx[p] < (unsigned)a.N;
  }
  double e = 0.0;
  V3 g[A - 1], d[A - 1];
#pragma unroll
  for (int k = 0; k < A - 1; ++k) g[k] = d[k] = {0.0, 0.0, 0.0};
  double* pg = PG ? a.pgrads + (size_t)a.P * t : nullptr;
  int sys = 0;
  if (ok) {
    V3 r[A];
#pragma unroll
    for (int p = 0; p < A; ++p) r[p] = load3(pos, (size_t)idx[p]);
    Cell c;
    const bool periodic = a.cell != nullptr;
    if (periodic) {
      const int s = a.batch ? a.batch[idx[0]] : 0;
      sys = (unsigned)s < (unsigned)a.nsys ? s : 0;
#pragma unroll
      for (int k = 0; k < 9; ++k) c.m[k] = (double)((const T*)a.cell)[9 * (size_t)sys + k];
      inverse3(c.m, c.inv);
    }
    if (KIND == MI_VALENCE_TORSION) {
#pragma unroll
      for (int k = 0; k < A - 1; ++k) d[k] = min_image(r[k + 1] - r[k], periodic, c);
    } else {  // every vector points away from atom 1 (b): the other end of the bond, the vertex, the centre
      d[0] = min_image(r[0] - r[1], periodic, c);
#pragma unroll
      for (int k = 1; k < A - 1; ++k) d[k] = min_image(r[k + 1] - r[1], periodic, c);
    }
    double w = 1.0;
    if (a.weights) {
      w = 0.0;
#pragma unroll
      for (int p = 0; p < A; ++p) w += a.weights[idx[p]];
      w *= 1.0 / A;
    }
    const T* par = (const T*)a.par + (size_t)a.P * t;
    if (KIND == MI_VALENCE_BOND) e = term_bond<GRAD, PG>(d, par, a, w, g, pg);
    if (KIND == MI_VALENCE_ANGLE) e = term_angle<GRAD, PG>(d, par, a, w, g, pg);
    if (KIND == MI_VALENCE_STRETCH_BEND) e = term_stretch_bend<GRAD, PG>(d, par, a, w, g, pg);
    if (KIND == MI_VALENCE_OUT_OF_PLANE) e = term_out_of_plane<GRAD, PG>(d, par, a, w, g, pg);
    if (KIND == MI_VALENCE_TORSION) e = term_torsion<GRAD, PG>(d, par, a, w, g, pg);
  } else if (PG) {
    for (int k = 0; k < a.P; ++k) pg[k] = 0.0;
  }
  a.et[t] = e;
  if (FORCES) {
    // the atom gradients from the vector gradients
    V3 ga[A];
    if (KIND == MI_VALENCE_TORSION) {
      ga[0] = -1.0 * g[0]; ga[1] = g[0] - g[1]; ga[2] = g[1] - g[2]; ga[3] = g[2];
    } else {
      ga[0] = g[0];
      V3 centre = -1.0 * g[0];
#pragma unroll
      for (int k = 1; k < A - 1; ++k) { ga[k + 1] = g[k]; centre = centre - g[k]; }
      ga[1] = centre;
    }
    double* rec = a.rec + (size_t)t * a.term_stride;
#pragma unroll
    for (int p = 0; p < A; ++p) {
      rec[(3 * p) * a.plane_stride] = ga[p].x;
      rec[(3 * p + 1) * a.plane_stride] = ga[p].y;
      rec[(3 * p + 2) * a.plane_stride] = ga[p].z;
    }
  }
  if (VIRIAL) {
    V3 r0 = {0.0, 0.0, 0.0}, r1 = r0, r2 = r0;  // rows of -sum_v g_v (x) v
#pragma unroll
    for (int k = 0; k < A - 1; ++k) { r0 = r0 - g[k].x * d[k]; r1 = r1 - g[k].y * d[k]; r2 = r2 - g[k].z * d[k]; }
    double* o = a.vir + t;
    const size_t T_ = (size_t)a.T;
    o[0] = r0.x; o[T_] = r0.y; o[2 * T_] = r0.z;
    o[3 * T_] = r1.x; o[4 * T_] = r1.y; o[5 * T_] = r1.z;
    o[6 * T_] = r2.x; o[7 * T_] = r2.y; o[8 * T_] = r2.z;
    a.tsys[t] = sys;
  }
}

// energies[i] = sum E_t / A, forces[i] = -sum record(t, p) over the slots t A + p of atom i in the stored order
template <int A, class TO>
__global__ __launch_bounds__(VA_THREADS) void va_gather_kernel(const double* __restrict__ et, const double* __restrict__ rec, size_t plane_stride,
                                                               size_t term_stride, const int* __restrict__ slot_ptr,
                                                               const int* __restrict__ slot_idx, int N, int T, long long n_slots,
                                                               TO* __restrict__ energies, TO* __restrict__ forces) {
  const int i = blockIdx.x * VA_THREADS + threadIdx.x;
  if (i >= N) return;
  long long beg = slot_ptr[i], end = slot_ptr[i + 1];
  if (beg < 0) beg = 0;
  if (end > n_slots) end = n_slots;
  double e = 0.0;
  V3 f = {0.0, 0.0, 0.0};
  for (long long s = beg; s < end; ++s) {
    const unsigned slot = (unsigned)slot_idx[s];
    const unsigned t = slot / A, p = slot - t * A;
    if (t >= (unsigned)T) continue;
    if (energies) e += et[t];
    if (forces) {
      const double* r = rec + (size_t)t * term_stride + (3 * (size_t)p) * plane_stride;
      f.x += r[0]; f.y += r[plane_stride]; f.z += r[2 * plane_stride];
    }
  }
  if (energies) energies[i] = (TO)(e * (1.0 / A));
  if (forces) { TO* o = forces + 3 * (size_t)i; o[0] = (TO)(-f.x); o[1] = (TO)(-f.y); o[2] = (TO)(-f.z); }
}

// per-system fold of the per-term virial words (planes [9][T]): partial[s][x][0..9) with plain stores; the caller sums the MI_FOLD_BLOCKS rows
__global__ __launch_bounds__(256) void va_fold_kernel(const double* __restrict__ vir, const int* __restrict__ tsys, int T,
                                                      double* __restrict__ partial) {
  mi_system_fold<VA_VIR_WORDS, MI_FOLD_BLOCKS>(tsys, T, VA_VIR_WORDS, partial, [&](long long r, double* a) {
#pragma unroll
    for (int k = 0; k < VA_VIR_WORDS; ++k) a[k] += vir[(size_t)k * T + r];
  });
}

template <int KIND, class T, int FLAGS> void va_launch_term(const VaArgs& a, hipStream_t st) {
  va_term_kernel<KIND, T, FLAGS><<<mi_blocks(a.T, VA_THREADS), VA_THREADS, 0, st>>>(a);
}
template <int KIND, class T> void va_launch_flags(const VaArgs& a, int flags, hipStream_t st) {
  switch (flags & 7) {
    case 0: va_launch_term<KIND, T, 0>(a, st); break;
    case 1: va_launch_term<KIND, T, 1>(a, st); break;
    case 2: va_launch_term<KIND, T, 2>(a, st); break;
    case 3: va_launch_term<KIND, T, 3>(a, st); break;
    case 4: va_launch_term<KIND, T, 4>(a, st); break;
    case 5: va_launch_term<KIND, T, 5>(a, st); break;
    case 6: va_launch_term<KIND, T, 6>(a, st); break;
    default: va_launch_term<KIND, T, 7>(a, st); break;
  }
}
template <int KIND> void va_launch_kind(const VaArgs& a, int dtype, int flags, long long n_slots, const int* slot_ptr, const int* slot_idx,
                                        void* energies, void* forces, hipStream_t st) {
  constexpr int A = va_arity(KIND);
  if (dtype == MI_F32) {
    va_launch_flags<KIND, float>(a, flags, st);
    va_gather_kernel<A, float><<<mi_blocks(a.N, VA_THREADS), VA_THREADS, 0, st>>>(a.et, a.rec, a.plane_stride, a.term_stride, slot_ptr, slot_idx, a.N,
                                                                                  a.T, n_slots, (float*)energies, (float*)forces);
  } else {
    va_launch_flags<KIND, double>(a, flags, st);
    va_gather_kernel<A, double><<<mi_blocks(a.N, VA_THREADS), VA_THREADS, 0, st>>>(a.et, a.rec, a.plane_stride, a.term_stride, slot_ptr, slot_idx, a.N,
                                                                                   a.T, n_slots, (double*)energies, (double*)forces);
  }
}

// scratch: E_t [T] | record [3 A T] (with forces) | virial words [9 T] and term systems int [T] (with the virial)
struct VaScratch { size_t et, rec, vir, tsys, total; };
VaScratch va_scratch(int arity, long long T, int flags) {
  VaScratch s;
  size_t off = 0;
  s.et = off; off += mi_align((size_t)T * sizeof(double));
  s.rec = off; if (flags & MI_VALENCE_FORCES) off += mi_align(3 * (size_t)arity * T * sizeof(double));
  s.vir = off; if (flags & MI_VALENCE_VIRIAL) off += mi_align((size_t)VA_VIR_WORDS * T * sizeof(double));
  s.tsys = off; if (flags & MI_VALENCE_VIRIAL) off += mi_align((size_t)T * sizeof(int));
  s.total = off;
  return s;
}

}  // namespace

extern "C" {

int mi_valence_blocks(void) { return MI_FOLD_BLOCKS; }
int mi_valence_arity(int kind) { return (kind >= MI_VALENCE_BOND && kind <= MI_VALENCE_TORSION) ? va_arity(kind) : 0; }

size_t mi_valence_scratch_bytes(int kind, int n_terms, int flags) {
  if (n_terms <= 0 || mi_valence_arity(kind) == 0) return 0;
  return va_scratch(va_arity(kind), n_terms, flags).total;
}

int mi_valence(int kind, const void* positions, const int32_t* atoms, const void* parameters, int n_params, const void* cell,
               const int32_t* batch_idx, const double* weights, const int32_t* slot_ptr, const int32_t* slot_idx, long long n_slots, int n_atoms,
               int n_terms, int n_systems, int dtype, double cubic, double quartic, double pentic, double sextic, int plane, int flags,
               void* energies, void* forces, double* parameter_grads, double* virial_partial, void* scratch, size_t scratch_bytes, void* stream) {
  MI_REQUIRE(kind >= MI_VALENCE_BOND && kind <= MI_VALENCE_TORSION, "kind must be one of MI_VALENCE_BOND .. MI_VALENCE_TORSION");
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  MI_REQUIRE(n_atoms >= 0 && n_atoms <= (1 << 29), "n_atoms must be in [0, 2^29]");
  MI_REQUIRE(n_terms >= 0 && n_terms <= (1 << 28), "n_terms must be in [0, 2^28]");
  MI_REQUIRE(n_slots >= 0, "n_slots must not be negative");
  MI_REQUIRE((flags & ~(MI_VALENCE_FORCES | MI_VALENCE_PARAMETER_GRAD | MI_VALENCE_VIRIAL | MI_VALENCE_TERM_MAJOR)) == 0, "unknown flag");
  const int want[5] = {2, 2, 5, 1, 0};
  if (kind == MI_VALENCE_TORSION)
    MI_REQUIRE(n_params >= 2 && n_params <= 2 * VA_MAX_FOLDS && n_params % 2 == 0, "a torsion takes 2 F parameters, F in 1..6");
  else
    MI_REQUIRE(n_params == want[kind], "wrong number of parameters for this kind");
  MI_REQUIRE(plane == MI_VALENCE_PLANE_WDC || plane == MI_VALENCE_PLANE_ALLINGER, "plane must be MI_VALENCE_PLANE_WDC or MI_VALENCE_PLANE_ALLINGER");
  if (n_atoms == 0 || n_terms == 0) return MI_OK;
  MI_REQUIRE(positions && atoms && parameters && slot_ptr && scratch, "null pointer");
  MI_REQUIRE(n_slots == 0 || slot_idx, "null pointer");
  MI_REQUIRE(((flags & MI_VALENCE_FORCES) != 0) == (forces != nullptr), "forces is written exactly with MI_VALENCE_FORCES");
  MI_REQUIRE(((flags & MI_VALENCE_PARAMETER_GRAD) != 0) == (parameter_grads != nullptr), "parameter_grads is written exactly with MI_VALENCE_PARAMETER_GRAD");
  MI_REQUIRE(((flags & MI_VALENCE_VIRIAL) != 0) == (virial_partial != nullptr), "virial_partial is written exactly with MI_VALENCE_VIRIAL");
  MI_REQUIRE(!(flags & MI_VALENCE_VIRIAL) || cell, "the virial needs a cell");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(n_systems == 1 || (batch_idx && cell), "more than one system needs cell and batch_idx");
  const int A = va_arity(kind);
  const VaScratch s = va_scratch(A, n_terms, flags);
  MI_REQUIRE(scratch_bytes >= s.total, "scratch is smaller than mi_valence_scratch_bytes");
  char* base = (char*)scratch;
  VaArgs a;
  a.pos = positions; a.atoms = atoms; a.par = parameters; a.cell = cell; a.batch = cell ? batch_idx : nullptr; a.weights = weights;
  a.P = n_params; a.N = n_atoms; a.T = n_terms; a.nsys = n_systems; a.plane = plane;
  a.c3 = cubic; a.c4 = quartic; a.c5 = pentic; a.c6 = sextic;
  const bool term_major = flags & MI_VALENCE_TERM_MAJOR;
  a.plane_stride = term_major ? 1 : (size_t)n_terms;
  a.term_stride = term_major ? 3 * (size_t)A : 1;
  a.et = (double*)(base + s.et); a.rec = (double*)(base + s.rec); a.pgrads = parameter_grads;
  a.vir = (double*)(base + s.vir); a.tsys = (int*)(base + s.tsys);
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin("valence", stream);
  switch (kind) {
    case MI_VALENCE_BOND: va_launch_kind<MI_VALENCE_BOND>(a, dtype, flags, n_slots, slot_ptr, slot_idx, energies, forces, st); break;
    case MI_VALENCE_ANGLE: va_launch_kind<MI_VALENCE_ANGLE>(a, dtype, flags, n_slots, slot_ptr, slot_idx, energies, forces, st); break;
    case MI_VALENCE_STRETCH_BEND: va_launch_kind<MI_VALENCE_STRETCH_BEND>(a, dtype, flags, n_slots, slot_ptr, slot_idx, energies, forces, st); break;
    case MI_VALENCE_OUT_OF_PLANE: va_launch_kind<MI_VALENCE_OUT_OF_PLANE>(a, dtype, flags, n_slots, slot_ptr, slot_idx, energies, forces, st); break;
    default: va_launch_kind<MI_VALENCE_TORSION>(a, dtype, flags, n_slots, slot_ptr, slot_idx, energies, forces, st); break;
  }
  if (flags & MI_VALENCE_VIRIAL)
    va_fold_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>(a.vir, n_systems > 1 ? a.tsys : nullptr, n_terms, virial_partial);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

}  // extern "C"
