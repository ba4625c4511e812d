// valence.hip -- the bonded (valence) terms of an AMOEBA-class or fixed-charge force field: bond stretch, angle bend, stretch-bend, out-of-plane
// bend and Fourier torsion, and the coupled torsion terms (stretch-torsion, angle-torsion, pi-torsion, torsion-torsion) below.  gfx950.
// Driver: nvalchemiops/interactions/valence.  The reference package has no counterpart; the definitions are Tinker's, written from their formulas (angles in radians, no 1/2 in front of any force constant):
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
//   STRETCH_TORSION a b c d (4)       b1, b2, b3                              sum_{m=1..3} (|b_m| - r0_m) S_m,  S_m = sum_{n=1..3} k_mn (1 + cos(n phi - gamma_n))
//   ANGLE_TORSION  a b c d  (4)       b1, b2, b3                              sum_{m=1,2} (theta_m - theta0_m) S_m,  theta_1 = angle(-b1, b2), theta_2 = angle(-b2, b3)
//   PI_TORSION     a b c d e f (6)    v0 = r_a - r_d, v1 = r_b - r_d,         k (1 - cos 2 phi) = 2 k sin^2 phi,  phi = phi(-p, v4, q),  p = v0 x v1,  q = v2 x v3
//                                     v2 = r_e - r_c, v3 = r_f - r_c, v4 = r_d - r_c
//   torsion-torsion a b c d e (5)     b1 .. b4                                F_m(s phi_1, s phi_2),  phi_1 = phi(b1, b2, b3), phi_2 = phi(b2, b3, b4), s = +-1,
//   (mi_torsion_torsion)                                                      F_m the bicubic Hermite patch of map m on a uniform periodic grid over [-pi, pi)^2
//
// Every kind is a function of its A - 1 difference vectors (minimum images when a cell is given), so each computes dE/d(vector) once; the
// atom gradients are the fixed linear map of the table above applied to them and the virial is -sum_v dE/dv (x) v.
//   theta = atan2(|u x v|, u . v);  dtheta/du = u x (u x v) / (|u|^2 |u x v|),  dtheta/dv = (u x v) x v / (|v|^2 |u x v|)
//   dphi/db1 = |b2| m / |m|^2,  dphi/db3 = |b2| n / |n|^2,  dphi/db2 = -(b1 . b2) m / (|m|^2 |b2|) - (b2 . b3) n / (|n|^2 |b2|)
//   cos n phi, sin n phi by the angle-addition recurrence from (cos phi, sin phi) = (m . n, |b2| b1 . n) / (|m| |n|); the phases enter as
//   sincos(gamma_n), a call on the parameter and none on n phi
//   coupled terms: E = sum_m D_m S_m(phi) gives dE = sum_m (S_m dD_m + D_m S_m' dphi), S_m' = -sum_n n k_mn sin(n phi - gamma_n); the three
//   folds of the recurrence serve every row m.  Pi-torsion: phi depends on v0 .. v3 through p and q only, (v0 x v1) . x = v0 . (v1 x x) =
//   v1 . (x x v0), so dphi/dv0 = v1 x dphi/dp, dphi/dv1 = dphi/dp x v0 with dphi/dp = -dphi/db1, and the same for q = b3; dphi/dv4 is direct.
//   Torsion-torsion: with x = s phi_1 = -pi + (i + t) h the patch is sum over the corners (a, b) in {0, 1}^2 of
//   H0a(t1) H0b(t2) f + h1 H1a(t1) H0b(t2) f_1 + h2 H0a(t1) H1b(t2) f_2 + h1 h2 H1a(t1) H1b(t2) f_12 with the cubic Hermite basis
//   H00 = 2 t^3 - 3 t^2 + 1, H01 = 3 t^2 - 2 t^3, H10 = t^3 - 2 t^2 + t, H11 = t^3 - t^2; dE/dphi_1 = s dF/dx from the derivative basis.  The
//   cell index is reduced modulo n, so phi = pi and any other edge land in a valid cell; the patch is C^1, either neighbour serves.
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

constexpr int VA_TORSION_TORSION = 8;  // the kind of mi_torsion_torsion inside this file; mi_valence does not take it

__host__ __device__ constexpr int va_arity(int kind) {
  return kind == MI_VALENCE_BOND ? 2 : (kind == MI_VALENCE_ANGLE || kind == MI_VALENCE_STRETCH_BEND) ? 3 : kind == VA_TORSION_TORSION ? 5 :
         kind == MI_VALENCE_PI_TORSION ? 6 : 4;
}
// the kinds whose difference vectors are the chain b_k = r_{k+1} - r_k
__host__ __device__ constexpr bool va_chain(int kind) {
  return kind == MI_VALENCE_TORSION || kind == MI_VALENCE_STRETCH_TORSION || kind == MI_VALENCE_ANGLE_TORSION || kind == VA_TORSION_TORSION;
}

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
  const double* nodes; const int* map_index; const double* signs; int n_maps, n1, n2;  // torsion-torsion: node records [n_maps][n1][n2][4]
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

// (cos phi, sin phi) of the dihedral of b1, b2, b3 and dphi/db1, dphi/db2, dphi/db3 from the normals m = b1 x b2, n = b2 x b3:
// term_torsion's expressions
struct Dihedral { double c, s; V3 g1, g2, g3; };
__device__ __forceinline__ Dihedral dihedral_of(V3 b1, V3 b2, V3 b3, V3 m, V3 n) {
  const double mm = dot(m, m), nn = dot(n, n), lb2 = sqrt(dot(b2, b2));
  const double inv_mn = 1.0 / sqrt(mm * nn);
  Dihedral D;
  D.c = dot(m, n) * inv_mn;
  D.s = lb2 * dot(b1, n) * inv_mn;
  D.g1 = (lb2 / mm) * m;
  D.g3 = (lb2 / nn) * n;
  D.g2 = (-dot(b1, b2) / (mm * lb2)) * m + (-dot(b2, b3) / (nn * lb2)) * n;
  return D;
}
__device__ __forceinline__ Dihedral dihedral_of(V3 b1, V3 b2, V3 b3) { return dihedral_of(b1, b2, b3, cross(b1, b2), cross(b2, b3)); }

// Stretch-torsion (ROWS = 3: D_m = |b_m| - r0_m) and angle-torsion (ROWS = 2: D_m = theta_m - theta0_m):
// E = sum_m D_m S_m, S_m = sum_n k_mn (1 + cos(n phi - gamma_n)); parameters (k_11 .. k_ROWS3, the ROWS references, gamma_1..3)
template <int ROWS, bool GRAD, bool PG, class T>
__device__ __forceinline__ double term_coupled_torsion(const V3* d, const T* __restrict__ p, double w, V3* g, double* __restrict__ pg) {
  const Dihedral D = dihedral_of(d[0], d[1], d[2]);
  double Dm[ROWS];
  V3 dD[ROWS][2];  // stretch: dD_m/db_m; angle: dD_m/db_m and dD_m/db_{m+1}
  if (ROWS == 3) {
#pragma unroll
    for (int m = 0; m < ROWS; ++m) {
      const double r = sqrt(dot(d[m], d[m]));
      Dm[m] = r - (double)p[3 * ROWS + m];
      dD[m][0] = (1.0 / r) * d[m];
    }
  } else {
#pragma unroll
    for (int m = 0; m < ROWS; ++m) {
      V3 dtu, dtv;
      Dm[m] = angle_of(-1.0 * d[m], d[m + 1], dtu, dtv) - (double)p[3 * ROWS + m];
      dD[m][0] = -1.0 * dtu;
      dD[m][1] = dtv;
    }
  }
  double S[ROWS], dS[ROWS], e = 0.0, cn = 1.0, sn = 0.0;
#pragma unroll
  for (int m = 0; m < ROWS; ++m) S[m] = dS[m] = 0.0;
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const double c = cn * D.c - sn * D.s;  // cos (f + 1) phi, sin (f + 1) phi
    sn = sn * D.c + cn * D.s;
    cn = c;
    double sg, cg;
    sincos((double)p[4 * ROWS + f], &sg, &cg);
    const double cosd = cn * cg + sn * sg, sind = sn * cg - cn * sg;  // cos, sin of (n phi - gamma)
    double dgamma = 0.0;
#pragma unroll
    for (int m = 0; m < ROWS; ++m) {
      const double k = (double)p[3 * m + f];
      S[m] += k * (1.0 + cosd);
      dS[m] -= (double)(f + 1) * k * sind;
      dgamma += Dm[m] * k * sind;
      if (PG) pg[3 * m + f] = w * Dm[m] * (1.0 + cosd);
    }
    if (PG) pg[4 * ROWS + f] = w * dgamma;
  }
  double dEdphi = 0.0;
#pragma unroll
  for (int m = 0; m < ROWS; ++m) {
    e += Dm[m] * S[m];
    dEdphi += Dm[m] * dS[m];
    if (PG) pg[3 * ROWS + m] = -w * S[m];
  }
  if (GRAD) {
    const double q = w * dEdphi;
    g[0] = q * D.g1; g[1] = q * D.g2; g[2] = q * D.g3;
#pragma unroll
    for (int m = 0; m < ROWS; ++m) {
      g[m] = g[m] + (w * S[m]) * dD[m][0];
      if (ROWS == 2) g[m + 1] = g[m + 1] + (w * S[m]) * dD[m][1];
    }
  }
  return e;
}

template <bool GRAD, bool PG, class T>
__device__ __forceinline__ double term_pi_torsion(const V3* d, const T* __restrict__ p, double w, V3* g, double* __restrict__ pg) {
  const double k = (double)p[0];
  const V3 pp = cross(d[0], d[1]), qq = cross(d[2], d[3]);
  const Dihedral D = dihedral_of(-1.0 * pp, d[4], qq);
  const double s2 = 2.0 * D.s * D.s;  // 1 - cos 2 phi
  if (GRAD) {
    const double q = w * 4.0 * k * D.s * D.c;  // dE/dphi = 2 k sin 2 phi
    const V3 dp = -q * D.g1, dq = q * D.g3;    // dE/dp, dE/dq
    g[0] = cross(d[1], dp); g[1] = cross(dp, d[0]);
    g[2] = cross(d[3], dq); g[3] = cross(dq, d[2]);
    g[4] = q * D.g2;
  }
  if (PG) pg[0] = w * s2;
  return k * s2;
}

// cubic Hermite basis at t in [0, 1] for a cell of width h: b = (H00, H01, h H10, h H11), db = d/dx of them
__device__ __forceinline__ void hermite(double t, double h, double* b, double* db) {
  const double t2 = t * t, t3 = t2 * t, ih = 1.0 / h;
  b[0] = 2.0 * t3 - 3.0 * t2 + 1.0; b[1] = 3.0 * t2 - 2.0 * t3; b[2] = h * (t3 - 2.0 * t2 + t); b[3] = h * (t3 - t2);
  db[0] = ih * 6.0 * (t2 - t); db[1] = -db[0]; db[2] = 3.0 * t2 - 4.0 * t + 1.0; db[3] = 3.0 * t2 - 2.0 * t;
}
// the cell of x in [-pi, pi] on n nodes: index reduced modulo n (x = pi and every edge land in a valid cell; a NaN goes to cell 0), offset t
__device__ __forceinline__ void cell_of(double x, int n, int& i0, int& i1, double& t) {
  const double u = (x + M_PI) * ((double)n * (0.5 * M_1_PI));
  const double fl = floor(u);
  t = u - fl;
  int i = fl >= 0.0 && fl <= (double)n ? (int)fl % n : 0;  // 0 <= fl <= n for x in [-pi, pi]; anything else, a NaN included, is not converted
  if (i < 0) i += n;
  i0 = i;
  i1 = i + 1 == n ? 0 : i + 1;
}

// Torsion-torsion: E = F_m(s phi_1, s phi_2).  `rec` is the map's node records [n1][n2][4].
template <bool GRAD>
__device__ __forceinline__ double term_torsion_torsion(const V3* d, const double* rec, int n1, int n2, double sign, double w, V3* g) {
  const V3 mid = cross(d[1], d[2]);  // the normal both dihedrals share
  const Dihedral D1 = dihedral_of(d[0], d[1], d[2], cross(d[0], d[1]), mid), D2 = dihedral_of(d[1], d[2], d[3], mid, cross(d[2], d[3]));
  int i[2], j[2];
  double t1, t2, a[4], da[4], b[4], db[4];
  cell_of(sign * atan2(D1.s, D1.c), n1, i[0], i[1], t1);
  cell_of(sign * atan2(D2.s, D2.c), n2, j[0], j[1], t2);
  hermite(t1, 2.0 * M_PI / n1, a, da);
  hermite(t2, 2.0 * M_PI / n2, b, db);
  double F = 0.0, Fx = 0.0, Fy = 0.0;
#pragma unroll
  for (int ca = 0; ca < 2; ++ca) {
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
      const double2* node = (const double2*)(rec + 4 * ((size_t)i[ca] * n2 + j[cb]));  // 32-byte record: two 16-byte loads
      const double2 lo = node[0], hi = node[1];  // (f, f_1), (f_2, f_12)
      const double row0 = b[cb] * lo.x + b[2 + cb] * hi.x, row1 = b[cb] * lo.y + b[2 + cb] * hi.y;  // summed over the second direction
      F += a[ca] * row0 + a[2 + ca] * row1;
      if (GRAD) {
        Fx += da[ca] * row0 + da[2 + ca] * row1;
        Fy += a[ca] * (db[cb] * lo.x + db[2 + cb] * hi.x) + a[2 + ca] * (db[cb] * lo.y + db[2 + cb] * hi.y);
      }
    }
  }
  if (GRAD) {
    const double q1 = w * sign * Fx, q2 = w * sign * Fy;
    g[0] = q1 * D1.g1;
    g[1] = q1 * D1.g2 + q2 * D2.g1;
    g[2] = q1 * D1.g3 + q2 * D2.g2;
    g[3] = q2 * D2.g3;
  }
  return F;
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
  int map = 0;
  if (KIND == VA_TORSION_TORSION) {
    map = a.map_index[t];
    ok = ok && (unsigned)map < (unsigned)a.n_maps;
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
    if (va_chain(KIND)) {
#pragma unroll
      for (int k = 0; k < A - 1; ++k) d[k] = min_image(r[k + 1] - r[k], periodic, c);
    } else if (KIND == MI_VALENCE_PI_TORSION) {  // a, b from d; e, f from c; the bond c -> d
      d[0] = min_image(r[0] - r[3], periodic, c); d[1] = min_image(r[1] - r[3], periodic, c);
      d[2] = min_image(r[4] - r[2], periodic, c); d[3] = min_image(r[5] - r[2], periodic, c);
      d[4] = min_image(r[3] - r[2], periodic, c);
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
    if (KIND == MI_VALENCE_STRETCH_TORSION) e = term_coupled_torsion<3, GRAD, PG>(d, par, w, g, pg);
    if (KIND == MI_VALENCE_ANGLE_TORSION) e = term_coupled_torsion<2, GRAD, PG>(d, par, w, g, pg);
    if (KIND == MI_VALENCE_PI_TORSION) e = term_pi_torsion<GRAD, PG>(d, par, w, g, pg);
    if (KIND == VA_TORSION_TORSION) e = term_torsion_torsion<GRAD>(d, a.nodes + 4 * (size_t)a.n1 * a.n2 * map, a.n1, a.n2, a.signs[t], w, g);
  } else if (PG) {
    for (int k = 0; k < a.P; ++k) pg[k] = 0.0;
  }
  a.et[t] = e;
  if (FORCES) {
    // the atom gradients from the vector gradients
    V3 ga[A];
    if (va_chain(KIND)) {
      ga[0] = -1.0 * g[0];
#pragma unroll
      for (int p = 1; p < A - 1; ++p) ga[p] = g[p - 1] - g[p];
      ga[A - 1] = g[A - 2];
    } else if (KIND == MI_VALENCE_PI_TORSION) {
      ga[0] = g[0]; ga[1] = g[1]; ga[4] = g[2]; ga[5] = g[3];
      ga[2] = -1.0 * (g[2] + g[3] + g[4]);
      ga[3] = g[4] - (g[0] + g[1]);
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
  constexpr int PG = KIND == VA_TORSION_TORSION ? 0 : MI_VALENCE_PARAMETER_GRAD;  // torsion-torsion has no parameters: four instantiations, not eight
  switch (flags & 7) {
    case 0: va_launch_term<KIND, T, 0>(a, st); break;
    case 1: va_launch_term<KIND, T, 1>(a, st); break;
    case 2: va_launch_term<KIND, T, PG>(a, st); break;
    case 3: va_launch_term<KIND, T, 1 | PG>(a, st); break;
    case 4: va_launch_term<KIND, T, 4>(a, st); break;
    case 5: va_launch_term<KIND, T, 5>(a, st); break;
    case 6: va_launch_term<KIND, T, 4 | PG>(a, st); break;
    default: va_launch_term<KIND, T, 5 | PG>(a, st); break;
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

// The checks both entry points make first, in mi_valence's order
int va_sizes(int dtype, int n_atoms, int n_terms, long long n_slots) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype must be MI_F32 or MI_F64");
  MI_REQUIRE(n_atoms >= 0 && n_atoms <= (1 << 29), "n_atoms must be in [0, 2^29]");
  MI_REQUIRE(n_terms >= 0 && n_terms <= (1 << 28), "n_terms must be in [0, 2^28]");
  MI_REQUIRE(n_slots >= 0, "n_slots must not be negative");
  return MI_OK;
}

// What mi_valence and mi_torsion_torsion share once their own arguments are checked and in `a`: the remaining checks in mi_valence's order,
// the scratch layout, the term and gather launches and the virial fold.  `small`: the entry's message for a scratch that is too small.
int va_run(int kind, VaArgs a, const char* label, const char* small, const void* positions, const int32_t* atoms, const void* cell,
           const int32_t* batch_idx, const double* weights, const int32_t* slot_ptr, const int32_t* slot_idx, long long n_slots, int n_atoms,
           int n_terms, int n_systems, int dtype, int flags, void* energies, void* forces, double* virial_partial, void* scratch,
           size_t scratch_bytes, void* stream) {
  if (n_atoms == 0 || n_terms == 0) return MI_OK;
  MI_REQUIRE(positions && atoms && (a.par || kind == VA_TORSION_TORSION) && slot_ptr && scratch, "null pointer");
  MI_REQUIRE(n_slots == 0 || slot_idx, "null pointer");
  MI_REQUIRE(((flags & MI_VALENCE_FORCES) != 0) == (forces != nullptr), "forces is written exactly with MI_VALENCE_FORCES");
  MI_REQUIRE(((flags & MI_VALENCE_PARAMETER_GRAD) != 0) == (a.pgrads != nullptr), "parameter_grads is written exactly with MI_VALENCE_PARAMETER_GRAD");
  MI_REQUIRE(((flags & MI_VALENCE_VIRIAL) != 0) == (virial_partial != nullptr), "virial_partial is written exactly with MI_VALENCE_VIRIAL");
  MI_REQUIRE(!(flags & MI_VALENCE_VIRIAL) || cell, "the virial needs a cell");
  MI_REQUIRE(n_systems >= 1, "n_systems must be at least 1");
  MI_REQUIRE(n_systems == 1 || (batch_idx && cell), "more than one system needs cell and batch_idx");
  const int A = va_arity(kind);
  const VaScratch s = va_scratch(A, n_terms, flags);
  MI_REQUIRE(scratch_bytes >= s.total, small);
  char* base = (char*)scratch;
  a.pos = positions; a.atoms = atoms; a.cell = cell; a.batch = cell ? batch_idx : nullptr; a.weights = weights;
  a.N = n_atoms; a.T = n_terms; a.nsys = n_systems;
  const bool term_major = flags & MI_VALENCE_TERM_MAJOR;
  a.plane_stride = term_major ? 1 : (size_t)n_terms;
  a.term_stride = term_major ? 3 * (size_t)A : 1;
  a.et = (double*)(base + s.et); a.rec = (double*)(base + s.rec);
  a.vir = (double*)(base + s.vir); a.tsys = (int*)(base + s.tsys);
  hipStream_t st = (hipStream_t)stream;
  mi_timing_begin(label, stream);
  switch (kind) {
    case MI_VALENCE_BOND: va_launch_kind<MI_VALENCE_BOND>(a, dtype, flags, n_slots, slot_ptr, slot_idx, energies, forces, st); break;
    case MI_VALENCE_ANGLE: va_launch_kind<MI_VALENCE_ANGLE>(a, dtype, flags, n_slots, slot_ptr, slot_idx, energies, forces, st); break;
    case MI_VALENCE_STRETCH_BEND: va_launch_kind<MI_VALENCE_STRETCH_BEND>(a, dtype, flags, n_slots, slot_ptr, slot_idx, energies, forces, st); break;
    case MI_VALENCE_OUT_OF_PLANE: va_launch_kind<MI_VALENCE_OUT_OF_PLANE>(a, dtype, flags, n_slots, slot_ptr, slot_idx, energies, forces, st); break;
    case MI_VALENCE_TORSION: va_launch_kind<MI_VALENCE_TORSION>(a, dtype, flags, n_slots, slot_ptr, slot_idx, energies, forces, st); break;
    case MI_VALENCE_STRETCH_TORSION: va_launch_kind<MI_VALENCE_STRETCH_TORSION>(a, dtype, flags, n_slots, slot_ptr, slot_idx, energies, forces, st); break;
    case MI_VALENCE_ANGLE_TORSION: va_launch_kind<MI_VALENCE_ANGLE_TORSION>(a, dtype, flags, n_slots, slot_ptr, slot_idx, energies, forces, st); break;
    case MI_VALENCE_PI_TORSION: va_launch_kind<MI_VALENCE_PI_TORSION>(a, dtype, flags, n_slots, slot_ptr, slot_idx, energies, forces, st); break;
    default: va_launch_kind<VA_TORSION_TORSION>(a, dtype, flags, n_slots, slot_ptr, slot_idx, energies, forces, st); break;
  }
  if (flags & MI_VALENCE_VIRIAL)
    va_fold_kernel<<<dim3(MI_FOLD_BLOCKS, n_systems), 256, 0, st>>>(a.vir, n_systems > 1 ? a.tsys : nullptr, n_terms, virial_partial);
  mi_timing_end(stream);
  MI_LAUNCH_CHECK();
  return MI_OK;
}

}  // namespace

extern "C" {

int mi_valence_blocks(void) { return MI_FOLD_BLOCKS; }
int mi_valence_arity(int kind) { return (kind >= MI_VALENCE_BOND && kind <= MI_VALENCE_PI_TORSION) ? va_arity(kind) : 0; }

size_t mi_valence_scratch_bytes(int kind, int n_terms, int flags) {
  if (n_terms <= 0 || mi_valence_arity(kind) == 0) return 0;
  return va_scratch(va_arity(kind), n_terms, flags).total;
}

int mi_valence(int kind, const void* positions, const int32_t* atoms, const void* parameters, int n_params, const void* cell,
               const int32_t* batch_idx, const double* weights, const int32_t* slot_ptr, const int32_t* slot_idx, long long n_slots, int n_atoms,
               int n_terms, int n_systems, int dtype, double cubic, double quartic, double pentic, double sextic, int plane, int flags,
               void* energies, void* forces, double* parameter_grads, double* virial_partial, void* scratch, size_t scratch_bytes, void* stream) {
  MI_REQUIRE(kind >= MI_VALENCE_BOND && kind <= MI_VALENCE_PI_TORSION, "kind must be one of MI_VALENCE_BOND .. MI_VALENCE_PI_TORSION");
  if (const int rc = va_sizes(dtype, n_atoms, n_terms, n_slots)) return rc;
  MI_REQUIRE((flags & ~(MI_VALENCE_FORCES | MI_VALENCE_PARAMETER_GRAD | MI_VALENCE_VIRIAL | MI_VALENCE_TERM_MAJOR)) == 0, "unknown flag");
  const int want[8] = {2, 2, 5, 1, 0, 15, 11, 1};
  if (kind == MI_VALENCE_TORSION)
    MI_REQUIRE(n_params >= 2 && n_params <= 2 * VA_MAX_FOLDS && n_params % 2 == 0, "a torsion takes 2 F parameters, F in 1..6");
  else
    MI_REQUIRE(n_params == want[kind], "wrong number of parameters for this kind");
  MI_REQUIRE(plane == MI_VALENCE_PLANE_WDC || plane == MI_VALENCE_PLANE_ALLINGER, "plane must be MI_VALENCE_PLANE_WDC or MI_VALENCE_PLANE_ALLINGER");
  VaArgs a = {};
  a.par = parameters; a.P = n_params; a.plane = plane; a.pgrads = parameter_grads;
  a.c3 = cubic; a.c4 = quartic; a.c5 = pentic; a.c6 = sextic;
  return va_run(kind, a, "valence", "scratch is smaller than mi_valence_scratch_bytes", positions, atoms, cell, batch_idx, weights, slot_ptr, slot_idx, n_slots, n_atoms, n_terms, n_systems, dtype, flags,
                energies, forces, virial_partial, scratch, scratch_bytes, stream);
}

size_t mi_torsion_torsion_scratch_bytes(int n_terms, int flags) {
  return n_terms <= 0 ? 0 : va_scratch(va_arity(VA_TORSION_TORSION), n_terms, flags).total;
}

int mi_torsion_torsion(const void* positions, const int32_t* atoms, const double* nodes, const int32_t* map_index, const double* signs, int n_maps,
                       int n1, int n2, const void* cell, const int32_t* batch_idx, const double* weights, const int32_t* slot_ptr,
                       const int32_t* slot_idx, long long n_slots, int n_atoms, int n_terms, int n_systems, int dtype, int flags, void* energies,
                       void* forces, double* virial_partial, void* scratch, size_t scratch_bytes, void* stream) {
  if (const int rc = va_sizes(dtype, n_atoms, n_terms, n_slots)) return rc;
  MI_REQUIRE((flags & ~(MI_VALENCE_FORCES | MI_VALENCE_VIRIAL | MI_VALENCE_TERM_MAJOR)) == 0, "unknown flag");
  MI_REQUIRE(n_maps >= 1 && n1 >= 2 && n2 >= 2 && (long long)n_maps * n1 * n2 <= (1LL << 28), "maps must be [n_maps >= 1][n1 >= 2][n2 >= 2], at most 2^28 nodes");
  if (n_atoms > 0 && n_terms > 0) MI_REQUIRE(nodes && map_index && signs, "null pointer");
  VaArgs a = {};
  a.nodes = nodes; a.map_index = map_index; a.signs = signs; a.n_maps = n_maps; a.n1 = n1; a.n2 = n2;
  return va_run(VA_TORSION_TORSION, a, "torsion_torsion", "scratch is smaller than mi_torsion_torsion_scratch_bytes", positions, atoms, cell, batch_idx, weights, slot_ptr, slot_idx, n_slots, n_atoms, n_terms,
                n_systems, dtype, flags, energies, forces, virial_partial, scratch, scratch_bytes, stream);
}

}  // extern "C"
