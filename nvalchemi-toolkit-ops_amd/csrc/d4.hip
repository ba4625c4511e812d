// d4.hip -- DFT-D4 two-body dispersion with charge-dependent C6 (mi_d4).  gfx950, wave64.  The reference package has no counterpart.
//
// Model (include/nvalchemiops_hip.h has the full statement).  Over the entries (i, j, S) of a FULL list, r = r_j - r_i + S . cell:
//     CN_i   = sum_row delta(Z_i, Z_j) 1/2 (1 + erf(-k_cn (r / (rcov_i + rcov_j) - 1)))      delta = k4 exp(-(|en_i - en_j| + k5)^2 / k6)
//     w_i[a] = W_a(CN_i) zeta_a(q_i)      W: max-shifted Gaussian weights over the references of Z_i, zeta: the charge scaling
//     C6_ij  = sum_ab w_i[a] c6_ref[Z_i, Z_j, a, b] w_j[b]
//     E      = 1/2 sum_entries -C6_ij (s6 / (r^6 + R0^6) + s8 Q / (r^8 + R0^8))               Q = 3 r4r2_i r4r2_j, R0 = a1 sqrt(Q) + a2
//
// Execution shape (csrc/d3.hip's): one wave64 per atom, lanes stride the row; only the row owner writes -- the list is full, so an owner
// gets its force, dE/dCN_i and dE/dq_i from its own row alone (entry and mirror are equal by c6_ref[A,B,a,b] = c6_ref[B,A,b,a]; self-image
// entries (i, i, +-S) come out right the same way).  No atomics anywhere; per-system sums are written per row and folded in a fixed order
// (mi_system_fold of pair_row.h), so two identical calls give bit-identical outputs.  Pair math fp32 (the pair vector is formed in the
// positions dtype), accumulators fp64; the per-atom weights are evaluated in fp64 (O(N), seven references) and stored as fp32.
//
// Passes:  species (mark / compact / tables) -> pack -> CN -> weights -> energy -> chain -> fold -> finish.
//
// Energy pass.  The owner contracts its three weight vectors (w, dw/dCN, dw/dq) with c6_ref[Z_i, t, :, :] once per row for every species t
// present in the call: v_t^k[b] = sum_a w_i^k[a] c6[Z_i, t, a, b], kept in LDS.  A pair then costs three 8-term dot products against the
// neighbour's plain weights (one aligned 32-byte gather), not a 49-term table gather.  LDS layout per wave: [slot][k = 0..2][8] floats, a
// slot every 96 B.  Pairs read it with 16-byte loads, whose bank is (byte / 4) mod 64: slot s starts at bank 24 s mod 64, so any 8 distinct
// slots met inside one 16-lane group are conflict-free, 16 are 2-way (s and s + 8); a 128-byte slot stride would make s and s + 2 collide.
// Equal species broadcast.  4 waves x 1.5 KB per block: occupancy is not bounded by LDS.  With more species than D4_SLOTS the owner walks
// its row once per group of D4_SLOTS species (refill, then only the entries of that group): slower, same sums in a fixed order.
#include "common.h"

namespace {

#include "pair_row.h"  // the fixed-order fold of d4_fold_kernel (MI_FOLD_BLOCKS, mi_system_fold)

#define D4_REFS 7          // references per element
#define D4_SLOTS 16        // species whose contracted vectors one wave holds in LDS
#define D4_WAVES 4         // waves (atoms) per block
#define D4_WREC 24         // floats per atom in the weight records: w[8], dw/dCN[8], dw/dq[8]
#define D4_PAIR 8          // floats per species pair: {1 / (rcov_i + rcov_j), delta, Q, R0^6, R0^8, 0, 0, 0}
#define D4_ROW_WORDS 13    // doubles per row: energy, 6 virial words of the energy pass, 6 of the chain pass {xx, yy, zz, xy, xz, yz}

template <class T> struct D4Rec;
template <> struct D4Rec<float> { float x, y, z; int code; };             // 16 bytes: one vector load per neighbour
template <> struct D4Rec<double> { double x, y, z; long long code; };     // 32 bytes

struct D4Scalars { float a1, a2, s6, s8, k_cn, k4, k5, k6, wf, ga, gc, cn_cut; };

__device__ __forceinline__ bool d4_element_ok(int z, int nz, const int* __restrict__ n_ref) { return z > 0 && z < nz && n_ref[z] > 0; }

__global__ void d4_mark_species_kernel(const int* __restrict__ numbers, int N, int nz, const int* __restrict__ n_ref, int* __restrict__ present) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int z = numbers[i];
  if (d4_element_ok(z, nz, n_ref)) present[z] = 1;  // benign race: every writer stores 1
}

// compact ids of the species present: smap[z] = id or -1, zlist[id] = z, info[0] = S
__global__ void d4_compact_species_kernel(const int* __restrict__ present, int nz, int* __restrict__ smap, int* __restrict__ zlist, int* __restrict__ info) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int S = 0;
  for (int z = 0; z < nz; ++z) {
    if (z > 0 && present[z]) { smap[z] = S; zlist[S] = z; ++S; }
    else smap[z] = -1;
  }
  info[0] = S;
}

// dense tables of the species present: ptab[S][S][D4_PAIR] and cc6[S][S][7][8] (entries beyond n_ref, whatever they hold, become 0)
__global__ void d4_tables_kernel(const int* __restrict__ zlist, const int* __restrict__ info, int nz, const float* __restrict__ rcov,
                                 const float* __restrict__ en, const float* __restrict__ r4r2, const int* __restrict__ n_ref,
                                 const float* __restrict__ c6_ref, D4Scalars P, float* __restrict__ ptab, float* __restrict__ cc6) {
  const int S = info[0];
  const long long stride = (long long)gridDim.x * blockDim.x, t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long k = t0; k < (long long)S * S; k += stride) {
    const int zi = zlist[k / S], zj = zlist[k % S];
    const float q = 3.0f * r4r2[zi] * r4r2[zj];
    const float r0 = P.a1 * sqrtf(q) + P.a2, r02 = r0 * r0, r06 = r02 * r02 * r02;
    const float de = fabsf(en[zi] - en[zj]) + P.k5;
    float* o = ptab + D4_PAIR * k;
    o[0] = 1.0f / (rcov[zi] + rcov[zj]);
    o[1] = P.k4 * expf(-(de * de) / P.k6);
    o[2] = q; o[3] = r06; o[4] = r06 * r02;
    o[5] = o[6] = o[7] = 0.0f;
  }
  for (long long k = t0; k < (long long)S * S * 56; k += stride) {
    const int b = (int)(k % 8), a = (int)((k / 8) % D4_REFS);
    const long long pr = k / 56;
    const int zi = zlist[pr / S], zj = zlist[pr % S];
    const int ni = min(n_ref[zi], D4_REFS), nj = min(n_ref[zj], D4_REFS);
    cc6[k] = (a < ni && b < nj) ? c6_ref[(((size_t)zi * nz + zj) * D4_REFS + a) * D4_REFS + b] : 0.0f;
  }
}

template <class T>
__global__ void d4_pack_kernel(const T* __restrict__ pos, const int* __restrict__ numbers, int N, int nz, const int* __restrict__ smap,
                               D4Rec<T>* __restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int z = numbers[i];
  D4Rec<T> r;
  r.x = pos[3 * (size_t)i]; r.y = pos[3 * (size_t)i + 1]; r.z = pos[3 * (size_t)i + 2];
  r.code = (z > 0 && z < nz) ? smap[z] : -1;  // -1: padding (outside the tables, or an element without references)
  rec[i] = r;
}

// pair vector in the positions dtype, everything after it fp32; false for r <= 1e-8 (and NaN)
template <class T>
__device__ __forceinline__ bool d4_geom(const D4Rec<T>& ri, const D4Rec<T>& rj, bool shifted, const int* __restrict__ ush, long long e,
                                        const T* cm, float& r, float& rx, float& ry, float& rz) {
  T sx = rj.x - ri.x, sy = rj.y - ri.y, sz = rj.z - ri.z;
  if (shifted) {
    const T fs[3] = {(T)ush[3 * e], (T)ush[3 * e + 1], (T)ush[3 * e + 2]};
    T sh[3];
    rowvec_mat3(fs, cm, sh);
    sx += sh[0]; sy += sh[1]; sz += sh[2];
  }
  rx = (float)sx; ry = (float)sy; rz = (float)sz;
  r = sqrtf(rx * rx + ry * ry + rz * rz);
  return r > 1e-8f;
}

template <bool CSR> __device__ __forceinline__ unsigned d4_index_limit(int N, int fill_value) {
  return CSR ? (unsigned)N : (unsigned)min(N, max(fill_value, 0));  // mi_d3's rule: a matrix entry >= fill_value is padding
}

template <class T>
__device__ __forceinline__ void d4_load_cell(const T* __restrict__ cell, const int* __restrict__ batch_idx, int i, T* cm) {
  const int s = batch_idx ? batch_idx[i] : 0;
#pragma unroll
  for (int k = 0; k < 9; ++k) cm[k] = cell[9 * (size_t)s + k];
}

// ---- CN pass ----------------------------------------------------------------------------------------------------------------------------
template <class T, bool CSR>
__global__ __launch_bounds__(D4_WAVES * MI_WAVE) void d4_cn_kernel(const D4Rec<T>* __restrict__ rec, int N, const int* __restrict__ idx,
                                                                   const int* __restrict__ ush, const int* __restrict__ nptr, int M, int fill_value,
                                                                   const T* __restrict__ cell, const int* __restrict__ batch_idx,
                                                                   const int* __restrict__ info, const float* __restrict__ ptab, D4Scalars P,
                                                                   double* __restrict__ cn64, float* __restrict__ cn_out) {
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * D4_WAVES + threadIdx.x / MI_WAVE);
  if (i >= N) return;
  const D4Rec<T> ri = rec[i];
  const int ci = (int)ri.code;
  double acc = 0.0;
  if (ci >= 0) {
    const int S = info[0];
    const bool shifted = ush != nullptr && cell != nullptr;
    T cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (shifted) d4_load_cell(cell, batch_idx, i, cm);
    const unsigned jlim = d4_index_limit<CSR>(N, fill_value);
    long long beg, end;
    if (CSR) { beg = nptr[i]; end = nptr[i + 1]; } else { beg = (long long)i * M; end = beg + M; }
    for (long long e = beg + lane; e < end; e += MI_WAVE) {
      const int j = idx[e];
      if ((unsigned)j >= jlim) continue;
      const D4Rec<T> rj = rec[j];
      const int cj = (int)rj.code;
      if (cj < 0) continue;
      float r, rx, ry, rz;
      if (!d4_geom(ri, rj, shifted, ush, e, cm, r, rx, ry, rz)) continue;
      if (P.cn_cut > 0.0f && r >= P.cn_cut) continue;
      const float* p = ptab + D4_PAIR * ((size_t)ci * S + cj);
      const float x = P.k_cn * (r * p[0] - 1.0f);
      acc += (double)(p[1] * 0.5f * (1.0f + erff(-x)));
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) { cn64[i] = acc; cn_out[i] = (float)acc; }
}

// ---- weights: w_i[a] = W_a(CN_i) zeta_a(q_i) and its two derivatives, one thread per atom, fp64 -----------------------------------------
__global__ void d4_weights_kernel(const int* __restrict__ numbers, const float* __restrict__ charges, int N, int nz, const int* __restrict__ n_ref,
                                  const int* __restrict__ ngw, const float* __restrict__ cn_ref, const float* __restrict__ q_ref,
                                  const float* __restrict__ zeff, const float* __restrict__ gam, D4Scalars P, const double* __restrict__ cn64,
                                  float* __restrict__ wrec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  float* o = wrec + D4_WREC * (size_t)i;
  float w[D4_WREC];
#pragma unroll
  for (int k = 0; k < D4_WREC; ++k) w[k] = 0.0f;
  const int z = numbers[i];
  if (d4_element_ok(z, nz, n_ref)) {
    const int nr = min(n_ref[z], D4_REFS);
    const double cn = cn64[i], wf = (double)P.wf, ga = (double)P.ga, gc = (double)P.gc;
    double g[D4_REFS], dg[D4_REFS], m = -INFINITY, norm = 0.0, dnorm = 0.0;
    for (int a = 0; a < nr; ++a) {
      const double d = cn - (double)cn_ref[z * D4_REFS + a];
      m = fmax(m, -wf * d * d);
    }
    for (int a = 0; a < nr; ++a) {
      const double d = cn - (double)cn_ref[z * D4_REFS + a];
      const int ns = min(max(ngw[z * D4_REFS + a], 1), 3);
      double ga_ = 0.0, dga = 0.0;
      for (int s = 1; s <= ns; ++s) {
        const double t = exp(-wf * s * d * d - m);  // the largest exponent is subtracted: the largest term is 1, the sum never 0
        ga_ += t;
        dga += -2.0 * wf * s * d * t;
      }
      g[a] = ga_; dg[a] = dga; norm += ga_; dnorm += dga;
    }
    const double ze = (double)zeff[z], zq = ze + (double)charges[i], gz = gc * (double)gam[z];
    for (int a = 0; a < nr; ++a) {
      const double W = g[a] / norm, dW = (dg[a] - W * dnorm) / norm;
      double zeta, dzeta;
      if (zq > 0.0) {
        const double zr = ze + (double)q_ref[z * D4_REFS + a];
        const double inner = exp(gz * (1.0 - zr / zq));
        zeta = exp(ga * (1.0 - inner));
        dzeta = -zeta * ga * inner * gz * zr / (zq * zq);
      } else {
        zeta = exp(ga);
        dzeta = 0.0;
      }
      w[a] = (float)(W * zeta); w[8 + a] = (float)(dW * zeta); w[16 + a] = (float)(W * dzeta);
    }
  }
#pragma unroll
  for (int k = 0; k < D4_WREC; ++k) o[k] = w[k];
}

// ---- energy pass ------------------------------------------------------------------------------------------------------------------------
template <class T, bool CSR>
__global__ __launch_bounds__(D4_WAVES * MI_WAVE) void d4_energy_kernel(const D4Rec<T>* __restrict__ rec, int N, const int* __restrict__ idx,
                                                                       const int* __restrict__ ush, const int* __restrict__ nptr, int M,
                                                                       int fill_value, const T* __restrict__ cell, const int* __restrict__ batch_idx,
                                                                       const int* __restrict__ info, const float* __restrict__ ptab,
                                                                       const float* __restrict__ cc6, const float* __restrict__ wrec, D4Scalars P,
                                                                       int want_virial, double* __restrict__ row, double* __restrict__ dEdCN,
                                                                       double* __restrict__ fdir, float* __restrict__ charge_grad) {
  __shared__ __attribute__((aligned(16))) float lds[D4_WAVES][D4_SLOTS * 24];
  const int lane = threadIdx.x & (MI_WAVE - 1), wave = threadIdx.x / MI_WAVE;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * D4_WAVES + wave);
  const bool live = i < N;  // (no early return: every wave of the block meets the barriers below)
  const int S = info[0];
  D4Rec<T> ri;
  ri.x = ri.y = ri.z = T(0); ri.code = -1;
  if (live) ri = rec[i];
  const int ci = (int)ri.code;
  const bool shifted = ush != nullptr && cell != nullptr;
  T cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  long long beg = 0, end = 0;
  float wi[21];
#pragma unroll
  for (int k = 0; k < 21; ++k) wi[k] = 0.0f;
  if (ci >= 0) {
    if (shifted) d4_load_cell(cell, batch_idx, i, cm);
    if (CSR) { beg = nptr[i]; end = nptr[i + 1]; } else { beg = (long long)i * M; end = beg + M; }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int a = 0; a < D4_REFS; ++a) wi[7 * k + a] = wrec[D4_WREC * (size_t)i + 8 * k + a];
  }
  const unsigned jlim = d4_index_limit<CSR>(N, fill_value);
  float* mine = lds[wave];
  double eacc = 0.0, dcn = 0.0, dq = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
  double v[6] = {0, 0, 0, 0, 0, 0};
  for (int t0 = 0; t0 < S; t0 += D4_SLOTS) {  // (S is the same for every wave: uniform trip count)
    __syncthreads();                           // the previous group's readers are done
    if (ci >= 0) {
      // lane (tl, b) of trip p contracts species t0 + 8 p + tl: v^k[b] = sum_a w^k[a] c6[ci, t, a, b] for k = 0..2 from the same seven loads
#pragma unroll
      for (int p = 0; p < D4_SLOTS / 8; ++p) {
        const int slot = 8 * p + lane / 8, b = lane & 7, t = t0 + slot;
        float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
        if (t < S) {
          const float* c = cc6 + ((size_t)ci * S + t) * 56 + b;
#pragma unroll
          for (int a = 0; a < D4_REFS; ++a) {
            const float x = c[8 * a];
            o0 = fmaf(wi[a], x, o0); o1 = fmaf(wi[7 + a], x, o1); o2 = fmaf(wi[14 + a], x, o2);
          }
        }
        mine[slot * 24 + b] = o0; mine[slot * 24 + 8 + b] = o1; mine[slot * 24 + 16 + b] = o2;
      }
    }
    __syncthreads();
    for (long long e = beg + lane; e < end; e += MI_WAVE) {
      const int j = idx[e];
      if ((unsigned)j >= jlim) continue;
      const D4Rec<T> rj = rec[j];
      const int cj = (int)rj.code;
      const int slot = cj - t0;
      if (cj < 0 || slot < 0 || slot >= D4_SLOTS) continue;  // padding, or a species of another group
      float r, rx, ry, rz;
      if (!d4_geom(ri, rj, shifted, ush, e, cm, r, rx, ry, rz)) continue;
      const float4* wj4 = reinterpret_cast<const float4*>(wrec + D4_WREC * (size_t)j);
      const float4 wa = wj4[0], wb = wj4[1];
      const float4* vv = reinterpret_cast<const float4*>(mine + slot * 24);
      const float4 a0 = vv[0], a1 = vv[1], b0 = vv[2], b1 = vv[3], c0 = vv[4], c1 = vv[5];
      const float c6 = a0.x * wa.x + a0.y * wa.y + a0.z * wa.z + a0.w * wa.w + a1.x * wb.x + a1.y * wb.y + a1.z * wb.z + a1.w * wb.w;
      const float c6cn = b0.x * wa.x + b0.y * wa.y + b0.z * wa.z + b0.w * wa.w + b1.x * wb.x + b1.y * wb.y + b1.z * wb.z + b1.w * wb.w;
      const float c6q = c0.x * wa.x + c0.y * wa.y + c0.z * wa.z + c0.w * wa.w + c1.x * wb.x + c1.y * wb.y + c1.z * wb.z + c1.w * wb.w;
      const float* p = ptab + D4_PAIR * ((size_t)ci * S + cj);
      const float Q = p[2], r06 = p[3], r08 = p[4];
      const float r2 = r * r, r4 = r2 * r2, r6 = r4 * r2, r8 = r4 * r4;
      const float t6 = 1.0f / (r6 + r06), t8 = 1.0f / (r8 + r08);
      const float f = P.s6 * t6 + P.s8 * Q * t8;
      const float gr = 6.0f * P.s6 * r4 * t6 * t6 + 8.0f * P.s8 * Q * r6 * t8 * t8;  // -(df/dr) / r
      eacc += (double)(-0.5f * c6 * f);
      dcn += (double)(-f * c6cn);
      dq += (double)(-f * c6q);
      const float fm = c6 * gr;  // force on the owner: entry + mirror = c6 gr r
      fx += (double)(fm * rx); fy += (double)(fm * ry); fz += (double)(fm * rz);
      if (want_virial) {
        const float h = -0.5f * fm;
        v[0] += (double)(h * rx * rx); v[1] += (double)(h * ry * ry); v[2] += (double)(h * rz * rz);
        v[3] += (double)(h * rx * ry); v[4] += (double)(h * rx * rz); v[5] += (double)(h * ry * rz);
      }
    }
  }
  eacc = wave_sum(eacc); dcn = wave_sum(dcn); dq = wave_sum(dq);
  fx = wave_sum(fx); fy = wave_sum(fy); fz = wave_sum(fz);
  if (want_virial) {
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = wave_sum(v[k]);
  }
  if (live && lane == 0) {
    double* o = row + D4_ROW_WORDS * (size_t)i;
    o[0] = eacc;
    if (want_virial) {
#pragma unroll
      for (int k = 0; k < 6; ++k) o[1 + k] = v[k];
    }
    dEdCN[i] = dcn;
    charge_grad[i] = (float)dq;
    fdir[3 * (size_t)i] = fx; fdir[3 * (size_t)i + 1] = fy; fdir[3 * (size_t)i + 2] = fz;
  }
}

// ---- chain pass: F_i += sum_row (dE/dCN_i + dE/dCN_j) dcount/dr r^ -----------------------------------------------------------------------
template <class T, bool CSR>
__global__ __launch_bounds__(D4_WAVES * MI_WAVE) void d4_chain_kernel(const D4Rec<T>* __restrict__ rec, int N, const int* __restrict__ idx,
                                                                      const int* __restrict__ ush, const int* __restrict__ nptr, int M,
                                                                      int fill_value, const T* __restrict__ cell, const int* __restrict__ batch_idx,
                                                                      const int* __restrict__ info, const float* __restrict__ ptab, D4Scalars P,
                                                                      int want_virial, const double* __restrict__ dEdCN,
                                                                      const double* __restrict__ fdir, double* __restrict__ row,
                                                                      float* __restrict__ forces) {
  const int lane = threadIdx.x & (MI_WAVE - 1);
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * D4_WAVES + threadIdx.x / MI_WAVE);
  if (i >= N) return;
  const D4Rec<T> ri = rec[i];
  const int ci = (int)ri.code;
  double fx = 0.0, fy = 0.0, fz = 0.0;
  double v[6] = {0, 0, 0, 0, 0, 0};
  if (ci >= 0) {
    const int S = info[0];
    const bool shifted = ush != nullptr && cell != nullptr;
    T cm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (shifted) d4_load_cell(cell, batch_idx, i, cm);
    const unsigned jlim = d4_index_limit<CSR>(N, fill_value);
    const float di = (float)dEdCN[i];
    const float inv_sqrt_pi = 0.5641895835f;
    long long beg, end;
    if (CSR) { beg = nptr[i]; end = nptr[i + 1]; } else { beg = (long long)i * M; end = beg + M; }
    for (long long e = beg + lane; e < end; e += MI_WAVE) {
      const int j = idx[e];
      if ((unsigned)j >= jlim) continue;
      const D4Rec<T> rj = rec[j];
      const int cj = (int)rj.code;
      if (cj < 0) continue;
      float r, rx, ry, rz;
      if (!d4_geom(ri, rj, shifted, ush, e, cm, r, rx, ry, rz)) continue;
      if (P.cn_cut > 0.0f && r >= P.cn_cut) continue;
      const float* p = ptab + D4_PAIR * ((size_t)ci * S + cj);
      const float x = P.k_cn * (r * p[0] - 1.0f);
      const float dc_over_r = -p[1] * inv_sqrt_pi * P.k_cn * p[0] * expf(-x * x) / r;  // (dcount/dr) / r
      const float fm = (di + (float)dEdCN[j]) * dc_over_r;
      fx += (double)(fm * rx); fy += (double)(fm * ry); fz += (double)(fm * rz);
      if (want_virial) {
        const float h = -0.5f * fm;
        v[0] += (double)(h * rx * rx); v[1] += (double)(h * ry * ry); v[2] += (double)(h * rz * rz);
        v[3] += (double)(h * rx * ry); v[4] += (double)(h * rx * rz); v[5] += (double)(h * ry * rz);
      }
    }
  }
  fx = wave_sum(fx); fy = wave_sum(fy); fz = wave_sum(fz);
  if (want_virial) {
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] = wave_sum(v[k]);
  }
  if (lane == 0) {
    forces[3 * (size_t)i] = (float)(fdir[3 * (size_t)i] + fx);
    forces[3 * (size_t)i + 1] = (float)(fdir[3 * (size_t)i + 1] + fy);
    forces[3 * (size_t)i + 2] = (float)(fdir[3 * (size_t)i + 2] + fz);
    if (want_virial) {
      double* o = row + D4_ROW_WORDS * (size_t)i + 7;
#pragma unroll
      for (int k = 0; k < 6; ++k) o[k] = v[k];
    }
  }
}

// ---- fold: mi_system_fold of pair_row.h over the first `words` words of a row; all D4_ROW_WORDS are written (the others as zeros) ------------
__global__ __launch_bounds__(256) void d4_fold_kernel(const double* __restrict__ row, const int* __restrict__ batch_idx, int N, int words,
                                                      double* __restrict__ partial) {
  mi_system_fold<D4_ROW_WORDS, MI_FOLD_BLOCKS>(batch_idx, N, D4_ROW_WORDS, partial, [&](long long r, double* a) {
#pragma unroll
    for (int k = 0; k < D4_ROW_WORDS; ++k) if (k < words) a[k] += row[D4_ROW_WORDS * r + k];
  });
}

__global__ void d4_finish_kernel(const double* __restrict__ partial, int B, int want_virial, float* __restrict__ energy, float* __restrict__ virial) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 7 * B) return;
  const int s = t / 7, k = t - 7 * s;
  if (k > 0 && !want_virial) return;
  double x = 0.0;
  for (int q = 0; q < MI_FOLD_BLOCKS; ++q) {
    const double* p = partial + ((size_t)s * MI_FOLD_BLOCKS + q) * D4_ROW_WORDS;
    x += k == 0 ? p[0] : p[k] + p[6 + k];
  }
  if (k == 0) { energy[s] = (float)x; return; }
  float* o = virial + 9 * (size_t)s;
  const float f = (float)x;
  switch (k) {
    case 1: o[0] = f; break;
    case 2: o[4] = f; break;
    case 3: o[8] = f; break;
    case 4: o[1] = f; o[3] = f; break;
    case 5: o[2] = f; o[6] = f; break;
    default: o[5] = f; o[7] = f; break;
  }
}

struct D4Layout { size_t rec, cn64, wrec, dEdCN, fdir, row, partial, present, smap, zlist, info, ptab, cc6, total; };
D4Layout d4_layout(int N, int B, int nz) {
  D4Layout L;
  const size_t n = (size_t)(N > 0 ? N : 0), z = (size_t)(nz > 0 ? nz : 0), b = (size_t)(B > 0 ? B : 0);
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t at = off; off += mi_align(bytes); return at; };
  L.rec = take(sizeof(D4Rec<double>) * n);  // sized for the wider dtype
  L.cn64 = take(sizeof(double) * n);
  L.wrec = take(sizeof(float) * D4_WREC * n);
  L.dEdCN = take(sizeof(double) * n);
  L.fdir = take(sizeof(double) * 3 * n);
  L.row = take(sizeof(double) * D4_ROW_WORDS * n);
  L.partial = take(sizeof(double) * D4_ROW_WORDS * MI_FOLD_BLOCKS * b);
  L.present = take(sizeof(int) * z);
  L.smap = take(sizeof(int) * z);
  L.zlist = take(sizeof(int) * z);
  L.info = take(sizeof(int) * 4);
  L.ptab = take(sizeof(float) * D4_PAIR * z * z);
  L.cc6 = take(sizeof(float) * 56 * z * z);
  L.total = off;
  return L;
}

template <class T, bool CSR>
int d4_impl(const T* positions, const int32_t* numbers, int N, const int32_t* idx, const int32_t* ush, const int32_t* nptr, int M, int fill_value,
            const T* cell, const int32_t* bi, int B, const mi_d4_params* q, const float* charges, int want_virial, float* energy, float* forces,
            float* coord_num, float* charge_grad, float* virial, char* ws, const D4Layout& L, hipStream_t st) {
  D4Rec<T>* rec = reinterpret_cast<D4Rec<T>*>(ws + L.rec);
  double* cn64 = reinterpret_cast<double*>(ws + L.cn64);
  float* wrec = reinterpret_cast<float*>(ws + L.wrec);
  double* dEdCN = reinterpret_cast<double*>(ws + L.dEdCN);
  double* fdir = reinterpret_cast<double*>(ws + L.fdir);
  double* row = reinterpret_cast<double*>(ws + L.row);
  double* partial = reinterpret_cast<double*>(ws + L.partial);
  int* present = reinterpret_cast<int*>(ws + L.present);
  int* smap = reinterpret_cast<int*>(ws + L.smap);
  int* zlist = reinterpret_cast<int*>(ws + L.zlist);
  int* info = reinterpret_cast<int*>(ws + L.info);
  float* ptab = reinterpret_cast<float*>(ws + L.ptab);
  float* cc6 = reinterpret_cast<float*>(ws + L.cc6);
  const int nz = q->nz;
  const D4Scalars P = {q->a1, q->a2, q->s6, q->s8, q->k_cn, q->k4, q->k5, q->k6, q->wf, q->ga, q->gc, q->cn_cutoff > 0.0f ? q->cn_cutoff : 0.0f};
  const int rows = mi_blocks(N, D4_WAVES), per_atom = mi_blocks(N, 256);
  MI_HIP_CHECK(hipMemsetAsync(present, 0, sizeof(int) * (size_t)nz, st));
  MI_TIMED("d4_species", st, {
    d4_mark_species_kernel<<<per_atom, 256, 0, st>>>(numbers, N, nz, q->n_ref, present);
    d4_compact_species_kernel<<<1, 64, 0, st>>>(present, nz, smap, zlist, info);
    d4_tables_kernel<<<64, 256, 0, st>>>(zlist, info, nz, q->rcov, q->en, q->r4r2, q->n_ref, q->c6_ref, P, ptab, cc6);
  });
  MI_LAUNCH_CHECK();
  MI_TIMED("d4_pack", st, (d4_pack_kernel<T><<<per_atom, 256, 0, st>>>(positions, numbers, N, nz, smap, rec)));
  MI_TIMED("d4_cn", st, (d4_cn_kernel<T, CSR><<<rows, D4_WAVES * MI_WAVE, 0, st>>>(rec, N, idx, ush, nptr, M, fill_value, cell, bi, info, ptab, P, cn64,
                                                                                  coord_num)));
  MI_LAUNCH_CHECK();
  MI_TIMED("d4_weights", st, (d4_weights_kernel<<<per_atom, 256, 0, st>>>(numbers, charges, N, nz, q->n_ref, q->ngw, q->cn_ref, q->q_ref, q->zeff,
                                                                         q->gam, P, cn64, wrec)));
  MI_TIMED("d4_energy", st, (d4_energy_kernel<T, CSR><<<rows, D4_WAVES * MI_WAVE, 0, st>>>(rec, N, idx, ush, nptr, M, fill_value, cell, bi, info, ptab,
                                                                                          cc6, wrec, P, want_virial, row, dEdCN, fdir, charge_grad)));
  MI_LAUNCH_CHECK();
  MI_TIMED("d4_chain", st, (d4_chain_kernel<T, CSR><<<rows, D4_WAVES * MI_WAVE, 0, st>>>(rec, N, idx, ush, nptr, M, fill_value, cell, bi, info, ptab, P,
                                                                                        want_virial, dEdCN, fdir, row, forces)));
  MI_TIMED("d4_fold", st, {
    d4_fold_kernel<<<dim3(MI_FOLD_BLOCKS, B), 256, 0, st>>>(row, bi, N, want_virial ? D4_ROW_WORDS : 1, partial);
    d4_finish_kernel<<<mi_blocks(7ll * B, 256), 256, 0, st>>>(partial, B, want_virial, energy, virial);
  });
  MI_LAUNCH_CHECK();
  return MI_OK;
}

#include "d4_atm.h"  // the three-body term: the triple pass and its driver, on the kernels above

}  // namespace

extern "C" int mi_d4_species_slots(void) { return D4_SLOTS; }
extern "C" int mi_d4_fold_blocks(void) { return MI_FOLD_BLOCKS; }

extern "C" size_t mi_d4_workspace_bytes(int n_atoms, int n_systems, int nz) {
  if (n_atoms < 0 || nz < 1 || n_systems < 1) return 0;
  return d4_layout(n_atoms, n_systems, nz).total;
}

extern "C" int mi_d4(const void* positions, const int32_t* numbers, int n_atoms, int dtype, const int32_t* idx_j, const int32_t* unit_shifts,
                     const int32_t* neighbor_ptr, int max_neighbors, long long n_list_entries, int fill_value, const void* cell,
                     const int32_t* batch_idx, int n_systems, const mi_d4_params* params, const float* charges, int compute_virial, float* energy,
                     float* forces, float* coord_num, float* charge_grad, float* virial, void* workspace, size_t workspace_bytes, void* stream) {
  (void)n_list_entries;
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0 && n_systems >= 1, "sizes");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && numbers && params && charges && energy && forces && coord_num && charge_grad && workspace, "null pointer");
  MI_REQUIRE(idx_j || neighbor_ptr || max_neighbors == 0, "idx_j is NULL (only a CSR list without entries has none)");
  MI_REQUIRE(params->rcov && params->en && params->r4r2 && params->zeff && params->gam && params->n_ref && params->ngw && params->cn_ref &&
                 params->q_ref && params->c6_ref && params->nz >= 2,
             "D4 parameter tables");
  MI_REQUIRE(params->k6 > 0.0f, "k6 must be positive");
  MI_REQUIRE(!compute_virial || (virial && cell && unit_shifts), "virial needs its output, a cell and unit shifts");
  MI_REQUIRE(!unit_shifts || cell, "unit_shifts without a cell");
  const D4Layout L = d4_layout(n_atoms, n_systems, params->nz);
  if (workspace_bytes < L.total) { mi_set_error("workspace too small: %zu < %zu", workspace_bytes, L.total); return MI_EWORKSPACE; }
  MI_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;  // one system: every atom belongs to system 0 and the batch index is not read
  const bool csr = neighbor_ptr != nullptr;
#define MI_D4_CALL(T_, CSR_)                                                                                                                   \
  return d4_impl<T_, CSR_>((const T_*)positions, numbers, n_atoms, idx_j, unit_shifts, neighbor_ptr, max_neighbors, fill_value, (const T_*)cell, bi, \
                           n_systems, params, charges, compute_virial, energy, forces, coord_num, charge_grad, virial, (char*)workspace, L, st)
  if (dtype == MI_F32) { if (csr) MI_D4_CALL(float, true); else MI_D4_CALL(float, false); }
  else { if (csr) MI_D4_CALL(double, true); else MI_D4_CALL(double, false); }
#undef MI_D4_CALL
}

// ---- the three-body (Axilrod-Teller-Muto) term: csrc/d4_atm.h -----------------------------------------------------------------------------
extern "C" size_t mi_d4_atm_workspace_bytes(int n_atoms, int n_systems, int nz) {
  if (n_atoms < 0 || nz < 1 || n_systems < 1) return 0;
  return d4_atm_layout(n_atoms, n_systems, nz).total;
}

extern "C" size_t mi_d4_atm_visits_offset(int n_atoms, int n_systems, int nz) {
  if (n_atoms < 0 || nz < 1 || n_systems < 1) return 0;
  return d4_atm_layout(n_atoms, n_systems, nz).visits;
}

extern "C" int mi_d4_atm_tile(void) { return D4_ATM_TILE; }

extern "C" int mi_d4_atm(const void* positions, const int32_t* numbers, int n_atoms, int dtype, const int32_t* idx_j, const int32_t* unit_shifts,
                         const int32_t* neighbor_ptr, int max_neighbors, int fill_value, const void* cell, const int32_t* batch_idx, int n_systems,
                         const mi_d4_params* params, float s9, float alpha, float three_body_cutoff, int compute_virial, float* energy,
                         float* forces, float* virial, void* workspace, size_t workspace_bytes, void* stream) {
  MI_REQUIRE(dtype == MI_F32 || dtype == MI_F64, "dtype");
  MI_REQUIRE(n_atoms >= 0 && n_systems >= 1, "sizes");
  MI_REQUIRE(neighbor_ptr || max_neighbors >= 0, "max_neighbors must not be negative");
  MI_REQUIRE(n_systems == 1 || batch_idx, "batch_idx is required for more than one system");
  MI_REQUIRE(std::isfinite(three_body_cutoff) && three_body_cutoff > 0.0f && std::isfinite(alpha) && alpha > 0.0f,
             "three_body_cutoff and alpha must be positive and finite");
  MI_REQUIRE(std::isfinite(s9), "s9 must be finite");
  if (n_atoms == 0) return MI_OK;
  MI_REQUIRE(positions && numbers && params && energy && forces && workspace, "null pointer");
  MI_REQUIRE(idx_j || neighbor_ptr || max_neighbors == 0, "idx_j is NULL (only a CSR list without entries has none)");
  MI_REQUIRE(params->rcov && params->en && params->r4r2 && params->zeff && params->gam && params->n_ref && params->ngw && params->cn_ref &&
                 params->q_ref && params->c6_ref && params->nz >= 2,
             "D4 parameter tables");
  MI_REQUIRE(params->k6 > 0.0f, "k6 must be positive");
  MI_REQUIRE(!compute_virial || (virial && cell && unit_shifts), "virial needs its output, a cell and unit shifts");
  MI_REQUIRE(!unit_shifts || cell, "unit_shifts without a cell");
  const D4AtmLayout L = d4_atm_layout(n_atoms, n_systems, params->nz);
  if (workspace_bytes < L.total) { mi_set_error("workspace too small: %zu < %zu", workspace_bytes, L.total); return MI_EWORKSPACE; }
  MI_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int32_t* bi = n_systems > 1 ? batch_idx : nullptr;  // one system: every atom belongs to system 0 and the batch index is not read
  const bool csr = neighbor_ptr != nullptr;
#define MI_D4_ATM_CALL(T_, CSR_)                                                                                                                       \
  return d4_atm_impl<T_, CSR_>((const T_*)positions, numbers, n_atoms, idx_j, unit_shifts, neighbor_ptr, max_neighbors, fill_value, (const T_*)cell, bi, \
                               n_systems, params, s9, alpha, three_body_cutoff, compute_virial, energy, forces, virial, (char*)workspace, L, st)
  if (dtype == MI_F32) { if (csr) MI_D4_ATM_CALL(float, true); else MI_D4_ATM_CALL(float, false); }
  else { if (csr) MI_D4_ATM_CALL(double, true); else MI_D4_ATM_CALL(double, false); }
#undef MI_D4_ATM_CALL
}
