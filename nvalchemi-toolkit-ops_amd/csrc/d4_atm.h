// d4_atm.h -- DFT-D4 three-body (Axilrod-Teller-Muto) term: the triple pass and its driver (mi_d4_atm).  Included by d4.hip inside its
// anonymous namespace: the species compaction and the dense tables, the packed records, the coordination-number pass, the weight kernel,
// the chain-rule pass (linear in dE/dCN, so it runs unchanged on the three-body dE/dCN) and the fixed-order fold are the two-body code's
// own kernels, launched exactly as mi_d4 launches them.
//
// The triangle energy is atm_core.h's E_ABC, with D4's pair coefficients and the BJ radii (a triple with any C6 < 1e-12 contributes nothing):
//   C6_XY = sum_ab w_X[a] c6_ref[Z_X, Z_Y, a, b] w_Y[b],   w_X[a] = W_a(CN_X) zeta_a(q = 0)       (the weight kernel on a zeroed charge array)
//   R0_XY = a1 sqrt(3 r4r2_X r4r2_Y) + a2
// The triple pass -- the triangle, its schedule, the ordinal staging, the tile-pair loop and the block reduction -- is csrc/atm_core.h's,
// shared with the DFT-D3 kernel; read the algorithm there.  This file keeps what is D4's: the record tail (the neighbour's eight weights; 16
// floats per record), C6_ij and C6_jk from the `ctr` and `strip` contractions, the fp64 row words written through pointers parked in LDS,
// the workspace layout and the host driver -- and ITS OWN TEXT of the accumulators and of the per-triple arithmetic, which is atm_core.h's
// atm_triple line for line: d4.hip is built with the SLP vectoriser on, and through AtmAcc / atm_triple it packed the visit's products
// differently (forces moved in the last bit, the pass ran 0.5 - 1.9 % slower).  A fix to the arithmetic goes into both places.
//
// The C6 values, the energy pass's contraction applied twice:
//   centre      the block contracts w_i and dw_i/dCN with cc6[c_i, t, :, :] once for the first D4_SLOTS species t (LDS `ctr`); C6_ij and its
//               CN derivative are two 8-term dot products against the neighbour's weights when its record is staged.
//   pair (p, q) for each row p the wave contracts w_p with cc6[c_p, t, :, :] for the first D4_SLOTS species into its own LDS strip; C6_pq is
//               one 8-term dot product per lane against the staged weights of q.
//   A neighbour whose species id is >= D4_SLOTS takes the direct 49-term form from cc6 (through L1) in both places: slower, the same sums.
// LDS per block: two tiles 2 x 16 x D4_ATM_TILE x 4 B + ctr 1 KB + strips 2 KB + reduction + the parked block-uniform values: 40 432 B
// (fp32 positions) / 40 480 B (fp64) at 288 records per tile, i.e. four blocks (16 waves) per CU of 160 KB, as for the D3 triple pass.
// Block-uniform values that are needed only while staging (the cell, the centre's position) or only in the last lines (the output
// pointers) are parked in LDS: held in scalar registers through every loop they made the kernel spill SGPRs.
#pragma once
#include "atm_core.h"

#define D4_ATM_TILE 288   // staged records per LDS tile
#define D4_ATM_REC 16     // floats per record

// a wave's own LDS writes become visible to its own later reads (the strip is private to the wave: no block barrier)
__device__ __forceinline__ void d4_atm_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// sum_a u[a] sum_b c[8 a + b] v[b] twice (u0, u1) from the same 56 table words: the direct form for species outside the LDS slots
__device__ __forceinline__ void d4_atm_direct(const float* __restrict__ c, const float* u0, const float* u1, const float* v, float& o0, float& o1) {
  o0 = 0.0f; o1 = 0.0f;
#pragma unroll
  for (int a = 0; a < D4_REFS; ++a) {
    float s = 0.0f;
#pragma unroll
    for (int b = 0; b < 8; ++b) s = fmaf(c[8 * a + b], v[b], s);
    o0 = fmaf(u0[a], s, o0);
    if (u1) o1 = fmaf(u1[a], s, o1);
  }
}

template <class T, bool CSR, bool VIR>
__global__ __launch_bounds__(ATM_WAVES * MI_WAVE) void d4_atm_kernel(const D4Rec<T>* __restrict__ rec, int N, const int* __restrict__ idx,
                                                                        const int* __restrict__ ush, const int* __restrict__ nptr, int M,
                                                                        int fill_value, const T* __restrict__ cell, const int* __restrict__ batch_idx,
                                                                        const int* __restrict__ info, const float* __restrict__ ptab,
                                                                        const float* __restrict__ cc6, const float* __restrict__ wrec, D4Scalars P,
                                                                        AtmParams A, double* __restrict__ row,
                                                                        double* __restrict__ dEdCN, double* __restrict__ fdir) {
  __shared__ __attribute__((aligned(16))) float tiles[2][D4_ATM_REC][D4_ATM_TILE];
  __shared__ __attribute__((aligned(16))) float ctr[D4_SLOTS][16];                  // [slot][k = 0 (w_i), 1 (dw_i/dCN)][8]
  __shared__ __attribute__((aligned(16))) float strip[ATM_WAVES][D4_SLOTS * 8];  // per wave: [slot][8] of its current row p
  __shared__ double red[ATM_WAVES][12];
  __shared__ int cnt_sh[2][ATM_WAVES];
  __shared__ void* out_sh[4];  // the output pointers, parked for the block's last lines (scalar registers again)
  __shared__ T geo[12];  // the cell of the centre's system (zero without shifts) and the centre's position
  const int i = blockIdx.x;
  const int lane = threadIdx.x & (MI_WAVE - 1), wave = threadIdx.x / MI_WAVE;
  const D4Rec<T> ri = rec[i];
  const int ci = (int)ri.code;
  if (ci < 0) {  // (block-uniform) padding: part of no triple; the chain pass and the fold read these words
    if (threadIdx.x == 0) {
      double* o = row + D4_ROW_WORDS * (size_t)i;
      o[0] = 0.0;
      if constexpr (VIR) {
#pragma unroll
        for (int k = 0; k < 6; ++k) o[1 + k] = 0.0;
      }
      dEdCN[i] = 0.0;
      fdir[3 * (size_t)i] = 0.0; fdir[3 * (size_t)i + 1] = 0.0; fdir[3 * (size_t)i + 2] = 0.0;
    }
    return;
  }
  if (threadIdx.x == 0) {  // (already offset to this centre: the last lines need no index)
    out_sh[0] = row + D4_ROW_WORDS * (size_t)i; out_sh[1] = dEdCN + i; out_sh[2] = fdir + 3 * (size_t)i;
    out_sh[3] = A.visits ? A.visits + i : nullptr;
  }
  const int S = info[0];
  const int ns = min(S, D4_SLOTS);
  const bool shifted = ush != nullptr && cell != nullptr;
  const unsigned jlim = d4_index_limit<CSR>(N, fill_value);
  long long beg;
  int len;  // (a row holds fewer than 2^31 entries in either layout)
  if (CSR) { beg = nptr[i]; len = nptr[i + 1] - nptr[i]; } else { beg = (long long)i * M; len = M; }
  const int* __restrict__ idx_row = idx + beg;
  const int* __restrict__ ush_row = shifted ? ush + 3 * beg : nullptr;  // (null: no shifts are read)
  if (threadIdx.x < 9) geo[threadIdx.x] = shifted ? cell[9 * (size_t)(batch_idx ? batch_idx[i] : 0) + threadIdx.x] : T(0);
  if (threadIdx.x == 9) { geo[9] = ri.x; geo[10] = ri.y; geo[11] = ri.z; }
  if (threadIdx.x < D4_SLOTS * 8) {
    const int slot = threadIdx.x / 8, b = threadIdx.x & 7;
    float o0 = 0.0f, o1 = 0.0f;
    if (slot < ns) {
      const float* wi = wrec + D4_WREC * (size_t)i;  // w_i[0..7], dw_i/dCN[8..15]
      const float* c = cc6 + ((size_t)ci * S + slot) * 56 + b;
#pragma unroll
      for (int a = 0; a < D4_REFS; ++a) {
        const float x = c[8 * a];
        o0 = fmaf(wi[a], x, o0); o1 = fmaf(wi[8 + a], x, o1);
      }
    }
    ctr[slot][b] = o0; ctr[slot][8 + b] = o1;
  }
  __syncthreads();

  // Streams the row once and stages the kept entries whose ordinal (count of kept entries in row order) lies in [k_lo, k_lo + TILE).
  // Returns the number of kept entries of the whole row.  Block-cooperative; ends with a barrier.
  auto stage = [&](float (*tile)[D4_ATM_TILE], int k_lo) -> int {
    int running = 0, par = 0;
    for (int e0 = 0; e0 < len; e0 += ATM_WAVES * MI_WAVE, par ^= 1) {
      const int e = e0 + (int)threadIdx.x;
      bool keep = false;
      int j = i, cj = -1;
      float r = 0.0f, rx = 0.0f, ry = 0.0f, rz = 0.0f;
      if (e < len) {
        const int jr = idx_row[e];
        if ((unsigned)jr < jlim) {
          const D4Rec<T> rj = rec[jr];
          // the centre and its cell come from LDS (broadcast reads, short-lived vector registers): as block-uniform scalars they would
          // compete with the kernel's pointers for scalar registers through every loop of the kernel
          D4Rec<T> rc;
          rc.x = geo[9]; rc.y = geo[10]; rc.z = geo[11]; rc.code = 0;
          T cm[9];
#pragma unroll
          for (int k = 0; k < 9; ++k) cm[k] = geo[k];
          if ((int)rj.code >= 0 && d4_geom(rc, rj, ush_row != nullptr, ush_row, e, cm, r, rx, ry, rz) && (rx * rx + ry * ry + rz * rz < A.rc2)) {
            keep = true; j = jr; cj = (int)rj.code;
          }
        }
      }
      int total;
      const int slot = atm_stage_slot(keep, cnt_sh, par, running, k_lo, lane, wave, total);
      if (keep && slot >= 0 && slot < D4_ATM_TILE) {
        const float4* wj4 = reinterpret_cast<const float4*>(wrec + D4_WREC * (size_t)j);
        const float4 wa = wj4[0], wb = wj4[1];
        float c6, dci;
        if (cj < D4_SLOTS) {
          const float4* vv = reinterpret_cast<const float4*>(ctr[cj]);
          const float4 a0 = vv[0], a1 = vv[1], b0 = vv[2], b1 = vv[3];
          c6 = a0.x * wa.x + a0.y * wa.y + a0.z * wa.z + a0.w * wa.w + a1.x * wb.x + a1.y * wb.y + a1.z * wb.z + a1.w * wb.w;
          dci = b0.x * wa.x + b0.y * wa.y + b0.z * wa.z + b0.w * wa.w + b1.x * wb.x + b1.y * wb.y + b1.z * wb.z + b1.w * wb.w;
        } else {
          const float wj[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
          const float* wi = wrec + D4_WREC * (size_t)i;
          d4_atm_direct(cc6 + ((size_t)ci * S + cj) * 56, wi, wi + 8, wj, c6, dci);
        }
        const bool live = !(c6 < 1e-12f);  // a triple with any C6 < 1e-12 contributes nothing: sqrt(C6) = 0 zeroes every term of it
        tile[ATM_RX][slot] = rx; tile[ATM_RY][slot] = ry; tile[ATM_RZ][slot] = rz;
        tile[ATM_SC][slot] = live ? sqrtf(c6) : 0.0f;
        tile[ATM_G][slot] = live ? dci / c6 : 0.0f;
        tile[ATM_R0][slot] = P.a1 * sqrtf(ptab[D4_PAIR * ((size_t)ci * S + cj) + 2]) + P.a2;
        tile[ATM_H][slot] = sqrtf(sqrtf(ptab[D4_PAIR * ((size_t)cj * S + cj) + 2]));  // h_j h_k = sqrt(3 r4r2_j r4r2_k)
        tile[ATM_CODE][slot] = __int_as_float(cj);
        tile[ATM_TAIL + 0][slot] = wa.x; tile[ATM_TAIL + 1][slot] = wa.y; tile[ATM_TAIL + 2][slot] = wa.z; tile[ATM_TAIL + 3][slot] = wa.w;
        tile[ATM_TAIL + 4][slot] = wb.x; tile[ATM_TAIL + 5][slot] = wb.y; tile[ATM_TAIL + 6][slot] = wb.z; tile[ATM_TAIL + 7][slot] = wb.w;
      }
      running += total;
    }
    __syncthreads();
    return running;
  };

  double Fx = 0, Fy = 0, Fz = 0, E = 0, dacc = 0;
  float V[6] = {0, 0, 0, 0, 0, 0};  // xx yy zz xy xz yz: fp32 lane partials flushed into fp64 once per row of the triangle
  double V6[6] = {0, 0, 0, 0, 0, 0};
  unsigned visits = 0;
  const float alpha3 = A.alpha * (1.0f / 3.0f);
  float* mine = strip[wave];

  // all pairs (p in tile tp, q in tile tq); same tile: q > p
  auto pairs = [&](const float (*tp)[D4_ATM_TILE], int np, const float (*tq)[D4_ATM_TILE], int nq, bool same) {
    for (int p = wave; p < np; p += ATM_WAVES) {
      const int q0 = same ? p + 1 : 0;
      if (q0 >= nq) continue;  // (wave-uniform)
      const float px = tp[ATM_RX][p], py = tp[ATM_RY][p], pz = tp[ATM_RZ][p];  // wave-uniform: LDS broadcasts
      const float scp = tp[ATM_SC][p], gp = tp[ATM_G][p], r0p = tp[ATM_R0][p], hp = tp[ATM_H][p];
      const int cp = __float_as_int(tp[ATM_CODE][p]);
      // the wave's strip: v_t[b] = sum_a w_p[a] c6[c_p, t, a, b] for the species in the slots; lane (tl, b) of trip k takes t = 8 k + tl
      d4_atm_wave_sync();  // the readers of the previous row are done
      for (int k = 0; 8 * k < ns; ++k) {
        const int t = 8 * k + lane / 8, b = lane & 7;
        float o = 0.0f;
        if (t < ns) {
          const float* c = cc6 + ((size_t)cp * S + t) * 56 + b;
#pragma unroll
          for (int a = 0; a < D4_REFS; ++a) o = fmaf(tp[ATM_TAIL + a][p], c[8 * a], o);
        }
        mine[t * 8 + b] = o;
      }
      d4_atm_wave_sync();
      const float a = px * px + py * py + pz * pz;
      const float inva = __builtin_amdgcn_rcpf(a);
      for (int q = q0 + lane; q < nq; q += MI_WAVE) {
        const float qx = tq[ATM_RX][q], qy = tq[ATM_RY][q], qz = tq[ATM_RZ][q];
        const float jx = qx - px, jy = qy - py, jz = qz - pz;  // r_jk
        const float c = jx * jx + jy * jy + jz * jz;
        if (!(c < A.rc2) || c < 1e-24f) continue;
        ++visits;
        const int cq = __float_as_int(tq[ATM_CODE][q]);
        float wq[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) wq[b] = tq[ATM_TAIL + b][q];
        float c6jk;
        if (cq < D4_SLOTS) {
          const float4* sv = reinterpret_cast<const float4*>(mine + cq * 8);
          const float4 s0 = sv[0], s1 = sv[1];
          c6jk = s0.x * wq[0] + s0.y * wq[1] + s0.z * wq[2] + s0.w * wq[3] + s1.x * wq[4] + s1.y * wq[5] + s1.z * wq[6] + s1.w * wq[7];
        } else {
          float unused, wp[D4_REFS];
#pragma unroll
          for (int a = 0; a < D4_REFS; ++a) wp[a] = tp[ATM_TAIL + a][p];
          d4_atm_direct(cc6 + ((size_t)cp * S + cq) * 56, wp, nullptr, wq, c6jk, unused);
        }
        const float sjk = c6jk < 1e-12f ? 0.0f : __builtin_amdgcn_sqrtf(c6jk);
        const float b = qx * qx + qy * qy + qz * qz;
        // a + b - c = 2 r_ij.r_ik etc.: the three factors as dot products, not as differences of squared lengths
        const float x = 2.0f * (px * qx + py * qy + pz * qz), y = -2.0f * (px * jx + py * jy + pz * jz), z = 2.0f * (qx * jx + qy * jy + qz * jz);
        const float pinv = __builtin_amdgcn_rsqf(a * b * c);
        const float pinv3 = pinv * pinv * pinv, k5 = 0.375f * pinv3 * pinv * pinv;
        const float yz = y * z, xz = x * z, xy = x * y, nn = xy * z;
        const float ang = fmaf(k5, nn, pinv3);
        const float r0 = r0p * tq[ATM_R0][q] * fmaf(P.a1, hp * tq[ATM_H][q], P.a2);
        // (R0 / P)^(alpha / 3) with a runtime exponent: one log2 / exp2 pair per triple
        const float t = __builtin_amdgcn_exp2f(alpha3 * __builtin_amdgcn_logf(r0 * pinv));
        const float fd = __builtin_amdgcn_rcpf(fmaf(6.0f, t, 1.0f));
        const float c9 = A.s9 * scp * tq[ATM_SC][q] * sjk;
        const float e = c9 * ang * fd;
        // dE/da = C9 fd (k5 dN/da + B0 / a),  B0 = ang fd t alpha - (2.5 k5 N + 1.5 / P^3); likewise b, c
        const float b0 = ang * fd * t * A.alpha - fmaf(2.5f * k5, nn, 1.5f * pinv3);
        const float cf = c9 * fd;
        const float dEda = cf * fmaf(k5, yz + xz - xy, b0 * inva);
        const float dEdb = cf * fmaf(k5, yz - xz + xy, b0 * __builtin_amdgcn_rcpf(b));
        E += (double)e;
        dacc += (double)(0.5f * e * (gp + tq[ATM_G][q]));
        const float fx = 2.0f * (dEda * px + dEdb * qx), fy = 2.0f * (dEda * py + dEdb * qy), fz = 2.0f * (dEda * pz + dEdb * qz);
        Fx += (double)fx; Fy += (double)fy; Fz += (double)fz;
        if constexpr (VIR) {
          const float dEdc = cf * fmaf(k5, xz + xy - yz, b0 * __builtin_amdgcn_rcpf(c));
          const float ax = dEda * px, ay = dEda * py, az = dEda * pz, bx = dEdb * qx, by = dEdb * qy, bz = dEdb * qz;
          const float cx = dEdc * jx, cy = dEdc * jy, cz = dEdc * jz;
          V[0] += ax * px + bx * qx + cx * jx; V[1] += ay * py + by * qy + cy * jy; V[2] += az * pz + bz * qz + cz * jz;
          V[3] += ax * py + bx * qy + cx * jy; V[4] += ax * pz + bx * qz + cx * jz; V[5] += ay * pz + by * qz + cy * jz;
        }
      }
      if constexpr (VIR) {
#pragma unroll
        for (int k = 0; k < 6; ++k) { V6[k] += (double)V[k]; V[k] = 0.0f; }
      }
    }
  };

  atm_tile_pairs(stage, pairs, tiles);
  const double r12[12] = {E, Fx, Fy, Fz, dacc, V6[0], V6[1], V6[2], V6[3], V6[4], V6[5], (double)visits};
  atm_block_reduce(r12, red, lane, wave, VIR);
  if (threadIdx.x == 0) {
    double* o = static_cast<double*>(out_sh[0]);
    double* dcn_o = static_cast<double*>(out_sh[1]);
    double* f_o = static_cast<double*>(out_sh[2]);
    unsigned* vis_o = static_cast<unsigned*>(out_sh[3]);
    f_o[0] = red[0][1]; f_o[1] = red[0][2]; f_o[2] = red[0][3];
    dcn_o[0] = red[0][4];
    o[0] = red[0][0] * (1.0 / 3.0);
    if constexpr (VIR) {
      // per edge dE/dr / r = 2 dE/d(r^2); a third of the triangle's -sum_edges (dE/dr / r) r (x) r per visit
#pragma unroll
      for (int k = 0; k < 6; ++k) o[1 + k] = -(2.0 / 3.0) * red[0][5 + k];
    }
    if (vis_o) vis_o[0] = (unsigned)red[0][11];
  }
}

struct D4AtmLayout { D4Layout base; size_t q0, cn, visits, total; };
D4AtmLayout d4_atm_layout(int N, int B, int nz) {
  D4AtmLayout L;
  L.base = d4_layout(N, B, nz);
  const size_t n = (size_t)(N > 0 ? N : 0);
  L.q0 = L.base.total;
  L.cn = L.q0 + mi_align(sizeof(float) * n);
  L.visits = L.cn + mi_align(sizeof(float) * n);
  L.total = L.visits + mi_align(sizeof(unsigned) * n);
  return L;
}

template <class T, bool CSR>
int d4_atm_impl(const T* positions, const int32_t* numbers, int N, const int32_t* idx, const int32_t* ush, const int32_t* nptr, int M, int fill_value,
                const T* cell, const int32_t* bi, int B, const mi_d4_params* q, float s9, float alpha, float cutoff, int want_virial, float* energy,
                float* forces, float* virial, char* ws, const D4AtmLayout& LA, hipStream_t st) {
  const D4Layout& L = LA.base;
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
  float* q0 = reinterpret_cast<float*>(ws + LA.q0);
  float* cn = reinterpret_cast<float*>(ws + LA.cn);
  unsigned* visits = reinterpret_cast<unsigned*>(ws + LA.visits);
  const int nz = q->nz;
  const D4Scalars P = {q->a1, q->a2, 0.0f, 0.0f, q->k_cn, q->k4, q->k5, q->k6, q->wf, q->ga, q->gc, q->cn_cutoff > 0.0f ? q->cn_cutoff : 0.0f};
  const int rows = mi_blocks(N, D4_WAVES), per_atom = mi_blocks(N, 256);
  MI_HIP_CHECK(hipMemsetAsync(present, 0, sizeof(int) * (size_t)nz, st));
  MI_HIP_CHECK(hipMemsetAsync(q0, 0, sizeof(float) * (size_t)N, st));  // the charge scaling of the three-body term is zeta(q = 0)
  MI_HIP_CHECK(hipMemsetAsync(visits, 0, sizeof(unsigned) * (size_t)N, st));
  MI_TIMED("d4_atm_species", st, {
    d4_mark_species_kernel<<<per_atom, 256, 0, st>>>(numbers, N, nz, q->n_ref, present);
    d4_compact_species_kernel<<<1, 64, 0, st>>>(present, nz, smap, zlist, info);
    d4_tables_kernel<<<64, 256, 0, st>>>(zlist, info, nz, q->rcov, q->en, q->r4r2, q->n_ref, q->c6_ref, P, ptab, cc6);
  });
  MI_LAUNCH_CHECK();
  MI_TIMED("d4_atm_pack", st, (d4_pack_kernel<T><<<per_atom, 256, 0, st>>>(positions, numbers, N, nz, smap, rec)));
  // 1. coordination numbers over the WHOLE list, then the weights at q = 0
  MI_TIMED("d4_atm_cn", st, (d4_cn_kernel<T, CSR><<<rows, D4_WAVES * MI_WAVE, 0, st>>>(rec, N, idx, ush, nptr, M, fill_value, cell, bi, info, ptab, P, cn64,
                                                                                      cn)));
  MI_LAUNCH_CHECK();
  MI_TIMED("d4_atm_weights", st, (d4_weights_kernel<<<per_atom, 256, 0, st>>>(numbers, q0, N, nz, q->n_ref, q->ngw, q->cn_ref, q->q_ref, q->zeff,
                                                                             q->gam, P, cn64, wrec)));
  // 2. triples
  const AtmParams A{s9, alpha, cutoff * cutoff, visits};
  MI_TIMED("d4_atm_triples", st, {
    if (want_virial)
      d4_atm_kernel<T, CSR, true><<<N, ATM_WAVES * MI_WAVE, 0, st>>>(rec, N, idx, ush, nptr, M, fill_value, cell, bi, info, ptab, cc6, wrec, P, A, row, dEdCN, fdir);
    else
      d4_atm_kernel<T, CSR, false><<<N, ATM_WAVES * MI_WAVE, 0, st>>>(rec, N, idx, ush, nptr, M, fill_value, cell, bi, info, ptab, cc6, wrec, P, A, row, dEdCN, fdir);
  });
  MI_LAUNCH_CHECK();
  // 3. chain rule through the coordination numbers, over the whole list; 4. per-system sums
  MI_TIMED("d4_atm_chain", st, (d4_chain_kernel<T, CSR><<<rows, D4_WAVES * MI_WAVE, 0, st>>>(rec, N, idx, ush, nptr, M, fill_value, cell, bi, info, ptab, P,
                                                                                            want_virial, dEdCN, fdir, row, forces)));
  MI_TIMED("d4_atm_fold", st, {
    d4_fold_kernel<<<dim3(MI_FOLD_BLOCKS, B), 256, 0, st>>>(row, bi, N, want_virial ? D4_ROW_WORDS : 1, partial);
    d4_finish_kernel<<<mi_blocks(7ll * B, 256), 256, 0, st>>>(partial, B, want_virial, energy, virial);
  });
  MI_LAUNCH_CHECK();
  return MI_OK;
}
