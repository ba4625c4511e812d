// d3_atm.h -- DFT-D3 three-body (Axilrod-Teller-Muto) term: the triple pass and its driver.  Included by d3.hip inside its anonymous
// namespace: the coordination-number pass, the species compaction, the chain-rule pass and the per-system reduction are the two-body
// code's own kernels (the chain pass is linear in dE/dCN, so it runs unchanged on the three-body dE/dCN).
//
// The triple pass itself -- the triangle, its schedule, the ordinal staging, the per-triple arithmetic, the accumulators and the block
// reduction -- is csrc/atm_core.h's, shared with the DFT-D4 kernel; read the algorithm there.  This file keeps what is D3's: the record
// tail (the five factorised Gaussian weights of j, or CN_j), C6_jk from the three table MODEs, the radii of the two DAMPs, the fp32
// outputs with a 3x3 per-atom virial, the workspace layout and the host driver.  R0_XY = a1 sqrt(3 r4r2_X r4r2_Y) + a2 with D3_DAMP_BJ.
//
// DAMP (compile-time, as in the two-body energy pass): D3_DAMP_BJ takes the radii from the BJ parameters as above; D3_DAMP_ZERO
// (mi_d3_zero_atm) takes R0_XY = rs9 r0ab[Z_X, Z_Y] from the table of pair cutoff radii.  The radius of a species pair rides where its c6
// does: the table kernels are run with D3ZeroSpec{r0ab, 1, 1, rs9}, whose third value per pair (D3ZeroPair::bR = "beta R0") IS rs9 R0 -- the
// fourth float behind the factorised c6 rows (in LDS with them for <= D3_ATM_LDS_S species, through L1 otherwise), the spare word of entry 2
// of the 25-entry tables (MODE 0 / 1).  So the centre-neighbour radius is staged per tile slot as before and the neighbour-neighbour
// radius is one more read next to the c6 of that pair, indexed by the two species codes the tile already holds; no argument and no LDS is
// added.  A pair whose radius is <= 0 is stored as 0 and takes every triple it is part of out (its sqrt(C6) is staged / taken as 0).
#pragma once
#include "atm_core.h"

#define D3_ATM_TILE 320   // staged records per LDS tile; two tiles + the species table = 40 KB per block: four blocks (16 waves) per CU
#define D3_ATM_REC 13     // floats per record
#define D3_ATM_LDS_S 6    // factorised form: up to this many species keep the whole [S][S] c6 table in LDS (6.2 KB); more read it through L1
#define D3_ATM_E12 6.14421235e-06f  // e^-12: the reference's cut on a Gaussian weight relative to the dominant one

struct D3AtmMath { static __device__ __forceinline__ float rcp(float x) { return D3_RCP(x); } };  // (the IEEE divide in the test library)

// C6 of the pair (record p, record q) of two staged neighbours: no derivative (the visits from j and from k carry it)
template <int MODE>
__device__ __forceinline__ float d3_atm_c6_jk(const float (*tp)[D3_ATM_TILE], int p, const float (*tq)[D3_ATM_TILE], int q, int S, int nz,
                                              const float* ft, const float4* __restrict__ t25base, float k3) {
  const int cp = __float_as_int(tp[ATM_CODE][p]), cq = __float_as_int(tq[ATM_CODE][q]);
  if constexpr (MODE == 2) {
    const float* rows = ft + (size_t)(cp * S + cq) * D3_FROW;
    float w = 0.0f, z = 0.0f;
#pragma unroll
    for (int a = 0; a < 5; ++a) {
      const float va = tp[ATM_TAIL + a][p];  // wave-uniform
      if (__builtin_amdgcn_readfirstlane(__float_as_int(va)) == 0) continue;
#pragma unroll
      for (int b = 0; b < 5; ++b) {
        float L = va * tq[ATM_TAIL + b][q];
        L = L >= D3_ATM_E12 ? L : 0.0f;
        w += L;
        z = fmaf(L, rows[a * 8 + b], z);
      }
    }
    return w > 1e-12f ? z * D3_RCP(w) : 0.0f;
  } else {
    const float4* t25 = t25base + (size_t)(cp * (MODE == 1 ? S : nz) + cq) * 25;
    float c6, dci;
    d3_c6(tp[ATM_TAIL][p], tq[ATM_TAIL][q], t25, k3, c6, dci);
    return c6;
  }
}

// rs9 r0ab of the pair of two species codes (D3_DAMP_ZERO), from the table the c6 of that pair is read from
template <int MODE>
__device__ __forceinline__ float d3_atm_radius(int cp, int cq, int S, int nz, const float* ft, const float4* __restrict__ t25base) {
  if constexpr (MODE == 2) return ft[(size_t)(cp * S + cq) * D3_FROW + 43];
  else return t25base[(size_t)(cp * (MODE == 1 ? S : nz) + cq) * 25 + 2].w;
}

template <class T, bool CSR, int MODE, int DAMP>
__global__ __launch_bounds__(ATM_WAVES * MI_WAVE) void d3_atm_kernel(
    const T* __restrict__ pos, const int* __restrict__ numbers, int N, const int* __restrict__ idx, const int* __restrict__ ush,
    const int* __restrict__ nptr, int M, int fill_value, const T* __restrict__ cell, const int* __restrict__ batch_idx, D3Dev P, AtmParams A,
    const float* __restrict__ cn, int want_virial, const int* __restrict__ smap, const D3Species* __restrict__ sinfo,
    const float4* __restrict__ ctab, const float* __restrict__ ftab, const float* __restrict__ fcr,
    const typename Vec4<T>::type* __restrict__ apos, const float4* __restrict__ aaux, const float4* __restrict__ aw,
    float* __restrict__ dEdCN, float* __restrict__ forces, float* __restrict__ e_atom, double* __restrict__ v_atom) {
  __shared__ float tiles[2][D3_ATM_REC][D3_ATM_TILE];
  __shared__ float ft_lds[MODE == 2 ? D3_ATM_LDS_S * D3_ATM_LDS_S * D3_FROW : 1];
  __shared__ double red[ATM_WAVES][12];
  __shared__ int cnt_sh[2][ATM_WAVES];
  const int S = sinfo->S;
  const int want_mode = S > D3_SMAX ? 0 : (sinfo->factorized ? 2 : 1);
  if (want_mode != MODE) return;  // all three variants are launched, as for the two-body energy pass
  const int i = blockIdx.x;
  const int zi = numbers[i];
  if (zi <= 0 || zi >= P.nz) return;  // (block-uniform) outputs of such atoms stay zero
  const int lane = threadIdx.x & (MI_WAVE - 1), wave = threadIdx.x / MI_WAVE;
  const bool periodic = (cell != nullptr) && (ush != nullptr);
  T cm[9];
  if (periodic) { const T* c = cell + 9 * (size_t)(batch_idx ? batch_idx[i] : 0); for (int k = 0; k < 9; ++k) cm[k] = d3_uni(c[k]); }
  const T pix = d3_uni(pos[3 * (size_t)i]), piy = d3_uni(pos[3 * (size_t)i + 1]), piz = d3_uni(pos[3 * (size_t)i + 2]);
  const float cn_i = d3_uni(cn[i]), r4r2_i = d3_uni(P.r4r2[zi]);
  const int si = MODE == 0 ? zi : smap[zi];  // the code the tables of this MODE are indexed by
  D3Half hi;
  const float* ft = ftab;
  if constexpr (MODE == 2) {
    hi = d3_half_i(cn_i, fcr + si * 8, P.k3);
    if (S <= D3_ATM_LDS_S) {
      for (int k = threadIdx.x; k < S * S * D3_FROW; k += blockDim.x) ft_lds[k] = ftab[k];
      ft = ft_lds;
    }
  }
  const float4* __restrict__ t25base = MODE == 1 ? ctab : P.tab;
  long long beg, end;
  d3_row<T, CSR>(i, M, nptr, beg, end);
  const Int3* __restrict__ ush3 = reinterpret_cast<const Int3*>(ush);
  const unsigned jlim = d3_index_limit<CSR>(N, fill_value);

  // Streams the row once and stages the kept entries whose ordinal (count of kept entries in row order) lies in [k_lo, k_lo + TILE).
  // Returns the number of kept entries of the whole row.  Block-cooperative; ends with a barrier.
  auto stage = [&](float (*tile)[D3_ATM_TILE], int k_lo) -> int {
    int running = 0, par = 0;
    for (long long e0 = beg; e0 < end; e0 += ATM_WAVES * MI_WAVE, par ^= 1) {
      const D3Step s = d3_fetch<false>(idx, ush3, e0 + threadIdx.x, end, periodic);
      const bool v = s.in && ((unsigned)s.j < jlim);
      const int j = v ? s.j : i;
      const auto pj = apos[j];
      const PairGeom<T> g = d3_geom<T>(pj, pix, piy, piz, s.sh, cm, periodic);
      const bool keep = v && !(pj.w < (T)0) && g.ok && (g.r * g.r < A.rc2);
      int total;
      const int slot = atm_stage_slot(keep, cnt_sh, par, running, k_lo, lane, wave, total);
      const bool mine = keep && slot >= 0 && slot < D3_ATM_TILE;
      if (__any(mine)) {
        const int jj = mine ? j : i;
        const float4 ax = aaux[jj];  // {CN_j, r4r2_j, Z_j << 8 | species id, 0}
        const int code = __float_as_int(ax.z);
        const int cj = MODE == 0 ? (code >> 8) : (code & 0xff);
        float c6, dci, vj[5] = {0, 0, 0, 0, 0};
        if constexpr (MODE == 2) {
          const float4 w0 = aw[2 * (size_t)jj];
          vj[0] = w0.x; vj[1] = w0.y; vj[2] = w0.z; vj[3] = w0.w; vj[4] = aw[2 * (size_t)jj + 1].x;
          d3_c6_fact(hi, vj, ftab + (size_t)(si * S + cj) * D3_FROW, P.k3, c6, dci);
        } else {
          vj[0] = ax.x;
          d3_c6(cn_i, ax.x, t25base + (size_t)(si * (MODE == 1 ? S : P.nz) + cj) * 25, P.k3, c6, dci);
        }
        if (mine) {
          bool live = !(c6 < 1e-12f);  // a triple with any C6 < 1e-12 contributes nothing: sqrt(C6) = 0 zeroes every term of it
          float r0z = 0.0f;
          if constexpr (DAMP == D3_DAMP_ZERO) {
            r0z = d3_atm_radius<MODE>(si, cj, S, P.nz, ftab, t25base);
            live = live && r0z > 0.0f;  // no radius for this pair: likewise
          }
          tile[ATM_RX][slot] = g.rx; tile[ATM_RY][slot] = g.ry; tile[ATM_RZ][slot] = g.rz;
          tile[ATM_SC][slot] = live ? D3_SQRT(c6) : 0.0f;
          tile[ATM_G][slot] = live ? dci * D3_RCP(c6) : 0.0f;
          if constexpr (DAMP == D3_DAMP_ZERO) tile[ATM_R0][slot] = r0z;
          else
          tile[ATM_R0][slot] = P.a1 * D3_SQRT(3.0f * r4r2_i * ax.y) + P.a2;
          tile[ATM_H][slot] = D3_SQRT(1.73205081f * ax.y);  // h_j h_k = sqrt(3 r4r2_j r4r2_k)
          tile[ATM_CODE][slot] = __int_as_float(cj);
#pragma unroll
          for (int b = 0; b < 5; ++b) tile[ATM_TAIL + b][slot] = vj[b];
        }
      }
      running += total;
    }
    __syncthreads();
    return running;
  };

  AtmAcc acc;

  // all pairs (p in tile tp, q in tile tq); same tile: q > p
  auto pairs = [&](const float (*tp)[D3_ATM_TILE], int np, const float (*tq)[D3_ATM_TILE], int nq, bool same) {
    for (int p = wave; p < np; p += ATM_WAVES) {
      const float px = tp[ATM_RX][p], py = tp[ATM_RY][p], pz = tp[ATM_RZ][p];  // wave-uniform: LDS broadcasts
      const float scp = tp[ATM_SC][p], gp = tp[ATM_G][p], r0p = tp[ATM_R0][p], hp = tp[ATM_H][p];
      const float a = px * px + py * py + pz * pz;
      const float inva = D3_RCP(a);
      for (int q = (same ? p + 1 : 0) + lane; q < nq; q += MI_WAVE) {
        const float qx = tq[ATM_RX][q], qy = tq[ATM_RY][q], qz = tq[ATM_RZ][q];
        const float jx = qx - px, jy = qy - py, jz = qz - pz;  // r_jk
        const float c = jx * jx + jy * jy + jz * jz;
        if (!(c < A.rc2) || c < 1e-24f) continue;
        ++acc.visits;
        const float c6jk = d3_atm_c6_jk<MODE>(tp, p, tq, q, S, P.nz, ft, t25base, P.k3);
        float sjk = c6jk < 1e-12f ? 0.0f : D3_SQRT(c6jk);
        float r0;
        if constexpr (DAMP == D3_DAMP_ZERO) {
          const float r0jk = d3_atm_radius<MODE>(__float_as_int(tp[ATM_CODE][p]), __float_as_int(tq[ATM_CODE][q]), S, P.nz, ft, t25base);
          sjk = r0jk > 0.0f ? sjk : 0.0f;
          r0 = r0p * tq[ATM_R0][q] * r0jk;
        } else {
          r0 = r0p * tq[ATM_R0][q] * fmaf(P.a1, hp * tq[ATM_H][q], P.a2);
        }
        atm_triple<D3AtmMath>(px, py, pz, a, inva, scp, gp, qx, qy, qz, tq[ATM_SC][q], tq[ATM_G][q], sjk, r0, A, acc, want_virial);
      }
      if (want_virial) acc.flush_row();
    }
  };

  atm_tile_pairs(stage, pairs, tiles);
  const double r12[12] = {acc.E, acc.Fx, acc.Fy, acc.Fz, acc.dacc, acc.V6[0], acc.V6[1], acc.V6[2], acc.V6[3], acc.V6[4], acc.V6[5], (double)acc.visits};
  atm_block_reduce(r12, red, lane, wave, want_virial);
  if (threadIdx.x == 0) {
    forces[3 * (size_t)i] = (float)red[0][1]; forces[3 * (size_t)i + 1] = (float)red[0][2]; forces[3 * (size_t)i + 2] = (float)red[0][3];
    dEdCN[i] = (float)red[0][4];
    e_atom[i] = (float)(red[0][0] * (1.0 / 3.0));
    if (A.visits) A.visits[i] = (unsigned)red[0][11];
  }
  if (want_virial && threadIdx.x < 9) {
    const int r = threadIdx.x / 3, c = threadIdx.x - 3 * r;
    const int m = r == c ? r : r + c + 2;  // row-major (r, c) -> index in {xx, yy, zz, xy, xz, yz}
    // per edge dE/dr / r = 2 dE/d(r^2); a third of the triangle's -sum_edges (dE/dr / r) r (x) r per visit
    v_atom[9 * (size_t)i + threadIdx.x] = -(2.0 / 3.0) * red[0][5 + m];
  }
}

struct D3AtmLayout { D3Layout base; size_t cn, visits, total; };
D3AtmLayout d3_atm_layout(int N, int nz, int dtype, int B) {
  D3AtmLayout L;
  L.base = d3_layout(N, nz, dtype, B);
  L.cn = L.base.total;
  L.visits = L.cn + mi_align(sizeof(float) * (size_t)N);
  L.total = L.visits + mi_align(sizeof(unsigned) * (size_t)N);
  return L;
}

template <class T, bool CSR, int DAMP>
int d3_atm_impl(const T* pos, const int* numbers, int N, const int* idx, const int* ush, const int* nptr, int M, int fill_value, const T* cell,
                const int* batch_idx, int B, const mi_d3_params* hp, float s9, float alpha, float cutoff, int want_virial, float* energy,
                float* forces, float* virial, char* ws, const D3AtmLayout& LA, float rs9, const float* r0ab /* D3_DAMP_ZERO only */, hipStream_t st) {
  const D3Layout& L = LA.base;
  int* gflag = reinterpret_cast<int*>(ws + L.guard + sizeof(unsigned long long) * MI_CN_SLOTS);
  float* dEdCN = reinterpret_cast<float*>(ws + L.dEdCN);
  float* e_atom = reinterpret_cast<float*>(ws + L.e_atom);
  double* v_atom = reinterpret_cast<double*>(ws + L.v_atom);
  float4* tab = reinterpret_cast<float4*>(ws + L.tab);
  int* present = reinterpret_cast<int*>(ws + L.present);
  int* smap = reinterpret_cast<int*>(ws + L.smap);
  D3Species* sinfo = reinterpret_cast<D3Species*>(ws + L.sinfo);
  float4* ctab = reinterpret_cast<float4*>(ws + L.ctab);
  float* ftab = reinterpret_cast<float*>(ws + L.ftab);
  float* fcr = reinterpret_cast<float*>(ws + L.fcr);
  auto* apos = reinterpret_cast<typename Vec4<T>::type*>(ws + L.apos);
  auto* apos_s = reinterpret_cast<typename Vec4<T>::type*>(ws + L.apos_s);
  auto* acn = reinterpret_cast<typename Vec4<T>::type*>(ws + L.acn);
  float4* aaux = reinterpret_cast<float4*>(ws + L.aaux);
  float4* aaux_s = reinterpret_cast<float4*>(ws + L.aaux_s);
  float4* aw = reinterpret_cast<float4*>(ws + L.aw);
  float4* aw_s = reinterpret_cast<float4*>(ws + L.aw_s);
  float* dEdCN_s = reinterpret_cast<float*>(ws + L.dEdCN_s);
  float* cn = reinterpret_cast<float*>(ws + LA.cn);
  D3Dev P;
  P.rcov = hp->rcov; P.r4r2 = hp->r4r2; P.tab = tab; P.nz = hp->nz;
  P.a1 = hp->a1; P.a2 = hp->a2; P.s6 = hp->s6; P.s8 = hp->s8; P.k1 = hp->k1; P.k3 = hp->k3; P.s5_on = hp->s5_on; P.s5_off = hp->s5_off;
  P.inv_w = 0.0f;
  // D3_DAMP_ZERO: every table carries rs9 r0ab of its species pair in the "beta R0" place (see the head of this file)
  const D3ZeroSpec zero = DAMP == D3_DAMP_ZERO ? D3ZeroSpec{r0ab, 1.0f, 1.0f, rs9} : D3ZeroSpec{nullptr, 0.0f, 0.0f, 0.0f};
  P.crec = nullptr;  // the chain pass then runs its plain-array form on the three-body dE/dCN
  P.crc = reinterpret_cast<const float*>(ws + L.crc);
  P.cflag = gflag + 4;
  MI_HIP_CHECK(hipMemsetAsync(ws + L.guard, 0, ((L.present - L.guard) + sizeof(int) * ((size_t)hp->nz + 2) + 15) / 16 * 16, st));
  MI_HIP_CHECK(hipMemsetAsync(ws + LA.visits, 0, sizeof(unsigned) * (size_t)N, st));
  d3_mark_species_kernel<<<mi_blocks(N, 256), 256, 0, st>>>(numbers, N, hp->nz, present);
  MI_LAUNCH_CHECK();
  d3_compact_species_kernel<<<1, 256, 0, st>>>(present, hp->c6ab, hp->cn_ref, hp->nz, smap, sinfo, ctab, ftab, fcr, hp->k3, hp->r4r2, hp->a1, hp->a2, hp->rcov,
                                               reinterpret_cast<float*>(ws + L.crc), zero);
  MI_LAUNCH_CHECK();
  const long long nt = (long long)hp->nz * hp->nz * 25;
  D3Guard G{};
  G.atom_blocks = mi_blocks(N, 256);
  const D3Tables TB{hp->c6ab, hp->cn_ref, hp->nz, sinfo, tab, G.atom_blocks, zero};
  d3_pack_atoms_kernel<T><<<G.atom_blocks + mi_blocks(nt, 256), 256, 0, st>>>(pos, numbers, N, hp->rcov, hp->r4r2, smap, hp->nz, apos, aaux, forces, cn, dEdCN, e_atom,
                                                                            want_virial ? v_atom : nullptr, nullptr, apos_s, aaux_s, acn, G, TB, nullptr);
  MI_LAUNCH_CHECK();
  // 1. coordination numbers over the WHOLE list (the two-body pass's kernel); plain weight records {v_0..v_3 | v_4, ...} for both dtypes
  const D3Weights W{sinfo, fcr, hp->k3, nullptr, aw, aw_s};
  MI_TIMED("d3_atm_cn", st, (d3_cn_kernel<T, CSR, false, false, false><<<mi_blocks(N, D3_LS_WAVES), D3_LS_WAVES * MI_WAVE, 0, st>>>(
                                pos, numbers, N, idx, ush, nptr, M, fill_value, cell, batch_idx, P, apos, aaux, cn, nullptr, nullptr, nullptr, acn, aaux_s, nullptr,
                                nullptr, W, nullptr, 0)));
  MI_LAUNCH_CHECK();
  // 2. triples
  const AtmParams A{s9, alpha, cutoff * cutoff, reinterpret_cast<unsigned*>(ws + LA.visits)};
  auto launch = [&](auto mode) {
    constexpr int MODE_ = decltype(mode)::value;
    d3_atm_kernel<T, CSR, MODE_, DAMP><<<N, ATM_WAVES * MI_WAVE, 0, st>>>(pos, numbers, N, idx, ush, nptr, M, fill_value, cell, batch_idx, P, A, cn, want_virial, smap,
                                                                    sinfo, ctab, ftab, fcr, apos, aaux, aw, dEdCN, forces, e_atom, v_atom);
  };
  MI_TIMED("d3_atm_triples", st, (launch(std::integral_constant<int, 2>{}), launch(std::integral_constant<int, 1>{}), launch(std::integral_constant<int, 0>{})));
  MI_LAUNCH_CHECK();
  // 3. chain rule through the coordination numbers, over the whole list
  MI_TIMED("d3_atm_chain", st, (d3_chain_kernel<T, CSR, false><<<mi_blocks(N, D3_CH_LS_WAVES), D3_CH_LS_WAVES * MI_WAVE, 0, st>>>(
                                   pos, numbers, N, idx, ush, nptr, M, fill_value, cell, batch_idx, P, apos, dEdCN, want_virial, forces, v_atom, nullptr, nullptr,
                                   nullptr, apos_s, dEdCN_s, sinfo)));
  MI_LAUNCH_CHECK();
  // 4. per-system sums
  double* sums = reinterpret_cast<double*>(ws + L.sums);
  d3_reduce_kernel<<<D3_REDUCE_WAVES / 4, 256, 0, st>>>(e_atom, v_atom, batch_idx, N, want_virial, sums);
  MI_LAUNCH_CHECK();
  d3_finish_kernel<<<mi_blocks(10ll * B, 256), 256, 0, st>>>(sums, B, want_virial, energy, virial);
  MI_LAUNCH_CHECK();
  return MI_OK;
}
