// atm_core.h -- the triple pass that the three-body (Axilrod-Teller-Muto) kernels of DFT-D3 (d3_atm.h) and DFT-D4 (d4_atm.h) share.  Included
// by both inside the anonymous namespace of their translation unit; __device__ __forceinline__ pieces only, nothing here launches a kernel.
//
// For every unordered triple of distinct atom images A, B, C with all three distances below `cutoff`:
//   C9 = sqrt(C6_AB C6_AC C6_BC),  a, b, c = r_AB^2, r_AC^2, r_BC^2,  P = r_AB r_AC r_BC,  R0 = R0_AB R0_AC R0_BC
//   ang = 0.375 (a + b - c)(a + c - b)(b + c - a) / P^5 + 1 / P^3,   fdamp = 1 / (1 + 6 (R0 / P)^(alpha / 3)),   E_ABC = s9 C9 ang fdamp
// Owner-computes, no atomics: ONE BLOCK OF FOUR WAVES PER CENTRE ATOM i.  Seen from i the vector between two of its neighbours is
// r_ik - r_ij with the unit shifts already applied, so a triangle needs no look-up of the j-k pair in anybody's row.  The block streams
// row i, keeps the entries inside the cutoff and stages one record per kept entry in LDS, structure of arrays: the common prefix below
// (displacement, sqrt(C6_ij), dC6_ij/dCN_i / C6_ij, R0_ij, sqrt(sqrt(3) r4r2_j), species code) and a tail that is the kernel's own (what it
// needs to form C6_jk).  A kept entry's slot is its ordinal -- the count of kept entries before it in row order -- so the assignment is
// reproducible (atm_stage_slot).  Waves then take rows p of the triangle (p, q > p) of staged records: record p is wave-uniform (LDS
// broadcast), lanes take consecutive q -- no integer division, conflict-free LDS reads.  Every triangle is visited from each of its three
// vertices; a visit (atm_triple) adds ONE THIRD of the energy and of the explicit virial, the FULL explicit force on the centre and the
// FULL dE/dC6_ij dC6_ij/dCN_i + dE/dC6_ik dC6_ik/dCN_i = 1/2 E (g_ij + g_ik) to the centre's dE/dCN -- complete without a write to j or
// k.  fp32 per-triple arithmetic, fp64 lane accumulators (AtmAcc; the virial in fp32 per row of the triangle, flushed to fp64), one block
// reduction (atm_block_reduce).  Rows with more kept entries than a tile holds go tile pair by tile pair (atm_tile_pairs; the row is
// streamed again per staged tile).  A kernel supplies C6_jk, the radius product R0 and its own store epilogue.
// (d4_atm.h uses the slot, the tile-pair loop and the reduction, and keeps its own text of AtmAcc / atm_triple: see its head.)
#pragma once

#define ATM_WAVES 4

enum { ATM_RX = 0, ATM_RY, ATM_RZ, ATM_SC, ATM_G, ATM_R0, ATM_H, ATM_CODE, ATM_TAIL };  // the record prefix; the kernel's tail starts at ATM_TAIL

struct AtmParams { float s9, alpha, rc2; unsigned* visits; };

// The tile slot of this thread's row entry in a tile that starts at ordinal k_lo (anything outside [0, TILE) is not staged), for one trip
// of ATM_WAVES * MI_WAVE entries after `running` kept ones; `total` = kept entries of the trip.  cnt_sh is double-buffered by the trip's
// parity `par`: one barrier per trip.
__device__ __forceinline__ int atm_stage_slot(bool keep, int (*cnt_sh)[ATM_WAVES], int par, int running, int k_lo, int lane, int wave, int& total) {
  const unsigned long long m = __ballot(keep);
  if (lane == 0) cnt_sh[par][wave] = (int)__popcll(m);
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < ATM_WAVES; ++w) { const int c = cnt_sh[par][w]; before += w < wave ? c : 0; total += c; }
  return running + before + (int)__popcll(m & lanemask_lt()) - k_lo;
}

struct AtmAcc {
  double E = 0, Fx = 0, Fy = 0, Fz = 0, dacc = 0;
  float V[6] = {0, 0, 0, 0, 0, 0};  // xx yy zz xy xz yz: fp32 lane partials, flushed into V6 once per row of the triangle
  double V6[6] = {0, 0, 0, 0, 0, 0};
  unsigned visits = 0;
  __device__ __forceinline__ void flush_row() {
#pragma unroll
    for (int k = 0; k < 6; ++k) { V6[k] += (double)V[k]; V[k] = 0.0f; }
  }
};

// One visit of the triangle (i; p, q) that passed the cutoff test on r_jk.  p: the wave-uniform record (a = |r_ip|^2, inva = 1 / a); q: the
// lane's record; sjk = sqrt(C6_jk), or 0 to take the triple out; r0 = R0_ip R0_iq R0_pq.  Math::rcp is the kernel's reciprocal (the D3 test
// library swaps in the IEEE divide); rsq, log2 and exp2 are the hardware's in every build.  `vir` folds after inlining.
template <class Math>
__device__ __forceinline__ void atm_triple(float px, float py, float pz, float a, float inva, float scp, float gp, float qx, float qy, float qz,
                                           float scq, float gq, float sjk, float r0, const AtmParams& A, AtmAcc& acc, bool vir) {
  const float jx = qx - px, jy = qy - py, jz = qz - pz;  // r_jk
  const float c = jx * jx + jy * jy + jz * jz;
  const float b = qx * qx + qy * qy + qz * qz;
  // a + b - c = 2 r_ij.r_ik etc.: the three factors as dot products, not as differences of squared lengths
  const float x = 2.0f * (px * qx + py * qy + pz * qz), y = -2.0f * (px * jx + py * jy + pz * jz), z = 2.0f * (qx * jx + qy * jy + qz * jz);
  const float pinv = __builtin_amdgcn_rsqf(a * b * c);
  const float pinv3 = pinv * pinv * pinv, k5 = 0.375f * pinv3 * pinv * pinv;
  const float yz = y * z, xz = x * z, xy = x * y, nn = xy * z;
  const float ang = fmaf(k5, nn, pinv3);
  // (R0 / P)^(alpha / 3) with a runtime exponent: one log2 / exp2 pair per triple
  const float t = __builtin_amdgcn_exp2f(A.alpha * (1.0f / 3.0f) * __builtin_amdgcn_logf(r0 * pinv));
  const float fd = Math::rcp(fmaf(6.0f, t, 1.0f));
  const float c9 = A.s9 * scp * scq * sjk;
  const float e = c9 * ang * fd;
  // dE/da = C9 fd (k5 dN/da + B0 / a),  B0 = ang fd t alpha - (2.5 k5 N + 1.5 / P^3); likewise b, c
  const float b0 = ang * fd * t * A.alpha - fmaf(2.5f * k5, nn, 1.5f * pinv3);
  const float cf = c9 * fd;
  const float dEda = cf * fmaf(k5, yz + xz - xy, b0 * inva);
  const float dEdb = cf * fmaf(k5, yz - xz + xy, b0 * Math::rcp(b));
  acc.E += (double)e;
  acc.dacc += (double)(0.5f * e * (gp + gq));
  const float fx = 2.0f * (dEda * px + dEdb * qx), fy = 2.0f * (dEda * py + dEdb * qy), fz = 2.0f * (dEda * pz + dEdb * qz);
  acc.Fx += (double)fx; acc.Fy += (double)fy; acc.Fz += (double)fz;
  if (vir) {
    const float dEdc = cf * fmaf(k5, xz + xy - yz, b0 * Math::rcp(c));
    const float ax = dEda * px, ay = dEda * py, az = dEda * pz, bx = dEdb * qx, by = dEdb * qy, bz = dEdb * qz;
    const float cx = dEdc * jx, cy = dEdc * jy, cz = dEdc * jz;
    acc.V[0] += ax * px + bx * qx + cx * jx; acc.V[1] += ay * py + by * qy + cy * jy; acc.V[2] += az * pz + bz * qz + cz * jz;
    acc.V[3] += ax * py + bx * qy + cx * jy; acc.V[4] += ax * pz + bx * qz + cx * jz; acc.V[5] += ay * pz + by * qz + cy * jz;
  }
}

// Tile pairs (tp, tq >= tp) of a row: the p tile in tiles[0], a later q tile in tiles[1] (selected by index: two
// tile pointers held through the loops cost scalar registers).  stage(tile, k_lo) -> kept entries of the whole row
// (the same number every time: 0 ends both loops); pairs(tp, np, tq, nq, same) runs all pairs (p in tp, q in tq; same tile: q > p).
template <int REC, int TILE, class Stage, class Pairs>
__device__ __forceinline__ void atm_tile_pairs(Stage stage, Pairs pairs, float (*tiles)[REC][TILE]) {
  for (int tp = 0, ntiles = 1; tp < ntiles; ++tp) {
    for (int tq = tp; tq < ntiles; ++tq) {
      const int w = tq == tp ? 0 : 1;
      __syncthreads();  // the waves are done with the tile that is staged over
      const int n = stage(tiles[w], tq * TILE);
      ntiles = (n + TILE - 1) / TILE;
      pairs(tiles[0], min(TILE, n - tp * TILE), tiles[w], min(TILE, n - tq * TILE), w == 0);
    }
  }
}

// The block's twelve sums into red[0][0..11]: E, Fx, Fy, Fz, dE/dCN share, the six virial words (AtmAcc's order; only with `vir`), visits.
__device__ __forceinline__ void atm_block_reduce(const double (&r12)[12], double (*red)[12], int lane, int wave, bool vir) {
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    if (k >= 5 && k < 11 && !vir) continue;
    const double s = wave_sum(r12[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < 12 && (vir || threadIdx.x < 5 || threadIdx.x == 11)) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < ATM_WAVES; ++w) s += red[w][threadIdx.x];
    red[0][threadIdx.x] = s;
  }
  __syncthreads();
}
