// fin_stash.h -- the weights-only stash of the gradient / Adam tail (internal): its layout and the role that fills it.
// The role runs in whichever launch precedes the tail: k_tail_ts / k_reduce_partials (model.hip) or, in front of the
// one-launch tail k_tail_fin, four workgroups appended to k_graph_step2 (g2_subgraph.h).
#pragma once
#include "model.h"
// what fin_stash_body reads of a model
struct FinStashModel {
  int R, L;
  int64_t off_basis[4], off_att[4];
  float* fin_stash;
  const float* adam_m1;
  const float* adam_m2;
  float* arr_part;
};

// Weights-only quantities of conv layer l for k_finalize_ts, formed while the tables are being reduced: Gram matrix of
// the bases, ARR matrix M[b][b'] = sum_r att[r,b] c[r,b'], the ARR value, a copy of att (k_finalize_ts updates att in
// place while other workgroups still need the old values) and, from the control block, the Adam scalars of the step.
#define IGMC_STASH_G 0
#define IGMC_STASH_M 16
#define IGMC_STASH_ATTM1 32       // Adam moments of att before the step (R <= 16; k_finalize_ts with img: every workgroup of
#define IGMC_STASH_ATTM2 96       // the layer forms the new att, while the owner updates the moments in place)
#define IGMC_STASH_ATT 160        // copy of att: R <= 128
// (IGMC_STASH_LAYER floats per layer: model.h)
#define IGMC_STASH_SCAL (4 * IGMC_STASH_LAYER)
#define IGMC_STASH_SEQ 8           // ... [SCAL + 8]: launch sequence number of the subgraph kernel (bits), for the one-launch tail
// (M: ModelDev, or the few fields of it the role reads -- FinStashModel, which rides in k_graph_step2's compact arguments)
template <typename M>
__device__ __forceinline__ void fin_stash_body(const M& m, const float* __restrict__ P, int l, const int64_t* ctrl) {
  __shared__ float sg10[4][10];
  __shared__ float sG[16];
  __shared__ float s_att[128];                       // att[r][b] of the layer (R <= 32: else read from HBM where needed)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nE = ((l == 0) ? m.L : 32) * 32, R = m.R, na = R * 4;
  const float* basis = P + m.off_basis[l];
  const float* attg = P + m.off_att[l];
  float* st = m.fin_stash + l * IGMC_STASH_LAYER;
  // Every load of the role is requested HERE, before the first use: att, the thread's (<= 4) elements of the four bases, att's
  // Adam moments, the step's scalars.  Left inside the loops below they were a dozen dependent round trips -- the longest
  // chain of the whole k_tail_ts launch.
  const bool small = na <= 128;
  const float attv = (small && tid < na) ? attg[tid] : 0.f;
  float bq[4][4];
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int e = tid + it * IGMC_BLOCK, ec = e < nE ? e : nE - 1;
#pragma unroll
    for (int q = 0; q < 4; ++q) bq[it][q] = (e < nE) ? basis[q * nE + ec] : 0.f;
  }
  float m1v = 0.f, m2v = 0.f;
  const bool mom = m.adam_m1 && na <= 64 && tid >= 128 && tid < 128 + na;
  if (mom) {
    m1v = m.adam_m1[m.off_att[l] + tid - 128];
    m2v = m.adam_m2[m.off_att[l] + tid - 128];
  }
  double scal = 0.0;
  const bool sc = l == 0 && ctrl && tid >= 192 && tid < 198;
  if (sc) {
    const double* d = (const double*)ctrl;
    const int k = tid - 192;
    const int src = (k == 0) ? IGMC_CTRL_STEP_SIZE : (k == 1) ? IGMC_CTRL_INV_SQRT_BC2 : (k == 2) ? IGMC_CTRL_BETA1
                  : (k == 3) ? IGMC_CTRL_BETA2 : (k == 4) ? IGMC_CTRL_EPS : IGMC_CTRL_WD;
    scal = d[src];
  }
  if (small && tid < na) s_att[tid] = attv;
  float gp[10];
#pragma unroll
  for (int q = 0; q < 10; ++q) gp[q] = 0.f;
#pragma unroll
  for (int it = 0; it < 4; ++it) {                     // (element order per thread as before: e = tid, tid + 256, ..)
    if (tid + it * IGMC_BLOCK < nE) {
      const float b0 = bq[it][0], b1 = bq[it][1], b2 = bq[it][2], b3 = bq[it][3];
      gp[0] += b0 * b0; gp[1] += b0 * b1; gp[2] += b0 * b2; gp[3] += b0 * b3;
      gp[4] += b1 * b1; gp[5] += b1 * b2; gp[6] += b1 * b3;
      gp[7] += b2 * b2; gp[8] += b2 * b3; gp[9] += b3 * b3;
    }
  }
  for (int e = tid + 4 * IGMC_BLOCK; e < nE; e += IGMC_BLOCK) {      // (nE <= 1024: never)
    const float b0 = basis[e], b1 = basis[nE + e], b2 = basis[2 * nE + e], b3 = basis[3 * nE + e];
    gp[0] += b0 * b0; gp[1] += b0 * b1; gp[2] += b0 * b2; gp[3] += b0 * b3;
    gp[4] += b1 * b1; gp[5] += b1 * b2; gp[6] += b1 * b3;
    gp[7] += b2 * b2; gp[8] += b2 * b3; gp[9] += b3 * b3;
  }
#pragma unroll
  for (int q = 0; q < 10; ++q) gp[q] = igmc_wave_sum_f(gp[q]);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 10; ++q) sg10[wave][q] = gp[q];
  }
  __syncthreads();                                   // s_att, sg10
  const float* att = small ? (const float*)s_att : attg;
  if (tid >= 64 && tid < 80) {           // M[b][b'] = sum_r att[r,b] c[r,b'],  c[r] = 2 (d[r-1] - d[r]),  d[r] = att[r+1]-att[r]
    const int bb = (tid - 64) >> 2, bp = tid & 3;
    float sacc = 0.f;
    for (int r = 0; r < R; ++r) {
      const float dm = (r > 0) ? att[r * 4 + bp] - att[(r - 1) * 4 + bp] : 0.f;
      const float dn = (r + 1 < R) ? att[(r + 1) * 4 + bp] - att[r * 4 + bp] : 0.f;
      sacc += att[r * 4 + bb] * 2.f * (dm - dn);
    }
    st[IGMC_STASH_M + tid - 64] = sacc;
  }
  if (tid >= 128 && na <= IGMC_STASH_LAYER - IGMC_STASH_ATT) {
    for (int i = tid - 128; i < na; i += IGMC_BLOCK - 128) {
      st[IGMC_STASH_ATT + i] = att[i];
      if (m.adam_m1 && na <= 64) {
        st[IGMC_STASH_ATTM1 + i] = mom && i == tid - 128 ? m1v : m.adam_m1[m.off_att[l] + i];
        st[IGMC_STASH_ATTM2 + i] = mom && i == tid - 128 ? m2v : m.adam_m2[m.off_att[l] + i];
      }
    }
  }
  if (sc) m.fin_stash[IGMC_STASH_SCAL + tid - 192] = (float)scal;
  if (tid == 0) {
    const int ij[10][2] = {{0, 0}, {0, 1}, {0, 2}, {0, 3}, {1, 1}, {1, 2}, {1, 3}, {2, 2}, {2, 3}, {3, 3}};
    for (int q = 0; q < 10; ++q) {
      const float v = (sg10[0][q] + sg10[1][q]) + (sg10[2][q] + sg10[3][q]);
      sG[ij[q][0] * 4 + ij[q][1]] = v;
      sG[ij[q][1] * 4 + ij[q][0]] = v;
    }
    float reg = 0.f;                       // reg = sum_r d[r]^T Gm d[r]   (reference train_eval.py:167-174)
    for (int r = 0; r + 1 < R; ++r) {
      float d[4];
      for (int q = 0; q < 4; ++q) d[q] = att[(r + 1) * 4 + q] - att[r * 4 + q];
      for (int p1 = 0; p1 < 4; ++p1)
        for (int p2 = 0; p2 < 4; ++p2) reg += d[p1] * sG[p1 * 4 + p2] * d[p2];
    }
    m.arr_part[l] = reg;
    for (int q = 0; q < 16; ++q) st[IGMC_STASH_G + q] = sG[q];
  }
}
