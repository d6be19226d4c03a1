// model.hip -- IGMC forward / backward / optimiser kernels for gfx950 (CDNA4).
//
// Math (reference models.py:190-217, PyG-1.4.2 RGCNConv):
//   conv_l(x)[i] = sum_{(j->i, r)} x[j] W_l[r] + x[i] root_l + bias_l,  W_l[r] = sum_b att_l[r,b] basis_l[b]
//   h_l = tanh(conv_l(h_{l-1}));  readout = [h_0..h_3](target user) | [h_0..h_3](target item)
//   out = lin2(dropout(relu(lin1(readout)))) * multiply_by
//
// MI355X formulation (NOT the reference's per-edge [E,32,32] weight materialisation):
//   * aggregate in BASIS space:  A[i][b] = sum_e att[rel_e, b] * x[src_e]   (4 accumulators per
//     feature, independent of the number of relations R), then ONE dense transform
//     [A | x] (N x 160) @ [basis ; root] (160 x 32) on f32 MFMA (16x16x4), + bias, tanh fused.
//   * the gather walks a dst-sorted CSR (atomic-free, bit-reproducible): one wave per row.
//   * layer 0 has one-hot inputs: it degenerates to a table lookup W0[rel*L + label] per edge.
//   * backward reuses the same gather on the symmetric CSR (keep-bit 1 = transposed edge):
//       G[j][b]   = sum_{e: src=j} att[rel_e,b] dPre[dst_e]
//       dX        = [G | dPre] @ [basis^T ; root^T]
//       d basis_b = X^T G_b,  d root = X^T dPre,  d bias = sum dPre      (MFMA, per-block partials)
//       d att[r,b]= sum_j < (x_j basis_b), sum_{e: src=j, rel=r} dPre[dst_e] >   (rows are sorted
//                   by relation, so this is one dot product per relation RUN, not per edge)
//   * every serialized kernel costs >= 4.7 us on this part even when trivial (rocprofv3), so the step is
//     organised for FEW launches: derived weight layouts are produced while staging into LDS (no prep
//     kernel), the three Y products and the three weight-gradient products are batched into one launch
//     each (blockIdx.y = layer), and loss / epoch-total / control-block tick ride in the Adam kernel.
#include "launch.h"      // StepHead, AdamHyper, AdamTail; the launch sequences are at the end of the file
#include "g2_image.h"
#include "fin_stash.h"      // layout of the weights-only stash (IGMC_STASH_*) and the role that fills it
#include "g2_words.h"       // {f32, tag} words (the one-launch tail's hand-off)
#include <stdlib.h>
#include <string.h>

// ---- XCD affinity -------------------------------------------------------------------------------------
// MI355X has 8 XCDs with private, mutually non-coherent 4 MiB L2s, and workgroup b of a launch runs on XCD
// b % 8 (observed placement; used for SPEED only, never for correctness).  Subgraphs are independent: a row of
// graph g only ever reads rows of graph g.  So the graphs of a batch are split into 8 contiguous segments and
// every row-walking kernel lets XCD x work on segment x: what layer l wrote stays in the L2 that layer l+1
// reads it from, instead of being re-fetched from the other XCDs / Infinity Cache by all eight L2s
// (rocprofv3: TCC hit rate 50 % and FETCH_SIZE = 8 x the feature matrix without this).
struct XcdSeg {
  int lo, hi;      // row range [lo, hi) of this workgroup's XCD segment
  int j, nj;       // index of the workgroup within its XCD, workgroups per XCD
};
__device__ __forceinline__ XcdSeg igmc_xcd_segment(const BatchDev& b) {
  XcdSeg s;
  const int B = b.totals[3];
  const int x = blockIdx.x & 7;
  s.j = blockIdx.x >> 3;
  s.nj = (gridDim.x + 7 - x) >> 3;          // workgroups with this residue
  s.lo = b.node_off[(x * B) >> 3];
  s.hi = b.node_off[((x + 1) * B) >> 3];
  return s;
}

// =================================================================== row walkers
// One WAVE per destination row.  The row's CSR entries are consumed in chunks of 16: 16-lane group
// `grp` of the wave owns chunks grp, grp+4, ...; lane t of the group loads entry c0+t (one coalesced
// 64-byte index load per chunk) and the group then broadcasts entry k with a width-16 shuffle, so
// 4 x 4 feature-row loads (128 B each, float2 per lane) are in flight per wave instruction.  The four
// partial sums are combined with two xor-shuffles at the end of the row.

// =================================================================== layer 0 forward (one-hot input)
// h0[i] = tanh( sum_e W0[rel_e*L + label(src_e)] + root0[label_i] + bias0 ),  W0[r][c] = sum_b att0[r,b] basis0[b][c]
// STORE (training): also emits cnt0[i][code] = number of kept incoming edges with that code, so that the
// layer-0 weight gradient is a dense [codes x N] @ [N x 32] product that never touches the edges again.
template <bool FLAGS, bool STORE>
__global__ __launch_bounds__(IGMC_BLOCK) void k_l0_fwd(BatchDev b, ModelDev m, const float* __restrict__ P,
                                                         float* __restrict__ out) {
  igmc_kernarg_warm<sizeof(BatchDev) + sizeof(ModelDev) + 32>();
  IGMC_DYN_SMEM(smem);
  const int RL = m.R * m.L, LF = m.L * 32;
  float* sW0 = (float*)smem;                 // [R*L][32]
  float* sroot = sW0 + RL * 32;              // [L][32]
  float* sbias = sroot + LF;                 // [32]
  int* shist = (int*)(sbias + 32);           // [4 waves][R*L]   (STORE only)
  for (int i = threadIdx.x; i < RL * 32; i += IGMC_BLOCK) {
    const int r = i / LF, cf = i % LF;
    float s = 0.f;
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) s += P[m.off_att[0] + r * 4 + bb] * P[m.off_basis[0] + bb * LF + cf];
    sW0[i] = s;
  }
  for (int i = threadIdx.x; i < LF; i += IGMC_BLOCK) sroot[i] = P[m.off_root[0] + i];
  if (threadIdx.x < 32) sbias[threadIdx.x] = P[m.off_bias[0] + threadIdx.x];
  __syncthreads();
  const int N = b.totals[0];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = lane >> 4, t = lane & 15;
  int* hist = shist + wave * RL;
  const XcdSeg seg = igmc_xcd_segment(b);
  (void)N;
  for (int i = seg.lo + seg.j * 4 + wave; i < seg.hi; i += seg.nj * 4) {
    float ax = 0.f, ay = 0.f;
    if (STORE) {
      for (int c = lane; c < RL; c += 64) hist[c] = 0;
      IGMC_WAVE_SYNC();
    }
    const int beg = b.row_ptr[i], end = b.row_ptr[i + 1];
    for (int c0 = beg + grp * 16; c0 < end; c0 += 64) {
      const int e = c0 + t;
      int w = -1;                              // code, or -1 = skip
      if (e < end && (!FLAGS || (b.eflag[e] & 1))) w = b.ecode[e];
      if (STORE && w >= 0) atomicAdd(&hist[w], 1);
      const int n = (end - c0 < 16) ? end - c0 : 16;
      for (int k = 0; k < n; ++k) {
        const int code = __shfl(w, k, 16);
        if (code >= 0) {
          ax += sW0[code * 32 + 2 * t];
          ay += sW0[code * 32 + 2 * t + 1];
        }
      }
    }
    ax += __shfl_xor(ax, 16, 64);
    ay += __shfl_xor(ay, 16, 64);
    ax += __shfl_xor(ax, 32, 64);
    ay += __shfl_xor(ay, 32, 64);
    if (grp == 0) {
      const int lab = b.node_label[i];
      float2 o;
      o.x = tanhf(ax + sbias[2 * t] + sroot[lab * 32 + 2 * t]);
      o.y = tanhf(ay + sbias[2 * t + 1] + sroot[lab * 32 + 2 * t + 1]);
      *(float2*)(out + (size_t)i * 32 + 2 * t) = o;
    }
    if (STORE) {
      IGMC_WAVE_SYNC();
      for (int c = lane; c < RL; c += 64) m.cnt0[(size_t)i * RL + c] = (uint16_t)hist[c];
      IGMC_WAVE_SYNC();
    }
  }
}

// Basis-space aggregate of ONE row (see "row walkers" above) by NG 16-lane groups: NG = 4 -> the whole wave
// works on row i and lanes of group 0 hold the result; NG = 1 -> every group walks its OWN row i (i differs
// between the groups of a wave) and holds its own result.  ax[bb], ay[bb] = features 2t, 2t+1 of A[i][bb].
template <bool FLAGS, bool TRANS, bool ATTG, int NG = 4>
__device__ __forceinline__ void gather_row(const BatchDev& b, const float* __restrict__ in, const float* s_att,
                                           float* my_gatt, const float* __restrict__ Y, int i, int beg, int end,
                                           int lane, float (&ax)[4], float (&ay)[4]) {
  const int grp = lane >> 4, t = lane & 15;
  const int kbit = TRANS ? 1 : 0;
  (void)grp;
#pragma unroll
  for (int bb = 0; bb < 4; ++bb) { ax[bb] = 0.f; ay[bb] = 0.f; }
  {
    float yx[4], yy[4];
    float tx = 0.f, ty = 0.f;
    int cur = -1;
    if (ATTG) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float2 v = *(const float2*)(Y + (size_t)i * 128 + q * 32 + 2 * t);
        yx[q] = v.x;
        yy[q] = v.y;
      }
    }
    int c0 = beg + (NG == 4 ? grp * 16 : 0);
    uint32_t w_next = 0u;
    int kp_next = 0;
    {
      const int e = c0 + t;
      if (e < end) {
        w_next = b.ecr[e];
        kp_next = FLAGS ? (b.eflag[e] >> kbit) & 1 : 1;
      }
    }
    for (; c0 < end; c0 += 16 * NG) {
      const uint32_t w = w_next;
      const int kp = kp_next;
      {   // prefetch the NEXT chunk's entries: the load overlaps with this chunk's feature-row loads
        const int e1 = c0 + 16 * NG + t;
        w_next = 0u;
        kp_next = 0;
        if (e1 < end) {
          w_next = b.ecr[e1];
          kp_next = FLAGS ? (b.eflag[e1] >> kbit) & 1 : 1;
        }
      }
      // broadcast the 16 entries of the chunk and issue ALL their feature-row loads before any use:
      // one memory round trip per chunk instead of four
      uint32_t wk[16];
      float2 x[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        wk[q] = __shfl(w, q, 16);
        const int kk = __shfl(kp, q, 16);          // 0 for dropped edges and for lanes past the row end
        wk[q] = kk ? wk[q] : 0xFFFFFFFFu;
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        if (wk[q] != 0xFFFFFFFFu) x[q] = *(const float2*)(in + (size_t)(wk[q] & 0xFFFFFFu) * 32 + 2 * t);
        else { x[q].x = 0.f; x[q].y = 0.f; }
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        if (wk[q] == 0xFFFFFFFFu) continue;
        const int r = (int)(wk[q] >> 24);
        if (!ATTG) {
          const float* a = s_att + r * 4;
#pragma unroll
          for (int bb = 0; bb < 4; ++bb) {
            ax[bb] += a[bb] * x[q].x;
            ay[bb] += a[bb] * x[q].y;
          }
        } else {
          if (r != cur) {
            if (cur >= 0) {   // flush the finished relation run
              const float* a = s_att + cur * 4;
#pragma unroll
              for (int bb = 0; bb < 4; ++bb) {
                ax[bb] += a[bb] * tx;
                ay[bb] += a[bb] * ty;
                const float p = igmc_group16_sum_f(yx[bb] * tx + yy[bb] * ty);
                if (t == 0) my_gatt[cur * 4 + bb] += p;
              }
            }
            cur = r;
            tx = 0.f;
            ty = 0.f;
          }
          tx += x[q].x;
          ty += x[q].y;
        }
      }
    }
    if (ATTG && cur >= 0) {
      const float* a = s_att + cur * 4;
#pragma unroll
      for (int bb = 0; bb < 4; ++bb) {
        ax[bb] += a[bb] * tx;
        ay[bb] += a[bb] * ty;
        const float p = igmc_group16_sum_f(yx[bb] * tx + yy[bb] * ty);
        if (t == 0) my_gatt[cur * 4 + bb] += p;
      }
    }
    if (NG == 4) {
#pragma unroll
      for (int bb = 0; bb < 4; ++bb) {
        ax[bb] += __shfl_xor(ax[bb], 16, 64);
        ay[bb] += __shfl_xor(ay[bb], 16, 64);
        ax[bb] += __shfl_xor(ax[bb], 32, 64);
        ay[bb] += __shfl_xor(ay[bb], 32, 64);
      }
    }
  }
}

// =================================================================== dense row transform on f32 MFMA
// OUT[N,NO] = epilogue([A1[N,K1] | A2[N,K2]] @ W[K1+K2, NO]).  One wave = 16 rows x NO columns,
// v_mfma_f32_16x16x4_f32; W is staged once per block in LDS (pitch NO+4: conflict-free b32 reads).
// WMODE selects how W is derived from the layer's parameters WHILE staging (no prep kernel):
//   W_PLAIN : [basis ; root] as stored (contiguous in the flat buffer)           -> forward
//   W_BWD_T : [basis_b^T ; root^T]   sW[b*32+fo][f] = basis[b][f][fo]            -> dLoss/dx
//   W_YCAT  : [basis_0|..|basis_3]   sW[f][b*32+fo] = basis[b][f][fo]            -> Y (att gradient)
enum { EPI_NONE = 0, EPI_BIAS_TANH = 1, EPI_BWD = 2 };
enum { W_PLAIN = 0, W_BWD_T = 1, W_YCAT = 2 };

template <int K1, int K2, int NO, int EPI, int WMODE, int NTH = IGMC_BLOCK>
__device__ __forceinline__ void dense_body(const BatchDev& b, const float* __restrict__ A1,
                                           const float* __restrict__ A2, const float* __restrict__ basis,
                                           const float* __restrict__ root, const float* __restrict__ bias,
                                           float* __restrict__ out, const float* __restrict__ xin,
                                           const float* __restrict__ gfeat, int D, int rlayer,
                                           float* __restrict__ zero_out, float* sW) {
  constexpr int K = K1 + K2, PITCH = NO + 4, NT = NO / 16;
  if (WMODE == W_PLAIN) {
    for (int idx = threadIdx.x; idx < K * NO; idx += NTH) sW[(idx / NO) * PITCH + (idx % NO)] = basis[idx];
  } else {
    for (int idx = threadIdx.x; idx < 4096; idx += NTH) {     // coalesced read of basis[b][f][fo]
      const int bb = idx >> 10, f = (idx >> 5) & 31, fo = idx & 31;
      if (WMODE == W_BWD_T) sW[(bb * 32 + fo) * PITCH + f] = basis[idx];
      else sW[f * PITCH + bb * 32 + fo] = basis[idx];
    }
    if (WMODE == W_BWD_T)
      for (int idx = threadIdx.x; idx < 1024; idx += NTH) sW[(128 + (idx & 31)) * PITCH + (idx >> 5)] = root[idx];
  }
  __syncthreads();
  const int N = b.totals[0];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, kq = lane >> 4;
  constexpr int ROWS = NTH / 4;      // 16 rows per wave
  for (int tile = blockIdx.x; tile * ROWS < N; tile += gridDim.x) {
    const int row0 = tile * ROWS + wave * 16;
    if (row0 >= N) continue;
    const int row = (row0 + li < N) ? row0 + li : N - 1;
    f32x4 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < K / 16; ++s) {
      const float* src = (s * 16 < K1) ? (A1 + (size_t)row * K1 + s * 16) : (A2 + (size_t)row * K2 + (s * 16 - K1));
      const float4 a4 = *(const float4*)(src + 4 * kq);
      const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
      for (int mm = 0; mm < 4; ++mm) {
        const int k = s * 16 + 4 * kq + mm;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const float bv = sW[k * PITCH + nt * 16 + li];
          acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mm], bv, acc[nt], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int orow = row0 + kq * 4 + rr;
        if (orow >= N) continue;
        const int n = nt * 16 + li;
        float v = acc[nt][rr];
        if (EPI == EPI_BIAS_TANH) {
          v = tanhf(v + bias[n]);
          if (zero_out) zero_out[(size_t)orow * 32 + n] = 0.f;
        }
        if (EPI == EPI_BWD) {
          const int lab = b.node_label[orow];
          if (lab < 2) v += gfeat[(size_t)b.node_graph[orow] * D + lab * 128 + rlayer * 32 + n];
          const float xv = xin[(size_t)orow * 32 + n];
          v *= (1.f - xv * xv);
        }
        out[(size_t)orow * NO + n] = v;
      }
    }
  }
}

// Y_l = h_{l-1} @ [basis_0|..|basis_3] for l = 1..3 in ONE launch (blockIdx.y = l-1)
__global__ __launch_bounds__(IGMC_BLOCK) void k_dense_y_all(BatchDev b, ModelDev m, const float* __restrict__ P) {
  igmc_kernarg_warm<sizeof(BatchDev) + sizeof(ModelDev) + 32>();
  IGMC_DYN_SMEM(smem);
  const int li = blockIdx.y;
  dense_body<0, 32, 128, EPI_NONE, W_YCAT>(b, nullptr, m.h[li], P + m.off_basis[li + 1], nullptr, nullptr, m.Y[li],
                                           nullptr, nullptr, 0, 0, nullptr, (float*)smem);
}

// =================================================================== fused R-GCN layer (gather + dense)
// One 256-thread workgroup per tile of 16 rows: wave w walks rows 4w..4w+3 of the tile in basis space straight into an LDS
// tile [16][A(128) | self(32)], ONE 16-lane group per row (all 2400 waves of an ml_1m batch are resident at once), then
// the 4 waves multiply the tile with the layer's [basis ; root] operand on f32 MFMA (2 column tiles x 2 K-slices of 80,
// 20 MFMAs each) and the epilogue (bias + tanh, or the tanh' / readout-gradient backward epilogue) writes the 128-byte
// output rows.  Forward never materialises the 512-byte basis-space rows in HBM; backward writes them once (the weight
// gradient needs them).  (Rounds 1-2 kept three more formulations selectable -- separate gather + dense kernels,
// 16-wave tiles, tiles of row segments: all measured slower, removed in round 3.)
#define IGMC_TP 164
template <bool FLAGS, bool BWD>
__global__ __launch_bounds__(IGMC_BLOCK) void k_rgcn_layer4(BatchDev b, ModelDev m, const float* __restrict__ P, int l,
                                                             float* __restrict__ zero_out) {
  igmc_kernarg_warm<sizeof(BatchDev) + sizeof(ModelDev) + 32>();
  IGMC_DYN_SMEM(smem);
  const int R = m.R;
  float* tile = (float*)smem;               // [16][IGMC_TP]
  float* red = tile + 16 * IGMC_TP;         // [2 k-slices][2 col tiles][64 lanes * 4]
  float* s_att = red + 1024;                // [R][4]
  float* s_gatt = s_att + R * 4;            // BWD: [16 groups][R*4]
  const float* __restrict__ in = BWD ? m.dpre[l] : m.h[l - 1];
  const float* __restrict__ Yl = BWD ? m.Y[l - 1] : nullptr;
  const float* att = P + m.off_att[l];
  const float* basis = P + m.off_basis[l];
  const float* root = P + m.off_root[l];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = lane >> 4, t = lane & 15;
  const int li = lane & 15, kq = lane >> 4;
  for (int i = tid; i < R * 4; i += IGMC_BLOCK) s_att[i] = att[i];
  if (BWD)
    for (int i = tid; i < 16 * R * 4; i += IGMC_BLOCK) s_gatt[i] = 0.f;
  const int nt = wave & 1, ks = wave >> 1;
  float bw[20];
#pragma unroll
  for (int j = 0; j < 20; ++j) {
    const int k = ks * 80 + 4 * j + kq, n = nt * 16 + li;
    if (!BWD) bw[j] = basis[k * 32 + n];
    else bw[j] = (k < 128) ? basis[((k >> 5) * 32 + n) * 32 + (k & 31)] : root[n * 32 + (k - 128)];
  }
  __syncthreads();
  const int N = b.totals[0];
  const int trow = wave * 4 + grp;            // row of the tile owned by this 16-lane group
  float* my_gatt = s_gatt + trow * R * 4;
  const XcdSeg seg = igmc_xcd_segment(b);
  (void)N;
  for (int tl = seg.j; seg.lo + tl * 16 < seg.hi; tl += seg.nj) {
    const int trow0 = seg.lo + tl * 16;       // first row of the tile (tiles are cut per XCD segment)
    const int i = trow0 + trow;
    // everything that does not depend on the gather is requested FIRST, so that it is in flight during the
    // index / feature-row round trips: row bounds, the self row, and the epilogue operands of this thread
    int beg = 0, end = 0;
    float2 xs;
    xs.x = 0.f;
    xs.y = 0.f;
    if (i < seg.hi) {
      beg = b.row_ptr[i];
      end = b.row_ptr[i + 1];
      xs = *(const float2*)(in + (size_t)i * 32 + 2 * t);
    }
    float epi_x[2] = {0.f, 0.f}, epi_b[2] = {0.f, 0.f};
    int epi_lab[2] = {9, 9}, epi_g[2] = {0, 0};
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
      const int o = tid + h2 * IGMC_BLOCK;
      const int ol = (o & 255) >> 2, rr = o & 3;
      const int orow = trow0 + (ol >> 4) * 4 + rr, n = (o >> 8) * 16 + (ol & 15);
      if (!BWD) {
        epi_b[h2] = P[m.off_bias[l] + n];
      } else if (orow < seg.hi) {
        epi_lab[h2] = b.node_label[orow];
        epi_g[h2] = b.node_graph[orow];
        epi_x[h2] = m.h[l - 1][(size_t)orow * 32 + n];
      }
    }
    if (i < seg.hi) {
      float ax[4], ay[4];
#ifdef IGMC_EXP_CAPROW
      if (end > beg + IGMC_EXP_CAPROW) end = beg + IGMC_EXP_CAPROW;      // timing experiment only (wrong results)
#endif
      gather_row<FLAGS, BWD, BWD, 1>(b, in, s_att, my_gatt, Yl, i, beg, end, lane, ax, ay);
#pragma unroll
      for (int bb = 0; bb < 4; ++bb) {
        tile[trow * IGMC_TP + bb * 32 + 2 * t] = ax[bb];
        tile[trow * IGMC_TP + bb * 32 + 2 * t + 1] = ay[bb];
        if (BWD) {
          float2 o;
          o.x = ax[bb];
          o.y = ay[bb];
          *(float2*)(m.gagg[l - 1] + (size_t)i * 128 + bb * 32 + 2 * t) = o;
        }
      }
      tile[trow * IGMC_TP + 128 + 2 * t] = xs.x;
      tile[trow * IGMC_TP + 128 + 2 * t + 1] = xs.y;
    } else {
#pragma unroll
      for (int q = 0; q < 5; ++q) {
        tile[trow * IGMC_TP + q * 32 + 2 * t] = 0.f;
        tile[trow * IGMC_TP + q * 32 + 2 * t + 1] = 0.f;
      }
    }
    __syncthreads();
    {
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 20; ++j) {
        const float a = tile[li * IGMC_TP + ks * 80 + 4 * j + kq];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bw[j], acc, 0, 0, 0);
      }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) red[(ks * 2 + nt) * 256 + lane * 4 + rr] = acc[rr];
    }
    __syncthreads();
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
      const int o = tid + h2 * IGMC_BLOCK;
      const int ont = o >> 8, idx = o & 255, ol = idx >> 2, rr = idx & 3;
      const float v0 = red[(0 * 2 + ont) * 256 + idx] + red[(1 * 2 + ont) * 256 + idx];
      const int orow = trow0 + (ol >> 4) * 4 + rr, n = ont * 16 + (ol & 15);
      if (orow < seg.hi) {
        float v = v0;
        if (!BWD) {
          v = tanhf(v + epi_b[h2]);
          m.h[l][(size_t)orow * 32 + n] = v;
          if (zero_out) zero_out[(size_t)orow * 32 + n] = 0.f;
        } else {
          const int lab = epi_lab[h2];
          if (m.dcat[l - 1]) v += m.dcat[l - 1][(size_t)orow * 32 + n];
          else if (lab < 2) v += m.gfeat[(size_t)epi_g[h2] * m.D + lab * 128 + (l - 1) * 32 + n];
          const float xv = epi_x[h2];
          m.dpre[l - 1][(size_t)orow * 32 + n] = v * (1.f - xv * xv);
        }
      }
    }
    __syncthreads();
  }
  if (BWD) {
    float* gp = m.gatt_part + ((size_t)(l - 1) * IGMC_GATHER_BLOCKS + blockIdx.x) * R * 4;
    for (int i = tid; i < R * 4; i += IGMC_BLOCK) {
      float sacc = 0.f;
      for (int g = 0; g < 16; ++g) sacc += s_gatt[g * R * 4 + i];
      gp[i] = sacc;
    }
  }
}

// =================================================================== weight gradients  G = X^T [D1 | D2]
// X = h_{l-1} [N,32], D1 = G_l [N,128], D2 = dPre_l [N,32]  ->  per-block partial [32][160] (+ column sums of
// D2 = d bias).  Layer slices ly = ly_base + blockIdx.y (0..2 = conv layers 1..3, 3 = layer 0) in ONE launch.
// (Running the slices as parallel graph branches on auxiliary streams was measured SLOWER: every cross-stream
// edge of the hipGraph costs several microseconds on this part -- more than the kernels it would hide.)
__device__ __forceinline__ void wgrad_body(const BatchDev& b, const ModelDev& m, int ly) {
  __shared__ float sacc[32 * IGMC_KCAT + 32];
  // ly == 3: layer 0, whose "X" is synthesised from the per-node code histogram cnt0 plus the one-hot
  // columns for d root0[label] / d bias0 (codes < 32 only; larger tables use k_l0_bwd)
  const bool is_l0 = ly == 3;
  const int RL = m.R * m.L;
  const float* __restrict__ X = m.h[is_l0 ? 0 : ly];
  const float* __restrict__ D1 = m.gagg[is_l0 ? 0 : ly];
  const float* __restrict__ D2 = m.dpre[is_l0 ? 0 : ly + 1];
  float* part = m.wg_part + ((size_t)ly * IGMC_WG_BLOCKS + blockIdx.x) * (32 * IGMC_KCAT + 32);
  const int N = b.totals[0];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, kq = lane >> 4;
  f32x4 acc[2][10];
#pragma unroll
  for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
    for (int nt = 0; nt < 10; ++nt) acc[m2][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bsum[2] = {0.f, 0.f};
  const int ntile = (N + 15) >> 4;
  // A tile = 16 rows = four row-groups (row 4 rg + kq feeds k-slot kq of MFMA step rg).  All operands of a tile are
  // requested at once and the next tile's before this tile's 80 MFMAs, as 16-byte loads: lane li takes the B columns
  // 8 li .. 8 li + 7 of G (tile nt <-> column 8 li + nt) and 2 li, 2 li + 1 of dPre -- the column order inside the
  // product is free, the copy-out below undoes it (4 loads per row-group instead of 11 four-byte ones).
  struct WgTile {
    float2 a2[4];
    float4 ga[4], gb[4];
    float2 d2[4];
  };
  auto load_tile = [&](int tile, WgTile& t) {
    const int row0 = tile * 16;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int row = row0 + 4 * rg + kq;
      const bool ok = row < N;
      const int rs = ok ? row : 0;
      t.ga[rg] = make_float4(0.f, 0.f, 0.f, 0.f);
      t.gb[rg] = t.ga[rg];
      if (!is_l0) {
        t.a2[rg] = *(const float2*)(X + (size_t)rs * 32 + 2 * li);
        if (ok) {
          t.ga[rg] = *(const float4*)(D1 + (size_t)rs * 128 + 8 * li);
          t.gb[rg] = *(const float4*)(D1 + (size_t)rs * 128 + 8 * li + 4);
        }
      } else {
        const int lab = b.node_label[rs];
        const int c0 = 2 * li, c1 = 2 * li + 1;
        t.a2[rg].x = (c0 < RL) ? (float)m.cnt0[(size_t)rs * RL + c0] : ((c0 == RL + lab || c0 == RL + m.L) ? 1.f : 0.f);
        t.a2[rg].y = (c1 < RL) ? (float)m.cnt0[(size_t)rs * RL + c1] : ((c1 == RL + lab || c1 == RL + m.L) ? 1.f : 0.f);
      }
      if (!ok) { t.a2[rg].x = 0.f; t.a2[rg].y = 0.f; }
      t.d2[rg] = ok ? *(const float2*)(D2 + (size_t)rs * 32 + 2 * li) : make_float2(0.f, 0.f);
    }
  };
  const int tstep = gridDim.x * 4;
  int tile = blockIdx.x * 4 + wave;
  WgTile cur;
  if (tile < ntile) load_tile(tile, cur);
  for (; tile < ntile; tile += tstep) {
    WgTile nxt;
    const bool more = tile + tstep < ntile;
    if (more) load_tile(tile + tstep, nxt);
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const float bv[10] = {cur.ga[rg].x, cur.ga[rg].y, cur.ga[rg].z, cur.ga[rg].w, cur.gb[rg].x,
                            cur.gb[rg].y, cur.gb[rg].z, cur.gb[rg].w, cur.d2[rg].x, cur.d2[rg].y};
#pragma unroll
      for (int nt = 0; nt < 10; ++nt) {
        if (is_l0 && nt < 8) continue;
        if (nt >= 8) bsum[nt - 8] += bv[nt];
        acc[0][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a2[rg].x, bv[nt], acc[0][nt], 0, 0, 0);
        acc[1][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.a2[rg].y, bv[nt], acc[1][nt], 0, 0, 0);
      }
    }
    if (more) cur = nxt;
  }
  // d bias: reduce the 4 row-slots (kq) of each column
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    bsum[q] += __shfl_xor(bsum[q], 16, 64);
    bsum[q] += __shfl_xor(bsum[q], 32, 64);
  }
  // deterministic cross-wave reduction through LDS, wave 0 first (LDS keeps the product's column order: tile-major)
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
        for (int nt = 0; nt < 10; ++nt)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const int f = 2 * (kq * 4 + rr) + m2, n = nt * 16 + li;
            const float v = acc[m2][nt][rr];
            if (w == 0) sacc[f * IGMC_KCAT + n] = v;
            else sacc[f * IGMC_KCAT + n] += v;
          }
      if (kq == 0) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          if (w == 0) sacc[32 * IGMC_KCAT + q * 16 + li] = bsum[q];
          else sacc[32 * IGMC_KCAT + q * 16 + li] += bsum[q];
        }
      }
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < 32 * IGMC_KCAT + 32; i += IGMC_BLOCK) {
    int src;
    if (i < 32 * IGMC_KCAT) {
      const int f = i / IGMC_KCAT, n = i - f * IGMC_KCAT;
      const int np = (n < 128) ? (n & 7) * 16 + (n >> 3) : (8 + ((n - 128) & 1)) * 16 + ((n - 128) >> 1);
      src = f * IGMC_KCAT + np;
    } else {
      const int c = i - 32 * IGMC_KCAT;
      src = 32 * IGMC_KCAT + (c & 1) * 16 + (c >> 1);
    }
    part[i] = sacc[src];
  }
}

__global__ __launch_bounds__(IGMC_BLOCK) void k_wgrad(BatchDev b, ModelDev m, int ly_base) {
  igmc_kernarg_warm<sizeof(BatchDev) + sizeof(ModelDev) + 32>();
  wgrad_body(b, m, ly_base + blockIdx.y);
}

// =================================================================== layer 0 backward (dense, no edges)
// T[c][f] = sum_i weight(i,c) * dPre0[i][f],  c < R*L: cnt0[i][c] (kept in-edges with that code);
// c = R*L + label_i: d root0;  c = R*L + L: d bias0.   Thread (cg = tid>>5, f = tid&31) owns codes cg + 8k.
// Each block reduces a contiguous node range into its own partial (fixed order -> reproducible).
template <int KMAX>
__global__ __launch_bounds__(IGMC_BLOCK) void k_l0_bwd(BatchDev b, ModelDev m, const float* __restrict__ dpre,
                                                         float* __restrict__ part) {
  igmc_kernarg_warm<sizeof(BatchDev) + sizeof(ModelDev) + 32>();
  const int N = b.totals[0];
  const int RL = m.R * m.L, rows = RL + m.L + 1;
  const int f = threadIdx.x & 31, cg = threadIdx.x >> 5;
  float acc[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) acc[k] = 0.f;
  const int chunk = (N + (int)gridDim.x - 1) / (int)gridDim.x;
  const int lo = blockIdx.x * chunk, hi = (lo + chunk < N) ? lo + chunk : N;
  for (int i0 = lo; i0 < hi; i0 += 4) {          // 4 nodes in flight: the loads of a group are independent
    float d[4];
    int lab[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = (i0 + u < hi) ? i0 + u : hi - 1;
      d[u] = (i0 + u < hi) ? dpre[(size_t)i * 32 + f] : 0.f;
      lab[u] = b.node_label[i];
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int c = cg + 8 * k;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = (i0 + u < hi) ? i0 + u : hi - 1;
        float w = 0.f;
        if (c < RL) w = (float)m.cnt0[(size_t)i * RL + c];
        else if (c == RL + lab[u] || c == RL + m.L) w = 1.f;
        acc[k] += w * d[u];
      }
    }
  }
  float* dst = part + (size_t)blockIdx.x * rows * 32;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int c = cg + 8 * k;
    if (c < rows) dst[c * 32 + f] = acc[k];
  }
}

// =================================================================== head: readout + MLP (+loss residual)
// reference models.py:203-215.  IGMC_HG graphs per workgroup; lin1.weight [128, D] is read in its native
// layout: one wave per output unit j, lanes across the fan-in (coalesced), wave reduction per (graph, j).
__device__ __forceinline__ float head_feat(const BatchDev& b, const ModelDev& m, int g, int k) {
  if (k < 256) {
    const int side = k >> 7, l = (k >> 5) & 3, f = k & 31;
    const int nu = b.node_off[g], nv = nu + b.n_users[g];
    return m.h[l][(size_t)(side ? nv : nu) * 32 + f];
  }
  return m.side[(size_t)g * m.S + (k - 256)];
}

template <bool FEAT_LDS>
__global__ __launch_bounds__(512) void k_head_fwd(BatchDev b, ModelDev m, const float* __restrict__ P, int training,
                                                    const uint8_t* __restrict__ inj_mask, uint64_t seed,
                                                    uint64_t step_arg, float mult, float* __restrict__ out) {
  igmc_kernarg_warm<sizeof(BatchDev) + sizeof(ModelDev) + 32>();
  IGMC_DYN_SMEM(smem);
  const uint64_t step = m.ctrl ? (uint64_t)m.ctrl[IGMC_CTRL_STEP] : step_arg;
  __shared__ float sa[IGMC_HG][128];
  __shared__ float red[2][IGMC_HG];
  float* sfeat = (float*)smem;      // [HG][D]  (FEAT_LDS)
  const int B = b.totals[3];
  const int g0 = blockIdx.x * IGMC_HG, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int D = m.D;
  for (int idx = tid; idx < IGMC_HG * D; idx += 512) {
    const int gg = idx / D, k = idx % D, g = g0 + gg;
    const float v = (g < B) ? head_feat(b, m, g, k) : 0.f;
    if (g < B) m.feat[(size_t)g * D + k] = v;
    if (FEAT_LDS) sfeat[idx] = v;
  }
  __syncthreads();
  for (int j = wave; j < 128; j += 8) {
    float acc[IGMC_HG];
#pragma unroll
    for (int gg = 0; gg < IGMC_HG; ++gg) acc[gg] = 0.f;
    const float* wrow = P + m.off_l1w + (int64_t)j * D;
    for (int k = lane; k < D; k += 64) {
      const float w = wrow[k];
#pragma unroll
      for (int gg = 0; gg < IGMC_HG; ++gg) {
        const float fv = FEAT_LDS ? sfeat[gg * D + k] : ((g0 + gg < B) ? m.feat[(size_t)(g0 + gg) * D + k] : 0.f);
        acc[gg] += w * fv;
      }
    }
#pragma unroll
    for (int gg = 0; gg < IGMC_HG; ++gg) {
      const float s = igmc_wave_sum_f(acc[gg]);
      if (lane == 0) sa[gg][j] = s + P[m.off_l1b + j];
    }
  }
  __syncthreads();
  if (tid < 128) {
    const int j = tid;
    const float w2 = P[m.off_l2w + j];
#pragma unroll
    for (int gg = 0; gg < IGMC_HG; ++gg) {
      const int g = g0 + gg;
      float a = sa[gg][j] > 0.f ? sa[gg][j] : 0.f;
      if (training && g < B) {
        m.a1[g * 128 + j] = a;
        const int keep = inj_mask ? (int)inj_mask[g * 128 + j]
                                  : (int)(igmc_u01(igmc_unit_hash(seed, step, (uint32_t)g, (uint32_t)j)) >= 0.5f);
        m.lmask[g * 128 + j] = (uint8_t)keep;
        a = keep ? a * 2.f : 0.f;    // F.dropout(p=0.5): kept units scaled by 1/(1-p)
      }
      const float p = igmc_wave_sum_f(a * w2);
      if ((j & 63) == 0) red[j >> 6][gg] = p;
    }
  }
  __syncthreads();
  if (tid < IGMC_HG && g0 + tid < B) {
    const float o = (red[0][tid] + red[1][tid] + P[m.off_l2b]) * mult;
    out[g0 + tid] = o;
    m.err[g0 + tid] = o - b.y[g0 + tid];
  }
}

// backward A: dz, d feat, and dPre of the top layer on the two target rows of each graph.
// 1024 threads = 4 slices of the 128 hidden units x 256 fan-in columns.
__global__ __launch_bounds__(1024) void k_head_bwd_a(BatchDev b, ModelDev m, const float* __restrict__ P,
                                                       const float* __restrict__ gout, int from_err,
                                                       float grad_scale, float mult, float drop_scale,
                                                       float* __restrict__ dpre_top) {
  igmc_kernarg_warm<sizeof(BatchDev) + sizeof(ModelDev) + 32>();
  __shared__ float sdz[IGMC_HG][128];
  __shared__ float sred[3][IGMC_HG][256];
  const int B = b.totals[3];
  const int g0 = blockIdx.x * IGMC_HG, tid = threadIdx.x;
  const int D = m.D;
  for (int idx = tid; idx < IGMC_HG * 128; idx += 1024) {
    const int gg = idx >> 7, j = idx & 127, g = g0 + gg;
    float dzv = 0.f;
    if (g < B) {
      const float dp = (from_err ? 2.f * m.err[g] * grad_scale : gout[g]) * mult;
      const float a = m.a1[g * 128 + j];
      dzv = (a > 0.f && m.lmask[g * 128 + j]) ? dp * P[m.off_l2w + j] * drop_scale : 0.f;
      m.dz[g * 128 + j] = dzv;
    }
    sdz[gg][j] = dzv;
  }
  __syncthreads();
  const int kk = tid & 255, js = tid >> 8;
  for (int kc = 0; kc < D; kc += 256) {
    const int k = kc + kk;
    float acc[IGMC_HG];
#pragma unroll
    for (int gg = 0; gg < IGMC_HG; ++gg) acc[gg] = 0.f;
    if (k < D) {
#pragma unroll 8
      for (int jj = js * 32; jj < js * 32 + 32; ++jj) {
        const float w = P[m.off_l1w + (int64_t)jj * D + k];
#pragma unroll
        for (int gg = 0; gg < IGMC_HG; ++gg) acc[gg] += sdz[gg][jj] * w;
      }
    }
    if (js > 0) {
#pragma unroll
      for (int gg = 0; gg < IGMC_HG; ++gg) sred[js - 1][gg][kk] = acc[gg];
    }
    __syncthreads();
    if (js == 0 && k < D) {
#pragma unroll
      for (int gg = 0; gg < IGMC_HG; ++gg) {
        const int g = g0 + gg;
        if (g >= B) continue;
        const float v = ((acc[gg] + sred[0][gg][kk]) + sred[1][gg][kk]) + sred[2][gg][kk];
        m.gfeat[(size_t)g * D + k] = v;
        if (k < 256 && ((k >> 5) & 3) == 3) {
          const int side = k >> 7, f = k & 31;
          const int nu = b.node_off[g], nv = nu + b.n_users[g];
          const size_t node = (size_t)(side ? nv : nu);
          const float hv = m.h[3][node * 32 + f];
          dpre_top[node * 32 + f] = v * (1.f - hv * hv);
        }
      }
    }
    __syncthreads();
  }
}

// backward B: d lin1.weight [128, D] = dz^T @ feat.  Block (jt, kc): 8 hidden units x 256 fan-in columns;
// feat / dz are staged through LDS in chunks of 32 graphs.  One extra block row does the bias/lin2 grads.
#define IGMC_HW_G 32
__global__ __launch_bounds__(IGMC_BLOCK) void k_head_bwd_w(BatchDev b, ModelDev m, const float* __restrict__ P,
                                                             const float* __restrict__ gout, int from_err,
                                                             float grad_scale, float mult, float drop_scale,
                                                             float* __restrict__ grad) {
  igmc_kernarg_warm<sizeof(BatchDev) + sizeof(ModelDev) + 32>();
  __shared__ float sfe[IGMC_HW_G][256];
  __shared__ float sdz[IGMC_HW_G][8];
  const int B = b.totals[3];
  const int D = m.D, tid = threadIdx.x;
  if (blockIdx.x == 16) {                 // d lin1.bias, d lin2.weight, d lin2.bias (blockIdx.y == 0 only)
    if (blockIdx.y != 0) return;
    if (tid < 128) {
      float s = 0.f;
      for (int g = 0; g < B; ++g) s += m.dz[g * 128 + tid];
      grad[m.off_l1b + tid] = s;
    } else {
      const int j = tid - 128;
      float s = 0.f, s2 = 0.f;
      for (int g = 0; g < B; ++g) {
        const float dp = (from_err ? 2.f * m.err[g] * grad_scale : gout[g]) * mult;
        const float a = m.lmask[g * 128 + j] ? m.a1[g * 128 + j] * drop_scale : 0.f;
        s += dp * a;
        s2 += dp;
      }
      grad[m.off_l2w + j] = s;
      if (j == 0) grad[m.off_l2b] = s2;
    }
    return;
  }
  const int j0 = blockIdx.x * 8, k = blockIdx.y * 256 + tid;
  float acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = 0.f;
  for (int gc = 0; gc < B; gc += IGMC_HW_G) {
    const int ng = (B - gc < IGMC_HW_G) ? B - gc : IGMC_HW_G;
    for (int gg = 0; gg < ng; ++gg) sfe[gg][tid] = (k < D) ? m.feat[(size_t)(gc + gg) * D + k] : 0.f;
    if (tid < ng * 8) sdz[tid >> 3][tid & 7] = m.dz[(gc + (tid >> 3)) * 128 + j0 + (tid & 7)];
    __syncthreads();
    for (int gg = 0; gg < ng; ++gg) {
      const float fv = sfe[gg][tid];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] += sdz[gg][q] * fv;
    }
    __syncthreads();
  }
  if (k < D) {
#pragma unroll
    for (int q = 0; q < 8; ++q) grad[m.off_l1w + (int64_t)(j0 + q) * D + k] = acc[q];
  }
}

// =================================================================== head on f32 MFMA (D % 16 == 0)
// The three head products are tiny GEMMs ([B,D]x[D,128], [B,128]x[128,D], [128,B]x[B,D]); both MFMA operands
// are loaded straight from global memory as float4 / 64-byte row segments (no LDS staging), so each kernel is
// a handful of MFMAs per wave and finishes in the launch floor.
__device__ __forceinline__ const float* head_feat_ptr(const BatchDev& b, const ModelDev& m, int g, int k) {
  if (k < 256) {
    const int side = k >> 7, l = (k >> 5) & 3, f = k & 31;
    const int nu = b.node_off[g], nv = nu + b.n_users[g];
    return m.h[l] + (size_t)(side ? nv : nu) * 32 + f;
  }
  return m.side + (size_t)g * m.S + (k - 256);
}

// lin1 (+ReLU, dropout) + lin2 for 16 graphs per workgroup; wave w owns hidden units [16w, 16w+16)
__global__ __launch_bounds__(512) void k_head_fwd_mfma(BatchDev b, ModelDev m, const float* __restrict__ P,
                                                         int training, const uint8_t* __restrict__ inj_mask,
                                                         uint64_t seed, uint64_t step_arg, float mult,
                                                         float* __restrict__ out) {
  igmc_kernarg_warm<sizeof(BatchDev) + sizeof(ModelDev) + 32>();
  __shared__ float spart[8][16];
  const uint64_t step = m.ctrl ? (uint64_t)m.ctrl[IGMC_CTRL_STEP] : step_arg;
  const int B = b.totals[3], D = m.D;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, kq = lane >> 4;
  const int row0 = blockIdx.x * 16, n0 = wave * 16;
  const int ga = (row0 + li < B) ? row0 + li : B - 1;        // graph feeding the A fragment of this lane
  const float* wrow = P + m.off_l1w + (int64_t)(n0 + li) * D;
  f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nch = D / 16;
  for (int s0 = 0; s0 < nch; s0 += 8) {          // 8 chunks (16 float4 loads) in flight before the MFMAs
    float4 a4[8], b4[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k0 = ((s0 + u < nch) ? s0 + u : nch - 1) * 16 + 4 * kq;
      a4[u] = *(const float4*)head_feat_ptr(b, m, ga, k0);
      b4[u] = *(const float4*)(wrow + k0);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (s0 + u >= nch) continue;
      const int k0 = (s0 + u) * 16 + 4 * kq;
      if (training && wave == 0 && row0 + li < B) *(float4*)(m.feat + (size_t)ga * D + k0) = a4[u];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u].x, b4[u].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u].y, b4[u].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u].z, b4[u].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u].w, b4[u].w, acc, 0, 0, 0);
    }
  }
  const int n = n0 + li;
  const float b1 = P[m.off_l1b + n], w2 = P[m.off_l2w + n];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int r = kq * 4 + rr, g = row0 + r;
    float a = acc[rr] + b1;
    a = a > 0.f ? a : 0.f;
    if (training && g < B) {
      m.a1[g * 128 + n] = a;
      const int keep = inj_mask ? (int)inj_mask[g * 128 + n]
                                : (int)(igmc_u01(igmc_unit_hash(seed, step, (uint32_t)g, (uint32_t)n)) >= 0.5f);
      m.lmask[g * 128 + n] = (uint8_t)keep;
      a = keep ? a * 2.f : 0.f;    // F.dropout(p=0.5): kept units scaled by 1/(1-p)
    }
    const float p = igmc_group16_sum_f(a * w2);
    if (li == 0) spart[wave][r] = p;
  }
  __syncthreads();
  if (threadIdx.x < 16 && row0 + (int)threadIdx.x < B) {
    const int g = row0 + threadIdx.x;
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) s += spart[w][threadIdx.x];
    const float o = (s + P[m.off_l2b]) * mult;
    out[g] = o;
    m.err[g] = o - b.y[g];
  }
}

// Training head in ONE launch (fused-step path): blockIdx.y == 0 -> forward of 16 graphs, their residual, and
// immediately the backward down to d feat / dPre of the top layer (dz never leaves the workgroup except for
// the copy the lin1 weight gradient needs); blockIdx.y = 1..3 -> the Y products of the conv layers.
__global__ __launch_bounds__(512) void k_head_train(BatchDev b, ModelDev m, const float* __restrict__ P,
                                                      const uint8_t* __restrict__ inj_mask, uint64_t seed,
                                                      uint64_t step_arg, float mult, float grad_scale,
                                                      float* __restrict__ out) {
  igmc_kernarg_warm<sizeof(BatchDev) + sizeof(ModelDev) + 32>();
  IGMC_DYN_SMEM(smem);
  if (blockIdx.y > 0) {
    const int ly = blockIdx.y - 1;
    if ((int)blockIdx.x * 128 >= b.totals[0]) return;       // sized by the arena's node capacity: no tile, no staging
    dense_body<0, 32, 128, EPI_NONE, W_YCAT, 512>(b, nullptr, m.h[ly], P + m.off_basis[ly + 1], nullptr, nullptr,
                                                  m.Y[ly], nullptr, nullptr, 0, 0, nullptr, (float*)smem);
    return;
  }
  const int B = b.totals[3], D = m.D;
  const int row0 = blockIdx.x * 16;
  if (row0 >= B) return;
  __shared__ float spart[8][16];
  __shared__ float serr[16];
  __shared__ float sdz[16][132];
  // Four workgroups carry this role at batch 50, so its duration is the number of DEPENDENT memory round trips, not a
  // throughput: everything a later stage reads from memory (labels, lin2, the lin1 columns of the d feat product, the
  // top-layer rows of the target nodes) is requested up front, next to the operands of lin1.
  const uint64_t step = m.ctrl ? (uint64_t)m.ctrl[IGMC_CTRL_STEP] : step_arg;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, kq = lane >> 4;
  const int n0 = wave * 16;
  const int ga = (row0 + li < B) ? row0 + li : B - 1;
  const int n = n0 + li;
  const float* wrow = P + m.off_l1w + (int64_t)n * D;
  const int nch = D / 16;
  // targets' node rows of this lane's graphs (A rows of lin1: graph ga; epilogue of d feat: graphs row0 + 4 kq + rr)
  const int nu_a = b.node_off[ga], nv_a = nu_a + b.n_users[ga];
  int nu_e[4], nv_e[4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int g = row0 + kq * 4 + rr, gs = g < B ? g : B - 1;
    nu_e[rr] = b.node_off[gs];
    nv_e[rr] = nu_e[rr] + b.n_users[gs];
  }
  auto feat_ptr = [&](int k0) -> const float* {
    if (k0 < 256) return m.h[(k0 >> 5) & 3] + (size_t)((k0 >> 7) ? nv_a : nu_a) * 32 + (k0 & 31);
    return m.side + (size_t)ga * m.S + (k0 - 256);
  };
  // addresses as (uniform base) + (32-bit byte offset of the lane): one offset register serves every load of a kind and
  // the bases live in scalar registers -- the role is VALU-bound, not memory-bound, once its loads are batched (8 waves
  // on each of 4 CUs; address arithmetic was a third of its instructions)
  auto ld4 = [](const float* base, uint32_t byte) { return *(const float4*)((const char*)base + byte); };
  auto ld1 = [](const float* base, uint32_t byte) { return *(const float*)((const char*)base + byte); };
  const uint32_t offU = ((uint32_t)nu_a * 32u + 4u * kq) * 4u, offV = ((uint32_t)nv_a * 32u + 4u * kq) * 4u;
  const uint32_t offW = ((uint32_t)n * (uint32_t)D + 4u * kq) * 4u;
  f32x4 acc4[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) acc4[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float4 a4[16], b4[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) {                    // chunks 0..15 = the 256 conv features (D >= 256): k0 = 16 u + 4 kq
    a4[u] = ld4(m.h[(u >> 1) & 3] + (u & 1) * 16, (u >> 3) ? offV : offU);
    b4[u] = ld4(P + m.off_l1w + u * 16, offW);
  }
  const float b1 = P[m.off_l1b + n], w2 = P[m.off_l2w + n];
  const float l2b = P[m.off_l2b];
  const float yv = (threadIdx.x < 16 && row0 + (int)threadIdx.x < B) ? b.y[row0 + threadIdx.x] : 0.f;
  // d feat = dz @ lin1.weight: column tile nt = wave + 8 it (< 16: inside the conv features); its 32 x 4 weight values
  // and (tiles 6, 7 of a side = the top layer's slice of the concatenation) h_3 of the target rows
  float bvp[2][8][4];
  float hvp[2][4];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int c0 = (wave + 8 * it) * 16;
    const uint32_t offB = ((uint32_t)(4 * kq) * (uint32_t)D + (uint32_t)(c0 + li)) * 4u;
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int mm = 0; mm < 4; ++mm) bvp[it][u][mm] = ld1(P + m.off_l1w + (size_t)(u * 16 + mm) * D, offB);
    const int k = c0 + li;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      hvp[it][rr] = 0.f;
      if (((k >> 5) & 3) == 3) hvp[it][rr] = ld1(m.h[3], ((uint32_t)((k >> 7) ? nv_e[rr] : nu_e[rr]) * 32u + (uint32_t)(k & 31)) * 4u);
    }
  }
  for (int s0 = 0; s0 < nch; s0 += 16) {
    if (s0 > 0) {                                   // side features: D > 256
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int k0 = ((s0 + u < nch) ? s0 + u : nch - 1) * 16 + 4 * kq;
        a4[u] = *(const float4*)feat_ptr(k0);
        b4[u] = *(const float4*)(wrow + k0);
      }
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      if (s0 + u >= nch) continue;
      const int k0 = (s0 + u) * 16 + 4 * kq;
      if (wave == 0 && row0 + li < B) *(float4*)(m.feat + (size_t)ga * D + k0) = a4[u];
      f32x4& acc = acc4[u & 3];                     // four independent chains instead of 64 dependent MFMAs
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u].x, b4[u].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u].y, b4[u].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u].z, b4[u].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[u].w, b4[u].w, acc, 0, 0, 0);
    }
  }
  float av[4];
  int kp[4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int r = kq * 4 + rr, g = row0 + r;
    float a = ((acc4[0][rr] + acc4[1][rr]) + (acc4[2][rr] + acc4[3][rr])) + b1;
    a = a > 0.f ? a : 0.f;
    av[rr] = a;
    kp[rr] = 0;
    if (g < B) {
      m.a1[g * 128 + n] = a;
      kp[rr] = inj_mask ? (int)inj_mask[g * 128 + n]
                        : (int)(igmc_u01(igmc_unit_hash(seed, step, (uint32_t)g, (uint32_t)n)) >= 0.5f);
      m.lmask[g * 128 + n] = (uint8_t)kp[rr];
    }
    const float p = igmc_group16_sum_f((kp[rr] ? a * 2.f : 0.f) * w2);
    if (li == 0) spart[wave][r] = p;
  }
  __syncthreads();
  if (threadIdx.x < 16) {
    const int g = row0 + threadIdx.x;
    float e = 0.f;
    if (g < B) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < 8; ++w) s += spart[w][threadIdx.x];
      const float o = (s + l2b) * mult;
      out[g] = o;
      e = o - yv;
      m.err[g] = e;
    }
    serr[threadIdx.x] = e;
  }
  __syncthreads();
  // ---- backward through lin2 / dropout / relu: dz (kept in LDS for the next product, copied out for d lin1.weight)
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int r = kq * 4 + rr, g = row0 + r;
    const float dp = 2.f * serr[r] * grad_scale * mult;
    const float dzv = (g < B && av[rr] > 0.f && kp[rr]) ? dp * w2 * 2.f : 0.f;
    sdz[r][n] = dzv;
    if (g < B) m.dz[g * 128 + n] = dzv;
  }
  __syncthreads();
  // ---- d feat = dz @ lin1.weight  (16 x 128 @ 128 x D), column tiles strided over the 8 waves
  for (int nt = wave, it = 0; nt * 16 < D; nt += 8, ++it) {
    const int c0 = nt * 16;
    f32x4 g4a = (f32x4){0.f, 0.f, 0.f, 0.f}, g4b = g4a;
    if (it < 2) {
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int mm = 0; mm < 4; ++mm) {
          f32x4& g4 = (u & 1) ? g4b : g4a;
          g4 = __builtin_amdgcn_mfma_f32_16x16x4f32(sdz[li][u * 16 + 4 * kq + mm], bvp[it][u][mm], g4, 0, 0, 0);
        }
    } else {
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int mm = 0; mm < 4; ++mm)
          g4a = __builtin_amdgcn_mfma_f32_16x16x4f32(sdz[li][u * 16 + 4 * kq + mm],
                                                     P[m.off_l1w + (int64_t)(u * 16 + 4 * kq + mm) * D + c0 + li], g4a, 0, 0, 0);
    }
    const int k = c0 + li;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int g = row0 + kq * 4 + rr;
      if (g >= B) continue;
      const float v = g4a[rr] + g4b[rr];
      m.gfeat[(size_t)g * D + k] = v;
      if (k < 256 && ((k >> 5) & 3) == 3) {
        const size_t node = (size_t)((k >> 7) ? nv_e[rr] : nu_e[rr]);
        const float hv = hvp[it & 1][rr];
        m.dpre[3][node * 32 + (k & 31)] = v * (1.f - hv * hv);
      }
    }
  }
}

// d feat = dz @ lin1.weight, dz formed on the fly; wave -> 16 fan-in columns; also dPre of the top layer
__global__ __launch_bounds__(512) void k_head_bwd_a_mfma(BatchDev b, ModelDev m, const float* __restrict__ P,
                                                           const float* __restrict__ gout, int from_err,
                                                           float grad_scale, float mult, float drop_scale,
                                                           float* __restrict__ dpre_top) {
  igmc_kernarg_warm<sizeof(BatchDev) + sizeof(ModelDev) + 32>();
  const int B = b.totals[3], D = m.D;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, kq = lane >> 4;
  const int row0 = blockIdx.x * 16;
  const int nt = blockIdx.y * 8 + wave;
  if (nt * 16 >= D) return;
  const int n0 = nt * 16;
  const int ga = (row0 + li < B) ? row0 + li : B - 1;
  const bool arow_ok = row0 + li < B;
  const float dp = (from_err ? 2.f * m.err[ga] * grad_scale : gout[ga]) * mult;
  const float* w1 = P + m.off_l1w;
  f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const int j0 = s * 16 + 4 * kq;
    const float4 a4 = *(const float4*)(m.a1 + ga * 128 + j0);
    const uint32_t mk = *(const uint32_t*)(m.lmask + ga * 128 + j0);
    const float4 w4 = *(const float4*)(P + m.off_l2w + j0);
    float dzv[4];
    dzv[0] = (arow_ok && a4.x > 0.f && (mk & 0xFFu)) ? dp * w4.x * drop_scale : 0.f;
    dzv[1] = (arow_ok && a4.y > 0.f && ((mk >> 8) & 0xFFu)) ? dp * w4.y * drop_scale : 0.f;
    dzv[2] = (arow_ok && a4.z > 0.f && ((mk >> 16) & 0xFFu)) ? dp * w4.z * drop_scale : 0.f;
    dzv[3] = (arow_ok && a4.w > 0.f && ((mk >> 24) & 0xFFu)) ? dp * w4.w * drop_scale : 0.f;
    if (nt == 0 && arow_ok) {
      float4 o;
      o.x = dzv[0]; o.y = dzv[1]; o.z = dzv[2]; o.w = dzv[3];
      *(float4*)(m.dz + ga * 128 + j0) = o;
    }
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) {
      const float bv = w1[(int64_t)(j0 + mm) * D + n0 + li];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dzv[mm], bv, acc, 0, 0, 0);
    }
  }
  const int k = n0 + li;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int g = row0 + kq * 4 + rr;
    if (g >= B) continue;
    const float v = acc[rr];
    m.gfeat[(size_t)g * D + k] = v;
    if (k < 256 && ((k >> 5) & 3) == 3) {
      const int side = k >> 7, f = k & 31;
      const int nu = b.node_off[g], nv = nu + b.n_users[g];
      const size_t node = (size_t)(side ? nv : nu);
      const float hv = m.h[3][node * 32 + f];
      dpre_top[node * 32 + f] = v * (1.f - hv * hv);
    }
  }
}

// d lin1.weight = dz^T @ feat (reduction over the B graphs, 4 per MFMA); block x = 16 hidden units, wave -> 16
// fan-in columns.  Wave 0 of the y == 0 blocks also forms d lin1.bias = dz^T 1, d lin2.weight = adrop^T dp and
// d lin2.bias = 1^T dp with three more MFMAs per step (B operand = 1 / dp_g), so there is no serial tail.
__device__ __forceinline__ void head_bwd_w_body(const BatchDev& b, const ModelDev& m, const float* __restrict__ P,
                                                const float* __restrict__ gout, int from_err, float grad_scale,
                                                float mult, float drop_scale, float* __restrict__ grad, int bx, int by,
                                                int B_known = -1) {
  // (the batch size: a caller that has it in its arguments saves the dependent round trip to the arena's totals)
  const int B = B_known >= 0 ? B_known : b.totals[3], D = m.D, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kq = lane >> 4;
  const int j0 = bx * 16;
  const int nt = by * 4 + wave;
  if (nt * 16 >= D) return;
  const int n0 = nt * 16;
  const bool extra = nt == 0;
  f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
  f32x4 accb1 = acc, accw2 = acc, accb2 = acc;
  for (int g0 = 0; g0 < B; g0 += 32) {            // 8 MFMA steps (32 graphs) of loads in flight
    // every operand of the 8 steps is requested before the first use, at clamped addresses (a predicated load is a branch
    // and a wait; lmask -> a1 was a dependent pair): the wave with the extra products sits on the critical path of the
    // launch (k_tail_ts / k_wgrad_head), 32 serial round trips before
    float av[8], bv[8], ad[8], dpv[8];
    uint32_t mk[8];                     // (one register each: packed bytes would need every value right after its load)
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int g = g0 + 4 * u + kq;
      const int gs = g < B ? g : B - 1;
      av[u] = m.dz[gs * 128 + j0 + li];
      bv[u] = m.feat[(size_t)gs * D + n0 + li];
      dpv[u] = 0.f;
      ad[u] = 0.f;
      mk[u] = 0;
      if (extra) {
        dpv[u] = from_err ? m.err[gs] : gout[gs];
        ad[u] = m.a1[gs * 128 + j0 + li];
        mk[u] = m.lmask[gs * 128 + j0 + li];
      }
    }
#ifndef IGMC_HIPEMU
    __builtin_amdgcn_sched_barrier(0);        // (keeps the uses below from being hoisted between the loads)
    asm volatile("" : "+v"(mk[0]), "+v"(mk[1]), "+v"(mk[2]), "+v"(mk[3]), "+v"(mk[4]), "+v"(mk[5]), "+v"(mk[6]), "+v"(mk[7]));
#endif
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool ok = g0 + 4 * u + kq < B;
      if (!ok) { av[u] = 0.f; bv[u] = 0.f; }
      if (extra) {
        dpv[u] = ok ? (from_err ? 2.f * dpv[u] * grad_scale : dpv[u]) * mult : 0.f;
        ad[u] = (ok && mk[u]) ? ad[u] * drop_scale : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
      if (extra) {
        accb1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], (g0 + 4 * u + kq < B) ? 1.f : 0.f, accb1, 0, 0, 0);
        accw2 = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[u], dpv[u], accw2, 0, 0, 0);
        accb2 = __builtin_amdgcn_mfma_f32_16x16x4f32(1.f, dpv[u], accb2, 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) grad[m.off_l1w + (int64_t)(j0 + kq * 4 + rr) * D + n0 + li] = acc[rr];
  if (extra && li == 0) {       // every column of the extra accumulators holds the same sums
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      grad[m.off_l1b + j0 + kq * 4 + rr] = accb1[rr];
      grad[m.off_l2w + j0 + kq * 4 + rr] = accw2[rr];
    }
    if (bx == 0 && kq == 0) grad[m.off_l2b] = accb2[0];
  }
}

__global__ __launch_bounds__(IGMC_BLOCK) void k_head_bwd_w_mfma(BatchDev b, ModelDev m, const float* __restrict__ P,
                                                                  const float* __restrict__ gout, int from_err,
                                                                  float grad_scale, float mult, float drop_scale,
                                                                  float* __restrict__ grad) {
  igmc_kernarg_warm<sizeof(BatchDev) + sizeof(ModelDev) + 32>();
  head_bwd_w_body(b, m, P, gout, from_err, grad_scale, mult, drop_scale, grad, blockIdx.x, blockIdx.y);
}

// ONE launch for every weight-gradient product of the step: blockIdx.y < nsl -> conv weight-gradient slice,
// blockIdx.y == nsl -> d lin1 / d lin2 (linear block id = (j tile, column tile)).
__global__ __launch_bounds__(IGMC_BLOCK) void k_wgrad_head(BatchDev b, ModelDev m, const float* __restrict__ P,
                                                             const float* __restrict__ gout, int from_err,
                                                             float grad_scale, float mult, float drop_scale,
                                                             float* __restrict__ grad, int nsl) {
  igmc_kernarg_warm<sizeof(BatchDev) + sizeof(ModelDev) + 32>();
  if ((int)blockIdx.y < nsl) {
    wgrad_body(b, m, blockIdx.y);
  } else {
    const int ny = (m.D / 16 + 3) / 4;
    if ((int)blockIdx.x < 8 * ny)
      head_bwd_w_body(b, m, P, gout, from_err, grad_scale, mult, drop_scale, grad, blockIdx.x & 7, blockIdx.x >> 3);
  }
}

// =================================================================== partial reduction + finalize
// graw layout: [3][5152] conv1..3 (32x160 + 32) | [3][R*4] d att | [(R*L+L+1)*32] layer-0 table
// Sections A (weight-gradient partials) and C (layer-0 tables): 64 outputs x 4 partial-slices per block;
// section B (d att, few outputs x many partials): one wave per output.  Fixed summation order.

// nstash = 4: four extra workgroups stash the weights-only quantities of the conv layers for k_finalize_ts (basis-space
// mode), like the stash role of k_tail_ts.
__global__ __launch_bounds__(IGMC_BLOCK) void k_reduce_partials(ModelDev m, int n_gatt_parts, int l0_mfma,
                                                                  int n_wg_parts, const float* __restrict__ P,
                                                                  const int64_t* ctrl, int nstash) {
  igmc_kernarg_warm<sizeof(ModelDev) + 32>();
  __shared__ float sred[4][64];
  if (nstash && (int)blockIdx.x >= (int)gridDim.x - nstash) {
    fin_stash_body(m, P, (int)blockIdx.x - ((int)gridDim.x - nstash), ctrl);
    return;
  }
  const int wgs = 32 * IGMC_KCAT + 32, na = m.R * 4, rows0 = m.R * m.L + m.L + 1, n0 = rows0 * 32;
  const int nlay = l0_mfma ? 4 : 3;
  const int nblkA = (nlay * wgs + 63) / 64, nblkB = (3 * na + 3) / 4, nblkC = l0_mfma ? 0 : (n0 + 63) / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int blk = blockIdx.x;
  if (blk < nblkA + nblkC) {
    const bool secA = blk < nblkA;
    const int o = (secA ? blk : blk - nblkA) * 64 + lane;
    const int nout = secA ? nlay * wgs : n0;
    float s = 0.f;
    if (o < nout) {
      if (secA) {
        const int l = o / wgs, i = o % wgs;
        // 16 partials of a wave per round trip (clamped addresses; same order of additions)
        const float* p = m.wg_part + (size_t)l * IGMC_WG_BLOCKS * wgs + i;
        for (int k0 = wave; k0 < n_wg_parts; k0 += 64) {
          float v[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) {
            const int k = k0 + 4 * u;
            v[u] = p[(size_t)(k < n_wg_parts ? k : n_wg_parts - 1) * wgs];
          }
#pragma unroll
          for (int u = 0; u < 16; ++u)
            if (k0 + 4 * u < n_wg_parts) s += v[u];
        }
      } else {
        const float* p = m.l0_part + o;
        for (int k0 = wave; k0 < IGMC_L0_BLOCKS; k0 += 64) {
          float v[16];
#pragma unroll
          for (int u = 0; u < 16; ++u) {
            const int k = k0 + 4 * u;
            v[u] = p[(size_t)(k < IGMC_L0_BLOCKS ? k : IGMC_L0_BLOCKS - 1) * n0];
          }
#pragma unroll
          for (int u = 0; u < 16; ++u)
            if (k0 + 4 * u < IGMC_L0_BLOCKS) s += v[u];
        }
      }
    }
    sred[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && o < nout) {
      const float tot = (sred[0][lane] + sred[1][lane]) + (sred[2][lane] + sred[3][lane]);
      if (secA && o >= 3 * wgs) {
        // layer-0 slice of k_wgrad_all: partial[c][128 + f]  ->  table T0[c][f]
        const int i = o - 3 * wgs, c = i / IGMC_KCAT, col = i % IGMC_KCAT;
        if (i < 32 * IGMC_KCAT && c < rows0 && col >= 128) m.graw[3 * wgs + 3 * na + c * 32 + (col - 128)] = tot;
      } else {
        m.graw[secA ? o : 3 * wgs + 3 * na + o] = tot;
      }
    }
  } else {
    blk -= nblkA + nblkC;
    const int o = blk * 4 + wave;
    if (o < 3 * na && blk < nblkB) {
      const int l = o / na, i = o % na;
      const float* p = m.gatt_part + (size_t)l * IGMC_GATHER_BLOCKS * na + i;
      float s = 0.f;
      for (int k0 = lane; k0 < n_gatt_parts; k0 += 64 * 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int k = k0 + 64 * u;
          v[u] = p[(size_t)(k < n_gatt_parts ? k : n_gatt_parts - 1) * na];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (k0 + 64 * u < n_gatt_parts) s += v[u];
      }
      s = igmc_wave_sum_f(s);
      if (lane == 0) m.graw[3 * wgs + o] = s;
    }
  }
}

// The partial-table slots a launch filled, in the order their sums take them: member c of subgraph g sits in slot g + c * stride
// (one-workgroup launches: stride = IGMC_TS_BLOCKS, one member); the valid slots in the order (c, g) are numbered q = c * ng + g
struct TsSlots {
  int ng, nq, stride;
};
__device__ __forceinline__ TsSlots ts_slots(int nparts, int stride, int B) {
  TsSlots s;
  s.ng = (nparts < stride) ? nparts : ((B < stride) ? B : stride);
  s.nq = ((nparts + stride - 1) / stride) * s.ng;
  s.stride = stride;
  return s;
}
// slot of q (clamped to the last valid one: loads past the end are requested and not added)
__device__ __forceinline__ int ts_slot(const TsSlots& s, int q) {
  const int qc = q < s.nq ? q : s.nq - 1;
  const int c = qc / s.ng, g = qc - c * s.ng;
  return c * s.stride + g;
}

// Layer 3 where the subgraph kernel left centre vectors instead of tables (StepPlan::l3_vec = mv, the member that owns the
// item centre; vec = ModelDev::l3_vec): partial group pg's sum of one float4 column of the layer's table -- row j (j < R:
// dW_j, j == R: d root, j > R: the bias row), input row c, outputs c4 .. c4 + 3 -- over the slots q = pg, pg + 16, .. in order,
// as the table loops of reduce_ts_body / tf_sum_set form it.  Slot q is (member q / ng, subgraph g = q % ng), and its table is
//   member 0:   T_j[cu] (x) dPre_3[cu] of the user centre (d root: h_2[cu] (x) dPre_3[cu]; bias row: dPre_3[cu]),
//   member mv:  the item centre's likewise,
//   any other:  zeros,
// so the thread takes the subgraphs g = (pg - member * ng) mod 16, + 16, .. < ng of member 0, then those of member mv:
// ascending q, the table loop's order without its zero addends.
// WHY THE BITS ARE THE TABLE MODE'S (cs > 1): there an owner's slot holds round(t * d) + 0.f (the other centre's term of the
// two-term sum is a literal zero; fused or not, the sum rounds once, to round(t * d), and a product of -0.0 becomes +0.0) and
// every other member's holds +0.0.  The accumulators start at +0.0 and x + y is -0.0 only where both are, so they never
// become -0.0: adding +0.0 to one, or -0.0 where the table held +0.0, changes no bit of it, and dropping the addend changes
// none either.  What is left is acc += round(t * d) in the same order -- __fmul_rn, so that the product is rounded before the
// add here as well (it must not contract into an fma).  The bias row's slot held dPre_3[c] + zeros: the same argument.
// All loads of a thread are requested before its first add wherever a member has <= 64 subgraphs (<= 4 a thread and side).
__device__ __forceinline__ float4 l3_vec_sum(const float* __restrict__ vec, const TsSlots& sl, int mv, int R, int j, int c,
                                             int c4, int pg) {
  const int ng = sl.ng;
  const bool bias = j > R;
  const int trow = j < R ? j : G2_NR;                     // T_j[centre] or h_2[centre]
  float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f);
  auto request = [&](int side, int i0, float (&t)[4], float4 (&d)[4]) {
    const int r0 = (pg - (side ? mv : 0) * ng) & 15;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int g = r0 + 16 * (i0 + u), gc = g < ng ? g : ng - 1;      // (past the end: requested and not added, like ts_slot)
      const float* v = vec + ((size_t)gc * 2 + side) * ((G2_NR + 2) * 32);
      t[u] = bias ? 1.f : v[trow * 32 + c];
      d[u] = *(const float4*)(v + (G2_NR + 1) * 32 + c4);
    }
  };
  auto add = [&](int side, int i0, const float (&t)[4], const float4 (&d)[4]) {
    // (__fmul_rn alone is x * y to the compiler, which fuses it with the add under the default contraction: measured)
#ifndef IGMC_HIPEMU
#pragma clang fp contract(off)
#endif
    const int r0 = (pg - (side ? mv : 0) * ng) & 15;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (r0 + 16 * (i0 + u) < ng) {
        if (bias) {
          s4.x += d[u].x; s4.y += d[u].y; s4.z += d[u].z; s4.w += d[u].w;
        } else {
          s4.x += __fmul_rn(t[u], d[u].x); s4.y += __fmul_rn(t[u], d[u].y);
          s4.z += __fmul_rn(t[u], d[u].z); s4.w += __fmul_rn(t[u], d[u].w);
        }
      }
  };
  float tu[4], tv[4];
  float4 du[4], dv[4];
  if (ng <= 64) {
    request(0, 0, tu, du);
    request(1, 0, tv, dv);
    add(0, 0, tu, du);
    add(1, 0, tv, dv);
  } else {
    for (int side = 0; side < 2; ++side)
      for (int i0 = 0; 16 * i0 < ng; i0 += 4) {
        request(side, i0, tu, du);
        add(side, i0, tu, du);
      }
  }
  return s4;
}

// relation-space tables of graphstep.hip: ts_raw[l][i] = sum over the workgroups' partials (fixed order);
// 64 outputs per block, the 4 waves split the partial slices
// Pold != NULL: wave 0 also forms, per 32 consecutive outputs (always inside one dW_r block: ts_stride and fin*32 are
// multiples of 32), the partial dot products <dW_r, basis_b> (b = 0..3) with the CURRENT parameters -- d att[r,b] is
// the sum of the fin partials of its block (k_finalize_ts), so that kernel never reads a basis element it does not own.
// l3v != 0 (StepPlan::l3_vec): layer 3's tables were not stored -- its sums come from the centre vectors (l3_vec_sum)
__device__ __forceinline__ void reduce_ts_body(const ModelDev& m, int nparts, int stride, int B, int blk, int l3v,
                                               const float* __restrict__ Pold = nullptr) {
  // 64 outputs a workgroup as 16 float4 columns x 16 partial groups: thread (column o4 = lane & 15, group pg = 4 wave +
  // (lane >> 4)) sums the partial slots pg, pg + 16, .. of its four outputs (<= 14 sixteen-byte loads, all requested before
  // the first add: ONE round trip; a wave's load instruction covers four 256-byte runs), the 16 groups are then added in
  // index order through LDS -- a fixed order, so the result does not depend on the launch.  ~90 registers a thread: every
  // workgroup of the launch is resident at once (the 56-loads-a-thread form needed 292 and took two residency rounds).
  __shared__ float4 sred4[16][16];
  const int ts = m.ts_stride, rows0 = m.R * m.L + m.L + 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int o4 = lane & 15, pg = wave * 4 + (lane >> 4);
  const int o0 = blk * 64 + 4 * o4;                     // first of the thread's four outputs (ts is a multiple of 32: the four share a layer)
  const int l = o0 / ts, i0 = o0 % ts;
  const bool ok4 = l < 4 && (l > 0 || i0 < rows0 * 32);
  // wave 0's second role (Pold): the four basis values of ITS output blk * 64 + lane, requested together with the partials
  float pbv[4] = {0.f, 0.f, 0.f, 0.f};
  if (Pold && wave == 0) {
    const int o = blk * 64 + lane, lo_ = o / ts, i = o % ts;
    if (lo_ < 4) {
      const int nE = ((lo_ == 0) ? m.L : 32) * 32;
      if (i < m.R * nE) {
        const float* basis = Pold + m.off_basis[lo_] + i % nE;
#pragma unroll
        for (int bb = 0; bb < 4; ++bb) pbv[bb] = basis[bb * nE];
      }
    }
  }
  float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok4 && l == 3 && l3v) {
    // table element i0 = row * 32 + out, rows [R x 32 of dW_r | 32 of d root | bias]
    const int row = i0 >> 5, R = m.R;
    s4 = l3_vec_sum(m.l3_vec, ts_slots(nparts, stride, B), l3v, R, row < R * 32 ? row >> 5 : row < R * 32 + 32 ? R : R + 1,
                    row & 31, i0 & 31, pg);
  } else if (ok4) {
    const float* p = m.ts_part + (size_t)l * IGMC_TS_BLOCKS * ts + i0;
    const TsSlots sl = ts_slots(nparts, stride, B);
    const int nq = sl.nq;
    for (int q0 = pg; q0 < nq; q0 += 16 * 14) {
      float4 v[14];
#pragma unroll
      for (int u = 0; u < 14; ++u) v[u] = *(const float4*)(p + (size_t)ts_slot(sl, q0 + 16 * u) * ts);
#pragma unroll
      for (int u = 0; u < 14; ++u)
        if (q0 + 16 * u < nq) {
          s4.x += v[u].x; s4.y += v[u].y; s4.z += v[u].z; s4.w += v[u].w;
        }
    }
  }
  sred4[pg][o4] = s4;
  __syncthreads();
  if (wave == 0) {
    // lane -> output blk * 64 + lane: component (lane & 3) of column (lane >> 2), the 16 groups in index order
    const float* sr = (const float*)sred4;
    float tot = 0.f;
#pragma unroll
    for (int g16 = 0; g16 < 16; ++g16) tot += sr[(g16 * 16 + (lane >> 2)) * 4 + (lane & 3)];
    const int o = blk * 64 + lane;
    const int lo_ = o / ts, i = o % ts;
    const bool ok = lo_ < 4 && (lo_ > 0 || i < rows0 * 32);
    if (!ok) tot = 0.f;
    if (ok) m.ts_raw[o] = tot;
    if (Pold) {
      float pb[4];
#pragma unroll
      for (int bb = 0; bb < 4; ++bb) pb[bb] = tot * pbv[bb];      // (pbv is zero outside the dW_r blocks)
#pragma unroll
      for (int bb = 0; bb < 4; ++bb)
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) pb[bb] += __shfl_xor(pb[bb], d, 64);     // stays inside a 32-lane half
      if ((lane & 31) == 0 && lo_ < 4) *(float4*)(m.datt_part + (size_t)(o >> 5) * 4) = make_float4(pb[0], pb[1], pb[2], pb[3]);
    }
  }
}


// Both consumers of k_graph_step's outputs in ONE launch (they are independent of each other): the first `nlin`
// workgroups form d lin1 / d lin2 (batched product over the subgraphs), the others sum the relation-space tables.
// nstash = 4: the last four workgroups stash the weights-only quantities k_finalize_ts needs and the reduction also
// forms the d att partial products (0: the tables only, for k_finalize).
__global__ __launch_bounds__(IGMC_BLOCK) void k_tail_ts(BatchDev b, ModelDev m, const float* __restrict__ P,
                                                          float grad_scale, float mult, float drop_scale,
                                                          float* __restrict__ grad, int nlin, int nparts, int stride,
                                                          int B, int nstash, const int64_t* ctrl, int bump_seq, int l3v) {
  __builtin_amdgcn_s_setprio(3);      // (step chain: ahead of the extraction chain's waves wherever the two share a SIMD)
  igmc_kernarg_warm<sizeof(BatchDev) + sizeof(ModelDev) + 64>();
  const int nred = (int)gridDim.x - nlin - nstash;
  if (bump_seq && blockIdx.x == 0 && threadIdx.x == 0) m.gs_bar[1] += 1;      // (every workgroup of k_graph_step2 is done)
  if ((int)blockIdx.x < nlin)
    head_bwd_w_body(b, m, P, nullptr, 1, grad_scale, mult, drop_scale, grad, blockIdx.x & 7, blockIdx.x >> 3, B);
  else if ((int)blockIdx.x < nlin + nred)
    reduce_ts_body(m, nparts, stride, B, blockIdx.x - nlin, l3v, nstash ? P : nullptr);
  else
    fin_stash_body(m, P, blockIdx.x - nlin - nred, ctrl);
}

struct FinishArgs {
  int enabled;
  int use_flags;      // the step ran under edge dropout (the tick then also checks the arena's dropout stamp)
  BatchDev b;
  ModelDev m;
  float ARR;
  float* loss;
  double* total;
};

// (ctrl_advance, the end of a step: model.h -- shared with the scoring tail of scores.hip)
// ... after checking that the arena the step consumed held the batch of its cursor (and, under edge dropout, that batch's
// draws): every extraction stamps its arena with the `first` it resolved.  A mismatch means a batch extracted from a stale
// cursor or an arena overwritten too early; it sets sync_err instead of training on silently.
__device__ __forceinline__ void ctrl_check_and_advance(int64_t* ctrl, const BatchDev& b, int use_flags) {
  const int64_t gq = ctrl[IGMC_CTRL_GQ] & 1;
  const int64_t want = ctrl[gq ? IGMC_CTRL_FIRST_ODD : IGMC_CTRL_FIRST] + ctrl[IGMC_CTRL_GK] * ctrl[IGMC_CTRL_BATCH];
  const int64_t got = b.stamp[0];
  int bad = 0;
  if (got >= 0 && got != want) bad |= 2;
  if (use_flags && got >= 0 && b.stamp[1] >= 0 && (uint64_t)b.stamp[1] != igmc_ctrl_drop_key(ctrl, (int)want)) bad |= 4;
  if (bad) atomicOr((unsigned long long*)(ctrl + IGMC_CTRL_SYNC_ERR), (unsigned long long)bad);      // (k_tail_fin: other workgroups of the launch may raise their bit)
  ctrl_advance(ctrl);
}

// loss[0] = mean_g err^2 + ARR * sum_l reg_l   (reference train_eval.py:162-174); loss[1] = sum err^2
__device__ __forceinline__ void loss_body(const BatchDev& b, const ModelDev& m, float ARR, float* loss,
                                          double* total, float* smf) {
  const int B = b.totals[3];
  float s = 0.f;
  for (int g = threadIdx.x; g < B; g += IGMC_BLOCK) s += m.err[g] * m.err[g];
  s = igmc_block_sum_f(s, smf);
  if (threadIdx.x == 0) {
    const float reg = m.arr_part[0] + m.arr_part[1] + m.arr_part[2] + m.arr_part[3];
    const float l0 = s / (float)B + ARR * reg;
    loss[0] = l0;
    loss[1] = s;
    if (total) total[0] += (double)l0 * (double)B;     // epoch total of loss * num_graphs (ref :176)
  }
}

// The Adam scalars of a step under hipGraph replay live in HBM: in the control block, or (behind k_tail_ts / the stash role
// of the subgraph kernel's launch) in the stash
__device__ __forceinline__ AdamHyper adam_hyper_from_ctrl(const int64_t* ctrl) {
  const double* d = (const double*)ctrl;
  return {(float)d[IGMC_CTRL_STEP_SIZE], (float)d[IGMC_CTRL_INV_SQRT_BC2], (float)d[IGMC_CTRL_BETA1],
          (float)d[IGMC_CTRL_BETA2], (float)d[IGMC_CTRL_EPS], (float)d[IGMC_CTRL_WD]};
}
__device__ __forceinline__ AdamHyper adam_hyper_from_stash(const float* stash) {
  return {stash[IGMC_STASH_SCAL + 0], stash[IGMC_STASH_SCAL + 1], stash[IGMC_STASH_SCAL + 2],
          stash[IGMC_STASH_SCAL + 3], stash[IGMC_STASH_SCAL + 4], stash[IGMC_STASH_SCAL + 5]};
}

// One Adam update (torch.optim.Adam semantics) of an element whose gradient, parameter and moments are in registers already,
// with the two products of each moment rounded SEPARATELY (no fused multiply-add): the form of every walk over
// the lin parameters -- adam_range and the lin role of k_tail_fin, which visits the same elements in its own order.  Left to
// the compiler, a * b + c * d becomes two packed multiplies and an add in one caller and an fma in another (it depends on the
// unroll count): a last-bit difference in the moments between kernels that must leave the same bits.
__device__ __forceinline__ void adam_store_sep(float* p, float* m1, float* m2, int64_t i, float gi, float pv, float av, float vv,
                                               const AdamHyper& h) {
  const float step_size = h.step_size, inv_sqrt_bc2 = h.inv_sqrt_bc2, beta1 = h.beta1, beta2 = h.beta2, eps = h.eps, wd = h.wd;
  if (wd != 0.f) gi += wd * pv;
  float a, v;
  {
#pragma clang fp contract(off)
    a = beta1 * av + (1.f - beta1) * gi;
    v = beta2 * vv + (1.f - beta2) * gi * gi;
  }
  m1[i] = a;
  m2[i] = v;
  p[i] = pv - step_size * a / (sqrtf(v) * inv_sqrt_bc2 + eps);
}

// Adam on [lo, hi) by one workgroup: NB elements per thread and round, all 4 NB loads requested before the first use
// (the element-by-element loop pays one memory round trip per element: the stores of element k keep the compiler from
// requesting element k + 1 early)
template <int NB>
__device__ __forceinline__ void adam_range(float* p, const float* g, float* m1, float* m2, int64_t lo, int64_t hi,
                                           const AdamHyper& h) {
  for (int64_t i0 = lo + threadIdx.x; i0 < hi; i0 += (int64_t)NB * IGMC_BLOCK) {
    float gv[NB], pv[NB], av[NB], vv[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const int64_t i = i0 + (int64_t)k * IGMC_BLOCK;
      const int64_t ic = i < hi ? i : hi - 1;      // clamped, not predicated: the 4 NB loads go out back to back
      gv[k] = g[ic];
      pv[k] = p[ic];
      av[k] = m1[ic];
      vv[k] = m2[ic];
    }
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const int64_t i = i0 + (int64_t)k * IGMC_BLOCK;
      if (i < hi) adam_store_sep(p, m1, m2, i, gv[k], pv[k], av[k], vv[k], h);
    }
  }
}

// IGMC_FIN_NB workgroups per conv layer: turn the reduced partials into the flat gradient, add the
// adjacent-rating-regulariser gradient (reference train_eval.py:167-174), emit the ARR value, and (AdamTail) update
// the parameters -- every element in ONE pass (gradient, ARR term, store, Adam), elements interleaved over the
// layer's workgroups, the small per-layer quantities (Gram matrix of the bases) recomputed by each of them.
// ARR through the 4x4 Gram matrix of the bases:  W[r] = sum_b att[r,b] basis[b]  =>
//   D[r] = W[r+1]-W[r] = sum_b d[r,b] basis[b],  d[r] = att[r+1]-att[r]
//   reg = sum_r d[r]^T Gm d[r],  dreg/dW[r] = 2(D[r-1]-D[r]) = sum_b c[r,b] basis[b],  c[r] = 2(d[r-1]-d[r])
//   d att[r,b] += ARR * sum_b' c[r,b'] Gm[b',b];   d basis[b] += ARR * sum_b' (sum_r att[r,b] c[r,b']) basis[b']
// ts_mode: every layer's gradient arrives as a relation-space table [R*fin + fin + 1][32] (graphstep.hip; rows
// r*fin + c = d W[r][c], then d root[c], then d bias) instead of basis-space partials (fin = L for layer 0, else 32).
#define IGMC_FIN_NB 8
__global__ __launch_bounds__(IGMC_BLOCK) void k_finalize(ModelDev m, const float* P, float* __restrict__ grad,
                                                           float arr_coef, AdamTail at, int ts_mode) {
  igmc_kernarg_warm<sizeof(ModelDev) + sizeof(AdamTail) + 32>();
  if (at.skip && *at.skip) return;      // (uniform over the launch: written by the kernel in front of it)
  __shared__ float smf[8];
  __shared__ float sG[16], sM[16];
  __shared__ int s_lastl;
  __shared__ float sg10[4][10];
  __shared__ int s_last;
  if (at.enabled && at.ctrl) at.h = adam_hyper_from_ctrl(at.ctrl);      // hipGraph replay
  auto finish = [&](int64_t i, float g) { grad[i] = g; };
  if (blockIdx.x >= 4 * IGMC_FIN_NB) {   // extra workgroups: Adam on lin1 / lin2 (their gradients are final already)
    const int64_t n_lin = m.n_params - m.off_l1w;
    const int nb = gridDim.x - 4 * IGMC_FIN_NB;
    const int64_t chunk = (n_lin + nb - 1) / nb;
    const int64_t lo = m.off_l1w + (int64_t)(blockIdx.x - 4 * IGMC_FIN_NB) * chunk;
    const int64_t hi = (lo + chunk < m.n_params) ? lo + chunk : m.n_params;
    adam_range<8>(at.p, grad, at.m1, at.m2, lo, hi, at.h);
  } else {
    const int l = blockIdx.x / IGMC_FIN_NB, part = blockIdx.x % IGMC_FIN_NB, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int fin = (l == 0) ? m.L : 32;
    const int nE = fin * 32;                 // elements of one W[r] / basis[b]
    const int wgs = 32 * IGMC_KCAT + 32, na = m.R * 4, R = m.R;
    const float* basis = P + m.off_basis[l];
    const float* att = P + m.off_att[l];
    const int e0 = part * IGMC_BLOCK + tid, estep = IGMC_FIN_NB * IGMC_BLOCK;     // this thread's elements
    // ---- Gram matrix of the bases (10 unique entries), recomputed by every workgroup of the layer
    float gp[10];
#pragma unroll
    for (int q = 0; q < 10; ++q) gp[q] = 0.f;
    for (int e = tid; e < nE; e += IGMC_BLOCK) {
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
    __syncthreads();
    if (tid == 0) {
      const int ij[10][2] = {{0, 0}, {0, 1}, {0, 2}, {0, 3}, {1, 1}, {1, 2}, {1, 3}, {2, 2}, {2, 3}, {3, 3}};
      for (int q = 0; q < 10; ++q) {
        const float v = (sg10[0][q] + sg10[1][q]) + (sg10[2][q] + sg10[3][q]);
        sG[ij[q][0] * 4 + ij[q][1]] = v;
        sG[ij[q][1] * 4 + ij[q][0]] = v;
      }
    }
    // c[r][b] = 2 (d[r-1][b] - d[r][b]),  d[r] = att[r+1]-att[r]  (d[-1] = d[R-1] = 0)
    if (tid >= 64 && tid < 80) {           // M[b][b'] = sum_r att[r,b] c[r,b']
      const int bb = (tid - 64) >> 2, bp = tid & 3;
      float sacc = 0.f;
      for (int r = 0; r < R; ++r) {
        const float dm = (r > 0) ? att[r * 4 + bp] - att[(r - 1) * 4 + bp] : 0.f;
        const float dn = (r + 1 < R) ? att[(r + 1) * 4 + bp] - att[r * 4 + bp] : 0.f;
        sacc += att[r * 4 + bb] * 2.f * (dm - dn);
      }
      sM[tid - 64] = sacc;
    }
    __syncthreads();
    if (tid == 0 && part == 0) {           // reg = sum_r d[r]^T Gm d[r]
      float reg = 0.f;
      for (int r = 0; r + 1 < R; ++r) {
        float d[4];
        for (int q = 0; q < 4; ++q) d[q] = att[(r + 1) * 4 + q] - att[r * 4 + q];
        for (int p1 = 0; p1 < 4; ++p1)
          for (int p2 = 0; p2 < 4; ++p2) reg += d[p1] * sG[p1 * 4 + p2] * d[p2];
      }
      m.arr_part[l] = reg;
    }
    const bool table = (l == 0) || ts_mode;
    const float* raw = m.graw + (size_t)(l >= 1 ? l - 1 : 0) * wgs;                 // basis-space partial sums (l >= 1)
    const float* t0 = ts_mode ? m.ts_raw + (size_t)l * m.ts_stride : m.graw + 3 * wgs + 3 * na;
    // ---- d basis (+ ARR):  element e = (b, c, f)
    for (int e = e0; e < 4 * nE; e += estep) {
      const int bb = e / nE, cf = e % nE;
      float g;
      if (!table) {
        g = raw[(cf >> 5) * IGMC_KCAT + bb * 32 + (cf & 31)];
      } else {
        g = 0.f;
        for (int r = 0; r < R; ++r) g += att[r * 4 + bb] * t0[(size_t)r * nE + cf];
      }
      if (arr_coef != 0.f) {
        const float b0 = basis[cf], b1 = basis[nE + cf], b2 = basis[2 * nE + cf], b3 = basis[3 * nE + cf];
        g += arr_coef * (sM[bb * 4 + 0] * b0 + sM[bb * 4 + 1] * b1 + sM[bb * 4 + 2] * b2 + sM[bb * 4 + 3] * b3);
      }
      finish(m.off_basis[l] + e, g);
    }
    // ---- d root, d bias
    for (int e = e0; e < nE; e += estep)
      finish(m.off_root[l] + e, table ? t0[(size_t)R * nE + e] : raw[(e >> 5) * IGMC_KCAT + 128 + (e & 31)]);
    if (part == 0 && tid < 32)
      finish(m.off_bias[l] + tid, table ? t0[(size_t)(R * fin + fin) * 32 + tid] : raw[32 * IGMC_KCAT + tid]);
    // ---- d att (+ ARR): one wave per entry; table form: d att[r,b] = <dW[r], basis[b]>
    for (int rb = part * 4 + wave; rb < na; rb += IGMC_FIN_NB * 4) {
      const int r = rb >> 2, bb = rb & 3;
      float g;
      if (!table) {
        g = m.graw[3 * wgs + (size_t)(l - 1) * na + rb];
      } else {
        float sacc = 0.f;
        {   // nE <= 1024: at most 16 (table, basis) pairs per lane, all requested before the sum
          float tv[16], bv[16];
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            const int e = lane + 64 * k;
            tv[k] = (e < nE) ? t0[(size_t)r * nE + e] : 0.f;
            bv[k] = (e < nE) ? basis[bb * nE + e] : 0.f;
          }
#pragma unroll
          for (int k = 0; k < 16; ++k) sacc += tv[k] * bv[k];
        }
        g = igmc_wave_sum_f(sacc);
      }
      if (arr_coef != 0.f) {
        float sacc = 0.f;
        for (int bp = 0; bp < 4; ++bp) {
          const float dm = (r > 0) ? att[r * 4 + bp] - att[(r - 1) * 4 + bp] : 0.f;
          const float dn = (r + 1 < R) ? att[(r + 1) * 4 + bp] - att[r * 4 + bp] : 0.f;
          sacc += 2.f * (dm - dn) * sG[bp * 4 + bb];
        }
        g += arr_coef * sacc;
      }
      if (lane == 0) finish(m.off_att[l] + rb, g);
    }
    if (at.enabled) {
      // Adam on this layer's parameters (basis, root, bias, att are contiguous) by the LAST of the layer's
      // workgroups to finish: by then every workgroup of the layer has read the old parameters and stored its
      // share of the gradient (no spinning; at.done[1 + l] counts the arrivals)
      __syncthreads();
      if (tid == 0) {
        __threadfence();
        s_lastl = (atomicAdd(at.done + 1 + l, 1) == IGMC_FIN_NB - 1);
      }
      __syncthreads();
      if (s_lastl) {
        __threadfence();
        adam_range<12>(at.p, grad, at.m1, at.m2, m.off_basis[l], m.off_att[l] + na, at.h);
        if (tid == 0) at.done[1 + l] = 0;
      }
    }
  }   // conv-layer workgroups
  if (at.enabled) {
    // the last workgroup to arrive has every arr_part / err in sight: loss, epoch total, control-block tick
    __syncthreads();
    if (threadIdx.x == 0) {
      __threadfence();
      s_last = (atomicAdd(at.done, 1) == (int)gridDim.x - 1);
    }
    __syncthreads();
    if (s_last) {
      __threadfence();
      loss_body(at.b, m, at.ARR, at.loss, at.total, smf);
      if (threadIdx.x == 0) {
        *at.done = 0;
        if (at.ctrl) ctrl_check_and_advance(at.ctrl, at.b, at.use_flags);
      }
    }
  }
}

// Relation-space tables -> flat gradient (+ ARR) -> Adam, with NO hand-off between workgroups: k_tail_ts has already
// formed everything that needs parameters a thread does not own (Gram / ARR matrices, the ARR value, a copy of att,
// the <dW_r, basis_b> partials, the Adam scalars), so a thread reads the table rows of ITS column (c, f), produces the
// gradient of basis[0..3][c][f] and root[c][f], and updates exactly those parameters in the same pass; bias and att
// are taken by the layer's first workgroup.  Workgroups 4*IGMC_FTS_NB.. : Adam on slices of lin1 / lin2, the last one
// loss + epoch total + control-block tick (nobody else reads the control block in this launch).
// (k_finalize needs two in-kernel hand-offs for the same work -- layer-wide before Adam, grid-wide before the tick --
//  each an agent-scope fence pair + an atomic round trip.)
#define IGMC_FTS_NB 4
// (its basis-space mode takes up to IGMC_FBS_MAX_R relations: model.h)
// gradient g of parameter i -> flat gradient, Adam moments, parameter; returns the parameter's value after the step.
// store = false: the value only (a workgroup that needs a neighbour's updated parameter forms it itself; the owner stores)
__device__ __forceinline__ float fts_emit(float* __restrict__ grad, const AdamTail& at, int64_t i, float g, float pold,
                                          float m1old, float m2old, bool store = true) {
  if (store) grad[i] = g;
  if (!at.enabled) return pold;
  float gi = g;
  if (at.h.wd != 0.f) gi += at.h.wd * pold;
  const float a = at.h.beta1 * m1old + (1.f - at.h.beta1) * gi;
  const float v = at.h.beta2 * m2old + (1.f - at.h.beta2) * gi * gi;
  const float pnew = pold - at.h.step_size * a / (sqrtf(v) * at.h.inv_sqrt_bc2 + at.h.eps);
  if (store) {
    at.m1[i] = a;
    at.m2[i] = v;
    at.p[i] = pnew;
  }
  return pnew;
}

// ---- the roles of a conv layer's tail, shared by k_finalize_ts and the one-launch tail k_tail_fin: ONE body each, so that the
//      two kernels form every gradient, moment, parameter and image word with the same operations in the same order
// d att[r,b] (entry rb) from the sum g of its fin partial products: + ARR term, then the update; returns att[r,b] after the step
__device__ __forceinline__ float fts_att_entry(float* __restrict__ grad, const AdamTail& at, const float* st, int R, int rb,
                                               float g, float arr_coef, int64_t i, float pold, float m1o, float m2o, bool store) {
  const int r = rb >> 2, bb = rb & 3;
  if (arr_coef != 0.f) {
    float sacc = 0.f;
    for (int bp = 0; bp < 4; ++bp) {
      const float a0 = st[IGMC_STASH_ATT + r * 4 + bp];
      const float dm = (r > 0) ? a0 - st[IGMC_STASH_ATT + (r - 1) * 4 + bp] : 0.f;
      const float dn = (r + 1 < R) ? st[IGMC_STASH_ATT + (r + 1) * 4 + bp] - a0 : 0.f;
      sacc += 2.f * (dm - dn) * st[IGMC_STASH_G + bp * 4 + bb];
    }
    g += arr_coef * sacc;
  }
  return fts_emit(grad, at, i, g, pold, m1o, m2o, store);
}
// column (c, f) of a layer: d basis_b[c][f] += sum_{r < min(R, 8)} att[r,b] dW_r[c][f] from the column's table values
__device__ __forceinline__ void fts_col_table8(float (&g)[5], const float* st, const float (&tv)[8], int R) {
#pragma unroll
  for (int r = 0; r < 8; ++r)
    if (r < R) {
#pragma unroll
      for (int bb = 0; bb < 4; ++bb) g[bb] += st[IGMC_STASH_ATT + r * 4 + bb] * tv[r];
    }
}
// ... + ARR term, then the update of basis_0..3[c][f] and root[c][f]; pn: their values after the step
__device__ __forceinline__ void fts_col_emit(float* __restrict__ grad, const AdamTail& at, const float* st, float arr_coef,
                                             const int64_t (&idx)[5], float (&g)[5], const float (&pv)[5], const float (&m1v)[5],
                                             const float (&m2v)[5], float (&pn)[5]) {
  if (arr_coef != 0.f) {
    // (the roundings of  g += arr_coef (M0 p0 + M1 p1 + M2 p2 + M3 p3)  are spelled out: left to the compiler, the sum came out
    //  as an fma chain in one kernel and as four products and three adds in another -- last bits of every basis gradient.  This
    //  is the chain k_finalize_ts has always computed: M1 p1 rounded, the other three products fused)
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
      float t = fmaf(st[IGMC_STASH_M + bb * 4 + 0], pv[0], st[IGMC_STASH_M + bb * 4 + 1] * pv[1]);
      t = fmaf(st[IGMC_STASH_M + bb * 4 + 2], pv[2], t);
      t = fmaf(st[IGMC_STASH_M + bb * 4 + 3], pv[3], t);
      g[bb] = fmaf(arr_coef, t, g[bb]);
    }
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) pn[q] = fts_emit(grad, at, idx[q], g[q], pv[q], m1v[q], m2v[q]);
}
// weight-image words of column (c, f) after the step, relations r0, r0 + rstep, .. (R = the root): layer 0 -> its rows of the
// layer-0 table [W_0[r * L + c] | root_0[c] | bias_0] (rows past R L + L stay zero: first compose); layers 1..3 -> forward
// image element (k = c, n = f) and transposed image element (k = f, n = c): relation r -> block r % G2_NR of group r / G2_NR,
// root -> block G2_NR of group 0 (blocks of relations the model does not have stay zero: first compose)
__device__ __forceinline__ void fts_image_col(const ModelDev& m, int ng, int l, int R, int fin, int c, int f, const float* s_attn,
                                              const float (&pn)[5], int r0, int rstep) {
  if (l == 0) {
    float* t0w = m.g2_w + g2_t0_off(ng);
    for (int r = r0; r <= R; r += rstep)
      t0w[(r * fin + c) * 32 + f] = (r == R) ? pn[4]
                                  : g2_wsum(s_attn[r * 4], s_attn[r * 4 + 1], s_attn[r * 4 + 2], s_attn[r * 4 + 3], pn[0], pn[1], pn[2], pn[3]);
  } else {
#pragma unroll 3
    for (int r = r0; r <= R; r += rstep) {
      const float v = (r == R) ? pn[4]
                    : g2_wsum(s_attn[r * 4], s_attn[r * 4 + 1], s_attn[r * 4 + 2], s_attn[r * 4 + 3], pn[0], pn[1], pn[2], pn[3]);
      const int grp = (r == R) ? 0 : r / G2_NR, blk = (r == R) ? G2_NR : r % G2_NR;
      uint16_t* imf = (uint16_t*)(m.g2_w + g2_img_off(ng, l, 0, grp));
      uint16_t* imt = (uint16_t*)(m.g2_w + g2_img_off(ng, l, 1, grp));
      uint32_t h, mi, lo;
      g2_split2(v, 0.f, h, mi, lo);
      const uint32_t t3[3] = {h, mi, lo};
#pragma unroll
      for (int t = 0; t < G2_NT; ++t) {
        imf[g2_img_index(t, blk, c, f)] = (uint16_t)t3[t];
        imt[g2_img_index(t, blk, f, c)] = (uint16_t)t3[t];
      }
    }
  }
}
// d bias[f] of a layer (bq: gradient, parameter, moments); layer 0 with images: the bias row of the layer-0 table
__device__ __forceinline__ void fts_bias(const ModelDev& m, float* __restrict__ grad, const AdamTail& at, int ng, int l, int R,
                                         int fin, int f, const float (&bq)[4], bool emit) {
  const int64_t i = m.off_bias[l] + f;
  const float bnew = fts_emit(grad, at, i, bq[0], bq[1], bq[2], bq[3]);
  if (emit && l == 0) m.g2_w[g2_t0_off(ng) + (R * fin + fin) * 32 + f] = bnew;
}

// img != 0 (with Adam): the weight images of the UPDATED parameters are written too -- what k_g2_compose would form from
// them for the next step's subgraph / dense-layer kernels (g2_image.h): a thread holds the new basis_0..3[c][f] and
// root[c][f] of its column; the layer's new att (20 values) is formed by EVERY workgroup of the layer (the owner stores it),
// so W_r[c][f] = sum_b att[r,b] basis_b[c][f] needs nothing from another workgroup.  The next step then starts with the
// subgraph kernel: one launch and one round trip to the weights less per step.
__global__ __launch_bounds__(IGMC_BLOCK) void k_finalize_ts(ModelDev m, const float* P, float* __restrict__ grad,
                                                              float arr_coef, AdamTail at, int nlin, int bs, int img) {
  __builtin_amdgcn_s_setprio(3);      // (step chain: ahead of the extraction chain's waves wherever the two share a SIMD)
  igmc_kernarg_warm<sizeof(ModelDev) + sizeof(AdamTail) + 48>();
  // bs != 0: the per-layer path's sources -- conv layers 1..3 in BASIS space (graw: d basis_b, d root, d bias straight
  // from the weight-gradient kernel, d att from the layer kernels' partials), layer 0 as its relation-space table in graw;
  // the stash comes from k_reduce_partials.  bs == 0: the relation-space tables of the subgraph kernels (ts_raw).
  if (at.skip && *at.skip) return;      // (uniform over the launch: written by the kernel in front of it)
  __shared__ float smf[8];
  const int tid = threadIdx.x;
  const float* stash = m.fin_stash;
  if (at.enabled && at.ctrl) at.h = adam_hyper_from_stash(stash);      // hipGraph replay: stashed by k_tail_ts
  if ((int)blockIdx.x < 4 * IGMC_FTS_NB) {
    const int l = blockIdx.x / IGMC_FTS_NB, part = blockIdx.x % IGMC_FTS_NB;
    const int fin = (l == 0) ? m.L : 32, nE = fin * 32, R = m.R, na = R * 4;
    const float* stg = stash + l * IGMC_STASH_LAYER;
    __shared__ float s_st[IGMC_STASH_LAYER];      // the layer's stash: requested first, read from LDS after the barrier below
    float stq[(IGMC_STASH_LAYER + IGMC_BLOCK - 1) / IGMC_BLOCK];
#pragma unroll
    for (int u = 0; u < (IGMC_STASH_LAYER + IGMC_BLOCK - 1) / IGMC_BLOCK; ++u) {
      const int i = tid + u * IGMC_BLOCK;
      stq[u] = stg[i < IGMC_STASH_LAYER ? i : IGMC_STASH_LAYER - 1];
    }
    const float* st = s_st;
    const int wgs = 32 * IGMC_KCAT + 32;
    const bool table = !bs || l == 0;
    const float* t0 = bs ? m.graw + 3 * wgs + 3 * na : m.ts_raw + (size_t)l * m.ts_stride;
    const float* raw = m.graw + (size_t)(l >= 1 ? l - 1 : 0) * wgs;
    // basis-space mode, layer 0: d att[r,b] = <dW_r, basis_b> needs every basis element of the layer BEFORE its owner
    // (a thread of this very workgroup: nE <= 256) updates it -> formed first, then a barrier
    __shared__ float s_gatt0[512];
    if (bs && l == 0) {
      if (part == 0) {
        // a thread owns element e = tid (strided by the workgroup for fin > 8) of every product: the R table values and
        // the 4 basis values of e requested together, the na = 4 R wave sums taken side by side (a round trip and six
        // crossbar steps in all; entry after entry it was 5 dependent rounds of both), waves combined in fixed order
        __shared__ float s_gpart[IGMC_BLOCK / 64][32];
        const int lane = tid & 63, wave = tid >> 6;
        if (R <= 8) {
          float acc[32];
#pragma unroll
          for (int i = 0; i < 32; ++i) acc[i] = 0.f;
          for (int e0 = 0; e0 < nE; e0 += IGMC_BLOCK) {
            const int e = e0 + tid, ec = e < nE ? e : nE - 1;
            float tv[8], bq[4];
#pragma unroll
            for (int r = 0; r < 8; ++r) tv[r] = t0[(size_t)(r < R ? r : R - 1) * nE + ec];
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) bq[bb] = P[m.off_basis[0] + (int64_t)bb * nE + ec];
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
              for (int bb = 0; bb < 4; ++bb)
                if (r < R && e < nE) acc[r * 4 + bb] += tv[r] * bq[bb];
          }
#pragma unroll
          for (int d = 32; d >= 1; d >>= 1) {
            float t[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) t[i] = __shfl_xor(acc[i], d, 64);
#pragma unroll
            for (int i = 0; i < 32; ++i) acc[i] += t[i];
          }
          if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 32; ++i) s_gpart[wave][i] = acc[i];
          }
          __syncthreads();
          if (tid < na) {
            float sacc = 0.f;
#pragma unroll
            for (int w = 0; w < IGMC_BLOCK / 64; ++w) sacc += s_gpart[w][tid];
            s_gatt0[tid] = sacc;
          }
        } else {                  // more than 8 relations: one wave per entry, lanes over the nE elements
          for (int rb = wave; rb < na; rb += IGMC_BLOCK / 64) {
            const int r = rb >> 2, bb = rb & 3;
            float sacc = 0.f;
            for (int e = lane; e < nE; e += 64) sacc += t0[(size_t)r * nE + e] * P[m.off_basis[0] + (int64_t)bb * nE + e];
            sacc = igmc_wave_sum_f(sacc);
            if (lane == 0) s_gatt0[rb] = sacc;
          }
        }
      }
      __syncthreads();
    }
    __shared__ float s_attn[64];                // the layer's att after the step (img)
    float pn[5] = {0.f, 0.f, 0.f, 0.f, 0.f};    // this thread's basis_0..3[c][f], root[c][f] after the step (img)
    int e_img = -1;
    const bool emit = img && at.enabled && m.g2_w && R <= G2_NR * G2_NG_MAX && fin <= 32;
    const int ng = g2_groups(R, m.L);
    // ---- every load of the workgroup is requested here, before the first store: the thread's column of the main pass
    // (nE <= 1024: ONE element a thread), the bias role's four values, the att role's first entry (its fin partial sums or
    // the basis-space gradient, the parameter and its moments).  The stores of the main pass used to come first: the two
    // roles then paid a second round trip, and the weight images wait for the att role.
    const int e = part * IGMC_BLOCK + tid;
    const bool has = e < nE;
    int64_t idx[5];
    float pv[5], m1v[5], m2v[5], g[5], tv[8];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      idx[q] = (q < 4) ? m.off_basis[l] + (int64_t)q * nE + (has ? e : 0) : m.off_root[l] + (has ? e : 0);
      pv[q] = has ? P[idx[q]] : 0.f;
      m1v[q] = (has && at.enabled) ? at.m1[idx[q]] : 0.f;
      m2v[q] = (has && at.enabled) ? at.m2[idx[q]] : 0.f;
      g[q] = 0.f;
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) tv[r] = 0.f;
    if (has) {
      if (table) {
#pragma unroll
        for (int r = 0; r < 8; ++r) tv[r] = (r < R) ? t0[(size_t)r * nE + e] : 0.f;
        g[4] = t0[(size_t)R * nE + e];
      } else {
#pragma unroll
        for (int bb = 0; bb < 4; ++bb) g[bb] = raw[(e >> 5) * IGMC_KCAT + bb * 32 + (e & 31)];
        g[4] = raw[(e >> 5) * IGMC_KCAT + 128 + (e & 31)];
      }
    }
    const bool roles = part == 0 || emit;
    const bool bias_role = roles && tid < 32 && part == 0;
    const bool att_role = roles && !bias_role && tid >= 64 && tid - 64 < na;
    float bq[4] = {0.f, 0.f, 0.f, 0.f};          // bias role: gradient source, parameter, moments
    if (bias_role) {
      const int64_t i = m.off_bias[l] + tid;
      bq[0] = table ? t0[(size_t)(R * fin + fin) * 32 + tid] : raw[32 * IGMC_KCAT + tid];
      bq[1] = P[i];
      bq[2] = at.enabled ? at.m1[i] : 0.f;
      bq[3] = at.enabled ? at.m2[i] : 0.f;
    }
    float dpre[32], am1 = 0.f, am2 = 0.f, ag = 0.f;      // att role, entry tid - 64
#pragma unroll
    for (int k = 0; k < 32; ++k) dpre[k] = 0.f;
    if (att_role) {
      const int rb = tid - 64, r = rb >> 2, bb = rb & 3;
      const int64_t i = m.off_att[l] + rb;
      if (at.enabled && !emit) {
        am1 = at.m1[i];
        am2 = at.m2[i];
      }
      if (bs) {
        if (l > 0) ag = m.graw[3 * wgs + (size_t)(l - 1) * na + rb];
      } else {
        const float* dp = m.datt_part + ((size_t)l * m.ts_stride + (size_t)r * nE) / 32 * 4 + bb;
#pragma unroll
        for (int k = 0; k < 32; ++k) dpre[k] = (k < fin) ? dp[(size_t)k * 4] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < (IGMC_STASH_LAYER + IGMC_BLOCK - 1) / IGMC_BLOCK; ++u) {
      const int i = tid + u * IGMC_BLOCK;
      if (i < IGMC_STASH_LAYER) s_st[i] = stq[u];
    }
    __syncthreads();
    // (the bias / att roles FIRST: the weight images wait for the layer's new att, formed by wave 1 -- behind its share of the
    //  main pass it kept every other wave of the workgroup waiting at the barrier below for 2.6 k cycles)
    if (roles) {
      if (bias_role) {                             // d bias (layer-0 table: bias row)
        fts_bias(m, grad, at, ng, l, R, fin, tid, bq, emit);
      } else if (tid >= 64) {                      // d att[r,b] = <dW_r, basis_b> (+ ARR): fin partials, fixed order
       for (int rb = tid - 64; rb < na; rb += IGMC_BLOCK - 64) {      // (one entry a thread up to 48 relations)
        const int r = rb >> 2, bb = rb & 3;
        const bool first = rb == tid - 64;         // (its operands were requested above)
        const int64_t i = m.off_att[l] + rb;
        const float pold = st[IGMC_STASH_ATT + rb];
        // (img: the moments before the step come from the stash -- the owner workgroup updates them in place meanwhile)
        const float m1o = !at.enabled ? 0.f : emit ? st[IGMC_STASH_ATTM1 + rb] : first ? am1 : at.m1[i];
        const float m2o = !at.enabled ? 0.f : emit ? st[IGMC_STASH_ATTM2 + rb] : first ? am2 : at.m2[i];
        float g = 0.f;
        if (bs) {
          g = (l == 0) ? s_gatt0[rb] : first ? ag : m.graw[3 * wgs + (size_t)(l - 1) * na + rb];
        } else if (first && fin <= 32) {
#pragma unroll
          for (int k = 0; k < 32; ++k) g += dpre[k];
        } else {
          const float* dp = m.datt_part + ((size_t)l * m.ts_stride + (size_t)r * nE) / 32 * 4 + bb;
          for (int k0 = 0; k0 < fin; k0 += 32) {
            float v[32];
#pragma unroll
            for (int k = 0; k < 32; ++k) v[k] = (k0 + k < fin) ? dp[(size_t)(k0 + k) * 4] : 0.f;
#pragma unroll
            for (int k = 0; k < 32; ++k) g += v[k];
          }
        }
        const float anew = fts_att_entry(grad, at, st, R, rb, g, arr_coef, i, pold, m1o, m2o, part == 0);
        if (emit) s_attn[rb] = anew;
       }
      }
    }
    if (has) {       // one round for fin <= 32
      if (table) {
        fts_col_table8(g, st, tv, R);
        for (int r = 8; r < R; ++r) {
          const float tvr = t0[(size_t)r * nE + e];
#pragma unroll
          for (int bb = 0; bb < 4; ++bb) g[bb] += st[IGMC_STASH_ATT + r * 4 + bb] * tvr;
        }
      }
      fts_col_emit(grad, at, st, arr_coef, idx, g, pv, m1v, m2v, pn);
      e_img = e;
    }
    if (emit) {
      __syncthreads();
      if (e_img >= 0) fts_image_col(m, ng, l, R, fin, e_img >> 5, e_img & 31, s_attn, pn, 0, 1);
    }
  } else if ((int)blockIdx.x < 4 * IGMC_FTS_NB + nlin) {      // Adam on lin1 / lin2 (their gradients are final already)
    const int64_t n_lin = m.n_params - m.off_l1w;
    const int64_t chunk = (n_lin + nlin - 1) / nlin;
    const int64_t lo = m.off_l1w + (int64_t)(blockIdx.x - 4 * IGMC_FTS_NB) * chunk;
    const int64_t hi = (lo + chunk < m.n_params) ? lo + chunk : m.n_params;
    adam_range<8>(at.p, grad, at.m1, at.m2, lo, hi, at.h);
  } else {                                                     // loss, epoch total, control-block tick
    loss_body(at.b, m, at.ARR, at.loss, at.total, smf);
    if (tid == 0 && at.ctrl) ctrl_check_and_advance(at.ctrl, at.b, at.use_flags);
  }
}

// ===================================================================== the tail of the subgraph kernel in ONE launch
// k_tail_ts -> k_finalize_ts without the launch between them.  k_tail_ts does ~1 us of work; what it is there for is the
// grid-wide fence between "every table is summed" and "every parameter is updated".  Here the only table data that crosses a
// workgroup are REDUCED rows, 64 floats a producer, as tagged words:
//   * conv layers -- the rows (layer l, input row c) consumes (dW_r[c] for r < R, d root[c]) are 8 (R + 1) float4 columns,
//     taken in sets of 16 (R = 5: dW_0|dW_1, dW_2|dW_3, dW_4|d root).  A workgroup sums ONE set from the nq partial tables
//     (tf_sum_set: 14 sixteen-byte loads a thread) in reduce_ts_body's order -- per float4 column 16 partial groups that take
//     the slots pg, pg + 16, .. one after the other, then the groups in index order through LDS.  The "main" workgroup of
//     (l, c) takes set 0, a "row producer" each of the other sets, and one "bias producer" a layer the bias row.  A producer
//     publishes its <= 64 sums as {f32, tag} words (device scope: the readers sit on any XCD); the main polls those of its
//     row (every main of the layer also the bias words, so that a layer whose words never arrive is left untouched as a
//     whole; c == 0 consumes them) and runs k_finalize_ts's column body on its 32 columns (c, f);
//   * d att[r,b] = <dW_r, basis_b> needs every input row of the layer: the workgroup that reduced dW_r[c] -- the main for the
//     relations of set 0, a row producer for the others -- forms the row's share (tf_datt_pub: the very values k_tail_ts
//     leaves in datt_part) and publishes it the same way; every main of the layer polls the fin x 4 R words, adds them over c
//     in index order and forms the layer's new att from the stashed moments, as k_finalize_ts does for its weight images;
//     main c == 0 stores att;
//   * lin1 / lin2 -- the workgroups that form the gradient (head_bwd_w_body) update exactly the elements they formed;
//   * the last workgroup -- loss, epoch total, control-block tick, launch sequence number.
// Grid: [row producers: main-major, set-minor | 4 bias producers | workgroups that return at once, up to a multiple of 32 |
// mains of layers 1, 2, 3: 32 each | layer 0's L mains | nlin lin workgroups | tick] -- 200 + 4 + 20 + 100 + 32 + 1 = 357
// workgroups of 256 threads at R = 5, L = 4: all resident together.  No deadlock: a producer waits for nothing; a main waits
// for producers, which have lower indices and so were dispatched before it, and for the mains of its own layer, 32 consecutive
// indices (the CPU emulator runs aligned groups of 32 consecutive workgroups together, one group after the other: every
// producer group is complete before a main runs, and the mains of a layer run together).
// The weights-only stash (fin_stash_body) reads parameters this launch updates in place: it rides in the launch in front
// (k_graph_step2's appended workgroups) and also leaves the TAG of the words: that launch's sequence number, a word nobody
// writes here.  Nothing but the words is waited for (no fence, no release / acquire: value and tag are one store), the wait
// is bounded by the wall clock, and a workgroup that gives up updates nothing and reports it (gs_err, sync_err bit 8).
// Every sum keeps the order the two-launch tail gives it: the step's results are the same bits.
#define IGMC_TF_ROWS 384                  // LDS floats of the reduced rows: up to 6 sets of 16 columns (R <= 8: 80 columns)
#define IGMC_TF_O_ROWS 1024               // (in front: one set of [16 partial groups][16 float4 columns])
#define IGMC_TF_O_ST (IGMC_TF_O_ROWS + IGMC_TF_ROWS)
#define IGMC_TF_O_DATT (IGMC_TF_O_ST + IGMC_STASH_LAYER)
#define IGMC_TF_O_ATTN (IGMC_TF_O_DATT + 32 * IGMC_FOLD_NA)
#define IGMC_TF_O_PN (IGMC_TF_O_ATTN + 64)
#define IGMC_TF_O_SMF (IGMC_TF_O_PN + 5 * 32)
#define IGMC_TF_WORDS (IGMC_TF_O_SMF + 16)
// words a thread of a main polls: its row's (<= IGMC_FOLD_PSETS x 64), the layer's d att (<= 32 x IGMC_FOLD_NA), the bias row's
#define IGMC_TF_POLL ((IGMC_FOLD_PSETS * 64 + 32 * IGMC_FOLD_NA + 32 + IGMC_BLOCK - 1) / IGMC_BLOCK)
#define IGMC_TF_TIMEOUT_TICKS 20000000ll  // 200 ms of the 100 MHz wall clock
#define IGMC_SYNC_ERR_FOLD 8              // sync_err bit: a hand-off of k_tail_fin timed out

// Phase stamps (a variant library built with -DIGMC_FIN_CLOCKS; tools/exp_fin_clocks.py): shader-clock values of the first main
// workgroup (layer 1, row 0: slots 0..), the first lin workgroup (16..), the loss / tick workgroup (32..), the first row
// producer (layer 1, row 0, set 1: 40..) and layer 1's bias producer (48..).  The product build carries none of it.
#if defined(IGMC_FIN_CLOCKS) && !defined(IGMC_HIPEMU)
__device__ unsigned long long g_fin_clk[64];
extern "C" int igmc_debug_fin_clocks(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fin_clk), sizeof(g_fin_clk)) != hipSuccess;
}
#define TF_STAMP(on, k) do { if ((on) && threadIdx.x == 0) g_fin_clk[k] = __builtin_readcyclecounter(); } while (0)
#else
#define TF_STAMP(on, k) do { } while (0)
#endif

// One set of <= 16 float4 columns of (layer, input row c) summed over the nq partial tables, the ONE body of the mains and the
// producers of k_tail_fin: column k = (row j = k >> 3, float4 k & 7) for k0 <= k < k1 (j < R: dW_j[c], j == R: d root[c],
// j == R + 1: the bias row); thread (o4, pg) sums the slots pg, pg + 16, .. of column k0 + o4 in order (14 sixteen-byte loads
// in flight, all requested before the first add), wave 0 adds the 16 groups in index order through LDS (sred4: 1024 floats).
// Returns, in wave 0, component (lane & 3) of column k0 + (lane >> 2): element lane of the set's 64 floats.  One barrier;
// sred4 must not be in use by the workgroup.  vec != NULL (layer 3 under StepPlan::l3_vec = mv): the same sums from the centre
// vectors (l3_vec_sum) -- same threads, same slots in the same order, same groups; only the addend is formed here.
__device__ __forceinline__ float tf_sum_set(const float* __restrict__ pl, const TsSlots& sl, int ts, int R, int fin, int c,
                                            int k0, int k1, float4* sred4, const float* __restrict__ vec = nullptr, int mv = 0) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int o4 = lane & 15, pg = wave * 4 + (lane >> 4);
  const int k = k0 + o4, kc = k < k1 ? k : k1 - 1, j = kc >> 3;
  const int row = j < R ? j * fin + c : j == R ? R * fin + c : R * fin + fin;
  const int i0 = row * 32 + 4 * (kc & 7);
  float4 s4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const int nq = sl.nq;
  if (vec) s4 = l3_vec_sum(vec, sl, mv, R, j, c, 4 * (kc & 7), pg);
  else for (int q0 = pg; q0 < nq; q0 += 16 * 14) {
    float4 v[14];
#pragma unroll
    for (int u = 0; u < 14; ++u) v[u] = *(const float4*)(pl + (size_t)ts_slot(sl, q0 + 16 * u) * ts + i0);
#pragma unroll
    for (int u = 0; u < 14; ++u)
      if (q0 + 16 * u < nq) {
        s4.x += v[u].x; s4.y += v[u].y; s4.z += v[u].z; s4.w += v[u].w;
      }
  }
  sred4[pg * 16 + o4] = s4;
  __syncthreads();
  float tot = 0.f;
  if (wave == 0) {
    const float* sr = (const float*)sred4;
#pragma unroll
    for (int g16 = 0; g16 < 16; ++g16) tot += sr[(g16 * 16 + (lane >> 2)) * 4 + (lane & 3)];
  }
  return tot;
}

// A row's share of d att[r,b] = <dW_r, basis_b> for the two relations r = r2 + h of a set (wave 0 only; half h = lane >> 5,
// feature f = lane & 31; tot: dW_r[c][f], the lane's own element of the set; pvb: basis_b[c][f]): the butterfly of
// reduce_ts_body inside a 32-lane half, published by the half's first lane as the launch's words
__device__ __forceinline__ void tf_datt_pub(float tot, int r, int R, const float (&pvb)[4], unsigned long long* wrow, uint32_t tag,
                                            bool mute) {
  const int f = threadIdx.x & 31;
  if (r >= R) tot = 0.f;
  float pb[4];
#pragma unroll
  for (int bb = 0; bb < 4; ++bb) pb[bb] = tot * pvb[bb];
#pragma unroll
  for (int bb = 0; bb < 4; ++bb)
#pragma unroll
    for (int d = 16; d >= 1; d >>= 1) pb[bb] += __shfl_xor(pb[bb], d, 64);     // stays inside a 32-lane half
  if (mute) return;      // (emulator's timeout test)
  if (f == 0 && r < R) {
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) g2_pub_f32_agent(wrow + r * 4 + bb, pb[bb], tag);
  }
}

__global__ __launch_bounds__(IGMC_BLOCK) void k_tail_fin(BatchDev b, ModelDev m, const float* P, float grad_scale, float mult,
                                                           float drop_scale, float* grad, float arr_coef, AdamTail at, int nlin,
                                                           int nparts, int stride, int B, int bump_seq, int mute, int l3v) {
  __builtin_amdgcn_s_setprio(3);      // (step chain: ahead of the extraction chain's waves wherever the two share a SIMD)
  igmc_kernarg_warm<sizeof(BatchDev) + sizeof(ModelDev) + sizeof(AdamTail) + 64>();
  IGMC_DYN_SMEM(smem);
  float* S = (float*)smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* stash = m.fin_stash;
  const int R = m.R, L = m.L, na = R * 4;
  const int nconv = 96 + L;                 // mains -- layers 1..3: 32 workgroups each, then layer 0's L
  const int ncol_a = 8 * (R + 1), nsets = (ncol_a + 15) >> 4;
  const int nprod_r = (nsets - 1) * nconv, nprod = (nprod_r + 4 + 31) & ~31;      // row producers; + bias producers, padded
  const int blk = blockIdx.x;
#ifdef IGMC_HIPEMU
  // (the timeout test: publishers of layer mute & 255 stay silent -- all of them, or (mute >> 8) 1: its row producers, 2: its bias producer)
  const int mute_layer = mute < 0 ? -1 : (mute & 255), mute_role = mute < 0 ? 0 : (mute >> 8);
#else
  const int mute_layer = -1, mute_role = 0;
#endif
  TF_STAMP(blk == nprod, 0);
  TF_STAMP(blk == nprod + nconv, 16);
  TF_STAMP(blk == nprod + nconv + nlin, 32);
  TF_STAMP(blk == 0, 40);
  TF_STAMP(blk == nprod_r + 1, 48);
  if (blk < nprod) {
    // ---- producers: one set of one row summed and published; they wait for nothing
    if (blk >= nprod_r + 4) return;      // (padding: the mains of a layer stay an aligned run of 32 workgroups)
    const bool brow = blk >= nprod_r;
    const int mi = brow ? 0 : blk / (nsets - 1), set = brow ? 0 : 1 + blk % (nsets - 1);
    const int l = brow ? blk - nprod_r : mi < 96 ? 1 + (mi >> 5) : 0, c = brow ? 0 : mi < 96 ? (mi & 31) : mi - 96;
    const int fin = (l == 0) ? L : 32, nE = fin * 32, ts = m.ts_stride;
    const uint32_t tag = __float_as_uint(stash[IGMC_STASH_SCAL + IGMC_STASH_SEQ]) * 2u + 1u;      // (never 0)
    // the basis values of the d att products are requested with the table loads.  The main (l, c) updates these parameters
    // only behind its poll of the layer's words, this workgroup's among them: the read is ordered before that write by data
    // dependence
    float pvb[4] = {0.f, 0.f, 0.f, 0.f};
    if (wave == 0 && !brow) {
#pragma unroll
      for (int bb = 0; bb < 4; ++bb) pvb[bb] = P[m.off_basis[l] + (int64_t)bb * nE + c * 32 + (lane & 31)];
    }
    TF_STAMP(blk == 0, 41);
    TF_STAMP(blk == nprod_r + 1, 49);
    const TsSlots sl = ts_slots(nparts, stride, B);
    const int k0 = brow ? ncol_a : 16 * set, k1 = brow ? ncol_a + 8 : (k0 + 16 < ncol_a ? k0 + 16 : ncol_a);
    const float tot = tf_sum_set(m.ts_part + (size_t)l * IGMC_TS_BLOCKS * ts, sl, ts, R, fin, c, k0, k1, (float4*)S,
                                 (l == 3 && l3v) ? m.l3_vec : nullptr, l3v);
    TF_STAMP(blk == 0, 42);
    TF_STAMP(blk == nprod_r + 1, 50);
    if (wave == 0) {
      const bool silent = l == mute_layer && mute_role != (brow ? 1 : 2);
      unsigned long long* w = brow ? m.fold_w + IGMC_FOLD_O_BIAS + l * 32
                                   : m.fold_w + IGMC_FOLD_O_ROWS + (size_t)((l * 32 + c) * IGMC_FOLD_PSETS + set - 1) * 64;
      if (!silent && k0 + (lane >> 2) < k1) g2_pub_f32_agent(w + lane, tot, tag);
      if (!brow) tf_datt_pub(tot, 2 * set + (lane >> 5), R, pvb, m.fold_w + (size_t)(l * 32 + c) * IGMC_FOLD_NA, tag, silent);
    }
    TF_STAMP(blk == 0, 43);
    TF_STAMP(blk == nprod_r + 1, 51);
    return;
  }
  if (at.ctrl) at.h = adam_hyper_from_stash(stash);      // hipGraph replay: stashed in the launch in front
  const int mb = blk - nprod;
  if (mb < nconv) {
    const int l = mb < 96 ? 1 + (mb >> 5) : 0, c = mb < 96 ? (mb & 31) : mb - 96;
    const int fin = (l == 0) ? L : 32, nE = fin * 32, ts = m.ts_stride;
    const uint32_t tag = __float_as_uint(stash[IGMC_STASH_SCAL + IGMC_STASH_SEQ]) * 2u + 1u;      // (never 0)
    float4* sred4 = (float4*)S;                       // [16 partial groups][16 columns]
    float* rows = S + IGMC_TF_O_ROWS;                 // [R dW_r[c] | d root[c] | d bias][32]
    float* s_st = S + IGMC_TF_O_ST;                   // the layer's stash
    float* s_datt = S + IGMC_TF_O_DATT;               // [fin][IGMC_FOLD_NA] the layer's d att partial products
    float* s_attn = S + IGMC_TF_O_ATTN;               // the layer's att after the step
    float* s_pn = S + IGMC_TF_O_PN;                   // [5][32] the columns' basis_0..3 / root after the step
    int* s_flag = (int*)(S + IGMC_TF_O_SMF + 8);      // a poll of the workgroup ran out
    const int ng = g2_groups(R, L);
    // ---- every load that does not depend on another workgroup is requested here, in front of the partial tables: the layer's
    // stash, the column threads' (tid < 32: f = tid) parameters and moments, wave 0's basis values for the d att products
    // (both 32-lane halves: f = lane & 31), the bias role's (c == 0: tid 32..63)
    float stq[(IGMC_STASH_LAYER + IGMC_BLOCK - 1) / IGMC_BLOCK];
#pragma unroll
    for (int u = 0; u < (IGMC_STASH_LAYER + IGMC_BLOCK - 1) / IGMC_BLOCK; ++u) {
      const int i = tid + u * IGMC_BLOCK;
      stq[u] = stash[l * IGMC_STASH_LAYER + (i < IGMC_STASH_LAYER ? i : IGMC_STASH_LAYER - 1)];
    }
    const int f = tid & 31, e = c * 32 + f;
    const bool col = tid < 32, bias_role = c == 0 && tid >= 32 && tid < 64;
    int64_t idx[5];
    float pv[5], m1v[5], m2v[5], pvb[4] = {0.f, 0.f, 0.f, 0.f}, bq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      idx[q] = (q < 4) ? m.off_basis[l] + (int64_t)q * nE + e : m.off_root[l] + e;
      pv[q] = col ? P[idx[q]] : 0.f;
      m1v[q] = col ? at.m1[idx[q]] : 0.f;
      m2v[q] = col ? at.m2[idx[q]] : 0.f;
    }
    if (wave == 0) {
#pragma unroll
      for (int bb = 0; bb < 4; ++bb) pvb[bb] = P[idx[bb]];
    }
    if (bias_role) {
      const int64_t i = m.off_bias[l] + f;
      bq[1] = P[i];
      bq[2] = at.m1[i];
      bq[3] = at.m2[i];
    }
    if (tid == 0) *s_flag = 0;
    TF_STAMP(mb == 0, 1);      // the independent loads are requested
    // ---- set 0 of this workgroup's rows (dW_0[c] | dW_1[c], or d root[c] behind the last relation) summed over the partial
    // tables; the other sets and the bias row arrive as words from their producers
    const TsSlots sl = ts_slots(nparts, stride, B);
#pragma unroll
    for (int u = 0; u < (IGMC_STASH_LAYER + IGMC_BLOCK - 1) / IGMC_BLOCK; ++u) {
      const int i = tid + u * IGMC_BLOCK;
      if (i < IGMC_STASH_LAYER) s_st[i] = stq[u];
    }
    const float tot = tf_sum_set(m.ts_part + (size_t)l * IGMC_TS_BLOCKS * ts, sl, ts, R, fin, c, 0, ncol_a < 16 ? ncol_a : 16, sred4,
                                 (l == 3 && l3v) ? m.l3_vec : nullptr, l3v);
    if (wave == 0 && (lane >> 2) < ncol_a) rows[lane] = tot;
    TF_STAMP(mb == 0, 2);      // the set is reduced (the partial tables' round trip)
    // ---- this row's share of d att for the relations of set 0
    unsigned long long* words = m.fold_w + (size_t)l * 32 * IGMC_FOLD_NA;
    if (wave == 0) tf_datt_pub(tot, lane >> 5, R, pvb, words + c * IGMC_FOLD_NA, tag, l == mute_layer && mute_role == 0);
    TF_STAMP(mb == 0, 3);      // the row's words are published
    // ---- the words this workgroup needs, in ONE loop: its row's other sets, the layer's fin x 4 R d att products and the
    // layer's bias row -- <= IGMC_TF_POLL a thread, looked at together until every one carries the launch's tag; each goes to
    // its place in LDS (rows / s_datt)
    {
      const int nrw = 4 * ncol_a - 64, ndw = fin * na, nw = nrw + ndw + 32, npoll = (nw + IGMC_BLOCK - 1) / IGMC_BLOCK;
      const unsigned long long* wrow = m.fold_w + IGMC_FOLD_O_ROWS + (size_t)(l * 32 + c) * IGMC_FOLD_PSETS * 64;
      const unsigned long long* wp[IGMC_TF_POLL];
      int wi[IGMC_TF_POLL];      // destination, in floats of S
#pragma unroll
      for (int u = 0; u < IGMC_TF_POLL; ++u) {
        const int w = tid + u * IGMC_BLOCK, wc = w < nw ? w : nw - 1;
        if (wc < nrw) {                  // (sets 1.. are contiguous: [set - 1][64])
          wp[u] = wrow + wc;
          wi[u] = IGMC_TF_O_ROWS + 64 + wc;
        } else if (wc < nrw + ndw) {
          const int x = wc - nrw, y = (x / na) * IGMC_FOLD_NA + x % na;
          wp[u] = words + y;
          wi[u] = IGMC_TF_O_DATT + y;
        } else {
          const int x = wc - nrw - ndw;
          wp[u] = m.fold_w + IGMC_FOLD_O_BIAS + l * 32 + x;
          wi[u] = IGMC_TF_O_ROWS + (R + 1) * 32 + x;
        }
      }
      bool ok = false;
#ifndef IGMC_HIPEMU
      const long long t0 = (long long)wall_clock64();
#endif
      for (long it = 0;; ++it) {
        unsigned long long w[IGMC_TF_POLL];
        bool all = true;
#pragma unroll
        for (int u = 0; u < IGMC_TF_POLL; ++u)
          if (u < npoll) w[u] = g2_ld_word(wp[u]);      // (uniform over the workgroup)
#pragma unroll
        for (int u = 0; u < IGMC_TF_POLL; ++u) all = all && (u >= npoll || (uint32_t)(w[u] >> 32) == tag);
        if (all) {
#pragma unroll
          for (int u = 0; u < IGMC_TF_POLL; ++u)
            if (u < npoll) S[wi[u]] = __uint_as_float((uint32_t)w[u]);     // (clamped repeats: the same value again)
          ok = true;
          break;
        }
#ifndef IGMC_HIPEMU
        if ((it & 15) == 15 && (long long)wall_clock64() - t0 > IGMC_TF_TIMEOUT_TICKS) break;
        __builtin_amdgcn_s_sleep(2);
#else
        if (it > (1L << 12)) break;
        hipemu::yield();
#endif
      }
      if (!ok) *s_flag = 1;
    }
    __syncthreads();
    TF_STAMP(mb == 0, 5);      // the words are in
    if (*s_flag) {      // nothing of this workgroup's is updated
      if (tid == 0) {
        *m.gs_err = 1;
        if (at.ctrl) atomicOr((unsigned long long*)(at.ctrl + IGMC_CTRL_SYNC_ERR), (unsigned long long)IGMC_SYNC_ERR_FOLD);
      }
      return;
    }
    const float* st = s_st;
    // ---- the layer's new att (every workgroup forms it for its image words; c == 0 stores it, its moments and d att): the
    // fin partial products in index order, as k_finalize_ts adds them
    if (tid >= 64 && tid - 64 < na) {
      const int rb = tid - 64;
      float g = 0.f;
#pragma unroll
      for (int k = 0; k < 32; ++k) g += (k < fin) ? s_datt[k * IGMC_FOLD_NA + rb] : 0.f;
      s_attn[rb] = fts_att_entry(grad, at, st, R, rb, g, arr_coef, m.off_att[l] + rb, st[IGMC_STASH_ATT + rb],
                                 st[IGMC_STASH_ATTM1 + rb], st[IGMC_STASH_ATTM2 + rb], c == 0);
    }
    if (bias_role) {
      bq[0] = rows[(R + 1) * 32 + f];
      fts_bias(m, grad, at, ng, l, R, fin, f, bq, true);
    }
    if (col) {       // the column body of k_finalize_ts on (c, f)
      float g[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, tv[8], pn[5];
#pragma unroll
      for (int r = 0; r < 8; ++r) tv[r] = (r < R) ? rows[r * 32 + f] : 0.f;
      g[4] = rows[R * 32 + f];
      fts_col_table8(g, st, tv, R);
      fts_col_emit(grad, at, st, arr_coef, idx, g, pv, m1v, m2v, pn);
#pragma unroll
      for (int q = 0; q < 5; ++q) s_pn[q * 32 + f] = pn[q];
    }
    TF_STAMP(mb == 0, 6);      // the main pass is stored
    __syncthreads();
    {   // the image words of the 32 columns: thread -> (relation tid >> 5 of eight at a time, column f)
      float pn[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) pn[q] = s_pn[q * 32 + f];
      fts_image_col(m, ng, l, R, fin, c, f, s_attn, pn, tid >> 5, IGMC_BLOCK / 32);
    }
    TF_STAMP(mb == 0, 7);      // the image words are stored
  } else if (mb < nconv + nlin) {
    // ---- d lin1 / d lin2 and Adam on exactly the elements this workgroup formed: the 16 x 64 tile of lin1.weight and, for the
    // first column tile, 16 entries of lin1.bias / lin2.weight (+ lin2.bias)
    const int bx = (mb - nconv) & 7, by = (mb - nconv) >> 3, D = m.D;
    head_bwd_w_body(b, m, P, nullptr, 1, grad_scale, mult, drop_scale, grad, bx, by, B);
    __syncthreads();
    TF_STAMP(mb == nconv, 17);      // the tile's gradient is formed
    int64_t ix[5];
    bool okx[5];
    float gv[5], pv[5], av[5], vv[5];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int el = tid + k * IGMC_BLOCK, colx = by * 64 + (el & 63);
      okx[k] = colx < D;
      ix[k] = m.off_l1w + (int64_t)(bx * 16 + (el >> 6)) * D + (okx[k] ? colx : 0);
    }
    okx[4] = by == 0 && (tid < 32 || (tid == 32 && bx == 0));
    ix[4] = tid < 16 ? m.off_l1b + bx * 16 + tid : tid < 32 ? m.off_l2w + bx * 16 + tid - 16 : m.off_l2b;
    const float* gsrc = grad;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int64_t i = okx[k] ? ix[k] : m.off_l1w;      // clamped, not predicated: the loads go out back to back
      gv[k] = gsrc[i];
      pv[k] = at.p[i];
      av[k] = at.m1[i];
      vv[k] = at.m2[i];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (okx[k]) adam_store_sep(at.p, at.m1, at.m2, ix[k], gv[k], pv[k], av[k], vv[k], at.h);      // (adam_range's bits: k_finalize_ts's lin workgroups)
    TF_STAMP(mb == nconv, 18);
  } else {                                                     // loss, epoch total, control-block tick, sequence number
    if (bump_seq && tid == 0) m.gs_bar[1] += 1;               // (every workgroup of k_graph_step2 is done)
    loss_body(at.b, m, at.ARR, at.loss, at.total, S + IGMC_TF_O_SMF);
    TF_STAMP(true, 33);
    if (tid == 0 && at.ctrl) ctrl_check_and_advance(at.ctrl, at.b, at.use_flags);
    TF_STAMP(true, 34);
  }
}

__global__ __launch_bounds__(IGMC_BLOCK) void k_loss(BatchDev b, ModelDev m, float ARR, float* __restrict__ loss) {
  igmc_kernarg_warm<sizeof(BatchDev) + sizeof(ModelDev) + 32>();
  __shared__ float smf[8];
  loss_body(b, m, ARR, loss, nullptr, smf);
}

__global__ __launch_bounds__(IGMC_BLOCK) void k_sse_acc(BatchDev b, const float* __restrict__ out, double* acc, int64_t* ctrl) {
  igmc_kernarg_warm<sizeof(BatchDev) + 32>();
  __shared__ float smf[8];
  const int B = b.totals[3];
  float s = 0.f;
  for (int g = threadIdx.x; g < B; g += IGMC_BLOCK) {
    const float d = out[g] - b.y[g];
    s += d * d;
  }
  s = igmc_block_sum_f(s, smf);
  if (threadIdx.x == 0) {
    acc[0] += (double)s;
    acc[1] += (double)B;
    if (ctrl) ctrl_advance(ctrl);      // the evaluation step's tick in the same launch (igmc_sse_accumulate_tick)
  }
}

// =================================================================== fused Adam (flat buffer) + step epilogue
// With `fin` set, block 0 also produces the step's loss / epoch total, and the LAST block to finish advances
// the device-side step control (igmc_hip.h) for the next replay of the step graph.
__global__ void k_tick(int64_t* ctrl) {
  if (threadIdx.x == 0 && blockIdx.x == 0) ctrl_advance(ctrl);
}
// a new group of M steps starts at the current position (igmc_ctrl_regroup)
__global__ void k_regroup(int64_t* ctrl, int M, int64_t first_cur, int64_t first_next) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  ctrl[IGMC_CTRL_GROUP] = M > 0 ? M : 1;
  ctrl[IGMC_CTRL_GK] = 0;
  ctrl[IGMC_CTRL_GQ] = 0;
  ctrl[IGMC_CTRL_FIRST] = first_cur;
  ctrl[IGMC_CTRL_FIRST_ODD] = first_next;
}

// pacing gate of the extraction chain (igmc_ctrl_gate): one wave that returns once `gk_min` steps of the group of parity q
// are done -- or that group is over, or `timeout_ticks` of the 100 MHz wall clock have passed -- and then, if it had to wait
// for that step (or `delay_always`), `delay_ticks` later: the step that has just begun gets its workgroups onto the chip first.
// The kernels queued behind the gate on its stream start then.  A HINT, never a dependency: whatever follows the gate is
// correct at any time (the extraction of the NEXT group touches nothing the running group reads), so a gate that gives up
// only costs the pacing.
__global__ void k_step_gate(int64_t* ctrl, int q, int gk_min, long long delay_ticks, int delay_always,
                            long long timeout_ticks) {
#ifndef IGMC_HIPEMU
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const long long t0 = wall_clock64();
  bool waited = false;
  for (;;) {
    if ((igmc_ctrl_ld(ctrl + IGMC_CTRL_GQ) & 1) != (int64_t)(q & 1)) return;
    if (igmc_ctrl_ld(ctrl + IGMC_CTRL_GK) >= (int64_t)gk_min) break;
    if (wall_clock64() - t0 > timeout_ticks) {      // (counted: a caller whose gates keep giving up paces by edges instead)
      atomicAdd((unsigned long long*)(ctrl + IGMC_CTRL_GATE_TIMEOUTS), 1ull);
      return;
    }
    waited = true;
    __builtin_amdgcn_s_sleep(16);
  }
  if (waited || delay_always) {
    const long long t1 = wall_clock64();
    while (wall_clock64() - t1 < delay_ticks) __builtin_amdgcn_s_sleep(8);
  }
#endif
}

__global__ __launch_bounds__(IGMC_BLOCK) void k_adam(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m1, float* __restrict__ m2, int64_t n,
                                                       float step_size, float inv_sqrt_bc2, float beta1, float beta2,
                                                       float eps, float wd, int64_t* ctrl, int tick, FinishArgs fin) {
  // (the six scalars of an AdamHyper stay six arguments: as one by-value block they are no longer loaded together with ctrl,
  //  three scalar loads where one stands)
  __shared__ float smf[8];
  AdamHyper h = {step_size, inv_sqrt_bc2, beta1, beta2, eps, wd};
  if (ctrl) h = adam_hyper_from_ctrl(ctrl);      // hipGraph replay
  {   // a contiguous slice per workgroup, eight elements a thread and round with all their loads in flight (adam_range)
    const int64_t chunk = ((n + gridDim.x - 1) / gridDim.x + IGMC_BLOCK - 1) / IGMC_BLOCK * IGMC_BLOCK;
    const int64_t lo = (int64_t)blockIdx.x * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
    if (lo < n) adam_range<8>(p, g, m1, m2, lo, hi, h);
  }
  if (fin.enabled && blockIdx.x == 0) loss_body(fin.b, fin.m, fin.ARR, fin.loss, fin.total, smf);
  if (ctrl && tick) {
    // every block has read its scalars above; the last one to get here advances the control block
    __syncthreads();
    if (threadIdx.x == 0) {
      __threadfence();
      int* done = (int*)&ctrl[IGMC_CTRL_DONE];
      if (atomicAdd(done, 1) == (int)gridDim.x - 1) {
        *done = 0;
        if (fin.enabled) ctrl_check_and_advance(ctrl, fin.b, fin.use_flags);
        else ctrl_advance(ctrl);
      }
    }
  }
}

// =================================================================== host launch sequences

// grid for row-parallel kernels: enough workgroups for the capacity, capped, and a multiple of 8 (>= 8) so
// that every XCD residue owns workgroups (XCD-affine segments, see igmc_xcd_segment)
static inline int igmc_rows_grid(int cap_rows, int rows_per_block, int max_blocks) {
  int g = (cap_rows + rows_per_block - 1) / rows_per_block;
  if (g > max_blocks) g = max_blocks;
  g = (g + 7) & ~7;
  return g < 8 ? 8 : g;
}
// grid for the XCD-segmented kernels: 8 x (workgroups needed by the LARGEST segment = ceil(B/8) graphs of at
// most `slot` rows each), so that no XCD has to take a second round
static inline int igmc_xcd_grid(const ModelDev& m, int B, int rows_per_block, int max_blocks) {
  const int slot = (m.node_cap + m.graph_cap - 1) / m.graph_cap;
  const long rows = (long)((B + 7) / 8) * slot;
  long per = (rows + rows_per_block - 1) / rows_per_block;
  if (per < 1) per = 1;
  long g = 8 * per;
  if (g > max_blocks) g = max_blocks & ~7;
  return (int)(g < 8 ? 8 : g);
}

// grid of k_l0_fwd: every workgroup composes the layer-0 table W0[r * L + c] (R L x 32 values, 4 fmas + 5 loads each) before
// it walks rows; with many relations (yahoo_music: 284 table rows) thousands of 4-row workgroups spend their time on that
// -- there a workgroup takes 8 rows per table row of work it has to amortise
static inline int igmc_l0_grid(const ModelDev& m, int B) {
  int rows = 4;
  if (m.R * m.L > 32) rows = (m.R * m.L) / 8;
  return igmc_xcd_grid(m, B, rows, IGMC_GATHER_BLOCKS);
}

// k_rgcn_layer4's instantiations by their flags: the launches take their kernel from here, igmc_model_prepare walks all four
using RgcnKernel = decltype(&k_rgcn_layer4<false, false>);
static RgcnKernel rgcn_layer_kernel(bool use_flags, bool bwd) {
  RgcnKernel k = nullptr;
  igmc_dispatch([&](auto uf, auto bw) { k = k_rgcn_layer4<uf(), bw()>; }, use_flags, bwd);
  return k;
}

// ---- the phases of a call, each written once; sp (launch.h: StepPlan) says which kernels take them

// The four conv layers (h_0..h_3 left in HBM): all of them in ONE launch (k_dl_fwd; nothing follows that would advance its
// exchange tags unless sp.self_seq is 0: k_tail_ts then does), the dense per-layer kernels from the blocks alone -- no edge list
// is read -- or the row walkers; then the products Y_l = h_{l-1} @ [basis_0 | .. | basis_3] a separate backward's att gradient reads
static void launch_conv_fwd(const ModelDev& m, const BatchDev& b, const StepPlan& sp, const float* P, int B, int training,
                            int use_flags, void* stream) {
  if (sp.dl) igmc_launch_g2_compose(m, P, stream);        // the step's weight images + layer-0 table
  if (sp.dlf) {
    igmc_launch_dl_fwd(m, b, sp, P, B, training, use_flags, training ? m.dpre[3] : nullptr, stream);
  } else if (sp.dl) {
    igmc_launch_dl_layer0(m, b, B, training, use_flags, stream);
  } else {
    const size_t l0s = (size_t)(m.R * m.L * 32 + m.L * 32 + 32) * sizeof(float) + (size_t)4 * m.R * m.L * sizeof(int);
    igmc_dispatch([&](auto uf, auto tr) {
      IGMC_PLAUNCH("k_l0_fwd", (k_l0_fwd<uf(), tr()>), igmc_l0_grid(m, B), IGMC_BLOCK, l0s, stream, b, m, P, m.h[0]);
    }, use_flags != 0, training != 0);
  }
  const int gt = igmc_xcd_grid(m, B, 16, 2048);                        // fused layer: 16 rows per workgroup
  const size_t fsm4 = (size_t)(16 * IGMC_TP + 1024 + m.R * 4) * sizeof(float);
  for (int l = 1; l < 4 && !sp.dlf; ++l) {
    // the top layer's launch also clears dPre_3 (only its target rows are written by the head backward)
    float* zo = (training && l == 3) ? m.dpre[3] : nullptr;
    if (sp.dl) igmc_launch_dl_layer(m, b, P, B, l, 0, use_flags, zo, stream);
    else IGMC_PLAUNCH("k_rgcn_layer_fwd", rgcn_layer_kernel(use_flags != 0, false), gt, IGMC_BLOCK, fsm4, stream, b, m, P, l, zo);
  }
  if (training && sp.need_y)
    IGMC_PLAUNCH("k_dense_y_all", k_dense_y_all, dim3(igmc_rows_grid(m.node_cap, 64, 512), 3), IGMC_BLOCK,
                 (size_t)32 * (128 + 4) * sizeof(float), stream, b, m, P);
}

// The three backward layer passes, one launch each: transposed gather of dPre_l (+ d att partials, or relation-space tables),
// then [G | dPre_l] @ [basis^T ; root^T] + backward epilogue
static void launch_layers_bwd(const ModelDev& m, const BatchDev& b, const StepPlan& sp, const float* P, int B, int use_flags,
                              int tables, void* stream) {
  const int gt = igmc_xcd_grid(m, B, 16, 2048);
  const size_t bsm4 = (size_t)(16 * IGMC_TP + 1024 + m.R * 4 + 16 * m.R * 4) * sizeof(float);
  for (int l = 3; l >= 1; --l) {
    if (sp.bwd_dense) igmc_launch_dl_layer(m, b, P, B, l, 1, use_flags, nullptr, stream, tables);
    else IGMC_PLAUNCH("k_rgcn_layer_bwd", rgcn_layer_kernel(use_flags != 0, true), gt, IGMC_BLOCK, bsm4, stream, b, m, P, l,
                      (float*)nullptr);
  }
}

// The layer-0 table gradient where it does not ride in the MFMA weight-gradient kernel, then the reduction of every partial
// (nstash = 4: its extra workgroups prepare the stash of k_finalize_ts in basis-space mode)
static void launch_reduce(const ModelDev& m, const BatchDev& b, const StepPlan& sp, const float* P, int B, const int64_t* ctrl,
                          int nstash, void* stream) {
  const int rows0 = m.R * m.L + m.L + 1, l0_mfma = rows0 <= 32;
  const float* d0 = m.dpre[0];
  if (l0_mfma) {
  } else if (rows0 <= 64) IGMC_PLAUNCH("k_l0_bwd", (k_l0_bwd<8>), IGMC_L0_BLOCKS, IGMC_BLOCK, 0, stream, b, m, d0, m.l0_part);
  else IGMC_PLAUNCH("k_l0_bwd", (k_l0_bwd<40>), IGMC_L0_BLOCKS, IGMC_BLOCK, 0, stream, b, m, d0, m.l0_part);
  const int nblk = ((l0_mfma ? 4 : 3) * igmc_wg_stride() + 63) / 64 + (l0_mfma ? 0 : (rows0 * 32 + 63) / 64) + (3 * m.R * 4 + 3) / 4;
  IGMC_PLAUNCH("k_reduce_partials", k_reduce_partials, nblk + nstash, IGMC_BLOCK, 0, stream, m,
               sp.bwd_dense ? sp.dl_grid : igmc_xcd_grid(m, B, 16, 2048), l0_mfma, IGMC_WG_BLOCKS, P, ctrl, nstash);
}

// Sum of the workgroups' relation-space tables (+ nlin workgroups that form d lin1 / d lin2, + the stash of k_finalize_ts)
static void launch_tail_ts(const ModelDev& m, const BatchDev& b, const float* P, int B, float grad_scale, float mult, float* grad,
                           int nlin, int nparts, int stride, int nstash, const int64_t* ctrl, int bump_seq, int l3v, void* stream) {
  IGMC_PLAUNCH("k_tail_ts", k_tail_ts, nlin + (4 * m.ts_stride + 63) / 64 + nstash, IGMC_BLOCK, 0, stream, b, m, P, grad_scale,
               mult, 2.f, grad, nlin, nparts, stride, B, nstash, ctrl, bump_seq, l3v);
}

// ... and the whole tail behind the subgraph kernel as ONE launch (sp.tail_fold; the stash role ran in the launch in front)
static void launch_tail_fin(const ModelDev& m, const BatchDev& b, const float* P, int B, float grad_scale, float mult, float* grad,
                            float arr_coef, const AdamTail& at, int nlin, int nparts, int stride, int bump_seq, int l3v,
                            void* stream) {
  int mute = -1;
#ifdef IGMC_HIPEMU
  // (emulator only -- the timeout test: the publishers of this layer stay silent and its pollers give up; with
  // IGMC_EMU_FOLD_MUTE_ROLE=rows / bias only the layer's row producers / its bias producer)
  if (const char* e = getenv("IGMC_EMU_FOLD_MUTE")) {
    mute = atoi(e);
    const char* role = getenv("IGMC_EMU_FOLD_MUTE_ROLE");
    if (mute >= 0 && role) mute |= (!strcmp(role, "rows") ? 1 : !strcmp(role, "bias") ? 2 : 0) << 8;
  }
#endif
  // the mains of a layer wait for each other's words and for producers: aligned groups of 32 consecutive workgroups run
  // together, one group after the other (layout: above k_tail_fin)
  igmc_emu_cluster(32, -1, 0);
  const int nconv = 96 + m.L, nsets = (8 * (m.R + 1) + 15) / 16, nprod = ((nsets - 1) * nconv + 4 + 31) & ~31;
  IGMC_PLAUNCH("k_tail_fin", k_tail_fin, nprod + nconv + nlin + 1, IGMC_BLOCK, (size_t)IGMC_TF_WORDS * sizeof(float), stream, b, m, P,
               grad_scale, mult, 2.f, grad, arr_coef, at, nlin, nparts, stride, B, bump_seq, mute, l3v);
}

// The reduced gradient sources of a data-parallel step, summed over the ranks: tables + d att partials (one allocation), or the
// basis-space sums (+ layer-0 table, d att); and the lin gradients (the tail of the flat parameter vector)
static int launch_exchange(const ModelDev& m, int tail, const StepExchange* xch, float* grad, void* stream) {
  if (!xch || tail == IGMC_TAIL_HANDOFF) return 0;
  const int rows0 = m.R * m.L + m.L + 1;
  const int64_t n = tail == IGMC_TAIL_TS ? (int64_t)4 * m.ts_stride + (int64_t)4 * m.ts_stride / 32 * 4
                                         : (int64_t)3 * igmc_wg_stride() + 3 * m.R * 4 + rows0 * 32;
  return xch->sum(xch->user, tail == IGMC_TAIL_TS ? m.ts_raw : m.graw, n, grad + m.off_l1w, m.n_params - m.off_l1w, stream);
}

// Gradient (+ ARR) of the conv parameters from the reduced sources; at.enabled: Adam on every parameter rides in it (and the
// weight images of the updated parameters, img) -- else the loss is a launch of its own where one is asked for.
// (ts_mode: k_finalize reads relation-space tables -- the subgraph kernel's, IGMC_FIN_MODE=0)
static void launch_finalize(const ModelDev& m, const BatchDev& b, const float* P, float* grad, float arr_coef, int tail,
                            int ts_mode, const AdamTail& at, int img, float ARR, float* loss, int* img_emitted, void* stream) {
  const int bs = tail == IGMC_TAIL_BS;
  if (tail == IGMC_TAIL_HANDOFF) {
    if (at.enabled) IGMC_PLAUNCH("k_finalize_adam", k_finalize, 4 * IGMC_FIN_NB + 32, IGMC_BLOCK, 0, stream, m, P, grad, arr_coef, at, ts_mode);
    else IGMC_PLAUNCH("k_finalize", k_finalize, 4 * IGMC_FIN_NB, IGMC_BLOCK, 0, stream, m, P, grad, arr_coef, at, ts_mode);
  } else if (at.enabled) {
    IGMC_PLAUNCH("k_finalize_adam", k_finalize_ts, 4 * IGMC_FTS_NB + 32 + 1, IGMC_BLOCK, 0, stream, m, P, grad, arr_coef, at, 32, bs, img);
    if (img_emitted) *img_emitted = img;
  } else {
    IGMC_PLAUNCH("k_finalize", k_finalize_ts, 4 * IGMC_FTS_NB, IGMC_BLOCK, 0, stream, m, P, grad, arr_coef, at, 0, bs, 0);
  }
  if (!at.enabled && loss) igmc_launch_loss(m, b, ARR, loss, stream);
}

// ---- the public sequences

void igmc_launch_forward(const ModelDev& m, const BatchDev& b, const StepPlan& sp, int B, int training, int use_flags,
                         const StepHead& hd, void* stream) {
  if (sp.family == IGMC_FAM_G2) {      // (evaluation only: IGMC_CALL_EVAL -- no dropout mask, no loss gradient)
    const StepHead ev = {hd.P, nullptr, hd.seed, hd.step, hd.mult, 0.f, hd.out};
    igmc_launch_graph_step2(m, b, sp, B, 0, use_flags, ev, stream);
    return;
  }
  launch_conv_fwd(m, b, sp, hd.P, B, training, use_flags, stream);
  const int hgrid = (B + IGMC_HG - 1) / IGMC_HG;
  const size_t fs = (size_t)IGMC_HG * m.D * sizeof(float);
  if (m.D % 16 == 0)
    IGMC_PLAUNCH("k_head_fwd", k_head_fwd_mfma, (B + 15) / 16, 512, 0, stream, b, m, hd.P, training, hd.inj_mask, hd.seed,
                 hd.step, hd.mult, hd.out);
  else if (fs <= 48 * 1024)
    IGMC_PLAUNCH("k_head_fwd", (k_head_fwd<true>), hgrid, 512, fs, stream, b, m, hd.P, training, hd.inj_mask, hd.seed,
                 hd.step, hd.mult, hd.out);
  else
    IGMC_PLAUNCH("k_head_fwd", (k_head_fwd<false>), hgrid, 512, 0, stream, b, m, hd.P, training, hd.inj_mask, hd.seed,
                 hd.step, hd.mult, hd.out);
}

// The four conv layers alone, whatever the readout that follows (centre-node readout of IGMC: igmc_launch_forward; sort-pool
// readout of DGCNN_RS: sortpool.hip)
void igmc_launch_conv_forward(const ModelDev& m, const BatchDev& b, const StepPlan& sp, const float* P, int B, int training,
                              int use_flags, void* stream) {
  launch_conv_fwd(m, b, sp, P, B, training, use_flags, stream);
}

void igmc_launch_backward(const ModelDev& m, const BatchDev& b, const StepPlan& sp, const float* P, int B, int use_flags,
                          const float* gout, int from_err, float grad_scale, float mult, float drop_scale,
                          float arr_coef, float* grad, void* stream) {
  const int hgrid = (B + IGMC_HG - 1) / IGMC_HG;
  if (m.D % 16 == 0)
    IGMC_PLAUNCH("k_head_bwd_a", k_head_bwd_a_mfma, dim3((B + 15) / 16, (m.D / 16 + 7) / 8), 512, 0, stream, b, m, P,
                 gout, from_err, grad_scale, mult, drop_scale, m.dpre[3]);
  else
    IGMC_PLAUNCH("k_head_bwd_a", k_head_bwd_a, hgrid, 1024, 0, stream, b, m, P, gout, from_err, grad_scale, mult,
                 drop_scale, m.dpre[3]);
  if (m.D % 16 == 0)      // (same stream: see the note at k_wgrad)
    IGMC_PLAUNCH("k_head_bwd_w", k_head_bwd_w_mfma, dim3(8, (m.D / 16 + 3) / 4), IGMC_BLOCK, 0, stream, b, m, P, gout,
                 from_err, grad_scale, mult, drop_scale, grad);
  else
    IGMC_PLAUNCH("k_head_bwd_w", k_head_bwd_w, dim3(17, (m.D + 255) / 256), IGMC_BLOCK, 0, stream, b, m, P, gout, from_err,
                 grad_scale, mult, drop_scale, grad);
  igmc_launch_conv_backward(m, b, sp, P, B, use_flags, arr_coef, grad, stream);
}

// Backward of the four conv layers from dPre_3 (in m.dpre[3]) and the readout's gradient w.r.t. h_0..h_2 (gfeat on the
// target rows, or the dense m.dcat[l]): dPre_2..0, weight-gradient partials, their reduction, gradient (+ ARR) of the conv
// parameters into `grad` (no Adam).
// sp.dlb -- a dense readout gradient (sort-pool family) on the one-launch backward of the dense layers: dPre_3 of every row from
// m.dpre[3], the readout gradient of layers 0..2 added per row from m.dcat, relation-space tables -> k_tail_ts (no lin1 / lin2
// role) -> k_finalize_ts: three launches instead of the three layer passes, the Y products' consumers (k_wgrad), the
// partials' reduction and k_finalize.  (IGMC_DL_TS=0 / IGMC_DL_FUSED=0|1: the per-layer form.)
void igmc_launch_conv_backward(const ModelDev& m, const BatchDev& b, const StepPlan& sp, const float* P, int B, int use_flags,
                               float arr_coef, float* grad, void* stream) {
  AdamTail none;
  memset(&none, 0, sizeof(none));
  if (sp.dlb) {
    const int gstride = (B + 7) & ~7;
    igmc_launch_dl_bwd(m, b, sp, B, use_flags, stream, nullptr, 1);
    launch_tail_ts(m, b, P, B, 0.f, 1.f, grad, 0, (sp.nqu + sp.nqv) * gstride, gstride, 4, nullptr, 1, 0, stream);
  } else {
    const int l0_mfma = m.R * m.L + m.L + 1 <= 32;       // layer-0 table gradient rides in the MFMA weight-gradient kernel
    launch_layers_bwd(m, b, sp, P, B, use_flags, 0, stream);
    IGMC_PLAUNCH("k_wgrad", k_wgrad, dim3(IGMC_WG_BLOCKS, l0_mfma ? 4 : 3), IGMC_BLOCK, 0, stream, b, m, 0);
    launch_reduce(m, b, sp, nullptr, B, nullptr, 0, stream);
  }
  launch_finalize(m, b, P, grad, arr_coef, sp.tail, 0, none, 0, 0.f, nullptr, nullptr, stream);
}

// Fused-step sequence (loss + gradients [+ Adam]) with the multi-role launches -- per family: forward, head, backward, tail,
// exchange, finalize
//   subgraph kernel:   k_graph_step (all of it down to per-workgroup tables), k_tail_ts, finalize
//   dense + tables:    k_dl_fwd | layers, {head in k_dl_bwd | k_head_sub + k_dl_bwd | k_head_sub + 3 x layer_bwd}, k_tail_ts, finalize
//   per layer:         l0_fwd, 3 x layer_fwd, {head fwd+bwd | Y}, 3 x layer_bwd, {weight grads | lin grads}, reduce, finalize
int igmc_launch_loss_grad(const ModelDev& m_in, const BatchDev& b, const StepPlan& sp, int B, int use_flags, const StepHead& hd,
                          float ARR, float arr_scale, float* grad, float* loss, const AdamTail* adam, void* stream,
                          const StepExchange* xch, int* img_emitted) {
  ModelDev m = m_in;
  m.adam_m1 = adam ? adam->m1 : nullptr;       // (the stash roles keep att's moments of before the step)
  m.adam_m2 = adam ? adam->m2 : nullptr;
  if (img_emitted) *img_emitted = 0;
  const int rows0 = m.R * m.L + m.L + 1;
  // the gradient / Adam kernel also leaves the weight images of the updated parameters
  const int img = adam && m.g2_w && m.R <= G2_NR * G2_NG_MAX && rows0 <= (g2_t0_rows(m.R, m.L) == 32 ? 32 : 48);
  const int ny = (m.D / 16 + 3) / 4;
  const float* Pc = hd.P;
  const float grad_scale = hd.grad_scale, mult = hd.mult;
  AdamTail at;
  memset(&at, 0, sizeof(at));
  if (adam) {
    at = *adam;
    at.enabled = sp.fast_head;      // (the generic sequence: Adam is a launch of its own)
    at.b = b;
    at.ARR = ARR;
  }
  at.use_flags = use_flags;
  at.skip = xch ? xch->failed : nullptr;
  const int64_t* ctrl = adam ? at.ctrl : nullptr;
  if (!sp.fast_head) {      // generic sequence
    igmc_launch_forward(m, b, sp, B, 1, use_flags, hd, stream);
    igmc_launch_backward(m, b, sp, Pc, B, use_flags, nullptr, 1, grad_scale, mult, 2.f, ARR * arr_scale, grad, stream);
    if (adam) {
      igmc_launch_finish(m, b, at.p, grad, at.m1, at.m2, at.h, at.ctrl, ARR, at.loss, at.total, use_flags, stream);
    } else if (loss) {
      igmc_launch_loss(m, b, ARR, loss, stream);
    }
    return 0;
  }
  const int tables = sp.tail == IGMC_TAIL_TS;
  if (sp.family == IGMC_FAM_G2) {
    // one workgroup (cluster) per subgraph: forward, residual and backward down to the per-workgroup gradient partials;
    // bump_seq = 1: k_tail_ts advances the launch sequence number of the subgraph kernel's exchange tags
    // sp.tail_fold, a step with Adam that leaves the weight images, no exchange: the tail is ONE launch behind the subgraph
    // kernel, whose launch then carries the stash role (four more workgroups)
    const int fold = sp.tail_fold && tables && adam && at.enabled && img && !xch;
    const int stride = (sp.cs > 1) ? ((B + 7) & ~7) : IGMC_TS_BLOCKS;
    const int bump_seq = igmc_launch_graph_step2(m, b, sp, B, 1, use_flags, hd, stream, fold ? 4 : 0, ctrl);
    if (fold) {
      launch_tail_fin(m, b, Pc, B, grad_scale, mult, grad, ARR * arr_scale, at, 8 * ny, sp.grid, stride, bump_seq, sp.l3_vec, stream);
      if (img_emitted) *img_emitted = 1;
      return 0;
    }
    launch_tail_ts(m, b, Pc, B, grad_scale, mult, grad, 8 * ny, sp.grid, (sp.cs > 1) ? ((B + 7) & ~7) : IGMC_TS_BLOCKS,
                   tables ? 4 : 0, ctrl, bump_seq, sp.l3_vec, stream);
  } else {
    launch_conv_fwd(m, b, sp, Pc, B, 1, use_flags, stream);
    if (sp.dlts) {
      // the head: in the set-up of the one-launch backward (side features included), or one workgroup per subgraph in front of
      // the backward -- one launch, or one per layer
      const int inside = sp.dlb && sp.head_inside;
      if (!inside) igmc_launch_head_sub(m, b, B, hd, stream);
      if (sp.dlb) igmc_launch_dl_bwd(m, b, sp, B, use_flags, stream, inside ? &hd : nullptr);
      else launch_layers_bwd(m, b, sp, Pc, B, use_flags, 1, stream);
      const int gstride = (B + 7) & ~7;
      launch_tail_ts(m, b, Pc, B, grad_scale, mult, grad, 8 * ny, (sp.nqu + sp.nqv) * gstride, gstride, 4, ctrl, sp.dlf ? 1 : 0, 0, stream);
    } else {
      const int gy = igmc_rows_grid(m.node_cap, 128, 512), hb = (B + 15) / 16, nsl = rows0 <= 32 ? 4 : 3;
      IGMC_PLAUNCH("k_head_train", k_head_train, dim3(hb > gy ? hb : gy, 4), 512, (size_t)32 * (128 + 4) * sizeof(float), stream,
                   b, m, Pc, hd.inj_mask, hd.seed, hd.step, mult, grad_scale, hd.out);
      launch_layers_bwd(m, b, sp, Pc, B, use_flags, 0, stream);
      IGMC_PLAUNCH("k_wgrad_head", k_wgrad_head, dim3(IGMC_WG_BLOCKS, nsl + 1), IGMC_BLOCK, 0, stream, b, m, Pc,
                   (const float*)nullptr, 1, grad_scale, mult, 2.f, grad, nsl);
      launch_reduce(m, b, sp, Pc, B, ctrl, sp.tail == IGMC_TAIL_BS ? 4 : 0, stream);
    }
  }
  // (the ARR term depends on the weights only: every rank adds it in full AFTER the exchange)
  if (const int rc = launch_exchange(m, sp.tail, xch, grad, stream)) return rc;
  launch_finalize(m, b, Pc, grad, ARR * arr_scale, sp.tail, sp.family == IGMC_FAM_G2, at, img, ARR, loss, img_emitted, stream);
  return 0;
}

void igmc_launch_loss(const ModelDev& m, const BatchDev& b, float ARR, float* loss, void* stream) {
  IGMC_PLAUNCH("k_loss", k_loss, 1, IGMC_BLOCK, 0, stream, b, m, ARR, loss);
}

void igmc_launch_sse(const BatchDev& b, const float* out, double* acc, int64_t* ctrl, void* stream) {
  IGMC_PLAUNCH("k_sse_acc", k_sse_acc, 1, IGMC_BLOCK, 0, stream, b, out, acc, ctrl);
}

void igmc_launch_tick(int64_t* ctrl, void* stream) { IGMC_PLAUNCH("k_tick", k_tick, 1, 64, 0, stream, ctrl); }
void igmc_launch_regroup(int64_t* ctrl, int M, int64_t first_cur, int64_t first_next, void* stream) {
  IGMC_PLAUNCH("k_regroup", k_regroup, 1, 64, 0, stream, ctrl, M, first_cur, first_next);
}
void igmc_launch_gate(int64_t* ctrl, int q, int gk_min, long long delay_ticks, int delay_always, long long timeout_ticks,
                      void* stream) {
  IGMC_PLAUNCH("k_step_gate", k_step_gate, 1, 64, 0, stream, ctrl, q, gk_min, delay_ticks, delay_always, timeout_ticks);
}

// (one workgroup per 2048 elements, at most 256: the tick of the step's last workgroup is an atomic round trip per workgroup on
//  ONE counter -- 550 single-round workgroups spent 20 us of a 28 us launch queueing on it)
static int adam_grid(int64_t n) {
  int grid = (int)((n + 8 * IGMC_BLOCK - 1) / (8 * IGMC_BLOCK));
  if (grid > 256) grid = 256;
  return grid < 1 ? 1 : grid;
}

void igmc_launch_adam(float* p, const float* g, float* m1, float* m2, int64_t n, const AdamHyper& h, int64_t* ctrl, int tick,
                      void* stream) {
  FinishArgs fin;
  memset(&fin, 0, sizeof(fin));
  IGMC_PLAUNCH("k_adam", k_adam, adam_grid(n), IGMC_BLOCK, 0, stream, p, g, m1, m2, n, h.step_size, h.inv_sqrt_bc2, h.beta1, h.beta2,
               h.eps, h.wd, ctrl, tick, fin);
}

// Adam + loss + epoch total (+ control-block tick) in ONE launch
void igmc_launch_finish(const ModelDev& m, const BatchDev& b, float* p, const float* g, float* m1, float* m2, const AdamHyper& h,
                        int64_t* ctrl, float ARR, float* loss, double* total, int use_flags, void* stream) {
  FinishArgs fin;
  fin.enabled = 1;
  fin.use_flags = use_flags;
  fin.b = b;
  fin.m = m;
  fin.ARR = ARR;
  fin.loss = loss;
  fin.total = total;
  IGMC_PLAUNCH("k_step_finish", k_adam, adam_grid(m.n_params), IGMC_BLOCK, 0, stream, p, g, m1, m2,
               (int64_t)m.n_params, h.step_size, h.inv_sqrt_bc2, h.beta1, h.beta2, h.eps, h.wd, ctrl, ctrl ? 1 : 0, fin);
}

int igmc_model_prepare(const ModelDev& m) {
#ifndef IGMC_HIPEMU
  // dynamic LDS above 48 KB needs an explicit opt-in on HIP (many relations -> large d-att tables in the backward)
  const int bsm4 = (int)((size_t)(16 * IGMC_TP + 1024 + m.R * 4 + 16 * m.R * 4) * sizeof(float));
  if (bsm4 > 48 * 1024) {
    if (bsm4 > 150 * 1024) return 1;
    for (int v = 0; v < 4; ++v)      // (the backward's size: the forward's is smaller)
      if (hipFuncSetAttribute((const void*)rgcn_layer_kernel(v & 1, v & 2), hipFuncAttributeMaxDynamicSharedMemorySize, bsm4) != hipSuccess) return 1;
  }
#endif
  (void)m;
  return igmc_gs_prepare();
}
