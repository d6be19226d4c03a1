// pairs.hip -- pair training (no reference counterpart: the reference trains on observed links with MSE alone; by hand a ranking
// objective there is a host loop drawing an unseen item per link and an autograd loss over the two scores).
//
// THE NEGATIVE of positive k = (u, i) of a pair list (igmc_hip.h states it for callers): with c_t = igmc_pair_candidate(
// igmc_pair_salt(seed, epoch, k), t, n_items), the c_t of the smallest t < T that is not in the user's row and passes item_ok;
// where none of the T tries qualifies, the first qualifying item of c_0, c_0 + 1, .., n_items - 1, 0, .., c_0 - 1; where no
// item qualifies the pair is void.  Keyed by the positive's position in the list: no shuffle or batch size changes a draw.
//
// k_pair_negatives  one WAVE per positive (grid-stride), no workgroup barrier: lane t holds try 64 r + t of round r; the user's
//                   row -- sorted by (relation, item), so not searchable by id -- goes through a 64-entry LDS stage of the wave,
//                   chunk after chunk, and every lane compares its candidate with the 64 staged entries (LDS broadcast reads,
//                   four entries a read); the first qualifying lane is a ballot + ffs.  A row has no size limit and there is
//                   no second path.  The cyclic scan takes 64 consecutive items a step against the same row walk.
//                   <HARD> (igmc_pair_negatives_shortlist) puts one question in front of the tries: where 32 hashed bits of the
//                   salt decide so, ONE entry of the user's shortlist segment -- decision and pick uniform over the wave -- goes
//                   through the same row walk as the only live candidate (lane 0); if it qualifies it is the negative (label
//                   2), else the tries run as they always do.  <false> is the kernel igmc_pair_negatives has always launched.
// k_pair_loss       one workgroup over a batch whose even slots are positives and odd slots their negatives: every pair in
//                   float64, the sums by a strided loop and a fixed LDS tree -- the same bits on every run.
// k_pair_kind_stats one workgroup over the same batch: count, ordered pairs and pair term per kind of negative (label 1 / 2), the
//                   sums as k_pair_loss forms them.
// Plain vector stores only (error word: a vector atomic OR, reached on errors only).
#include "capi.h"
#include <stdlib.h>

#define PAIR_GRID_MAX 2048      // workgroups of the sampler at most: four positives each, the rest by the grid stride
#define IGMC_PAIR_TRIES 256             // hashed candidates tried before the cyclic scan decides (IGMC_PAIR_TRIES: test hook)
struct PairArgs {
  GraphDev g;
  const int32_t* pos_u;
  const int32_t* pos_v;
  int64_t n;
  const uint8_t* item_ok;       // may be null
  uint64_t seed, epoch;
  int tries;
  int32_t* link_u;              // [2n] each
  int32_t* link_v;
  float* link_y;
  int32_t* err;
  const int64_t* sl_off;        // igmc_pair_negatives_shortlist alone: the per-user table, its entries, floor(share * 2^32)
  const int32_t* sl_item;
  int64_t sl_total;
  uint64_t hard_thr;
};

template <bool HARD>
__global__ __launch_bounds__(IGMC_BLOCK) void k_pair_negatives(PairArgs a) {
  __shared__ __attribute__((aligned(16))) int32_t stage[IGMC_BLOCK / 64][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = IGMC_BLOCK >> 6;
  int32_t* st = stage[wave];
  const uint32_t n_items = (uint32_t)a.g.n_items;
  for (int64_t k = (int64_t)blockIdx.x * nwave + wave; k < a.n; k += (int64_t)gridDim.x * nwave) {
    const int u = a.pos_u[k], i = a.pos_v[k];
    if (u < 0 || u >= a.g.n_users || i < 0 || i >= a.g.n_items) {      // (uniform over the wave) no row is read: a void pair
      if (lane == 0) {
        a.link_u[2 * k] = a.link_u[2 * k + 1] = u;
        a.link_v[2 * k] = a.link_v[2 * k + 1] = i;
        a.link_y[2 * k + 1] = 0.f;
        atomicOr(a.err, 1);
      }
      continue;
    }
    const int lo = a.g.u_ptr[u], hi = a.g.u_ptr[u + 1];
    // live lanes whose item is not in the row; every lane of the wave walks the row (the stage is the wave's)
    auto unseen = [&](int c, bool live) -> bool {
      if (__ballot(live) == 0ull) return false;
      bool seen = false;
      for (int base = lo; base < hi; base += 64) {
        st[lane] = lane < hi - base ? a.g.u_idx[base + lane] : -1;
        IGMC_WAVE_SYNC();
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int4 e = ((const int4*)st)[q];
          seen |= (e.x == c) | (e.y == c) | (e.z == c) | (e.w == c);
        }
        IGMC_WAVE_SYNC();      // (the next chunk overwrites the stage)
      }
      return live && !seen;
    };
    const uint64_t salt = igmc_pair_salt(a.seed, a.epoch, (uint64_t)k);
    int j = -1;
    bool hard = false;
    if constexpr (HARD) {
      if (igmc_pair_hard(salt, a.hard_thr)) {      // (uniform over the wave: u and the salt are)
        const int64_t sa = a.sl_off[u], sb = a.sl_off[u + 1];
        if (sa < 0 || sb < sa || sb > a.sl_total) {      // not a segment of the table: nothing is read from it
          if (lane == 0) atomicOr(a.err, 8);
        } else if (sb > sa) {
          const int c = a.sl_item[sa + (int64_t)igmc_pair_pick(salt, (uint32_t)(sb - sa))];
          const bool live = lane == 0 && c >= 0 && c < a.g.n_items && (!a.item_ok || a.item_ok[c] != 0);
          if (__ballot(unseen(c, live))) {
            j = c;
            hard = true;
          } else if (lane == 0) {
            atomicOr(a.err, 4);      // a stale table: the uniform draw decides
          }
        }
      }
    }
    for (int t0 = 0; t0 < a.tries && j < 0; t0 += 64) {
      const int t = t0 + lane;
      const uint32_t c = igmc_pair_candidate(salt, (uint64_t)t, n_items);
      const bool live = t < a.tries && (!a.item_ok || a.item_ok[c] != 0);
      const unsigned long long m = __ballot(unseen((int)c, live));
      if (m) j = __shfl((int)c, __ffsll((long long)m) - 1, 64);
    }
    if (j < 0) {      // the cyclic order from c_0: 64 consecutive items a step
      const uint32_t c0 = igmc_pair_candidate(salt, 0, n_items);
      for (uint32_t o0 = 0; o0 < n_items && j < 0; o0 += 64) {
        const uint32_t o = o0 + lane;
        uint32_t c = c0 + o;
        if (c >= n_items) c -= n_items;
        const bool live = o < n_items && (!a.item_ok || a.item_ok[c] != 0);
        const unsigned long long m = __ballot(unseen((int)c, live));
        if (m) j = __shfl((int)c, __ffsll((long long)m) - 1, 64);
      }
    }
    if (lane == 0) {
      a.link_u[2 * k] = a.link_u[2 * k + 1] = u;
      a.link_v[2 * k] = i;
      a.link_v[2 * k + 1] = j >= 0 ? j : i;      // (a void pair: every slot stays an extractable link)
      a.link_y[2 * k + 1] = j >= 0 ? (hard ? 2.f : 1.f) : 0.f;
      if (j < 0) atomicOr(a.err, 2);
    }
  }
}

// stats[0] = sum_ok softplus(-d), [1] = sum_ok (s_pos - y)^2, [2] = #{ok: d > 0}, [3] = P_ok;  gout: igmc_hip.h
__global__ __launch_bounds__(IGMC_BLOCK) void k_pair_loss(const float* __restrict__ out, const float* __restrict__ y, int P,
                                                          double A, float* __restrict__ gout, double* __restrict__ stats) {
  __shared__ double sm[4][IGMC_BLOCK];
  const int t = threadIdx.x;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p = t; p < P; p += IGMC_BLOCK) {
    if (y[2 * p + 1] != 0.f) {
      const double sp = (double)out[2 * p], d = sp - (double)out[2 * p + 1], e = sp - (double)y[2 * p];
      acc[0] += fmax(-d, 0.0) + log1p(exp(-fabs(d)));
      acc[1] += e * e;
      acc[2] += d > 0.0 ? 1.0 : 0.0;
      acc[3] += 1.0;
    }
  }
  for (int q = 0; q < 4; ++q) sm[q][t] = acc[q];
  __syncthreads();
  for (int h = IGMC_BLOCK / 2; h >= 1; h >>= 1) {
    if (t < h)
      for (int q = 0; q < 4; ++q) sm[q][t] += sm[q][t + h];
    __syncthreads();
  }
  const double p_ok = sm[3][0];
  if (t < 4) stats[t] = sm[t][0];
  for (int p = t; p < P; p += IGMC_BLOCK) {
    float gp = 0.f, gn = 0.f;
    if (y[2 * p + 1] != 0.f) {
      const double sp = (double)out[2 * p], d = sp - (double)out[2 * p + 1], e = sp - (double)y[2 * p];
      const double sg = 1.0 / (1.0 + exp(d));
      gp = (float)((-sg + 2.0 * A * e) / p_ok);
      gn = (float)(sg / p_ok);
    }
    gout[2 * p] = gp;
    gout[2 * p + 1] = gn;
  }
}

// stats6[0..3) = count, #{d > 0}, sum softplus(-d) over the pairs whose negative's label is 1; [3..6) the same for label 2
__global__ __launch_bounds__(IGMC_BLOCK) void k_pair_kind_stats(const float* __restrict__ out, const float* __restrict__ y, int P,
                                                                double* __restrict__ stats6) {
  __shared__ double sm[6][IGMC_BLOCK];
  const int t = threadIdx.x;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int p = t; p < P; p += IGMC_BLOCK) {
    const float l = y[2 * p + 1];
    if (l == 1.f || l == 2.f) {
      const int o = l == 2.f ? 3 : 0;
      const double d = (double)out[2 * p] - (double)out[2 * p + 1];
      acc[o] += 1.0;
      acc[o + 1] += d > 0.0 ? 1.0 : 0.0;
      acc[o + 2] += fmax(-d, 0.0) + log1p(exp(-fabs(d)));
    }
  }
  for (int q = 0; q < 6; ++q) sm[q][t] = acc[q];
  __syncthreads();
  for (int h = IGMC_BLOCK / 2; h >= 1; h >>= 1) {
    if (t < h)
      for (int q = 0; q < 6; ++q) sm[q][t] += sm[q][t + h];
    __syncthreads();
  }
  if (t < 6) stats6[t] = sm[t][0];
}

// stats[4] = the ARR term of the step, from the per-layer sums the gradient kernel left (as k_loss forms it)
__global__ void k_pair_arr(const float* __restrict__ arr_part, float ARR, double* __restrict__ stats) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const float reg = arr_part[0] + arr_part[1] + arr_part[2] + arr_part[3];
    stats[4] = (double)(ARR * reg);
  }
}

// ------------------------------------------------------------------ host
static int pair_grid(int64_t n) {
  const int nwave = IGMC_BLOCK >> 6;
  const int64_t blocks = (n + nwave - 1) / nwave;
  return (int)(blocks < 1 ? 1 : blocks > PAIR_GRID_MAX ? PAIR_GRID_MAX : blocks);
}

static void igmc_launch_pair_negatives(const PairArgs& a, void* stream) {
  IGMC_PLAUNCH("k_pair_negatives", k_pair_negatives<false>, pair_grid(a.n), IGMC_BLOCK, 0, stream, a);
}

static void igmc_launch_pair_negatives_shortlist(const PairArgs& a, void* stream) {
  IGMC_PLAUNCH("k_pair_negatives_shortlist", k_pair_negatives<true>, pair_grid(a.n), IGMC_BLOCK, 0, stream, a);
}

static void igmc_launch_pair_kind_stats(const float* out, const float* y, int B, double* stats6, void* stream) {
  IGMC_PLAUNCH("k_pair_kind_stats", k_pair_kind_stats, 1, IGMC_BLOCK, 0, stream, out, y, B / 2, stats6);
}

void igmc_launch_pair_loss(const float* out, const float* y, int B, float mse_weight, float* gout, double* stats, void* stream) {
  IGMC_PLAUNCH("k_pair_loss", k_pair_loss, 1, IGMC_BLOCK, 0, stream, out, y, B / 2, (double)mse_weight, gout, stats);
}

void igmc_launch_pair_arr(const float* arr_part, float ARR, double* stats, void* stream) {
  IGMC_PLAUNCH("k_pair_arr", k_pair_arr, 1, 64, 0, stream, arr_part, ARR, stats);
}

// ------------------------------------------------------------------ C ABI (igmc_pair_loss_grad runs the model: capi.hip)
static int pair_tries() {
  int tries = IGMC_PAIR_TRIES;
  if (const char* e = getenv("IGMC_PAIR_TRIES")) tries = atoi(e);      // (test hook: the cyclic scan after few tries, or none)
  return tries < 0 ? 0 : tries > (1 << 20) ? (1 << 20) : tries;
}

extern "C" int igmc_pair_negatives(const igmc_graph* g, const int32_t* d_pos_u, const int32_t* d_pos_v, int64_t n,
                                   const uint8_t* d_item_ok, uint64_t seed, uint64_t epoch, int32_t* d_link_u,
                                   int32_t* d_link_v, float* d_link_y, int32_t* d_err, void* stream) {
  if (!g || !d_pos_u || !d_pos_v || !d_link_u || !d_link_v || !d_link_y || !d_err) IGMC_FAIL("null argument");
  if (n < 1 || n >= ((int64_t)1 << 30)) IGMC_FAIL("n must be in [1, 2^30): the 2 n link positions are int32");
  const PairArgs a = {g->d, d_pos_u, d_pos_v, n, d_item_ok, seed, epoch, pair_tries(), d_link_u, d_link_v, d_link_y, d_err};
  igmc_launch_pair_negatives(a, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int igmc_pair_negatives_shortlist(const igmc_graph* g, const int32_t* d_pos_u, const int32_t* d_pos_v, int64_t n,
                                             const uint8_t* d_item_ok, uint64_t seed, uint64_t epoch, const int64_t* d_sl_off,
                                             const int32_t* d_sl_item, int64_t sl_total, double hard_share, int32_t* d_link_u,
                                             int32_t* d_link_v, float* d_link_y, int32_t* d_err, void* stream) {
  if (!g || !d_pos_u || !d_pos_v || !d_link_u || !d_link_v || !d_link_y || !d_err) IGMC_FAIL("null argument");
  if (n < 1 || n >= ((int64_t)1 << 30)) IGMC_FAIL("n must be in [1, 2^30): the 2 n link positions are int32");
  if (!(hard_share >= 0.0 && hard_share <= 1.0)) IGMC_FAIL("hard_share must be in [0, 1]");
  if (hard_share > 0.0 && (!d_sl_off || !d_sl_item)) IGMC_FAIL("a share above 0 needs the table: d_sl_off and d_sl_item");
  if (sl_total < 0 || sl_total >= ((int64_t)1 << 31)) IGMC_FAIL("sl_total must be in [0, 2^31)");
  PairArgs a = {g->d, d_pos_u, d_pos_v, n, d_item_ok, seed, epoch, pair_tries(), d_link_u, d_link_v, d_link_y, d_err};
  a.sl_off = d_sl_off;
  a.sl_item = d_sl_item;
  a.sl_total = sl_total;
  a.hard_thr = igmc_pair_hard_threshold(hard_share);
  if (a.hard_thr == 0) igmc_launch_pair_negatives(a, stream);      // (no pair can decide hard: the table is not looked at)
  else igmc_launch_pair_negatives_shortlist(a, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int igmc_pair_kind_stats(const float* d_out, const float* d_y, int B, double* d_stats6, void* stream) {
  if (!d_out || !d_y || !d_stats6) IGMC_FAIL("null argument");
  if (B < 2 || (B & 1)) IGMC_FAIL("a pair batch holds an even number of links, at least two");
  igmc_launch_pair_kind_stats(d_out, d_y, B, d_stats6, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int igmc_pair_loss(const float* d_out, const float* d_y, int B, float mse_weight, float* d_gout, double* d_stats,
                              void* stream) {
  if (!d_out || !d_y || !d_gout || !d_stats) IGMC_FAIL("null argument");
  if (B < 2 || (B & 1)) IGMC_FAIL("a pair batch holds an even number of links, at least two");
  igmc_launch_pair_loss(d_out, d_y, B, mse_weight, d_gout, d_stats, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
