// scores.hip -- per-link predictions kept on the device, and the selection of their extremes
// (reference train_eval.py:248-272, the first two thirds of `visualize`: score every link, argsort, take `num` at both ends).
//
// k_scores_store   the tail of a SCORING step: k_sse_acc (model.hip) -- same launch shape, same summation, same tick, so the
//                  pass's squared-error sum is bit-identical to eval_loss's -- which also files the batch's outputs and labels
//                  at their positions of the pass: scores[first + g] = out[g], labels[first + g] = y[g].
// k_select_part    a grid of workgroups, each reducing a strided slice of the keys to its own `num` lowest and `num` highest;
// k_select_merge   one workgroup over the partial lists.
//
// THE ORDER (the only one; igmc_hip.h states it for callers):  (key ascending, index ascending), every NaN behind every
// number, -0.0 == 0.0.  That is np.argsort(keys, kind='stable').  A key and its index travel as ONE 64-bit word --
// order-preserving image of the float in the high half, index in the low half -- so "the i-th of the order" is "the i-th
// smallest word", words are distinct, and minima / maxima of words are associative and commutative: the result does not
// depend on how the keys are divided among threads, waves or workgroups (any grid gives the same lists).
// Selection is `num` rounds of "smallest word above the last one taken" (and its mirror): no sorting network, no atomics,
// plain vector stores only; num <= 64 rounds over data that sits in L2 (1 M keys = 4 MB).
#include "capi.h"
#include "select.h"      // sel_image / sel_word, SEL_LOW_NONE / SEL_HIGH_NONE, IGMC_SELECT_MAX_NUM

#define IGMC_SELECT_MAX_GRID 1024

// (min, max) over the workgroup, result in every thread.  sm: 2 * 4 words of LDS.
__device__ __forceinline__ void sel_block_minmax(unsigned long long& lo, unsigned long long& hi, unsigned long long* sm) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long a = __shfl_xor(lo, d, 64), b = __shfl_xor(hi, d, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sm[wave] = lo;
    sm[4 + wave] = hi;
  }
  __syncthreads();
  const int nw = (blockDim.x + 63) >> 6;
  for (int w = 0; w < nw; ++w) {
    lo = sm[w] < lo ? sm[w] : lo;
    hi = sm[4 + w] > hi ? sm[4 + w] : hi;
  }
  __syncthreads();
}

// workgroup b reduces keys[b], keys[b + G], ... (thread t of it: every IGMC_BLOCK-th of those) to part_low[b * num + r] = the
// r-th smallest word of its slice and part_high[b * num + r] = the r-th largest (none left: SEL_LOW_NONE / SEL_HIGH_NONE)
__global__ __launch_bounds__(IGMC_BLOCK) void k_select_part(const float* __restrict__ keys, int64_t n, int num,
                                                            unsigned long long* __restrict__ part_low,
                                                            unsigned long long* __restrict__ part_high) {
  __shared__ unsigned long long sm[8];
  const int64_t start = (int64_t)blockIdx.x * IGMC_BLOCK + threadIdx.x, stride = (int64_t)gridDim.x * IGMC_BLOCK;
  unsigned long long last_lo = SEL_HIGH_NONE, last_hi = SEL_LOW_NONE;      // (taken so far: everything <= / >= these)
  for (int r = 0; r < num; ++r) {
    unsigned long long lo = SEL_LOW_NONE, hi = SEL_HIGH_NONE;
    for (int64_t i = start; i < n; i += stride) {
      const unsigned long long w = sel_word(keys[i], (uint32_t)i);
      if (w > last_lo && w < lo) lo = w;
      if (w < last_hi && w > hi) hi = w;
    }
    sel_block_minmax(lo, hi, sm);
    if (threadIdx.x == 0) {
      part_low[(int64_t)blockIdx.x * num + r] = lo;
      part_high[(int64_t)blockIdx.x * num + r] = hi;
    }
    last_lo = lo;       // (nothing left: the bound is then SEL_LOW_NONE / SEL_HIGH_NONE and later rounds find nothing either)
    last_hi = hi;
  }
}

// one workgroup: the same rounds over the `np` = G * num partial words of each side; entry r of the result is written by
// thread 0 (index, the key's own bits read back from `keys`); entries past count = min(n, num) get index -1, key 0
__global__ __launch_bounds__(IGMC_BLOCK) void k_select_merge(const float* __restrict__ keys, int64_t n, int num,
                                                             const unsigned long long* __restrict__ part_low,
                                                             const unsigned long long* __restrict__ part_high, int np,
                                                             int32_t* __restrict__ idx_low, int32_t* __restrict__ idx_high,
                                                             float* __restrict__ key_low, float* __restrict__ key_high,
                                                             int32_t* __restrict__ count) {
  __shared__ unsigned long long sm[8];
  unsigned long long last_lo = SEL_HIGH_NONE, last_hi = SEL_LOW_NONE;
  for (int r = 0; r < num; ++r) {
    unsigned long long lo = SEL_LOW_NONE, hi = SEL_HIGH_NONE;
    for (int i = threadIdx.x; i < np; i += IGMC_BLOCK) {
      const unsigned long long a = part_low[i], b = part_high[i];
      if (a > last_lo && a < lo) lo = a;
      if (b < last_hi && b > hi) hi = b;
    }
    sel_block_minmax(lo, hi, sm);
    if (threadIdx.x == 0) {
      const bool has_lo = lo != SEL_LOW_NONE, has_hi = hi != SEL_HIGH_NONE;
      const int64_t il = (int64_t)(lo & 0xFFFFFFFFull), ih = (int64_t)(hi & 0xFFFFFFFFull);
      idx_low[r] = has_lo && il < n ? (int32_t)il : -1;
      idx_high[r] = has_hi && ih < n ? (int32_t)ih : -1;
      if (key_low) key_low[r] = has_lo && il < n ? keys[il] : 0.f;
      if (key_high) key_high[r] = has_hi && ih < n ? keys[ih] : 0.f;
    }
    last_lo = lo;
    last_hi = hi;
  }
  if (threadIdx.x == 0 && count) count[0] = (int32_t)(n < (int64_t)num ? n : (int64_t)num);
}

// the scoring step's tail.  `first` = the batch's first position in the pass's link order: `first_arg` where the caller knows it
// (>= 0: eager launches), else the one the node-set kernel of the batch in this arena resolved from the control block
// (BatchDev::stamp[0]; -1 where the arena has none).  A position outside [0, n) is NOT written and raises err[0]
// (bit 0: past the buffers; bit 1: no position known); the sums and the tick are k_sse_acc's in every case.
__global__ __launch_bounds__(IGMC_BLOCK) void k_scores_store(BatchDev b, const float* __restrict__ out, double* acc,
                                                             int64_t* ctrl, float* __restrict__ scores,
                                                             float* __restrict__ labels, int64_t n, int64_t first_arg,
                                                             int32_t* err) {
  igmc_kernarg_warm<sizeof(BatchDev) + 64>();
  __shared__ float smf[8];
  const int B = b.totals[3];
  const int64_t first = first_arg >= 0 ? first_arg : b.stamp[0];
  float s = 0.f;
  for (int g = threadIdx.x; g < B; g += IGMC_BLOCK) {
    const float o = out[g], y = b.y[g];
    const float d = o - y;
    s += d * d;
    const int64_t pos = first + g;
    if (first >= 0 && pos < n) {
      scores[pos] = o;
      labels[pos] = y;
    }
  }
  s = igmc_block_sum_f(s, smf);
  if (threadIdx.x == 0) {
    acc[0] += (double)s;
    acc[1] += (double)B;
    const int bad = first < 0 ? 2 : (B > 0 && first + B > n) ? 1 : 0;
    if (bad) err[0] |= bad;
    if (ctrl) ctrl_advance(ctrl);
  }
}

// ------------------------------------------------------------------ host
static void igmc_launch_scores_store(const BatchDev& b, const float* out, double* acc, int64_t* ctrl, float* scores, float* labels,
                              int64_t n, int64_t first, int32_t* err, void* stream) {
  IGMC_PLAUNCH("k_scores_store", k_scores_store, 1, IGMC_BLOCK, 0, stream, b, out, acc, ctrl, scores, labels, n, first, err);
}

// workgroups of the partial pass where the caller names none: 16 keys per thread and round, at most SEL_MAX_GRID lists to merge
static int igmc_select_default_grid(int64_t n) {
  const int64_t per = (int64_t)IGMC_BLOCK * 16;
  const int64_t g = (n + per - 1) / per;
  return (int)(g < 1 ? 1 : g > IGMC_SELECT_MAX_GRID ? IGMC_SELECT_MAX_GRID : g);
}

static void igmc_launch_select(const float* keys, int64_t n, int num, int grid, void* scratch, int32_t* idx_low, int32_t* idx_high,
                        float* key_low, float* key_high, int32_t* count, void* stream) {
  unsigned long long* part_low = (unsigned long long*)scratch;
  unsigned long long* part_high = part_low + (size_t)grid * num;
  IGMC_PLAUNCH("k_select_part", k_select_part, grid, IGMC_BLOCK, 0, stream, keys, n, num, part_low, part_high);
  IGMC_PLAUNCH("k_select_merge", k_select_merge, 1, IGMC_BLOCK, 0, stream, keys, n, num,
               (const unsigned long long*)part_low, (const unsigned long long*)part_high, grid * num, idx_low, idx_high,
               key_low, key_high, count);
}

// ------------------------------------------------------------------ C ABI
extern "C" int igmc_scores_store(const float* d_out, const igmc_batch* b, double* d_acc, float* d_scores, float* d_labels,
                                 int64_t n, int64_t first_or_minus1, int64_t* d_ctrl, int32_t* d_err, void* stream) {
  if (!d_out || !b || !d_acc || !d_scores || !d_labels || !d_err) IGMC_FAIL("null argument");
  if (n < 1 || n > (int64_t)INT32_MAX) IGMC_FAIL("n must be in [1, 2^31)");
  if (first_or_minus1 < -1 || first_or_minus1 >= n) IGMC_FAIL("first must be -1 (the arena's stamp) or a position below n");
  igmc_launch_scores_store(b->d, d_out, d_acc, d_ctrl, d_scores, d_labels, n, first_or_minus1, d_err, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
static int select_grid(int64_t n, int num, int grid) {
  if (n < 1 || n > (int64_t)INT32_MAX || num < 1 || num > IGMC_SELECT_MAX_NUM || grid < 0 || grid > IGMC_SELECT_MAX_GRID) return -1;
  return grid > 0 ? grid : igmc_select_default_grid(n);
}
extern "C" int64_t igmc_select_scratch_bytes(int64_t n, int num, int grid) {
  const int g = select_grid(n, num, grid);
  if (g < 0) {
    igmc_err() = std::string(__func__) + ": n must be in [1, 2^31), num in [1, 64], grid in [0, 1024]";
    return -1;
  }
  return (int64_t)2 * g * num * (int64_t)sizeof(uint64_t);
}
extern "C" int igmc_select_extremes(const float* d_keys, int64_t n, int num, int32_t* d_idx_low, int32_t* d_idx_high,
                                    float* d_key_low, float* d_key_high, int32_t* d_count, void* d_scratch,
                                    int64_t scratch_bytes, int grid, void* stream) {
  if (!d_keys || !d_idx_low || !d_idx_high || !d_scratch) IGMC_FAIL("null argument");
  const int g = select_grid(n, num, grid);
  if (g < 0) IGMC_FAIL("n must be in [1, 2^31), num in [1, 64], grid in [0, 1024]");
  if (scratch_bytes < (int64_t)2 * g * num * (int64_t)sizeof(uint64_t)) IGMC_FAIL("scratch too small (igmc_select_scratch_bytes)");
  if (((uintptr_t)d_scratch & 7) != 0) IGMC_FAIL("scratch must be 8-byte aligned");
  igmc_launch_select(d_keys, n, num, g, d_scratch, d_idx_low, d_idx_high, d_key_low, d_key_high, d_count, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
