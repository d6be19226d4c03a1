// ranking.hip -- where GIVEN items stand in the score segments of a candidate pass, and the per-user sums of the held-out
// ranking metrics (no reference counterpart: the reference stops at the test RMSE; by hand this is every candidate score pulled
// to the host and one np.lexsort per user).
//
// THE ORDER of a segment is the one of igmc_select_segments (select.h: sel_word_desc): key descending, position ascending, every
// NaN behind every number, -0.0 == 0.0.  Words are distinct, so the 0-based place of an entry in that order is the NUMBER OF
// WORDS OF ITS SEGMENT BELOW ITS OWN: one streaming pass over the keys, an integer, the same under every launch geometry.
//
// k_rank_check    every query's answer starts as -1 / -1; the query offsets are checked as a whole (err bit 0) and the segment
//                 offsets against the number of keys (err bit 1).
// k_rank_find     one workgroup per segment, a thread per query: binary search of the query's id in the segment's ids (strictly
//                 ascending) -> its position; rank 0 where it is found.  Nothing where k_rank_check raised bit 0.
// k_rank_count    workgroup (s, j) counts slice j of the k contiguous slices of segment s (the slices of k_segsel_part).  The
//                 queries of the segment are taken RANK_TILE at a time -- longer lists: tile after tile, the slice streamed again
//                 --; the slice's words go through LDS in chunks of RANK_CHUNK.  A tile of nqt queries is padded to a power of
//                 two QP and the workgroup is cut into IGMC_BLOCK / QP groups: thread t counts, for query t % QP, the words
//                 t / QP, t / QP + G, ... of the chunk (an LDS broadcast read per word), the groups' counts meet in LDS and one
//                 vector atomic add per query and slice lands on the output.  Integer sums commute: the result does not depend
//                 on k.
// k_rank_metrics  one WAVE per user: lane l takes the user's queries l, l + 64, ..., and the 64 partial sums meet in a fixed
//                 xor butterfly -- float64 sums in an order that depends on the user's queries alone, so the output is
//                 bit-identical for every grid.
// Plain vector loads and stores; atomics: the LDS and global integer adds of the counts, the OR of the error word.
#include "capi.h"
#include "select.h"

#define IGMC_RANK_MAX_KS 8              // cut-offs K of one metrics launch at most
#define RANK_TILE IGMC_BLOCK      // queries of one tile: at most one per thread
#define RANK_CHUNK 2048           // selection words of a slice staged at a time (16 KB)

// [lo, hi) of segment s where it lies inside the n keys, else an empty range at 0
__device__ __forceinline__ bool rank_segment(const int64_t* __restrict__ seg_off, int64_t s, int64_t n, int64_t* lo,
                                             int64_t* hi) {
  const int64_t a = seg_off[s], b = seg_off[s + 1];
  const bool ok = a >= 0 && a <= b && b <= n;
  *lo = ok ? a : 0;
  *hi = ok ? b : 0;
  return ok;
}
// [qa, qb) of the queries of segment s where that lies inside the nq queries, else empty
__device__ __forceinline__ bool rank_queries(const int64_t* __restrict__ q_off, int64_t s, int64_t nq, int64_t* qa,
                                             int64_t* qb) {
  const int64_t a = q_off[s], b = q_off[s + 1];
  const bool ok = a >= 0 && a <= b && b <= nq;
  *qa = ok ? a : 0;
  *qb = ok ? b : 0;
  return ok;
}

__global__ __launch_bounds__(IGMC_BLOCK) void k_rank_check(const int64_t* __restrict__ seg_off, const int64_t* __restrict__ q_off,
                                                           int ns, int64_t n, int64_t nq, int32_t* __restrict__ q_pos,
                                                           int32_t* __restrict__ q_rank, int32_t* err) {
  const int64_t stride = (int64_t)gridDim.x * IGMC_BLOCK;
  const int64_t i0 = (int64_t)blockIdx.x * IGMC_BLOCK + threadIdx.x;
  for (int64_t i = i0; i < nq; i += stride) {
    q_pos[i] = -1;
    q_rank[i] = -1;
  }
  int bad = 0;
  for (int64_t s = i0; s < ns; s += stride) {
    int64_t a, b;
    if (!rank_queries(q_off, s, nq, &a, &b) || (s == 0 && q_off[0] != 0) || (s == ns - 1 && q_off[ns] != nq)) bad |= 1;
    if (!rank_segment(seg_off, s, n, &a, &b)) bad |= 2;
  }
  if (bad) atomicOr(err, bad);
}

__global__ __launch_bounds__(IGMC_BLOCK) void k_rank_find(const int32_t* __restrict__ ids, const int64_t* __restrict__ seg_off,
                                                          const int64_t* __restrict__ q_off, const int32_t* __restrict__ q_id,
                                                          int ns, int64_t n, int64_t nq, int32_t* __restrict__ q_pos,
                                                          int32_t* __restrict__ q_rank, const int32_t* err) {
  if (*err & 1) return;        // (uniform over the launch: the queries cannot be told apart, every answer stays -1 / -1)
  for (int64_t s = blockIdx.x; s < ns; s += gridDim.x) {
    int64_t lo, hi, qa, qb;
    rank_segment(seg_off, s, n, &lo, &hi);
    rank_queries(q_off, s, nq, &qa, &qb);
    for (int64_t q = qa + threadIdx.x; q < qb; q += IGMC_BLOCK) {
      const int32_t want = q_id[q];
      int64_t a = lo, b = hi;        // first position of [lo, hi) whose id is not below `want`
      while (a < b) {
        const int64_t mid = a + ((b - a) >> 1);
        if (ids[mid] < want) a = mid + 1;
        else b = mid;
      }
      if (a < hi && ids[a] == want) {
        q_pos[q] = (int32_t)a;
        q_rank[q] = 0;
      }
    }
  }
}

__global__ __launch_bounds__(IGMC_BLOCK) void k_rank_count(const float* __restrict__ keys, const int64_t* __restrict__ seg_off,
                                                           const int64_t* __restrict__ q_off, int ns, int k, int64_t n,
                                                           int64_t nq, const int32_t* __restrict__ q_pos,
                                                           int32_t* __restrict__ q_rank, const int32_t* err) {
  __shared__ unsigned long long st[RANK_CHUNK];
  __shared__ int cnt[RANK_TILE];
  if (*err & 1) return;
  const int t = threadIdx.x;
  const int64_t jobs = (int64_t)ns * k;
  for (int64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int64_t s = job / k;
    const int j = (int)(job - s * k);
    int64_t lo, hi, qa, qb;
    rank_segment(seg_off, s, n, &lo, &hi);
    rank_queries(q_off, s, nq, &qa, &qb);
    const int64_t chunk = (hi - lo + k - 1) / k;
    const int64_t a = lo + j * chunk;
    const int64_t e = a + chunk < hi ? a + chunk : hi;
    if (e <= a) continue;        // (uniform: an empty slice adds nothing)
    for (int64_t q0 = qa; q0 < qb; q0 += RANK_TILE) {
      const int nqt = (int)(qb - q0 < RANK_TILE ? qb - q0 : RANK_TILE);
      int qp = 1;
      while (qp < nqt) qp <<= 1;
      const int groups = IGMC_BLOCK / qp, mine = t & (qp - 1), group = t / qp;
      // a query nobody found, or a padding lane: the word below every word, which counts nothing
      unsigned long long word = SEL_HIGH_NONE;
      if (mine < nqt) {
        const int32_t p = q_pos[q0 + mine];
        if (p >= 0) word = sel_word_desc(keys[p], (uint32_t)p);
      }
      cnt[t] = 0;
      int c = 0;
      for (int64_t c0 = a; c0 < e; c0 += RANK_CHUNK) {
        const int m = (int)(e - c0 < RANK_CHUNK ? e - c0 : RANK_CHUNK);
        __syncthreads();        // (the last chunk has been read; cnt is cleared)
        for (int i = t; i < m; i += IGMC_BLOCK) st[i] = sel_word_desc(keys[c0 + i], (uint32_t)(c0 + i));
        __syncthreads();
        for (int i = group; i < m; i += groups) c += st[i] < word ? 1 : 0;
      }
      if (c) atomicAdd(&cnt[mine], c);
      __syncthreads();
      if (t < nqt && cnt[t]) atomicAdd(&q_rank[q0 + t], cnt[t]);
      __syncthreads();        // (the next tile clears cnt)
    }
  }
}

// sum over the wave in a fixed order, result in every lane
__device__ __forceinline__ double rank_wave_sum(double v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__device__ __forceinline__ double rank_gain(int place) { return 1.0 / log2((double)place + 2.0); }

__global__ __launch_bounds__(IGMC_BLOCK) void k_rank_metrics(const int32_t* __restrict__ q_rank, const int64_t* __restrict__ q_off,
                                                             const uint8_t* __restrict__ q_rel, const int32_t* __restrict__ ks,
                                                             int nk, int ns, int64_t nq, int32_t* __restrict__ cnt_out,
                                                             double* __restrict__ dcg_out, int32_t* err) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * (IGMC_BLOCK >> 6) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (IGMC_BLOCK >> 6);
  int K[IGMC_RANK_MAX_KS];
#pragma unroll
  for (int i = 0; i < IGMC_RANK_MAX_KS; ++i) K[i] = i < nk ? ks[i] : 0;
  for (int64_t s = wave0; s < ns; s += nwaves) {        // (uniform over the wave)
    int64_t qa, qb;
    if (!rank_queries(q_off, s, nq, &qa, &qb) && lane == 0) atomicOr(err, 1);        // (the user then has no query)
    int n_rel = 0, first = 0x7FFFFFFF;
    int hits[IGMC_RANK_MAX_KS];
    double dcg[IGMC_RANK_MAX_KS];
#pragma unroll
    for (int i = 0; i < IGMC_RANK_MAX_KS; ++i) hits[i] = 0, dcg[i] = 0.0;
    for (int64_t q = qa + lane; q < qb; q += 64) {
      const int r = q_rank[q];
      if (r < 0 || (q_rel && q_rel[q] == 0)) continue;
      ++n_rel;
      first = r < first ? r : first;
      const double gain = rank_gain(r);
#pragma unroll
      for (int i = 0; i < IGMC_RANK_MAX_KS; ++i)
        if (r < K[i]) ++hits[i], dcg[i] += gain;
    }
    n_rel = igmc_wave_sum_i(n_rel);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const int o = __shfl_xor(first, d, 64);
      first = o < first ? o : first;
    }
    int32_t* co = cnt_out + s * (2 + nk);
    double* dq = dcg_out + s * (2 * nk);
    if (lane == 0) {
      co[0] = n_rel;
      co[1] = n_rel > 0 ? first : -1;
    }
#pragma unroll
    for (int i = 0; i < IGMC_RANK_MAX_KS; ++i) {
      if (i < nk) {        // (uniform)
        const int h = igmc_wave_sum_i(hits[i]);
        const double d = rank_wave_sum(dcg[i]);
        const int ideal = K[i] < n_rel ? K[i] : n_rel;        // the best list: the user's relevant items in its first places
        double id = 0.0;
        for (int p = lane; p < ideal; p += 64) id += rank_gain(p);
        id = rank_wave_sum(id);
        if (lane == 0) {
          co[2 + i] = h;
          dq[i] = d;
          dq[nk + i] = id;
        }
      }
    }
  }
}

// ------------------------------------------------------------------ host
static int rank_grid(int64_t jobs) { return (int)(jobs < 1 ? 1 : jobs > 65536 ? 65536 : jobs); }

static void igmc_launch_rank_segments(const float* keys, const int32_t* ids, int64_t n, const int64_t* seg_off, int ns,
                               const int64_t* q_off, const int32_t* q_id, int64_t nq, int k, int32_t* q_pos, int32_t* q_rank,
                               int32_t* err, void* stream) {
  const int64_t most = nq > ns ? nq : (int64_t)ns;
  IGMC_PLAUNCH("k_rank_check", k_rank_check, rank_grid((most + IGMC_BLOCK - 1) / IGMC_BLOCK), IGMC_BLOCK, 0, stream, seg_off,
               q_off, ns, n, nq, q_pos, q_rank, err);
  if (nq < 1) return;
  IGMC_PLAUNCH("k_rank_find", k_rank_find, rank_grid(ns), IGMC_BLOCK, 0, stream, ids, seg_off, q_off, q_id, ns, n, nq, q_pos,
               q_rank, (const int32_t*)err);
  IGMC_PLAUNCH("k_rank_count", k_rank_count, rank_grid((int64_t)ns * k), IGMC_BLOCK, 0, stream, keys, seg_off, q_off, ns, k, n,
               nq, (const int32_t*)q_pos, q_rank, (const int32_t*)err);
}

static void igmc_launch_rank_metrics(const int32_t* q_rank, const int64_t* q_off, const uint8_t* q_rel, const int32_t* ks, int nk,
                              int ns, int64_t nq, int grid, int32_t* cnt, double* dcg, int32_t* err, void* stream) {
  const int waves = IGMC_BLOCK >> 6;
  IGMC_PLAUNCH("k_rank_metrics", k_rank_metrics, grid > 0 ? grid : rank_grid(((int64_t)ns + waves - 1) / waves), IGMC_BLOCK, 0,
               stream, q_rank, q_off, q_rel, ks, nk, ns, nq, cnt, dcg, err);
}

// ------------------------------------------------------------------ C ABI
extern "C" int igmc_rank_segments(const float* d_keys, const int32_t* d_ids, int64_t n, const int64_t* d_seg_off, int ns,
                                  const int64_t* d_q_off, const int32_t* d_q_id, int64_t nq, int32_t* d_q_pos,
                                  int32_t* d_q_rank, int32_t* d_err, int geometry, void* stream) {
  if (!d_keys || !d_ids || !d_seg_off || !d_q_off || !d_err) IGMC_FAIL("null argument");
  if (nq > 0 && (!d_q_id || !d_q_pos || !d_q_rank)) IGMC_FAIL("null argument");
  if (n < 1 || n > (int64_t)INT32_MAX) IGMC_FAIL("n must be in [1, 2^31)");
  if (nq < 0 || nq > (int64_t)INT32_MAX) IGMC_FAIL("nq must be in [0, 2^31)");
  if (ns < 1 || geometry < 0 || geometry > IGMC_SEGSEL_MAX_SPLIT) IGMC_FAIL("ns must be at least 1, geometry in [0, 64]");
  igmc_launch_rank_segments(d_keys, d_ids, n, d_seg_off, ns, d_q_off, d_q_id, nq,
                            geometry > 0 ? geometry : igmc_segsel_default_split(ns), d_q_pos, d_q_rank, d_err, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
extern "C" int igmc_rank_metrics(const int32_t* d_q_rank, const int64_t* d_q_off, const uint8_t* d_q_rel, int64_t nq, int ns,
                                 const int32_t* d_ks, int nk, int32_t* d_cnt, double* d_dcg, int32_t* d_err, int grid,
                                 void* stream) {
  if (!d_q_off || !d_ks || !d_cnt || !d_dcg || !d_err) IGMC_FAIL("null argument");
  if (nq > 0 && !d_q_rank) IGMC_FAIL("null argument");
  if (nq < 0 || nq > (int64_t)INT32_MAX) IGMC_FAIL("nq must be in [0, 2^31)");
  if (ns < 1 || nk < 1 || nk > IGMC_RANK_MAX_KS || grid < 0 || grid > 65536)
    IGMC_FAIL("ns must be at least 1, nk in [1, 8], grid in [0, 65536]");
  igmc_launch_rank_metrics(d_q_rank, d_q_off, d_q_rel, d_ks, nk, ns, nq, grid, d_cnt, d_dcg, d_err, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
