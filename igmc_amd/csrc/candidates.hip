// candidates.hip -- what surrounds a scoring pass over links NOBODY RATED: the candidate links of a set of users written straight
// into device link arrays, and the `num` best of every user's score segment (no reference counterpart: the reference stops at the
// test RMSE; a top-N list there would be a host loop over the complement of every user's row and a host argsort of its scores).
//
// k_candidates<0>  per-user counts; k_candidates<1>  the links, at offsets the caller derived from the counts.  One workgroup
//                  per requested user (grid-stride).  The user's row -- sorted by (relation, item), so not searchable -- is
//                  MARKED into an LDS bitmap over a tile of CAND_TILE items; wave w then takes the 64-item words w, w + 4, ...:
//                  a lane per item, survivors (in range, not marked, item_ok) as one ballot; the word's place in the segment is
//                  a block scan of the words' popcounts, a lane's place in its word the popcount of the ballot below it.
//                  Output order = (users as given, item ascending), a function of the inputs alone: the only atomic is the
//                  LDS bit-set of the marking, which commutes.  Graphs wider than a tile: the tiles one after the other, the
//                  row walked once per tile.
// k_segsel_part    workgroup (s, j) reduces slice j of the k contiguous slices of segment s to its `num` first words -- staged
// k_segsel_merge   in LDS when the slice fits --; k == 1 writes the segment's result itself, k > 1 leaves partial lists that
//                  one workgroup per segment merges.
//
// THE ORDER of a segment (igmc_hip.h states it for callers): (key descending, index ascending), every NaN behind every number,
// -0.0 == 0.0 -- np.lexsort((idx, np.where(np.isnan(k), 0, -k), np.isnan(k))); the two-key np.lexsort((idx, np.where(np.isnan(k),
// np.inf, -k))) is that order only for segments without a -inf key.  A key and its GLOBAL position travel as one 64-bit
// word (select.h: sel_word_desc), the order is "word ascending", words are distinct: the lists do not depend on k.
// Plain vector stores only (error words: a vector atomic OR, reached on errors only).
#include "launch.h"
#include "select.h"

#define CAND_TILE_WORDS IGMC_BLOCK                 // 64-item words of a bitmap tile: one per thread of the scan
#define CAND_TILE (CAND_TILE_WORDS * 64)
static_assert(CAND_TILE == IGMC_CAND_TILE_ITEMS, "launch.h names the tile");
#define SEG_LDS_WORDS 4096                         // selection words a workgroup stages (32 KB); also 64 lists of 64 to merge
static_assert(IGMC_SEGSEL_MAX_SPLIT * IGMC_SELECT_MAX_NUM <= SEG_LDS_WORDS, "the merge stages every partial list");

template <int FILL>
__global__ __launch_bounds__(IGMC_BLOCK) void k_candidates(GraphDev g, const int32_t* __restrict__ users, int nq,
                                                           const uint8_t* __restrict__ item_ok, int exclude_seen,
                                                           int64_t* __restrict__ counts, const int64_t* __restrict__ off,
                                                           int32_t* __restrict__ link_u, int32_t* __restrict__ link_v,
                                                           int64_t capacity, int32_t* err) {
  __shared__ uint32_t bm[2 * CAND_TILE_WORDS];              // items of the tile the user rated
  __shared__ unsigned long long surv[CAND_TILE_WORDS];      // candidates of the tile
  __shared__ int woff[CAND_TILE_WORDS];
  __shared__ int smi[8];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nwave = IGMC_BLOCK >> 6;
  for (int q = blockIdx.x; q < nq; q += gridDim.x) {
    const int u = users[q];
    if (u < 0 || u >= g.n_users) {        // (uniform over the workgroup) no row is read; the segment is empty
      if (t == 0) {
        atomicOr(err, 2);
        if (!FILL) counts[q] = 0;
      }
      continue;
    }
    const int lo = exclude_seen ? g.u_ptr[u] : 0, hi = exclude_seen ? g.u_ptr[u + 1] : 0;
    const int64_t base = FILL ? off[q] : 0;
    int64_t end = FILL ? off[q + 1] : 0;
    if (end > capacity) end = capacity;
    int total = 0;
    for (int tile0 = 0; tile0 < g.n_items; tile0 += CAND_TILE) {
      const int left = g.n_items - tile0;
      const int nw = left >= CAND_TILE ? CAND_TILE_WORDS : (left + 63) >> 6;
      bm[2 * t] = 0u;
      bm[2 * t + 1] = 0u;
      __syncthreads();
      for (int p = lo + t; p < hi; p += IGMC_BLOCK) {
        const int v = g.u_idx[p] - tile0;
        if (v >= 0 && v < CAND_TILE) atomicOr(&bm[v >> 5], 1u << (v & 31));
      }
      __syncthreads();
      for (int w = wave; w < nw; w += nwave) {
        const int v = tile0 + w * 64 + lane;
        const bool keep = v < g.n_items && !((bm[2 * w + (lane >> 5)] >> (lane & 31)) & 1u) && (!item_ok || item_ok[v] != 0);
        const unsigned long long m = __ballot(keep);
        if (lane == 0) surv[w] = m;
      }
      __syncthreads();
      int tile_total;
      const int ex = igmc_block_scan_excl(t < nw ? __popcll(surv[t]) : 0, &tile_total, smi);
      if (FILL) {
        woff[t] = ex;
        __syncthreads();
        for (int w = wave; w < nw; w += nwave) {
          const unsigned long long m = surv[w];
          if ((m >> lane) & 1ull) {
            const int64_t pos = base + total + woff[w] + __popcll(m & ((1ull << lane) - 1ull));
            if (pos >= 0 && pos < end) {        // (what has no place is reported below, never written)
              link_u[pos] = u;
              link_v[pos] = tile0 + w * 64 + lane;
            }
          }
        }
      }
      total += tile_total;
      __syncthreads();
    }
    if (!FILL) {
      if (t == 0) counts[q] = total;
    } else {
      // bit 0: the segment reaches past `capacity` (nothing was written there); bit 2: the offsets are not the counts'
      const int bad = ((base + total > capacity) ? 1 : 0) | ((base < 0 || off[q + 1] - base != (int64_t)total) ? 4 : 0);
      if (t == 0 && bad) atomicOr(err, bad);
    }
  }
}

// min over the workgroup, result in every thread.  sm: 4 words of LDS.
__device__ __forceinline__ unsigned long long seg_block_min(unsigned long long lo, unsigned long long* sm) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long a = __shfl_xor(lo, d, 64);
    lo = a < lo ? a : lo;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) sm[wave] = lo;
  __syncthreads();
  const int nw = (blockDim.x + 63) >> 6;
  for (int w = 0; w < nw; ++w) lo = sm[w] < lo ? sm[w] : lo;
  __syncthreads();
  return lo;
}

// `num` rounds of "smallest word above the last one taken" over words 0 .. m-1 (st: staged in LDS, else load(i) every round);
// emit(r, word) in every thread, SEL_LOW_NONE once nothing is left
template <class Load, class Emit>
__device__ __forceinline__ void seg_rounds(int64_t m, const unsigned long long* st, Load load, int num,
                                           unsigned long long* sm, Emit emit) {
  unsigned long long last = SEL_HIGH_NONE;
  int r = 0;
  for (; r < num; ++r) {
    unsigned long long lo = SEL_LOW_NONE;
    if (st) {
      for (int i = threadIdx.x; i < (int)m; i += IGMC_BLOCK) {
        const unsigned long long w = st[i];
        if (w > last && w < lo) lo = w;
      }
    } else {
      for (int64_t i = threadIdx.x; i < m; i += IGMC_BLOCK) {
        const unsigned long long w = load(i);
        if (w > last && w < lo) lo = w;
      }
    }
    lo = seg_block_min(lo, sm);
    if (lo == SEL_LOW_NONE) break;        // (uniform: the minimum is in every thread)
    emit(r, lo);
    last = lo;
  }
  for (; r < num; ++r) emit(r, SEL_LOW_NONE);
}

// entry r of a segment's result from its word (thread 0)
__device__ __forceinline__ void seg_write(const float* __restrict__ keys, int64_t at, unsigned long long w,
                                          int32_t* __restrict__ idx_out, float* __restrict__ key_out) {
  const bool has = w != SEL_LOW_NONE;
  const uint32_t i = (uint32_t)(w & 0xFFFFFFFFull);
  idx_out[at] = has ? (int32_t)i : -1;
  if (key_out) key_out[at] = has ? keys[i] : 0.f;
}

__global__ __launch_bounds__(IGMC_BLOCK) void k_segsel_part(const float* __restrict__ keys, const int64_t* __restrict__ seg_off,
                                                            int ns, int num, int k, unsigned long long* __restrict__ part,
                                                            int32_t* __restrict__ idx_out, float* __restrict__ key_out,
                                                            int32_t* __restrict__ count) {
  __shared__ unsigned long long st[SEG_LDS_WORDS];
  __shared__ unsigned long long sm[4];
  const int64_t jobs = (int64_t)ns * k;
  for (int64_t job = blockIdx.x; job < jobs; job += gridDim.x) {
    const int64_t s = job / k;
    const int j = (int)(job - s * k);
    const int64_t lo = seg_off[s], hi = seg_off[s + 1];
    const int64_t len = hi > lo ? hi - lo : 0;
    const int64_t chunk = (len + k - 1) / k;
    const int64_t a = lo + j * chunk;
    int64_t m = (a + chunk < hi ? a + chunk : hi) - a;
    if (m < 0) m = 0;
    const bool staged = m <= SEG_LDS_WORDS;
    if (staged) {
      for (int i = threadIdx.x; i < (int)m; i += IGMC_BLOCK) st[i] = sel_word_desc(keys[a + i], (uint32_t)(a + i));
      __syncthreads();
    }
    seg_rounds(
        m, staged ? st : nullptr, [&](int64_t i) { return sel_word_desc(keys[a + i], (uint32_t)(a + i)); }, num, sm,
        [&](int r, unsigned long long w) {
          if (threadIdx.x == 0) {
            if (k == 1)
              seg_write(keys, s * num + r, w, idx_out, key_out);
            else
              part[job * num + r] = w;
          }
        });
    if (k == 1 && threadIdx.x == 0 && count) count[s] = (int32_t)(len < (int64_t)num ? len : (int64_t)num);
    __syncthreads();        // (the next job stages over st)
  }
}

// one workgroup per segment over its k partial lists (k * num <= SEG_LDS_WORDS words, staged)
__global__ __launch_bounds__(IGMC_BLOCK) void k_segsel_merge(const float* __restrict__ keys, const int64_t* __restrict__ seg_off,
                                                             int ns, int num, int k,
                                                             const unsigned long long* __restrict__ part,
                                                             int32_t* __restrict__ idx_out, float* __restrict__ key_out,
                                                             int32_t* __restrict__ count) {
  __shared__ unsigned long long st[SEG_LDS_WORDS];
  __shared__ unsigned long long sm[4];
  const int np = k * num;
  for (int64_t s = blockIdx.x; s < ns; s += gridDim.x) {
    for (int i = threadIdx.x; i < np; i += IGMC_BLOCK) st[i] = part[s * np + i];
    __syncthreads();
    seg_rounds(
        np, st, [&](int64_t i) { return st[i]; }, num, sm,
        [&](int r, unsigned long long w) {
          if (threadIdx.x == 0) seg_write(keys, s * num + r, w, idx_out, key_out);
        });
    if (threadIdx.x == 0 && count) {
      const int64_t len = seg_off[s + 1] - seg_off[s];
      count[s] = (int32_t)(len < 0 ? 0 : len < (int64_t)num ? len : (int64_t)num);
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ host
static int cand_grid(int64_t jobs) { return (int)(jobs < 1 ? 1 : jobs > 65536 ? 65536 : jobs); }

void igmc_launch_candidates_count(const GraphDev& g, const int32_t* users, int nq, const uint8_t* item_ok, int exclude_seen,
                                  int64_t* counts, int32_t* err, void* stream) {
  IGMC_PLAUNCH("k_candidates_count", k_candidates<0>, cand_grid(nq), IGMC_BLOCK, 0, stream, g, users, nq, item_ok,
               exclude_seen, counts, (const int64_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (int64_t)0, err);
}

void igmc_launch_candidates_fill(const GraphDev& g, const int32_t* users, int nq, const uint8_t* item_ok, int exclude_seen,
                                 const int64_t* off, int32_t* link_u, int32_t* link_v, int64_t capacity, int32_t* err,
                                 void* stream) {
  IGMC_PLAUNCH("k_candidates_fill", k_candidates<1>, cand_grid(nq), IGMC_BLOCK, 0, stream, g, users, nq, item_ok,
               exclude_seen, (int64_t*)nullptr, off, link_u, link_v, capacity, err);
}

// workgroups per segment where the caller names none.  The segments' lengths are on the device only, so the choice is made
// from their NUMBER: few segments (a handful of users, possibly 10^5..10^6 items each) are split until the grid has about
// two workgroups per CU; from 257 segments on every segment is one workgroup and the launch is the only one.
int igmc_segsel_default_split(int ns) {
  const int k = 512 / (ns < 1 ? 1 : ns);
  return k < 1 ? 1 : k > IGMC_SEGSEL_MAX_SPLIT ? IGMC_SEGSEL_MAX_SPLIT : k;
}

void igmc_launch_select_segments(const float* keys, const int64_t* seg_off, int ns, int num, int k, void* scratch,
                                 int32_t* idx_out, float* key_out, int32_t* count, void* stream) {
  unsigned long long* part = (unsigned long long*)scratch;
  IGMC_PLAUNCH("k_segsel_part", k_segsel_part, cand_grid((int64_t)ns * k), IGMC_BLOCK, 0, stream, keys, seg_off, ns, num, k,
               part, idx_out, key_out, count);
  if (k > 1)
    IGMC_PLAUNCH("k_segsel_merge", k_segsel_merge, cand_grid(ns), IGMC_BLOCK, 0, stream, keys, seg_off, ns, num, k,
                 (const unsigned long long*)part, idx_out, key_out, count);
}
