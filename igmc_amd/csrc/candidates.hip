// candidates.hip -- what surrounds a scoring pass over links NOBODY RATED: the candidate links of a set of users written straight
// into device link arrays -- all of them, or cut down to K SAMPLED negatives --, and the `num` best of every user's score segment
// (no reference counterpart: the reference stops at the test RMSE; a top-N list there would be a host loop over the complement
// of every user's row and a host argsort of its scores, the sampled ranking protocol of the top-N literature -- every held-out
// item ranked among K uniformly drawn unseen items -- a host loop of random.sample over that complement).
//
// THE SEGMENT of request q (user u = users[q]), igmc_hip.h states it for callers:
//   C = the candidates: items in range, not in the user's row (exclude_seen), item_ok      -- cand_build_tile, the ONE definition
//   exhaustive: segment = C, item ascending.
//   sampled:    M = the must items of the request, must_item[must_off[q] .. must_off[q + 1])  (any order, duplicates allowed)
//               N = C \ M, the negatives' pool;  S = the min(k, |N|) items of N with the smallest igmc_sample_key(salt, item),
//               salt = igmc_negative_salt(seed, draw, u) -- keyed by the user ID, so S does not depend on q, on the users that
//               share the launch or on the grid
//               segment = (M n C) u S, item ascending; forced[pos] = 1 where the item is of M.
//
// k_candidates<FILL, SAMPLED>  <0, .> per-user counts (|C|, or |M n C| + min(k, |N|): no key is computed); <1, .> the links, at
//                  offsets the caller derived from the counts.  One workgroup per requested user (grid-stride).  The user's row
//                  -- sorted by (relation, item), so not searchable -- and, sampled, the must list are MARKED into LDS bitmaps
//                  over a tile of CAND_TILE items; wave w then takes the 64-item words w, w + 4, ...: a lane per item, pool
//                  and forced items as ballots; the word's place in the segment is a block scan of the words' popcounts, a
//                  lane's place in its word the popcount of the ballot below it.  Output order = (users as given, item
//                  ascending), a function of the inputs alone: the atomics are LDS bit-sets, which commute, and -- sampled
//                  -- LDS histogram / list-cursor adds.
//                  SAMPLED = false compiles the must bitmap, the forced ballots and every key out: the count is one walk,
//                  the fill is one walk (the emission; it learns the segment's total there).
//                  SAMPLED = true, the fill: the threshold T = the k-th smallest key of the pool (kth_key.h's steps, shared with
//                  the extraction's per-hop cap and the shortlist's vote order): one histogram walk over the
//                  keys' top byte finds the byte b that holds it, the keys OF b (|N| / 256 on average) are parked in a short
//                  list and the r-th of them is found by counting; a byte with more keys than the list holds goes through
//                  the remaining three radix passes instead.  Keys are a bijection of the id (igmc_rng.h): exactly k keys
//                  are <= T either way.  The emission then keeps pool items with key <= T and every forced item.
//                  Graphs wider than a tile (the definition knows no tiles): every walk -- count, histogram, parking, radix
//                  passes, emission -- goes over the tiles one after the other and rebuilds the tile's ballots, the row
//                  walked once per tile; a graph of one tile (every bundled dataset, ml_10m) builds them once per request.
// k_segsel_part    workgroup (s, j) reduces slice j of the k contiguous slices of segment s to its `num` first words -- staged
// k_segsel_merge   in LDS when the slice fits --; k == 1 writes the segment's result itself, k > 1 leaves partial lists that
//                  one workgroup per segment merges.
//
// THE ORDER of a segment (igmc_hip.h states it for callers): (key descending, index ascending), every NaN behind every number,
// -0.0 == 0.0 -- np.lexsort((idx, np.where(np.isnan(k), 0, -k), np.isnan(k))); the two-key np.lexsort((idx, np.where(np.isnan(k),
// np.inf, -k))) is that order only for segments without a -inf key.  A key and its GLOBAL position travel as one 64-bit
// word (select.h: sel_word_desc), the order is "word ascending", words are distinct: the lists do not depend on k.
// Plain vector stores only (error words: a vector atomic OR, reached on errors only).
#include "capi.h"
#include "select.h"
#include "cand_tile.h"      // CAND_TILE, CandLds, cand_build_tile: the one definition of C; CandTiles, cand_place_tile
#include "kth_key.h"        // the k-th smallest key of the pool

#define SEG_LDS_WORDS 4096                         // selection words a workgroup stages (32 KB); also 64 lists of 64 to merge
static_assert(IGMC_SEGSEL_MAX_SPLIT * IGMC_SELECT_MAX_NUM <= SEG_LDS_WORDS, "the merge stages every partial list");

template <bool FILL, bool SAMPLED>
__global__ __launch_bounds__(IGMC_BLOCK) void k_candidates(CandArgs a) {
  __shared__ CandLds<SAMPLED> s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nwave = IGMC_BLOCK >> 6;
  for (int q = blockIdx.x; q < a.nq; q += gridDim.x) {
    const int u = a.users[q];
    if (u < 0 || u >= a.g.n_users) {        // (uniform over the workgroup) no row is read; the segment is empty
      if (t == 0) {
        atomicOr(a.err, 2);
        if (!FILL) a.counts[q] = 0;
      }
      continue;
    }
    const int lo = a.exclude_seen ? a.g.u_ptr[u] : 0, hi = a.exclude_seen ? a.g.u_ptr[u + 1] : 0;
    int64_t mo = 0, me = 0;
    if constexpr (SAMPLED) {
      if (a.must_off) {
        mo = a.must_off[q];
        me = a.must_off[q + 1];
        if (mo < 0 || me < mo || me > a.n_must) {        // not followed: the must list is empty
          if (t == 0) atomicOr(a.err, 16);
          mo = me = 0;
        }
      }
    }
    CandTiles<SAMPLED> tiles{a, s, lo, hi, mo, me, true};        // every walk below

    // ---- walk 1: |N| and |M n C|.  Not for the exhaustive fill: its emission is its only walk
    int n_pool = 0, n_forc = 0;
    if constexpr (SAMPLED || !FILL) {
      tiles([&](int, int nw) {
        int tp;
        igmc_block_scan_excl(t < nw ? __popcll(s.pool[t]) : 0, &tp, s.smi);
        n_pool += tp;
        if constexpr (SAMPLED) {
          int tf;
          igmc_block_scan_excl(t < nw ? __popcll(s.forc[t]) : 0, &tf, s.smi);
          n_forc += tf;
        }
      });
    }
    const int kk = SAMPLED && a.k < n_pool ? a.k : n_pool;
    int total = n_forc + kk;
    if constexpr (!FILL) {
      if (t == 0) a.counts[q] = total;
      __syncthreads();        // (the next request builds over the tile)
    } else {
      // ---- sampled: the threshold, for kk in (0, |N|) only -- nothing or everything of the pool otherwise
      uint32_t T = 0u;
      uint64_t salt = 0;
      bool by_key = false, all = true;
      if constexpr (SAMPLED) {
        // f(key) for the pool items, a lane per item (a key walk reads the pool alone, which a tile rebuild writes behind its
        // own barriers: no barrier per tile)
        auto walk = [&](auto&& f) {
          tiles([&](int tile0, int nw) {
            for (int w = wave; w < nw; w += nwave)
              if ((s.pool[w] >> lane) & 1ull) f(igmc_sample_key(salt, (uint32_t)(tile0 + w * 64 + lane)));
          });
        };
        by_key = kk > 0 && kk < n_pool;
        all = kk == n_pool;
        salt = igmc_negative_salt(a.seed, a.draw, (uint64_t)(uint32_t)u);
        if (by_key) {
          const KthBin top = kth_pass(walk, 0u, 0u, 24, kk, s.hist, s.smi);
          if (kth_parks(top.c)) {
            walk([&](uint32_t key) {
              if ((key >> 24) == top.b) s.ckey[atomicAdd(&s.smi[KTH_SM_CURSOR], 1)] = key;
            });
            __syncthreads();
            if (t < top.c && kth_parked_below(s.ckey, top.c) == top.r - 1) s.smi[KTH_SM_T] = (int)s.ckey[t];        // (one thread)
            __syncthreads();
            T = (uint32_t)s.smi[KTH_SM_T];
          } else {
            int r = top.r;
            T = kth_radix(walk, top.b << 24, 0xFF000000u, 2, r, s.hist, s.smi);
          }
        }
      }
      // ---- the emission: every pool item -- sampled: those with key <= T (kk == |N|: all of them, kk == 0: none) and the
      // forced ones
      const int64_t base = a.off[q];
      int64_t end = a.off[q + 1];
      if (end > a.capacity) end = a.capacity;
      int done = 0;
      tiles([&](int tile0, int nw) {
        if constexpr (SAMPLED) {
          for (int w = wave; w < nw; w += nwave) {
            const bool in = (s.pool[w] >> lane) & 1ull;
            const unsigned long long m =
                __ballot(in && (all || (by_key && igmc_sample_key(salt, (uint32_t)(tile0 + w * 64 + lane)) <= T)));
            if (lane == 0) s.pool[w] = m | s.forc[w];
          }
          __syncthreads();
        }
        done += cand_place_tile(s, tile0, nw, base, done, end, [&](int64_t pos, int item, int w, int ln) {
          a.link_u[pos] = u;
          a.link_v[pos] = item;
          if constexpr (SAMPLED)
            if (a.forced) a.forced[pos] = (uint8_t)((s.forc[w] >> ln) & 1ull);
        });
      });
      if constexpr (!SAMPLED) total = done;        // (the exhaustive fill took no count walk)
      // bit 0: the segment reaches past `capacity` (nothing was written there); bit 2: the offsets are not the counts'
      const int bad = ((base + total > a.capacity) ? 1 : 0) | ((base < 0 || a.off[q + 1] - base != (int64_t)total) ? 4 : 0);
      if (t == 0 && bad) atomicOr(a.err, bad);
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

static void igmc_launch_candidates(const CandArgs& a, int fill, int sampled, void* stream) {
  static const char* const names[2][2] = {{"k_candidates_count", "k_candidates_fill"},
                                          {"k_sampled_candidates_count", "k_sampled_candidates_fill"}};
  igmc_dispatch(
      [&](auto fl, auto sa) {
        IGMC_PLAUNCH(names[sa()][fl()], (k_candidates<fl(), sa()>), cand_grid(a.nq), IGMC_BLOCK, 0, stream, a);
      },
      fill != 0, sampled != 0);
}

// workgroups per segment where the caller names none.  The segments' lengths are on the device only, so the choice is made
// from their NUMBER: few segments (a handful of users, possibly 10^5..10^6 items each) are split until the grid has about
// two workgroups per CU; from 257 segments on every segment is one workgroup and the launch is the only one.
int igmc_segsel_default_split(int ns) {
  const int k = 512 / (ns < 1 ? 1 : ns);
  return k < 1 ? 1 : k > IGMC_SEGSEL_MAX_SPLIT ? IGMC_SEGSEL_MAX_SPLIT : k;
}

static void igmc_launch_select_segments(const float* keys, const int64_t* seg_off, int ns, int num, int k, void* scratch,
                                 int32_t* idx_out, float* key_out, int32_t* count, void* stream) {
  unsigned long long* part = (unsigned long long*)scratch;
  IGMC_PLAUNCH("k_segsel_part", k_segsel_part, cand_grid((int64_t)ns * k), IGMC_BLOCK, 0, stream, keys, seg_off, ns, num, k,
               part, idx_out, key_out, count);
  if (k > 1)
    IGMC_PLAUNCH("k_segsel_merge", k_segsel_merge, cand_grid(ns), IGMC_BLOCK, 0, stream, keys, seg_off, ns, num, k,
                 (const unsigned long long*)part, idx_out, key_out, count);
}

// ------------------------------------------------------------------ C ABI
// The four entry points -- every candidate, or (sample) cut down to k sampled negatives + the must items of every request --
// fill ONE argument block: cand_args checks and files what all four take (the exhaustive pair: no must list, k = 0),
// cand_fill_args what the two fills add.  Either returns the refusal, or null.
static const char* cand_args(CandArgs* a, const igmc_graph* g, const int32_t* d_users, int nq, const uint8_t* d_item_ok,
                             int exclude_seen, const int64_t* d_must_off, const int32_t* d_must_item, int64_t n_must, int64_t k,
                             int32_t* d_err) {
  if (!g || !d_users || !d_err) return "null argument";
  if (nq < 1) return "nq must be at least 1";
  if (k < 0 || k > (int64_t)INT32_MAX) return "k must be in [0, 2^31)";
  if (n_must < 0 || n_must > (int64_t)INT32_MAX) return "n_must must be in [0, 2^31)";
  if (d_must_off && n_must > 0 && !d_must_item) return "null argument";
  *a = CandArgs{g->d, d_users, nq, d_item_ok, exclude_seen != 0, d_must_off, d_must_item, n_must, (int)k};
  a->err = d_err;
  return nullptr;
}
static const char* cand_fill_args(CandArgs* a, const int64_t* d_offsets, int32_t* d_link_u, int32_t* d_link_v,
                                  int64_t capacity) {
  if (!d_offsets || !d_link_u || !d_link_v) return "null argument";
  if (capacity < 1 || capacity > (int64_t)INT32_MAX) return "capacity must be in [1, 2^31)";
  a->off = d_offsets;
  a->link_u = d_link_u;
  a->link_v = d_link_v;
  a->capacity = capacity;
  return nullptr;
}
extern "C" int igmc_candidates_count(const igmc_graph* g, const int32_t* d_users, int nq, const uint8_t* d_item_ok,
                                     int exclude_seen, int64_t* d_counts, int32_t* d_err, void* stream) {
  CandArgs a;
  const char* bad = cand_args(&a, g, d_users, nq, d_item_ok, exclude_seen, nullptr, nullptr, 0, 0, d_err);
  if (bad) IGMC_FAIL(bad);
  if (!d_counts) IGMC_FAIL("null argument");
  a.counts = d_counts;
  igmc_launch_candidates(a, 0, 0, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
extern "C" int igmc_candidates_fill(const igmc_graph* g, const int32_t* d_users, int nq, const uint8_t* d_item_ok,
                                    int exclude_seen, const int64_t* d_offsets, int32_t* d_link_u, int32_t* d_link_v,
                                    int64_t capacity, int32_t* d_err, void* stream) {
  CandArgs a;
  const char* bad = cand_args(&a, g, d_users, nq, d_item_ok, exclude_seen, nullptr, nullptr, 0, 0, d_err);
  if (!bad) bad = cand_fill_args(&a, d_offsets, d_link_u, d_link_v, capacity);
  if (bad) IGMC_FAIL(bad);
  igmc_launch_candidates(a, 1, 0, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
extern "C" int igmc_candidates_sample_count(const igmc_graph* g, const int32_t* d_users, int nq, const uint8_t* d_item_ok,
                                            int exclude_seen, const int64_t* d_must_off, const int32_t* d_must_item,
                                            int64_t n_must, int64_t k, int64_t* d_counts, int32_t* d_err, void* stream) {
  CandArgs a;
  const char* bad = cand_args(&a, g, d_users, nq, d_item_ok, exclude_seen, d_must_off, d_must_item, n_must, k, d_err);
  if (bad) IGMC_FAIL(bad);
  if (!d_counts) IGMC_FAIL("null argument");
  a.counts = d_counts;
  igmc_launch_candidates(a, 0, 1, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
extern "C" int igmc_candidates_sample_fill(const igmc_graph* g, const int32_t* d_users, int nq, const uint8_t* d_item_ok,
                                           int exclude_seen, const int64_t* d_must_off, const int32_t* d_must_item,
                                           int64_t n_must, int64_t k, uint64_t seed, uint64_t draw, const int64_t* d_offsets,
                                           int32_t* d_link_u, int32_t* d_link_v, uint8_t* d_forced, int64_t capacity,
                                           int32_t* d_err, void* stream) {
  CandArgs a;
  const char* bad = cand_args(&a, g, d_users, nq, d_item_ok, exclude_seen, d_must_off, d_must_item, n_must, k, d_err);
  if (!bad) bad = cand_fill_args(&a, d_offsets, d_link_u, d_link_v, capacity);
  if (bad) IGMC_FAIL(bad);
  a.seed = seed;
  a.draw = draw;
  a.forced = d_forced;
  igmc_launch_candidates(a, 1, 1, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}

static int segsel_split(int ns, int num, int geometry) {
  if (ns < 1 || num < 1 || num > IGMC_SELECT_MAX_NUM || geometry < 0 || geometry > IGMC_SEGSEL_MAX_SPLIT) return -1;
  return geometry > 0 ? geometry : igmc_segsel_default_split(ns);
}
static int64_t segsel_bytes(int ns, int num, int k) {      // (one workgroup per segment writes the result itself: a token word)
  return k > 1 ? (int64_t)ns * k * num * (int64_t)sizeof(uint64_t) : (int64_t)sizeof(uint64_t);
}
extern "C" int64_t igmc_select_segments_scratch_bytes(int ns, int num, int geometry) {
  const int k = segsel_split(ns, num, geometry);
  if (k < 0) {
    igmc_err() = std::string(__func__) + ": ns must be at least 1, num in [1, 64], geometry in [0, 64]";
    return -1;
  }
  return segsel_bytes(ns, num, k);
}
extern "C" int igmc_select_segments(const float* d_keys, const int64_t* d_seg_off, int ns, int num, int32_t* d_idx_out,
                                    float* d_key_out, int32_t* d_count, void* d_scratch, int64_t scratch_bytes, int geometry,
                                    void* stream) {
  if (!d_keys || !d_seg_off || !d_idx_out || !d_count || !d_scratch) IGMC_FAIL("null argument");
  const int k = segsel_split(ns, num, geometry);
  if (k < 0) IGMC_FAIL("ns must be at least 1, num in [1, 64], geometry in [0, 64]");
  if (scratch_bytes < segsel_bytes(ns, num, k)) IGMC_FAIL("scratch too small (igmc_select_segments_scratch_bytes)");
  if (((uintptr_t)d_scratch & 7) != 0) IGMC_FAIL("scratch must be 8-byte aligned");
  igmc_launch_select_segments(d_keys, d_seg_off, ns, num, k, d_scratch, d_idx_out, d_key_out, d_count, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
