// sampled_candidates.hip -- the candidate segment of a user cut down to K SAMPLED negatives, written straight into device link
// arrays (no reference counterpart: the reference stops at the test RMSE; the sampled ranking protocol of the top-N literature
// -- every held-out item ranked among K uniformly drawn unseen items -- would be a host loop of random.sample over the
// complement of every user's row there).
//
// THE SEGMENT of request q (user u = users[q]), igmc_hip.h states it for callers:
//   C = the candidates of k_candidates (candidates.hip): items in range, not in the user's row (exclude_seen), item_ok
//   M = the must items of the request, must_item[must_off[q] .. must_off[q + 1])      (any order, duplicates allowed)
//   N = C \ M, the negatives' pool;  S = the min(k, |N|) items of N with the smallest igmc_sample_key(salt, item),
//       salt = igmc_negative_salt(seed, draw, u) -- keyed by the user ID, so S does not depend on q, on the users that share
//       the launch or on the grid
//   segment = (M n C) u S, item ascending; forced[pos] = 1 where the item is of M.
//
// k_sampled_candidates<0>  per-user counts |M n C| + min(k, |N|) (no key is computed); <1> the links, at offsets the caller
//                  derived from the counts.  One workgroup per requested user (grid-stride), as k_candidates: the row and the
//                  must list are MARKED into two LDS bitmaps over a tile of CAND_TILE items, wave w takes the 64-item words
//                  w, w + 4, ..: a lane per item, pool and forced items as ballots.  The threshold T = the k-th smallest key
//                  of the pool: one histogram walk over the keys' top byte finds the byte b that holds it, the keys OF b
//                  (|N| / 256 on average) are parked in a short list and the r-th of them is found by counting; a byte with
//                  more keys than the list holds goes through the remaining three radix passes instead.  Keys are a
//                  bijection of the id (igmc_rng.h): exactly k keys are <= T either way.  The emission then keeps pool items
//                  with key <= T and every forced item, placed by a block scan of the words' popcounts + the popcount of
//                  the ballot below the lane: the order is a function of the inputs alone.
//                  Graphs wider than a tile (the definition knows no tiles): every walk -- count, histogram, parking, radix
//                  passes, emission -- goes over the tiles one after the other and rebuilds the tile's ballots; a graph of
//                  one tile (every bundled dataset, ml_10m) builds them once.
// Plain vector stores only; the atomics are LDS bit-sets, LDS histogram / list-cursor adds and the error word's OR.
#include "launch.h"

#define SC_TILE_WORDS IGMC_BLOCK                   // 64-item words of a bitmap tile: one per thread of the scan
#define SC_TILE (SC_TILE_WORDS * 64)
static_assert(SC_TILE == IGMC_CAND_TILE_ITEMS, "launch.h names the tile");

#ifdef IGMC_HIPEMU
// (CPU emulation only: the tests lower the bound through the environment to drive the four-pass path)
static inline int sc_park() { const char* e = getenv("IGMC_SAMPLE_PARK"); return e ? atoi(e) : IGMC_BLOCK; }
#define SC_PARK sc_park()
#else
#define SC_PARK IGMC_BLOCK
#endif

struct SampledArgs {
  GraphDev g;
  const int32_t* users;
  int nq;
  const uint8_t* item_ok;
  int exclude_seen;
  const int64_t* must_off;      // null: no request has must items
  const int32_t* must_item;
  int64_t n_must;
  int k;
  uint64_t seed, draw;
  int64_t* counts;              // <0>
  const int64_t* off;           // <1>
  int32_t* link_u;
  int32_t* link_v;
  uint8_t* forced;              // may be null
  int64_t capacity;
  int32_t* err;
};

// LDS of one workgroup
struct SampledLds {
  uint32_t row[2 * SC_TILE_WORDS];                 // items of the tile the user rated
  uint32_t must[2 * SC_TILE_WORDS];                // must items of the tile
  unsigned long long pool[SC_TILE_WORDS];          // N of the tile; the emission overwrites it with the words it writes
  unsigned long long forc[SC_TILE_WORDS];          // M n C of the tile
  int woff[SC_TILE_WORDS];
  int hist[IGMC_BLOCK];
  uint32_t ckey[IGMC_BLOCK];                       // parked keys of the deciding byte
  int smi[16];
};

// pool / forc of the tile at tile0 (nw words).  report: a must item outside [0, n_items) raises bit 3 (first walk only)
__device__ __forceinline__ void sc_build_tile(const SampledArgs& a, SampledLds& s, int u, int lo, int hi, int64_t mo, int64_t me,
                                              int tile0, int nw, bool report) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nwave = IGMC_BLOCK >> 6;
  s.row[2 * t] = s.row[2 * t + 1] = 0u;
  s.must[2 * t] = s.must[2 * t + 1] = 0u;
  __syncthreads();
  for (int p = lo + t; p < hi; p += IGMC_BLOCK) {
    const int v = a.g.u_idx[p] - tile0;
    if (v >= 0 && v < SC_TILE) atomicOr(&s.row[v >> 5], 1u << (v & 31));
  }
  for (int64_t p = mo + t; p < me; p += IGMC_BLOCK) {
    const int id = a.must_item[p];
    if (id < 0 || id >= a.g.n_items) {        // ignored and reported
      if (report) atomicOr(a.err, 8);
      continue;
    }
    const int v = id - tile0;
    if (v >= 0 && v < SC_TILE) atomicOr(&s.must[v >> 5], 1u << (v & 31));
  }
  __syncthreads();
  for (int w = wave; w < nw; w += nwave) {
    const int v = tile0 + w * 64 + lane;
    const int h = 2 * w + (lane >> 5), bit = lane & 31;
    const bool cand = v < a.g.n_items && !((s.row[h] >> bit) & 1u) && (!a.item_ok || a.item_ok[v] != 0);
    const unsigned long long c = __ballot(cand), m = __ballot(cand && ((s.must[h] >> bit) & 1u));
    if (lane == 0) {
      s.pool[w] = c & ~m;
      s.forc[w] = m;
    }
  }
  __syncthreads();
}

template <int FILL>
__global__ __launch_bounds__(IGMC_BLOCK) void k_sampled_candidates(SampledArgs a) {
  __shared__ SampledLds s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nwave = IGMC_BLOCK >> 6;
  const int n_items = a.g.n_items;
  const bool one_tile = n_items <= SC_TILE;
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
    if (a.must_off) {
      mo = a.must_off[q];
      me = a.must_off[q + 1];
      if (mo < 0 || me < mo || me > a.n_must) {        // not followed: the must list is empty
        if (t == 0) atomicOr(a.err, 16);
        mo = me = 0;
      }
    }
    // every walk: the tiles one after the other, their ballots rebuilt unless the graph is one tile (built by the first walk)
    bool built = false;
    auto tiles = [&](auto&& body) {
      for (int tile0 = 0; tile0 < n_items; tile0 += SC_TILE) {
        const int left = n_items - tile0;
        const int nw = left >= SC_TILE ? SC_TILE_WORDS : (left + 63) >> 6;
        if (!(one_tile && built)) sc_build_tile(a, s, u, lo, hi, mo, me, tile0, nw, !built);
        body(tile0, nw);
      }
      built = true;
    };
    // keys of the pool items of a tile, a lane per item
    auto keys = [&](int tile0, int nw, uint64_t salt, auto&& f) {
      for (int w = wave; w < nw; w += nwave)
        if ((s.pool[w] >> lane) & 1ull) f(igmc_sample_key(salt, (uint32_t)(tile0 + w * 64 + lane)));
    };

    // ---- walk 1: |N| and |M n C|
    int n_pool = 0, n_forc = 0;
    tiles([&](int, int nw) {
      int tp, tf;
      igmc_block_scan_excl(t < nw ? __popcll(s.pool[t]) : 0, &tp, s.smi);
      igmc_block_scan_excl(t < nw ? __popcll(s.forc[t]) : 0, &tf, s.smi);
      n_pool += tp;
      n_forc += tf;
    });
    const int kk = a.k < n_pool ? a.k : n_pool;
    const int total = n_forc + kk;
    if (!FILL) {
      if (t == 0) a.counts[q] = total;
      __syncthreads();        // (the next request builds over the tile)
      continue;
    }

    // ---- the threshold: kk in (0, |N|) only -- nothing or everything of the pool otherwise
    uint32_t T = 0u;
    const bool by_key = kk > 0 && kk < n_pool;
    const uint64_t salt = igmc_negative_salt(a.seed, a.draw, (uint64_t)(uint32_t)u);
    if (by_key) {
      s.hist[t] = 0;
      __syncthreads();
      tiles([&](int tile0, int nw) {
        keys(tile0, nw, salt, [&](uint32_t key) { atomicAdd(&s.hist[key >> 24], 1); });
        __syncthreads();
      });
      int tot;
      int c = s.hist[t];
      int ex = igmc_block_scan_excl(c, &tot, s.smi);
      if (c > 0 && ex < kk && kk <= ex + c) {
        s.smi[8] = t;
        s.smi[9] = kk - ex;
        s.smi[10] = c;
      }
      if (t == 0) s.smi[11] = 0;
      __syncthreads();
      const uint32_t b = (uint32_t)s.smi[8];
      int r = s.smi[9];
      const int cb = s.smi[10];
      __syncthreads();
      if (cb <= SC_PARK) {
        tiles([&](int tile0, int nw) {
          keys(tile0, nw, salt, [&](uint32_t key) {
            if ((key >> 24) == b) s.ckey[atomicAdd(&s.smi[11], 1)] = key;
          });
          __syncthreads();
        });
        if (t < cb) {
          const uint32_t mine = s.ckey[t];
          int below = 0;
          for (int j = 0; j < cb; ++j) below += s.ckey[j] < mine;
          if (below == r - 1) s.smi[12] = (int)mine;        // (keys never tie: one thread)
        }
        __syncthreads();
        T = (uint32_t)s.smi[12];
      } else {
        uint32_t prefix = b << 24, mask = 0xFF000000u;
        for (int pass = 2; pass >= 0; --pass) {
          const int shift = pass * 8;
          s.hist[t] = 0;
          __syncthreads();
          tiles([&](int tile0, int nw) {
            keys(tile0, nw, salt, [&](uint32_t key) {
              if ((key & mask) == prefix) atomicAdd(&s.hist[(key >> shift) & 255u], 1);
            });
            __syncthreads();
          });
          c = s.hist[t];
          ex = igmc_block_scan_excl(c, &tot, s.smi);
          if (c > 0 && ex < r && r <= ex + c) {
            s.smi[8] = t;
            s.smi[9] = r - ex;
          }
          __syncthreads();
          prefix |= ((uint32_t)s.smi[8]) << shift;
          mask |= 0xFFu << shift;
          r = s.smi[9];
          __syncthreads();
        }
        T = prefix;
      }
    }
    // ---- the emission: the pool items with key <= T (kk == |N|: all of them, kk == 0: none) and the forced ones
    const bool all = kk == n_pool;
    const int64_t base = a.off[q];
    int64_t end = a.off[q + 1];
    if (end > a.capacity) end = a.capacity;
    int done = 0;
    tiles([&](int tile0, int nw) {
      for (int w = wave; w < nw; w += nwave) {
        const bool in = (s.pool[w] >> lane) & 1ull;
        const unsigned long long m =
            __ballot(in && (all || (by_key && igmc_sample_key(salt, (uint32_t)(tile0 + w * 64 + lane)) <= T)));
        if (lane == 0) s.pool[w] = m | s.forc[w];
      }
      __syncthreads();
      int tile_total;
      s.woff[t] = igmc_block_scan_excl(t < nw ? __popcll(s.pool[t]) : 0, &tile_total, s.smi);
      __syncthreads();
      for (int w = wave; w < nw; w += nwave) {
        const unsigned long long m = s.pool[w];
        if ((m >> lane) & 1ull) {
          const int64_t pos = base + done + s.woff[w] + __popcll(m & ((1ull << lane) - 1ull));
          if (pos >= 0 && pos < end) {        // (what has no place is reported below, never written)
            a.link_u[pos] = u;
            a.link_v[pos] = tile0 + w * 64 + lane;
            if (a.forced) a.forced[pos] = (uint8_t)((s.forc[w] >> lane) & 1ull);
          }
        }
      }
      done += tile_total;
      __syncthreads();
    });
    // bit 0: the segment reaches past `capacity` (nothing was written there); bit 2: the offsets are not the counts'
    const int bad = ((base + total > a.capacity) ? 1 : 0) | ((base < 0 || a.off[q + 1] - base != (int64_t)total) ? 4 : 0);
    if (t == 0 && bad) atomicOr(a.err, bad);
  }
}

// ------------------------------------------------------------------ host
static int sampled_grid(int64_t jobs) { return (int)(jobs < 1 ? 1 : jobs > 65536 ? 65536 : jobs); }

void igmc_launch_sampled_count(const GraphDev& g, const int32_t* users, int nq, const uint8_t* item_ok, int exclude_seen,
                               const int64_t* must_off, const int32_t* must_item, int64_t n_must, int k, int64_t* counts,
                               int32_t* err, void* stream) {
  const SampledArgs a = {g, users, nq, item_ok, exclude_seen, must_off, must_item, n_must, k, 0, 0, counts, nullptr, nullptr,
                         nullptr, nullptr, 0, err};
  IGMC_PLAUNCH("k_sampled_candidates_count", k_sampled_candidates<0>, sampled_grid(nq), IGMC_BLOCK, 0, stream, a);
}

void igmc_launch_sampled_fill(const GraphDev& g, const int32_t* users, int nq, const uint8_t* item_ok, int exclude_seen,
                              const int64_t* must_off, const int32_t* must_item, int64_t n_must, int k, uint64_t seed,
                              uint64_t draw, const int64_t* off, int32_t* link_u, int32_t* link_v, uint8_t* forced,
                              int64_t capacity, int32_t* err, void* stream) {
  const SampledArgs a = {g, users, nq, item_ok, exclude_seen, must_off, must_item, n_must, k, seed, draw, nullptr, off, link_u,
                         link_v, forced, capacity, err};
  IGMC_PLAUNCH("k_sampled_candidates_fill", k_sampled_candidates<1>, sampled_grid(nq), IGMC_BLOCK, 0, stream, a);
}
