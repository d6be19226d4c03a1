// cand_tile.h -- THE definition of a user's candidates C (items in range, not in the user's row where exclude_seen, item_ok),
// as LDS ballots over a tile of items: shared by candidates.hip (the exhaustive and the sampled lists) and shortlist.hip (the
// co-rating shortlist), so that the three kinds of segment can never disagree about what a candidate is -- nor, with the tile
// walk (CandTiles) and the placement (cand_place_tile) below, about where it lands in its segment.
#pragma once
#include "launch.h"

#define IGMC_CAND_TILE_ITEMS 16384      // items of one LDS bitmap tile of the enumeration (wider graphs: tile after tile)
#define CAND_TILE_WORDS IGMC_BLOCK                 // 64-item words of a bitmap tile: one per thread of the scan
#define CAND_TILE (CAND_TILE_WORDS * 64)
static_assert(CAND_TILE == IGMC_CAND_TILE_ITEMS, "the tile is named in items");

// the argument block of k_candidates (candidates.hip); the tile build reads its graph, item_ok, must list and error word, which
// is all that shortlist.hip fills in
struct CandArgs {
  GraphDev g;
  const int32_t* users;
  int nq;
  const uint8_t* item_ok;
  int exclude_seen;
  const int64_t* must_off;      // sampled; null: no request has must items
  const int32_t* must_item;
  int64_t n_must;
  int k;
  uint64_t seed, draw;          // sampled fill
  int64_t* counts;              // count
  const int64_t* off;           // fill
  int32_t* link_u;
  int32_t* link_v;
  uint8_t* forced;              // sampled fill; may be null
  int64_t capacity;
  int32_t* err;
};

// LDS of one workgroup: the must bitmap, the forced ballots, the histogram and the parked keys exist in the SAMPLED
// instantiations alone (members in this order: the sampled fill's register count depends on it)
template <bool SAMPLED>
struct CandLds;
template <>
struct CandLds<false> {
  uint32_t row[2 * CAND_TILE_WORDS];               // items of the tile the user rated
  unsigned long long pool[CAND_TILE_WORDS];        // C of the tile
  int woff[CAND_TILE_WORDS];
  int smi[16];
};
template <>
struct CandLds<true> {
  uint32_t row[2 * CAND_TILE_WORDS];
  uint32_t must[2 * CAND_TILE_WORDS];              // must items of the tile
  unsigned long long pool[CAND_TILE_WORDS];        // N of the tile; the emission overwrites it with the words it writes
  unsigned long long forc[CAND_TILE_WORDS];        // M n C of the tile
  int woff[CAND_TILE_WORDS];
  int hist[IGMC_BLOCK];
  uint32_t ckey[IGMC_BLOCK];                       // parked keys of the deciding byte
  int smi[16];
};

// pool (and forc) of the tile at tile0 (nw words).  report: a must item outside [0, n_items) raises bit 3 (first walk only)
template <bool SAMPLED>
__device__ __forceinline__ void cand_build_tile(const CandArgs& a, CandLds<SAMPLED>& s, int lo, int hi, int64_t mo, int64_t me,
                                                int tile0, int nw, bool report) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nwave = IGMC_BLOCK >> 6;
  s.row[2 * t] = s.row[2 * t + 1] = 0u;
  if constexpr (SAMPLED) s.must[2 * t] = s.must[2 * t + 1] = 0u;
  __syncthreads();
  for (int p = lo + t; p < hi; p += IGMC_BLOCK) {
    const int v = a.g.u_idx[p] - tile0;
    if (v >= 0 && v < CAND_TILE) atomicOr(&s.row[v >> 5], 1u << (v & 31));
  }
  if constexpr (SAMPLED) {
    for (int64_t p = mo + t; p < me; p += IGMC_BLOCK) {
      const int id = a.must_item[p];
      if (id < 0 || id >= a.g.n_items) {        // ignored and reported
        if (report) atomicOr(a.err, 8);
        continue;
      }
      const int v = id - tile0;
      if (v >= 0 && v < CAND_TILE) atomicOr(&s.must[v >> 5], 1u << (v & 31));
    }
  }
  __syncthreads();
  for (int w = wave; w < nw; w += nwave) {
    const int v = tile0 + w * 64 + lane;
    const int h = 2 * w + (lane >> 5), bit = lane & 31;
    const bool cand = v < a.g.n_items && !((s.row[h] >> bit) & 1u) && (!a.item_ok || a.item_ok[v] != 0);
    const unsigned long long c = __ballot(cand);
    if constexpr (SAMPLED) {
      const unsigned long long m = __ballot(cand && ((s.must[h] >> bit) & 1u));
      if (lane == 0) {
        s.pool[w] = c & ~m;
        s.forc[w] = m;
      }
    } else {
      if (lane == 0) s.pool[w] = c;
    }
  }
  __syncthreads();
}

// every walk over C: body(tile0, nw) for the tiles one after the other, their ballots rebuilt unless the graph is one tile
// (built by the first walk).  report: the first walk reports the must items out of range
template <bool SAMPLED>
struct CandTiles {
  const CandArgs& a;
  CandLds<SAMPLED>& s;
  int lo, hi;              // the user's row, where seen items are excluded
  int64_t mo, me;          // the request's must list
  bool report;
  bool built = false;
  template <class Body>
  __device__ __forceinline__ void operator()(Body&& body) {
    const int n_items = a.g.n_items;
    for (int tile0 = 0; tile0 < n_items; tile0 += CAND_TILE) {
      const int left = n_items - tile0;
      const int nw = left >= CAND_TILE ? CAND_TILE_WORDS : (left + 63) >> 6;
      if (!(n_items <= CAND_TILE && built)) cand_build_tile(a, s, lo, hi, mo, me, tile0, nw, report && !built);
      body(tile0, nw);
    }
    built = true;
  }
};

// WHERE a candidate lands: the items of s.pool (the words a tile emits) go to base + done + their rank in the tile, the
// word's share a block scan of the words' popcounts, a lane's the popcount of its word below it; store(pos, item, w, lane)
// only for pos in [0, end) -- what has no place is reported by the caller, never written.  Returns the tile's total; pool and
// woff may be rebuilt once it returns.
template <bool SAMPLED, class Store>
__device__ __forceinline__ int cand_place_tile(CandLds<SAMPLED>& s, int tile0, int nw, int64_t base, int done, int64_t end,
                                               Store&& store) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nwave = IGMC_BLOCK >> 6;
  int tile_total;
  s.woff[t] = igmc_block_scan_excl(t < nw ? __popcll(s.pool[t]) : 0, &tile_total, s.smi);
  __syncthreads();
  for (int w = wave; w < nw; w += nwave) {
    const unsigned long long m = s.pool[w];
    if ((m >> lane) & 1ull) {
      const int64_t pos = base + done + s.woff[w] + __popcll(m & ((1ull << lane) - 1ull));
      if (pos >= 0 && pos < end) store(pos, tile0 + w * 64 + lane, w, lane);
    }
  }
  __syncthreads();
  return tile_total;
}
