// shortlist.hip -- a cheap retrieval stage in front of the scoring pass: per requested user the min(m, |C|) candidates with the
// most CO-RATING VOTES, "people who liked what you liked also liked ..." as a two-hop integer walk over the resident CSR + CSC
// (no reference counterpart: the reference has no recommendation path at all).
//
// THE DEFINITION (igmc_hip.h states it for callers).  L_s = [entry present and relation >= seed_min_rel], L_t alike for
// vote_min_rel.  For request q, user u:
//   w[u']    = #{ i : L_s[u, i] and L_s[u', i] }  (u' != u; w[u] = 0)          co-liked items: the user itself never votes
//   votes[j] = sum over u' of w[u'] * L_t[u', j]                               exact unsigned integers, < 2^31 (checked by the host)
//   C        = the candidates of igmc_candidates_fill                          cand_tile.h: cand_build_tile, the ONE definition
//   THE VOTE ORDER over C: (votes descending, item id ascending); the shortlist = its first min(m, |C|) items, WRITTEN ITEM
//   ASCENDING like every candidate segment.
//
// k_shortlist<PLACES, WL, VL>   one workgroup per request (grid-stride).  WL: w (uint32[n_users]) sits in LDS, else in the
//                  workgroup's row of caller-owned scratch; VL: the votes (uint32[n_items]) sit in LDS (graphs of one tile:
//                  every bundled dataset, ml_10m), else behind w in the scratch row -- wider graphs SPILL the votes once and
//                  select from there, instead of repeating phase B per tile: phase B is the expensive walk (up to nnz adds),
//                  the selection's walks are n_items loads each.
//   phase A (w)    the seeding suffix of the user's row (rows are sorted by (relation, item): "relation >= s" is a suffix,
//                  found by a search on u_rel), a wave per item; lanes over the seeding suffix of the item's column:
//                  atomicAdd(w[u'], 1) for u' != u.
//   phase B (votes) the waves scan w 64 users at a time (a lane per user, the non-zero ones as a ballot); per non-zero u' the
//                  wave walks the voting suffix of row u', a lane per entry: atomicAdd(votes[item], w[u']).
//   cleanup        w is zeroed once when the workgroup starts; phase B CLEARS every non-zero word as it reads it -- it visits
//                  each of them exactly once anyway --, so the table is all zeros again when the request ends, without a second
//                  walk of phase A (which would cost as much as phase A itself: the sum of the seeding columns' lengths) and
//                  without a fill of n_users words.  The votes are zeroed per request (n_items words, what one selection walk
//                  costs).
//   selection      the threshold is the kk-th entry of the vote order over C, kk = min(m, |C|): four radix passes (byte
//                  histograms in LDS: kth_key.h's kth_radix) over key = ~votes of the pool items give the vote value V that holds it and r = how many
//                  items with exactly V votes are admitted (the lowest ids); kk == |C| admits everything and skips the passes.
//                  (select.h's 64-bit word carries a FLOAT image in its high half and does not fit integer votes: the order
//                  here is the pair (key, item id) itself -- the radix passes settle the key, the emission's running count of
//                  ties the id.)
//   emission       one walk in item order: ballots of "more than V votes" and of "exactly V", a block scan of the tie words'
//                  popcounts admits the first r ties, k_candidates' own cand_place_tile places the words.
//   PLACES         instead of selection + emission: for the request's queries, 256 at a time, place = #{i in C: votes[i] >
//                  votes[j] or (votes[i] == votes[j] and i < j)}, counted per wave and summed by LDS integer adds; -1 where j is
//                  not in C.
// k_short_check    (places) every answer starts as -1 / 0; the query offsets are checked as a whole (err bit 0), as
//                  k_rank_check does.
// All adds are integer atomics (LDS, or vector atomics on the scratch row), which commute: the output is a function of the
// inputs alone, whatever the grid.  No float anywhere.  Plain vector loads and stores; the error word: a vector atomic OR.
#include "capi.h"
#include "cand_tile.h"
#include "kth_key.h"

#define IGMC_SHORT_TILE_ITEMS IGMC_CAND_TILE_ITEMS      // items of the LDS vote table (uint32 each, 64 KB): every bundled dataset
                                                        // and ml_10m (10 677 items) in one tile; wider graphs keep their votes in
                                                        // the workgroup's scratch row
#define IGMC_SHORT_LDS_BYTES (160 * 1024)               // LDS of one workgroup at most (gfx950: 160 KB a CU): w sits in LDS
                                                        // where it fits beside the fixed part and the vote table, else in scratch
#define IGMC_SHORT_MAX_GRID 512                         // workgroups (and scratch rows) where the caller names no grid: 2 a CU
struct ShortArgs {
  GraphDev g;
  const int32_t* users;
  int nq;
  const uint8_t* item_ok;
  int exclude_seen;
  int seed_min_rel, vote_min_rel;
  int64_t m;                    // fill
  const int64_t* off;
  int32_t* link_u;
  int32_t* link_v;
  uint32_t* votes_out;          // may be null
  int64_t capacity;
  const int64_t* q_off;         // places
  const int32_t* q_id;
  int64_t n_query;
  int32_t* q_place;
  uint32_t* q_votes;            // may be null
  int32_t* err;
  uint32_t* scratch;            // [grid] rows of row_words: w (n_users words, where not in LDS), then the votes (n_items words,
  int64_t row_words;            // where the graph is wider than the LDS vote table)
};
struct ShortPlan {
  int grid, w_lds, v_lds;       // workgroups; w / the vote table in LDS
  int lds_bytes;                // dynamic LDS of the launch
  int64_t row_words, scratch_bytes;
  int w_lds_max_users;          // the most users whose w fits LDS for this graph's item count
};

static_assert(IGMC_SHORT_TILE_ITEMS == CAND_TILE, "the vote table and the candidate ballots cover the same tile");

struct ShortLds {
  CandLds<false> c;                                // the user's row, C of the tile, word offsets, scan scratch
  unsigned long long tie[CAND_TILE_WORDS];         // items of the tile with exactly V votes
  int toff[CAND_TILE_WORDS];
  int hist[IGMC_BLOCK];
  int qid[IGMC_BLOCK];                             // places: the tile of queries -- item (-1: out of range), its votes, the
  uint32_t qv[IGMC_BLOCK];                         // candidates before it, "is in C"
  int qcnt[IGMC_BLOCK];
  int qin[IGMC_BLOCK];
};
static_assert(sizeof(ShortLds) % 16 == 0, "the tables behind it stay aligned");

static inline __host__ __device__ int short_pad64(int n) { return (n + 63) & ~63; }

// first position of [lo, hi) whose relation is not below min_rel (the rows and columns are sorted by relation first)
__device__ __forceinline__ int short_suffix(const uint8_t* __restrict__ rel, int lo, int hi, int min_rel) {
  if (min_rel <= 0) return lo;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int)rel[mid] < min_rel) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

template <bool PLACES, bool WL, bool VL>
__global__ __launch_bounds__(IGMC_BLOCK) void k_shortlist(ShortArgs a) {
  IGMC_DYN_SMEM(smem);
  ShortLds& s = *reinterpret_cast<ShortLds*>(smem);
  uint32_t* const lds_tab = reinterpret_cast<uint32_t*>(smem + sizeof(ShortLds));
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nwave = IGMC_BLOCK >> 6;
  const int n_users = a.g.n_users, n_items = a.g.n_items;
  uint32_t* const row = a.scratch + (int64_t)blockIdx.x * a.row_words;
  uint32_t* votes;
  uint32_t* w;
  if constexpr (VL) votes = lds_tab;
  else votes = row + (WL ? 0 : short_pad64(n_users));
  if constexpr (WL) w = lds_tab + (VL ? short_pad64(n_items) : 0);
  else w = row;
  if constexpr (PLACES)
    if (*a.err & 1) return;        // (uniform over the launch: k_short_check found the query offsets inconsistent)
  CandArgs ca{};
  ca.g = a.g;
  ca.item_ok = a.item_ok;
  ca.err = a.err;

  for (int i = t; i < n_users; i += IGMC_BLOCK) w[i] = 0u;        // once: every request leaves it zero (phase B)
  __syncthreads();

  for (int q = blockIdx.x; q < a.nq; q += gridDim.x) {
    const int u = a.users[q];
    if (u < 0 || u >= n_users) {        // (uniform over the workgroup) no row is read; the segment is empty, the queries keep -1
      if (t == 0) atomicOr(a.err, 2);
      continue;
    }
    for (int i = t; i < n_items; i += IGMC_BLOCK) votes[i] = 0u;
    // ---- phase A: w
    const int r0 = a.g.u_ptr[u], r1 = a.g.u_ptr[u + 1];
    const int ra = short_suffix(a.g.u_rel, r0, r1, a.seed_min_rel);
    for (int p = ra + wave; p < r1; p += nwave) {
      const int item = a.g.u_idx[p];
      const int c1 = a.g.v_ptr[item + 1];
      const int c0 = short_suffix(a.g.v_rel, a.g.v_ptr[item], c1, a.seed_min_rel);
      for (int e = c0 + lane; e < c1; e += 64) {
        const int u2 = a.g.v_idx[e];
        if (u2 != u) atomicAdd(&w[u2], 1u);
      }
    }
    __syncthreads();
    // ---- phase B: votes; every non-zero word of w is read once and cleared
    for (int ub = wave * 64; ub < n_users; ub += nwave * 64) {
      const int uu = ub + lane;
      uint32_t wv = 0u;
      if (uu < n_users) {
        wv = w[uu];
        if (wv) w[uu] = 0u;
      }
      unsigned long long nz = __ballot(wv != 0u);
      while (nz) {        // (uniform over the wave)
        const int b = __ffsll((long long)nz) - 1;
        nz &= nz - 1ull;
        const uint32_t wb = __shfl(wv, b, 64);
        const int p1 = a.g.u_ptr[ub + b + 1];
        const int p0 = short_suffix(a.g.u_rel, a.g.u_ptr[ub + b], p1, a.vote_min_rel);
        for (int e = p0 + lane; e < p1; e += 64) atomicAdd(&votes[a.g.u_idx[e]], wb);
      }
    }
    __syncthreads();

    const int lo = a.exclude_seen ? r0 : 0, hi = a.exclude_seen ? r1 : 0;
    CandTiles<false> tiles{ca, s.c, lo, hi, 0, 0, false};        // every walk over C below

    if constexpr (PLACES) {
      int64_t qa = a.q_off[q], qb = a.q_off[q + 1];
      if (qa < 0 || qa > qb || qb > a.n_query) qa = qb = 0;        // (k_short_check has raised bit 0)
      for (int64_t q0 = qa; q0 < qb; q0 += IGMC_BLOCK) {
        const int nqt = (int)(qb - q0 < IGMC_BLOCK ? qb - q0 : IGMC_BLOCK);
        if (t < nqt) {
          const int id = a.q_id[q0 + t];
          const bool ok = id >= 0 && id < n_items;
          s.qid[t] = ok ? id : -1;
          s.qv[t] = ok ? votes[id] : 0u;
          s.qcnt[t] = 0;
          s.qin[t] = 0;
        }
        __syncthreads();
        tiles([&](int tile0, int nw) {
          for (int qi = 0; qi < nqt; ++qi) {
            const int id = s.qid[qi];
            if (id < 0) continue;        // (uniform)
            const uint32_t v = s.qv[qi];
            int c = 0;
            for (int wd = wave; wd < nw; wd += nwave) {
              if ((s.c.pool[wd] >> lane) & 1ull) {
                const int item = tile0 + wd * 64 + lane;
                const uint32_t vi = votes[item];
                c += (vi > v || (vi == v && item < id)) ? 1 : 0;
                if (item == id) s.qin[qi] = 1;
              }
            }
            c = igmc_wave_sum_i(c);
            if (lane == 0 && c) atomicAdd(&s.qcnt[qi], c);
          }
          __syncthreads();
        });
        if (t < nqt) {
          a.q_place[q0 + t] = s.qin[t] ? s.qcnt[t] : -1;
          if (a.q_votes) a.q_votes[q0 + t] = s.qv[t];
        }
        __syncthreads();        // (the next tile of queries, or the next request's zeroing of the votes)
      }
    } else {
      // ---- |C|
      int n_pool = 0;
      tiles([&](int, int nw) {
        int tp;
        igmc_block_scan_excl(t < nw ? __popcll(s.c.pool[t]) : 0, &tp, s.c.smi);
        n_pool += tp;
      });
      const int kk = a.m < (int64_t)n_pool ? (int)a.m : n_pool;
      const bool by_key = kk > 0 && kk < n_pool, all = kk == n_pool;
      // ---- the threshold: T = the key (~votes) of the kk-th of the vote order, r = the items of that key admitted
      uint32_t T = 0u;
      int r = kk;
      if (by_key) {        // (the walk reads the pool and the votes alone: no barrier per tile)
        auto walk = [&](auto&& f) {
          tiles([&](int tile0, int nw) {
            for (int wd = wave; wd < nw; wd += nwave)
              if ((s.c.pool[wd] >> lane) & 1ull) f(~votes[tile0 + wd * 64 + lane]);
          });
        };
        T = kth_radix(walk, 0u, 0u, 3, r, s.hist, s.c.smi);
      }
      // ---- the emission
      const int64_t base = a.off[q];
      int64_t end = a.off[q + 1];
      if (end > a.capacity) end = a.capacity;
      int done = 0, tdone = 0;
      tiles([&](int tile0, int nw) {
        for (int wd = wave; wd < nw; wd += nwave) {
          const bool in = (s.c.pool[wd] >> lane) & 1ull;
          const uint32_t key = in ? ~votes[tile0 + wd * 64 + lane] : 0u;
          const unsigned long long ms = __ballot(in && (all || (by_key && key < T)));
          const unsigned long long mt = __ballot(in && by_key && key == T);
          if (lane == 0) {
            s.c.pool[wd] = ms;
            s.tie[wd] = mt;
          }
        }
        __syncthreads();
        int tie_total;
        s.toff[t] = igmc_block_scan_excl(t < nw ? __popcll(s.tie[t]) : 0, &tie_total, s.c.smi);
        __syncthreads();
        for (int wd = wave; wd < nw; wd += nwave) {
          const unsigned long long mt = s.tie[wd];
          const bool adm = ((mt >> lane) & 1ull) && tdone + s.toff[wd] + __popcll(mt & ((1ull << lane) - 1ull)) < r;
          const unsigned long long ma = __ballot(adm);
          if (lane == 0) s.c.pool[wd] |= ma;
        }
        __syncthreads();
        done += cand_place_tile(s.c, tile0, nw, base, done, end, [&](int64_t pos, int item, int, int) {
          a.link_u[pos] = u;
          a.link_v[pos] = item;
          if (a.votes_out) a.votes_out[pos] = votes[item];
        });
        tdone += tie_total;
      });
      // bit 0: the segment reaches past `capacity` (nothing was written there); bit 2: the offsets are not the clamped counts'
      const int bad = ((base + kk > a.capacity) ? 1 : 0) | ((base < 0 || a.off[q + 1] - base != (int64_t)kk) ? 4 : 0);
      if (t == 0 && bad) atomicOr(a.err, bad);
    }
  }
}

__global__ __launch_bounds__(IGMC_BLOCK) void k_short_check(const int64_t* __restrict__ q_off, int nq, int64_t n_query,
                                                            int32_t* __restrict__ q_place, uint32_t* __restrict__ q_votes,
                                                            int32_t* err) {
  const int64_t stride = (int64_t)gridDim.x * IGMC_BLOCK;
  const int64_t i0 = (int64_t)blockIdx.x * IGMC_BLOCK + threadIdx.x;
  for (int64_t i = i0; i < n_query; i += stride) {
    q_place[i] = -1;
    if (q_votes) q_votes[i] = 0u;
  }
  int bad = 0;
  for (int64_t s = i0; s < nq; s += stride) {
    const int64_t a = q_off[s], b = q_off[s + 1];
    if (a < 0 || a > b || b > n_query || (s == 0 && a != 0) || (s == nq - 1 && b != n_query)) bad = 1;
  }
  if (bad) atomicOr(err, bad);
}

// ------------------------------------------------------------------ host
static void igmc_shortlist_plan(int n_users, int n_items, int nq, int grid, ShortPlan* p) {
  const int64_t fixed = (int64_t)sizeof(ShortLds);
  p->v_lds = n_items <= IGMC_SHORT_TILE_ITEMS;
  const int64_t vbytes = p->v_lds ? (int64_t)short_pad64(n_items) * 4 : 0;
  p->w_lds_max_users = (int)((IGMC_SHORT_LDS_BYTES - fixed - vbytes) / 4);
  p->w_lds = n_users <= p->w_lds_max_users;
  p->lds_bytes = (int)((fixed + vbytes + (p->w_lds ? (int64_t)n_users * 4 : 0) + 15) & ~(int64_t)15);
  p->row_words = (p->w_lds ? 0 : (int64_t)short_pad64(n_users)) + (p->v_lds ? 0 : (int64_t)short_pad64(n_items));
  int g = grid > 0 ? grid : IGMC_SHORT_MAX_GRID;
  if (g > nq) g = nq;
  p->grid = g < 1 ? 1 : g;
  p->scratch_bytes = (int64_t)p->grid * p->row_words * 4;
}

// dynamic LDS above 64 KB needs an explicit opt-in on HIP (per device, once)
static int igmc_shortlist_prepare() {
#ifndef IGMC_HIPEMU
  static bool done[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 1;
  if (done[dev]) return 0;
  const void* fns[8] = {(const void*)k_shortlist<false, false, false>, (const void*)k_shortlist<false, false, true>,
                        (const void*)k_shortlist<false, true, false>,  (const void*)k_shortlist<false, true, true>,
                        (const void*)k_shortlist<true, false, false>,  (const void*)k_shortlist<true, false, true>,
                        (const void*)k_shortlist<true, true, false>,   (const void*)k_shortlist<true, true, true>};
  for (const void* fn : fns)
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, IGMC_SHORT_LDS_BYTES) != hipSuccess) return 1;
  done[dev] = true;
#endif
  return 0;
}

static void igmc_launch_shortlist(const ShortArgs& a, const ShortPlan& p, int places, void* stream) {
  if (places) {
    const int64_t most = a.n_query > a.nq ? a.n_query : (int64_t)a.nq;
    const int64_t cg = (most + IGMC_BLOCK - 1) / IGMC_BLOCK;
    IGMC_PLAUNCH("k_short_check", k_short_check, (int)(cg < 1 ? 1 : cg > 65536 ? 65536 : cg), IGMC_BLOCK, 0, stream, a.q_off,
                 a.nq, a.n_query, a.q_place, a.q_votes, a.err);
    if (a.n_query < 1) return;
  }
  igmc_dispatch(
      [&](auto pl, auto wl, auto vl) {
        IGMC_PLAUNCH(pl() ? "k_shortlist_places" : "k_shortlist_fill", (k_shortlist<pl(), wl(), vl()>), p.grid, IGMC_BLOCK,
                     p.lds_bytes, stream, a);
      },
      places != 0, p.w_lds != 0, p.v_lds != 0);
}

// ------------------------------------------------------------------ C ABI
// short_args checks and files what both entry points take, and plans the launch.  Returns the refusal, or null.
static const char* short_args(ShortArgs* a, ShortPlan* p, const igmc_graph* g, const int32_t* d_users, int nq,
                              const uint8_t* d_item_ok, int exclude_seen, int seed_min_rel, int vote_min_rel, int32_t* d_err,
                              void* d_scratch, int64_t scratch_bytes, int grid) {
  if (!g || !d_users || !d_err) return "null argument";
  if (nq < 1) return "nq must be at least 1";
  if (seed_min_rel < 0 || vote_min_rel < 0) return "seed_min_rel and vote_min_rel must be at least 0";
  if (grid < 0 || grid > 65536) return "grid must be in [0, 65536]";
  if ((int64_t)g->max_deg_u * (int64_t)g->max_deg_v > (int64_t)INT32_MAX)
    return "max_deg_u * max_deg_v reaches 2^31: the vote counts may not fit";
  igmc_shortlist_plan(g->d.n_users, g->d.n_items, nq, grid, p);
  if (p->scratch_bytes > 0) {
    if (!d_scratch) return "null argument";
    if (scratch_bytes < p->scratch_bytes) return "scratch too small (igmc_shortlist_scratch_bytes)";
    if (((uintptr_t)d_scratch & 3) != 0) return "scratch must be 4-byte aligned";
  }
  *a = ShortArgs{};
  a->g = g->d;
  a->users = d_users;
  a->nq = nq;
  a->item_ok = d_item_ok;
  a->exclude_seen = exclude_seen != 0;
  a->seed_min_rel = seed_min_rel;
  a->vote_min_rel = vote_min_rel;
  a->err = d_err;
  a->scratch = (uint32_t*)d_scratch;
  a->row_words = p->row_words;
  if (igmc_shortlist_prepare()) return "the kernels' LDS size could not be set";
  return nullptr;
}
extern "C" int64_t igmc_shortlist_scratch_bytes(const igmc_graph* g, int nq, int grid) {
  if (!g || nq < 1 || grid < 0 || grid > 65536) {
    igmc_err() = std::string(__func__) + ": a graph, nq of at least 1, grid in [0, 65536]";
    return -1;
  }
  ShortPlan p;
  igmc_shortlist_plan(g->d.n_users, g->d.n_items, nq, grid, &p);
  return p.scratch_bytes;
}
extern "C" int igmc_shortlist_plan_info(const igmc_graph* g, int nq, int grid, int64_t out6[6]) {
  if (!g || !out6) IGMC_FAIL("null argument");
  if (nq < 1 || grid < 0 || grid > 65536) IGMC_FAIL("nq must be at least 1, grid in [0, 65536]");
  ShortPlan p;
  igmc_shortlist_plan(g->d.n_users, g->d.n_items, nq, grid, &p);
  out6[0] = p.grid;
  out6[1] = p.lds_bytes;
  out6[2] = p.w_lds;
  out6[3] = p.v_lds;
  out6[4] = p.scratch_bytes;
  out6[5] = p.w_lds_max_users;
  return 0;
}
extern "C" int igmc_shortlist_fill(const igmc_graph* g, const int32_t* d_users, int nq, const uint8_t* d_item_ok,
                                   int exclude_seen, int seed_min_rel, int vote_min_rel, int64_t m, const int64_t* d_offsets,
                                   int32_t* d_link_u, int32_t* d_link_v, uint32_t* d_votes, int64_t capacity, int32_t* d_err,
                                   void* d_scratch, int64_t scratch_bytes, int grid, void* stream) {
  ShortArgs a;
  ShortPlan p;
  if (!d_offsets || !d_link_u || !d_link_v) IGMC_FAIL("null argument");
  if (m < 1 || m > (int64_t)INT32_MAX) IGMC_FAIL("m must be in [1, 2^31)");
  if (capacity < 1 || capacity > (int64_t)INT32_MAX) IGMC_FAIL("capacity must be in [1, 2^31)");
  const char* bad = short_args(&a, &p, g, d_users, nq, d_item_ok, exclude_seen, seed_min_rel, vote_min_rel, d_err, d_scratch,
                               scratch_bytes, grid);
  if (bad) IGMC_FAIL(bad);
  a.m = m;
  a.off = d_offsets;
  a.link_u = d_link_u;
  a.link_v = d_link_v;
  a.votes_out = d_votes;
  a.capacity = capacity;
  igmc_launch_shortlist(a, p, 0, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
extern "C" int igmc_shortlist_places(const igmc_graph* g, const int32_t* d_users, int nq, const uint8_t* d_item_ok,
                                     int exclude_seen, int seed_min_rel, int vote_min_rel, const int64_t* d_q_off,
                                     const int32_t* d_q_id, int64_t n_query, int32_t* d_q_place, uint32_t* d_q_votes,
                                     int32_t* d_err, void* d_scratch, int64_t scratch_bytes, int grid, void* stream) {
  ShortArgs a;
  ShortPlan p;
  if (!d_q_off) IGMC_FAIL("null argument");
  if (n_query < 0 || n_query > (int64_t)INT32_MAX) IGMC_FAIL("n_query must be in [0, 2^31)");
  if (n_query > 0 && (!d_q_id || !d_q_place)) IGMC_FAIL("null argument");
  const char* bad = short_args(&a, &p, g, d_users, nq, d_item_ok, exclude_seen, seed_min_rel, vote_min_rel, d_err, d_scratch,
                               scratch_bytes, grid);
  if (bad) IGMC_FAIL(bad);
  a.q_off = d_q_off;
  a.q_id = d_q_id;
  a.n_query = n_query;
  a.q_place = d_q_place;
  a.q_votes = d_q_votes;
  igmc_launch_shortlist(a, p, 1, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
