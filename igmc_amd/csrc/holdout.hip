// holdout.hip -- the Given-k split of a set of users ON THE DEVICE: per requested user a uniform subset of the row is kept and
// the rest is written out as a held-out link list, which is at once the removal list of igmc_graph_apply (no reference
// counterpart: the reference evaluates one fixed train / test split by RMSE; by hand a Given-N protocol is a host loop over
// every user's row, a host RNG and a rebuilt matrix per level).
//
// THE SPLIT of request q (user u = users[q], row of d entries), igmc_hip.h states it for callers:
//   held = min(hold, max(0, d - keep)), kept = d - held
//   kept entries = the `kept` entries of the row with the smallest igmc_sample_key(igmc_holdout_salt(seed, draw, u), item) --
//                  keyed by the user ID, so the split of a user does not depend on q, on the users that share the launch or
//                  on the grid; the key is a bijection of the item id, so exactly `kept` keys are <= the threshold T
//   segment      = the other entries IN THE ROW'S OWN ORDER (relation ascending, then item ascending), as (u, item, relation + 1).
//
// k_holdout<FILL>  <0> the segments' lengths: the row pointers alone, one THREAD per request (grid-stride).
//                  <1> the links, at offsets the caller derived from the counts: one workgroup per request (grid-stride).  The
//                  threshold T by kth_key.h's steps composed as k_candidates<1, 1> composes them -- the walk is a strided pass
//                  over the row in global memory, one key per thread: no tiles and no bitmap, the set is the row itself --: a
//                  histogram pass over the keys' top byte, the keys of the deciding byte parked and counted where kth_parks()
//                  allows it, the remaining three radix passes otherwise; kept == 0 and kept == d need no threshold.  The
//                  emission takes the row in chunks of IGMC_BLOCK entries in row order, a lane per entry: held <=> key > T;
//                  a lane's place = the popcount of its wave's ballot below it + a block scan of the waves' popcounts + the
//                  chunks before it.  The output is a function of the inputs alone: the only atomics are the LDS histogram /
//                  list-cursor adds, which commute, and the error word's OR, reached on errors only.  Plain vector stores.
//                  Rows of any length: LDS holds the histogram, the parked list and the scan words, never the row.
#include "capi.h"
#include "kth_key.h"        // the k-th smallest key of the row

struct HoldArgs {
  GraphDev g;
  const int32_t* users;
  int nq;
  int64_t keep, hold;
  uint64_t seed, draw;          // fill
  int64_t* counts;              // count
  const int64_t* off;           // fill
  int32_t* link_u;
  int32_t* link_v;
  uint8_t* rating;
  int64_t capacity;
  int32_t* err;
};

struct HoldLds {
  int hist[IGMC_BLOCK];
  uint32_t ckey[IGMC_BLOCK];        // parked keys of the deciding byte
  int smi[16];
};

// entries of a row of d that the split holds out
__device__ __forceinline__ int hold_count(int d, int64_t keep, int64_t hold) {
  const int64_t over = (int64_t)d > keep ? (int64_t)d - keep : 0;
  return (int)(hold < over ? hold : over);
}

template <bool FILL>
__global__ __launch_bounds__(IGMC_BLOCK) void k_holdout(HoldArgs a) {
  const int t = threadIdx.x;
  if constexpr (!FILL) {
    for (int64_t q = (int64_t)blockIdx.x * IGMC_BLOCK + t; q < a.nq; q += (int64_t)gridDim.x * IGMC_BLOCK) {
      const int u = a.users[q];
      if (u < 0 || u >= a.g.n_users) {        // no row is read; the segment is empty
        atomicOr(a.err, 2);
        a.counts[q] = 0;
        continue;
      }
      a.counts[q] = hold_count(a.g.u_ptr[u + 1] - a.g.u_ptr[u], a.keep, a.hold);
    }
  } else {
    __shared__ HoldLds s;
    const int lane = t & 63;
    for (int q = blockIdx.x; q < a.nq; q += gridDim.x) {
      const int u = a.users[q];
      if (u < 0 || u >= a.g.n_users) {        // (uniform over the workgroup)
        if (t == 0) atomicOr(a.err, 2);
        continue;
      }
      const int lo = a.g.u_ptr[u], hi = a.g.u_ptr[u + 1];
      const int d = hi - lo, held = hold_count(d, a.keep, a.hold), kept = d - held;
      const int64_t base = a.off[q];
      // bit 0: the segment reaches past `capacity` (nothing is written there); bit 2: the offsets are not the counts'
      const int bad = ((base + held > a.capacity) ? 1 : 0) | ((base < 0 || a.off[q + 1] - base != (int64_t)held) ? 4 : 0);
      if (t == 0 && bad) atomicOr(a.err, bad);
      if (held == 0) continue;        // (uniform) nothing to write
      // ---- the threshold, for kept in (0, d) only -- nothing or everything of the row is held otherwise
      const uint64_t salt = igmc_holdout_salt(a.seed, a.draw, (uint64_t)(uint32_t)u);
      const bool by_key = kept > 0;        // (held > 0: kept < d)
      uint32_t T = 0u;
      if (by_key) {
        // f(key) for the entries of the row, one key per thread (the row is read-only: no barrier of its own)
        auto walk = [&](auto&& f) {
          for (int p = lo + t; p < hi; p += IGMC_BLOCK) f(igmc_sample_key(salt, (uint32_t)a.g.u_idx[p]));
        };
        const KthBin top = kth_pass(walk, 0u, 0u, 24, kept, s.hist, s.smi);
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
      // ---- the emission: the row in chunks of a workgroup, in row order; held <=> key > T (kept == 0: every entry)
      int64_t end = a.off[q + 1];
      if (end > a.capacity) end = a.capacity;
      int done = 0;
      for (int c0 = lo; c0 < hi; c0 += IGMC_BLOCK) {        // (every bound is uniform: the scan's barriers are the workgroup's)
        const int p = hi - c0 > t ? c0 + t : -1;
        const int item = p >= 0 ? a.g.u_idx[p] : 0;
        const bool out = p >= 0 && (!by_key || igmc_sample_key(salt, (uint32_t)item) > T);
        const unsigned long long m = __ballot(out);
        int chunk_total;
        const int ex = igmc_block_scan_excl(lane == 0 ? __popcll(m) : 0, &chunk_total, s.smi);
        const int wave_base = __shfl(ex, 0, 64);
        if (out) {
          const int64_t pos = base + done + wave_base + __popcll(m & ((1ull << lane) - 1ull));
          if (pos >= 0 && pos < end) {
            a.link_u[pos] = u;
            a.link_v[pos] = item;
            a.rating[pos] = (uint8_t)(a.g.u_rel[p] + 1);
          }
        }
        done += chunk_total;
        if (hi - c0 <= IGMC_BLOCK) break;        // (the last chunk: c0 + IGMC_BLOCK may not fit an int)
      }
    }
  }
}

// ------------------------------------------------------------------ host
static void igmc_launch_holdout(const HoldArgs& a, int fill, void* stream) {
  if (a.nq < 1) return;
  const int64_t jobs = fill ? (int64_t)a.nq : ((int64_t)a.nq + IGMC_BLOCK - 1) / IGMC_BLOCK;
  const int grid = (int)(jobs > 65536 ? 65536 : jobs);        // as k_candidates caps it: a workgroup takes a second request
  if (fill)
    IGMC_PLAUNCH("k_holdout_fill", k_holdout<true>, grid, IGMC_BLOCK, 0, stream, a);
  else
    IGMC_PLAUNCH("k_holdout_count", k_holdout<false>, grid, IGMC_BLOCK, 0, stream, a);
}

// ------------------------------------------------------------------ C ABI
// what both entry points take; returns the refusal, or null
static const char* hold_args(HoldArgs* a, const igmc_graph* g, const int32_t* d_users, int nq, int64_t keep, int64_t hold,
                             int32_t* d_err) {
  if (!g || !d_users || !d_err) return "null argument";
  if (nq < 0) return "nq must be at least 0";
  if (keep < 0) return "keep must be at least 0";
  if (hold < 0) return "hold must be at least 0";
  *a = HoldArgs{g->d, d_users, nq, keep, hold};
  a->err = d_err;
  return nullptr;
}
extern "C" int igmc_holdout_count(const igmc_graph* g, const int32_t* d_users, int nq, int64_t keep, int64_t hold,
                                  int64_t* d_counts, int32_t* d_err, void* stream) {
  HoldArgs a;
  const char* bad = hold_args(&a, g, d_users, nq, keep, hold, d_err);
  if (bad) IGMC_FAIL(bad);
  if (!d_counts) IGMC_FAIL("null argument");
  a.counts = d_counts;
  igmc_launch_holdout(a, 0, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
extern "C" int igmc_holdout_fill(const igmc_graph* g, const int32_t* d_users, int nq, int64_t keep, int64_t hold, uint64_t seed,
                                 uint64_t draw, const int64_t* d_offsets, int32_t* d_link_u, int32_t* d_link_v,
                                 uint8_t* d_rating, int64_t capacity, int32_t* d_err, void* stream) {
  HoldArgs a;
  const char* bad = hold_args(&a, g, d_users, nq, keep, hold, d_err);
  if (bad) IGMC_FAIL(bad);
  if (!d_offsets || !d_link_u || !d_link_v || !d_rating) IGMC_FAIL("null argument");
  if (capacity < 0) IGMC_FAIL("capacity must be at least 0");
  a.seed = seed;
  a.draw = draw;
  a.off = d_offsets;
  a.link_u = d_link_u;
  a.link_v = d_link_v;
  a.rating = d_rating;
  a.capacity = capacity;
  igmc_launch_holdout(a, 1, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
