// graph_update.hip -- a list of rating changes applied to a resident rating graph, on the device: the arrays of a NEW graph that
// are, byte for byte, what igmc_graph_create builds from the changed matrix (no reference counterpart: the reference rebuilds
// SparseRowIndexer / SparseColIndexer from scratch, util_functions.py:20-66).  The same kernels serve both orientations -- "row"
// is the user and "col" the item for u_ptr / u_idx / u_rel, the other way round for v_* --, each on a sorted copy of the list:
//
// k_gu_keys        change j -> the word (row << 32 | col) and its list position j; ids out of range raise the error word.  The
//                  list is padded to a power of two with words that sort behind every change.
// k_gu_sort_local  bitonic sort of (word, position) pairs, ascending, positions breaking ties: all pairs are distinct, so the
// k_gu_sort_global result is a function of the list alone.  Strides below GU_TILE run in LDS (one tile per workgroup), wider ones
//                  as one launch each.  After it the changes of a row are one contiguous segment ordered by (col, position), and
//                  the LAST of every run of equal words is the assignment that wins.
// k_gu_mark        per sorted position: -1 (overridden by a later assignment), 0 (the winner removes), rating (the winner writes).
// k_gu_rows        one wave per row: every old entry looks its column up in the row's segment (a binary search) and leaves its
//                  relation with the winner it finds; new length = old length - winners that hit an entry + winners that
//                  write.
// k_gu_scan        lengths -> pointers in place (one workgroup, 4096 rows a round, 64-bit carry), nnz, the int32 check and the
//                  longest row.
// k_gu_copy        the rows without changes, one thread per old entry (row by a binary search over the old pointers): the bulk
//                  of the bytes, and independent of how long a row is.
// k_gu_write       one wave per row with changes.  Every element's place is COUNTED: an old
//                  entry of key (rel, col) that no winner hit moves down by the hit entries below it and up by the written
//                  winners below it; a written winner goes behind the old entries below it (a binary search: the old row is
//                  sorted by that key) with the same two corrections.  Places are a function of the keys, keys are distinct:
//                  no order a kernel produced by atomics reaches the output.  max_rel: an integer atomicMax over what is written.
//
//                  The counts: a wave stages the two keys of up to GU_ROW_STAGE changes of its row in LDS, sorts both arrays
//                  (bitonic, in the wave) and counts by binary search -- (old length + changes) x log(changes) per row.  A row
//                  with more changes counts by a pass over its segment in memory, (old length + changes) x changes: slow
//                  (quadratic in the changes of that one row), never refused.
// Plain vector stores only (error word: a vector atomic OR, reached on errors only).
#include "capi.h"
#include <stdlib.h>
#include <map>
#include <mutex>

// One orientation at a time (side 0: rows are users, side 1: rows are items).  plan: the sorted change list, the new row
// lengths, their prefix sums, nnz and the longest row; write: the rows of the new graph, once the host has read nnz and
// allocated them.
struct GuStats {
  int32_t err;              // bit 0: a user id out of range, bit 1: an item id out of range, bit 2: nnz does not fit int32
  int32_t max_deg[2];
  int32_t max_rel;
  long long nnz[2];
};
struct GuSide {
  const int32_t* optr;      // the old graph's arrays of this orientation
  const int32_t* oidx;
  const uint8_t* orel;
  int rows_old, rows_new;
  unsigned long long* keys; // [padded n] sorted (row << 32 | col) words
  uint32_t* idx;            // [padded n] their list positions
  int16_t* s_new;           // [n] -1: overridden, 0: the winner removes, else the winner's rating
  int16_t* s_old;           // [n] a winner's relation in the old row, or -1
  uint8_t* touched;         // [rows_new] the row has changes in the list
  int32_t* nptr;            // the new graph's arrays
  int32_t* nidx;
  uint8_t* nrel;
};

#define GU_TILE 2048          // pairs of one LDS tile of the sort (24 KB)
#define GU_SCAN_ITEMS 16      // rows per thread and round of the scan
#define GU_PAD (~0ull)
#define GU_NONE (~0ull)       // a key no entry has (relations are below 255)
#define GU_ROW_STAGE 256      // changes of one row whose keys a wave of k_gu_write stages in LDS (4 waves x 2 x 2 KB)

typedef unsigned long long gu_word;

__global__ __launch_bounds__(IGMC_BLOCK) void k_gu_keys(const int32_t* __restrict__ user, const int32_t* __restrict__ item,
                                                        int64_t n, int64_t P, int swap, int n_users, int n_items,
                                                        gu_word* __restrict__ keys, uint32_t* __restrict__ idx, GuStats* st) {
  for (int64_t i = (int64_t)blockIdx.x * IGMC_BLOCK + threadIdx.x; i < P; i += (int64_t)gridDim.x * IGMC_BLOCK) {
    gu_word k = GU_PAD;
    if (i < n) {
      const int32_t u = user[i], v = item[i];
      const int bad = ((u < 0 || u >= n_users) ? 1 : 0) | ((v < 0 || v >= n_items) ? 2 : 0);
      if (bad) atomicOr(&st->err, bad);
      k = swap ? (((gu_word)(uint32_t)v << 32) | (uint32_t)u) : (((gu_word)(uint32_t)u << 32) | (uint32_t)v);
    }
    keys[i] = k;
    idx[i] = (uint32_t)i;
  }
}

__device__ __forceinline__ bool gu_after(gu_word ka, uint32_t ia, gu_word kb, uint32_t ib) {
  return ka > kb || (ka == kb && ia > ib);
}

// stages k = kfirst .. klast of the bitonic network, of each the strides below GU_TILE, on tiles of T = min(GU_TILE, P) pairs
__global__ __launch_bounds__(IGMC_BLOCK) void k_gu_sort_local(gu_word* __restrict__ keys, uint32_t* __restrict__ idx, int64_t P,
                                                              int64_t kfirst, int64_t klast) {
  __shared__ gu_word sk[GU_TILE];
  __shared__ uint32_t si[GU_TILE];
  const int T = (int)(P < GU_TILE ? P : GU_TILE);
  const int64_t ntiles = P / T;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * T;
    for (int i = threadIdx.x; i < T; i += IGMC_BLOCK) {
      sk[i] = keys[base + i];
      si[i] = idx[base + i];
    }
    for (int64_t k = kfirst; k <= klast; k <<= 1) {
      int j = (int)((k >> 1) < (T >> 1) ? (k >> 1) : (T >> 1));
      for (; j > 0; j >>= 1) {
        __syncthreads();
        for (int t = threadIdx.x; t < (T >> 1); t += IGMC_BLOCK) {
          const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
          const bool asc = ((base + i) & k) == 0;
          const gu_word ka = sk[i], kb = sk[l];
          const uint32_t ia = si[i], ib = si[l];
          if (gu_after(ka, ia, kb, ib) == asc) {
            sk[i] = kb; si[i] = ib;
            sk[l] = ka; si[l] = ia;
          }
        }
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < T; i += IGMC_BLOCK) {
      keys[base + i] = sk[i];
      idx[base + i] = si[i];
    }
    __syncthreads();        // (the next tile stages over sk / si)
  }
}

// stride j >= GU_TILE of stage k: one compare-exchange per thread
__global__ __launch_bounds__(IGMC_BLOCK) void k_gu_sort_global(gu_word* __restrict__ keys, uint32_t* __restrict__ idx, int64_t P,
                                                               int64_t k, int64_t j) {
  for (int64_t t = (int64_t)blockIdx.x * IGMC_BLOCK + threadIdx.x; t < (P >> 1); t += (int64_t)gridDim.x * IGMC_BLOCK) {
    const int64_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
    const bool asc = (i & k) == 0;
    const gu_word ka = keys[i], kb = keys[l];
    const uint32_t ia = idx[i], ib = idx[l];
    if (gu_after(ka, ia, kb, ib) == asc) {
      keys[i] = kb; idx[i] = ib;
      keys[l] = ka; idx[l] = ia;
    }
  }
}

__global__ __launch_bounds__(IGMC_BLOCK) void k_gu_mark(const gu_word* __restrict__ keys, const uint32_t* __restrict__ idx,
                                                        const uint8_t* __restrict__ rating, int64_t n,
                                                        int16_t* __restrict__ s_new, int16_t* __restrict__ s_old) {
  for (int64_t p = (int64_t)blockIdx.x * IGMC_BLOCK + threadIdx.x; p < n; p += (int64_t)gridDim.x * IGMC_BLOCK) {
    const bool wins = p + 1 == n || keys[p + 1] != keys[p];
    s_new[p] = wins ? (int16_t)rating[idx[p]] : (int16_t)-1;
    s_old[p] = -1;
  }
}

// first sorted position whose word is not below `target`
__device__ __forceinline__ int64_t gu_lower(const gu_word* __restrict__ keys, int64_t n, gu_word target) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < target) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(IGMC_BLOCK) void k_gu_rows(GuSide s, int64_t n) {
  const int lane = threadIdx.x & 63, wpb = IGMC_BLOCK >> 6;
  for (int64_t r = (int64_t)blockIdx.x * wpb + (threadIdx.x >> 6); r < s.rows_new; r += (int64_t)gridDim.x * wpb) {
    const int o0 = r < s.rows_old ? s.optr[r] : 0, olen = r < s.rows_old ? s.optr[r + 1] - o0 : 0;
    const int64_t lo = gu_lower(s.keys, n, (gu_word)r << 32), hi = gu_lower(s.keys, n, (gu_word)(r + 1) << 32);
    int delta = 0;
    if (lo < hi) {        // (lo, hi, r: uniform over the wave)
      // every old entry looks its column up among the row's changes: the LAST of a run of equal words is the winner, and
      // columns of a row are distinct, so no two lanes find the same one
      for (int q = lane; q < olen; q += 64) {
        const gu_word target = ((gu_word)r << 32) | (uint32_t)s.oidx[o0 + q];
        int64_t a = lo, b = hi;        // first position above target
        while (a < b) {
          const int64_t mid = (a + b) >> 1;
          if (s.keys[mid] <= target) a = mid + 1; else b = mid;
        }
        if (a > lo && s.keys[a - 1] == target) {
          s.s_old[a - 1] = (int16_t)s.orel[o0 + q];
          delta -= 1;
        }
      }
      for (int64_t p = lo + lane; p < hi; p += 64) delta += s.s_new[p] > 0 ? 1 : 0;
      delta = igmc_wave_sum_i(delta);
    }
    if (lane == 0) {
      s.nptr[r] = olen + delta;
      s.touched[r] = lo < hi ? 1 : 0;
    }
  }
}

// exclusive scan over the workgroup of a 64-bit value; *total = sum.  sm: 4 words of LDS.
__device__ __forceinline__ long long gu_block_scan_excl(long long v, long long* total, long long* sm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const long long t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  if (lane == 63) sm[wave] = inc;
  __syncthreads();
  long long base = 0, tot = 0;
  for (int w = 0; w < (IGMC_BLOCK >> 6); ++w) {
    const long long x = sm[w];
    if (w < wave) base += x;
    tot += x;
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

// ptr[0 .. rows): lengths -> ptr[0 .. rows]: their exclusive prefix sums; nnz and the longest row on the way (one workgroup)
__global__ __launch_bounds__(IGMC_BLOCK) void k_gu_scan(int32_t* __restrict__ ptr, int64_t rows, int side, GuStats* st) {
  __shared__ long long sm[4];
  __shared__ int smx[4];
  long long carry = 0;
  int longest = 0;
  const int64_t m = rows + 1, round = (int64_t)IGMC_BLOCK * GU_SCAN_ITEMS;
  for (int64_t c0 = 0; c0 < m; c0 += round) {
    const int64_t a = c0 + (int64_t)threadIdx.x * GU_SCAN_ITEMS;
    int v[GU_SCAN_ITEMS];
    long long sum = 0;
#pragma unroll
    for (int e = 0; e < GU_SCAN_ITEMS; ++e) {
      v[e] = a + e < rows ? ptr[a + e] : 0;
      sum += v[e];
      longest = v[e] > longest ? v[e] : longest;
    }
    long long tot;
    long long at = carry + gu_block_scan_excl(sum, &tot, sm);
#pragma unroll
    for (int e = 0; e < GU_SCAN_ITEMS; ++e) {
      if (a + e < m) ptr[a + e] = (int32_t)(at < (long long)INT32_MAX ? at : (long long)INT32_MAX);
      at += v[e];
    }
    carry += tot;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int o = __shfl_xor(longest, d, 64);
    longest = o > longest ? o : longest;
  }
  if ((threadIdx.x & 63) == 0) smx[threadIdx.x >> 6] = longest;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < (IGMC_BLOCK >> 6); ++w) longest = smx[w] > longest ? smx[w] : longest;
    st->max_deg[side] = longest;
    st->nnz[side] = carry;
    if (carry >= (long long)INT32_MAX) atomicOr(&st->err, 4);
  }
}

__device__ __forceinline__ gu_word gu_key(int rel, int32_t col) { return ((gu_word)(uint32_t)rel << 32) | (uint32_t)col; }

__device__ __forceinline__ int gu_peek(const int32_t* p) {
#ifdef IGMC_HIPEMU
  return *p;
#else
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}

// max_rel: the wave's largest relation, and an atomic only from a wave that would raise the word (it only grows: a stale read
// costs one atomic).  Every lane of the wave calls it.
__device__ __forceinline__ void gu_raise_max_rel(int track_rel, int top, GuStats* st) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int o = __shfl_xor(top, d, 64);
    top = o > top ? o : top;
  }
  if (track_rel && (threadIdx.x & 63) == 0 && top > gu_peek(&st->max_rel)) atomicMax(&st->max_rel, top);
}

// keys of a sorted LDS array of m that are below k
__device__ __forceinline__ int gu_below(const gu_word* a, int m, gu_word k) {
  int lo = 0, hi = m;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the two keys of sorted position p: where the winner's column was in the old row, and where it goes (GU_NONE: nowhere)
__device__ __forceinline__ void gu_pair(const GuSide& s, int64_t p, gu_word* ko, gu_word* kn) {
  const int nw = s.s_new[p], was = s.s_old[p];
  const int32_t c = (int32_t)(uint32_t)s.keys[p];
  *ko = (nw >= 0 && was >= 0) ? gu_key(was, c) : GU_NONE;
  *kn = nw > 0 ? gu_key(nw - 1, c) : GU_NONE;
}

// the rows without changes, one thread per OLD entry (a row's length does not matter: the longest column of a MovieLens-shaped
// graph would keep a single wave busy for longer than the rest of the update takes): the entry's row by a binary search over
// the old pointers, its place the same offset into the new row
__global__ __launch_bounds__(IGMC_BLOCK) void k_gu_copy(GuSide s, int track_rel, GuStats* st) {
  const int64_t total = s.rows_old > 0 ? s.optr[s.rows_old] : 0;
  int top = 0;
  for (int64_t p = (int64_t)blockIdx.x * IGMC_BLOCK + threadIdx.x; p < total; p += (int64_t)gridDim.x * IGMC_BLOCK) {
    int a = 0, b = s.rows_old;        // the last row that starts at or in front of p
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (s.optr[mid + 1] <= p) a = mid + 1; else b = mid;
    }
    if (a >= s.rows_old || s.touched[a]) continue;
    const int64_t q = (int64_t)s.nptr[a] + (p - s.optr[a]);
    if (q >= s.nptr[a + 1]) continue;
    const int rel = s.orel[p];
    s.nidx[q] = s.oidx[p];
    s.nrel[q] = (uint8_t)rel;
    top = rel > top ? rel : top;
  }
  gu_raise_max_rel(track_rel, top, st);
}

__global__ __launch_bounds__(IGMC_BLOCK) void k_gu_write(GuSide s, int track_rel, int64_t n, GuStats* st) {
  __shared__ gu_word sko[IGMC_BLOCK >> 6][GU_ROW_STAGE];
  __shared__ gu_word skn[IGMC_BLOCK >> 6][GU_ROW_STAGE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = IGMC_BLOCK >> 6;
  int top = 0;
  for (int64_t r = (int64_t)blockIdx.x * wpb + wave; r < s.rows_new; r += (int64_t)gridDim.x * wpb) {
    if (!s.touched[r]) continue;        // (uniform over the wave; k_gu_copy wrote the row)
    const int o0 = r < s.rows_old ? s.optr[r] : 0, olen = r < s.rows_old ? s.optr[r + 1] - o0 : 0;
    const int n0 = s.nptr[r], nlen = s.nptr[r + 1] - n0;
    const int64_t lo = gu_lower(s.keys, n, (gu_word)r << 32), hi = gu_lower(s.keys, n, (gu_word)(r + 1) << 32);
    // up to GU_ROW_STAGE changes of a row are staged as their two keys; a longer segment is read from memory every time
    const int64_t seg = hi - lo;
    const bool staged = seg <= GU_ROW_STAGE;
    int m = 1;        // staged keys: seg rounded up to a power of two, GU_NONE behind them
    if (staged) {
      while (m < (int)seg) m <<= 1;
      for (int x = lane; x < m; x += 64) {
        gu_word ko = GU_NONE, kn = GU_NONE;
        if (x < (int)seg) gu_pair(s, lo + x, &ko, &kn);
        sko[wave][x] = ko;
        skn[wave][x] = kn;
      }
      IGMC_WAVE_SYNC();
      // both arrays sorted ascending by the wave (bitonic; the keys of an array are distinct but for GU_NONE): a count
      // "keys below k" is then a binary search
      for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
          for (int t = lane; t < (m >> 1); t += 64) {
            const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
            const bool asc = (i & k) == 0;
            const gu_word a0 = sko[wave][i], a1 = sko[wave][l], b0 = skn[wave][i], b1 = skn[wave][l];
            if ((a0 > a1) == asc) {
              sko[wave][i] = a1;
              sko[wave][l] = a0;
            }
            if ((b0 > b1) == asc) {
              skn[wave][i] = b1;
              skn[wave][l] = b0;
            }
          }
          IGMC_WAVE_SYNC();
        }
    }
    // old entries no winner hit
    for (int q = lane; q < olen; q += 64) {
      const int rel = s.orel[o0 + q];
      const int32_t col = s.oidx[o0 + q];
      const gu_word ke = gu_key(rel, col);
      int gone = 0, come = 0;
      bool hit = false;
      if (staged) {
        gone = gu_below(sko[wave], m, ke);
        hit = gone < m && sko[wave][gone] == ke;
        come = gu_below(skn[wave], m, ke);
      } else {
        for (int64_t x = lo; x < hi; ++x) {
          gu_word ko, kn;
          gu_pair(s, x, &ko, &kn);
          gone += ko < ke ? 1 : 0;
          hit = hit || ko == ke;
          come += kn < ke ? 1 : 0;
        }
      }
      const int at = q - gone + come;
      if (!hit && at >= 0 && at < nlen) {
        s.nidx[n0 + at] = col;
        s.nrel[n0 + at] = (uint8_t)rel;
        top = rel > top ? rel : top;
      }
    }
    // winners that write
    for (int64_t p = lo + lane; p < hi; p += 64) {
      const int nw = s.s_new[p];
      if (nw <= 0) continue;
      const int32_t col = (int32_t)(uint32_t)s.keys[p];
      const gu_word kw = gu_key(nw - 1, col);
      int a = 0, b = olen;        // old entries below kw
      while (a < b) {
        const int mid = (a + b) >> 1;
        if (gu_key(s.orel[o0 + mid], s.oidx[o0 + mid]) < kw) a = mid + 1; else b = mid;
      }
      int gone = 0, come = 0;
      if (staged) {
        gone = gu_below(sko[wave], m, kw);
        come = gu_below(skn[wave], m, kw);
      } else {
        for (int64_t x = lo; x < hi; ++x) {
          gu_word ko, kn;
          gu_pair(s, x, &ko, &kn);
          gone += ko < kw ? 1 : 0;
          come += kn < kw ? 1 : 0;
        }
      }
      const int at = a - gone + come;
      if (at >= 0 && at < nlen) {
        s.nidx[n0 + at] = col;
        s.nrel[n0 + at] = (uint8_t)(nw - 1);
        top = nw - 1 > top ? nw - 1 : top;
      }
    }
    if (staged) IGMC_WAVE_SYNC();        // (the wave's next row stages over sko / skn)
  }
  gu_raise_max_rel(track_rel, top, st);
}

// ------------------------------------------------------------------ host
// IGMC_GU_GRID=<workgroups> (test hook): every grid-stride launch of an update runs on that many workgroups
static int gu_grid(int64_t jobs) {
  const char* e = getenv("IGMC_GU_GRID");
  const int forced = e ? atoi(e) : 0;
  if (forced > 0) return forced;
  return (int)(jobs < 1 ? 1 : jobs > 65536 ? 65536 : jobs);
}

static int64_t igmc_graph_update_padded(int64_t n) {
  if (n < 1) return 0;
  int64_t P = 2;
  while (P < n) P <<= 1;
  return P;
}

static void igmc_launch_graph_update_plan(const GuSide& s, int side, const int32_t* user, const int32_t* item, const uint8_t* rating,
                                   int64_t n, int n_users, int n_items, GuStats* st, void* stream) {
  const int64_t P = igmc_graph_update_padded(n);
  if (n > 0) {
    IGMC_PLAUNCH("k_gu_keys", k_gu_keys, gu_grid((P + IGMC_BLOCK - 1) / IGMC_BLOCK), IGMC_BLOCK, 0, stream, user, item, n, P, side,
                 n_users, n_items, s.keys, s.idx, st);
    const int64_t T = P < GU_TILE ? P : GU_TILE;
    IGMC_PLAUNCH("k_gu_sort_local", k_gu_sort_local, gu_grid(P / T), IGMC_BLOCK, 0, stream, s.keys, s.idx, P, (int64_t)2, T);
    for (int64_t k = 2 * T; k <= P; k <<= 1) {
      for (int64_t j = k >> 1; j >= T; j >>= 1)
        IGMC_PLAUNCH("k_gu_sort_global", k_gu_sort_global, gu_grid((P / 2 + IGMC_BLOCK - 1) / IGMC_BLOCK), IGMC_BLOCK, 0, stream,
                     s.keys, s.idx, P, k, j);
      IGMC_PLAUNCH("k_gu_sort_local", k_gu_sort_local, gu_grid(P / T), IGMC_BLOCK, 0, stream, s.keys, s.idx, P, k, k);
    }
    IGMC_PLAUNCH("k_gu_mark", k_gu_mark, gu_grid((n + IGMC_BLOCK - 1) / IGMC_BLOCK), IGMC_BLOCK, 0, stream,
                 (const gu_word*)s.keys, (const uint32_t*)s.idx, rating, n, s.s_new, s.s_old);
  }
  const int wpb = IGMC_BLOCK >> 6;
  IGMC_PLAUNCH("k_gu_rows", k_gu_rows, gu_grid(((int64_t)s.rows_new + wpb - 1) / wpb), IGMC_BLOCK, 0, stream, s, n);
  IGMC_PLAUNCH("k_gu_scan", k_gu_scan, 1, IGMC_BLOCK, 0, stream, s.nptr, (int64_t)s.rows_new, side, st);
}

static void igmc_launch_graph_update_write(const GuSide& s, int side, int64_t n, int64_t nnz_old, GuStats* st, void* stream) {
  const int wpb = IGMC_BLOCK >> 6;
  if (nnz_old > 0) {
    const int64_t blocks = (nnz_old + IGMC_BLOCK - 1) / IGMC_BLOCK;
    IGMC_PLAUNCH("k_gu_copy", k_gu_copy, gu_grid(blocks > 8192 ? 8192 : blocks), IGMC_BLOCK, 0, stream, s, side == 0 ? 1 : 0, st);
  }
  if (n > 0)
  IGMC_PLAUNCH("k_gu_write", k_gu_write, gu_grid(((int64_t)s.rows_new + wpb - 1) / wpb), IGMC_BLOCK, 0, stream, s,
               side == 0 ? 1 : 0, n, st);
}

// ------------------------------------------------------------------ C ABI
// Scratch of an update (sorted change lists, flags, the new pointer arrays, the block of sizes): one allocation per device,
// kept between calls and grown on demand -- an update of a few ratings would otherwise spend most of its time in hipMalloc /
// hipFree.  A call is synchronous and holds the lock from its first launch to its last read, so the next call finds the
// scratch idle.  Lists whose scratch exceeds GU_SCRATCH_KEEP get an allocation of their own that the call releases.
#define GU_SCRATCH_KEEP ((size_t)64 << 20)
static std::mutex g_gu_lock;
static std::map<int, std::pair<void*, size_t>> g_gu_scratch;      // device -> (allocation, bytes)

static int gu_scratch_get(int device, size_t bytes, void** out, bool* owned) {
  *owned = bytes > GU_SCRATCH_KEEP;
  if (*owned) return hipMalloc(out, bytes) != hipSuccess;
  std::pair<void*, size_t>& c = g_gu_scratch[device];
  if (c.second < bytes) {
    if (c.first) hipFree(c.first);
    c = std::make_pair((void*)nullptr, (size_t)0);
    const size_t want = std::max(bytes, (size_t)1 << 20);
    if (hipMalloc(&c.first, want) != hipSuccess) {
      c.first = nullptr;
      return 1;
    }
    c.second = want;
  }
  *out = c.first;
  return 0;
}

#define GU_TRY(expr, what)                                     \
  do {                                                         \
    if ((expr) != 0) {                                         \
      if (owned) hipFree(scratch);                             \
      ng->mem.release();                                       \
      delete ng;                                               \
      IGMC_FAIL(what);                                         \
    }                                                          \
  } while (0)
extern "C" int igmc_graph_apply(const igmc_graph* g, int n_users_new, int n_items_new, const int32_t* d_user,
                                const int32_t* d_item, const uint8_t* d_rating, int64_t n, void* stream, igmc_graph** out) {
  if (!g || !out) IGMC_FAIL("null argument");
  if (n < 0 || n > ((int64_t)1 << 30)) IGMC_FAIL("n must be in [0, 2^30]");
  if (n > 0 && (!d_user || !d_item || !d_rating)) IGMC_FAIL("null argument");
  if (n_users_new < g->d.n_users || n_items_new < g->d.n_items) IGMC_FAIL("a graph grows or keeps its size, it does not shrink");
  if (n_users_new == INT_MAX || n_items_new == INT_MAX) IGMC_FAIL("sizes must be below 2^31 - 1");
  HIPCHECK(hipSetDevice(g->device));
  std::lock_guard<std::mutex> lock(g_gu_lock);
  hipStream_t st = (hipStream_t)stream;
  GuSide sd[2];
  memset(sd, 0, sizeof(sd));
  sd[0].optr = g->d.u_ptr; sd[0].oidx = g->d.u_idx; sd[0].orel = g->d.u_rel;
  sd[0].rows_old = g->d.n_users; sd[0].rows_new = n_users_new;
  sd[1].optr = g->d.v_ptr; sd[1].oidx = g->d.v_idx; sd[1].orel = g->d.v_rel;
  sd[1].rows_old = g->d.n_items; sd[1].rows_new = n_items_new;
  // the scratch, carved at 256-byte steps
  const int64_t P = igmc_graph_update_padded(n);
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  size_t need = al(sizeof(GuStats));
  for (int s = 0; s < 2; ++s)
    need += al(((size_t)sd[s].rows_new + 1) * 4) + al((size_t)sd[s].rows_new) + al((size_t)P * 8) + al((size_t)P * 4) + 2 * al((size_t)n * 2);
  igmc_graph* ng = new igmc_graph();
  void* scratch = nullptr;
  bool owned = false;
  if (gu_scratch_get(g->device, need, &scratch, &owned)) {
    delete ng;
    IGMC_FAIL("hipMalloc failed");
  }
  char* at = (char*)scratch;
  auto carve = [&](size_t b) { char* p = at; at += al(b); return (void*)p; };
  GuStats* d_st = (GuStats*)carve(sizeof(GuStats));
  for (int s = 0; s < 2; ++s) {
    sd[s].nptr = (int32_t*)carve(((size_t)sd[s].rows_new + 1) * 4);
    sd[s].touched = (uint8_t*)carve((size_t)sd[s].rows_new);
    sd[s].keys = (unsigned long long*)carve((size_t)P * 8);
    sd[s].idx = (uint32_t*)carve((size_t)P * 4);
    sd[s].s_new = (int16_t*)carve((size_t)n * 2);
    sd[s].s_old = (int16_t*)carve((size_t)n * 2);
  }
  GuStats h;
  GU_TRY(hipMemsetAsync(d_st, 0, sizeof(GuStats), st), "hipMemsetAsync failed");
  for (int s = 0; s < 2; ++s)
    igmc_launch_graph_update_plan(sd[s], s, d_user, d_item, d_rating, n, n_users_new, n_items_new, d_st, stream);
  GU_TRY(hipGetLastError(), "a launch failed");
  GU_TRY(hipMemcpyAsync(&h, d_st, sizeof(GuStats), hipMemcpyDeviceToHost, st), "hipMemcpyAsync failed");
  GU_TRY(hipStreamSynchronize(st), "hipStreamSynchronize failed");
  if (h.err & 1) GU_TRY(1, "a user id outside [0, n_users_new)");
  if (h.err & 2) GU_TRY(1, "an item id outside [0, n_items_new)");
  if (h.err & 4) GU_TRY(1, "the resulting nnz must fit int32");
  if (h.nnz[0] != h.nnz[1]) GU_TRY(1, "internal: the two orientations disagree about nnz");
  // the new graph: ONE allocation of exactly its six arrays
  const int64_t nz = h.nnz[0];
  int32_t* fptr[2];
  GU_TRY(ng->mem.reserve(al(((size_t)n_users_new + 1) * 4) + al(((size_t)n_items_new + 1) * 4) +
                         2 * (al((size_t)std::max<int64_t>(nz, 1) * 4) + al((size_t)std::max<int64_t>(nz, 1)))),
         "hipMalloc failed");
  for (int s = 0; s < 2; ++s)
    GU_TRY(ng->mem.get(&fptr[s], (size_t)sd[s].rows_new + 1) || ng->mem.get(&sd[s].nidx, (size_t)nz) ||
               ng->mem.get(&sd[s].nrel, (size_t)nz),
           "hipMalloc failed");
  for (int s = 0; s < 2; ++s) {
    igmc_launch_graph_update_write(sd[s], s, n, g->nnz, d_st, stream);
    GU_TRY(hipMemcpyAsync(fptr[s], sd[s].nptr, ((size_t)sd[s].rows_new + 1) * 4, hipMemcpyDeviceToDevice, st),
           "hipMemcpyAsync failed");
  }
  GU_TRY(hipGetLastError(), "a launch failed");
  GU_TRY(hipMemcpyAsync(&h, d_st, sizeof(GuStats), hipMemcpyDeviceToHost, st), "hipMemcpyAsync failed");
  GU_TRY(hipStreamSynchronize(st), "hipStreamSynchronize failed");
  if (owned) hipFree(scratch);
  ng->device = g->device;
  ng->nnz = nz;
  ng->max_rel = h.max_rel;
  ng->max_deg_u = h.max_deg[0];
  ng->max_deg_v = h.max_deg[1];
  ng->d.n_users = n_users_new;
  ng->d.n_items = n_items_new;
  ng->d.u_ptr = fptr[0]; ng->d.u_idx = sd[0].nidx; ng->d.u_rel = sd[0].nrel;
  ng->d.v_ptr = fptr[1]; ng->d.v_idx = sd[1].nidx; ng->d.v_rel = sd[1].nrel;
  *out = ng;
  return 0;
}
#undef GU_TRY
