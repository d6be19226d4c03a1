// kth_key.h -- THE k-th smallest 32-bit key of a set spread over the workgroup, by byte histograms in LDS, as steps the callers
// compose: extract.hip (sample_fringe: the per-hop cap), candidates.hip (the sampled fill), shortlist.hip (the vote order) and
// holdout.hip (the kept subset of a row).
//   walk(f)   the caller's lambda: f(key) for every key of the set, each key in one thread.  Nothing it reads is written by
//             these steps, so it needs no barriers of its own beyond those of the tile rebuilds it may contain.
//   hist      256 ints of LDS, one bin per thread;  sm: the 16 ints igmc_block_scan_excl shares with the mailbox below.
// A top-byte pass (kth_pass) names the bin b of the r-th key; a bin that kth_parks() is settled by the caller parking its keys
// in a list of IGMC_SAMPLE_PARK entries (in the walk that suits it: extraction FUSES "keep what lies below b" into that walk)
// and counting each against the others (kth_parked_below); a fuller bin by the remaining passes (kth_radix).
// Barriers: every step is entered and left by the whole workgroup.  A mailbox slot is read behind the barrier that follows its
// write and written again only behind the two barriers of a later scan, so the steps need no barrier at their end.
#pragma once
#include "launch.h"

enum {                 // sm[0 .. 8) belongs to igmc_block_scan_excl
  KTH_SM_BIN = 8,      // the bin that holds the r-th key
  KTH_SM_RANK,         // the r-th key's rank inside it (1-based)
  KTH_SM_COUNT,        // keys in it
  KTH_SM_CURSOR,       // the parked list's cursor: zero after every kth_bin
  KTH_SM_T             // the caller's, for a threshold found by one thread
};

struct KthBin {
  uint32_t b;
  int r, c;
};

// the bin of a filled histogram that holds the r-th key (1-based; 1 <= r <= the sum of the bins).  hist may be overwritten
// once this returns: every thread has read its bin before the scan's barriers.
__device__ __forceinline__ KthBin kth_bin(const int* hist, int r, int* sm) {
  const int c = hist[threadIdx.x];
  int tot;
  const int ex = igmc_block_scan_excl(c, &tot, sm);
  if (c > 0 && ex < r && r <= ex + c) {
    sm[KTH_SM_BIN] = (int)threadIdx.x;
    sm[KTH_SM_RANK] = r - ex;
    sm[KTH_SM_COUNT] = c;
  }
  if (threadIdx.x == 0) sm[KTH_SM_CURSOR] = 0;
  __syncthreads();
  return KthBin{(uint32_t)sm[KTH_SM_BIN], sm[KTH_SM_RANK], sm[KTH_SM_COUNT]};
}

// one histogram pass over the byte at `shift` of the keys that agree with `prefix` on `mask`
template <class Walk>
__device__ __forceinline__ KthBin kth_pass(Walk&& walk, uint32_t prefix, uint32_t mask, int shift, int r, int* hist, int* sm) {
  hist[threadIdx.x] = 0;
  __syncthreads();
  walk([&](uint32_t key) {
    if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
  });
  __syncthreads();
  return kth_bin(hist, r, sm);
}

// passes from_pass .. 0 below a settled prefix: returns the r-th key T and leaves in r how many keys EQUAL to T are admitted
// (1 where keys are a bijection, the number of ties taken where they are votes)
template <class Walk>
__device__ __forceinline__ uint32_t kth_radix(Walk&& walk, uint32_t prefix, uint32_t mask, int from_pass, int& r, int* hist,
                                              int* sm) {
#pragma unroll 1        // (one copy of the caller's walk, tile rebuilds included, not from_pass + 1)
  for (int pass = from_pass; pass >= 0; --pass) {
    const int shift = pass * 8;
    const KthBin k = kth_pass(walk, prefix, mask, shift, r, hist, sm);
    prefix |= k.b << shift;
    mask |= 0xFFu << shift;
    r = k.r;
  }
  return prefix;
}

// a bin of c keys fits the parked list (launch.h: the device's constant, the emulator's environment hook)
__device__ __forceinline__ bool kth_parks(int c) { return c <= IGMC_SAMPLE_PARK; }

// thread t < c: how many of the c parked keys lie below ckey[t]
__device__ __forceinline__ int kth_parked_below(const uint32_t* ckey, int c) {
  const uint32_t mine = ckey[threadIdx.x];
  int below = 0;
  for (int j = 0; j < c; ++j) below += ckey[j] < mine;
  return below;
}
