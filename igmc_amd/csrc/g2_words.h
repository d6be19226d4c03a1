// g2_words.h -- 8-byte {f32, tag} words that cross workgroups INSIDE a launch (internal): value and tag sit in one store, so
// a reader that sees the tag has the value and no fence is needed.  Used by the subgraph kernel's centre-node readout
// (graphstep2.hip: writer and readers on one XCD) and by the one-launch tail's d att partials (model.hip: any XCD).
#pragma once
#include "common.h"

// ---- the readout words of the subgraph kernel: 8-byte {f32, tag}, polled ------------------------------------------------
// (an ORDINARY 8-byte store: its readers -- g2_poll_f32, sc1 loads -- sit on the writer's XCD and find it in the shared L2
//  ~250 ns after issue; written through to memory with sc1 it took ~570 ns, profiles/r05_experiments/xcd_oneway.txt)
__device__ __forceinline__ void g2_pub_f32(unsigned long long* p, float v, uint32_t tag) {
#ifndef IGMC_HIPEMU
  __hip_atomic_store(p, ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_WAVEFRONT);
#else
  uint32_t bits;
  memcpy(&bits, &v, 4);
  *p = ((unsigned long long)tag << 32) | (unsigned long long)bits;
#endif
}

// ... the same word for readers on ANY XCD: a device-scope store goes past the writer's L2 to the coherent level (one-way
// latency ~550 ns, profiles/r05_experiments/xcd_oneway.txt)
__device__ __forceinline__ void g2_pub_f32_agent(unsigned long long* p, float v, uint32_t tag) {
#ifndef IGMC_HIPEMU
  __hip_atomic_store(p, ((unsigned long long)tag << 32) | (unsigned long long)__float_as_uint(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
#else
  g2_pub_f32(p, v, tag);
#endif
}
// one look at a word (device scope)
__device__ __forceinline__ unsigned long long g2_ld_word(const unsigned long long* p) {
#ifndef IGMC_HIPEMU
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}

// between two looks of a polling loop that holds several words
__device__ __forceinline__ void g2_poll_pause() {
#ifndef IGMC_HIPEMU
  __builtin_amdgcn_s_sleep(2);
#else
  hipemu::yield();
#endif
}

// one 8-byte {f32, tag} word, polled
__device__ __forceinline__ float g2_poll_f32(const unsigned long long* p, uint32_t tag, int* err) {
  for (long it = 0;; ++it) {
#ifndef IGMC_HIPEMU
    const unsigned long long w = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    const unsigned long long w = *p;
#endif
    if ((uint32_t)(w >> 32) == tag) return __uint_as_float((uint32_t)w);
    if (it > (1L << 22)) {
      *err = 1;
      return 0.f;
    }
#ifndef IGMC_HIPEMU
    __builtin_amdgcn_s_sleep(2);
#else
    hipemu::yield();
#endif
  }
}

