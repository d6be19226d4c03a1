// g2_probe.h -- debug aid (tests/prims_checks.py): the primitives of g2_prims.h / g2_image.h one at a time, so that what each
// form of them (device, CPU stand-in) computes can be held to a restatement of its own -- the split against a bit-level
// round-to-nearest-even, the byte masks per byte, the matrix-core step against the float64 sum of its exact products, the tanh
// and the two instructions it is made of against float64.  Every lane reads its own inputs and stores its own results with
// ordinary per-lane stores; nothing here is on a step's path.  (internal; included once, by graphstep2.hip, after g2_prims.h)
#pragma once
#include "capi.h"

// words a lane reads / writes per item of an op
__host__ __device__ static inline int g2_prims_in_words(int op) {
  return op == IGMC_PRIM_SPLIT ? 2 : op == IGMC_PRIM_MFMA ? 12 : op == IGMC_PRIM_MASK ? 4 : 1;
}
__host__ __device__ static inline int g2_prims_out_words(int op) {
  return op == IGMC_PRIM_SPLIT ? 3 : op == IGMC_PRIM_MFMA ? 4 : op == IGMC_PRIM_MASK ? 8 : 1;
}

template <bool FLAGS>
__device__ __forceinline__ void g2_probe_mask(uint32_t w, uint32_t r1, int keepbit, uint32_t* o) {
  g2_expand4<FLAGS>(w, r1, keepbit, o[0], o[1]);
  const uint32_t m0 = g2_bytemask<FLAGS>(w, r1, keepbit), m1 = g2_bytemask<FLAGS>((w >> 8) | (w << 24), r1, keepbit);
  const u32x4 f = g2_mask_frag(m0, m1);
  o[2] = m0;
  o[3] = m1;
  o[4] = f[0];
  o[5] = f[1];
  o[6] = f[2];
  o[7] = f[3];
}

// items i, i + (threads of the grid), ..: item i's inputs at in + i * in_words, its results at out + i * out_words.  (MFMA: an
// item is one LANE of a wave's step -- n is a whole number of waves, so a wave is in the loop or out of it as one)
__global__ __launch_bounds__(64) void k_g2_prims(int op, const uint32_t* in, int64_t n, uint32_t* out) {
  const int64_t step = (int64_t)gridDim.x * 64;
  for (int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x; i < n; i += step) {
    if (op == IGMC_PRIM_SPLIT) {
      uint32_t h, mi, lo;
      g2_split2(__uint_as_float(in[2 * i]), __uint_as_float(in[2 * i + 1]), h, mi, lo);
      out[3 * i] = h;
      out[3 * i + 1] = mi;
      out[3 * i + 2] = lo;
    } else if (op == IGMC_PRIM_TANH) {
      out[i] = __float_as_uint(g2_tanh(__uint_as_float(in[i])));
    } else if (op == IGMC_PRIM_EXP) {
#ifdef IGMC_HIPEMU
      out[i] = __float_as_uint(expf(__uint_as_float(in[i])));
#else
      out[i] = __float_as_uint(__expf(__uint_as_float(in[i])));
#endif
    } else if (op == IGMC_PRIM_RCP) {
#ifdef IGMC_HIPEMU
      out[i] = __float_as_uint(1.f / __uint_as_float(in[i]));
#else
      out[i] = __float_as_uint(__builtin_amdgcn_rcpf(__uint_as_float(in[i])));
#endif
    } else if (op == IGMC_PRIM_MFMA) {
      const uint32_t* p = in + 12 * i;
      const u32x4 a = {p[0], p[1], p[2], p[3]}, b = {p[4], p[5], p[6], p[7]};
      const f32x4 c = {__uint_as_float(p[8]), __uint_as_float(p[9]), __uint_as_float(p[10]), __uint_as_float(p[11])};
      const f32x4 d = g2_mfma_bf16(a, b, c);
      for (int q = 0; q < 4; ++q) out[4 * i + q] = __float_as_uint(d[q]);
    } else {
      const uint32_t* p = in + 4 * i;
      uint32_t o[8];
      if (p[3]) g2_probe_mask<true>(p[0], p[1], (int)(p[2] & 7u), o);
      else g2_probe_mask<false>(p[0], p[1], (int)(p[2] & 7u), o);
      for (int q = 0; q < 8; ++q) out[8 * i + q] = o[q];
    }
  }
}

// debug aid (tests): one primitive over n items, device buffers of n * {2, 1, 1, 1, 12, 4} input and n * {3, 1, 1, 1, 4, 8} output
// 4-byte words for op = IGMC_PRIM_{SPLIT, TANH, EXP, RCP, MFMA, MASK}:
//   SPLIT (x, y) -> the three packed words of g2_split2;  TANH x -> g2_tanh(x);  EXP / RCP: the two instructions g2_tanh is made of;
//   MFMA  per lane of a wave (n % 64 == 0): A words [4], B words [4], C [4] -> D [4] of one g2_mfma_bf16;
//   MASK  (word, r1, keep bit, FLAGS) -> g2_expand4's two words, g2_bytemask of the word and of the word rotated by one byte,
//         g2_mask_frag of those two masks [4].
// Asynchronous on `stream`.
extern "C" int igmc_debug_g2_prims(int op, const void* in, int64_t n, void* out, void* stream) {
  if (!in || !out) IGMC_FAIL("null argument");
  if (op < 0 || op >= IGMC_PRIM_OPS) IGMC_FAIL("no such op");
  if (n < 0 || n > ((int64_t)1 << 26)) IGMC_FAIL("size out of range");
  if (op == IGMC_PRIM_MFMA && n % 64 != 0) IGMC_FAIL("the matrix-core step takes whole waves");
  if (n == 0) return 0;
  const int grid = (int)std::min<int64_t>((n + 63) / 64, 2048);
  IGMC_LAUNCH(k_g2_prims, grid, 64, 0, stream, op, (const uint32_t*)in, n, (uint32_t*)out);
#ifndef IGMC_HIPEMU
  HIPCHECK(hipGetLastError());
#endif
  return 0;
}
