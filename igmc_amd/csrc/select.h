// select.h -- the 64-bit selection word shared by scores.hip (extremes of one key vector), candidates.hip (the first `num` of
// every segment) and ranking.hip (places in that order): order-preserving image of the float key in the high half, index in the low half.  Words are distinct, so
// "the i-th of the order" is "the i-th smallest word" and minima / maxima of words are associative and commutative.
#pragma once
#include "common.h"

// what the selections of scores.hip, candidates.hip and ranking.hip agree on
#define IGMC_SELECT_MAX_NUM 64
#define IGMC_SEGSEL_MAX_SPLIT 64        // workgroups per segment at most (64 lists of 64 words are what the merge stages)
int igmc_segsel_default_split(int ns);      // candidates.hip; igmc_rank_segments (ranking.hip) splits its segments the same way

#define SEL_LOW_NONE 0xFFFFFFFFFFFFFFFFull      // no word: above every word (a NaN's image is 0xFFFFFFFF, an index < 2^31)
#define SEL_HIGH_NONE 0ull                       // no word: below every word (the image of -inf is 0x007FFFFF)

// order-preserving image of a float: a < b  <=>  image(a) < image(b); -0.0 -> the image of +0.0; every NaN -> 0xFFFFFFFF
__device__ __forceinline__ uint32_t sel_image(float f) {
  if (f != f) return 0xFFFFFFFFu;
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long sel_word(float f, uint32_t idx) {
  return ((unsigned long long)sel_image(f) << 32) | (unsigned long long)idx;
}
// the same word with the key half INVERTED for numbers: a > b  <=>  image(a) < image(b); NaNs stay at 0xFFFFFFFF, behind every
// number (+inf -> 0x007FFFFF ... -inf -> 0xFF800000).  Ascending words = (key descending, index ascending).
__device__ __forceinline__ unsigned long long sel_word_desc(float f, uint32_t idx) {
  const uint32_t im = sel_image(f);
  return ((unsigned long long)(f != f ? im : ~im) << 32) | (unsigned long long)idx;
}
