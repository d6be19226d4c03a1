/* igmc_rng.h -- counter-based hashes shared by the HIP kernels and the C oracle.
 *
 * The reference draws per-hop samples with CPython random.sample over a set
 * (util_functions.py:222-229) and dropout masks with torch RNG streams; neither
 * is reproducible across devices/worker counts.  The engine uses
 * stateless hashes instead, keyed by what identifies the draw:
 *
 *   per-hop sampling : uniform k-subset = the k candidates with the smallest
 *                      igmc_sample_key(salt, id); the key is a BIJECTION of the
 *                      32-bit id for a fixed salt, so keys never tie and the
 *                      selection is an exact uniform k-subset w.r.t. the salt.
 *   dropout          : keep iff igmc_u01(hash) >= p.
 */
#ifndef IGMC_RNG_H
#define IGMC_RNG_H
#include <stdint.h>

#if defined(__HIPCC__) && !defined(IGMC_HIPEMU)
#define IGMC_HD __host__ __device__ static inline
#else
#define IGMC_HD static inline
#endif

IGMC_HD uint64_t igmc_splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

IGMC_HD uint32_t igmc_fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

/* salt for one (dataset seed, epoch, link position, hop distance, side) draw */
IGMC_HD uint64_t igmc_sample_salt(uint64_t seed, uint64_t epoch, uint64_t link, uint32_t dist, uint32_t side) {
  uint64_t s = igmc_splitmix64(seed ^ 0x49474D43ull);
  s = igmc_splitmix64(s ^ epoch);
  s = igmc_splitmix64(s ^ link);
  s = igmc_splitmix64(s ^ (((uint64_t)dist << 1) | side));
  return s;
}

/* salt for the sampled negatives of one (dataset seed, draw, user ID): keyed by the id, not by the user's place in a request,
 * so a user's negatives do not depend on the users asked for with it */
IGMC_HD uint64_t igmc_negative_salt(uint64_t seed, uint64_t draw, uint64_t user) {
  uint64_t s = igmc_splitmix64(seed ^ 0x4E454753ull);
  s = igmc_splitmix64(s ^ draw);
  s = igmc_splitmix64(s ^ user);
  return s;
}

/* salt for the Given-k split of one (dataset seed, draw, user ID) (igmc_holdout_fill): the kept entries of the user's row are
 * those with the smallest igmc_sample_key(salt, item).  Keyed by the id, not by the user's place in a request, so a user's split
 * does not depend on the users asked for with it, on their order or on the grid.  The key order of a row does not depend on how
 * many entries are kept: with no limit on the held entries the kept sets are NESTED, kept(k) is a subset of kept(k + 1). */
IGMC_HD uint64_t igmc_holdout_salt(uint64_t seed, uint64_t draw, uint64_t user) {
  uint64_t s = igmc_splitmix64(seed ^ 0x484F4C44ull); /* "HOLD" */
  s = igmc_splitmix64(s ^ draw);
  s = igmc_splitmix64(s ^ user);
  return s;
}

/* salt for the negative of one (dataset seed, epoch, positive link) of pair training: `pos` is the positive's position in the
 * pair list, not its place in a batch, so a link's negative does not depend on the shuffle or on the batch size */
IGMC_HD uint64_t igmc_pair_salt(uint64_t seed, uint64_t epoch, uint64_t pos) {
  uint64_t s = igmc_splitmix64(seed ^ 0x50414952ull);
  s = igmc_splitmix64(s ^ epoch);
  s = igmc_splitmix64(s ^ pos);
  return s;
}

/* try t of a pair's negative: an item id in [0, n_items) by multiply-shift of 32 hashed bits -- no division; an item is hit by
 * floor or ceil of 2^32 / n_items of the 2^32 words, so the bias of any item's probability is at most n_items / 2^32 relative */
IGMC_HD uint32_t igmc_pair_candidate(uint64_t salt, uint64_t t, uint32_t n_items) {
  return (uint32_t)(((igmc_splitmix64(salt ^ t) >> 32) * (uint64_t)n_items) >> 32);
}

/* igmc_pair_negatives_shortlist: two more words of a pair's salt, under keys no try index can equal (tries stop below 2^20).
 * KEY_HARD decides whether the negative is asked of the user's shortlist segment, KEY_PICK which of its entries. */
#define IGMC_PAIR_KEY_HARD 0x4841524400000000ull /* "HARD" << 32 */
#define IGMC_PAIR_KEY_PICK 0x5049434B00000000ull /* "PICK" << 32 */

/* floor(hard_share * 2^32) for hard_share in [0, 1]: exact in double; 0 never decides hard, 2^32 always does */
IGMC_HD uint64_t igmc_pair_hard_threshold(double hard_share) { return (uint64_t)(hard_share * 4294967296.0); }

/* the pair asks the shortlist iff 32 hashed bits fall below the threshold */
IGMC_HD int igmc_pair_hard(uint64_t salt, uint64_t thr) { return (igmc_splitmix64(salt ^ IGMC_PAIR_KEY_HARD) >> 32) < thr; }

/* the entry of a segment of `len` entries (1 <= len < 2^31) a hard-decided pair picks: the multiply-shift of igmc_pair_candidate */
IGMC_HD uint32_t igmc_pair_pick(uint64_t salt, uint32_t len) {
  return (uint32_t)(((igmc_splitmix64(salt ^ IGMC_PAIR_KEY_PICK) >> 32) * (uint64_t)len) >> 32);
}

/* bijective in `id` for fixed salt */
IGMC_HD uint32_t igmc_sample_key(uint64_t salt, uint32_t id) {
  return igmc_fmix32(igmc_fmix32(id + (uint32_t)salt) ^ (uint32_t)(salt >> 32));
}

/* edge dropout: dir = 0 user->item, 1 item->user, 2 undirected (force_undirected) */
IGMC_HD uint32_t igmc_edge_hash(uint64_t seed, uint64_t step, uint32_t graph, uint32_t u, uint32_t v, uint32_t dir) {
  uint64_t s = igmc_splitmix64(seed ^ 0x45444745ull);
  s = igmc_splitmix64(s ^ step);
  s = igmc_splitmix64(s ^ (((uint64_t)graph << 2) | dir));
  s = igmc_splitmix64(s ^ (((uint64_t)u << 32) | v));
  return (uint32_t)(s >> 32);
}

/* MLP dropout(0.5) on hidden unit j of graph g */
IGMC_HD uint32_t igmc_unit_hash(uint64_t seed, uint64_t step, uint32_t graph, uint32_t j) {
  uint64_t s = igmc_splitmix64(seed ^ 0x4D4C5044ull);
  s = igmc_splitmix64(s ^ step);
  s = igmc_splitmix64(s ^ (((uint64_t)graph << 32) | j));
  return (uint32_t)(s >> 32);
}

/* uniform in [0,1) with 24 bits */
IGMC_HD float igmc_u01(uint32_t h) { return (float)(h >> 8) * (1.0f / 16777216.0f); }

#endif /* IGMC_RNG_H */
