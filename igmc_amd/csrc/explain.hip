// explain.hip -- leave-one-out neighbour attribution of a prediction (no reference counterpart: the reference's `visualize`
// draws an enclosing subgraph and leaves the reading to the eye; by hand an attribution is the subgraph pulled to the host,
// one node deleted, the node sets rebuilt in Python and pushed through igmc_extract_batch_replay, one variant at a time).
//
// A prediction is a function of one enclosing subgraph.  For the link in slot g of an extracted arena, with users U[0..nu) and
// items V[0..nv) in slot order (target first, the rest by ascending id), its VARIANTS are, in this order,
//     0                   the whole node set (the base)
//     1 .. nu-1           the set without user U[k]
//     nu .. nu+nv-2       the set without item V[k - nu + 1]
// every remaining node with the hop distance it has in the whole set.  The kernels here write the variants of a batch of links
// into a node-set cache of the format igmc_extract_batch_cached reads (so the ordinary cached extraction + forward scores
// them), and turn the variant scores into attributions score(variant) - score(base).
//
// k_loo_count   per link: the variants nu + nv - 1 and the user / item entries they occupy in the cache,
//                   users  nu + (nu-1)(nu-1) + (nv-1) nu        items  nv + (nu-1) nv + (nv-1)(nv-1)
//               from n_users / n_items alone (lean arenas, arenas without dense blocks; no CSR is asked for).
// k_loo_fill    workgroup (g, c) of a (B, chunks) grid takes the variants 4 c + w, 4 (c + chunks) + w, ... of link g, wave w one
//               variant at a time: a variant's places in the cache follow in closed form from the link's three base offsets
//               (below: loo_places), so no variant waits for another and a 128 + 128 link spreads its 255 variants over
//               4 * chunks waves.  The copy is "the slot's list minus one element", lane i taking elements i, i + 64, ...;
//               ids from s_gid, distances from s_lab (label / 2).  Output = a function of the inputs alone, whatever the
//               grid: every word has one writer but the variants' END offset uoff / voff[var_off + nvar], which the next link
//               writes too -- with the same value, or the launch raises error bit 3.
//               var_rating: the entry (removed user, target item) / (target user, removed item) of the rating graph.  Rows are
//               sorted by (relation, id), not by id, so a row cannot be bisected as a whole; the wave SCANS the shorter of the
//               removed node's own row and the opposite target's row, 64 entries a step.  On a 2 400-entry row that is 38
//               coalesced 256-byte loads per variant when both are that long (bisecting each of R relation runs instead would
//               be ~2 R log2(2400) = 110 dependent loads of one lane at R = 5); the common case is a short row on one side.
// k_loo_deltas  workgroup per link: base = score of variant 0, delta = score - base and key = |delta| of the others, filed at
//               seg_off[i] = var_off[i] - i -- the base entries drop out, the attribution segments are contiguous and go
//               straight into igmc_select_segments.  A NaN score gives a NaN key, which that selection ranks last.
//
// Plain vector stores only, no float atomics (error word: a vector atomic OR, reached on errors only).
#include "capi.h"
#include <math.h>
#include <stdlib.h>

struct LooPlaces {
  int64_t u, v;      // first user / item entry of the variant, relative to the link's base offsets
  int skip_u, skip_v;      // slot index left out on each side (0: none -- the targets are never removed)
};

// variant k of a link with nu users and nv items
__device__ __forceinline__ LooPlaces loo_places(int k, int nu, int nv) {
  LooPlaces p;
  if (k == 0) {
    p.u = 0; p.v = 0; p.skip_u = 0; p.skip_v = 0;
  } else if (k < nu) {
    p.u = (int64_t)nu + (int64_t)(k - 1) * (nu - 1);
    p.v = (int64_t)nv + (int64_t)(k - 1) * nv;
    p.skip_u = k; p.skip_v = 0;
  } else {
    p.u = (int64_t)nu + (int64_t)(nu - 1) * (nu - 1) + (int64_t)(k - nu) * nu;
    p.v = (int64_t)nv + (int64_t)(nu - 1) * nv + (int64_t)(k - nu) * (nv - 1);
    p.skip_u = 0; p.skip_v = k - nu + 1;
  }
  return p;
}
__device__ __forceinline__ int64_t loo_uent(int nu, int nv) { return (int64_t)nu + (int64_t)(nu - 1) * (nu - 1) + (int64_t)(nv - 1) * nu; }
__device__ __forceinline__ int64_t loo_vent(int nu, int nv) { return (int64_t)nv + (int64_t)(nu - 1) * nv + (int64_t)(nv - 1) * (nv - 1); }

__global__ __launch_bounds__(IGMC_BLOCK) void k_loo_count(const int32_t* __restrict__ n_users, const int32_t* __restrict__ n_items,
                                                           int B, int64_t* __restrict__ nvar, int64_t* __restrict__ nu_ids,
                                                           int64_t* __restrict__ nv_ids) {
  for (int g = blockIdx.x * IGMC_BLOCK + threadIdx.x; g < B; g += gridDim.x * IGMC_BLOCK) {
    const int nu = n_users[g], nv = n_items[g];
    const bool ok = nu >= 1 && nv >= 1;        // (an arena nothing was extracted into: the fill reports it)
    nvar[g] = ok ? (int64_t)nu + nv - 1 : 0;
    nu_ids[g] = ok ? loo_uent(nu, nv) : 0;
    nv_ids[g] = ok ? loo_vent(nu, nv) : 0;
  }
}

struct LooFill {
  GraphDev g;
  const int32_t* n_users;      // the arena: sizes and slots
  const int32_t* n_items;
  const int32_t* s_gid;
  const uint8_t* s_lab;
  int cap_u, cap_v, slot;
  int B;
  int64_t link0;
  const int64_t* var_off;      // [B + 1] each
  const int64_t* uent_off;
  const int64_t* vent_off;
  int64_t cap_var, cap_uent, cap_vent;
  int64_t* uoff;               // [cap_var + 1]
  int32_t* unodes;             // [cap_uent]
  uint8_t* udist;
  int64_t* voff;
  int32_t* vnodes;             // [cap_vent]
  uint8_t* vdist;
  int32_t* var_link;           // [cap_var] each
  uint8_t* var_side;
  int32_t* var_node;
  uint8_t* var_rating;
  int32_t* err;
};

// rating + 1 of the entry (row, col) of one orientation, 0 if there is none: the wave scans the row (see the head comment)
__device__ __forceinline__ int loo_row_find(const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                            const uint8_t* __restrict__ rel, int row, int col, int lane) {
  const int lo = ptr[row], hi = ptr[row + 1];
  int found = 0;
  for (int p = lo + lane; p < hi; p += 64)
    if (idx[p] == col) found = (int)rel[p] + 1;      // (a pair has one entry at most)
  return found;
}

__global__ __launch_bounds__(IGMC_BLOCK) void k_loo_fill(LooFill a) {
  igmc_kernarg_warm<sizeof(LooFill)>();
  const int g = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = IGMC_BLOCK >> 6;
  const int nu = a.n_users[g], nv = a.n_items[g];
  const int64_t v0 = a.var_off[g], ue0 = a.uent_off[g], ve0 = a.vent_off[g];
  // (everything below is uniform over the workgroups of link g: all of them write, or none)
  int bad = 0;
  if (nu < 1 || nv < 1 || nu > a.cap_u || nv > a.cap_v) {
    bad = 16;                                                  // bit 4: no extracted link in the slot
  } else {
    const int64_t nvar = (int64_t)nu + nv - 1, ue = loo_uent(nu, nv), ve = loo_vent(nu, nv);
    if (v0 < 0 || ue0 < 0 || ve0 < 0 || a.var_off[g + 1] - v0 != nvar || a.uent_off[g + 1] - ue0 != ue ||
        a.vent_off[g + 1] - ve0 != ve)
      bad = 8;                                                 // bit 3: the offsets are not the prefix sums of the counts
    else
      bad = (v0 + nvar > a.cap_var ? 1 : 0) | (ue0 + ue > a.cap_uent ? 2 : 0) | (ve0 + ve > a.cap_vent ? 4 : 0);      // bits 0..2: a capacity
  }
  if (bad) {
    if (blockIdx.y == 0 && threadIdx.x == 0) atomicOr(a.err, bad);
    return;                                                    // (nothing of this link is written)
  }
  const int nvar = nu + nv - 1;
  const int32_t* sg = a.s_gid + (size_t)g * a.slot;
  const uint8_t* sl = a.s_lab + (size_t)g * a.slot;
  const int tu = sg[0], tv = sg[a.cap_u];
  if (blockIdx.y == 0 && threadIdx.x == 0) {      // the end of the link's last variant
    a.uoff[v0 + nvar] = ue0 + loo_uent(nu, nv);
    a.voff[v0 + nvar] = ve0 + loo_vent(nu, nv);
  }
  for (int k = (int)blockIdx.y * nwave + wave; k < nvar; k += (int)gridDim.y * nwave) {
    const LooPlaces p = loo_places(k, nu, nv);
    const int cu = nu - (p.skip_u ? 1 : 0), cv = nv - (p.skip_v ? 1 : 0);
    int32_t* un = a.unodes + ue0 + p.u;
    uint8_t* ud = a.udist + ue0 + p.u;
    for (int i = lane; i < cu; i += 64) {
      const int s = i + ((p.skip_u && i >= p.skip_u) ? 1 : 0);
      un[i] = sg[s];
      ud[i] = (uint8_t)(sl[s] >> 1);
    }
    int32_t* vn = a.vnodes + ve0 + p.v;
    uint8_t* vd = a.vdist + ve0 + p.v;
    for (int i = lane; i < cv; i += 64) {
      const int s = a.cap_u + i + ((p.skip_v && i >= p.skip_v) ? 1 : 0);
      vn[i] = sg[s];
      vd[i] = (uint8_t)(sl[s] >> 1);
    }
    int node = -1, rating = 0;
    if (p.skip_u) {
      node = sg[p.skip_u];
      const bool own = a.g.u_ptr[node + 1] - a.g.u_ptr[node] <= a.g.v_ptr[tv + 1] - a.g.v_ptr[tv];
      rating = own ? loo_row_find(a.g.u_ptr, a.g.u_idx, a.g.u_rel, node, tv, lane)
                   : loo_row_find(a.g.v_ptr, a.g.v_idx, a.g.v_rel, tv, node, lane);
    } else if (p.skip_v) {
      node = sg[a.cap_u + p.skip_v];
      const bool own = a.g.v_ptr[node + 1] - a.g.v_ptr[node] <= a.g.u_ptr[tu + 1] - a.g.u_ptr[tu];
      rating = own ? loo_row_find(a.g.v_ptr, a.g.v_idx, a.g.v_rel, node, tu, lane)
                   : loo_row_find(a.g.u_ptr, a.g.u_idx, a.g.u_rel, tu, node, lane);
    }
    rating = igmc_wave_sum_i(rating);      // (one lane at most found the entry)
    if (lane == 0) {
      a.uoff[v0 + k] = ue0 + p.u;
      a.voff[v0 + k] = ve0 + p.v;
      a.var_link[v0 + k] = (int32_t)(a.link0 + g);
      a.var_side[v0 + k] = (uint8_t)(p.skip_u ? 0 : p.skip_v ? 1 : 255);
      a.var_node[v0 + k] = node;
      a.var_rating[v0 + k] = (uint8_t)rating;
    }
  }
}

__global__ __launch_bounds__(IGMC_BLOCK) void k_loo_deltas(const float* __restrict__ scores, const int64_t* __restrict__ var_off,
                                                            int64_t n_links, float* __restrict__ base_out,
                                                            float* __restrict__ delta, float* __restrict__ key,
                                                            const int64_t* __restrict__ seg_off) {
  for (int64_t i = blockIdx.x; i < n_links; i += gridDim.x) {
    const int64_t lo = var_off[i], hi = var_off[i + 1], s0 = seg_off[i];
    if (hi <= lo) {        // (a link without variants: no score to take a base from)
      if (threadIdx.x == 0) base_out[i] = 0.f;
      continue;
    }
    const float base = scores[lo];
    if (threadIdx.x == 0) base_out[i] = base;
    for (int64_t k = 1 + threadIdx.x; k < hi - lo; k += IGMC_BLOCK) {
      const float d = scores[lo + k] - base;
      delta[s0 + k - 1] = d;
      key[s0 + k - 1] = fabsf(d);
    }
  }
}

// ------------------------------------------------------------------ host
struct LooCache {
  const int64_t* var_off;   // [B + 1] each: the batch's slice of the prefix sums of the three counts
  const int64_t* uent_off;
  const int64_t* vent_off;
  int64_t cap_var, cap_uent, cap_vent;
  int64_t* uoff;            // [cap_var + 1]  the cache arrays igmc_launch_load_nodes reads
  int32_t* unodes;          // [cap_uent]
  uint8_t* udist;
  int64_t* voff;
  int32_t* vnodes;          // [cap_vent]
  uint8_t* vdist;
  int32_t* var_link;        // [cap_var] each
  uint8_t* var_side;
  int32_t* var_node;
  uint8_t* var_rating;
};
static void igmc_launch_loo_count(const BatchDev& b, int B, int64_t* nvar, int64_t* nu_ids, int64_t* nv_ids, void* stream) {
  IGMC_PLAUNCH("k_loo_count", k_loo_count, (B + IGMC_BLOCK - 1) / IGMC_BLOCK, IGMC_BLOCK, 0, stream, (const int32_t*)b.n_users,
               (const int32_t*)b.n_items, B, nvar, nu_ids, nv_ids);
}

// workgroups per link of the fill where the caller names none: 16 x 4 waves take a 128 + 128 link's 255 variants in four rounds
static int igmc_loo_default_chunks() {
  const char* e = getenv("IGMC_LOO_CHUNKS");      // (test hook: the output does not depend on it)
  const int c = e ? atoi(e) : 16;
  return c < 1 ? 1 : c > 1024 ? 1024 : c;
}

static void igmc_launch_loo_fill(const GraphDev& g, const BatchDev& b, int B, int64_t link0, const LooCache& c, int chunks, int32_t* err,
                          void* stream) {
  LooFill a;
  a.g = g;
  a.n_users = b.n_users; a.n_items = b.n_items; a.s_gid = b.s_gid; a.s_lab = b.s_lab;
  a.cap_u = b.cap_u; a.cap_v = b.cap_v; a.slot = b.slot;
  a.B = B; a.link0 = link0;
  a.var_off = c.var_off; a.uent_off = c.uent_off; a.vent_off = c.vent_off;
  a.cap_var = c.cap_var; a.cap_uent = c.cap_uent; a.cap_vent = c.cap_vent;
  a.uoff = c.uoff; a.unodes = c.unodes; a.udist = c.udist; a.voff = c.voff; a.vnodes = c.vnodes; a.vdist = c.vdist;
  a.var_link = c.var_link; a.var_side = c.var_side; a.var_node = c.var_node; a.var_rating = c.var_rating;
  a.err = err;
  IGMC_PLAUNCH("k_loo_fill", k_loo_fill, dim3(B, chunks), IGMC_BLOCK, 0, stream, a);
}

static void igmc_launch_loo_deltas(const float* scores, const int64_t* var_off, int64_t n_links, float* base, float* delta, float* key,
                            const int64_t* seg_off, void* stream) {
  const int grid = (int)(n_links < 1 ? 1 : n_links > 65536 ? 65536 : n_links);
  IGMC_PLAUNCH("k_loo_deltas", k_loo_deltas, grid, IGMC_BLOCK, 0, stream, scores, var_off, n_links, base, delta, key, seg_off);
}

// ------------------------------------------------------------------ C ABI
extern "C" int igmc_loo_count(const igmc_batch* base, int B, int64_t* d_nvar, int64_t* d_nu_ids, int64_t* d_nv_ids,
                              void* stream) {
  if (!base || !d_nvar || !d_nu_ids || !d_nv_ids) IGMC_FAIL("null argument");
  if (B < 1 || B > base->last_B) IGMC_FAIL("B must be in [1, the number of links extracted into the arena]");
  igmc_launch_loo_count(base->d, B, d_nvar, d_nu_ids, d_nv_ids, stream);      // (sizes only: a lean arena is not made to emit)
  HIPCHECK(hipGetLastError());
  return 0;
}
extern "C" int igmc_loo_fill(const igmc_graph* g, const igmc_batch* base, int B, int64_t link0, const int64_t* d_var_off,
                             const int64_t* d_uent_off, const int64_t* d_vent_off, int64_t cap_var, int64_t cap_uent,
                             int64_t cap_vent, int64_t* d_uoff, int32_t* d_unodes, uint8_t* d_udist, int64_t* d_voff,
                             int32_t* d_vnodes, uint8_t* d_vdist, int32_t* d_var_link, uint8_t* d_var_side,
                             int32_t* d_var_node, uint8_t* d_var_rating, int32_t* d_err, void* stream) {
  if (!g || !base || base->g != g) IGMC_FAIL("the arena does not belong to this graph");
  if (B < 1 || B > base->last_B) IGMC_FAIL("B must be in [1, the number of links extracted into the arena]");
  if (!d_var_off || !d_uent_off || !d_vent_off || !d_uoff || !d_unodes || !d_udist || !d_voff || !d_vnodes || !d_vdist ||
      !d_var_link || !d_var_side || !d_var_node || !d_var_rating || !d_err)
    IGMC_FAIL("null argument");
  if (cap_var < 1 || cap_uent < 1 || cap_vent < 1) IGMC_FAIL("capacities must be at least 1");
  if (link0 < 0 || link0 + B > (int64_t)INT32_MAX) IGMC_FAIL("link indices must stay below 2^31");
  LooCache c;
  c.var_off = d_var_off; c.uent_off = d_uent_off; c.vent_off = d_vent_off;
  c.cap_var = cap_var; c.cap_uent = cap_uent; c.cap_vent = cap_vent;
  c.uoff = d_uoff; c.unodes = d_unodes; c.udist = d_udist; c.voff = d_voff; c.vnodes = d_vnodes; c.vdist = d_vdist;
  c.var_link = d_var_link; c.var_side = d_var_side; c.var_node = d_var_node; c.var_rating = d_var_rating;
  igmc_launch_loo_fill(g->d, base->d, B, link0, c, igmc_loo_default_chunks(), d_err, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
extern "C" int igmc_loo_deltas(const float* d_scores, const int64_t* d_var_off, int64_t n_links, float* d_base, float* d_delta,
                               float* d_key, const int64_t* d_seg_off, void* stream) {
  if (!d_scores || !d_var_off || !d_base || !d_delta || !d_key || !d_seg_off) IGMC_FAIL("null argument");
  if (n_links < 1 || n_links > (int64_t)INT32_MAX) IGMC_FAIL("n_links must be in [1, 2^31)");
  igmc_launch_loo_deltas(d_scores, d_var_off, n_links, d_base, d_delta, d_key, d_seg_off, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
