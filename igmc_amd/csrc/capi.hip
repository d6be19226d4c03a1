// capi.hip -- C-ABI host layer of libigmc_hip.so (see include/igmc_hip.h for the contract): the handle objects and the calls
// that run the model.  A serving family's entry points stand in the family's own file, the gradient exchange in comm.hip.
#include "capi.h"
#include "sortpool.h"
#include "g2_image.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>

std::string& igmc_err() {
  static thread_local std::string err;
  return err;
}
int g_igmc_prof_on = 0;
extern int g_igmc_compose_count;      // graphstep2.hip: launches of k_g2_compose so far

// One call's view of the images: the compose launch is skipped when the caller asserted unchanged parameters AND the
// library knows the images in place are those of the previous call's (possibly updated) parameters.
struct ImgScope {
  igmc_model* m;
  const float* p;
  int cur, before;
  ImgScope(igmc_model* m_, const float* p_) : m(m_), p(p_) {
    cur = m->img_hint && m->img_valid && m->img_params == p;
    m->img_hint = 0;
    m->d.img_current = cur;
    before = g_igmc_compose_count;
  }
  void done_unchanged() {       // the call left the parameters as they were
    m->img_valid = cur || g_igmc_compose_count != before;
    m->img_params = p;
    m->d.img_current = 0;
  }
  void done_updated(int emitted) {      // the call updated the parameters (images: only if its last kernel wrote them)
    m->img_valid = emitted;
    m->img_params = p;
    m->d.img_current = 0;
  }
};

extern "C" int igmc_model_weights_unchanged(igmc_model* m, int on) {
  if (!m) IGMC_FAIL("null model");
  m->img_hint = on ? 1 : 0;
  return 0;
}

extern "C" const char* igmc_last_error(void) { return igmc_err().c_str(); }
extern "C" int igmc_version(void) { return 100; }

// ------------------------------------------------------------------ profiling
struct ProfRec {
  std::string name;
  hipEvent_t a, b;
};
static std::vector<ProfRec> g_prof;

void igmc_prof_begin(const char* name, void* stream) {
  ProfRec r;
  r.name = name;
  hipEventCreate(&r.a);
  hipEventCreate(&r.b);
  hipEventRecord(r.a, (hipStream_t)stream);
  g_prof.push_back(r);
}
void igmc_prof_end(void* stream) { hipEventRecord(g_prof.back().b, (hipStream_t)stream); }

// on = 1: HIP events around every kernel launch (eager launches only; igmc_profile_fetch).
// on = 2: no events (legal inside hipGraph capture); k_graph_step launches enqueued / captured from now on clock
//         themselves on the device (igmc_profile_gs_clock).
extern "C" int igmc_profile_enable(int on) {
  g_igmc_prof_on = on;
  return 0;
}

// Launch clock of k_graph_step since the last reset: launches, mean duration in microseconds (device wall clock,
// earliest workgroup start -> last workgroup end).  Synchronises the device.
extern "C" int igmc_profile_gs_clock(const igmc_model* m, int64_t* launches, double* mean_us, int reset) {
  if (!m) IGMC_FAIL("null model");
  unsigned long long ts[4];
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(ts, m->d.gs_ts, sizeof(ts), hipMemcpyDeviceToHost));
  int khz = 0;
#ifndef IGMC_HIPEMU
  HIPCHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, m->device));
#endif
  if (launches) *launches = (int64_t)ts[2];
  if (mean_us) *mean_us = (ts[2] && khz > 0) ? (double)ts[1] / (double)ts[2] * 1e3 / (double)khz : 0.0;
  if (reset) {
    const unsigned long long ts0[4] = {~0ull, 0ull, 0ull, 0ull};
    HIPCHECK(hipMemcpy(m->d.gs_ts, ts0, sizeof(ts0), hipMemcpyHostToDevice));
  }
  return 0;
}

extern "C" int igmc_profile_fetch(char names[][48], float* ms, int* calls, int cap) {
  std::vector<std::string> order;
  std::map<std::string, std::pair<double, int>> agg;
  for (auto& r : g_prof) {
    hipEventSynchronize(r.b);
    float t = 0.f;
    hipEventElapsedTime(&t, r.a, r.b);
    if (!agg.count(r.name)) order.push_back(r.name);
    agg[r.name].first += t;
    agg[r.name].second += 1;
    hipEventDestroy(r.a);
    hipEventDestroy(r.b);
  }
  g_prof.clear();
  int n = 0;
  for (auto& nm : order) {
    if (n >= cap) break;
    snprintf(names[n], 48, "%s", nm.c_str());
    ms[n] = (float)agg[nm].first;
    if (calls) calls[n] = agg[nm].second;
    ++n;
  }
  return n;
}

// ------------------------------------------------------------------ rating graph
extern "C" int igmc_graph_create(int n_users, int n_items, int64_t nnz, const int32_t* h_indptr,
                                 const int32_t* h_indices, const uint8_t* h_rating, int device,
                                 igmc_graph** out) {
  if (n_users <= 0 || n_items <= 0 || nnz < 0 || !h_indptr || !out) IGMC_FAIL("bad arguments");
  if (nnz >= INT_MAX) IGMC_FAIL("nnz must fit int32");
  HIPCHECK(hipSetDevice(device));
  // drop explicit zeros, convert label+1 -> relation id, sort rows by (relation, item)
  std::vector<int32_t> uptr(n_users + 1, 0), uidx, vptr(n_items + 1, 0), vidx;
  std::vector<uint8_t> urel, vrel;
  uidx.reserve(nnz);
  urel.reserve(nnz);
  int max_rel = 0;
  std::vector<std::pair<int32_t, int32_t>> row;   // (rel, item)
  for (int u = 0; u < n_users; ++u) {
    row.clear();
    for (int32_t p = h_indptr[u]; p < h_indptr[u + 1]; ++p) {
      if (h_rating[p] == 0) continue;
      const int it = h_indices[p];
      if (it < 0 || it >= n_items) IGMC_FAIL("column index out of range");
      row.emplace_back((int32_t)h_rating[p] - 1, it);
    }
    std::sort(row.begin(), row.end());
    for (size_t k = 1; k < row.size(); ++k)
      if (row[k].second == row[k - 1].second && row[k].first == row[k - 1].first) IGMC_FAIL("duplicate entries in CSR row");
    for (auto& e : row) {
      urel.push_back((uint8_t)e.first);
      uidx.push_back(e.second);
      max_rel = std::max(max_rel, (int)e.first);
      vptr[e.second + 1]++;
    }
    uptr[u + 1] = (int32_t)uidx.size();
  }
  const int64_t nz = (int64_t)uidx.size();
  for (int v = 0; v < n_items; ++v) vptr[v + 1] += vptr[v];
  vidx.assign(nz, 0);
  vrel.assign(nz, 0);
  {
    // counting sort by (item, relation, user): pass over relations keeps columns relation-sorted
    std::vector<int32_t> cur(vptr.begin(), vptr.end() - 1);
    for (int r = 0; r <= max_rel; ++r)
      for (int u = 0; u < n_users; ++u)
        for (int32_t p = uptr[u]; p < uptr[u + 1]; ++p)
          if (urel[p] == r) {
            const int32_t q = cur[uidx[p]]++;
            vidx[q] = u;
            vrel[q] = (uint8_t)r;
          }
  }
  igmc_graph* g = new igmc_graph();
  g->device = device;
  g->nnz = nz;
  g->max_rel = max_rel;
  g->max_deg_u = g->max_deg_v = 0;
  for (int u = 0; u < n_users; ++u) g->max_deg_u = std::max(g->max_deg_u, uptr[u + 1] - uptr[u]);
  for (int v = 0; v < n_items; ++v) g->max_deg_v = std::max(g->max_deg_v, vptr[v + 1] - vptr[v]);
  int32_t *d_uptr, *d_uidx, *d_vptr, *d_vidx;
  uint8_t *d_urel, *d_vrel;
  if (g->mem.get(&d_uptr, n_users + 1) || g->mem.get(&d_uidx, nz) || g->mem.get(&d_urel, nz) ||
      g->mem.get(&d_vptr, n_items + 1) || g->mem.get(&d_vidx, nz) || g->mem.get(&d_vrel, nz)) {
    g->mem.release();
    delete g;
    IGMC_FAIL("hipMalloc failed");
  }
  HIPCHECK(hipMemcpy(d_uptr, uptr.data(), (n_users + 1) * 4, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(d_vptr, vptr.data(), (n_items + 1) * 4, hipMemcpyHostToDevice));
  if (nz) {
    HIPCHECK(hipMemcpy(d_uidx, uidx.data(), nz * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_urel, urel.data(), nz, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_vidx, vidx.data(), nz * 4, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(d_vrel, vrel.data(), nz, hipMemcpyHostToDevice));
  }
  g->d.n_users = n_users;
  g->d.n_items = n_items;
  g->d.u_ptr = d_uptr; g->d.u_idx = d_uidx; g->d.u_rel = d_urel;
  g->d.v_ptr = d_vptr; g->d.v_idx = d_vidx; g->d.v_rel = d_vrel;
  *out = g;
  return 0;
}

extern "C" void igmc_graph_destroy(igmc_graph* g) {
  if (!g) return;
  g->mem.release();
  delete g;
}
extern "C" int64_t igmc_graph_hbm_bytes(const igmc_graph* g) { return g ? (int64_t)g->mem.bytes : 0; }

extern "C" int igmc_graph_info(const igmc_graph* g, int64_t out6[6]) {
  if (!g || !out6) IGMC_FAIL("null argument");
  out6[0] = g->d.n_users;
  out6[1] = g->d.n_items;
  out6[2] = g->nnz;
  out6[3] = g->max_rel;
  out6[4] = g->max_deg_u;
  out6[5] = g->max_deg_v;
  return 0;
}

extern "C" int igmc_graph_download(const igmc_graph* g, int32_t* u_ptr, int32_t* u_idx, uint8_t* u_rel, int32_t* v_ptr,
                                   int32_t* v_idx, uint8_t* v_rel) {
  if (!g) IGMC_FAIL("null argument");
  HIPCHECK(hipSetDevice(g->device));
  const size_t nz = (size_t)g->nnz;
  if (u_ptr) HIPCHECK(hipMemcpy(u_ptr, g->d.u_ptr, ((size_t)g->d.n_users + 1) * 4, hipMemcpyDeviceToHost));
  if (v_ptr) HIPCHECK(hipMemcpy(v_ptr, g->d.v_ptr, ((size_t)g->d.n_items + 1) * 4, hipMemcpyDeviceToHost));
  if (nz) {
    if (u_idx) HIPCHECK(hipMemcpy(u_idx, g->d.u_idx, nz * 4, hipMemcpyDeviceToHost));
    if (u_rel) HIPCHECK(hipMemcpy(u_rel, g->d.u_rel, nz, hipMemcpyDeviceToHost));
    if (v_idx) HIPCHECK(hipMemcpy(v_idx, g->d.v_idx, nz * 4, hipMemcpyDeviceToHost));
    if (v_rel) HIPCHECK(hipMemcpy(v_rel, g->d.v_rel, nz, hipMemcpyDeviceToHost));
  }
  return 0;
}

// ------------------------------------------------------------------ batch arena
extern "C" int igmc_batch_create(const igmc_graph* g, int max_graphs, int hop, int max_nodes_per_hop,
                                 igmc_batch** out) {
  if (!g || !out || max_graphs <= 0 || hop < 1) IGMC_FAIL("bad arguments");
  if (2 * hop + 2 > 250) IGMC_FAIL("hop too large");
  HIPCHECK(hipSetDevice(g->device));
  const size_t smem = igmc_extract_smem_bytes(g->d);
  if (smem > 150 * 1024) IGMC_FAIL("graph too large for the LDS bitmaps (users+items must be < ~300k)");
  if (igmc_extract_prepare(smem)) IGMC_FAIL("hipFuncSetAttribute failed");
  // slot capacity of one side: the target plus, per hop, at most max_nodes_per_hop new nodes; the hop-1 fringe of a
  // side is the neighbourhood of ONE node of the other side, so the longest row / column of the rating matrix bounds
  // it as well (an uncapped run on a sparse graph -- the Monti datasets -- then still gets slots small enough for the
  // dense induced blocks and the subgraph kernel)
  auto side_cap = [&](int n, int opposite_max_deg) -> int64_t {
    int64_t per = (max_nodes_per_hop < 0) ? (int64_t)n : std::min<int64_t>(max_nodes_per_hop, n);
    if (hop == 1) per = std::min<int64_t>(per, opposite_max_deg);
    return std::min<int64_t>(n, 1 + (int64_t)hop * per);
  };
  const int64_t cap_u = side_cap(g->d.n_users, g->max_deg_v), cap_v = side_cap(g->d.n_items, g->max_deg_u);
  const int64_t slot = cap_u + cap_v;
  const int64_t node_cap = (int64_t)max_graphs * slot;
  const int64_t per_graph_e = std::min<int64_t>(2 * cap_u * cap_v, 2 * g->nnz);
  int64_t edge_cap = (int64_t)max_graphs * per_graph_e;
  if (node_cap >= (1 << 24)) IGMC_FAIL("node capacity exceeds the 24-bit source index of a CSR entry; lower the batch size");
  edge_cap = std::min<int64_t>(edge_cap, (int64_t)INT_MAX - 65536);
  if (g->max_rel * (2 * hop + 2) + (2 * hop + 1) > 65535) IGMC_FAIL("relation*label code exceeds uint16");
  igmc_batch* b = new igmc_batch();
  b->g = g;
  b->last_B = 0;
  b->side = nullptr;
  b->n_side = 0;
  b->side_src = nullptr;
  b->side_u = b->side_v = nullptr;
  b->side_nu = b->side_fu = b->side_nv = b->side_fv = 0;
  b->side_buf = nullptr;
  b->side_buf_cols = 0;
  b->lean = 0;
  b->ctrl = nullptr;
  BatchDev& d = b->d;
  Allocs& M = b->mem;
  const int Bc = max_graphs;
  int fail = 0;
  fail |= M.get(&d.node_off, Bc + 1) | M.get(&d.n_users, Bc) | M.get(&d.n_items, Bc) | M.get(&d.edge_cnt, Bc) |
          M.get(&d.edge_off, Bc + 1);
  fail |= M.get(&d.node_label, node_cap) | M.get(&d.node_gid, node_cap) | M.get(&d.node_graph, node_cap) |
          M.get(&d.row_ptr, node_cap + 1);
  fail |= M.get(&d.ecr, edge_cap) | M.get(&d.ecode, edge_cap) | M.get(&d.eflag, edge_cap) |
          M.get(&d.edst, edge_cap);
  fail |= M.get(&d.y, Bc) | M.get(&d.totals, 8) | M.get(&d.stamp, 4);
  d.relm = nullptr;
  d.relmT = nullptr;
  d.relmT_ld = (int)((cap_u + 3) & ~(size_t)3);
  d.max_rel = g->max_rel;
  d.relm_ld = (int)((cap_v + 3) & ~(size_t)3);
  // dense path: rows of the block fit one 256-entry super-chunk and block + row starts fit the default LDS window
  // (a byte of the block holds relation + 1 in bits 0-3 and the two keep bits of edge dropout in bits 4-5: <= 15 relations)
  if (g->max_rel + 1 <= (int)IGMC_RELM_CODE && cap_u <= 256 && cap_v <= 256 && cap_u * (size_t)d.relm_ld + slot * 4 <= 60 * 1024) fail |= M.get(&d.relm, (size_t)Bc * cap_u * d.relm_ld + (size_t)128 * d.relm_ld + 128);   // dense induced block per link (+ a tail pad: the subgraph kernel's lanes read up to 128 rows from a slot's start unguarded)
  // slots too large for the subgraph kernel (> 128 nodes a side) but with a dense block: the transposed copy feeds the
  // item-side workgroups of the dense per-layer kernels (denselayer.hip)
  // (IGMC_DL_ALWAYS=1: also for small slots -- lets tests run those kernels on small cases)
  {
    // (more than five relations: the subgraph kernel does not take the arena whatever its slots, the dense-layer kernels do)
    // ... and so for a layer-0 table of more than 32 rows (two hops: the graph's relations x 6 labels)
    const int nlab = 2 * hop + 2;
    if (d.relm && (cap_u > 128 || cap_v > 128 || g->max_rel + 1 > G2_NR || (g->max_rel + 1) * nlab + nlab + 1 > 32 || igmc_dl_always())) fail |= M.get(&d.relmT, (size_t)Bc * cap_v * d.relmT_ld);
  }
  fail |= M.get(&d.s_gid, Bc * slot) | M.get(&d.s_lab, Bc * slot) | M.get(&d.s_deg, Bc * slot) |
          M.get(&d.t_list, Bc * slot) | M.get(&d.t_dist, Bc * slot);
  if (fail) {
    M.release();
    delete b;
    IGMC_FAIL("hipMalloc failed (batch arena)");
  }
  HIPCHECK(hipMemset(d.totals, 0, 8 * sizeof(int32_t)));
  HIPCHECK(hipMemset(d.stamp, 0xFF, 4 * sizeof(int64_t)));        // -1: no batch of a known cursor in the arena
  d.cap_u = (int)cap_u;
  d.cap_v = (int)cap_v;
  d.slot = (int)slot;
  d.node_cap = (int)node_cap;
  d.edge_cap = (int)edge_cap;
  d.graph_cap = Bc;
  d.hop = hop;
  d.max_nodes_per_hop = max_nodes_per_hop;
  d.num_labels = 2 * hop + 2;
  *out = b;
  return 0;
}

extern "C" void igmc_batch_destroy(igmc_batch* b) {
  if (!b) return;
  b->mem.release();
  delete b;
}

// The transposed copy of the dense blocks for an arena whose slots would not get one by size (<= 128 nodes a side): what
// the dense-layer kernels (k_dl_fwd / k_dl_bwd / k_dl_layer) read on the item side.  For models the subgraph kernel does
// not take although the blocks exist -- the sort-pool family, side features -- so that their conv layers run on the matrix
// cores instead of the CSR row walkers.  A no-op without dense blocks; a batch already in the arena is dropped.
extern "C" int igmc_batch_want_transposed(igmc_batch* b) {
  if (!b) IGMC_FAIL("null arena");
  if (b->d.relmT || !b->d.relm) return 0;
  if (b->mem.get(&b->d.relmT, (size_t)b->d.graph_cap * b->d.cap_v * b->d.relmT_ld)) IGMC_FAIL("hipMalloc failed (transposed blocks)");
  b->last_B = 0;      // (a batch extracted before has no transposed blocks: the arena counts as empty until the next extraction)
  return 0;
}

// Side features of the target nodes travel with the extraction (reference :250-253), behind its launches on the same stream:
// by link position from a bound source, by node id -- the targets the extraction has just left in the arena's slots -- from
// bound tables.
static void gather_side(const igmc_batch* b, const int32_t* d_link_idx, int first, int B, void* stream) {
  if (b->side_src) igmc_launch_side_gather(b->side_src, b->n_side, d_link_idx, first, B, b->ctrl, b->side_buf, stream);
  if (b->side_u || b->side_v)
    igmc_launch_side_gather_nodes(b->d, b->side_u, b->side_nu, b->side_fu, b->side_v, b->side_nv, b->side_fv, B, b->side_buf,
                                  stream);
}

extern "C" int igmc_extract_batch(const igmc_graph* g, igmc_batch* b, const int32_t* d_link_u,
                                  const int32_t* d_link_v, const float* d_link_y, const int32_t* d_link_idx,
                                  int first, int B, double sample_ratio, uint64_t seed, uint64_t epoch,
                                  void* stream) {
  if (!g || !b || b->g != g) IGMC_FAIL("batch does not belong to this graph");
  if (B <= 0 || B > b->d.graph_cap) IGMC_FAIL("B exceeds the batch capacity");
  if (!d_link_u || !d_link_v || !d_link_y) IGMC_FAIL("null link arrays");
  igmc_launch_extract(g->d, b->d, d_link_u, d_link_v, d_link_y, d_link_idx, first, B, 0, sample_ratio, seed, epoch,
                      b->ctrl, b->lean && b->d.relm, stream);
  gather_side(b, d_link_idx, first, B, stream);
  HIPCHECK(hipGetLastError());
  b->last_B = B;
  return 0;
}

extern "C" int igmc_extract_batch_replay(const igmc_graph* g, igmc_batch* b, int B, const int32_t* h_unodes,
                                         const uint8_t* h_udist, const int32_t* h_uoff, const int32_t* h_vnodes,
                                         const uint8_t* h_vdist, const int32_t* h_voff, const float* h_y,
                                         void* stream) {
  if (!g || !b || b->g != g) IGMC_FAIL("batch does not belong to this graph");
  if (B <= 0 || B > b->d.graph_cap) IGMC_FAIL("B exceeds the batch capacity");
  const BatchDev& d = b->d;
  std::vector<int32_t> tl((size_t)B * d.slot, 0), nu(B), nv(B);
  std::vector<uint8_t> td((size_t)B * d.slot, 0);
  for (int gi = 0; gi < B; ++gi) {
    const int cu = h_uoff[gi + 1] - h_uoff[gi], cv = h_voff[gi + 1] - h_voff[gi];
    if (cu < 1 || cv < 1 || cu > d.cap_u || cv > d.cap_v) IGMC_FAIL("replayed node list exceeds the slot capacity");
    nu[gi] = cu;
    nv[gi] = cv;
    for (int i = 0; i < cu; ++i) {
      const int id = h_unodes[h_uoff[gi] + i];
      if (id < 0 || id >= g->d.n_users) IGMC_FAIL("user id out of range");
      tl[(size_t)gi * d.slot + i] = id;
      td[(size_t)gi * d.slot + i] = h_udist[h_uoff[gi] + i];
    }
    for (int i = 0; i < cv; ++i) {
      const int id = h_vnodes[h_voff[gi] + i];
      if (id < 0 || id >= g->d.n_items) IGMC_FAIL("item id out of range");
      tl[(size_t)gi * d.slot + d.cap_u + i] = id;
      td[(size_t)gi * d.slot + d.cap_u + i] = h_vdist[h_voff[gi] + i];
    }
  }
  HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
  HIPCHECK(hipMemcpy(d.t_list, tl.data(), tl.size() * 4, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(d.t_dist, td.data(), td.size(), hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(d.n_users, nu.data(), B * 4, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(d.n_items, nv.data(), B * 4, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(d.y, h_y, B * sizeof(float), hipMemcpyHostToDevice));
  HIPCHECK(hipMemset(d.stamp, 0xFF, 4 * sizeof(int64_t)));        // node sets from the host: no cursor to compare with
  igmc_launch_extract(g->d, b->d, nullptr, nullptr, nullptr, nullptr, 0, B, 1, 1.0, 0, 0, nullptr, 0, stream);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
  b->last_B = B;
  return 0;
}

extern "C" int igmc_extract_batch_cached(const igmc_graph* g, igmc_batch* b, const int64_t* d_uoff, const int32_t* d_unodes,
                                         const uint8_t* d_udist, const int64_t* d_voff, const int32_t* d_vnodes,
                                         const uint8_t* d_vdist, const float* d_link_y, const int32_t* d_link_idx, int first,
                                         int B, void* stream) {
  if (!g || !b || b->g != g) IGMC_FAIL("batch does not belong to this graph");
  if (B <= 0 || B > b->d.graph_cap) IGMC_FAIL("B exceeds the batch capacity");
  if (!d_uoff || !d_unodes || !d_udist || !d_voff || !d_vnodes || !d_vdist || !d_link_y) IGMC_FAIL("null cache arrays");
  igmc_launch_load_nodes(b->d, d_uoff, d_unodes, d_udist, d_voff, d_vnodes, d_vdist, d_link_y, d_link_idx, first, B, b->ctrl,
                         stream);
  igmc_launch_extract(g->d, b->d, nullptr, nullptr, nullptr, nullptr, 0, B, 1, 1.0, 0, 0, nullptr, b->lean && b->d.relm, stream);
  gather_side(b, d_link_idx, first, B, stream);
  HIPCHECK(hipGetLastError());
  b->last_B = B;
  return 0;
}

// ---- a group of arenas extracted in one launch per stage
struct igmc_batch_set {
  std::vector<igmc_batch*> arenas;
  BatchDev* d_views;        // device array of the arenas' views
};

extern "C" int igmc_batch_set_create(igmc_batch* const* batches, int count, igmc_batch_set** out) {
  if (!batches || count < 1 || !out) IGMC_FAIL("bad arguments");
  std::vector<BatchDev> views;
  for (int i = 0; i < count; ++i) {
    const igmc_batch* b = batches[i];
    if (!b) IGMC_FAIL("null arena");
    const BatchDev &d = b->d, &d0 = batches[0]->d;
    if (b->g != batches[0]->g || d.cap_u != d0.cap_u || d.cap_v != d0.cap_v || d.graph_cap != d0.graph_cap || d.hop != d0.hop ||
        d.max_nodes_per_hop != d0.max_nodes_per_hop || (d.relm != nullptr) != (d0.relm != nullptr) ||
        (d.relmT != nullptr) != (d0.relmT != nullptr))
      IGMC_FAIL("the arenas of a set must share graph and geometry");
    if (!d.relm) IGMC_FAIL("group extraction needs arenas with dense induced blocks");
    views.push_back(d);
  }
  HIPCHECK(hipSetDevice(batches[0]->g->device));
  igmc_batch_set* s = new igmc_batch_set();
  s->arenas.assign(batches, batches + count);
  s->d_views = nullptr;
  if (hipMalloc((void**)&s->d_views, views.size() * sizeof(BatchDev)) != hipSuccess) {
    delete s;
    IGMC_FAIL("hipMalloc failed (arena set)");
  }
  HIPCHECK(hipMemcpy(s->d_views, views.data(), views.size() * sizeof(BatchDev), hipMemcpyHostToDevice));
  *out = s;
  return 0;
}

extern "C" void igmc_batch_set_destroy(igmc_batch_set* s) {
  if (!s) return;
  if (s->d_views) hipFree(s->d_views);
  delete s;
}

extern "C" int igmc_extract_group(const igmc_graph* g, igmc_batch_set* s, int count, const int32_t* d_link_u,
                                  const int32_t* d_link_v, const float* d_link_y, const int32_t* d_link_idx, int sel0,
                                  int B, double sample_ratio, uint64_t seed, float drop_p, int force_undirected,
                                  uint64_t drop_seed, void* stream) {
  if (!g || !s || count < 1 || count > (int)s->arenas.size()) IGMC_FAIL("bad arguments");
  if (!d_link_u || !d_link_v || !d_link_y) IGMC_FAIL("null link arrays");
  const igmc_batch* b0 = s->arenas[0];
  if (b0->g != g) IGMC_FAIL("the set does not belong to this graph");
  if (B <= 0 || B > b0->d.graph_cap) IGMC_FAIL("B exceeds the batch capacity");
  for (int i = 0; i < count; ++i) {
    const igmc_batch* b = s->arenas[i];
    if (!b->lean || !b->ctrl || b->ctrl != b0->ctrl || b->side_src || b->side_u || b->side_v)
      IGMC_FAIL("group extraction needs lean arenas with one control block attached and no side-feature source");
  }
  igmc_launch_extract_set(g->d, s->d_views, b0->d, count, d_link_u, d_link_v, d_link_y, d_link_idx, sel0, B, sample_ratio,
                          seed, b0->ctrl, drop_p, force_undirected, drop_seed, stream);
  HIPCHECK(hipGetLastError());
  for (int i = 0; i < count; ++i) s->arenas[i]->last_B = B;
  return 0;
}

// A lean arena carries no collated CSR after an extraction: whoever needs it (inspection, the flag kernels, the
// per-layer model kernels) emits it first.  Emission is idempotent, and a hipGraph replay of the extraction leaves no
// host-side trace, so a lean arena re-emits on every such call.
static void ensure_csr(const igmc_batch* b, void* stream) {
  if (b->lean && b->d.relm && b->last_B > 0) igmc_launch_emit(b->d, b->last_B, stream);
}

extern "C" int igmc_batch_assume_size(igmc_batch* b, int B) {
  if (!b) IGMC_FAIL("null batch");
  if (B <= 0 || B > b->d.graph_cap) IGMC_FAIL("batch size out of range");
  b->last_B = B;
  return 0;
}

extern "C" int igmc_batch_set_lean(igmc_batch* b, int lean) {
  if (!b) IGMC_FAIL("null batch");
  b->lean = lean ? 1 : 0;
  return 0;
}

extern "C" int igmc_batch_edge_dropout(igmc_batch* b, float p, int force_undirected, uint64_t seed, uint64_t step,
                                       void* stream) {
  if (!b) IGMC_FAIL("null batch");
  if (b->lean && b->d.relm && b->last_B > 0) {
    // lean arena: the same draws taken on the dense blocks; a CSR emitted later derives its flags from them
    igmc_launch_relm_dropout(b->d, b->last_B, p, force_undirected, seed, step, b->ctrl, stream);
  } else {
    // the flag kernel walks the collated CSR (and mirrors the bits into the dense block)
    igmc_launch_edge_flags(b->d, p, force_undirected, seed, step, b->ctrl, stream);
  }
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int igmc_batch_get_info(const igmc_batch* b, igmc_batch_info* out, void* stream) {
  if (!b || !out) IGMC_FAIL("null argument");
  ensure_csr(b, stream);
  int32_t t[8];
  HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
  HIPCHECK(hipMemcpy(t, b->d.totals, sizeof(t), hipMemcpyDeviceToHost));
  out->num_graphs = t[3];
  out->num_nodes = t[2] ? t[4] : t[0];
  out->num_edges = t[2] ? t[5] : t[1];
  out->overflow = t[2];
  out->node_capacity = b->d.node_cap;
  out->edge_capacity = b->d.edge_cap;
  out->num_labels = b->d.num_labels;
  out->hop = b->d.hop;
  return 0;
}

extern "C" int igmc_batch_set_edge_flags(igmc_batch* b, const uint8_t* h_flags, int64_t n) {
  if (!b || !h_flags) IGMC_FAIL("null argument");
  if (n > b->d.edge_cap) IGMC_FAIL("too many flags");
  ensure_csr(b, nullptr);
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(b->d.eflag, h_flags, (size_t)n, hipMemcpyHostToDevice));
  igmc_launch_relm_flags(b->d, nullptr);        // the dense block mirrors the keep bits
  HIPCHECK(hipDeviceSynchronize());
  return 0;
}

extern "C" int igmc_batch_clear_edge_flags(igmc_batch* b) {
  if (!b) IGMC_FAIL("null batch");
  igmc_batch_info info;
  if (igmc_batch_get_info(b, &info, nullptr)) return 1;
  if (info.num_edges > 0) {
    HIPCHECK(hipMemset(b->d.eflag, 3, (size_t)info.num_edges));
    igmc_launch_relm_flags(b->d, nullptr);
    HIPCHECK(hipDeviceSynchronize());
  }
  return 0;
}

extern "C" int igmc_batch_download(const igmc_batch* b, int32_t* node_off, int32_t* n_users, uint8_t* node_label,
                                   int32_t* node_gid, int32_t* node_graph, int32_t* row_ptr, int32_t* col,
                                   uint8_t* erel, uint8_t* elab, uint8_t* eflag, float* y, void* stream) {
  igmc_batch_info info;
  if (igmc_batch_get_info(b, &info, stream)) return 1;
  if (info.overflow) IGMC_FAIL("batch arena overflow");
  const int B = info.num_graphs, N = info.num_nodes, E = info.num_edges;
  const BatchDev& d = b->d;
  if (node_off) HIPCHECK(hipMemcpy(node_off, d.node_off, (B + 1) * 4, hipMemcpyDeviceToHost));
  if (n_users) HIPCHECK(hipMemcpy(n_users, d.n_users, B * 4, hipMemcpyDeviceToHost));
  if (node_label && N) HIPCHECK(hipMemcpy(node_label, d.node_label, N, hipMemcpyDeviceToHost));
  if (node_gid && N) HIPCHECK(hipMemcpy(node_gid, d.node_gid, N * 4, hipMemcpyDeviceToHost));
  if (node_graph && N) HIPCHECK(hipMemcpy(node_graph, d.node_graph, N * 4, hipMemcpyDeviceToHost));
  if (row_ptr) HIPCHECK(hipMemcpy(row_ptr, d.row_ptr, (N + 1) * 4, hipMemcpyDeviceToHost));
  if ((col || erel) && E) {
    std::vector<uint32_t> ecr(E);
    HIPCHECK(hipMemcpy(ecr.data(), d.ecr, (size_t)E * 4, hipMemcpyDeviceToHost));
    for (int e = 0; e < E; ++e) {
      if (col) col[e] = (int32_t)(ecr[e] & 0xFFFFFFu);
      if (erel) erel[e] = (uint8_t)(ecr[e] >> 24);
    }
  }
  if (elab && E) {
    std::vector<uint16_t> code(E);
    HIPCHECK(hipMemcpy(code.data(), d.ecode, (size_t)E * 2, hipMemcpyDeviceToHost));
    for (int e = 0; e < E; ++e) elab[e] = (uint8_t)(code[e] % d.num_labels);
  }
  if (eflag && E) HIPCHECK(hipMemcpy(eflag, d.eflag, E, hipMemcpyDeviceToHost));
  if (y) HIPCHECK(hipMemcpy(y, d.y, B * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

extern "C" void* igmc_batch_device_ptr(const igmc_batch* b, int which) {
  if (!b) return nullptr;
  const BatchDev& d = b->d;
  switch (which) {
    case IGMC_BUF_NODE_OFF: return d.node_off;
    case IGMC_BUF_N_USERS: return d.n_users;
    case IGMC_BUF_NODE_LABEL: return d.node_label;
    case IGMC_BUF_NODE_GID: return d.node_gid;
    case IGMC_BUF_NODE_GRAPH: return d.node_graph;
    case IGMC_BUF_ROW_PTR: return d.row_ptr;
    case IGMC_BUF_ECR: return d.ecr;
    case IGMC_BUF_ECODE: return d.ecode;
    case IGMC_BUF_EFLAG: return d.eflag;
    case IGMC_BUF_Y: return d.y;
    case IGMC_BUF_TOTALS: return d.totals;
    case IGMC_BUF_SIDE: return (void*)b->side;
  }
  return nullptr;
}

static void side_unbind(igmc_batch* b) {
  b->side_src = nullptr;
  b->side_u = b->side_v = nullptr;
  b->side_nu = b->side_fu = b->side_nv = b->side_fv = 0;
  b->side = nullptr;
  b->n_side = 0;
}

// the arena-owned buffer the gathered rows of a batch go to, at least n_side columns wide
static int side_buf_reserve(igmc_batch* b, int n_side) {
  if (b->side_buf_cols < n_side) {
    // (a wider re-bind carves a new buffer out of the arena's slabs; the old one stays part of them and is released with
    //  the arena -- slabs have no per-buffer free -- so grow geometrically to bound what repeated re-binds can take)
    HIPCHECK(hipSetDevice(b->g->device));
    const int cols = std::max(n_side, 2 * b->side_buf_cols);
    if (b->mem.get(&b->side_buf, (size_t)b->d.graph_cap * cols)) IGMC_FAIL("hipMalloc failed (side features)");
    b->side_buf_cols = cols;
  }
  return 0;
}

extern "C" int igmc_batch_set_side_features(igmc_batch* b, const float* d_feat, int n_side) {
  if (!b) IGMC_FAIL("null batch");
  side_unbind(b);
  b->side = d_feat;
  b->n_side = n_side;
  return 0;
}

extern "C" int igmc_batch_bind_side_source(igmc_batch* b, const float* d_side_all, int n_side) {
  if (!b) IGMC_FAIL("null batch");
  if (!d_side_all || n_side <= 0) {      // unbind
    side_unbind(b);
    return 0;
  }
  if (side_buf_reserve(b, n_side)) return 1;
  side_unbind(b);
  b->side_src = d_side_all;
  b->side = b->side_buf;
  b->n_side = n_side;
  return 0;
}

extern "C" int igmc_batch_bind_side_tables(igmc_batch* b, const float* d_u_feat, int n_u_rows, int fu, const float* d_v_feat,
                                           int n_v_rows, int fv) {
  if (!b) IGMC_FAIL("null batch");
  if (!d_u_feat && !d_v_feat && fu == 0 && fv == 0) {      // unbind
    side_unbind(b);
    return 0;
  }
  if (fu < 0 || fv < 0 || (int64_t)fu + fv < 1 || n_u_rows < 0 || n_v_rows < 0) IGMC_FAIL("bad side-feature table sizes");
  if (((int64_t)fu + fv) * b->d.graph_cap >= ((int64_t)1 << 31)) IGMC_FAIL("side-feature rows of a full batch exceed 2^31 floats");
  if ((fu > 0 && !d_u_feat) || (fv > 0 && !d_v_feat)) IGMC_FAIL("a null side-feature table with a non-zero width");
  if (side_buf_reserve(b, fu + fv)) return 1;
  side_unbind(b);
  b->side_u = fu > 0 ? d_u_feat : nullptr;
  b->side_nu = n_u_rows; b->side_fu = fu;
  b->side_v = fv > 0 ? d_v_feat : nullptr;
  b->side_nv = n_v_rows; b->side_fv = fv;
  b->side = b->side_buf;
  b->n_side = fu + fv;
  return 0;
}

// ------------------------------------------------------------------ model
extern "C" int igmc_model_create(int device, int num_relations, int num_bases, int num_labels, int n_side,
                                 int max_nodes, int max_edges, int max_graphs, igmc_model** out) {
  if (!out) IGMC_FAIL("null out");
  if (num_bases != 4) IGMC_FAIL("the gfx950 kernels are built for num_bases == 4 (reference Main.py:393)");
  if (num_relations < 1 || num_relations > 255) IGMC_FAIL("num_relations out of range");
  if (num_relations * num_labels + num_labels + 1 > 320) IGMC_FAIL("num_relations * num_labels too large for the layer-0 gradient kernel");
  if (num_labels < 2 || n_side < 0 || max_nodes < 1 || max_graphs < 1) IGMC_FAIL("bad sizes");
  HIPCHECK(hipSetDevice(device));
  igmc_model* m = new igmc_model();
  m->device = device;
  m->last_B = 0;
  m->last_training = 0;
  m->last_flags = 0;
  m->img_valid = 0;
  m->img_hint = 0;
  m->img_params = nullptr;
  ModelDev& d = m->d;
  d.img_current = 0;
  d.adam_m1 = nullptr;
  d.adam_m2 = nullptr;
  d.R = num_relations;
  d.Bs = 4;
  d.L = num_labels;
  d.S = n_side;
  d.D = 256 + n_side;
  int64_t off = 0;
  for (int l = 0; l < 4; ++l) {
    const int fin = l == 0 ? d.L : 32;
    d.off_basis[l] = off; off += (int64_t)4 * fin * 32;
    d.off_root[l] = off;  off += (int64_t)fin * 32;
    d.off_bias[l] = off;  off += 32;
    d.off_att[l] = off;   off += (int64_t)d.R * 4;
  }
  d.off_l1w = off; off += (int64_t)128 * d.D;
  d.off_l1b = off; off += 128;
  d.off_l2w = off; off += 128;
  d.off_l2b = off; off += 1;
  d.n_params = off;
  d.node_cap = max_nodes;
  d.edge_cap = max_edges;
  d.graph_cap = max_graphs;
  Allocs& M = m->mem;
  int fail = 0;
  const size_t N = (size_t)max_nodes, Bc = (size_t)max_graphs;
  for (int l = 0; l < 4; ++l) fail |= M.get(&d.h[l], N * 32) | M.get(&d.dpre[l], N * 32);
  fail |= M.get(&d.agg, N * 128);
  for (int l = 0; l < 3; ++l) fail |= M.get(&d.gagg[l], N * 128) | M.get(&d.Y[l], N * 128);
  fail |= M.get(&d.feat, Bc * d.D) | M.get(&d.a1, Bc * 128) | M.get(&d.lmask, Bc * 128) | M.get(&d.dz, Bc * 128) |
          M.get(&d.gfeat, Bc * d.D) | M.get(&d.err, Bc) | M.get(&d.cnt0, N * d.R * d.L);
  const size_t rows0 = (size_t)d.R * d.L + d.L + 1;
  // relation-space gradient tables of the subgraph kernel (graphstep2.hip), R <= 5 only
  d.ts_part = nullptr;
  d.ts_raw = nullptr;
  d.ts_stride = (d.R * 32 + 33) * 32;
  d.fin_stash = nullptr;
  d.datt_part = nullptr;
  d.fold_w = nullptr;
  d.l3_vec = nullptr;
  if (d.R <= G2_NR * G2_NG_MAX)
  {   // (sums + d att partials in ONE allocation: a data-parallel step exchanges them as one span)
    fail |= M.get(&d.ts_part, (size_t)4 * IGMC_TS_BLOCKS * d.ts_stride) |
            M.get(&d.ts_raw, (size_t)4 * d.ts_stride + (size_t)4 * d.ts_stride / 32 * 4);
    if (!fail) d.datt_part = d.ts_raw + (size_t)4 * d.ts_stride;
    fail |= M.get(&d.fold_w, (size_t)IGMC_FOLD_WORDS);      // hand-off words of the one-launch tail
    fail |= M.get(&d.l3_vec, Bc * 2 * (G2_NR + 2) * 32);    // layer 3's centre vectors (clustered training steps)
  }
  if (d.R <= 128) fail |= M.get(&d.fin_stash, (size_t)4 * IGMC_STASH_LAYER + 16);     // weights-only stash of k_finalize_ts (both modes)
  d.g2_ex = nullptr;
  d.g2_fx = nullptr;
  d.g2_tw = nullptr;
  d.g2_px = nullptr;
  d.g2_px_stride = 0;
  d.g2_w = nullptr;
  d.g2_graphs = 0;
  // exchange regions [32 features][256 nodes a side] of the one-launch dense layers (k_dl_fwd / k_dl_bwd); the subgraph
  // kernel uses the first 128 nodes of a region.  655 KB per subgraph slot: HBM is not what this path is short of.
  d.ex_nodes = 256;
  d.g2_ex_stride = (size_t)Bc * 2 * 32 * d.ex_nodes;
  const int wide = d.R <= G2_NR * G2_NG_MAX;      // relation groups of the dense-layer kernels (g2_image.h)
  // (both exchanges go through the L2 of one XCD: where the probe says workgroups b and b + 8 do not share one, neither kernel
  //  family is eligible and ~1 MB per subgraph slot of exchange regions would be allocated for nothing -- ADVICE r5)
  const int xcd_ok = igmc_g2_xcd_ok();
  if (wide && Bc <= 2048 && xcd_ok) {
    fail |= M.get(&d.g2_ex, 5 * d.g2_ex_stride) | M.get(&d.g2_fx, Bc * 256) | M.get(&d.g2_w, g2_w_words(d.R, d.L));
    d.g2_graphs = (int)Bc;
    // the subgraph kernel's plane exchange (R <= 5): 320 KB per subgraph slot
    if (d.R <= G2_NR && Bc <= 1024) {
      d.g2_px_stride = (size_t)Bc * 2 * 32768;
      fail |= M.get(&d.g2_px, 5 * d.g2_px_stride);
      fail |= M.get(&d.g2_tw, Bc * IGMC_G2_TW_WORDS);      // centre-sum words of layer 3's forward (20 KB per subgraph slot)
    } else if (d.R <= G2_NR) {
      static bool told = false;
      if (!told) fprintf(stderr, "[igmc] batches of more than 1024 subgraphs: no plane-exchange regions -- the dense-layer / per-layer kernels take the steps, not the subgraph kernel\n");
      told = true;
    }
  } else if (wide) {
    fail |= M.get(&d.g2_w, g2_w_words(d.R, d.L));      // weight images alone: the dense per-layer kernels (any head)
  }
  fail |= M.get(&d.gs_bar, 2 * Bc + 1);
  fail |= M.get(&d.gs_ts, 4);
  d.gs_err = d.gs_bar ? d.gs_bar + 2 * Bc : nullptr;
  fail |= M.get(&d.wg_part, (size_t)4 * IGMC_WG_BLOCKS * igmc_wg_stride()) |
          M.get(&d.gatt_part, (size_t)3 * IGMC_GATHER_BLOCKS * d.R * 4) |
          M.get(&d.l0_part, (size_t)IGMC_L0_BLOCKS * rows0 * 32) |
          M.get(&d.graw, (size_t)3 * igmc_wg_stride() + 3 * d.R * 4 + rows0 * 32) | M.get(&d.arr_part, 4);
  d.side = nullptr;
  d.ctrl = nullptr;
  d.dcat[0] = d.dcat[1] = d.dcat[2] = nullptr;
  fail |= M.get(&m->done_ctr, 8);      // [0] step-wide, [1..4] per conv layer (k_finalize)
  if (fail) {
    M.release();
    delete m;
    IGMC_FAIL("hipMalloc failed (model workspace)");
  }
  {
    hipStream_t st1, st2;
    if (hipStreamCreateWithFlags(&st1, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&st2, hipStreamNonBlocking) != hipSuccess) {
      M.release();
      delete m;
      IGMC_FAIL("hipStreamCreate failed");
    }
    m->ax.s1 = st1;
    m->ax.s2 = st2;
    for (int i = 0; i < 8; ++i) {
      hipEvent_t e;
      if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) IGMC_FAIL("hipEventCreate failed");
      m->ax.ev[i] = e;
    }
  }
  HIPCHECK(hipMemset(m->done_ctr, 0, 8 * sizeof(int)));
  HIPCHECK(hipMemset(m->d.gs_bar, 0, (2 * (size_t)max_graphs + 1) * sizeof(int)));
  {
    const unsigned long long ts0[4] = {~0ull, 0ull, 0ull, 0ull};
    HIPCHECK(hipMemcpy(m->d.gs_ts, ts0, sizeof(ts0), hipMemcpyHostToDevice));
  }
  if (m->d.fold_w) HIPCHECK(hipMemset(m->d.fold_w, 0, (size_t)IGMC_FOLD_WORDS * sizeof(unsigned long long)));      // tag 0: never issued
  if (m->d.g2_ex) {
    HIPCHECK(hipMemset(m->d.g2_ex, 0, 5 * m->d.g2_ex_stride * sizeof(unsigned long long)));
    HIPCHECK(hipMemset(m->d.g2_fx, 0, (size_t)max_graphs * 256 * sizeof(unsigned long long)));
    if (m->d.g2_px) HIPCHECK(hipMemset(m->d.g2_px, 0, 5 * m->d.g2_px_stride));      // flags 0 (never a launch's tag), planes finite
    if (m->d.g2_tw) HIPCHECK(hipMemset(m->d.g2_tw, 0, (size_t)max_graphs * IGMC_G2_TW_WORDS * sizeof(unsigned long long)));
  }
  if (igmc_model_prepare(d)) {
    M.release();
    delete m;
    IGMC_FAIL("hipFuncSetAttribute failed");
  }
  *out = m;
  return 0;
}

// debug aid (tests): host copy of the keep mask the last TRAINING forward drew / was given for the 0.5 MLP dropout
// (reference models.py:212), uint8 [n <= max_graphs * 128].  Synchronises the device.
extern "C" int igmc_debug_lin_mask(const igmc_model* m, uint8_t* h_out, int64_t n) {
  if (!m || !h_out) IGMC_FAIL("null argument");
  if (n < 0 || n > (int64_t)m->d.graph_cap * 128) IGMC_FAIL("mask size out of range");
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(h_out, m->d.lmask, (size_t)n, hipMemcpyDeviceToHost));
  return 0;
}

// debug aid (tests): host copy of what the head of the last TRAINING step left per subgraph -- which = 0: a1 [128], 1: dz [128],
// 2: feat [D], 3: gfeat [D]; n floats from the start of the array.  Synchronises the device.
extern "C" int igmc_debug_head_array(const igmc_model* m, int which, float* h_out, int64_t n) {
  if (!m || !h_out) IGMC_FAIL("null argument");
  if (which < 0 || which > 3) IGMC_FAIL("no such array");
  const float* src = which == 0 ? m->d.a1 : which == 1 ? m->d.dz : which == 2 ? m->d.feat : m->d.gfeat;
  if (n < 0 || n > (int64_t)m->d.graph_cap * (which < 2 ? 128 : m->d.D)) IGMC_FAIL("size out of range");
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(h_out, src, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// debug aid (tests): host copy of what the last TRAINING launch of the subgraph kernel left of conv layer 3's centre rows -- which = 0:
// the centre vectors ModelDev::l3_vec [graphs][2 sides][G2_NR + 2][32] (rows r < R: the summed T_r[centre]; clustered steps under
// StepPlan::l3_vec), 1: the h_2 rows the kernel stored for its backward, which the sums were formed from, per subgraph slot of the
// arena `b` as [graphs][2 sides][128 rows][32] (rows past a side's capacity are left as the caller set them).  n floats: a whole
// number of subgraphs.  Synchronises the device.
extern "C" int igmc_debug_l3_sums(const igmc_model* m, const igmc_batch* b, int which, float* h_out, int64_t n) {
  if (!m || !b || !h_out) IGMC_FAIL("null argument");
  if (which < 0 || which > 1) IGMC_FAIL("no such array");
  if (which == 1) return igmc_debug_layer_rows(m, b, 2, 0, h_out, n);      // (its own checks and synchronisation)
  const int64_t per = 2 * (G2_NR + 2) * 32;
  if (n < 0 || n % per != 0 || n / per > (int64_t)m->d.graph_cap || n / per > (int64_t)b->d.graph_cap) IGMC_FAIL("size out of range");
  HIPCHECK(hipDeviceSynchronize());
  if (!m->d.l3_vec) IGMC_FAIL("array not allocated");
  HIPCHECK(hipMemcpy(h_out, m->d.l3_vec, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

// debug aid (tests): host copy of the rows h_layer (layer 0..2; h_3 of the centres is in feat: igmc_debug_head_array) the last
// TRAINING launch stored for its backward.  form 0: per subgraph slot of the arena `b`, as the subgraph kernel addresses them --
// [graphs][2 sides][128 rows][32], rows past a side's capacity left as the caller set them, n floats = a whole number of
// subgraphs; form 1: by collated node index, as the dense-layer and the per-layer kernels address them -- the first n floats
// (whole rows) of the array.  Synchronises the device.
extern "C" int igmc_debug_layer_rows(const igmc_model* m, const igmc_batch* b, int layer, int form, float* h_out, int64_t n) {
  if (!m || !b || !h_out) IGMC_FAIL("null argument");
  if (layer < 0 || layer > 2) IGMC_FAIL("no such layer");
  if (form < 0 || form > 1) IGMC_FAIL("no such form");
  if (form == 1) {
    if (n < 0 || n % 32 != 0 || n / 32 > (int64_t)m->d.node_cap || n / 32 > (int64_t)b->d.node_cap) IGMC_FAIL("size out of range");
    HIPCHECK(hipDeviceSynchronize());
    if (n) HIPCHECK(hipMemcpy(h_out, m->d.h[layer], (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
  }
  const int64_t per = 2 * 128 * 32;
  if (n < 0 || n % per != 0 || n / per > (int64_t)m->d.graph_cap || n / per > (int64_t)b->d.graph_cap) IGMC_FAIL("size out of range");
  if ((int64_t)b->d.graph_cap * b->d.slot > (int64_t)m->d.node_cap) IGMC_FAIL("the arena's slots exceed the workspace");
  HIPCHECK(hipDeviceSynchronize());
  for (int64_t g = 0; g < n / per; ++g)
    for (int sd = 0; sd < 2; ++sd) {
      const int rows = std::min(sd ? b->d.cap_v : b->d.cap_u, 128);
      HIPCHECK(hipMemcpy(h_out + (g * 2 + sd) * 128 * 32, m->d.h[layer] + ((size_t)g * b->d.slot + (sd ? b->d.cap_u : 0)) * 32,
                         (size_t)rows * 32 * sizeof(float), hipMemcpyDeviceToHost));
    }
  return 0;
}

// debug aid (tests): host copy of the staged weight images + layer-0 table (g2_image.h) as the last step or compose left them;
// h_out == NULL: *n_words alone.  Synchronises the device.
extern "C" int igmc_debug_weight_images(const igmc_model* m, float* h_out, int64_t* n_words) {
  if (!m || !n_words) IGMC_FAIL("null argument");
  const int64_t n = m->d.g2_w ? (int64_t)g2_w_words(m->d.R, m->d.L) : 0;
  if (h_out) {
    if (*n_words < 0 || *n_words > n) IGMC_FAIL("size out of range");
    HIPCHECK(hipDeviceSynchronize());
    if (*n_words) HIPCHECK(hipMemcpy(h_out, m->d.g2_w, (size_t)*n_words * sizeof(float), hipMemcpyDeviceToHost));
  } else {
    *n_words = n;
  }
  return 0;
}

// debug aid (tests): every byte of what the model step writes for a later launch and never clears itself -- the partial
// weight-gradient tables, layer 3's centre vectors and the h_l rows -- set to `byte` (0xFF: NaNs).  A step must leave results
// that do not depend on it: it stores every element the tail reads.  Synchronises the device.
extern "C" int igmc_debug_fill_tables(igmc_model* m, int byte) {
  if (!m) IGMC_FAIL("null argument");
  if (byte < 0 || byte > 255) IGMC_FAIL("not a byte");
  const ModelDev& d = m->d;
  HIPCHECK(hipDeviceSynchronize());
  if (d.ts_part) HIPCHECK(hipMemset(d.ts_part, byte, (size_t)4 * IGMC_TS_BLOCKS * d.ts_stride * sizeof(float)));
  if (d.l3_vec) HIPCHECK(hipMemset(d.l3_vec, byte, (size_t)d.graph_cap * 2 * (G2_NR + 2) * 32 * sizeof(float)));
  for (int l = 0; l < 4; ++l) HIPCHECK(hipMemset(d.h[l], byte, (size_t)d.node_cap * 32 * sizeof(float)));
  HIPCHECK(hipDeviceSynchronize());
  return 0;
}

extern "C" void igmc_model_destroy(igmc_model* m) {
  if (!m) return;
  for (int i = 0; i < 8; ++i) hipEventDestroy((hipEvent_t)m->ax.ev[i]);
  hipStreamDestroy((hipStream_t)m->ax.s1);
  hipStreamDestroy((hipStream_t)m->ax.s2);
  m->mem.release();
  delete m;
}

extern "C" int64_t igmc_param_count(const igmc_model* m) { return m ? m->d.n_params : 0; }

extern "C" int64_t igmc_param_offset(const igmc_model* m, int layer, int which, int64_t* count) {
  if (!m) return -1;
  const ModelDev& d = m->d;
  const int fin = (layer == 0) ? d.L : 32;
  int64_t off = -1, n = 0;
  switch (which) {
    case IGMC_P_BASIS: off = d.off_basis[layer & 3]; n = (int64_t)4 * fin * 32; break;
    case IGMC_P_ROOT: off = d.off_root[layer & 3]; n = (int64_t)fin * 32; break;
    case IGMC_P_BIAS: off = d.off_bias[layer & 3]; n = 32; break;
    case IGMC_P_ATT: off = d.off_att[layer & 3]; n = (int64_t)d.R * 4; break;
    case IGMC_P_LIN1_W: off = d.off_l1w; n = (int64_t)128 * d.D; break;
    case IGMC_P_LIN1_B: off = d.off_l1b; n = 128; break;
    case IGMC_P_LIN2_W: off = d.off_l2w; n = 128; break;
    case IGMC_P_LIN2_B: off = d.off_l2b; n = 1; break;
  }
  if (count) *count = n;
  return off;
}

static StepPlan plan_query(const igmc_model* m, const igmc_batch* b, int B) {      // what a step on (arena, B) would launch
  StepPlan sp;
  igmc_step_plan(m->d, b->d, B, IGMC_CALL_STEP, &sp);
  return sp;
}

// 1 when the dense-layer kernels (k_dl_*) take the conv layers of this arena
extern "C" int igmc_model_dense_layers(const igmc_model* m, const igmc_batch* b, int B) {
  return (m && b) ? plan_query(m, b, B).dense_layers : 0;
}

extern "C" int igmc_model_dense_path(const igmc_model* m, const igmc_batch* b, int B) {
  return (m && b) ? plan_query(m, b, B).family == IGMC_FAM_G2 : 0;
}

extern "C" int igmc_model_step_form(const igmc_model* m, const igmc_batch* b, int B) {
  return (m && b) ? plan_query(m, b, B).step_form : 0;
}

// debug aid (tests): non-zero when a training step on (arena, B) hands conv layer 3's weight gradient from the subgraph kernel to
// its tail as the centre rows' vectors instead of per-workgroup tables (StepPlan::l3_vec: the member that owns the item centre)
extern "C" int igmc_debug_l3_vectors(const igmc_model* m, const igmc_batch* b, int B) {
  return (m && b) ? plan_query(m, b, B).l3_vec : 0;
}

extern "C" int igmc_model_step_geometry(const igmc_model* m, const igmc_batch* b, int B, int32_t* out, int n) {
  if (!m || !b || !out || n < 0) IGMC_FAIL("bad arguments");
  if (B < 1 || B > b->d.graph_cap) IGMC_FAIL("batch size outside the arena's capacity");
  const StepPlan sp = plan_query(m, b, B);
  const int g2 = sp.family == IGMC_FAM_G2, dense = sp.family == IGMC_FAM_DLF || sp.family == IGMC_FAM_DL;
  const int32_t v[IGMC_GEOM_N] = {sp.step_form,
                                  sp.family,
                                  g2 ? sp.cs : 0,
                                  g2 ? sp.grid : 0,
                                  sp.nqu,
                                  sp.nqv,
                                  sp.family == IGMC_FAM_ROWS ? 0 : sp.wide ? g2_groups(m->d.R, m->d.L) : 1,
                                  sp.wide && sp.gsplit,
                                  g2 || sp.dlts,
                                  g2 ? sp.lay.kp : 0,
                                  dense && sp.dlb};
  for (int i = 0; i < n && i < IGMC_GEOM_N; ++i) out[i] = v[i];
  return 0;
}

static int check_fit(igmc_model* m, const igmc_batch* b, std::string* why) {
  if (!m || !b) { *why = "null model or batch"; return 1; }
  if (b->last_B <= 0) { *why = "batch is empty (run igmc_extract_batch first)"; return 1; }
  if (b->d.node_cap > m->d.node_cap || b->d.graph_cap > m->d.graph_cap) { *why = "batch capacity exceeds the model workspace"; return 1; }
  if (b->d.num_labels != m->d.L) { *why = "num_labels mismatch (hop)"; return 1; }
  if (b->g->max_rel >= m->d.R) { *why = "graph has more relations than the model"; return 1; }
  if (m->d.S != b->n_side && m->d.S > 0) { *why = "side feature width mismatch"; return 1; }
  return 0;
}

// What the calls that run the model on a batch share.  check_call: the fit and the caller's buffers; begin_call: the arena's
// side features, the plan of the call and -- where that plan walks rows -- the collated CSR, which a lean extraction has not
// emitted; end_call: what igmc_model_backward / igmc_step_finish need to know about the call.
static int check_call(igmc_model* m, const igmc_batch* b, bool buffers, std::string* why) {
  if (check_fit(m, b, why)) return 1;
  if (!buffers) { *why = "null buffer"; return 1; }
  return 0;
}
static StepPlan begin_call(igmc_model* m, const igmc_batch* b, int kind, void* stream) {
  m->d.side = b->side;
  StepPlan sp;
  igmc_step_plan(m->d, b->d, b->last_B, kind, &sp);
  if (b->lean && sp.needs_csr) ensure_csr(b, stream);
  return sp;
}
static void end_call(igmc_model* m, const igmc_batch* b, int training, int use_edge_flags) {
  m->last_B = b->last_B;
  m->last_training = training;
  m->last_flags = use_edge_flags;
}

// Adam's scalars of step t as the kernels take them: the bias corrections lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t), then the
// constants.  With a control block the kernel takes all six from the block, the corrections from its own step counter: zeros
static AdamHyper adam_scalars(const int64_t* d_ctrl, int64_t t, float lr, float beta1, float beta2, float eps, float wd) {
  AdamHyper h = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (!d_ctrl) {
    const double bc1 = 1.0 - std::pow((double)beta1, (double)t);
    const double bc2 = 1.0 - std::pow((double)beta2, (double)t);
    h = {(float)((double)lr / bc1), (float)(1.0 / std::sqrt(bc2)), beta1, beta2, eps, wd};
  }
  return h;
}
// The fused step's optimiser tail
static AdamTail adam_tail(igmc_model* m, float* d_params, float* d_exp_avg, float* d_exp_avg_sq, const AdamHyper& h, int64_t* d_ctrl,
                          float* d_loss, double* d_total) {
  AdamTail at;
  memset(&at, 0, sizeof(at));
  at.p = d_params; at.m1 = d_exp_avg; at.m2 = d_exp_avg_sq;
  at.h = h;
  at.ctrl = d_ctrl; at.done = m->done_ctr; at.loss = d_loss; at.total = d_total;
  return at;
}

extern "C" int igmc_model_forward(igmc_model* m, const float* d_params, const igmc_batch* b, int training,
                                  int use_edge_flags, const uint8_t* d_lin_mask, uint64_t seed, uint64_t step,
                                  float multiply_by, float* d_out, void* stream) {
  std::string why;
  if (check_call(m, b, d_params && d_out, &why)) IGMC_FAIL(why);
  const StepPlan sp = begin_call(m, b, training ? IGMC_CALL_CONV : IGMC_CALL_EVAL, stream);
  ImgScope img(m, d_params);
  const StepHead hd = {d_params, d_lin_mask, seed, step, multiply_by, 0.f, d_out};
  igmc_launch_forward(m->d, b->d, sp, b->last_B, training, use_edge_flags, hd, stream);
  img.done_unchanged();
  HIPCHECK(hipGetLastError());
  end_call(m, b, training, use_edge_flags);
  return 0;
}

extern "C" int igmc_model_backward(igmc_model* m, const float* d_params, const igmc_batch* b, const float* d_gout,
                                   float multiply_by, float* d_grad, void* stream) {
  std::string why;
  if (check_fit(m, b, &why)) IGMC_FAIL(why);
  if (!m->last_training || m->last_B != b->last_B) IGMC_FAIL("backward needs a preceding training-mode forward on this batch");
  if (!d_params || !d_gout || !d_grad) IGMC_FAIL("null buffer");
  StepPlan sp;      // (the arena's CSR: the training forward's call saw to it)
  igmc_step_plan(m->d, b->d, b->last_B, IGMC_CALL_CONV, &sp);
  igmc_launch_backward(m->d, b->d, sp, d_params, b->last_B, m->last_flags, d_gout, 0, 0.f, multiply_by, 2.f, 0.f, d_grad,
                       stream);
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int igmc_model_loss_grad(igmc_model* m, const float* d_params, const igmc_batch* b, int use_edge_flags,
                                    const uint8_t* d_lin_mask, uint64_t seed, uint64_t step, float multiply_by,
                                    float ARR, float grad_scale, float arr_scale, float* d_out, float* d_grad,
                                    float* d_loss, void* stream) {
  std::string why;
  if (check_call(m, b, d_params && d_out && d_grad, &why)) IGMC_FAIL(why);
  const StepPlan sp = begin_call(m, b, IGMC_CALL_STEP, stream);
  ImgScope img(m, d_params);
  const StepHead hd = {d_params, d_lin_mask, seed, step, multiply_by, grad_scale, d_out};
  igmc_launch_loss_grad(m->d, b->d, sp, b->last_B, use_edge_flags, hd, ARR, arr_scale, d_grad, d_loss, nullptr, stream);
  img.done_unchanged();
  HIPCHECK(hipGetLastError());
  end_call(m, b, 1, use_edge_flags);
  return 0;
}

extern "C" int igmc_adam_step(float* d_params, const float* d_grad, float* d_exp_avg, float* d_exp_avg_sq, int64_t n,
                              int64_t step, float lr, float beta1, float beta2, float eps, float weight_decay,
                              void* stream) {
  if (!d_params || !d_grad || !d_exp_avg || !d_exp_avg_sq || n <= 0 || step < 1) IGMC_FAIL("bad arguments");
  igmc_launch_adam(d_params, d_grad, d_exp_avg, d_exp_avg_sq, n, adam_scalars(nullptr, step, lr, beta1, beta2, eps, weight_decay),
                   nullptr, 0, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int igmc_sse_accumulate(const float* d_out, const igmc_batch* b, double* d_acc, void* stream) {
  if (!d_out || !b || !d_acc) IGMC_FAIL("null argument");
  igmc_launch_sse(b->d, d_out, d_acc, nullptr, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
extern "C" int igmc_sse_accumulate_tick(const float* d_out, const igmc_batch* b, double* d_acc, int64_t* d_ctrl, void* stream) {
  if (!d_out || !b || !d_acc || !d_ctrl) IGMC_FAIL("null argument");
  igmc_launch_sse(b->d, d_out, d_acc, d_ctrl, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ pair training (pairs.hip)
extern "C" int igmc_pair_loss_grad(igmc_model* m, const float* d_params, const igmc_batch* b, int use_edge_flags,
                                   const uint8_t* d_lin_mask, uint64_t seed, uint64_t step, float multiply_by, float ARR,
                                   float mse_weight, float* d_out, float* d_gout, float* d_grad, double* d_stats,
                                   void* stream) {
  std::string why;
  if (check_call(m, b, d_params && d_out && d_gout && d_grad && d_stats, &why)) IGMC_FAIL(why);
  if (b->last_B & 1) IGMC_FAIL("a pair batch holds an even number of links: positives in the even slots, their negatives behind them");
  const int B = b->last_B;
  const StepPlan sp = begin_call(m, b, IGMC_CALL_CONV, stream);
  ImgScope img(m, d_params);
  const StepHead hd = {d_params, d_lin_mask, seed, step, multiply_by, 0.f, d_out};
  igmc_launch_forward(m->d, b->d, sp, B, 1, use_edge_flags, hd, stream);
  igmc_launch_pair_loss(d_out, b->d.y, B, mse_weight, d_gout, d_stats, stream);
  igmc_launch_backward(m->d, b->d, sp, d_params, B, use_edge_flags, d_gout, 0, 0.f, multiply_by, 2.f, ARR, d_grad, stream);
  igmc_launch_pair_arr(m->d.arr_part, ARR, d_stats, stream);
  img.done_unchanged();
  HIPCHECK(hipGetLastError());
  end_call(m, b, 1, use_edge_flags);
  return 0;
}
// ------------------------------------------------------------------ device-side step control
extern "C" int igmc_ctrl_tick(int64_t* d_ctrl, void* stream) {
  if (!d_ctrl) IGMC_FAIL("null ctrl");
  igmc_launch_tick(d_ctrl, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
extern "C" int igmc_ctrl_regroup(int64_t* d_ctrl, int M, int64_t first_cur, int64_t first_next, void* stream) {
  if (!d_ctrl || M < 1 || first_cur < 0 || first_next < 0) IGMC_FAIL("bad arguments");
  igmc_launch_regroup(d_ctrl, M, first_cur, first_next, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
extern "C" int igmc_ctrl_gate(int64_t* d_ctrl, int q, int gk_min, double delay_us, int delay_always, double timeout_us,
                              void* stream) {
  if (!d_ctrl || gk_min < 0 || !(timeout_us >= 0.0) || !(delay_us >= 0.0) || delay_us > 1000.0) IGMC_FAIL("bad arguments");
  // (wall_clock64: 100 MHz)
  igmc_launch_gate(d_ctrl, q & 1, gk_min, (long long)(delay_us * 100.0), delay_always != 0, (long long)(timeout_us * 100.0), stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
extern "C" int igmc_batch_set_ctrl(igmc_batch* b, const int64_t* d_ctrl) {
  if (!b) IGMC_FAIL("null batch");
  b->ctrl = d_ctrl;
  return 0;
}
extern "C" int igmc_model_set_ctrl(igmc_model* m, const int64_t* d_ctrl) {
  if (!m) IGMC_FAIL("null model");
  m->d.ctrl = d_ctrl;
  return 0;
}
// INVARIANT of the plane / row exchange regions (g2_px, g2_ex, g2_fx): every value in them is FINITE.  A consumer copies the
// whole plane image of the opposite side, rows past that side's extent included -- whatever an earlier launch left in the
// subgraph slot --, and relies on 0 * stale == 0 (the A-block bytes there are zero).  Steps that ran on non-finite parameters
// can leave NaN / Inf rows behind which would poison every later gather of the slot, even after the parameters are restored:
// the regions are cleared (flags included: 0 is never a launch's tag) whenever parameters are replaced wholesale and when an
// exchange timed out (igmc_model_check below).  The Python entry points that uphold it: models.IGMC.load_state_dict and
// models.IGMC.reset_parameters (DGCNN_RS too; train_multiple_epochs re-initialises a reused model with the latter), both
// through IGMC._params_replaced, and models.IGMC.reset_exchange for callers that write the flat parameter buffer themselves.
// A caller of the C ABI that restores parameters after a diverged step calls this function itself
// (tests/history_checks.py: run_nonfinite_history holds the kernels to it).
extern "C" int igmc_model_reset_exchange(igmc_model* m, void* stream) {
  if (!m) IGMC_FAIL("null model");
  hipStream_t st = (hipStream_t)stream;
  // (the tail's hand-off words carry the launch sequence number, which restarts with the flags)
  if (m->d.fold_w) HIPCHECK(hipMemsetAsync(m->d.fold_w, 0, (size_t)IGMC_FOLD_WORDS * sizeof(unsigned long long), st));
  if (m->d.g2_ex) {
    HIPCHECK(hipMemsetAsync(m->d.g2_ex, 0, 5 * m->d.g2_ex_stride * sizeof(unsigned long long), st));
    HIPCHECK(hipMemsetAsync(m->d.g2_fx, 0, (size_t)m->d.g2_graphs * 256 * sizeof(unsigned long long), st));
    if (m->d.g2_px) HIPCHECK(hipMemsetAsync(m->d.g2_px, 0, 5 * m->d.g2_px_stride, st));
    if (m->d.g2_tw) HIPCHECK(hipMemsetAsync(m->d.g2_tw, 0, (size_t)m->d.g2_graphs * IGMC_G2_TW_WORDS * sizeof(unsigned long long), st));
  }
  return 0;
}
extern "C" int igmc_model_check(igmc_model* m, void* stream) {
  if (!m) IGMC_FAIL("null model");
  int v = 0;
  if (m->d.gs_err) {
    HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
    HIPCHECK(hipMemcpy(&v, m->d.gs_err, sizeof(int), hipMemcpyDeviceToHost));
    if (v) {
      HIPCHECK(hipMemset(m->d.gs_bar, 0, (2 * (size_t)m->d.graph_cap + 1) * sizeof(int)));
      (void)igmc_model_reset_exchange(m, stream);        // (sequence number and flags restart together; partial rows gone)
      HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
      IGMC_FAIL("a workgroup-cluster exchange of k_graph_step2 or a hand-off of the one-launch tail k_tail_fin timed out (GPU "
                "shared with another job?): results of the affected steps are invalid; set IGMC_GS_CLUSTER=1 or "
                "IGMC_GRAPH_STEP=0 (the tail alone: IGMC_TAIL_FOLD=0)");
    }
  }
  return 0;
}
extern "C" int igmc_adam_step_ctrl(float* d_params, const float* d_grad, float* d_exp_avg, float* d_exp_avg_sq,
                                   int64_t n, const int64_t* d_ctrl, void* stream) {
  if (!d_params || !d_grad || !d_exp_avg || !d_exp_avg_sq || n <= 0 || !d_ctrl) IGMC_FAIL("bad arguments");
  igmc_launch_adam(d_params, d_grad, d_exp_avg, d_exp_avg_sq, n, AdamHyper{}, (int64_t*)d_ctrl, 0, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int igmc_step_finish(igmc_model* m, const igmc_batch* b, float* d_params, const float* d_grad,
                                float* d_exp_avg, float* d_exp_avg_sq, float ARR, float* d_loss, double* d_total,
                                int64_t* d_ctrl, int64_t step, float lr, float beta1, float beta2, float eps,
                                float weight_decay, void* stream) {
  if (!m || !b || !d_params || !d_grad || !d_exp_avg || !d_exp_avg_sq || !d_loss) IGMC_FAIL("bad arguments");
  if (!d_ctrl && step < 1) IGMC_FAIL("step must be >= 1");
  igmc_launch_finish(m->d, b->d, d_params, d_grad, d_exp_avg, d_exp_avg_sq, adam_scalars(d_ctrl, step, lr, beta1, beta2, eps, weight_decay),
                     d_ctrl, ARR, d_loss, d_total, m->last_flags, stream);
  m->img_valid = 0;      // (the parameters moved, the weight images did not)
  m->img_hint = 0;
  HIPCHECK(hipGetLastError());
  return 0;
}

extern "C" int igmc_train_step(igmc_model* m, float* d_params, const igmc_batch* b, int use_edge_flags,
                               const uint8_t* d_lin_mask, uint64_t seed, uint64_t step, float multiply_by, float ARR,
                               float* d_out, float* d_grad, float* d_exp_avg, float* d_exp_avg_sq, float* d_loss,
                               double* d_total, int64_t* d_ctrl, int64_t adam_t, float lr, float beta1, float beta2,
                               float eps, float weight_decay, void* stream) {
  std::string why;
  if (check_call(m, b, d_params && d_out && d_grad && d_exp_avg && d_exp_avg_sq && d_loss, &why)) IGMC_FAIL(why);
  if (!d_ctrl && adam_t < 1) IGMC_FAIL("adam_t must be >= 1");
  const AdamTail at = adam_tail(m, d_params, d_exp_avg, d_exp_avg_sq, adam_scalars(d_ctrl, adam_t, lr, beta1, beta2, eps, weight_decay),
                                d_ctrl, d_loss, d_total);
  const StepPlan sp = begin_call(m, b, IGMC_CALL_STEP, stream);
  ImgScope img(m, d_params);
  int emitted = 0;
  const StepHead hd = {d_params, d_lin_mask, seed, step, multiply_by, 1.0f / (float)b->last_B, d_out};      // (one rank: the mean over the batch)
  igmc_launch_loss_grad(m->d, b->d, sp, b->last_B, use_edge_flags, hd, ARR, 1.0f, d_grad, nullptr, &at, stream, nullptr, &emitted);
  img.done_updated(emitted);
  HIPCHECK(hipGetLastError());
  end_call(m, b, 1, use_edge_flags);
  return 0;
}

// One optimisation step of a data-parallel job (reference train_eval.py:157-177 per rank, gradients averaged over the
// ranks): igmc_train_step with the exchange INSIDE the step.  Where the step keeps its gradient sources in reduced form
// (StepPlan::exchange_inside: the subgraph kernel's tables, the per-layer path's basis-space sums) those are summed over
// the ranks between their reduction and the gradient / Adam kernel -- the kernels of the single-GPU step, one grouped
// collective more; elsewhere the flat gradient is formed, all-reduced and handed to the Adam kernel.  comm == NULL: one rank.
extern "C" int igmc_train_step_dp(igmc_model* m, igmc_comm* comm, float* d_params, const igmc_batch* b, int use_edge_flags,
                                  const uint8_t* d_lin_mask, uint64_t seed, uint64_t step, float multiply_by, float ARR,
                                  float* d_out, float* d_grad, float* d_exp_avg, float* d_exp_avg_sq, float* d_loss,
                                  double* d_total, int64_t* d_ctrl, int64_t adam_t, float lr, float beta1, float beta2,
                                  float eps, float weight_decay, void* stream) {
  std::string why;
  if (check_call(m, b, d_params && d_out && d_grad && d_exp_avg && d_exp_avg_sq && d_loss, &why)) IGMC_FAIL(why);
  if (!d_ctrl && adam_t < 1) IGMC_FAIL("adam_t must be >= 1");
  const AdamHyper ah = adam_scalars(d_ctrl, adam_t, lr, beta1, beta2, eps, weight_decay);
  const int world = igmc_comm_world(comm);
  const int B = b->last_B;
  const float gscale = 1.0f / ((float)B * (float)world);
  const StepPlan sp = begin_call(m, b, IGMC_CALL_STEP, stream);
  ImgScope img(m, d_params);
  int emitted = 0;
  const StepHead hd = {d_params, d_lin_mask, seed, step, multiply_by, gscale, d_out};
  if (sp.exchange_inside) {
    StepExchange x = igmc_comm_exchange(comm);
    // (the ARR term depends on the weights only: every rank adds it in full AFTER the exchange)
    const AdamTail at = adam_tail(m, d_params, d_exp_avg, d_exp_avg_sq, ah, d_ctrl, d_loss, d_total);
    const int rc = igmc_launch_loss_grad(m->d, b->d, sp, B, use_edge_flags, hd, ARR, 1.0f, d_grad, nullptr, &at, stream,
                                         comm ? &x : nullptr, &emitted);
    img.done_updated(emitted);
    if (rc) return 1;
  } else {
    igmc_launch_loss_grad(m->d, b->d, sp, B, use_edge_flags, hd, ARR, 1.0f / (float)world, d_grad, nullptr, nullptr, stream);
    if (comm && igmc_comm_sum_flat(comm, d_grad, m->d.n_params, stream)) return 1;
    igmc_launch_finish(m->d, b->d, d_params, d_grad, d_exp_avg, d_exp_avg_sq, ah, d_ctrl, ARR, d_loss, d_total, use_edge_flags, stream);
    img.done_updated(0);
  }
  HIPCHECK(hipGetLastError());
  end_call(m, b, 1, use_edge_flags);
  return 0;
}

// ------------------------------------------------------------------ sort-pool readout family (DGCNN_RS)
struct igmc_sortpool {
  igmc_model* m;
  SpDev d;
  float* pe;        // engine-layout copy of the conv parameters (layer 3 zero-padded to 32 columns)
  float* ge;        // engine-layout gradient scratch
  Allocs mem;
};

extern "C" int igmc_sortpool_create(igmc_model* m, int k, int max_nodes_per_graph, igmc_sortpool** out) {
  if (!m || !out) IGMC_FAIL("null argument");
  if (k < 10) IGMC_FAIL("sort-pool k must be >= 10 (reference models.py:73)");
  if (m->d.S != 0) IGMC_FAIL("the sort-pool readout takes no side features");
  if (max_nodes_per_graph < 2 || max_nodes_per_graph > 4096) IGMC_FAIL("subgraphs of 2..4096 nodes");
  HIPCHECK(hipSetDevice(m->device));
  igmc_sortpool* sp = new igmc_sortpool();
  sp->m = m;
  SpDev& d = sp->d;
  const ModelDev& md = m->d;
  d.k = k;
  d.Q1 = k / 2;                       // int((k - 2) / 2 + 1), reference models.py:83
  d.Q2 = d.Q1 - 5 + 1;
  if (d.Q2 < 1) { delete sp; IGMC_FAIL("k too small for Conv1d(16, 32, 5)"); }
  d.dense = d.Q2 * 32;
  d.nmax = max_nodes_per_graph;
  d.P = 1;
  while (d.P < d.nmax) d.P <<= 1;
  // true layout: layers 0..2 at the engine offsets, then layer 3 with one output column
  int64_t off = md.off_basis[3];
  d.t_basis3 = off; off += 4 * 32;
  d.t_root3 = off;  off += 32;
  d.t_bias3 = off;  off += 1;
  d.t_att3 = off;   off += (int64_t)md.R * 4;
  d.t_conv_end = off;
  d.t_c1w = off; off += 16 * 97 + 16;
  d.t_c2w = off; off += 32 * 16 * 5 + 32;
  d.t_l1w = off; off += (int64_t)128 * d.dense;
  d.t_l1b = off; off += 128;
  d.t_l2w = off; off += 128;
  d.t_l2b = off; off += 1;
  d.n_params = off;
  if (!igmc_sp_lds_ok(d)) { delete sp; IGMC_FAIL("k / subgraph size too large for the LDS plan of the sort-pool kernels"); }
  Allocs& M = sp->mem;
  const size_t Bc = (size_t)md.graph_cap, N = (size_t)md.node_cap;
  int fail = 0;
  fail |= M.get(&d.sel, Bc * k) | M.get(&d.y1, Bc * 16 * k) | M.get(&d.flat, Bc * d.dense) | M.get(&d.dflat, Bc * d.dense) | M.get(&d.lin_part, 8 * Bc) | M.get(&d.lin_ctr, Bc / 16 + 1) | M.get(&d.a1, Bc * 128) |
          M.get(&d.lmask, Bc * 128) | M.get(&d.dz, Bc * 128) | M.get(&d.dout, Bc) |
          M.get(&d.part_c1, Bc * (16 * 97 + 16)) | M.get(&d.part_c2, Bc * (32 * 16 * 5 + 32));
  for (int l = 0; l < 3; ++l) fail |= M.get(&d.dcat[l], N * 32);
  fail |= M.get(&sp->pe, (size_t)md.n_params) | M.get(&sp->ge, (size_t)md.n_params);
  if (fail) {
    M.release();
    delete sp;
    IGMC_FAIL("hipMalloc failed (sort-pool workspace)");
  }
  HIPCHECK(hipMemset(d.lin_ctr, 0, (Bc / 16 + 1) * sizeof(int)));        // arrival counters: zero between launches
  HIPCHECK(hipMemset(sp->pe, 0, (size_t)md.n_params * sizeof(float)));
  HIPCHECK(hipMemset(sp->ge, 0, (size_t)md.n_params * sizeof(float)));
  if (igmc_sp_prepare(d)) { M.release(); delete sp; IGMC_FAIL("hipFuncSetAttribute failed"); }
  *out = sp;
  return 0;
}

extern "C" void igmc_sortpool_destroy(igmc_sortpool* sp) {
  if (!sp) return;
  sp->mem.release();
  delete sp;
}

// [0..16): basis, root, bias, att of conv layers 0..3; then conv1.weight, conv1.bias, conv2.weight, conv2.bias,
// lin1.weight, lin1.bias, lin2.weight, lin2.bias; [24] = number of parameters, [25] = dense width, [26] = k
extern "C" int igmc_sortpool_layout(const igmc_sortpool* sp, int64_t* out27) {
  if (!sp || !out27) IGMC_FAIL("null argument");
  const ModelDev& md = sp->m->d;
  const SpDev& d = sp->d;
  for (int l = 0; l < 3; ++l) {
    out27[4 * l + 0] = md.off_basis[l]; out27[4 * l + 1] = md.off_root[l];
    out27[4 * l + 2] = md.off_bias[l];  out27[4 * l + 3] = md.off_att[l];
  }
  out27[12] = d.t_basis3; out27[13] = d.t_root3; out27[14] = d.t_bias3; out27[15] = d.t_att3;
  out27[16] = d.t_c1w; out27[17] = d.t_c1w + 16 * 97; out27[18] = d.t_c2w; out27[19] = d.t_c2w + 32 * 16 * 5;
  out27[20] = d.t_l1w; out27[21] = d.t_l1b; out27[22] = d.t_l2w; out27[23] = d.t_l2b;
  out27[24] = d.n_params; out27[25] = d.dense; out27[26] = d.k;
  return 0;
}

static int sp_check(igmc_sortpool* sp, const igmc_batch* b, std::string* why) {
  if (!sp) { *why = "null sort-pool workspace"; return 1; }
  if (check_fit(sp->m, b, why)) return 1;
  if (b->d.slot > sp->d.nmax) { *why = "subgraph slots larger than the sort-pool workspace was created for"; return 1; }
  return 0;
}

// reference DGCNN_RS.forward (models.py:142-167) on an extracted batch
extern "C" int igmc_sortpool_forward(igmc_sortpool* sp, const float* d_params, const igmc_batch* b, int training,
                                     int use_edge_flags, const uint8_t* d_lin_mask, uint64_t seed, uint64_t step,
                                     float* d_out, void* stream) {
  std::string why;
  if (sp_check(sp, b, &why)) IGMC_FAIL(why);
  if (!d_params || !d_out) IGMC_FAIL("null buffer");
  igmc_model* m = sp->m;
  ensure_csr(b, stream);
  igmc_launch_sp_pack(m->d, sp->d, d_params, sp->pe, stream);
  StepPlan plan;
  igmc_step_plan(m->d, b->d, b->last_B, IGMC_CALL_CONV, &plan);
  igmc_launch_conv_forward(m->d, b->d, plan, sp->pe, b->last_B, training, use_edge_flags, stream);
  const StepHead hd = {d_params, d_lin_mask, seed, step, 1.f, 0.f, d_out};
  igmc_launch_sp_forward(m->d, sp->d, b->d, b->last_B, training, hd, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}

// forward + MSE (+ ARR over the conv layers, reference train_eval.py:162-174) + backward: d_grad in the true layout
extern "C" int igmc_sortpool_loss_grad(igmc_sortpool* sp, const float* d_params, const igmc_batch* b, int use_edge_flags,
                                       const uint8_t* d_lin_mask, uint64_t seed, uint64_t step, float ARR,
                                       float grad_scale, float arr_scale, float* d_out, float* d_grad, float* d_loss,
                                       void* stream) {
  std::string why;
  if (sp_check(sp, b, &why)) IGMC_FAIL(why);
  if (!d_params || !d_out || !d_grad) IGMC_FAIL("null buffer");
  igmc_model* m = sp->m;
  const int B = b->last_B;
  ensure_csr(b, stream);
  igmc_launch_sp_pack(m->d, sp->d, d_params, sp->pe, stream);
  ModelDev md = m->d;        // (with the dense readout gradient: the conv kernels then know which backward form follows)
  for (int l = 0; l < 3; ++l) md.dcat[l] = sp->d.dcat[l];
  StepPlan plan;
  igmc_step_plan(md, b->d, B, IGMC_CALL_CONV, &plan);
  igmc_launch_conv_forward(md, b->d, plan, sp->pe, B, 1, use_edge_flags, stream);
  const StepHead hd = {d_params, d_lin_mask, seed, step, 1.f, 0.f, d_out};
  igmc_launch_sp_forward(m->d, sp->d, b->d, B, 1, hd, stream);
  igmc_launch_sp_backward(m->d, sp->d, b->d, d_params, B, grad_scale > 0.f ? grad_scale : 1.f / (float)B, stream);
  igmc_launch_conv_backward(md, b->d, plan, sp->pe, B, use_edge_flags, ARR * arr_scale, sp->ge, stream);
  igmc_launch_sp_wgrad(m->d, sp->d, b->d, B, sp->ge, d_grad, stream);
  if (d_loss) igmc_launch_loss(m->d, b->d, ARR, d_loss, stream);
  HIPCHECK(hipGetLastError());
  m->last_flags = use_edge_flags;
  return 0;
}

extern "C" int igmc_sortpool_step_finish(igmc_sortpool* sp, const igmc_batch* b, float* d_params, const float* d_grad,
                                         float* d_exp_avg, float* d_exp_avg_sq, float ARR, float* d_loss, double* d_total,
                                         int64_t* d_ctrl, int64_t step, float lr, float beta1, float beta2, float eps,
                                         float weight_decay, void* stream) {
  if (!sp || !b || !d_params || !d_grad || !d_exp_avg || !d_exp_avg_sq || !d_loss) IGMC_FAIL("bad arguments");
  if (!d_ctrl && step < 1) IGMC_FAIL("step must be >= 1");
  ModelDev md = sp->m->d;
  md.n_params = sp->d.n_params;          // Adam runs over the sort-pool family's own flat buffer
  igmc_launch_finish(md, b->d, d_params, d_grad, d_exp_avg, d_exp_avg_sq, adam_scalars(d_ctrl, step, lr, beta1, beta2, eps, weight_decay),
                     d_ctrl, ARR, d_loss, d_total, sp->m->last_flags, stream);
  HIPCHECK(hipGetLastError());
  return 0;
}
