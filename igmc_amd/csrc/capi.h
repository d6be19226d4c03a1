// capi.h -- what the translation units that hold extern "C" entry points agree on (internal): the error string, the refusal
// macros, the slab allocator and the handle objects.  capi.hip owns the objects; a serving family's file (scores.hip,
// candidates.hip, ...) holds its own entry points below its launchers and reads the handles through these definitions.
#pragma once
#include "launch.h"

#include <algorithm>
#include <climits>
#include <string>
#include <vector>

#define IGMC_INTERNAL __attribute__((visibility("hidden")))      // crosses translation units, never the library's boundary

IGMC_INTERNAL std::string& igmc_err();      // the calling thread's igmc_last_error (ONE definition: capi.hip)

#define IGMC_FAIL(msg)                                                      \
  do {                                                                      \
    igmc_err() = std::string(__func__) + ": " + (msg);                      \
    return 1;                                                               \
  } while (0)
#define HIPCHECK(expr)                                                      \
  do {                                                                      \
    hipError_t e_ = (expr);                                                 \
    if (e_ != hipSuccess) {                                                 \
      igmc_err() = std::string(__func__) + ": " #expr " -> " + hipGetErrorString(e_); \
      return 1;                                                             \
    }                                                                       \
  } while (0)

// Buffers of one handle are carved out of a few large slabs (256-byte aligned) instead of one hipMalloc each: the
// ~40 arrays a kernel chain touches then share a handful of large pages (fewer address-translation misses on the
// first touch of every hop) and creation does 1-2 driver calls instead of 40.
struct Allocs {
  std::vector<void*> ptrs;
  size_t bytes = 0;
  char* slab = nullptr;
  size_t slab_left = 0;
  static constexpr size_t SLAB = (size_t)32 << 20;
  template <typename T> int get(T** out, size_t n) {
    const size_t b = (std::max<size_t>(n, 1) * sizeof(T) + 255) & ~(size_t)255;
    bytes += b;
    if (b > SLAB / 2 && !(packed && b <= slab_left)) {                 // large arrays get their own allocation
      void* p = nullptr;
      if (hipMalloc(&p, b) != hipSuccess) return 1;
      ptrs.push_back(p);
      *out = (T*)p;
      return 0;
    }
    if (b > slab_left) {
      void* p = nullptr;
      if (hipMalloc(&p, SLAB) != hipSuccess) return 1;
      ptrs.push_back(p);
      slab = (char*)p;
      slab_left = SLAB;
    }
    *out = (T*)slab;
    slab += b;
    slab_left -= b;
    return 0;
  }
  // the arrays that follow were counted into `b` bytes (256-byte steps): one allocation of exactly that size takes them all
  bool packed = false;
  int reserve(size_t b) {
    void* p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(b, 256)) != hipSuccess) return 1;
    ptrs.push_back(p);
    slab = (char*)p;
    slab_left = std::max<size_t>(b, 256);
    packed = true;
    return 0;
  }
  void release() {
    for (void* p : ptrs) hipFree(p);
    ptrs.clear();
    slab = nullptr;
    slab_left = 0;
  }
};

struct igmc_graph {
  int device;
  GraphDev d;
  int64_t nnz;
  int max_rel;
  int max_deg_u, max_deg_v;     // longest user row / item column (bounds the hop-1 subgraph sides)
  Allocs mem;
};

struct igmc_batch {
  const igmc_graph* g;
  BatchDev d;
  int last_B;
  const float* side;
  int n_side;
  const float* side_src;    // dataset-wide [n_links, n_side] matrix (igmc_batch_bind_side_source); rows gathered per batch
  const float *side_u, *side_v;      // per-node tables [side_nu, side_fu] / [side_nv, side_fv] (igmc_batch_bind_side_tables);
  int side_nu, side_fu, side_nv, side_fv;      // rows of the batch's target nodes gathered per batch; both NULL: none bound
  float* side_buf;          // [graph_cap, n_side] owned by the arena
  int side_buf_cols;
  int lean;                 // igmc_batch_set_lean: extraction stops after the dense blocks (capped arenas)
  const int64_t* ctrl;
  Allocs mem;
};

struct igmc_model {
  int device;
  ModelDev d;
  ModelAux ax;
  int* done_ctr;
  int last_B, last_training, last_flags;
  // weight images (g2_w) of the subgraph / dense-layer kernels: whose parameters they hold, and the caller's one-shot
  // assertion that those parameters have not changed since the previous call (igmc_model_weights_unchanged)
  int img_valid, img_hint;
  const float* img_params;
  Allocs mem;
};

// g2_probe.h (graphstep2.hip): debug aid of the tests -- one primitive of g2_prims.h / g2_image.h over n items of device memory
#define IGMC_PRIM_SPLIT 0    // (x, y) -> the three packed words of g2_split2
#define IGMC_PRIM_TANH 1     // x -> g2_tanh(x)
#define IGMC_PRIM_EXP 2      // x -> the exponential g2_tanh uses
#define IGMC_PRIM_RCP 3      // x -> the reciprocal g2_tanh uses
#define IGMC_PRIM_MFMA 4     // per lane of a wave: A [4], B [4], C [4] -> D [4] of one g2_mfma_bf16
#define IGMC_PRIM_MASK 5     // (word, r1, keep bit, FLAGS) -> g2_expand4, g2_bytemask, g2_mask_frag
#define IGMC_PRIM_OPS 6
extern "C" int igmc_debug_g2_prims(int op, const void* in, int64_t n, void* out, void* stream);

// capi.hip: debug aid of the tests -- the stored rows h_0 .. h_2 of the last training launch (igmc_debug_l3_sums reads h_2 through it)
extern "C" int igmc_debug_layer_rows(const igmc_model* m, const igmc_batch* b, int layer, int form, float* h_out, int64_t n);

// comm.hip: what igmc_train_step_dp needs of a communicator, and no more (c == NULL: one rank)
IGMC_INTERNAL int igmc_comm_world(const igmc_comm* c);
IGMC_INTERNAL StepExchange igmc_comm_exchange(igmc_comm* c);      // the sum of two spans, its user pointer, the peer failure word
IGMC_INTERNAL int igmc_comm_sum_flat(igmc_comm* c, float* d_flat, int64_t n, void* stream);      // 0, or 1 with the error set
