// comm.hip -- gradient exchange (RCCL behind the C ABI): the communicator object in its three forms (RCCL, host callback,
// peer-mapped buffers), the one-shot peer all-reduce kernel and the igmc_comm_* entry points.  igmc_train_step_dp (capi.hip)
// reaches a communicator through the three functions at the end of this file (capi.h), never through the struct.
#include "capi.h"

#include <cstdlib>
#include <cstring>

#define IGMC_MAX_PEERS 16
struct igmc_comm {
  void* nccl;        // ncclComm_t (NULL: host-callback / peer communicator, or the emulation build's single rank)
  int rank, world, device;
  igmc_allreduce_fn host_fn;      // igmc_comm_create_host: the caller's own sum over the ranks
  void* host_user;
  // peer communicator (igmc_comm_peer_alloc / _connect): every rank publishes into its OWN buffer, mapped by the others
  unsigned long long* pub[IGMC_MAX_PEERS];      // [2 slots][cap] {f32, tag} words of rank r (pub[rank] = the local buffer)
  int64_t cap;                                  // floats a slot holds
  int* d_state;                                 // device: [0] launch sequence number, [1] workgroups done, [2] poll timed out
  int peer;                                     // 1 = peer communicator
  int connected;
  int fine;                                     // the local buffer is fine-grained device memory
};
#ifndef IGMC_HIPEMU
#include <dlfcn.h>
// RCCL's entry points, resolved at the first use.  The few types needed are restated here (rccl.h: ncclUniqueId = 128
// opaque bytes; ncclFloat = 7, ncclSum = 0; results: 0 = success) so that the build needs no RCCL headers.
struct NcclId { char internal[128]; };
struct RcclApi {
  int (*GetUniqueId)(NcclId*);
  int (*CommInitRank)(void**, int, NcclId, int);
  int (*CommDestroy)(void*);
  int (*CommCount)(const void*, int*);
  int (*CommUserRank)(const void*, int*);
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t);
  int (*GroupStart)();
  int (*GroupEnd)();
  const char* (*GetErrorString)(int);
  bool ok = false;
};
static RcclApi g_rccl;
static int rccl_load(std::string* why) {
  if (g_rccl.ok) return 0;
  void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);      // the copy the process already holds, if any (same soname)
  if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!h) { *why = std::string("cannot load librccl.so.1: ") + dlerror(); return 1; }
  struct { const char* name; void** slot; } syms[] = {
      {"ncclGetUniqueId", (void**)&g_rccl.GetUniqueId}, {"ncclCommInitRank", (void**)&g_rccl.CommInitRank},
      {"ncclCommDestroy", (void**)&g_rccl.CommDestroy}, {"ncclCommCount", (void**)&g_rccl.CommCount},
      {"ncclCommUserRank", (void**)&g_rccl.CommUserRank}, {"ncclAllReduce", (void**)&g_rccl.AllReduce},
      {"ncclGroupStart", (void**)&g_rccl.GroupStart}, {"ncclGroupEnd", (void**)&g_rccl.GroupEnd},
      {"ncclGetErrorString", (void**)&g_rccl.GetErrorString}};
  for (auto& sy : syms) {
    *sy.slot = dlsym(h, sy.name);
    if (!*sy.slot) { *why = std::string("librccl.so.1 lacks ") + sy.name; return 1; }
  }
  g_rccl.ok = true;
  return 0;
}
#define RCCLCHECK(expr)                                                                              \
  do {                                                                                               \
    int r_ = (expr);                                                                                 \
    if (r_ != 0) {                                                                                   \
      igmc_err() = std::string(__func__) + ": " #expr " -> " + g_rccl.GetErrorString(r_);            \
      return 1;                                                                                      \
    }                                                                                                \
  } while (0)
#endif

__global__ __launch_bounds__(IGMC_BLOCK) void k_scale_flat(float* p, int64_t n, float s) {
  for (int64_t i = (int64_t)blockIdx.x * IGMC_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * IGMC_BLOCK) p[i] *= s;
}

extern "C" int igmc_comm_unique_id(uint8_t* h_id128) {
  if (!h_id128) IGMC_FAIL("null id buffer");
#ifndef IGMC_HIPEMU
  std::string why;
  if (rccl_load(&why)) IGMC_FAIL(why);
  NcclId id;
  RCCLCHECK(g_rccl.GetUniqueId(&id));
  memcpy(h_id128, id.internal, 128);
#else
  memset(h_id128, 0, 128);
#endif
  return 0;
}

extern "C" int igmc_comm_create(const uint8_t* h_id128, int rank, int world, int device, igmc_comm** out) {
  if (!h_id128 || !out || world < 1 || rank < 0 || rank >= world) IGMC_FAIL("bad arguments");
  igmc_comm* c = new igmc_comm();
  c->nccl = nullptr;
  c->rank = rank;
  c->world = world;
  c->device = device;
  c->host_fn = nullptr;
  c->host_user = nullptr;
  c->peer = 0;
  c->d_state = nullptr;
#ifndef IGMC_HIPEMU
  std::string why;
  if (rccl_load(&why)) { delete c; IGMC_FAIL(why); }
  HIPCHECK(hipSetDevice(device));
  NcclId id;
  memcpy(id.internal, h_id128, 128);
  const int r = g_rccl.CommInitRank(&c->nccl, world, id, rank);
  if (r != 0) {
    delete c;
    IGMC_FAIL(std::string("ncclCommInitRank -> ") + g_rccl.GetErrorString(r));
  }
#else
  if (world != 1) { delete c; IGMC_FAIL("the emulation build has no RCCL: one rank only"); }
#endif
  *out = c;
  return 0;
}

extern "C" int igmc_comm_create_host(igmc_allreduce_fn fn, void* user, int rank, int world, igmc_comm** out) {
  if (!fn || !out || world < 1 || rank < 0 || rank >= world) IGMC_FAIL("bad arguments");
  igmc_comm* c = new igmc_comm();
  c->nccl = nullptr;
  c->rank = rank;
  c->world = world;
  c->device = -1;
  c->host_fn = fn;
  c->host_user = user;
  c->peer = 0;
  c->d_state = nullptr;
  *out = c;
  return 0;
}

// ---- peer communicator: a one-shot all-reduce over peer-mapped buffers ------------------------------------------------
// The exchange of a step is ~60 k floats between a handful of GPUs of ONE node: a ring collective pays 2 (G - 1) hops of
// launch + link latency for it, while every rank can simply READ the other ranks' values -- xGMI is point to point.  Every
// rank owns a publish buffer (hipMalloc + hipIpcGetMemHandle, mapped by the others with hipIpcOpenMemHandle); a launch
// of k_peer_allreduce writes the rank's span into its own buffer as 8-byte {value, tag} words (flag in data: single-copy
// atomic, system scope), then reads the same words of EVERY rank in rank order -- polling a word until its tag is this
// launch's -- and leaves the sum in place.  Same order on every rank: bit-identical replicas.  No barrier, no second
// launch: about one xGMI round trip.  Two slots alternate: a rank can only be ONE launch ahead of the slowest one (it
// cannot finish launch s + 1 before every rank published s + 1, i.e. finished reading s), so slot s & 1 is never
// overwritten while someone still reads it.  The launch sequence number lives in device memory and is advanced by the
// launch's last workgroup -- a hipGraph replay carries no host-side counter.  Bounded polls raise d_state[2].
struct PeerArgs {
  unsigned long long* pub[IGMC_MAX_PEERS];
  int world, rank;
  int64_t cap;
  unsigned long long timeout_ticks;      // bound of a poll on the device's constant-rate clock (100 MHz)
  int* state;
  float* a;
  int64_t na;
  float* b;
  int64_t nb;
};
__global__ __launch_bounds__(IGMC_BLOCK) void k_peer_allreduce(PeerArgs p) {
#ifndef IGMC_HIPEMU
  const uint32_t seq = (uint32_t)__hip_atomic_load(p.state, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  const uint32_t seq = (uint32_t)p.state[0];
#endif
  const unsigned long long tag = (unsigned long long)seq << 32;
  const int64_t n = p.na + p.nb, base = (int64_t)(seq & 1u) * p.cap;
  const int64_t T = (int64_t)gridDim.x * IGMC_BLOCK, t0 = (int64_t)blockIdx.x * IGMC_BLOCK + threadIdx.x;
  unsigned long long* mine = p.pub[p.rank] + base;
  for (int64_t i = t0; i < n; i += T) {
    const float v = (i < p.na) ? p.a[i] : p.b[i - p.na];
    const unsigned long long w = tag | (unsigned long long)__float_as_uint(v);
#ifndef IGMC_HIPEMU
    __hip_atomic_store(mine + i, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#else
    mine[i] = w;
#endif
  }
  // A rank may be late by far more than a kernel's length -- first-step capture, a checkpoint write on rank 0, a
  // time-sliced device: the polls are bounded by WALL-CLOCK time (p.timeout_ticks, a minute by default), not by an
  // iteration count.  A word that never arrives raises the sticky p.state[2]: the element is left as it was, every thread
  // that sees the flag stops summing, but elements summed BEFORE a thread gave up stay summed -- after a time-out the spans
  // are a mixture of sums and local values and MUST NOT be used (no foreign or torn value is ever written: a word counts
  // only with this launch's tag in it).  The gradient / Adam kernel of igmc_train_step_dp behind this launch reads the
  // flag and leaves parameters, moments and counters alone (AdamTail::skip); the host raises at its next check
  // (igmc_comm_check).  Callers of the bare igmc_allreduce_grads must call igmc_comm_check before they use the spans.
  //
  // CROSS-DEVICE visibility (the words of rank r live in r's HBM, fine-grained, mapped over xGMI): value and flag are ONE
  // 8-byte word written by ONE system-scope atomic store (global_store_dwordx2 sc0 sc1: written through, never parked in the
  // writer's L2) and read by ONE system-scope atomic load (sc0 sc1: never served from the reader's L2) -- single-copy
  // atomic, so a reader sees either the old word (old tag: polls again) or the whole new one.  Nothing else is published
  // through these buffers, so no release / acquire ordering BETWEEN words is needed: every word validates itself.
#ifndef IGMC_HIPEMU
  const unsigned long long t_start = wall_clock64();
#endif
  for (int64_t i = t0; i < n; i += T) {
    float s = 0.f;
    bool ok = true;
    for (int r = 0; r < p.world && ok; ++r) {
      const unsigned long long* src = p.pub[r] + base + i;
      unsigned long long w = 0;
      for (long it = 0;; ++it) {
#ifndef IGMC_HIPEMU
        w = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#else
        w = *src;
#endif
        if ((w >> 32) == (unsigned long long)seq) break;
#ifndef IGMC_HIPEMU
        if ((it & 63) == 63 && wall_clock64() - t_start > p.timeout_ticks) ok = false;
        if (__hip_atomic_load(p.state + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) ok = false;      // (another thread gave up)
#else
        if (it > (1L << 22)) ok = false;
#endif
        if (!ok) {
          p.state[2] = 1;
          break;
        }
#ifndef IGMC_HIPEMU
        __builtin_amdgcn_s_sleep(4);
#endif
      }
      s += __uint_as_float((uint32_t)w);
    }
    if (ok) {
      if (i < p.na) p.a[i] = s;
      else p.b[i - p.na] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#ifndef IGMC_HIPEMU
    if (__hip_atomic_fetch_add(p.state + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1) {
      __hip_atomic_store(p.state + 1, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(p.state, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#else
    if (p.state[1]++ == (int)gridDim.x - 1) {
      p.state[1] = 0;
      p.state[0] += 1;
    }
#endif
  }
}

extern "C" int igmc_comm_peer_alloc(int rank, int world, int device, int64_t max_floats, igmc_comm** out, uint8_t* h_handle64) {
  if (!out || !h_handle64 || world < 1 || world > IGMC_MAX_PEERS || rank < 0 || rank >= world || max_floats < 1) IGMC_FAIL("bad arguments");
  igmc_comm* c = new igmc_comm();
  c->nccl = nullptr;
  c->rank = rank;
  c->world = world;
  c->device = device;
  c->host_fn = nullptr;
  c->host_user = nullptr;
  c->peer = 1;
  c->connected = 0;
  c->cap = (max_floats + 63) & ~(int64_t)63;
  for (int r = 0; r < IGMC_MAX_PEERS; ++r) c->pub[r] = nullptr;
  memset(h_handle64, 0, 64);
#ifndef IGMC_HIPEMU
  HIPCHECK(hipSetDevice(device));
  // FINE-GRAINED device memory where the runtime can share it (coherent between devices while kernels run: what RCCL's
  // own buffers are); else ordinary device memory -- the words are written and read with system-scope accesses either way
  const size_t bytes = (size_t)2 * c->cap * sizeof(unsigned long long);
  hipIpcMemHandle_t h;
  static_assert(sizeof(hipIpcMemHandle_t) <= 64, "IPC handle larger than the 64 bytes of the C ABI");
  bool fine = hipExtMallocWithFlags((void**)&c->pub[rank], bytes, hipDeviceMallocFinegrained) == hipSuccess;
  if (fine && hipIpcGetMemHandle(&h, c->pub[rank]) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(c->pub[rank]);
    c->pub[rank] = nullptr;
    fine = false;
  }
  if (!fine) {
    (void)hipGetLastError();
    HIPCHECK(hipMalloc((void**)&c->pub[rank], bytes));
    HIPCHECK(hipIpcGetMemHandle(&h, c->pub[rank]));
  }
  c->fine = fine ? 1 : 0;
  HIPCHECK(hipMemset(c->pub[rank], 0, bytes));      // tag 0 is never a launch's
  HIPCHECK(hipMalloc((void**)&c->d_state, 4 * sizeof(int)));
  const int init[4] = {1, 0, 0, 0};
  HIPCHECK(hipMemcpy(c->d_state, init, sizeof(init), hipMemcpyHostToDevice));
  memcpy(h_handle64, &h, sizeof(h));
  HIPCHECK(hipDeviceSynchronize());
#else
  if (world != 1) { delete c; IGMC_FAIL("the emulation build has one rank only"); }
  c->pub[rank] = (unsigned long long*)calloc((size_t)2 * c->cap, sizeof(unsigned long long));
  c->d_state = (int*)calloc(4, sizeof(int));
  c->d_state[0] = 1;
#endif
  *out = c;
  return 0;
}

extern "C" int igmc_comm_peer_connect(igmc_comm* c, const uint8_t* h_handles) {
  if (!c || !c->peer || !h_handles) IGMC_FAIL("not a peer communicator");
#ifndef IGMC_HIPEMU
  HIPCHECK(hipSetDevice(c->device));
  for (int r = 0; r < c->world; ++r) {
    if (r == c->rank) continue;
    hipIpcMemHandle_t h;
    memcpy(&h, h_handles + (size_t)r * 64, sizeof(h));
    void* ptr = nullptr;
    HIPCHECK(hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess));
    c->pub[r] = (unsigned long long*)ptr;
  }
#endif
  c->connected = 1;
  return 0;
}

// 0 = the communicator's device-side state is sane; synchronises `stream`.  A peer communicator whose bounded poll ran out
// (a rank that never published: not co-resident, crashed, or peer memory that is not visible) reports it here.
extern "C" int igmc_comm_check(igmc_comm* c, void* stream) {
  if (!c) IGMC_FAIL("null communicator");
#ifndef IGMC_HIPEMU
  HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
  if (c->peer && c->d_state) {
    int st[4];
    HIPCHECK(hipMemcpy(st, c->d_state, sizeof(st), hipMemcpyDeviceToHost));
    if (st[2]) {
      // reported once: the flag is cleared so that a caller that recovers (or tears the job down in order) is not told again
      const int zero = 0;
      (void)hipMemcpy(c->d_state + 2, &zero, sizeof(int), hipMemcpyHostToDevice);
      IGMC_FAIL("peer all-reduce: another rank's words did not arrive within the time limit (IGMC_PEER_TIMEOUT_S); the spans of that "
                "launch were left unsummed and the optimiser step behind it was skipped");
    }
  }
#endif
  return 0;
}

// 0 none (one rank), 1 RCCL, 2 host callback, 3 peer-mapped buffers (4: in fine-grained device memory)
extern "C" int igmc_comm_kind(const igmc_comm* c) {
  if (!c) return 0;
  if (c->peer) return c->fine ? 4 : 3;
  if (c->host_fn) return 2;
  return c->nccl ? 1 : 0;
}

static int peer_sum2(igmc_comm* c, float* a, int64_t na, float* b, int64_t nb, void* stream) {
  if (!c->connected) { igmc_err() = "peer communicator is not connected (igmc_comm_peer_connect)"; return 1; }
  if (c->world == 1 && !getenv("IGMC_PEER_ALWAYS")) return 0;      // one rank: the spans ARE the sums (IGMC_PEER_ALWAYS: test hook)
  if (!a) na = 0;
  if (!b) nb = 0;
  double tmo = 60.0;
  if (const char* e = getenv("IGMC_PEER_TIMEOUT_S")) tmo = atof(e) > 0 ? atof(e) : tmo;
  // spans beyond a slot go in pieces (each piece is a launch of its own: the sequence number advances per launch)
  while (na + nb > 0) {
    PeerArgs p;
    memset(&p, 0, sizeof(p));
    for (int r = 0; r < c->world; ++r) p.pub[r] = c->pub[r];
    p.world = c->world; p.rank = c->rank; p.cap = c->cap; p.state = c->d_state;
    p.timeout_ticks = (unsigned long long)(tmo * 1e8);
    const int64_t ta = na < c->cap ? na : c->cap;
    const int64_t tb = (nb < c->cap - ta) ? nb : c->cap - ta;
    p.a = a; p.na = ta; p.b = b; p.nb = tb;
    int grid = (int)((ta + tb + 4 * IGMC_BLOCK - 1) / (4 * IGMC_BLOCK));      // four words a thread; few workgroups: every
    if (grid > 64) grid = 64;                                                  // rank's launch must be on its chip at once
    if (grid < 1) grid = 1;
    IGMC_PLAUNCH("k_peer_allreduce", k_peer_allreduce, grid, IGMC_BLOCK, 0, stream, p);
    a += ta; na -= ta;
    b += tb; nb -= tb;
  }
#ifndef IGMC_HIPEMU
  if (hipGetLastError() != hipSuccess) { igmc_err() = "k_peer_allreduce launch failed"; return 1; }
#endif
  return 0;
}

extern "C" void igmc_comm_destroy(igmc_comm* c) {
  if (!c) return;
#ifndef IGMC_HIPEMU
  if (c->nccl && g_rccl.ok) g_rccl.CommDestroy(c->nccl);
  if (c->peer) {
    for (int r = 0; r < c->world; ++r)
      if (c->pub[r]) {
        if (r == c->rank) hipFree(c->pub[r]);
        else hipIpcCloseMemHandle(c->pub[r]);
      }
    if (c->d_state) hipFree(c->d_state);
  }
#else
  if (c->peer) {
    free(c->pub[c->rank]);
    free(c->d_state);
  }
#endif
  delete c;
}

extern "C" int igmc_comm_info(const igmc_comm* c, int* rank, int* world) {
  if (!c) IGMC_FAIL("null communicator");
  int r = c->rank, w = c->world;
#ifndef IGMC_HIPEMU
  if (c->nccl) {
    RCCLCHECK(g_rccl.CommUserRank(c->nccl, &r));
    RCCLCHECK(g_rccl.CommCount(c->nccl, &w));
  }
#endif
  if (rank) *rank = r;
  if (world) *world = w;
  return 0;
}

// sum of up to two spans over the ranks, in place: ONE grouped collective (RCCL), or the host callback once per span
static int comm_sum2(void* user, float* a, int64_t na, float* b, int64_t nb, void* stream) {
  igmc_comm* c = (igmc_comm*)user;
  if (c->peer) return peer_sum2(c, a, na, b, nb, stream);
  if (c->host_fn) {
    if (a && na > 0 && c->host_fn(c->host_user, a, na, stream)) { igmc_err() = "comm_sum2: the host all-reduce callback failed"; return 1; }
    if (b && nb > 0 && c->host_fn(c->host_user, b, nb, stream)) { igmc_err() = "comm_sum2: the host all-reduce callback failed"; return 1; }
    return 0;
  }
#ifndef IGMC_HIPEMU
  if (!c->nccl) return 0;
  const bool two = a && na > 0 && b && nb > 0;
  if (two) RCCLCHECK(g_rccl.GroupStart());
  if (a && na > 0) RCCLCHECK(g_rccl.AllReduce(a, a, (size_t)na, /*ncclFloat*/ 7, /*ncclSum*/ 0, c->nccl, (hipStream_t)stream));
  if (b && nb > 0) RCCLCHECK(g_rccl.AllReduce(b, b, (size_t)nb, 7, 0, c->nccl, (hipStream_t)stream));
  if (two) RCCLCHECK(g_rccl.GroupEnd());
#endif
  return 0;
}

extern "C" int igmc_allreduce_grads(igmc_comm* c, float* d_flat_grad, int64_t n, float scale, void* stream) {
  if (!c || !d_flat_grad || n <= 0) IGMC_FAIL("bad arguments");
  if (comm_sum2(c, d_flat_grad, n, nullptr, 0, stream)) return 1;
  if (scale != 1.0f) {
    int grid = (int)((n + IGMC_BLOCK - 1) / IGMC_BLOCK);
    IGMC_PLAUNCH("k_scale_flat", k_scale_flat, grid > 1024 ? 1024 : grid, IGMC_BLOCK, 0, stream, d_flat_grad, n, scale);
    HIPCHECK(hipGetLastError());
  }
  return 0;
}

// ---- igmc_train_step_dp's view of a communicator (capi.h)
int igmc_comm_world(const igmc_comm* c) { return c ? c->world : 1; }
StepExchange igmc_comm_exchange(igmc_comm* c) { return {comm_sum2, c, (c && c->peer) ? c->d_state + 2 : nullptr}; }
int igmc_comm_sum_flat(igmc_comm* c, float* d_flat, int64_t n, void* stream) { return comm_sum2(c, d_flat, n, nullptr, 0, stream); }
