// launch.h -- host-side launcher declarations that cross translation units + optional per-kernel HIP-event timing (internal).
#pragma once
#include "model.h"
#include <string.h>
#include <type_traits>

// extract.hip
size_t igmc_extract_smem_bytes(const GraphDev& g);
void igmc_launch_extract(const GraphDev& g, const BatchDev& b, const int32_t* link_u, const int32_t* link_v,
                         const float* link_y, const int32_t* link_idx, int first, int B, int replay,
                         double sample_ratio, uint64_t seed, uint64_t epoch, const int64_t* ctrl, int lean, void* stream);
void igmc_launch_extract_set(const GraphDev& g, const BatchDev* d_set, const BatchDev& b0, int count, const int32_t* link_u,
                             const int32_t* link_v, const float* link_y, const int32_t* link_idx, int sel0, int B,
                             double sample_ratio, uint64_t seed, const int64_t* ctrl, float drop_p, int force_undirected,
                             uint64_t drop_seed, void* stream);
void igmc_launch_emit(const BatchDev& b, int B, void* stream);
void igmc_launch_emit_nodes(const BatchDev& b, int B, void* stream);
void igmc_launch_load_nodes(const BatchDev& b, const int64_t* uoff, const int32_t* unodes, const uint8_t* udist,
                            const int64_t* voff, const int32_t* vnodes, const uint8_t* vdist, const float* link_y,
                            const int32_t* link_idx, int first, int B, const int64_t* ctrl, void* stream);
void igmc_launch_edge_flags(const BatchDev& b, float p, int force_undirected, uint64_t seed, uint64_t step,
                            const int64_t* ctrl, void* stream);
void igmc_launch_relm_flags(const BatchDev& b, void* stream);
void igmc_launch_relm_dropout(const BatchDev& b, int B, float p, int force_undirected, uint64_t seed, uint64_t step,
                              const int64_t* ctrl, void* stream);
void igmc_launch_tick(int64_t* ctrl, void* stream);
void igmc_launch_regroup(int64_t* ctrl, int M, int64_t first_cur, int64_t first_next, void* stream);
void igmc_launch_gate(int64_t* ctrl, int q, int gk_min, long long delay_ticks, int delay_always, long long timeout_ticks,
                      void* stream);
void igmc_launch_fill_u8(uint8_t* p, int64_t n, uint8_t v, void* stream);
int igmc_extract_prepare(size_t smem);
// keys of the deciding byte that a k-th-key selection parks in its short list; more go through the radix passes.  Read in one
// place: kth_key.h's kth_parks (extract.hip: sample_fringe; candidates.hip: the sampled fill)
#ifdef IGMC_HIPEMU
// (CPU emulation only: the tests lower the bound through the environment to drive the radix path)
#include <stdlib.h>
static inline int igmc_sample_park() { const char* e = getenv("IGMC_SAMPLE_PARK"); return e ? atoi(e) : IGMC_BLOCK; }
#define IGMC_SAMPLE_PARK igmc_sample_park()
#else
#define IGMC_SAMPLE_PARK IGMC_BLOCK
#endif
// (IGMC_CAND_TILE_ITEMS, the enumeration's tile that tests/selection_checks.py restates, stands with CandArgs in cand_tile.h)

// model.hip
// auxiliary streams / events of a model (created with it; no launch sequence uses them at present: see the note at k_wgrad)
struct ModelAux {
  void* s1;
  void* s2;
  void* ev[8];
};
// The head's inputs of a call: parameters, the injected dropout mask (or null: drawn from seed / step), the output scale, the
// scale of the loss gradient (training steps; 0 elsewhere) and where the predictions go.  Filled once per call (capi.hip).
struct StepHead {
  const float* P;
  const uint8_t* inj_mask;
  uint64_t seed, step;
  float mult, grad_scale;
  float* out;
};
// Adam's scalars of one step: lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t) and the optimiser's constants.  All zero where the
// kernel reads them from a control block (adam_hyper_from_ctrl) or the stash (adam_hyper_from_stash) instead.
struct AdamHyper {
  float step_size, inv_sqrt_bc2, beta1, beta2, eps, wd;
};
// optional optimiser tail of k_finalize (single-GPU fused step): Adam on the parameters whose gradient the
// workgroup just produced (conv layers) / on a slice of the lin parameters (extra workgroups), then the LAST
// workgroup to finish emits loss / epoch total and advances the control block.
struct AdamTail {
  int enabled;
  float* p;
  float* m1;
  float* m2;
  AdamHyper h;
  int64_t* ctrl;
  int* done;
  BatchDev b;
  float ARR;
  float* loss;
  double* total;
  int use_flags;      // the step ran under edge dropout (the tick then also checks the arena's dropout stamp)
  const int* skip;    // data-parallel step: set by the gradient exchange when its sums did not arrive (StepExchange::failed);
                      // the whole launch then returns at once -- no parameter, moment or counter is touched
};
// (kernel arguments: the six floats stand where they always stood)
static_assert(sizeof(AdamHyper) == 24 && offsetof(AdamTail, h) == 32 && offsetof(AdamTail, ctrl) == 56 &&
              offsetof(AdamTail, b) == 72, "AdamTail's kernarg layout");
struct StepPlan;      // what a call launches: below (step_plan.h builds it, the launch sequences read it)
void igmc_launch_forward(const ModelDev& m, const BatchDev& b, const StepPlan& sp, int B, int training, int use_flags,
                         const StepHead& hd, void* stream);
void igmc_launch_conv_forward(const ModelDev& m, const BatchDev& b, const StepPlan& sp, const float* P, int B, int training,
                              int use_flags, void* stream);
void igmc_launch_conv_backward(const ModelDev& m, const BatchDev& b, const StepPlan& sp, const float* P, int B, int use_flags,
                               float arr_coef, float* grad, void* stream);
void igmc_launch_backward(const ModelDev& m, const BatchDev& b, const StepPlan& sp, const float* P, int B, int use_flags,
                          const float* gout, int from_err, float grad_scale, float mult, float drop_scale,
                          float arr_coef, float* grad, void* stream);
// Data-parallel step: the REDUCED gradient sources of the step (relation-space tables + d att partials of the subgraph
// kernel, or the basis-space partial sums of the per-layer path; plus the lin1 / lin2 gradients in `grad`) are summed over
// the ranks between their reduction and the gradient / Adam kernel -- the step keeps its single-GPU kernels, the exchange
// is one grouped collective of two spans.  sum() returns 0 on success.
struct StepExchange {
  int (*sum)(void* user, float* a, int64_t na, float* b, int64_t nb, void* stream);
  void* user;
  const int* failed;      // device word the exchange raises when its sums are NOT in place (a peer never delivered): the
                          // gradient / Adam kernel behind it then leaves parameters, moments and step counters alone; or null
};
// returns 0, or the exchange's error code
int igmc_launch_loss_grad(const ModelDev& m, const BatchDev& b, const StepPlan& sp, int B, int use_flags, const StepHead& hd,
                          float ARR, float arr_scale, float* grad, float* loss, const AdamTail* adam, void* stream,
                          const StepExchange* xch = nullptr, int* img_emitted = nullptr);
// (sp: a plan of kind IGMC_CALL_STEP; xch: see StepExchange -- only where sp.exchange_inside says so;
//  *img_emitted = 1 when the step's last kernel also left the weight images of the updated parameters in m.g2_w)
void igmc_launch_loss(const ModelDev& m, const BatchDev& b, float ARR, float* loss, void* stream);
void igmc_launch_sse(const BatchDev& b, const float* out, double* acc, int64_t* ctrl, void* stream);
// pairs.hip: the pair loss of a batch of (positive, negative) slots with its gradient w.r.t. the outputs, and the ARR term
// filed into its stats -- igmc_pair_loss_grad (capi.hip) runs them between the model's forward and backward
void igmc_launch_pair_loss(const float* out, const float* y, int B, float mse_weight, float* gout, double* stats, void* stream);
void igmc_launch_pair_arr(const float* arr_part, float ARR, double* stats, void* stream);
int igmc_model_prepare(const ModelDev& m);
void igmc_launch_adam(float* p, const float* g, float* m1, float* m2, int64_t n, const AdamHyper& h, int64_t* ctrl, int tick,
                      void* stream);
void igmc_launch_finish(const ModelDev& m, const BatchDev& b, float* p, const float* g, float* m1, float* m2, const AdamHyper& h,
                        int64_t* ctrl, float ARR, float* loss, double* total, int use_flags, void* stream);

// graphstep2.hip: one cluster of workgroups per enclosing subgraph, relational aggregation on the matrix cores
int igmc_g2_xcd_ok();      // g2_compose.h: 1 = workgroups b and b + 8 of a launch share an XCD on the current device
struct G2Layout {      // LDS plan of graphstep2.hip, offsets in 4-byte words
  int kp, nsides, rmr, rmc, pside;
  int planes, ohp, lab, xo, hs, tile, hist, px, wreg, t0, att, head, words;
};
void igmc_launch_side_gather(const float* src, int S, const int32_t* link_idx, int first, int B, const int64_t* ctrl,
                             float* dst, void* stream);
void igmc_launch_side_gather_nodes(const BatchDev& b, const float* uf, int n_u, int fu, const float* vf, int n_v, int fv,
                                   int B, float* dst, void* stream);
int igmc_gs_prepare();
int igmc_g2_prepare();

// What a call on (model, arena, B) launches (step_plan.h): THE decision.  Every launch sequence of model.hip takes its
// branches from a plan and every query of the C ABI reports one; the eligibility predicates and the environment hooks
// behind it are private to step_plan.h.
#define IGMC_CALL_EVAL 0     // evaluation forward: the subgraph kernel whatever the head's width, no backward
#define IGMC_CALL_CONV 1     // training forward, then backward, as calls of their own: the generic sequence and the sort-pool family
#define IGMC_CALL_STEP 2     // the fused step (loss + gradients [+ Adam]): needs fast_head, else the generic sequence
#define IGMC_FAM_ROWS 0      // the CSR row walkers (k_l0_fwd / k_rgcn_layer4)
#define IGMC_FAM_G2 1        // the subgraph kernel (k_graph_step)
#define IGMC_FAM_DLF 2       // the one-launch dense layers (k_dl_fwd)
#define IGMC_FAM_DL 3        // the per-layer dense layers (k_dl_layer0 / k_dl_layer)
#define IGMC_TAIL_HANDOFF 0  // gradient / Adam tail: k_finalize (in-kernel hand-offs)
#define IGMC_TAIL_TS 1       // ... k_tail_ts -> k_finalize_ts on relation-space tables (or both in one launch: StepPlan::tail_fold)
#define IGMC_TAIL_BS 2       // ... k_finalize_ts on the reduced basis-space sums
struct StepPlan {
  int kind;                  // IGMC_CALL_*
  int fast_head;             // 0: the generic sequence (igmc_launch_forward + igmc_launch_backward)
  int family;                // IGMC_FAM_* of the forward
  int cs, grid;              // subgraph kernel: workgroups per subgraph, grid
  G2Layout lay;              // ... its LDS plan
  int wide, dl, dlts, dlf, dlb;      // dense layers: relation groups, per-layer / one-launch eligible, relation-space tables,
                                     // one-launch forward, one-launch backward
  int nqu, nqv, dl_grid;     // ... workgroups of a subgraph's two sides (0 where no dense-layer kernel runs), B * (nqu + nqv)
  int gsplit;                // ... k_dl_fwd / k_dl_bwd in the group-split form
  int self_seq;              // ... k_dl_fwd's last workgroup advances the exchange tags itself (else: k_tail_ts behind it)
  int head_inside;           // ... the loss head runs in k_dl_bwd's set-up (IGMC_DL_HEAD=0: k_head_sub in front of it)
  int bwd_dense;             // the per-layer backward passes: k_dl_layer (else the row walkers)
  int need_y;                // the forward leaves the Y products behind (k_dense_y_all)
  int tail;                  // IGMC_TAIL_*
  int exchange_inside;       // the step keeps its gradient sources in exchangeable form (StepExchange)
  int tail_fold;             // subgraph kernel, IGMC_TAIL_TS: a single-GPU step with Adam and weight images runs the tail as ONE launch
                             // (k_tail_fin; its stash role rides in the subgraph kernel's launch) -- IGMC_TAIL_FOLD=0: never
  int l3_vec;                // subgraph kernel, IGMC_TAIL_TS: a clustered training step (cs > 1: every subgraph its own cluster) hands
                             // layer 3's weight gradient to the tail as the centre vectors (ModelDev::l3_vec), not as tables: 0, or
                             // the member that owns the item centre (2 cs / G2_NB >= 1; the user centre's is member 0) --
                             // IGMC_L3_VEC=0: never
  int needs_csr;             // some kernel of the call reads the collated CSR (a lean arena must emit it first)
  int dense_layers;          // the dense-layer kernels take this arena (igmc_model_dense_layers)
  int step_form;             // igmc_model_step_form
};
void igmc_step_plan(const ModelDev& m, const BatchDev& b, int B, int kind, StepPlan* p);
int igmc_dl_always();        // IGMC_DL_ALWAYS=1 (test hook): arenas with small slots get the transposed block as well
void igmc_launch_g2_compose(const ModelDev& m, const float* P, void* stream);
void igmc_launch_dl_layer0(const ModelDev& m, const BatchDev& b, int B, int training, int use_flags, void* stream);
// (head != NULL: the launch runs the subgraphs' loss head itself -- no k_head_sub launch in front of it)
// (dense3: the sort-pool family's backward -- dPre_3 of every row from m.dpre[3], the readout gradient of layers 0..2 from m.dcat)
void igmc_launch_dl_bwd(const ModelDev& m, const BatchDev& b, const StepPlan& sp, int B, int use_flags, void* stream,
                        const StepHead* head = nullptr, int dense3 = 0);
void igmc_launch_dl_fwd(const ModelDev& m, const BatchDev& b, const StepPlan& sp, const float* P, int B, int training,
                        int use_flags, float* zero_out, void* stream);
void igmc_launch_head_sub(const ModelDev& m, const BatchDev& b, int B, const StepHead& hd, void* stream);
void igmc_launch_dl_layer(const ModelDev& m, const BatchDev& b, const float* P, int B, int l, int bwd, int use_flags,
                          float* zero_out, void* stream, int tables = 0);
// (stash_ctrl / nstash = 4: four more workgroups behind sp.grid run the stash role of the one-launch tail that follows)
int igmc_launch_graph_step2(const ModelDev& m, const BatchDev& b, const StepPlan& sp, int B, int training, int use_flags,
                            const StepHead& hd, void* stream, int nstash = 0, const int64_t* stash_ctrl = nullptr);

// ---- per-kernel timing (HIP events on the launch stream; bench.py's roofline leg) ----
void igmc_prof_begin(const char* name, void* stream);
void igmc_prof_end(void* stream);
extern int g_igmc_prof_on;

#define IGMC_PLAUNCH(name, kern, grid, block, shmem, stream, ...)          \
  do {                                                                     \
    if (g_igmc_prof_on == 1) igmc_prof_begin(name, stream);                \
    IGMC_LAUNCH(kern, grid, block, shmem, stream, __VA_ARGS__);            \
    if (g_igmc_prof_on == 1) igmc_prof_end(stream);                        \
  } while (0)

// The NEXT launch's workgroups wait for each other: the CPU emulation must run the cs members x, x + stride, .. of a cluster
// together (inside blocks of `block` consecutive workgroups; hipemu::Runtime::co_cs).  The device needs no such request.
static inline void igmc_emu_cluster(int cs, int stride, int block) {
#ifdef IGMC_HIPEMU
  hipemu::rt().co_cs = cs;
  hipemu::rt().co_stride = stride;
  hipemu::rt().co_block = block;
#else
  (void)cs; (void)stride; (void)block;
#endif
}

// Runtime flags -> template arguments: igmc_dispatch([&](auto uf, auto tr) { ... k<uf(), tr()> ... }, use_flags, training) calls
// the generic lambda with one std::bool_constant per flag, so a kernel templated on bools has ONE launch site per variant.
template <typename F>
static inline void igmc_dispatch(F&& f) { f(); }
template <typename F, typename... Rest>
static inline void igmc_dispatch(F&& f, bool v, Rest... rest) {
  if (v) igmc_dispatch([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
  else igmc_dispatch([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}
