// launch.h -- host-side launcher declarations + optional per-kernel HIP-event timing (internal).
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
// scores.hip: the scoring step's tail (k_sse_acc + the outputs / labels filed at their positions) and the extremes of a key array
#define IGMC_SELECT_MAX_GRID 1024
#define IGMC_SELECT_MAX_NUM 64
void igmc_launch_scores_store(const BatchDev& b, const float* out, double* acc, int64_t* ctrl, float* scores, float* labels,
                              int64_t n, int64_t first, int32_t* err, void* stream);
int igmc_select_default_grid(int64_t n);
void igmc_launch_select(const float* keys, int64_t n, int num, int grid, void* scratch, int32_t* idx_low, int32_t* idx_high,
                        float* key_low, float* key_high, int32_t* count, void* stream);
// candidates.hip: the candidate links of a set of users (count, then fill at the offsets of the counts) -- every candidate, or
// (sampled) cut down to k sampled negatives + the must items of every request: ONE kernel template, k_candidates<fill, sampled>
// -- and the `num` first of every segment of a key array in the order (key descending, index ascending)
#define IGMC_CAND_TILE_ITEMS 16384      // items of one LDS bitmap tile of the enumeration (wider graphs: tile after tile)
#define IGMC_SEGSEL_MAX_SPLIT 64        // workgroups per segment at most (64 lists of 64 words are what the merge stages)
struct CandArgs {
  GraphDev g;
  const int32_t* users;
  int nq;
  const uint8_t* item_ok;
  int exclude_seen;
  const int64_t* must_off;      // sampled; null: no request has must items
  const int32_t* must_item;
  int64_t n_must;
  int k;
  uint64_t seed, draw;          // sampled fill
  int64_t* counts;              // count
  const int64_t* off;           // fill
  int32_t* link_u;
  int32_t* link_v;
  uint8_t* forced;              // sampled fill; may be null
  int64_t capacity;
  int32_t* err;
};
void igmc_launch_candidates(const CandArgs& a, int fill, int sampled, void* stream);
int igmc_segsel_default_split(int ns);
void igmc_launch_select_segments(const float* keys, const int64_t* seg_off, int ns, int num, int k, void* scratch,
                                 int32_t* idx_out, float* key_out, int32_t* count, void* stream);
// holdout.hip: the Given-k split of a set of users -- per user a uniform `kept`-subset of the row stays, the rest is written as
// held-out links in the row's own order (count, then fill at the offsets of the counts): k_holdout<fill>
struct HoldArgs {
  GraphDev g;
  const int32_t* users;
  int nq;
  int64_t keep, hold;
  uint64_t seed, draw;          // fill
  int64_t* counts;              // count
  const int64_t* off;           // fill
  int32_t* link_u;
  int32_t* link_v;
  uint8_t* rating;
  int64_t capacity;
  int32_t* err;
};
void igmc_launch_holdout(const HoldArgs& a, int fill, void* stream);
// pairs.hip: pair training -- one negative per positive link and epoch drawn into a link list of (positive, negative) slots, and
// the pair loss of a batch of such slots with its gradient w.r.t. the outputs
#define IGMC_PAIR_TRIES 256             // hashed candidates tried before the cyclic scan decides (IGMC_PAIR_TRIES: test hook)
struct PairArgs {
  GraphDev g;
  const int32_t* pos_u;
  const int32_t* pos_v;
  int64_t n;
  const uint8_t* item_ok;       // may be null
  uint64_t seed, epoch;
  int tries;
  int32_t* link_u;              // [2n] each
  int32_t* link_v;
  float* link_y;
  int32_t* err;
  const int64_t* sl_off;        // igmc_pair_negatives_shortlist alone: the per-user table, its entries, floor(share * 2^32)
  const int32_t* sl_item;
  int64_t sl_total;
  uint64_t hard_thr;
};
void igmc_launch_pair_negatives(const PairArgs& a, void* stream);
void igmc_launch_pair_negatives_shortlist(const PairArgs& a, void* stream);
void igmc_launch_pair_kind_stats(const float* out, const float* y, int B, double* stats6, void* stream);
void igmc_launch_pair_loss(const float* out, const float* y, int B, float mse_weight, float* gout, double* stats, void* stream);
void igmc_launch_pair_arr(const float* arr_part, float ARR, double* stats, void* stream);
// shortlist.hip: the co-rating shortlist of a set of users (igmc_hip.h states the definition) -- the segments themselves, or
// the places of given items in the full vote order
#define IGMC_SHORT_TILE_ITEMS IGMC_CAND_TILE_ITEMS      // items of the LDS vote table (uint32 each, 64 KB): every bundled dataset
                                                        // and ml_10m (10 677 items) in one tile; wider graphs keep their votes in
                                                        // the workgroup's scratch row
#define IGMC_SHORT_LDS_BYTES (160 * 1024)               // LDS of one workgroup at most (gfx950: 160 KB a CU): w sits in LDS
                                                        // where it fits beside the fixed part and the vote table, else in scratch
#define IGMC_SHORT_MAX_GRID 512                         // workgroups (and scratch rows) where the caller names no grid: 2 a CU
struct ShortArgs {
  GraphDev g;
  const int32_t* users;
  int nq;
  const uint8_t* item_ok;
  int exclude_seen;
  int seed_min_rel, vote_min_rel;
  int64_t m;                    // fill
  const int64_t* off;
  int32_t* link_u;
  int32_t* link_v;
  uint32_t* votes_out;          // may be null
  int64_t capacity;
  const int64_t* q_off;         // places
  const int32_t* q_id;
  int64_t n_query;
  int32_t* q_place;
  uint32_t* q_votes;            // may be null
  int32_t* err;
  uint32_t* scratch;            // [grid] rows of row_words: w (n_users words, where not in LDS), then the votes (n_items words,
  int64_t row_words;            // where the graph is wider than the LDS vote table)
};
struct ShortPlan {
  int grid, w_lds, v_lds;       // workgroups; w / the vote table in LDS
  int lds_bytes;                // dynamic LDS of the launch
  int64_t row_words, scratch_bytes;
  int w_lds_max_users;          // the most users whose w fits LDS for this graph's item count
};
void igmc_shortlist_plan(int n_users, int n_items, int nq, int grid, ShortPlan* p);
int igmc_shortlist_prepare();
void igmc_launch_shortlist(const ShortArgs& a, const ShortPlan& p, int places, void* stream);
// ranking.hip: the position and the 0-based place (the order of igmc_launch_select_segments) of given ids in their segments,
// and the per-segment sums of the ranking metrics over those places
#define IGMC_RANK_MAX_KS 8              // cut-offs K of one metrics launch at most
void igmc_launch_rank_segments(const float* keys, const int32_t* ids, int64_t n, const int64_t* seg_off, int ns,
                               const int64_t* q_off, const int32_t* q_id, int64_t nq, int k, int32_t* q_pos, int32_t* q_rank,
                               int32_t* err, void* stream);
void igmc_launch_rank_metrics(const int32_t* q_rank, const int64_t* q_off, const uint8_t* q_rel, const int32_t* ks, int nk,
                              int ns, int64_t nq, int grid, int32_t* cnt, double* dcg, int32_t* err, void* stream);
// graph_update.hip: rating changes applied to a resident graph -- one orientation at a time (side 0: rows are users, side 1:
// rows are items).  plan: the sorted change list, the new row lengths, their prefix sums, nnz and the longest row; write: the
// rows of the new graph, once the caller has read nnz and allocated them.
struct GuStats {
  int32_t err;              // bit 0: a user id out of range, bit 1: an item id out of range, bit 2: nnz does not fit int32
  int32_t max_deg[2];
  int32_t max_rel;
  long long nnz[2];
};
struct GuSide {
  const int32_t* optr;      // the old graph's arrays of this orientation
  const int32_t* oidx;
  const uint8_t* orel;
  int rows_old, rows_new;
  unsigned long long* keys; // [padded n] sorted (row << 32 | col) words
  uint32_t* idx;            // [padded n] their list positions
  int16_t* s_new;           // [n] -1: overridden, 0: the winner removes, else the winner's rating
  int16_t* s_old;           // [n] a winner's relation in the old row, or -1
  uint8_t* touched;         // [rows_new] the row has changes in the list
  int32_t* nptr;            // the new graph's arrays
  int32_t* nidx;
  uint8_t* nrel;
};
int64_t igmc_graph_update_padded(int64_t n);
void igmc_launch_graph_update_plan(const GuSide& s, int side, const int32_t* user, const int32_t* item, const uint8_t* rating,
                                   int64_t n, int n_users, int n_items, GuStats* st, void* stream);
void igmc_launch_graph_update_write(const GuSide& s, int side, int64_t n, int64_t nnz_old, GuStats* st, void* stream);
// explain.hip: leave-one-out variants of the links of an extracted arena written into a node-set cache (count, then fill at
// the offsets of the counts), and the variant scores turned into per-link attribution segments
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
void igmc_launch_loo_count(const BatchDev& b, int B, int64_t* nvar, int64_t* nu_ids, int64_t* nv_ids, void* stream);
int igmc_loo_default_chunks();
void igmc_launch_loo_fill(const GraphDev& g, const BatchDev& b, int B, int64_t link0, const LooCache& c, int chunks, int32_t* err,
                          void* stream);
void igmc_launch_loo_deltas(const float* scores, const int64_t* var_off, int64_t n_links, float* base, float* delta, float* key,
                            const int64_t* seg_off, void* stream);
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
