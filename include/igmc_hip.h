/* igmc_hip.h -- C ABI of libigmc_hip.so, the MI355X (gfx950) engine behind the IGMC hot path.
 *
 * The reference (muhanzhang/IGMC) has no FFI layer: its boundary is a Python call
 * surface.  Every entry point below therefore cites the reference Python
 * function(s) it replaces; the Python mirror in igmc_amd/{util_functions,models,
 * train_eval}.py binds them with ctypes (see INTEGRATION.md for the stub).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; the message is
 *     available from igmc_last_error() (thread-local).
 *   - "d_" arguments are DEVICE pointers (HBM), "h_" arguments are HOST pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls
 *     are asynchronous on that stream unless documented otherwise.
 *   - handles own their HBM; borrowed buffers (parameters, gradients, outputs)
 *     stay owned by the caller.
 *   - no torch types anywhere in this interface.
 */
#ifndef IGMC_HIP_H
#define IGMC_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct igmc_graph igmc_graph;   /* bipartite rating graph (CSR + CSC) resident in HBM */
typedef struct igmc_batch igmc_batch;   /* one extracted + collated batch of enclosing subgraphs */
typedef struct igmc_model igmc_model;   /* model geometry + activation / gradient workspace */

#define IGMC_HIDDEN 32        /* latent_dim = [32,32,32,32]  (reference Main.py:391) */
#define IGMC_NUM_LAYERS 4
#define IGMC_LIN1_OUT 128     /* reference models.py:25 */

const char* igmc_last_error(void);
int igmc_version(void);

/* ------------------------------------------------------------------ rating graph
 * Replaces SparseRowIndexer / SparseColIndexer construction
 * (reference util_functions.py:20-66, built in MyDataset/MyDynamicDataset.__init__
 * :72-73, :116-117).  Input = scipy CSR of the training rating matrix whose stored
 * values are rating-label + 1 (reference preprocessing.py:190-197); `h_rating`
 * holds label+1 as uint8 (1..R).  Rows are re-sorted by (relation, id) on the host
 * and both orientations are uploaded once. Synchronous. */
int igmc_graph_create(int n_users, int n_items, int64_t nnz,
                      const int32_t* h_indptr, const int32_t* h_indices, const uint8_t* h_rating,
                      int device, igmc_graph** out);
void igmc_graph_destroy(igmc_graph* g);
int64_t igmc_graph_hbm_bytes(const igmc_graph* g);

/* ------------------------------------------------------------------ batch arena
 * Capacity is fixed at creation from (max_graphs, hop, max_nodes_per_hop) and the
 * graph's sizes; nothing is allocated per step. */
int igmc_batch_create(const igmc_graph* g, int max_graphs, int hop, int max_nodes_per_hop,
                      igmc_batch** out);
void igmc_batch_destroy(igmc_batch* b);

/* Enclosing-subgraph extraction + labelling + collation for B links.
 * Replaces MyDynamicDataset.get -> subgraph_extraction_labeling + construct_pyg_graph
 * (reference util_functions.py:138-145, :208-297) and the PyG DataLoader collate
 * (reference train_eval.py:44-51) for a whole batch, in HBM.
 *   d_link_u/d_link_v/d_link_y : dataset-wide link arrays (user id, item id, rating VALUE
 *                                class_values[label], reference :247)
 *   d_link_idx                 : permutation of dataset positions; the batch is
 *                                d_link_idx[first .. first+B-1]  (NULL = identity)
 *   sample_ratio, max_nodes_per_hop(from create), hop : reference :222-229
 *   seed, epoch                : counter-based sampler key (seed, epoch, link position, hop, side);
 *                                a static dataset (MyDataset) passes a constant epoch.
 */
int igmc_extract_batch(const igmc_graph* g, igmc_batch* b,
                       const int32_t* d_link_u, const int32_t* d_link_v, const float* d_link_y,
                       const int32_t* d_link_idx, int first, int B,
                       double sample_ratio, uint64_t seed, uint64_t epoch, void* stream);

/* Parity mode: node sets are supplied (e.g. by the reference / oracle), only the
 * induced-edge, labelling and collation stages run on the GPU.
 *   h_unodes/h_vnodes : concatenated global ids, target first within each graph
 *   h_udist/h_vdist   : hop distance per node;  h_uoff/h_voff : B+1 offsets.  Synchronous. */
int igmc_extract_batch_replay(const igmc_graph* g, igmc_batch* b, int B,
                              const int32_t* h_unodes, const uint8_t* h_udist, const int32_t* h_uoff,
                              const int32_t* h_vnodes, const uint8_t* h_vdist, const int32_t* h_voff,
                              const float* h_y, void* stream);

/* Static dataset (reference MyDataset + links2subgraphs, util_functions.py:69-110, :148-205: subgraphs extracted once
 * and cached in <root>/processed/data.pt).  The native cache = the node sets of every link with their hop distances,
 * packed in HBM: d_uoff / d_voff [n_links + 1] offsets into d_unodes / d_vnodes (global ids, target first) and d_udist /
 * d_vdist.  The batch d_link_idx[first .. first + B - 1] is rebuilt from it: induced edges, labels and collation run on
 * the GPU as in igmc_extract_batch (asynchronous; honours the control block and the lean mode). */
int igmc_extract_batch_cached(const igmc_graph* g, igmc_batch* b,
                              const int64_t* d_uoff, const int32_t* d_unodes, const uint8_t* d_udist,
                              const int64_t* d_voff, const int32_t* d_vnodes, const uint8_t* d_vdist,
                              const float* d_link_y, const int32_t* d_link_idx, int first, int B, void* stream);

/* A GROUP of batches extracted in one launch per stage (no reference counterpart: the reference extracts subgraph by subgraph
 * in worker processes, util_functions.py:138-145).  Extraction is a dependent chain per link, so its throughput is the number
 * of links in flight: the batches sel0 + 2 i (i = 0 .. count-1; selectors q | (i << 1) of the device-side step control) go
 * into the arenas of `set` with the kernels of igmc_extract_batch launched ONCE over all of them, followed -- drop_p > 0 --
 * by their edge dropout (igmc_batch_edge_dropout with step = the batch's selector).  Every arena of the set must belong to
 * `g`, share one geometry, carry dense induced blocks, be lean (igmc_batch_set_lean), have the same control block attached
 * and no side-feature source or tables; anything else is an error (callers then extract arena by arena). */
typedef struct igmc_batch_set igmc_batch_set;
int igmc_batch_set_create(igmc_batch* const* batches, int count, igmc_batch_set** out);
void igmc_batch_set_destroy(igmc_batch_set* s);
int igmc_extract_group(const igmc_graph* g, igmc_batch_set* s, int count,
                       const int32_t* d_link_u, const int32_t* d_link_v, const float* d_link_y,
                       const int32_t* d_link_idx, int sel0, int B, double sample_ratio, uint64_t seed,
                       float drop_p, int force_undirected, uint64_t drop_seed, void* stream);

/* Edge dropout (reference models.py:193-198 -> PyG dropout_adj): fills the per-entry keep
 * flags (bit0: edge col->row kept, bit1: edge row->col kept) from a counter-based hash of
 * (seed, step, graph, user id, item id, direction).  p = drop probability. */
int igmc_batch_edge_dropout(igmc_batch* b, float p, int force_undirected,
                            uint64_t seed, uint64_t step, void* stream);
/* Parity mode: inject the flags (host array, one byte per CSR entry). Synchronous. */
int igmc_batch_set_edge_flags(igmc_batch* b, const uint8_t* h_flags, int64_t n);
int igmc_batch_clear_edge_flags(igmc_batch* b);   /* no dropout: every edge kept */

/* Batch introspection (synchronises the stream; used by the Python Data view and tests). */
typedef struct igmc_batch_info {
  int32_t num_graphs, num_nodes, num_edges, overflow;
  int32_t node_capacity, edge_capacity, num_labels, hop;
} igmc_batch_info;
int igmc_batch_get_info(const igmc_batch* b, igmc_batch_info* out, void* stream);
/* Copies to host (any pointer may be NULL):
 *  node_off[B+1], n_users[B], node_label[N](u8), node_gid[N], node_graph[N], row_ptr[N+1],
 *  col[E], erel[E](u8), elab[E](u8), eflag[E](u8), y[B] */
int igmc_batch_download(const igmc_batch* b, int32_t* node_off, int32_t* n_users, uint8_t* node_label,
                        int32_t* node_gid, int32_t* node_graph, int32_t* row_ptr, int32_t* col,
                        uint8_t* erel, uint8_t* elab, uint8_t* eflag, float* y, void* stream);
/* Device pointers of the collated batch (for zero-copy views): index by IGMC_BUF_*.  IGMC_BUF_SIDE: the [B, n_side] fp32 side
 * features the next forward reads (the arena's gathered rows, or the pointer handed to igmc_batch_set_side_features; NULL:
 * none). */
enum { IGMC_BUF_NODE_OFF = 0, IGMC_BUF_N_USERS, IGMC_BUF_NODE_LABEL, IGMC_BUF_NODE_GID,
       IGMC_BUF_NODE_GRAPH, IGMC_BUF_ROW_PTR, IGMC_BUF_ECR, IGMC_BUF_ECODE,
       IGMC_BUF_EFLAG, IGMC_BUF_Y, IGMC_BUF_TOTALS, IGMC_BUF_SIDE, IGMC_BUF_COUNT };
void* igmc_batch_device_ptr(const igmc_batch* b, int which);
/* Optional side features of the two target nodes (reference util_functions.py:250-253,
 * models.py:208-209): d_feat[B, n_side] fp32, borrowed for the next forward. */
int igmc_batch_set_side_features(igmc_batch* b, const float* d_feat, int n_side);
/* The same, resolved on the device: d_side_all[n_links, n_side] holds, for EVERY link of the dataset, the feature
 * rows of its two target nodes ([u_features[link_u] | v_features[link_v]], reference MyDynamicDataset.get ->
 * util_functions.py:272-275); every following igmc_extract_batch on this arena gathers the rows of the batch's
 * links (same d_link_idx / first / control-block indexing as the extraction) into an arena-owned buffer that the
 * model then reads -- nothing happens on the host per step, so the step stays hipGraph-capturable.  NULL unbinds. */
int igmc_batch_bind_side_source(igmc_batch* b, const float* d_side_all, int n_side);
/* The same, keyed by NODE (no reference counterpart: the reference indexes u_features / v_features by the target ids on the
 * host, util_functions.py:250-253): d_u_feat[n_u_rows, fu] and d_v_feat[n_v_rows, fv], fp32 row-major, borrowed, hold one row
 * per user / item.  Every following igmc_extract_batch / igmc_extract_batch_cached on this arena writes, behind its own launches
 * on the same stream, row g < B of the arena-owned buffer = [d_u_feat[tu] | d_v_feat[tv]] with tu / tv the target user / item
 * the extraction left in slot g -- no link array, permutation or control-block cursor is read, so the launch is the same for
 * free-running extraction, cached node sets and a hipGraph replay, and serves links that are no dataset's own (candidate
 * lists, leave-one-out variants).  A target id at or beyond its table's row count reads zeros (a node the graph gained after
 * the tables were built); nothing is read outside the tables or written at or beyond row B.  fu, fv >= 0, fu + fv >= 1
 * (n_side becomes fu + fv); a NULL table with a non-zero width is an error; both NULL with zero widths unbinds.  Tables, a
 * side source and igmc_batch_set_side_features replace one another: the last call holds.  igmc_extract_group refuses an
 * arena with tables as it refuses one with a source. */
int igmc_batch_bind_side_tables(igmc_batch* b, const float* d_u_feat, int n_u_rows, int fu, const float* d_v_feat, int n_v_rows,
                                int fv);
/* Lean extraction (arenas with a per-hop cap only; ignored otherwise): igmc_extract_batch stops after the node sets,
 * labels, ratings and the dense induced blocks -- everything the matrix-core subgraph kernel reads -- and the collated
 * CSR (reference construct_pyg_graph + Batch.from_data_list, util_functions.py:280-297) is emitted on demand by the
 * calls that need it (get_info / download / edge flags / model calls that run the per-layer kernels).  The training
 * loop sets it when igmc_model_dense_path() says the model will take the dense path for this arena and batch size. */
int igmc_batch_set_lean(igmc_batch* b, int lean);
/* The arena holds a batch of B subgraphs that a REPLAYED launch extracted (a captured igmc_extract_batch / igmc_extract_group
 * leaves no host-side trace when its hipGraph is replayed): the model calls take the batch size of an arena from its last
 * extraction call on the host, which may be an older one with another size (the ragged last batch of an epoch).  Callers
 * that consume a prefetched arena outside the graph that filled it say so here.  No reference counterpart. */
int igmc_batch_assume_size(igmc_batch* b, int B);
/* Keep the transposed copy of the dense induced blocks too (arenas get one by themselves when a side exceeds 128 nodes):
 * the item-side operand of the dense-layer kernels, for models the subgraph kernel does not take although the blocks exist
 * (sort-pool readout, side features) -- their conv layers then run on the matrix cores instead of walking CSR rows.
 * No-op without dense blocks; a batch already in the arena is dropped (extract again).  No reference counterpart. */
int igmc_batch_want_transposed(igmc_batch* b);

/* ------------------------------------------------------------------ model
 * Flat fp32 parameter buffer layout (offsets in floats; query with igmc_param_offset):
 *   for l in 0..3:  conv{l}.basis [Bs, Fin_l, 32]   conv{l}.root [Fin_l, 32]
 *                   conv{l}.bias [32]               conv{l}.att [R, Bs]
 *   lin1.weight [128, 256+n_side]  lin1.bias [128]  lin2.weight [1,128]  lin2.bias [1]
 * with Fin_0 = 2*hop+2, Fin_l = 32.  Shapes = PyG-1.4.2 RGCNConv / torch.nn.Linear, i.e. the
 * reference state_dict keys convs.{l}.{basis,att,root,bias}, lin1.*, lin2.* (Main.py:36-45). */
enum { IGMC_P_BASIS = 0, IGMC_P_ROOT, IGMC_P_BIAS, IGMC_P_ATT,
       IGMC_P_LIN1_W, IGMC_P_LIN1_B, IGMC_P_LIN2_W, IGMC_P_LIN2_B };
int igmc_model_create(int device, int num_relations, int num_bases, int num_labels /*2*hop+2*/,
                      int n_side_features, int max_nodes, int max_edges, int max_graphs,
                      igmc_model** out);
void igmc_model_destroy(igmc_model* m);
int64_t igmc_param_count(const igmc_model* m);
/* offset (floats) and element count of a tensor; layer is ignored for lin1/lin2. */
int64_t igmc_param_offset(const igmc_model* m, int layer, int which, int64_t* count);

/* IGMC.forward (reference models.py:190-217): 4x (RGCNConv + tanh), centre-node readout,
 * lin1+ReLU+dropout(0.5)+lin2, * multiply_by.  Writes d_out[B].
 *   training      : 0 = eval (no dropout), 1 = train
 *   d_lin_mask    : optional injected keep-mask for the 0.5 dropout, uint8 [B,128] (parity);
 *                   NULL = draw from the counter-based hash (seed, step)
 *   use_edge_flags: 1 = honour the batch's edge keep flags (training with adj_dropout>0) */
int igmc_model_forward(igmc_model* m, const float* d_params, const igmc_batch* b,
                       int training, int use_edge_flags, const uint8_t* d_lin_mask,
                       uint64_t seed, uint64_t step, float multiply_by,
                       float* d_out, void* stream);
/* Backward of the last igmc_model_forward(training=1) given d_gout[B] = dLoss/d_out.
 * Accumulates nothing: d_grad (flat, same layout as params) is overwritten. */
int igmc_model_backward(igmc_model* m, const float* d_params, const igmc_batch* b,
                        const float* d_gout, float multiply_by, float* d_grad, void* stream);

/* One optimisation step's loss + gradient (reference train_eval.py:158-175):
 * (d_loss may be NULL when igmc_step_finish will produce it.)
 * forward, loss = mse_loss(out, y) (mean over the B graphs * loss_scale) + ARR * sum_l sum_r
 * ||W_l[r+1]-W_l[r]||^2, backward.  d_loss[0] = loss, d_loss[1] = sum of squared errors.
 * `grad_scale` multiplies the data-term gradient (1/B for the reference; 1/(global B) under
 * data parallelism, where `arr_scale` = 1/world_size keeps the all-reduced ARR term exact). */
int igmc_model_loss_grad(igmc_model* m, const float* d_params, const igmc_batch* b,
                         int use_edge_flags, const uint8_t* d_lin_mask, uint64_t seed, uint64_t step,
                         float multiply_by, float ARR, float grad_scale, float arr_scale,
                         float* d_out, float* d_grad, float* d_loss, void* stream);

/* Fused Adam over the flat buffer (reference train_eval.py:54,177: torch.optim.Adam,
 * betas (0.9,0.999), eps 1e-8, weight_decay added to the gradient).  `step` is 1-based. */
int igmc_adam_step(float* d_params, const float* d_grad, float* d_exp_avg, float* d_exp_avg_sq,
                   int64_t n, int64_t step, float lr, float beta1, float beta2, float eps,
                   float weight_decay, void* stream);

/* ------------------------------------------------------------------ device-side step control
 * A hipGraph replay cannot change kernel arguments, so the per-step scalars live in HBM instead:
 * d_ctrl is an int64[IGMC_CTRL_WORDS] device buffer (slots 8..14 hold doubles, bit-cast):
 *   [0] step   [1] cursor_0   [2] epoch   [3] adam_t   [4] batch size B   [5] internal arrival counter (keep 0)
 *   [6] cursor_1   [7] k = steps done in this epoch
 *   [8] lr  [9] beta1  [10] beta2  [11] eps  [12] weight_decay   [13] lr/(1-beta1^t)  [14] 1/sqrt(1-beta2^t)
 *   [15] M = steps per GROUP (0 is read as 1)   [16] gk = steps done in the current group   [17] gq = parity of the
 *   current group   [18] sync_err (bit 1: a step consumed an arena whose stamp is not the batch of its cursor; bit 2:
 *   ... whose edge-dropout key is not that batch's)
 * Steps run in GROUPS of M: the batches of a group sit in M arenas (one set per group parity), extracted while the
 * previous group trained.  cursor_q = offset into the link permutation of the FIRST batch of the group of parity q; batch i
 * of that group starts at cursor_q + i * B.  A tick (end of a step, igmc_ctrl_tick or the step's last kernel) does
 * step += 1, k += 1, adam_t += 1, slots 13/14 recomputed, gk += 1 and -- when gk reaches M -- cursor_gq += 2 * M * B,
 * gk = 0, gq ^= 1: the cursor a concurrent prefetch of the NEXT group reads (cursor_{1-gq}) is never written while it may
 * be read.  M = 1 is the plain even / odd double buffer.
 * Once attached (igmc_batch_set_ctrl), the host `first` of igmc_extract_batch / igmc_extract_batch_cached and the host
 * `step` of igmc_batch_edge_dropout become a SELECTOR sel = q | (i << 1): first = cursor_q + i * B, epoch = ctrl.epoch,
 * dropout key = (epoch, first / B); the forward's MLP dropout uses ctrl.step.  Every extraction stamps its arena with the
 * `first` (and every edge dropout with the key) it resolved; the tick of the step that consumed the arena compares the
 * stamp with cursor_gq + gk * B and raises sync_err on a mismatch (igmc_model_check reports it).  NULL detaches. */
enum { IGMC_CTRL_STEP = 0, IGMC_CTRL_FIRST = 1, IGMC_CTRL_EPOCH = 2, IGMC_CTRL_ADAM_T = 3, IGMC_CTRL_BATCH = 4,
       IGMC_CTRL_DONE = 5, IGMC_CTRL_FIRST_ODD = 6, IGMC_CTRL_K = 7,
       IGMC_CTRL_LR = 8, IGMC_CTRL_BETA1 = 9, IGMC_CTRL_BETA2 = 10, IGMC_CTRL_EPS = 11, IGMC_CTRL_WD = 12,
       IGMC_CTRL_STEP_SIZE = 13, IGMC_CTRL_INV_SQRT_BC2 = 14, IGMC_CTRL_GROUP = 15, IGMC_CTRL_GK = 16,
       IGMC_CTRL_GQ = 17, IGMC_CTRL_SYNC_ERR = 18, IGMC_CTRL_GATE_TIMEOUTS = 19, IGMC_CTRL_WORDS = 24 };
int igmc_ctrl_tick(int64_t* d_ctrl, void* stream);
/* Starts a new group at the current position (no reference counterpart): M steps per group, gk = 0, gq = 0,
 * cursor_0 = first_cur (the batch of the next step), cursor_1 = first_next (first batch of the group after it). */
int igmc_ctrl_regroup(int64_t* d_ctrl, int M, int64_t first_cur, int64_t first_next, void* stream);
/* Pacing gate for work on ANOTHER stream (no reference counterpart): a one-wave kernel on `stream` that ends once gk_min
 * steps of the running group of parity q are done (ctrl.gk >= gk_min), or that group is over (ctrl.gq != q), or timeout_us
 * microseconds have passed -- whichever comes first; when it had to wait for the step counter (or delay_always != 0) it ends
 * delay_us (<= 1000) later, so that the step which has just begun has its workgroups on the chip before whatever is queued
 * behind the gate on `stream` (the extraction of the next group's batches) starts beside it: an extraction launch dispatched
 * TOGETHER with the subgraph kernel costs that step ~14 us, one dispatched 10 us behind it ~3 (profiles/r05_experiments).
 * No graph edge leaves the step chain.  A hint, not a dependency: the work behind the gate must be correct whenever it runs.
 * A gate that gives up counts itself in ctrl[IGMC_CTRL_GATE_TIMEOUTS]: where the two streams are not served concurrently (a
 * profiler or AMD_SERIALIZE_KERNEL serialising dispatches, both streams on one hardware queue) every gate would cost its
 * timeout -- the caller reads the counter and goes back to pacing by graph edges (StepGraph.check). */
int igmc_ctrl_gate(int64_t* d_ctrl, int q, int gk_min, double delay_us, int delay_always, double timeout_us, void* stream);
int igmc_batch_set_ctrl(igmc_batch* b, const int64_t* d_ctrl);
int igmc_model_set_ctrl(igmc_model* m, const int64_t* d_ctrl);
/* Adam + loss/epoch-total epilogue in ONE launch (the step's last kernel): updates d_params like
 * igmc_adam_step, writes d_loss[0..1] like igmc_model_loss_grad (call that one with d_loss = NULL), adds
 * loss*num_graphs to d_total[0] (reference train_eval.py:176), and -- when d_ctrl is given -- takes the Adam
 * scalars from the control block and ADVANCES it for the next step (the tick rides in this kernel). */
int igmc_step_finish(igmc_model* m, const igmc_batch* b, float* d_params, const float* d_grad,
                     float* d_exp_avg, float* d_exp_avg_sq, float ARR, float* d_loss, double* d_total,
                     int64_t* d_ctrl, int64_t step, float lr, float beta1, float beta2, float eps,
                     float weight_decay, void* stream);
/* The whole single-GPU optimisation step on an extracted batch (reference train_eval.py:158-177: forward, loss,
 * backward, optimizer.step) in the minimum number of launches: the last kernel applies Adam to the parameters
 * whose gradients it finalises, emits d_loss[0..1], adds loss*num_graphs to d_total[0] and (with d_ctrl) advances
 * the control block.  grad_scale = 1/B.  Data-parallel runs use igmc_model_loss_grad + all-reduce +
 * igmc_step_finish instead. */
int igmc_train_step(igmc_model* m, float* d_params, const igmc_batch* b, int use_edge_flags,
                    const uint8_t* d_lin_mask, uint64_t seed, uint64_t step, float multiply_by, float ARR,
                    float* d_out, float* d_grad, float* d_exp_avg, float* d_exp_avg_sq, float* d_loss,
                    double* d_total, int64_t* d_ctrl, int64_t adam_t, float lr, float beta1, float beta2,
                    float eps, float weight_decay, void* stream);

/* Weight images.  The subgraph kernel and the dense per-layer kernels read each conv layer's weights as staged images
 * (W_r = sum_b att[r,b] basis_b per relation, split into bf16 terms in MFMA fragment order; the layer-0 table), composed
 * from d_params by a small kernel at the start of every forward / step.  igmc_train_step[_dp]'s last kernel (gradient +
 * Adam) ALSO writes the images of the parameters it has just updated, and an evaluation leaves the images of its
 * parameters behind -- so a caller that knows d_params has not been touched since the PREVIOUS call on this model (the
 * next step of a training loop, the next batch of an evaluation) says so, and that call starts with the subgraph kernel:
 * one launch less per step.  One-shot: applies to the next igmc_model_forward / igmc_model_loss_grad / igmc_train_step /
 * igmc_train_step_dp on `m` only, and only if the library itself left the images of the same d_params pointer behind
 * (else it composes as usual).  Never assert it after changing the parameters by other means (igmc_adam_step, a
 * checkpoint load, a broadcast).  Reference: there is none -- PyG's RGCNConv forms W_r on every forward (models.py:200). */
int igmc_model_weights_unchanged(igmc_model* m, int on);
int igmc_adam_step_ctrl(float* d_params, const float* d_grad, float* d_exp_avg, float* d_exp_avg_sq,
                        int64_t n, const int64_t* d_ctrl, void* stream);

/* ------------------------------------------------------------------ gradient exchange (data parallelism)
 * The reference has no distributed code (single process, single device: train_eval.py:20); the hot path shards by LINKS
 * (SURVEY.md 8(e)): one process per GPU, graph + parameters replicated, and the only exchange of a step is ONE sum
 * all-reduce of the flat gradient buffer (49 233 floats at R = 5) between the gradient kernels and the Adam kernel.
 * It is an RCCL ncclAllReduce enqueued on the caller's stream -- capturable into the step's hipGraph like any kernel --
 * on a communicator owned by this library (RCCL is resolved with dlopen("librccl.so.1") at the first use: a process
 * that never creates a communicator never loads it).
 *   igmc_comm_unique_id : rank 0 draws the 128-byte RCCL id; the caller hands it to the other ranks (any transport)
 *   igmc_comm_create    : collective over the `world` ranks; `device` = this rank's GPU.  world == 1 is valid.
 *   igmc_comm_info      : rank / size AS SEEN BY RCCL (bench.py checks them against the launcher's)
 *   igmc_allreduce_grads: d_flat_grad[i] = scale * sum over ranks of d_flat_grad[i], in place, asynchronous on `stream`.
 *                         The gradient kernels already scale by 1/(B * world) (igmc_model_loss_grad), so scale = 1.
 *   igmc_comm_create_host: a communicator whose sum is the CALLER's: fn(user, d_buf, n, stream) must leave the sum over the
 *                         `world` ranks in d_buf (in place, ordered on `stream`), return 0 on success.  For a host that already
 *                         owns a process group (torch.distributed, MPI): the library's steps then run on it unchanged.
 *   igmc_train_step_dp  : igmc_train_step of a data-parallel job, the exchange INSIDE the step: the step's reduced gradient
 *                         sources (the subgraph kernel's relation-space tables, or the per-layer path's basis-space sums, plus
 *                         the lin1 / lin2 gradients: about the size of the flat gradient) are summed over the ranks between
 *                         their reduction and the gradient / Adam kernel, as ONE grouped collective -- the kernels of the
 *                         single-GPU step and nothing else; arenas whose step keeps no such form (generic sequence) form the
 *                         flat gradient, all-reduce it and run the Adam kernel.  Loss terms are scaled by 1/(B * world), the
 *                         ARR term is added by every rank after the exchange.  comm == NULL: one rank (= igmc_train_step).
 *                         d_loss / d_total stay per rank (this rank's batches), as in igmc_train_step.
 *   igmc_comm_peer_alloc / igmc_comm_peer_connect: a communicator whose sum is a ONE-SHOT all-reduce over peer-mapped
 *                         buffers (the ranks of ONE node): every rank publishes its span into its own device buffer as
 *                         {value, tag} words and reads every rank's words in rank order -- one launch, about one xGMI round
 *                         trip, bit-identical replicas, capturable.  _alloc creates the rank's buffer (slots of `max_floats`)
 *                         and returns its 64-byte IPC handle; the caller hands the handles of all ranks (world x 64 bytes,
 *                         rank order, any transport) to _connect.  Used like any other communicator afterwards.
 *                         A one-rank peer communicator launches nothing (the spans are the sums).  The polls are bounded by
 *                         WALL-CLOCK time (IGMC_PEER_TIMEOUT_S, default 60 s): a word that never arrives raises a sticky
 *                         device word -- the spans of that launch are then PARTLY summed (elements finished before the
 *                         time-out hold sums, the others their local values; never a foreign or torn value) and must not be
 *                         used -- and the gradient / Adam kernel of igmc_train_step_dp behind the exchange touches no
 *                         parameter, moment or step counter.  After a bare igmc_allreduce_grads call igmc_comm_check.
 *   igmc_comm_check     : synchronises `stream`; fails -- once -- if a rank's words did not arrive in time in a peer exchange
 *                         since the last check; igmc_comm_kind: 0 one rank, 1 RCCL, 2 host callback, 3 peer-mapped buffers (4: in fine-grained memory).
 */
typedef struct igmc_comm igmc_comm;
typedef int (*igmc_allreduce_fn)(void* user, float* d_buf, int64_t n, void* stream);
int igmc_comm_unique_id(uint8_t* h_id128);
int igmc_comm_create(const uint8_t* h_id128, int rank, int world, int device, igmc_comm** out);
int igmc_comm_create_host(igmc_allreduce_fn fn, void* user, int rank, int world, igmc_comm** out);
int igmc_comm_peer_alloc(int rank, int world, int device, int64_t max_floats, igmc_comm** out, uint8_t* h_handle64);
int igmc_comm_peer_connect(igmc_comm* c, const uint8_t* h_handles);
int igmc_comm_check(igmc_comm* c, void* stream);
int igmc_comm_kind(const igmc_comm* c);
void igmc_comm_destroy(igmc_comm* c);
int igmc_comm_info(const igmc_comm* c, int* rank, int* world);
int igmc_allreduce_grads(igmc_comm* c, float* d_flat_grad, int64_t n, float scale, void* stream);
int igmc_train_step_dp(igmc_model* m, igmc_comm* comm, float* d_params, const igmc_batch* b, int use_edge_flags,
                       const uint8_t* d_lin_mask, uint64_t seed, uint64_t step, float multiply_by, float ARR, float* d_out,
                       float* d_grad, float* d_exp_avg, float* d_exp_avg_sq, float* d_loss, double* d_total,
                       int64_t* d_ctrl, int64_t adam_t, float lr, float beta1, float beta2, float eps, float weight_decay,
                       void* stream);

/* Eval reduction helper (reference train_eval.py:195): d_acc[0] += sum_g (out-y)^2, d_acc[1] += B. */
int igmc_sse_accumulate(const float* d_out, const igmc_batch* b, double* d_acc, void* stream);
/* ... and, in the same launch, the tick that ends an evaluation step of the grouped pipeline (igmc_ctrl_tick): an evaluation step
 * is then the forward launch + this one. */
int igmc_sse_accumulate_tick(const float* d_out, const igmc_batch* b, double* d_acc, int64_t* d_ctrl, void* stream);

/* ---- Scores kept on the device, and their extremes (reference train_eval.py:248-272: `visualize` scores every link of a
 * dataset batch by batch, argsorts the scores -- or the labels -- and takes `num` links at both ends).
 *
 * igmc_scores_store is the tail of a SCORING step and replaces `R.extend(r.view(-1).tolist()); Y.extend(y.view(-1).tolist())`
 * (train_eval.py:255-261) without the two host round trips per batch: igmc_sse_accumulate(_tick) -- same launch shape, same
 * summation, same tick where d_ctrl is given, so d_acc is bit-identical to an evaluation pass's -- which also writes
 * d_scores[first + g] = d_out[g] and d_labels[first + g] = y[g] for the batch's graphs g.  `first` is the batch's first
 * position in the pass's link order: first_or_minus1 where it is >= 0 (eager launches), else the position the batch's
 * extraction resolved from the device-side step control and left in its arena (captured / replayed launches: the step
 * control's cursor is known on the device only).  n = capacity of d_scores / d_labels, in [1, 2^31).  A position outside
 * [0, n) is not written and sets d_err[0] (int32, zeroed by the caller before the pass: bit 0 = a batch reached past n,
 * bit 1 = no position given and the arena carries none); the caller reads d_err after the pass -- nothing is truncated
 * silently. */
int igmc_scores_store(const float* d_out, const igmc_batch* b, double* d_acc, float* d_scores, float* d_labels, int64_t n,
                      int64_t first_or_minus1, int64_t* d_ctrl /* may be NULL: no tick */, int32_t* d_err, void* stream);
/* igmc_select_extremes replaces `order = np.argsort(keys)`, `order[:num]`, `order[-num:][::-1]` (train_eval.py:262-272) for
 * n float keys on the device, 1 <= n < 2^31, 1 <= num <= 64.
 * THE ORDER: (key ascending, index ascending); every NaN behind every number (NaNs among themselves by index); -0.0 == 0.0.
 * This is np.argsort(keys, kind='stable').  (The reference calls np.argsort with its default kind, which is not stable: among
 * EQUAL keys its pick is an implementation detail; this one is defined.)
 *   d_idx_low[i]  = order[i]              i < count = min(n, num)      d_key_low[i]  = d_keys[d_idx_low[i]]
 *   d_idx_high[i] = order[n - 1 - i]      (the last `num` of the order, reversed)
 * entries i >= count hold index -1, key 0; d_count[0] = count (d_key_low, d_key_high, d_count may be NULL).
 * The result is a function of the keys alone: it does not depend on `grid`, the number of workgroups of the partial pass
 * (0 = chosen from n; at most 1024).  d_scratch: igmc_select_scratch_bytes(n, num, grid) bytes (-1 on bad arguments), 8-byte
 * aligned, owned by the caller -- nothing is allocated here, the two launches are capturable. */
int64_t igmc_select_scratch_bytes(int64_t n, int num, int grid);
int igmc_select_extremes(const float* d_keys, int64_t n, int num, int32_t* d_idx_low, int32_t* d_idx_high, float* d_key_low,
                         float* d_key_high, int32_t* d_count, void* d_scratch, int64_t scratch_bytes, int grid, void* stream);

/* ---- Rating changes applied to a resident graph (no reference counterpart: the reference rebuilds SparseRowIndexer /
 * SparseColIndexer from scratch, util_functions.py:20-66, and so does igmc_graph_create, through the host).
 *
 * igmc_graph_apply is a FUNCTIONAL update: *out is a new graph, g -- and every arena and captured launch bound to it -- stays
 * valid.  d_user / d_item (int32) / d_rating (uint8) are DEVICE arrays of n >= 0 changes; the result is the matrix after
 * A[d_user[j], d_item[j]] = d_rating[j] for j = 0 .. n-1 IN ORDER: d_rating is rating label + 1 as in igmc_graph_create,
 * 0 removes the entry; of a pair that occurs more than once the last occurrence wins; removing an absent entry and re-writing
 * the present rating change nothing.  n_users_new >= n_users and n_items_new >= n_items: the graph may grow, new rows and
 * columns start empty (n == 0: a copy, possibly grown).  The arrays of *out -- rows by (relation, item), columns by
 * (relation, user) -- and its nnz, max_rel, max_deg_u, max_deg_v are bit for bit those igmc_graph_create builds from the
 * changed matrix, whatever the launch geometry.  Errors (non-zero, igmc_last_error, *out not written, nothing kept): a null
 * argument, a shrinking size, an id outside [0, n_users_new) / [0, n_items_new), n above 2^30, a resulting nnz that does not
 * fit int32.  SYNCHRONOUS like igmc_graph_create (the new nnz sizes the allocation); what crosses to the host is one block of
 * sizes and the error word, twice -- never an array of the graph.  A row's cost is (old length + its changes) x log(its
 * changes) up to 256 changes of one row in one call, (old length + its changes) x its changes beyond.  The library keeps the
 * call's scratch (sorted lists, flags, pointers: ~32 bytes per change, one allocation per device, at most 64 MB) between calls;
 * *out is one allocation of exactly its six arrays.  Calls are serialised by a lock.
 *
 * igmc_graph_info: n_users, n_items, nnz, max_rel, max_deg_u, max_deg_v.  igmc_graph_download: the six arrays to HOST buffers
 * (u_ptr int32[n_users + 1], u_idx int32[nnz], u_rel uint8[nnz], v_* alike); any pointer may be NULL. */
int igmc_graph_apply(const igmc_graph* g, int n_users_new, int n_items_new, const int32_t* d_user, const int32_t* d_item,
                     const uint8_t* d_rating, int64_t n, void* stream, igmc_graph** out);
int igmc_graph_info(const igmc_graph* g, int64_t out6[6]);
int igmc_graph_download(const igmc_graph* g, int32_t* u_ptr, int32_t* u_idx, uint8_t* u_rel, int32_t* v_ptr, int32_t* v_idx,
                        uint8_t* v_rel);

/* ---- Candidate links and the best of every user's segment (no reference counterpart: the reference has no recommendation
 * path; by hand it would be a host loop over the complement of every user's row, an upload of the pairs and a host argsort of
 * the scores pulled back).
 *
 * igmc_candidates_count / igmc_candidates_fill enumerate, for the users d_users[0..nq) IN THE ORDER GIVEN (duplicates allowed:
 * each gets a segment of its own), the items v ascending with d_item_ok[v] != 0 (uint8[n_items]; NULL = every item) and, where
 * exclude_seen != 0, no entry (u, v) in the graph.  _count writes the segments' lengths to d_counts (int64[nq]); the caller
 * turns them into d_offsets (int64[nq + 1], offsets[0] = 0, an inclusive prefix sum behind it) and _fill writes
 * d_link_u[p] = u, d_link_v[p] = v (int32) for the p of [offsets[q], offsets[q + 1]).  capacity = entries of d_link_u /
 * d_link_v, in [1, 2^31): nothing is written at or past it.  d_err[0] (int32, zeroed by the caller, read after the launches):
 * bit 0 = a segment reaches past capacity (its links there are missing), bit 1 = a user id outside [0, n_users) (no row is
 * read; its segment is empty), bit 2 = the offsets are not the prefix sums of the counts.  One launch each, capturable. */
int igmc_candidates_count(const igmc_graph* g, const int32_t* d_users, int nq, const uint8_t* d_item_ok /* may be NULL */,
                          int exclude_seen, int64_t* d_counts, int32_t* d_err, void* stream);
int igmc_candidates_fill(const igmc_graph* g, const int32_t* d_users, int nq, const uint8_t* d_item_ok /* may be NULL */,
                         int exclude_seen, const int64_t* d_offsets, int32_t* d_link_u, int32_t* d_link_v, int64_t capacity,
                         int32_t* d_err, void* stream);
/* igmc_candidates_sample_count / igmc_candidates_sample_fill: the same segments cut down to k SAMPLED negatives (no reference
 * counterpart; the sampled ranking protocol of the top-N literature -- held-out items among k uniformly drawn unseen items).
 * With C(u) = the candidates of igmc_candidates_fill, M(q) = the MUST items d_must_item[d_must_off[q] .. d_must_off[q + 1])
 * of request q (int32[n_must], any order, duplicates allowed; d_must_off int64[nq + 1]; d_must_off == NULL = no must items)
 * and N = C(u) \ M(q), the segment of q is (M(q) n C(u)) u S, item ascending, where S = the min(k, |N|) items of N with the
 * smallest sampling key of igmc_rng.h under that header's negative salt of (seed, draw, u): a uniform subset keyed by the user
 * ID, so it does not depend on the users asked for with it or on the launch.  A must item that is no candidate is not listed.
 * 0 <= k < 2^31, 0 <= n_must < 2^31; k >= |N| writes all of C(u) (with no must items: the bytes of igmc_candidates_fill),
 * k = 0 the must items only.  _count writes |M n C| + min(k, |N|) (it needs no seed); _fill also writes d_forced[p] (uint8,
 * may be NULL) = 1 where the item at p is a must item, 0 where it was drawn.  d_err: bits 0 / 1 / 2 as above; bit 3 = a must
 * item outside [0, n_items) (ignored); bit 4 = d_must_off[q] > d_must_off[q + 1] or outside [0, n_must] (that request's must
 * list is treated as empty; nothing is read out of range).  One launch each, capturable. */
int igmc_candidates_sample_count(const igmc_graph* g, const int32_t* d_users, int nq, const uint8_t* d_item_ok /* may be NULL */,
                                 int exclude_seen, const int64_t* d_must_off /* may be NULL */, const int32_t* d_must_item,
                                 int64_t n_must, int64_t k, int64_t* d_counts, int32_t* d_err, void* stream);
int igmc_candidates_sample_fill(const igmc_graph* g, const int32_t* d_users, int nq, const uint8_t* d_item_ok /* may be NULL */,
                                int exclude_seen, const int64_t* d_must_off /* may be NULL */, const int32_t* d_must_item,
                                int64_t n_must, int64_t k, uint64_t seed, uint64_t draw, const int64_t* d_offsets,
                                int32_t* d_link_u, int32_t* d_link_v, uint8_t* d_forced /* may be NULL */, int64_t capacity,
                                int32_t* d_err, void* stream);
/* ---- The Given-k split: hold ratings out on the device (no reference counterpart: the reference evaluates one fixed split by
 * RMSE; the Given-N protocol of the collaborative-filtering literature is, by hand, a host loop over every user's row, a host
 * RNG and a rebuilt matrix per level).
 *
 * For request q of user u = d_users[q] (IN THE ORDER GIVEN), whose row has d entries:
 *   held = min(hold, max(0, d - keep)),  kept = d - held            keep >= 0, hold >= 0; hold = INT64_MAX: no limit
 *   the kept entries are the `kept` entries of the row with the smallest sampling key of igmc_rng.h under that header's holdout
 *   salt of (seed, draw, u) -- a uniform subset keyed by the user ID (the key is a bijection of the item id: no ties), so it
 *   does not depend on the users asked for with it, on their order or on the launch;
 *   the segment of q is the OTHER entries in the row's own order -- relation ascending, then item ascending, as the CSR stores
 *   them --: d_link_u[p] = u, d_link_v[p] = item (int32), d_rating[p] = relation + 1 (uint8, the convention of
 *   igmc_graph_create and igmc_graph_apply: the list with its ratings zeroed is the removal list of igmc_graph_apply).
 * Consequences: at hold = INT64_MAX the kept sets are NESTED in keep, kept(k) c kept(k + 1) for the same (seed, draw, u); a user
 * with d <= keep loses nothing; keep = 1, hold = 1 is leave-one-out and never strips a user bare.
 * _count writes the segments' lengths to d_counts (int64[nq]; it reads the row pointers only and needs no seed); the caller
 * forms d_offsets (int64[nq + 1], offsets[0] = 0, their inclusive prefix sums behind it) and _fill writes the segments.
 * capacity = entries of d_link_u / d_link_v / d_rating (>= 0): nothing is written at or past it.  d_err[0] (int32, zeroed by
 * the caller, read after the launches): bit 0 = a segment reaches past capacity (its links there are missing), bit 1 = a user id
 * outside [0, n_users) (no row is read; its segment is empty), bit 2 = the offsets are not the prefix sums of the counts.
 * Refused (non-zero, nothing launched): a null argument, nq < 0, keep < 0, hold < 0, capacity < 0; nq = 0 launches nothing.
 * One launch each, asynchronous on `stream`, capturable; the output does not depend on the launch geometry. */
int igmc_holdout_count(const igmc_graph* g, const int32_t* d_users, int nq, int64_t keep, int64_t hold, int64_t* d_counts,
                       int32_t* d_err, void* stream);
int igmc_holdout_fill(const igmc_graph* g, const int32_t* d_users, int nq, int64_t keep, int64_t hold, uint64_t seed,
                      uint64_t draw, const int64_t* d_offsets, int32_t* d_link_u, int32_t* d_link_v, uint8_t* d_rating,
                      int64_t capacity, int32_t* d_err, void* stream);
/* igmc_select_segments: the `num` first of every segment [d_seg_off[s], d_seg_off[s + 1]) of d_keys, s < ns (no reference
 * counterpart; by hand `np.lexsort` per user on the host), 1 <= num <= 64, d_seg_off[ns] < 2^31.
 * THE ORDER: key DESCENDING, then index ascending; every NaN behind every number (NaNs among themselves by index);
 * -0.0 == 0.0.  Per segment that is the three-key np.lexsort((idx, np.where(np.isnan(k), 0, -k), np.isnan(k))): the NaNs are
 * set behind the numbers by a key of their own.  (The two-key np.lexsort((idx, np.where(np.isnan(k), np.inf, -k))) maps -inf
 * and NaN to the same value and orders the two among themselves by index: it is THE ORDER only for segments without a -inf
 * key.)  It is NOT the reverse of igmc_select_extremes' order: among equal keys the LOWER index comes first here (of two items predicted alike the lower id
 * ranks first), where the "highest" list of igmc_select_extremes takes the higher index first.
 *   d_idx_out[s * num + r] = position IN d_keys (not in the segment) of the r-th of segment s     r < count_s = min(len_s, num)
 *   d_key_out[s * num + r] = d_keys[that position], its own bits (d_key_out may be NULL)
 * entries r >= count_s hold index -1, key 0; d_count[s] = count_s.
 * geometry: 0 = chosen from ns (one workgroup per segment from 257 segments on; fewer segments are split so that long ones do
 * not sit on one workgroup); k in [1, 64] = k workgroups per segment and a merge.  The result is a function of the keys and
 * the offsets alone, whatever the geometry.  d_scratch: igmc_select_segments_scratch_bytes(ns, num, geometry) bytes (-1 on bad
 * arguments), 8-byte aligned, owned by the caller; nothing is allocated here, the launches are capturable. */
int64_t igmc_select_segments_scratch_bytes(int ns, int num, int geometry);
int igmc_select_segments(const float* d_keys, const int64_t* d_seg_off, int ns, int num, int32_t* d_idx_out, float* d_key_out,
                         int32_t* d_count, void* d_scratch, int64_t scratch_bytes, int geometry, void* stream);

/* ---- Pair training: a ranking objective on top of a regression checkpoint (no reference counterpart: the reference trains on
 * observed links with MSE alone; by hand this is a host loop drawing an unseen item for every training link plus an autograd
 * loss over the two scores).
 *
 * igmc_pair_negatives draws ONE negative per positive link and epoch.  d_pos_u / d_pos_v (int32[n], 1 <= n < 2^30) are the
 * positives; for positive k = (u, i), with c_t = try t of igmc_rng.h's igmc_pair_candidate under the salt igmc_pair_salt of (seed,
 * epoch, k), an item id in [0, n_items):
 *   the negative j = c_t of the smallest t < T = 256 with no entry (u, c_t) in the graph and d_item_ok[c_t] != 0 (uint8[n_items];
 *   NULL = every item); if none of the T tries qualifies, the first qualifying item of the cyclic order c_0, c_0 + 1, ..,
 *   n_items - 1, 0, .., c_0 - 1; if no item qualifies the pair is VOID.
 * The key is the positive's position k in the list: a link's negative depends neither on a shuffle nor on a batch size.  Left of
 * the try list j is uniform over the qualifying items up to the multiply-shift's bias (n_items / 2^32); the cyclic scan is
 * deterministic and reached with probability (share of non-qualifying items)^T.
 * Written, all arrays [2 n]: d_link_u[2k] = d_link_u[2k+1] = u; d_link_v[2k] = i; d_link_v[2k+1] = j, or i for a void pair (every
 * slot stays an extractable link); d_link_y[2k+1] = 1.0f, or 0.0f for a void pair -- the negative's label slot carries the
 * pair's validity; d_link_y[2k] is NOT written: the caller keeps the positive's rating there.
 * d_err[0] (int32, zeroed by the caller, read after the launch): bit 0 = a user or item id of a positive outside the graph --
 * that pair is void (ids written as given, label 0) and no row is read; bit 1 = at least one pair void for lack of an unseen
 * item.  One wave per positive over a grid-stride loop; one launch, nothing allocated, capturable.
 *
 * igmc_pair_loss_grad is one pair step's loss and gradient on an extracted batch whose EVEN slots are positives and whose ODD
 * slots are their negatives (an odd batch size is refused): exactly igmc_model_forward(training = 1), the pair loss kernel,
 * the backward of igmc_model_backward with the ARR coefficient -- for every arena those calls serve.  With s = d_out, y_p =
 * the arena's label of slot 2p, ok_p = (label of slot 2p+1 != 0), d_p = s[2p] - s[2p+1], P_ok = #ok, A = mse_weight:
 *   pair term  l_p = softplus(-d_p) = max(-d_p, 0) + log1p(exp(-|d_p|))                                     (ok_p only)
 *   loss       L   = (sum_ok l_p + A * sum_ok (s[2p] - y_p)^2) / max(P_ok, 1) + ARR * sum_l sum_r ||W_l[r+1] - W_l[r]||^2
 *   d_gout[2p] = (-1 / (1 + exp(d_p)) + 2 A (s[2p] - y_p)) / P_ok    d_gout[2p+1] = (1 / (1 + exp(d_p))) / P_ok    (0, 0: void)
 *   d_stats (double[5]) = sum_ok l_p, sum_ok (s[2p] - y_p)^2, #{ok: d_p > 0}, P_ok, the ARR term (coefficient included)
 * every pair evaluated in float64, d_gout its float32 rounding, the sums in a fixed order: the same bits on every run.  A = 0
 * is the plain BPR objective; A = 1 keeps the scores ratings.  d_grad (flat, the layout of the parameters) is overwritten
 * with dL/dparams; d_out[B], d_gout[B] and d_stats are overwritten.  Asynchronous on `stream`.
 * igmc_pair_loss is the middle launch alone, on scores and labels the caller holds (d_out / d_y float[B], B even and >= 2):
 * d_gout[0..B) and d_stats[0..4) as above; d_stats[4] is not written.
 *
 * igmc_pair_negatives_shortlist is igmc_pair_negatives with a share of HARD negatives: items of a per-user table, meant to be
 * every user's co-rating shortlist (below) -- the unseen items the serving path would put in front of the ranker.  The table is
 * indexed by USER ID: user u owns d_sl_item[d_sl_off[u] .. d_sl_off[u + 1]) (d_sl_off int64[n_users + 1], d_sl_item int32,
 * sl_total entries, 0 <= sl_total < 2^31) -- the layout igmc_shortlist_fill leaves for d_users = 0 .. n_users - 1.  With
 * thr = (uint64) floor(hard_share * 2^32), 0 <= hard_share <= 1, for positive k = (u, i) with both ids inside the graph, salt =
 * the igmc_pair_salt of (seed, epoch, k) and H = igmc_splitmix64, in igmc_rng.h's words:
 *   HARD-DECIDED  iff igmc_pair_hard: (H(salt ^ IGMC_PAIR_KEY_HARD) >> 32) < thr.  Share 0 never decides hard, share 1 always
 *                 does.
 *   SEGMENT       of a hard-decided pair: [a, b) = [d_sl_off[u], d_sl_off[u + 1]).  Usable iff 0 <= a <= b <= sl_total; else
 *                 d_err bit 3, its length counts as 0 and nothing is read from it.  If b > a: x = igmc_pair_pick =
 *                 ((H(salt ^ IGMC_PAIR_KEY_PICK) >> 32) * (b - a)) >> 32 and j = d_sl_item[a + x].
 *   QUALIFYING    j qualifies iff 0 <= j < n_items, d_item_ok[j] != 0 (or d_item_ok is NULL) and the graph has no entry (u, j).
 *                 Then j is the negative and d_link_y[2k+1] = 2.0f.  ONE pick, no retry: over a clean segment the pick is
 *                 uniform up to the multiply-shift's bias ((b - a) / 2^32).
 *   STALE TABLE   j does not qualify: d_err bit 2 ("the table does not belong to this graph or mask"), and the uniform draw
 *                 decides.  An empty segment goes on to the uniform draw silently.
 *   UNIFORM DRAW  not hard-decided, or no qualifying pick: EXACTLY the negative of igmc_pair_negatives for this (seed, epoch, k,
 *                 mask) -- label 1.0f, or void (label 0, bit 1).  Ids out of range: bit 0, neither row nor segment is read.
 * Both keys are >= 2^20, so neither word is a try's.  A negative is never an item the user has rated, whatever the table
 * holds.  With hard_share == 0, or d_sl_off == NULL (allowed only with hard_share == 0; d_sl_item is then not read either),
 * every output byte and the error word are igmc_pair_negatives'.  Refused: what igmc_pair_negatives refuses, a share outside
 * [0, 1] or NaN, a NULL d_sl_off or d_sl_item with a share above 0, sl_total outside [0, 2^31).  One wave per positive, the
 * decision and the pick uniform over it; the pick goes through the same row walk as a try, one live lane.
 *
 * igmc_pair_kind_stats tells a step's pairs apart by the kind of their negative (d_out / d_y float[B] as for igmc_pair_loss,
 * B even and >= 2): d_stats6 (double[6]) = for the pairs with d_y[2p+1] == 1.0f their count, #{d_p > 0} and sum softplus(-d_p);
 * then the same three for d_y[2p+1] == 2.0f.  Void pairs (and any other label) are counted nowhere.  One workgroup, float64,
 * the sums in the fixed order of igmc_pair_loss: the same bits on every run. */
int igmc_pair_negatives(const igmc_graph* g, const int32_t* d_pos_u, const int32_t* d_pos_v, int64_t n,
                        const uint8_t* d_item_ok /* may be NULL */, uint64_t seed, uint64_t epoch, int32_t* d_link_u,
                        int32_t* d_link_v, float* d_link_y, int32_t* d_err, void* stream);
int igmc_pair_negatives_shortlist(const igmc_graph* g, const int32_t* d_pos_u, const int32_t* d_pos_v, int64_t n,
                                  const uint8_t* d_item_ok /* may be NULL */, uint64_t seed, uint64_t epoch,
                                  const int64_t* d_sl_off, const int32_t* d_sl_item, int64_t sl_total, double hard_share,
                                  int32_t* d_link_u, int32_t* d_link_v, float* d_link_y, int32_t* d_err, void* stream);
int igmc_pair_kind_stats(const float* d_out, const float* d_y, int B, double* d_stats6, void* stream);
int igmc_pair_loss(const float* d_out, const float* d_y, int B, float mse_weight /* A */, float* d_gout, double* d_stats,
                   void* stream);
int igmc_pair_loss_grad(igmc_model* m, const float* d_params, const igmc_batch* b, int use_edge_flags,
                        const uint8_t* d_lin_mask, uint64_t seed, uint64_t step, float multiply_by, float ARR,
                        float mse_weight /* A */, float* d_out, float* d_gout, float* d_grad, double* d_stats, void* stream);

/* ---- Co-rating shortlists: a retrieval stage in front of the scoring pass (no reference counterpart: the reference has no
 * recommendation path; by hand this is row u of (L L^T) L as scipy sparse products and one np.lexsort per user).
 *
 * RELATIONS.  rel(u, v) is the 0-based relation index of the entry (u, v): the graph's u_rel / v_rel arrays hold exactly it,
 * i.e. h_rating - 1 of igmc_graph_create (h_rating is rating label + 1, 1..R; the arrays hold the label, 0..R-1), and it
 * rises with the rating value as the loaders order class_values.
 *
 * THE DEFINITION.  Two thresholds seed_min_rel = s >= 0 and vote_min_rel = t >= 0 give the binary matrices
 * L_s[u, v] = [the graph has an entry (u, v) and rel(u, v) >= s] and L_t alike; with s = t = 0 every rating counts, with a
 * threshold above every relation the matrix is empty.  For request q, user u = d_users[q]:
 *   w[u']    = #{ i : L_s[u, i] and L_s[u', i] } for u' != u, and w[u] = 0: the items both like.  The user itself never votes.
 *   votes[j] = sum over u' of w[u'] * L_t[u', j]: row u of (L_s L_s^T with its diagonal zeroed) L_t, exact unsigned integers,
 *              defined for EVERY item j, candidates or not.
 *   C        = the candidates of igmc_candidates_fill under the same d_item_ok / exclude_seen.
 *   THE VOTE ORDER over C: votes descending, then item id ascending -- np.lexsort((item, -votes)) over the items of C.
 *   The shortlist of q = the first min(m, |C|) items of C in the vote order, 1 <= m < 2^31; its segment is WRITTEN ITEM
 *   ASCENDING, like every candidate segment (igmc_rank_segments binary-searches it).
 * Items without a vote are ordinary members of C: they fill a short list by ascending id, and a user with no seeding entry
 * (an empty row, or no rating at or above s) gets the m lowest candidate ids.
 * LIMIT.  votes[j] <= max_deg_u * max_deg_v (igmc_graph_info); both entry points refuse -- non-zero return, igmc_last_error,
 * nothing launched -- a graph whose product reaches 2^31.
 *
 * igmc_shortlist_fill writes d_link_u[p] = u, d_link_v[p] = item (int32) and, where d_votes is given, d_votes[p] = votes[item]
 * (uint32) for the p of [d_offsets[q], d_offsets[q + 1]).  There is no count entry: the segment's length is min(m, the count
 * of igmc_candidates_count); the caller clamps those counts and forms d_offsets (int64[nq + 1], offsets[0] = 0, their
 * inclusive prefix sums behind it).  capacity = entries of d_link_u / d_link_v / d_votes, in [1, 2^31): nothing is written
 * at or past it.  d_err[0] (int32, zeroed by the caller, read after the launch), the bits of igmc_candidates_fill:
 *   bit 0 = a segment reaches past capacity (its links there are missing);
 *   bit 1 = a user id outside [0, n_users): its segment is empty and no row is read;
 *   bit 2 = the offsets are not the prefix sums of the clamped counts.
 * igmc_shortlist_places answers, for queries grouped by request -- request q owns the queries [d_q_off[q], d_q_off[q + 1]) of
 * d_q_id (int32[n_query], any order, duplicates allowed; d_q_off int64[nq + 1], d_q_off[0] = 0, d_q_off[nq] = n_query,
 * 0 <= n_query < 2^31: the convention of igmc_rank_segments) --, where each queried item stands in the FULL vote order of its
 * user:
 *   d_q_place[k] = the number of items of C before it in the vote order (int32), or -1 when it is not in C (an item the user
 *                  has rated under exclude_seen, one d_item_ok leaves out, an id outside [0, n_items), a user id out of range);
 *   d_q_votes[k] = votes[d_q_id[k]] (uint32; may be NULL), in C or not; 0 for an id outside [0, n_items) and for a user id out
 *                  of range.
 * "Item j is in the shortlist of size m" is 0 <= place < m.  d_err[0]: bit 0 = d_q_off is not 0 = q_off[0] <= q_off[1] <= ...
 * <= q_off[nq] = n_query: the queries cannot be told apart and EVERY query gets -1 / 0; bit 1 = a user id outside
 * [0, n_users).  Nothing is read outside the n_query queries or written outside d_q_place / d_q_votes, whatever d_q_off holds.
 *
 * Both: one workgroup per request, `grid` workgroups in all (0 = chosen: min(nq, 512); at most 65536; more than nq are not
 * launched), each working through the requests q, q + grid, ...  The outputs are a function of the inputs alone -- every sum
 * is an integer sum -- and do not depend on grid.  d_scratch: igmc_shortlist_scratch_bytes(g, nq, grid) bytes (-1 on bad
 * arguments; 0 where both tables of a workgroup fit its LDS, d_scratch may then be NULL), 4-byte aligned, owned by the caller,
 * its contents before and after the call meaningless: a row per workgroup for w (uint32[n_users], where it does not fit LDS)
 * and the votes (uint32[n_items], for graphs of more than 16384 items).  Nothing is allocated; _fill is one launch, _places
 * two, capturable.  Refusals: a null argument, nq < 1, m outside [1, 2^31), a negative threshold, capacity outside [1, 2^31),
 * grid outside [0, 65536], scratch too small or misaligned, the LIMIT above.
 * igmc_shortlist_plan_info: what a launch over (g, nq, grid) looks like -- [0] workgroups, [1] LDS bytes of a workgroup,
 * [2] 1 = w in LDS, [3] 1 = the votes in LDS, [4] igmc_shortlist_scratch_bytes, [5] the largest n_users whose w fits LDS at
 * this graph's item count. */
int64_t igmc_shortlist_scratch_bytes(const igmc_graph* g, int nq, int grid);
int igmc_shortlist_plan_info(const igmc_graph* g, int nq, int grid, int64_t out6[6]);
int igmc_shortlist_fill(const igmc_graph* g, const int32_t* d_users, int nq, const uint8_t* d_item_ok /* may be NULL */,
                        int exclude_seen, int seed_min_rel, int vote_min_rel, int64_t m, const int64_t* d_offsets,
                        int32_t* d_link_u, int32_t* d_link_v, uint32_t* d_votes /* may be NULL */, int64_t capacity,
                        int32_t* d_err, void* d_scratch, int64_t scratch_bytes, int grid, void* stream);
int igmc_shortlist_places(const igmc_graph* g, const int32_t* d_users, int nq, const uint8_t* d_item_ok /* may be NULL */,
                          int exclude_seen, int seed_min_rel, int vote_min_rel, const int64_t* d_q_off, const int32_t* d_q_id,
                          int64_t n_query, int32_t* d_q_place, uint32_t* d_q_votes /* may be NULL */, int32_t* d_err,
                          void* d_scratch, int64_t scratch_bytes, int grid, void* stream);

/* ---- Where given ids stand in their segments, and the ranking metrics' per-segment sums (no reference counterpart: the
 * reference judges rating regression only, by the test RMSE; by hand this is every candidate score pulled to the host and one
 * `np.lexsort` per user).
 *
 * igmc_rank_segments: for the segments [d_seg_off[s], d_seg_off[s + 1]) of d_keys (float[n]) and d_ids (int32[n], STRICTLY
 * ASCENDING inside every segment: the link_v of a candidate list), s < ns, 1 <= n < 2^31, and queries grouped by segment --
 * segment s owns the queries [d_q_off[s], d_q_off[s + 1]) of d_q_id (int32[nq], in any order, duplicates allowed; d_q_off
 * int64[ns + 1], d_q_off[0] = 0, d_q_off[ns] = nq, 0 <= nq < 2^31) --, per query q of segment s:
 *   d_q_pos[q]  = the position IN d_keys (not in the segment) of the segment's entry with d_ids[position] == d_q_id[q];
 *                 -1 when the segment has none (with candidate lists: an item the user has rated, or one masked out)
 *   d_q_rank[q] = the number of entries of the segment that come BEFORE that entry in THE ORDER of igmc_select_segments (key
 *                 descending, then position ascending; every NaN behind every number, NaNs among themselves by position;
 *                 -0.0 == 0.0), i.e. its 0-based place in np.lexsort((idx, np.where(np.isnan(k), 0, -k), np.isnan(k))) -- querying
 *                 the id at d_idx_out[s * num + r] of igmc_select_segments returns r; a NaN-keyed entry has a place like any
 *                 other; -1 where d_q_pos[q] is -1
 * geometry: 0 = chosen from ns as igmc_select_segments chooses, k in [1, 64] = k workgroups per segment, each counting one
 * contiguous slice.  The counts are integers summed by vector atomic adds on d_q_rank: the result is a function of the inputs
 * alone, whatever the geometry; no scratch.  d_err[0] (int32, ZEROED BY THE CALLER, read after the launches):
 *   bit 0 = d_q_off is not 0 = q_off[0] <= q_off[1] <= ... <= q_off[ns] = nq: the queries cannot be told apart and EVERY query
 *           gets -1 / -1;
 *   bit 1 = a segment is not inside [0, n) (d_seg_off decreasing or out of range): it is taken as empty, its queries get
 *           -1 / -1.
 * Nothing is read outside the n entries of d_keys / d_ids or the nq queries and nothing is written outside the nq entries of
 * d_q_pos / d_q_rank, whatever the offsets hold.  Nothing is allocated here, the three launches are capturable. */
int igmc_rank_segments(const float* d_keys, const int32_t* d_ids, int64_t n, const int64_t* d_seg_off, int ns,
                       const int64_t* d_q_off, const int32_t* d_q_id, int64_t nq, int32_t* d_q_pos, int32_t* d_q_rank,
                       int32_t* d_err, int geometry, void* stream);
/* igmc_rank_metrics: the per-segment (per-user) sums of the held-out ranking metrics with BINARY relevance, over the ranks
 * igmc_rank_segments left.  A query COUNTS when d_q_rel[q] != 0 (uint8[nq]; NULL = every query is relevant) and
 * d_q_rank[q] >= 0; a query without a place is left out, never counted as a miss.  d_ks: int32[nk] cut-offs K on the device,
 * 1 <= nk <= 8, each K >= 1 (a K below 1 counts nothing).  For segment s < ns:
 *   d_cnt[s * (2 + nk) + 0]     = n_rel, the queries that count
 *   d_cnt[s * (2 + nk) + 1]     = first_rank, the smallest rank among them (-1 when n_rel = 0)
 *   d_cnt[s * (2 + nk) + 2 + j] = hits_K = #{rank < K}                                        K = d_ks[j]
 *   d_dcg[s * 2 * nk + j]       = dcg_K  = sum over {rank < K} of 1 / log2(rank + 2)          (float64)
 *   d_dcg[s * 2 * nk + nk + j]  = idcg_K = sum over i < min(K, n_rel) of 1 / log2(i + 2)
 * One wave per segment; the float64 sums are taken in a fixed order (lane l: the segment's queries l, l + 64, ..., then a
 * fixed butterfly), so the output is bit-identical from launch to launch and for every grid (workgroups of the launch: 0 =
 * chosen from ns, at most 65536).  A segment whose query range is not inside [0, nq] has no query and raises bit 0 of
 * d_err[0] (int32, zeroed by the caller).  One launch, capturable. */
int igmc_rank_metrics(const int32_t* d_q_rank, const int64_t* d_q_off, const uint8_t* d_q_rel /* may be NULL */, int64_t nq,
                      int ns, const int32_t* d_ks, int nk, int32_t* d_cnt, double* d_dcg, int32_t* d_err, int grid,
                      void* stream);

/* ---- Leave-one-out neighbour attribution (no reference counterpart: the reference's `visualize` draws an enclosing subgraph
 * and leaves the reading to the eye; by hand an attribution is the subgraph pulled to the host, one node deleted, the node
 * sets rebuilt and replayed one variant at a time).
 *
 * The link in slot i of an EXTRACTED arena `base` has users U[0..nu) and items V[0..nv) in slot order (target first, the rest
 * by ascending id).  Its VARIANTS, in this order: 0 = the whole node set (the base); 1 .. nu-1 = the set without U[k];
 * nu .. nu+nv-2 = the set without V[k - nu + 1].  The two targets are never removed; every remaining node keeps the hop
 * distance -- and so the label -- it has in the whole set: at hop 2 a node reachable only through the removed one STAYS, with
 * its old label.  Scoring the variants is the caller's business (igmc_extract_batch_cached + a forward: the induced edges of
 * the remaining nodes, without the target edge); the attribution of a node is score(variant without it) - score(base).
 *
 * igmc_loo_count (no reference counterpart): for the B links of `base`, d_nvar[i] = nu + nv - 1, d_nu_ids[i] = the user
 * entries the link's variants occupy in a cache, nu + (nu-1)(nu-1) + (nv-1) nu, d_nv_ids[i] = the item entries,
 * nv + (nu-1) nv + (nv-1)(nv-1) (int64[B] each).  B: at most the links the last extraction call put into the arena (after a
 * replayed launch: igmc_batch_assume_size).  Reads the sizes of the arena only: works on lean arenas and on arenas without
 * dense blocks and never makes an arena emit its CSR. */
int igmc_loo_count(const igmc_batch* base, int B, int64_t* d_nvar, int64_t* d_nu_ids, int64_t* d_nv_ids, void* stream);
/* igmc_loo_fill (no reference counterpart): writes every variant of the B links of `base` (an arena of graph g) into a cache of
 * the format igmc_extract_batch_cached reads.  d_var_off / d_uent_off / d_vent_off: int64[B + 1], the batch's slice of the
 * exclusive prefix sums of the three counts over the pass, so that link i owns the variants [d_var_off[i], d_var_off[i + 1])
 * and the entries [d_uent_off[i], d_uent_off[i + 1]) of d_unodes / d_udist (items alike).  Variant k of link i at v =
 * d_var_off[i] + k:
 *   d_uoff[v], d_voff[v]   int64, the variant's first entry -- and d_uoff / d_voff[d_var_off[i + 1]] = the end of the link's
 *                          last variant, so d_uoff / d_voff need cap_var + 1 entries
 *   d_unodes / d_vnodes    int32 ids, target first, then ascending;  d_udist / d_vdist  uint8 hop distances (slot label / 2)
 *   d_var_link[v]          int32  link0 + i
 *   d_var_side[v]          uint8  0 = a user was removed, 1 = an item, 255 = the base
 *   d_var_node[v]          int32  the removed global id, -1 for the base
 *   d_var_rating[v]        uint8  rating + 1 of the entry of g that joins the removed node to the OPPOSITE target -- (u', v) for a
 *                          removed user u', (u, v') for a removed item v' --, 0 if they share none (and for the base)
 * d_err[0] (int32, ZEROED BY THE CALLER, read after the launch): bits 0 / 1 / 2 = a link's variants / user entries / item
 * entries reach past cap_var / cap_uent / cap_vent; bit 3 = the offsets of a link are not the prefix sums of its counts;
 * bit 4 = a slot's sizes are not those of an extracted link.  A link that raises a bit has NOTHING written, the other links are complete.
 * Nothing is written outside the capacities.  The output is a function of the inputs alone (plain stores, no atomics besides
 * the error word); one launch, capturable; nothing is allocated. */
int igmc_loo_fill(const igmc_graph* g, const igmc_batch* base, int B, int64_t link0, const int64_t* d_var_off,
                  const int64_t* d_uent_off, const int64_t* d_vent_off, int64_t cap_var, int64_t cap_uent, int64_t cap_vent,
                  int64_t* d_uoff, int32_t* d_unodes, uint8_t* d_udist, int64_t* d_voff, int32_t* d_vnodes, uint8_t* d_vdist,
                  int32_t* d_var_link, uint8_t* d_var_side, int32_t* d_var_node, uint8_t* d_var_rating, int32_t* d_err,
                  void* stream);
/* igmc_loo_deltas (no reference counterpart): d_scores float[d_var_off[n_links]] = one score per variant, d_var_off int64
 * [n_links + 1] over the whole pass.  d_base[i] = the score of link i's variant 0; for its variants k >= 1,
 * d_delta[d_seg_off[i] + k - 1] = score - base and d_key[...] = |delta| (a NaN score or base gives a NaN key), with
 * d_seg_off[i] = d_var_off[i] - i (int64[n_links + 1], computed by the caller): the base entries drop out and the segments
 * [d_seg_off[i], d_seg_off[i + 1]) are what igmc_select_segments takes -- its order (key descending, index ascending, NaNs
 * last) ranks, among equal |delta|, users before items and lower ids first.  One launch, capturable. */
int igmc_loo_deltas(const float* d_scores, const int64_t* d_var_off, int64_t n_links, float* d_base, float* d_delta,
                    float* d_key, const int64_t* d_seg_off, void* stream);

/* Per-kernel timing of the last call (HIP events on the launch stream); names/ms arrays are
 * filled up to `cap` (ms = total over `calls` launches of that kernel since the last fetch);
 * returns the number of distinct kernels recorded, or <0 on error. */
int igmc_profile_enable(int on);
int igmc_profile_fetch(char names[][48], float* ms, int* calls, int cap);
/* igmc_profile_enable(2): no events (legal inside a hipGraph capture); instead every k_graph_step launch enqueued or
 * captured from then on clocks itself on the device (earliest workgroup start -> last workgroup end, constant-rate
 * wall clock), which is how bench.py times the dominant kernel UNDER graph replay.  Returns the launches and their
 * mean duration since the last reset; synchronises the device. */
int igmc_profile_gs_clock(const igmc_model* m, int64_t* launches, double* mean_us, int reset);

/* Health check of the workspace (synchronises `stream`): fails when a bounded device-side wait of the
 * one-workgroup-per-subgraph step kernel ever timed out since the last check.  No reference counterpart. */
int igmc_model_check(igmc_model* m, void* stream);
/* 1 when forward / loss_grad / train_step on (this arena, batch size B) run the matrix-core subgraph kernel, which
 * reads the dense blocks only (see igmc_batch_set_lean); 0 otherwise.  No reference counterpart. */
int igmc_model_dense_path(const igmc_model* m, const igmc_batch* b, int B);
/* Which kernels a training step on (this arena, batch size B) is made of -- what a caller that overlaps the extraction of
 * the next batches with the steps needs to know to pace it (igmc_ctrl_gate): 1 = the subgraph kernel (igmc_model_dense_path),
 * 2 = the one-launch dense-layer kernels, 3 = those in their group-split form (two relation groups at once), 0 = the
 * per-layer kernels.  No reference counterpart. */
int igmc_model_step_form(const igmc_model* m, const igmc_batch* b, int B);
/* The launch geometry of a training step on (this arena, batch size B), from the same decision the launch sequence takes its
 * branches from.  Writes min(n, IGMC_GEOM_N) values to out[]:
 *   [0] igmc_model_step_form
 *   [1] kernel family: 0 = CSR row walkers, 1 = subgraph kernel, 2 = one-launch dense layers, 3 = per-layer dense layers
 *   [2] subgraph kernel: workgroups per subgraph (4, 2, 1), else 0
 *   [3] subgraph kernel: grid (fewer workgroups than subgraphs at 1 per subgraph: each loops over several), else 0
 *   [4] [5] dense layers: workgroups of a subgraph's user side / item side, else 0
 *   [6] relation groups (0 for the row walkers)
 *   [7] 1 = the two relation groups at once (group split), 0 = group after group or one group
 *   [8] 1 = the backward leaves relation-space tables (k_tail_ts -> k_finalize_ts)
 *   [9] subgraph kernel: padded k extent of its planes (kp), else 0
 *   [10] dense layers: 1 = the backward as one launch (k_dl_bwd)
 * Fails when B is outside 1 .. the arena's max_graphs.  No reference counterpart. */
#define IGMC_GEOM_N 11
int igmc_model_step_geometry(const igmc_model* m, const igmc_batch* b, int B, int32_t* out, int n);
/* Clears the row / plane exchange regions of the subgraph and dense-layer kernels (enqueued on `stream`).  They must only ever
 * hold finite values (a consumer copies whole plane images, stale rows of earlier launches included, and multiplies them by
 * zero block entries): call it after steps that ran on non-finite parameters, e.g. when parameters are restored. */
int igmc_model_reset_exchange(igmc_model* m, void* stream);

/* 1 when the arena's slots (129..256 nodes a side, dense block + transposed copy) send the conv layers of the per-layer
 * sequence to the matrix-core layer kernels (k_dl_layer) instead of the CSR row walkers. */
int igmc_model_dense_layers(const igmc_model* m, const igmc_batch* b, int B);

/* ---- Sort-pool readout family: DGCNN_RS (reference models.py:123-167 on the DGCNN base :63-120; Main.py:364-380).
 * Four R-GCN layers with latent_dim [32, 32, 32, 1] (the conv kernels of igmc_model), concat (97 channels),
 * global_sort_pool(k) (PyG 1.4.2: nodes of a graph by the last channel, descending; first k rows, zero padding),
 * Conv1d(1,16,97,97) + ReLU, MaxPool1d(2,2), Conv1d(16,32,5,1) + ReLU, lin1 (dense -> 128) + ReLU, dropout(0.5), lin2.
 * Parameters live in ONE flat buffer in the "true" layout reported by igmc_sortpool_layout (offsets of
 * convs.{0..3}.{basis,root,bias,att}, conv1d_params1.{weight,bias}, conv1d_params2.{weight,bias}, lin1.{weight,bias},
 * lin2.{weight,bias}; [24] parameter count, [25] dense width 32 * (k/2 - 4), [26] k).  `m` supplies the conv workspace
 * (create it with n_side = 0); max_nodes_per_graph >= the arena's slot size (users + items of one subgraph). */
typedef struct igmc_sortpool igmc_sortpool;
int igmc_sortpool_create(igmc_model* m, int k, int max_nodes_per_graph, igmc_sortpool** out);
void igmc_sortpool_destroy(igmc_sortpool* sp);
int igmc_sortpool_layout(const igmc_sortpool* sp, int64_t* out27);
/* replaces DGCNN_RS.forward (models.py:142-167); training != 0: dropout active, activations kept for the backward */
int igmc_sortpool_forward(igmc_sortpool* sp, const float* d_params, const igmc_batch* b, int training,
                          int use_edge_flags, const uint8_t* d_lin_mask, uint64_t seed, uint64_t step,
                          float* d_out, void* stream);
/* replaces out = model(data); loss = mse (+ ARR over model.convs, train_eval.py:162-174); loss.backward():
 * d_grad (true layout) is overwritten, d_loss[0] = loss, d_loss[1] = sum of squared errors. */
int igmc_sortpool_loss_grad(igmc_sortpool* sp, const float* d_params, const igmc_batch* b, int use_edge_flags,
                            const uint8_t* d_lin_mask, uint64_t seed, uint64_t step, float ARR, float grad_scale,
                            float arr_scale, float* d_out, float* d_grad, float* d_loss, void* stream);

/* optimizer.step() + loss bookkeeping of a sort-pool step in ONE launch, like igmc_step_finish for IGMC: Adam over the
 * sort-pool family's flat buffer (igmc_sortpool_layout [24] parameters), d_loss[0..1], d_total[0] += loss * num_graphs and,
 * with d_ctrl, the Adam scalars from / the tick of the control block -- so that the step is hipGraph-capturable
 * (call igmc_sortpool_loss_grad with d_loss = NULL). */
int igmc_sortpool_step_finish(igmc_sortpool* sp, const igmc_batch* b, float* d_params, const float* d_grad,
                              float* d_exp_avg, float* d_exp_avg_sq, float ARR, float* d_loss, double* d_total,
                              int64_t* d_ctrl, int64_t step, float lr, float beta1, float beta2, float eps,
                              float weight_decay, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IGMC_HIP_H */
