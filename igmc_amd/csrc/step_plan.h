// step_plan.h -- which kernels take a call on (model, arena, B): the environment hooks, the eligibility predicates of the
// kernel families and the ONE function that turns them into a StepPlan (launch.h).  Last file of the graphstep2.hip
// translation unit: the predicates size their kernels with the LDS plans of g2_compose.h / dl_kernels.h.  Nothing outside
// this file reads a decision hook or calls a predicate -- the launch sequences (model.hip) and the queries of the C ABI
// (capi.hip) read plans.
#include <limits.h>

// The decision hooks, read on EVERY call (tests switch them per case).  IGMC_HOOK_UNSET: the variable is not set.
#define IGMC_HOOK_UNSET INT_MIN
struct StepHooks {
  int graph_step;      // IGMC_GRAPH_STEP=0: never the subgraph kernel
  int gs_cluster;      // IGMC_GS_CLUSTER: workgroups per subgraph asked for
  int gs_grid;         // IGMC_GS_GRID: fewer workgroups than graphs (accumulating partials)
  int dl;              // IGMC_DL=0: never the dense-layer kernels
  int dl_fused;        // IGMC_DL_FUSED: 0 the per-layer launches, 1 the one-launch forward only, 2 as unset (wide arenas: only 2)
  int dl_ts;           // IGMC_DL_TS=0: no relation-space tables behind the dense layers
  int dl_gsplit;       // IGMC_DL_GSPLIT=0: the group-after-group form
  int dl_head;         // IGMC_DL_HEAD=0: the loss head as a launch of its own in front of k_dl_bwd
  int fin_mode;        // IGMC_FIN_MODE=0: the hand-off version of the gradient / Adam tail (k_finalize)
  int tail_fold;       // IGMC_TAIL_FOLD=0: the two-launch tail behind the subgraph kernel (k_tail_ts -> k_finalize_ts)
  int l3_vec;          // IGMC_L3_VEC=0: layer 3's weight gradient leaves the subgraph kernel as tables in every launch form
};
static int step_hook(const char* name, int unset) {
  const char* e = getenv(name);
  return e ? atoi(e) : unset;
}
static StepHooks step_hooks() {
  StepHooks hk;
  hk.graph_step = step_hook("IGMC_GRAPH_STEP", 1);
  hk.gs_cluster = step_hook("IGMC_GS_CLUSTER", IGMC_HOOK_UNSET);
  hk.gs_grid = step_hook("IGMC_GS_GRID", 0);
  hk.dl = step_hook("IGMC_DL", 1);
  hk.dl_fused = step_hook("IGMC_DL_FUSED", IGMC_HOOK_UNSET);
  hk.dl_ts = step_hook("IGMC_DL_TS", 1);
  hk.dl_gsplit = step_hook("IGMC_DL_GSPLIT", 1);
  hk.dl_head = step_hook("IGMC_DL_HEAD", 1);
  hk.fin_mode = step_hook("IGMC_FIN_MODE", 1);
  hk.tail_fold = step_hook("IGMC_TAIL_FOLD", 1);
  hk.l3_vec = step_hook("IGMC_L3_VEC", 1);
  return hk;
}
int igmc_dl_always() { return step_hook("IGMC_DL_ALWAYS", 0) == 1; }

// ---- the subgraph kernel
// workgroups per subgraph: 4 (2) when 4 (2) x the padded batch still fits one workgroup per CU with a margin
static int gs_cluster(const StepHooks& hk, int B) {
#ifdef IGMC_HIPEMU
  // the emulator runs workgroups one after the other unless a test asks for clusters (their members then run
  // together: hipemu::Runtime::co_cs)
  int want = 1;
#else
  static int cus = -1;
  if (cus < 0) {
    hipDeviceProp_t prop;
    int dev = 0;
    cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) ? prop.multiProcessorCount : 0;
  }
  int want = (cus >= 240) ? 4 : 1;        // the clustered launch needs (almost) every CU of an MI355X to itself
#endif
  if (hk.gs_cluster != IGMC_HOOK_UNSET) want = hk.gs_cluster;
  const int stride = (B + 7) & ~7;
  if (want >= 4 && 4 * stride <= 224) return 4;
  if (want >= 2 && 2 * stride <= 224) return 2;
  return 1;
}
static int gs_grid(const StepHooks& hk, int B) {
  int cap = IGMC_WG_BLOCKS;
  if (hk.gs_grid > 0 && hk.gs_grid < cap) cap = hk.gs_grid;
  return B < cap ? B : cap;
}
// 1 = the matrix-core subgraph kernel takes this batch configuration
static int g2_eligible(const StepHooks& hk, const ModelDev& m, const BatchDev& b, int B, G2Layout* lay, int* cs_out) {
  if (hk.graph_step == 0 || !igmc_g2_xcd_ok()) return 0;
  const int cs = gs_cluster(hk, B);
  if (!igmc_g2_layout(m, b, cs, lay)) return 0;
  *cs_out = cs;
  return 1;
}

// ---- the dense-layer kernels
// 1 = the dense per-layer kernels take the conv layers of this arena
static int dl_base_ok(const StepHooks& hk, const ModelDev& m, const BatchDev& b, int B, int wide) {
  if (hk.dl == 0) return 0;
  if (!b.relm || !b.relmT || !m.g2_w || m.L > 8) return 0;
  const int rows0 = m.R * m.L + m.L + 1;
  // wide: the two-group layout -- six to ten relations, or a layer-0 table of 33..48 rows (two hops)
  if (wide ? (g2_groups(m.R, m.L) == 1 || m.R > G2_NR * G2_NG_MAX || rows0 > 48) : (m.R > G2_NR || rows0 > 32)) return 0;
  const int cmax = b.cap_u > b.cap_v ? b.cap_u : b.cap_v;
  const DlSplit sq = dl_split(b.cap_u, b.cap_v, B);
  return cmax <= 256 && B * (sq.nqu + sq.nqv) <= IGMC_GATHER_BLOCKS;
}
static int dl_eligible(const StepHooks& hk, const ModelDev& m, const BatchDev& b, int B) {
  return dl_base_ok(hk, m, b, B, 0) && dl_lds(dl_kp(b)) <= (size_t)160 * 1024;
}
// 1 = the backward passes of this arena can leave relation-space tables (k_dl_layer<*, true, true>): the tail of the
// subgraph kernel (k_tail_ts -> k_finalize_ts) then replaces G / Y / the weight-gradient products
static int dl_ts_eligible(const StepHooks& hk, const ModelDev& m, const BatchDev& b, int B) {
  if (hk.dl_ts == 0 || !dl_eligible(hk, m, b, B) || !m.ts_part || !m.cnt0) return 0;
  const DlSplit sq = dl_split(b.cap_u, b.cap_v, B);
  const int stride = (B + 7) & ~7;
  if ((sq.nqu + sq.nqv) * stride > IGMC_TS_BLOCKS || m.R * m.L > 20) return 0;
  return dl_lds(dl_kp(b), true) <= (size_t)160 * 1024;
}
// 1 = the forward of this arena's dense layers runs as ONE launch (k_dl_fwd): exchange regions for 256 nodes a side, every
// workgroup of the launch resident at once
static int dl_fwd_eligible(const StepHooks& hk, const ModelDev& m, const BatchDev& b, int B) {
  if (!igmc_g2_xcd_ok() || hk.dl_fused == 0) return 0;      // (the members' exchange goes through the L2 of one XCD)
  if (!dl_eligible(hk, m, b, B) || !m.g2_ex || m.ex_nodes < DLX_K || b.graph_cap > m.g2_graphs) return 0;
  const DlSplit sq = dl_split(b.cap_u, b.cap_v, B);
  if (B * (sq.nqu + sq.nqv) > 224) return 0;                  // (one workgroup per CU, all of them resident: the members wait for each other)
  return (size_t)dlf_words(dl_kp(b)) * 4 <= (size_t)160 * 1024;
}
// 1 = ... and the backward (k_dl_bwd: same conditions as k_dl_fwd -- whose launch precedes it and maintains the exchange
// regions -- plus the tables')
static int dl_bwd_eligible(const StepHooks& hk, const ModelDev& m, const BatchDev& b, int B) {
  if (!dl_fwd_eligible(hk, m, b, B) || !dl_ts_eligible(hk, m, b, B) || hk.dl_fused == 1) return 0;
  return (size_t)dlb_words(dl_kp(b)) * 4 <= (size_t)160 * 1024;
}
// 1 = more than G2_NR relations (<= G2_NR * G2_NG_MAX, layer-0 table <= 48 rows) on the one-launch dense kernels, which take the
// relations in groups: k_dl_fwd / k_head_sub / k_dl_bwd<*, NG> with the relation-space tables behind them -- all of it or
// nothing (the per-layer kernels k_dl_layer0 / k_dl_layer stop at G2_NR relations).  tables_tail: the tail of the tables runs
// (IGMC_FIN_MODE, its stash) -- without it the step does NOT go wide, and the arena must then carry the CSR the row walkers read
static int dl_wide(const StepHooks& hk, const ModelDev& m, const BatchDev& b, int B, int tables_tail) {
  if (!igmc_g2_xcd_ok() || !dl_base_ok(hk, m, b, B, 1)) return 0;
  if ((hk.dl_fused != IGMC_HOOK_UNSET && hk.dl_fused != 2) || hk.dl_ts == 0 || !tables_tail) return 0;
  if (!m.g2_ex || m.ex_nodes < DLX_K || b.graph_cap > m.g2_graphs || !m.ts_part || !m.cnt0) return 0;
  const DlSplit sq = dl_split(b.cap_u, b.cap_v, B);
  const int stride = (B + 7) & ~7, kp = dl_kp(b);
  if (B * (sq.nqu + sq.nqv) > 224 || (sq.nqu + sq.nqv) * stride > IGMC_TS_BLOCKS) return 0;
  const int ng = g2_groups(m.R, m.L);
  return (size_t)dlf_words(kp, ng) * 4 <= (size_t)160 * 1024 && (size_t)dlb_words(kp, ng) * 4 <= (size_t)160 * 1024;
}
// 1 = the group-split forms of k_dl_fwd / k_dl_bwd take this arena: two relation groups, no workgroup with more than DL_NW / 2
// bundles (dl_split / dl_rows over the slot capacities), both images beside the planes in LDS
static int dl_gsplit(const StepHooks& hk, const ModelDev& m, const BatchDev& b, int B) {
  if (g2_groups(m.R, m.L) != 2 || g2_rel_groups(m.R) != 2 || hk.dl_gsplit == 0) return 0;
  const DlSplit sq = dl_split(b.cap_u, b.cap_v, B);
  const int nbu = (b.cap_u + 15) >> 4, nbv = (b.cap_v + 15) >> 4;
  if ((nbu + sq.nqu - 1) / sq.nqu > DL_GB || (nbv + sq.nqv - 1) / sq.nqv > DL_GB) return 0;
  const int kp = dl_kp(b);
  return (size_t)dlf_words_gs(kp) * 4 <= 160 * 1024 && (size_t)dlb_words_gs(kp) * 4 <= 160 * 1024;
}

// ---- the plan
void igmc_step_plan(const ModelDev& m, const BatchDev& b, int B, int kind, StepPlan* p) {
  memset(p, 0, sizeof(*p));
  const StepHooks hk = step_hooks();
  const int ny = (m.D / 16 + 3) / 4;
  const int l0_mfma = m.R * m.L + m.L + 1 <= 32;      // the layer-0 table (gradient) rides on the matrix cores
  const int fin = hk.fin_mode && m.fin_stash;                        // k_finalize_ts may run at all
  const int tables_tail = fin && m.datt_part;                        // ... on relation-space tables (up to ten relations)
  const int fts = tables_tail && m.R <= 8;                           // ... behind the subgraph kernel / the narrow dense layers
  p->kind = kind;
  p->fast_head = (m.D % 16 == 0) && 8 * ny <= IGMC_WG_BLOCKS;
  const int fused = kind == IGMC_CALL_STEP && p->fast_head;          // (a step without fast_head: the generic sequence)
  const int g2 = l0_mfma && g2_eligible(hk, m, b, B, &p->lay, &p->cs);
  const int narrow = dl_eligible(hk, m, b, B), wide = dl_wide(hk, m, b, B, tables_tail);
  p->dense_layers = narrow || wide;
  // The CSR is read by the row walkers: the forward's where no dense family runs, the separate backward's (IGMC_CALL_CONV)
  // unless the per-layer dense kernels take it.  FINDING kept as it was: a step WITHOUT fast_head (side features whose width
  // is no multiple of 16) on a wide arena runs the generic sequence, whose backward walks rows, and reports 0 here.
  p->needs_csr = !(narrow || (kind != IGMC_CALL_CONV && (g2 || wide)));
  if (g2 && (fused || kind == IGMC_CALL_EVAL)) {
    p->family = IGMC_FAM_G2;
    p->grid = (p->cs > 1) ? p->cs * ((B + 7) & ~7) : gs_grid(hk, B);
    p->tail = fts ? IGMC_TAIL_TS : IGMC_TAIL_HANDOFF;
    p->exchange_inside = fused && fts;
    // the tail as ONE launch (k_tail_fin): a workgroup per input row of a layer, which takes no more than 32 of them and hands
    // over no more than IGMC_FOLD_NA d att entries (R <= 8: also no more than IGMC_FOLD_PSETS row producers a row).  The call decides the rest: Adam with the weight images, no exchange
    // (the four stash workgroups appended to the subgraph kernel's launch take a CU each -- the launch's dynamic LDS -- and are
    //  resident with the rest: a clustered grid is <= 224 on >= 240 CUs (gs_cluster), any other <= IGMC_WG_BLOCKS)
    p->tail_fold = fused && fts && hk.tail_fold != 0 && m.fold_w && m.L <= 32 && 4 * m.R <= IGMC_FOLD_NA;
    // layer 3's weight gradient as centre vectors: dPre_3 lives on the two centre rows, so a cluster's layer-3 tables are one
    // outer product a side -- the member that owns the centre leaves its factors, nobody stores a table, and both tails
    // (k_tail_ts, k_tail_fin) form the products where they add them.  Only where a slot holds ONE such product: a training step
    // whose subgraphs have a cluster each (cs > 1: the straight-line form, two different centre members).  The looping grid
    // accumulates several subgraphs in a slot, and at cs == 1 the slot is the sum of both sides' products: tables
    p->l3_vec = (fused && fts && p->cs > 1 && hk.l3_vec != 0 && m.l3_vec) ? 2 * p->cs / G2_NB : 0;
    p->step_form = 1;
    return;
  }
  const int dlf1 = narrow && dl_fwd_eligible(hk, m, b, B), dlb1 = dlf1 && dl_bwd_eligible(hk, m, b, B);
  p->wide = wide;
  p->dl = wide || narrow;
  p->dlf = wide || dlf1;
  if (fused) {
    // relation-space tables behind the dense layers: k_tail_ts sums them and forms d lin1 / d lin2, k_finalize_ts turns them into
    // gradients (+ Adam) -- instead of the Y products, G, the weight-gradient products and their reduction
    p->dlts = wide || (narrow && l0_mfma && fts && dl_ts_eligible(hk, m, b, B));
    p->dlb = p->dlts && (wide || dlb1);
    p->self_seq = !p->dlts;
    p->head_inside = hk.dl_head != 0;
    p->bwd_dense = p->dl;
    // (basis-space mode: the layer-0 table comes from the MFMA weight-gradient kernel or from k_l0_bwd's partials)
    p->exchange_inside = fin && m.R <= IGMC_FBS_MAX_R;
    p->tail = p->dlts ? IGMC_TAIL_TS : p->exchange_inside ? IGMC_TAIL_BS : IGMC_TAIL_HANDOFF;
  } else {
    // the conv layers as calls of their own.  A dense readout gradient (sort-pool family: m.dcat) takes the one-launch
    // backward with relation-space tables; the forward then need not leave the Y products behind
    p->dlts = p->dlb = fts && l0_mfma && m.dcat[0] && dlb1;
    p->self_seq = 1;
    p->bwd_dense = narrow;
    p->need_y = kind != IGMC_CALL_EVAL && !p->dlts;
    p->tail = p->dlts ? IGMC_TAIL_TS : IGMC_TAIL_HANDOFF;
  }
  p->gsplit = p->dlf && dl_gsplit(hk, m, b, B);
  p->family = p->dlf ? IGMC_FAM_DLF : p->dl ? IGMC_FAM_DL : IGMC_FAM_ROWS;
  if (p->dl) {
    const DlSplit sq = dl_split(b.cap_u, b.cap_v, B);
    p->nqu = sq.nqu;
    p->nqv = sq.nqv;
    p->dl_grid = B * (sq.nqu + sq.nqv);
  }
  p->step_form = (wide && p->gsplit) ? 3 : p->dlf ? 2 : 0;
}
