"""The launch geometries of a training step (``igmc_model_step_geometry``) that the batch size, the slot capacities and the
side-feature width select -- one row on each side of every threshold that B and the slot extents cross in ``gs_cluster`` /
``igmc_g2_layout`` (step_plan.h, g2_compose.h), ``dl_split`` (dl_kernels.h) / ``dl_*_eligible`` / ``dl_wide`` /
``dl_gsplit`` (step_plan.h) and the dense block of ``igmc_batch_create`` (capi.hip).  The relation count is 5 or 10 and the
label count 4 throughout, but for one two-hop row at R = 5 (a 37-row layer-0 table): the thresholds the relation and label
counts cross -- the (R, L) plane -- are the rows of tests/relation_label_checks.py (tests/test_emu_relation_labels.py,
tests/test_gpu_relation_labels.py).

tests/test_gpu_geometry.py runs every row against the oracle on an MI355X; tests/test_emu_geometry.py checks the query's
answer for every row on the CPU (the emulator picks the clusters an MI355X picks when ``IGMC_GS_CLUSTER=4``)."""
import collections

import numpy as np

Row = collections.namedtuple('Row', 'id dataset mnph R hops side B cap env geometry')


def G(family, wg=0, grid=0, nq=(0, 0), groups=1, gsplit=0, tables=1, kp=0, dl_bwd=0):
    """Expected ``ModelWorkspace.step_geometry`` dict."""
    form = {'subgraph': 1, 'dense_fused': 3 if gsplit else 2}.get(family, 0)
    if family == 'rows':
        groups, tables = 0, 0
    return dict(form=form, family=family, wg_per_graph=wg, grid=grid, nqu=nq[0], nqv=nq[1], groups=groups, gsplit=gsplit,
                tables=tables, kp=kp, dl_bwd=dl_bwd)


def row(id, dataset, mnph, B, geometry, R=5, hops=1, side=0, cap=None, env=None):
    return Row(id, dataset, mnph, R, hops, side, B, cap or B, env or {}, geometry)


ROWS = [
    # ---- ml_1m, the subgraph kernel: 4 workgroups per subgraph up to B = 56 (4 x 56 workgroups), slots of <= 128 a side
    row('ml1m_128_b50_cs4', 'ml_1m', 127, 50, G('subgraph', 4, 224, kp=136)),
    row('ml1m_128_b1_cs4_ragged', 'ml_1m', 127, 1, G('subgraph', 4, 32, kp=136), cap=50),
    row('ml1m_128_b7_cs4_ragged', 'ml_1m', 127, 7, G('subgraph', 4, 32, kp=136), cap=50),
    row('ml1m_128_b56_cs4', 'ml_1m', 127, 56, G('subgraph', 4, 224, kp=136)),
    # 129 nodes a side: beyond the subgraph kernel, the dense layers take it (without a dense block's transposed copy
    # the arena would fall to the row walkers)
    row('ml1m_129_b50_dense', 'ml_1m', 128, 50, G('dense_fused', nq=(2, 2), dl_bwd=1)),
    # ---- 2 workgroups per subgraph from B = 57 to 112: slots of <= 64 a side
    row('ml1m_64_b57_cs2', 'ml_1m', 63, 57, G('subgraph', 2, 128, kp=72)),
    row('ml1m_64_b112_cs2', 'ml_1m', 63, 112, G('subgraph', 2, 224, kp=72)),
    row('ml1m_65_b57_refused', 'ml_1m', 64, 57, G('rows')),
    # ---- 1 workgroup per subgraph from B = 113: slots of <= 32 a side, a grid of 64 workgroups looping over the subgraphs
    row('ml1m_32_b113_cs1_loop', 'ml_1m', 31, 113, G('subgraph', 1, 64, kp=40)),
    row('ml1m_32_b130_cs1_loop', 'ml_1m', 31, 130, G('subgraph', 1, 64, kp=40)),
    row('ml1m_32_b200_cs1_loop', 'ml_1m', 31, 200, G('subgraph', 1, 64, kp=40)),
    row('ml1m_33_b113_refused', 'ml_1m', 32, 113, G('rows')),
    # ... and one workgroup per subgraph without the loop (test hook: the cluster size an MI355X does not pick at B = 50)
    row('ml1m_32_b50_cs1_hook', 'ml_1m', 31, 50, G('subgraph', 1, 50, kp=40), env={'IGMC_GS_CLUSTER': '1'}),
    # 32 against 33 nodes a side at 2 workgroups per subgraph: one k step of 32 or two
    row('ml1m_32_b100_cs2_kp40', 'ml_1m', 31, 100, G('subgraph', 2, 208, kp=40)),
    row('ml1m_33_b100_cs2_kp72', 'ml_1m', 32, 100, G('subgraph', 2, 208, kp=72)),
    # ---- ml_100k at cap 200 (201 a side): how dl_split shares a subgraph's bundles depends on B
    row('ml100k_201_b7_members', 'ml_100k', 200, 7, G('dense_fused', nq=(7, 7), dl_bwd=1)),
    row('ml100k_201_b50_2p2', 'ml_100k', 200, 50, G('dense_fused', nq=(2, 2), dl_bwd=1)),
    row('ml100k_201_b57_layer_tables', 'ml_100k', 200, 57, G('dense_layer', nq=(2, 2))),
    row('ml100k_201_b64_layer_tables', 'ml_100k', 200, 64, G('dense_layer', nq=(2, 2))),
    row('ml100k_201_b65_layer_gy', 'ml_100k', 200, 65, G('dense_layer', nq=(2, 2), tables=0)),
    row('ml100k_201_b130_layer_gy', 'ml_100k', 200, 130, G('dense_layer', nq=(2, 2), tables=0)),
    # ---- the dense block's 60 KB (capi.hip): square slots of 243 nodes a side fit, 244 do not
    row('ml100k_243_b16_dense', 'ml_100k', 242, 16, G('dense_fused', nq=(8, 6), dl_bwd=1)),
    row('ml100k_244_b16_no_block', 'ml_100k', 243, 16, G('rows')),
    # ---- ten relations at cap 100: two relation groups, at once while no workgroup holds more than 4 bundles
    row('ml10m_101_b7_gsplit', 'ml_10m_lite', 100, 7, G('dense_fused', nq=(4, 4), groups=2, gsplit=1, dl_bwd=1), R=10),
    row('ml10m_101_b50_gsplit', 'ml_10m_lite', 100, 50, G('dense_fused', nq=(2, 2), groups=2, gsplit=1, dl_bwd=1), R=10),
    row('ml10m_101_b57_groups', 'ml_10m_lite', 100, 57, G('dense_fused', nq=(2, 1), groups=2, dl_bwd=1), R=10),
    row('ml10m_101_b100_groups', 'ml_10m_lite', 100, 100, G('dense_fused', nq=(1, 1), groups=2, dl_bwd=1), R=10),
    row('ml10m_101_b113_rows', 'ml_10m_lite', 100, 113, G('rows'), R=10),
    # ---- two hops: a layer-0 table of 5 x 6 + 6 + 1 = 37 rows takes the two-group layout
    row('ml100k_h2_41_b50_wide', 'ml_100k', 20, 50, G('dense_fused', nq=(2, 2), groups=2, dl_bwd=1), hops=2),
    # ---- side features (32 per link): the dense layers with the side features in their loss head
    row('ml100k_201_b50_side', 'ml_100k', 200, 50, G('dense_fused', nq=(2, 2), dl_bwd=1), side=32),
]

FAMILIES = ('rows', 'subgraph', 'dense_fused', 'dense_layer')


def geometry_kinds(geometries):
    """What a set of geometries covers: kernel families, subgraph-kernel forms (workgroups per subgraph, looping grid),
    dense splits with and without tables (``dense_fused_tables0``: the one-launch forward whose backward leaves no tables),
    relation groups with and without the split."""
    kinds = set()
    for g, B in geometries:
        kinds.add(g['family'])
        if g['family'] == 'subgraph':
            kinds.add('wg%d%s' % (g['wg_per_graph'], '_loop' if g['grid'] < B else ''))
        if g['family'] in ('dense_fused', 'dense_layer'):
            kinds.add('%s_tables%d' % (g['family'], g['tables']))
        if g['groups'] == 2:
            kinds.add('groups_gsplit%d' % g['gsplit'])
    return kinds


REQUIRED_KINDS = set(FAMILIES) | {'wg4', 'wg2', 'wg1', 'wg1_loop', 'dense_fused_tables1', 'dense_layer_tables1',
                                  'dense_layer_tables0', 'groups_gsplit0', 'groups_gsplit1'}

_SPLITS = {}


def load_split(dataset):
    from igmc_amd import preprocessing
    if dataset not in _SPLITS:
        kw = {}
        if dataset == 'ml_10m_lite':       # bench.py's ml_10m_lite: ML-10M's ten half-star levels on the ml_1m-shaped graph
            kw['rating_map'] = {float(i): i / 2.0 for i in range(1, 11)}
        _SPLITS[dataset] = preprocessing.create_trainvaltest_split(dataset, 1234, True, verbose=False, **kw)
    return _SPLITS[dataset]


def ml_case(dataset, mnph, n, hops=1, seed=3):
    """``n`` training links of a bundled MovieLens-shaped dataset as a parity case (no reference records)."""
    (_, _, A, tr_l, tr_u, tr_v, _, _, _, _, _, _, cv) = load_split(dataset)
    pick = np.random.default_rng(seed).permutation(len(tr_u))[:n]
    links = np.stack([tr_u[pick], tr_v[pick]], 1).astype(np.int64)
    return dict(A=A, links=links, link_labels=np.asarray(tr_l)[pick].astype(np.int64),
                class_values=np.asarray(cv, dtype=np.float64), h=hops, sample_ratio=1.0, mnph=mnph, recs=[None] * n)
