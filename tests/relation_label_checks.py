"""The model step across the (relation count R, label count L = 2 hops + 2) plane, shared by
tests/test_emu_relation_labels.py (host emulation of the HIP sources) and tests/test_gpu_relation_labels.py (the gfx950
library).

The step planner (``igmc_step_plan``, step_plan.h; ``igmc_g2_layout``, g2_compose.h; ``g2_groups``, g2_image.h) picks
kernels, weight-image layouts, table sizes and tails from R and L, mostly through ``rows0 = R L + L + 1``, the rows of the
layer-0 table:

* R <= 5, L <= 8, rows0 <= 32: the subgraph kernel / the narrow dense layers, a 32-row layer-0 table;
* rows0 of 33 .. 48 or R of 6 .. 10: the two-group dense kernels, a 64-row table; the split is in the relations
  (``g2_rel_groups(R) == 2``: gsplit) or only in the table;
* R L <= 20: the narrow dense layers may leave relation-space tables (``dl_ts_eligible``);
* R <= 8: ``fts``; 4 R <= IGMC_FOLD_NA with L layer-0 mains: ``k_tail_fin``, whose row producers come in sets of 16 of the
  8 (R + 1) float4 columns (R = 1: none; R = 2, 4: a half-filled last set);
* R > 10, rows0 > 48 or L > 8: the row walkers.

tests/geometry_cases.py stays on MovieLens-shaped graphs at R = 5 and 10 with L = 4 (one row at L = 6).  Here ROWS has one
row on each side of every threshold above, on crafted multi-ring rating graphs (``ring_graph``) whose ``hops``-hop subgraphs
carry every label 0 .. 2 hops + 1 and every relation, at extents on both sides of the 16-row bundle and the 32-column k-step.
Per row, with and without edge dropout: the extraction gave the crafted extents, labels and relations; the geometry is the
table's; eval outputs, train outputs, loss and every gradient tensor against ``oracle/pyg_ref`` at the parity tolerances of
tests/parity_checks.py (``check_row``).  ``TRAJECTORIES``: steps with Adam, one per distinct tail (``check_trajectory``), and
for the one-launch tail the same bits as the two-launch tail (``check_tail_fold``)."""
import collections

import numpy as np
import scipy.sparse as ssp

import geometry_cases as GC
import parity_checks as PC
from igmc_amd import engine

HOOKS = ('IGMC_GRAPH_STEP', 'IGMC_GS_CLUSTER', 'IGMC_GS_GRID', 'IGMC_DL', 'IGMC_DL_ALWAYS', 'IGMC_DL_FUSED', 'IGMC_DL_TS',
         'IGMC_DL_GSPLIT', 'IGMC_DL_HEAD', 'IGMC_FIN_MODE', 'IGMC_TAIL_FOLD', 'IGMC_L3_VEC')
# the kernel that marks each family in the step's launches (tests/test_gpu_geometry.py)
MARKER = {'subgraph': 'k_graph_step', 'dense_fused': 'k_dl_fwd', 'dense_layer': 'k_dl_layer_fwd', 'rows': 'k_rgcn_layer_fwd'}
OUT_PAD = 8


# ====================================================================== crafted multi-ring rating graphs
def ring_graph(blocks, R, seed=20):
    """Rating matrix of disjoint blocks, one per link.  ``blocks``: ``[(U, V, density)]`` with the ring sizes ``U = (U_1 .. U_H)``
    and ``V = (V_1 .. V_H)`` of a side; ``U_0`` = {target user} and ``V_0`` = {target item} (the block's first user and item,
    which rate each other).  A rating between ``U_a`` and ``V_b`` exists only where ``|a - b| <= 1``; every user of ``U_h``
    (h >= 1) rates an item of ``V_{h-1}`` and every item of ``V_h`` is rated by a user of ``U_{h-1}``; the other allowed pairs are
    rated with probability ``density``; ratings cycle through all ``R`` values.  The uncapped H-hop subgraph of the block's link
    is then the whole block, ring h at distance h: label 2 h on the user side, 2 h + 1 on the item side.
    -> (csr matrix with values 1 .. R, links [n, 2])"""
    rng = np.random.default_rng(seed)
    rows, cols, vals, links = [], [], [], []
    u0 = v0 = 0
    for k, (U, V, dens) in enumerate(blocks):
        U, V = [1] + [int(x) for x in U], [1] + [int(x) for x in V]
        assert len(U) == len(V), (U, V)
        H = len(U) - 1
        for h in range(1, H + 1):       # a ring is reached through the ring before it on the OTHER side
            assert (U[h] == 0 or V[h - 1] > 0) and (V[h] == 0 or U[h - 1] > 0), (U, V)
        nu, nv = sum(U), sum(V)
        ru, rv = np.repeat(np.arange(H + 1), U), np.repeat(np.arange(H + 1), V)      # ring of every user / item
        ou, ov = np.concatenate([[0], np.cumsum(U)]), np.concatenate([[0], np.cumsum(V)])
        allowed = np.abs(ru[:, None] - rv[None, :]) <= 1
        m = (rng.random((nu, nv)) < dens) & allowed
        m[0, 0] = True
        for h in range(1, H + 1):
            for t in range(U[h]):
                m[ou[h] + t, ov[h - 1] + t % V[h - 1]] = True
            for t in range(V[h]):
                m[ou[h - 1] + t % U[h - 1], ov[h] + t] = True
        assert not (m & ~allowed).any()
        i, j = np.nonzero(m)
        rows.append(u0 + i)
        cols.append(v0 + j)
        vals.append(1 + (i * nv + j + k) % R)
        links.append((u0, v0))
        u0 += nu
        v0 += nv
    A = ssp.csr_matrix((np.concatenate(vals).astype(np.float32), (np.concatenate(rows), np.concatenate(cols))),
                       shape=(u0, v0))
    return A, np.array(links, np.int64)


def rings(n, hops, mnph):
    """``n`` nodes of a side (the target among them) as ring sizes: as even as ``hops`` rings allow, the nearer rings first."""
    q, r = divmod(n - 1, hops)
    sizes = tuple(q + (1 if h < r else 0) for h in range(hops))
    assert max(sizes) <= mnph, 'a ring of %d nodes is cut by the per-hop cap %d' % (max(sizes), mnph)
    return sizes


def blocks_of(extents, hops, mnph, density=0.6):
    """Blocks of the given extents ``(users, items)`` a side, each side's nodes spread over ``hops`` rings.  An extent of one
    node on a side leaves the other side its first ring only (ring 2 is reached through ring 1 of the other side)."""
    out = []
    for nu, nv in extents:
        U, V = rings(nu, hops, mnph), rings(nv, hops, mnph)
        if nu == 1 or nv == 1:
            assert max(nu, nv) - 1 <= mnph, (nu, nv, mnph)
            U, V = (nu - 1,) + (0,) * (hops - 1), (nv - 1,) + (0,) * (hops - 1)
        out.append((U, V, density))
    return out


def make_case(blocks, R, hops, mnph):
    """Parity case (tests/parity_checks.py) of the blocks' links on their ring graph; link k is rated ``1 + k % R``."""
    A, links = ring_graph(blocks, R)
    n = len(links)
    return dict(A=A, links=links, link_labels=(np.arange(n) % R).astype(np.int64),
                class_values=np.arange(1, R + 1, dtype=np.float64), h=hops, sample_ratio=1.0, mnph=mnph, recs=[None] * n)


def check_batch(d, blocks, R, hops, first=0):
    """Host assertions on a downloaded batch, before any model number: subgraph g is block ``first + g`` ring by ring, the batch
    carries every label 0 .. 2 hops + 1 and every relation 0 .. R - 1."""
    B = d['B']
    assert first + B <= len(blocks)
    want_u = [1 + sum(blocks[first + g][0]) for g in range(B)]
    want_n = [2 + sum(blocks[first + g][0]) + sum(blocks[first + g][1]) for g in range(B)]
    assert [int(x) for x in d['n_users']] == want_u, (list(d['n_users']), want_u)
    assert [int(x) for x in np.diff(d['node_off'])] == want_n, (np.diff(d['node_off']).tolist(), want_n)
    lab = d['node_label']
    for g in range(B):
        c = np.bincount(lab[d['node_off'][g]:d['node_off'][g + 1]], minlength=2 * hops + 2)
        U, V = blocks[first + g][0], blocks[first + g][1]
        want = [1, 1] + [x for h in range(hops) for x in (U[h], V[h])]
        assert c.tolist() == want, 'subgraph %d: nodes per label %s, crafted %s' % (g, c.tolist(), want)
    return set(int(x) for x in np.unique(lab)), set(int(x) for x in np.unique(d['erel']))


def assert_covers(labels, rels, R, hops):
    assert labels == set(range(2 * hops + 2)), 'labels of the batch: %s' % sorted(labels)
    assert rels == set(range(R)), 'relations of the batch: %s' % sorted(rels)


# ====================================================================== the table
def X(family, wg=0, groups=1, gsplit=0, tables=1, dl_bwd=0):
    """Expected subset of ``ModelWorkspace.step_geometry`` (the keys ``history_checks.Crafted.assert_geometry`` takes)."""
    if family == 'rows':
        groups, tables = 0, 0
    return dict(family=family, wg_per_graph=wg, groups=groups, gsplit=gsplit, tables=tables, dl_bwd=dl_bwd)


SUBGRAPH = X('subgraph', wg=4)                               # 4 workgroups per subgraph (B <= 56), tables through its tail
TABLE64 = X('dense_fused', groups=2, gsplit=0, dl_bwd=1)     # 64-row table, one group of relations: group after group
GSPLIT = X('dense_fused', groups=2, gsplit=1, dl_bwd=1)      # two groups of relations, both at once
NARROW = X('dense_fused', dl_bwd=1)                          # the narrow dense layers with relation-space tables
NARROW_BS = X('dense_fused', tables=0, dl_bwd=0)             # R L > 20: no tables, the basis-space tail
WALKERS = X('rows')

Row = collections.namedtuple('Row', 'id R hops mnph extents geometry')
MNPH = {1: 40, 2: 20, 3: 13, 4: 10}          # slots of 41, 41, 40 and 41 nodes a side


def slot(hops, mnph):
    return 1 + hops * mnph


def small_extents(hops, mnph, free=(25, 9)):
    """Eight subgraphs: 1 x 1, 2 x 3, one user and as many items as one ring takes, both sides of the 16-row bundle and of the
    32-column k-step, the full slot, one free."""
    s = slot(hops, mnph)
    return [(1, 1), (2, 3), (1, 1 + mnph), (17, 16), (16, 33), (33, 40), (s, s), free]


def row(R, hops, geometry, mnph=None, extents=None, tag=''):
    mnph = mnph or MNPH[hops]
    return Row('r%d_h%d%s' % (R, hops, tag), R, hops, mnph, extents or small_extents(hops, mnph), geometry)


BIG = [(65, 64), (101, 127)]         # slots of 127 a side: every member of a cluster of four is active
ROWS = [
    # ---- the subgraph kernel: rows0 = 9, 13, 21 (L = 4), 25, 31 (L = 6; 31 is the last that fits), 17, 25 (L = 8)
    row(1, 1, SUBGRAPH), row(2, 1, SUBGRAPH), row(4, 1, SUBGRAPH),
    row(3, 2, SUBGRAPH), row(4, 2, SUBGRAPH),
    row(1, 3, SUBGRAPH), row(2, 3, SUBGRAPH),
    row(4, 2, SUBGRAPH, mnph=63, extents=BIG, tag='_slot127'), row(2, 3, SUBGRAPH, mnph=42, extents=BIG, tag='_slot127'),
    # ---- a 64-row table through rows0 = 37, 33, 41 at R <= 5: the second group holds no relation
    row(5, 2, TABLE64), row(3, 3, TABLE64), row(4, 3, TABLE64),
    # ---- a partly filled second relation group: rows0 = 29, 33, 37, 41 (R = 9: beyond fts) and 43
    row(6, 1, GSPLIT), row(7, 1, GSPLIT), row(8, 1, GSPLIT), row(9, 1, GSPLIT), row(6, 2, GSPLIT),
    # ---- the first configuration beyond each limit: R = 11, rows0 = 49 twice, L = 10
    row(11, 1, WALKERS), row(7, 2, WALKERS), row(5, 3, WALKERS), row(2, 4, WALKERS),
    # ---- the narrow dense layers, on slots of 129 (130) a side, which the subgraph kernel does not take: R L = 20 (control),
    #      24 (no tables), 18 and 16
    row(5, 1, NARROW, mnph=128, extents=small_extents(1, 128, free=(65, 97)), tag='_slot129'),
    row(4, 2, NARROW_BS, mnph=64, extents=small_extents(2, 64, free=(65, 97)), tag='_slot129'),
    row(3, 2, NARROW, mnph=64, extents=small_extents(2, 64, free=(65, 97)), tag='_slot129'),
    row(2, 3, NARROW, mnph=43, extents=small_extents(3, 43, free=(65, 97)), tag='_slot130'),
]
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


def geometry_kinds(reached):
    """``geometry_cases.geometry_kinds`` of ``[(geometry, B, labels)]`` plus the label counts the subgraph kernel ran at."""
    kinds = GC.geometry_kinds([(g, B) for g, B, _ in reached])
    kinds |= {'subgraph_L%d' % L for g, _, L in reached if g['family'] == 'subgraph'}
    return kinds


REQUIRED_KINDS = {'subgraph', 'wg4', 'subgraph_L4', 'subgraph_L6', 'subgraph_L8', 'dense_fused', 'dense_fused_tables1',
                  'dense_fused_tables0', 'groups_gsplit0', 'groups_gsplit1', 'rows'}


def expected_kinds():
    """What the table covers if every row gives the geometry it lists."""
    return geometry_kinds([(dict(r.geometry, grid=4 * 8), len(r.extents), 2 * r.hops + 2) for r in ROWS])


# ====================================================================== one row on a backend
def row_case(r, times=1, n=None):
    blocks = blocks_of(r.extents, r.hops, r.mnph) * times
    blocks = blocks[:n] if n else blocks
    return blocks, make_case(blocks, r.R, r.hops, r.mnph)


def assert_geometry(geo, r, what=''):
    for k, v in r.geometry.items():
        assert geo[k] == v, (r.id, what, k, v, geo)


def precheck(be, r, blocks, case):
    """The extraction's batch against the crafted blocks and the geometry against the table, on an arena and a workspace of
    their own, before any model number exists."""
    B = len(blocks)
    g, b, d = PC.extract_case(be, case, replay=False)
    ws = engine.ModelWorkspace(be.lib, be.device, r.R, 4, 2 * r.hops + 2, 0, b.node_capacity, b.edge_capacity, B)
    try:
        assert d['B'] == B
        assert b.node_capacity == 2 * B * slot(r.hops, r.mnph), (b.node_capacity, B, slot(r.hops, r.mnph))
        assert_covers(*check_batch(d, blocks, r.R, r.hops), R=r.R, hops=r.hops)
        geo = ws.step_geometry(b, B)
        assert_geometry(geo, r, 'before the step')
    finally:
        ws.close()
        b.close()
    return geo


def tensor_errors(res):
    """{tensor: max error relative to the reference tensor's peak} of a ``run_model_parity`` result."""
    return {k: float(np.abs(res['grads'][k] - rg).max() / max(np.abs(rg).max(), 1e-6)) for k, rg in res['oracle'][2].items()}


def check_row(be, r, drop, kernels=False):
    """One row, one mask form.  ``kernels``: also the kernels that launched against the family (device).
    -> (geometry, figures)"""
    blocks, case = row_case(r)
    B = len(blocks)
    precheck(be, r, blocks, case)
    seen = {}

    def around_step(ws, batch, n):
        seen['geometry'] = ws.step_geometry(batch, n)
        assert_geometry(seen['geometry'], r, 'at the step')
        if not kernels:
            return None
        engine.profile_fetch(be.lib, 128)          # (drops what earlier calls left)
        engine.profile_enable(be.lib, True)

        def after():
            be.sync()
            seen['kernels'] = {name for name, _, _ in engine.profile_fetch(be.lib, 128)}
            engine.profile_enable(be.lib, False)
        return after

    try:
        res = PC.run_model_parity(be, case, R=r.R, use_dropout=drop, out_pad=OUT_PAD, on_step=around_step)
    finally:
        if kernels:
            engine.profile_enable(be.lib, False)
    geo = seen['geometry']
    assert res['d']['B'] == B
    rl, ro, _ = res['oracle']
    errs = tensor_errors(res)
    worst = max(errs, key=errs.get)
    fig = dict(row=r.id, backend=be.name, R=r.R, L=2 * r.hops + 2, B=B, N=int(res['d']['N']), E=int(res['d']['E']),
               dropout=bool(drop), family=geo['family'], eval_out_rel=res['eval_err'],
               train_out_rel=PC.rel_err(res['train_out'], ro),
               loss_rel=abs(float(res['loss'][0]) - rl) / max(abs(rl), 1e-12), worst_grad_rel=errs[worst],
               worst_grad_tensor=worst)
    fig.update({k.replace('.', '_') + '_rel': v for k, v in sorted(errs.items()) if k.startswith('convs.0.')})
    PC.record_observed('relation_label_parity', **fig)
    print('%s dropout=%d: %s' % (r.id, drop, '  '.join('%s=%.3e' % (k, v) for k, v in sorted(errs.items())
                                                      if k.startswith('convs.0.'))))
    assert errs[worst] < PC.GRAD_TOL, '%s: worst gradient tensor %s, %.3e of its peak' % (r.id, worst, errs[worst])
    if kernels:
        names = seen['kernels']
        assert MARKER[geo['family']] in names, (geo['family'], sorted(names))
        for fam, k in MARKER.items():
            if fam != geo['family']:
                assert k not in names, (geo['family'], k, sorted(names))
        assert ('k_tail_ts' in names) == bool(geo['tables']), sorted(names)
        assert ('k_dl_bwd' in names) == bool(geo['dl_bwd']), sorted(names)
    return geo, fig


# ====================================================================== steps with Adam, one per distinct tail
SIZES = [6, 6, (3, 'train_step'), 2]
# (row, the tail it is here for, compared with the two-launch tail)
TRAJECTORIES = [
    ('r1_h1', 'k_tail_fin without row producers', True),
    ('r4_h2', 'k_tail_fin with 6 layer-0 mains', True),
    ('r2_h3', 'k_tail_fin with 8 layer-0 mains', True),
    ('r6_h1', 'k_tail_ts -> k_finalize_ts behind a partly filled group', False),
    ('r9_h1', 'the same beyond fts', False),
    ('r3_h3', 'a 64-row table at R <= 5', False),
    ('r4_h2_slot129', 'the narrow dense layers without tables: the basis-space tail', False),
    ('r11_h1', 'row walkers and k_finalize', False),
    ('r5_h3', 'row walkers and k_finalize at L = 8', False),
]


def run_trajectory(be, r, profile=False):
    """``SIZES`` steps on 18 links (the row's blocks three times) against ``pyg_ref.train_step`` + torch Adam: the ``TRAJ_*``
    assertions of ``parity_checks.run_fused_train_trajectory``; every step's batch and geometry against the table."""
    blocks, case = row_case(r, times=3, n=18)
    labels, rels, first = set(), set(), 0
    g = engine.Graph(case['A'], device=be.device, lib=be.lib)
    b = engine.Batch(g, max_graphs=6, hop=r.hops, max_nodes_per_hop=r.mnph)
    try:
        lu, lv = be.dev(case['links'][:, 0].astype(np.int32)), be.dev(case['links'][:, 1].astype(np.int32))
        ly = be.dev(case['class_values'][case['link_labels']].astype(np.float32))
        for s in SIZES:
            n = s if isinstance(s, int) else s[0]
            b.extract(be.ptr(lu), be.ptr(lv), be.ptr(ly), None, first, n, sample_ratio=1.0, seed=2, epoch=1)
            be.sync()
            la, re = check_batch(b.download(), blocks, r.R, r.hops, first)
            labels |= la
            rels |= re
            first += n
    finally:
        b.close()
    assert_covers(labels, rels, r.R, r.hops)
    names = None
    if profile:
        engine.profile_fetch(be.lib, 128)
        engine.profile_enable(be.lib, True)
    try:
        res = PC.run_fused_train_trajectory(be, case, r.R, use_dropout=True, sizes=SIZES)
        if profile:
            be.sync()
            names = {name for name, _, _ in engine.profile_fetch(be.lib, 128)}
    finally:
        if profile:
            engine.profile_enable(be.lib, False)
    assert len(res['geometries']) == len(SIZES)
    for geo in res['geometries']:
        assert_geometry(geo, r, 'trajectory')
    return res, names


def check_trajectory(be, r):
    res, _ = run_trajectory(be, r)
    assert res['frac_off'] < PC.TRAJ_FRAC_OFF and res['max_diff'] <= PC.TRAJ_P_MAX
    return res


def check_tail_fold(be, r, monkeypatch, first=None):
    """The trajectory with the one-launch tail (``first``: its result, if it ran already) and once more under
    ``IGMC_TAIL_FOLD=0``: parameters, both Adam moments and the losses byte for byte."""
    monkeypatch.delenv('IGMC_TAIL_FOLD', raising=False)
    new, k_new = run_trajectory(be, r, profile=True) if first is None else first
    monkeypatch.setenv('IGMC_TAIL_FOLD', '0')
    old, k_old = run_trajectory(be, r, profile=True)
    assert 'k_tail_fin' in k_new and 'k_tail_fin' not in k_old and 'k_tail_ts' in k_old, (sorted(k_new), sorted(k_old))
    for k in ('params', 'm1', 'm2'):
        assert new[k].tobytes() == old[k].tobytes(), '%s: %s differs between the one-launch and the two-launch tail' % (r.id, k)
    a, c = np.array([x for x, _ in new['losses']], np.float64), np.array([x for x, _ in old['losses']], np.float64)
    assert a.tobytes() == c.tobytes(), (r.id, a, c)
    assert not np.array_equal(new['params'], PC.flatten_params(new['ws'], PC.make_ref_model(2 * r.hops + 2, r.R, seed=4)))
    return new
