"""Cases, proofs and checks of the extraction kernels (``igmc_amd/csrc/extract.hip``) on WIDE rating graphs: id spaces of more
than 256 bitmap words a side, fringes of up to 90 000 candidates, batches of more than 256 links.  Shared by the emulator test
(tests/test_emu_extract_wide.py) and the GPU test (tests/test_gpu_extract_wide.py); every function takes a backend ``be`` of
parity_checks.

Every other extraction test runs on graphs of at most 189 bitmap words a side (``IGMC_BLOCK`` is 256: every
``for (w = tid; w < W; w += IGMC_BLOCK)`` loop runs once, the ``running`` carries of ``bm_prefix`` / ``append_fringe`` are never
used) or, on the one wider graph (test_gpu_headline), one hop with cap 100 and fringes of 3 000.  The rows here:

  a  h = 1, cap 100, links on a 90 000-user item     split launch + k_relm; the deciding byte holds > 256 keys: kth_radix
  b  h = 1, ratio 0.5, no cap, the same item         k_count / k_fill on sides of 45 000; radix with a non-zero prefix
  c  h = 1, ratio 0.29, a 70 000- and the 90 000-    the 256-key bound between parking and the radix passes from both sides
     user item
  d  h = 2, cap 20 / ratio 0.29 + cap 40             the non-split body of k_extract_nodes on 3 125 words, sampling at both hops
  e  h = 1, nothing sampled                          k_count / k_fill with 90 000 rows on a side; also against oracle/extract_ref
  f  rows a and d through ``extract_replay``         the twin's node lists replayed == the free run
  g  batches of 300, 513 and 257 links               second and third round of the emission kernels' prefix loops over the batch
                                                     (k_emit; k_emit_nodes, whose node part is read from the lean arena before
                                                     anything emits the CSR over it; k_fill where there is no dense block)
  h  ratios whose double product with the fringe     int(ratio * n) as Python computes it; a side that samples to nothing with
     size falls just under an integer; k = 0         the other kept; both (the hops end)

REFERENCES, both independent of the kernels: ``oracle/extract_cpu.extract_batch`` (the host twin: a plain qsort of the keys,
no bitmaps, no radix) wherever something is sampled, ``oracle/extract_ref`` (pinned to the reference project) where nothing
is.  Everything is integer: every comparison is exact.

PROOFS that a row reached its path are computed on the host from the text of ``include/igmc_rng.h`` restated in numpy
(``sample_salt`` here, ``sampled_candidates_checks.sample_key``) and asserted BEFORE any comparison: per hop-1 draw the
histogram of ``key >> 24`` over the candidate set, the byte that holds the k-th smallest key and that byte's count -- more than
256 is ``kth_radix``, at most 256 the parked list (``sample_fringe``).  A device build has no hook to force either."""
import ctypes
import functools

import numpy as np
import scipy.sparse as ssp

import parity_checks as PC
import sampled_candidates_checks as SC
from igmc_amd import engine
from oracle import extract_cpu
from test_extract_twin import compare

CV = np.arange(1, 6, dtype=np.float64)
SEED, EPOCH = 11, 4
PARK = 256                       # keys of the deciding byte that sample_fringe parks (IGMC_BLOCK); more: kth_radix
HUB = 60000                      # a hop-1 draw over at least this many candidates is a "hub draw"
KEYS = ('node_off', 'n_users', 'node_label', 'node_gid', 'node_graph', 'row_ptr', 'col', 'erel', 'elab', 'eflag', 'y')
QUIET = 16                       # rows of more links than this print a summary, not a line per link and side


# ------------------------------------------------------------------ the salt, from the header's text
def sample_salt(seed, epoch, link, dist, side):
    """``igmc_sample_salt`` of include/igmc_rng.h."""
    s = SC.splitmix64((seed ^ 0x49474D43) & SC.M64)
    s = SC.splitmix64(s ^ epoch)
    s = SC.splitmix64(s ^ link)
    return SC.splitmix64(s ^ ((dist << 1) | side))


# ------------------------------------------------------------------ the graphs
def _finish(name, nu, nv, u, v, rng, **special):
    r = rng.integers(1, 6, len(u)).astype(np.float32)
    A = ssp.csr_matrix(ssp.coo_matrix((r, (u, v)), shape=(nu, nv)))
    A.data = np.clip(np.rint(A.data), 1, 5).astype(np.float32)           # (duplicate pairs were summed)
    A.sort_indices()
    Acsc = A.tocsc()
    Acsc.sort_indices()
    G = dict(name=name, A=A, Acsc=Acsc, nu=nu, nv=nv, Wu=(nu + 31) // 32, Wv=(nv + 31) // 32, prep=extract_cpu.prepare(A),
             max_deg_u=int(np.diff(A.indptr).max()), max_deg_v=int(np.diff(Acsc.indptr).max()), dev={}, links={})
    G.update(special)
    return G


def _wide():
    """100 000 users x 9 000 items, about 300 000 background ratings; the reserved ids below take no background rating, so
    their rows and columns are exactly what is written here."""
    rng = np.random.default_rng(41)
    nu, nv = 100000, 9000
    UH, U4 = 11, 99990                          # rates 8 000 items / exactly 4 items
    H90, H70, I101, IQ = 17, 4242, 8100, 8999   # rated by 90 000 / 70 000 / exactly 101 / exactly 3 users
    u, v = rng.integers(0, nu, 300000), rng.integers(0, nv, 300000)
    keep = ~np.isin(u, [UH, U4]) & ~np.isin(v, [H90, H70, I101, IQ])
    u, v = u[keep], v[keep]
    plain_u = np.setdiff1d(np.arange(nu), [UH, U4])
    plain_v = np.setdiff1d(np.arange(nv), [H90, H70, I101, IQ])
    r90 = np.concatenate([rng.choice(plain_u, 89998, replace=False), [UH, U4]])
    r70 = np.concatenate([rng.choice(plain_u, 69999, replace=False), [UH]])
    r101 = rng.choice(plain_u, 101, replace=False)
    rq = np.concatenate([rng.choice(plain_u, 2, replace=False), [U4]])
    hub_items = np.concatenate([rng.choice(plain_v, 7998, replace=False), [H90, H70]])
    u4_items = rng.choice(plain_v, 2, replace=False)                      # (+ H90 and IQ above: 4 items)
    u = np.concatenate([u, r90, r70, r101, rq, np.full(8000, UH), np.full(2, U4)])
    v = np.concatenate([v, np.full(90000, H90), np.full(70000, H70), np.full(101, I101), np.full(3, IQ), hub_items, u4_items])
    G = _finish('WIDE', nu, nv, u, v, rng, UH=UH, U4=U4, H90=H90, H70=H70, I101=I101, IQ=IQ)
    A, Acsc = G['A'], G['Acsc']
    assert np.diff(Acsc.indptr)[[H90, H70, I101, IQ]].tolist() == [90000, 70000, 101, 3]
    assert np.diff(A.indptr)[[UH, U4]].tolist() == [8000, 4]
    coo = A.tocoo()
    plain = np.flatnonzero(~np.isin(coo.row, [UH, U4]) & ~np.isin(coo.col, [H90, H70, I101, IQ]))
    rnd = [(int(coo.row[p]), int(coo.col[p])) for p in rng.choice(plain, 3, replace=False)]
    a, b = int(r90[0]), int(r90[1])
    L = G['links']
    L['six'] = [(UH, H90), (a, H90), (b, H90)] + rnd                      # 3 hub links + 3 random
    L['two_on_h90'] = [(UH, H90), (a, H90)]
    L['h70_h90'] = [(int(r70[0]), H70), (a, H90)]
    L['hub_two_random'] = [(UH, H90)] + rnd[:2]
    L['i101'] = [(int(r101[0]), I101)]
    L['i101_zero'] = [(int(r101[0]), I101), (U4, H90), (U4, IQ)]          # 100 candidates; (89 999, 3 -> k = 0); (2, 3 -> both 0)
    L['zero'] = [(U4, IQ), (U4, H90)]
    return G


def _many(hub=0):
    """20 000 x 12 000 with 200 000 ratings: narrow rows (dense blocks whatever the cap), batches of more than 256 links.
    ``hub``: one item rated by that many more users -- an uncapped arena then has slots of more than 256 users and no dense
    block, so the batch goes through k_count / k_fill."""
    rng = np.random.default_rng(43)
    nu, nv = 20000, 12000
    u, v = rng.integers(0, nu, 200000), rng.integers(0, nv, 200000)
    if hub:
        u, v = np.concatenate([u, rng.choice(nu, hub, replace=False)]), np.concatenate([v, np.full(hub, 5)])
    G = _finish('MANY_HUB' if hub else 'MANY', nu, nv, u, v, rng)
    coo = G['A'].tocoo()
    G['links']['many'] = [(int(coo.row[p]), int(coo.col[p])) for p in rng.choice(coo.nnz, 513, replace=False)]
    return G


@functools.lru_cache(maxsize=None)
def graphs():
    """Built once per driver module: its module-scoped fixture builds them here and gives them up in ``release``."""
    return dict(WIDE=_wide(), MANY=_many(), MANY_HUB=_many(hub=300))


def release():
    """End of a driver module: the device graphs are closed; the host graphs, twins and downloads are dropped."""
    if graphs.cache_info().currsize:
        for G in graphs().values():
            for g in G['dev'].values():
                g.close()
            G['dev'].clear()
    graphs.cache_clear()
    _twins.clear()
    _free.clear()


# ------------------------------------------------------------------ the rows
def _row(graph, h, mnph, ratio, links, n=None, radix=None, kernels=(), **more):
    return dict(graph=graph, h=h, mnph=mnph, ratio=ratio, links=links, n=n, radix=radix, kernels=set(kernels), **more)


COUNT_FILL = ('k_extract_nodes', 'k_count', 'k_fill')
ROWS = {
    'a': _row('WIDE', 1, 100, 1.0, 'six', radix='above', top_byte_zero=True, kernels=('k_extract_nodes', 'k_relm', 'k_emit')),
    'b': _row('WIDE', 1, None, 0.5, 'two_on_h90', radix='above', every_byte_nonzero=True, kernels=COUNT_FILL),
    'c': _row('WIDE', 1, None, 0.29, 'h70_h90', radix='both', kernels=COUNT_FILL),
    'd_cap20': _row('WIDE', 2, 20, 1.0, 'six', radix='above', hop2_full=True, kernels=('k_extract_nodes', 'k_relm', 'k_emit')),
    'd_ratio_cap40': _row('WIDE', 2, 40, 0.29, 'six', radix='above', hop2_full=True, kernels=('k_extract_nodes', 'k_relm', 'k_emit')),
    'e': _row('WIDE', 1, None, 1.0, 'hub_two_random', oracle=True, kernels=COUNT_FILL),
    'g_300_cap5': _row('MANY', 1, 5, 1.0, 'many', n=300, kernels=('k_relm', 'k_emit')),
    'g_513_cap3_lean': _row('MANY', 1, 3, 1.0, 'many', n=513, lean=True, kernels=('k_relm', 'k_emit_nodes', 'k_emit')),
    'g_257_h2_cap3': _row('MANY', 2, 3, 1.0, 'many', n=257, kernels=('k_relm', 'k_emit')),
    'g_300_nocap': _row('MANY', 1, None, 1.0, 'many', n=300, kernels=('k_relm', 'k_emit')),
    # (k_fill has k_emit's prefix loop over the batch: an item with 300 raters takes the dense block of an uncapped arena away)
    'g_300_nocap_fill': _row('MANY_HUB', 1, None, 1.0, 'many', n=300, kernels=COUNT_FILL),
    # int(ratio * 100) as Python computes it: the double products are 28.999999999999996, 56.99999999999999, 57.99999999999999, 70.0
    'h_029': _row('WIDE', 1, None, 0.29, 'i101_zero', sizes={0: (28, None), 1: (26099, 0), 2: (0, 0)}, kernels=COUNT_FILL),
    'h_057': _row('WIDE', 1, None, 0.57, 'i101', sizes={0: (56, None)}, kernels=COUNT_FILL),
    'h_058': _row('WIDE', 1, None, 0.58, 'i101', sizes={0: (57, None)}, kernels=COUNT_FILL),
    'h_07': _row('WIDE', 1, None, 0.7, 'i101', sizes={0: (70, None)}, kernels=COUNT_FILL),
    # two hops: both fringes empty ends the hops (1 + 1 nodes); one empty does not (hop 2 goes on from the side that is kept)
    'h_029_h2': _row('WIDE', 2, None, 0.29, 'zero', sizes={0: (0, 0)}, hop2_after_empty_side=1, kernels=COUNT_FILL),
}
REPLAYED = ['a', 'd_cap20', 'd_ratio_cap40']        # row f, and the rows run again for the same bits


def links_of(G, row):
    L = G['links'][row['links']]
    return L[:row['n']] if row['n'] else L


def caps(G, row):
    """Slots a side the row can fill (igmc_batch_create's rule), for the twin's buffers."""
    def side(n, opposite_max_deg):
        per = n if row['mnph'] is None else min(row['mnph'], n)
        if row['h'] == 1:
            per = min(per, opposite_max_deg)
        return min(n, 1 + row['h'] * per)
    return side(G['nu'], G['max_deg_v']), side(G['nv'], G['max_deg_u'])


def link_arrays(G, links):
    lu = np.array([l[0] for l in links], np.int32)
    lv = np.array([l[1] for l in links], np.int32)
    lab = np.asarray(G['A'][lu, lv]).ravel().astype(np.int64) - 1
    assert lab.min() >= 0                                       # every link is a rated pair: its entry is removed
    return lu, lv, lab, CV[lab].astype(np.float32)


# ------------------------------------------------------------------ the proofs
def hop1_draws(G, links, ratio, mnph, seed, epoch):
    """Every hop-1 draw of the links that samples (0 < k < n): n candidates, k kept, the top key byte that holds the k-th
    smallest key, how many keys that byte holds, the ids of the k smallest keys."""
    A, Acsc = G['A'], G['Acsc']
    out = []
    for pos, (u0, v0) in enumerate(links):
        for side in (0, 1):
            if side == 0:
                cand = Acsc.indices[Acsc.indptr[v0]:Acsc.indptr[v0 + 1]]
                cand = cand[cand != u0]
            else:
                cand = A.indices[A.indptr[u0]:A.indptr[u0 + 1]]
                cand = cand[cand != v0]
            n = len(cand)
            k = n if ratio >= 1.0 else int(ratio * n)            # util_functions.py:222-229
            if mnph is not None and mnph < k:
                k = mnph
            rec = dict(pos=pos, side=side, n=n, k=k, byte=None, count=None, kept=None, kth=None)
            if 0 < k < n:
                keys = SC.sample_key(sample_salt(seed, epoch, pos, 1, side), cand)
                hist = np.bincount((keys >> np.uint64(24)).astype(np.int64), minlength=256)
                byte = int(np.searchsorted(np.cumsum(hist), k))
                order = np.argsort(keys, kind='stable')
                rec.update(byte=byte, count=int(hist[byte]), kept=np.sort(cand[order[:k]]), kth=int(keys[order[k - 1]]))
            out.append(rec)
    return out


def prove_paths(name, row, G, links, seed, epoch):
    """Host-side proof that the row's draws take the paths it is for; prints what the log must show."""
    draws = hop1_draws(G, links, row['ratio'], row['mnph'], seed, epoch)
    if len(links) <= QUIET:
        for d in draws:
            print('row %s link %d side %d: %d candidates, k = %d, deciding byte %s holds %s keys, k-th key %s' % (
                name, d['pos'], d['side'], d['n'], d['k'], d['byte'], d['count'], d['kth'] if d['kth'] is None else '%08x' % d['kth']))
    else:
        cut = [d for d in draws if d['count'] is not None]
        print('row %s: %d links, %d hop-1 draws of %d to %d candidates, %d of them sampled%s' % (
            name, len(links), len(draws), min(d['n'] for d in draws), max(d['n'] for d in draws), len(cut),
            ', deciding bytes of %d to %d keys' % (min(d['count'] for d in cut), max(d['count'] for d in cut)) if cut else ''))
    assert G['Wu'] > 256 and G['Wv'] > 256, 'not a wide graph'
    hub = [d for d in draws if d['n'] >= HUB and d['count'] is not None]
    if row['radix']:
        assert hub, 'row %s has no hub draw' % name
    if row['radix'] == 'above':
        assert all(d['count'] > PARK for d in hub), 'row %s: a hub draw would be parked, not radix-selected' % name
    if row['radix'] == 'both':
        assert any(d['count'] <= PARK for d in hub) and any(d['count'] > PARK for d in hub), \
            'row %s does not take the park / radix bound from both sides: %s' % (name, [d['count'] for d in hub])
    if row.get('top_byte_zero'):
        assert all(d['byte'] == 0 for d in hub)
    if row.get('every_byte_nonzero'):       # the k-th smallest key IS kth_radix's prefix: a non-zero byte found in every pass
        assert all((d['kth'] >> s) & 255 for d in hub for s in (24, 16, 8, 0)), ['%08x' % d['kth'] for d in hub]
        assert all(d['kth'] >> 24 == d['byte'] for d in hub)
    return draws


# ------------------------------------------------------------------ the backend, the twin, the oracle
def dev_graph(be, G):
    if be.name not in G['dev']:
        G['dev'][be.name] = engine.Graph(G['A'], device=be.device, lib=be.lib)
    return G['dev'][be.name]


def free_run(be, G, row, links, seed, epoch):
    """Free-running extraction of the links on the backend -> (download, names of the kernels that ran)."""
    lu, lv, _, ys = link_arrays(G, links)
    B = len(links)
    b = engine.Batch(dev_graph(be, G), max_graphs=B, hop=row['h'], max_nodes_per_hop=row['mnph'])
    if row.get('lean'):
        b.want_transposed()      # (the node part of the emission runs inside a lean extraction only beside transposed blocks)
        b.set_lean(True)
    dlu, dlv, dly = be.dev(lu), be.dev(lv), be.dev(ys)
    engine.profile_fetch(be.lib, 128)          # (drops what earlier calls left)
    engine.profile_enable(be.lib, True)
    try:
        b.extract(be.ptr(dlu), be.ptr(dlv), be.ptr(dly), None, 0, B, sample_ratio=row['ratio'], seed=seed, epoch=epoch)
        be.sync()
        # a lean arena: what k_emit_nodes left, read BEFORE anything asks for the CSR (info / download emit it, and k_emit
        # writes the node part again)
        nodes = node_part(be, b, B) if row.get('lean') else None
        d = b.download()                       # (a lean arena emits its CSR here)
        d['nodes_before_emit'] = nodes
    finally:
        engine.profile_enable(be.lib, False)
    ran = sorted(n for n, _, c in engine.profile_fetch(be.lib, 128) if c > 0)
    b.close()
    return d, ran


def peek(be, ptr, n, dtype):
    """Copy of ``n`` elements at an address of the backend's memory."""
    dt = np.dtype(dtype)
    assert ptr
    if be.name == 'gpu':
        class View(object):
            pass
        v = View()
        v.__cuda_array_interface__ = dict(shape=(int(n),), typestr=dt.str, data=(int(ptr), False), version=2)
        return be.torch.as_tensor(v, device='cuda').cpu().numpy().copy()
    return np.frombuffer((ctypes.c_uint8 * (n * dt.itemsize)).from_address(ptr), dt).copy()


def node_part(be, b, B):
    """The node part of the collated batch as it stands in the arena: totals, batch offsets, per-node label / id / graph."""
    totals = peek(be, b.device_ptr('TOTALS'), 6, np.int32)
    N = int(totals[0])
    assert 0 < N <= b.node_capacity and totals[2] == 0, totals
    return dict(totals=totals, node_off=peek(be, b.device_ptr('NODE_OFF'), B + 1, np.int32),
                n_users=peek(be, b.device_ptr('N_USERS'), B, np.int32), node_label=peek(be, b.device_ptr('NODE_LABEL'), N, np.uint8),
                node_gid=peek(be, b.device_ptr('NODE_GID'), N, np.int32), node_graph=peek(be, b.device_ptr('NODE_GRAPH'), N, np.int32))


def replay_run(be, G, row, links, twin):
    _, _, _, ys = link_arrays(G, links)
    b = engine.Batch(dev_graph(be, G), max_graphs=len(links), hop=row['h'], max_nodes_per_hop=row['mnph'])
    ul, vl = [t[0] for t in twin], [t[1] for t in twin]
    ud = [[t[2][int(i)] // 2 for i in t[0]] for t in twin]
    vd = [[t[3][int(i)] // 2 for i in t[1]] for t in twin]
    b.extract_replay(ul, vl, ud, vd, ys)
    be.sync()
    d = b.download()
    b.close()
    return d


_twins, _free = {}, {}


def twin_of(name, G, row, links, seed, epoch):
    key = (name, seed, epoch)
    if key not in _twins:
        lu, lv, _, _ = link_arrays(G, links)
        cap_u, cap_v = caps(G, row)
        _twins[key] = extract_cpu.extract_batch(G['prep'], lu, lv, 0, len(links), hop=row['h'], sample_ratio=row['ratio'],
                                                max_nodes_per_hop=row['mnph'], seed=seed, epoch=epoch, cap_u=cap_u, cap_v=cap_v)
    return _twins[key]


def free_of(be, name, G, row, links, seed, epoch):
    key = (be.name, name, seed, epoch)
    if key not in _free:
        _free[key] = free_run(be, G, row, links, seed, epoch)
    return _free[key]


def compare_with_oracle(d, G, row, links):
    """Nothing is sampled: node sets, labels and induced edges of ``oracle/extract_ref`` (pinned to the reference)."""
    from helpers import graph_canonical
    from oracle import extract_ref as X
    _, _, lab, _ = link_arrays(G, links)
    for g, (i, j) in enumerate(links):
        users, items, ulab, vlab, edges = graph_canonical(d, g)
        u, v, r, labels, _, y, _, (un, vn) = X.subgraph_extraction_labeling((i, j), G['A'], G['Acsc'], row['h'], 1.0, None, None,
                                                                             None, CV, lab[g])
        assert users[0] == un[0] and items[0] == vn[0]
        assert sorted(users.tolist()) == sorted(un) and sorted(items.tolist()) == sorted(vn), 'node sets of link %d' % g
        assert ulab == dict(zip(un, labels[:len(un)])) and vlab == dict(zip(vn, labels[len(un):])), 'labels of link %d' % g
        assert np.array_equal(X.canonical_edges(un, vn, u, v, r), edges), 'induced edges of link %d' % g
        assert d['y'][g] == np.float32(y)


# ------------------------------------------------------------------ the checks
def check_row(be, name, seed=SEED, epoch=EPOCH):
    """One row: proofs of the path, free-running extraction on the backend, the twin, every link compared."""
    row = ROWS[name]
    G = graphs()[row['graph']]
    links = links_of(G, row)
    B = len(links)
    if row['n']:
        assert B == row['n'] and B > 256
    draws = prove_paths(name, row, G, links, seed, epoch)
    twin = twin_of(name, G, row, links, seed, epoch)
    assert len(twin) == B
    if B <= QUIET:
        for g, t in enumerate(twin):
            print('row %s link %d (%d, %d): %d users, %d items, %d induced ratings' % (name, g, links[g][0], links[g][1], len(t[0]),
                                                                                     len(t[1]), len(t[4])))
    else:
        print('row %s: sides of %d to %d users and %d to %d items, %d induced ratings in all' % (
            name, min(len(t[0]) for t in twin), max(len(t[0]) for t in twin), min(len(t[1]) for t in twin),
            max(len(t[1]) for t in twin), sum(len(t[4]) for t in twin)))
    # the restated salt and key are the header's: the k smallest keys ARE the twin's hop-1 fringe
    for dr in draws:
        t = twin[dr['pos']]
        hop1 = sorted(i for i, l in t[2 + dr['side']].items() if l // 2 == 1)
        assert len(hop1) == dr['k'], (name, dr['pos'], dr['side'], len(hop1), dr['k'])
        if dr['kept'] is not None:
            assert hop1 == dr['kept'].tolist()
    for pos, (ku, kv) in row.get('sizes', {}).items():
        assert len(twin[pos][0]) == 1 + ku, (name, pos, len(twin[pos][0]))
        if kv is not None:
            assert len(twin[pos][1]) == 1 + kv, (name, pos, len(twin[pos][1]))
    if row.get('hop2_full'):           # sampling at the second hop too: some side's hop-2 fringe was cut to the cap
        assert any(sum(1 for l in t[s].values() if l // 2 == 2) == row['mnph'] for t in twin for s in (2, 3))
    if 'hop2_after_empty_side' in row:  # hop 1 kept users only; hop 2 went on and found items
        t = twin[row['hop2_after_empty_side']]
        assert sum(1 for l in t[3].values() if l // 2 == 1) == 0 and sum(1 for l in t[2].values() if l // 2 == 1) > 0
        assert sum(1 for l in t[3].values() if l // 2 == 2) > 0 and sum(1 for l in t[2].values() if l // 2 == 2) == 0
    d, ran = free_of(be, name, G, row, links, seed, epoch)
    print('row %s on %s: kernels %s' % (name, be.name, ', '.join(ran)))
    assert row['kernels'] <= set(ran), 'row %s: %s did not run (ran: %s)' % (name, sorted(row['kernels'] - set(ran)), ran)
    assert d['B'] == B
    _, _, _, ys = link_arrays(G, links)
    assert np.array_equal(d['y'], ys)
    PC.check_batch_structure(d, 2 * row['h'] + 2)
    compare(d, None, twin)
    if row.get('lean'):                # k_emit_nodes' own output (the download above came after k_emit had written it again)
        pre = d['nodes_before_emit']
        assert pre['totals'].tolist() == [d['N'], d['E'], 0, B, d['N'], d['E']], pre['totals']
        for k in ('node_off', 'n_users', 'node_label', 'node_gid', 'node_graph'):
            assert np.array_equal(pre[k], d[k]), 'row %s: %s as k_emit_nodes left it is not the checked batch' % (name, k)
    if row.get('oracle'):
        compare_with_oracle(d, G, row, links)
    return d, twin


def check_replay(be, name, seed=SEED, epoch=EPOCH):
    """Row f: the twin's node lists through ``extract_replay`` (the non-split body also at one hop): the twin's subgraphs again,
    and the free run's batch byte for byte."""
    row = ROWS[name]
    G = graphs()[row['graph']]
    links = links_of(G, row)
    twin = twin_of(name, G, row, links, seed, epoch)
    d = replay_run(be, G, row, links, twin)
    PC.check_batch_structure(d, 2 * row['h'] + 2)
    compare(d, None, twin)
    free, _ = free_of(be, name, G, row, links, seed, epoch)
    for k in KEYS:
        assert np.array_equal(d[k], free[k]), 'replay of row %s differs from the free run in %s' % (name, k)


def check_same_bits(be, name, seed=SEED, epoch=EPOCH):
    """The same (seed, epoch) again: byte-equal downloads.  Another epoch: other nodes on every hub link (and the twin's)."""
    row = ROWS[name]
    G = graphs()[row['graph']]
    links = links_of(G, row)
    first, _ = free_of(be, name, G, row, links, seed, epoch)
    again, _ = free_run(be, G, row, links, seed, epoch)
    for k in KEYS:
        assert again[k].tobytes() == first[k].tobytes(), 'row %s: a second launch differs in %s' % (name, k)
    other, _ = free_run(be, G, row, links, seed, epoch + 1)
    twin = twin_of(name, G, row, links, seed, epoch + 1)
    compare(other, None, twin)
    hubs = [g for g, (_, v0) in enumerate(links) if v0 in (G['H90'], G['H70'])]
    assert hubs
    for g in hubs:
        lo, hi = first['node_off'][g], first['node_off'][g + 1]
        lo2, hi2 = other['node_off'][g], other['node_off'][g + 1]
        assert not np.array_equal(first['node_gid'][lo:hi], other['node_gid'][lo2:hi2]), 'row %s link %d: epoch %d draws the nodes of epoch %d' % (name, g, epoch + 1, epoch)
