"""Cases, numpy references and checks of ``igmc_loo_count`` / ``igmc_loo_fill`` / ``igmc_loo_deltas``
(igmc_amd/csrc/explain.hip), shared by the emulator test (tests/test_emu_explain.py) and the GPU test
(tests/test_gpu_explain.py).  Every function takes a backend ``be`` of parity_checks (``EmuBackend`` / ``GpuBackend``).

All comparisons are exact.  The variants of a link are built in numpy from the DOWNLOADED base arena (ids and labels of its
nodes in slot order), so the check is "copy the list, leave one element out" stated a second time, not the kernel against
itself; ``var_rating`` is looked up in the scipy matrix.

THE GRAPH (:func:`corner_graph`): ``helpers.random_rating_graph`` in the block behind K = 8 hand-placed corner rows and
columns; corner row k and corner column k hold ``DEGS[k]`` entries, the K x K corner block is empty.  The link (k, j) of
the corner block therefore has ``nu = 1 + DEGS[j]`` users and ``nv = 1 + DEGS[k]`` items at hop 1 without a cap: 1 (no
neighbour on that side), 2, 63 / 64 / 65 (the wave of the copy loop) and 255 / 256 / 257 (the workgroup width), and (0, 0) is
the link with the base variant only.  The longest row makes the uncapped arena's slots wider than 256 nodes a side: that
arena has no dense blocks.  With ``max_nodes_per_hop = 100`` the same graph gives an arena WITH dense blocks (the long rows
are sampled down to 101 nodes), taken lean and not lean; two hops with a cap of 10 bind on nearly every link and bring in
users that share no entry with the target item (``var_rating`` 0)."""
import os

import numpy as np
import scipy.sparse as ssp

from helpers import random_rating_graph
from igmc_amd import engine

P = engine._p
DEGS = [0, 1, 62, 63, 64, 254, 255, 256]
K = len(DEGS)
W = max(DEGS)
ERR_VAR, ERR_UENT, ERR_VENT, ERR_OFFSETS, ERR_EMPTY = 1, 2, 4, 8, 16


def corner_graph():
    M = np.zeros((K + W, K + W), np.float32)
    M[K:, K:] = random_rating_graph(W, W, 0.05, 5, 17).toarray()
    for k, L in enumerate(DEGS):
        M[k, K:K + L] = 1 + (np.arange(L) * 3 + k) % 5
        M[K:K + L, k] = 1 + (np.arange(L) * 2 + k) % 5
    A = ssp.csr_matrix(M)
    A.eliminate_zeros()
    assert [A[k].nnz for k in range(K)] == DEGS and [A[:, k].nnz for k in range(K)] == DEGS
    return A


def corner_links():
    """64 links: the diagonal of the corner block first (every size on both sides, (0, 0) the empty one), then the rest of the
    block with a few RATED pairs of the random block in between."""
    A = corner_graph()
    rows, cols = A[K:, K:].nonzero()
    pairs = [(k, k) for k in range(K)]
    rest = [(k, j) for k in range(K) for j in range(K) if k != j]
    for i, p in enumerate(rest):
        pairs.append(p)
        if i % 5 == 0:
            pairs.append((K + int(rows[7 * i]), K + int(cols[7 * i])))
    return np.asarray(pairs[:64], np.int32)


def base_arena(be, g, links, hop, mnph, lean, B, first=0):
    """An arena holding the extraction of ``links[first:first + B]`` (not downloaded: a lean arena has emitted nothing)."""
    b = engine.Batch(g, B, hop, mnph)
    if lean:
        b.set_lean(True)
    lu, lv = be.dev(links[:, 0].copy()), be.dev(links[:, 1].copy())
    ly = be.dev(np.zeros(len(links), np.float32))
    _, ran = profiled(be, lambda: b.extract(be.ptr(lu), be.ptr(lv), be.ptr(ly), None, first, B, sample_ratio=1.0, seed=3, epoch=5))
    b.dense = 'k_relm' in ran          # (arenas without dense blocks induce their edges with k_count / k_fill)
    assert b.dense != ('k_fill' in ran)
    if b.dense:
        assert ('k_emit' in ran) != bool(lean)
    return b


def node_lists(d):
    """Per link of a downloaded arena: (user ids, user labels, item ids, item labels) in slot order."""
    out = []
    for g in range(d['B']):
        lo, hi, nu = int(d['node_off'][g]), int(d['node_off'][g + 1]), int(d['n_users'][g])
        out.append((d['node_gid'][lo:lo + nu], d['node_label'][lo:lo + nu], d['node_gid'][lo + nu:hi], d['node_label'][lo + nu:hi]))
    return out


def closed_forms(nu, nv):
    return nu + nv - 1, nu + (nu - 1) * (nu - 1) + (nv - 1) * nu, nv + (nu - 1) * nv + (nv - 1) * (nv - 1)


def reference_variants(lists, A, link0=0):
    """The variants of every link in the documented order, in numpy: the six cache arrays and the four per-variant arrays."""
    A = ssp.csr_matrix(A)
    uoff, voff, un, ud, vn, vd = [0], [0], [], [], [], []
    link, side, node, rating = [], [], [], []
    for g, (U, UL, V, VL) in enumerate(lists):
        nu, nv = len(U), len(V)
        variants = [(255, 0)] + [(0, j) for j in range(1, nu)] + [(1, j) for j in range(1, nv)]
        for s, j in variants:
            ku = np.ones(nu, bool)
            kv = np.ones(nv, bool)
            if s == 0:
                ku[j] = False
            elif s == 1:
                kv[j] = False
            un.append(U[ku]); ud.append(UL[ku] // 2); vn.append(V[kv]); vd.append(VL[kv] // 2)
            uoff.append(uoff[-1] + int(ku.sum()))
            voff.append(voff[-1] + int(kv.sum()))
            link.append(link0 + g)
            side.append(s)
            node.append(-1 if s == 255 else int(U[j]) if s == 0 else int(V[j]))
            rating.append(0 if s == 255 else int(A[int(U[j]), int(V[0])]) if s == 0 else int(A[int(U[0]), int(V[j])]))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    return dict(uoff=np.asarray(uoff, np.int64), voff=np.asarray(voff, np.int64), unodes=cat(un, np.int32), udist=cat(ud, np.uint8),
                vnodes=cat(vn, np.int32), vdist=cat(vd, np.uint8), var_link=np.asarray(link, np.int32),
                var_side=np.asarray(side, np.uint8), var_node=np.asarray(node, np.int32), var_rating=np.asarray(rating, np.uint8))


CACHE_KEYS = ('uoff', 'unodes', 'udist', 'voff', 'vnodes', 'vdist')
VAR_KEYS = ('var_link', 'var_side', 'var_node', 'var_rating')
DTYPES = dict(uoff=np.int64, voff=np.int64, unodes=np.int32, vnodes=np.int32, udist=np.uint8, vdist=np.uint8, var_link=np.int32,
              var_side=np.uint8, var_node=np.int32, var_rating=np.uint8)
SENTINEL = dict(uoff=-7, voff=-7, unodes=-9, vnodes=-9, udist=201, vdist=201, var_link=-5, var_side=77, var_node=-3, var_rating=99)


def loo_count(be, b, B):
    c = [be.dev(np.full(B, -1, np.int64)) for _ in range(3)]
    be.lib.call('igmc_loo_count', b.handle, B, P(be.ptr(c[0])), P(be.ptr(c[1])), P(be.ptr(c[2])), None)
    return [be.host(x) for x in c]


def loo_fill(be, g, b, B, offs, caps, link0=0, pad=3):
    """-> (the ten output arrays on the host, allocated ``pad`` entries beyond their capacities and pre-filled with
    sentinels; the error word)."""
    cap_var, cap_u, cap_v = caps
    size = dict(uoff=cap_var + 1, voff=cap_var + 1, unodes=cap_u, udist=cap_u, vnodes=cap_v, vdist=cap_v, var_link=cap_var,
                var_side=cap_var, var_node=cap_var, var_rating=cap_var)
    buf = {k: be.dev(np.full(size[k] + pad, SENTINEL[k], DTYPES[k])) for k in CACHE_KEYS + VAR_KEYS}
    o = [be.dev(np.asarray(x, np.int64)) for x in offs]
    err = be.dev(np.zeros(1, np.int32))
    be.lib.call('igmc_loo_fill', g.handle, b.handle, B, link0, P(be.ptr(o[0])), P(be.ptr(o[1])), P(be.ptr(o[2])), cap_var, cap_u,
                cap_v, *([P(be.ptr(buf[k])) for k in CACHE_KEYS + VAR_KEYS] + [P(be.ptr(err)), None]))
    return {k: be.host(v) for k, v in buf.items()}, int(be.host(err)[0])


def prefix(c):
    return np.concatenate([[0], np.cumsum(c)]).astype(np.int64)


def assert_outputs(got, want, what, skip_links=(), var_off=None, uent_off=None, vent_off=None):
    """Element for element; whatever lies behind the written part (and the whole share of ``skip_links``) is the sentinel."""
    exp = {}
    for k in CACHE_KEYS + VAR_KEYS:
        e = np.full(len(got[k]), SENTINEL[k], DTYPES[k])
        e[:len(want[k])] = want[k]
        exp[k] = e
    for g in skip_links:
        v0, v1 = int(var_off[g]), int(var_off[g + 1])
        for k in VAR_KEYS:
            exp[k][v0:v1] = SENTINEL[k]
        last = g == len(var_off) - 2
        for k in ('uoff', 'voff'):       # (a link's first offset is also the end of the link before it, which wrote it)
            exp[k][v0 + (1 if g > 0 else 0):v1 + (1 if last else 0)] = SENTINEL[k]
        for k in ('unodes', 'udist'):
            exp[k][int(uent_off[g]):int(uent_off[g + 1])] = SENTINEL[k]
        for k in ('vnodes', 'vdist'):
            exp[k][int(vent_off[g]):int(vent_off[g + 1])] = SENTINEL[k]
    for k in CACHE_KEYS + VAR_KEYS:
        assert got[k].dtype == exp[k].dtype and got[k].shape == exp[k].shape, (what, k)
        if got[k].tobytes() != exp[k].tobytes():
            bad = np.nonzero(got[k] != exp[k])[0]
            raise AssertionError('%s: %s differs at %d places, first %d: got %s, expected %s' % (
                what, k, len(bad), bad[0], got[k][bad[0]], exp[k][bad[0]]))


def profiled(be, fn):
    """The kernels the library launched during ``fn()``, by its own per-kernel record."""
    engine.profile_fetch(be.lib, 128)
    engine.profile_enable(be.lib, True)
    try:
        out = fn()
        be.sync()
    finally:
        engine.profile_enable(be.lib, False)
    return out, sorted(n for n, _, c in engine.profile_fetch(be.lib, 128) if c > 0)


def check_case(be, hop, mnph, lean, B, first=0, want_dense=None, link0=11):
    """One arena geometry and batch size: counts = the closed forms, the ten arrays = numpy's, ``var_rating`` = scipy's.
    INSTEAD OF comparing ``igmc_batch_get_info`` before and after (that call itself makes a lean arena emit its CSR) the test
    asserts what the library launched during the two calls, by its own per-kernel record: ``k_loo_count`` and ``k_loo_fill``
    and nothing else -- no ``k_emit``; the arena is downloaded (which emits) only AFTER both calls."""
    A = corner_graph()
    g = engine.Graph(A, device=be.device, lib=be.lib)
    links = corner_links()
    b = base_arena(be, g, links, hop, mnph, lean, B, first)
    (nvar, nue, nve), ran = profiled(be, lambda: loo_count(be, b, B))
    assert ran == ['k_loo_count'], ran
    offs = [prefix(nvar), prefix(nue), prefix(nve)]
    caps = (int(offs[0][-1]), int(offs[1][-1]), int(offs[2][-1]))
    (got, err), ran = profiled(be, lambda: loo_fill(be, g, b, B, offs, caps, link0=link0))
    assert ran == ['k_loo_fill'], ran
    assert err == 0
    d = b.download()
    assert d['B'] == B
    if want_dense is not None:
        assert b.dense == want_dense
    lists = node_lists(d)
    for i, (U, _, V, _) in enumerate(lists):
        assert (int(nvar[i]), int(nue[i]), int(nve[i])) == closed_forms(len(U), len(V)), i
        assert U[0] == links[first + i, 0] and V[0] == links[first + i, 1]
        assert (np.diff(U[1:]) > 0).all() and (np.diff(V[1:]) > 0).all()
    want = reference_variants(lists, A, link0)
    assert len(want['var_link']) == caps[0] and len(want['unodes']) == caps[1] and len(want['vnodes']) == caps[2]
    assert_outputs(got, want, 'hop %d cap %s lean %s B %d' % (hop, mnph, lean, B))
    return lists, want


def check_sizes_covered(be):
    """The uncapped batch of 50 holds every size the kernels' loops care about, on both sides, and the empty link."""
    lists, want = check_case(be, 1, None, False, 50, want_dense=False)
    nus, nvs = {len(U) for U, _, V, _ in lists}, {len(V) for U, _, V, _ in lists}
    need = {1, 2, 63, 64, 65, 255, 256, 257}
    assert need <= nus and need <= nvs, (sorted(nus), sorted(nvs))
    assert (len(lists[0][0]), len(lists[0][2])) == (1, 1)          # link (0, 0): the base variant only
    assert want['var_side'][0] == 255 and want['var_link'][1] == want['var_link'][0] + 1
    assert (want['var_rating'][want['var_side'] != 255] > 0).any()


def check_capacities(be):
    """One entry short in each of the three dimensions: the bit of that dimension, the last link unwritten, the others whole."""
    A = corner_graph()
    g = engine.Graph(A, device=be.device, lib=be.lib)
    links = corner_links()
    B = 7
    b = base_arena(be, g, links, 1, 100, False, B, first=1)
    nvar, nue, nve = loo_count(be, b, B)
    offs = [prefix(nvar), prefix(nue), prefix(nve)]
    want = reference_variants(node_lists(b.download()), A, 0)
    full = (int(offs[0][-1]), int(offs[1][-1]), int(offs[2][-1]))
    for dim, bit in enumerate((ERR_VAR, ERR_UENT, ERR_VENT)):
        caps = tuple(c - 1 if i == dim else c for i, c in enumerate(full))
        got, err = loo_fill(be, g, b, B, offs, caps)
        assert err == bit, (dim, err)
        assert_outputs(got, want, 'capacity %d short' % dim, skip_links=(B - 1,), var_off=offs[0], uent_off=offs[1], vent_off=offs[2])
    # offsets that are not the prefix sums of the counts: bit 3, that link unwritten
    wrong = [o.copy() for o in offs]
    wrong[0][3:] += 1
    got, err = loo_fill(be, g, b, B, wrong, (full[0] + 1, full[1], full[2]))
    assert err == ERR_OFFSETS
    # more links than were extracted into the arena (here: none) are refused on the host, nothing is launched
    import pytest
    empty = engine.Batch(g, 2, 1, 100)
    with pytest.raises(RuntimeError, match='extracted'):
        loo_count(be, empty, 2)
    with pytest.raises(RuntimeError, match='extracted'):
        loo_fill(be, g, empty, 2, [np.zeros(3, np.int64)] * 3, (4, 4, 4))
    with pytest.raises(RuntimeError, match='extracted'):
        loo_count(be, b, B + 1)


def check_grid(be):
    """The fill's output does not depend on its grid (``IGMC_LOO_CHUNKS``: workgroups per link)."""
    A = corner_graph()
    g = engine.Graph(A, device=be.device, lib=be.lib)
    b = base_arena(be, g, corner_links(), 1, None, False, 7, first=2)
    nvar, nue, nve = loo_count(be, b, 7)
    offs = [prefix(nvar), prefix(nue), prefix(nve)]
    caps = (int(offs[0][-1]), int(offs[1][-1]), int(offs[2][-1]))
    old = os.environ.get('IGMC_LOO_CHUNKS')
    outs = []
    try:
        for chunks in ('1', '3', '16', '200'):
            os.environ['IGMC_LOO_CHUNKS'] = chunks
            got, err = loo_fill(be, g, b, 7, offs, caps)
            assert err == 0
            outs.append(got)
    finally:
        if old is None:
            os.environ.pop('IGMC_LOO_CHUNKS', None)
        else:
            os.environ['IGMC_LOO_CHUNKS'] = old
    for o in outs[1:]:
        for k in CACHE_KEYS + VAR_KEYS:
            assert o[k].tobytes() == outs[0][k].tobytes(), k


def check_deltas(be):
    """``igmc_loo_deltas`` against numpy on scores with NaN, +-0 and +-inf, segments of 0 / 1 / 300 attributions."""
    rng = np.random.default_rng(5)
    nvar = np.asarray([1, 2, 301, 1, 5, 65, 1], np.int64)
    var_off = prefix(nvar)
    n = len(nvar)
    seg_off = var_off - np.arange(n + 1)
    s = rng.standard_normal(int(var_off[-1])).astype(np.float32)
    s[var_off[2] + 3] = np.nan
    s[var_off[2] + 4] = np.inf
    s[var_off[2] + 5] = -np.inf
    s[var_off[2] + 6] = s[var_off[2]]              # delta +0
    s[var_off[4]] = np.nan                         # a NaN base: every key of the link is NaN
    s[var_off[5]] = np.inf                         # an infinite base: inf - inf is NaN, -inf - inf is -inf
    s[var_off[5] + 1] = np.inf
    s[var_off[5] + 2] = -np.inf
    s[var_off[1]:var_off[1] + 2] = [0.0, -0.0]
    nd = int(seg_off[-1])
    base, delta, key = be.dev(np.full(n, 9, np.float32)), be.dev(np.full(nd + 2, 7, np.float32)), be.dev(np.full(nd + 2, 7, np.float32))
    ds, dv, dso = be.dev(s), be.dev(var_off), be.dev(seg_off)
    be.lib.call('igmc_loo_deltas', P(be.ptr(ds)), P(be.ptr(dv)), n, P(be.ptr(base)), P(be.ptr(delta)), P(be.ptr(key)),
                P(be.ptr(dso)), None)
    base, delta, key = be.host(base), be.host(delta), be.host(key)
    with np.errstate(invalid='ignore'):
        wb = s[var_off[:-1]]
        wd = np.concatenate([s[var_off[i] + 1:var_off[i + 1]] - s[var_off[i]] for i in range(n)]).astype(np.float32)
    wk = np.abs(wd)
    assert base.tobytes() == wb.tobytes()
    for got, want in ((delta, wd), (key, wk)):
        assert (got[nd:] == 7).all()
        got = got[:nd]
        nan = np.isnan(want)
        assert nan.any() and np.array_equal(np.isnan(got), nan)
        assert got[~nan].tobytes() == want[~nan].tobytes()
    assert np.isnan(key[seg_off[4]:seg_off[5]]).all() and not (np.signbit(key[~np.isnan(key)])).any()


# ------------------------------------------------------------------ the CPU oracle's attributions
def oracle_graph():
    """The 30 x 40 graph of the recommendation test's oracle case, its class values and its rated links."""
    A = random_rating_graph(30, 40, 0.3, 5, 21)
    A.eliminate_zeros()
    rows, cols = A.nonzero()
    return A, np.arange(1, 6, dtype=np.float64), rows, cols


def oracle_deltas(ref, A, cv, pairs):
    """Per pair: (base score, {(side, global id): delta}) by the CPU oracle -- ``oracle.extract_ref.extract`` of the pair, then
    one copy of the subgraph per neighbour with the edges incident to that neighbour deleted, all scored by
    ``pyg_ref.eval_sse``.  Deleting a node's edges equals removing the node for IGMC, whose readout sees the two targets only
    and whose convolutions carry nothing from an isolated node to them."""
    from oracle import extract_ref as X
    from oracle import pyg_ref
    Acsc = ssp.csc_matrix(A)
    out = []
    for u, v in pairs:
        d = X.extract((int(u), int(v)), A, Acsc, 1, 1.0, None, cv, 0)
        nu = len(d.u_nodes)
        names = [(0, int(x)) for x in d.u_nodes[1:]] + [(1, int(x)) for x in d.v_nodes[1:]]
        local = list(range(1, nu)) + list(range(nu + 1, nu + len(d.v_nodes)))
        datas = [d]
        for li in local:
            keep = (d.edge_index[0] != li) & (d.edge_index[1] != li)
            datas.append(X.Data(d.x, d.edge_index[:, keep], edge_type=d.edge_type[keep], y=d.y))
        _, o = pyg_ref.eval_sse(ref, pyg_ref.Batch.from_data_list(datas))
        o = o.detach().numpy().astype(np.float64).ravel()
        out.append((o[0], {k: o[1 + i] - o[0] for i, k in enumerate(names)}))
    return out


def oracle_pairs(A, rows, cols, users=(0, 3, 7, 12, 20, 29)):
    """Every rated link of six users."""
    keep = np.isin(rows, users)
    return np.stack([rows[keep], cols[keep]], 1).astype(np.int64)
