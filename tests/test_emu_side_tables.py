"""``igmc_batch_bind_side_tables`` / ``k_side_gather_nodes`` (igmc_amd/csrc/extract.hip) on the CPU emulation of the same sources:
the side-feature rows of a batch's two TARGET nodes gathered from per-node tables by the ids the extraction left in the arena's
slots -- the route of every source whose links are not a dataset's own (candidate lists, leave-one-out variants, views)."""
import ctypes as C

import numpy as np
import pytest

import parity_checks as PC
from helpers import random_rating_graph
from igmc_amd import engine

N_USERS, N_ITEMS = 12, 9
# 8 links over a 12 x 9 graph: a repeated pair (0, 3), a user shared by two pairs (4), the last two users (10, 11), and pairs
# the graph has no rating for; the first 5 already hold the repeated pair and the shared user
LINK_U = np.array([3, 4, 3, 4, 11, 10, 0, 7], np.int32)
LINK_V = np.array([2, 8, 2, 0, 5, 1, 6, 3], np.int32)
LINK_Y = np.arange(1, 9, dtype=np.float32)


@pytest.fixture(scope='module')
def be():
    return PC.EmuBackend()


@pytest.fixture(scope='module')
def graph(be):
    return engine.Graph(random_rating_graph(N_USERS, N_ITEMS, 0.4, 5, seed=11), lib=be.lib)


def tables(fu, fv, seed, n_u=N_USERS, n_v=N_ITEMS):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n_u, fu)).astype(np.float32), rng.standard_normal((n_v, fv)).astype(np.float32)


def bind(b, U, V):
    b.bind_side_tables(U.ctypes.data if U.shape[1] else None, U.shape[0], U.shape[1],
                       V.ctypes.data if V.shape[1] else None, V.shape[0], V.shape[1])


def extract(b, first, B, perm=None):
    b.extract(LINK_U.ctypes.data, LINK_V.ctypes.data, LINK_Y.ctypes.data, None if perm is None else perm.ctypes.data, first, B)


def side_rows(b, rows, cols):
    """The arena's side-feature rows as the next forward reads them (``IGMC_BUF_SIDE``), copied."""
    ptr = b.device_ptr('SIDE')
    assert ptr
    return np.ctypeslib.as_array((C.c_float * (rows * cols)).from_address(ptr)).reshape(rows, cols).copy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def expected(U, V, u, v):
    """numpy.hstack([U[u], V[v]]) with zero rows for ids the tables do not hold."""
    eu, ev = np.zeros((len(u), U.shape[1]), np.float32), np.zeros((len(v), V.shape[1]), np.float32)
    ok = u < U.shape[0]
    eu[ok] = U[u[ok]]
    ok = v < V.shape[0]
    ev[ok] = V[v[ok]]
    return np.hstack([eu, ev])


@pytest.mark.parametrize('fu,fv', [(3, 5), (0, 4)])
@pytest.mark.parametrize('mnph', [None, 3])
def test_exact_gather(graph, fu, fv, mnph):
    B = 5
    U, V = tables(fu, fv, seed=1)
    b = engine.Batch(graph, B, 1, mnph)
    bind(b, U, V)
    extract(b, 0, B)
    got = side_rows(b, B, fu + fv)
    assert np.array_equal(bits(got), bits(np.hstack([U[LINK_U[:B]], V[LINK_V[:B]]])))
    # ... and through a permutation with an offset: the rows follow the links the extraction took, not the positions
    perm = np.array([6, 1, 7, 0, 2, 5, 3, 4], np.int32)
    extract(b, 2, B, perm)
    at = perm[2:2 + B]
    assert np.array_equal(bits(side_rows(b, B, fu + fv)), bits(np.hstack([U[LINK_U[at]], V[LINK_V[at]]])))


def test_ids_beyond_the_tables_read_zeros(graph):
    fu, fv = 3, 5
    U, V = tables(fu, fv, seed=2, n_u=N_USERS - 2)
    b = engine.Batch(graph, 8, 1)
    bind(b, U, V)
    extract(b, 0, 8)
    got = side_rows(b, 8, fu + fv)
    late = LINK_U >= N_USERS - 2
    assert late.sum() == 2
    assert np.array_equal(bits(got[late, :fu]), np.zeros((2, fu), np.uint32))            # +0.0, bit for bit
    assert np.array_equal(bits(got[:, fu:]), bits(V[LINK_V]))                            # the item halves are still exact
    assert np.array_equal(bits(got[~late, :fu]), bits(U[LINK_U[~late]]))
    # the same on the item side, and a table without any row
    U2, V2 = tables(fu, fv, seed=3, n_v=5)
    bind(b, U2, V2)
    extract(b, 0, 8)
    assert np.array_equal(bits(side_rows(b, 8, fu + fv)), bits(expected(U2, V2, LINK_U, LINK_V)))
    assert (LINK_V >= 5).sum() >= 2
    b.bind_side_tables(U2.ctypes.data, 0, fu, V2.ctypes.data, 5, fv)
    extract(b, 0, 8)
    assert np.array_equal(bits(side_rows(b, 8, fu + fv)), bits(expected(U2[:0], V2, LINK_U, LINK_V)))


def test_rows_at_or_beyond_B_are_not_written(graph):
    fu, fv = 3, 5
    U, V = tables(fu, fv, seed=4)
    U2, V2 = tables(fu, fv, seed=5)
    b = engine.Batch(graph, 8, 1)
    bind(b, U, V)
    extract(b, 0, 8)
    first = side_rows(b, 8, fu + fv)
    bind(b, U2, V2)
    extract(b, 0, 5)
    got = side_rows(b, 8, fu + fv)
    assert np.array_equal(bits(got[:5]), bits(np.hstack([U2[LINK_U[:5]], V2[LINK_V[:5]]])))
    assert np.array_equal(bits(got[5:]), bits(first[5:]))
    assert not np.array_equal(bits(got[:5]), bits(first[:5]))


@pytest.mark.parametrize('mnph', [None, 3])
def test_cached_node_sets_gather_the_same_rows(graph, mnph):
    """``igmc_extract_batch_cached`` over the node sets of a first extraction (the route of the leave-one-out variants),
    through a permutation: the targets come from the stored lists, no link array is given."""
    fu, fv, B = 3, 5, 8
    U, V = tables(fu, fv, seed=6)
    b = engine.Batch(graph, B, 1, mnph)
    bind(b, U, V)
    extract(b, 0, B)
    want = side_rows(b, B, fu + fv)
    d = b.download()
    uoff, voff = np.zeros(B + 1, np.int64), np.zeros(B + 1, np.int64)
    un, vn, ud, vd = [], [], [], []
    for g in range(B):
        lo, hi, nu = int(d['node_off'][g]), int(d['node_off'][g + 1]), int(d['n_users'][g])
        un.append(d['node_gid'][lo:lo + nu])
        vn.append(d['node_gid'][lo + nu:hi])
        ud.append(d['node_label'][lo:lo + nu] // 2)
        vd.append(d['node_label'][lo + nu:hi] // 2)
        uoff[g + 1], voff[g + 1] = uoff[g] + nu, voff[g] + (hi - lo - nu)
    keep = dict(uoff=uoff, voff=voff, unodes=np.concatenate(un).astype(np.int32), vnodes=np.concatenate(vn).astype(np.int32),
                udist=np.concatenate(ud).astype(np.uint8), vdist=np.concatenate(vd).astype(np.uint8))
    cache = {k: a.ctypes.data for k, a in keep.items()}
    perm = np.array([5, 0, 7, 2, 2, 6, 1, 3], np.int32)
    c = engine.Batch(graph, B, 1, mnph)
    bind(c, U, V)
    c.extract_cached(cache, LINK_Y.ctypes.data, perm.ctypes.data, 1, 6)
    assert np.array_equal(bits(side_rows(c, 6, fu + fv)), bits(want[perm[1:7]]))
    assert np.array_equal(c.download()['y'], LINK_Y[perm[1:7]])


def test_binding_rules(be, graph):
    from igmc_amd.stepgraph import _ctrl_words
    U, V = tables(3, 5, seed=7)
    b = engine.Batch(graph, 8, 1)
    with pytest.raises(RuntimeError, match='null side-feature table'):
        b.bind_side_tables(None, N_USERS, 3, V.ctypes.data, N_ITEMS, 5)
    with pytest.raises(RuntimeError, match='null side-feature table'):
        b.bind_side_tables(U.ctypes.data, N_USERS, 3, None, N_ITEMS, 5)
    with pytest.raises(RuntimeError):
        b.bind_side_tables(U.ctypes.data, N_USERS, -1, V.ctypes.data, N_ITEMS, 5)
    with pytest.raises(RuntimeError):
        b.bind_side_tables(U.ctypes.data, N_USERS, 0, V.ctypes.data, N_ITEMS, 0)
    assert not b.device_ptr('SIDE')                                # nothing bound by a refused call
    # tables unbind a side source ...
    side_all = np.random.default_rng(8).standard_normal((8, 8)).astype(np.float32)
    b.bind_side_source(side_all.ctypes.data, 8)
    extract(b, 0, 8)
    assert np.array_equal(bits(side_rows(b, 8, 8)), bits(side_all))
    bind(b, U, V)
    extract(b, 0, 8)
    assert np.array_equal(bits(side_rows(b, 8, 8)), bits(np.hstack([U[LINK_U], V[LINK_V]])))
    # ... and the reverse: the source's rows again, not the tables'
    b.bind_side_source(side_all.ctypes.data, 8)
    extract(b, 0, 8)
    assert np.array_equal(bits(side_rows(b, 8, 8)), bits(side_all))
    # a borrowed set_side_features pointer replaces tables too: the next extraction gathers nothing over it
    bind(b, U, V)
    handed = np.full((8, 8), 7.0, np.float32)
    b.set_side_features(handed.ctypes.data, 8)
    extract(b, 0, 8)
    assert b.device_ptr('SIDE') == handed.ctypes.data and np.all(handed == 7.0)
    # a wider re-bind works (the arena's buffer grows), a narrower one after it too
    for fu, fv in ((3, 5), (20, 17), (2, 1)):
        Uw, Vw = tables(fu, fv, seed=9)
        bind(b, Uw, Vw)
        extract(b, 0, 8)
        assert np.array_equal(bits(side_rows(b, 8, fu + fv)), bits(np.hstack([Uw[LINK_U], Vw[LINK_V]])))
    # an unbind leaves n_side = 0: a model without side features takes the arena, one with them does not
    b.bind_side_tables(None, 0, 0, None, 0, 0)
    assert not b.device_ptr('SIDE')
    extract(b, 0, 8)
    out = np.zeros(8, np.float32)
    for n_side, ok in ((0, True), (8, False)):
        ws = engine.ModelWorkspace(be.lib, 0, 5, 4, 4, n_side, b.node_capacity, b.edge_capacity, 8)
        P = PC.flatten_params(ws, PC.make_ref_model(4, 5, n_side=n_side, seed=2))
        if ok:
            ws.forward(P.ctypes.data, b, out.ctypes.data, training=False)
            assert np.all(np.isfinite(out))
        else:
            with pytest.raises(RuntimeError):
                ws.forward(P.ctypes.data, b, out.ctypes.data, training=False)
    # igmc_extract_group takes lean capped arenas under one control block -- and refuses one with tables
    ctrl = _ctrl_words(0, 0, 1, 2, 2, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    arenas = [engine.Batch(graph, 2, 1, 3) for _ in range(2)]
    for a in arenas:
        a.set_lean(True)
        be.lib.call('igmc_batch_set_ctrl', a.handle, C.c_void_p(ctrl.ctypes.data))
    bset = engine.BatchSet(arenas)
    ident = np.arange(64, dtype=np.int32) % 8
    group = lambda: bset.extract(2, LINK_U.ctypes.data, LINK_V.ctypes.data, LINK_Y.ctypes.data, ident.ctypes.data, 0, 2)
    group()
    bind(arenas[1], U, V)
    with pytest.raises(RuntimeError, match='no side-feature source'):
        group()
    arenas[1].bind_side_tables(None, 0, 0, None, 0, 0)
    group()


@pytest.mark.parametrize('fu,fv', [(6, 10), (3, 5)])
def test_model_consumes_the_gathered_rows(be, graph, fu, fv):
    """n_side = 16: the MFMA head kernels (D % 16 == 0); 8: the generic ones.  A forward over rows gathered from tables equals,
    bit for bit, the forward over the same rows handed in with ``igmc_batch_set_side_features``."""
    S, B = fu + fv, 8
    assert ((256 + S) % 16 == 0) == (S == 16)
    U, V = tables(fu, fv, seed=10)
    ref = PC.make_ref_model(4, 5, n_side=S, seed=2)
    outs = []
    for mode in ('tables', 'handed', 'zeros'):
        b = engine.Batch(graph, B, 1)
        ws = engine.ModelWorkspace(be.lib, 0, 5, 4, 4, S, b.node_capacity, b.edge_capacity, B)
        P = PC.flatten_params(ws, ref)
        if mode == 'tables':
            bind(b, U, V)
        extract(b, 0, B)
        if mode != 'tables':
            rows = np.ascontiguousarray(np.hstack([U[LINK_U], V[LINK_V]])) if mode == 'handed' else np.zeros((B, S), np.float32)
            b.set_side_features(rows.ctypes.data, S)
        out = np.zeros(B, np.float32)
        ws.forward(P.ctypes.data, b, out.ctypes.data, training=False)
        outs.append(out.copy())
    assert np.array_equal(bits(outs[0]), bits(outs[1])) and np.all(np.isfinite(outs[0]))
    assert not np.array_equal(outs[0], outs[2])          # the rows matter
