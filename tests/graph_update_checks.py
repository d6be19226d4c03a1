"""Cases, numpy references and checks of ``igmc_graph_apply`` / ``igmc_graph_info`` / ``igmc_graph_download``
(igmc_amd/csrc/graph_update.hip, ``engine.Graph.updated``), shared by the emulator test (tests/test_emu_graph_update.py) and the
GPU test (tests/test_gpu_graph_update.py).  Every function takes a backend ``be`` of parity_checks (``EmuBackend`` /
``GpuBackend``).

All comparisons are exact.  The arrays of an updated graph must equal BOTH

* ``engine.Graph(A')`` downloaded, ``A'`` being the matrix after the assignments were executed in order on the host, and
* the layout stated in numpy (:func:`expected_layout`): ``np.lexsort`` by (row, relation, id) per orientation, pointers by
  ``bincount``, degrees and ``max_rel`` by numpy -- so the check is not the library against itself.

Matrices are dense uint8 arrays here (value = rating label + 1, 0 = no entry): the graphs are small.

Two quantities are staged in LDS and the cases cross both: the sort's tile of ``SORT_TILE`` changes (longer lists take the
global strides) and the ``ROW_STAGE`` changes of ONE row whose keys a wave of ``k_gu_write`` stages (a row with more in one
call takes the pass over memory)."""
import ctypes as C
import os

import numpy as np
import scipy.sparse as ssp

from igmc_amd import engine

P = engine._p
SORT_TILE = 2048                                   # graph_update.hip: GU_TILE, changes of one LDS tile of the sort
ROW_STAGE = 256                                    # graph_update.hip: GU_ROW_STAGE, changes of one row a wave stages in LDS
LENS = [0, 1, 63, 64, 65, 255, 256, 257]           # the wave (64) and workgroup (256) widths of the kernels
KEYS = ('u_ptr', 'u_idx', 'u_rel', 'v_ptr', 'v_idx', 'v_rel')


# ------------------------------------------------------------------ references
def apply_host(M, changes, n_users=None, n_items=None):
    """``M`` grown to the new sizes, then ``M[u, i] = r`` for every change in order."""
    u, i, r = changes
    nu = max(M.shape[0], int(max(u)) + 1 if len(u) else 0) if n_users is None else n_users
    ni = max(M.shape[1], int(max(i)) + 1 if len(i) else 0) if n_items is None else n_items
    out = np.zeros((nu, ni), np.uint8)
    out[:M.shape[0], :M.shape[1]] = M
    for a, b, c in zip(u, i, r):
        out[a, b] = c
    return out


def expected_layout(M):
    """The six arrays and the six sizes of the graph of ``M``, in numpy."""
    rows, cols = np.nonzero(M)
    rel = M[rows, cols].astype(np.int64) - 1
    ou, ov = np.lexsort((cols, rel, rows)), np.lexsort((rows, rel, cols))
    d = dict(u_ptr=np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=M.shape[0]))]).astype(np.int32),
             u_idx=cols[ou].astype(np.int32), u_rel=rel[ou].astype(np.uint8),
             v_ptr=np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=M.shape[1]))]).astype(np.int32),
             v_idx=rows[ov].astype(np.int32), v_rel=rel[ov].astype(np.uint8))
    info = dict(n_users=M.shape[0], n_items=M.shape[1], nnz=len(rows), max_rel=int(rel.max()) if len(rel) else 0,
                max_deg_u=int((M != 0).sum(1).max()), max_deg_v=int((M != 0).sum(0).max()))
    return d, info


def to_csr(M):
    return ssp.csr_matrix(M.astype(np.float32))


def graph_of(be, M):
    return engine.Graph(to_csr(M), device=be.device, lib=be.lib)


def assert_same_arrays(got, want, what):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, '%s: %s %s %s' % (what, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), '%s: %s differs' % (what, k)


def check_graph(be, g, M, what=''):
    """``g`` is the graph of ``M``: equal to the numpy layout and to a graph built from ``M`` through the host."""
    got, info = g.download(), g.info()
    want, winfo = expected_layout(M)
    assert info == winfo, '%s: info %s, numpy %s' % (what, info, winfo)
    assert_same_arrays(got, want, what + ' (numpy layout)')
    ref = graph_of(be, M)
    assert ref.info() == info, '%s: info %s, igmc_graph_create %s' % (what, info, ref.info())
    assert_same_arrays(got, ref.download(), what + ' (igmc_graph_create)')
    assert (g.n_users, g.n_items, g.nnz, g.max_rel) == (M.shape[0], M.shape[1], winfo['nnz'], winfo['max_rel'])
    assert (g.to_scipy() != to_csr(M)).nnz == 0
    return got


def as_changes(triples):
    t = np.asarray(triples, np.int64).reshape(-1, 3)
    return t[:, 0].astype(np.int32), t[:, 1].astype(np.int32), t[:, 2].astype(np.uint8)


def update(be, g, changes, n_users=None, n_items=None, device_arrays=True):
    """``g.updated`` from arrays on the backend (or from host arrays, which ``updated`` places itself)."""
    u, i, r = changes
    if device_arrays:
        u, i, r = be.dev(u), be.dev(i), be.dev(r)
    return g.updated(u, i, r, n_users, n_items)


def check_update(be, M, changes, n_users=None, n_items=None, what='', g=None):
    """One update of the graph of ``M`` checked both ways; the old graph is untouched.  -> (new graph, new matrix)."""
    g = g or graph_of(be, M)
    before = g.download()
    g2 = update(be, g, changes, n_users, n_items)
    M2 = apply_host(M, changes, n_users, n_items)
    check_graph(be, g2, M2, what)
    assert_same_arrays(g.download(), before, what + ' (the old graph)')
    return g2, M2


# ------------------------------------------------------------------ builders
def random_matrix(n_users, n_items, density, n_rel, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random((n_users, n_items)) < density) * rng.integers(1, n_rel + 1, (n_users, n_items))).astype(np.uint8)


def corner_matrix(extra=()):
    """Row k and column k hold ``(LENS + extra)[k]`` entries each: an L-shaped pattern -- row k fills the columns behind the
    corner block, column k the rows behind it -- with ratings 1..5 mixed along every row and column."""
    lens = list(LENS) + list(extra)
    K, W = len(lens), max(lens)
    M = np.zeros((K + W, K + W), np.uint8)
    for k, L in enumerate(lens):
        M[k, K:K + L] = 1 + (np.arange(L) * 3 + k) % 5
        M[K:K + L, k] = 1 + (np.arange(L) * 2 + k) % 5
    assert [(M[k] != 0).sum() for k in range(K)] == lens and [(M[:, k] != 0).sum() for k in range(K)] == lens
    return M, K


def corner_lists(M, K):
    """(grow, shrink): one insertion into / one removal from every corner row and every corner column, so that each of LENS
    is a length before a change and after one."""
    lens = [(M[k] != 0).sum() for k in range(K)]
    grow, shrink = [], []
    for k, L in enumerate(lens):
        # the free cell behind the row's / column's run, and the middle entry of the run
        grow += [(k, K + L, 1 + k % 5), (K + L, k, 1 + (k + 2) % 5)]
        if L:
            shrink += [(k, K + L // 2, 0), (K + L // 2, k, 0)]
    return as_changes(grow), as_changes(shrink)


def group_edges(M, row):
    """For every relation of ``row``: a free column in front of the group's first item and one behind its last (where one
    exists), as insertions with that relation -> they land at the front / at the back of the group."""
    out = []
    for r in np.unique(M[row][M[row] != 0]):
        cols = np.nonzero(M[row] == r)[0]
        free = np.nonzero(M[row] == 0)[0]
        front, back = free[free < cols[0]], free[free > cols[-1]]
        if len(front):
            out.append((row, int(front[-1]), int(r)))
        if len(back):
            out.append((row, int(back[0]), int(r)))
    return out


# ------------------------------------------------------------------ the cases
def single_change_cases():
    """name -> (M, triples): each alone; :func:`check_single_changes` also runs them mixed in one list."""
    M = random_matrix(30, 40, 0.3, 4, 7)
    M[3] = 0                                                         # an empty row
    M[5] = 0
    M[5, 9] = 2                                                      # a row of one entry
    M[:, 11] = 0
    M[7, 11] = 3                                                     # a column of one entry
    full = np.argwhere(M != 0)
    present = tuple(int(x) for x in full[len(full) // 2])
    absent = tuple(int(x) for x in np.argwhere(M == 0)[5])
    cases = {
        'insert_into_empty_row': [(3, 4, 2)],
        'front_and_back_of_groups_row': group_edges(M, 0),
        'front_and_back_of_groups_column': [(b, a, r) for a, b, r in group_edges(M.T, 2)],
        'remove_only_entry_of_row': [(5, 9, 0)],
        'remove_only_entry_of_column': [(7, 11, 0)],
        'remove_absent': [absent + (0,)],
        'rewrite_same_rating': [present + (int(M[present]),)],
        'change_rating_only': [present + (int(M[present]) % 4 + 1,)],
        'one_change': [(1, 1, 4)],
    }
    assert all(len(v) for v in cases.values())
    return M, cases


def check_single_changes(be):
    M, cases = single_change_cases()
    g = graph_of(be, M)
    for name, triples in cases.items():
        check_update(be, M, as_changes(triples), what=name, g=g)
    # one front / one back insertion at a time (n == 1 each), then all mixed in one list
    for t in cases['front_and_back_of_groups_row'] + cases['front_and_back_of_groups_column']:
        check_update(be, M, as_changes([t]), what='one group edge %s' % (t,), g=g)
    mixed = [t for v in cases.values() for t in v]
    check_update(be, M, as_changes(mixed), what='mixed', g=g)
    check_update(be, M, as_changes(mixed[::-1]), what='mixed, reversed', g=g)


def check_empty_list(be):
    M = random_matrix(9, 14, 0.3, 5, 3)
    g = graph_of(be, M)
    none = as_changes([])
    check_update(be, M, none, what='n == 0', g=g)
    check_update(be, M, none, 10, 15, what='n == 0, grown by one', g=g)
    check_update(be, M, none, 109, 14, what='n == 0, 100 users more', g=g)
    g0 = graph_of(be, np.zeros((3, 4), np.uint8))                   # an empty graph, then its first entry
    check_graph(be, update(be, g0, none), np.zeros((3, 4), np.uint8), 'empty graph')
    check_update(be, np.zeros((3, 4), np.uint8), as_changes([(2, 3, 1)]), what='first entry', g=g0)


def check_corner_rows(be, extra=()):
    M, K = corner_matrix(extra)
    g = graph_of(be, M)
    grow, shrink = corner_lists(M, K)
    check_update(be, M, grow, what='corner rows grow', g=g)
    check_update(be, M, shrink, what='corner rows shrink', g=g)
    both = tuple(np.concatenate([a, b]) for a, b in zip(grow, shrink))
    check_update(be, M, both, what='corner rows grow and shrink', g=g)
    # every corner row re-rated throughout: each entry moves to another relation group, in both orientations
    rows, cols = np.nonzero(M[:K])
    check_update(be, M, (rows.astype(np.int32), cols.astype(np.int32), (M[rows, cols] % 5 + 1).astype(np.uint8)),
                 what='corner rows re-rated', g=g)


def check_duplicates(be):
    M = random_matrix(10, 12, 0.4, 5, 11)
    g = graph_of(be, M)
    a, b = (int(x) for x in np.argwhere(M != 0)[3])                 # a present pair
    c, d = (int(x) for x in np.argwhere(M == 0)[3])                 # an absent one
    for (u, i) in ((a, b), (c, d)):
        check_update(be, M, as_changes([(u, i, 1), (u, i, 4)]), what='twice', g=g)
        check_update(be, M, as_changes([(u, i, 3), (u, i, 5), (u, i, 2)]), what='three times', g=g)
        check_update(be, M, as_changes([(u, i, 3), (u, i, 5), (u, i, 0)]), what='removal last', g=g)
        check_update(be, M, as_changes([(u, i, 3), (u, i, 0), (u, i, 2)]), what='removal in the middle', g=g)
        seventy = [(u, i, 1 + (k * 7) % 5) for k in range(70)]
        check_update(be, M, as_changes(seventy), what='70 times', g=g)
        seventy[-1] = (u, i, 0)
        check_update(be, M, as_changes(seventy), what='70 times, removal last', g=g)
        seventy[35], seventy[-1] = (u, i, 0), (u, i, 4)
        # ... spread among other changes, so that the sorted run is not the list's order by construction
        noise = [(int(x), int(y), 1 + (x + y) % 5) for x, y in np.random.default_rng(5).integers(0, 10, (200, 2))]
        mixed = [t for pair in zip(seventy, noise) for t in pair] + noise[70:]
        check_update(be, M, as_changes(mixed), what='70 times among others', g=g)


def concentrated(n, seed, width):
    """n changes of one row over ``width`` columns: insertions, re-ratings, removals and repeated pairs."""
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, width, n)
    return cols.astype(np.int32), rng.integers(0, 6, n).astype(np.uint8)


def check_concentration(be, n):
    """All ``n`` changes in one row, and all in one column."""
    width = max(200, (2 * n) // 3)
    M = random_matrix(6, width, 0.3, 5, n)
    cols, r = concentrated(n, n + 1, width)
    check_update(be, M, (np.full(n, 2, np.int32), cols, r), what='%d changes in one row' % n)
    check_update(be, np.ascontiguousarray(M.T), (cols, np.full(n, 2, np.int32), r), what='%d changes in one column' % n)


def check_max_rel_and_degrees(be):
    M = random_matrix(8, 10, 0.3, 3, 13)
    M[1] = np.where(M[1] == 0, 1, M[1])                              # THE longest row
    M[:, 4] = np.where(M[:, 4] == 0, 2, M[:, 4])                     # THE longest column
    M[1, 4] = 1
    g = graph_of(be, M)
    _, i0 = expected_layout(M)
    assert i0['max_rel'] == 2 and i0['max_deg_u'] == 10 and i0['max_deg_v'] == 8
    g2, M2 = check_update(be, M, as_changes([(6, 0, 7)]), what='a new highest relation', g=g)
    assert g2.info()['max_rel'] == 6
    g3, M3 = check_update(be, M2, as_changes([(6, 0, 0)]), what='the only entry of the highest relation removed', g=g2)
    assert g3.info()['max_rel'] == 2
    g4, _ = check_update(be, M3, as_changes([(1, 4, 0)]), what='the longest row and column shortened', g=g3)
    assert (g4.info()['max_deg_u'], g4.info()['max_deg_v']) == (9, 7)
    g5, _ = check_update(be, M, as_changes([(6, 0, 255), (0, 0, 255)]), what='relation 254', g=g)
    assert g5.info()['max_rel'] == 254


def check_growth(be):
    M = random_matrix(7, 9, 0.4, 5, 17)
    g = graph_of(be, M)
    check_update(be, M, as_changes([(7, 2, 3), (1, 9, 5), (7, 9, 1)]), what='one new user, one new item', g=g)
    check_update(be, M, as_changes([(2, 2, 3)]), 8, 10, what='grown by one, the new ones empty', g=g)
    check_update(be, M, as_changes([(106, 3, 2), (50, 108, 4), (0, 0, 0), (106, 108, 5)]), what='grown by 100', g=g)
    check_update(be, M, as_changes([(7, 0, 1)]), 107, 109, what='grown by 100, one entry among the new', g=g)
    g2 = update(be, g, as_changes([(9, 11, 2)]), device_arrays=False)          # default sizes from host arrays: greatest id + 1
    assert (g2.n_users, g2.n_items) == (10, 12)
    check_graph(be, g2, apply_host(M, as_changes([(9, 11, 2)])), 'default sizes')
    g3 = g.updated([1, 2], [3, 4], [5, 0])                                     # plain lists
    check_graph(be, g3, apply_host(M, as_changes([(1, 3, 5), (2, 4, 0)])), 'lists')


def random_case(seed):
    """(M, changes, n_users, n_items): a third of the changes hit existing entries, a tenth repeat an earlier pair, some
    grow the graph."""
    rng = np.random.default_rng(1000 + seed)
    nu, ni = int(rng.integers(40, 301)), int(rng.integers(60, 201))
    n_rel = 1 + seed % 10
    M = random_matrix(nu, ni, float(rng.choice([0.02, 0.1, 0.3])), n_rel, seed)
    n = [1, 2, 65, 2000][seed] if seed < 4 else int(rng.integers(1, 2001))
    grow_u, grow_i = (0, 0) if seed % 3 else (int(rng.integers(1, 30)), int(rng.integers(1, 30)))
    ex = np.argwhere(M != 0)
    us, it = rng.integers(0, nu + grow_u, n), rng.integers(0, ni + grow_i, n)
    hit = rng.random(n) < (1.0 / 3 if len(ex) else 0.0)
    pick = ex[rng.integers(0, max(len(ex), 1), n)] if len(ex) else np.zeros((n, 2), np.int64)
    us, it = np.where(hit, pick[:, 0], us), np.where(hit, pick[:, 1], it)
    for j in np.nonzero(rng.random(n) < 0.1)[0]:
        if j:
            k = int(rng.integers(0, j))
            us[j], it[j] = us[k], it[k]
    r = np.where(rng.random(n) < 0.25, 0, rng.integers(1, n_rel + 1, n))
    return M, (us.astype(np.int32), it.astype(np.int32), r.astype(np.uint8)), nu + grow_u, ni + grow_i


def check_random(be, seed):
    M, changes, nu, ni = random_case(seed)
    check_update(be, M, changes, nu, ni, what='seed %d' % seed)


def check_chained(be):
    M = random_matrix(60, 80, 0.1, 5, 31)
    g0 = graph_of(be, M)
    first = g0.download()
    graphs, mats = [g0], [M]
    for s in range(3):
        _, ch, _, _ = random_case(40 + s)
        ch = (ch[0] % (60 + 5 * s), ch[1] % (80 + 5 * s), np.minimum(ch[2], 5).astype(np.uint8))
        g, M = check_update(be, mats[-1], ch, 60 + 5 * s, 80 + 5 * s, what='chained %d' % s, g=graphs[-1])
        graphs.append(g)
        mats.append(M)
    assert_same_arrays(g0.download(), first, 'the first graph after three updates')
    for g, M in zip(graphs, mats):                                   # every stage is still what it was
        check_graph(be, g, M, 'a stage afterwards')
    graphs[1].close()                                                # a stage in the middle released: the others stand
    check_graph(be, graphs[2], mats[2], 'after a release')
    check_graph(be, graphs[3], mats[3], 'after a release')


def check_geometry(be):
    """``IGMC_GU_GRID`` (test hook) forces the grid of every grid-stride launch: the output does not depend on it."""
    M, changes, nu, ni = random_case(3)                              # 2000 changes
    g = graph_of(be, M)
    want = update(be, g, changes, nu, ni).download()
    old = os.environ.get('IGMC_GU_GRID')
    try:
        for grid in (1, 3, 64):
            os.environ['IGMC_GU_GRID'] = str(grid)
            assert_same_arrays(update(be, g, changes, nu, ni).download(), want, 'grid %d' % grid)
    finally:
        if old is None:
            os.environ.pop('IGMC_GU_GRID', None)
        else:
            os.environ['IGMC_GU_GRID'] = old
    check_graph(be, update(be, g, changes, nu, ni), apply_host(M, changes, nu, ni), 'default grid')


def raw_apply(be, g, u, i, r, n, n_users, n_items, null_out=False):
    """The C entry point itself: (return code, message, the out word)."""
    SENTINEL = 0x5A5A5A5A
    out = C.c_void_p(SENTINEL)
    rc = be.lib.cdll.igmc_graph_apply(g.handle if g is not None else None, n_users, n_items,
                                      None if u is None else P(be.ptr(u)), None if i is None else P(be.ptr(i)),
                                      None if r is None else P(be.ptr(r)), n, None, None if null_out else C.byref(out))
    be.sync()
    msg = be.lib.cdll.igmc_last_error()
    return rc, msg.decode() if msg else '', out.value == SENTINEL


def check_errors(be):
    M = random_matrix(6, 8, 0.4, 5, 19)
    g = graph_of(be, M)
    good = as_changes([(0, 0, 1), (1, 1, 2), (2, 2, 0), (5, 7, 3)])

    def refused(u, i, r, n, nu, ni, needle, gg=g, null_out=False):
        rc, msg, untouched = raw_apply(be, gg, u, i, r, n, nu, ni, null_out)
        assert rc != 0 and untouched, (rc, msg)
        assert 'igmc_graph_apply' in msg and needle in msg, msg
        check_update(be, M, good, what='a valid call after "%s"' % msg, g=g)          # the library still serves

    dev = lambda c: tuple(be.dev(x) for x in c)
    U, I, R = dev(good)
    for pos in (0, 3):                                               # either end of either array, either side of the range
        for which, bad, needle in ((0, 6, 'user id'), (0, -1, 'user id'), (1, 8, 'item id'), (1, -1, 'item id')):
            c = [x.copy() for x in good]
            c[which][pos] = bad
            u, i, r = dev(c)
            refused(u, i, r, 4, 6, 8, needle)
    u, i, r = dev(as_changes([(6, 0, 1)]))                          # in range only if the graph grows
    refused(u, i, r, 1, 6, 8, 'user id')
    refused(U, I, R, 4, 5, 8, 'shrink')
    refused(U, I, R, 4, 6, 7, 'shrink')
    refused(U, I, R, -1, 6, 8, 'n must be')
    refused(None, I, R, 4, 6, 8, 'null')
    refused(U, None, R, 4, 6, 8, 'null')
    refused(U, I, None, 4, 6, 8, 'null')
    refused(U, I, R, 4, 6, 8, 'null', gg=None)
    refused(U, I, R, 4, 6, 8, 'null', null_out=True)
    with np.testing.assert_raises(RuntimeError):
        g.updated([6], [0], [1], n_users=6)
    with np.testing.assert_raises(ValueError):
        g.updated([0], [0], [256])
    with np.testing.assert_raises(ValueError):
        g.updated([0, 1], [0], [1])
    # igmc_graph_info / igmc_graph_download: null handles are refused, null arrays are skipped
    assert be.lib.cdll.igmc_graph_info(None, None) != 0 and b'igmc_graph_info' in be.lib.cdll.igmc_last_error()
    assert be.lib.cdll.igmc_graph_download(None, None, None, None, None, None, None) != 0
    only = np.zeros(M.shape[0] + 1, np.int32)
    be.lib.call('igmc_graph_download', g.handle, P(only), None, None, None, None, None)
    assert np.array_equal(only, expected_layout(M)[0]['u_ptr'])
