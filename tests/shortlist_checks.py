"""Cases, scipy references and checks of ``igmc_shortlist_fill`` / ``igmc_shortlist_places`` (``igmc_amd/csrc/shortlist.hip``):
every user's candidate segment cut down to the items with the most co-rating votes.  Shared by the emulator test
(tests/test_emu_shortlist.py) and the GPU test (tests/test_gpu_shortlist.py), as ``selection_checks.py`` is; every function
takes a backend ``be`` of parity_checks and calls the C entry points directly, every buffer a call can write -- and every
input an offset could lead past -- sits between the guards of ``selection_checks.Guarded``.  Every comparison is exact.

THE DEFINITION, restated here in scipy from the text of ``include/igmc_hip.h``: rel(u, v) = the stored rating - 1; L_s =
[entry present and rel >= s], L_t alike; for request q of user u, w = row u of L_s L_s^T with w[u] = 0, votes = w L_t (exact
integers, defined for every item), C(u) = the candidates of ``igmc_candidates_fill``; the vote order over C is
``np.lexsort((item, -votes))``, the shortlist its first min(m, |C|) items, written item ascending."""
import numpy as np
import scipy.sparse as ssp

from helpers import random_rating_graph
from igmc_amd import engine
from sampled_candidates_checks import candidates_ref
from selection_checks import BAD_OFFSETS, GUARD, TILE, Guarded, P, filled, offsets

M_MAX = 2 ** 31 - 1
R = 5
THRESHOLDS = [(0, 0), (3, 3), (R - 1, 0), (0, R - 1), (R, 0)]          # the last: no seeds, every vote is zero
N_ITEMS_SMALL = [63, 64, 65]
N_ITEMS_WIDE = [TILE - 1, TILE, TILE + 1, 2 * TILE + TILE // 2]          # around the LDS vote table, and 2.5 tiles: the scratch row


# ------------------------------------------------------------------ the definition
def binary(A, min_rel):
    A = A.tocsr()
    return ssp.csr_matrix(((A.data - 1 >= min_rel).astype(np.int64), A.indices, A.indptr), shape=A.shape)


def votes_ref(A, users, s, t):
    """int64 [len(users), n_items]: the votes of every item for every request."""
    Ls, Lt = binary(A, s), binary(A, t)
    users = np.asarray(users, np.int64)
    W = np.asarray((Ls[users] @ Ls.T).todense())
    W[np.arange(len(users)), users] = 0          # the user itself never votes
    return np.asarray(W @ Lt.toarray() if Lt.shape[1] <= 4096 else (ssp.csr_matrix(W) @ Lt).todense()).astype(np.int64)


def order_ref(votes, cand):
    """The items of C in the vote order."""
    items = np.nonzero(cand)[0]
    return items[np.lexsort((items, -votes[items]))]


def segments_ref(A, users, m, s=0, t=0, item_ok=None, exclude_seen=1):
    """link_u, link_v, votes, counts of a request list."""
    A = A.tocsr()
    V = votes_ref(A, users, s, t)
    us, vs, ws = [], [], []
    for q, u in enumerate(users):
        cand = candidates_ref(A, int(u), item_ok, exclude_seen)
        v = np.sort(order_ref(V[q], cand)[:m]).astype(np.int32)
        us.append(np.full(len(v), u, np.int32))
        vs.append(v)
        ws.append(V[q][v].astype(np.uint32))
    return np.concatenate(us), np.concatenate(vs), np.concatenate(ws), np.array([len(v) for v in vs], np.int64)


def places_ref(A, users, q_off, q_id, s=0, t=0, item_ok=None, exclude_seen=1):
    """place int32 [n_query], votes uint32 [n_query]."""
    A = A.tocsr()
    n_items = A.shape[1]
    V = votes_ref(A, users, s, t)
    place, votes = np.full(len(q_id), -1, np.int32), np.zeros(len(q_id), np.uint32)
    for q, u in enumerate(users):
        order = order_ref(V[q], candidates_ref(A, int(u), item_ok, exclude_seen))
        where = np.full(n_items, -1, np.int32)
        where[order] = np.arange(len(order))
        for k in range(int(q_off[q]), int(q_off[q + 1])):
            if 0 <= q_id[k] < n_items:
                place[k], votes[k] = where[q_id[k]], V[q][q_id[k]]
    return place, votes


# ------------------------------------------------------------------ the device
def plan(be, g, nq, grid=0):
    out = np.zeros(6, np.int64)
    be.lib.call('igmc_shortlist_plan_info', g.handle, nq, grid, P(out.ctypes.data))
    return dict(zip(('grid', 'lds_bytes', 'w_lds', 'v_lds', 'scratch_bytes', 'w_lds_max_users'), out.tolist()))


def scratch(be, g, nq, grid):
    """The caller-owned scratch, full of garbage (its contents must not matter), between guards; None where none is needed."""
    nbytes = be.lib.igmc_shortlist_scratch_bytes(g.handle, nq, grid)
    assert nbytes >= 0 and nbytes % 4 == 0
    return (None, None, 0) if nbytes == 0 else (lambda S: (S, S.ptr, nbytes))(filled(be, nbytes // 4, np.uint32, 0xDEADBEEF))


def clamped_counts(be, g, U, nq, okp, exclude_seen, m):
    counts, err = filled(be, nq, np.int64, -7), Guarded(be, np.zeros(1, np.int32), -9)
    be.lib.call('igmc_candidates_count', g.handle, U.ptr, nq, okp, exclude_seen, counts.ptr, err.ptr, None)
    be.sync()
    return np.minimum(counts.host(), m), int(err.host()[0])


def fill_dev(be, g, users, m, s=0, t=0, item_ok=None, exclude_seen=1, grid=0, capacity=None, bad_off=None, with_votes=True):
    """counts, offsets, link_u, link_v, votes (``max(capacity, 1)`` entries each, guards checked), error word of the fill."""
    users = np.ascontiguousarray(users, np.int32)
    nq = len(users)
    U = Guarded(be, users, -3)
    ok = None if item_ok is None else Guarded(be, np.ascontiguousarray(item_ok, np.uint8), 1)
    okp = None if ok is None else ok.ptr
    counts, _ = clamped_counts(be, g, U, nq, okp, exclude_seen, m)
    off = offsets(counts)
    cap = max(int(off[-1]) if capacity is None else capacity, 1)
    O = Guarded(be, off if bad_off is None else np.ascontiguousarray(bad_off, np.int64), -1)
    lu, lv, vo = filled(be, cap, np.int32, -5), filled(be, cap, np.int32, -6), filled(be, cap, np.uint32, 0xABCDEF01)
    err = Guarded(be, np.zeros(1, np.int32), -9)
    S, sp, sb = scratch(be, g, nq, grid)
    be.lib.call('igmc_shortlist_fill', g.handle, U.ptr, nq, okp, exclude_seen, s, t, m, O.ptr, lu.ptr, lv.ptr,
                vo.ptr if with_votes else None, cap, err.ptr, sp, sb, grid, None)
    be.sync()
    for b in (U, O) + (() if ok is None else (ok,)) + (() if S is None else (S,)):
        b.check()
    return counts, off, lu.host(), lv.host(), vo.host(), int(err.host()[0])


def places_dev(be, g, users, q_off, q_id, s=0, t=0, item_ok=None, exclude_seen=1, grid=0, n_query=None, with_votes=True):
    """place, votes (guards checked), error word."""
    users = np.ascontiguousarray(users, np.int32)
    nq = len(users)
    U = Guarded(be, users, -3)
    ok = None if item_ok is None else Guarded(be, np.ascontiguousarray(item_ok, np.uint8), 1)
    QO = Guarded(be, np.ascontiguousarray(q_off, np.int64), -1)
    QI = Guarded(be, np.ascontiguousarray(q_id, np.int32), -2 ** 31)
    n = len(q_id) if n_query is None else n_query
    pl, vo = filled(be, len(q_id), np.int32, -5), filled(be, len(q_id), np.uint32, 0xABCDEF01)
    err = Guarded(be, np.zeros(1, np.int32), -9)
    S, sp, sb = scratch(be, g, nq, grid)
    be.lib.call('igmc_shortlist_places', g.handle, U.ptr, nq, None if ok is None else ok.ptr, exclude_seen, s, t, QO.ptr, QI.ptr,
                n, pl.ptr, vo.ptr if with_votes else None, err.ptr, sp, sb, grid, None)
    be.sync()
    for b in (U, QO, QI) + (() if ok is None else (ok,)) + (() if S is None else (S,)):
        b.check()
    return pl.host(), vo.host(), int(err.host()[0])


def compare(got, want, tag):
    counts, off, lu, lv, vo, e = got
    ru, rv, rw, rc = want
    assert e == 0, (tag, e)
    assert np.array_equal(counts, rc), (tag, counts, rc)
    n = int(off[-1])
    assert n == len(ru) and len(lu) == max(n, 1), tag
    assert np.array_equal(lu[:n], ru) and np.array_equal(lv[:n], rv) and np.array_equal(vo[:n], rw), tag
    assert (lu[n:] == -5).all() and (lv[n:] == -6).all() and (vo[n:] == 0xABCDEF01).all(), tag
    for q in range(len(counts)):
        assert (np.diff(lv[off[q]:off[q + 1]]) > 0).all(), tag          # item ascending: igmc_rank_segments bisects


# ------------------------------------------------------------------ graphs
def corner_graph(n_users, n_items, seed, density=0.3):
    """A random 5-relation graph whose user 0 rated nothing (no seeds) and whose user 1 rated every item (empty C)."""
    A = random_rating_graph(n_users, n_items, density, R, seed).toarray()
    A[0] = 0
    A[1] = 1 + (np.arange(n_items) % R)
    return ssp.csr_matrix(A.astype(np.float32))


def loner_graph(n_users=40, n_items=65):
    """User 2 rated two items that nobody else rated: it has seeds and no co-rater."""
    A = random_rating_graph(n_users, n_items, 0.3, R, 11).toarray()
    A[:, n_items - 2:] = 0
    A[2] = 0
    A[2, n_items - 2:] = [R, 1]
    return ssp.csr_matrix(A.astype(np.float32))


def corner_users(n_users):
    return np.array([1, 0, 3, 3, n_users - 1, 2, 0, 4, 1], np.int32)          # full row, empty row, duplicates


# ------------------------------------------------------------------ 1. segments and votes are the definition
def check_segments(be, n_users, n_items, thresholds=THRESHOLDS, masks=(False, True), excludes=(1, 0), ms=(7,)):
    A = corner_graph(n_users, n_items, 100 + n_items + n_users, 0.3 if n_items < 1000 else 0.05)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users = corner_users(n_users)
    mask = (np.random.default_rng(n_items).random(n_items) < 0.6).astype(np.uint8)
    for s, t in thresholds:
        for masked in masks:
            item_ok = mask if masked else None
            for excl in excludes:
                for m in ms:
                    tag = (n_users, n_items, s, t, masked, excl, m)
                    got = fill_dev(be, g, users, m, s, t, item_ok, excl)
                    compare(got, segments_ref(A, users, m, s, t, item_ok, excl), tag)
                    if s >= R:          # no seeds: every vote is zero and the list is the lowest candidate ids
                        assert not got[4][:int(got[1][-1])].any(), tag
                        for q, u in enumerate(users):
                            c = np.nonzero(candidates_ref(A.tocsr(), int(u), item_ok, excl))[0][:m]
                            assert np.array_equal(got[3][got[1][q]:got[1][q + 1]], c), tag
    g.close()


def check_degenerate_rows(be):
    """An empty row and a full row (``corner_graph``), and a user whose every item is rated by nobody else: no vote at all,
    the lowest candidate ids -- with the seen items kept (``exclude_seen=0``) this also proves the user's own row never votes:
    its own two items would otherwise collect its own co-rating count."""
    A = corner_graph(40, 65, 2)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    counts, off, lu, lv, vo, e = fill_dev(be, g, [0, 1, 0], 6)
    assert e == 0 and counts.tolist() == [6, 0, 6] and lv[:12].tolist() == list(range(6)) * 2 and not vo[:12].any()
    compare(fill_dev(be, g, [1, 0, 1], 6, exclude_seen=0), segments_ref(A, [1, 0, 1], 6, exclude_seen=0), 'full row, seen kept')
    g.close()
    A = loner_graph()
    g = engine.Graph(A, device=be.device, lib=be.lib)
    assert not votes_ref(A, [2], 0, 0).any()
    for excl in (1, 0):
        got = fill_dev(be, g, [2, 3, 2], 5, exclude_seen=excl)
        compare(got, segments_ref(A, [2, 3, 2], 5, exclude_seen=excl), ('loner', excl))
        assert got[3][:5].tolist() == [0, 1, 2, 3, 4] and not got[4][:5].any()
    pl, pv, e = places_dev(be, g, [2], [0, 3], [63, 64, 0], exclude_seen=0)
    assert e == 0 and pl.tolist() == [63, 64, 0] and not pv.any()          # its own items: zero votes, placed by id
    g.close()


# ------------------------------------------------------------------ 2. every kind of m, ties at the threshold
def check_every_m(be, n_users=60, n_items=65):
    A = corner_graph(n_users, n_items, 7)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users = corner_users(n_users)
    n_c = int(candidates_ref(A.tocsr(), 3).sum())
    assert n_c > 3
    for m in (1, n_c - 1, n_c, n_c + 1, M_MAX):
        compare(fill_dev(be, g, users, m), segments_ref(A, users, m), ('m', m))
        got = fill_dev(be, g, users, m, with_votes=False)          # the votes are optional
        assert (got[4] == 0xABCDEF01).all() and np.array_equal(got[3][:int(got[1][-1])], segments_ref(A, users, m)[1])
    g.close()


def block_graph(n_blocks=3, users_per_block=8, items_per_block=40):
    """Blocks of users who all rated the same first half of their block's items; user 0 of every block also rated ONE item of
    the second half.  For a user k > 0 of a block: the unseen second-half item that user 0 rated gets 1 x (half) votes ... and
    every other unseen item of the block ties with dozens of others -- the cut inside the tie is by item id."""
    n_users, n_items = n_blocks * users_per_block, n_blocks * items_per_block
    A = np.zeros((n_users, n_items), np.float32)
    half = items_per_block // 2
    for b in range(n_blocks):
        u0, i0 = b * users_per_block, b * items_per_block
        for k in range(users_per_block):
            A[u0 + k, i0:i0 + half] = 1 + (k + np.arange(half)) % R
            A[u0 + k, i0 + half + 1 + k] = 3          # one item of its own in the second half
        A[u0, i0 + half] = 5
    return ssp.csr_matrix(A)


def check_ties(be):
    A = block_graph()
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users = np.array([1, 9, 17, 0, 2], np.int32)
    V = votes_ref(A, users, 0, 0)
    for q, u in enumerate(users):          # dozens of candidates share a vote count
        c = candidates_ref(A.tocsr(), int(u))
        assert np.bincount(V[q][c]).max() >= 24
    for m in (1, 2, 5, 9, 10, 30, 64, 65, 100):
        compare(fill_dev(be, g, users, m), segments_ref(A, users, m), ('ties', m))
    g.close()
    # every candidate has the same vote count: two users with the same single item; the list is the lowest ids
    B = ssp.csr_matrix(np.array([[1] + [0] * 99, [2] + [0] * 99, [0] * 100], np.float32))
    g = engine.Graph(B, device=be.device, lib=be.lib)
    for m in (1, 50, 98, 99, 100):
        got = fill_dev(be, g, [0, 1, 2], m)
        compare(got, segments_ref(B, [0, 1, 2], m), ('flat', m))
        assert got[3][:min(m, 99)].tolist() == list(range(1, 1 + min(m, 99))) and not got[4][:int(got[1][-1])].any()
    g.close()


# ------------------------------------------------------------------ 3. / 4. degenerate rows, request order, grids
def heavy_light_graph(n_users=300, n_items=64):
    """User 5 rated every item (a heavy walk: every other user is its co-rater), user 6 one item, the rest random."""
    A = random_rating_graph(n_users, n_items, 0.25, R, 3).toarray()
    A[5] = 1 + (np.arange(n_items) % R)
    A[6] = 0
    A[6, 7] = 4
    A[0] = 0
    return ssp.csr_matrix(A.astype(np.float32))


def check_order_and_grids(be, n_users=300, n_items=64, bad_ids=(-1, M_MAX)):
    """More requests than workgroups with ``grid`` forced to 1, 2 and 3: the heavy user is followed by a light one and by an
    out-of-range id -- a ``w`` or vote table left dirty shows in the request behind it --; byte-identical across grids and
    across two launches; duplicated users; the same users in another order keep their segments."""
    A = heavy_light_graph(n_users, n_items)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users = np.array([5, 6, bad_ids[0], 5, 0, 6, 5, bad_ids[1], 6, 17, 5, 6, 6, 0, 5, 200, 6], np.int32)
    good = np.array([u for u in users if 0 <= u < n_users], np.int32)
    m, excl = 9, 0          # (the seen items stay: the heavy user has candidates)
    ru, rv, rw, rc = segments_ref(A, good, m, exclude_seen=excl)
    want_counts = np.zeros(len(users), np.int64)
    want_counts[(users >= 0) & (users < n_users)] = rc
    first = None
    for grid in (1, 2, 3, 0, 1):
        counts, off, lu, lv, vo, e = fill_dev(be, g, users, m, exclude_seen=excl, grid=grid)
        assert e == 2 and np.array_equal(counts, want_counts), (grid, e)
        n = int(off[-1])
        assert np.array_equal(lu[:n], ru) and np.array_equal(lv[:n], rv) and np.array_equal(vo[:n], rw), grid
        blob = lu.tobytes() + lv.tobytes() + vo.tobytes()
        first = first or blob
        assert blob == first, grid
    # places under the same grids
    q_id = np.tile(np.array([7, 0, 63, 30], np.int32), len(users))
    q_off = offsets([4] * len(users))
    want_p, want_v = places_ref(A, np.where((users >= 0) & (users < n_users), users, 0), q_off, q_id, exclude_seen=excl)
    out = ~((users >= 0) & (users < n_users))
    want_p[np.repeat(out, 4)], want_v[np.repeat(out, 4)] = -1, 0
    for grid in (1, 2, 3, 0):
        pl, pv, e = places_dev(be, g, users, q_off, q_id, exclude_seen=excl, grid=grid)
        assert e == 2 and np.array_equal(pl, want_p) and np.array_equal(pv, want_v), grid
    # another order
    perm = np.random.default_rng(1).permutation(len(good))
    c1, o1, lu1, lv1, vo1, e1 = fill_dev(be, g, good, m, exclude_seen=excl, grid=2)
    c2, o2, lu2, lv2, vo2, e2 = fill_dev(be, g, good[perm], m, exclude_seen=excl, grid=3)
    assert (e1, e2) == (0, 0) and np.array_equal(c2, c1[perm])
    src = np.repeat(o1[:-1][perm] - o2[:-1], c2) + np.arange(int(o2[-1]))
    assert np.array_equal(lu2, lu1[src]) and np.array_equal(lv2, lv1[src]) and np.array_equal(vo2, vo1[src])
    g.close()


# ------------------------------------------------------------------ w in LDS / in scratch, votes in LDS / in scratch
def check_w_table_switch(be, delta):
    """``n_users`` = the most users whose ``w`` fits LDS + ``delta``: a sparse graph over that many users whose requests reach
    co-raters at both ends of the table."""
    n_items = 64
    probe = engine.Graph(ssp.csr_matrix(np.ones((1, n_items), np.float32)), device=be.device, lib=be.lib)
    n_users = plan(be, probe, 1)['w_lds_max_users'] + delta
    probe.close()
    rng = np.random.default_rng(5)
    rows = np.concatenate([np.repeat(np.arange(8), 12), np.repeat(np.arange(n_users - 8, n_users), 12),
                           rng.integers(8, n_users - 8, 600)])
    cols = rng.integers(0, n_items, len(rows))
    A = ssp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n_users, n_items))
    A.data = (1 + (A.indices + np.repeat(np.arange(n_users), np.diff(A.indptr))) % R).astype(np.float32)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users = np.array([0, n_users - 1, 3, n_users - 5, 0, int(rows[-1])], np.int32)
    assert plan(be, g, len(users))['w_lds'] == (1 if delta <= 0 else 0)
    for grid in (0, 1):
        for s, t in ((0, 0), (2, 1)):
            compare(fill_dev(be, g, users, 6, s, t, grid=grid), segments_ref(A, users, 6, s, t), ('w', delta, grid, s, t))
    g.close()


# ------------------------------------------------------------------ 5. errors
def _error_case(be):
    A = corner_graph(10, 200, 3)
    return A, engine.Graph(A, device=be.device, lib=be.lib), np.array([4, 3, 7], np.int32)


def check_no_place(be):
    """A capacity one short (bit 0, nothing written past it) and offsets that are not the clamped counts' (bit 2)."""
    A, g, users = _error_case(be)
    m = 20
    ru, rv, rw, rc = segments_ref(A, users, m)
    total = len(ru)
    counts, off, lu, lv, vo, e = fill_dev(be, g, users, m, capacity=total - 1)
    assert e == 1 and np.array_equal(counts, rc)
    assert len(lu) == total - 1 and np.array_equal(lu, ru[:-1]) and np.array_equal(lv, rv[:-1]) and np.array_equal(vo, rw[:-1])
    bad = off.copy()
    bad[1] -= 3
    counts, _, lu, lv, vo, e = fill_dev(be, g, users, m, bad_off=bad)
    assert e == 4
    assert (lu[:bad[1]] == 4).all() and (lu[bad[1]:bad[2] - 3] == 3).all() and (lu[bad[2] - 3:bad[2]] == -5).all()
    assert np.array_equal(lv[bad[2]:], rv[bad[2]:])
    g.close()


def check_bad_user(be, bad_ids):
    A, g, users = _error_case(be)
    for bad in bad_ids:
        us = np.array([4, bad, 7], np.int32)
        counts, off, lu, lv, vo, e = fill_dev(be, g, us, 20)
        ru, rv, rw, rc = segments_ref(A, [4, 7], 20)
        assert e == 2 and counts.tolist() == [rc[0], 0, rc[1]]
        n = int(off[-1])
        assert np.array_equal(lu[:n], ru) and np.array_equal(lv[:n], rv) and np.array_equal(vo[:n], rw)
    g.close()


def check_bad_query_offsets(be, bad, wild=False):
    """``selection_checks.BAD_OFFSETS`` applied to the query offsets of ``igmc_shortlist_places``: bit 0, every answer -1 / 0."""
    assert bad in BAD_OFFSETS
    A, g, users = _error_case(be)
    q_off = np.array([0, 3, 5, 9], np.int64)
    q_id = np.array([1, 50, 199, 4, 4, 0, 100, 150, 199], np.int32)
    pl, pv, e = places_dev(be, g, users, q_off, q_id)
    want = places_ref(A, users, q_off, q_id)
    assert e == 0 and np.array_equal(pl, want[0]) and np.array_equal(pv, want[1])
    q_bad = q_off.copy()
    if bad == 'decreasing':
        q_bad[2] = 2
    elif bad == 'short_end':
        q_bad[3] = 8
    elif bad == 'long_end':
        q_bad[3] = 9 + (1000000 if wild else GUARD // 2)
    elif bad == 'negative':
        q_bad[1] = -5
    else:
        q_bad[0] = 1
    for grid in (0, 1):
        pl, pv, e = places_dev(be, g, users, q_bad, q_id, grid=grid)
        assert e & 1 and (pl == -1).all() and (pv == 0).all(), (bad, e)
    g.close()


def check_refusals(lib):
    """Null and range arguments raise ``RuntimeError`` naming the entry point.  Every call here is refused on the host and
    nothing is launched: the buffers are host arrays whatever the backend."""
    import pytest
    g = engine.Graph(corner_graph(4, 10, 5), lib=lib)
    users, err, off, l, w = np.zeros(2, np.int32), np.zeros(1, np.int32), np.zeros(3, np.int64), np.zeros(64, np.int32), \
        np.zeros(64, np.uint32)
    h, U, E, O, L, W = g.handle, P(users.ctypes.data), P(err.ctypes.data), P(off.ctypes.data), P(l.ctypes.data), P(w.ctypes.data)
    ok = (h, U, 2, None, 1, 0, 0, 5, O, L, L, W, 64, E, None, 0, 0, None)

    def but(base, **kw):
        names = ('g', 'users', 'nq', 'ok', 'excl', 's', 't', 'm', 'off', 'lu', 'lv', 'votes', 'cap', 'err', 'scratch', 'sbytes',
                 'grid', 'stream') if len(base) == 18 else \
                ('g', 'users', 'nq', 'ok', 'excl', 's', 't', 'qoff', 'qid', 'nquery', 'place', 'votes', 'err', 'scratch', 'sbytes',
                 'grid', 'stream')
        a = list(base)
        for k, v in kw.items():
            a[names.index(k)] = v
        return tuple(a)
    for kw in (dict(g=None), dict(users=None), dict(off=None), dict(lu=None), dict(lv=None), dict(err=None), dict(nq=0),
               dict(m=0), dict(m=-1), dict(m=2 ** 31), dict(s=-1), dict(t=-1), dict(cap=0), dict(cap=2 ** 31), dict(grid=-1),
               dict(grid=65537)):
        with pytest.raises(RuntimeError, match='igmc_shortlist_fill'):
            lib.call('igmc_shortlist_fill', *but(ok, **kw))
    okp = (h, U, 2, None, 1, 0, 0, O, L, 3, L, W, E, None, 0, 0, None)
    for kw in (dict(g=None), dict(users=None), dict(qoff=None), dict(qid=None), dict(place=None), dict(err=None), dict(nq=0),
               dict(s=-1), dict(t=-1), dict(nquery=-1), dict(nquery=2 ** 31), dict(grid=65537)):
        with pytest.raises(RuntimeError, match='igmc_shortlist_places'):
            lib.call('igmc_shortlist_places', *but(okp, **kw))
    assert lib.igmc_shortlist_scratch_bytes(None, 2, 0) == -1 and lib.igmc_shortlist_scratch_bytes(g.handle, 0, 0) == -1
    assert lib.igmc_shortlist_scratch_bytes(g.handle, 2, 0) == 0          # both tables in LDS
    g.close()
    # scratch too small / missing: a graph wider than the vote table needs a row per workgroup
    wide = engine.Graph(ssp.csr_matrix(([1.0], ([0], [TILE])), shape=(2, TILE + 1)).astype(np.float32), lib=lib)
    need = lib.igmc_shortlist_scratch_bytes(wide.handle, 2, 0)
    assert need == 2 * 4 * ((TILE + 1 + 63) // 64 * 64)
    big = np.zeros(need // 4, np.uint32)
    for kw in (dict(scratch=None, sbytes=need), dict(scratch=P(big.ctypes.data), sbytes=need - 1)):
        with pytest.raises(RuntimeError, match='igmc_shortlist_fill'):
            lib.call('igmc_shortlist_fill', *but(but(ok, g=wide.handle), **kw))
        with pytest.raises(RuntimeError, match='igmc_shortlist_places'):
            lib.call('igmc_shortlist_places', *but(but(okp, g=wide.handle), **kw))
    wide.close()
    # max_deg_u * max_deg_v reaches 2^31: one row and one column of 46 341 entries each -- refused, never launched
    n = 46341
    rows = np.concatenate([np.zeros(n, np.int64), np.arange(1, n)])
    cols = np.concatenate([np.arange(n), np.zeros(n - 1, np.int64)])
    cross = engine.Graph(ssp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n, n)), lib=lib)
    big = np.zeros(1, np.uint32)
    with pytest.raises(RuntimeError, match='igmc_shortlist_fill.*2\\^31'):
        lib.call('igmc_shortlist_fill', *but(ok, g=cross.handle, scratch=P(big.ctypes.data), sbytes=2 ** 40))
    with pytest.raises(RuntimeError, match='igmc_shortlist_places.*2\\^31'):
        lib.call('igmc_shortlist_places', *but(okp, g=cross.handle, scratch=P(big.ctypes.data), sbytes=2 ** 40))
    cross.close()


# ------------------------------------------------------------------ 6. places
def check_places(be, n_users, n_items, thresholds=((0, 0), (3, 1)), masks=(False, True), excludes=(1, 0)):
    """Every item asked of every request (more than one tile of 256 queries where the graph is wide enough), plus ids out of
    range and duplicates: the index in ``np.lexsort((item, -votes))`` over C, -1 outside C; and ``place < m`` exactly for the
    items of the ``_fill`` segment for the same m."""
    A = corner_graph(n_users, n_items, 100 + n_items + n_users, 0.3 if n_items < 1000 else 0.05)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users = corner_users(n_users)
    rng = np.random.default_rng(n_items)
    mask = (rng.random(n_items) < 0.6).astype(np.uint8)
    every = np.arange(n_items, dtype=np.int32) if n_items <= 1000 else \
        np.unique(np.concatenate([rng.integers(0, n_items, 600), [0, TILE - 1, n_items - 1]])).astype(np.int32)
    per = [np.concatenate([every, [-1, n_items, 3, 3]]).astype(np.int32) for _ in users]
    per[1] = np.zeros(0, np.int32)          # a request that asks nothing
    q_off, q_id = offsets([len(p) for p in per]), np.concatenate(per)
    m = 11
    for s, t in thresholds:
        for masked in masks:
            item_ok = mask if masked else None
            for excl in excludes:
                tag = (n_users, n_items, s, t, masked, excl)
                pl, pv, e = places_dev(be, g, users, q_off, q_id, s, t, item_ok, excl)
                want_p, want_v = places_ref(A, users, q_off, q_id, s, t, item_ok, excl)
                assert e == 0 and np.array_equal(pl, want_p) and np.array_equal(pv, want_v), tag
                assert np.array_equal(places_dev(be, g, users, q_off, q_id, s, t, item_ok, excl, with_votes=False)[0], want_p), tag
                if n_items <= 1000:          # place < m exactly for the items of the segment
                    counts, off, lu, lv, vo, e = fill_dev(be, g, users, m, s, t, item_ok, excl)
                    for q in range(len(users)):
                        if q == 1:
                            continue
                        p = pl[q_off[q]:q_off[q] + n_items]
                        assert np.array_equal(np.nonzero((p >= 0) & (p < m))[0], lv[off[q]:off[q + 1]]), tag
    g.close()
