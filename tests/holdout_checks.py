"""Cases, numpy references and checks of ``igmc_holdout_count`` / ``igmc_holdout_fill`` (``igmc_amd/csrc/holdout.hip``): the
Given-k split of a set of users -- per user a uniform subset of the row stays, the rest is written as held-out links.  Shared by
the emulator test (tests/test_emu_holdout.py) and the GPU test (tests/test_gpu_holdout.py), as ``sampled_candidates_checks.py``
is; every function takes a backend ``be`` of parity_checks and calls the C entry points directly, every buffer a call can
write -- and every input an offset could lead past -- sits between the guards of ``selection_checks.Guarded``.  Every
comparison is exact.

THE DEFINITION, restated here in numpy from the text of ``include/igmc_hip.h`` and ``include/igmc_rng.h`` (the hash functions are
those of ``sampled_candidates_checks``; ``holdout_salt`` is added from the header's text): for request q of user u with a row of
d entries, held = min(hold, max(0, d - keep)) and kept = d - held; the kept entries are the ``kept`` entries of the row with the
smallest ``igmc_sample_key(igmc_holdout_salt(seed, draw, u), item)``; the segment is the others in the row's own order
(relation ascending, then item ascending) as (u, item, relation + 1)."""
import numpy as np
import scipy.sparse as ssp

import sampler_stats as S
import sampled_candidates_checks as SC
from igmc_amd import engine
from sampled_candidates_checks import M64, sample_key, splitmix64
from selection_checks import MANY, Guarded, P, filled, graph_with_corner_rows, offsets

INF = 2 ** 63 - 1          # hold: no limit
HOLDS = [0, 1, 3, INF]
ROW_LENS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 300, 600]          # users 0 .. 10 of the definition's graph
N_USERS, N_ITEMS = 40, 700
KEEPS = sorted({0, 1, 2, 63, 64, 65, 255, 256, 257} | {d + e for d in (300, 600) for e in (-1, 0, 1)})
# (d - 1, d, d + 1 of the rows of 0 .. 257 entries are among the first nine already)
SEED = 1


# ------------------------------------------------------------------ the definition
def holdout_salt(seed, draw, user):
    s = splitmix64((seed ^ 0x484F4C44) & M64)
    s = splitmix64(s ^ draw)
    return splitmix64(s ^ user)


def row_of(A, u):
    """(items, ratings) of user ``u`` in the order the graph stores the row: relation ascending, then item ascending."""
    items = A.indices[A.indptr[u]:A.indptr[u + 1]]
    vals = A.data[A.indptr[u]:A.indptr[u + 1]]
    items, vals = items[vals != 0], vals[vals != 0]
    order = np.lexsort((items, vals))
    return items[order].astype(np.int32), vals[order].astype(np.uint8)


def held_count(d, keep, hold):
    return min(hold, max(0, d - keep))


def split_ref(A, u, keep, hold=INF, seed=SEED, draw=0):
    """(kept items, held items, held ratings) of one user; the held ones in row order."""
    items, vals = row_of(A, u)
    kept = len(items) - held_count(len(items), keep, hold)
    keys = sample_key(holdout_salt(seed, draw, int(u)), items)
    assert len(np.unique(keys)) == len(keys)          # a bijection of the id: no ties
    stay = np.zeros(len(items), bool)
    stay[np.argsort(keys, kind='stable')[:kept]] = True
    return items[stay], items[~stay], vals[~stay]


def segments_ref(A, users, keep, hold=INF, seed=SEED, draw=0):
    """link_u, link_v, rating, counts of a request list."""
    A = A.tocsr()
    us, vs, rs, seen = [], [], [], {}
    for u in users:
        if int(u) not in seen:
            seen[int(u)] = split_ref(A, int(u), keep, hold, seed, draw)[1:]
        v, r = seen[int(u)]
        us.append(np.full(len(v), u, np.int32))
        vs.append(v)
        rs.append(r)
    cat = lambda xs, dt: np.concatenate(xs + [np.zeros(0, dt)]).astype(dt)
    return cat(us, np.int32), cat(vs, np.int32), cat(rs, np.uint8), np.array([len(v) for v in vs], np.int64)


# ------------------------------------------------------------------ the device
def holdout_dev(be, g, users, keep, hold=INF, seed=SEED, draw=0, capacity=None, bad_off=None):
    """counts, offsets, link_u, link_v, rating (``max(capacity, 1)`` entries each, guards checked), error word of either call.
    ``bad_off``: the segment offsets the fill is given in place of the counts' prefix sums."""
    users = np.ascontiguousarray(users, np.int32)
    nq = len(users)
    U = Guarded(be, users, -3)          # (a user read outside the list would raise bit 1)
    counts, err = filled(be, nq, np.int64, -7), Guarded(be, np.zeros(1, np.int32), -9)
    be.lib.call('igmc_holdout_count', g.handle, U.ptr, nq, keep, hold, counts.ptr, err.ptr, None)
    be.sync()
    counts = counts.host()
    off = offsets(counts)
    total = int(off[-1])
    cap = max(total if capacity is None else capacity, 1)
    O = Guarded(be, off if bad_off is None else np.ascontiguousarray(bad_off, np.int64), -1)
    lu, lv, rt = filled(be, cap, np.int32, -5), filled(be, cap, np.int32, -6), filled(be, cap, np.uint8, 99)
    err2 = Guarded(be, np.zeros(1, np.int32), -9)
    be.lib.call('igmc_holdout_fill', g.handle, U.ptr, nq, keep, hold, seed, draw, O.ptr, lu.ptr, lv.ptr, rt.ptr, cap, err2.ptr,
                None)
    be.sync()
    U.check()
    O.check()
    return counts, off, lu.host(), lv.host(), rt.host(), int(err.host()[0]), int(err2.host()[0])


def compare(got, want, tag):
    """Counts, offsets and the three arrays element for element; the sentinels behind the last segment."""
    counts, off, lu, lv, rt, e1, e2 = got
    ru, rv, rr, rc = want
    assert e1 == 0 and e2 == 0, (tag, e1, e2)
    assert np.array_equal(counts, rc), (tag, counts, rc)
    assert off[0] == 0 and np.array_equal(off[1:], np.cumsum(rc)), tag
    n = int(off[-1])
    assert n == len(ru) and len(lu) == max(n, 1), tag
    assert np.array_equal(lu[:n], ru) and np.array_equal(lv[:n], rv) and np.array_equal(rt[:n], rr), tag
    assert (lu[n:] == -5).all() and (lv[n:] == -6).all() and (rt[n:] == 99).all(), tag


# ------------------------------------------------------------------ 1. the segments are the definition
def definition_graph():
    """``N_USERS`` x ``N_ITEMS``: users 0 .. 10 have rows of ``ROW_LENS`` entries, the others random ones; ratings over five
    relations, so that the row's order is not the item order."""
    rng = np.random.default_rng(5)
    lens = ROW_LENS + rng.integers(1, 200, N_USERS - len(ROW_LENS)).tolist()
    rows, cols = [], []
    for u, d in enumerate(lens):
        rows.append(np.full(d, u))
        cols.append(np.sort(rng.choice(N_ITEMS, d, replace=False)))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = (1 + rng.integers(0, 5, len(rows))).astype(np.float32)
    A = ssp.csr_matrix((vals, (rows, cols)), shape=(N_USERS, N_ITEMS))
    assert np.diff(A.indptr)[:len(ROW_LENS)].tolist() == ROW_LENS
    return A


def definition_users():
    """Every user once, in an order that is not the ids', and users 9 and 3 a second time."""
    return np.concatenate([np.random.default_rng(6).permutation(N_USERS), [9, 3]]).astype(np.int32)


def check_definition(be, keeps=KEEPS, holds=HOLDS):
    """Every keep x hold: counts, offsets, link_u, link_v and rating are the restatement's; kept and held partition the row."""
    A = definition_graph()
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users = definition_users()
    for keep in keeps:
        for hold in holds:
            tag = (keep, hold)
            got = holdout_dev(be, g, users, keep, hold)
            compare(got, segments_ref(A, users, keep, hold), tag)
            counts, off, lu, lv, rt = got[:5]
            for q, u in enumerate(users):
                items, vals = row_of(A, int(u))
                d = len(items)
                assert counts[q] == held_count(d, keep, hold), tag
                held = lv[off[q]:off[q + 1]]
                kept = split_ref(A, int(u), keep, hold)[0]
                assert len(np.intersect1d(kept, held)) == 0, tag
                assert np.array_equal(np.sort(np.concatenate([kept, held])), np.sort(items)), tag
                # the row's own order: a subsequence of the row, with the row's ratings
                at = np.nonzero(np.isin(items, held))[0]
                assert np.array_equal(items[at], held) and np.array_equal(vals[at], rt[off[q]:off[q + 1]]), tag
                if d <= keep:
                    assert counts[q] == 0, tag          # a user with no more than `keep` ratings loses nothing
            if (keep, hold) == (1, 1):                  # leave-one-out: one link of every user with two or more, none bare
                assert np.array_equal(counts, np.array([min(1, max(0, len(row_of(A, int(u))[0]) - 1)) for u in users]))
    g.close()


def check_nested(be, users=(4, 7, 10)):
    """``hold`` = no limit: kept(k) is a subset of kept(k + 1), one entry larger, over keep = 0 .. d."""
    A = definition_graph()
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users = np.array(users, np.int32)
    rows = [row_of(A, int(u))[0] for u in users]
    before = [np.zeros(0, np.int32) for _ in users]
    for keep in range(max(len(r) for r in rows) + 1):
        counts, off, lu, lv, rt, e1, e2 = holdout_dev(be, g, users, keep)
        assert (e1, e2) == (0, 0)
        for q, row in enumerate(rows):
            kept = np.setdiff1d(row, lv[off[q]:off[q + 1]])
            assert len(kept) == min(keep, len(row))
            assert len(np.setdiff1d(before[q], kept)) == 0, (keep, q)
            before[q] = kept
    g.close()


# ------------------------------------------------------------------ 2. the selection paths
def one_row_graph(n_items, d):
    """One user who rated the first ``d`` of ``n_items`` items, ratings over five relations."""
    cols = np.arange(d)
    vals = (1 + (cols * 7 + cols // 5) % 5).astype(np.float32)
    return ssp.csr_matrix((vals, (np.zeros(d, np.int64), cols)), shape=(1, n_items))


def deciding_byte_count(A, u, kept, seed=SEED, draw=0):
    """How many keys of the row share the top byte of the ``kept``-th smallest."""
    keys = np.sort(sample_key(holdout_salt(seed, draw, u), row_of(A.tocsr(), u)[0]))
    return int((keys >> np.uint64(24) == keys[kept - 1] >> np.uint64(24)).sum())


def check_long_row(be, more_than=256):
    """A row of 100 000 entries -- longer than anything LDS could hold -- split in half: more than ``more_than`` keys share
    the deciding top byte (the parked list's bound: 256, or what the emulator was told through IGMC_SAMPLE_PARK), so the
    radix passes run."""
    A = one_row_graph(100003, 100000).tocsr()
    keep = 50000
    assert deciding_byte_count(A, 0, keep) > max(more_than, 256)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users = np.array([0], np.int32)
    compare(holdout_dev(be, g, users, keep), segments_ref(A, users, keep), 'long row')
    g.close()


def park_bound_case():
    """(row length d, {256: keeps, 257: keeps}): a row of the items 0 .. d - 1 of user 0 in which one top byte holds exactly 256
    keys and another exactly 257, and per count the ``keep`` that makes the first and the last key of that byte the threshold
    -- searched on the CPU."""
    top_all = (sample_key(holdout_salt(SEED, 0, 0), np.arange(70000)) >> np.uint64(24)).astype(np.int64)
    for d in range(65000, 70000):
        hist = np.bincount(top_all[:d], minlength=256)
        if (hist == 256).any() and (hist == 257).any():
            before = np.cumsum(hist) - hist
            keeps = {}
            for count in (256, 257):
                b = int(np.nonzero(hist == count)[0][0])
                keeps[count] = (int(before[b]) + 1, int(before[b]) + count)
            return d, keeps
    raise AssertionError('no row length with top bytes of exactly 256 and 257 keys')


def check_park_bound(be):
    """The edge of "park or radix" (``kth_key.h``: ``kth_parks``): a deciding byte of exactly 256 keys is parked, one of
    exactly 257 goes through the radix passes, and either way the threshold may be the first or the last key of its byte."""
    d, keeps = park_bound_case()
    A = one_row_graph(d + 3, d).tocsr()
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users = np.array([0], np.int32)
    for count, ks in sorted(keeps.items()):
        for keep in ks:
            assert deciding_byte_count(A, 0, keep) == count
            compare(holdout_dev(be, g, users, keep), segments_ref(A, users, keep), (count, keep))
    g.close()


# ------------------------------------------------------------------ 3. many requests, any order
def check_many_users(be, n_requests=MANY, permuted=True):
    """``MANY`` requests over a 12 x 20 graph (the fill is capped at 65 536 workgroups: some take a second request), and
    (``permuted``) the same requests in another order: every user's segment is the same wherever it lands."""
    A = graph_with_corner_rows(12, 20, 8).tocsr()
    g = engine.Graph(A, device=be.device, lib=be.lib)
    rng = np.random.default_rng(9)
    users = rng.integers(0, 12, n_requests).astype(np.int32)
    keep = 3
    got = holdout_dev(be, g, users, keep)
    compare(got, segments_ref(A, users, keep), 'many')
    if permuted:
        perm = rng.permutation(n_requests)
        counts, off, lu, lv, rt = got[:5]
        counts2, off2, lu2, lv2, rt2, e1, e2 = holdout_dev(be, g, users[perm], keep)
        assert (e1, e2) == (0, 0) and np.array_equal(counts2, counts[perm])
        src = np.repeat(off[:-1][perm] - off2[:-1], counts2) + np.arange(int(off2[-1]))          # where each entry came from
        assert np.array_equal(lu2, lu[src]) and np.array_equal(lv2, lv[src]) and np.array_equal(rt2, rt[src])
    g.close()


# ------------------------------------------------------------------ 4. errors
def _error_case(be):
    A = graph_with_corner_rows(10, 200, 3).tocsr()
    g = engine.Graph(A, device=be.device, lib=be.lib)
    return A, g, np.array([4, 1, 7], np.int32), 5


def check_no_place(be):
    """A capacity one short (bit 0, nothing written past it, the complete segments intact) and offsets that are not the
    counts' (bit 2)."""
    A, g, users, keep = _error_case(be)
    ru, rv, rr, rc = segments_ref(A, users, keep)
    total = len(ru)
    assert rc.min() > 3
    counts, off, lu, lv, rt, e1, e2 = holdout_dev(be, g, users, keep, capacity=total - 1)
    assert e1 == 0 and e2 == 1 and np.array_equal(counts, rc)
    assert len(lu) == total - 1 and np.array_equal(lu, ru[:-1]) and np.array_equal(lv, rv[:-1]) and np.array_equal(rt, rr[:-1])
    bad = off.copy()
    bad[1] -= 3
    counts, _, lu, lv, rt, e1, e2 = holdout_dev(be, g, users, keep, bad_off=bad)
    assert e1 == 0 and e2 == 4
    assert np.array_equal(lv[:bad[1]], rv[:bad[1]])                                          # request 0: cut at its end
    assert np.array_equal(lv[bad[1]:bad[2] - 3], rv[off[1]:off[2]])                          # request 1: three places early
    assert (lu[bad[2] - 3:bad[2]] == -5).all() and (rt[bad[2] - 3:bad[2]] == 99).all()       # ... nothing behind it
    assert np.array_equal(lv[bad[2]:], rv[bad[2]:]) and np.array_equal(rt[bad[2]:], rr[bad[2]:])
    g.close()


def check_bad_user(be, bad_ids):
    """A user id out of range: bit 1 from either launch, an empty segment, the other requests intact."""
    A, g, users, keep = _error_case(be)
    for bad in bad_ids:
        us = np.array([4, bad, 7], np.int32)
        counts, off, lu, lv, rt, e1, e2 = holdout_dev(be, g, us, keep)
        ru, rv, rr, rc = segments_ref(A, [4, 7], keep)
        assert e1 == 2 and e2 == 2
        assert counts.tolist() == [rc[0], 0, rc[1]]
        n = int(off[-1])
        assert np.array_equal(lu[:n], ru) and np.array_equal(lv[:n], rv) and np.array_equal(rt[:n], rr)
    g.close()


def check_refusals(lib):
    """Null and range arguments raise ``RuntimeError`` naming the entry point.  Every call here is refused on the host and
    nothing is launched: the buffers are host arrays whatever the backend.  ``nq = 0`` is accepted and launches nothing."""
    import pytest
    g = engine.Graph(graph_with_corner_rows(4, 10, 5), lib=lib)
    users, cnt, err = np.zeros(2, np.int32), np.zeros(2, np.int64), np.zeros(1, np.int32)
    off, l, r = np.zeros(3, np.int64), np.zeros(64, np.int32), np.zeros(64, np.uint8)
    h, U, C, E, O, L, R = g.handle, P(users.ctypes.data), P(cnt.ctypes.data), P(err.ctypes.data), P(off.ctypes.data), \
        P(l.ctypes.data), P(r.ctypes.data)
    for args in ((None, U, 2, 1, 1, C, E, None), (h, None, 2, 1, 1, C, E, None), (h, U, 2, 1, 1, None, E, None),
                 (h, U, 2, 1, 1, C, None, None), (h, U, -1, 1, 1, C, E, None), (h, U, 2, -1, 1, C, E, None),
                 (h, U, 2, 1, -1, C, E, None)):
        with pytest.raises(RuntimeError, match='igmc_holdout_count'):
            lib.call('igmc_holdout_count', *args)
    for args in ((None, U, 2, 1, 1, 1, 0, O, L, L, R, 64, E, None), (h, None, 2, 1, 1, 1, 0, O, L, L, R, 64, E, None),
                 (h, U, 2, 1, 1, 1, 0, None, L, L, R, 64, E, None), (h, U, 2, 1, 1, 1, 0, O, None, L, R, 64, E, None),
                 (h, U, 2, 1, 1, 1, 0, O, L, None, R, 64, E, None), (h, U, 2, 1, 1, 1, 0, O, L, L, None, 64, E, None),
                 (h, U, 2, 1, 1, 1, 0, O, L, L, R, 64, None, None), (h, U, -1, 1, 1, 1, 0, O, L, L, R, 64, E, None),
                 (h, U, 2, -1, 1, 1, 0, O, L, L, R, 64, E, None), (h, U, 2, 1, -1, 1, 0, O, L, L, R, 64, E, None),
                 (h, U, 2, 1, 1, 1, 0, O, L, L, R, -1, E, None)):
        with pytest.raises(RuntimeError, match='igmc_holdout_fill'):
            lib.call('igmc_holdout_fill', *args)
    lib.call('igmc_holdout_count', h, U, 0, 1, 1, C, E, None)
    lib.call('igmc_holdout_fill', h, U, 0, 1, 1, 1, 0, O, L, L, R, 64, E, None)
    assert not cnt.any() and not err.any() and not l.any() and not r.any()
    g.close()


# ------------------------------------------------------------------ 5. the reduced graph
REDUCED = [(0, INF), (1, 1), (5, INF), (64, 3)]


def check_reduced_graph(be, keep, hold):
    """``graph.updated(held_u, held_v, zeros)`` is ``engine.Graph`` of the matrix without the restatement's held entries:
    arrays, nnz, max_rel and both longest-row figures; the original graph stays as it was."""
    A = definition_graph()
    g = engine.Graph(A, device=be.device, lib=be.lib)
    was, was_info = g.download(), g.info()
    users = np.arange(N_USERS, dtype=np.int32)
    counts, off, lu, lv, rt, e1, e2 = holdout_dev(be, g, users, keep, hold)
    n = int(off[-1])
    ru, rv, rr, rc = segments_ref(A, users, keep, hold)
    assert (e1, e2) == (0, 0) and n == len(ru)
    new = g.updated(lu[:n], lv[:n], np.zeros(n, np.int64))
    B = A.tolil(copy=True)
    B[ru, rv] = 0
    B = B.tocsr()
    B.eliminate_zeros()
    want = engine.Graph(B, device=be.device, lib=be.lib)
    assert new.info() == want.info() and new.nnz == A.nnz - n
    got_arrays, want_arrays = new.download(), want.download()
    for k in want_arrays:
        assert got_arrays[k].tobytes() == want_arrays[k].tobytes(), (keep, hold, k)
    now = g.download()
    assert g.info() == was_info and all(now[k].tobytes() == was[k].tobytes() for k in was)
    for x in (new, want, g):
        x.close()


# ------------------------------------------------------------------ 6. distribution
N_DRAWS = SC.N_DRAWS          # distinct users 0 .. 4199, each one split that keeps K = 100 of the same n items


def stats_graph(n):
    """``N_DRAWS`` users who all rated the same ``n`` items 7 + 3 j, ratings over five relations."""
    rows = np.repeat(np.arange(N_DRAWS), n)
    j = np.tile(np.arange(n), N_DRAWS)
    return ssp.csr_matrix((1.0 + (rows + j) % 5, (rows, 7 + 3 * j)), shape=(N_DRAWS, 7 + 3 * n)).astype(np.float32)


def inclusion_ref(n, draw):
    X = np.zeros((N_DRAWS, n), bool)
    ids = 7 + 3 * np.arange(n)
    for u in range(N_DRAWS):
        X[u, np.argsort(sample_key(holdout_salt(SEED, draw, u), ids), kind='stable')[:S.K]] = True
    return X


def inclusion_dev(be, g, n, draw):
    """The device's kept-set inclusion matrix: ONE count and one fill launch for all ``N_DRAWS`` users."""
    users = np.arange(N_DRAWS, dtype=np.int32)
    counts, off, lu, lv, rt, e1, e2 = holdout_dev(be, g, users, S.K, seed=SEED, draw=draw)
    assert (e1, e2) == (0, 0) and (counts == n - S.K).all() and np.array_equal(lu, np.repeat(users, n - S.K))
    assert ((lv - 7) % 3 == 0).all()
    X = np.ones((N_DRAWS, n), bool)
    X[lu, (lv - 7) // 3] = False
    assert (X.sum(1) == S.K).all()
    return X


def check_distribution(be, n):
    """The kept sets of 4200 users are the restatement's bit for bit, and distributed like uniform k-subsets under the bounds
    of ``sampled_candidates_checks`` (p > 1e-3, |z| < 5 for id-rank, pairs and draw against draw)."""
    g = engine.Graph(stats_graph(n), device=be.device, lib=be.lib)
    X0, X1 = inclusion_dev(be, g, n, 0), inclusion_dev(be, g, n, 1)
    g.close()
    assert np.array_equal(X0, inclusion_ref(n, 0)) and np.array_equal(X1, inclusion_ref(n, 1))          # bit for bit
    assert not np.array_equal(X0, X1)
    z = SC.z_scores(X0, X1, n)
    print('n = %d: singles p = %.3f, z_rank = %+.2f, z_pairs = %+.2f, z_draws = %+.2f' % (n, z['p'], z['z_rank'], z['z_pairs'],
                                                                                        z['z_draws']))
    assert SC.within_bounds(z), z
