"""``igmc_rank_segments`` / ``igmc_rank_metrics`` (``igmc_amd/csrc/ranking.hip``) on the CPU emulation of the HIP sources: the rank
of a queried id is its place in ``np.lexsort((idx, np.where(np.isnan(k), np.inf, -k)))`` of its segment whatever the geometry
(and the place ``igmc_select_segments`` gives it), ids a segment does not hold come back as -1 / -1, the metric sums are their
numpy float64 restatement and do not depend on the grid, and inconsistent query offsets are reported, not followed."""
import numpy as np
import pytest

from helpers import emu_lib
from igmc_amd import engine

P = engine._p
GUARD = 16
LENS = [0, 1, 63, 64, 65, 1000, 5000]          # 5000: past the 4096 words candidates.hip stages, and the 2048 ranking.hip does


def make_segments(lens, seed):
    """Keys quantised to five values (ties everywhere) with NaN, +-0.0 and +-inf sprinkled in; ids strictly ascending inside
    every segment, with gaps (so that absent ids exist between present ones)."""
    rng = np.random.default_rng(seed)
    n = int(sum(lens))
    keys = rng.integers(1, 6, n).astype(np.float32)
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf], np.float32)
    where = rng.random(n) < 0.15
    keys[where] = special[rng.integers(0, 5, int(where.sum()))]
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    ids = np.concatenate([np.cumsum(rng.integers(1, 4, m)) for m in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return keys, ids, off


def descending_order(k, idx):
    """THE ORDER of ``igmc_select_segments`` (igmc_hip.h): key descending, index ascending, EVERY NaN behind EVERY number.
    Its usual restatement ``np.lexsort((idx, np.where(np.isnan(k), np.inf, -k)))`` maps -inf and NaN to the same value and
    then orders the two among themselves by index, so it is that order only for segments without a -inf key; these segments
    hold both, and the NaNs are set behind the numbers by a key of their own."""
    nan = np.isnan(k)
    order = np.lexsort((idx, np.where(nan, 0.0, -k), nan))
    if not np.isneginf(k).any():
        assert np.array_equal(order, np.lexsort((idx, np.where(nan, np.inf, -k))))
    return order


def rank_ref(keys, ids, off, q_off, q_id):
    """(pos, rank) by numpy: per segment the inverse permutation of the descending lexsort."""
    pos, rank = np.full(len(q_id), -1, np.int32), np.full(len(q_id), -1, np.int32)
    for s in range(len(off) - 1):
        lo, hi = off[s], off[s + 1]
        k, idx = keys[lo:hi], np.arange(lo, hi)
        order = descending_order(k, idx)
        place = np.argsort(order)
        where = {int(v): lo + i for i, v in enumerate(ids[lo:hi])}
        for q in range(q_off[s], q_off[s + 1]):
            p = where.get(int(q_id[q]), -1)
            if p >= 0:
                pos[q], rank[q] = p, place[p - lo]
    return pos, rank


def rank_dev(lib, keys, ids, off, q_off, q_id, geometry=0, nq=None):
    nq = len(q_id) if nq is None else nq
    pos, rank = np.full(len(q_id) + GUARD, -7, np.int32), np.full(len(q_id) + GUARD, -8, np.int32)
    err = np.zeros(1, np.int32)
    lib.call('igmc_rank_segments', P(keys), P(ids), len(keys), P(off), len(off) - 1, P(q_off), P(q_id), nq, P(pos), P(rank),
             P(err), geometry, None)
    return pos, rank, int(err[0])


def check_all_geometries(lib, keys, ids, off, q_off, q_id, tag):
    want_pos, want_rank = rank_ref(keys, ids, off, q_off, q_id)
    nq = len(q_id)
    first = None
    for geometry in (0, 1, 3, 64):
        pos, rank, err = rank_dev(lib, keys, ids, off, q_off, q_id, geometry)
        assert err == 0, (tag, geometry)
        assert np.array_equal(pos[:nq], want_pos), (tag, geometry)
        assert np.array_equal(rank[:nq], want_rank), (tag, geometry)
        assert (pos[nq:] == -7).all() and (rank[nq:] == -8).all(), (tag, geometry)      # guard elements untouched
        if first is None:
            first = (pos.tobytes(), rank.tobytes())
        assert (pos.tobytes(), rank.tobytes()) == first, (tag, geometry)
    return want_pos, want_rank


def queries(kind, keys, ids, off, seed):
    """Per-segment query lists of one kind -> (q_off, q_id)."""
    rng = np.random.default_rng(seed)
    lists = []
    for s in range(len(off) - 1):
        seg = ids[off[s]:off[s + 1]]
        if kind == 'none' or (len(seg) == 0 and kind != 'absent'):
            q = np.zeros(0, np.int32)
        elif kind == 'one':
            q = seg[rng.integers(0, len(seg), 1)]
        elif kind == 'every':
            q = rng.permutation(seg)          # (in any order)
        elif kind == 'three_hundred':         # more than one tile of 256: duplicates where the segment is shorter
            q = seg[rng.integers(0, len(seg), 300)]
        elif kind == 'absent':                # ids in the gaps, below the first and past the last
            gaps = np.setdiff1d(np.arange(-2, (seg[-1] if len(seg) else 0) + 3), seg)
            q = gaps[rng.integers(0, len(gaps), 5)]
        elif kind == 'duplicates':
            q = np.repeat(seg[rng.integers(0, len(seg), 3)], 4)
        elif kind == 'mixed':                 # present, absent and repeated ids side by side; every third segment asks nothing
            gaps = np.setdiff1d(np.arange(0, seg[-1] + 2), seg)
            q = np.concatenate([seg[rng.integers(0, len(seg), 7)], gaps[rng.integers(0, len(gaps), 3)], seg[:1], seg[:1]])
            q = rng.permutation(q) if s % 3 else q[:0]
        lists.append(np.asarray(q, np.int32))
    q_off = np.zeros(len(off), np.int64)
    q_off[1:] = np.cumsum([len(q) for q in lists])
    q_id = np.concatenate(lists + [np.zeros(0, np.int32)]).astype(np.int32)
    return q_off, q_id


@pytest.mark.parametrize('kind', ['none', 'one', 'every', 'three_hundred', 'absent', 'duplicates', 'mixed'])
def test_ranks_are_the_numpy_order_under_every_geometry(kind):
    lib = emu_lib()
    keys, ids, off = make_segments(LENS, 11)
    q_off, q_id = queries(kind, keys, ids, off, 5)
    if len(q_id) == 0:          # the buffers still exist
        q_id = np.zeros(1, np.int32)
        for geometry in (0, 1, 3, 64):
            pos, rank, err = rank_dev(lib, keys, ids, off, q_off, q_id, geometry, nq=0)
            assert err == 0 and (pos == -7).all() and (rank == -8).all()
        return
    want_pos, want_rank = check_all_geometries(lib, keys, ids, off, q_off, q_id, kind)
    if kind == 'absent':
        assert (want_pos == -1).all() and (want_rank == -1).all()
    if kind == 'every':           # every place of every segment exactly once
        for s in range(len(off) - 1):
            assert sorted(want_rank[q_off[s]:q_off[s + 1]].tolist()) == list(range(off[s + 1] - off[s]))
    if kind == 'duplicates':
        assert (want_rank.reshape(-1, 4) == want_rank.reshape(-1, 4)[:, :1]).all() and (want_rank >= 0).all()


def test_a_nan_scored_query_and_signed_zeros_are_ranked_by_the_word_order():
    lib = emu_lib()
    keys = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, -np.nan, 1.0, -0.0], np.float32)
    ids = np.arange(10, 18, dtype=np.int32)
    off, q_off = np.array([0, 8], np.int64), np.array([0, 8], np.int64)
    pos, rank, err = rank_dev(lib, keys, ids, off, q_off, ids.copy())
    # the order of the segment: +inf, 1, the zeros by position, -inf, the NaNs by position = positions 3, 6, 1, 2, 7, 4, 0, 5
    assert err == 0 and pos[:8].tolist() == list(range(8))
    assert rank[:8].tolist() == [6, 2, 3, 0, 5, 7, 1, 4]


def test_ranks_agree_with_the_selection():
    """Querying the ids at ``idx_out[s, r]`` of ``igmc_select_segments(num=64)`` returns rank r for every r < count."""
    lib = emu_lib()
    keys, ids, off = make_segments(LENS, 12)
    ns, num = len(off) - 1, 64
    nbytes = lib.igmc_select_segments_scratch_bytes(ns, num, 0)
    scratch = np.zeros(nbytes // 8, np.uint64)
    idx, cnt = np.full(ns * num, -9, np.int32), np.full(ns, -9, np.int32)
    lib.call('igmc_select_segments', P(keys), P(off), ns, num, P(idx), None, P(cnt), P(scratch), nbytes, 0, None)
    idx = idx.reshape(ns, num)
    assert np.array_equal(cnt, np.minimum(np.diff(off), num))
    q_off = np.zeros(ns + 1, np.int64)
    q_off[1:] = np.cumsum(cnt)
    q_id = np.concatenate([ids[idx[s, :cnt[s]]] for s in range(ns)]).astype(np.int32)
    for geometry in (0, 2):
        pos, rank, err = rank_dev(lib, keys, ids, off, q_off, q_id, geometry)
        assert err == 0
        for s in range(ns):
            assert rank[q_off[s]:q_off[s + 1]].tolist() == list(range(cnt[s]))
            assert np.array_equal(pos[q_off[s]:q_off[s + 1]], idx[s, :cnt[s]])


# ------------------------------------------------------------------ metrics
def metrics_dev(lib, rank, q_off, ks, rel=None, grid=0, nq=None):
    ns, nk = len(q_off) - 1, len(ks)
    nq = len(rank) if nq is None else nq
    cnt = np.full(ns * (2 + nk) + GUARD, -7, np.int32)
    dcg = np.full(ns * 2 * nk + GUARD, -7.0, np.float64)
    err = np.zeros(1, np.int32)
    lib.call('igmc_rank_metrics', P(rank), P(q_off), P(rel), nq, ns, P(np.asarray(ks, np.int32)), nk, P(cnt), P(dcg), P(err),
             grid, None)
    assert (cnt[ns * (2 + nk):] == -7).all() and (dcg[ns * 2 * nk:] == -7.0).all()
    return cnt[:ns * (2 + nk)].reshape(ns, 2 + nk), dcg[:ns * 2 * nk].reshape(ns, 2 * nk), int(err[0])


def metrics_ref(rank, q_off, ks, rel=None):
    ns, nk = len(q_off) - 1, len(ks)
    cnt, dcg = np.zeros((ns, 2 + nk), np.int32), np.zeros((ns, 2 * nk), np.float64)
    for s in range(ns):
        r = rank[q_off[s]:q_off[s + 1]].astype(np.int64)
        keep = r >= 0
        if rel is not None:
            keep &= rel[q_off[s]:q_off[s + 1]] != 0
        r = np.sort(r[keep])
        cnt[s, 0], cnt[s, 1] = len(r), r[0] if len(r) else -1
        for j, K in enumerate(ks):
            hit = r[r < K]
            cnt[s, 2 + j] = len(hit)
            dcg[s, j] = (1.0 / np.log2(hit.astype(np.float64) + 2.0)).sum()
            dcg[s, nk + j] = (1.0 / np.log2(np.arange(min(K, len(r)), dtype=np.float64) + 2.0)).sum()
    return cnt, dcg


def metric_case(seed):
    """Users with no query, with irrelevant queries only, with ranks of -1 only, with one query, with hundreds."""
    rng = np.random.default_rng(seed)
    per_user = [0, 5, 4, 1, 64, 65, 300, 0, 7, 129] + rng.integers(0, 40, 30).tolist()
    q_off = np.zeros(len(per_user) + 1, np.int64)
    q_off[1:] = np.cumsum(per_user)
    nq = int(q_off[-1])
    rank = rng.integers(0, 600, nq).astype(np.int32)
    rank[rng.random(nq) < 0.2] = -1
    rel = (rng.random(nq) < 0.7).astype(np.uint8)
    rel[q_off[1]:q_off[2]] = 0                 # user 1: all irrelevant
    rank[q_off[2]:q_off[3]] = -1               # user 2: no query has a place
    rank[q_off[4]:q_off[4] + 3] = [0, 1, 2]
    return rank, q_off, rel


@pytest.mark.parametrize('ks', [(1, 5, 10, 1000), (10,), (1, 2, 3, 4, 5, 6, 7, 2 ** 31 - 1)])
def test_metric_sums_are_their_numpy_restatement_and_do_not_depend_on_the_grid(ks):
    lib = emu_lib()
    rank, q_off, rel = metric_case(3)
    for r in (rel, None):
        want_cnt, want_dcg = metrics_ref(rank, q_off, ks, r)
        cnt, dcg, err = metrics_dev(lib, rank, q_off, ks, r)
        assert err == 0
        assert np.array_equal(cnt, want_cnt)
        np.testing.assert_allclose(dcg, want_dcg, rtol=1e-12, atol=0)
        for grid in (1, 3):          # fewer workgroups than users: the same bits
            cnt2, dcg2, err = metrics_dev(lib, rank, q_off, ks, r, grid)
            assert err == 0 and cnt2.tobytes() == cnt.tobytes() and dcg2.tobytes() == dcg.tobytes()
    cnt, dcg, _ = metrics_dev(lib, rank, q_off, ks, rel)
    assert cnt[0].tolist() == [0, -1] + [0] * len(ks) and cnt[1].tolist() == cnt[0].tolist() == cnt[2].tolist()
    assert not dcg[:3].any()
    assert (dcg[:, :len(ks)] <= dcg[:, len(ks):] * (1 + 1e-12)).all()          # no list beats the ideal one


# ------------------------------------------------------------------ errors
@pytest.mark.parametrize('bad', ['decreasing', 'short_end', 'long_end', 'negative', 'first_not_zero'])
def test_inconsistent_query_offsets_are_reported_and_nothing_is_touched_out_of_range(bad):
    lib = emu_lib()
    keys, ids, off = make_segments([40, 50, 60, 70], 13)
    q_off, q_id = np.array([0, 3, 5, 9, 12], np.int64), np.concatenate([ids[0:3], ids[40:42], ids[90:94], ids[150:153]])
    pos, rank, err = rank_dev(lib, keys, ids, off, q_off, q_id)
    assert err == 0 and (rank[:12] >= 0).all()
    q_bad = q_off.copy()
    if bad == 'decreasing':
        q_bad[2] = 2
    elif bad == 'short_end':
        q_bad[4] = 11
    elif bad == 'long_end':
        q_bad[4] = 12 + 1000000
    elif bad == 'negative':
        q_bad[1] = -5
    else:
        q_bad[0] = 1
    for geometry in (0, 1, 64):
        pos, rank, err = rank_dev(lib, keys, ids, off, q_bad, q_id, geometry)
        assert err & 1
        assert (pos[:12] == -1).all() and (rank[:12] == -1).all()          # the queries cannot be told apart: -1 / -1
        assert (pos[12:] == -7).all() and (rank[12:] == -8).all()
    cnt, dcg, err = metrics_dev(lib, np.arange(12, dtype=np.int32), q_bad, (5,))
    if bad not in ('short_end', 'first_not_zero'):          # (what one user's range shows: a range outside the queries)
        assert err & 1
    # a segment outside the keys is empty and reported; the other segments are answered
    s_bad = off.copy()
    s_bad[4] = len(keys) + 1000
    pos, rank, err = rank_dev(lib, keys, ids, s_bad, q_off, q_id)
    want_pos, want_rank = rank_ref(keys, ids, off, q_off, q_id)
    assert err == 2 and np.array_equal(pos[:9], want_pos[:9]) and np.array_equal(rank[:9], want_rank[:9])
    assert (pos[9:12] == -1).all() and (rank[9:12] == -1).all()


def test_rank_entry_points_refuse_bad_arguments():
    lib = emu_lib()
    keys, ids = np.zeros(16, np.float32), np.arange(16, dtype=np.int32)
    off, q_off, q = np.array([0, 16], np.int64), np.array([0, 2], np.int64), np.array([3, 4], np.int32)
    pos, rank, err = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(1, np.int32)
    good = [P(keys), P(ids), 16, P(off), 1, P(q_off), P(q), 2, P(pos), P(rank), P(err), 0, None]
    lib.call('igmc_rank_segments', *good)
    assert err[0] == 0 and pos.tolist() == [3, 4]
    for i, v in ((0, None), (1, None), (3, None), (5, None), (6, None), (8, None), (9, None), (10, None), (2, 0), (2, 2 ** 31),
                 (4, 0), (7, -1), (11, -1), (11, 65)):
        args = list(good)
        args[i] = v
        with pytest.raises(RuntimeError, match='igmc_rank_segments'):
            lib.call('igmc_rank_segments', *args)
    ks, cnt, dcg = np.array([5], np.int32), np.zeros(3, np.int32), np.zeros(2, np.float64)
    good = [P(rank), P(q_off), None, 2, 1, P(ks), 1, P(cnt), P(dcg), P(err), 0, None]
    lib.call('igmc_rank_metrics', *good)
    for i, v in ((0, None), (1, None), (5, None), (7, None), (8, None), (9, None), (3, -1), (4, 0), (6, 0), (6, 9), (10, -1)):
        args = list(good)
        args[i] = v
        with pytest.raises(RuntimeError, match='igmc_rank_metrics'):
            lib.call('igmc_rank_metrics', *args)
