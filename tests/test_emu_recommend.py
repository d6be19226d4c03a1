"""``igmc_candidates_count`` / ``igmc_candidates_fill`` and ``igmc_select_segments`` (``igmc_amd/csrc/candidates.hip``) on the CPU
emulation of the HIP sources: the enumeration is the numpy complement of every requested user's row, in (users as given,
item ascending) order, and refuses what it has no place for; the segmented selection is, per segment,
``np.lexsort((idx, np.where(np.isnan(k), np.inf, -k)))`` whatever the geometry."""
import numpy as np
import pytest

from helpers import emu_lib, random_rating_graph
from igmc_amd import engine

P = engine._p
TILE = 16384          # items of one LDS bitmap tile of the enumeration (launch.h: IGMC_CAND_TILE_ITEMS)


# ------------------------------------------------------------------ enumeration
def enumerate_dev(lib, g, users, item_ok=None, exclude_seen=1, capacity=None, guard=0):
    users = np.ascontiguousarray(users, np.int32)
    nq = len(users)
    counts = np.full(nq, -7, np.int64)
    err = np.zeros(1, np.int32)
    ok = None if item_ok is None else np.ascontiguousarray(item_ok, np.uint8)
    lib.call('igmc_candidates_count', g.handle, P(users), nq, P(ok), exclude_seen, P(counts), P(err), None)
    off = np.zeros(nq + 1, np.int64)
    off[1:] = np.cumsum(counts)
    total = int(off[-1])
    cap = total if capacity is None else capacity
    lu = np.full(max(cap, 1) + guard, -5, np.int32)
    lv = np.full(max(cap, 1) + guard, -6, np.int32)
    err2 = np.zeros(1, np.int32)
    lib.call('igmc_candidates_fill', g.handle, P(users), nq, P(ok), exclude_seen, P(off), P(lu), P(lv), max(cap, 1), P(err2),
             None)
    return counts, off, lu, lv, int(err[0]), int(err2[0])


def enumerate_ref(A, users, item_ok=None, exclude_seen=1):
    A = A.tocsr()
    n_items = A.shape[1]
    us, vs, counts = [], [], []
    for u in users:
        keep = np.ones(n_items, bool) if item_ok is None else np.asarray(item_ok) != 0
        if exclude_seen:
            row = A.indices[A.indptr[u]:A.indptr[u + 1]]
            keep[row[A.data[A.indptr[u]:A.indptr[u + 1]] != 0]] = False
        v = np.nonzero(keep)[0]
        us.append(np.full(len(v), u, np.int32))
        vs.append(v.astype(np.int32))
        counts.append(len(v))
    return np.concatenate(us), np.concatenate(vs), np.asarray(counts, np.int64)


def graph_with_corner_rows(n_users, n_items, seed):
    """A random rating graph whose user 0 rated nothing and whose user 1 rated every item."""
    A = random_rating_graph(n_users, n_items, 0.3, 5, seed).toarray()
    A[0] = 0
    A[1] = 1 + (np.arange(n_items) % 5)
    import scipy.sparse as ssp
    return ssp.csr_matrix(A.astype(np.float32))


@pytest.mark.parametrize('n_items', [1, 63, 64, 65, 1000, TILE + 1000])
def test_enumeration_is_the_numpy_complement(n_items):
    lib = emu_lib()
    n_users = 6 if n_items > 1000 else 12
    A = graph_with_corner_rows(n_users, n_items, 10 + n_items)
    g = engine.Graph(A, lib=lib)
    rng = np.random.default_rng(n_items)
    users = np.array([1, 0, 3, 3, n_users - 1, 0, 2, 1], np.int32)          # full row, empty row, duplicates
    mask = (rng.random(n_items) < 0.6).astype(np.uint8)
    for item_ok, excl in ((None, 1), (mask, 1), (None, 0), (mask, 0)):
        counts, off, lu, lv, e1, e2 = enumerate_dev(lib, g, users, item_ok, excl, guard=8)
        ru, rv, rc = enumerate_ref(A, users, item_ok, excl)
        assert e1 == 0 and e2 == 0
        assert np.array_equal(counts, rc)
        assert np.array_equal(off[1:], np.cumsum(counts)) and off[0] == 0
        n = int(off[-1])
        assert n == len(ru)
        assert np.array_equal(lu[:n], ru) and np.array_equal(lv[:n], rv)
        for q in range(len(users)):                                         # item ids ascending within every segment
            seg = lv[off[q]:off[q + 1]]
            assert (np.diff(seg) > 0).all() and (lu[off[q]:off[q + 1]] == users[q]).all()
        if excl:
            assert counts[0] == 0 and counts[1] == (n_items if item_ok is None else int(mask.sum()))
        assert (lu[max(n, 1):] == -5).all() and (lv[max(n, 1):] == -6).all()      # nothing behind the last segment


def test_enumeration_reports_what_has_no_place_and_writes_nothing_there():
    lib = emu_lib()
    A = graph_with_corner_rows(10, 200, 3)
    g = engine.Graph(A, lib=lib)
    users = np.array([4, 0, 7], np.int32)
    ru, rv, rc = enumerate_ref(A, users)
    total = len(ru)
    counts, off, lu, lv, e1, e2 = enumerate_dev(lib, g, users, capacity=total - 1, guard=16)
    assert e1 == 0 and e2 & 1 and not e2 & 6
    assert np.array_equal(lu[:total - 1], ru[:-1]) and np.array_equal(lv[:total - 1], rv[:-1])
    assert (lu[total - 1:] == -5).all() and (lv[total - 1:] == -6).all()          # guard elements past capacity untouched
    # offsets that are not the counts' prefix sums are reported too, and stay inside their own segment
    bad = off.copy()
    bad[1] -= 3
    lu2, lv2, err = np.full(total + 4, -5, np.int32), np.full(total + 4, -6, np.int32), np.zeros(1, np.int32)
    lib.call('igmc_candidates_fill', g.handle, P(users), 3, None, 1, P(bad), P(lu2), P(lv2), total, P(err), None)
    assert err[0] & 4
    assert (lu2[total:] == -5).all()
    assert (lu2[:bad[1]] == 4).all() and (lu2[bad[1]:bad[2] - 3] == 0).all() and (lu2[bad[2] - 3:bad[2]] == -5).all()


def test_enumeration_reports_a_user_id_out_of_range():
    lib = emu_lib()
    A = graph_with_corner_rows(10, 100, 4)
    g = engine.Graph(A, lib=lib)
    for bad in (10, -1, 2 ** 31 - 1):
        users = np.array([2, bad, 5], np.int32)
        counts, off, lu, lv, e1, e2 = enumerate_dev(lib, g, users, guard=4)
        assert e1 == 2 and e2 == 2
        ru, rv, rc = enumerate_ref(A, [2, 5])
        assert counts.tolist() == [rc[0], 0, rc[1]]          # the bad user's segment is empty, its neighbours' are whole
        n = int(off[-1])
        assert np.array_equal(lu[:n], ru) and np.array_equal(lv[:n], rv)


def test_enumeration_refuses_bad_arguments():
    lib = emu_lib()
    g = engine.Graph(graph_with_corner_rows(4, 10, 5), lib=lib)
    users, cnt, err = np.zeros(2, np.int32), np.zeros(2, np.int64), np.zeros(1, np.int32)
    off, l = np.zeros(3, np.int64), np.zeros(64, np.int32)
    for args in ((None, P(users), 2, None, 1, P(cnt), P(err), None), (g.handle, None, 2, None, 1, P(cnt), P(err), None),
                 (g.handle, P(users), 2, None, 1, None, P(err), None), (g.handle, P(users), 2, None, 1, P(cnt), None, None),
                 (g.handle, P(users), 0, None, 1, P(cnt), P(err), None)):
        with pytest.raises(RuntimeError, match='igmc_candidates_count'):
            lib.call('igmc_candidates_count', *args)
    for args in ((g.handle, P(users), 2, None, 1, None, P(l), P(l), 64, P(err), None),
                 (g.handle, P(users), 2, None, 1, P(off), None, P(l), 64, P(err), None),
                 (g.handle, P(users), 2, None, 1, P(off), P(l), P(l), 64, None, None),
                 (g.handle, P(users), 0, None, 1, P(off), P(l), P(l), 64, P(err), None),
                 (g.handle, P(users), 2, None, 1, P(off), P(l), P(l), 0, P(err), None),
                 (g.handle, P(users), 2, None, 1, P(off), P(l), P(l), 2 ** 31, P(err), None)):
        with pytest.raises(RuntimeError, match='igmc_candidates_fill'):
            lib.call('igmc_candidates_fill', *args)


# ------------------------------------------------------------------ segmented selection
def select_segments(lib, keys, lens, num, geometry=0):
    keys = np.ascontiguousarray(keys, np.float32)
    ns = len(lens)
    off = np.zeros(ns + 1, np.int64)
    off[1:] = np.cumsum(lens)
    assert off[-1] == len(keys)
    nbytes = lib.igmc_select_segments_scratch_bytes(ns, num, geometry)
    assert nbytes > 0
    scratch = np.zeros(nbytes // 8, np.uint64)
    idx, key, cnt = np.full(ns * num, -9, np.int32), np.full(ns * num, -9.0, np.float32), np.full(ns, -9, np.int32)
    lib.call('igmc_select_segments', P(keys if len(keys) else np.zeros(1, np.float32)), P(off), ns, num, P(idx), P(key), P(cnt),
             P(scratch), nbytes, geometry, None)
    return idx.reshape(ns, num), key.reshape(ns, num), cnt


def expect_segments(keys, lens, num):
    keys = np.asarray(keys, np.float32)
    ns = len(lens)
    idx, key, cnt = np.full((ns, num), -1, np.int32), np.zeros((ns, num), np.float32), np.zeros(ns, np.int32)
    lo = 0
    for s, n in enumerate(lens):
        k = keys[lo:lo + n]
        i = np.arange(lo, lo + n)
        order = np.lexsort((i, np.where(np.isnan(k), np.inf, -k)))[:num]
        c = len(order)
        idx[s, :c], key[s, :c], cnt[s] = i[order], k[order], c
        lo += n
    return idx, key, cnt


def key_sets(n, seed):
    rng = np.random.default_rng(seed)
    special = rng.normal(0, 1, n).astype(np.float32)
    for j, v in enumerate((np.inf, -np.inf, np.nan, -0.0, 0.0, np.nan, -np.inf, 0.0, -0.0, np.inf)):
        special[(j * 7919) % n] = v
    return {
        'random': rng.normal(0, 1, n).astype(np.float32),
        'five_levels': rng.integers(1, 6, n).astype(np.float32),
        'all_equal': np.full(n, 2.5, np.float32),
        'special': special,
    }


def check_all_geometries(lib, keys, lens, num, tag):
    want = expect_segments(keys, lens, num)
    for geometry in (0, 1, 3, 8):
        idx, key, cnt = select_segments(lib, keys, lens, num, geometry)
        assert np.array_equal(cnt, want[2]), (tag, geometry)
        assert np.array_equal(idx, want[0]), (tag, geometry)
        assert key.tobytes() == want[1].tobytes(), (tag, geometry)          # the keys' own bits; 0 behind the count


@pytest.mark.parametrize('num', [1, 5, 64])
def test_select_segments_is_the_descending_lexsort(num):
    lib = emu_lib()
    rng = np.random.default_rng(num)
    layouts = {
        'mixed': [0, 3, num - 1, num, num + 1, 0, 64, 65, 1000, 1, 0],           # empty segments, shorter than num
        'many_short': rng.integers(0, 12, 300).tolist(),
        'one': [777],
    }
    for lname, lens in layouts.items():
        lens = [max(0, int(x)) for x in lens]
        n = sum(lens)
        for kname, keys in key_sets(n, 100 * num + n).items():
            check_all_geometries(lib, keys, lens, num, (lname, kname))


def test_select_segments_one_long_segment():
    lib = emu_lib()
    n = 20500          # past what a workgroup stages in LDS: one workgroup reads the keys every round, eight stage a slice each
    for kname, keys in key_sets(n, 5).items():
        check_all_geometries(lib, keys, [3, n - 10, 7], 5, ('long', kname))


def test_select_segments_nan_and_signed_zero_order():
    lib = emu_lib()
    keys = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, -np.nan, 1.0, -0.0], np.float32)
    idx, key, cnt = select_segments(lib, keys, [8], 8)
    assert cnt[0] == 8
    assert idx[0].tolist() == [3, 6, 1, 2, 7, 4, 0, 5]          # +inf, 1, the zeros by index, -inf, the NaNs by index
    # ... which is NOT the reverse of the stable ascending order: equal keys keep the lower index first
    assert idx[0].tolist() != np.argsort(keys, kind='stable')[::-1].tolist()


def test_select_segments_refuses_bad_arguments():
    lib = emu_lib()
    keys, off = np.zeros(16, np.float32), np.array([0, 16], np.int64)
    i, k, c, s = np.zeros(64, np.int32), np.zeros(64, np.float32), np.zeros(1, np.int32), np.zeros(4096, np.uint64)
    assert lib.igmc_select_segments_scratch_bytes(0, 5, 0) < 0 and lib.igmc_select_segments_scratch_bytes(1, 65, 0) < 0
    assert lib.igmc_select_segments_scratch_bytes(1, 0, 0) < 0 and lib.igmc_select_segments_scratch_bytes(1, 5, 65) < 0
    assert lib.igmc_select_segments_scratch_bytes(1, 5, -1) < 0
    assert lib.igmc_select_segments_scratch_bytes(7, 5, 3) == 7 * 3 * 5 * 8
    for ns, num, nbytes, geometry in ((0, 5, 32768, 0), (1, 0, 32768, 0), (1, 65, 32768, 0), (1, 5, 8, 3), (1, 5, 32768, -1),
                                      (1, 5, 32768, 65)):
        with pytest.raises(RuntimeError, match='igmc_select_segments'):
            lib.call('igmc_select_segments', P(keys), P(off), ns, num, P(i), P(k), P(c), P(s), nbytes, geometry, None)
    for args in ((None, P(off), 1, 5, P(i), P(k), P(c), P(s), 32768, 0, None),
                 (P(keys), None, 1, 5, P(i), P(k), P(c), P(s), 32768, 0, None),
                 (P(keys), P(off), 1, 5, None, P(k), P(c), P(s), 32768, 0, None),
                 (P(keys), P(off), 1, 5, P(i), P(k), None, P(s), 32768, 0, None),
                 (P(keys), P(off), 1, 5, P(i), P(k), P(c), None, 32768, 0, None)):
        with pytest.raises(RuntimeError, match='igmc_select_segments: null'):
            lib.call('igmc_select_segments', *args)
    lib.call('igmc_select_segments', P(keys), P(off), 1, 5, P(i), None, P(c), P(s), 32768, 0, None)      # keys out: optional
