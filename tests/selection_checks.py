"""Cases, numpy references and checks of the selection, enumeration and ranking entry points -- ``igmc_select_extremes``
(scores.hip), ``igmc_candidates_count`` / ``_fill`` and ``igmc_select_segments`` (candidates.hip), ``igmc_rank_segments`` /
``igmc_rank_metrics`` (ranking.hip), all resting on the 64-bit selection word of select.h -- shared by the emulator tests
(tests/test_emu_scores.py, test_emu_recommend.py, test_emu_rank_eval.py) and the GPU test (tests/test_gpu_selection.py).
Every function takes a backend ``be`` of parity_checks (``EmuBackend`` / ``GpuBackend``) and calls the C entry points directly.

Guards: every buffer a call can write, and every input an offset could lead past, is a :class:`Guarded` buffer -- ``GUARD``
sentinel elements in front of and behind the interior whose address the library gets -- and the guards are compared after the
call.  The cases that feed inconsistent offsets or capacities keep the bad values within ``GUARD`` elements of the buffers
unless told otherwise (``wild``: the emulator, where a stray address is a failed test and not a faulted card), so that a clamp
the kernel lost fails a guard instead of leaving the allocation."""
import functools

import numpy as np
import scipy.sparse as ssp

from helpers import random_rating_graph
from igmc_amd import engine

P = engine._p
GUARD = 16
TILE = 16384          # items of one LDS bitmap tile of the enumeration (launch.h: IGMC_CAND_TILE_ITEMS)
LENS = [0, 1, 63, 64, 65, 1000, 5000]          # 5000: past the 4096 words candidates.hip stages, and the 2048 ranking.hip does
MANY = 70000          # segments / users of the cases whose launches are capped at 65 536 workgroups: some take a second job
NEG_NAN = np.array([0xFFC00000], np.uint32).view(np.float32)[0]
# -inf, the zeros by index, 1, +inf, the NaNs by index ascending; +inf, 1, the zeros by index, -inf, the NaNs by index descending
KNOWN_KEYS = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, NEG_NAN, 1.0, -0.0], np.float32)
KNOWN_ASCENDING = [4, 1, 2, 7, 6, 3, 0, 5]
KNOWN_DESCENDING = [3, 6, 1, 2, 7, 4, 0, 5]
KNOWN_RANKS = [6, 2, 3, 0, 5, 7, 1, 4]


# ------------------------------------------------------------------ buffers
class Guarded(object):
    """``values`` on the backend between two runs of ``GUARD`` sentinels; ``ptr`` is the interior's address."""

    def __init__(self, be, values, sentinel):
        values = np.ascontiguousarray(values)
        self.be, self.n = be, len(values)
        self.pad = np.full(GUARD, sentinel, values.dtype)
        self.buf = be.dev(np.concatenate([self.pad, values, self.pad]))
        self.inner = self.buf[GUARD:]          # (never empty: the guard behind)

    @property
    def ptr(self):
        return P(self.be.ptr(self.inner))

    def check(self):
        """Both guards hold their sentinels, bit for bit."""
        front, behind = self.be.host(self.buf[:GUARD]), self.be.host(self.buf[GUARD + self.n:])
        assert front.tobytes() == self.pad.tobytes(), 'written in front of the buffer: %s' % front
        assert behind.tobytes() == self.pad.tobytes(), 'written behind the buffer: %s' % behind

    def host(self):
        """The interior, once both guards are checked."""
        h = self.be.host(self.buf)
        assert h[:GUARD].tobytes() == self.pad.tobytes(), 'written in front of the buffer: %s' % h[:GUARD]
        assert h[GUARD + self.n:].tobytes() == self.pad.tobytes(), 'written behind the buffer: %s' % h[GUARD + self.n:]
        return h[GUARD:GUARD + self.n]


def filled(be, n, dtype, value):
    """An output buffer: interior and guards hold ``value``."""
    return Guarded(be, np.full(n, value, dtype), value)


def guarded_keys(be, keys):
    """Keys behind +inf guards: a key read outside the interior would come first in THE ORDER and last in the ascending one."""
    return keys if isinstance(keys, Guarded) else Guarded(be, np.ascontiguousarray(keys, np.float32), np.inf)


def offsets(lens):
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return off


# ------------------------------------------------------------------ keys and THE ORDER
def key_sets(n, seed):
    rng = np.random.default_rng(seed)
    special = rng.normal(0, 1, n).astype(np.float32)
    for j, v in enumerate((np.inf, -np.inf, np.nan, -0.0, 0.0, np.nan, -np.inf, 0.0, -0.0, np.inf)):
        special[(j * 7919) % n] = v
    sets = {
        'random': rng.normal(0, 1, n).astype(np.float32),
        'five_levels': rng.integers(1, 6, n).astype(np.float32),          # heavy ties, as sort_by='true' has
        'all_equal': np.full(n, 2.5, np.float32),
        'special': special,
    }
    # every fourth key a number, the others NaN, -inf, NaN with the sign bit set: from the second key on every segment holds a NaN
    # at a lower index than a -inf, and where it is no longer than `num` (or holds fewer than `num` numbers) both are in its list
    i = np.arange(n)
    behind = rng.normal(0, 1, n).astype(np.float32)
    behind[i % 4 == 0], behind[i % 4 == 1], behind[i % 4 == 2] = np.nan, -np.inf, NEG_NAN
    sets['inf_behind_nan'] = behind
    return sets


def descending_order(k, idx, seg=None):
    """THE ORDER of ``igmc_select_segments`` (igmc_hip.h): key descending, index ascending, EVERY NaN behind EVERY number.
    Its usual restatement ``np.lexsort((idx, np.where(np.isnan(k), np.inf, -k)))`` maps -inf and NaN to the same value and
    then orders the two among themselves by index, so it is that order only for segments without a -inf key; these segments
    hold both, and the NaNs are set behind the numbers by a key of their own.  ``seg``: the segment of every key as the
    slowest key -- all segments in one lexsort."""
    nan = np.isnan(k)
    slowest = () if seg is None else (seg,)
    order = np.lexsort((idx, np.where(nan, 0.0, -k), nan) + slowest)
    if not np.isneginf(k).any():
        assert np.array_equal(order, np.lexsort((idx, np.where(nan, np.inf, -k)) + slowest))
    return order


def segment_places(keys, off):
    """(order, seg, place): all keys in THE ORDER segment after segment, and the segment and 0-based place of order[i]."""
    keys = np.asarray(keys, np.float32)
    seg = np.repeat(np.arange(len(off) - 1), np.diff(off))
    order = descending_order(keys, np.arange(len(keys)), seg)
    return order, seg, np.arange(len(keys)) - off[:-1][seg]          # (seg[order] == seg: the segments are contiguous)


# ------------------------------------------------------------------ extremes of one key vector
def select_extremes(be, keys, num, grid=0):
    K = guarded_keys(be, keys)
    nbytes = be.lib.igmc_select_scratch_bytes(K.n, num, grid)
    assert nbytes > 0
    scratch = Guarded(be, np.zeros(nbytes // 8, np.int64), -3)
    il, ih = filled(be, num, np.int32, -9), filled(be, num, np.int32, -9)
    kl, kh = filled(be, num, np.float32, -9.0), filled(be, num, np.float32, -9.0)
    cnt = Guarded(be, np.zeros(1, np.int32), -9)
    be.lib.call('igmc_select_extremes', K.ptr, K.n, num, il.ptr, ih.ptr, kl.ptr, kh.ptr, cnt.ptr, scratch.ptr, nbytes, grid, None)
    be.sync()
    K.check()
    scratch.host()
    return il.host(), ih.host(), kl.host(), kh.host(), int(cnt.host()[0])


def expect_extremes(keys, num):
    order = np.argsort(np.asarray(keys, np.float32), kind='stable')
    return order[:num], order[-num:][::-1]


def check_extremes(be, keys, num, grids, tag):
    """Indices, the keys' own bits, -1 / 0 behind the count, under every grid."""
    keys = np.ascontiguousarray(keys, np.float32)
    n = len(keys)
    lo, hi = expect_extremes(keys, num)
    K = guarded_keys(be, keys)
    for grid in grids:
        il, ih, kl, kh, cnt = select_extremes(be, K, num, grid)
        c = min(n, num)
        assert cnt == c, (tag, n, grid)
        assert np.array_equal(il[:c], lo) and np.array_equal(ih[:c], hi), (tag, n, grid, il[:c], lo, ih[:c], hi)
        assert kl[:c].tobytes() == keys[lo].tobytes() and kh[:c].tobytes() == keys[hi].tobytes()      # the keys' own bits
        assert (il[c:] == -1).all() and (ih[c:] == -1).all() and (kl[c:] == 0).all() and (kh[c:] == 0).all()


def check_extremes_known_answer(be, grids=(0,)):
    for grid in grids:
        il, ih, _, _, cnt = select_extremes(be, KNOWN_KEYS, 8, grid)
        assert cnt == 8
        assert il.tolist() == KNOWN_ASCENDING          # -inf, the zeros by index, 1, +inf, the NaNs by index
        assert il.tolist() == np.argsort(KNOWN_KEYS, kind='stable').tolist()
        assert ih.tolist() == il.tolist()[::-1]


# ------------------------------------------------------------------ enumeration
def enumerate_dev(be, g, users, item_ok=None, exclude_seen=1, capacity=None):
    """counts, offsets, link_u, link_v (``max(capacity, 1)`` entries each, guards checked), error word of either call."""
    users = np.ascontiguousarray(users, np.int32)
    nq = len(users)
    U = Guarded(be, users, -3)          # (a user read outside the list would raise bit 1)
    ok = None if item_ok is None else Guarded(be, np.ascontiguousarray(item_ok, np.uint8), 1)
    okp = None if ok is None else ok.ptr
    counts, err = filled(be, nq, np.int64, -7), Guarded(be, np.zeros(1, np.int32), -9)
    be.lib.call('igmc_candidates_count', g.handle, U.ptr, nq, okp, exclude_seen, counts.ptr, err.ptr, None)
    be.sync()
    counts = counts.host()
    off = offsets(counts)
    total = int(off[-1])
    cap = max(total if capacity is None else capacity, 1)
    O = Guarded(be, off, -1)
    lu, lv, err2 = filled(be, cap, np.int32, -5), filled(be, cap, np.int32, -6), Guarded(be, np.zeros(1, np.int32), -9)
    be.lib.call('igmc_candidates_fill', g.handle, U.ptr, nq, okp, exclude_seen, O.ptr, lu.ptr, lv.ptr, cap, err2.ptr, None)
    be.sync()
    for b in (U, O) + (() if ok is None else (ok,)):
        b.check()
    return counts, off, lu.host(), lv.host(), int(err.host()[0]), int(err2.host()[0])


def enumerate_ref(A, users, item_ok=None, exclude_seen=1):
    A = A.tocsr()
    n_items = A.shape[1]
    us, vs, counts, seen = [], [], [], {}
    for u in users:
        u = int(u)
        if u not in seen:          # (a user asked for again has the same complement)
            keep = np.ones(n_items, bool) if item_ok is None else np.asarray(item_ok) != 0
            if exclude_seen:
                row = A.indices[A.indptr[u]:A.indptr[u + 1]]
                keep[row[A.data[A.indptr[u]:A.indptr[u + 1]] != 0]] = False
            v = np.nonzero(keep)[0]
            seen[u] = (np.full(len(v), u, np.int32), v.astype(np.int32))
        us.append(seen[u][0])
        vs.append(seen[u][1])
        counts.append(len(seen[u][1]))
    return np.concatenate(us), np.concatenate(vs), np.asarray(counts, np.int64)


def graph_with_corner_rows(n_users, n_items, seed):
    """A random rating graph whose user 0 rated nothing and whose user 1 rated every item."""
    A = random_rating_graph(n_users, n_items, 0.3, 5, seed).toarray()
    A[0] = 0
    A[1] = 1 + (np.arange(n_items) % 5)
    return ssp.csr_matrix(A.astype(np.float32))


def check_enumeration(be, n_items):
    """The numpy complement with the corner rows (user 1's full row: every thread of the workgroup marks the same bitmap
    words), duplicates in the user list, ``item_ok`` x ``exclude_seen``."""
    n_users = 6 if n_items > 1000 else 12
    A = graph_with_corner_rows(n_users, n_items, 10 + n_items)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    rng = np.random.default_rng(n_items)
    users = np.array([1, 0, 3, 3, n_users - 1, 0, 2, 1], np.int32)          # full row, empty row, duplicates
    mask = (rng.random(n_items) < 0.6).astype(np.uint8)
    for item_ok, excl in ((None, 1), (mask, 1), (None, 0), (mask, 0)):
        counts, off, lu, lv, e1, e2 = enumerate_dev(be, g, users, item_ok, excl)
        ru, rv, rc = enumerate_ref(A, users, item_ok, excl)
        assert e1 == 0 and e2 == 0
        assert np.array_equal(counts, rc)
        assert np.array_equal(off[1:], np.cumsum(counts)) and off[0] == 0
        n = int(off[-1])
        assert n == len(ru) and len(lu) == max(n, 1)          # (nothing behind the last segment: the guards)
        assert np.array_equal(lu[:n], ru) and np.array_equal(lv[:n], rv)
        for q in range(len(users)):                                         # item ids ascending within every segment
            seg = lv[off[q]:off[q + 1]]
            assert (np.diff(seg) > 0).all() and (lu[off[q]:off[q + 1]] == users[q]).all()
        if excl:
            assert counts[0] == 0 and counts[1] == (n_items if item_ok is None else int(mask.sum()))
        assert (lu[n:] == -5).all() and (lv[n:] == -6).all()
    g.close()


def check_enumeration_no_place(be, n_items=200):
    """What has no place is reported and not written: a capacity one short, offsets that are not the counts' prefix sums.
    ``n_items`` past a tile: the fill forms both bits from a total it only knows after the last tile."""
    A = graph_with_corner_rows(10, n_items, 3)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users = np.array([4, 0, 7], np.int32)
    ru, rv, rc = enumerate_ref(A, users)
    total = len(ru)
    counts, off, lu, lv, e1, e2 = enumerate_dev(be, g, users, capacity=total - 1)          # (the guards: nothing past capacity)
    assert e1 == 0 and e2 & 1 and not e2 & 6
    assert len(lu) == total - 1 and np.array_equal(lu, ru[:-1]) and np.array_equal(lv, rv[:-1])
    # offsets that are not the counts' prefix sums are reported too, and stay inside their own segment
    bad = off.copy()
    bad[1] -= 3
    U, O = Guarded(be, users, -3), Guarded(be, bad, -1)
    lu2, lv2, err = filled(be, total, np.int32, -5), filled(be, total, np.int32, -6), Guarded(be, np.zeros(1, np.int32), -9)
    be.lib.call('igmc_candidates_fill', g.handle, U.ptr, 3, None, 1, O.ptr, lu2.ptr, lv2.ptr, total, err.ptr, None)
    be.sync()
    lu2, lv2 = lu2.host(), lv2.host()
    assert err.host()[0] & 4
    assert (lu2[:bad[1]] == 4).all() and (lu2[bad[1]:bad[2] - 3] == 0).all() and (lu2[bad[2] - 3:bad[2]] == -5).all()
    g.close()


def check_enumeration_bad_user(be, bad_ids):
    A = graph_with_corner_rows(10, 100, 4)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    for bad in bad_ids:
        users = np.array([2, bad, 5], np.int32)
        counts, off, lu, lv, e1, e2 = enumerate_dev(be, g, users)
        assert e1 == 2 and e2 == 2
        ru, rv, rc = enumerate_ref(A, [2, 5])
        assert counts.tolist() == [rc[0], 0, rc[1]]          # the bad user's segment is empty, its neighbours' are whole
        n = int(off[-1])
        assert np.array_equal(lu[:n], ru) and np.array_equal(lv[:n], rv)
    g.close()


def check_enumeration_many_users(be):
    """``MANY`` requested users drawn from a 12 x 40 graph (about 1.9 M links): more users than the 65 536 workgroups of a
    launch, so workgroups of both kernels take a second user."""
    A = graph_with_corner_rows(12, 40, 8)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users = np.random.default_rng(9).integers(0, 12, MANY).astype(np.int32)
    counts, off, lu, lv, e1, e2 = enumerate_dev(be, g, users)
    ru, rv, rc = enumerate_ref(A, users)
    assert e1 == 0 and e2 == 0
    assert np.array_equal(counts, rc) and int(off[-1]) == len(ru) > 1800000
    assert np.array_equal(lu, ru) and np.array_equal(lv, rv)
    g.close()


# ------------------------------------------------------------------ segmented selection
def select_segments(be, keys, off, num, geometry=0, with_keys=True):
    """idx [ns, num], key [ns, num] (None without ``with_keys``), count [ns]; guards checked."""
    K, ns = guarded_keys(be, keys), len(off) - 1
    assert off[-1] == K.n
    O = Guarded(be, np.ascontiguousarray(off, np.int64), -1)
    nbytes = be.lib.igmc_select_segments_scratch_bytes(ns, num, geometry)
    assert nbytes > 0
    scratch = Guarded(be, np.zeros(nbytes // 8, np.int64), -3)
    idx, cnt = filled(be, ns * num, np.int32, -9), filled(be, ns, np.int32, -9)
    key = filled(be, ns * num, np.float32, -9.0) if with_keys else None
    be.lib.call('igmc_select_segments', K.ptr, O.ptr, ns, num, idx.ptr, key.ptr if with_keys else None, cnt.ptr, scratch.ptr,
                nbytes, geometry, None)
    be.sync()
    K.check()
    O.check()
    scratch.host()
    return idx.host().reshape(ns, num), key.host().reshape(ns, num) if with_keys else None, cnt.host()


def expect_segments(keys, off, num):
    """The first ``num`` of every segment in THE ORDER (``descending_order``), -1 / 0 behind the count: one lexsort."""
    keys = np.asarray(keys, np.float32)
    ns = len(off) - 1
    idx, key = np.full((ns, num), -1, np.int32), np.zeros((ns, num), np.float32)
    order, seg, place = segment_places(keys, off)
    keep = place < num
    idx[seg[keep], place[keep]] = order[keep]
    key[seg[keep], place[keep]] = keys[order[keep]]
    return idx, key, np.minimum(np.diff(off), num).astype(np.int32)


def check_segments(be, keys, lens, num, tag, geometries=(0, 1, 3, 8, 64)):
    off = offsets(lens)
    want = expect_segments(keys, off, num)
    K = guarded_keys(be, keys)
    for geometry in geometries:
        idx, key, cnt = select_segments(be, K, off, num, geometry)
        assert np.array_equal(cnt, want[2]), (tag, geometry)
        assert np.array_equal(idx, want[0]), (tag, geometry)
        assert key.tobytes() == want[1].tobytes(), (tag, geometry)          # the keys' own bits; 0 behind the count


def segment_layouts(num):
    rng = np.random.default_rng(num)
    layouts = {
        'mixed': [0, 3, num - 1, num, num + 1, 0, 64, 65, 1000, 1, 0],           # empty segments, shorter than num
        'many_short': rng.integers(0, 12, 300).tolist(),
        'one': [777],
    }
    return {name: [max(0, int(x)) for x in lens] for name, lens in layouts.items()}


def check_segments_layouts(be, num, geometries=(0, 1, 3, 8, 64), many_short=None):
    """Every layout x every key set under every geometry (``many_short``: the geometries of that layout where they differ --
    its 300 segments cut into 64 slices are 19 200 workgroups per key set, half a minute per ``num`` on the emulator, which
    takes segments shorter than their number of slices from ``mixed``)."""
    for lname, lens in segment_layouts(num).items():
        n = sum(lens)
        for kname, keys in key_sets(n, 100 * num + n).items():
            check_segments(be, keys, lens, num, (lname, kname), many_short if many_short and lname == 'many_short' else geometries)


def check_segments_long(be):
    n = 20500          # past what a workgroup stages in LDS: one workgroup reads the keys every round, eight stage a slice each
    for kname, keys in key_sets(n, 5).items():
        check_segments(be, keys, [3, n - 10, 7], 5, ('long', kname))


def check_segments_known_answer(be, geometries=(0,)):
    for geometry in geometries:
        idx, key, cnt = select_segments(be, KNOWN_KEYS, offsets([8]), 8, geometry)
        assert cnt[0] == 8
        assert idx[0].tolist() == KNOWN_DESCENDING          # +inf, 1, the zeros by index, -inf, the NaNs by index
        # ... which is NOT the reverse of the stable ascending order: equal keys keep the lower index first
        assert idx[0].tolist() != np.argsort(KNOWN_KEYS, kind='stable')[::-1].tolist()
        assert key[0].tobytes() == KNOWN_KEYS[KNOWN_DESCENDING].tobytes()
        # -0.0 == 0.0 with the -0.0 at the lower index (above, a +0.0 comes first whether or not the two are told apart)
        zeros = np.array([-0.0, 0.0, -0.0, 1.0, 0.0, -1.0], np.float32)
        idx, key, cnt = select_segments(be, zeros, offsets([6]), 5, geometry)
        assert cnt[0] == 5 and idx[0].tolist() == [3, 0, 1, 2, 4] and key[0].tobytes() == zeros[[3, 0, 1, 2, 4]].tobytes()


@functools.lru_cache(maxsize=None)
def many_segments_case(min_len=0, ns=MANY, seed=21):
    """``ns`` segments of ``min_len`` to 11 keys -- five levels with NaN, +-0.0 and +-inf sprinkled in, as ``make_segments``
    has them --, ids strictly ascending with gaps inside every segment, and one query, of a present id, for every segment that
    holds a key: (keys, ids, off, q_off, q_id), built without a loop over the segments and shared, so never written."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(min_len, 12, ns)
    off = offsets(lens)
    n = int(off[-1])
    keys = rng.integers(1, 6, n).astype(np.float32)
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf], np.float32)
    where = rng.random(n) < 0.15
    keys[where] = special[rng.integers(0, 5, int(where.sum()))]
    seg = np.repeat(np.arange(ns), lens)
    steps = np.cumsum(rng.integers(1, 4, n))
    ids = (steps - np.concatenate([[0], steps])[off[:-1]][seg]).astype(np.int32)
    has = lens > 0
    pick = off[:-1][has] + (rng.random(int(has.sum())) * lens[has]).astype(np.int64)
    case = (keys, ids, off, offsets(has.astype(np.int64)), ids[pick].astype(np.int32))
    for a in case:
        a.setflags(write=False)
    return case


def check_segments_many(be, geometries=(0, 1, 2)):
    """``MANY`` segments of 0 to 11 keys, num 5.  Geometry 0 and 1: one launch, more jobs than its 65 536 workgroups;
    geometry 2: twice as many part jobs, and the merge's own stride."""
    keys, _, off, _, _ = many_segments_case()
    assert len(off) - 1 > 65536
    check_segments(be, keys, np.diff(off), 5, 'many', geometries)


# ------------------------------------------------------------------ ranks
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


def rank_ref_flat(keys, ids, off, q_off, q_id):
    """``rank_ref`` without a loop over the segments: one lexsort with the segment as the slowest key gives every position's
    place, and one ``searchsorted`` over (segment, id) -- ascending, as the ids are inside every segment -- finds the queries."""
    order, seg, place = segment_places(keys, off)
    place_of = np.empty(len(keys), np.int64)
    place_of[order] = place
    both = (seg.astype(np.int64) << 32) + (ids.astype(np.int64) + 2 ** 31)
    assert (np.diff(both) > 0).all()
    q_seg = np.repeat(np.arange(len(q_off) - 1), np.diff(q_off))
    want = (q_seg.astype(np.int64) << 32) + (q_id.astype(np.int64) + 2 ** 31)
    p = np.searchsorted(both, want)
    found = both[np.minimum(p, len(both) - 1)] == want
    pos, rank = np.full(len(q_id), -1, np.int32), np.full(len(q_id), -1, np.int32)
    pos[found], rank[found] = p[found], place_of[p[found]]
    return pos, rank


def rank_dev(be, keys, ids, off, q_off, q_id, geometry=0, nq=None):
    """pos, rank (one entry per element of ``q_id``), error word; the guards of every buffer checked."""
    nq = len(q_id) if nq is None else nq
    K, I = guarded_keys(be, keys), Guarded(be, np.ascontiguousarray(ids, np.int32), -2 ** 31)
    O, QO = Guarded(be, np.ascontiguousarray(off, np.int64), -1), Guarded(be, np.ascontiguousarray(q_off, np.int64), -1)
    Q = Guarded(be, np.ascontiguousarray(q_id, np.int32), -2 ** 31)
    pos, rank = filled(be, len(q_id), np.int32, -7), filled(be, len(q_id), np.int32, -8)
    err = Guarded(be, np.zeros(1, np.int32), -9)
    be.lib.call('igmc_rank_segments', K.ptr, I.ptr, K.n, O.ptr, len(off) - 1, QO.ptr, Q.ptr, nq, pos.ptr, rank.ptr, err.ptr,
                geometry, None)
    be.sync()
    for b in (K, I, O, QO, Q):
        b.check()
    return pos.host(), rank.host(), int(err.host()[0])


def check_rank_geometries(be, keys, ids, off, q_off, q_id, tag, geometries=(0, 1, 3, 64), ref=rank_ref):
    """Positions and ranks are the numpy ones under every geometry, and the same bytes (the guards: inside ``rank_dev``)."""
    want_pos, want_rank = ref(keys, ids, off, q_off, q_id)
    first = None
    for geometry in geometries:
        pos, rank, err = rank_dev(be, keys, ids, off, q_off, q_id, geometry)
        assert err == 0, (tag, geometry)
        assert np.array_equal(pos, want_pos), (tag, geometry)
        assert np.array_equal(rank, want_rank), (tag, geometry)
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


QUERY_KINDS = ['none', 'one', 'every', 'three_hundred', 'absent', 'duplicates', 'mixed']


def check_ranks_of_kind(be, kind, geometries=(0, 1, 3, 64)):
    keys, ids, off = make_segments(LENS, 11)
    q_off, q_id = queries(kind, keys, ids, off, 5)
    if len(q_id) == 0:          # the buffers still exist
        q_id = np.zeros(1, np.int32)
        for geometry in geometries:
            pos, rank, err = rank_dev(be, keys, ids, off, q_off, q_id, geometry, nq=0)
            assert err == 0 and (pos == -7).all() and (rank == -8).all()
        return
    want_pos, want_rank = check_rank_geometries(be, keys, ids, off, q_off, q_id, kind, geometries)
    if kind == 'absent':
        assert (want_pos == -1).all() and (want_rank == -1).all()
    if kind == 'every':           # every place of every segment exactly once
        for s in range(len(off) - 1):
            assert sorted(want_rank[q_off[s]:q_off[s + 1]].tolist()) == list(range(off[s + 1] - off[s]))
    if kind == 'duplicates':
        assert (want_rank.reshape(-1, 4) == want_rank.reshape(-1, 4)[:, :1]).all() and (want_rank >= 0).all()


def check_ranks_long_segment(be, geometries=(1, 64)):
    """One segment of 300 000 keys and 300 queries -- two tiles -- by one workgroup, and by 64 that add their slices' counts
    into the same ``q_rank`` words at once."""
    keys, ids, off = make_segments([300000], 14)
    q_off, q_id = queries('three_hundred', keys, ids, off, 6)
    assert len(q_id) == 300
    check_rank_geometries(be, keys, ids, off, q_off, q_id, 'long', geometries, ref=rank_ref_flat)


def check_ranks_many(be, geometries=(0, 2)):
    """``MANY`` segments of 1 to 11 keys with one query each: more segments than the 65 536 workgroups of a launch."""
    keys, ids, off, q_off, q_id = many_segments_case(min_len=1)
    assert len(q_id) == len(off) - 1 > 65536
    want_pos, want_rank = check_rank_geometries(be, keys, ids, off, q_off, q_id, 'many', geometries, ref=rank_ref_flat)
    assert (want_pos >= 0).all() and (want_rank >= 0).all()


def check_ranks_known_answer(be, geometries=(0,)):
    ids = np.arange(10, 18, dtype=np.int32)
    off, q_off = np.array([0, 8], np.int64), np.array([0, 8], np.int64)
    for geometry in geometries:
        pos, rank, err = rank_dev(be, KNOWN_KEYS, ids, off, q_off, ids.copy(), geometry)
        # the order of the segment: +inf, 1, the zeros by position, -inf, the NaNs by position = positions 3, 6, 1, 2, 7, 4, 0, 5
        assert err == 0 and pos.tolist() == list(range(8))
        assert rank.tolist() == KNOWN_RANKS


def check_ranks_agree_with_the_selection(be):
    """Querying the ids at ``idx_out[s, r]`` of ``igmc_select_segments(num=64)`` returns rank r for every r < count."""
    keys, ids, off = make_segments(LENS, 12)
    ns, num = len(off) - 1, 64
    idx, _, cnt = select_segments(be, keys, off, num, 0, with_keys=False)
    assert np.array_equal(cnt, np.minimum(np.diff(off), num))
    q_off = np.zeros(ns + 1, np.int64)
    q_off[1:] = np.cumsum(cnt)
    q_id = np.concatenate([ids[idx[s, :cnt[s]]] for s in range(ns)]).astype(np.int32)
    for geometry in (0, 2):
        pos, rank, err = rank_dev(be, keys, ids, off, q_off, q_id, geometry)
        assert err == 0
        for s in range(ns):
            assert rank[q_off[s]:q_off[s + 1]].tolist() == list(range(cnt[s]))
            assert np.array_equal(pos[q_off[s]:q_off[s + 1]], idx[s, :cnt[s]])


# ------------------------------------------------------------------ metric sums
def metrics_dev(be, rank, q_off, ks, rel=None, grid=0, nq=None):
    ns, nk = len(q_off) - 1, len(ks)
    nq = len(rank) if nq is None else nq
    R, QO = Guarded(be, np.ascontiguousarray(rank, np.int32), -1), Guarded(be, np.ascontiguousarray(q_off, np.int64), -1)
    rl = None if rel is None else Guarded(be, np.ascontiguousarray(rel, np.uint8), 0)
    K = Guarded(be, np.asarray(ks, np.int32), 0)
    cnt, dcg = filled(be, ns * (2 + nk), np.int32, -7), filled(be, ns * 2 * nk, np.float64, -7.0)
    err = Guarded(be, np.zeros(1, np.int32), -9)
    be.lib.call('igmc_rank_metrics', R.ptr, QO.ptr, None if rl is None else rl.ptr, nq, ns, K.ptr, nk, cnt.ptr, dcg.ptr, err.ptr,
                grid, None)
    be.sync()
    for b in (R, QO, K) + (() if rl is None else (rl,)):
        b.check()
    return cnt.host().reshape(ns, 2 + nk), dcg.host().reshape(ns, 2 * nk), int(err.host()[0])


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


KS_TUPLES = [(1, 5, 10, 1000), (10,), (1, 2, 3, 4, 5, 6, 7, 2 ** 31 - 1)]


def check_metric_sums(be, ks, grids=(1, 3, 1000)):
    """Integer outputs equal, float64 sums within rtol 1e-12 of numpy's, the same bytes for every grid."""
    rank, q_off, rel = metric_case(3)
    for r in (rel, None):
        want_cnt, want_dcg = metrics_ref(rank, q_off, ks, r)
        cnt, dcg, err = metrics_dev(be, rank, q_off, ks, r)
        assert err == 0
        assert np.array_equal(cnt, want_cnt)
        np.testing.assert_allclose(dcg, want_dcg, rtol=1e-12, atol=0)
        for grid in grids:          # fewer workgroups than users, and more: the same bits
            cnt2, dcg2, err = metrics_dev(be, rank, q_off, ks, r, grid)
            assert err == 0 and cnt2.tobytes() == cnt.tobytes() and dcg2.tobytes() == dcg.tobytes()
    cnt, dcg, _ = metrics_dev(be, rank, q_off, ks, rel)
    assert cnt[0].tolist() == [0, -1] + [0] * len(ks) and cnt[1].tolist() == cnt[0].tolist() == cnt[2].tolist()
    assert not dcg[:3].any()
    assert (dcg[:, :len(ks)] <= dcg[:, len(ks):] * (1 + 1e-12)).all()          # no list beats the ideal one


# ------------------------------------------------------------------ inconsistent offsets
BAD_OFFSETS = ['decreasing', 'short_end', 'long_end', 'negative', 'first_not_zero']


def check_bad_offsets(be, bad, wild=False):
    """Inconsistent query offsets are reported and not followed; a segment outside the keys is empty and reported.  The bad
    values stay within ``GUARD`` elements of the buffers (``wild``: far outside them)."""
    keys, ids, off = make_segments([40, 50, 60, 70], 13)
    q_off, q_id = np.array([0, 3, 5, 9, 12], np.int64), np.concatenate([ids[0:3], ids[40:42], ids[90:94], ids[150:153]])
    pos, rank, err = rank_dev(be, keys, ids, off, q_off, q_id)
    assert err == 0 and (rank >= 0).all()
    q_bad = q_off.copy()
    if bad == 'decreasing':
        q_bad[2] = 2
    elif bad == 'short_end':
        q_bad[4] = 11
    elif bad == 'long_end':
        q_bad[4] = 12 + (1000000 if wild else GUARD // 2)
    elif bad == 'negative':
        q_bad[1] = -5
    else:
        assert bad == 'first_not_zero'
        q_bad[0] = 1
    for geometry in (0, 1, 64):
        pos, rank, err = rank_dev(be, keys, ids, off, q_bad, q_id, geometry)
        assert err & 1
        assert (pos == -1).all() and (rank == -1).all()          # the queries cannot be told apart: -1 / -1
    cnt, dcg, err = metrics_dev(be, np.arange(12, dtype=np.int32), q_bad, (5,))
    if bad not in ('short_end', 'first_not_zero'):          # (what one user's range shows: a range outside the queries)
        assert err & 1
    # a segment outside the keys is empty and reported; the other segments are answered
    s_bad = off.copy()
    s_bad[4] = len(keys) + (1000 if wild else GUARD // 2)
    pos, rank, err = rank_dev(be, keys, ids, s_bad, q_off, q_id)
    want_pos, want_rank = rank_ref(keys, ids, off, q_off, q_id)
    assert err == 2 and np.array_equal(pos[:9], want_pos[:9]) and np.array_equal(rank[:9], want_rank[:9])
    assert (pos[9:12] == -1).all() and (rank[9:12] == -1).all()
