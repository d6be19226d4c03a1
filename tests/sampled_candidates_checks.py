"""Cases, numpy references and checks of ``igmc_candidates_sample_count`` / ``igmc_candidates_sample_fill``
(``igmc_amd/csrc/candidates.hip``): every user's candidate segment cut down to k sampled negatives, the must items of
the request always kept.  Shared by the emulator test (tests/test_emu_sampled_candidates.py) and the GPU test
(tests/test_gpu_sampled_candidates.py), as ``selection_checks.py`` is; every function takes a backend ``be`` of parity_checks
and calls the C entry points directly, every buffer a call can write -- and every input an offset could lead past -- sits
between the guards of ``selection_checks.Guarded``.

THE DEFINITION, restated here in numpy from the text of ``include/igmc_rng.h`` (uint64 / uint32 arithmetic on Python ints and
numpy arrays, so the emulator tests hold the restatement to the header's own code): for request q of user u, with C(u) the
candidates of ``igmc_candidates_fill``, M(q) the must items and N = C(u) \\ M(q), the segment is (M(q) n C(u)) u S, item
ascending, S = the min(k, |N|) items of N with the smallest ``igmc_sample_key(igmc_negative_salt(seed, draw, u), item)``."""
import numpy as np
import scipy.sparse as ssp

import sampler_stats as S
from igmc_amd import engine
from selection_checks import BAD_OFFSETS, GUARD, MANY, Guarded, P, enumerate_dev, filled, graph_with_corner_rows, offsets

M64 = (1 << 64) - 1
K_MAX = 2 ** 31 - 1
N_ITEMS = [63, 64, 65, 16383, 16384, 16385, 40000]          # around a 64-item word, around the tile, three tiles
K_KINDS = ['0', '1', '99', 'pool-1', 'pool', 'pool+1', 'max']
MUST_KINDS = ['empty', 'one', 'seventy_with_duplicates', 'all_of_the_row', 'unsorted']


# ------------------------------------------------------------------ the hash, from the header's text
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def negative_salt(seed, draw, user):
    s = splitmix64((seed ^ 0x4E454753) & M64)
    s = splitmix64(s ^ draw)
    return splitmix64(s ^ user)


def fmix32(h):
    """``igmc_fmix32`` of a uint64 array holding 32-bit values (products of 32-bit values fit 64 bits)."""
    m = np.uint64(0xFFFFFFFF)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & m
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & m
    return h ^ (h >> np.uint64(16))


def sample_key(salt, ids):
    m = np.uint64(0xFFFFFFFF)
    ids = np.asarray(ids).astype(np.uint64)
    return fmix32(fmix32((ids + np.uint64(salt & 0xFFFFFFFF)) & m) ^ np.uint64(salt >> 32))


# ------------------------------------------------------------------ the definition
def candidates_ref(A, u, item_ok=None, exclude_seen=1):
    """bool[n_items]: C(u)."""
    keep = np.ones(A.shape[1], bool) if item_ok is None else np.asarray(item_ok) != 0
    if exclude_seen:
        row = A.indices[A.indptr[u]:A.indptr[u + 1]]
        keep[row[A.data[A.indptr[u]:A.indptr[u + 1]] != 0]] = False
    return keep


def segment_ref(A, u, k, must=(), item_ok=None, exclude_seen=1, seed=1, draw=0):
    """(items int32 ascending, forced uint8) of one request."""
    n_items = A.shape[1]
    cand = candidates_ref(A, u, item_ok, exclude_seen)
    must = np.asarray(must, np.int64)
    is_must = np.zeros(n_items, bool)
    is_must[must[(must >= 0) & (must < n_items)]] = True
    pool = np.nonzero(cand & ~is_must)[0]
    keys = sample_key(negative_salt(seed, draw, int(u)), pool)
    assert len(np.unique(keys)) == len(keys)          # a bijection of the id: no ties
    chosen = pool[np.argsort(keys, kind='stable')[:min(k, len(pool))]]
    take = cand & is_must
    take[chosen] = True
    items = np.nonzero(take)[0].astype(np.int32)
    return items, is_must[items].astype(np.uint8)


def segments_ref(A, users, k, musts=None, item_ok=None, exclude_seen=1, seed=1, draw=0):
    """link_u, link_v, forced, counts of a request list; ``musts``: one id list per request (None: no must items)."""
    A = A.tocsr()
    us, vs, fs, seen = [], [], [], {}
    for q, u in enumerate(users):
        must = () if musts is None else musts[q]
        key = (int(u), tuple(np.asarray(must).tolist()))
        if key not in seen:
            seen[key] = segment_ref(A, int(u), k, must, item_ok, exclude_seen, seed, draw)
        v, f = seen[key]
        us.append(np.full(len(v), u, np.int32))
        vs.append(v)
        fs.append(f)
    return np.concatenate(us), np.concatenate(vs), np.concatenate(fs), np.array([len(v) for v in vs], np.int64)


# ------------------------------------------------------------------ the device
def must_arrays(musts, nq):
    if musts is None:
        return None, None
    assert len(musts) == nq
    return offsets([len(m) for m in musts]), np.concatenate([np.asarray(m, np.int32) for m in musts] + [np.zeros(0, np.int32)])


def sample_dev(be, g, users, k, musts=None, item_ok=None, exclude_seen=1, seed=1, draw=0, capacity=None, must_off=None,
               n_must=None, bad_off=None, with_forced=True):
    """counts, offsets, link_u, link_v, forced (``max(capacity, 1)`` entries each, guards checked), error word of either call.
    ``must_off`` / ``n_must``: what the library is told in place of the lists' own offsets; ``bad_off``: the segment offsets
    the fill is given in place of the counts' prefix sums."""
    users = np.ascontiguousarray(users, np.int32)
    nq = len(users)
    U = Guarded(be, users, -3)
    ok = None if item_ok is None else Guarded(be, np.ascontiguousarray(item_ok, np.uint8), 1)
    okp = None if ok is None else ok.ptr
    m_off, m_item = must_arrays(musts, nq)
    if must_off is not None:
        m_off = np.ascontiguousarray(must_off, np.int64)
    MO = None if m_off is None else Guarded(be, m_off, -1)
    MI = None if m_off is None else Guarded(be, m_item, -2 ** 31)          # (a must item read outside the list: bit 3)
    mop, mip = (None, None) if MO is None else (MO.ptr, MI.ptr)
    nm = (0 if m_item is None else len(m_item)) if n_must is None else n_must
    counts, err = filled(be, nq, np.int64, -7), Guarded(be, np.zeros(1, np.int32), -9)
    be.lib.call('igmc_candidates_sample_count', g.handle, U.ptr, nq, okp, exclude_seen, mop, mip, nm, k, counts.ptr, err.ptr, None)
    be.sync()
    counts = counts.host()
    off = offsets(counts)
    total = int(off[-1])
    cap = max(total if capacity is None else capacity, 1)
    O = Guarded(be, off if bad_off is None else np.ascontiguousarray(bad_off, np.int64), -1)
    lu, lv, fo = filled(be, cap, np.int32, -5), filled(be, cap, np.int32, -6), filled(be, cap, np.uint8, 9)
    err2 = Guarded(be, np.zeros(1, np.int32), -9)
    be.lib.call('igmc_candidates_sample_fill', g.handle, U.ptr, nq, okp, exclude_seen, mop, mip, nm, k, seed, draw, O.ptr, lu.ptr,
                lv.ptr, fo.ptr if with_forced else None, cap, err2.ptr, None)
    be.sync()
    for b in (U, O) + (() if ok is None else (ok,)) + (() if MO is None else (MO, MI)):
        b.check()
    return counts, off, lu.host(), lv.host(), fo.host(), int(err.host()[0]), int(err2.host()[0])


def compare(got, want, tag):
    """Counts, offsets and the three arrays element for element; the sentinels behind the last segment."""
    counts, off, lu, lv, fo, e1, e2 = got
    ru, rv, rf, rc = want
    assert e1 == 0 and e2 == 0, (tag, e1, e2)
    assert np.array_equal(counts, rc), (tag, counts, rc)
    n = int(off[-1])
    assert n == len(ru) and len(lu) == max(n, 1), tag
    assert np.array_equal(lu[:n], ru) and np.array_equal(lv[:n], rv) and np.array_equal(fo[:n], rf), tag
    assert (lu[n:] == -5).all() and (lv[n:] == -6).all() and (fo[n:] == 9).all(), tag


# ------------------------------------------------------------------ 1. the segments are the definition
N_USERS = 6
REQUESTS = [(2, 'empty'), (3, 'one'), (4, 'seventy_with_duplicates'), (5, 'all_of_the_row'), (2, 'unsorted'),
            (0, 'seventy_with_duplicates'), (1, 'one'), (3, 'one'), (0, 'all_of_the_row')]          # user 3 twice, the same request


assert {kind for _, kind in REQUESTS} == set(MUST_KINDS)


def case_graph(n_items):
    return graph_with_corner_rows(N_USERS, n_items, 10 + n_items).tocsr()


def must_list(A, u, kind, rng):
    """A must list of one kind for user ``u``: items of the complement of the row (candidates unless the mask drops them)
    and, for the longer kinds, of the row itself."""
    n_items = A.shape[1]
    row = A.indices[A.indptr[u]:A.indptr[u + 1]]
    free = np.setdiff1d(np.arange(n_items), row)
    anyof = free if len(free) else np.arange(n_items)
    if kind == 'empty':
        return np.zeros(0, np.int32)
    if kind == 'one':
        return anyof[[len(anyof) // 2]].astype(np.int32)
    if kind == 'seventy_with_duplicates':          # 50 drawn with replacement + 20 of them again, some from the row
        a = anyof[rng.integers(0, len(anyof), 45)]
        b = row[rng.integers(0, len(row), 5)] if len(row) else a[:5]
        m = np.concatenate([a, b])
        return rng.permutation(np.concatenate([m, m[:20]])).astype(np.int32)
    if kind == 'all_of_the_row':                   # no candidates where the row is excluded
        return row.astype(np.int32)
    assert kind == 'unsorted'
    return np.sort(anyof[rng.choice(len(anyof), min(11, len(anyof)), replace=False)])[::-1].astype(np.int32)


def requests(A, seed):
    rng = np.random.default_rng(seed)
    users = np.array([u for u, _ in REQUESTS], np.int32)
    musts, made = [], {}
    for u, kind in REQUESTS:
        if (u, kind) not in made:
            made[(u, kind)] = must_list(A, u, kind, rng)
        musts.append(made[(u, kind)])
    assert [len(m) for m in musts][2] == 70 and not (np.diff(musts[4]) > 0).any()
    return users, musts


def k_of(kind, n_pool):
    return {'0': 0, '1': 1, '99': 99, 'pool-1': max(n_pool - 1, 0), 'pool': n_pool, 'pool+1': n_pool + 1, 'max': K_MAX}[kind]


def check_segments(be, n_items, k_kinds=K_KINDS, masks=(False, True), excludes=(1, 0)):
    """Every k x mask x exclude_seen: one count and one fill launch over ``REQUESTS`` (every must kind, the corner rows, a
    request given twice), equal to the definition element for element; 'pool' is |N| of request 2 (70 must items)."""
    A = case_graph(n_items)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users, musts = requests(A, n_items)
    mask = (np.random.default_rng(n_items).random(n_items) < 0.6).astype(np.uint8)
    for masked in masks:
        item_ok = mask if masked else None
        for excl in excludes:
            cand = candidates_ref(A, int(users[2]), item_ok, excl)
            n_pool = int(cand.sum()) - len(np.intersect1d(np.nonzero(cand)[0], musts[2]))
            for kind in k_kinds:
                k = k_of(kind, n_pool)
                tag = (n_items, kind, k, masked, excl)
                got = sample_dev(be, g, users, k, musts, item_ok, excl)
                want = segments_ref(A, users, k, musts, item_ok, excl)
                compare(got, want, tag)
                counts, off, lu, lv, fo = got[:5]
                for q in range(len(users)):
                    seg = lv[off[q]:off[q + 1]]
                    assert (np.diff(seg) > 0).all(), tag                         # item ascending: igmc_rank_segments bisects
                    assert int((fo[off[q]:off[q + 1]] == 0).sum()) <= k, tag
                assert np.array_equal(lv[off[1]:off[2]], lv[off[7]:off[8]]) and np.array_equal(fo[off[1]:off[2]], fo[off[7]:off[8]])
                if excl:
                    assert counts[6] == 0          # the full row: nothing is a candidate, the must item included
                if kind == '0':
                    assert (fo[:int(off[-1])] == 1).all()          # the must items only
                if kind == 'max':                                  # all of C(u), whatever the user
                    full = enumerate_dev(be, g, users, item_ok, excl)
                    assert np.array_equal(full[0], counts) and np.array_equal(full[2], lu) and np.array_equal(full[3], lv)
    g.close()


def check_all_negatives_is_the_enumeration(be, n_items):
    """2. ``k = 2^31 - 1`` and no must items (``must_off`` NULL): the bytes of ``igmc_candidates_fill`` on the same inputs."""
    A = case_graph(n_items)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users = np.array([1, 0, 3, 3, N_USERS - 1, 0, 2, 1], np.int32)
    mask = (np.random.default_rng(n_items).random(n_items) < 0.6).astype(np.uint8)
    for item_ok, excl in ((None, 1), (mask, 1), (None, 0), (mask, 0)):
        counts, off, lu, lv, fo, e1, e2 = sample_dev(be, g, users, K_MAX, None, item_ok, excl)
        c2, off2, lu2, lv2, f1, f2 = enumerate_dev(be, g, users, item_ok, excl)
        assert (e1, e2, f1, f2) == (0, 0, 0, 0)
        assert counts.tobytes() == c2.tobytes() and lu.tobytes() == lu2.tobytes() and lv.tobytes() == lv2.tobytes()
        assert (fo[:int(off[-1])] == 0).all()
        lu3, lv3 = sample_dev(be, g, users, K_MAX, None, item_ok, excl, with_forced=False)[2:4]          # forced: optional
        assert lu3.tobytes() == lu2.tobytes() and lv3.tobytes() == lv2.tobytes()
    g.close()


def deciding_byte_count(A, u, k, seed=1, draw=0):
    """How many pool keys share the top byte of the k-th smallest (no must items, no mask)."""
    pool = np.nonzero(candidates_ref(A.tocsr(), u))[0]
    keys = np.sort(sample_key(negative_salt(seed, draw, u), pool))
    return int((keys >> np.uint64(24) == keys[k - 1] >> np.uint64(24)).sum())


def check_fallback_selection(be, n_items, more_than):
    """3. More than ``more_than`` pool keys share the deciding top byte (the parked list's bound: 256, or what the emulator
    was told through IGMC_SAMPLE_PARK): the radix passes return the same set."""
    A = graph_with_corner_rows(3, n_items, 77).tocsr()
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users = np.array([0, 2], np.int32)
    musts = [np.array([5, 3], np.int32), np.zeros(0, np.int32)]
    k = n_items // 3
    assert deciding_byte_count(A, 0, k) > more_than and deciding_byte_count(A, 2, k) > more_than
    compare(sample_dev(be, g, users, k, musts), segments_ref(A, users, k, musts), (n_items, k))
    g.close()


def check_park_bound(be):
    """3b. The edge of "park or radix" (``kth_key.h``: ``kth_parks``, the one comparison with the list's 256 entries): a deciding
    byte of exactly 256 pool keys is parked, one of exactly 257 goes through the radix passes, and either way the k-th key may be
    the first or the last of its byte.  User 0 of the graph has an empty row: the pool is all 66 000 items, five tiles."""
    n_items = 66000
    A = graph_with_corner_rows(3, n_items, 77).tocsr()
    assert A.indptr[1] == A.indptr[0]
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users = np.array([0], np.int32)
    top = (sample_key(negative_salt(1, 0, 0), np.arange(n_items)) >> np.uint64(24)).astype(np.int64)
    hist = np.bincount(top, minlength=256)
    before = np.cumsum(hist) - hist
    for count in (256, 257):
        bins = np.nonzero(hist == count)[0]
        assert len(bins), 'no top byte holds exactly %d keys' % count
        b = int(bins[0])
        for k in (int(before[b]) + 1, int(before[b]) + count):          # the first and the last key of the byte
            assert deciding_byte_count(A, 0, k) == count
            compare(sample_dev(be, g, users, k, seed=1, draw=0), segments_ref(A, users, k, seed=1, draw=0), (count, b, k))
    g.close()


def check_many_users(be, n_requests=MANY, permuted=True):
    """4. ``MANY`` requests over a 12 x 20 graph (the launch is capped at 65 536 workgroups: some take a second request),
    and (``permuted``) the same requests in another order: every segment unchanged, so the draw is keyed by the user id."""
    A = graph_with_corner_rows(12, 20, 8).tocsr()
    g = engine.Graph(A, device=be.device, lib=be.lib)
    rng = np.random.default_rng(9)
    users = rng.integers(0, 12, n_requests).astype(np.int32)
    musts = [np.array([q % 20], np.int32) for q in range(n_requests)]
    k = 4
    got = sample_dev(be, g, users, k, musts)
    compare(got, segments_ref(A, users, k, musts), 'many')
    if not permuted:
        g.close()
        return
    perm = rng.permutation(n_requests)
    counts, off, lu, lv, fo = got[:5]
    counts2, off2, lu2, lv2, fo2, e1, e2 = sample_dev(be, g, users[perm], k, [musts[i] for i in perm])
    assert (e1, e2) == (0, 0) and np.array_equal(counts2, counts[perm])
    src = np.repeat(off[:-1][perm] - off2[:-1], counts2) + np.arange(int(off2[-1]))          # where each entry came from
    assert np.array_equal(lu2, lu[src]) and np.array_equal(lv2, lv[src]) and np.array_equal(fo2, fo[src])
    g.close()


# ------------------------------------------------------------------ 5. errors
def _error_case(be):
    A = graph_with_corner_rows(10, 200, 3).tocsr()
    g = engine.Graph(A, device=be.device, lib=be.lib)
    users = np.array([4, 0, 7], np.int32)
    row4 = A.indices[A.indptr[4]:A.indptr[4 + 1]]
    free4 = np.setdiff1d(np.arange(200), row4)
    musts = [free4[[3, 9, 1]].astype(np.int32), np.array([7], np.int32), np.zeros(0, np.int32)]
    return A, g, users, musts


def check_no_place(be):
    """A capacity one short (bit 0, nothing written past it) and offsets that are not the counts' (bit 2)."""
    A, g, users, musts = _error_case(be)
    k = 20
    ru, rv, rf, rc = segments_ref(A, users, k, musts)
    total = len(ru)
    counts, off, lu, lv, fo, e1, e2 = sample_dev(be, g, users, k, musts, capacity=total - 1)
    assert e1 == 0 and e2 == 1 and np.array_equal(counts, rc)
    assert len(lu) == total - 1 and np.array_equal(lu, ru[:-1]) and np.array_equal(lv, rv[:-1]) and np.array_equal(fo, rf[:-1])
    bad = off.copy()
    bad[1] -= 3
    counts, _, lu, lv, fo, e1, e2 = sample_dev(be, g, users, k, musts, bad_off=bad)
    assert e1 == 0 and e2 == 4
    assert (lu[:bad[1]] == 4).all() and (lu[bad[1]:bad[2] - 3] == 0).all() and (lu[bad[2] - 3:bad[2]] == -5).all()
    assert (fo[bad[2] - 3:bad[2]] == 9).all() and np.array_equal(lv[bad[2]:], rv[bad[2]:])
    g.close()


def check_bad_user(be, bad_ids):
    A, g, users, musts = _error_case(be)
    for bad in bad_ids:
        us = np.array([4, bad, 7], np.int32)
        counts, off, lu, lv, fo, e1, e2 = sample_dev(be, g, us, 20, musts)
        ru, rv, rf, rc = segments_ref(A, [4, 7], 20, [musts[0], musts[2]])
        assert e1 == 2 and e2 == 2
        assert counts.tolist() == [rc[0], 0, rc[1]]
        n = int(off[-1])
        assert np.array_equal(lu[:n], ru) and np.array_equal(lv[:n], rv) and np.array_equal(fo[:n], rf)
    g.close()


def check_bad_must_item(be):
    """A must item of -1 and one of ``n_items``: bit 3 from either launch, the rest of the segments as without them."""
    A, g, users, musts = _error_case(be)
    for bad in (-1, 200):
        with_bad = [np.concatenate([musts[0][:1], [bad], musts[0][1:]]).astype(np.int32), musts[1], np.array([bad], np.int32)]
        counts, off, lu, lv, fo, e1, e2 = sample_dev(be, g, users, 20, with_bad)
        assert e1 == 8 and e2 == 8
        ru, rv, rf, rc = segments_ref(A, users, 20, musts)
        n = int(off[-1])
        assert np.array_equal(counts, rc) and np.array_equal(lu[:n], ru) and np.array_equal(lv[:n], rv) and np.array_equal(fo[:n], rf)
    g.close()


def check_bad_must_offsets(be, bad, wild=False):
    """``selection_checks.BAD_OFFSETS`` applied to ``must_off``: a request whose range is decreasing or leaves [0, n_must]
    raises bit 4 and has NO must items, every other request follows its range as given -- 'short_end' and 'first_not_zero'
    are ranges inside the list, so nothing is reported and the lists are the shorter ones.  The bad values stay within
    ``GUARD`` elements of the list (``wild``: far outside it)."""
    assert bad in BAD_OFFSETS
    A, g, users, _ = _error_case(be)
    items = np.setdiff1d(np.arange(200), A.indices[A.indptr[4]:A.indptr[7 + 1]])[:12].astype(np.int32)
    m_off = np.array([0, 5, 8, 12], np.int64)
    if bad == 'decreasing':
        m_off[1] = 9                      # request 1: [9, 8)
    elif bad == 'short_end':
        m_off[3] = 11
    elif bad == 'long_end':
        m_off[3] = 12 + (1000000 if wild else GUARD // 2)
    elif bad == 'negative':
        m_off[1] = -5                     # request 0: [0, -5), request 1: [-5, 8)
    else:
        m_off[0] = 1
    ranges = [(int(m_off[q]), int(m_off[q + 1])) for q in range(3)]
    valid = [0 <= a <= b <= 12 for a, b in ranges]
    musts = [items[a:b] if ok else items[:0] for (a, b), ok in zip(ranges, valid)]
    want_err = 0 if all(valid) else 16
    assert (want_err == 0) == (bad in ('short_end', 'first_not_zero'))
    listed = [items, items[:0], items[:0]]          # (the list the library is given: all twelve, whatever the offsets say)
    counts, off, lu, lv, fo, e1, e2 = sample_dev(be, g, users, 20, listed, must_off=m_off, n_must=12)
    assert e1 == want_err and e2 == want_err, (bad, e1, e2)
    ru, rv, rf, rc = segments_ref(A, users, 20, musts)
    n = int(off[-1])
    assert np.array_equal(counts, rc) and np.array_equal(lu[:n], ru) and np.array_equal(lv[:n], rv) and np.array_equal(fo[:n], rf)
    g.close()


def check_refusals(lib):
    """Null and range arguments raise ``RuntimeError`` naming the entry point.  Every call here is refused on the host and
    nothing is launched: the buffers are host arrays whatever the backend."""
    import pytest
    g = engine.Graph(graph_with_corner_rows(4, 10, 5), lib=lib)
    users, cnt, err = np.zeros(2, np.int32), np.zeros(2, np.int64), np.zeros(1, np.int32)
    off, l, f = np.zeros(3, np.int64), np.zeros(64, np.int32), np.zeros(64, np.uint8)
    mo, mi = np.zeros(3, np.int64), np.zeros(4, np.int32)
    h, U, C, E, O, L, F, MO, MI = g.handle, P(users.ctypes.data), P(cnt.ctypes.data), P(err.ctypes.data), P(off.ctypes.data), \
        P(l.ctypes.data), P(f.ctypes.data), P(mo.ctypes.data), P(mi.ctypes.data)
    for args in ((None, U, 2, None, 1, MO, MI, 4, 5, C, E, None), (h, None, 2, None, 1, MO, MI, 4, 5, C, E, None),
                 (h, U, 2, None, 1, MO, MI, 4, 5, None, E, None), (h, U, 2, None, 1, MO, MI, 4, 5, C, None, None),
                 (h, U, 0, None, 1, MO, MI, 4, 5, C, E, None), (h, U, 2, None, 1, MO, None, 4, 5, C, E, None),
                 (h, U, 2, None, 1, MO, MI, -1, 5, C, E, None), (h, U, 2, None, 1, MO, MI, 2 ** 31, 5, C, E, None),
                 (h, U, 2, None, 1, MO, MI, 4, -1, C, E, None), (h, U, 2, None, 1, MO, MI, 4, 2 ** 31, C, E, None)):
        with pytest.raises(RuntimeError, match='igmc_candidates_sample_count'):
            lib.call('igmc_candidates_sample_count', *args)
    for args in ((None, U, 2, None, 1, MO, MI, 4, 5, 1, 0, O, L, L, F, 64, E, None),
                 (h, None, 2, None, 1, MO, MI, 4, 5, 1, 0, O, L, L, F, 64, E, None),
                 (h, U, 2, None, 1, MO, MI, 4, 5, 1, 0, None, L, L, F, 64, E, None),
                 (h, U, 2, None, 1, MO, MI, 4, 5, 1, 0, O, None, L, F, 64, E, None),
                 (h, U, 2, None, 1, MO, MI, 4, 5, 1, 0, O, L, None, F, 64, E, None),
                 (h, U, 2, None, 1, MO, MI, 4, 5, 1, 0, O, L, L, F, 64, None, None),
                 (h, U, 0, None, 1, MO, MI, 4, 5, 1, 0, O, L, L, F, 64, E, None),
                 (h, U, 2, None, 1, MO, None, 4, 5, 1, 0, O, L, L, F, 64, E, None),
                 (h, U, 2, None, 1, MO, MI, 4, -1, 1, 0, O, L, L, F, 64, E, None),
                 (h, U, 2, None, 1, MO, MI, 4, 2 ** 31, 1, 0, O, L, L, F, 64, E, None),
                 (h, U, 2, None, 1, MO, MI, 4, 5, 1, 0, O, L, L, F, 0, E, None),
                 (h, U, 2, None, 1, MO, MI, 4, 5, 1, 0, O, L, L, F, 2 ** 31, E, None)):
        with pytest.raises(RuntimeError, match='igmc_candidates_sample_fill'):
            lib.call('igmc_candidates_sample_fill', *args)
    g.close()


# ------------------------------------------------------------------ 6. distribution
N_DRAWS = 4200          # distinct users 0 .. 4199, each one draw of K = 100 from the same pool
SEED = 1


def stats_graph(n):
    """``N_DRAWS`` users who all rated the items n .. n + 2 (so they have rows) and none of 0 .. n - 1: the same pool of n
    items for every user, as the three links of ``sampler_stats.graph()`` have the same fringe at every position."""
    rows = np.repeat(np.arange(N_DRAWS), 3)
    cols = np.tile(n + np.arange(3), N_DRAWS)
    return ssp.csr_matrix((1.0 + (rows + cols) % 5, (rows, cols)), shape=(N_DRAWS, n + 3)).astype(np.float32)


def inclusion_ref(n, draw):
    X = np.zeros((N_DRAWS, n), bool)
    ids = np.arange(n)
    for u in range(N_DRAWS):
        X[u, np.argsort(sample_key(negative_salt(SEED, draw, u), ids), kind='stable')[:S.K]] = True
    return X


def inclusion_dev(be, n, draw):
    """The device's inclusion matrix: ONE count and one fill launch for all ``N_DRAWS`` users."""
    g = engine.Graph(stats_graph(n), device=be.device, lib=be.lib)
    users = np.arange(N_DRAWS, dtype=np.int32)
    counts, off, lu, lv, fo, e1, e2 = sample_dev(be, g, users, S.K, None, seed=SEED, draw=draw)
    g.close()
    assert (e1, e2) == (0, 0) and (counts == S.K).all() and np.array_equal(lu, np.repeat(users, S.K)) and not fo.any()
    X = np.zeros((N_DRAWS, n), bool)
    X[lu, lv] = True
    assert (X.sum(1) == S.K).all()
    return X


def z_scores(X0, X1, n, reps=10):
    """p of the singles' chi-square, z of the mean id-rank, of the calibrated pair statistic and of draw 0 against draw 1
    (the statistics of ``sampler_stats``, null replicates from numpy's uniform k-subsets)."""
    p = S.singles_chi2(X0)[2]
    mr, sd = S.mean_rank(X0)
    rng = np.random.default_rng(1000 + n)
    zp = S.calibrated_z(lambda Z: S.pairs_stat(Z)[0], S.pairs_stat(X0)[0], lambda r: (S.uniform_inclusion(N_DRAWS, n, rng),), reps)[0]
    rng = np.random.default_rng(2000 + n)
    zd = S.calibrated_z(lambda a, b: S.joint_stat(a, b)[0], S.joint_stat(X0, X1)[0],
                        lambda r: (S.uniform_inclusion(N_DRAWS, n, rng), S.uniform_inclusion(N_DRAWS, n, rng)), reps)[0]
    return dict(p=p, z_rank=(mr - 0.5) / sd, z_pairs=zp, z_draws=zd)


def within_bounds(z):
    return z['p'] > 1e-3 and abs(z['z_rank']) < 5 and abs(z['z_pairs']) < 5 and abs(z['z_draws']) < 5


def check_distribution(be, n):
    X0, X1 = inclusion_dev(be, n, 0), inclusion_dev(be, n, 1)
    assert np.array_equal(X0, inclusion_ref(n, 0)) and np.array_equal(X1, inclusion_ref(n, 1))          # bit for bit
    assert not np.array_equal(X0, X1)
    z = z_scores(X0, X1, n)
    print('n = %d: singles p = %.3f, z_rank = %+.2f, z_pairs = %+.2f, z_draws = %+.2f' % (n, z['p'], z['z_rank'], z['z_pairs'],
                                                                                        z['z_draws']))
    assert within_bounds(z), z


def check_lowest_ids_violate_the_bounds(n):
    """The negative control: a sampler that takes the K lowest ids every time."""
    X = np.zeros((N_DRAWS, n), bool)
    X[:, :S.K] = True
    z = z_scores(X, X, n, reps=3)
    assert z['p'] < 1e-12 and min(abs(z['z_rank']), abs(z['z_pairs']), abs(z['z_draws'])) > 100, z
    assert not within_bounds(z)
