"""Cases, the numpy restatement and checks of ``igmc_pair_negatives_shortlist`` and ``igmc_pair_kind_stats``
(``igmc_amd/csrc/pairs.hip``): pair negatives of which a share comes from a per-user shortlist table.  Shared by the emulator
test (tests/test_emu_pair_hard.py) and the GPU test (tests/test_gpu_pair_hard.py) as ``pair_checks.py`` is: every function
takes a backend ``be`` of parity_checks and calls the C entry points directly, and every buffer of a call -- the table's
offsets and items included -- sits between the guards of ``selection_checks.Guarded``.  Every sampler comparison is exact.

THE DEFINITION, restated here in Python integers from the text of ``include/igmc_hip.h`` and ``include/igmc_rng.h``: with
thr = floor(share * 2^32) and salt = pair_salt(seed, epoch, k), positive k = (u, i) is HARD-DECIDED iff
(splitmix64(salt ^ KEY_HARD) >> 32) < thr; its segment [a, b) = [off[u], off[u + 1]) is usable iff 0 <= a <= b <= sl_total
(else bit 3 and length 0); of a non-empty segment it picks j = item[a + (((splitmix64(salt ^ KEY_PICK) >> 32) * (b - a)) >>
32)]; j is the negative, label 2, iff 0 <= j < n_items, the mask passes it and the user has not rated it; else bit 2.  Every
other pair carries the negative of ``pair_checks.negatives_ref``: label 1, or void."""
import math

import numpy as np
import scipy.sparse as ssp

import pair_checks as PK
from igmc_amd import engine
from pair_checks import NAN32, TRIES, negatives_ref, pair_salt, splitmix64
from selection_checks import Guarded, P, filled, offsets
from shortlist_checks import segments_ref

KEY_HARD = 0x4841524400000000          # igmc_rng.h: IGMC_PAIR_KEY_HARD / IGMC_PAIR_KEY_PICK
KEY_PICK = 0x5049434B00000000
BIT_ID, BIT_VOID, BIT_STALE, BIT_OFFSETS = 1, 2, 4, 8


# ------------------------------------------------------------------ the definition
def threshold(share):
    return int(math.floor(share * 2.0 ** 32))


def hard_decided(salt, thr):
    return (splitmix64(salt ^ KEY_HARD) >> 32) < thr


def pick(salt, length):
    return ((splitmix64(salt ^ KEY_PICK) >> 32) * length) >> 32


def hard_negatives_ref(A, pos_u, pos_v, seed, epoch, off, item, sl_total, share, item_ok=None, tries=TRIES):
    """link_u, link_v, the odd labels (0 / 1 / 2), the error word, and per pair what decided it: 'bad' (an id out of range),
    'uniform' (not hard-decided), 'hard', 'stale', 'empty' or 'broken' (hard-decided, and why the uniform draw decided)."""
    A = A.tocsr()
    n_users, n_items = A.shape
    lu, lv, ly, err, how = negatives_ref(A, pos_u, pos_v, seed, epoch, item_ok, tries)
    lv, ly = lv.copy(), ly.copy()
    thr = threshold(share)
    kinds, qs = [], {}
    for k, (u, i) in enumerate(zip(pos_u.tolist(), pos_v.tolist())):
        if not (0 <= u < n_users and 0 <= i < n_items):
            kinds.append('bad')
            continue
        salt = pair_salt(seed, epoch, k)
        if not hard_decided(salt, thr):
            kinds.append('uniform')
            continue
        a, b = int(off[u]), int(off[u + 1])
        if not 0 <= a <= b <= sl_total:
            err |= BIT_OFFSETS
            kinds.append('broken')
            continue
        if b == a:
            kinds.append('empty')
            continue
        j = int(item[a + pick(salt, b - a)])
        if u not in qs:
            qs[u] = PK.qualifying(A, u, item_ok)
        if 0 <= j < n_items and qs[u][j]:
            lv[2 * k + 1], ly[k] = j, 2.0
            kinds.append('hard')
        else:
            err |= BIT_STALE
            kinds.append('stale')
    return lu, lv, ly, err, kinds, how


def table_ref(A, m, item_ok=None, s=0, t=0):
    """Offsets (int64 [n_users + 1]) and items (int32) of every user's shortlist: ``segments_ref`` for users 0 .. n_users - 1."""
    _, lv, _, counts = segments_ref(A, np.arange(A.shape[0], dtype=np.int32), m, s, t, item_ok, 1)
    return offsets(counts), lv.astype(np.int32)


# ------------------------------------------------------------------ the device
def hard_dev(be, g, pos_u, pos_v, seed, epoch, off, item, sl_total, share, item_ok=None, null_table=False):
    """link_u, link_v, link_y (2 n entries each; link_y starts as NaN sentinels) and the error word; the guards of every input
    and output are checked, those around the table's items among them."""
    n = len(pos_u)
    U, V = Guarded(be, np.ascontiguousarray(pos_u, np.int32), -3), Guarded(be, np.ascontiguousarray(pos_v, np.int32), -3)
    ok = None if item_ok is None else Guarded(be, np.ascontiguousarray(item_ok, np.uint8), 1)
    O = None if null_table else Guarded(be, np.ascontiguousarray(off, np.int64), -1)
    I = None if null_table else Guarded(be, np.ascontiguousarray(item, np.int32), -2 ** 31)
    lu, lv, ly = filled(be, 2 * n, np.int32, -5), filled(be, 2 * n, np.int32, -6), filled(be, 2 * n, np.float32, NAN32)
    err = Guarded(be, np.zeros(1, np.int32), -9)
    be.lib.call('igmc_pair_negatives_shortlist', g.handle, U.ptr, V.ptr, n, None if ok is None else ok.ptr, seed, epoch,
                None if O is None else O.ptr, None if I is None else I.ptr, sl_total, float(share), lu.ptr, lv.ptr, ly.ptr,
                err.ptr, None)
    be.sync()
    for b in (U, V) + (() if ok is None else (ok,)) + (() if O is None else (O, I)):
        b.check()
    return lu.host(), lv.host(), ly.host(), int(err.host()[0])


def same_bytes(got, want):
    return all(a.tobytes() == b.tobytes() for a, b in zip(got[:3], want[:3])) and got[3] == want[3]


# ------------------------------------------------------------------ 1. the definition, bit for bit
N_ITEMS = [63, 64, 65, 300, 6000]


def case_degrees(n_items):
    """Rows of 0, 1, 63, 64, 65 entries wherever the graph is wide enough for them -- one chunk of the row walk and its edges;
    the full row of the 63-item graph is one of them --, and 5000 in the one graph that can hold such a row."""
    if n_items == 6000:
        return [5000, 0, 1, 63, 64, 65, 700]
    return sorted(set(min(d, n_items) for d in (0, 1, 63, 64, 65)) | {n_items // 3, n_items // 2})


def check_definition(be, n_items, n=200, seed=1):
    """Tables of M = 1, 7 and more than any user's candidates, shares 0 / 0.5 / 1, with and without an item mask, 200
    positives: links, labels and the error word are the restatement's; a clean table raises neither bit 2 nor bit 3; the
    same epoch twice gives the same bytes."""
    A = PK.rows_graph(n_items, case_degrees(n_items), 20 + n_items)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    pu, pv = PK.positives(A, n, n_items)
    mask = (np.random.default_rng(n_items).random(n_items) < 0.6).astype(np.uint8)
    for item_ok in (None, mask):
        for m in (1, 7, n_items + 10):
            off, item = table_ref(A, m, item_ok)
            for share in (0.0, 0.5, 1.0):
                tag = (n_items, item_ok is not None, m, share)
                want = hard_negatives_ref(A, pu, pv, seed, 3, off, item, len(item), share, item_ok)
                got = hard_dev(be, g, pu, pv, seed, 3, off, item, len(item), share, item_ok)
                PK.compare(got, want, tag)
                assert not got[3] & (BIT_STALE | BIT_OFFSETS), tag
                hard = (got[2][1::2] == 2.0).sum()
                assert hard == want[4].count('hard') and (hard > 0) == (share > 0), tag
                if share == 1.0:          # every pair asked its segment: only users without a candidate stay uniform / void
                    assert set(want[4]) <= {'hard', 'empty'}, tag
                if item_ok is not None:
                    assert (mask[got[1][1::2][got[2][1::2] != 0]] != 0).all(), tag
            assert same_bytes(hard_dev(be, g, pu, pv, seed, 3, off, item, len(item), 1.0, item_ok), got), (n_items, m, 'again')
            if m > 1:          # (a segment of one item has one pick)
                assert not np.array_equal(hard_dev(be, g, pu, pv, seed, 4, off, item, len(item), 1.0, item_ok)[1], got[1])
    g.close()


# ------------------------------------------------------------------ 2. share 0 / no table: the bytes of igmc_pair_negatives
def check_share_zero_is_the_old_entry(be, seed=1):
    """Share 0 with a table, share 0 with NULL pointers: every output byte and the error word of ``igmc_pair_negatives`` --
    on a graph with a full row, so that the word is not zero."""
    n_items = 130
    A = PK.rows_graph(n_items, [n_items, 100, 20, 0], 5)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    pu, pv = PK.positives(A, 200, 8)
    mask = (np.random.default_rng(4).random(n_items) < 0.5).astype(np.uint8)
    for item_ok in (None, mask):
        off, item = table_ref(A, 7, item_ok)
        for epoch in (1, 2):
            old = PK.negatives_dev(be, g, pu, pv, seed, epoch, item_ok)
            assert old[3] == BIT_VOID
            assert same_bytes(hard_dev(be, g, pu, pv, seed, epoch, off, item, len(item), 0.0, item_ok), old)
            assert same_bytes(hard_dev(be, g, pu, pv, seed, epoch, None, None, 0, 0.0, item_ok, null_table=True), old)
    g.close()


def check_uniform_positions_keep_their_negative(be, seed=2, epoch=4):
    """Share 0.5: every position the restatement decides uniform carries exactly the item of ``negatives_ref``, label 1; the
    others carry an item of the user's own segment, label 2."""
    A = PK.rows_graph(300, [150, 0, 40, 299, 10], 310)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    pu, pv = PK.positives(A, 200, 9)
    off, item = table_ref(A, 7)
    lu, lv, ly, err = hard_dev(be, g, pu, pv, seed, epoch, off, item, len(item), 0.5)
    want = hard_negatives_ref(A, pu, pv, seed, epoch, off, item, len(item), 0.5)
    uni = negatives_ref(A, pu, pv, seed, epoch)
    kinds = np.array(want[4])
    assert err == 0 and 40 < (kinds == 'uniform').sum() < 160 and (kinds == 'hard').sum() > 40
    for k, kind in enumerate(kinds):
        if kind == 'hard':
            assert ly[2 * k + 1] == 2.0 and lv[2 * k + 1] in item[off[pu[k]]:off[pu[k] + 1]]
        else:
            assert ly[2 * k + 1] == 1.0 and lv[2 * k + 1] == uni[1][2 * k + 1], (k, kind)
    g.close()


def check_a_full_row_gives_void_pairs(be, seed=1, epoch=1):
    """A user whose every item is rated has an empty segment and no uniform negative either: void pairs, bit 1 alone."""
    n_items = 130
    A = PK.rows_graph(n_items, [n_items, 100, 20], 5)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    off, item = table_ref(A, 7)
    assert off[1] == off[0]
    pu, pv = np.array([0, 2, 0, 1, 2], np.int32), np.array([3, 5, 129, 7, 9], np.int32)
    for share in (0.5, 1.0):
        got = hard_dev(be, g, pu, pv, seed, epoch, off, item, len(item), share)
        PK.compare(got, hard_negatives_ref(A, pu, pv, seed, epoch, off, item, len(item), share), ('full row', share))
        assert got[3] == BIT_VOID and got[2][1::2][[0, 2]].tolist() == [0.0, 0.0] and got[1][1] == 3 and got[1][5] == 129
        assert (got[2][1::2][[1, 3, 4]] != 0).all()
    g.close()


# ------------------------------------------------------------------ 3. a stale table, broken offsets
STALE = ['in_row', 'masked', 'minus_one', 'n_items']


def check_stale_pick(be, which, seed=3, epoch=2, n=60):
    """User 0's segment holds ONE item that cannot be its negative, share 1: every pair falls back to the uniform negative,
    label 1, and bit 2 is set; user 1's clean segment beside it still serves."""
    n_items = 100
    A = PK.rows_graph(n_items, [30, 12], 41)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    row0, row1 = (A.indices[A.indptr[u]:A.indptr[u + 1]] for u in (0, 1))
    free = np.setdiff1d(np.arange(n_items), np.concatenate([row0, row1]))
    mask = None
    if which == 'masked':
        mask = np.ones(n_items, np.uint8)
        mask[free[0]] = 0
    bad = {'in_row': int(row0[7]), 'masked': int(free[0]), 'minus_one': -1, 'n_items': n_items}[which]
    off, item = np.array([0, 1, 4], np.int64), np.array([bad, free[1], free[2], free[3]], np.int32)
    pu = (np.arange(n) % 3 == 2).astype(np.int32)          # two of three positives are user 0's
    pv = np.where(pu == 0, row0[0], row1[0]).astype(np.int32)
    got = hard_dev(be, g, pu, pv, seed, epoch, off, item, 4, 1.0, mask)
    want = hard_negatives_ref(A, pu, pv, seed, epoch, off, item, 4, 1.0, mask)
    PK.compare(got, want, ('stale', which))
    uni = negatives_ref(A, pu, pv, seed, epoch, mask)
    assert got[3] == BIT_STALE
    assert np.array_equal(got[1][1::2][pu == 0], uni[1][1::2][pu == 0]) and (got[2][1::2][pu == 0] == 1.0).all()
    assert (got[2][1::2][pu == 1] == 2.0).all() and set(got[1][1::2][pu == 1]) <= set(free[1:4].tolist())
    g.close()


BAD_OFFSETS = ['decreasing', 'negative', 'past_total', 'far_past_total']


def check_broken_offsets(be, which, seed=3, epoch=2, n=90):
    """Offsets that are no segment of the table: bit 3, the pair takes the uniform negative, nothing is read through them --
    the values reach far outside the item buffer -- and the guards around ``d_sl_item`` hold (``hard_dev`` checks them)."""
    n_items = 100
    A = PK.rows_graph(n_items, [30, 12, 20], 43)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    off, item = table_ref(A, 5)
    assert off.tolist() == [0, 5, 10, 15]
    broken = off.copy()
    if which == 'decreasing':
        broken[2] = 3          # user 1: [5, 3); user 2: [3, 15) is a segment of the table, whatever it holds
    elif which == 'negative':
        broken[1] = -2 ** 40          # user 0: [0, -2^40), user 1: [-2^40, 10)
    elif which == 'past_total':
        broken[3] = 16          # user 2: one entry past the table
    else:
        broken[3] = 2 ** 40
    pu = (np.arange(n) % 3).astype(np.int32)
    pv = np.array([A.indices[A.indptr[u]] for u in pu], np.int32)
    got = hard_dev(be, g, pu, pv, seed, epoch, broken, item, len(item), 1.0)
    want = hard_negatives_ref(A, pu, pv, seed, epoch, broken, item, len(item), 1.0)
    PK.compare(got, want, ('offsets', which))
    assert got[3] & BIT_OFFSETS and 'broken' in want[4]
    uni = negatives_ref(A, pu, pv, seed, epoch)
    at = np.array([k == 'broken' for k in want[4]])
    assert np.array_equal(got[1][1::2][at], uni[1][1::2][at]) and (got[2][1::2][at] == 1.0).all()
    g.close()


# ------------------------------------------------------------------ 4. robustness
def check_bad_ids(be, bad_users, seed=1, epoch=1):
    """A positive outside the graph: bit 0, ids written as given, label 0; its neighbours as without it.  The offsets hold
    one entry per user of the graph and nothing else: an id followed into them would land in the guards or far outside."""
    A = PK.rows_graph(200, [30, 50, 0, 10], 3)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    pu, pv = PK.positives(A, 12, 4)
    off, item = table_ref(A, 7)
    clean = hard_negatives_ref(A, pu, pv, seed, epoch, off, item, len(item), 1.0)
    for where, (u, i) in zip((0, 5, 11, 3, 7), [(b, 1) for b in bad_users] + [(1, -1), (1, 200)]):
        qu, qv = pu.copy(), pv.copy()
        qu[where], qv[where] = u, i
        got = hard_dev(be, g, qu, qv, seed, epoch, off, item, len(item), 1.0)
        PK.compare(got, hard_negatives_ref(A, qu, qv, seed, epoch, off, item, len(item), 1.0), ('bad id', u, i))
        assert got[3] == BIT_ID and got[2][2 * where + 1] == 0.0
        assert got[0][2 * where:2 * where + 2].tolist() == [u, u] and got[1][2 * where:2 * where + 2].tolist() == [i, i]
        keep = np.ones(24, bool)
        keep[2 * where:2 * where + 2] = False
        assert np.array_equal(got[1][keep], clean[1][keep]) and np.array_equal(got[0][keep], clean[0][keep])
    g.close()


def check_many_positives(be, n=20000, seed=1, epoch=1):
    """More positives than waves in the grid (2048 workgroups of four)."""
    A = PK.rows_graph(300, [150, 0, 40, 299], 310)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    pu, pv = PK.positives(A, n, 9)
    off, item = table_ref(A, 7)
    got = hard_dev(be, g, pu, pv, seed, epoch, off, item, len(item), 0.5)
    want = hard_negatives_ref(A, pu, pv, seed, epoch, off, item, len(item), 0.5)
    PK.compare(got, want, 'many')
    assert got[3] == 0 and 0.4 * n < want[4].count('uniform') < 0.6 * n
    g.close()


def check_scan_behind_a_fall_through(be, n=300, seed=2, epoch=5):
    """``IGMC_PAIR_TRIES = 0`` (set by the caller), share 0.5, and a segment half of whose entries the user has rated: the
    cyclic scan decides the pairs that were not hard-decided AND those whose pick was stale, its wrap included."""
    seen = np.concatenate([np.arange(200, 300), np.random.default_rng(310).choice(200, 50, replace=False)])
    A = ssp.csr_matrix((1.0 + seen % 5, (np.zeros(150, np.int64), seen)), shape=(2, 300)).astype(np.float32)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    free = np.setdiff1d(np.arange(300), seen)
    item = np.concatenate([free[:4], seen[:4]]).astype(np.int32)
    off = np.array([0, 8, 8], np.int64)
    pu, pv = np.zeros(n, np.int32), np.full(n, A.indices[0], np.int32)
    want = hard_negatives_ref(A, pu, pv, seed, epoch, off, item, 8, 0.5, tries=0)
    kinds = np.array(want[4])
    wrapped = np.array([w for _, w in want[5]])
    for kind in ('uniform', 'stale'):          # both reach the scan, both wrap somewhere
        assert (kinds == kind).sum() >= 30 and wrapped[kinds == kind].any() and not wrapped[kinds == kind].all(), kind
    assert (kinds == 'hard').sum() >= 30 and want[3] == BIT_STALE
    PK.compare(hard_dev(be, g, pu, pv, seed, epoch, off, item, 8, 0.5), want, 'scan behind a fall-through')
    g.close()


def check_refusals(lib):
    """Refused on the host, nothing launched: what ``igmc_pair_negatives`` refuses, a share outside [0, 1] or NaN, a NULL table
    with a share above 0, ``sl_total`` outside [0, 2^31); and the arguments of ``igmc_pair_kind_stats``."""
    import pytest
    g = engine.Graph(PK.rows_graph(10, [3, 2], 1), lib=lib)
    a, f, e, o = np.zeros(8, np.int32), np.zeros(8, np.float32), np.zeros(1, np.int32), np.zeros(3, np.int64)
    h, I, F, E, O = g.handle, P(a.ctypes.data), P(f.ctypes.data), P(e.ctypes.data), P(o.ctypes.data)
    ok = dict(g=h, pu=I, pv=I, n=2, ok=None, seed=1, epoch=1, off=O, item=I, total=4, share=0.5, lu=I, lv=I, ly=F, err=E, st=None)
    for kw in (dict(g=None), dict(pu=None), dict(pv=None), dict(n=0), dict(n=2 ** 30), dict(lu=None), dict(lv=None), dict(ly=None),
               dict(err=None), dict(share=-0.01), dict(share=1.01), dict(share=float('nan')), dict(share=float('inf')),
               dict(off=None), dict(item=None), dict(off=None, item=None, share=1.0), dict(total=-1), dict(total=2 ** 31),
               dict(off=None, item=None, share=0.0, total=-1)):
        with pytest.raises(RuntimeError, match='igmc_pair_negatives_shortlist'):
            lib.call('igmc_pair_negatives_shortlist', *dict(ok, **kw).values())
    assert not a.any() and not f.any() and not e.any()
    d = np.zeros(6, np.float64)
    D = P(d.ctypes.data)
    for args in ((None, F, 4, D, None), (F, None, 4, D, None), (F, F, 4, None, None), (F, F, 3, D, None), (F, F, 0, D, None),
                 (F, F, -2, D, None)):
        with pytest.raises(RuntimeError, match='igmc_pair_kind_stats'):
            lib.call('igmc_pair_kind_stats', *args)
    g.close()


# ------------------------------------------------------------------ 5. distribution
SEGMENT = 24
SHARE = 0.5


def stats_case():
    """One user with 40 of 100 items rated and a shortlist of 24 of the others (a second user keeps the graph a graph)."""
    A = PK.rows_graph(100, [40, 2], 1100)
    free = np.setdiff1d(np.arange(100), A.indices[A.indptr[0]:A.indptr[1]])
    item = np.sort(np.random.default_rng(5).choice(free, SEGMENT, replace=False)).astype(np.int32)
    return A, np.array([0, SEGMENT, SEGMENT], np.int64), item


def draws_ref(A, off, item, n, seed):
    """(items, labels) of position 0 over the epochs 0 .. n - 1."""
    pu, pv = np.zeros(1, np.int32), np.full(1, A.indices[0], np.int32)
    out = [hard_negatives_ref(A, pu, pv, seed, e, off, item, len(item), SHARE) for e in range(n)]
    return np.array([o[1][1] for o in out]), np.array([o[2][0] for o in out])


def draws_dev(be, g, A, off, item, n, seed):
    """The real entry over epochs, as ``pair_checks.draws_dev`` does: one launch of one positive per epoch, each into its
    own two slots of the same buffers."""
    U, V = Guarded(be, np.zeros(1, np.int32), -3), Guarded(be, np.full(1, A.indices[0], np.int32), -3)
    O, I = Guarded(be, off, -1), Guarded(be, item, -2 ** 31)
    lu, lv, ly = filled(be, 2 * n, np.int32, -5), filled(be, 2 * n, np.int32, -6), filled(be, 2 * n, np.float32, NAN32)
    err = Guarded(be, np.zeros(1, np.int32), -9)
    au, av, ay = be.ptr(lu.inner), be.ptr(lv.inner), be.ptr(ly.inner)
    for e in range(n):
        be.lib.call('igmc_pair_negatives_shortlist', g.handle, U.ptr, V.ptr, 1, None, seed, e, O.ptr, I.ptr, len(item), SHARE,
                    P(au + 8 * e), P(av + 8 * e), P(ay + 8 * e), err.ptr, None)
    be.sync()
    for b in (U, V, O, I):
        b.check()
    assert int(err.host()[0]) == 0 and (lu.host() == 0).all()
    return lv.host()[1::2], ly.host()[1::2]


def judge(items, labels, item):
    """(z of the hard count against Binomial(N, thr / 2^32), chi-square of the hard picks over the segment's items, dof)."""
    n, p = len(items), threshold(SHARE) / 2.0 ** 32
    hard = labels == 2.0
    assert np.isin(items[hard], item).all() and set(labels.tolist()) <= {1.0, 2.0}
    z = (hard.sum() - n * p) / math.sqrt(n * p * (1 - p))
    counts = np.array([(items[hard] == j).sum() for j in item])
    exp = hard.sum() / float(len(item))
    return float(z), float(((counts - exp) ** 2).sum() / exp), len(item) - 1


def check_distribution(be, seed=1, n=100 * SEGMENT):
    A, off, item = stats_case()
    g = engine.Graph(A, device=be.device, lib=be.lib)
    got = draws_dev(be, g, A, off, item, n, seed)
    want = draws_ref(A, off, item, n, seed)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])          # bit for bit
    z, chi2, dof = judge(got[0], got[1], item)
    print('%d draws at share %.1f: z = %.2f, chi2 = %.1f (dof %d, bound %.1f)' % (n, SHARE, z, chi2, dof, PK.chi2_bound(dof)))
    assert abs(z) < 5 and chi2 <= PK.chi2_bound(dof), (z, chi2)
    g.close()


def check_restatement_within_bounds(seeds=(1, 2, 3), n=100 * SEGMENT):
    A, off, item = stats_case()
    for seed in seeds:
        z, chi2, dof = judge(*draws_ref(A, off, item, n, seed), item=item)
        assert abs(z) < 5 and chi2 <= PK.chi2_bound(dof), (seed, z, chi2)


def check_first_item_sampler_violates_the_bound(n=100 * SEGMENT):
    """The negative control: a sampler whose hard pairs all take the first item of the segment."""
    A, off, item = stats_case()
    items, labels = draws_ref(A, off, item, n, 1)
    items = np.where(labels == 2.0, item[0], items)
    z, chi2, dof = judge(items, labels, item)
    assert chi2 > 10 * PK.chi2_bound(dof)


# ------------------------------------------------------------------ 6. igmc_pair_kind_stats against float64 numpy
KINDS = ['uniform', 'hard', 'interleaved', 'voids']


def kind_case(n_pairs, kinds, seed):
    """The scores of ``pair_checks.loss_case``; the odd labels all 1, all 2, alternating 1 / 2, or 0 / 1 / 2 in turn."""
    s, y = PK.loss_case(n_pairs, 'none', seed)
    p = np.arange(n_pairs)
    y[1::2] = {'uniform': np.ones(n_pairs), 'hard': np.full(n_pairs, 2.0), 'interleaved': 1.0 + p % 2,
               'voids': (p + 1) % 3}[kinds]
    return s, y


def kind_stats_ref(s, y):
    s64 = s.astype(np.float64)
    d = s64[0::2] - s64[1::2]
    term = np.maximum(-d, 0.0) + np.log1p(np.exp(-np.abs(d)))
    out = []
    for label in (1.0, 2.0):
        at = y[1::2] == label
        out += [float(at.sum()), float((d[at] > 0).sum()), math.fsum(term[at])]
    return out


def kind_stats_dev(be, s, y, pad=8):
    n = len(s)
    S = Guarded(be, np.concatenate([s, np.full(pad, NAN32)]), NAN32)
    Y = Guarded(be, np.concatenate([y, np.full(pad, np.float32(2.0))]), np.float32(2.0))          # (labels behind the batch: 2)
    st = Guarded(be, np.full(6, -7.0, np.float64), -7.0)
    be.lib.call('igmc_pair_kind_stats', S.ptr, Y.ptr, n, st.ptr, None)
    be.sync()
    S.check()
    Y.check()
    return st.host()


def check_kind_stats(be, n_pairs, kinds):
    """Counts exact, sums within 1e-12 relative (the bound of ``pair_checks.check_pair_loss``); a second run, the same bits."""
    s, y = kind_case(n_pairs, kinds, 300 * n_pairs + KINDS.index(kinds))
    got, ref = kind_stats_dev(be, s, y), kind_stats_ref(s, y)
    tag = (n_pairs, kinds)
    for q in (0, 1, 3, 4):
        assert got[q] == ref[q], (tag, q, got[q], ref[q])
    for q in (2, 5):
        assert abs(got[q] - ref[q]) <= 1e-12 * abs(ref[q]), (tag, q, got[q], ref[q])
    assert got[0] + got[3] == n_pairs - (y[1::2] == 0).sum()
    assert kind_stats_dev(be, s, y).tobytes() == got.tobytes()
