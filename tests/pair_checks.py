"""Cases, numpy / float64 references and checks of pair training -- ``igmc_pair_negatives``, ``igmc_pair_loss``,
``igmc_pair_loss_grad`` (``igmc_amd/csrc/pairs.hip``) and ``igmc_amd/pair_train.py`` --, shared by the emulator test
(tests/test_emu_pairs.py) and the GPU test (tests/test_gpu_pairs.py) as ``sampled_candidates_checks.py`` is: every function
takes a backend ``be`` of parity_checks and calls the C entry points directly, every buffer a call can write sits between
the guards of ``selection_checks.Guarded``.

THE NEGATIVE, restated here in numpy / Python integers from the text of ``include/igmc_rng.h`` and ``include/igmc_hip.h``
(so the emulator tests hold the restatement to the header's own code): for positive k = (u, i), with
c_t = pair_candidate(pair_salt(seed, epoch, k), t, n_items), the c_t of the smallest t < T = 256 that is not in the user's row
and passes the item mask; else the first such item of c_0, c_0 + 1, .., n_items - 1, 0, .., c_0 - 1; else the pair is void."""
import math

import numpy as np
import scipy.sparse as ssp

import parity_checks as PC
from helpers import batch_to_pyg
from igmc_amd import engine
from selection_checks import Guarded, P, filled

M64 = (1 << 64) - 1
TRIES = 256
NAN32 = np.float32(np.nan)


# ------------------------------------------------------------------ the hash, from the header's text
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def pair_salt(seed, epoch, pos):
    s = splitmix64((seed ^ 0x50414952) & M64)
    s = splitmix64(s ^ epoch)
    return splitmix64(s ^ pos)


def pair_candidate(salt, t, n_items):
    return (((splitmix64(salt ^ t) >> 32) * n_items) >> 32) & 0xFFFFFFFF


# ------------------------------------------------------------------ the definition
def qualifying(A, u, item_ok=None):
    """bool[n_items]: the items a negative of user ``u`` may be."""
    q = np.ones(A.shape[1], bool) if item_ok is None else np.asarray(item_ok) != 0
    q = q.copy()
    q[A.indices[A.indptr[u]:A.indptr[u + 1]]] = False
    return q


def negative_ref(q, k, seed, epoch, tries=TRIES):
    """(j or -1, the try that decided or None, True where the cyclic scan wrapped past n_items - 1)."""
    n_items = len(q)
    salt = pair_salt(seed, epoch, k)
    for t in range(tries):
        c = pair_candidate(salt, t, n_items)
        if q[c]:
            return c, t, False
    c0 = pair_candidate(salt, 0, n_items)
    hits = np.nonzero(np.roll(q, -c0))[0]
    if not len(hits):
        return -1, None, False
    return int((c0 + hits[0]) % n_items), None, bool(c0 + hits[0] >= n_items)


def negatives_ref(A, pos_u, pos_v, seed, epoch, item_ok=None, tries=TRIES):
    """link_u, link_v, the odd labels, the error word and per-pair (try, wrapped) of a pair list."""
    A = A.tocsr()
    n_users, n_items = A.shape
    lu, lv, ly, err, how, qs = [], [], [], 0, [], {}
    for k, (u, i) in enumerate(zip(pos_u.tolist(), pos_v.tolist())):
        if not (0 <= u < n_users and 0 <= i < n_items):
            j, t, wrapped, err = -1, None, False, err | 1
        else:
            if u not in qs:
                qs[u] = qualifying(A, u, item_ok)
            j, t, wrapped = negative_ref(qs[u], k, seed, epoch, tries)
            if j < 0:
                err |= 2
        lu += [u, u]
        lv += [i, j if j >= 0 else i]
        ly.append(1.0 if j >= 0 else 0.0)
        how.append((t, wrapped))
    return np.array(lu, np.int32), np.array(lv, np.int32), np.array(ly, np.float32), err, how


# ------------------------------------------------------------------ the device
def negatives_dev(be, g, pos_u, pos_v, seed, epoch, item_ok=None):
    """link_u, link_v, link_y (2 n entries each, guards checked; link_y starts as NaN sentinels) and the error word."""
    n = len(pos_u)
    U, V = Guarded(be, np.ascontiguousarray(pos_u, np.int32), -3), Guarded(be, np.ascontiguousarray(pos_v, np.int32), -3)
    ok = None if item_ok is None else Guarded(be, np.ascontiguousarray(item_ok, np.uint8), 1)
    lu, lv, ly = filled(be, 2 * n, np.int32, -5), filled(be, 2 * n, np.int32, -6), filled(be, 2 * n, np.float32, NAN32)
    err = Guarded(be, np.zeros(1, np.int32), -9)
    be.lib.call('igmc_pair_negatives', g.handle, U.ptr, V.ptr, n, None if ok is None else ok.ptr, seed, epoch, lu.ptr, lv.ptr,
                ly.ptr, err.ptr, None)
    be.sync()
    for b in (U, V) + (() if ok is None else (ok,)):
        b.check()
    return lu.host(), lv.host(), ly.host(), int(err.host()[0])


def compare(got, want, tag):
    lu, lv, ly, err = got
    ru, rv, ry, rerr = want[:4]
    assert err == rerr, (tag, err, rerr)
    assert np.array_equal(lu, ru), tag
    assert np.array_equal(lv, rv), (tag, np.nonzero(lv != rv)[0][:8])
    assert np.array_equal(ly[1::2], ry), tag
    assert np.isnan(ly[0::2]).all() and ly[0::2].tobytes() == np.full(len(ry), NAN32).tobytes(), (tag, 'a positive\'s label was written')


# ------------------------------------------------------------------ 1. the definition, bit for bit
def rows_graph(n_items, degrees, seed, n_rel=5):
    """One user per entry of ``degrees``: that many items drawn uniformly, their ratings 1 .. n_rel spread over the row -- the
    library stores a row by (relation, item), so a long row is nowhere near sorted by item."""
    rng = np.random.default_rng(seed)
    rows, cols, vals = [], [], []
    for u, d in enumerate(degrees):
        rows.append(np.full(d, u))
        cols.append(rng.choice(n_items, d, replace=False))
        vals.append(1 + rng.integers(0, n_rel, d))
    return ssp.csr_matrix((np.concatenate(vals).astype(np.float32), (np.concatenate(rows), np.concatenate(cols))),
                          shape=(len(degrees), n_items))


def case_degrees(n_items):
    if n_items == 300:
        return [150, 0, 40, 299]
    if n_items == 40000:
        return [5000, 0, 130, 64, 1]
    return [n_items // 3, 0, n_items - 5, n_items // 2, 1, 24]          # 63, 64, 65: a chunk of the row walk and its edges


def positives(A, n, seed):
    """``n`` positives in shuffled order: a user at random and an item of its row (any item for an empty row)."""
    rng = np.random.default_rng(seed)
    A = A.tocsr()
    u = rng.integers(0, A.shape[0], n)
    v = np.empty(n, np.int64)
    for k, uu in enumerate(u):
        row = A.indices[A.indptr[uu]:A.indptr[uu + 1]]
        v[k] = row[rng.integers(0, len(row))] if len(row) else rng.integers(0, A.shape[1])
    return u.astype(np.int32), v.astype(np.int32)


def check_definition(be, n_items, n=200, seed=1):
    """With and without an item mask: two epochs differ, the same epoch twice gives the same bytes, everything equals the
    restatement; the positives' labels stay the NaN sentinels."""
    A = rows_graph(n_items, case_degrees(n_items), 10 + n_items)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    pu, pv = positives(A, n, n_items)
    mask = (np.random.default_rng(n_items).random(n_items) < 0.6).astype(np.uint8)
    for item_ok in (None, mask):
        runs = {}
        for epoch in (1, 2, 1):
            got = negatives_dev(be, g, pu, pv, seed, epoch, item_ok)
            compare(got, negatives_ref(A, pu, pv, seed, epoch, item_ok), (n_items, epoch, item_ok is not None))
            if epoch in runs:
                assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[epoch][:3], got[:3]))
            runs[epoch] = got
        assert not np.array_equal(runs[1][1], runs[2][1])
        if item_ok is not None:
            assert (mask[runs[1][1][1::2][runs[1][2][1::2] != 0]] != 0).all()
    g.close()


# ------------------------------------------------------------------ 2. more than one round of 64 tries
def crowded_case(be):
    """65 items, one user who has seen 60 of them."""
    A = rows_graph(65, [60, 3], 7)
    return A, engine.Graph(A, device=be.device, lib=be.lib)


def check_second_round(be, n=2000, seed=1, epoch=3):
    A, g = crowded_case(be)
    pu, pv = np.zeros(n, np.int32), np.full(n, A.indices[0], np.int32)
    want = negatives_ref(A, pu, pv, seed, epoch)
    tries = [t for t, _ in want[4]]
    assert max(tries) >= 64 and min(tries) < 64          # both rounds decide some draws
    compare(negatives_dev(be, g, pu, pv, seed, epoch), want, 'second round')
    g.close()


# ------------------------------------------------------------------ 3. the cyclic scan, void pairs
def check_fallback(be, which, tries, n=300, seed=2, epoch=5):
    """``IGMC_PAIR_TRIES = tries`` (set by the caller): the cyclic scan decides draws, its wrap past n_items - 1 included."""
    if which == 'crowded':
        A, g = crowded_case(be)
    else:          # 300 items, 150 seen: the top hundred and fifty below them, so that a scan from the top third wraps
        seen = np.concatenate([np.arange(200, 300), np.random.default_rng(310).choice(200, 50, replace=False)])
        A = ssp.csr_matrix((1.0 + seen % 5, (np.zeros(150, np.int64), seen)), shape=(2, 300)).astype(np.float32)
        g = engine.Graph(A, device=be.device, lib=be.lib)
    pu, pv = np.zeros(n, np.int32), np.full(n, A.indices[0], np.int32)
    want = negatives_ref(A, pu, pv, seed, epoch, tries=tries)
    scanned = [w for t, w in want[4] if t is None]
    assert len(scanned) >= (n if tries == 0 else 20) and any(scanned) and not all(scanned)
    assert want[3] == 0
    compare(negatives_dev(be, g, pu, pv, seed, epoch), want, ('fallback', which, tries))
    g.close()


def check_void_pairs(be, seed=1, epoch=1):
    """A user who has rated every item (a full row), and one whose unseen items the mask all drops: void pairs -- the slot
    repeats the positive, label 0, bit 1 -- beside ordinary ones."""
    n_items = 130
    A = rows_graph(n_items, [n_items, 100, 20], 5)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    mask = np.zeros(n_items, np.uint8)
    row1 = A.tocsr().indices[A.indptr[1]:A.indptr[2]]
    mask[row1[:50]] = 1          # user 1: every allowed item is seen
    pu = np.array([0, 2, 0, 1, 2], np.int32)
    pv = np.array([3, 5, 129, 7, 9], np.int32)
    got = negatives_dev(be, g, pu, pv, seed, epoch)
    compare(got, negatives_ref(A, pu, pv, seed, epoch), 'full row')
    assert got[3] == 2 and got[2][1::2].tolist() == [0.0, 1.0, 0.0, 1.0, 1.0] and got[1][1] == 3 and got[1][5] == 129
    got = negatives_dev(be, g, pu, pv, seed, epoch, mask)
    want = negatives_ref(A, pu, pv, seed, epoch, mask)
    compare(got, want, 'mask')
    assert mask[qualifying(A.tocsr(), 2)].any()          # (user 2 keeps an allowed unseen item)
    assert got[3] == 2 and got[2][1::2].tolist() == [0.0, 1.0, 0.0, 0.0, 1.0] and got[1][7] == 7
    g.close()


# ------------------------------------------------------------------ 4. bad ids
def check_bad_ids(be, bad_users, seed=1, epoch=1):
    A = rows_graph(200, [30, 50, 0, 10], 3)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    pu, pv = positives(A, 12, 4)
    clean = negatives_ref(A, pu, pv, seed, epoch)
    for where, (u, i) in zip((0, 5, 11, 3, 7), [(b, 1) for b in bad_users] + [(1, -1), (1, 200)]):
        qu, qv = pu.copy(), pv.copy()
        qu[where], qv[where] = u, i
        got = negatives_dev(be, g, qu, qv, seed, epoch)
        want = negatives_ref(A, qu, qv, seed, epoch)
        compare(got, want, ('bad id', u, i))
        assert got[3] == 1 and got[2][2 * where + 1] == 0.0
        assert got[0][2 * where:2 * where + 2].tolist() == [u, u] and got[1][2 * where:2 * where + 2].tolist() == [i, i]
        keep = np.ones(24, bool)
        keep[2 * where:2 * where + 2] = False          # the neighbouring pairs: as without the bad one
        assert np.array_equal(got[1][keep], clean[1][keep]) and np.array_equal(got[0][keep], clean[0][keep])
    g.close()


def check_refusals(lib):
    import pytest
    g = engine.Graph(rows_graph(10, [3, 2], 1), lib=lib)
    a, f, e = np.zeros(4, np.int32), np.zeros(8, np.float32), np.zeros(1, np.int32)
    h, I, F, E = g.handle, P(a.ctypes.data), P(f.ctypes.data), P(e.ctypes.data)
    big = np.zeros(8, np.int32)
    L = P(big.ctypes.data)
    for args in ((None, I, I, 2, None, 1, 1, L, L, F, E, None), (h, None, I, 2, None, 1, 1, L, L, F, E, None),
                 (h, I, None, 2, None, 1, 1, L, L, F, E, None), (h, I, I, 0, None, 1, 1, L, L, F, E, None),
                 (h, I, I, 2 ** 30, None, 1, 1, L, L, F, E, None), (h, I, I, 2, None, 1, 1, None, L, F, E, None),
                 (h, I, I, 2, None, 1, 1, L, None, F, E, None), (h, I, I, 2, None, 1, 1, L, L, None, E, None),
                 (h, I, I, 2, None, 1, 1, L, L, F, None, None)):
        with pytest.raises(RuntimeError, match='igmc_pair_negatives'):
            lib.call('igmc_pair_negatives', *args)
    d = np.zeros(5, np.float64)
    D = P(d.ctypes.data)
    for args in ((None, F, 4, 1.0, F, D, None), (F, None, 4, 1.0, F, D, None), (F, F, 4, 1.0, None, D, None),
                 (F, F, 4, 1.0, F, None, None), (F, F, 3, 1.0, F, D, None), (F, F, 0, 1.0, F, D, None)):
        with pytest.raises(RuntimeError, match='igmc_pair_loss'):
            lib.call('igmc_pair_loss', *args)
    g.close()


# ------------------------------------------------------------------ 5. more positives than waves in the grid
def check_many_positives(be, n=20000, seed=1, epoch=1):
    A = rows_graph(300, [150, 0, 40, 299], 310)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    pu, pv = positives(A, n, 9)
    compare(negatives_dev(be, g, pu, pv, seed, epoch), negatives_ref(A, pu, pv, seed, epoch), 'many')
    g.close()


# ------------------------------------------------------------------ 6. distribution
STAT_USERS = {(64, 24): 0, (65, 60): 1, (300, 150): 2}


def stats_graph(n_items, seen):
    return rows_graph(n_items, [seen, 2], 1000 + n_items)


def chi2_bound(dof):
    return dof + 4.5 * math.sqrt(2.0 * dof)


def chi2_of(draws, q):
    """Chi-square of the unseen items' counts against the uniform expectation; every draw must be an unseen item."""
    unseen = np.nonzero(q)[0]
    counts = np.bincount(draws, minlength=len(q))
    assert counts[~q].sum() == 0
    exp = len(draws) / float(len(unseen))
    return float(((counts[unseen] - exp) ** 2).sum() / exp), len(unseen) - 1


def draws_ref(q, n, seed, over):
    if over == 'epochs':
        return np.array([negative_ref(q, 0, seed, e)[0] for e in range(n)])
    return np.array([negative_ref(q, k, seed, 7)[0] for k in range(n)])


def draws_dev(be, g, item, n, seed, over):
    """``n`` draws of user 0: over positions at epoch 7 in ONE launch, or over epochs at position 0 -- one launch of one
    positive per epoch, each into its own two slots of the same buffers."""
    if over == 'positions':
        got = negatives_dev(be, g, np.zeros(n, np.int32), np.full(n, item, np.int32), seed, 7)
        assert got[3] == 0
        return got[1][1::2]
    U, V = Guarded(be, np.zeros(1, np.int32), -3), Guarded(be, np.full(1, item, np.int32), -3)
    lu, lv, ly = filled(be, 2 * n, np.int32, -5), filled(be, 2 * n, np.int32, -6), filled(be, 2 * n, np.float32, NAN32)
    err = Guarded(be, np.zeros(1, np.int32), -9)
    au, av, ay = be.ptr(lu.inner), be.ptr(lv.inner), be.ptr(ly.inner)
    for e in range(n):
        be.lib.call('igmc_pair_negatives', g.handle, U.ptr, V.ptr, 1, None, seed, e, P(au + 8 * e), P(av + 8 * e), P(ay + 8 * e),
                    err.ptr, None)
    be.sync()
    assert int(err.host()[0]) == 0 and (lu.host() == 0).all() and (ly.host()[1::2] == 1.0).all()
    return lv.host()[1::2]


def check_distribution(be, n_items, seen, seed=1):
    A = stats_graph(n_items, seen)
    g = engine.Graph(A, device=be.device, lib=be.lib)
    q = qualifying(A.tocsr(), 0)
    n = 100 * int(q.sum())
    item = int(A.tocsr().indices[0])
    for over in ('epochs', 'positions'):
        got = draws_dev(be, g, item, n, seed, over)
        assert np.array_equal(got, draws_ref(q, n, seed, over)), over          # bit for bit
        chi2, dof = chi2_of(got, q)
        print('%d items, %d seen, over %s: chi2 = %.1f (dof %d, bound %.1f)' % (n_items, seen, over, chi2, dof, chi2_bound(dof)))
        assert chi2 <= chi2_bound(dof), (over, chi2, dof)
    g.close()


def check_restatement_within_bounds(n_items, seen, seeds=(1, 2, 3)):
    """The restatement alone, more seeds than the device runs."""
    q = qualifying(stats_graph(n_items, seen).tocsr(), 0)
    n = 100 * int(q.sum())
    for seed in seeds:
        for over in ('epochs', 'positions'):
            chi2, dof = chi2_of(draws_ref(q, n, seed, over), q)
            assert chi2 <= chi2_bound(dof), (seed, over, chi2, dof)


def check_lowest_ids_violate_the_bound(n_items, seen):
    """The negative control: a sampler that returns the lowest unseen id every time."""
    q = qualifying(stats_graph(n_items, seen).tocsr(), 0)
    n = 100 * int(q.sum())
    chi2, dof = chi2_of(np.full(n, np.nonzero(q)[0][0]), q)
    assert chi2 > 10 * chi2_bound(dof)


# ------------------------------------------------------------------ 7. the pair loss against float64 numpy
VOIDS = ['none', 'first', 'last', 'interleaved', 'all']


def loss_case(n_pairs, void, seed):
    """Scores with d spanning +-40 (both branches of softplus, the sigmoid at saturation) and exact ties, ratings 1 .. 5, the
    odd labels 1 / 0 by ``void``."""
    rng = np.random.default_rng(seed)
    sp = rng.normal(3.0, 1.0, n_pairs).astype(np.float32)
    d = rng.permutation(np.linspace(-40.0, 40.0, n_pairs)) if n_pairs > 1 else np.array([0.7])
    sn = (sp.astype(np.float64) - d).astype(np.float32)
    ties = np.arange(n_pairs) % 7 == 3
    sn[ties] = sp[ties]
    s = np.empty(2 * n_pairs, np.float32)
    s[0::2], s[1::2] = sp, sn
    y = np.empty(2 * n_pairs, np.float32)
    y[0::2] = rng.integers(1, 6, n_pairs)
    ok = {'none': np.ones(n_pairs, bool), 'first': np.arange(n_pairs) != 0, 'last': np.arange(n_pairs) != n_pairs - 1,
          'interleaved': np.arange(n_pairs) % 2 == 1, 'all': np.zeros(n_pairs, bool)}[void]
    y[1::2] = ok
    return s, y


def pair_loss_ref(s, y, A):
    """gout (float64, before its one rounding) and the four statistics, in float64 / exact sums."""
    s64, y64 = s.astype(np.float64), y.astype(np.float64)
    d, e, ok = s64[0::2] - s64[1::2], s64[0::2] - y64[0::2], y[1::2] != 0
    term = np.maximum(-d, 0.0) + np.log1p(np.exp(-np.abs(d)))
    sg = 1.0 / (1.0 + np.exp(d))
    p_ok = int(ok.sum())
    g = np.zeros(len(s), np.float64)
    if p_ok:
        g[0::2] = np.where(ok, (-sg + 2.0 * A * e) / p_ok, 0.0)
        g[1::2] = np.where(ok, sg / p_ok, 0.0)
    return g, [math.fsum(term[ok]), math.fsum(e[ok] ** 2), float((d[ok] > 0).sum()), float(p_ok)]


def pair_loss_dev(be, s, y, A, pad=8):
    n = len(s)
    S = Guarded(be, np.concatenate([s, np.full(pad, NAN32)]), NAN32)
    Y = Guarded(be, np.concatenate([y, np.full(pad, NAN32)]), NAN32)
    G = filled(be, n + pad, np.float32, NAN32)
    st = Guarded(be, np.full(5, -7.0, np.float64), -7.0)
    be.lib.call('igmc_pair_loss', S.ptr, Y.ptr, n, float(A), G.ptr, st.ptr, None)
    be.sync()
    S.check()
    Y.check()
    g = G.host()
    assert np.isnan(g[n:]).all(), 'a gradient behind the batch was written'
    return g[:n], st.host()


def check_pair_loss(be, n_pairs, void, A):
    s, y = loss_case(n_pairs, void, 100 * n_pairs + VOIDS.index(void))
    got_g, got_st = pair_loss_dev(be, s, y, A)
    ref_g, ref_st = pair_loss_ref(s, y, A)
    tag = (n_pairs, void, A)
    assert np.isfinite(got_g).all(), tag
    # one float32 spacing: the float64 evaluation (error far below half a spacing) plus one rounding
    assert (np.abs(got_g.astype(np.float64) - ref_g) <= np.spacing(np.abs(ref_g).astype(np.float32)).astype(np.float64)).all(), tag
    for q in (0, 1):
        assert abs(got_st[q] - ref_st[q]) <= 1e-12 * abs(ref_st[q]), (tag, q, got_st[q], ref_st[q])
    assert got_st[2] == ref_st[2] and got_st[3] == ref_st[3], tag
    assert got_st[4] == -7.0          # (the ARR term is the step entry's)
    if void == 'all':
        assert not got_g.any() and got_st[3] == 0.0 and got_st[0] == 0.0
    again_g, again_st = pair_loss_dev(be, s, y, A)
    assert again_g.tobytes() == got_g.tobytes() and again_st.tobytes() == got_st.tobytes()


# ------------------------------------------------------------------ 8. the step against the oracle
def extract_pairs(be, case, n):
    """The first ``n`` links of a golden case as a pair batch: odd-indexed links are the negatives, only the label slot
    differs -- 1, and 0 for the last pair where there are three or more."""
    g = engine.Graph(case['A'], device=be.device, lib=be.lib)
    b = engine.Batch(g, max_graphs=n, hop=case['h'], max_nodes_per_hop=case['mnph'])
    ys = case['class_values'][case['link_labels'][:n]].astype(np.float32)
    ys[1::2] = 1.0
    if n >= 6:
        ys[n - 1] = 0.0
    bufs = (be.dev(case['links'][:n, 0].astype(np.int32)), be.dev(case['links'][:n, 1].astype(np.int32)), be.dev(ys))
    b.extract(be.ptr(bufs[0]), be.ptr(bufs[1]), be.ptr(bufs[2]), None, 0, n, sample_ratio=case['sample_ratio'], seed=0, epoch=0)
    be.sync()
    return g, b, b.download(), bufs


def pair_oracle(ref, pyg, A, ARR, edge_mask, lin_mask):
    """``pyg_ref.IGMCRef.forward`` + the pair loss in torch float64 + ``pyg_ref.arr_loss``: loss, outputs, gradients, P_ok."""
    import torch
    from oracle import pyg_ref
    ref.train()
    ref.zero_grad()
    out = ref(pyg, edge_mask=edge_mask, lin_mask=lin_mask)
    s, y = out.double(), pyg.y.double()
    d, ok = s[0::2] - s[1::2], y[1::2] != 0
    p_ok = int(ok.sum())
    loss = (torch.nn.functional.softplus(-d)[ok].sum() + A * ((s[0::2] - y[0::2]) ** 2)[ok].sum()) / max(p_ok, 1)
    if ARR != 0:
        loss = loss + ARR * pyg_ref.arr_loss(ref).double()
    loss.backward()
    return float(loss.detach()), out.detach().numpy(), {k: p.grad.detach().clone().numpy() for k, p in ref.named_parameters()}, p_ok


def stats_loss(st, A):
    return (st[0] + A * st[1]) / max(st[3], 1.0) + st[4]


class PairStep(object):
    """A pair batch of a golden case in an arena, a workspace, the oracle model with the same weights."""

    def __init__(self, be, case, n, R, use_dropout, n_side=0, seed=3):
        import torch
        self.be, self.n, self.use_dropout = be, n, use_dropout
        self.g, self.b, self.d, self.bufs = extract_pairs(be, case, n)
        L = 2 * case['h'] + 2
        self.ws = engine.ModelWorkspace(be.lib, be.device, R, 4, L, n_side, self.b.node_capacity, self.b.edge_capacity,
                                        self.b.max_graphs)
        self.ref = PC.make_ref_model(L, R, n_side=n_side, seed=seed, adj_dropout=0.2 if use_dropout else 0.0)
        self.P = be.dev(PC.flatten_params(self.ws, self.ref))
        self.pyg = batch_to_pyg(self.d, L)
        if n_side:
            side = np.random.default_rng(seed + 1).standard_normal((n, n_side)).astype(np.float32)
            self.side = be.dev(side)
            self.b.set_side_features(be.ptr(self.side), n_side)
            self.pyg.u_feature = torch.from_numpy(side[:, :n_side // 2].copy())
            self.pyg.v_feature = torch.from_numpy(side[:, n_side // 2:].copy())
        self.rng = np.random.default_rng(seed)
        self.out = be.dev(np.concatenate([np.zeros(n, np.float32), np.full(8, NAN32)]))
        self.gout = be.dev(np.concatenate([np.zeros(n, np.float32), np.full(8, NAN32)]))
        self.grad = be.dev(np.zeros(self.ws.n_params, np.float32))
        self.stats = be.dev(np.zeros(5, np.float64))

    def masks(self):
        """Fresh injected masks: (lin mask bool [n, 128], its device copy, the oracle's edge mask or None)."""
        import torch
        lm = self.rng.random((self.n, 128)) < 0.5
        edge_mask = None
        if self.use_dropout:
            keep = self.rng.random(self.d['E']) >= 0.2
            rev = PC.reverse_positions(self.d)
            self.b.set_edge_flags(keep.astype(np.uint8) | (keep[rev].astype(np.uint8) << 1))
            edge_mask = torch.from_numpy(keep)
        return lm, self.be.dev(lm.astype(np.uint8).reshape(-1)), edge_mask

    def step(self, LM, A, ARR):
        be = self.be
        self.ws.pair_loss_grad(be.ptr(self.P), self.b, be.ptr(self.out), be.ptr(self.gout), be.ptr(self.grad),
                               be.ptr(self.stats), use_edge_flags=self.use_dropout, lin_mask=be.ptr(LM), ARR=ARR, mse_weight=A)
        be.sync()
        o, go = be.host(self.out), be.host(self.gout)
        assert np.isnan(o[self.n:]).all() and np.isnan(go[self.n:]).all(), 'written behind the batch'
        assert np.isfinite(o[:self.n]).all() and np.isfinite(go[:self.n]).all()
        return o[:self.n], go[:self.n], be.host(self.stats), be.host(self.grad)


def check_step(be, case, n, R, use_dropout, n_side=0, A=1.0, ARR=0.001):
    """``igmc_pair_loss_grad`` on identical subgraphs, weights and injected masks: outputs, loss and every gradient under the
    tolerances of parity_checks; the gradient w.r.t. the outputs is what ``igmc_pair_loss`` gives on those outputs."""
    import torch
    ps = PairStep(be, case, n, R, use_dropout, n_side)
    lm, LM, edge_mask = ps.masks()
    out, gout, st, flat_grad = ps.step(LM, A, ARR)
    rl, ro, rg, p_ok = pair_oracle(ps.ref, ps.pyg, A, ARR, edge_mask, torch.from_numpy(lm))
    assert st[3] == p_ok and p_ok == (n // 2 - 1 if n >= 6 else n // 2)
    assert PC.rel_err(out, ro) < PC.OUT_TOL, PC.rel_err(out, ro)
    assert stats_loss(st, A) == PC.pytest_approx(rl, PC.LOSS_RTOL), (stats_loss(st, A), rl)
    assert np.isfinite(flat_grad).all()
    gg = PC.unflatten_grads(ps.ws, flat_grad)
    worst, worst_key = 0.0, ''
    for key, rgn in rg.items():
        err = np.abs(gg[key] - rgn).max() / max(np.abs(rgn).max(), 1e-6)
        if err > worst:
            worst, worst_key = err, key
    print('pair step R = %d, B = %d: outputs %.2e, loss %.2e, worst gradient %.2e (%s)' % (
        R, n, PC.rel_err(out, ro), abs(stats_loss(st, A) - rl) / abs(rl), worst, worst_key))
    assert worst < PC.GRAD_TOL, '%s: max rel-to-peak grad error %.3e' % (worst_key, worst)
    alone_g, alone_st = pair_loss_dev(be, out, ps.d['y'][:n].astype(np.float32), A)
    assert alone_g.tobytes() == gout.tobytes() and alone_st[:4].tobytes() == st[:4].tobytes()
    if n >= 6:
        assert gout[n - 2] == 0.0 and gout[n - 1] == 0.0          # the void pair
    return ps


def check_odd_batch_is_refused(be, case):
    import pytest
    ps = PairStep(be, case, 3, 5, False)
    _, LM, _ = ps.masks()
    with pytest.raises(RuntimeError, match='igmc_pair_loss_grad.*even number'):
        ps.step(LM, 1.0, 0.001)
    assert not be.host(ps.grad).any() and not be.host(ps.out)[:3].any()          # (an error string, not a launch)


# ------------------------------------------------------------------ 9. trajectory
def check_trajectory(be, case, n, R, steps=3, lr=1e-3, A=1.0, ARR=0.001):
    """``steps`` pair steps (``igmc_pair_loss_grad`` + ``igmc_adam_step``) with fresh injected masks against the oracle +
    ``torch.optim.Adam``, under the trajectory tolerances of parity_checks; the oracle on one torch thread as there."""
    import torch
    nt = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        ps = PairStep(be, case, n, R, True, seed=4)
        ws = ps.ws
        opt = torch.optim.Adam(ps.ref.parameters(), lr=lr)
        M1, M2 = be.dev(np.zeros(ws.n_params, np.float32)), be.dev(np.zeros(ws.n_params, np.float32))
        losses = []
        for step in range(1, steps + 1):
            lm, LM, edge_mask = ps.masks()
            _, _, st, _ = ps.step(LM, A, ARR)
            ws.adam_step(be.ptr(ps.P), be.ptr(ps.grad), be.ptr(M1), be.ptr(M2), step, lr)
            rl = pair_oracle(ps.ref, ps.pyg, A, ARR, edge_mask, torch.from_numpy(lm))[0]
            opt.step()
            losses.append((stats_loss(st, A), rl))
        be.sync()
        m1, m2 = PC.unflatten_grads(ws, be.host(M1)), PC.unflatten_grads(ws, be.host(M2))
        worst_m1 = worst_m2 = 0.0
        for k, prm in ps.ref.named_parameters():
            ea, es = opt.state[prm]['exp_avg'].numpy(), opt.state[prm]['exp_avg_sq'].numpy()
            worst_m1 = max(worst_m1, float(np.abs(m1[k] - ea).max() / max(np.abs(ea).max(), 1e-9)))
            worst_m2 = max(worst_m2, float(np.abs(m2[k] - es).max() / max(np.abs(es).max(), 1e-12)))
        got_p, want_p = be.host(ps.P), PC.flatten_params(ws, ps.ref)
        diff = np.abs(got_p - want_p)
        bad = diff > PC.TRAJ_P_ATOL + PC.TRAJ_P_RTOL * np.abs(want_p)
        loss_rel = max(abs(a - b) / max(abs(b), 1e-12) for a, b in losses)
        print('pair trajectory: loss %.2e, exp_avg %.2e, exp_avg_sq %.2e, off %.2e, max diff %.2e' % (
            loss_rel, worst_m1, worst_m2, bad.mean(), diff.max()))
        assert np.isfinite(got_p).all()
        assert loss_rel < PC.TRAJ_LOSS_RTOL, losses
        assert worst_m1 <= PC.TRAJ_M1_TOL and worst_m2 <= PC.TRAJ_M2_TOL, (worst_m1, worst_m2)
        assert bad.mean() < PC.TRAJ_FRAC_OFF and diff.max() <= PC.TRAJ_P_MAX, (bad.mean(), diff.max())
    finally:
        torch.set_num_threads(nt)
