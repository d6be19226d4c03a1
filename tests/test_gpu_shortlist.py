"""``k_shortlist`` (``igmc_amd/csrc/shortlist.hip``) on a real MI355X through its C entry points, against the scipy definition of
``tests/shortlist_checks.py`` -- the cases, references and checks the emulator test runs (test_emu_shortlist.py) --, and the
Python surface on top of it: ``CandidateLinks.refill(shortlist=M)``, ``recommend``, ``rank_eval``, ``shortlist_recall`` and
``Main.py --shortlist``.  What the single-threaded emulator cannot show is what the kernel-level cases are for here: four waves
adding into the same LDS words of ``w`` and of the vote table, a table left dirty for the next request of the same workgroup,
ballot placement of ties, and the dynamic LDS above 64 KB.

Every buffer sits between guard elements that are checked after every call.  Every kernel-level comparison is exact; the
Python-level ones are exact wherever the device computes the compared value (lists, score bits, integer sums); the float64
MEANS of ``rank_eval`` are recomputed in numpy in another summation order over at most 60 users, so they are held to a
relative 1e-12 (60 terms x 2^-53, with room for a last-bit difference between the two ``log2``)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as ssp

import parity_checks as PC
import shortlist_checks as SL
from helpers import ROOT, random_rating_graph
from selection_checks import BAD_OFFSETS, descending_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    return PC.GpuBackend()


# ------------------------------------------------------------------ the kernels
@pytest.mark.parametrize('n_items', SL.N_ITEMS_SMALL)
@pytest.mark.parametrize('n_users', [40, 300])
def test_segments_and_votes_are_the_definition(be, n_users, n_items):
    SL.check_segments(be, n_users, n_items)


@pytest.mark.parametrize('n_items', SL.N_ITEMS_WIDE)
def test_segments_and_votes_are_the_definition_around_the_vote_table_and_past_it(be, n_items):
    SL.check_segments(be, 8, n_items, thresholds=((0, 0), (3, 1)), ms=(7, 3000))


def test_every_kind_of_m(be):
    SL.check_every_m(be)


def test_ties_at_the_threshold_are_cut_by_item_id(be):
    SL.check_ties(be)


def test_degenerate_rows(be):
    SL.check_degenerate_rows(be)


def test_request_order_grids_and_tables_left_clean(be):
    SL.check_order_and_grids(be)          # (ids -1 and 2^31 - 1: refused before any row pointer is read)


@pytest.mark.parametrize('delta', [-1, 0, 1])
def test_w_in_lds_and_in_the_scratch_row(be, delta):
    SL.check_w_table_switch(be, delta)


def test_what_has_no_place_is_reported_and_not_written(be):
    SL.check_no_place(be)


def test_a_user_id_out_of_range_is_reported(be):
    SL.check_bad_user(be, (10, -1, 2 ** 31 - 1))


@pytest.mark.parametrize('bad', BAD_OFFSETS)
def test_inconsistent_query_offsets_are_reported_and_not_followed(be, bad):
    SL.check_bad_query_offsets(be, bad, wild=False)


def test_bad_arguments_and_a_graph_past_the_vote_bound_are_refused(be):
    SL.check_refusals(be.lib)
    be.sync()          # (nothing was launched: nothing can have gone wrong behind the calls)


@pytest.mark.parametrize('n_items', SL.N_ITEMS_SMALL + [SL.TILE + 1, 2 * SL.TILE + SL.TILE // 2])
def test_places_are_the_index_in_the_vote_order(be, n_items):
    if n_items > 1000:
        SL.check_places(be, 8, n_items, thresholds=((0, 0),), masks=(True,), excludes=(1,))
    else:
        SL.check_places(be, 60, n_items)


# ------------------------------------------------------------------ the Python surface
N_U, N_I, M_SMALL, KS = 60, 80, 12, (1, 5, 10)


class Case(object):
    """A 60 x 80 graph WITHOUT a per-hop cap -- the extraction draws nothing, so a score does not depend on the link's place
    in its pass --, a sixth of its ratings held out, the exhaustive score of every candidate (computed once) and the
    reference shortlists."""

    def __init__(self):
        import torch
        from igmc_amd.models import IGMC
        from igmc_amd.recommend import CandidateLinks, score_candidates
        from igmc_amd.util_functions import MyDynamicDataset
        full = random_rating_graph(N_U, N_I, 0.25, 5, 21)
        full.eliminate_zeros()
        rows, cols = full.nonzero()
        vals = np.asarray(full[rows, cols]).ravel()
        held = np.random.default_rng(4).random(len(rows)) < 1 / 6
        held[rows == 7] = False          # user 7 keeps every rating: no held-out link
        self.A = ssp.csr_matrix((vals[~held], (rows[~held], cols[~held])), shape=full.shape).astype(np.float32)
        self.cv = np.arange(1, 6, dtype=np.float64)
        tr, tc = self.A.nonzero()
        labels = np.asarray(self.A[tr, tc]).ravel().astype(np.int64) - 1
        self.ds = MyDynamicDataset('data/t/short_a', self.A, (tr, tc), labels, 1, 1.0, None, None, None, self.cv, seed=1)
        torch.manual_seed(4)
        self.model = IGMC(self.ds, latent_dim=[32, 32, 32, 32], num_relations=5, num_bases=4, regression=True, adj_dropout=0.2,
                          seed=3).to('cuda')
        self.model.reset_parameters()
        self.model.eval()
        # held-out links: the removed ratings, and a few links that are STILL in the training graph (no candidates)
        self.hu = np.concatenate([rows[held], tr[:9]]).astype(np.int32)
        self.hv = np.concatenate([cols[held], tc[:9]]).astype(np.int32)
        self.hr = np.concatenate([vals[held], np.full(9, 5.0)]).astype(np.float32)
        self.users = np.arange(N_U, dtype=np.int32)
        cands = CandidateLinks.for_users(self.ds, self.users)
        self.off = cands.offsets.cpu().numpy()
        self.items = cands.link_v[:len(cands)].cpu().numpy()
        self.scores = score_candidates(self.model, cands, 50).cpu().numpy()
        self.short = SL.segments_ref(self.A, self.users, M_SMALL)          # link_u, link_v, votes, counts

    def shortlist_of(self, u):
        o = SL.offsets(self.short[3])
        return self.short[1][o[u]:o[u + 1]]


@pytest.fixture(scope='module')
def case():
    return Case()


def test_refill_with_a_shortlist_writes_the_reference_segments_and_their_votes(case):
    import torch
    from igmc_amd.recommend import CandidateLinks
    ru, rv, rw, rc = case.short
    cl = CandidateLinks.for_users(case.ds, case.users, shortlist=M_SMALL)
    assert len(cl) == len(ru) and cl.votes.dtype == torch.int32 and cl.votes.numel() == len(cl) and cl.forced is None
    assert np.array_equal(cl.link_u[:len(cl)].cpu().numpy(), ru) and np.array_equal(cl.link_v[:len(cl)].cpu().numpy(), rv)
    assert np.array_equal(cl.votes.cpu().numpy().astype(np.uint32), rw)
    assert np.array_equal(cl.offsets.cpu().numpy(), SL.offsets(rc))
    cl.refill(case.users[:5])
    assert cl.votes is None
    for call in (lambda: cl.refill(case.users, negatives=5, shortlist=5),
                 lambda: CandidateLinks.for_users(case.ds, case.users, negatives=5, shortlist=5),
                 lambda: cl.refill(case.users, shortlist=0)):
        with pytest.raises(ValueError, match='shortlist'):
            call()


def test_recommend_over_a_shortlist(case):
    import torch
    from igmc_amd.recommend import candidate_passes, recommend
    plain = recommend(case.model, case.ds, n=5)
    stats = {}
    every = recommend(case.model, case.ds, n=5, shortlist=N_I, stats=stats)          # M >= every |C|: the exhaustive result
    assert stats['shortlist'] == N_I and stats['candidates'] == len(case.items)
    for a, b in zip(plain, every):
        assert torch.equal(a, b)
    # a small M: the top-n of the exhaustive scores restricted to the reference shortlist, items and score bits
    stats = {}
    items, scores, counts = [t.cpu().numpy() for t in recommend(case.model, case.ds, n=5, shortlist=M_SMALL, stats=stats)]
    assert stats == dict(users=N_U, candidates=int(case.short[3].sum()), passes=1, shortlist=M_SMALL)
    differs = 0
    for u in range(N_U):
        idx = np.arange(case.off[u], case.off[u + 1])
        idx = idx[np.isin(case.items[idx], case.shortlist_of(u))]
        order = descending_order(case.scores[idx], idx)[:5]
        c = len(order)
        assert counts[u] == c and np.array_equal(items[u, :c], case.items[idx[order]])
        assert scores[u, :c].tobytes() == case.scores[idx[order]].tobytes()
        differs += not np.array_equal(items[u], plain[0][u].cpu().numpy())
    assert differs > 0          # (the shortlist does cut something a full ranking would have listed)
    with pytest.raises(ValueError, match='shortlist'):
        list(candidate_passes(case.model, case.ds, negatives=3, shortlist=3))


def _metrics_ref(case, heldout_u, heldout_v, relevant, m):
    """Per-user integer sums and float64 means with links the shortlist cut as misses, from the exhaustive scores."""
    nk = len(KS)
    per = {}
    cut = notc = 0
    for u, v, rel in zip(heldout_u, heldout_v, relevant):
        idx = np.arange(case.off[u], case.off[u + 1])
        if v not in case.items[idx]:
            notc += 1
            continue
        sl = case.shortlist_of(u) if m < N_I else case.items[idx]
        if v not in sl:
            cut += 1
            rank = None
        else:
            idx = idx[np.isin(case.items[idx], sl)]
            order = descending_order(case.scores[idx], idx)
            rank = int(np.nonzero(case.items[idx[order]] == v)[0][0])
        if rel:
            per.setdefault(int(u), []).append(rank)
    rows = []
    for u in sorted(per):
        ranks = per[u]
        real = [r for r in ranks if r is not None]
        n_rel = len(ranks)
        row = dict(n_rel=n_rel, first=min(real) if real else None)
        for j, k in enumerate(KS):
            hit = [r for r in real if r < k]
            row['hits%d' % j] = len(hit)
            row['dcg%d' % j] = sum(1.0 / np.log2(r + 2.0) for r in sorted(hit))
            row['idcg%d' % j] = sum(1.0 / np.log2(i + 2.0) for i in range(min(k, n_rel)))
        rows.append(row)
    n = float(len(rows))
    means = {}
    for j, k in enumerate(KS):
        means['hr@%d' % k] = sum(r['hits%d' % j] > 0 for r in rows) / n
        means['recall@%d' % k] = sum(r['hits%d' % j] / r['n_rel'] for r in rows) / n
        means['precision@%d' % k] = sum(r['hits%d' % j] / float(k) for r in rows) / n
        means['ndcg@%d' % k] = sum(r['dcg%d' % j] / r['idcg%d' % j] for r in rows) / n
    means['mrr'] = sum(0.0 if r['first'] is None else 1.0 / (r['first'] + 1.0) for r in rows) / n
    return rows, means, cut, notc


def test_rank_eval_counts_what_the_shortlist_cut_as_misses(case):
    import torch
    from igmc_amd.rank_eval import MISS_RANK, HeldOut, metric_names, rank_eval
    heldout = HeldOut.from_links(case.ds, case.hu, case.hv, ratings=case.hr, min_rating=3.0)
    s0, s1, s2 = {}, {}, {}
    plain = rank_eval(case.model, case.ds, heldout, ks=KS, stats=s0)
    every = rank_eval(case.model, case.ds, heldout, ks=KS, shortlist=N_I, stats=s1)
    assert s1['cut_by_shortlist'] == 0 and s1['shortlist'] == N_I and s1['not_candidates'] == s0['not_candidates'] == 9
    for k in metric_names(KS) + ['users_evaluated']:
        assert np.float64(plain[k]).tobytes() == np.float64(every[k]).tobytes(), k
    for k in ('rank', 'pos', 'cnt', 'dcg'):
        assert torch.equal(plain['per_user'][k], every['per_user'][k]), k
    small = rank_eval(case.model, case.ds, heldout, ks=KS, shortlist=M_SMALL, stats=s2)
    hu = np.repeat(heldout.users.cpu().numpy(), np.diff(heldout.offsets.cpu().numpy()))
    rows, means, cut, notc = _metrics_ref(case, hu, heldout.items.cpu().numpy(), heldout.relevant.cpu().numpy(), M_SMALL)
    assert cut > 0 and s2['cut_by_shortlist'] == cut and s2['not_candidates'] == notc == 9 and s2['shortlist'] == M_SMALL
    assert s2['candidates'] == int(case.short[3][heldout.users.cpu().numpy()].sum())          # (the held-out users' lists)
    cnt =small['per_user']['cnt'].cpu().numpy()
    dcg = small['per_user']['dcg'].cpu().numpy()
    keep = cnt[:, 0] > 0
    assert small['users_evaluated'] == len(rows) == int(keep.sum())
    assert cnt[keep, 0].tolist() == [r['n_rel'] for r in rows]
    assert cnt[keep, 1].tolist() == [MISS_RANK if r['first'] is None else r['first'] for r in rows]
    assert any(r['first'] is None for r in rows)          # a user whose every relevant link was cut: reciprocal rank 0
    for j in range(len(KS)):
        assert cnt[keep, 2 + j].tolist() == [r['hits%d' % j] for r in rows]
        assert np.allclose(dcg[keep, j], [r['dcg%d' % j] for r in rows], rtol=1e-12, atol=0)
        assert np.allclose(dcg[keep, len(KS) + j], [r['idcg%d' % j] for r in rows], rtol=1e-12, atol=0)
    for k in metric_names(KS):
        assert np.isclose(small[k], means[k], rtol=1e-12, atol=0), (k, small[k], means[k])
    # a cut link: no position in the pass, the miss rank, a place at or beyond M
    pu = small['per_user']
    cut_links = (pu['pos'] < 0) & (pu['place'] >= 0)
    assert int(cut_links.sum()) == cut and bool((pu['rank'][cut_links] == MISS_RANK).all()) and bool((pu['place'][cut_links] >= M_SMALL).all())
    with pytest.raises(ValueError, match='shortlist'):
        rank_eval(case.model, case.ds, heldout, ks=KS, shortlist=5, negatives=5)


def test_shortlist_recall_is_the_share_of_places_below_m(case):
    from igmc_amd.rank_eval import HeldOut, shortlist_recall
    heldout = HeldOut.from_links(case.ds, case.hu, case.hv, ratings=case.hr, min_rating=3.0)
    users = heldout.users.cpu().numpy()
    q_off, q_id, rel = heldout.offsets.cpu().numpy(), heldout.items.cpu().numpy(), heldout.relevant.cpu().numpy() != 0
    place, _ = SL.places_ref(case.A, users, q_off, q_id)
    owner = np.repeat(np.arange(len(users)), np.diff(q_off))
    counts = rel & (place >= 0)
    ms = (1, 5, M_SMALL, 40, N_I)
    stats = {}
    got = shortlist_recall(case.ds, heldout, ms=ms, stats=stats, users_per_pass=17)          # (four passes)
    per = np.bincount(owner[counts], minlength=len(users))
    assert stats == dict(users=len(users), queries=len(q_id), links=int(counts.sum()), users_counted=int((per > 0).sum()),
                         not_candidates=9, passes=4)
    for m in ms:
        hit = counts & (place < m)
        mine = np.bincount(owner[hit], minlength=len(users))
        assert got[m]['micro'] == hit.sum() / counts.sum()          # (one division of two exact integers)
        assert np.isclose(got[m]['macro'], (mine[per > 0] / per[per > 0]).mean(), rtol=1e-12, atol=0)
    assert got[N_I] == dict(micro=1.0, macro=1.0) and got[1]['micro'] < got[40]['micro']


def test_a_shortlist_over_a_graph_view_comes_from_the_new_graph(case):
    from igmc_amd.recommend import CandidateLinks, GraphView
    u = 7
    new_items = np.setdiff1d(np.arange(N_I), case.A.indices[case.A.indptr[u]:case.A.indptr[u + 1]])[[0, 5, 9]]
    g2 = case.ds.graph.updated(np.full(3, u), new_items, np.array([5, 4, 5]))
    B = case.A.tolil()
    B[u, new_items] = [5, 4, 5]
    B = B.tocsr()
    old = CandidateLinks.for_users(case.ds, [u], shortlist=M_SMALL)
    new = CandidateLinks.for_users(GraphView(case.ds, g2), [u], shortlist=M_SMALL)
    want = SL.segments_ref(B, [u], M_SMALL)
    assert np.array_equal(new.link_v[:len(new)].cpu().numpy(), want[1])
    assert np.array_equal(new.votes.cpu().numpy().astype(np.uint32), want[2])
    assert not np.array_equal(new.votes.cpu().numpy(), old.votes.cpu().numpy())
    assert not set(new.link_v[:len(new)].cpu().numpy().tolist()) & set(new_items.tolist())
    g2.close()


def test_main_shortlist_end_to_end(tmp_path):
    """``Main.py ... --epochs 1`` and then the same command with ``--no-train --recommend 5 --rank-eval 5,10 --shortlist 50``
    for the first 50 users."""
    from igmc_amd import preprocessing
    cmd = [sys.executable, os.path.join(ROOT, 'Main.py'), '--data-name', 'douban', '--epochs', '1', '--testing',
           '--save-interval', '1', '--dynamic-train', '--max-train-num', '2000', '--max-test-num', '700',
           '--max-nodes-per-hop', '100']
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = tmp_path / 'results' / 'douban_testmode'
    for extra in ([], ['--no-train', '--recommend', '5', '--recommend-users', '50', '--rank-eval', '5,10', '--shortlist', '50',
                       '--shortlist-min-rating', '3']):
        r = subprocess.run(cmd + extra, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=600)
        out = r.stdout.decode()
        assert r.returncode == 0, out[-3000:]
    assert '(shortlist 50)' in out and 'shortlist recall' in out
    A = ssp.csr_matrix(preprocessing.load_data_monti('douban', testing=True)[2])
    rec = [l.split('\t') for l in (res / 'recommendations_douban.tsv').read_text().splitlines()]
    assert len(rec) == 250
    short = SL.segments_ref(A, np.arange(50), 50, 2, 2)          # class_values 1..5: ratings >= 3 are relations >= 2
    off = SL.offsets(short[3])
    for k, u in enumerate(range(50)):
        mine = rec[5 * k:5 * k + 5]
        assert [int(x[0]) for x in mine] == [u] * 5 and [int(x[1]) for x in mine] == [1, 2, 3, 4, 5]
        s = [float(x[3]) for x in mine]
        assert all(a >= b for a, b in zip(s, s[1:]))
        assert {int(x[2]) for x in mine} <= set(short[1][off[u]:off[u + 1]].tolist())
    rank = [l.split('\t') for l in (res / 'ranking_douban.tsv').read_text().splitlines()]
    assert [x[0] for x in rank[-3:]] == ['shortlist', 'cut_by_shortlist', 'shortlist_recall'] and len(rank) == 2 * 4 + 1 + 3
    assert rank[-3][1] == '50' and int(rank[-2][1]) >= 0 and 0.0 <= float(rank[-1][1]) <= 1.0
    assert len(rank[-1][1].split('.')[1]) == 6
