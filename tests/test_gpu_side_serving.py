"""Serving a ``--use-features`` model on a real MI355X: candidate lists, leave-one-out variants and graph views gather the side
features of their links' two target nodes from per-node tables (``igmc_batch_bind_side_tables``, ``k_side_gather_nodes``).

THE ORACLE is the dataset's own path -- its per-position matrix gathered by ``k_side_gather``, held to the reference by
``test_side_features`` and the ``igmc_side`` fixture --: the same pairs at the same positions must score bit for bit the same
through both.  On top of it ``recommend`` / ``rank_eval`` / ``explain`` are held to their own pass's scores as the featureless
tests hold them (tests/test_gpu_recommend.py, tests/test_gpu_rank_eval.py, tests/test_gpu_explain.py), a ``GraphView`` to a dataset
rebuilt from scratch, and ``Main.py`` end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as ssp

from helpers import ROOT
from test_gpu_rank_eval import _check_metrics, _numpy_metrics, _numpy_ranks
from test_gpu_recommend import _complement, _expect_lists

pytestmark = pytest.mark.gpu
B = 8


@pytest.fixture(scope='module')
def flix():
    """The flixster split with random fp32 side features: ``uf [n_users, 12]``, ``vf [n_items, 20]``."""
    from igmc_amd import preprocessing
    (_, _, adj, trl, tru, trv, _, _, _, tel, teu, tev, cv) = preprocessing.load_data_monti('flixster', testing=True)
    rng = np.random.default_rng(0)
    uf = rng.standard_normal((adj.shape[0], 12)).astype(np.float32)
    vf = rng.standard_normal((adj.shape[1], 20)).astype(np.float32)
    return dict(adj=ssp.csr_matrix(adj), trl=trl, tru=tru, trv=trv, tel=tel, teu=teu, tev=tev, cv=cv, uf=uf, vf=vf)


def _dataset(flix, tag, cap, n=200, uf=None, vf=None, adj=None, links=None):
    from igmc_amd.util_functions import MyDynamicDataset
    u, v, l = (flix['tru'][:n], flix['trv'][:n], flix['trl'][:n]) if links is None else links
    uf, vf = flix['uf'] if uf is None else uf, flix['vf'] if vf is None else vf
    return MyDynamicDataset('data/t/ss_' + tag, flix['adj'] if adj is None else adj, (u, v), l, 1, 1.0, cap, uf, vf, flix['cv'],
                            seed=2)


def _igmc(ds, R, n_side, seed=4):
    import torch
    from igmc_amd.models import IGMC
    torch.manual_seed(seed)
    model = IGMC(ds, latent_dim=[32, 32, 32, 32], num_relations=R, num_bases=4, regression=True, adj_dropout=0.2,
                 side_features=n_side > 0, n_side_features=n_side, seed=3).to('cuda')
    model.reset_parameters()
    model.eval()
    return model


@pytest.fixture(scope='module')
def served(flix):
    """200 training links under a per-hop cap of 10 (sampling binds: positions matter), a model of random parameters over the
    32 feature columns."""
    ds = _dataset(flix, 'train', 10)
    return dict(ds=ds, model=_igmc(ds, len(flix['cv']), 32))


@pytest.mark.parametrize('cap', [10000, 10])
@pytest.mark.parametrize('fu,fv', [(12, 20), (3, 5)])
def test_pairs_score_like_the_dataset_of_the_same_links(flix, cap, fu, fv):
    """19 links, batches of 8 (the last one ragged); 32 columns: the MFMA head, 8: the generic one (D % 16 != 0).  Positions and
    sampling keys coincide, so the subgraphs do; the rows come by link position on one side and by node id on the other."""
    import torch
    from igmc_amd.recommend import CandidateLinks, score_candidates
    from igmc_amd.train_eval import score_links
    ds = _dataset(flix, 'p%d_%d' % (cap, fu + fv), cap, n=19, uf=flix['uf'][:, :fu], vf=flix['vf'][:, :fv])
    assert ds.n_side_features == fu + fv and len(ds) == 19
    model = _igmc(ds, len(flix['cv']), fu + fv)
    want, _, _ = score_links(model, ds, B)
    pairs = CandidateLinks.from_pairs(ds, ds.link_u, ds.link_v)
    assert pairs.n_side_features == fu + fv and not pairs.group_extractable and pairs._side is None
    tables = ds.node_side()
    assert pairs.node_side() is tables and ds.node_side() is tables          # built once, one copy for every derived source
    assert tuple(tables[0].shape) == (flix['adj'].shape[0], fu) and tuple(tables[1].shape) == (flix['adj'].shape[1], fv)
    got = score_candidates(model, pairs, B)
    print('cap %d, %d + %d columns: max |by node - by position| = %g' % (cap, fu, fv, (got - want).abs().max().item()))
    assert torch.isfinite(want).all() and torch.equal(got, want)
    # the rows a batch carries are its links' target rows (DeviceBatch.side: the arena's gathered rows)
    db = pairs.extract(None, 8, 8, max_graphs=B)
    rows = np.hstack([flix['uf'][flix['tru'][8:16], :fu], flix['vf'][flix['trv'][8:16], :fv]])
    assert db.side.shape == (8, fu + fv) and db.side.cpu().numpy().tobytes() == rows.tobytes()
    # THE FEATURES MATTER: the same pairs under a model whose lin1 side columns are zero score differently
    blind = _igmc(ds, len(flix['cv']), fu + fv)
    blind.load_state_dict(model.state_dict())
    with torch.no_grad():
        blind.lin1.weight[:, 256:].zero_()
    dark = score_candidates(blind, CandidateLinks.from_pairs(ds, ds.link_u, ds.link_v), B)
    assert torch.isfinite(dark).all() and not torch.equal(dark, want) and (dark - want).abs().max().item() > 1e-3


def test_recommend_lists_are_the_lexsort_of_the_pass_and_a_replayed_pass_equals_a_fresh_one(flix, served):
    import torch
    from igmc_amd.recommend import CandidateLinks, recommend, score_candidates
    ds, model = served['ds'], served['model']
    users = np.array([int(np.argmax(np.diff(flix['adj'].indptr))), 7, 1500], np.int32)
    hu, hv, off = _complement(flix['adj'], users)
    stats = {}
    items, scores, counts = recommend(model, ds, users=users, n=5, batch_size=B, stats=stats)
    assert stats == dict(users=3, candidates=len(hu), passes=1)
    fresh = CandidateLinks.for_users(ds, users)
    R = score_candidates(model, fresh, B)
    assert fresh._scoregraph.graph is not None and ds._recommend_links._scoregraph.graph is not None      # both passes replayed a captured graph
    I, S, C = _expect_lists(R.cpu().numpy(), hv, off, 5)
    assert np.array_equal(counts.cpu().numpy(), C) and np.array_equal(items.cpu().numpy(), I)
    assert scores.cpu().numpy().tobytes() == S.tobytes() and np.isfinite(S).all()
    # other users through the kept CandidateLinks: the graph its first pass captured, replayed with the tables it holds
    kept, graph = ds._recommend_links, ds._recommend_links._scoregraph.graph
    others = np.array([2, 2999, 11], np.int32)
    again = recommend(model, ds, users=others, n=5, batch_size=B)
    assert ds._recommend_links is kept and kept._scoregraph.graph is graph
    _, ov, ooff = _complement(flix['adj'], others)
    R2 = score_candidates(model, CandidateLinks.for_users(ds, others), B)
    I2, S2, C2 = _expect_lists(R2.cpu().numpy(), ov, ooff, 5)
    assert np.array_equal(again[0].cpu().numpy(), I2) and again[1].cpu().numpy().tobytes() == S2.tobytes()
    assert np.array_equal(again[2].cpu().numpy(), C2)
    assert not torch.equal(again[1], scores)


@pytest.mark.parametrize('negatives', [None, 20])
def test_rank_eval_equals_the_host_metrics_of_the_same_scores(flix, served, negatives):
    from igmc_amd.rank_eval import HeldOut, rank_eval
    from igmc_amd.recommend import CandidateLinks, score_candidates
    ds, model = served['ds'], served['model']
    teu, tev = np.asarray(flix['teu']), np.asarray(flix['tev'])
    users = np.unique(teu)[:3].astype(np.int32)
    keep = np.isin(teu, users)
    hu, hv = teu[keep], tev[keep]
    order = np.lexsort((hv, hu))
    hu, hv = hu[order], hv[order]
    heldout = HeldOut.from_links(ds, hu, hv)
    ks = (1, 5, 10)
    stats = {}
    res = rank_eval(model, ds, heldout, ks=ks, batch_size=B, stats=stats, negatives=negatives)
    must = None if negatives is None else (heldout.offsets, heldout.items)
    cands = CandidateLinks.for_users(ds, users, negatives=negatives, must=must)
    assert stats['users'] == 3 and stats['candidates'] == len(cands) and stats['queries'] == len(hu) and stats['not_candidates'] == 0
    R = score_candidates(model, cands, B).cpu().numpy()
    off, seg_items = cands.offsets.cpu().numpy(), cands.link_v[:len(cands)].cpu().numpy()
    rank, pos = _numpy_ranks(R, seg_items, off, {int(u): i for i, u in enumerate(users)}, hu, hv)
    assert (rank >= 0).all() and np.isfinite(R).all()
    assert np.array_equal(res['per_user']['rank'].cpu().numpy(), rank) and np.array_equal(res['per_user']['pos'].cpu().numpy(), pos)
    _check_metrics(res, *_numpy_metrics(rank, hu, ks))


def test_explain_variants_carry_their_base_links_rows(flix, served):
    import torch
    from igmc_amd.explain import explain, explain_all
    from igmc_amd.recommend import CandidateLinks, score_candidates
    from igmc_amd.train_eval import SCORE_EPOCH
    ds, model = served['ds'], served['model']
    u = np.array([flix['tru'][0], flix['teu'][0], 7, flix['tru'][0]], np.int32)
    v = np.array([flix['trv'][0], flix['tev'][0], 1234, flix['trv'][3]], np.int32)
    res = explain_all(model, ds, u, v, batch_size=B)
    base = score_candidates(model, CandidateLinks.from_pairs(ds, u, v), B)
    var_off = res['var_off'].cpu().numpy()
    assert torch.isfinite(res['scores']).all() and int(var_off[-1]) > 4 + 4          # neighbours to remove
    assert torch.equal(res['scores'][res['var_off'][:-1]], base) and torch.equal(res['base'], base)
    removed = res['var_side'] != 255
    link = res['var_link'].long()
    assert torch.equal(res['delta'], (res['scores'] - base[link])[removed])
    assert (res['delta'] != 0).any()
    # the variants of the pass still sit in the kept LeaveOneOutLinks: a batch of them across the end of link 0 carries, row by
    # row, the feature rows of its base link's targets
    loo = ds._explain_links
    assert loo.n_side_features == 32 and loo.node_side() is ds.node_side() and len(loo) == int(var_off[-1])
    first = max(0, int(var_off[1]) - 3)
    assert first + B <= len(loo)
    db = loo.extract(None, first, B, epoch=SCORE_EPOCH, slot='rows', max_graphs=B)
    li = res['var_link'][first:first + B].cpu().numpy()
    assert len(set(li.tolist())) >= 2
    rows = np.hstack([flix['uf'][u[li]], flix['vf'][v[li]]])
    assert db.side.cpu().numpy().tobytes() == rows.tobytes()
    # the selection is made of those deltas
    top = explain(model, ds, u, v, m=3, batch_size=B)
    assert torch.equal(top['base'], base) and int(top['counts'][0]) >= 1
    d0 = res['delta'][int(res['seg_off'][0]):int(res['seg_off'][1])].abs().max()
    assert top['deltas'][0, 0].abs() == d0


def test_graph_view_with_and_without_the_new_nodes_rows(flix, served):
    """One new user with three ratings and one new item: with extended feature arrays the view equals a dataset built from
    scratch on the changed matrix with those arrays; without them the same with ZERO rows appended."""
    import torch
    from igmc_amd.recommend import CandidateLinks, GraphView, score_candidates
    from igmc_amd.train_eval import score_links
    ds, model, adj = served['ds'], served['model'], flix['adj']
    nu, ni = adj.shape
    rated, ratings = np.array([3, 812, 17], np.int32), np.array([4, 9, 1], np.uint8)
    g2 = ds.graph.updated(np.full(3, nu, np.int32), rated, ratings, n_items=ni + 1)
    assert (g2.n_users, g2.n_items) == (nu + 1, ni + 1)
    A2 = adj.tolil()
    A2.resize((nu + 1, ni + 1))
    A2[nu, rated] = ratings
    A2 = ssp.csr_matrix(A2)
    rng = np.random.default_rng(5)
    u = np.array([nu, nu, 5, 5, nu, int(flix['tru'][0])] + rng.integers(0, nu, 5).tolist(), np.int32)
    v = np.array([812, 40, ni, 3, ni, int(flix['trv'][0])] + rng.integers(0, ni, 5).tolist(), np.int32)
    new_u, new_v = rng.standard_normal((1, 12)).astype(np.float32), rng.standard_normal((1, 20)).astype(np.float32)
    got = {}
    for tag, xu, xv, given in (('named', new_u, new_v, True), ('zeros', np.zeros_like(new_u), np.zeros_like(new_v), False)):
        uf2, vf2 = np.vstack([flix['uf'], xu]), np.vstack([flix['vf'], xv])
        view = GraphView(ds, g2, uf2, vf2) if given else GraphView(ds, g2)
        assert (view.node_side() is ds.node_side()) == (not given) and view.n_side_features == 32
        got[tag] = score_candidates(model, CandidateLinks.from_pairs(view, u, v), B)
        rebuilt = _dataset(flix, 'gv_' + tag, 10, uf=uf2, vf=vf2, adj=A2, links=(u, v, np.zeros(len(u), np.int64)))
        want, _, _ = score_links(model, rebuilt, B)
        assert torch.isfinite(want).all() and torch.equal(got[tag], want), tag
    touched = torch.from_numpy((u == nu) | (v == ni)).cuda()          # only the pairs of the new nodes read other rows
    assert int(touched.sum()) == 4
    assert (got['named'][touched] != got['zeros'][touched]).all() and torch.equal(got['named'][~touched], got['zeros'][~touched])
    # arrays that do not fit the dataset's tables
    with pytest.raises(ValueError):
        GraphView(ds, g2, flix['uf'][:-1], flix['vf'])
    with pytest.raises(ValueError):
        GraphView(ds, g2, flix['uf'], flix['vf'][:, :19])
    with pytest.raises(ValueError):
        GraphView(ds, g2, flix['uf'])


def test_main_serves_a_use_features_checkpoint_end_to_end(tmp_path):
    """``Main.py --data-name douban --use-features --epochs 1`` on a few hundred links for a checkpoint, then ``--no-train
    --use-features --recommend 3 --recommend-users 2 --rank-eval 5 --explain 2``: the three TSVs exist, are well formed and hold
    finite scores.  (1000 test links: user 1 has a held-out link among them.)"""
    cmd = [sys.executable, os.path.join(ROOT, 'Main.py'), '--data-name', 'douban', '--use-features', '--epochs', '1', '--testing',
           '--save-interval', '1', '--dynamic-train', '--max-train-num', '300', '--max-test-num', '1000',
           '--max-nodes-per-hop', '100']
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = tmp_path / 'results' / 'douban_testmode'
    for extra in ([], ['--no-train', '--recommend', '3', '--recommend-users', '2', '--rank-eval', '5', '--explain', '2']):
        r = subprocess.run(cmd + extra, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        out = r.stdout.decode()
        assert r.returncode == 0, out[-3000:]
    rec = [l.split('\t') for l in (res / 'recommendations_douban.tsv').read_text().splitlines()]
    assert [int(x[0]) for x in rec] == [0] * 3 + [1] * 3 and [int(x[1]) for x in rec] == [1, 2, 3] * 2
    assert all(len(x) == 4 and 0 <= int(x[2]) < 3000 and np.isfinite(float(x[3])) for x in rec)
    rk = dict(l.split('\t') for l in (res / 'ranking_douban.tsv').read_text().splitlines())
    assert list(rk) == ['hr@5', 'recall@5', 'precision@5', 'ndcg@5', 'mrr']
    assert all(np.isfinite(float(x)) and 0.0 <= float(x) <= 1.0 for x in rk.values())
    ex = [l.split('\t') for l in (res / 'explanations_douban.tsv').read_text().splitlines()]
    assert ex[0] == ['user', 'item', 'score', 'place', 'side', 'node', 'rating', 'delta', 'score_without']
    body = ex[1:]
    assert all(len(x) == 9 for x in body) and len(body) >= 6
    assert [(int(x[0]), int(x[1])) for x in body if x[3] in ('0', '1')] == [(int(x[0]), int(x[2])) for x in rec]
    assert all(np.isfinite([float(x[2]), float(x[7]), float(x[8])]).all() for x in body)
    assert 'Explained 6 links' in out and 'Recommended for 2 users' in out and 'Ranked' in out
