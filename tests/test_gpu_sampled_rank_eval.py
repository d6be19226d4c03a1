"""Held-out ranking among K SAMPLED negatives on a real MI355X (``rank_eval(..., negatives=K)``, ``CandidateLinks.refill(...,
negatives=, must=)``, ``igmc_amd/csrc/candidates.hip``) on the small case of ``tests/test_gpu_rank_eval.py`` (30 x 40,
70 held-out links, no cap): with more negatives than any user has candidates it is the exhaustive evaluation bit for bit; with
7 the pass's list is the numpy definition of ``tests/sampled_candidates_checks.py``, ranks are the lexsort of that pass's own
scores and the metrics their float64 restatement; passes do not matter; a ``GraphView`` and ``DGCNN_RS`` are served alike; and
``Main.py --rank-negatives`` end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as ssp

import sampled_candidates_checks as SC
from helpers import ROOT
from test_gpu_rank_eval import _check_metrics, _numpy_metrics, _numpy_ranks, small          # noqa: F401  (small: the fixture)

pytestmark = pytest.mark.gpu
KS = (1, 5, 10)


def _musts(heldout):
    off, items = heldout.offsets.cpu().numpy(), heldout.items.cpu().numpy()
    return [items[off[q]:off[q + 1]] for q in range(len(off) - 1)]


def _list_is_the_definition(cands, A, users, musts, k, seed, draw=0):
    ru, rv, rf, rc = SC.segments_ref(A, users, k, musts, seed=seed, draw=draw)
    n = len(cands)
    assert n == len(ru) and np.array_equal(cands.offsets.cpu().numpy(), SC.offsets(rc))
    assert np.array_equal(cands.link_u[:n].cpu().numpy(), ru) and np.array_equal(cands.link_v[:n].cpu().numpy(), rv)
    assert np.array_equal(cands.forced.cpu().numpy(), rf) and cands.forced.numel() == n


def test_more_negatives_than_candidates_is_the_exhaustive_evaluation_bit_for_bit(small):
    import torch
    from igmc_amd.rank_eval import HeldOut, rank_eval
    ds, model, hu, hv, hy = small['ds'], small['model'], small['hu'], small['hv'], small['hy']
    heldout = HeldOut.from_links(ds, hu, hv, ratings=hy, min_rating=3)
    stats, stats_s = {}, {}
    full = rank_eval(model, ds, heldout, ks=KS, stats=stats)
    sampled = rank_eval(model, ds, heldout, ks=KS, stats=stats_s, negatives=10_000)
    assert stats_s == dict(stats, negatives=10_000, draw=0) and 'negatives' not in stats
    for k in ('rank', 'pos', 'cnt', 'dcg'):
        assert torch.equal(full['per_user'][k], sampled['per_user'][k]), k
    assert full.keys() == sampled.keys()
    for k in full:
        if k != 'per_user':
            assert full[k] == sampled[k], k


def test_seven_negatives_the_list_is_the_definition_and_ranks_the_lexsort_of_its_scores(small):
    import torch
    from igmc_amd.rank_eval import HeldOut, rank_eval
    from igmc_amd.recommend import CandidateLinks, score_candidates
    from igmc_amd.util_functions import MyDynamicDataset
    ds, model, hu, hv, hy, At = small['ds'], small['model'], small['hu'], small['hv'], small['hy'], small['A']
    heldout = HeldOut.from_links(ds, hu, hv)
    users, musts = np.arange(30, dtype=np.int32), _musts(heldout)
    stats = {}
    res = rank_eval(model, ds, heldout, ks=KS, stats=stats, negatives=7)
    cands = CandidateLinks.for_users(ds, users, negatives=7, must=(heldout.offsets, heldout.items))
    _list_is_the_definition(cands, At, users, musts, 7, ds.seed)
    forced = cands.forced.cpu().numpy()
    assert int(forced.sum()) == 70 and len(cands) == 70 + 30 * 7          # every held-out link a candidate, 7 more per user
    assert stats == dict(users=30, candidates=len(cands), passes=1, queries=70, not_candidates=0, negatives=7, draw=0)
    R = score_candidates(model, cands, 50).cpu().numpy()
    off, seg_items = cands.offsets.cpu().numpy(), cands.link_v[:len(cands)].cpu().numpy()
    rank, pos = _numpy_ranks(R, seg_items, off, {u: u for u in range(30)}, hu, hv)
    assert (rank >= 0).all() and rank.max() < 7 + np.diff(heldout.offsets.cpu().numpy()).max()
    assert np.array_equal(res['per_user']['rank'].cpu().numpy(), rank) and np.array_equal(res['per_user']['pos'].cpu().numpy(), pos)
    _check_metrics(res, *_numpy_metrics(rank, hu, KS))
    # another draw: other negatives beside the same must items, the definition again
    other = CandidateLinks.for_users(ds, users, negatives=7, must=(heldout.offsets, heldout.items), draw=1)
    _list_is_the_definition(other, At, users, musts, 7, ds.seed, draw=1)
    assert len(other) == len(cands) and not torch.equal(other.link_v[:len(other)], cands.link_v[:len(cands)])
    res1 = rank_eval(model, ds, heldout, ks=KS, negatives=7, draw=1)
    assert not torch.equal(res1['per_user']['rank'], res['per_user']['rank'])
    # without negatives the list is the exhaustive one, and forced is gone
    plain = CandidateLinks(ds, 30 * 40).refill(users, negatives=7, must=(heldout.offsets, heldout.items))
    assert torch.equal(plain.forced, cands.forced)
    plain.refill(users)
    assert plain.forced is None and len(plain) == 30 * 40 - At.nnz
    with pytest.raises(ValueError, match='negatives=K'):
        plain.refill(users, must=(heldout.offsets, heldout.items))
    # a held-out link that was also left in the training graph is no candidate in either protocol
    k = 17
    A2 = At.tolil()
    A2[hu[k], hv[k]] = hy[k]
    A2 = ssp.csr_matrix(A2)
    tu2, tv2 = A2.nonzero()
    ds2 = MyDynamicDataset('data/t/rk_s2', A2, (tu2, tv2), np.asarray(A2[tu2, tv2]).ravel().astype(np.int64) - 1, 1, 1.0, None,
                           None, None, small['cv'], seed=1)
    full2, samp2 = {}, {}
    rank_eval(model, ds2, HeldOut.from_links(ds2, hu, hv), ks=KS, stats=full2)
    res2 = rank_eval(model, ds2, HeldOut.from_links(ds2, hu, hv), ks=KS, stats=samp2, negatives=7)
    assert full2['not_candidates'] == 1 == samp2['not_candidates'] and samp2['candidates'] == 69 + 30 * 7
    assert res2['per_user']['rank'][k].item() == -1 and int((res2['per_user']['rank'] < 0).sum()) == 1


def test_one_user_per_pass_gives_the_lists_ranks_and_metrics_of_one_pass(small):
    import torch
    from igmc_amd.rank_eval import HeldOut, rank_eval
    from igmc_amd.recommend import candidate_passes
    ds, model, hu, hv = small['ds'], small['model'], small['hu'], small['hv']
    heldout = HeldOut.from_links(ds, hu, hv)
    must = (heldout.offsets, heldout.items)

    def lists(upp):
        v, f, n = [], [], 0
        for q0, cands, R in candidate_passes(model, ds, heldout.users, users_per_pass=upp, negatives=7, must=must):
            assert q0 == (n if upp else 0) and cands.users.numel() == (1 if upp else 30)
            n += cands.users.numel()
            v.append(cands.link_v[:len(cands)].clone())
            f.append(cands.forced.clone())
            assert R.numel() == len(cands)
        return torch.cat(v), torch.cat(f), len(v)

    v1, f1, p1 = lists(None)
    v30, f30, p30 = lists(1)
    assert (p1, p30) == (1, 30)
    assert torch.equal(v1, v30) and torch.equal(f1, f30)
    stats = {}
    one = rank_eval(model, ds, heldout, ks=KS, negatives=7)
    each = rank_eval(model, ds, heldout, ks=KS, negatives=7, users_per_pass=1, stats=stats)
    assert stats['passes'] == 30 and stats['candidates'] == v1.numel()
    for k in ('rank', 'cnt', 'dcg'):
        assert torch.equal(one['per_user'][k], each['per_user'][k]), k
    assert all(one[k] == each[k] for k in one if k != 'per_user')


def test_over_a_graph_view_with_a_brand_new_user(small):
    from igmc_amd.rank_eval import HeldOut, rank_eval
    from igmc_amd.recommend import CandidateLinks, GraphView, score_candidates
    ds, model, At = small['ds'], small['model'], small['A']
    g2 = ds.graph.updated(np.array([30, 30, 30, 2], np.int32), np.array([3, 17, 25, 40], np.int32), np.array([5, 1, 4, 3], np.uint8))
    view = GraphView(ds, g2)
    A2 = ssp.lil_matrix((31, 41), dtype=np.float32)
    A2[:30, :40] = At
    A2[30, 3], A2[30, 17], A2[30, 25], A2[2, 40] = 5, 1, 4, 3
    A2 = ssp.csr_matrix(A2)
    free = int(np.setdiff1d(np.arange(40), A2[2].indices)[0])
    hu, hv = np.array([2, 30, 30, 30]), np.array([free, 3, 8, 40])          # (30, 3) is in the graph: no candidate
    heldout = HeldOut.from_links(view, hu, hv)
    stats = {}
    res = rank_eval(model, view, heldout, ks=KS, negatives=5, stats=stats)
    assert stats['not_candidates'] == 1 and stats['users'] == 2 and stats['candidates'] == 3 + 2 * 5
    users, musts = np.array([2, 30], np.int32), _musts(heldout)
    cands = CandidateLinks.for_users(view, users, negatives=5, must=(heldout.offsets, heldout.items))
    _list_is_the_definition(cands, A2, users, musts, 5, ds.seed)
    R = score_candidates(model, cands, 50).cpu().numpy()
    rank, pos = _numpy_ranks(R, cands.link_v[:len(cands)].cpu().numpy(), cands.offsets.cpu().numpy(), {2: 0, 30: 1}, hu, hv)
    assert rank.tolist()[1] == -1 and (np.delete(rank, 1) >= 0).all()
    assert np.array_equal(res['per_user']['rank'].cpu().numpy(), rank) and np.array_equal(res['per_user']['pos'].cpu().numpy(), pos)
    _check_metrics(res, *_numpy_metrics(rank, hu, KS))


def test_dgcnn_rs_sampled_ranks_are_the_lexsort_of_its_own_scores(small):
    import torch
    from igmc_amd.models import DGCNN_RS
    from igmc_amd.rank_eval import HeldOut, rank_eval
    from igmc_amd.recommend import score_candidates
    from igmc_amd.util_functions import MyDynamicDataset
    hu, hv, At = small['hu'], small['hv'], small['A']
    tu, tv = At.nonzero()
    ds = MyDynamicDataset('data/t/rk_sd', At, (tu, tv), np.asarray(At[tu, tv]).ravel().astype(np.int64) - 1, 1, 1.0, None, None,
                          None, small['cv'], seed=2)
    torch.manual_seed(4)
    model = DGCNN_RS(ds, latent_dim=[32, 32, 32, 1], k=30, num_relations=5, num_bases=4, regression=True, adj_dropout=0.2,
                     seed=1).to('cuda')
    model.reset_parameters()
    model.eval()
    heldout = HeldOut.from_links(ds, hu, hv)
    res = rank_eval(model, ds, heldout, ks=KS, negatives=7)
    cands = ds._recommend_links
    _list_is_the_definition(cands, At, np.arange(30, dtype=np.int32), _musts(heldout), 7, 2)
    R = score_candidates(model, cands, 50).cpu().numpy()
    rank, pos = _numpy_ranks(R, cands.link_v[:len(cands)].cpu().numpy(), cands.offsets.cpu().numpy(), {u: u for u in range(30)},
                             hu, hv)
    assert np.array_equal(res['per_user']['rank'].cpu().numpy(), rank) and np.array_equal(res['per_user']['pos'].cpu().numpy(), pos)
    _check_metrics(res, *_numpy_metrics(rank, hu, KS))


def test_main_rank_negatives_end_to_end(tmp_path):
    """``Main.py ... --epochs 1 --max-train-num 2000`` for a checkpoint, then ``--no-train --rank-eval 5,10 --rank-negatives 7``:
    the file has the two extra lines; ``--rank-negatives`` without ``--rank-eval`` is the parser's error."""
    cmd = [sys.executable, os.path.join(ROOT, 'Main.py'), '--data-name', 'douban', '--epochs', '1', '--testing',
           '--save-interval', '1', '--dynamic-train', '--dynamic-test', '--max-train-num', '2000', '--max-nodes-per-hop', '100']
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(cmd + ['--rank-negatives', '7'], cwd=str(tmp_path), env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 2 and '--rank-negatives samples the negatives of --rank-eval' in r.stdout.decode()
    tsv = tmp_path / 'results' / 'douban_testmode' / 'ranking_douban.tsv'
    for extra in ([], ['--no-train', '--rank-eval', '5,10', '--recommend-users', '50', '--rank-negatives', '7']):
        r = subprocess.run(cmd + extra, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=600)
        out = r.stdout.decode()
        assert r.returncode == 0, out[-3000:]
    line = [l for l in out.splitlines() if l.startswith('Ranked ')]
    assert len(line) == 1 and 'hr@5' in line[0]
    print(line[0])
    rec = dict(l.split('\t') for l in tsv.read_text().splitlines())
    assert list(rec) == ['hr@5', 'recall@5', 'precision@5', 'ndcg@5', 'hr@10', 'recall@10', 'precision@10', 'ndcg@10', 'mrr',
                         'negatives', 'draw']
    assert rec['negatives'] == '7' and rec['draw'] == '0'
    assert all(0.0 <= float(rec[k]) <= 1.0 for k in list(rec)[:9])
