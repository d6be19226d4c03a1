"""Held-out ranking evaluation on a real MI355X (``igmc_amd/rank_eval.py``, ``igmc_amd/csrc/ranking.hip``): the rank of a held-out
link is its place in the numpy lexsort of its pass's scores, the metrics are their numpy float64 restatement, passes do not
matter where no cap binds, ranks agree with ``recommend`` and -- within what the score tolerance allows -- with the CPU oracle,
links that are no candidates are reported and left out, and ``Main.py --rank-eval`` end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as ssp

import parity_checks as PC
from helpers import ROOT, random_rating_graph

pytestmark = pytest.mark.gpu


def _numpy_ranks(scores, seg_items, off, users_of, hu, hv):
    """Rank and position of every link (hu[i], hv[i]) in the descending lexsort of its user's score segment (-1: no
    candidate).  users_of: user id -> segment."""
    rank, pos = np.full(len(hu), -1, np.int64), np.full(len(hu), -1, np.int64)
    place = {}
    for i, (u, v) in enumerate(zip(hu, hv)):
        s = users_of[int(u)]
        lo, hi = off[s], off[s + 1]
        if s not in place:
            k, idx = scores[lo:hi], np.arange(lo, hi)
            assert not np.isneginf(k).any()
            place[s] = np.argsort(np.lexsort((idx, np.where(np.isnan(k), np.inf, -k))))
        p = lo + np.searchsorted(seg_items[lo:hi], v)
        if p < hi and seg_items[p] == v:
            rank[i], pos[i] = place[s][p - lo], p
    return rank, pos


def _numpy_metrics(rank, hu, ks, relevant=None):
    """The metrics of rank_eval.py's docstring, restated: float64 means over users with a relevant ranked link."""
    out = {('%s@%d' % (m, k)): [] for k in ks for m in ('hr', 'recall', 'precision', 'ndcg')}
    out['mrr'] = []
    for u in np.unique(hu):
        keep = (hu == u) & (rank >= 0)
        if relevant is not None:
            keep &= relevant
        r = np.sort(rank[keep]).astype(np.float64)
        if not len(r):
            continue
        for k in ks:
            hit = r[r < k]
            out['hr@%d' % k].append(float(len(hit) > 0))
            out['recall@%d' % k].append(len(hit) / len(r))
            out['precision@%d' % k].append(len(hit) / k)
            out['ndcg@%d' % k].append((1.0 / np.log2(hit + 2.0)).sum() / (1.0 / np.log2(np.arange(min(k, len(r))) + 2.0)).sum())
        out['mrr'].append(1.0 / (r[0] + 1.0))
    n = len(out['mrr'])
    return {k: float(np.mean(np.asarray(v, np.float64))) for k, v in out.items()}, n


def _check_metrics(res, want, n):
    assert res['users_evaluated'] == n
    for k, v in want.items():
        assert isinstance(res[k], float)
        assert abs(res[k] - v) <= 1e-12 * max(abs(v), 1e-300), (k, res[k], v)


@pytest.fixture(scope='module')
def small():
    """``random_rating_graph(30, 40, 0.3, 5, 21)`` with every fifth rating held out (70 links over 30 users; the smallest
    training row keeps 5 entries), no cap, and the weights of ``PC.make_ref_model(4, 5, seed=6)``."""
    import torch
    from igmc_amd.models import IGMC
    from igmc_amd.util_functions import MyDynamicDataset
    A = random_rating_graph(30, 40, 0.3, 5, 21)
    A.eliminate_zeros()
    cv = np.arange(1, 6, dtype=np.float64)
    rows, cols = A.nonzero()
    vals = np.asarray(A[rows, cols]).ravel()
    held = np.arange(len(rows)) % 5 == 2
    hu, hv, hy = rows[held], cols[held], vals[held]
    tu, tv = rows[~held], cols[~held]
    At = ssp.csr_matrix((vals[~held].astype(np.float32), (tu, tv)), shape=A.shape)
    assert len(hu) == 70 and len(np.unique(hu)) == 30 and np.diff(At.indptr).min() == 5
    ds = MyDynamicDataset('data/t/rk_s', At, (tu, tv), vals[~held].astype(np.int64) - 1, 1, 1.0, None, None, None, cv, seed=1)
    torch.manual_seed(4)
    model = IGMC(ds, latent_dim=[32, 32, 32, 32], num_relations=5, num_bases=4, regression=True, adj_dropout=0.2,
                 seed=3).to('cuda')
    model.reset_parameters()
    model.eval()
    ref = PC.make_ref_model(4, 5, seed=6)
    ref.eval()
    ws = model._workspace(ds.extract(None, 0, 1))
    model.flat_parameters().data.copy_(torch.from_numpy(PC.flatten_params(ws, ref)).cuda())
    return dict(A=At, cv=cv, ds=ds, model=model, ref=ref, hu=hu, hv=hv, hy=hy)


def test_ranks_are_the_lexsort_of_the_pass_and_metrics_their_restatement(small):
    import torch
    from igmc_amd.rank_eval import HeldOut, rank_eval
    from igmc_amd.recommend import CandidateLinks, recommend, score_candidates
    from igmc_amd.util_functions import MyDynamicDataset
    ds, model, hu, hv, hy, At = small['ds'], small['model'], small['hu'], small['hv'], small['hy'], small['A']
    ks = (1, 5, 10)
    heldout = HeldOut.from_links(ds, hu, hv, ratings=hy, min_rating=3)
    assert np.array_equal(heldout.users.cpu().numpy(), np.arange(30)) and len(heldout) == 70
    assert np.array_equal(heldout.items.cpu().numpy(), hv)          # nonzero() order is (user, item) order already
    assert np.array_equal(heldout.relevant.cpu().numpy() != 0, hy >= 3)
    stats = {}
    res = rank_eval(model, ds, heldout, ks=ks, stats=stats)
    assert stats == dict(users=30, candidates=30 * 40 - At.nnz, passes=1, queries=70, not_candidates=0)
    pu = res['per_user']
    assert all(pu[k].is_cuda for k in ('users', 'offsets', 'items', 'cnt', 'dcg', 'rank', 'pos'))
    assert pu['rank'].dtype == torch.int32 and pu['cnt'].shape == (30, 5) and pu['dcg'].shape == (30, 6)
    assert pu['dcg'].dtype == torch.float64
    # the same pass, its score bits pulled from the device
    cands = CandidateLinks.for_users(ds, np.arange(30))
    R = score_candidates(model, cands, 50).cpu().numpy()
    off, seg_items = cands.offsets.cpu().numpy(), cands.link_v[:len(cands)].cpu().numpy()
    rank, pos = _numpy_ranks(R, seg_items, off, {u: u for u in range(30)}, hu, hv)
    assert (rank >= 0).all()
    assert np.array_equal(pu['rank'].cpu().numpy(), rank) and np.array_equal(pu['pos'].cpu().numpy(), pos)
    want, n = _numpy_metrics(rank, hu, ks, hy >= 3)
    print('small case: %d users evaluated, ranks %d..%d, %s' % (n, rank.min(), rank.max(),
                                                                 ', '.join('%s %.4f' % (k, res[k]) for k in sorted(want))))
    _check_metrics(res, want, n)
    cnt = pu['cnt'].cpu().numpy()
    for u in range(30):
        mine = rank[(hu == u) & (hy >= 3)]
        assert cnt[u, 0] == len(mine) and cnt[u, 1] == (mine.min() if len(mine) else -1)
    # every link relevant: another restatement, the same ranks
    res_all = rank_eval(model, ds, HeldOut.from_links(ds, hu, hv), ks=ks)
    assert torch.equal(res_all['per_user']['rank'], pu['rank'])
    _check_metrics(res_all, *_numpy_metrics(rank, hu, ks))
    # no cap binds: passes of 7 users give the same ranks and the same metrics, to the bit
    stats7 = {}
    res7 = rank_eval(model, ds, heldout, ks=ks, users_per_pass=7, stats=stats7)
    assert stats7['passes'] == 5 and stats7['candidates'] == stats['candidates']
    assert torch.equal(res7['per_user']['rank'], pu['rank'])
    assert torch.equal(res7['per_user']['cnt'], pu['cnt']) and torch.equal(res7['per_user']['dcg'], pu['dcg'])
    assert all(res7[k] == res[k] for k in want) and res7['users_evaluated'] == res['users_evaluated']
    # the items with rank < 10 are exactly the columns of recommend() for that user, at column = rank
    items = recommend(model, ds, n=10)[0].cpu().numpy()
    for u, v, r in zip(hu, hv, rank):
        if r < 10:
            assert items[u, r] == v
        else:
            assert v not in items[u].tolist()
    # restricted to some users: their ranks, means over them alone
    some = np.array([3, 29, 11, 3], np.int32)
    res_some = rank_eval(model, ds, heldout, ks=ks, users=some)
    in_some = np.isin(hu, some)
    assert np.array_equal(res_some['per_user']['users'].cpu().numpy(), [3, 11, 29])
    assert np.array_equal(res_some['per_user']['rank'].cpu().numpy(), rank[in_some])
    assert np.array_equal(res_some['per_user']['index'].cpu().numpy(), np.nonzero(in_some)[0])
    _check_metrics(res_some, *_numpy_metrics(rank[in_some], hu[in_some], ks, (hy >= 3)[in_some]))
    # a held-out link that was also left in the training graph is no candidate: reported, and left out of the metrics
    k = 17
    A2 = At.tolil()
    A2[hu[k], hv[k]] = hy[k]
    A2 = ssp.csr_matrix(A2)
    tu2, tv2 = A2.nonzero()
    ds2 = MyDynamicDataset('data/t/rk_s2', A2, (tu2, tv2), np.asarray(A2[tu2, tv2]).ravel().astype(np.int64) - 1, 1, 1.0, None,
                           None, None, small['cv'], seed=1)
    stats2 = {}
    res2 = rank_eval(model, ds2, HeldOut.from_links(ds2, hu, hv), ks=ks, stats=stats2)
    assert stats2['not_candidates'] == 1 and stats2['queries'] == 70 and stats2['candidates'] == stats['candidates'] - 1
    cands2 = CandidateLinks.for_users(ds2, np.arange(30))
    R2 = score_candidates(model, cands2, 50).cpu().numpy()
    rank2, pos2 = _numpy_ranks(R2, cands2.link_v[:len(cands2)].cpu().numpy(), cands2.offsets.cpu().numpy(),
                               {u: u for u in range(30)}, hu, hv)
    assert rank2[k] == -1 and (np.delete(rank2, k) >= 0).all()
    assert np.array_equal(res2['per_user']['rank'].cpu().numpy(), rank2)
    assert np.array_equal(res2['per_user']['pos'].cpu().numpy(), pos2)
    assert res2['per_user']['cnt'][hu[k], 0].item() == (hu == hu[k]).sum() - 1
    _check_metrics(res2, *_numpy_metrics(rank2, hu, ks))


def test_ranks_agree_with_the_cpu_oracle(small):
    """Every device rank lies in [#{s > q + 2 tol}, #{s >= q - 2 tol} - 1] of the oracle's segment -- an interval computed
    from the oracle alone, exact as long as every device score is within tol of the oracle's -- and the interval is a
    single point for at least 65 of the 70 queries (the oracle on the CPU: 69 of 70, largest width 1, no exact ties, scores
    between 0.083 and 0.252)."""
    from igmc_amd.rank_eval import HeldOut, rank_eval
    from igmc_amd.recommend import CandidateLinks, score_candidates
    from oracle import extract_ref as X
    from oracle import pyg_ref
    ds, model, ref, hu, hv, At, cv = (small[k] for k in ('ds', 'model', 'ref', 'hu', 'hv', 'A', 'cv'))
    res = rank_eval(model, ds, HeldOut.from_links(ds, hu, hv), ks=(10,))
    rank = res['per_user']['rank'].cpu().numpy()
    cands = CandidateLinks.for_users(ds, np.arange(30))
    cu, cv_items = cands.link_u[:len(cands)].cpu().numpy(), cands.link_v[:len(cands)].cpu().numpy()
    off = cands.offsets.cpu().numpy()
    Acsc = At.tocsc()
    datas = [X.extract((int(u), int(v)), At, Acsc, 1, 1.0, None, cv, 0) for u, v in zip(cu, cv_items)]
    _, out = pyg_ref.eval_sse(ref, pyg_ref.Batch.from_data_list(datas))
    oracle = out.detach().numpy().astype(np.float64).ravel()
    assert np.isfinite(oracle).all()
    tol = PC.OUT_TOL * np.abs(oracle).max()
    dev = score_candidates(model, cands, 50).cpu().numpy().astype(np.float64)
    worst = np.abs(dev - oracle).max()
    single, widest = 0, 0
    for i, (u, v) in enumerate(zip(hu, hv)):
        seg = oracle[off[u]:off[u + 1]]
        p = np.searchsorted(cv_items[off[u]:off[u + 1]], v)
        assert cv_items[off[u] + p] == v
        q = seg[p]
        lo, hi = int((seg > q + 2 * tol).sum()), int((seg >= q - 2 * tol).sum()) - 1
        assert lo <= rank[i] <= hi, (u, v, rank[i], lo, hi)
        single += lo == hi
        widest = max(widest, hi - lo)
    print('oracle: worst |score - oracle| = %.3e (tolerance %.3e, peak %.3f, scores %.3f..%.3f); rank interval a single '
          'point for %d of %d queries, largest width %d' % (worst, tol, np.abs(oracle).max(), oracle.min(), oracle.max(),
                                                             single, len(hu), widest))
    assert worst <= tol
    assert single >= 65


def test_dgcnn_rs_ranks_are_the_lexsort_of_its_own_scores():
    import torch
    from igmc_amd import preprocessing
    from igmc_amd.models import DGCNN_RS
    from igmc_amd.rank_eval import HeldOut, rank_eval
    from igmc_amd.recommend import score_candidates
    from igmc_amd.util_functions import MyDynamicDataset
    (_, _, adj, trl, tru, trv, _, _, _, tel, teu, tev, cv) = preprocessing.load_data_monti('flixster', testing=True)
    ds = MyDynamicDataset('data/t/rk_d', adj, (tru, trv), trl, 1, 1.0, 40, None, None, cv, seed=2)
    torch.manual_seed(4)
    model = DGCNN_RS(ds, latent_dim=[32, 32, 32, 1], k=30, num_relations=len(cv), num_bases=4, regression=True,
                     adj_dropout=0.2, seed=1).to('cuda')
    model.reset_parameters()
    model.eval()
    users = np.random.default_rng(3).permutation(np.unique(teu))[:5].astype(np.int32)
    teu, tev = np.asarray(teu), np.asarray(tev)
    stats = {}
    res = rank_eval(model, ds, HeldOut.from_links(ds, teu, tev), ks=(5, 10), users=users, stats=stats)
    cands = ds._recommend_links
    assert getattr(cands, '_scoregraph', None) is None          # the sort-pool family: score_links' eager path
    assert stats['users'] == 5 and stats['passes'] == 1 and stats['candidates'] == len(cands)
    mine = np.isin(teu, users)
    order = np.lexsort((tev[mine], teu[mine]))
    hu, hv = teu[mine][order], tev[mine][order]
    assert stats['queries'] == len(hu)
    R = score_candidates(model, cands, 50).cpu().numpy()
    seg_users = cands.users.cpu().numpy()
    rank, pos = _numpy_ranks(R, cands.link_v[:len(cands)].cpu().numpy(), cands.offsets.cpu().numpy(),
                             {int(u): s for s, u in enumerate(seg_users)}, hu, hv)
    assert np.array_equal(res['per_user']['rank'].cpu().numpy(), rank)
    assert np.array_equal(res['per_user']['pos'].cpu().numpy(), pos)
    assert stats['not_candidates'] == int((rank < 0).sum())
    _check_metrics(res, *_numpy_metrics(rank, hu, (5, 10)))


def test_main_rank_eval_end_to_end(tmp_path):
    """``Main.py ... --epochs 1 --max-train-num 2000`` and then the same command with ``--no-train --rank-eval 5,10
    --recommend-users 50``."""
    cmd = [sys.executable, os.path.join(ROOT, 'Main.py'), '--data-name', 'douban', '--epochs', '1', '--testing',
           '--save-interval', '1', '--dynamic-train', '--dynamic-test', '--max-train-num', '2000', '--max-nodes-per-hop', '100']
    env = dict(os.environ, PYTHONPATH=ROOT)
    tsv = tmp_path / 'results' / 'douban_testmode' / 'ranking_douban.tsv'
    for extra in ([], ['--no-train', '--rank-eval', '5,10', '--recommend-users', '50']):
        r = subprocess.run(cmd + extra, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=600)
        out = r.stdout.decode()
        assert r.returncode == 0, out[-3000:]
        assert tsv.exists() == bool(extra)          # without the flag nothing changes
    line = [l for l in out.splitlines() if l.startswith('Ranked ')]
    assert len(line) == 1 and 'candidates/s' in line[0] and 'held-out links of' in line[0] and 'hr@5' in line[0]
    assert 'Test rmse is' not in out
    print(line[0])
    rec = dict(l.split('\t') for l in tsv.read_text().splitlines())
    assert list(rec) == ['hr@5', 'recall@5', 'precision@5', 'ndcg@5', 'hr@10', 'recall@10', 'precision@10', 'ndcg@10', 'mrr']
    val = {k: float(v) for k, v in rec.items()}
    assert all(0.0 <= v <= 1.0 for v in val.values()), val
    assert val['hr@5'] <= val['hr@10'] and val['recall@5'] <= val['recall@10']
    assert not (tmp_path / 'results' / 'douban_testmode' / 'recommendations_douban.tsv').exists()
