"""Top-N recommendation on a real MI355X (``igmc_amd/recommend.py``, ``igmc_amd/csrc/candidates.hip``): candidate links
enumerated on the device score bit for bit like the same links uploaded from the host, the ranked lists are the numpy
lexsort of those scores (``selection_checks.descending_order``), passes replay one captured graph, the lists agree with the
CPU oracle, and ``Main.py --recommend`` end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as ssp

import parity_checks as PC
from helpers import ROOT, random_rating_graph
from selection_checks import descending_order

pytestmark = pytest.mark.gpu


def _igmc(ds, R, seed=4, cls=None):
    import torch
    from igmc_amd.models import IGMC
    torch.manual_seed(seed)
    if cls is None:
        model = IGMC(ds, latent_dim=[32, 32, 32, 32], num_relations=R, num_bases=4, regression=True, adj_dropout=0.2,
                     seed=3).to('cuda')
    else:
        model = cls(ds, latent_dim=[32, 32, 32, 1], k=30, num_relations=R, num_bases=4, regression=True, adj_dropout=0.2,
                    seed=1).to('cuda')
    model.reset_parameters()
    model.eval()
    return model


def _complement(adj, users, item_mask=None, exclude_seen=True):
    """The candidate list on the host: (u, v, offsets), users in the order given, item ascending."""
    A = ssp.csr_matrix(adj)
    us, vs, off = [], [], [0]
    for u in users:
        keep = np.ones(A.shape[1], bool) if item_mask is None else np.asarray(item_mask) != 0
        if exclude_seen:
            lo, hi = A.indptr[u], A.indptr[u + 1]
            keep[A.indices[lo:hi][A.data[lo:hi] != 0]] = False
        v = np.nonzero(keep)[0]
        us.append(np.full(len(v), u, np.int64))
        vs.append(v.astype(np.int64))
        off.append(off[-1] + len(v))
    return np.concatenate(us), np.concatenate(vs), np.asarray(off, np.int64)


def _expect_lists(scores, items, off, n):
    """Per segment THE ORDER (selection_checks.descending_order): (items [nq, n], scores [nq, n], counts)."""
    nq = len(off) - 1
    I, S, C = np.full((nq, n), -1, np.int32), np.zeros((nq, n), np.float32), np.zeros(nq, np.int32)
    for q in range(nq):
        k = scores[off[q]:off[q + 1]]
        idx = np.arange(off[q], off[q + 1])
        order = descending_order(k, idx)[:n]
        c = len(order)
        I[q, :c], S[q, :c], C[q] = items[idx[order]], k[order], c
    return I, S, C


@pytest.fixture(scope='module')
def douban():
    from igmc_amd import preprocessing
    return preprocessing.load_data_monti('douban', testing=True)


def _train_set(douban, cap, tag):
    from igmc_amd.util_functions import MyDynamicDataset
    (_, _, adj, trl, tru, trv, _, _, _, _, _, _, cv) = douban
    return MyDynamicDataset('data/t/rec_' + tag, adj, (tru, trv), trl, 1, 1.0, cap, None, None, cv, seed=2)


def _some_users(adj, k, seed=0):
    """k users of the rating graph, the ones with the most and the fewest training ratings among them."""
    deg = np.diff(ssp.csr_matrix(adj).indptr)
    rng = np.random.default_rng(seed)
    rest = rng.permutation(len(deg))[:k - 2].tolist()
    return np.asarray([int(np.argmax(deg)), int(np.argmin(deg))] + rest, np.int32)


def test_candidates_score_like_the_same_links_built_on_the_host_and_the_lists_are_their_lexsort(douban):
    import torch
    from igmc_amd.recommend import CandidateLinks, recommend, score_candidates
    from igmc_amd.train_eval import score_links
    from igmc_amd.util_functions import MyDynamicDataset
    adj, cv = douban[2], douban[12]
    ds = _train_set(douban, 40, 'a')          # cap 40: sampling binds, the position of a link in its pass matters
    model = _igmc(ds, len(cv))
    users = _some_users(adj, 40)
    hu, hv, off = _complement(adj, users)
    cands = CandidateLinks.for_users(ds, users)
    assert len(cands) == len(hu) and np.array_equal(cands.offsets.cpu().numpy(), off)
    assert np.array_equal(cands.link_u[:len(cands)].cpu().numpy(), hu) and np.array_equal(cands.link_v[:len(cands)].cpu().numpy(), hv)
    assert not bool(cands.link_y.any())
    R = score_candidates(model, cands, 50)
    assert cands._scoregraph.graph is not None          # thousands of batches of 50: the pass replayed a captured graph
    host = MyDynamicDataset('data/t/rec_a_host', adj, (hu, hv), np.zeros(len(hu), np.int64), 1, 1.0, 40, None, None, cv, seed=2)
    want, _, _ = score_links(model, host, 50)
    print('%d users, %d candidates: max |device-enumerated - host-built| = %g' % (
        len(users), len(hu), (R - want).abs().max().item()))
    assert R.dtype == torch.float32 and R.is_cuda and torch.equal(R, want)
    # recommend() in one pass: the same list at the same positions -> the numpy lexsort of those scores, items and score bits
    stats = {}
    items, scores, counts = recommend(model, ds, users=users, n=10, stats=stats)
    assert stats == dict(users=len(users), candidates=len(hu), passes=1)
    assert items.is_cuda and scores.is_cuda and counts.is_cuda and items.dtype == torch.int32 and counts.dtype == torch.int32
    I, S, C = _expect_lists(want.cpu().numpy(), hv, off, 10)
    assert np.array_equal(counts.cpu().numpy(), C) and np.array_equal(items.cpu().numpy(), I)
    assert scores.cpu().numpy().tobytes() == S.tobytes()
    assert ds._recommend_links._scoregraph.graph is not None
    # no recommended item is in the user's training row
    A = ssp.csr_matrix(adj)
    for u, row in zip(users, items.cpu().numpy()):
        assert not set(row.tolist()) & set(A.indices[A.indptr[u]:A.indptr[u + 1]].tolist())


def test_passes_are_independent_where_no_cap_binds_and_replay_one_graph(douban):
    import torch
    from igmc_amd.recommend import recommend
    adj, cv = douban[2], douban[12]
    ds = _train_set(douban, 10000, 'b')
    model = _igmc(ds, len(cv))
    users = _some_users(adj, 12, seed=1)
    one = recommend(model, ds, users=users, n=10)
    cands = ds._recommend_links
    sg, graph = cands._scoregraph, cands._scoregraph.graph
    assert graph is not None
    stats = {}
    many = recommend(model, ds, users=users, n=10, users_per_pass=5, stats=stats)
    assert stats['passes'] == 3
    for a, b in zip(one, many):
        assert torch.equal(a, b)
    assert ds._recommend_links is cands and cands._scoregraph is sg and sg.graph is graph      # nothing was captured again


def test_lists_agree_with_the_cpu_oracle():
    import torch
    from igmc_amd.recommend import recommend
    from igmc_amd.util_functions import MyDynamicDataset
    from oracle import extract_ref as X
    from oracle import pyg_ref
    A = random_rating_graph(30, 40, 0.3, 5, 21)
    A.eliminate_zeros()
    cv = np.arange(1, 6, dtype=np.float64)
    rows, cols = A.nonzero()
    labels = np.asarray(A[rows, cols]).ravel().astype(np.int64) - 1
    ds = MyDynamicDataset('data/t/rec_o', A, (rows, cols), labels, 1, 1.0, None, None, None, cv, seed=1)
    model = _igmc(ds, 5)
    ref = PC.make_ref_model(4, 5, seed=6)
    ref.eval()
    ws = model._workspace(ds.extract(None, 0, 1))
    model.flat_parameters().data.copy_(torch.from_numpy(PC.flatten_params(ws, ref)).cuda())
    n = 5
    items, scores, counts = [t.cpu().numpy() for t in recommend(model, ds, n=n)]
    assert items.shape == (30, n) and counts.shape == (30,)
    # the oracle's score of every candidate: no cap, so the extraction draws nothing
    hu, hv, off = _complement(A, np.arange(30))
    Acsc = A.tocsc()
    datas = [X.extract((int(u), int(v)), A, Acsc, 1, 1.0, None, cv, 0) for u, v in zip(hu, hv)]
    _, out = pyg_ref.eval_sse(ref, pyg_ref.Batch.from_data_list(datas))
    oracle = out.detach().numpy().astype(np.float64).ravel()
    assert np.isfinite(oracle).all()
    tol = PC.OUT_TOL * np.abs(oracle).max()
    worst = 0.0
    for u in range(30):                                         # no user is left out
        seg = oracle[off[u]:off[u + 1]]
        seg_items = hv[off[u]:off[u + 1]]
        c = min(n, len(seg))
        assert counts[u] == c and c > 0
        assert (items[u, c:] == -1).all()
        nth = np.sort(seg)[::-1][c - 1]
        assert len(set(items[u, :c].tolist())) == c
        for r in range(c):
            pos = np.searchsorted(seg_items, items[u, r])
            assert seg_items[pos] == items[u, r], 'user %d: item %d is no candidate' % (u, items[u, r])
            worst = max(worst, abs(float(scores[u, r]) - seg[pos]))
            assert abs(float(scores[u, r]) - seg[pos]) <= tol, (u, r, scores[u, r], seg[pos])
            assert seg[pos] >= nth - tol, (u, r, seg[pos], nth)
    print('oracle: worst |score - oracle| = %.3e (tolerance %.3e, peak %.3f)' % (worst, tol, np.abs(oracle).max()))


def test_masks_seen_items_short_lists_and_arbitrary_pairs(douban):
    import torch
    from igmc_amd.recommend import CandidateLinks, recommend, score_candidates
    from igmc_amd.train_eval import score_links
    from igmc_amd.util_functions import MyDynamicDataset
    (_, _, adj, _, _, _, _, _, _, tel, teu, tev, cv) = douban
    A = ssp.csr_matrix(adj)
    ds = _train_set(douban, 40, 'c')
    model = _igmc(ds, len(cv))
    users = _some_users(adj, 6, seed=2)
    top = int(users[0])                                         # the user with the most training ratings
    # exclude_seen=False: every item is a candidate, rated ones included
    stats = {}
    items, _, counts = recommend(model, ds, users=users, n=64, exclude_seen=False, stats=stats)
    assert stats['candidates'] == len(users) * A.shape[1] and (counts.cpu().numpy() == 64).all()
    cl = CandidateLinks.for_users(ds, [top], exclude_seen=False)
    row = set(A.indices[A.indptr[top]:A.indptr[top + 1]].tolist())
    assert row and row <= set(cl.link_v[:len(cl)].cpu().numpy().tolist())
    # item_mask: candidates come from its items only
    mask = np.zeros(A.shape[1], bool)
    mask[np.random.default_rng(3).permutation(A.shape[1])[:200]] = True
    items, scores, counts = [t.cpu().numpy() for t in recommend(model, ds, users=users, n=10, item_mask=mask)]
    for u, row_items, c in zip(users, items, counts):
        got = row_items[:c]
        assert mask[got].all() and (row_items[c:] == -1).all()
        assert not set(got.tolist()) & set(A.indices[A.indptr[u]:A.indptr[u + 1]].tolist())
    # fewer candidates than n: count < n, -1 / 0 behind it
    few = np.zeros(A.shape[1], bool)
    unseen = np.setdiff1d(np.arange(A.shape[1]), A.indices[A.indptr[top]:A.indptr[top + 1]])[:3]
    few[unseen] = True
    few[A.indices[A.indptr[top]]] = True                        # ... and one item the user rated: no candidate
    items, scores, counts = [t.cpu().numpy() for t in recommend(model, ds, users=[top], n=5, item_mask=few)]
    assert counts.tolist() == [3] and sorted(items[0, :3].tolist()) == unseen.tolist()
    assert items[0, 3:].tolist() == [-1, -1] and scores[0, 3:].tolist() == [0.0, 0.0]
    assert (np.diff(scores[0, :3]) <= 0).all()
    # arbitrary pairs: the first 330 test links score like the test dataset of the same links, bit for bit
    te = MyDynamicDataset('data/t/rec_c_test', adj, (teu[:330], tev[:330]), tel[:330], 1, 1.0, 40, None, None, cv, seed=2)
    want, _, _ = score_links(model, te, 50)
    pairs = CandidateLinks.from_pairs(ds, teu[:330], torch.from_numpy(np.asarray(tev[:330])).cuda())
    assert len(pairs) == 330 and pairs.offsets is None
    assert torch.equal(score_candidates(model, pairs, 50), want)
    with pytest.raises(ValueError):
        CandidateLinks.from_pairs(ds, [0], [A.shape[1]])
    with pytest.raises(RuntimeError, match='user id'):
        CandidateLinks.for_users(ds, [A.shape[0]])

    class _WithFeatures(object):
        u_features, v_features, _side = np.zeros((1, 1)), np.zeros((1, 1)), None
    with pytest.raises(NotImplementedError, match='--use-features'):
        CandidateLinks(_WithFeatures(), 10)


def test_dgcnn_rs_lists_are_the_lexsort_of_its_own_scores():
    from igmc_amd import preprocessing
    from igmc_amd.models import DGCNN_RS
    from igmc_amd.recommend import recommend, score_candidates
    from igmc_amd.util_functions import MyDynamicDataset
    (_, _, adj, trl, tru, trv, _, _, _, _, _, _, cv) = preprocessing.load_data_monti('flixster', testing=True)
    ds = MyDynamicDataset('data/t/rec_d', adj, (tru, trv), trl, 1, 1.0, 40, None, None, cv, seed=2)
    model = _igmc(ds, len(cv), cls=DGCNN_RS)
    users = _some_users(adj, 5, seed=3)
    items, scores, counts = [t.cpu().numpy() for t in recommend(model, ds, users=users, n=10)]
    cands = ds._recommend_links
    assert getattr(cands, '_scoregraph', None) is None          # the sort-pool family: score_links' eager path
    R = score_candidates(model, cands, 50).cpu().numpy()
    I, S, C = _expect_lists(R, cands.link_v[:len(cands)].cpu().numpy(), cands.offsets.cpu().numpy(), 10)
    assert np.array_equal(items, I) and np.array_equal(counts, C) and scores.tobytes() == S.tobytes()


def test_main_recommend_end_to_end(tmp_path):
    """``Main.py ... --epochs 1`` and then the same command with ``--no-train --recommend 5 --recommend-users 20``."""
    from igmc_amd import preprocessing
    cmd = [sys.executable, os.path.join(ROOT, 'Main.py'), '--data-name', 'douban', '--epochs', '1', '--testing',
           '--save-interval', '1', '--dynamic-train', '--max-train-num', '2000', '--max-test-num', '700',
           '--max-nodes-per-hop', '100']
    env = dict(os.environ, PYTHONPATH=ROOT)
    tsv = tmp_path / 'results' / 'douban_testmode' / 'recommendations_douban.tsv'
    for extra in ([], ['--no-train', '--recommend', '5', '--recommend-users', '20']):
        r = subprocess.run(cmd + extra, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=600)
        out = r.stdout.decode()
        assert r.returncode == 0, out[-3000:]
        assert tsv.exists() == bool(extra)
    assert 'Test rmse is' not in out and 'candidates/s' in out
    lines = tsv.read_text().splitlines()
    assert len(lines) == 100
    rec = [l.split('\t') for l in lines]
    A = ssp.csr_matrix(preprocessing.load_data_monti('douban', testing=True)[2])
    for k, u in enumerate(range(20)):
        mine = rec[5 * k:5 * k + 5]
        assert [int(x[0]) for x in mine] == [u] * 5 and [int(x[1]) for x in mine] == [1, 2, 3, 4, 5]
        s = [float(x[3]) for x in mine]
        assert all(a >= b for a, b in zip(s, s[1:]))
        assert all(len(x[3].split('.')[1]) == 6 for x in mine)
        assert not {int(x[2]) for x in mine} & set(A.indices[A.indptr[u]:A.indptr[u + 1]].tolist())
