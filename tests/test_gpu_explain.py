"""Leave-one-out neighbour attribution on a real MI355X (``igmc_amd/explain.py``, ``igmc_amd/csrc/explain.hip``): the kernel
checks of tests/explain_checks.py unchanged, then the pipeline -- variants written on the device score bit for bit like the
same variants built in numpy and uploaded at the same positions, the base score is the pair's prediction, the selection is
the numpy lexsort of the pass's own |delta|, passes do not matter, the deltas agree with the CPU oracle, ``DGCNN_RS``,
``GraphView``, the refusals and ``Main.py --explain`` end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as ssp

import explain_checks as EX
import parity_checks as PC
from helpers import ROOT
from selection_checks import descending_order

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    return PC.GpuBackend()


# ------------------------------------------------------------------ kernel level (the emulator's cases)
def test_every_size_without_a_cap_and_without_dense_blocks(be):
    EX.check_sizes_covered(be)


@pytest.mark.parametrize('lean', [False, True])
@pytest.mark.parametrize('B', [1, 7, 50])
def test_arena_with_dense_blocks(be, lean, B):
    EX.check_case(be, 1, 100, lean, B, first=3 if B == 1 else 0, want_dense=True)


@pytest.mark.parametrize('B', [1, 7])
def test_arena_without_dense_blocks(be, B):
    EX.check_case(be, 1, None, False, B, first=6 if B == 1 else 0, want_dense=False)


@pytest.mark.parametrize('B', [7, 50])
def test_two_hops_under_a_cap_that_binds(be, B):
    lists, want = EX.check_case(be, 2, 10, True, B, want_dense=True)
    assert max(len(U) for U, _, _, _ in lists) == 21 and max(ul.max() for _, ul, _, _ in lists) == 4
    removed = want['var_side'] != 255
    assert (want['var_rating'][removed] == 0).any() and (want['var_rating'][removed] > 0).any()


def test_capacities_one_short_and_bad_offsets(be):
    EX.check_capacities(be)


def test_fill_does_not_depend_on_the_grid(be):
    EX.check_grid(be)


def test_deltas_against_numpy(be):
    EX.check_deltas(be)


# ------------------------------------------------------------------ pipeline
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


@pytest.fixture(scope='module')
def douban():
    from igmc_amd import preprocessing
    return preprocessing.load_data_monti('douban', testing=True)


def _train_set(douban, cap, tag):
    from igmc_amd.util_functions import MyDynamicDataset
    (_, _, adj, trl, tru, trv, _, _, _, _, _, _, cv) = douban
    return MyDynamicDataset('data/t/exp_' + tag, adj, (tru, trv), trl, 1, 1.0, cap, None, None, cv, seed=2)


def _some_pairs(adj, k, seed=0):
    """k pairs of the rating graph: the users with the most and the fewest ratings among them, the (fewest ratings, fewest
    raters) pair first; every other pair a rated one and an arbitrary one in turn."""
    A = ssp.csr_matrix(adj)
    deg_u, deg_v = np.diff(A.indptr), np.diff(A.tocsc().indptr)
    rng = np.random.default_rng(seed)
    users = [int(np.argmin(deg_u)), int(np.argmax(deg_u))] + rng.permutation(A.shape[0])[:k - 2].tolist()
    items = [int(np.argmin(deg_v))]
    for i, u in enumerate(users[1:]):
        row = A.indices[A.indptr[u]:A.indptr[u + 1]]
        items.append(int(row[rng.integers(len(row))]) if (i % 2 == 0 and len(row)) else int(rng.integers(A.shape[1])))
    return np.asarray(users, np.int32), np.asarray(items, np.int32)


def _host_built(ds, A, u, v):
    """The variants of the pairs built in numpy from the DOWNLOADED base extraction (scoring key, position = index in the list)
    and uploaded into a LeaveOneOutLinks of their own at the same positions: (that object, the numpy arrays, the node lists)."""
    import torch
    from igmc_amd.explain import LeaveOneOutLinks
    from igmc_amd.recommend import CandidateLinks
    from igmc_amd.train_eval import SCORE_EPOCH
    cands = CandidateLinks.from_pairs(ds, u, v)
    db = cands.extract(None, 0, len(u), epoch=SCORE_EPOCH, slot='host', max_graphs=len(u))
    lists = EX.node_lists(db.arena.download(torch.cuda.current_stream().cuda_stream))
    want = EX.reference_variants(lists, A)
    host = LeaveOneOutLinks(ds)
    for k in EX.CACHE_KEYS:
        host._cache_t[k][:len(want[k])].copy_(torch.from_numpy(want[k]))
    host._close_tail(len(want['var_link']), len(want['unodes']), len(want['vnodes']))
    return host, want, lists


def _expect_selection(res, m):
    """nodes / sides / ratings / deltas / counts by THE ORDER (selection_checks.descending_order) of every link's own |delta|."""
    r = {k: t.cpu().numpy() for k, t in res.items()}
    n = len(r['base'])
    N, S, Rt = np.full((n, m), -1, np.int32), np.full((n, m), 255, np.uint8), np.zeros((n, m), np.uint8)
    D, C = np.zeros((n, m), np.float32), np.zeros(n, np.int32)
    for i in range(n):
        lo, hi = int(r['seg_off'][i]), int(r['seg_off'][i + 1])
        idx = np.arange(lo, hi)
        order = idx[descending_order(np.abs(r['delta'][lo:hi]), idx)[:m]]
        c = len(order)
        var = order + i + 1
        assert (r['var_link'][var] == i).all()
        N[i, :c], S[i, :c], Rt[i, :c], D[i, :c], C[i] = r['var_node'][var], r['var_side'][var], r['var_rating'][var], r['delta'][order], c
    return dict(nodes=N, sides=S, ratings=Rt, deltas=D, counts=C, base=r['base'])


def _assert_selection(out, want):
    for k, w in want.items():
        g = out[k].cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, k
        assert g.tobytes() == w.tobytes(), k


@pytest.mark.parametrize('cap', [40, 10000])
def test_variants_score_like_the_same_variants_built_on_the_host(douban, cap):
    """cap 40: sampling binds on the busy pairs; cap 10000: no cap binds.  Bit-identity of the variant scores, the base score
    against the pair's prediction, and the selection -- on one set of about 20 pairs."""
    import torch
    from igmc_amd.explain import explain, explain_all
    from igmc_amd.recommend import CandidateLinks, score_candidates
    adj, cv = douban[2], douban[12]
    ds = _train_set(douban, cap, 'a%d' % cap)
    model = _igmc(ds, len(cv))
    u, v = _some_pairs(adj, 20)
    stats = {}
    res = explain_all(model, ds, u, v, stats=stats)
    nvar = res['scores'].numel()
    assert stats == dict(links=20, variants=nvar, attributions=nvar - 20, passes=1)
    if nvar // 50 >= 8:
        # a pass of n steps replays a captured pair of groups once n - 1 >= 2 M (its first step runs eagerly, stepgraph.steps):
        # the 35 steps of the uncapped pairs do (M = 17), the 26 steps at cap 40 (M = 13) are one short
        sg = ds._explain_links._scoregraph
        print('cap %d: %d variants, groups of %d steps, captured: %s' % (cap, nvar, sg.M, sg.graph is not None))
        if nvar // 50 - 1 >= 2 * sg.M:
            assert sg.graph is not None
        assert cap == 40 or sg.graph is not None
    host, want, lists = _host_built(ds, ssp.csr_matrix(adj), u, v)
    assert nvar == len(want['var_link'])
    for k in EX.VAR_KEYS:
        assert np.array_equal(res[k].cpu().numpy(), want[k]), k
    assert np.array_equal(res['var_off'].cpu().numpy(), EX.prefix([len(U) + len(V) - 1 for U, _, V, _ in lists]))
    assert np.array_equal(res['seg_off'].cpu().numpy(), res['var_off'].cpu().numpy() - np.arange(21))
    ref = score_candidates(model, host, 50)
    print('cap %d: %d pairs, %d variants, sizes %s: max |device-built - host-built| = %g' % (
        cap, len(u), nvar, [(len(U), len(V)) for U, _, V, _ in lists][:4], (res['scores'] - ref).abs().max().item()))
    assert res['scores'].dtype == torch.float32 and res['scores'].is_cuda and torch.equal(res['scores'], ref)
    if cap == 40:
        assert max(max(len(U), len(V)) for U, _, V, _ in lists) == 41          # the cap binds
    # delta = score - base, in float32, for every attribution
    s, off = res['scores'].cpu().numpy(), res['var_off'].cpu().numpy()
    assert res['base'].cpu().numpy().tobytes() == s[off[:-1]].tobytes()
    wd = np.concatenate([s[off[i] + 1:off[i + 1]] - s[off[i]] for i in range(20)]).astype(np.float32)
    assert res['delta'].cpu().numpy().tobytes() == wd.tobytes()
    # the base variant is the pair's own subgraph through the cached extraction: its score is the pair's prediction
    pred = score_candidates(model, CandidateLinks.from_pairs(ds, u, v), 50)
    tol = PC.OUT_TOL * pred.abs().max().item()
    worst = (res['base'] - pred).abs().max().item()
    print('base variant against the prediction of the pair: worst |difference| = %.3e (tolerance %.3e)' % (worst, tol))
    assert worst <= tol
    # the selection: numpy's lexsort of the pass's own |delta| bits
    out = explain(model, ds, u, v, m=5)
    assert all(t.is_cuda for t in out.values()) and out['nodes'].dtype == torch.int32 and out['counts'].dtype == torch.int32
    _assert_selection(out, _expect_selection(res, 5))
    out = explain(model, ds, u, v, m=64)
    exp = _expect_selection(res, 64)
    _assert_selection(out, exp)
    short = exp['counts'] < 64
    assert short.any() and (exp['nodes'][short, -1] == -1).all() and (exp['deltas'][short, -1] == 0).all()


def test_results_do_not_depend_on_the_passes(douban):
    import torch
    from igmc_amd.explain import explain, explain_all
    adj, cv = douban[2], douban[12]
    ds = _train_set(douban, 10000, 'b')
    model = _igmc(ds, len(cv))
    u, v = _some_pairs(adj, 7, seed=1)
    one, one_all = explain(model, ds, u, v, m=5), explain_all(model, ds, u, v)
    for lpp in (1, 3):
        stats = {}
        many = explain(model, ds, u, v, m=5, links_per_pass=lpp, stats=stats)
        assert stats['passes'] == -(-7 // lpp)
        for k in one:
            assert torch.equal(one[k], many[k]), (lpp, k)
        many_all = explain_all(model, ds, u, v, links_per_pass=lpp)
        for k in one_all:
            assert torch.equal(one_all[k], many_all[k]), (lpp, k)
    with pytest.raises(ValueError, match='do not fit'):
        explain(model, ds, u, v, capacity_variants=8)


def test_deltas_agree_with_the_cpu_oracle():
    """The 30 x 40 graph of the recommendation test's oracle case: every rated link of six users, every neighbour.  The
    oracle's own deltas stand far outside the tolerance (largest |delta| of a link: 0.0096 or more against a tolerance of 1e-5,
    see tests/test_emu_explain.py), so the reference parameters are used unscaled."""
    import torch
    from igmc_amd.explain import explain, explain_all
    from igmc_amd.util_functions import MyDynamicDataset
    A, cv, rows, cols = EX.oracle_graph()
    labels = np.asarray(A[rows, cols]).ravel().astype(np.int64) - 1
    ds = MyDynamicDataset('data/t/exp_o', A, (rows, cols), labels, 1, 1.0, None, None, None, cv, seed=1)
    model = _igmc(ds, 5)
    ref = PC.make_ref_model(4, 5, seed=6)
    ref.eval()
    ws = model._workspace(ds.extract(None, 0, 1))
    model.flat_parameters().data.copy_(torch.from_numpy(PC.flatten_params(ws, ref)).cuda())
    pairs = EX.oracle_pairs(A, rows, cols)
    oracle = EX.oracle_deltas(ref, A, cv, pairs)
    m = 5
    res = {k: t.cpu().numpy() for k, t in explain_all(model, ds, pairs[:, 0], pairs[:, 1]).items()}
    out = {k: t.cpu().numpy() for k, t in explain(model, ds, pairs[:, 0], pairs[:, 1], m=m).items()}
    peak = max(abs(b) for b, _ in oracle)
    tol = 2 * PC.OUT_TOL * peak
    worst, worst_base, seen = 0.0, 0.0, 0
    for i, (b, deltas) in enumerate(oracle):                      # no link is left out
        worst_base = max(worst_base, abs(float(res['base'][i]) - b))
        assert abs(float(res['base'][i]) - b) <= PC.OUT_TOL * peak
        lo, hi = int(res['seg_off'][i]), int(res['seg_off'][i + 1])
        var = np.arange(lo, hi) + i + 1
        got = {(int(s), int(nd)): float(d) for s, nd, d in zip(res['var_side'][var], res['var_node'][var], res['delta'][lo:hi])}
        assert set(got) == set(deltas) and len(got) == hi - lo      # ... and no neighbour
        for key, d in deltas.items():
            worst = max(worst, abs(got[key] - d))
            assert abs(got[key] - d) <= tol, (i, key, got[key], d)
        seen += len(got)
        c = min(m, len(deltas))
        assert out['counts'][i] == c
        nth = np.sort(np.abs(list(deltas.values())))[::-1][c - 1] if c else 0.0
        for r in range(c):
            key = (int(out['sides'][i, r]), int(out['nodes'][i, r]))
            assert abs(deltas[key]) >= nth - tol, (i, r, key, deltas[key], nth)
    print('oracle: %d links, %d neighbours: worst |delta - oracle| = %.3e (tolerance %.3e), worst |base - oracle| = %.3e, peak %.3f' % (
        len(oracle), seen, worst, tol, worst_base, peak))


def test_dgcnn_rs_variants_score_like_the_host_built_cache():
    import torch
    from igmc_amd import preprocessing
    from igmc_amd.explain import explain_all
    from igmc_amd.models import DGCNN_RS
    from igmc_amd.recommend import score_candidates
    from igmc_amd.util_functions import MyDynamicDataset
    (_, _, adj, trl, tru, trv, _, _, _, _, _, _, cv) = preprocessing.load_data_monti('flixster', testing=True)
    ds = MyDynamicDataset('data/t/exp_d', adj, (tru, trv), trl, 1, 1.0, 40, None, None, cv, seed=2)
    model = _igmc(ds, len(cv), cls=DGCNN_RS)
    u, v = _some_pairs(adj, 6, seed=3)
    res = explain_all(model, ds, u, v)
    assert getattr(ds._explain_links, '_scoregraph', None) is None          # the sort-pool family: score_links' eager path
    host, want, _ = _host_built(ds, ssp.csr_matrix(adj), u, v)
    assert np.array_equal(res['var_node'].cpu().numpy(), want['var_node'])
    assert torch.equal(res['scores'], score_candidates(model, host, 50))


def test_graph_view_explains_a_brand_new_user(douban):
    import torch
    from igmc_amd.explain import explain
    from igmc_amd.recommend import GraphView
    from igmc_amd.util_functions import MyDynamicDataset
    (_, _, adj, trl, tru, trv, _, _, _, _, _, _, cv) = douban
    ds = _train_set(douban, 40, 'g')
    model = _igmc(ds, len(cv))
    A = ssp.lil_matrix(ssp.csr_matrix(adj))
    new = A.shape[0]
    items = np.asarray([3, 17, 256, 1000, 2999], np.int32)
    ratings = np.asarray([5, 1, 3, 4, 2], np.uint8)
    view = GraphView(ds, ds.graph.updated(np.full(5, new, np.int32), items, ratings))
    A.resize((new + 1, A.shape[1]))
    A[new, items] = ratings
    u, v = np.asarray([new, new, 5], np.int32), np.asarray([812, 17, 3], np.int32)
    got = explain(model, view, u, v, m=4)
    rebuilt = MyDynamicDataset('data/t/exp_g2', ssp.csr_matrix(A), (tru, trv), trl, 1, 1.0, 40, None, None, cv, seed=2)
    want = explain(model, rebuilt, u, v, m=4)
    for k in got:
        assert torch.equal(got[k], want[k]), k
    # the new user's neighbours in the first link are the items just rated (and nobody rated 812 with them... or did)
    sides, nodes = got['sides'][0].cpu().numpy(), got['nodes'][0].cpu().numpy()
    assert set(nodes[sides == 1].tolist()) <= set(items.tolist()) and int(got['counts'][0]) == 4
    with pytest.raises(ValueError):
        explain(model, ds, u, v)                                  # the old graph has no such user


def test_refusals(douban):
    from igmc_amd.explain import LeaveOneOutLinks, explain
    ds = _train_set(douban, 40, 'r')
    model = _igmc(ds, len(douban[12]))

    class _WithFeatures(object):
        u_features, v_features, _side = np.zeros((1, 1)), np.zeros((1, 1)), None
    with pytest.raises(NotImplementedError, match='--use-features'):
        LeaveOneOutLinks(_WithFeatures(), 10, 10)
    with pytest.raises(NotImplementedError, match='--use-features'):
        explain(model, _WithFeatures(), [0], [0])
    with pytest.raises(ValueError, match='outside the rating graph'):
        explain(model, ds, [0], [ds.graph.n_items])
    with pytest.raises(ValueError, match='outside the rating graph'):
        explain(model, ds, [-1], [0])
    with pytest.raises(ValueError):
        explain(model, ds, [0], [0], m=65)


def test_main_explain_end_to_end(tmp_path):
    """``Main.py ... --epochs 1`` (the checkpoint), then ``--no-train --explain 3 --explain-links FILE`` and ``--no-train
    --recommend 2 --explain 2``, each a fresh child process under a time limit."""
    cmd = [sys.executable, os.path.join(ROOT, 'Main.py'), '--data-name', 'douban', '--epochs', '1', '--testing',
           '--save-interval', '1', '--dynamic-train', '--max-train-num', '2000', '--max-test-num', '700',
           '--max-nodes-per-hop', '100']
    env = dict(os.environ, PYTHONPATH=ROOT)
    links = tmp_path / 'links.txt'
    links.write_text('# user item\n0 5\n7 812   # a comment\n\n2999 0\n')
    tsv = tmp_path / 'results' / 'douban_testmode' / 'explanations_douban.tsv'
    header = 'user\titem\tscore\tplace\tside\tnode\trating\tdelta\tscore_without'

    def run(extra):
        r = subprocess.run(cmd + extra, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        out = r.stdout.decode()
        assert r.returncode == 0, out[-3000:]
        return out

    def blocks(per_link):
        lines = tsv.read_text().splitlines()
        assert lines[0] == header
        rec = [l.split('\t') for l in lines[1:]]
        assert all(len(x) == 9 for x in rec)
        out = {}
        for x in rec:
            out.setdefault((int(x[0]), int(x[1])), []).append(x)
        for (u, v), rows in out.items():
            if rows[0][3] == '0':          # a link without neighbours: one line, nothing to rank
                assert len(rows) == 1 and rows[0][4:7] == ['-', '-', '-'] and float(rows[0][7]) == 0
                continue
            assert 1 <= len(rows) <= per_link and [int(x[3]) for x in rows] == list(range(1, len(rows) + 1))
            d = [abs(float(x[7])) for x in rows]
            assert all(a >= b for a, b in zip(d, d[1:]))
            for x in rows:
                assert x[4] in ('user', 'item') and int(x[5]) >= 0 and (x[6] == '-' or float(x[6]) in (1, 2, 3, 4, 5))
                assert abs(float(x[2]) + float(x[7]) - float(x[8])) < 2e-6
        return out

    run([])
    assert not tsv.exists()
    out = run(['--no-train', '--explain', '3', '--explain-links', str(links)])
    assert 'Test rmse is' not in out and 'Explained 3 links' in out
    assert list(blocks(3)) == [(0, 5), (7, 812), (2999, 0)]
    out = run(['--no-train', '--recommend', '2', '--recommend-users', '4', '--explain', '2'])
    assert 'Explained 8 links' in out
    rec = [l.split('\t') for l in (tmp_path / 'results' / 'douban_testmode' / 'recommendations_douban.tsv').read_text().splitlines()]
    assert list(blocks(2)) == [(int(x[0]), int(x[2])) for x in rec]
