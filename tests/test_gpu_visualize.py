"""``--visualize`` on a real MI355X: the scoring pass that keeps the per-link predictions on the device
(``train_eval.score_links`` / ``stepgraph.ScoreGraph`` / ``igmc_scores_store``), the device-side selection of the extremes
(``igmc_select_extremes``), ``train_eval.visualize`` against the reference's recorded selection
(``tests/golden/visualize_golden.npz``) and ``Main.py --visualize`` end to end."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as ssp

import parity_checks as PC
from helpers import ROOT

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'visualize_golden.npz')


def _igmc(ds, R, seed=4, cls=None, **kw):
    import torch
    from igmc_amd.models import IGMC
    torch.manual_seed(seed)
    if cls is None:
        model = IGMC(ds, latent_dim=[32, 32, 32, 32], num_relations=R, num_bases=4, regression=True, adj_dropout=0.2,
                     seed=3, **kw).to('cuda')
    else:
        model = cls(ds, latent_dim=[32, 32, 32, 1], k=30, num_relations=R, num_bases=4, regression=True, adj_dropout=0.2,
                    seed=1).to('cuda')
    model.reset_parameters()
    model.eval()
    return model


def _eager_reference(model, ds, B):
    """What the reference's loop collects: ``model(data)`` over ``DataLoader(graphs, B, shuffle=False)``, concatenated."""
    import torch
    from igmc_amd.train_eval import DataLoader
    outs = []
    with torch.no_grad():
        for data in DataLoader(ds, B, shuffle=False):
            outs.append(model(data).clone())
    return torch.cat(outs)


def _check_pass(model, ds, B, expect_graph):
    """score_links == the concatenated eager forwards, bit for bit; Y == the labels; sse_cnt == eval_loss's sums on a fresh
    loader, which returns the same value before and after the scoring pass."""
    import torch
    from igmc_amd.train_eval import DataLoader, eval_loss, score_links
    before = eval_loss(model, DataLoader(ds, B, shuffle=False), 'cuda', regression=True)
    want = _eager_reference(model, ds, B)
    R, Y, acc = score_links(model, ds, B)
    sg = getattr(ds, '_scoregraph', None)
    assert (sg is not None) == expect_graph
    assert R.dtype == torch.float32 and R.shape == (len(ds),) and R.is_cuda and Y.shape == (len(ds),)
    worst = (R - want).abs().max().item()
    print('%s n=%d B=%d graph=%s: max |score_links - eager| = %g' % (type(ds).__name__, len(ds), B, expect_graph, worst))
    assert torch.equal(R, want), worst
    assert torch.equal(Y, ds.link_y)
    sse, cnt = acc.tolist()
    assert cnt == len(ds)
    loader = DataLoader(ds, B, shuffle=False)
    after = eval_loss(model, loader, 'cuda', regression=True)
    eg = getattr(loader, '_evalgraph', None)
    if eg is not None:
        assert torch.equal(eg.acc, acc)                     # the accumulator itself, bit for bit
    assert sse / max(cnt, 1.0) == after == before
    # a second pass replays the captured graph from its first step: same scores
    R2, Y2, acc2 = score_links(model, ds, B)
    assert torch.equal(R2, R) and torch.equal(Y2, Y) and torch.equal(acc2, acc)
    if expect_graph:      # (the first pass of a process starts with an eager step; from the second on whole launches replay)
        assert sg.graph is not None and sg.steps_done >= 2 * (len(ds) // B)
    return R, Y


@pytest.fixture(scope='module')
def douban():
    from igmc_amd import preprocessing
    return preprocessing.load_data_monti('douban', testing=True)


@pytest.fixture(scope='module')
def ml1m():
    from igmc_amd import preprocessing
    return preprocessing.create_trainvaltest_split('ml_1m', 1234, True, verbose=False)


def test_score_links_replayed_pass_with_a_ragged_last_batch(douban, monkeypatch):
    from igmc_amd.util_functions import MyDynamicDataset
    (_, _, adj, _, _, _, _, _, _, tel, teu, tev, cv) = douban
    n = 1230                # 24 full batches + one of 30; cap 40: sampling binds, the pass's sampling key matters
    ds = MyDynamicDataset('data/t/viz_a', adj, (teu[:n], tev[:n]), tel[:n], 1, 1.0, 40, None, None, cv, seed=2)
    model = _igmc(ds, len(cv))
    R, _ = _check_pass(model, ds, 50, expect_graph=True)
    # model.to() re-creates the flat parameter buffer: a pass after it must not replay launches that hold the old address
    import torch
    numel = model.flat_parameters().numel()
    model.to('cuda')
    poison = [torch.full((numel,), float('nan'), device='cuda') for _ in range(8)]      # whoever gets the freed buffer
    from igmc_amd.train_eval import score_links
    R3, _, _ = score_links(model, ds, 50)
    assert torch.equal(R3, R)
    del poison
    # the same with the replayed pipeline switched off: the eager loop, the same bits
    monkeypatch.setenv('IGMC_NO_EVAL_GRAPH', '1')
    ds2 = MyDynamicDataset('data/t/viz_a', adj, (teu[:n], tev[:n]), tel[:n], 1, 1.0, 40, None, None, cv, seed=2)
    R2, _ = _check_pass(model, ds2, 50, expect_graph=False)
    assert torch.equal(R, R2)


def test_score_links_on_a_set_smaller_than_eight_batches(douban):
    from igmc_amd.util_functions import MyDynamicDataset
    (_, _, adj, _, _, _, _, _, _, tel, teu, tev, cv) = douban
    ds = MyDynamicDataset('data/t/viz_b', adj, (teu[:330], tev[:330]), tel[:330], 1, 1.0, 40, None, None, cv, seed=2)
    _check_pass(_igmc(ds, len(cv)), ds, 50, expect_graph=False)
    ds1 = MyDynamicDataset('data/t/viz_b1', adj, (teu[:7], tev[:7]), tel[:7], 1, 1.0, 40, None, None, cv, seed=2)
    _check_pass(_igmc(ds1, len(cv)), ds1, 50, expect_graph=False)


@pytest.mark.parametrize('cap,n', [(100, 620), (200, 430)], ids=['cap100_subgraph_kernel', 'cap200_dense_layers'])
def test_score_links_headline_shapes(ml1m, cap, n):
    from igmc_amd.util_functions import MyDynamicDataset
    (_, _, A, _, _, _, _, _, _, te_l, te_u, te_v, cv) = ml1m
    ds = MyDynamicDataset('data/t/viz_c%d' % cap, A, (te_u[:n], te_v[:n]), te_l[:n], 1, 1.0, cap, None, None, cv, seed=1)
    model = _igmc(ds, len(cv))
    _check_pass(model, ds, 50, expect_graph=True)
    sg = ds._scoregraph
    arena = sg.arenas[0]
    if cap == 100:
        assert sg.ws.dense_path(arena, 50)                       # the matrix-core subgraph kernel takes the steps
    else:
        assert arena.dense_layers(sg.ws)                         # the dense per-layer kernels


def test_score_links_ten_relations_dgcnn_rs_and_the_static_cache(tmp_path):
    from igmc_amd import preprocessing
    from igmc_amd.models import DGCNN_RS
    from igmc_amd.util_functions import MyDataset, MyDynamicDataset
    (_, _, adj, _, _, _, _, _, _, tel, teu, tev, cv) = preprocessing.load_data_monti('flixster', testing=True)
    assert len(cv) == 10
    n = 470
    dyn = MyDynamicDataset('data/t/viz_e', adj, (teu[:n], tev[:n]), tel[:n], 1, 1.0, 10000, None, None, cv, seed=2)
    _check_pass(_igmc(dyn, 10), dyn, 50, expect_graph=True)
    # the sort-pool family: the eager loop through forward_into (the replayed pipeline refuses it)
    dyn2 = MyDynamicDataset('data/t/viz_f', adj, (teu[:n], tev[:n]), tel[:n], 1, 1.0, 10000, None, None, cv, seed=2)
    _check_pass(_igmc(dyn2, 10, cls=DGCNN_RS), dyn2, 50, expect_graph=False)
    # a MyDataset: node sets from the HBM-resident cache (igmc_extract_batch_cached stamps its arenas too)
    st = MyDataset(str(tmp_path / 'static'), adj, (teu[:n], tev[:n]), tel[:n], 1, 1.0, 12, None, None, cv, seed=3)
    assert st._cache is not None
    _check_pass(_igmc(st, 10), st, 50, expect_graph=True)


def test_select_extremes_on_the_device_is_the_stable_argsort(douban):
    import torch
    from igmc_amd import engine
    from igmc_amd.train_eval import score_links
    from igmc_amd.util_functions import MyDynamicDataset
    (_, _, adj, _, _, _, _, _, _, tel, teu, tev, cv) = douban
    n = 2000
    ds = MyDynamicDataset('data/t/viz_s', adj, (teu[:n], tev[:n]), tel[:n], 1, 1.0, 40, None, None, cv, seed=2)
    R, Y, _ = score_links(_igmc(ds, len(cv)), ds, 50)
    rng = np.random.default_rng(0)
    big = torch.from_numpy(rng.normal(0, 1, 1000003).astype(np.float32)).cuda()
    ties = torch.from_numpy(rng.integers(1, 6, 300000).astype(np.float32)).cuda()
    for name, keys in (('R', R), ('Y', Y), ('big', big), ('ties', ties)):
        host = keys.cpu().numpy()
        order = np.argsort(host, kind='stable')
        for num in (1, 5, 64):
            for grid in (0, 1, 13, 1024):
                lo, hi, klo, khi = engine.select_extremes(keys, num, grid=grid)
                assert lo.cpu().numpy().tolist() == order[:num].tolist(), (name, num, grid)
                assert hi.cpu().numpy().tolist() == order[-num:][::-1].tolist(), (name, num, grid)
                assert np.array_equal(klo.cpu().numpy(), host[order[:num]])
                assert np.array_equal(khi.cpu().numpy(), host[order[-num:][::-1]])
    with pytest.raises(RuntimeError):
        engine.select_extremes(R, 65)


# ------------------------------------------------------------------ against the reference
def _fingerprint(A):
    A = ssp.csr_matrix(A)
    A.sort_indices()
    h = hashlib.sha256()
    for a in (A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.astype(np.float32)):
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest()[:8], np.uint64)[0]


def _golden_case(case):
    import torch
    from igmc_amd import preprocessing
    from igmc_amd.models import IGMC
    from igmc_amd.util_functions import MyDynamicDataset
    z = np.load(GOLDEN)
    g = lambda k: z[case + '/' + k]
    if case == 'igmc_r5':
        u, v, r = preprocessing.synth_ml(300, 200, 9000, preprocessing.ML_HIST['ml_100k'][3], seed=3)
        A = ssp.csr_matrix((r.astype(np.float32), (u, v)), shape=(300, 200))
    else:
        A = preprocessing.load_data_monti('flixster', testing=True)[2]
    assert _fingerprint(A) == g('graph_fingerprint')
    links, cv = g('links'), g('class_values')
    ds = MyDynamicDataset('data/t/viz_' + case, A, (links[:, 0], links[:, 1]), g('link_labels'), 1, 1.0, None, None, None,
                          cv, seed=1)
    model = IGMC(ds, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True,
                 adj_dropout=0.2).to('cuda')
    prefix = case + '/state/'
    model.load_state_dict({k[len(prefix):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(prefix)})
    return ds, model, cv, g


@pytest.mark.parametrize('case', ['igmc_r5', 'igmc_r10'])
def test_visualize_selects_what_the_reference_selected(case, tmp_path):
    """R within the suite's output tolerance of what the reference's ``visualize`` scored, and the same ``num`` highest /
    lowest links in the same order (the recorded ``num``: the generator asserts that the reference's selection is decided
    by gaps of more than 100 x that tolerance)."""
    from igmc_amd.train_eval import score_links, visualize
    ds, model, cv, g = _golden_case(case)
    R, Y, _ = score_links(model, ds, 50)
    err = PC.rel_err(R.cpu().numpy(), g('scores'))
    print('%s: scores vs the reference, relative to the peak: %.3e (tolerance %.1e)' % (case, err, PC.OUT_TOL))
    assert err < PC.OUT_TOL
    assert np.array_equal(Y.cpu().numpy(), g('ys'))
    num = int(g('num'))
    assert (case == 'igmc_r5' and len(cv) == 5) or (case == 'igmc_r10' and len(cv) == 10)
    res = visualize(model, ds, str(tmp_path), case, cv, num=num, sort_by='prediction')
    assert res['highest'] == g('highest').tolist() and res['lowest'] == g('lowest').tolist()
    assert ds._scoregraph.graph is not None                    # nine batches of 50: that pass replayed a captured graph
    assert res['path'] == str(tmp_path / ('visualization_%s_prediction.pdf' % case)) and os.path.getsize(res['path']) > 1000
    sel = res['highest'] + res['lowest']
    assert np.allclose(res['scores'], g('scores')[sel], rtol=0, atol=PC.OUT_TOL * np.abs(g('scores')).max())
    assert res['ys'] == g('ys')[sel].tolist()
    # sort_by='true': heavy ties, the defined order; 'random': the host permutation
    res_t = visualize(model, ds, str(tmp_path), case, cv, num=5, sort_by='true')
    order = np.argsort(g('ys'), kind='stable')
    assert res_t['lowest'] == order[:5].tolist() and res_t['highest'] == order[-5:][::-1].tolist()
    assert os.path.exists(str(tmp_path / ('visualization_%s_true.pdf' % case)))
    np.random.seed(5)
    res_r = visualize(model, ds, str(tmp_path), case, cv, num=3, sort_by='random')
    np.random.seed(5)
    perm = np.random.permutation(range(len(ds))).tolist()
    assert res_r['lowest'] == perm[:3] and res_r['highest'] == perm[-3:][::-1]


def test_the_drawn_subgraph_is_the_scored_one(ml1m, tmp_path):
    """On a capped dataset where sampling binds: the batch made of the 2 * num subgraphs ``visualize`` downloads gives,
    forwarded, their entries of R -- and the same links under another sampling key give other subgraphs."""
    import torch
    from igmc_amd.train_eval import SCORE_EPOCH, score_links, scored_subgraphs, visualize
    from igmc_amd.util_functions import MyDynamicDataset
    (_, _, A, _, _, _, _, _, _, te_l, te_u, te_v, cv) = ml1m
    n = 620
    ds = MyDynamicDataset('data/t/viz_d', A, (te_u[:n], te_v[:n]), te_l[:n], 1, 1.0, 100, None, None, cv, seed=1)
    model = _igmc(ds, len(cv))
    R, Y, _ = score_links(model, ds, 50)
    res = visualize(model, ds, str(tmp_path), 'ml', cv, num=5, sort_by='prediction')
    sel = res['highest'] + res['lowest']
    assert len(sel) == 10 and len(set(sel)) == 10
    assert res['scores'] == R[sel].tolist() and res['ys'] == Y[sel].tolist()
    datas, db = scored_subgraphs(ds, sel)
    gids = db._materialise()['raw']['node_gid'].copy()
    with torch.no_grad():
        out = model(db)
    err = PC.rel_err(out.cpu().numpy(), R[sel].cpu().numpy())
    print('forward of the downloaded subgraphs vs their scores: %.3e of the peak' % err)
    assert err < PC.OUT_TOL
    assert [d.num_nodes for d in datas] == np.diff(db._materialise()['raw']['node_off']).tolist()
    # sampling binds: the same links under the next epoch's key are other subgraphs with other scores
    pos = torch.tensor(sel, dtype=torch.int32, device='cuda')
    other = ds.extract(pos, 0, len(sel), epoch=SCORE_EPOCH + 1, slot='viz_other', max_graphs=len(sel))
    assert not np.array_equal(other._materialise()['raw']['node_gid'], gids)
    with torch.no_grad():
        out2 = model(other)
    assert PC.rel_err(out2.cpu().numpy(), R[sel].cpu().numpy()) > PC.OUT_TOL


# ------------------------------------------------------------------ end to end
def test_main_visualize_end_to_end(tmp_path):
    """``Main.py ... --epochs 1`` and then the same command with ``--visualize`` (reference ``Main.py:423-435``)."""
    cmd = [sys.executable, os.path.join(ROOT, 'Main.py'), '--data-name', 'douban', '--epochs', '1', '--testing',
           '--save-interval', '1', '--dynamic-train', '--max-train-num', '2000', '--max-test-num', '700',
           '--max-nodes-per-hop', '100']
    env = dict(os.environ, PYTHONPATH=ROOT)
    pdf = tmp_path / 'results' / 'douban_testmode' / 'visualization_douban_prediction.pdf'
    for extra in ([], ['--visualize']):
        r = subprocess.run(cmd + extra, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           timeout=600)
        out = r.stdout.decode()
        assert r.returncode == 0, out[-3000:]
        assert (tmp_path / 'results' / 'douban_testmode' / 'model_checkpoint1.pth').exists()
        assert pdf.exists() == bool(extra)
    assert pdf.stat().st_size > 1000 and pdf.read_bytes()[:5] == b'%PDF-'
    assert 'Transfer learning rmse' not in out


def test_main_visualize_with_transfer_prints_test_onces_rmse(tmp_path, monkeypatch, capsys):
    import importlib
    import torch
    from igmc_amd import preprocessing
    from igmc_amd.models import IGMC
    from igmc_amd.train_eval import test_once as run_test_once
    from igmc_amd.util_functions import MyDataset
    monkeypatch.chdir(tmp_path)
    src = tmp_path / 'ml_100k_ckpt'
    src.mkdir()

    class _DS(object):
        num_features = 4
    torch.manual_seed(100)
    m = IGMC(_DS(), latent_dim=[32, 32, 32, 32], num_relations=5, num_bases=4, regression=True)
    m.reset_parameters()
    ckpt = str(src / 'model_checkpoint1.pth')
    torch.save(m.state_dict(), ckpt)
    Main = importlib.import_module('Main')
    argv = ['--data-name', 'douban', '--epochs', '1', '--testing', '--no-train', '--visualize', '--transfer', str(src),
            '--num-relations', '5', '--multiply-by', '1', '--max-test-num', '600']
    rmse = Main.main(argv)
    out = capsys.readouterr().out
    found = re.findall(r'Transfer learning rmse is: ([0-9.]+)', out)
    assert len(found) == 1 and found[0] == '{:.6f}'.format(rmse)
    assert (tmp_path / 'results' / 'douban_testmode' / 'visualization_douban_prediction.pdf').stat().st_size > 1000
    assert 'Test rmse is' not in out                       # reference Main.py:423-435: --visualize and nothing else

    class _A(object):
        pass
    a = _A()
    a.standard_rating, a.transfer, a.data_name, a.num_relations = False, str(src), 'douban', 5
    rating_map, post_rating_map = Main.rating_maps(a)
    (_, _, adj, _, _, _, _, _, _, tel, teu, tev, cv) = preprocessing.load_data_monti('douban', True, rating_map, post_rating_map)
    te = MyDataset('data/x/test', adj, (teu, tev), tel, 1, 1.0, 10000, None, None, cv, max_num=600, seed=1)
    model = IGMC(te, latent_dim=[32, 32, 32, 32], num_relations=5, num_bases=4, regression=True)
    model.load_state_dict(torch.load(ckpt, map_location='cpu'))
    want = run_test_once(te, model, 50)
    assert '{:.6f}'.format(want) == found[0]
