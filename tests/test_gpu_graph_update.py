"""``igmc_graph_apply`` on a real MI355X: the cases and checks of tests/graph_update_checks.py as the emulator test runs them,
then what the update is for -- ``recommend`` / ``rank_eval`` / extraction over ``Graph.updated(...)`` through ``GraphView`` are
bit-equal to those over a dataset rebuilt from the changed matrix on the host -- and ``Main.py --new-ratings`` end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as ssp

import graph_update_checks as GU
import parity_checks as PC
from helpers import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    return PC.GpuBackend()


def test_single_changes_alone_and_mixed(be):
    GU.check_single_changes(be)


def test_empty_list_with_and_without_growth(be):
    GU.check_empty_list(be)


def test_row_lengths_across_the_wave_and_workgroup_widths(be):
    GU.check_corner_rows(be)


def test_row_longer_than_the_sort_tile(be):
    GU.check_corner_rows(be, extra=(GU.SORT_TILE + 1,))


def test_duplicates_the_last_wins(be):
    GU.check_duplicates(be)


@pytest.mark.parametrize('n', [GU.ROW_STAGE, GU.ROW_STAGE + 1, 300, GU.SORT_TILE, GU.SORT_TILE + 1])
def test_all_changes_in_one_row_and_in_one_column(be, n):
    GU.check_concentration(be, n)


def test_max_rel_and_degrees_follow_removals(be):
    GU.check_max_rel_and_degrees(be)


def test_growth(be):
    GU.check_growth(be)


@pytest.mark.parametrize('seed', range(20))
def test_random(be, seed):
    GU.check_random(be, seed)


def test_chained_updates_leave_every_stage_as_it_was(be):
    GU.check_chained(be)


def test_output_does_not_depend_on_the_grid(be):
    GU.check_geometry(be)


def test_errors_leave_out_untouched_and_the_library_serving(be):
    GU.check_errors(be)


def test_a_list_of_several_sort_tiles_from_every_kind_of_input(be):
    """20 000 changes: the sort takes its global strides (the padded list is 16 tiles); device tensors, host tensors and
    numpy arrays give the same graph."""
    import torch
    rng = np.random.default_rng(77)
    M = GU.random_matrix(300, 200, 0.1, 5, 77)
    n = 20000
    ch = (rng.integers(0, 330, n).astype(np.int32), rng.integers(0, 220, n).astype(np.int32), rng.integers(0, 6, n).astype(np.uint8))
    g2, M2 = GU.check_update(be, M, ch, what='20000 changes')
    g = GU.graph_of(be, M)
    want = g2.download()
    GU.assert_same_arrays(g.updated(*ch).download(), want, 'numpy arrays')
    GU.assert_same_arrays(g.updated(*[torch.from_numpy(x.astype(np.int64)) for x in ch]).download(), want, 'host int64 tensors')
    GU.assert_same_arrays(g.updated(*[torch.from_numpy(x).cuda() for x in ch]).download(), want, 'device tensors')


# ------------------------------------------------------------------ end to end
def _dataset(A, cv, tag):
    from igmc_amd.util_functions import MyDynamicDataset
    A = ssp.csr_matrix(A)
    A.eliminate_zeros()
    rows, cols = A.nonzero()
    labels = np.asarray(A[rows, cols]).ravel().astype(np.int64) - 1
    return MyDynamicDataset('data/t/gu_' + tag, A, (rows, cols), labels, 1, 1.0, None, None, None, cv, seed=1)      # hop 1, no cap


@pytest.fixture(scope='module')
def served():
    """A 30 x 40 graph, a model of fixed parameters, new ratings -- user 30 is brand-new and rates three items, user 2 gains
    two ratings, loses one and re-rates one, item 40 is brand-new -- and the same matrix rebuilt through the host."""
    import torch
    from igmc_amd.models import IGMC
    from igmc_amd.recommend import GraphView
    M = GU.random_matrix(30, 40, 0.3, 5, 21)
    M[2, 5], M[2, 6], M[2, 7], M[2, 8] = 0, 0, 3, 4
    cv = np.arange(1, 6, dtype=np.float64)
    ds = _dataset(M, cv, 'old')
    torch.manual_seed(4)
    model = IGMC(ds, latent_dim=[32, 32, 32, 32], num_relations=5, num_bases=4, regression=True, adj_dropout=0.2, seed=3).to('cuda')
    model.reset_parameters()
    model.eval()
    changes = GU.as_changes([(30, 3, 5), (30, 17, 1), (30, 25, 4), (2, 5, 2), (2, 6, 5), (2, 7, 0), (2, 8, 1), (5, 40, 3)])
    M2 = GU.apply_host(M, changes)
    assert M2.shape == (31, 41)
    before = ds.graph.download()
    g2 = ds.graph.updated(*changes)
    GU.assert_same_arrays(ds.graph.download(), before, 'the training graph')
    return dict(model=model, ds=ds, view=GraphView(ds, g2), rebuilt=_dataset(M2, cv, 'new'), M=M, M2=M2, changes=changes)


def test_recommend_over_the_updated_graph_equals_the_rebuilt_dataset(served):
    import torch
    from igmc_amd.recommend import recommend
    users = np.array([30, 2, 5, 0], np.int32)          # the brand-new user, the changed one, the one who rated the new item
    sa, sb = {}, {}
    got = recommend(served['model'], served['view'], users=users, n=5, stats=sa)
    want = recommend(served['model'], served['rebuilt'], users=users, n=5, stats=sb)
    assert sa == sb and sa['candidates'] == int((served['M2'][users] == 0).sum())
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert got[1].cpu().numpy().tobytes() == want[1].cpu().numpy().tobytes()
    items = got[0].cpu().numpy()
    assert (got[2].cpu().numpy() == 5).all() and np.isfinite(got[1].cpu().numpy()).all()
    assert not set(items[0].tolist()) & {3, 17, 25}          # what the new user just rated is no candidate
    assert not set(items[1].tolist()) & set(np.nonzero(served['M2'][2])[0].tolist())
    # the old graph still serves, and says something else about user 2 (whose row changed) than the updated one
    old = recommend(served['model'], served['ds'], users=users[1:], n=5)
    assert old[0].shape == (3, 5) and not torch.equal(old[1][0], got[1][1])
    # every user of the grown graph, by default
    allu = recommend(served['model'], served['view'], n=3)
    assert allu[0].shape == (31, 3) and torch.equal(allu[0], recommend(served['model'], served['rebuilt'], n=3)[0])


def test_rank_eval_over_the_updated_graph_equals_the_rebuilt_dataset(served):
    import torch
    from igmc_amd.rank_eval import HeldOut, rank_eval
    M2 = served['M2']
    hu, hv = [], []
    for u in (30, 2, 5, 11):                                  # three unseen items each as held-out links
        free = np.nonzero(M2[u] == 0)[0]
        hu += [u] * 3
        hv += free[[1, len(free) // 2, -1]].tolist()
    res = []
    for over in (served['view'], served['rebuilt']):
        held = HeldOut.from_links(over.graph, u=np.asarray(hu), v=np.asarray(hv))
        res.append(rank_eval(served['model'], over, held, ks=(3, 10)))
    a, b = res
    assert a['users_evaluated'] == b['users_evaluated'] == 4
    for k in ('cnt', 'dcg', 'rank', 'pos'):
        assert torch.equal(a['per_user'][k], b['per_user'][k]), k
    for k in a:
        if k != 'per_user':
            assert a[k] == b[k], k


def test_extraction_over_the_updated_graph_equals_the_rebuilt_graph(served):
    import torch
    from igmc_amd import engine
    M2 = served['M2']
    rng = np.random.default_rng(9)
    lu = np.concatenate([[30, 30, 2, 2, 5, 29], rng.integers(0, 31, 44)]).astype(np.int32)
    lv = np.concatenate([[3, 0, 5, 7, 40, 40], rng.integers(0, 41, 44)]).astype(np.int32)
    du, dv, dy = torch.from_numpy(lu).cuda(), torch.from_numpy(lv).cuda(), torch.zeros(50, device='cuda')
    out = []
    for graph in (served['view'].graph, served['rebuilt'].graph):
        arena = engine.Batch(graph, 50, 1, None)
        arena.extract(du.data_ptr(), dv.data_ptr(), dy.data_ptr(), None, 0, 50, 1.0, 1, 0, torch.cuda.current_stream().cuda_stream)
        out.append(arena.download())
    a, b = out
    assert a.keys() == b.keys() and a['B'] == 50 and a['E'] > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_graph_view_is_what_candidate_links_reads_and_refuses_side_features(served):
    from igmc_amd.recommend import CandidateLinks, GraphView
    ds, view = served['ds'], served['view']
    assert view.graph is not ds.graph and view.source is ds and view.device == ds.device
    assert (view.h, view.sample_ratio, view.seed, view.max_nodes_per_hop) == (ds.h, ds.sample_ratio, ds.seed, ds.max_nodes_per_hop)
    assert view.link_y.device == ds.link_y.device and view._side is None and view.u_features is None and view.v_features is None
    c = CandidateLinks.for_users(view, [30])
    assert c.graph is view.graph and len(c) == 41 - 3

    class _WithFeatures(object):
        u_features, v_features, _side = np.zeros((1, 1)), np.zeros((1, 1)), None
    with pytest.raises(NotImplementedError, match='--use-features'):
        GraphView(_WithFeatures(), view.graph)


def test_main_new_ratings_end_to_end(tmp_path):
    """``Main.py ... --epochs 1`` on a few hundred links for a checkpoint, then ``--no-train --recommend 3 --new-ratings FILE``:
    the TSV has rows for the brand-new user, and none of them is an item that user just rated."""
    cmd = [sys.executable, os.path.join(ROOT, 'Main.py'), '--data-name', 'douban', '--epochs', '1', '--testing',
           '--save-interval', '1', '--dynamic-train', '--max-train-num', '300', '--max-test-num', '100',
           '--max-nodes-per-hop', '100']
    env = dict(os.environ, PYTHONPATH=ROOT)
    new = tmp_path / 'new.txt'
    new.write_text('# a user the graph has never seen\n3000 10 5\n3000 20 4\n3000 30 1\n7 10 0   # and one rating withdrawn\n')
    who = tmp_path / 'who.txt'
    who.write_text('3000\n7\n')
    tsv = tmp_path / 'results' / 'douban_testmode' / 'recommendations_douban.tsv'
    for extra in ([], ['--no-train', '--recommend', '3', '--recommend-users', str(who), '--new-ratings', str(new)]):
        r = subprocess.run(cmd + extra, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        out = r.stdout.decode()
        assert r.returncode == 0, out[-3000:]
    assert 'Applied 4 rating change(s) on the device' in out and '-> 3001 x 3000' in out
    rec = [l.split('\t') for l in tsv.read_text().splitlines()]
    assert [int(x[0]) for x in rec] == [3000] * 3 + [7] * 3 and [int(x[1]) for x in rec] == [1, 2, 3] * 2
    assert not {int(x[2]) for x in rec[:3]} & {10, 20, 30}
    assert all(np.isfinite(float(x[3])) for x in rec)
