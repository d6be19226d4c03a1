"""Given-k cold-start evaluation on a real MI355X (``rank_eval.hold_out`` / ``cold_start_eval``, ``igmc_amd/csrc/holdout.hip``) on
the small case of ``tests/test_gpu_rank_eval.py`` (30 x 40, 70 test links, no cap, hop 1): the split is the numpy definition of
``tests/holdout_checks.py`` under the dataset's seed, every level's ranks are bit-equal to ``rank_eval`` over a dataset rebuilt on
the host from the reduced matrix, the ``extra`` block is the float64 restatement of the metrics over the test links alone, the
``full`` level is plain ``rank_eval``; sampled negatives, a shortlist and ``DGCNN_RS`` are served alike; and ``Main.py
--cold-start`` end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as ssp

import holdout_checks as HC
from helpers import ROOT
from test_gpu_rank_eval import _check_metrics, _numpy_metrics, small          # noqa: F401  (small: the fixture)

pytestmark = pytest.mark.gpu
KS = (1, 5, 10)
GIVEN = (1, 3)


@pytest.fixture(scope='module')
def case(small):
    """The small case, its 70 held-out links as the ``extra`` dataset, and per level the reduced matrix with a dataset rebuilt
    from it on the host."""
    from igmc_amd.util_functions import MyDynamicDataset
    ds, At, cv = small['ds'], small['A'].tocsr(), small['cv']
    extra = MyDynamicDataset('data/t/cs_x', At, (small['hu'], small['hv']), small['hy'].astype(np.int64) - 1, 1, 1.0, None, None,
                             None, cv, seed=1)
    users = np.arange(30, dtype=np.int32)
    levels = {}
    for k in GIVEN:
        held = [HC.split_ref(At, int(u), k, seed=ds.seed)[1:] for u in users]
        hu = np.concatenate([np.full(len(v), u, np.int32) for u, (v, _) in zip(users, held)])
        hv, hr = np.concatenate([v for v, _ in held]), np.concatenate([r for _, r in held])
        B = At.tolil(copy=True)
        B[hu, hv] = 0
        B = ssp.csr_matrix(B)
        B.eliminate_zeros()
        tu, tv = B.nonzero()
        host = MyDynamicDataset('data/t/cs_%d' % k, B, (tu, tv), np.asarray(B[tu, tv]).ravel().astype(np.int64) - 1, 1, 1.0, None,
                                None, None, cv, seed=1)
        levels[k] = dict(hu=hu, hv=hv, hr=hr, B=B, ds=host)
    return dict(small, extra=extra, levels=levels)


def test_the_split_is_the_definition_and_the_view_serves_the_reduced_graph(case):
    import torch
    from igmc_amd.rank_eval import hold_out
    ds, cv = case['ds'], case['cv']
    for k in GIVEN:
        want = case['levels'][k]
        split = hold_out(ds, keep=k)
        assert np.array_equal(split.users.cpu().numpy(), np.arange(30)) and len(split) == len(want['hu'])
        assert split.u.dtype == torch.int32 and split.rel.dtype == torch.uint8 and split.ratings.dtype == torch.float32
        assert np.array_equal(split.u.cpu().numpy(), want['hu']) and np.array_equal(split.v.cpu().numpy(), want['hv'])
        assert np.array_equal(split.rel.cpu().numpy(), want['hr'] - 1)
        assert np.array_equal(split.ratings.cpu().numpy(), cv[want['hr'] - 1].astype(np.float32))
        assert np.array_equal(split.offsets.cpu().numpy(), HC.offsets(np.diff(ds.graph.download()['u_ptr']) - k))
        got, ref = split.graph.download(), want['ds'].graph.download()
        assert all(got[x].tobytes() == ref[x].tobytes() for x in ref) and split.view.graph is split.graph
        # a user's split does not depend on the users asked for with it, nor on their order
        some = np.array([17, 3, 29], np.int32)
        part = hold_out(ds, some, keep=k)
        off = split.offsets.cpu().numpy()
        assert np.array_equal(part.v.cpu().numpy(), np.concatenate([want['hv'][off[u]:off[u + 1]] for u in some]))
        assert np.array_equal(part.heldout().source.cpu().numpy(), np.zeros(len(part), np.uint8))
    with pytest.raises(ValueError, match='more than once'):
        hold_out(ds, [3, 4, 3], keep=1)
    with pytest.raises(ValueError, match='outside'):
        hold_out(ds, [3, 30], keep=1)
    loo = hold_out(ds, keep=1, hold=1)          # leave-one-out: exactly one link of every user
    assert np.array_equal(loo.offsets.cpu().numpy(), np.arange(31)) and loo.graph.nnz == ds.graph.nnz - 30


def _rebuilt(case, model, k, heldout, **kw):
    from igmc_amd.rank_eval import rank_eval
    return rank_eval(model, case['levels'][k]['ds'], heldout, KS, **kw)


def test_levels_are_rank_eval_over_the_rebuilt_dataset_and_the_blocks_their_restatement(case):
    import torch
    from igmc_amd.rank_eval import HeldOut, cold_start_eval, hold_out, rank_eval
    ds, model, extra = case['ds'], case['model'], case['extra']
    stats = {}
    res = cold_start_eval(model, ds, given=GIVEN, extra=extra, ks=KS, min_rating=3, stats=stats)
    assert sorted(res, key=str) == [1, 3, 'full'] and stats['users'] == 30 and stats['users_skipped'] == 0
    for k in GIVEN:
        want = case['levels'][k]
        assert stats['removed'][k] == len(want['hu'])
        heldout = hold_out(ds, keep=k).heldout(extra, 3)
        source = heldout.source.cpu().numpy()
        assert len(heldout) == len(want['hu']) + 70 and int(source.sum()) == 70
        block = res[k]['heldout']
        ref = _rebuilt(case, model, k, heldout)
        for x in ('rank', 'pos', 'cnt', 'dcg'):
            assert torch.equal(block['per_user'][x], ref['per_user'][x]), (k, x)
        assert all(block[x] == ref[x] for x in ref if x != 'per_user')
        rank = block['per_user']['rank'].cpu().numpy()
        assert (rank >= 0).all()
        owner = np.repeat(heldout.users.cpu().numpy(), np.diff(heldout.offsets.cpu().numpy()))
        relevant = heldout.relevant.cpu().numpy() != 0
        _check_metrics(block, *_numpy_metrics(rank, owner, KS, relevant))
        _check_metrics(res[k]['extra'], *_numpy_metrics(rank, owner, KS, relevant & (source == 1)))
        print('given %d: heldout hr@10 %.4f, extra hr@10 %.4f' % (k, block['hr@10'], res[k]['extra']['hr@10']))
    full = rank_eval(model, ds, HeldOut.from_links(extra, min_rating=3), KS, users=np.arange(30))
    assert torch.equal(res['full']['extra']['per_user']['rank'], full['per_user']['rank'])
    assert all(res['full']['extra'][x] == full[x] for x in full if x != 'per_user')
    assert list(res['full']) == ['extra']
    # without an extra set: the removed links alone, no extra block and no full level
    alone = cold_start_eval(model, ds, given=(3,), ks=KS)
    assert list(alone) == [3] and list(alone[3]) == ['heldout']
    assert torch.equal(alone[3]['heldout']['per_user']['rank'],
                       _rebuilt(case, model, 3, hold_out(ds, keep=3).heldout())['per_user']['rank'])


def test_users_with_no_more_than_the_largest_level_are_skipped(case):
    from igmc_amd.rank_eval import cold_start_eval
    ds, model = case['ds'], case['model']
    d = np.diff(case['A'].tocsr().indptr)
    asked = np.array([29, 0, 5, 11, 12, 13, 20, 21], np.int32)
    assert 0 < (d[asked] > 7).sum() < len(asked)
    stats = {}
    res = cold_start_eval(model, ds, given=(7,), users=asked, ks=KS, stats=stats)
    kept = asked[d[asked] > 7]
    assert stats['users'] == len(kept) and stats['users_skipped'] == len(asked) - len(kept)
    assert np.array_equal(res[7]['heldout']['per_user']['users'].cpu().numpy(), np.sort(kept))
    assert stats['removed'][7] == int((d[kept] - 7).sum())
    with pytest.raises(ValueError, match='no user has more than'):
        cold_start_eval(model, ds, given=(1000,), ks=KS)


@pytest.mark.parametrize('kw', [dict(negatives=5), dict(shortlist=10)], ids=['negatives', 'shortlist'])
def test_sampled_negatives_and_a_shortlist_agree_with_the_rebuilt_dataset(case, kw):
    import torch
    from igmc_amd.rank_eval import cold_start_eval, hold_out
    ds, model, extra = case['ds'], case['model'], case['extra']
    res = cold_start_eval(model, ds, given=GIVEN, extra=extra, ks=KS, **kw)
    for k in GIVEN:
        heldout = hold_out(ds, keep=k).heldout(extra)
        ref = _rebuilt(case, model, k, heldout, **kw)
        for x in ('rank', 'pos', 'cnt', 'dcg'):
            assert torch.equal(res[k]['heldout']['per_user'][x], ref['per_user'][x]), (k, x)
        assert res[k]['extra']['users_evaluated'] == 30


def test_dgcnn_rs_is_served_alike():
    import torch
    from igmc_amd import preprocessing
    from igmc_amd.models import DGCNN_RS
    from igmc_amd.rank_eval import cold_start_eval, hold_out, rank_eval
    from igmc_amd.util_functions import MyDynamicDataset
    (_, _, adj, trl, tru, trv, _, _, _, tel, teu, tev, cv) = preprocessing.load_data_monti('flixster', testing=True)
    ds = MyDynamicDataset('data/t/cs_d', adj, (tru, trv), trl, 1, 1.0, 40, None, None, cv, seed=2)
    torch.manual_seed(4)
    model = DGCNN_RS(ds, latent_dim=[32, 32, 32, 1], k=30, num_relations=len(cv), num_bases=4, regression=True,
                     adj_dropout=0.2, seed=1).to('cuda')
    model.reset_parameters()
    model.eval()
    d = np.diff(ds.graph.download()['u_ptr'])
    users = np.nonzero(d > 2)[0][:5].astype(np.int32)
    stats = {}
    res = cold_start_eval(model, ds, given=(2,), users=users, ks=(5, 10), stats=stats)
    assert stats['users'] == 5 and stats['removed'][2] == int((d[users] - 2).sum())
    split = hold_out(ds, users, keep=2)
    ref = rank_eval(model, split.view, split.heldout(), (5, 10))
    assert torch.equal(res[2]['heldout']['per_user']['rank'], ref['per_user']['rank'])
    assert res[2]['heldout']['users_evaluated'] == 5 and 0.0 <= res[2]['heldout']['mrr'] <= 1.0


def test_main_cold_start_end_to_end(tmp_path):
    """``Main.py ... --epochs 1 --max-train-num 2000`` for a checkpoint, then ``--no-train --rank-eval 5 --cold-start 1,3
    --cold-users 20``: the file's lines and levels."""
    cmd = [sys.executable, os.path.join(ROOT, 'Main.py'), '--data-name', 'douban', '--epochs', '1', '--testing',
           '--save-interval', '1', '--dynamic-train', '--dynamic-test', '--max-train-num', '2000', '--max-nodes-per-hop', '100']
    env = dict(os.environ, PYTHONPATH=ROOT)
    tsv = tmp_path / 'results' / 'douban_testmode' / 'coldstart_douban.tsv'
    for more in ([], ['--no-train', '--rank-eval', '5', '--cold-start', '1,3', '--cold-users', '20']):
        r = subprocess.run(cmd + more, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        out = r.stdout.decode()
        assert r.returncode == 0, out[-3000:]
        assert tsv.exists() == bool(more)          # without the flag nothing changes
    assert not (tmp_path / 'results' / 'douban_testmode' / 'ranking_douban.tsv').exists()
    lines = [l.split('\t') for l in tsv.read_text().splitlines()]
    names = ['hr@5', 'recall@5', 'precision@5', 'ndcg@5', 'mrr']
    assert [l[:3] for l in lines] == [[g, b, m] for g, blocks in (('1', ('heldout', 'extra')), ('3', ('heldout', 'extra')),
                                                                 ('full', ('extra',))) for b in blocks for m in names]
    assert all(0.0 <= float(l[3]) <= 1.0 for l in lines)
    summary = [l for l in out.splitlines() if l.startswith('Given ')]
    assert [l.split(':')[0] for l in summary] == ['Given 1', 'Given 3', 'Given full'] and 'Cold start: ' in out
    print('\n'.join(summary))
