"""Pair training on a real MI355X: ``k_pair_negatives`` / ``k_pair_loss`` (``igmc_amd/csrc/pairs.hip``) and
``igmc_pair_loss_grad`` through their C entry points against the references of ``tests/pair_checks.py`` -- the cases and checks
the emulator test runs (test_emu_pairs.py) --, then what needs the device: ``pair_train.PairLinks``, ``train_pairs`` and
``Main.py --pair-epochs / --pair-checkpoint`` end to end.  What the single-threaded emulator cannot show is what the first
part is for: four waves of a workgroup walking rows of their own through their own LDS stage with no barrier between them,
ballots over real lanes, the workgroup tree of the loss.

Every buffer of the direct calls sits between guard elements checked after every call; the bad ids are refused before any
row pointer is read.  Every sampler comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as ssp

import pair_checks as PK
import parity_checks as PC
from helpers import ROOT, load_extract_golden

pytestmark = pytest.mark.gpu
CASES = load_extract_golden()


def sub(name, n):
    case = dict(CASES[name])
    case['recs'], case['links'], case['link_labels'] = case['recs'][:n], case['links'][:n], case['link_labels'][:n]
    return case


@pytest.fixture(scope='module')
def be():
    return PC.GpuBackend()


# ------------------------------------------------------------------ the sampler
@pytest.mark.parametrize('n_items', [63, 64, 65, 300, 40000])
def test_negatives_are_the_definition(be, n_items):
    PK.check_definition(be, n_items)


def test_a_second_round_of_tries_decides_some_draws(be):
    PK.check_second_round(be)


def test_the_cyclic_scan_decides_where_the_tries_give_out(be, monkeypatch):
    monkeypatch.setenv('IGMC_PAIR_TRIES', '2')
    PK.check_fallback(be, 'crowded', 2)
    monkeypatch.setenv('IGMC_PAIR_TRIES', '0')
    PK.check_fallback(be, 'half', 0)


def test_a_user_without_an_unseen_item_gets_void_pairs(be):
    PK.check_void_pairs(be)


def test_ids_out_of_range_are_reported_and_their_rows_not_read(be):
    PK.check_bad_ids(be, (-1, 4, 2 ** 31 - 1))


def test_bad_arguments_are_refused(be):
    PK.check_refusals(be.lib)
    be.sync()          # (nothing was launched: nothing can have gone wrong behind the calls)


def test_more_positives_than_waves_in_the_grid(be):
    PK.check_many_positives(be)


@pytest.mark.parametrize('n_items, seen', sorted(PK.STAT_USERS))
def test_draws_are_the_restatement_and_uniform_over_the_unseen_items(be, n_items, seen):
    PK.check_distribution(be, n_items, seen)


# ------------------------------------------------------------------ the pair loss
@pytest.mark.parametrize('A', [0.0, 1.0])
@pytest.mark.parametrize('n_pairs, void', [(1, 'none'), (1, 'all'), (2, 'first'), (31, 'last'), (32, 'interleaved'), (33, 'none'),
                                           (250, 'none'), (250, 'first'), (250, 'last'), (250, 'interleaved'), (250, 'all')])
def test_pair_loss_is_the_float64_reference(be, n_pairs, void, A):
    PK.check_pair_loss(be, n_pairs, void, A)


# ------------------------------------------------------------------ the step
@pytest.mark.parametrize('name, n, R, drop, n_side', [
    ('synth_cap', 6, 5, False, 0),
    ('synth_cap', 6, 5, True, 0),
    ('flixster', 4, 10, True, 0),
    ('synth_nocap', 2, 5, False, 10),
    ('hand_h2', 4, 5, True, 0),
])
def test_pair_step_matches_the_oracle(be, name, n, R, drop, n_side):
    PK.check_step(be, sub(name, n), n, R, drop, n_side)


def test_pure_pairwise_objective_matches_the_oracle(be):
    PK.check_step(be, sub('synth_cap', 8), 8, 5, True, A=0.0)


def test_an_odd_batch_is_refused(be):
    PK.check_odd_batch_is_refused(be, sub('synth_cap', 3))


def test_pair_steps_follow_the_oracle_trajectory(be):
    PK.check_trajectory(be, sub('synth_cap', 6), 6, 5)


# ------------------------------------------------------------------ PairLinks, train_pairs
def two_halves(seed, n_users=60, n_items=80, per_user=12):
    """Every user rates ``per_user`` items of ONE of two disjoint item halves: links (u, v, label) and the rating matrix."""
    rng = np.random.default_rng(seed)
    u = np.repeat(np.arange(n_users), per_user)
    half = n_items // 2
    v = np.concatenate([(uu >= n_users // 2) * half + rng.choice(half, per_user, replace=False) for uu in range(n_users)])
    lab = rng.integers(0, 5, len(u))
    A = ssp.csr_matrix((lab + 1.0, (u, v)), shape=(n_users, n_items)).astype(np.float32)
    return A, u, v, lab


def dataset(A, u, v, lab, seed, cls=None, root='data/pairs', feats=(None, None), **kw):
    from igmc_amd.util_functions import MyDynamicDataset
    return (cls or MyDynamicDataset)(root, A, (u, v), lab, 1, 1.0, 20, feats[0], feats[1], np.arange(1.0, 6.0), seed=seed, **kw)


def fresh_model(ds, seed, **kw):
    import torch
    from igmc_amd.models import IGMC
    torch.manual_seed(seed)
    model = IGMC(ds, latent_dim=[32, 32, 32, 32], num_relations=5, num_bases=4, regression=True, adj_dropout=0.0, seed=seed,
                 **kw).to('cuda')
    model.reset_parameters()
    return model


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_it_learns(seed):
    """60 x 80, every user inside one item half: two epochs of ``train_pairs`` (30 steps each) from ``reset_parameters()``.
    The mean pair term of a FIXED evaluation draw, scored in evaluation mode, must be lower after than before and the pair
    accuracy no lower (no magnitude is stated); two runs of the same seed leave bit-identical parameters."""
    from igmc_amd.pair_train import PairLinks, eval_pairs, train_pairs
    A, u, v, lab = two_halves(seed)
    ds = dataset(A, u, v, lab, seed)
    held = PairLinks(ds).redraw(1000)
    runs = []
    for _ in range(2):
        model = fresh_model(ds, seed)
        before = eval_pairs(model, held, 48)
        hist = train_pairs(model, ds, 2, 48, 2e-3, mse_weight=0.0, ARR=0.001)
        after = eval_pairs(model, held, 48)
        print('seed %d: pair term %.4f -> %.4f, accuracy %.3f -> %.3f' % ((seed,) + (before[0], after[0], before[1], after[1])))
        assert len(hist) == 2 and hist[0]['pairs'] == len(u) and hist[0]['void'] == 0
        assert after[0] < before[0] and after[1] >= before[1], (before, after)
        runs.append(model.flat_parameters().detach().cpu().numpy().copy())
    assert np.isfinite(runs[0]).all() and runs[0].tobytes() == runs[1].tobytes()


def test_train_pairs_refuses_what_is_out_of_scope(monkeypatch):
    from igmc_amd import parallel
    from igmc_amd.pair_train import train_pairs
    A, u, v, lab = two_halves(1)
    ds = dataset(A, u, v, lab, 1)
    model = fresh_model(ds, 1)
    monkeypatch.setattr(parallel, 'world_size', lambda: 2)
    with pytest.raises(RuntimeError, match='one rank'):
        train_pairs(model, ds, 1, 48, 1e-3)
    monkeypatch.undo()

    class NotIGMC(object):
        pass
    with pytest.raises(NotImplementedError, match='IGMC'):
        train_pairs(NotIGMC(), ds, 1, 48, 1e-3)


def test_pair_links_keep_pairs_adjacent_and_redraw_is_idempotent():
    import torch
    from igmc_amd.pair_train import PairLinks
    A, u, v, lab = two_halves(2)
    ds = dataset(A, u, v, lab, 2)
    pl = PairLinks(ds)
    n = len(u)
    assert pl.capacity == 2 * n and len(pl) == 2 * n
    for epoch in (1, 2):
        pos = pl.epoch_positions(epoch).cpu().numpy()
        assert pos.dtype == np.int32 and sorted(pos.tolist()) == list(range(2 * n))
        assert (pos[0::2] % 2 == 0).all() and (pos[1::2] == pos[0::2] + 1).all()
    assert not np.array_equal(pl.epoch_positions(1).cpu().numpy(), pl.epoch_positions(2).cpu().numpy())
    assert np.array_equal(pl.epoch_positions(1).cpu().numpy(), pl.epoch_positions(1).cpu().numpy())
    first = [t.clone() for t in (pl.redraw(1).link_u, pl.link_v, pl.link_y)]
    other = pl.redraw(2).link_v.clone()
    again = [t.clone() for t in (pl.redraw(1).link_u, pl.link_v, pl.link_y)]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, again)) and not torch.equal(first[1], other)
    lu, lv, ly = (t.cpu().numpy() for t in again)
    ru, rv, ry, err, _ = PK.negatives_ref(A, u.astype(np.int32), v.astype(np.int32), 2, 1)
    assert int(pl.err.item()) == err == 0
    assert np.array_equal(lu, ru) and np.array_equal(lv, rv) and np.array_equal(ly[1::2], ry)
    assert np.array_equal(ly[0::2], (lab + 1).astype(np.float32))          # the positives keep their ratings
    with pytest.raises(ValueError, match='outside the rating graph'):
        PairLinks(ds, [0, 60], [1, 1], [1.0, 2.0])


def test_a_source_with_side_features_serves_through_its_node_tables():
    import torch
    from igmc_amd.pair_train import PairLinks
    A, u, v, lab = two_halves(3)
    rng = np.random.default_rng(3)
    uf, vf = rng.standard_normal((60, 3)).astype(np.float32), rng.standard_normal((80, 5)).astype(np.float32)
    ds = dataset(A, u, v, lab, 3, feats=(uf, vf))
    pl = PairLinks(ds).redraw(1)
    assert pl._side is None and pl.node_side() is ds.node_side() and pl.n_side_features == 8
    pos = pl.epoch_positions(1)
    db = pl.extract(pos, 10, 12, epoch=1, max_graphs=12)
    torch.cuda.synchronize()
    at = pos[10:22].long()
    want = np.concatenate([uf[pl.link_u[at].cpu().numpy()], vf[pl.link_v[at].cpu().numpy()]], 1)
    assert np.array_equal(db.side.cpu().numpy(), want)
    model = fresh_model(ds, 3, side_features=True, n_side_features=8)
    model.train()
    st = model.pair_loss_grad(db, ARR=0.001, mse_weight=1.0)
    assert np.isfinite(st.cpu().numpy()).all() and float(st[3]) == 6.0 and torch.isfinite(model.flat_grad()).all()


def test_a_static_source_is_extracted_from_the_graph(tmp_path):
    import torch
    from igmc_amd.pair_train import PairLinks
    from igmc_amd.util_functions import MyDataset
    A, u, v, lab = two_halves(4)
    ds = dataset(A, u, v, lab, 4, cls=MyDataset, root=str(tmp_path / 'static'), cache=True)
    assert ds._cache is not None and not ds.dynamic
    pl = PairLinks(ds).redraw(1)
    assert pl._cache is None and not pl.dynamic
    db = pl.extract(None, 0, 8, epoch=5, max_graphs=8)
    torch.cuda.synchronize()
    d = db.arena.download()
    lo = d['node_off'][:8]
    assert np.array_equal(d['node_gid'][lo], pl.link_u[:8].cpu().numpy())
    assert np.array_equal(d['node_gid'][lo + d['n_users'][:8]], pl.link_v[:8].cpu().numpy())
    assert np.array_equal(d['y'][:8], pl.link_y[:8].cpu().numpy())


# ------------------------------------------------------------------ end to end
def test_main_pair_epochs_and_pair_checkpoint_end_to_end(tmp_path):
    """``Main.py ... --epochs 1 --pair-epochs 1`` trains, fine-tunes and saves both checkpoints and the pair log; then, with
    ``model_checkpoint1.pth`` gone, ``--no-train --pair-checkpoint 1 --rank-eval 5,10`` serves from the pair file."""
    cmd = [sys.executable, os.path.join(ROOT, 'Main.py'), '--data-name', 'douban', '--epochs', '1', '--testing',
           '--save-interval', '1', '--dynamic-train', '--dynamic-test', '--max-train-num', '600', '--max-test-num', '300',
           '--max-nodes-per-hop', '50']
    env = dict(os.environ, PYTHONPATH=ROOT)
    res = tmp_path / 'results' / 'douban_testmode'

    def run(extra):
        r = subprocess.run(cmd + extra, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        out = r.stdout.decode()
        assert r.returncode == 0, out[-3000:]
        return out

    out = run(['--pair-epochs', '1', '--pair-mse-weight', '0.5'])
    assert (res / 'model_checkpoint1.pth').exists() and (res / 'pair_checkpoint1.pth').exists()
    log = (res / 'pair_log.txt').read_text().splitlines()
    assert len(log) == 1 and log[0].startswith('Pair epoch 1, pair loss ') and log[0] in out
    assert all('Pair' not in l for l in (res / 'log.txt').read_text().splitlines())
    os.remove(str(res / 'model_checkpoint1.pth'))
    out = run(['--no-train', '--pair-checkpoint', '1', '--rank-eval', '5,10', '--recommend-users', '30'])
    assert 'Serving from pair_checkpoint1.pth' in out and len([l for l in out.splitlines() if l.startswith('Ranked ')]) == 1
    assert (res / 'ranking_douban.tsv').exists()
