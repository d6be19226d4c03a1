"""Hard pair negatives on a real MI355X: ``k_pair_negatives<true>`` / ``k_pair_kind_stats`` (``igmc_amd/csrc/pairs.hip``) through
their C entry points against the restatement of ``tests/pair_hard_checks.py`` -- the cases and checks the emulator test runs
(test_emu_pair_hard.py) --, then what needs the device: ``PairLinks.set_shortlist`` over the real ``igmc_shortlist_fill``,
``train_pairs(shortlist=...)`` and ``Main.py --pair-shortlist`` end to end.  What the single-threaded emulator cannot show is
what the first part is for: four waves of a workgroup deciding, picking and walking rows of their own with no barrier
between them, one live lane's ballot, the workgroup tree of the statistics.

Every buffer of the direct calls sits between guard elements checked after every call -- the table's items among them: a
segment followed past its table would show there.  Every sampler comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as ssp

import pair_hard_checks as PH
import parity_checks as PC
from helpers import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    return PC.GpuBackend()


# ------------------------------------------------------------------ the sampler
@pytest.mark.parametrize('n_items', PH.N_ITEMS)
def test_negatives_are_the_definition(be, n_items):
    PH.check_definition(be, n_items)


def test_share_zero_and_a_null_table_give_the_bytes_of_the_uniform_entry(be):
    PH.check_share_zero_is_the_old_entry(be)


def test_positions_decided_uniform_keep_their_uniform_negative(be):
    PH.check_uniform_positions_keep_their_negative(be)


def test_a_user_who_rated_every_item_gets_void_pairs(be):
    PH.check_a_full_row_gives_void_pairs(be)


@pytest.mark.parametrize('which', PH.STALE)
def test_a_pick_that_does_not_qualify_falls_back_and_is_reported(be, which):
    PH.check_stale_pick(be, which)


@pytest.mark.parametrize('which', PH.BAD_OFFSETS)
def test_broken_offsets_are_reported_and_not_followed(be, which):
    PH.check_broken_offsets(be, which)


def test_ids_out_of_range_are_reported_and_nothing_of_theirs_is_read(be):
    PH.check_bad_ids(be, (-1, 4, 2 ** 31 - 1))


def test_more_positives_than_waves_in_the_grid(be):
    PH.check_many_positives(be)


def test_the_cyclic_scan_decides_behind_a_fall_through(be, monkeypatch):
    monkeypatch.setenv('IGMC_PAIR_TRIES', '0')
    PH.check_scan_behind_a_fall_through(be)


def test_bad_arguments_are_refused(be):
    PH.check_refusals(be.lib)
    be.sync()          # (nothing was launched: nothing can have gone wrong behind the calls)


def test_draws_are_the_restatement_and_within_both_bounds(be):
    PH.check_distribution(be)


@pytest.mark.parametrize('kinds', PH.KINDS)
@pytest.mark.parametrize('n_pairs', [1, 2, 33, 250])
def test_kind_stats_are_the_float64_reference(be, n_pairs, kinds):
    PH.check_kind_stats(be, n_pairs, kinds)


# ------------------------------------------------------------------ PairLinks, train_pairs
def taste_blocks(seed, n_users=60, n_items=80, common=4, rate_common=2, rate_taste=14):
    """Two co-rating blocks of 30 users x 40 items; inside a block 4 items everybody may rate and two TASTES of 18 items and 15
    users each: a user rates 2 of the common items (any rating) and 14 of the 18 items of its taste (4 or 5) -- 960 links.
    The common items make every user of a block a co-rater of every other, so a user's shortlist of 10 holds its few unseen
    items of its own taste and of the common ones and then items of the OTHER taste: unseen items whose raters share almost
    nothing with the user, which is what tells them from the items it rated."""
    rng = np.random.default_rng(seed)
    blocks, per_block_u, per_block_i = 2, n_users // 2, n_items // 2
    taste_items = (per_block_i - common) // 2
    us, vs, labs = [], [], []
    for u in range(n_users):
        b, taste = u // per_block_u, (u % per_block_u) // (per_block_u // 2)
        i0 = b * per_block_i
        mine = np.concatenate([i0 + rng.choice(common, rate_common, replace=False),
                               i0 + common + taste * taste_items + rng.choice(taste_items, rate_taste, replace=False)])
        us.append(np.full(len(mine), u))
        vs.append(mine)
        labs.append(np.concatenate([rng.integers(0, 5, rate_common), rng.integers(3, 5, rate_taste)]))
    u, v, lab = np.concatenate(us), np.concatenate(vs), np.concatenate(labs)
    assert blocks * per_block_u == n_users
    A = ssp.csr_matrix((lab + 1.0, (u, v)), shape=(n_users, n_items)).astype(np.float32)
    return A, u, v, lab


def dataset(A, u, v, lab, seed):
    from igmc_amd.util_functions import MyDynamicDataset
    return MyDynamicDataset('data/pair_hard', A, (u, v), lab, 1, 1.0, 20, None, None, np.arange(1.0, 6.0), seed=seed)


def fresh_model(ds, seed):
    import torch
    from igmc_amd.models import IGMC
    torch.manual_seed(seed)
    model = IGMC(ds, latent_dim=[32, 32, 32, 32], num_relations=5, num_bases=4, regression=True, adj_dropout=0.0, seed=seed).to('cuda')
    model.reset_parameters()
    return model


def test_pair_links_draw_from_the_shortlist_table():
    """``set_shortlist(M)`` leaves the table of ``segments_ref`` on the device; ``redraw(e, hard_share=...)`` over it is the
    restatement; the same epoch twice gives the same bytes; without a table -- never set, or cleared -- and with share None or
    0, ``redraw`` gives today's bytes."""
    import torch
    from igmc_amd.pair_train import PairLinks
    import pair_checks as PK
    A, u, v, lab = taste_blocks(2)
    ds = dataset(A, u, v, lab, 2)
    pl = PairLinks(ds)
    pu, pv = u.astype(np.int32), v.astype(np.int32)
    plain = [t.clone() for t in (pl.redraw(1).link_u, pl.link_v, pl.link_y)]
    ru, rv, ry, err, _ = PK.negatives_ref(A, pu, pv, 2, 1)
    assert np.array_equal(plain[1].cpu().numpy(), rv) and err == 0
    for share in (0.3, 1.0):          # no table yet: the share is not looked at
        assert all(torch.equal(a, b) for a, b in zip(plain, (pl.redraw(1, hard_share=share).link_u, pl.link_v, pl.link_y)))
    for m, mask in ((10, None), (3, (np.arange(80) % 4 != 1))):
        assert pl.set_shortlist(m, item_mask=mask) is pl and pl.shortlist == m
        off, item = PH.table_ref(A, m, None if mask is None else mask.astype(np.uint8))
        assert pl.sl_off.dtype == torch.int64 and pl.sl_item.dtype == torch.int32 and pl.sl_total == len(item)
        assert np.array_equal(pl.sl_off.cpu().numpy(), off) and np.array_equal(pl.sl_item.cpu().numpy()[:len(item)], item)
        for share in (0.5, 1.0):
            pl.err.zero_()
            first = [t.clone() for t in (pl.redraw(7, item_mask=mask, hard_share=share).link_u, pl.link_v, pl.link_y)]
            want = PH.hard_negatives_ref(A, pu, pv, 2, 7, off, item, len(item), share, mask)
            assert int(pl.err.item()) == want[3] == 0
            lu, lv, ly = (t.cpu().numpy() for t in first)
            assert np.array_equal(lu, want[0]) and np.array_equal(lv, want[1]) and np.array_equal(ly[1::2], want[2])
            assert np.array_equal(ly[0::2], (lab + 1).astype(np.float32)) and (ly[1::2] == 2.0).sum() > 100
            other = pl.redraw(8, item_mask=mask, hard_share=share).link_v.clone()
            again = [t.clone() for t in (pl.redraw(7, item_mask=mask, hard_share=share).link_u, pl.link_v, pl.link_y)]
            assert all(torch.equal(a, b) for a, b in zip(first, again)) and not torch.equal(first[1], other)
        for share in (None, 0, 0.0):          # a table, and no share: today's call
            assert all(torch.equal(a, b) for a, b in zip(plain, (pl.redraw(1, hard_share=share).link_u, pl.link_v, pl.link_y)))
    assert pl.clear_shortlist() is pl and pl.sl_off is None
    assert all(torch.equal(a, b) for a, b in zip(plain, (pl.redraw(1, hard_share=1.0).link_u, pl.link_v, pl.link_y)))
    with pytest.raises(ValueError, match='hard_share'):
        pl.redraw(1, hard_share=1.5)
    with pytest.raises(ValueError, match='shortlist size'):
        pl.set_shortlist(0)


def test_a_table_built_in_passes_is_the_table(monkeypatch):
    """A link capacity that holds a few users' lists at a time: ``set_shortlist`` goes through several passes and leaves the
    same table."""
    from igmc_amd import recommend
    from igmc_amd.pair_train import PairLinks
    A, u, v, lab = taste_blocks(3)
    ds = dataset(A, u, v, lab, 3)
    monkeypatch.setattr(recommend, 'DEFAULT_CAPACITY', 7 * 10 + 3)          # seven users a pass, nine passes
    pl = PairLinks(ds).set_shortlist(10, seed_min_rel=3, vote_min_rel=1)
    off, item = PH.table_ref(A, 10, None, 3, 1)
    assert np.array_equal(pl.sl_off.cpu().numpy(), off) and np.array_equal(pl.sl_item.cpu().numpy(), item)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_it_learns_its_hard_pairs(seed):
    """60 x 80 taste blocks: two epochs of ``train_pairs(shortlist=10, hard_share=1.0)`` (30 steps each) from
    ``reset_parameters()``.  Every epoch has hard pairs and no stale pick; on a FIXED evaluation draw the mean pair term of the
    hard pairs, scored in evaluation mode, is lower after than before (no magnitude is stated); two runs of the same seed
    leave bit-identical parameters."""
    from igmc_amd.pair_train import PairLinks, eval_pairs, eval_pairs_by_kind, train_pairs
    A, u, v, lab = taste_blocks(seed)
    ds = dataset(A, u, v, lab, seed)
    held = PairLinks(ds).set_shortlist(10).redraw(1000, hard_share=1.0)
    runs = []
    for _ in range(2):
        model = fresh_model(ds, seed)
        before = eval_pairs_by_kind(model, held, 64)
        both = eval_pairs(model, held, 64)
        assert before[2][2] == len(u) and before[1] == (0.0, 0.0, 0) and both == before[2][:2]          # every pair is hard
        hist = train_pairs(model, ds, 2, 64, 2e-3, mse_weight=0.0, ARR=0.001, shortlist=10, hard_share=1.0)
        after = eval_pairs_by_kind(model, held, 64)
        print('seed %d: hard pair term %.4f -> %.4f, accuracy %.3f -> %.3f' % (seed, before[2][0], after[2][0], before[2][1],
                                                                               after[2][1]))
        assert len(hist) == 2 and all(h['steps'] == 30 and h['pairs'] == len(u) for h in hist)
        assert all(h['hard_pairs'] == len(u) and h['stale'] is False and 0.0 <= h['pair_acc_hard'] <= 1.0 for h in hist)
        assert all(h['pair_acc_hard'] == h['pair_acc'] and h['pair_acc_uniform'] == 0.0 for h in hist)
        assert after[2][0] < before[2][0], (before, after)
        runs.append(model.flat_parameters().detach().cpu().numpy().copy())
    assert np.isfinite(runs[0]).all() and runs[0].tobytes() == runs[1].tobytes()


def test_a_mixed_epoch_counts_both_kinds_and_plain_training_keeps_its_dict():
    from igmc_amd.pair_train import train_pairs
    A, u, v, lab = taste_blocks(4)
    ds = dataset(A, u, v, lab, 4)
    hist = train_pairs(fresh_model(ds, 4), ds, 1, 64, 1e-3, shortlist=10)          # the default share
    h = hist[0]
    assert 0.4 * len(u) < h['hard_pairs'] < 0.6 * len(u) and h['pairs'] == len(u) and h['stale'] is False
    ordered = h['pair_acc_hard'] * h['hard_pairs'] + h['pair_acc_uniform'] * (h['pairs'] - h['hard_pairs'])
    assert abs(ordered - h['pair_acc'] * h['pairs']) < 1e-6          # the kinds' ordered pairs add up to the step's
    plain = train_pairs(fresh_model(ds, 4), ds, 1, 64, 1e-3)[0]
    assert sorted(plain) == ['epoch', 'mse', 'pair_acc', 'pair_loss', 'pairs', 'seconds', 'steps', 'void']


# ------------------------------------------------------------------ end to end
def test_main_pair_shortlist_end_to_end(tmp_path):
    """``Main.py ... --epochs 1 --pair-epochs 1 --pair-shortlist 20 --pair-hard-share 0.5`` trains, fine-tunes on both kinds of
    negatives and saves the pair checkpoint; the one line of the pair log has the extended form and is what was printed."""
    cmd = [sys.executable, os.path.join(ROOT, 'Main.py'), '--data-name', 'douban', '--epochs', '1', '--testing',
           '--save-interval', '1', '--dynamic-train', '--dynamic-test', '--max-train-num', '300', '--max-test-num', '300',
           '--max-nodes-per-hop', '50', '--pair-epochs', '1', '--pair-shortlist', '20', '--pair-hard-share', '0.5']
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    res = tmp_path / 'results' / 'douban_testmode'
    assert (res / 'pair_checkpoint1.pth').exists()
    log = (res / 'pair_log.txt').read_text().splitlines()
    assert len(log) == 1 and log[0].startswith('Pair epoch 1, pair loss ') and log[0] in out
    assert ', hard 0.' in log[0] and ', pair acc hard ' in log[0] and ', uniform ' in log[0]
