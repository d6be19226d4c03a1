"""Pair training on the CPU emulation of the HIP sources: ``igmc_pair_negatives`` against the numpy restatement of
``tests/pair_checks.py`` -- written from the text of ``include/igmc_rng.h``, so these tests also hold that restatement to the
header's own code --, ``igmc_pair_loss`` against float64 numpy, ``igmc_pair_loss_grad`` against ``oracle/pyg_ref.py`` with the
pair loss in torch float64.  Cases, references and checks run unchanged on the device (``tests/test_gpu_pairs.py``)."""
import pytest

import pair_checks as PK
from helpers import emu_lib, load_extract_golden
from parity_checks import EmuBackend

CASES = load_extract_golden()


def sub(name, n):
    case = dict(CASES[name])
    case['recs'], case['links'], case['link_labels'] = case['recs'][:n], case['links'][:n], case['link_labels'][:n]
    return case


# ------------------------------------------------------------------ the sampler
@pytest.mark.parametrize('n_items', [63, 64, 65, 300, 40000])
def test_negatives_are_the_definition(n_items):
    PK.check_definition(EmuBackend(), n_items)


def test_a_second_round_of_tries_decides_some_draws():
    PK.check_second_round(EmuBackend())


def test_the_cyclic_scan_decides_where_the_tries_give_out(monkeypatch):
    monkeypatch.setenv('IGMC_PAIR_TRIES', '2')
    PK.check_fallback(EmuBackend(), 'crowded', 2)
    monkeypatch.setenv('IGMC_PAIR_TRIES', '0')          # ... and no try at all
    PK.check_fallback(EmuBackend(), 'half', 0)


def test_a_user_without_an_unseen_item_gets_void_pairs():
    PK.check_void_pairs(EmuBackend())


def test_ids_out_of_range_are_reported_and_their_rows_not_read():
    PK.check_bad_ids(EmuBackend(), (-1, 4, 2 ** 31 - 1))


def test_bad_arguments_are_refused():
    PK.check_refusals(emu_lib())


def test_more_positives_than_waves_in_the_grid():
    PK.check_many_positives(EmuBackend())


@pytest.mark.parametrize('n_items, seen', sorted(PK.STAT_USERS))
def test_draws_are_the_restatement_and_uniform_over_the_unseen_items(n_items, seen):
    PK.check_distribution(EmuBackend(), n_items, seen)


@pytest.mark.parametrize('n_items, seen', sorted(PK.STAT_USERS))
def test_the_restatement_stays_within_the_bound_and_a_lowest_id_sampler_does_not(n_items, seen):
    PK.check_restatement_within_bounds(n_items, seen)
    PK.check_lowest_ids_violate_the_bound(n_items, seen)


# ------------------------------------------------------------------ the pair loss
@pytest.mark.parametrize('A', [0.0, 1.0])
@pytest.mark.parametrize('n_pairs, void', [(1, 'none'), (1, 'all'), (2, 'first'), (31, 'last'), (32, 'interleaved'), (33, 'none'),
                                           (250, 'none'), (250, 'first'), (250, 'last'), (250, 'interleaved'), (250, 'all')])
def test_pair_loss_is_the_float64_reference(n_pairs, void, A):
    PK.check_pair_loss(EmuBackend(), n_pairs, void, A)


# ------------------------------------------------------------------ the step
@pytest.mark.parametrize('name, n, R, drop, n_side', [
    ('synth_cap', 6, 5, False, 0),      # R = 5, one hop
    ('synth_cap', 6, 5, True, 0),       # ... under edge dropout
    ('flixster', 4, 10, True, 0),       # ten relations
    ('synth_nocap', 2, 5, False, 10),   # side features (a width the MFMA head does not take)
    ('hand_h2', 4, 5, True, 0),         # two hops
])
def test_pair_step_matches_the_oracle(name, n, R, drop, n_side):
    PK.check_step(EmuBackend(), sub(name, n), n, R, drop, n_side)


def test_pure_pairwise_objective_matches_the_oracle():
    PK.check_step(EmuBackend(), sub('synth_cap', 8), 8, 5, True, A=0.0)


def test_an_odd_batch_is_refused():
    PK.check_odd_batch_is_refused(EmuBackend(), sub('synth_cap', 3))


def test_pair_steps_follow_the_oracle_trajectory():
    PK.check_trajectory(EmuBackend(), sub('synth_cap', 6), 6, 5)
