"""Hard pair negatives on the CPU emulation of the HIP sources: ``igmc_pair_negatives_shortlist`` against the numpy restatement
of ``tests/pair_hard_checks.py`` -- written from the text of ``include/igmc_hip.h`` / ``include/igmc_rng.h``, so these tests also
hold that restatement to the header's own code -- over the tables of ``shortlist_checks.segments_ref``, and
``igmc_pair_kind_stats`` against float64 numpy.  Cases and checks run unchanged on the device (``tests/test_gpu_pair_hard.py``)."""
import pytest

import pair_hard_checks as PH
from helpers import emu_lib
from parity_checks import EmuBackend


# ------------------------------------------------------------------ the definition
@pytest.mark.parametrize('n_items', PH.N_ITEMS)
def test_negatives_are_the_definition(n_items):
    PH.check_definition(EmuBackend(), n_items)


def test_share_zero_and_a_null_table_give_the_bytes_of_the_uniform_entry():
    PH.check_share_zero_is_the_old_entry(EmuBackend())


def test_positions_decided_uniform_keep_their_uniform_negative():
    PH.check_uniform_positions_keep_their_negative(EmuBackend())


def test_a_user_who_rated_every_item_gets_void_pairs():
    PH.check_a_full_row_gives_void_pairs(EmuBackend())


# ------------------------------------------------------------------ a stale table
@pytest.mark.parametrize('which', PH.STALE)
def test_a_pick_that_does_not_qualify_falls_back_and_is_reported(which):
    PH.check_stale_pick(EmuBackend(), which)


@pytest.mark.parametrize('which', PH.BAD_OFFSETS)
def test_broken_offsets_are_reported_and_not_followed(which):
    PH.check_broken_offsets(EmuBackend(), which)


# ------------------------------------------------------------------ robustness
def test_ids_out_of_range_are_reported_and_nothing_of_theirs_is_read():
    PH.check_bad_ids(EmuBackend(), (-1, 4, 2 ** 31 - 1))


def test_more_positives_than_waves_in_the_grid():
    PH.check_many_positives(EmuBackend())


def test_the_cyclic_scan_decides_behind_a_fall_through(monkeypatch):
    monkeypatch.setenv('IGMC_PAIR_TRIES', '0')
    PH.check_scan_behind_a_fall_through(EmuBackend())


def test_bad_arguments_are_refused():
    PH.check_refusals(emu_lib())


# ------------------------------------------------------------------ distribution
def test_draws_are_the_restatement_and_within_both_bounds():
    PH.check_distribution(EmuBackend())


def test_the_restatement_stays_within_the_bounds_and_a_first_item_sampler_does_not():
    PH.check_restatement_within_bounds()
    PH.check_first_item_sampler_violates_the_bound()


# ------------------------------------------------------------------ per-kind statistics
@pytest.mark.parametrize('kinds', PH.KINDS)
@pytest.mark.parametrize('n_pairs', [1, 2, 33, 250])
def test_kind_stats_are_the_float64_reference(n_pairs, kinds):
    PH.check_kind_stats(EmuBackend(), n_pairs, kinds)
