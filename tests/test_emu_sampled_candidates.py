"""``igmc_candidates_sample_count`` / ``igmc_candidates_sample_fill`` (``igmc_amd/csrc/candidates.hip``) on the CPU
emulation of the HIP sources: every segment is the numpy definition of ``tests/sampled_candidates_checks.py`` -- written from
the text of ``include/igmc_rng.h``, so these tests also hold that restatement to the header's own code.  Cases, references and
checks run unchanged on the device (``tests/test_gpu_sampled_candidates.py``)."""
import pytest

import sampled_candidates_checks as SC
from helpers import emu_lib
from parity_checks import EmuBackend
from selection_checks import BAD_OFFSETS


@pytest.mark.parametrize('n_items', [63, 64, 65])
def test_segments_are_the_definition(n_items):
    SC.check_segments(EmuBackend(), n_items)


@pytest.mark.parametrize('n_items', [16383, 16384, 16385, 40000])
@pytest.mark.parametrize('masked', [False, True])
def test_segments_are_the_definition_around_the_tile_and_past_it(n_items, masked):
    SC.check_segments(EmuBackend(), n_items, masks=(masked,), excludes=(1,))


@pytest.mark.slow
@pytest.mark.parametrize('n_items', [16383, 16384, 16385, 40000])
def test_segments_are_the_definition_around_the_tile_with_seen_items(n_items):
    SC.check_segments(EmuBackend(), n_items, excludes=(0,))


@pytest.mark.parametrize('n_items', [65, 16385])
def test_every_negative_and_no_must_item_is_the_enumeration_byte_for_byte(n_items):
    SC.check_all_negatives_is_the_enumeration(EmuBackend(), n_items)


def test_a_crowded_deciding_byte_goes_through_the_radix_passes(monkeypatch):
    monkeypatch.setenv('IGMC_SAMPLE_PARK', '2')
    SC.check_fallback_selection(EmuBackend(), 3000, 2)
    monkeypatch.setenv('IGMC_SAMPLE_PARK', '0')          # ... and a list that holds nothing at all
    SC.check_fallback_selection(EmuBackend(), 20000, 0)


def test_a_deciding_byte_of_256_keys_is_parked_and_one_of_257_is_not():
    SC.check_park_bound(EmuBackend())          # (the default bound: no IGMC_SAMPLE_PARK)


def test_the_same_users_in_another_order_keep_their_segments():
    SC.check_many_users(EmuBackend(), 3000)


@pytest.mark.slow
def test_more_users_than_workgroups():
    SC.check_many_users(EmuBackend(), permuted=False)          # (workgroups of both launches take a second request)


def test_what_has_no_place_is_reported_and_not_written():
    SC.check_no_place(EmuBackend())


def test_a_user_id_out_of_range_is_reported():
    SC.check_bad_user(EmuBackend(), (10, -1, 2 ** 31 - 1))


def test_a_must_item_out_of_range_is_ignored_and_reported():
    SC.check_bad_must_item(EmuBackend())


@pytest.mark.parametrize('bad', BAD_OFFSETS)
def test_inconsistent_must_offsets_are_reported_and_not_followed(bad):
    SC.check_bad_must_offsets(EmuBackend(), bad, wild=True)


def test_bad_arguments_are_refused():
    SC.check_refusals(emu_lib())


@pytest.mark.parametrize('n', [150, 400, 2000])
def test_draws_are_the_restatement_and_distributed_like_uniform_k_subsets(n, capsys):
    SC.check_distribution(EmuBackend(), n)


def test_the_statistics_reject_a_lowest_id_sampler():
    for n in (150, 400, 2000):
        SC.check_lowest_ids_violate_the_bounds(n)
