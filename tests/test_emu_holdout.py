"""``igmc_holdout_count`` / ``igmc_holdout_fill`` (``igmc_amd/csrc/holdout.hip``) on the CPU emulation of the HIP sources:
every segment is the numpy definition of ``tests/holdout_checks.py`` -- written from the text of ``include/igmc_hip.h`` and
``include/igmc_rng.h``, so these tests also hold that restatement to the headers' own code.  Cases, references and checks run
unchanged on the device (``tests/test_gpu_holdout.py``)."""
import pytest

import holdout_checks as HC
import sampled_candidates_checks as SC
from helpers import emu_lib
from parity_checks import EmuBackend


@pytest.mark.parametrize('hold', HC.HOLDS)
def test_segments_are_the_definition(hold):
    HC.check_definition(EmuBackend(), holds=(hold,))


def test_kept_sets_are_nested_in_keep():
    HC.check_nested(EmuBackend())


def test_a_long_row_goes_through_the_radix_passes():
    HC.check_long_row(EmuBackend())


@pytest.mark.parametrize('park', ['2', '0'])
def test_a_long_row_with_a_short_parked_list_and_with_none(monkeypatch, park):
    monkeypatch.setenv('IGMC_SAMPLE_PARK', park)
    HC.check_long_row(EmuBackend(), int(park))


def test_a_deciding_byte_of_256_keys_is_parked_and_one_of_257_is_not():
    HC.check_park_bound(EmuBackend())          # (the default bound: no IGMC_SAMPLE_PARK)


def test_the_same_users_in_another_order_keep_their_segments():
    HC.check_many_users(EmuBackend(), 3000)


def test_what_has_no_place_is_reported_and_not_written():
    HC.check_no_place(EmuBackend())


def test_a_user_id_out_of_range_is_reported():
    HC.check_bad_user(EmuBackend(), (10, -1, 2 ** 31 - 1))


def test_bad_arguments_are_refused():
    HC.check_refusals(emu_lib())


@pytest.mark.parametrize('keep,hold', HC.REDUCED)
def test_the_reduced_graph_is_the_graph_of_the_reduced_matrix(keep, hold):
    HC.check_reduced_graph(EmuBackend(), keep, hold)


@pytest.mark.parametrize('n', [150, 400])
def test_splits_are_the_restatement_and_distributed_like_uniform_k_subsets(n, capsys):
    HC.check_distribution(EmuBackend(), n)


def test_the_statistics_reject_a_lowest_id_sampler():
    for n in (150, 400):
        SC.check_lowest_ids_violate_the_bounds(n)
